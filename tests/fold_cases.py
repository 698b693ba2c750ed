"""Cases and references shared by test_fold_runs_host.py (which proves, without a GPU, what
shapes of the fold launcher the cases reach and that their sums are exact in float32) and
test_fold_runs_gpu.py (which runs them on the device): `hip.fold_runs` (bbt_fold_runs,
csrc/fold_kernels.hpp) against a NumPy fold in int64 / float64."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from baseband_tasks_amd.fold_table import unwrapped_bin

#: below this, every integer is a float32: sums of integers whose absolute values add up to
#: less than it are exact in float32 in any order of summation
EXACT = float(1 << 24)
#: samples a lane adds into a sub-sum before it flushes (BBT_FOLD_BLOCK of fold_kernels.hpp)
FOLD_BLOCK = 1024
#: hip.FOLD_MAX_SPLIT and the cap of the work area in hip._fold_launch
FOLD_MAX_SPLIT, WORK_CAP = 64, 1 << 24


# -- the fold of the tasks, in NumPy -------------------------------------------------------
def numpy_fold(x, edges, n_phase, ph, rate, t0):
    """float64 fold of x[edges[0]:edges[-1]] with the per-row times of the reference."""
    n_row = len(edges) - 1
    out = np.zeros((n_row, n_phase) + x.shape[1:], np.complex128 if x.dtype.kind == 'c' else np.float64)
    cnt = np.zeros((n_row, n_phase), np.int64)
    for r in range(n_row):
        n = np.arange(edges[r], edges[r + 1])
        t = (t0 + edges[r] / rate) + (n - edges[r]) / rate
        b = unwrapped_bin(ph(t), n_phase) % n_phase
        np.add.at(out[r], b, x[n])
        np.add.at(cnt[r], b, 1)
    return out, cnt


# -- the fold of a run table, in NumPy ------------------------------------------------------
def detect(x, mode):
    """What k_detect_integrate documents per sample, as (n_in, floats out per sample): mode 0
    ``|z|^2`` per complex element, 1 ``|X|^2, |Y|^2, Re XY*, Im XY*`` per (X, Y) pair, 2 the
    floats as they are.  int64 where the data are integer-valued, float64 otherwise."""
    x = np.asarray(x)
    n_in = x.shape[0]
    if mode == 2:
        parts = [x.reshape(n_in, -1)]
    else:
        z = x.reshape(n_in, -1)
        parts = [z.real, z.imag]
    whole = all(np.array_equal(p, np.rint(p)) for p in parts)
    parts = [p.astype(np.int64 if whole else np.float64) for p in parts]
    if mode == 2:
        return parts[0]
    re, im = parts
    if mode == 0:
        return re * re + im * im
    xr, xi, yr, yi = re[:, 0::2], im[:, 0::2], re[:, 1::2], im[:, 1::2]
    out = np.stack([xr * xr + xi * xi, yr * yr + yi * yi, xr * yr + xi * yi, xi * yr - xr * yi], axis=-1)
    return out.reshape(n_in, -1)


def fold_reference(x, mode, slot_ptr, run_begin, run_end, prev=None, scale=None):
    """``out[j] = (prev[j] + sum over the runs of slot j and their samples of detect(x)) * scale[j]``
    with the runs clipped to [0, n_in) and runs with ``end <= begin`` ignored, in float64 (the
    sums in int64 where the data are integer-valued).  Returns (out, mass), both (n_slot, floats
    per slot) float64; ``mass`` is the sum of the absolute values of every term and of ``prev``,
    the figure that bounds what any float32 partial sum can reach."""
    d = detect(x, mode)
    n_in, width = d.shape
    slot_ptr = np.asarray(slot_ptr, np.int64)
    n_slot = len(slot_ptr) - 1
    b = np.clip(np.asarray(run_begin, np.int64), 0, n_in)
    e = np.clip(np.asarray(run_end, np.int64), 0, n_in)
    keep = e > b
    slot = np.repeat(np.arange(n_slot), np.diff(slot_ptr))[keep]
    b, e = b[keep], e[keep]
    out = np.zeros((n_slot, width), d.dtype)
    mass = np.zeros((n_slot, width), d.dtype)
    # (sums along time once, differences at the run edges: wide cases stay fast)
    for terms, into in ((d, out), (np.abs(d), mass)):
        c = np.zeros((n_in + 1, width), d.dtype)
        np.cumsum(terms, axis=0, out=c[1:])
        np.add.at(into, slot, c[e] - c[b])
    out, mass = out.astype(np.float64), mass.astype(np.float64)
    if prev is not None:
        prev = np.asarray(prev, np.float64).reshape(n_slot, width)
        out += prev
        mass += np.abs(prev)
    if scale is not None:
        with np.errstate(invalid='ignore'):
            out = out * np.asarray(scale, np.float32).astype(np.float64)[:, None]
    return out, mass


def brute_force(x, mode, slot_ptr, run_begin, run_end, prev=None, scale=None):
    """`fold_reference` by loops over slots, runs and samples, with Python's complex numbers:
    for tiny cases."""
    x = np.asarray(x)
    n_in = x.shape[0]
    rows = x.reshape(n_in, -1)
    n_slot = len(slot_ptr) - 1
    out = []
    for j in range(n_slot):
        acc = None
        for r in range(slot_ptr[j], slot_ptr[j + 1]):
            for t in range(max(run_begin[r], 0), min(run_end[r], n_in)):
                if mode == 2:
                    term = [float(v) for v in rows[t]]
                elif mode == 0:
                    term = [complex(z).real ** 2 + complex(z).imag ** 2 for z in rows[t]]
                else:
                    term = []
                    for X, Y in zip(rows[t][0::2], rows[t][1::2]):
                        X, Y = complex(X), complex(Y)
                        xy = X * Y.conjugate()
                        term += [X.real ** 2 + X.imag ** 2, Y.real ** 2 + Y.imag ** 2, xy.real, xy.imag]
                acc = term if acc is None else [a + v for a, v in zip(acc, term)]
        width = rows.shape[1] * (2 if mode == 1 else 1)
        out.append(acc if acc is not None else [0.] * width)
    out = np.array(out, np.float64)
    if prev is not None:
        out = out + np.asarray(prev, np.float64).reshape(out.shape)
    if scale is not None:
        with np.errstate(invalid='ignore'):
            out = out * np.asarray(scale, np.float32).astype(np.float64)[:, None]
    return out


def expected_float32(total, scale):
    """What the kernels must give for sums that are exact in float32: the total itself, or with a
    scale the one float32 product ``float32(total) * float32(scale[j])``, formed in float32 as
    the kernels form it (k_fold_gather and k_fold_combine: the scale is their last operation)."""
    want = np.asarray(total).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), total), 'the totals are not float32 numbers'
    if scale is not None:
        with np.errstate(invalid='ignore'):
            want = want * np.asarray(scale, np.float32)[:, None]
        assert want.dtype == np.float32
    return want


# -- the launcher's choice, restated ---------------------------------------------------------
def fold_work_floats(n_slot, n_elem, mode):
    """The work area `hip._fold_launch` hands to bbt_fold_runs, in floats (0: none)."""
    n_out_f = 2 * n_elem if mode == 1 else n_elem
    work_floats = min(FOLD_MAX_SPLIT * n_slot * n_out_f, WORK_CAP)
    return work_floats if work_floats >= 2 * n_slot * n_out_f else 0


def fold_dispatch(n_in, n_elem, mode, n_slot, aligned16, work_floats):
    """The kernel shape bbt_fold_runs (csrc/bbt_hip.hip) picks for these arguments: a Python
    restatement of its ``vec``, ``n_unit``, ``lg_tc``, ``tt``, ``tiles`` and ``split`` (and, in
    `fold_work_floats`, of the work size of `hip._fold_launch`).

    It exists only to prove that the case list spans the grid of kernel shapes.  It is not a
    check of the library: nothing compares it with what the launcher does, and if the launcher's
    rule changes, this restatement must be updated by hand."""
    elems_per_vec = 4 if mode == 2 else 2
    vec = mode == 1 or (n_elem % elems_per_vec == 0 and bool(aligned16))
    n_unit = n_elem // elems_per_vec if vec else n_elem
    out_w = 4 if mode == 1 else ((2 if vec else 1) if mode == 0 else (4 if vec else 1))
    n_out_f = n_unit * out_w
    lg_tc = 0
    while lg_tc < 8 and (1 << lg_tc) < n_unit:
        lg_tc += 1
    tt = 256 >> lg_tc
    tiles = (n_unit + (1 << lg_tc) - 1) >> lg_tc
    base = tiles * n_slot
    split = (2048 + base - 1) // base
    split = min(split, 64)
    split = min(split, max(1, n_in // (n_slot * tt * 64)))
    split = min(split, max(1, work_floats // (n_slot * n_out_f)))
    if not work_floats:
        split = 1
    return dict(mode=mode, vec=int(vec), n_unit=n_unit, n_out_f=n_out_f, lg_tc=lg_tc, tt=tt, tiles=tiles,
                split=split)


# -- the cases ---------------------------------------------------------------------------------
#: mode, n_elem: as bbt_fold_runs takes them (complex elements per sample for modes 0 and 1,
#: floats for mode 2); aligned: the input starts on the 16-byte grid (else 8 bytes off it);
#: scale: None or 'scale' (arbitrary float32, some exact powers of two, NaN on the first slot
#: without samples); empty: slots without runs; long: (slot, length) of a slot that holds one
#: single run; many: a slot that gets half of all other runs; n_runs: runs cut from the input.
Case = namedtuple('Case', 'name mode n_elem aligned n_in n_slot accumulate scale empty long many n_runs')


def new_case(name, mode, n_elem, n_in, n_slot, aligned=True, accumulate=False, scale=None, empty=(),
          long=None, many=None, n_runs=None):
    if n_runs is None:
        n_runs = 6 * n_slot
    return Case(name, mode, n_elem, aligned, n_in, n_slot, accumulate, scale, tuple(empty), long, many, n_runs)


def _spread(n_slot):
    """Empty slots first, in the middle and last; a slot of many runs; a slot for one long run."""
    return dict(empty=(0, n_slot // 2, n_slot - 1), many=1, long=(2, None))


CASES = [
    # MODE 0, one complex element per lane (odd n_elem, or an input off the 16-byte grid)
    new_case('sq_odd_u1', 0, 1, 1000, 5, scale='scale', empty=(4,)),
    new_case('sq_odd_u3_flush', 0, 3, 1 << 17, 32, accumulate=True, n_runs=300, empty=(0, 16, 31), many=1,
          long=(2, 100000)),
    new_case('sq_off_grid_u2', 0, 2, 3000, 4, aligned=False, accumulate=True, scale='scale', empty=(0,)),
    new_case('sq_odd_u129_split', 0, 129, 4096, 2, n_runs=40),
    new_case('sq_off_grid_u300_split', 0, 300, 4096, 2, aligned=False, accumulate=True, scale='scale', n_runs=64),
    new_case('sq_odd_u1029', 0, 1029, 2048, 40, n_runs=200, **_spread(40)),
    new_case('sq_odd_u1029_split', 0, 1029, 2048, 2, scale='scale', empty=(1,), n_runs=30),
    # MODE 0, two complex elements per lane
    new_case('sq_vec_u1', 0, 2, 5000, 3, empty=(1,), n_runs=50),
    new_case('sq_vec_u5_flush_split', 0, 10, 1 << 17, 32, scale='scale', n_runs=300, empty=(0, 16, 31), many=1,
          long=(2, 120000)),
    new_case('sq_vec_u64_split', 0, 128, 8192, 3, accumulate=True, empty=(2,), n_runs=90),
    new_case('sq_vec_u256', 0, 512, 2048, 64, accumulate=True, scale='scale', n_runs=300, **_spread(64)),
    new_case('sq_vec_u257_split', 0, 514, 2048, 2, accumulate=True, n_runs=50),
    # MODE 1, one (X, Y) pair per lane
    new_case('pw_u1', 1, 2, 4000, 7, n_runs=80, **_spread(7)),
    new_case('pw_u2', 1, 4, 3000, 5, accumulate=True, scale='scale', empty=(0, 4)),
    new_case('pw_u3_split', 1, 6, 16384, 1, scale='scale', n_runs=25),
    new_case('pw_u12', 1, 24, 6000, 9, accumulate=True, **_spread(9)),
    new_case('pw_u128', 1, 256, 2048, 20, accumulate=True, n_runs=150, **_spread(20)),
    new_case('pw_u255_split', 1, 510, 2048, 3, empty=(0,), n_runs=40),
    new_case('pw_u300_split', 1, 600, 4096, 2, accumulate=True, scale='scale', n_runs=64),
    new_case('pw_u512_split', 1, 1024, 2048, 4, accumulate=True, empty=(3,), long=(1, 1500), n_runs=40),
    new_case('pw_u1000', 1, 2000, 1024, 24, scale='scale', n_runs=120, **_spread(24)),
    # MODE 2, four floats per lane
    new_case('sum_vec_u1', 2, 4, 3000, 6, accumulate=True, scale='scale', **_spread(6)),
    new_case('sum_vec_u2_split', 2, 8, 32768, 1, accumulate=True, n_runs=30),
    new_case('sum_vec_u64', 2, 256, 4096, 50, n_runs=300, **_spread(50)),
    new_case('sum_vec_u257', 2, 1028, 4096, 33, accumulate=True, scale='scale', n_runs=200, **_spread(33)),
    new_case('sum_vec_u512_split', 2, 2048, 2048, 2, scale='scale', n_runs=40),
    # MODE 2, one float per lane (n_elem no multiple of 4, or an input off the 16-byte grid)
    new_case('sum_odd_u1', 2, 1, 777, 4, empty=(3,)),
    new_case('sum_odd_u5_flush_split', 2, 5, 1 << 17, 32, accumulate=True, scale='scale', n_runs=300,
          empty=(0, 16, 31), many=1, long=(2, 125000)),
    new_case('sum_odd_u22_split', 2, 22, 32768, 2, scale='scale', n_runs=40),
    new_case('sum_off_grid_u256_split', 2, 256, 4096, 2, aligned=False, accumulate=True, n_runs=50),
    new_case('sum_odd_u255', 2, 255, 4096, 70, scale='scale', n_runs=400, **_spread(70)),
    new_case('sum_off_grid_u1000_split', 2, 1000, 2048, 2, aligned=False, scale='scale', empty=(0,), n_runs=30),
    new_case('sum_odd_u1029', 2, 1029, 4096, 100, accumulate=True, n_runs=500, **_spread(100)),
]
BY_NAME = {case.name: case for case in CASES}
assert len(BY_NAME) == len(CASES)


def _rng(case, what):
    return np.random.default_rng([zlib.crc32(case.name.encode()), what])


def make_table(case, rng=None):
    """(slot_ptr, run_begin, run_end) of a case, int64: the input cut into ``n_runs`` runs, one
    in ten left out, the rest dealt to the slots that may have runs (half of them to ``many``),
    so that the runs of a slot are in time order but the slots are not; then the one run of
    ``long`` (which overlaps others: samples may be summed twice), three runs of length 0 and
    three of length 1."""
    rng = _rng(case, 1) if rng is None else rng
    n_in, n_slot = case.n_in, case.n_slot
    long_slot = case.long[0] if case.long else None
    free = [j for j in range(n_slot) if j not in case.empty and j != long_slot]
    cuts = np.sort(rng.choice(np.arange(1, n_in), size=min(case.n_runs, n_in - 1) - 1, replace=False))
    begin = np.concatenate(([0], cuts))
    end = np.concatenate((cuts, [n_in]))
    keep = rng.random(len(begin)) >= 0.1
    begin, end = begin[keep], end[keep]
    slot = rng.choice(free, size=len(begin))
    if case.many is not None:
        slot = np.where(rng.random(len(begin)) < 0.5, case.many, slot)
    at = rng.integers(0, n_in, size=6)
    begin = np.concatenate((begin, at))
    end = np.concatenate((end, at[:3], at[3:] + 1))
    slot = np.concatenate((slot, rng.choice(free, size=6)))
    if case.long:
        length = case.long[1] or (3 * n_in) // 4
        first = (n_in - length) // 3
        begin, end, slot = np.append(begin, first), np.append(end, first + length), np.append(slot, long_slot)
    order = np.argsort(slot, kind='stable')
    slot_ptr = np.zeros(n_slot + 1, np.int64)
    np.cumsum(np.bincount(slot, minlength=n_slot), out=slot_ptr[1:])
    return slot_ptr, begin[order].astype(np.int64), end[order].astype(np.int64)


def slot_samples(slot_ptr, run_begin, run_end, n_in):
    """Samples per slot after clipping."""
    length = np.maximum(np.clip(run_end, 0, n_in) - np.clip(run_begin, 0, n_in), 0)
    return np.bincount(np.repeat(np.arange(len(slot_ptr) - 1), np.diff(slot_ptr)), weights=length,
                       minlength=len(slot_ptr) - 1).astype(np.int64)


def make_scale(case, table, rng=None):
    """float32 (n_slot): arbitrary values, every third an exact power of two, NaN on the first
    slot without samples (what `_run_fold` gives an empty bin of an average)."""
    if case.scale is None:
        return None
    rng = _rng(case, 2) if rng is None else rng
    scale = rng.uniform(0.05, 3., case.n_slot).astype(np.float32)
    scale[::3] = np.float32(2.) ** rng.integers(-6, 3, size=len(scale[::3])).astype(np.float32)
    hollow = np.flatnonzero(slot_samples(*table, case.n_in) == 0)
    if len(hollow):
        scale[hollow[0]] = np.nan
    return scale


def make_input(case, rng=None):
    """The input samples (n_in, n_elem), complex64 for modes 0 and 1 and float32 for mode 2,
    every component an integer in -4 ... 4."""
    rng = _rng(case, 3) if rng is None else rng
    if case.mode == 2:
        return rng.integers(-4, 5, size=(case.n_in, case.n_elem)).astype(np.float32)
    parts = rng.integers(-4, 5, size=(case.n_in, case.n_elem, 2)).astype(np.float32)
    return parts.view(np.complex64)[..., 0]


def make_prev(case, rng=None):
    """Integer-valued float32 (n_slot, floats per slot) to accumulate onto, or None."""
    if not case.accumulate:
        return None
    rng = _rng(case, 4) if rng is None else rng
    n_out_f = 2 * case.n_elem if case.mode == 1 else case.n_elem
    return rng.integers(-1000, 1001, size=(case.n_slot, n_out_f)).astype(np.float32)


def dispatch_of(case):
    return fold_dispatch(case.n_in, case.n_elem, case.mode, case.n_slot, case.aligned,
                         fold_work_floats(case.n_slot, case.n_elem, case.mode))


@functools.lru_cache(maxsize=None)
def cells_of(case):
    """The cells of the launcher's grid, and the kinds of table, that a case covers."""
    d = dispatch_of(case)
    table = make_table(case)
    slot_ptr, begin, end = table
    scale = make_scale(case, table)
    split = 'split' if d['split'] > 1 else 'one share'
    cells = {('kernel', d['mode'], d['vec'], split), ('n_unit', d['n_unit']), ('lg_tc', d['lg_tc']),
             ('tiles', d['tiles'])}
    if d['tiles'] > 1 and d['n_unit'] % 256:
        cells.add(('ragged last tile', split))
    if d['tiles'] > 1 and d['split'] > 1:
        cells.add(('several tiles and split',))
    if not d['vec']:
        per_vec = 4 if case.mode == 2 else 2
        cells.add(('one element per lane', case.mode, 'odd row' if case.n_elem % per_vec else 'off the grid'))
        assert case.n_elem % per_vec or not case.aligned
    if case.accumulate or case.scale:
        cells.add(('accumulate' if case.accumulate else 'overwrite', 'scale' if case.scale else 'no scale', split))
    runs = np.diff(slot_ptr)
    if runs[0] == 0:
        cells.add(('no runs', 'first slot'))
    if runs[-1] == 0:
        cells.add(('no runs', 'last slot'))
    if np.any(runs[1:-1] == 0):
        cells.add(('no runs', 'a middle slot'))
    length = end - begin
    if np.any(length == 0):
        cells.add(('run of length', 0))
    if np.any(length == 1):
        cells.add(('run of length', 1))
    if runs.max() >= 32:
        cells.add(('a slot of many runs',))
    if np.any((runs == 1) & (length[np.minimum(slot_ptr[:-1], len(length) - 1)] >= case.n_in // 2)):
        cells.add(('a slot of one long run',))
    if np.any(np.diff(begin) < 0):
        cells.add(('runs not in time order',))
    if scale is not None:
        if np.any(np.isnan(scale)):
            cells.add(('NaN scale on a slot without samples',))
        finite = scale[np.isfinite(scale)]
        if np.any(np.frexp(finite)[0] == 0.5):
            cells.add(('scale', 'a power of two'))
        if np.any(np.frexp(finite)[0] != 0.5):
            cells.add(('scale', 'arbitrary'))
    # a lane of one share gets every tt-th sample of the share's part of each run
    share = slot_samples(*table, case.n_in).max() // d['split']
    if share // d['tt'] > FOLD_BLOCK:
        cells.add(('sub-sum flush', split))
    return cells


#: what the case list must contain (the issue's list, as `fold_dispatch` sees it)
REQUIRED_CELLS = (
    [('kernel', m, v, s) for (m, v) in ((0, 0), (0, 1), (1, 1), (2, 0), (2, 1)) for s in ('split', 'one share')]
    + [('n_unit', n) for n in (1, 2, 3, 5, 64, 128, 129, 255, 256, 257, 300, 512, 1000, 1029)]
    + [('lg_tc', n) for n in range(9)]
    + [('tiles', n) for n in (1, 2, 4, 5)]
    + [('ragged last tile', 'split'), ('ragged last tile', 'one share'), ('several tiles and split',)]
    + [('one element per lane', m, why) for m in (0, 2) for why in ('odd row', 'off the grid')]
    + [('accumulate', 'no scale', 'split'), ('accumulate', 'scale', 'split'), ('accumulate', 'scale', 'one share'),
       ('overwrite', 'scale', 'split'), ('overwrite', 'scale', 'one share')]
    + [('no runs', where) for where in ('first slot', 'a middle slot', 'last slot')]
    + [('run of length', 0), ('run of length', 1), ('a slot of many runs',), ('a slot of one long run',),
       ('runs not in time order',), ('NaN scale on a slot without samples',), ('scale', 'a power of two'),
       ('scale', 'arbitrary'), ('sub-sum flush', 'split'), ('sub-sum flush', 'one share')])


def missing_cells(cases):
    """The required cells that no case of ``cases`` covers."""
    covered = set()
    for case in cases:
        covered |= cells_of(case)
    return [cell for cell in REQUIRED_CELLS if cell not in covered]
