"""`bbt_gather_execute` between guard bands (tests/guard_bands.py): every source of a call in a guarded array of
its own, so that each can sit at its own offset from 16, and a guarded output.  The plan chooses its kernel
from these bits -- `k_gather_map<B16>` or, with a pointer off 16, the direct kernel on `tab_elem`; the tile
kernel's `vec_mask` (which sources are staged 16 bytes a lane) and `vec_out` -- and until now every array came
from the pool.  Samples are only moved: every result is held byte for byte to NumPy indexing, then all bands to
their poison and the sources to what they were.  The random bytes hold no poison (no 0xa5 byte in one-byte
data, no half of a poison word in two-byte data, no poison word otherwise), so a sample loaded from a band
shows in the comparison.  `src_first_sample` is non-zero everywhere and the sources end with the last row
used: a load one sample too far is in the back band.

By name (the ids say which kernel and which `vec_mask` / `vec_out` a run takes):

  run_copy  `concat_map` of 3 sources of 64-byte rows: all aligned `k_gather_map<B16>`; the output off, or one
            source off: `k_gather_map<E>` on `tab_elem`, the fall-back, with the same bytes
  tile      an interleave of 3 x 3 elements (rows that are no multiple of 16: staged element by element
            whatever the pointers), a (24, 2) transpose of one source, and a map that uses bytes [8, 40) of
            64-byte rows (the stretch widened to [0, 48)); sources all aligned, all off and the first only off,
            crossed with the output aligned and off: `vec_mask` full, empty and mixed, `vec_out` 1 and 0
  direct    the random map of test_shaping_gpu.py at the smallest offset each element size allows

What stays outside: the tables the plan uploads."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, units as u
from baseband_tasks_amd.shaping import index_map

from guard_bands import BYTE_POISON, POISONS, Guarded, check_all
from test_shaping_gpu import DTYPES, T0, concat_map, device_stream, interleave_map

pytestmark = pytest.mark.gpu

both_poisons = pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))
FIRSTS = [3, 1, 2]


def clean_data(rng, shape, eb):
    """Random bytes as an array of the element type, free of every poison (see the module's docstring)."""
    raw = rng.integers(0, 256, size=int(np.prod(shape, dtype=np.int64)) * eb, dtype=np.uint8)
    if eb == 1:
        raw[raw == BYTE_POISON] = 0x5a
    elif eb == 2:
        half = raw.view('<u2')
        for p in POISONS.values():
            half[(half == (p & 0xffff)) | (half == (p >> 16))] = 0x1234
    else:
        word = raw.view('<u4')
        for p in POISONS.values():
            word[word == p] = 1
    return raw.view(DTYPES[eb]).reshape(shape)


def counts(plan):
    """1, 17, one more than a tile and 1037 samples (no multiple of any tile)."""
    return sorted({1, 17, plan.info()['tile_samples'] + 1, 1037})


def skews_for(targets, rows, eb, firsts):
    """The payloads' skews at which the first sample USED of each source sits at `targets` modulo 16."""
    return [(t - f * r * eb) % 16 for t, r, f in zip(targets, rows, firsts)]


def guarded_run(plan, src, elem, rows, eb, n, poison, src_at, out_at, what, seed=0):
    """`test_shaping_gpu.run_plan` on guarded arrays: source k's first used sample at `src_at[k]` modulo 16,
    the output at `out_at`.  Returns the output's bytes."""
    rng = np.random.default_rng(seed + 1000 * eb + n)
    src, elem = np.asarray(src), np.asarray(elem)
    firsts = FIRSTS[:len(rows)]
    datas = [clean_data(rng, (n + f, r), eb) for r, f in zip(rows, firsts)]          # (extra = 0)
    gs = [Guarded.load(d, poison, sk) for d, sk in zip(datas, skews_for(src_at, rows, eb, firsts))]
    go = Guarded((n, len(src)), DTYPES[eb], poison, out_at)
    for g, f, r, at in zip(gs, firsts, rows, src_at):
        assert (g.array.ptr + f * r * eb) % 16 == at
    plan.execute([g.array for g in gs], go.array, n, firsts)
    *got_src, got = check_all(gs + [go], what)
    want = np.empty((n, len(src)), DTYPES[eb])
    for k, (d, f) in enumerate(zip(datas, firsts)):
        sel = src == k
        want[:, sel] = d[f:f + n][:, elem[sel]]
    assert got.tobytes() == want.tobytes(), f'{what}: {np.count_nonzero(got.view(np.uint8) != want.view(np.uint8))} bytes differ'
    for k, (a, d) in enumerate(zip(got_src, datas)):
        assert a.tobytes() == d.tobytes(), f'{what}: source {k} changed'
    return got.tobytes()


# -- run copy and its fall-back -------------------------------------------------------------------------------
def _run_copy_variants(eb):
    """(id, sources at, output at).  A 16-byte element allows no offset."""
    off = max(eb, 4)
    out = [('all_aligned-B16', (0, 0, 0), 0)]
    if eb < 16:
        out.append((f'out_off{off}-fallback', (0, 0, 0), off))
        for k in range(3):
            out.append((f'src{k}_off{off}-fallback', tuple(off if j == k else 0 for j in range(3)), 0))
        if eb < off:                  # (the smallest offset the element allows)
            out.append((f'src1_off{eb}-fallback', (0, eb, 0), 0))
    return out


RUN_COPY = [(eb, v) for eb in (1, 2, 4, 8, 16) for v in _run_copy_variants(eb)]


@pytest.mark.parametrize('eb, variant', RUN_COPY, ids=[f'eb{eb}-{v[0]}' for eb, v in RUN_COPY])
@both_poisons
def test_run_copy_and_its_fallback(eb, variant, poison):
    _, src_at, out_at = variant
    src, elem, rows = concat_map(3, 4 * (16 // eb))
    plan = hip.GatherPlan(rows, src, elem, eb, route='run_copy')
    assert plan.info()['route'] == 'run_copy'
    for n in counts(plan):
        guarded_run(plan, src, elem, rows, eb, n, poison, src_at, out_at, f'run_copy eb{eb} {variant[0]} n{n}')
    plan.close()


# -- tile -----------------------------------------------------------------------------------------------------
def stretch_map(eb):
    """3 sources of 64-byte rows of which bytes [8, 40) are used, the middle source's backwards: the plan
    stages [0, 48), whole 16-byte pieces."""
    per = 64 // eb
    lo, hi = 8 // eb, 40 // eb
    src = np.repeat(np.arange(3, dtype=np.int32), hi - lo)
    one = np.arange(lo, hi, dtype=np.int64)
    return src, np.concatenate([one, one[::-1], one]), [per] * 3


def tile_map(name, eb):
    if name == 'interleave3x3':
        return interleave_map(3, 3)
    if name == 'transpose24x2':
        _, src, elem = index_map(lambda d: d.transpose(0, 2, 1), [(24, 2)])
        return src, elem, [48]
    return stretch_map(eb)


def mask_kind(rows, eb, src_at):
    """Which sources the tile kernel stages 16 bytes a lane (bbt_gather_execute: the row a multiple of 16 bytes
    and the staged stretch, which then starts at a multiple of 16 in the row, 16-byte aligned)."""
    bits = [r * eb % 16 == 0 and at % 16 == 0 for r, at in zip(rows, src_at)]
    return 'full' if all(bits) else 'mixed' if any(bits) else 'empty'


def _tile_cases():
    out = []
    for name, n_src in (('interleave3x3', 3), ('transpose24x2', 1), ('stretch8to40', 3)):
        for eb in (1, 2, 4, 8):
            rows = tile_map(name, eb)[2]
            kinds = [('aligned', (0,) * n_src), ('off', (eb,) * n_src)]
            if n_src > 1:
                kinds.append(('first_off', (eb,) + (0,) * (n_src - 1)))
            for kind, src_at in kinds:
                for out_at in (0, eb):
                    ident = (f'{name}-eb{eb}-src_{kind}-out_{"off" if out_at else "aligned"}-'
                             f'mask_{mask_kind(rows, eb, src_at)}-vec_out{0 if out_at else 1}')
                    out.append(pytest.param(name, eb, src_at, out_at, id=ident))
    return out


@pytest.mark.parametrize('name, eb, src_at, out_at', _tile_cases())
@both_poisons
def test_tile_masks_and_output_widths(name, eb, src_at, out_at, poison):
    src, elem, rows = tile_map(name, eb)
    plan = hip.GatherPlan(rows, src, elem, eb, route='tile')
    assert plan.info()['route'] == 'tile'
    for n in counts(plan):
        guarded_run(plan, src, elem, rows, eb, n, poison, src_at, out_at, f'tile {name} eb{eb} {src_at} {out_at} n{n}')
    plan.close()


def test_tile_cases_reach_every_mask():
    """The table above, not the device: all three kinds of `vec_mask` under both `vec_out`, at every element size."""
    seen = {(p.values[1], mask_kind(tile_map(p.values[0], p.values[1])[2], p.values[1], p.values[2]), p.values[3] == 0)
            for p in _tile_cases()}
    assert seen == {(eb, kind, vo) for eb in (1, 2, 4, 8) for kind in ('full', 'mixed', 'empty') for vo in (True, False)}


# -- direct ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eb', [1, 2, 4, 8, 16])
@both_poisons
def test_direct_at_the_smallest_offset(eb, poison):
    """The random map (repeats, gaps, any order) of `test_routes_agree_with_numpy`; every pointer one element
    off 16 (a 16-byte element allows none)."""
    rng = np.random.default_rng(100 * eb + 3)
    src = rng.integers(0, 3, 50).astype(np.int32)
    rows = [int(r) for r in rng.integers(1, 12, 3)]
    elem = np.array([rng.integers(0, rows[s]) for s in src], np.int64)
    plan = hip.GatherPlan(rows, src, elem, eb, route='direct')
    for n in counts(plan):
        guarded_run(plan, src, elem, rows, eb, n, poison, (eb % 16,) * 3, eb % 16, f'direct eb{eb} n{n}')
    plan.close()


# -- the tasks ------------------------------------------------------------------------------------------------
def test_stack_hands_on_a_view_off_16(monkeypatch):
    """Two streams of complex64 (3,), rows of 24 bytes, that start 13 samples apart: the earlier one is handed
    to the plan as a view 13 rows into its array, 8 bytes off 16."""
    rng = np.random.default_rng(5)
    n, shape = 4000, (3,)
    a = (rng.standard_normal((n,) + shape) + 1j * rng.standard_normal((n,) + shape)).astype(np.complex64)
    b = (rng.standard_normal((n,) + shape) + 1j * rng.standard_normal((n,) + shape)).astype(np.complex64)
    da, db = device_stream(a, 1000), device_stream(b, 1000, start=u.Time(T0) + 13e-6)
    seen = []
    execute = hip.GatherPlan.execute

    def watched(self, sources, out_dev, n_samples, first_samples=None):
        seen.append([s.ptr % 16 for s in sources])
        return execute(self, sources, out_dev, n_samples, first_samples)
    monkeypatch.setattr(hip.GatherPlan, 'execute', watched)
    st = bt.Stack([da, db], axis=-1, samples_per_frame=1000)
    want = np.stack([a[13:], b[:-13]], axis=-1)
    got = st.read()
    assert seen and all(p == [8, 0] for p in seen), seen
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    del seen[:]
    tr = bt.Transpose(bt.Stack([device_stream(a, 1000), device_stream(b, 1000, start=u.Time(T0) + 13e-6)], axis=-1,
                               samples_per_frame=1000), (2, 1))
    got = tr.read()
    assert [8, 0] in seen, seen
    assert got.tobytes() == np.ascontiguousarray(want.transpose(0, 2, 1)).tobytes()
