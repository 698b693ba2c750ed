"""Shared cases of the correlator tests (test_corr_host.py walks the geometry and proves the NumPy
restatement, test_corr_gpu.py and test_corr_guard_gpu.py hold the kernels to the rule): a table of small
shapes chosen where the kernel can go wrong -- full and ragged tiles, 1, 3, 6 and 10 tiles, fewer elements
than a tile packs, odd tails in the k pair, segment edges, several segments -- their integer and Gaussian
data, the exact integer results, the float64 values and the derived error bound."""
import collections
import functools

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import correlation

T0 = '2010-11-12T13:14:15'
RATE = 1e4
SEG = 1024

Case = collections.namedtuple('Case', 'name sample_shape axis n blocks tail')


def _case(a, rest, n, blocks, tail=0, axis=-1, name=None):
    """Inputs last unless ``axis`` says otherwise: ``rest`` are the other axes of the sample."""
    rest = tuple(rest)
    nd = len(rest) + 1
    ax = axis % nd
    shape = rest[:ax] + (a,) + rest[ax:]
    elements = int(np.prod(rest)) if rest else 1
    return Case(name or f'a{a}-e{elements}-n{n}-b{blocks}' + (f'-t{tail}' if tail else ''), shape, axis, n, blocks, tail)


#: every A of (2, 3, 4, 5, 8, 15, 16, 17, 32, 33, 64) meets an odd n and a segment edge; elements 1, 3, 7, 9, 40; n of
#: 1, 2, 3, 7, 1023, 1024, 1025, 2051, 3072; 1 to 3 blocks with and without a dropped tail; two cases whose inputs
#: are not the last axis
CASES = [
    _case(2, (40,), 1024, 3, 5), _case(2, (), 7, 3),
    _case(3, (7,), 1025, 2, 3), _case(3, (9,), 3, 3),
    _case(4, (9,), 2051, 1), _case(4, (3,), 1, 3),
    _case(5, (7,), 1023, 2, 1), _case(5, (40,), 2, 3),
    _case(8, (3,), 3072, 1, 100), _case(8, (7,), 7, 2),
    _case(15, (3,), 1025, 2), _case(15, (), 3, 1, 2),
    _case(16, (9,), 2051, 2), _case(16, (40,), 1023, 1),
    _case(17, (3,), 1025, 2, 7), _case(17, (7,), 7, 3),
    _case(32, (3,), 2051, 1), _case(32, (), 1023, 2),
    _case(33, (3,), 1025, 1, 1), _case(33, (7,), 3, 2),
    _case(64, (3,), 2051, 2), _case(64, (), 1023, 1, 3),
    _case(5, (7,), 1025, 2, 0, axis=0, name='axis0-a5-e7-n1025-b2'),
    _case(4, (3, 5), 7, 2, 1, axis=1, name='axis1-a4-e15-n7-b2-t1'),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
assert len(BY_NAME) == len(CASES)
#: the cases whose integer data differ between all (input, element) of every sample
DISTINCT = ('a8-e7-n7-b2', 'a17-e7-n7-b3')
#: the cases of the independence runs: 1 tile full, 3 tiles ragged, 10 tiles full, and packed elements
INDEPENDENCE = ('a16-e9-n2051-b2', 'a17-e3-n1025-b2-t7', 'a64-e3-n2051-b2', 'a3-e7-n1025-b2-t3')
#: the cases of the guard-band runs
GUARDED = ('a3-e7-n1025-b2-t3', 'a17-e3-n1025-b2-t7', 'a33-e3-n1025-b1-t1')


def n_inputs(case):
    return case.sample_shape[case.axis]


def n_elem(case):
    return int(np.prod(case.sample_shape)) // n_inputs(case)


def n_samples(case):
    return case.n * case.blocks + case.tail


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def integer_data(name):
    """complex64 with integer parts in [-7, 7], read-only.  For the DISTINCT cases no two (input, element) of a
    sample hold the same value: a swapped row or column or a missing conjugate changes the result."""
    case = BY_NAME[name]
    rng = np.random.default_rng(1000 + IDS.index(name))
    shape = (n_samples(case),) + case.sample_shape
    if name in DISTINCT:
        per = int(np.prod(case.sample_shape))
        assert per <= 225
        grid = (np.arange(225) // 15 - 7) + 1j * (np.arange(225) % 15 - 7)
        x = np.stack([grid[rng.permutation(225)[:per]] for _ in range(shape[0])]).reshape(shape)
    else:
        x = rng.integers(-7, 8, shape) + 1j * rng.integers(-7, 8, shape)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def gaussian_data(name):
    case = BY_NAME[name]
    rng = np.random.default_rng(2000 + IDS.index(name))
    shape = (n_samples(case),) + case.sample_shape
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    x.setflags(write=False)
    return x


def _blocks_last(x, case):
    """(blocks, n, elements..., A) of the whole blocks of ``x``, the inputs last."""
    ax = case.axis % len(case.sample_shape)
    y = np.moveaxis(x[:case.n * case.blocks], 1 + ax, -1)
    return y.reshape((case.blocks, case.n) + y.shape[1:]), ax


def _gram(p, q, pairs):
    """sum_t p_i q_j for the baselines: (blocks, elements..., B)."""
    return np.einsum('bt...i,bt...j->b...ij', p, q)[..., pairs[:, 0], pairs[:, 1]]


@functools.lru_cache(maxsize=None)
def integer_sums(name):
    """The exact sums of the integer data, (re, im) as int64 arrays in the output's layout."""
    case = BY_NAME[name]
    y, ax = _blocks_last(integer_data(name), case)
    re, im = np.rint(y.real).astype(np.int64), np.rint(y.imag).astype(np.int64)
    pairs = correlation.baseline_pairs(n_inputs(case))
    sr = _gram(re, re, pairs) + _gram(im, im, pairs)
    si = _gram(im, re, pairs) - _gram(re, im, pairs)
    assert max(np.abs(sr).max(), np.abs(si).max()) < 1 << 24
    return np.moveaxis(sr, -1, 1 + ax), np.moveaxis(si, -1, 1 + ax)


def integer_expected(name, average):
    """complex64: the sums themselves, or float32(total / n) computed in float64."""
    sr, si = integer_sums(name)
    n = np.float64(BY_NAME[name].n)
    out = np.empty(sr.shape, np.complex64)
    out.real = (sr / n if average else sr.astype(np.float64)).astype(np.float32)
    out.imag = (si / n if average else si.astype(np.float64)).astype(np.float32)
    return out


def bound(x, case, average=True):
    """(bound_re, bound_im) in the output's layout: ``(min(n, SEG) + 4) 2^-24 S``, S the float64 sum over the
    block of the absolute values of the real products of the part, divided by n if averaged."""
    y, ax = _blocks_last(x, case)
    re, im = np.abs(y.real.astype(np.float64)), np.abs(y.imag.astype(np.float64))
    pairs = correlation.baseline_pairs(n_inputs(case))
    s_re = _gram(re, re, pairs) + _gram(im, im, pairs)
    s_im = _gram(im, re, pairs) + _gram(re, im, pairs)
    scale = (min(case.n, SEG) + 4) * 2. ** -24 / (case.n if average else 1)
    return np.moveaxis(s_re, -1, 1 + ax) * scale, np.moveaxis(s_im, -1, 1 + ax) * scale


def within_bound(got, want, x, case, average=True):
    """The largest ratio of error to bound over both parts (<= 1 passes); a zero bound demands equality."""
    b_re, b_im = bound(x, case, average)
    worst = 0.
    for err, b in ((np.abs(got.real.astype(np.float64) - want.real), b_re), (np.abs(got.imag.astype(np.float64) - want.imag), b_im)):
        assert (err[b == 0] == 0).all()
        ratio = err[b > 0] / b[b > 0]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.)
    return worst


def stream(x, cls=None, **kwargs):
    """``x`` as a stream: a `HostStream` that is not page-locked, or ``cls`` (`DeviceStream`)."""
    kwargs.setdefault('samples_per_frame', x.shape[0])
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(x, bt.Time(T0), RATE, **kwargs)


def set_tiling(monkeypatch, pack=None, waves=None):
    for name, value in (('BBT_CORR_PACK', pack), ('BBT_CORR_WAVES', waves)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def tilings(a):
    """Every (BBT_CORR_PACK, BBT_CORR_WAVES) setting the geometry accepts for ``a`` inputs."""
    most = 32 // (2 * a) if a <= 16 else 1
    return [(pack, waves) for pack in range(1, most + 1) for waves in (1, 2, 4)]


# -- the shapes corr_geo_check.cpp walks: A E n blocks tail pack waves piece ---------------------------------------
def geo_shapes():
    shapes = []
    for c in CASES:
        a, e = n_inputs(c), n_elem(c)
        for pack, waves in [(0, 0)] + tilings(a):
            shapes.append((a, e, c.n, c.blocks, c.tail, pack, waves, 0))
        # pieces of one segment, of two, and of the blocks two at a time
        shapes.append((a, e, c.n, c.blocks, c.tail, 0, 0, SEG))
        shapes.append((a, e, c.n, c.blocks, c.tail, 0, 0, 2 * SEG))
        shapes.append((a, e, c.n, c.blocks, c.tail, 0, 0, -2))
    # the bench rows
    shapes += [(16, 1024, 1024, 16, 0, 0, 0, -4), (64, 1024, 1024, 4, 0, 0, 0, 0), (16, 1, 1 << 20, 4, 0, 0, 0, 0),
               (2, 1024, 1024, 64, 0, 0, 0, -32), (16, 1, 1 << 24, 1, 0, 0, 0, 1 << 22)]
    return shapes
