"""`Accelerate` without a GPU: the rule of `periodicity.accelerate_rows` against exact rational arithmetic,
its properties at the bound, the window formula, the twin, the task's surface and refusals, the grid, the
3-D candidate search, and csrc/accel_geo.hpp -- the rule's C++ definition and the kernel's indexing --
walked on the host under the sanitizers and compared with the NumPy rule (tests/accel_geo_check.cpp)."""
import json
import os
import re

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity
from baseband_tasks_amd.periodicity import LEVEL, OFFSET, SNR

import accel_cases
from accel_cases import CASES, IDS, RATE, T0, same_words, words
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')
#: the block lengths the bound is checked at (2^22 and 2^24 in the slow half of a second each)
BOUND_LENGTHS = [2, 3, 5, 64, 500, 512, 1000, 4096, 1 << 15, 1 << 22, 1 << 24]


# -- the rule -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, k', [(512, 2. ** -11), (512, -2. ** -11), (1000, -2. ** -12), (500, 2. ** -11),
                                  (64, 2. ** -8), (64, -2. ** -9), (2, .125), (3, -2. ** -4), (4096, 2. ** -14)])
def test_rows_against_exact_arithmetic(n, k):
    """Power-of-two factors: the product is exact, so the rule's one rounding is the rounding to an
    integer, and it must be half-even."""
    got = periodicity.accelerate_rows(n, [k, 0., -k])
    assert got.dtype == np.int64 and got.shape == (3, n)
    assert got[0].tolist() == accel_cases.exact_rows(n, k)
    assert got[1].tolist() == list(range(n))
    assert got[2].tolist() == accel_cases.exact_rows(n, -k)
    if (n, abs(k)) in ((512, 2. ** -11), (1000, 2. ** -12)):
        tied = accel_cases.ties(n, k) + accel_cases.ties(n, -k)
        assert len(tied) >= 8 and {up for _, up in tied} == {False, True}     # (ties, rounded both ways)


@pytest.mark.parametrize('n', BOUND_LENGTHS)
def test_rows_at_the_bound(n):
    """|k| n = 1/4, both signs: in range, never a step back, steps of 0, 1 or 2, at most n / 16 rows away,
    zero at both ends, and not increasing with k."""
    k = .25 / n
    i = np.arange(n)
    before = None
    for factor in (k, k / 2, -k):                                  # (one at a time: 2^24 rows are 128 MiB)
        src = periodicity.accelerate_rows(n, [factor])[0]
        assert src.min() >= 0 and src.max() <= n - 1 and src[0] == 0 and src[n - 1] == n - 1
        step = np.diff(src)
        assert step.min() >= 0 and step.max() <= 2
        assert np.abs(src - i).max() <= n / 16 + .5
        assert (src <= i).all() if factor > 0 else (src >= i).all()
        assert before is None or (before <= src).all()
        before = src


def test_rows_refusals():
    assert periodicity.accelerate_rows(2, [.125]).tolist() == [[0, 1]]
    for n, k in ((64, [1. / 255.]), (64, [0., -1. / 255.]), (64, [np.nan]), (64, [np.inf]), (1 << 24, [2. ** -25])):
        with pytest.raises(ValueError, match='1/4'):
            periodicity.accelerate_rows(n, k)
    for n in (1, 0, (1 << 24) + 1):
        with pytest.raises(ValueError, match='block'):
            periodicity.accelerate_rows(n, [0.])
    with pytest.raises(ValueError, match='trials'):
        periodicity.accelerate_rows(64, [])
    with pytest.raises(ValueError, match='trials'):
        periodicity.accelerate_rows(64, np.zeros(4097))
    with pytest.raises(ValueError, match='trials'):
        periodicity.accelerate_rows(64, np.zeros((2, 2)))
    with pytest.raises(TypeError):
        periodicity.accelerate_rows(64., [0.])
    assert periodicity.accelerate_rows(64, np.zeros(4096)).shape == (4096, 64)


def test_factors():
    a = [50., -3., 0.]
    k = periodicity.acceleration_factors(a, 15625.)
    assert k.dtype == np.float64 and k.tolist() == [v / (2. * 299792458. * 15625.) for v in a]
    assert periodicity.C_LIGHT == 299792458.
    assert periodicity.acceleration_factors(7., 10.).shape == (1,)
    for bad in ([np.nan], [np.inf], [], np.zeros(4097), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            periodicity.acceleration_factors(bad, 1e3)
    for rate in (0., -1., np.inf):
        with pytest.raises(ValueError, match='rate'):
            periodicity.acceleration_factors([1.], rate)


def test_window_is_the_extent_of_the_table():
    """For random runs of rows, also across blocks, the window formula gives exactly the smallest and the
    largest input row the table names."""
    rng = np.random.default_rng(11)
    for case in CASES[:8]:
        n = case.n
        src = periodicity.accelerate_rows(n, case.factors)
        k_min, k_max = min(case.factors), max(case.factors)
        table = np.concatenate([src + q * n for q in range(3)], axis=1)          # three blocks
        for _ in range(60):
            g0 = int(rng.integers(0, 3 * n))
            g1 = int(min(3 * n - 1, g0 + rng.integers(0, rng.choice([1, 3, n, 2 * n + 1]))))
            lo, hi = periodicity._accel_window(n, k_min, k_max, g0, g1)
            assert (lo, hi) == (table[:, g0:g1 + 1].min(), table[:, g0:g1 + 1].max()), (case.name, g0, g1)


# -- the twin -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_is_the_table_applied(case):
    x, got = accel_cases.data(case), accel_cases.expected(case)
    nb = case.length // case.n
    assert got.dtype == np.float32 and got.shape == (nb * case.n, len(case.factors)) + case.shape
    src = periodicity.accelerate_rows(case.n, case.factors)
    rng = np.random.default_rng(5)
    for _ in range(50):
        q, i, j = int(rng.integers(nb)), int(rng.integers(case.n)), int(rng.integers(len(case.factors)))
        assert np.array_equal(words(got[q * case.n + i, j]), words(x[q * case.n + src[j, i]]))
    # every planted pattern is still there, to the bit
    assert x.size < 1000 or set(accel_cases.SPECIALS.tolist()) <= set(words(x).reshape(-1).tolist())
    for j, k in enumerate(case.factors):
        if k == 0.:
            assert same_words(got[:, j], x[:nb * case.n])                # the identity, NaN payloads and -0 included


def test_twin_refusals():
    x = np.zeros((100, 2), np.float32)
    assert periodicity.accelerate_samples(x, [0.], 50).shape == (100, 1, 2)
    assert periodicity.accelerate_samples(x[:, 0], [0., 1e-3], 33).shape == (99, 2)
    with pytest.raises(ValueError, match='less than one block'):
        periodicity.accelerate_samples(x, [0.], 101)
    with pytest.raises(TypeError):
        periodicity.accelerate_samples(x.astype(np.float64), [0.], 50)
    with pytest.raises(ValueError, match='1/4'):
        periodicity.accelerate_samples(x, [.01], 50)


# -- the task's surface -------------------------------------------------------------------------------------
def _plane(length, shape=(4,), dtype=np.float32, rate=RATE, **kwargs):
    return bt.HostStream(np.zeros((length,) + shape, dtype), bt.Time(T0), rate, pin=False, **kwargs)


def test_construction_and_metadata():
    n = 500
    src = _plane(2 * n + 1, (2, 3), frequency=np.array([[1e8], [2e8]]), sideband=np.array([1, -1, 1]),
                 polarization=np.array(['X', 'Y', 'X']), samples_per_frame=100)
    accs = [5e7, -2.5e7, 0., 2.5e7]
    task = bt.Accelerate(src, accs, n)
    assert task.dtype == np.float32 and task.shape == (2 * n, 4, 2, 3) and task.n == n
    assert task.sample_rate == src.sample_rate and abs(task.start_time - src.start_time) < 1e-9
    assert task.samples_per_frame == 100
    assert task.accelerations.tolist() == accs
    assert task.factors.tolist() == periodicity.acceleration_factors(accs, RATE).tolist()
    rows = periodicity.accelerate_rows(n, task.factors)
    assert task.max_shift == np.abs(rows - np.arange(n)).max() > 0
    full = (4, 2, 3)
    np.testing.assert_array_equal(np.broadcast_to(task.frequency, full)[3], np.broadcast_to(src.frequency, (2, 3)))
    np.testing.assert_array_equal(np.broadcast_to(task.sideband, full)[0], np.broadcast_to(src.sideband, (2, 3)))
    np.testing.assert_array_equal(np.broadcast_to(task.polarization, full)[1, 1], ['X', 'Y', 'X'])
    assert bt.Accelerate.accel_budget == 1 << 29 == hip.ACCEL_BUDGET
    assert bt.Accelerate(src, accs, n, samples_per_frame=7).samples_per_frame == 7
    # no metadata at all, scalar samples, one trial given as a number
    bare = bt.Accelerate(_plane(64, ()), 0., 64)
    assert bare.shape == (64, 1) and bare.max_shift == 0
    with pytest.raises(AttributeError):
        bare.frequency
    # the downstream tasks take the result as it is
    long = bt.Accelerate(_plane(1 << 15, (2,)), [0., 1.], 1 << 15)
    hs = bt.HarmonicSearch(bt.Whiten(bt.LongSpectra(long, 1 << 15), 128), 64, n_levels=4)
    assert hs.shape == (1, 257, 3, 2, 2)


def test_a_lone_frequency_is_passed_on():
    src = bt.HostStream(np.zeros((2000, 4), np.float32), bt.Time(T0), 1e4, pin=False,
                        frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(src, [0., .1, .2])
    task = bt.Accelerate(plane, [0., 3.], 512)
    assert task.frequency == plane.frequency and task.shape == (plane.shape[0] // 512 * 512, 2, 3)
    with pytest.raises(AttributeError):
        task.sideband


def test_input_span_is_the_window():
    case = accel_cases.by_name('n64')
    n = case.n
    accs = np.array(case.factors) * (.999 * 2. * periodicity.C_LIGHT * RATE)
    src = _plane(case.length, case.shape)
    task = bt.Accelerate(src, accs, n, samples_per_frame=16)
    table = periodicity.accelerate_rows(n, task.factors)
    table = np.concatenate([table + q * n for q in range(3)], axis=1)
    for first, last in ((0, 1), (1, 3), (3, 5), (0, 12), (11, 12)):
        span = task._input_span(first, last)
        a, b = first * 16, min(last * 16, 3 * n)
        lo, hi = table[:, a:b].min(), table[:, a:b].max()
        assert span[0] is src and span[1:] == (lo, hi + 1 - lo), (first, last)
    # more rows than a chunk holds: no single fetch
    task.accel_budget = 17 * 5 * 3 * 4
    assert task._chunk_size() == 17 and task._input_span(0, 2) is None and task._input_span(0, 1) is not None
    task.accel_budget = 1
    assert task._chunk_size() == 1


def test_what_the_task_refuses():
    src = _plane(1000)
    bt.Accelerate(src, [0.], 1000)
    with pytest.raises(TypeError, match='Square'):
        bt.Accelerate(_plane(1000, dtype=np.complex64), [0.], 64)
    with pytest.raises(TypeError, match='float32'):
        bt.Accelerate(_plane(1000, dtype=np.float64), [0.], 64)
    with pytest.raises(ValueError, match='less than one block'):
        bt.Accelerate(src, [0.], 1001)
    for n in (1, 0, -5, (1 << 24) + 1):
        with pytest.raises(ValueError, match='block'):
            bt.Accelerate(src, [0.], n)
    with pytest.raises(TypeError):
        bt.Accelerate(src, [0.], 64.)
    for accs in ([], np.zeros(4097), np.zeros((2, 2)), [np.nan], [0., np.inf]):
        with pytest.raises(ValueError):
            bt.Accelerate(src, accs, 64)
    # |k| n <= 1/4:  a = 2 c rate k
    edge = .25 / 64 * 2. * periodicity.C_LIGHT * RATE
    assert bt.Accelerate(src, [edge * (1 - 1e-12), -edge * (1 - 1e-12)], 64).max_shift == 4
    for accs in ([edge * 1.001], [0., -edge * 1.001]):
        with pytest.raises(ValueError, match='1/4'):
            bt.Accelerate(src, accs, 64)
    with pytest.raises(ValueError, match='element'):
        bt.Accelerate(_plane(1000, (0,)), [0.], 64)


# -- the grid -----------------------------------------------------------------------------------------------
def test_acceleration_grid():
    n, rate = 1 << 20, 15625.
    grid = periodicity.acceleration_grid(50., n, rate)
    step = 8. * periodicity.C_LIGHT * rate / float(n) ** 2
    reach = int(np.ceil(50. / step))
    assert grid.shape == (2 * reach + 1,) and grid[reach] == 0. and (grid == -grid[::-1]).all()
    assert np.allclose(np.diff(grid), step, rtol=1e-12) and grid[-1] >= 50. > grid[-2]
    # neighbours differ by `tol` samples in the middle of a block
    for tol in (1., .5, 3.):
        g = periodicity.acceleration_grid(50., n, rate, tol)
        k = periodicity.acceleration_factors(g, rate)
        assert np.allclose(np.diff(k) * float(n) ** 2 / 4., tol, rtol=1e-9)
    assert periodicity.acceleration_grid(0., n, rate).tolist() == [0.]
    # the cap: 4095 trials pass, 4097 do not
    assert periodicity.acceleration_grid(2047 * step * (1 - 1e-9), n, rate).shape == (4095,)
    with pytest.raises(ValueError, match='4096'):
        periodicity.acceleration_grid(2047.5 * step, n, rate)
    for bad in ((-1., n, rate, 1.), (1., 1, rate, 1.), (1., n, 0., 1.), (1., n, rate, 0.), (np.nan, n, rate, 1.)):
        with pytest.raises(ValueError):
            periodicity.acceleration_grid(*bad)


# -- the candidates -----------------------------------------------------------------------------------------
def _cube():
    """(blocks 4, 3, A 3, ndm 4) by hand: a plateau of three equal cells, a peak in a corner, a peak next
    to NaNs, and a cell below the threshold."""
    best = np.zeros((4, 3, 3, 4), np.float32)
    best[:, SNR] = 1.
    best[1, SNR, 1, 1] = best[1, SNR, 1, 2] = best[2, SNR, 0, 1] = 9.      # a plateau: its first cell in raster order
    best[0, SNR, 0, 3] = 12.                                               # a corner of the cube
    best[3, SNR, 2, 0] = 7.
    best[3, SNR, 1, 0] = best[2, SNR, 2, 0] = best[3, SNR, 2, 1] = np.nan  # NaNs around a peak: no neighbours
    best[3, SNR, 0, 3] = 4.                                                # below the threshold
    best[1, OFFSET, 1, 1], best[1, LEVEL, 1, 1] = 10., 2.
    best[0, OFFSET, 0, 3], best[0, LEVEL, 0, 3] = 63., 0.
    best[3, OFFSET, 2, 0], best[3, LEVEL, 2, 0] = 5., 1.
    return best


def test_acceleration_candidates_on_a_cube_made_by_hand():
    best = _cube()
    accs = [-1.5, 0., 1.5]
    c = periodicity.acceleration_candidates(best, 64, 5., .25, accs)
    assert c.dtype.names == ('bin', 'trial', 'harmonics', 'snr', 'frequency', 'acc', 'acceleration')
    assert c['snr'].tolist() == [12., 9., 7.]
    assert c['acc'].tolist() == [0, 1, 2] and c['trial'].tolist() == [3, 1, 0]
    assert c['bin'].tolist() == [63., (64 + 10) / 4., (3 * 64 + 5) / 2.] and c['harmonics'].tolist() == [1, 4, 2]
    assert c['frequency'].tolist() == (c['bin'] * .25).tolist() and c['acceleration'].tolist() == [-1.5, 0., 1.5]
    plain = periodicity.acceleration_candidates(best, 64, 5.)
    assert plain.dtype.names == ('bin', 'trial', 'harmonics', 'snr', 'acc') and plain['acc'].tolist() == [0, 1, 2]
    # a threshold at the plateau's value keeps it; NaN everywhere gives nothing
    assert periodicity.acceleration_candidates(best, 64, 9.)['snr'].tolist() == [12., 9.]
    assert len(periodicity.acceleration_candidates(np.full_like(best, np.nan), 64, 0.)) == 0
    # diagonal neighbours in all three axes count: a larger cell at (+1, +1, +1) removes the plateau's cell
    best[2, SNR, 2, 2] = 9.5
    assert periodicity.acceleration_candidates(best, 64, 5.)['snr'].tolist() == [12., 9.5, 7.]
    for bad in (best[:, :, 0], best[:, :2], best[0]):
        with pytest.raises(ValueError, match='blocks, 3, A, ndm'):
            periodicity.acceleration_candidates(bad, 64, 5.)
    with pytest.raises(ValueError, match='accelerations'):
        periodicity.acceleration_candidates(best, 64, 5., None, [0., 1.])


def test_one_trial_is_harmonic_candidates_and_that_is_unchanged():
    rng = np.random.default_rng(8)
    best = np.empty((40, 3, 1, 6), np.float32)
    best[:, SNR] = rng.integers(0, 6, (40, 1, 6))                          # many ties
    best[:, OFFSET] = rng.integers(0, 32, (40, 1, 6))
    best[:, LEVEL] = rng.integers(0, 4, (40, 1, 6))
    best[3, SNR, 0, 2] = np.nan
    got = periodicity.acceleration_candidates(best, 32, 2., .5)
    want = periodicity.harmonic_candidates(best[:, :, 0], 32, 2., .5)
    assert len(got) == len(want) > 10 and (got['acc'] == 0).all()
    for name in want.dtype.names:
        assert np.array_equal(got[name], want[name]), name
    # harmonic_candidates itself: the 2-D rule, restated cell by cell
    snr = best[:, SNR, 0]
    keep = []
    for b in range(40):
        for d in range(6):
            v = snr[b, d]
            if not v >= 2.:
                continue
            ok = True
            for db in (-1, 0, 1):
                for dd in (-1, 0, 1):
                    bb, ee = b + db, d + dd
                    if (db, dd) == (0, 0) or not (0 <= bb < 40 and 0 <= ee < 6):
                        continue
                    o = snr[bb, ee]
                    if o > v or (o == v and (db, dd) < (0, 0)):
                        ok = False
            if ok:
                keep.append((b, d))
    assert sorted(zip(((want['bin'] * want['harmonics']).astype(int) // 32).tolist(), want['trial'].tolist())) == keep


# -- the library's surface ----------------------------------------------------------------------------------
def test_library_exports_and_limits():
    lib = hip.lib()
    assert lib.bbt_version() >= 167
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_accel_plan_create', 'bbt_accel_plan_destroy', 'bbt_accel_plan_info', 'bbt_accel_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'accel_geo.hpp')).read()
    for name, value in (('MIN_N', hip.ACCEL_MIN_N), ('MAX_TRIALS', hip.ACCEL_MAX_TRIALS),
                        ('LDS_BYTES', hip.ACCEL_LDS_BYTES), ('TILE_UNITS', hip.ACCEL_TILE_UNITS),
                        ('MAX_ROWS', hip.ACCEL_MAX_ROWS)):
        assert re.search(rf'#define BBT_ACCEL_{name} {value}\s', geo), name
    assert '#define BBT_ACCEL_MAX_N (1 << 24)' in geo and hip.ACCEL_MAX_N == 1 << 24
    assert '#define BBT_ACCEL_MAX_WIDTH (1ll << 28)' in geo and hip.ACCEL_MAX_WIDTH == 1 << 28
    assert '#define BBT_ACCEL_BUDGET (1ll << 29)' in geo and hip.ACCEL_BUDGET == 1 << 29
    names = ('Accelerate', 'accelerate_samples', 'accelerate_rows', 'acceleration_factors', 'acceleration_grid',
             'acceleration_candidates')
    assert all(name in periodicity.__all__ for name in names)
    assert bt.Accelerate is periodicity.Accelerate and bt.accelerate_samples is periodicity.accelerate_samples
    # every size and factor is refused before anything touches a device
    for args, what in (((1, 2, [0.]), r'2\^24'), (((1 << 24) + 1, 2, [0.]), r'2\^24'), ((64, 0, [0.]), 'elements'),
                       ((64, 2, []), 'trials'), ((64, 2, np.zeros(4097)), 'trials'),
                       ((64, 1 << 17, np.zeros(4096)), r'2\^28'), ((64, 2, [0., 1. / 255.]), '1/4'),
                       ((64, 2, [np.nan]), '1/4')):
        with pytest.raises(hip.HipError, match=what):
            hip.AccelPlan(*args)
    with pytest.raises(ValueError):
        hip.AccelPlan(64, 2, np.zeros((2, 2)))


# -- the index maps -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def geo_check(tmp_path_factory):
    return compile_check('accel_geo_check', tmp_path_factory.mktemp('accel'), opt='-O2')


def _walk_groups():
    """(n_rows, n, n_elem, unit, route, chunk, factors): every case of the table under every route, whole and
    in chunks of 1 row, of 37 rows and of a block and a half; the 16-byte unit wherever the elements allow
    it; and calls whose rows run past 2^31 values."""
    groups = []
    for case in CASES:
        n_elem = int(np.prod(case.shape, dtype=np.int64))
        units = (4, 16) if n_elem % 4 == 0 else (4,)
        chunks = (case.length,) if case.n >= 4096 else (case.length, 1, 37, case.n + case.n // 2)
        if len(case.factors) > 1000:
            chunks = (case.length, 37)                 # (every group repeats its factors on the command line)
        for unit in units:
            for route in (0, 1, 2):
                for chunk in chunks:
                    groups.append((case.length, case.n, n_elem, unit, route, chunk, case.factors))
    k = 1e-3 / (1 << 22)
    # 2^22 rows of 64 trials x 8 elements: 2^31 values, in launches of 2^29 bytes; and one launch of 2^33 values
    groups.append((1 << 22, 1 << 22, 8, 16, 0, (1 << 29) // (4 * 512), tuple(np.linspace(-k, k, 64))))
    groups.append((1 << 22, 1 << 22, 8, 4, 1, (1 << 29) // (4 * 512), tuple(np.linspace(-k, k, 64))))
    groups.append((1 << 24, 1 << 24, 64, 4, 2, 1 << 24, (-2. ** -26, 0., 2. ** -26, 1e-9, 1e-10, -1e-9, 3e-9, 5e-9)))
    # rows wider than a tile, cut into segments: walked whole, and past 2^31
    groups.append((64, 64, 20000, 4, 0, 64, (0., 1. / 512.)))
    groups.append((3 << 20, 1 << 20, 65536, 16, 0, 3 << 20, (-2. ** -22, 2. ** -22)))
    return groups


def _hex(factors):
    return tuple(float(k).hex() for k in factors)


def _walk_args(groups):
    return [(n_rows, n, n_elem, unit, route, chunk, len(factors)) + _hex(factors)
            for n_rows, n, n_elem, unit, route, chunk, factors in groups]


def test_kernel_indexing_on_the_host(geo_check):
    """Thread by thread, the loops of k_accel write every output unit of a launch exactly once, read only
    inside the window of their tile, which lies inside the input piece, stay below the LDS the kernel
    declares, and every tile lies in one block: the program reports otherwise, and the sanitizers abort it
    on a wild index or an overflow of its own."""
    groups = _walk_groups()
    lines = run_check(geo_check, _walk_args(groups), word='walk')
    past = 0
    for (n_rows, n, n_elem, unit, route, chunk, factors), g in zip(groups, lines):
        assert g.get('walk') == 0, g
        per = unit // 4
        width = n_elem // per * len(factors)
        assert g['rows'] == min(hip.ACCEL_MAX_ROWS, max(1, hip.ACCEL_TILE_UNITS // width))
        assert g['nx'] * g['ny'] == 256 and g['lds_units'] * unit == hip.ACCEL_LDS_BYTES
        assert g['n_seg'] == -(-width // hip.ACCEL_TILE_UNITS) and g['tpb'] == -(-n // g['rows'])
        length = n_rows // n * n
        assert g['launches'] >= min(2, -(-length // chunk))
        if route == 2 or 2 * (n_elem // per) > g['lds_units'] or g['n_seg'] > 1 or (route == 0 and n_elem < 4):
            assert g['staged'] == 0
        elif (g['rows'] + 2 * (max(abs(k) for k in factors) * n * n / 4 + 1)) * (n_elem // per) <= g['lds_units']:
            assert g['direct'] == 0, (n_rows, n, n_elem, unit, route, chunk, g)       # (every window fits)
        if n == 1 << 15:
            assert g['direct'] > 0            # (shifts of 2048 rows: no window of the middle fits)
        past += g['max_out'] * per >= 1 << 31
    assert past >= 2
    # the rows of the table that are wider than a tile: cut into segments in either unit, but for the fence
    # post, which in units of 16 bytes is exactly one tile wide
    seen = {(n_elem * len(factors), unit): g for (_, n, n_elem, unit, _, _, factors), g in zip(groups, lines) if n == 32}
    assert sorted(seen) == [(16510, 4), (65536, 4), (65536, 16), (65600, 4), (65600, 16)]
    assert [(seen[key]['n_seg'], seen[key]['ws'], seen[key]['rows']) for key in sorted(seen)] == [
        (2, 16384, 1), (4, 16384, 1), (1, 16384, 1), (5, 16384, 1), (2, 16384, 1)]
    # what the library refuses
    bad = run_raw(geo_check, '64 1 1 4 0 8 1 0  64 64 0 4 0 8 1 0  64 64 1 4 0 8 0  64 64 1 4 0 8 1 0.004'
                  '  64 64 2 16 0 8 1 0  10 64 1 4 0 8 1 0', word='walk')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 6 and '2^24' in errors[0] and 'elements' in errors[1] and 'trials' in errors[2]
    assert '1/4' in errors[3] and '16-byte' in errors[4] and 'block' in errors[5]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_the_rule_in_the_header_is_the_rule_in_numpy(case, geo_check, tmp_path):
    """accel_src of csrc/accel_geo.hpp -- what the launcher and the kernel call -- against `accelerate_rows`."""
    path = str(tmp_path / 'src.i64')
    assert run_raw(geo_check, [(case.n, path) + _hex(case.factors)], word='maps').returncode == 0
    got = np.fromfile(path, dtype=np.int64).reshape(len(case.factors), case.n)
    assert np.array_equal(got, periodicity.accelerate_rows(case.n, case.factors))


def test_the_rule_in_the_header_at_the_bound(geo_check, tmp_path):
    for n in (3, 1000, 1 << 22):
        k = [.25 / n, -.25 / n, .1 / n]
        path = str(tmp_path / f'src{n}.i64')
        assert run_raw(geo_check, [(n, path) + _hex(k)], word='maps').returncode == 0
        assert np.array_equal(np.fromfile(path, dtype=np.int64).reshape(3, n), periodicity.accelerate_rows(n, k))


# -- a binary pulsar, on the twins --------------------------------------------------------------------------
def test_the_twins_find_the_planted_binary_pulsar():
    """What test_accel_gpu.py asserts of the device chain, asserted of the NumPy twins first: the planted
    amplitude was fixed on this test alone."""
    x = accel_cases.pulsar_plane()
    n = accel_cases.PULSAR_N
    y = periodicity.accelerate_samples(x, accel_cases.PULSAR_TRIALS, n)
    spectra = periodicity.long_spectra_samples(y, n)
    best = periodicity.harmonic_search_samples(periodicity.whiten_samples(spectra, 128), 64, 4, 1., 1)
    assert best.shape == (1, 257, 3, 5, 2)
    accel_cases.pulsar_verdict(best[0], RATE / n)
