"""`LongSpectra` without a GPU: that `periodicity.long_spectra_samples` is the DFT sum it claims to be,
the task's surface and refusals, the routing of `fluctuation_spectra`, a NumPy model of the kernels'
decomposition driven by the very index maps the kernels use (tests/lspec_geo_check.cpp prints them
from csrc/lspec_geo.hpp), and the walk of those maps under the sanitizers."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity

import lspec_cases
from lspec_cases import RATE, T0
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')
LENGTHS = [1 << k for k in range(15, 23)]


# -- the yardstick --------------------------------------------------------------------------------------
def test_yardstick_is_the_dft_sum():
    """n = 32 through the internal entry (the public one takes the long lengths only): against the
    direct sum in float64, stacks of 1 and 3, two output spectra and a tail."""
    rng = np.random.default_rng(3)
    n = 32
    x = rng.standard_normal((2 * 3 * n + 7, 2, 3)).astype(np.float32)
    t = np.arange(n)
    w = np.exp(-2j * np.pi * np.outer(np.arange(n // 2 + 1), t) / n)
    for stack in (1, 3):
        got = periodicity._long_spectra(x, n, stack)
        nspec = x.shape[0] // (n * stack)
        assert got.dtype == np.float32 and got.shape == (nspec, n // 2 + 1, 2, 3)
        for m in range(nspec):
            acc = 0.
            for q in range(stack):
                seg = x[(m * stack + q) * n:(m * stack + q + 1) * n].astype(np.float64)
                acc = acc + np.abs(np.tensordot(w, seg, axes=(1, 0))) ** 2
            want = acc * np.float64(np.float32(1. / stack)) if stack > 1 else acc
            np.testing.assert_allclose(got[m], want, rtol=1e-6, atol=1e-9)
    # stack == 1 applies no scale: a constant gives exactly n^2 in bin 0
    one = periodicity._long_spectra(np.ones((n, 1), np.float32), n, 1)
    assert one[0, 0, 0] == n * n and abs(one[0, 1:]).max() < 1e-20


def test_yardstick_refusals():
    x = np.zeros((1 << 15, 2), np.float32)
    assert periodicity.long_spectra_samples(x, 1 << 15).shape == (1, (1 << 14) + 1, 2)
    for n in (32, 16384, 24576, 1 << 23, 0, -1 << 15):
        with pytest.raises(ValueError, match=r'2\^15.*2\^22'):
            periodicity.long_spectra_samples(x, n)
    with pytest.raises(ValueError, match='stack'):
        periodicity.long_spectra_samples(x, 1 << 15, 0)
    with pytest.raises(ValueError, match='less than one stack'):
        periodicity.long_spectra_samples(x, 1 << 15, 2)
    with pytest.raises(TypeError):
        periodicity.long_spectra_samples(x.astype(np.float64), 1 << 15)
    with pytest.raises(TypeError):
        periodicity.long_spectra_samples(x, 32768.)


# -- the task's surface ---------------------------------------------------------------------------------
def _plane(length, shape=(4,), **kwargs):
    return bt.HostStream(np.zeros((length,) + shape, np.float32), bt.Time(T0), RATE, pin=False, **kwargs)


def test_construction():
    n = 1 << 15
    src = _plane(5 * n + 100, (2, 3), frequency=np.array([[1e8], [2e8]]), sideband=np.array([1, -1, 1]),
                 polarization=np.array(['X', 'Y', 'X']))
    for stack, nspec in ((1, 5), (2, 2), (5, 1)):
        sp = bt.LongSpectra(src, n, stack)
        assert sp.dtype == np.float32 and sp.shape == (nspec, n // 2 + 1, 2, 3)
        assert sp.sample_rate == pytest.approx(RATE / (n * stack), rel=1e-12)
        assert sp.bin_width == RATE / n and sp.n == n and sp.stack == stack
        assert abs(sp.start_time - src.start_time) < 1e-9
        assert sp.samples_per_frame == 1
        full = (n // 2 + 1, 2, 3)
        np.testing.assert_array_equal(np.broadcast_to(sp.frequency, full)[7], np.broadcast_to(src.frequency, (2, 3)))
        np.testing.assert_array_equal(np.broadcast_to(sp.sideband, full)[0], np.broadcast_to(src.sideband, (2, 3)))
        np.testing.assert_array_equal(np.broadcast_to(sp.polarization, full)[3, 1], ['X', 'Y', 'X'])
    assert bt.LongSpectra(src, n, 2, samples_per_frame=2).samples_per_frame == 2
    assert bt.LongSpectra.spectra_budget == 1 << 29 == hip.LSPEC_BUDGET
    # no metadata at all
    bare = bt.LongSpectra(_plane(n, ()), n)
    assert bare.shape == (1, n // 2 + 1)
    with pytest.raises(AttributeError):
        bare.frequency
    # the span of one spectrum is one fetch of the whole stack
    sp = bt.LongSpectra(src, n, 2)
    assert sp._input_span(1, 2) == (src, 2 * n, 2 * n)


def test_a_lone_frequency_is_passed_on():
    src = bt.HostStream(np.zeros((33500, 4), np.float32), bt.Time(T0), 1e4, pin=False,
                        frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(src, [0., .1, .2])
    assert plane.shape[0] >= 1 << 15
    sp = bt.LongSpectra(plane, 1 << 15)
    assert sp.frequency == plane.frequency and sp.shape == (1, (1 << 14) + 1, 3)
    with pytest.raises(AttributeError):
        sp.sideband
    hs = bt.HarmonicSearch(bt.Whiten(sp, 128), 64, n_levels=4)
    assert hs.shape == (1, -(-((1 << 14) + 1) // 64), 3, 3) and hs.frequency == plane.frequency


def test_what_is_refused():
    n = 1 << 15
    src = _plane(2 * n)
    with pytest.raises(TypeError, match='Square'):
        bt.LongSpectra(bt.HostStream(np.zeros((n, 2), np.complex64), bt.Time(T0), RATE, pin=False), n)
    with pytest.raises(TypeError, match='float32'):
        bt.LongSpectra(bt.HostStream(np.zeros((n, 2), np.float64), bt.Time(T0), RATE, pin=False), n)
    for bad in (64, 16384, 24576, 1 << 23, 0, (1 << 15) + 1):
        with pytest.raises(ValueError, match=r'2\^15.*2\^22'):
            bt.LongSpectra(src, bad)
    for stack in (0, -1):
        with pytest.raises(ValueError, match='stack'):
            bt.LongSpectra(src, n, stack)
    with pytest.raises(ValueError, match='less than one stack'):
        bt.LongSpectra(src, n, 3)
    with pytest.raises(ValueError, match='less than one stack'):
        bt.LongSpectra(src, 1 << 17)
    with pytest.raises(TypeError):
        bt.LongSpectra(src, 32768.)
    bt.LongSpectra(src, n, 2)


def test_fluctuation_spectra_routing():
    src = _plane(1 << 22, (1,), frequency=np.array([5e8]), sideband=1)
    for n in (64, 16384):
        sp = bt.fluctuation_spectra(src, n, 2)
        assert not isinstance(sp, bt.LongSpectra) and sp.ih.ih.ih is src
        assert sp.shape == ((1 << 22) // (2 * n), n // 2 + 1, 1) and sp.bin_width == RATE / n
    for n, stack in ((32768, 2), (1 << 22, 1)):
        sp = bt.fluctuation_spectra(src, n, stack)
        assert isinstance(sp, bt.LongSpectra) and sp.ih is src
        assert sp.shape == ((1 << 22) // (n * stack), n // 2 + 1, 1) and sp.bin_width == RATE / n
        assert sp.sample_rate == pytest.approx(RATE / (n * stack), rel=1e-12)
    for n in (24576, 1 << 23):
        with pytest.raises(ValueError, match=r'16384.*2\^15.*2\^22'):
            bt.fluctuation_spectra(src, n)
    with pytest.raises(ValueError, match='stack'):
        bt.fluctuation_spectra(src, 32768, 0)
    with pytest.raises(TypeError):
        bt.fluctuation_spectra(bt.HostStream(np.zeros((1 << 15, 2), np.complex64), bt.Time(T0), RATE, pin=False), 32768)
    # the search builds on a long result as on a short one
    sp = bt.fluctuation_spectra(src, 1 << 20, 4)
    hs = bt.HarmonicSearch(bt.Whiten(sp, 1024), 4096, averaged=4)
    assert hs.shape == (1, -(-((1 << 19) + 1) // 4096), 3, 1)
    assert hs.sample_rate == sp.sample_rate and abs(hs.start_time - src.start_time) < 1e-9


# -- the library's surface ------------------------------------------------------------------------------
def test_library_exports_and_limits():
    lib = hip.lib()
    assert lib.bbt_version() >= 166
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_lspec_plan_create', 'bbt_lspec_plan_destroy', 'bbt_lspec_plan_info', 'bbt_lspec_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'lspec_geo.hpp')).read()
    for name, value in (('MIN_LOG2', hip.LSPEC_MIN_LOG2), ('MAX_LOG2', hip.LSPEC_MAX_LOG2),
                        ('LDS_CELLS', hip.LSPEC_LDS_CELLS), ('MAX_COLS', hip.LSPEC_MAX_COLS),
                        ('MAX_PAIRS', hip.LSPEC_MAX_PAIRS)):
        assert f'#define BBT_LSPEC_{name} {value} ' in geo, name
    assert '#define BBT_LSPEC_MAX_STACK (1 << 20)' in geo and hip.LSPEC_MAX_STACK == 1 << 20
    assert '#define BBT_LSPEC_BUDGET (1ll << 29)' in geo and hip.LSPEC_BUDGET == 1 << 29
    assert periodicity.LONG_LENGTHS == tuple(LENGTHS)
    assert all(name in periodicity.__all__ and hasattr(bt, name) for name in ('LongSpectra', 'long_spectra_samples'))
    # every size is refused before anything touches a device
    for args, what in (((1 << 14, 1, 2), r'2\^15'), ((1 << 23, 1, 2), r'2\^22'), ((24576, 1, 2), 'power of two'),
                       ((1 << 15, 0, 2), 'stack'), ((1 << 15, (1 << 20) + 1, 2), 'stack'),
                       ((1 << 15, 1, 0), 'elements'), ((1 << 22, 1 << 20, 2), r'2\^40')):
        with pytest.raises(hip.HipError, match=what):
            hip.LongSpectraPlan(*args)


# -- the index maps -------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def geo_check(tmp_path_factory):
    return compile_check('lspec_geo_check', tmp_path_factory.mktemp('lspec'), opt='-O2')


def _walk_shapes():
    """(n, n_elem, pairs per launch): all eight lengths with 1, 2, 5, 64 and 513 columns and a count that
    takes the input of one transform past 2^31 values; launches of every kind -- all pairs at once, fewer
    pairs than a workgroup has columns, a ragged last launch, one pair a launch."""
    shapes = []
    for n in LENGTHS:
        small, big = n <= 1 << 16, n >= 1 << 20
        shapes += [(n, 1, 1), (n, 2, 1), (n, 5, 3), (n, 64, 32 if n <= 1 << 18 else 1 if big else 3),
                   (n, 513, 100 if small else 1 if big else 3), (n, (1 << 31) // n + 3, 1 if big else 3)]
        if not big:
            shapes.append((n, 5, 2))
    shapes += [(1 << 16, 7, 1), (1 << 16, 7, 2), (1 << 16, 7, 4), (1 << 18, 66, 33), (1 << 15, 6, 3)]
    return shapes


def test_kernel_indexing_on_the_host(geo_check):
    """Every input sample of a launch read exactly once, every scratch cell written once and read once,
    every output bin 0 ... n / 2 of every element written exactly once and by the workgroup that holds its
    partner n - k, nothing addressed outside its buffer: the program reports otherwise, and the sanitizers
    abort it on a wild index or an overflow of its own."""
    shapes = _walk_shapes()
    plans = run_check(geo_check, shapes, word='walk')
    past = 0
    for (n, n_elem, per), g in zip(shapes, plans):
        assert g['walk'] == 0, g
        lg = n.bit_length() - 1
        assert g['n1'] == 1 << (lg // 2) and g['n1'] * g['n2'] == n
        assert g['c1'] == min(hip.LSPEC_MAX_COLS, hip.LSPEC_LDS_CELLS // g['n1'])
        assert g['cp'] == min(hip.LSPEC_MAX_PAIRS, hip.LSPEC_LDS_CELLS // g['n2'] // 2)
        n_pair = (n_elem + 1) // 2
        assert g['n_launch'] == -(-n_pair // per) and g['walked'] >= min(g['n_launch'], 2)
        assert g['n_wg1'] == g['n2'] * min(per, n_pair) // g['c1']
        assert g['n_wg2'] == g['n1'] // 2 * -(-min(per, n_pair) // g['cp'])
        assert g['max_in'] == n * n_elem - 1 and g['max_out'] == (n // 2 + 1) * n_elem - 1
        past += g['max_in'] >= 1 << 31
    assert past >= len(LENGTHS)
    # what the library refuses
    bad = run_raw(geo_check, '16384 2 1  8388608 2 1  24576 2 1  32768 0 1  32768 2 0', word='walk')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 5 and all('2^15' in e for e in errors[:3]) and 'elements' in errors[3]
    assert 'launch' in errors[4]


def _load(path, name, shape):
    return np.fromfile(os.path.join(path, name + '.i32'), dtype=np.int32).reshape(shape)


@pytest.mark.parametrize('n', LENGTHS, ids=[f'2^{k}' for k in range(15, 23)])
def test_model_of_the_decomposition(n, geo_check, tmp_path):
    """The kernels' route in NumPy, complex64 between the steps, driven by the maps lspec_geo.hpp gives
    the kernels: two columns as one complex stream, n1-point transforms over a, the twiddles W_n^m with
    the printed exponents, the scratch cells, n2-point transforms over b, the partner map, the untangling.
    Against rfft of each column, within the GPU tests' tolerance."""
    info, = run_check(geo_check, [(n, str(tmp_path))], word='maps')
    n1, n2 = info['n1'], info['n2']
    assert n1 * n2 == n
    nk, nh = n2 // 2 + 1, n1 // 2
    in_t, pos1 = _load(tmp_path, 'in_t', (n2, n1)), _load(tmp_path, 'pos1', (n1,))
    exp1, cell1 = _load(tmp_path, 'exp1', (n1, n2)), _load(tmp_path, 'cell1', (n1, n2))
    rows, cell2 = _load(tmp_path, 'rows', (nh, 2)), _load(tmp_path, 'cell2', (nh, 2, n2))
    pos2, partner = _load(tmp_path, 'pos2', (n2,)), _load(tmp_path, 'partner', (nh, 2, nk, 2))
    bins = _load(tmp_path, 'bin', (nh, 2, nk))
    assert sorted(in_t.ravel().tolist()) == list(range(n)) and sorted(cell1.ravel().tolist()) == list(range(n))
    assert sorted(cell2.ravel().tolist()) == list(range(n)) and sorted(rows.ravel().tolist()) == list(range(n1))
    assert sorted(bins[bins >= 0].tolist()) == list(range(n // 2 + 1))
    assert 0 <= exp1.min() and exp1.max() < n

    rng = np.random.default_rng(n.bit_length())
    x = rng.standard_normal((n, 2), dtype=np.float32)
    z = (x[:, 0] + 1j * x[:, 1]).astype(np.complex64)
    # pass 1: the value of k1 is left at position pos1[k1] of the column
    first = np.fft.fft(z[in_t], axis=1).astype(np.complex64)              # [b][k1]
    lds = np.empty_like(first)
    lds[:, pos1] = first
    twiddle = np.exp(-2j * np.pi * exp1.astype(np.float64) / n).astype(np.complex64)    # [k1][b]
    scratch = np.empty(n, np.complex64)
    scratch[cell1] = lds[:, pos1].T * twiddle
    # pass 2
    last = np.fft.fft(scratch[cell2], axis=2).astype(np.complex64)        # [h][ri][k2]
    lds = np.empty_like(last)
    lds[:, :, pos2] = last
    k2 = np.minimum(np.arange(nk), n2 - 1)
    zk = lds[:, :, pos2[k2]]                                              # [h][ri][k2 <= n2 / 2]
    h = np.arange(nh)[:, np.newaxis, np.newaxis]
    zp = lds[h, partner[..., 0], pos2[partner[..., 1]]]
    a = (zk + np.conj(zp)) * np.complex64(.5)
    b = (zk - np.conj(zp)) * np.complex64(-.5j)
    got = np.empty((1, n // 2 + 1, 2), np.float32)
    own = bins >= 0
    got[0, bins[own], 0] = (a.real ** 2 + a.imag ** 2)[own]
    got[0, bins[own], 1] = (b.real ** 2 + b.imag ** 2)[own]
    want = periodicity.long_spectra_samples(x, n)
    lspec_cases.assert_close(got, want, f'model 2^{n.bit_length() - 1}')
