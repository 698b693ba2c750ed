"""Host side of `DMTrials` (no GPU): the shift rule against `DedisperseSamples` and against the
geometry each shared case is named for, the NumPy twin against exact integer sums and against a
float64 sum within the bound its order implies, construction, metadata, framing and repr, the
argument checks, and the kernels' tiling (csrc/dmt_geo.hpp) walked on the host by a stand-alone
program under sanitizers."""
import json
import os
import warnings

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, search
from baseband_tasks_amd.dm import DispersionMeasure

import dmt_cases
from dmt_cases import CASES, IDS, RATE, T0
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


# -- the shift rule ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_shifts_are_those_of_dedisperse_samples(case):
    """Row d of `dm_trial_shifts` is the `_shift` of `DedisperseSamples` for trial d, to the bit."""
    sh = dmt_cases.stream(case)
    shifts = dmt_cases.shifts(case)
    assert shifts.shape == (len(case.dms), case.nchan) and shifts.dtype.kind == 'i'
    picked = sorted(set(np.linspace(0, len(case.dms) - 1, 7).astype(int)))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                      # (one sample per frame: "inefficient")
        for d in picked:
            one = bt.DedisperseSamples(sh, case.dms[d], reference_frequency=case.reference, samples_per_frame=1)
            want = np.broadcast_to(one._shift, (case.nchan,) + case.rest).reshape(case.nchan, -1)
            assert (want == want[:, :1]).all()
            np.testing.assert_array_equal(shifts[d], want[:, 0])
            assert one.reference_frequency == bt.DMTrials(sh, case.dms, reference_frequency=case.reference).reference_frequency


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_cases_have_the_geometry_they_are_named_for(case):
    """hi, lo and span as worked out with the plain formula: a drift in the shift rule -- the delay
    constant, the half-channel offset, the rounding, the sign -- is caught here by name."""
    shifts = dmt_cases.shifts(case)
    hi, lo = int(shifts.max()), int(shifts.min())
    if case.hi is not None:
        assert hi == case.hi
    if case.lo is not None:
        assert lo == case.lo
    if case.name in dmt_cases.SPANS:
        assert hi - lo == dmt_cases.SPANS[case.name]
    assert case.n > hi - lo
    # no delay on the doorstep of a rounding tie, where the last bit of a division would decide
    sh = dmt_cases.stream(case)
    f = sh.frequency + sh.sideband * RATE / 2.
    ref = np.mean(f) if case.reference is None else case.reference
    delay = np.stack([-DispersionMeasure(dm).time_delay(f, ref) * RATE for dm in case.dms])
    delay = delay.reshape(len(case.dms), case.nchan)
    np.testing.assert_array_equal(np.round(delay).astype(int), shifts)
    frac = np.abs(delay - np.floor(delay) - 0.5)
    assert frac[delay != 0.].min() > 1e-6 if (delay != 0.).any() else True


def test_plain_formula_by_hand():
    """3 channels, the numbers written out: 4148.808 s MHz^2 * DM * (f^-2 - fref^-2) at the
    mid-channel frequency f + rate / 2, negated, times the rate, rounded."""
    case = dmt_cases.by_name('narrow')
    f = (np.array([600e6, 605e6, 610e6]) + 5e3) / 1e6
    ref = f.mean()
    want = np.array([np.round(-(1. / 2.41e-4) * dm * (1. / f ** 2 - 1. / ref ** 2) * 1e4) for dm in case.dms]).astype(int)
    np.testing.assert_array_equal(dmt_cases.shifts(case), want)
    assert want.max() == 3 and want.min() == -3


def test_frequency_override_and_quantity_dms():
    case = dmt_cases.by_name('neg_unsorted')
    plain = bt.HostStream(dmt_cases.data(case), bt.Time(T0), RATE, pin=False)
    with pytest.raises((AttributeError, TypeError)):
        search.dm_trial_shifts(plain, case.dms)
    dt = bt.DMTrials(plain, [DispersionMeasure(dm) for dm in case.dms], frequency=dmt_cases.frequency(case),
                     sideband=case.sideband)
    np.testing.assert_array_equal(dt.shifts, dmt_cases.shifts(case))
    assert dt.dm.dtype == np.float64 and dt.dm.tolist() == list(case.dms)


# -- the twin ------------------------------------------------------------------------------------------
def _exact(case):
    """The sums in int64, by fancy indexing: out[i, d, r] = sum_c x[i + offsets[d, c], c, r]."""
    x = dmt_cases.data(case).astype(np.int64)
    shifts = dmt_cases.shifts(case)
    offsets = shifts.max() - shifts
    n_out = case.n - (shifts.max() - shifts.min())
    i = np.arange(n_out)[:, None, None]
    rows = i + offsets[None]                                   # (n_out, ndm, nchan)
    picked = x[rows, np.arange(case.nchan)[None, None]]        # (n_out, ndm, nchan) + rest
    return picked.sum(axis=2)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_sums_integers_exactly(case):
    got = dmt_cases.expected(case)
    want = _exact(case)
    assert got.dtype == np.float32 and got.shape == want.shape == (case.n - np.ptp(dmt_cases.shifts(case)), len(case.dms)) + case.rest
    assert np.abs(want).max() < 2 ** 24
    np.testing.assert_array_equal(got.astype(np.int64), want)
    assert not np.signbit(got[got == 0]).any()                 # (a sum that starts at +0 never is -0)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_on_noise_within_the_bound_of_its_order(case):
    """nchan - 1 rounded adds (the first, to +0, is exact), each off by at most half an ulp of a
    partial sum that is at most sum |x|: |error| <= (nchan - 1) * 2^-24 * sum_c |x|.  A bound, not
    a measurement."""
    x = dmt_cases.data(case, 'noise').astype(np.float64)
    shifts = dmt_cases.shifts(case)
    offsets = shifts.max() - shifts
    got = dmt_cases.expected(case, 'noise')
    n_out = got.shape[0]
    rows = np.arange(n_out)[:, None, None] + offsets[None]
    picked = x[rows, np.arange(case.nchan)[None, None]]
    want, mag = picked.sum(axis=2), np.abs(picked).sum(axis=2)
    assert (np.abs(got - want) <= (case.nchan - 1) * 2. ** -24 * mag).all()
    if case.nchan > 8:
        assert (got != want.astype(np.float32)).any()         # (so the order does matter for these data)


def test_twin_by_brute_force_and_special_values():
    x = np.arange(7 * 3, dtype=np.float32).reshape(7, 3) - 9.
    shifts = np.array([[1, 0, -1], [0, 0, 0], [-2, 1, 0]])
    got = search.dm_trials_samples(x, shifts)
    hi, span = 1, 3
    assert got.shape == (4, 3)
    for i in range(4):
        for d in range(3):
            acc = np.float32(0.)
            for c in range(3):
                acc = np.float32(acc + x[i + hi - shifts[d, c], c])
            assert got[i, d] == acc
    y = x.copy()
    y[3, 1] = np.nan
    nan = np.isnan(search.dm_trials_samples(y, shifts))
    crossing = np.array([[i + hi - shifts[d, 1] == 3 for d in range(3)] for i in range(4)])
    np.testing.assert_array_equal(nan, crossing)
    with pytest.raises(TypeError):
        search.dm_trials_samples(x.astype(np.float64), shifts)
    with pytest.raises(ValueError):
        search.dm_trials_samples(x, shifts[:, :2])
    with pytest.raises(ValueError):
        search.dm_trials_samples(x[:3], shifts)


# -- construction ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stream_surface(case):
    sh = dmt_cases.stream(case, samples_per_frame=50)
    dt = bt.DMTrials(sh, case.dms, reference_frequency=case.reference)
    shifts = dmt_cases.shifts(case)
    hi, span = int(shifts.max()), int(np.ptp(shifts))
    assert dt.shape == (case.n - span, len(case.dms)) + case.rest and dt.dtype == np.float32
    assert dt.sample_rate == RATE and dt.samples_per_frame == 50
    assert abs((dt.start_time - (bt.Time(T0) + hi / RATE))) < 1e-9
    assert abs((dt.stop_time - (bt.Time(T0) + (case.n + int(shifts.min())) / RATE))) < 1e-9
    np.testing.assert_array_equal(dt.shifts, shifts)
    assert dt.dm.dtype == np.float64 and dt.dm.shape == (len(case.dms),)
    f = sh.frequency + sh.sideband * RATE / 2.
    assert dt.reference_frequency == (np.mean(f) if case.reference is None else case.reference)
    assert np.shape(dt.frequency) == () and dt.frequency == dt.reference_frequency
    with pytest.raises(AttributeError):
        dt.sideband
    text = repr(dt)
    assert text.startswith('DMTrials(ih') and 'dms=' in text and 'ih: HostStream' in text
    assert bt.DMTrials(sh, case.dms, samples_per_frame=7).samples_per_frame == 7
    dt.close()
    assert dt.closed


def test_default_frame_fits_the_output_and_the_plane_can_be_stacked_on():
    case = dmt_cases.by_name('trailing')
    dt = bt.DMTrials(dmt_cases.stream(case), case.dms)         # (the input's frame, 1000 samples, exceeds the 554 left)
    assert dt.samples_per_frame == dt.shape[0] == 554
    part = dt[5:50]
    assert part.shape == (45, 2, 4) and part.frequency == dt.reference_frequency
    # a frequency without a sideband is not something the base classes hand on: relabel, then stack
    with pytest.raises(ValueError, match='sideband'):
        bt.Integrate(dt, 4)
    ig = bt.Integrate(bt.SetAttribute(dt, frequency=dt.frequency, sideband=1), 4)
    assert ig.shape == (138, 2, 4) and ig.frequency == dt.reference_frequency


def test_polarization_is_kept_where_the_channels_share_it():
    case = dmt_cases.by_name('trailing')
    x = dmt_cases.data(case)
    pol = np.array(['XX', 'YY', 'XY', 'YX'])
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=dmt_cases.frequency(case), sideband=1,
                       polarization=pol)
    dt = bt.DMTrials(sh, case.dms)
    np.testing.assert_array_equal(dt.polarization, pol)
    two = dmt_cases.by_name('zero_dm')
    sh = bt.HostStream(dmt_cases.data(two), bt.Time(T0), RATE, pin=False, frequency=dmt_cases.frequency(two),
                       sideband=1, polarization=np.array(['X', 'Y', 'X', 'Y', 'X']))
    with pytest.raises(AttributeError):
        bt.DMTrials(sh, two.dms).polarization


def test_what_is_refused():
    case = dmt_cases.by_name('ref_below')
    sh = dmt_cases.stream(case)
    z = bt.HostStream(np.zeros((50, 4), np.complex64), bt.Time(T0), RATE, pin=False,
                      frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    with pytest.raises(TypeError, match='Square'):
        bt.DMTrials(z, [1.])
    f64 = bt.HostStream(np.zeros((50, 4)), bt.Time(T0), RATE, pin=False, frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    with pytest.raises(TypeError, match='float32'):
        bt.DMTrials(f64, [1.])
    # a frequency that varies off the channel axis
    x = np.zeros((50, 4, 2), np.float32)
    off_axis = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=np.linspace(4e8, 8e8, 8).reshape(4, 2), sideband=1)
    with pytest.raises(ValueError, match='channel axis'):
        bt.DMTrials(off_axis, [1.])
    with pytest.raises(ValueError, match='channel axis'):
        search.dm_trial_shifts(off_axis, [1.])
    # N <= span: ref_below spans 2337 samples
    short = bt.HostStream(dmt_cases.data(case)[:2337], bt.Time(T0), RATE, pin=False, frequency=dmt_cases.frequency(case),
                          sideband=1)
    with pytest.raises(ValueError, match='span'):
        bt.DMTrials(short, case.dms, reference_frequency=case.reference)
    bt.DMTrials(bt.HostStream(dmt_cases.data(case)[:2338], bt.Time(T0), RATE, pin=False,
                              frequency=dmt_cases.frequency(case), sideband=1), case.dms, reference_frequency=case.reference)
    # the trials
    for bad in ([], 1.5, [[1., 2.]], np.zeros(hip.DMT_MAX_NDM + 1)):
        with pytest.raises(ValueError):
            bt.DMTrials(sh, bad)
    # the limits
    wide = bt.HostStream(np.zeros((3, 2, hip.DMT_MAX_REST + 1), np.float32), bt.Time(T0), RATE, pin=False,
                         frequency=np.array([[4e8], [8e8]]), sideband=1)
    with pytest.raises(ValueError, match='elements'):
        bt.DMTrials(wide, [0.])
    with pytest.raises(ValueError, match='span'):
        bt.DMTrials(sh, [1e6])                                 # (a span beyond 2^24 samples)
    assert (hip.DMT_MAX_NCHAN, hip.DMT_MAX_NDM, hip.DMT_MAX_REST, hip.DMT_MAX_SPAN) == (16384, 4096, 64, 1 << 24)


def test_library_exports_the_plan():
    lib = hip.lib()
    assert lib.bbt_version() >= 163
    for name in ('bbt_dmt_plan_create', 'bbt_dmt_plan_destroy', 'bbt_dmt_plan_info', 'bbt_dmt_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name)
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    geo = open(os.path.join(CSRC, 'dmt_geo.hpp')).read()
    for name, value in (('NCHAN', hip.DMT_MAX_NCHAN), ('NDM', hip.DMT_MAX_NDM), ('REST', hip.DMT_MAX_REST)):
        assert f'#define BBT_DMT_MAX_{name} {value}' in geo
    assert '#define BBT_DMT_MAX_SPAN (1 << 24)' in geo and 'bbt_dmt_execute' in header


# -- the tiling, on the host ------------------------------------------------------------------------------
def _geo_shapes():
    """(n_in, n_out, nchan, n_rest, ndm, span, tile_t, db): every shared case under every tiling
    the tests walk, the limits, and chunks of more than 2^31 elements."""
    shapes = []
    for case in CASES:
        span = int(np.ptp(dmt_cases.shifts(case)))
        rest = int(np.prod(case.rest, dtype=int))
        for tile_t, db in ((0, 0), (64, 1), (128, 4), (256, 16), (64, 16), (256, 2)):
            shapes.append((case.n, case.n - span, case.nchan, rest, len(case.dms), span, tile_t, db))
    shapes += [(1, 1, 1, 1, 1, 0, 0, 0), (65, 64, 1, 1, 1, 1, 64, 1), (64 + 5, 64, 3, 64, 17, 5, 128, 8),
               # the limits: every axis at its bound (few samples)
               (70, 3, 16384, 64, 5, 60, 0, 0), (300, 200, 7, 2, 4096, 100, 256, 8), ((1 << 24) + 40, 40, 2, 1, 3, 1 << 24, 0, 0),
               # more than 2^31 elements in the chunk, in the scratch and in the result
               ((1 << 18) + 1000, 1 << 18, 16384, 1, 2, 1000, 256, 16), ((1 << 22) + 3000, 1 << 22, 1024, 1, 16, 3000, 0, 0),
               ((1 << 20) + 9, 1 << 20, 2, 1, 4096, 9, 256, 16)]
    return shapes


def test_kernel_tiling_on_the_host(tmp_path):
    """Every (time, trial, r) of the result owned by exactly one wave, every read inside [0, n_in)
    of its row, the table validation refusing what it must: the program exits non-zero otherwise,
    and the sanitizers abort it on a wild index or an overflow of its own."""
    exe = compile_check('dmt_geo_check', tmp_path)
    shapes = _geo_shapes()
    plans = run_check(exe, shapes)
    for (n_in, n_out, nchan, rest, ndm, span, tile_t, db), g in zip(shapes, plans):
        assert g['walk'] == 0, (n_in, n_out, nchan, rest, ndm, span, tile_t, db, g)
        assert g['tile_t'] == (tile_t or 256) and g['db'] == (db or 8)
        assert g['waves_t'] * g['waves_d'] == 4 and g['tile_d'] == g['db'] * g['waves_d']
        assert g['pitch'] % 64 == 0 and n_in <= g['pitch'] < n_in + 64 and g['scratch'] == nchan * rest * g['pitch']
        assert g['n_wg'] == -(-n_out // g['tile_t']) * -(-ndm // g['tile_d']) * rest
    big = [g for s, g in zip(shapes, plans) if s[0] * s[2] * s[3] > 2 ** 31]
    assert len(big) >= 2 and all(g['scratch'] > 2 ** 31 for g in big)
    # what the library refuses: one sample short, a bad tile, a bad trial block, beyond the limits
    bad = run_raw(exe, '106 100 3 1 2 7 0 0  107 100 3 1 2 7 96 0  107 100 3 1 2 7 0 3  107 100 16385 1 2 7 0 0 '
                       '107 100 3 65 2 7 0 0  107 100 3 1 4097 7 0 0  16777317 100 3 1 2 16777217 0 0')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 7
    assert 'shorter' in errors[0] and 'time tile' in errors[1] and 'trial block' in errors[2]
    assert '16384' in errors[3] and '64' in errors[4] and '4096' in errors[5] and '2^24' in errors[6]
