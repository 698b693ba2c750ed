"""`LongSpectra` on the GPU against `periodicity.long_spectra_samples`, the float64 yardstick, within
the tolerance lspec_cases.py derives (per column: rel-L2 <= 2e-6, max |diff| / max <= 2e-5); and, on
bit patterns, that no value depends on how column pairs are grouped into launches, on the framing or
on where a read starts, and that a NaN stays within its column pair.  Noise at all eight lengths,
planted tones at the fence posts of the partner map, the chain on the device, a planted pulse train."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity
from baseband_tasks_amd.device_task import produces_on_device
from baseband_tasks_amd.periodicity import SNR

import lspec_cases
from lspec_cases import NOISE, NOISE_IDS, assert_close, same_bits

pytestmark = pytest.mark.gpu

T0 = bt.Time(lspec_cases.T0)


def _plan_run(x, n, stack, n_spec, budget=0):
    plan = hip.LongSpectraPlan(n, stack, x.shape[1])
    out = hip.DeviceArray((n_spec, n // 2 + 1, x.shape[1]), np.float32)
    plan.execute(hip.DeviceArray.from_host(x), n_spec, out, budget)
    got = out.to_host()
    plan.close()
    return got


# -- noise, every length ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', NOISE, ids=NOISE_IDS)
def test_noise_task_and_plan_meet_the_yardstick(case):
    x, want = lspec_cases.data(case), lspec_cases.expected(case)
    n = 1 << case.log2n
    assert want.shape == (case.nspec, n // 2 + 1, case.n_elem)
    host = bt.LongSpectra(lspec_cases.stream(x), n, case.stack)
    assert host.shape == want.shape
    got = host.read()
    assert_close(got, want, f'{case.name} host stream')
    dev = bt.LongSpectra(lspec_cases.stream(x, bt.DeviceStream), n, case.stack)
    assert produces_on_device(dev)
    got_dev = dev.read_device().to_host()
    assert_close(got_dev, want, f'{case.name} device stream')
    got_plan = _plan_run(x, n, case.stack, case.nspec)
    assert_close(got_plan, want, f'{case.name} plan')
    # one route, three ways in
    assert same_bits(got, got_dev) and same_bits(got, got_plan)
    host.close(), dev.close()


# -- planted tones ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('log2n', [15, 18])
def test_planted_tones_at_the_fence_posts_of_the_partner_map(log2n):
    n = 1 << log2n
    plan = hip.LongSpectraPlan(n, 1, 9)
    n1 = plan.info()['n1']
    plan.close()
    assert n1 == 1 << (log2n // 2)
    bins = lspec_cases.tone_bins(n, n1)
    got = bt.LongSpectra(lspec_cases.stream(lspec_cases.tones(n, n1), bt.DeviceStream), n).read()[0].astype(np.float64)
    assert got.shape == (n // 2 + 1, 9)
    for c, j in enumerate(bins):
        j, peak = (0, float(n) ** 2) if j is None else (j, float(n) ** 2 * (1. if j == n // 2 else .25))
        assert abs(got[j, c] - peak) <= lspec_cases.MAX_TOL * peak, (c, j, got[j, c], peak)
        rest = np.delete(got[:, c], j)
        print(f"2^{log2n} column {c} bin {j}: peak off by {abs(got[j, c] - peak) / peak:.3g}, "
              f"largest other bin {rest.max() / float(n) ** 2:.3g} n^2")
        assert rest.max() < 1e-9 * float(n) ** 2, (c, j, rest.max(), int(rest.argmax()))


# -- grouping ---------------------------------------------------------------------------------------------
def test_no_value_depends_on_the_grouping_the_framing_or_the_seek():
    """2^16 x 7 (four pairs, the last with a zero partner), two output spectra: one pair a launch, exactly
    two pairs a launch, the default; frames of one and of two spectra; a seek to the second spectrum."""
    n = 1 << 16
    rng = np.random.default_rng(77)
    x = rng.standard_normal((2 * n + 5, 7), dtype=np.float32)
    ref = bt.LongSpectra(lspec_cases.stream(x, bt.DeviceStream), n)
    want = ref.read()
    assert want.shape == (2, n // 2 + 1, 7)
    assert_close(want, periodicity.long_spectra_samples(x, n), 'grouping reference')
    plan = hip.LongSpectraPlan(n, 1, 7)
    assert plan.info()['pairs_per_launch'] == 4 and plan.info(1)['pairs_per_launch'] == 1
    assert plan.info(16 * n)['pairs_per_launch'] == 2 and plan.info(16 * n)['scratch_bytes'] == 16 * n
    plan.close()
    for budget in (1, 16 * n, 1 << 29):
        for spf in (1, 2):
            task = bt.LongSpectra(lspec_cases.stream(x, bt.DeviceStream), n, samples_per_frame=spf)
            task.spectra_budget = budget
            assert same_bits(task.read(), want), (budget, spf)
            task.seek(1)
            assert same_bits(task.read(1), want[1:]), (budget, spf)
            task.close()
        assert same_bits(_plan_run(x, n, 1, 2, budget), want), budget
    ref.close()


@pytest.mark.parametrize('threads', [256, 512, 1024])
def test_no_value_depends_on_the_workgroup_size(threads, monkeypatch):
    """BBT_LSPEC_THREADS changes which thread moves which cell, not what is computed."""
    case = lspec_cases.by_name('2^17x2')
    n = 1 << case.log2n
    want = _plan_run(lspec_cases.data(case), n, 1, 1)
    monkeypatch.setenv('BBT_LSPEC_THREADS', str(threads))
    plan = hip.LongSpectraPlan(n, 1, 2)
    assert plan.info()['threads'] == threads
    plan.close()
    assert same_bits(_plan_run(lspec_cases.data(case), n, 1, 1), want)
    assert_close(want, lspec_cases.expected(case), f'{threads} threads')


# -- isolation --------------------------------------------------------------------------------------------
def test_a_nan_stays_within_its_column_pair():
    case = lspec_cases.by_name('2^15x6')
    n = 1 << 15
    clean = bt.LongSpectra(lspec_cases.stream(lspec_cases.data(case), bt.DeviceStream), n).read()
    x = lspec_cases.data(case).copy()
    x[100, 0], x[20000, 0] = np.nan, np.inf
    got = bt.LongSpectra(lspec_cases.stream(x, bt.DeviceStream), n).read()
    assert same_bits(got[:, :, 2:], clean[:, :, 2:])
    assert np.isfinite(clean).all()
    # the column itself and its partner: non-finite throughout, as documented
    assert not np.isfinite(got[:, :, :2]).any()


# -- the chain on the device ------------------------------------------------------------------------------
def test_periodicity_chain_on_the_device():
    n = 1 << 15
    nh = bt.DeviceNoiseGenerator((32 * (n + 4096),), T0, 10e6, 32 * 4096, dtype=np.complex64, seed=5,
                                 frequency=600e6, sideband=1)
    dt = bt.DMTrials(bt.Integrate(bt.Square(bt.Channelize(nh, 16)), 2), [0., 1., 4., 2.5])
    plane = bt.Standardize(dt, 4096)
    assert plane.shape[0] >= n and plane.shape[1:] == (4,)
    sp = bt.fluctuation_spectra(plane, n)
    assert isinstance(sp, bt.LongSpectra)
    wh = bt.Whiten(sp, 128)
    hs = bt.HarmonicSearch(wh, 64, n_levels=4)
    stage = hs
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    assert produces_on_device(stage)
    assert sp.shape == (1, n // 2 + 1, 4) and wh.shape == sp.shape and hs.shape == (1, 257, 3, 4)
    assert sp.bin_width == plane.sample_rate / n and hs.sample_rate == sp.sample_rate
    assert abs(hs.start_time - plane.start_time) < 1e-9
    got = hs.read_device().to_host()
    sp.seek(0)
    spectra = sp.read()
    assert spectra.dtype == np.float32 and np.isfinite(spectra).all() and (spectra[:, 1:] > 0).all()
    # the spectra are those of the plane, within the tolerance
    plane.seek(0)
    assert_close(spectra, periodicity.long_spectra_samples(plane.read(n), n), 'chain spectra')
    # the two downstream tasks are bit-exact given their input
    z = periodicity.whiten_samples(spectra, 128)
    assert same_bits(got, periodicity.harmonic_search_samples(z, 64, 4, 1., 1))
    assert np.isfinite(got).all() and got[:, :, SNR].max() > 1.


# -- a pulsar -----------------------------------------------------------------------------------------------
def test_a_planted_pulse_train_is_the_one_candidate():
    """A faint pulse every 128 samples (Gaussian, sigma 6 samples, peak 0.1 on unit noise) in trial 2 of
    four, a plane of 2^17 samples searched as four stacked spectra of 2^15: the fundamental is bin 2^15 /
    128 = 256 exactly.  Above threshold 9 there is the train at bin 256 of trial 2 and nothing else.  (It
    is reported once per number of harmonics whose sum passes -- `harmonic_candidates` merges nothing
    across harmonics -- always at the same fundamental bin.  Run through the NumPy route on the host
    the four reports have S/N 10.0 ... 11.9 and the best cell elsewhere 7.5: both a unit away from the
    threshold, where a spectrum off by 1e-6 moves nothing.)"""
    n = 1 << 15
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1 << 17, 4), dtype=np.float32)
    phase = (np.arange(1 << 17) + 64) % 128 - 64
    x[:, 2] += (.1 * np.exp(-.5 * (phase / 6.) ** 2)).astype(np.float32)
    sp = bt.fluctuation_spectra(lspec_cases.stream(x, bt.DeviceStream), n, 4)
    assert isinstance(sp, bt.LongSpectra) and sp.shape == (1, n // 2 + 1, 4)
    hs = bt.HarmonicSearch(bt.Whiten(sp, 512), 64, n_levels=4, averaged=4)
    best = hs.read()
    cands = periodicity.harmonic_candidates(best[0], 64, 9., sp.bin_width)
    print(cands)
    assert len(cands) >= 1
    assert (cands['bin'] == 256.).all() and (cands['trial'] == 2).all()
    assert len(set(cands['harmonics'].tolist())) == len(cands) and cands['snr'][0] > 10.
    assert cands['frequency'][0] == pytest.approx(256. * lspec_cases.RATE / n)
    best[0, :, SNR, 2] = 0.
    assert best[0, :, SNR].max() < 8.5


# -- what the plan refuses --------------------------------------------------------------------------------
def test_plan_refuses_before_any_launch():
    n = 1 << 15
    plan = hip.LongSpectraPlan(n, 2, 3)
    info = plan.info()
    assert (info['n1'], info['n2'], info['cols'], info['pairs']) == (128, 256, 32, 16)
    assert info['threads'] in (256, 512, 1024)
    assert info['pairs_per_launch'] == 2 and info['scratch_bytes'] == 16 * n
    x = hip.DeviceArray((2 * n, 3), np.float32)
    out = hip.DeviceArray((1, n // 2 + 1, 3), np.float32)
    with pytest.raises(ValueError):
        plan.execute(x, 0, out)                         # no whole transform
    with pytest.raises(ValueError):
        plan.execute(x, 2, out)                         # more spectra than samples
    with pytest.raises(ValueError):
        plan.execute(x[:2 * n - 1], 1, out)
    with pytest.raises(TypeError):
        plan.execute(hip.DeviceArray((2 * n, 3), np.complex64), 1, out)
    lib = hip.lib()
    stream = hip._stream
    assert lib.bbt_lspec_execute(plan._h, None, 2 * n, out.ptr, 1, 0, stream) != 0          # null
    assert lib.bbt_lspec_execute(plan._h, x.ptr + 2, 2 * n, out.ptr, 1, 0, stream) != 0     # misaligned
    assert lib.bbt_lspec_execute(plan._h, x.ptr, 2 * n - 1, out.ptr, 1, 0, stream) != 0     # no whole transform
    assert lib.bbt_lspec_execute(plan._h, x.ptr, 2 * n, out.ptr, 0, 0, stream) != 0
    plan.close()
