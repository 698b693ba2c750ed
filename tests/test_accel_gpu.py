"""`Accelerate` on the GPU against `periodicity.accelerate_samples`, word for word (``uint32`` views: NaN
payloads and -0 included): the table of accel_cases.py as a task on a host stream, on a device stream and
through the plan, under every BBT_ACCEL_ROUTE; that no value depends on the budget, the framing or a seek;
what the plan refuses; the chain on the device; and a planted binary pulsar."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity
from baseband_tasks_amd.device_task import produces_on_device

import accel_cases
import lspec_cases
from accel_cases import CASES, IDS, RATE, same_words, stream

pytestmark = pytest.mark.gpu

#: a = 2 c rate k: the accelerations whose factors at RATE are (within an ulp) the table's
TO_ACC = 2. * periodicity.C_LIGHT * RATE


def _task(case, x, cls=None, **kwargs):
    """The task with exactly the factors of the table (the accelerations are only labels here)."""
    task = bt.Accelerate(stream(x, cls), np.array(case.factors) * (.5 * TO_ACC), case.n, **kwargs)
    task.factors = np.array(case.factors, dtype=np.float64)
    task._k_min, task._k_max = min(case.factors), max(case.factors)
    return task


def _plan_run(case, x):
    n_elem = int(np.prod(case.shape, dtype=np.int64))
    plan = hip.AccelPlan(case.n, n_elem, case.factors)
    rows = case.length // case.n * case.n
    out = hip.DeviceArray((rows, len(case.factors)) + case.shape, np.float32)
    plan.execute(hip.DeviceArray.from_host(x), 0, case.length, out, 0, rows, n_rows=case.length)
    got = out.to_host()
    plan.close()
    return got


# -- the table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', [0, 1, 2])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_table_against_the_twin(case, route, monkeypatch):
    """BBT_ACCEL_ROUTE is read at every call, so it is set in this process."""
    monkeypatch.setenv('BBT_ACCEL_ROUTE', str(route))
    x, want = accel_cases.data(case), accel_cases.expected(case)
    n_elem = int(np.prod(case.shape, dtype=np.int64))
    plan = hip.AccelPlan(case.n, n_elem, case.factors)
    info = plan.info(0, case.n)
    # the automatic rule: the window if a sample has 16 bytes at least and the tile in the middle of the block fits
    i0 = case.n // 2 // info['rows'] * info['rows']
    middle_fits = plan.info(i0, min(case.n, i0 + info['rows']) - i0)['fits']
    plan.close()
    # (info counts in units of 4 bytes: a row of more than a tile of them is cut into segments, and those go direct)
    segmented = n_elem * len(case.factors) > hip.ACCEL_TILE_UNITS
    assert segmented == (case.name in accel_cases.SEGMENTED + (accel_cases.FENCE_POST,))
    if segmented:
        assert info['route'] == 2 and info['rows'] == 1
    if route == 2 or 2 * n_elem * 4 > hip.ACCEL_LDS_BYTES or segmented:
        assert info['route'] == 2
    else:
        assert info['route'] == (1 if route == 1 or (n_elem >= 4 and middle_fits) else 2)
    assert info['lds_bytes'] == hip.ACCEL_LDS_BYTES and info['window_first'] == 0 and info['window_rows'] == case.n
    if case.name == 'n32768_far':
        assert not info['fits']
    host = _task(case, x)
    assert host.shape == want.shape
    got = host.read()
    assert same_words(got, want), f'{case.name} host stream, route {route}'
    dev = _task(case, x, bt.DeviceStream)
    assert produces_on_device(dev)
    assert same_words(dev.read_device().to_host(), want), f'{case.name} device stream, route {route}'
    assert same_words(_plan_run(case, x), want), f'{case.name} plan, route {route}'
    host.close(), dev.close()


def test_the_identity_trial_is_the_input():
    for name in ('n64', 'n500', 'n256_wide'):
        case = accel_cases.by_name(name)
        x = accel_cases.data(case)
        j = case.factors.index(0.)
        got = _task(case, x, bt.DeviceStream).read()
        assert same_words(got[:, j], x[:got.shape[0]])
    # through the public surface, accelerations and all
    x = accel_cases.data(accel_cases.by_name('n512'))
    task = bt.Accelerate(stream(x, bt.DeviceStream), [0., 1e7, 0.], 512)
    got = task.read()
    assert same_words(got[:, 0], x) and same_words(got[:, 2], x)
    assert same_words(got, periodicity.accelerate_samples(x, task.factors, 512)) and task.max_shift > 0


# -- independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['n64', 'n500'])
def test_no_value_depends_on_the_budget_the_framing_or_a_seek(name):
    case = accel_cases.by_name(name)
    x, want = accel_cases.data(case), accel_cases.expected(case)
    n, rows = case.n, want.shape[0]
    row_bytes = 4 * len(case.factors) * int(np.prod(case.shape))
    whole = _task(case, x, bt.DeviceStream)
    assert same_words(whole.read(), want)
    # chunks of 1 row, of 37 rows, and of 3 n / 4 rows: the second one straddles the block boundary
    for per in (1, 37, 3 * n // 4):
        task = _task(case, x, bt.DeviceStream, samples_per_frame=rows)
        task.accel_budget = per * row_bytes
        assert task._chunk_size() == per
        assert same_words(task.read(), want), per
        task.close()
    for spf in (1, 7, n):
        for cls in (None, bt.DeviceStream):
            task = _task(case, x, cls, samples_per_frame=spf)
            assert same_words(task.read(), want), spf
            # a seek into the middle of a block, a short read
            start = n + n // 2 + 3
            task.seek(start)
            assert same_words(task.read(9), want[start:start + 9]), spf
            task.seek(n - 2)
            assert same_words(task.read_device(5).to_host(), want[n - 2:n + 3]), spf
            task.close()
    whole.close()


# -- what the plan refuses ----------------------------------------------------------------------------------
def test_plan_refuses_before_any_launch():
    n = 64
    factors = [1. / 256., 0., -1. / 256.]
    plan = hip.AccelPlan(n, 3, factors)
    table = periodicity.accelerate_rows(n, factors)
    rows = slice(20, 50)
    lo, hi = int(table[:, rows].min()), int(table[:, rows].max())
    info = plan.info(n + 20, 30)
    assert (info['window_first'], info['window_rows']) == (n + lo, hi + 1 - lo) and info['fits']
    assert info['rows'] == min(hip.ACCEL_MAX_ROWS, hip.ACCEL_TILE_UNITS // 9) and info['route'] in (1, 2)
    x = hip.DeviceArray.from_host(np.arange(3 * n * 3, dtype=np.float32).reshape(3 * n, 3))
    sentinel = np.full((30, 3, 3), -7., np.float32)
    out = hip.DeviceArray.from_host(sentinel)
    # the exact window is enough ...
    plan.execute(x[n + lo:n + hi + 1], n + lo, hi + 1 - lo, out, n + 20, 30)
    want = periodicity.accelerate_samples(x.to_host(), factors, n)[n + 20:n + 50]
    assert same_words(out.to_host(), want)
    # ... and a piece that misses its first or its last row is refused, with nothing launched
    out.copy_from_host(sentinel)
    with pytest.raises(hip.HipError, match='window'):
        plan.execute(x[n + lo + 1:n + hi + 1], n + lo + 1, hi - lo, out, n + 20, 30)
    with pytest.raises(hip.HipError, match='window'):
        plan.execute(x[n + lo:n + hi], n + lo, hi - lo, out, n + 20, 30)
    hip.synchronize()
    assert same_words(out.to_host(), sentinel)
    with pytest.raises(ValueError, match='last whole block'):
        plan.execute(x, 0, 3 * n, hip.DeviceArray((n + 1, 3, 3), np.float32), 2 * n, n + 1, n_rows=3 * n + 10)
    with pytest.raises(ValueError):
        plan.execute(x, 0, 3 * n, out, 0, 31)                            # more rows than the output holds
    with pytest.raises(ValueError):
        plan.execute(x, 0, 3 * n + 1, out, 0, 30)                        # more rows than the input holds
    with pytest.raises(ValueError):
        plan.execute(x, 0, 3 * n, out, 0, 0)
    with pytest.raises(TypeError):
        plan.execute(hip.DeviceArray((3 * n, 3), np.complex64), 0, 3 * n, out, 0, 30)
    lib, st = hip.lib(), hip._stream
    assert lib.bbt_accel_execute(plan._h, None, 0, 3 * n, out.ptr, 0, 30, st) != 0               # null
    assert lib.bbt_accel_execute(plan._h, x.ptr + 2, 0, 3 * n - 1, out.ptr, 0, 30, st) != 0      # misaligned
    assert lib.bbt_accel_execute(plan._h, x.ptr, 0, 3 * n, out.ptr, -1, 30, st) != 0
    assert lib.bbt_accel_execute(plan._h, x.ptr, 0, 3 * n, out.ptr, 0, 0, st) != 0
    assert lib.bbt_accel_execute(plan._h, x.ptr, 0, 3 * n, out.ptr, 0, 1 << 41, st) != 0
    hip.synchronize()
    assert same_words(out.to_host(), sentinel)
    plan.close()


# -- the chain on the device --------------------------------------------------------------------------------
def test_periodicity_chain_on_the_device():
    n = 1 << 15
    rng = np.random.default_rng(31)
    x = rng.standard_normal((n + 4096 + 5, 2), dtype=np.float32) * np.float32(3.) + np.float32(10.)
    src = stream(x, bt.DeviceStream)
    k = np.linspace(-2., 2., 5) / (64 * n)
    plane = bt.Standardize(src, 4096)
    acc = bt.Accelerate(plane, k * TO_ACC, n)
    sp = bt.LongSpectra(acc, n)
    hs = bt.HarmonicSearch(bt.Whiten(sp, 128), 64, n_levels=4)
    stage = hs
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    assert acc.shape == (n, 5, 2) and sp.shape == (1, n // 2 + 1, 5, 2) and hs.shape == (1, 257, 3, 5, 2)
    got = hs.read_device().to_host()
    # the Accelerate stage is its twin, to the bit
    z = bt.standardize_samples(x, 4096)
    plane.seek(0)
    assert same_words(plane.read(), z)
    acc.seek(0)
    resampled = acc.read()
    assert same_words(resampled, periodicity.accelerate_samples(z, acc.factors, n))
    # the spectra are those of the twin's output, within LongSpectra's tolerance
    sp.seek(0)
    spectra = sp.read()
    lspec_cases.assert_close(spectra.reshape(1, n // 2 + 1, 10),
                             periodicity.long_spectra_samples(resampled, n).reshape(1, n // 2 + 1, 10), 'chain spectra')
    # the search stages are bit-exact given their input
    white = periodicity.whiten_samples(spectra, 128)
    assert lspec_cases.same_bits(got, periodicity.harmonic_search_samples(white, 64, 4, 1., 1))
    assert np.isfinite(got).all()


# -- a binary pulsar ----------------------------------------------------------------------------------------
def test_the_planted_binary_pulsar_is_found_at_its_acceleration():
    """A Gaussian pulse train of period 64 samples on unit noise in column 1 of a (2^15, 2) plane, its phase
    warped by the exact inverse of the rule for k0 = 1 / (64 n): 128 samples of shift in the middle of the
    block, the fundamental at bin 512 drifting over 16 bins.  Searched with k = k0 {-2, -1, 0, 1, 2}: the top
    candidate is at the planted trial, column and bin, and beats the best the trial of zero acceleration
    has in that column.  The same assertions are made of the NumPy twins first, here and in
    test_accel_host.py: the planted amplitude was fixed on the twins alone."""
    x = accel_cases.pulsar_plane()
    n = accel_cases.PULSAR_N
    y = periodicity.accelerate_samples(x, accel_cases.PULSAR_TRIALS, n)
    twin = periodicity.harmonic_search_samples(
        periodicity.whiten_samples(periodicity.long_spectra_samples(y, n), 128), 64, 4, 1., 1)
    accel_cases.pulsar_verdict(twin[0], RATE / n)

    acc = bt.Accelerate(stream(x, bt.DeviceStream), accel_cases.PULSAR_ACCELERATIONS, n)
    assert np.allclose(acc.factors, accel_cases.PULSAR_TRIALS, rtol=1e-14, atol=0.) and acc.max_shift == 256
    sp = bt.LongSpectra(acc, n)
    hs = bt.HarmonicSearch(bt.Whiten(sp, 128), 64, n_levels=4)
    best = hs.read()
    assert best.shape == (1, 257, 3, 5, 2)
    accel_cases.pulsar_verdict(best[0], sp.bin_width)
