"""`DMTrials` on the GPU against its NumPy twin (`search.dm_trials_samples`), bit for bit: one
float32 accumulator per output element and the channels added in ascending order, so a value has
one correct result whatever the tiling or the chunking.  The shared cases of dmt_cases.py
(test_dmtrials_host.py proves their geometry and that the twin sums exactly), every tiling the
environment can ask for, chunks, pieces and seeks, the identity with `DedisperseSamples`, NaN / Inf
/ -0, a dispersed impulse, a device chain, and the plan's refusals."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, search
from baseband_tasks_amd.device_task import produces_on_device

import dmt_cases
from dmt_cases import CASES, IDS, RATE, same_bits

pytestmark = pytest.mark.gpu

T0 = bt.Time(dmt_cases.T0)


def _task(case, kind='int', cls=None, x=None, **kwargs):
    return bt.DMTrials(dmt_cases.stream(case, kind, cls, x), case.dms, reference_frequency=case.reference, **kwargs)


def _plan_run(x, shifts, rest=()):
    offsets = shifts.max() - shifts
    n_rest = int(np.prod(rest, dtype=int))
    plan = hip.DmtPlan(offsets, n_rest)
    n_out = x.shape[0] - plan.span
    out = hip.DeviceArray((n_out, shifts.shape[0]) + tuple(rest), np.float32)
    plan.execute(hip.DeviceArray.from_host(x), x.shape[0], out, n_out)
    got = out.to_host()
    plan.close()
    return got


# -- the shared cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['int', 'noise'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_task_and_plan_equal_the_twin(case, kind):
    want = dmt_cases.expected(case, kind)
    got = _task(case, kind).read()
    assert got.dtype == np.float32 and same_bits(got, want)
    dev = _task(case, kind, bt.DeviceStream)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), want)
    shifts = dmt_cases.shifts(case)
    assert int(np.ptp(shifts)) == hip.DmtPlan(shifts.max() - shifts, 1).span
    assert same_bits(_plan_run(dmt_cases.data(case, kind), shifts, case.rest), want)


@pytest.mark.parametrize('tile, trials', [(64, 1), (128, 4), (256, 16), (64, 16), (256, 2)])
@pytest.mark.parametrize('name', ['tile_edges', 'wide_span', 'many_dm', 'many_chan'])
def test_no_value_depends_on_the_tiling(name, tile, trials, monkeypatch):
    """BBT_DMT_TILE and BBT_DMT_TRIALS reshape the workgroups, from the smallest tile to the
    largest; the order of the sums is the contract, so every bit stays."""
    case = dmt_cases.by_name(name)
    monkeypatch.setenv('BBT_DMT_TILE', str(tile))
    monkeypatch.setenv('BBT_DMT_TRIALS', str(trials))
    shifts = dmt_cases.shifts(case)
    plan = hip.DmtPlan(shifts.max() - shifts, 1)
    info = plan.info()
    assert (info['tile'], info['trials']) == (tile, trials)
    plan.close()
    for kind in ('int', 'noise'):
        assert same_bits(_task(case, kind, bt.DeviceStream).read(), dmt_cases.expected(case, kind))


# -- chunks, pieces, frames, seeks ----------------------------------------------------------------------
def test_chunks_pieces_frames_and_seeks(monkeypatch):
    case = dmt_cases.by_name('tile_edges')
    want = dmt_cases.expected(case, 'noise')
    n_out, span = want.shape[0], dmt_cases.SPANS['tile_edges']
    row_in, row_out = case.nchan * 4, len(case.dms) * 4
    calls = []
    execute = hip.DmtPlan.execute
    monkeypatch.setattr(hip.DmtPlan, 'execute',
                        lambda self, x, n_in, out, n: (calls.append((n_in, n)), execute(self, x, n_in, out, n))[1])
    for cls in (bt.HostStream, bt.DeviceStream):
        dt = _task(case, 'noise', cls, samples_per_frame=n_out)
        dt.dmt_budget = span * row_in + 300 * (row_in + row_out)           # 300 output samples a launch
        del calls[:]
        assert same_bits(dt.read(), want)
        assert calls == [(300 + span, 300), (300 + span, 300), (n_out - 600 + span, n_out - 600)]
        dt.dmt_budget = 1                                                   # (never less than a sample)
        dt.seek(n_out - 3)
        assert same_bits(dt.read(3), want[-3:])
    for spf in (1, 61, n_out):
        dt = _task(case, 'noise', bt.DeviceStream, samples_per_frame=spf)
        assert dt.samples_per_frame == spf
        for start, count in [(0, 1), (60, 2), (61, 61), (5, 700), (n_out - 1, 1), (333, 200), (0, n_out)]:
            dt.seek(start)
            assert same_bits(dt.read(count), want[start:start + count])
            assert dt.tell() == start + count
        dt.seek(123)
        assert same_bits(dt.read_device(77).to_host(), want[123:200])
        # by time: sample 400 of the output
        dt.seek(dt.start_time + 400 / RATE)
        assert dt.tell() == 400 and same_bits(dt.read(10), want[400:410])
        dt.close()


# -- the identity with DedisperseSamples ------------------------------------------------------------------
@pytest.mark.parametrize('name', ['neg_unsorted', 'ref_below'])
def test_each_trial_is_dedisperse_samples_summed(name):
    """out[i, d] is `DedisperseSamples` for trial d read at i + hi - shifts[d].max() and summed over
    the channels, here on the host in ascending float32."""
    case = dmt_cases.by_name(name)
    shifts = dmt_cases.shifts(case)
    hi = int(shifts.max())
    got = _task(case, 'noise', bt.DeviceStream).read()
    n_out = got.shape[0]
    dh = dmt_cases.stream(case, 'noise', bt.DeviceStream)
    for d, dm in enumerate(case.dms):
        one = bt.DedisperseSamples(dh, dm, reference_frequency=case.reference,
                                   samples_per_frame=case.n - int(np.ptp(shifts[d])))
        np.testing.assert_array_equal(one._shift, shifts[d])
        first = hi - int(shifts[d].max())
        rows = one.read()[first:first + n_out]
        assert rows.shape == (n_out, case.nchan)
        acc = np.zeros(n_out, np.float32)
        for c in range(case.nchan):
            acc += rows[:, c]
        assert same_bits(got[:, d], acc)
        # and on the clock: sample 0 of the trial plane is sample `first` of that task
        assert abs(bt.DMTrials(dh, case.dms, reference_frequency=case.reference).start_time
                   - (one.start_time + first / RATE)) < 1e-9


# -- special values -------------------------------------------------------------------------------------------
def test_nan_inf_and_negative_zero_go_where_their_sweep_goes():
    case = dmt_cases.by_name('neg_unsorted')
    x = dmt_cases.data(case, 'noise').copy()
    # (input times 919 ... 1080 are crossed by every trial's sweep of every channel)
    x[950, 3] = np.nan
    x[1000, 5] = np.inf
    x[1050] = -0.
    x[1060:1070] = 0.
    x[1065] = -0.
    shifts = dmt_cases.shifts(case)
    want = search.dm_trials_samples(x, shifts)
    got = _task(case, x=x, cls=bt.DeviceStream).read()
    assert same_bits(got, want)
    offsets = shifts.max() - shifts
    i = np.arange(got.shape[0])[:, None]
    np.testing.assert_array_equal(np.isnan(got), i + offsets[None, :, 3] == 950)
    np.testing.assert_array_equal(np.isposinf(got), (i + offsets[None, :, 5] == 1000) & ~np.isnan(got))
    assert np.isnan(got).sum() == len(case.dms) and np.isposinf(got).any()
    # a stream of -0 sums to +0 from a +0 start
    zeros = np.full((case.n, case.nchan), -0., np.float32)
    out = _task(case, x=zeros).read()
    assert not out.view(np.uint32).any()


# -- physics ------------------------------------------------------------------------------------------------------
def test_a_dispersed_impulse_peaks_at_its_dm_and_time():
    case = dmt_cases.by_name('neg_unsorted')
    dms = [0., 1.1, 2.3, 3.4]
    sh = dmt_cases.stream(case)
    shifts = search.dm_trial_shifts(sh, dms)
    tau = 1000                                                # arrival at the reference frequency, input sample
    x = np.zeros((case.n, case.nchan), np.float32)
    x[tau - shifts[2], np.arange(case.nchan)] = 1.            # later where the delay is larger (the shift more negative)
    dt = bt.DMTrials(dmt_cases.stream(case, x=x, cls=bt.DeviceStream), dms)
    out = dt.read()
    i = tau - int(shifts.max())
    assert out[i, 2] == case.nchan
    rest = out.copy()
    rest[i, 2] = 0.
    assert rest.max() < case.nchan
    assert abs((dt.start_time + i / RATE) - (T0 + tau / RATE)) < 1e-9


# -- a chain that never leaves HBM -----------------------------------------------------------------------------------
def test_search_chain_on_the_device():
    nh = bt.DeviceNoiseGenerator((64 * 8 * 600,), T0, 10e6, 64 * 8 * 50, dtype=np.complex64, seed=5,
                                 frequency=600e6, sideband=1)
    ig = bt.Integrate(bt.Square(bt.Channelize(nh, 64)), 8)
    dms = [0., 5., 20., 12.5]
    dt = bt.DMTrials(ig, dms)
    stage = dt
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    assert produces_on_device(stage)
    assert dt.shape == (600 - np.ptp(dt.shifts), 4) and dt._span > 100
    got = dt.read_device().to_host()
    ig.seek(0)
    upstream = ig.read()
    assert upstream.shape == (600, 64) and upstream.dtype == np.float32
    assert same_bits(got, search.dm_trials_samples(upstream, dt.shifts))
    dt.seek(17)
    assert same_bits(dt.read(100), got[17:117])


# -- what the plan refuses ------------------------------------------------------------------------------------------------
def test_plan_refuses_bad_tables_and_short_inputs_before_any_launch():
    good = np.array([[0, 3, 7], [7, 1, 0]], np.int32)
    for bad in (np.array([[0, -1, 7], [7, 1, 0]]), np.array([[0, (1 << 24) + 1, 7], [7, 1, 0]])):
        with pytest.raises(hip.HipError, match='offset|span'):
            hip.DmtPlan(bad, 1)
    with pytest.raises(hip.HipError, match='n_rest'):
        hip.DmtPlan(good, hip.DMT_MAX_REST + 1)
    with pytest.raises(hip.HipError, match='nchan'):
        hip.DmtPlan(np.zeros((1, hip.DMT_MAX_NCHAN + 1), np.int32), 1)
    with pytest.raises(hip.HipError, match='ndm'):
        hip.DmtPlan(np.zeros((hip.DMT_MAX_NDM + 1, 1), np.int32), 1)
    plan = hip.DmtPlan(good, 1)
    assert plan.span == 7
    x = hip.DeviceArray.from_host(np.ones((40, 3), np.float32))
    out = hip.DeviceArray.from_host(np.full((33, 2), 5., np.float32))
    with pytest.raises(hip.HipError, match='shorter'):
        plan.execute(x, 39, out, 33)                           # one sample short for 33 outputs
    with pytest.raises(hip.HipError, match='no output'):
        plan.execute(x, 40, out, 0)
    hip.synchronize()
    assert (out.to_host() == 5.).all()                         # nothing ran
    plan.execute(x, 40, out, 33)
    assert (out.to_host() == 3.).all()
    plan.close()
