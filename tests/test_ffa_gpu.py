"""`FFASearch` on the GPU against its NumPy twin (`ffa.ffa_search_samples`), bit for bit: a folded bin is a
fixed binary tree over its rows, a boxcar a fixed tree over its bins and the winner the maximum of a total
order, so a value has one correct result whatever the tiling or the chunking.  The shared cases of
ffa_cases.py (test_ffa_host.py proves the twin), every tiling the environment can ask for, chunks over
columns and base periods, frames and seeks, NaN / Inf / -0, a planted pulsar, a device chain from noise to
candidates, and the plan's refusals."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import ffa, hip
from baseband_tasks_amd.base import _stream_rate
from baseband_tasks_amd.device_task import produces_on_device
from baseband_tasks_amd.ffa import SNR

import ffa_cases
from ffa_cases import CASES, IDS, KINDS, RATE, same_bits

pytestmark = pytest.mark.gpu

T0 = bt.Time(ffa_cases.T0)


def _task(case, kind='int', cls=None, x=None, **kwargs):
    return bt.FFASearch(ffa_cases.stream(case, kind, cls, x), case.n, case.periods, case.K, **kwargs)


def _plan_run(x, n, periods, K):
    n_elem = int(np.prod(x.shape[1:], dtype=int))
    plan = hip.FfaPlan(n, periods, K, n_elem)
    nb = x.shape[0] // n
    got = np.empty((nb, periods[1] - periods[0], 4) + x.shape[1:], np.float32)
    for b in range(nb):
        out = hip.DeviceArray(got.shape[1:], np.float32)
        plan.execute(hip.DeviceArray.from_host(x[b * n:(b + 1) * n]), out)
        got[b] = out.to_host()
    plan.close()
    return got


# -- the shared cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_task_and_plan_equal_the_twin(case, kind):
    want = ffa_cases.expected(case, kind)
    got = _task(case, kind).read()
    assert got.dtype == np.float32 and same_bits(got, want)
    dev = _task(case, kind, bt.DeviceStream)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), want)
    assert same_bits(_plan_run(ffa_cases.data(case, kind), case.n, case.periods, case.K), want)


@pytest.mark.parametrize('fuse, width', ffa_cases.TILINGS)
@pytest.mark.parametrize('name', ['ragged', 'long_fold', 'wide'])
def test_no_value_depends_on_the_tiling(name, fuse, width, monkeypatch):
    """BBT_FFA_FUSE and BBT_FFA_WIDTH reshape the passes and the S/N workgroups; the tree and the total order
    are the contract, so every bit stays."""
    case = ffa_cases.by_name(name)
    monkeypatch.setenv('BBT_FFA_FUSE', str(fuse))
    monkeypatch.setenv('BBT_FFA_WIDTH', str(width))
    info = hip.ffa_info()
    assert (info['fuse'], info['width']) == (fuse, width)
    for kind in KINDS:
        assert same_bits(_task(case, kind, bt.DeviceStream).read(), ffa_cases.expected(case, kind))


# -- chunks, frames, seeks ----------------------------------------------------------------------------------
def test_budgets_cut_the_columns_then_the_base_periods(monkeypatch):
    case = ffa_cases.by_name('ragged')
    want = ffa_cases.expected(case, 'noise')
    calls = []
    execute = hip.FfaPlan.execute
    monkeypatch.setattr(hip.FfaPlan, 'execute', lambda self, x, out, e0, ne, pa, pb:
                        (calls.append((e0, ne, pa, pb)), execute(self, x, out, e0, ne, pa, pb))[1])
    block = case.n * 67 * 4
    column = (2 * (700 // 32 + 1) + 10 + 2 * 64 * 21) * 4
    for cls in (bt.HostStream, bt.DeviceStream):
        fs = _task(case, 'noise', cls, samples_per_frame=2)
        del calls[:]
        assert same_bits(fs.read(), want)
        assert calls == [(0, 67, 16, 23)] * 2
        assert fs._plan.info()['scratch_bytes'] == 67 * column
        # 30 columns a launch, all base periods: columns only
        fs.ffa_budget = block + 30 * (column + 16 * 7)
        fs.invalidate_cache()
        fs.seek(0)
        del calls[:]
        assert same_bits(fs.read(), want)
        assert calls == [(0, 30, 16, 23), (30, 30, 16, 23), (60, 7, 16, 23)] * 2
        assert fs._plan.info()['scratch_bytes'] == 67 * column                # (it only grows)
        # 19 columns of four base periods
        fs.ffa_budget = block + 19 * column + 19 * 16 * 4 + 100
        fs.invalidate_cache()
        fs.seek(0)
        del calls[:]
        assert same_bits(fs.read(), want)
        one = [(e0, 19, pa, pb) for e0 in (0, 19, 38) for pa, pb in ((16, 20), (20, 23))] + [(57, 10, 16, 23)]
        assert calls == one * 2
        # a budget of 1: one column of one base period a launch, never less
        fs.ffa_budget = 1
        fs.invalidate_cache()
        fs.seek(1)
        del calls[:]
        assert same_bits(fs.read(1), want[1:])
        assert calls == [(e, 1, p, p + 1) for e in range(67) for p in range(16, 23)] * 2      # (the frame is both blocks)
        fs.close()


def test_frames_and_seeks():
    case = ffa_cases.Case('blocks', (6,), 1000, 90, (7, 11), 2, 31)
    x = ffa_cases.data(case, 'noise')
    want = ffa.ffa_search_samples(x, case.n, case.periods, case.K)
    nb = want.shape[0]
    assert nb == 11
    for spf in (1, 4, nb):
        fs = _task(case, 'noise', bt.DeviceStream, samples_per_frame=spf)
        assert fs.samples_per_frame == spf and fs.shape == want.shape
        for start, count in [(0, 1), (3, 2), (4, 4), (2, nb - 3), (nb - 1, 1), (0, nb)]:
            fs.seek(start)
            assert same_bits(fs.read(count), want[start:start + count])
            assert fs.tell() == start + count
        fs.seek(3)
        assert same_bits(fs.read_device(5).to_host(), want[3:8])
        fs.close()
    # by time, into the second block of the case with two
    case = ffa_cases.by_name('wide')
    fs = _task(case, 'noise', bt.DeviceStream)
    fs.seek(fs.start_time + case.n / RATE)
    assert fs.tell() == 1 and same_bits(fs.read(1), ffa_cases.expected(case, 'noise')[1:])
    assert abs(fs.start_time - T0) < 1e-9 and fs.sample_rate == RATE / case.n


# -- special values -------------------------------------------------------------------------------------------
def test_nan_and_inf_spoil_exactly_the_periods_whose_used_samples_hold_them():
    case = ffa_cases.by_name('ragged')
    n = case.n
    x = ffa_cases.data(case, 'noise').copy()
    # block 1, sample 697 of it: used by p with 697 < (700 // p) p: 16 (688: no), 17 (697: no), 18 (684: no), 19 (684: no),
    # 20 (700: yes), 21 (693: no), 22 (682: no)
    used = {p: (n // p) * p for p in range(16, 23)}
    assert [p for p in used if 697 < used[p]] == [20]
    x[n + 697, 3] = np.nan
    x[300, 5] = np.inf                                         # block 0: every base period uses sample 300
    x[n + 699, 11] = np.inf                                    # in the dropped tail of every base period but 20
    assert [p for p in used if 699 < used[p]] == [20]
    x[:, 7] = np.nan
    x[:, 9] = -0.
    x[:, 13] = 0.
    want = ffa.ffa_search_samples(x, n, case.periods, case.K)
    got = _task(case, x=x, cls=bt.DeviceStream).read()
    assert same_bits(got, want)
    clean = ffa_cases.expected(case, 'noise')
    spoilt = np.zeros(got.shape[:2] + got.shape[3:], bool)     # (block, base period, column)
    spoilt[1, 20 - 16, 3] = spoilt[0, :, 5] = spoilt[1, 20 - 16, 11] = True
    spoilt[:, :, [7, 9, 13]] = True
    for f in range(4):
        assert same_bits(got[:, :, f][~spoilt], clean[:, :, f][~spoilt])
    nothing = np.array([-np.inf, 0., 0., 0.], np.float32)
    # a NaN never wins; a column that holds one is all NaN: nothing wins.  +inf makes T, and so every c_k, +inf:
    # every S/N is -inf or NaN, and -inf wins at the first cell that has it
    assert not np.isnan(got).any()
    assert (got[1, 4, :, 3] == nothing).all() and (got[:, :, :, 7] == nothing).all()
    assert (got[0, :, SNR, 5] == -np.inf).all() and (got[1, 4, SNR, 11] == -np.inf)
    # -0 and 0: every S/N is a zero; the first cell wins, and its bits are what the twin's are
    for col in (9, 13):
        assert (got[:, :, SNR, col] == 0.).all() and not got[:, :, 1:, col].any()
    assert not got[:, :, SNR, 13].view(np.uint32).any()


# -- a planted pulsar -------------------------------------------------------------------------------------------------
def test_a_planted_pulsar_is_recovered_with_its_period():
    c = ffa_cases.PLANTED
    x, want = ffa_cases.planted_data(), ffa_cases.planted_expected()
    sh = bt.DeviceStream(x, T0, RATE, samples_per_frame=x.shape[0], frequency=600e6, sideband=1)
    fs = bt.FFASearch(sh, c['n'], c['periods'], c['K'])
    best = fs.read()
    assert same_bits(best, want)
    snr, shift, k, j = best[0, 31 - 29, :, c['column']]
    assert abs(shift - 102) <= 3 and snr > 18.9 / 2
    cands = ffa.ffa_candidates(best[0], c['n'], c['periods'], 8., RATE)
    assert len(cands) == 1
    assert (cands['bins'][0], cands['trial'][0], cands['snr'][0]) == (31, c['column'], snr)
    assert abs(cands['period'][0] * RATE - c['period']) < 3 / 255 + 1e-9


# -- a chain that never leaves HBM -----------------------------------------------------------------------------------
def test_search_chain_on_the_device():
    nh = bt.DeviceNoiseGenerator((64 * 8 * 600,), T0, 10e6, 64 * 8 * 50, dtype=np.complex64, seed=5,
                                 frequency=600e6, sideband=1)
    dt = bt.DMTrials(bt.Integrate(bt.Square(bt.Channelize(nh, 64)), 8), [0., 5., 20., 12.5])
    plane = bt.SetAttribute(dt, frequency=dt.frequency, sideband=1)
    st = bt.Standardize(bt.Integrate(plane, 2), 64)
    fs = bt.FFASearch(st, 64, (10, 16), n_widths=3)
    stage = fs
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    assert produces_on_device(stage)
    assert fs.shape == (st.shape[0] // 64, 6, 4, 4) and fs.shape[0] >= 2 and abs(fs.start_time - dt.start_time) < 1e-9
    got = fs.read_device().to_host()
    st.seek(0)
    z = st.read()
    assert same_bits(got, ffa.ffa_search_samples(z, 64, (10, 16), 3))
    assert np.isfinite(got).all() and got[:, :, SNR].max() > 2.
    fs.seek(1)
    assert same_bits(fs.read(1), got[1:2])
    cands = ffa.ffa_candidates(got[0], 64, (10, 16), 2.5, _stream_rate(st))
    assert len(cands) and (cands['period'] >= 10 / _stream_rate(st)).all() and (cands['period'] <= 16 / _stream_rate(st)).all()
    assert cands.dtype == ffa.CANDIDATE_DTYPE and (np.diff(cands['snr']) <= 0).all()


# -- what the plan refuses ------------------------------------------------------------------------------------------------
def test_plan_refuses_bad_launches_before_any_launch():
    plan = hip.FfaPlan(100, (8, 12), 2, 3)
    x = hip.DeviceArray.from_host(np.ones((100, 3), np.float32))
    out = hip.DeviceArray.from_host(np.full((4, 4, 3), 5., np.float32))
    for e0, ne in ((0, 4), (1, 3), (3, 1), (-1, 2), (0, 0)):
        with pytest.raises(hip.HipError, match='columns'):
            plan.execute(x, out, e0, ne)
    for pa, pb in ((7, 9), (8, 13), (9, 9), (10, 9)):
        with pytest.raises(hip.HipError, match='periods'):
            plan.execute(x, out, 0, 3, pa, pb)
    with pytest.raises(ValueError):
        plan.execute(hip.DeviceArray((99, 3), np.float32), out)
    with pytest.raises(ValueError):
        plan.execute(x, hip.DeviceArray((3, 4, 3), np.float32))
    with pytest.raises(ValueError):
        plan.execute(hip.DeviceArray((100, 3), np.complex64), out)
    hip.synchronize()
    assert (out.to_host() == 5.).all()                         # nothing ran
    assert plan.info()['scratch_bytes'] == 0
    # one column of two base periods: the other cells stay
    plan.execute(x, out, 1, 1, 9, 11)
    got = out.to_host()
    touched = np.zeros((4, 4, 3), bool)
    touched[1:3, :, 1] = True
    assert (got[~touched] == 5.).all()
    # ones: every S/N is (m - m) a = 0 at the first cell
    assert not got[touched].any()
    assert plan.info()['scratch_bytes'] == plan.info()['column_floats'] * 4
    plan.close()
