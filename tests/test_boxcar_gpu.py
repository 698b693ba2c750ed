"""`Standardize` and `BoxcarSearch` on the GPU against their NumPy twins (`search.standardize_samples`,
`search.boxcar_search_samples`), bit for bit: a window sum is a fixed binary tree over its own
samples and the winner is the maximum of a total order, so a value has one correct result whatever
the tiling or the chunking.  The shared cases of sps_cases.py (test_boxcar_host.py proves the twins),
every tiling the environment can ask for, chunks, pieces and seeks, NaN / Inf / -0, a planted pulse,
a device chain from noise to candidates, and the plan's refusals."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, search
from baseband_tasks_amd.device_task import produces_on_device
from baseband_tasks_amd.search import OFFSET, SNR, WIDTH

import sps_cases
from sps_cases import CASES, IDS, KINDS, RATE, same_bits

pytestmark = pytest.mark.gpu

T0 = bt.Time(sps_cases.T0)


def _task(case, kind='int', cls=None, x=None, **kwargs):
    return bt.BoxcarSearch(sps_cases.stream(case, kind, cls, x), case.n, case.K, **kwargs)


def _plan_run(x, n, K):
    n_elem = int(np.prod(x.shape[1:], dtype=int))
    plan = hip.SpsPlan(n, K, n_elem)
    nb = x.shape[0] // n
    out = hip.DeviceArray((nb, 3) + x.shape[1:], np.float32)
    plan.execute(hip.DeviceArray.from_host(x), x.shape[0], out, nb)
    got = out.to_host()
    plan.close()
    return got


# -- the shared cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_task_and_plan_equal_the_twin(case, kind):
    want = sps_cases.expected(case, kind)
    got = _task(case, kind).read()
    assert got.dtype == np.float32 and same_bits(got, want)
    dev = _task(case, kind, bt.DeviceStream)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), want)
    assert same_bits(_plan_run(sps_cases.data(case, kind), case.n, case.K), want)


@pytest.mark.parametrize('width, fuse, split', sps_cases.TILINGS)
@pytest.mark.parametrize('name', ['ragged', 'long_halo', 'wide'])
def test_no_value_depends_on_the_tiling(name, width, fuse, split, monkeypatch):
    """BBT_SPS_WIDTH, BBT_SPS_FUSE and BBT_SPS_SPLIT reshape the workgroups and the passes, from the
    smallest to the largest; the tree and the total order are the contract, so every bit stays."""
    case = sps_cases.by_name(name)
    monkeypatch.setenv('BBT_SPS_WIDTH', str(width))
    monkeypatch.setenv('BBT_SPS_FUSE', str(fuse))
    monkeypatch.setenv('BBT_SPS_SPLIT', str(split))
    plan = hip.SpsPlan(case.n, case.K, 1)
    info = plan.info()
    assert (info['width'], info['fuse'], info['split']) == (width, fuse, split)
    plan.close()
    for kind in KINDS:
        assert same_bits(_task(case, kind, bt.DeviceStream).read(), sps_cases.expected(case, kind))


# -- Standardize ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sps_cases.STD_BLOCKS)
def test_standardize_equals_its_twin(n):
    want = sps_cases.std_expected(n)
    got = bt.Standardize(sps_cases.std_stream(), n).read()
    assert got.dtype == np.float32 and same_bits(got, want)
    dev = bt.Standardize(sps_cases.std_stream(bt.DeviceStream), n)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), want)
    x = sps_cases.std_data()
    out = hip.sps_standardize(hip.DeviceArray.from_host(x), n, x.shape[1])
    assert same_bits(out.to_host().reshape(want.shape), want)
    # the degenerate blocks are +0: the constant, the all-zero and the -0 column throughout
    assert not got[:, [0, 1, 4]].view(np.uint32).any()
    assert np.isfinite(got).all()


@pytest.mark.parametrize('rows', [1, 2, 4, 8, 16])
def test_standardize_does_not_depend_on_the_tiling(rows, monkeypatch):
    monkeypatch.setenv('BBT_SPS_STD_ROWS', str(rows))
    assert hip.sps_info()['std_rows'] == rows
    for n in sps_cases.STD_BLOCKS:
        got = bt.Standardize(sps_cases.std_stream(bt.DeviceStream), n).read()
        assert same_bits(got, sps_cases.std_expected(n))


def test_standardize_chunks_frames_and_seeks(monkeypatch):
    n = 33
    want = sps_cases.std_expected(n)
    length = want.shape[0]
    calls = []
    run = hip.sps_standardize
    monkeypatch.setattr(hip, 'sps_standardize',
                        lambda x, n_, e, out=None: (calls.append(x.size // e), run(x, n_, e, out=out))[1])
    for cls in (bt.HostStream, bt.DeviceStream):
        st = bt.Standardize(sps_cases.std_stream(cls), n, samples_per_frame=length)
        st.standardize_budget = 20 * n * 67 * 4                               # 20 blocks a launch
        del calls[:]
        assert same_bits(st.read(), want)
        assert calls == [20 * n] * 3 + [length - 60 * n]
        st.standardize_budget = 1                                             # (never less than a block)
        st.invalidate_cache()
        st.seek(length - 3)
        del calls[:]
        assert same_bits(st.read(3), want[-3:])
        assert calls == [n] * 63
    for spf in (n, 7 * n, length):
        st = bt.Standardize(sps_cases.std_stream(bt.DeviceStream), n, samples_per_frame=spf)
        for start, count in [(0, 1), (32, 2), (33, 33), (5, 700), (length - 1, 1), (0, length)]:
            st.seek(start)
            assert same_bits(st.read(count), want[start:start + count])
        st.seek(st.start_time + 400 / RATE)
        assert st.tell() == 400 and same_bits(st.read_device(10).to_host(), want[400:410])
        st.close()


# -- chunks, pieces, frames, seeks ----------------------------------------------------------------------
@pytest.mark.parametrize('name, per', [('ragged', 5), ('long_halo', 7)])
def test_chunks_pieces_frames_and_seeks(name, per, monkeypatch):
    case = sps_cases.by_name(name)
    want = sps_cases.expected(case, 'noise')
    nb, halo = want.shape[0], 2 ** (case.K - 1) - 1
    row = int(np.prod(case.s)) * 4
    calls = []
    execute = hip.SpsPlan.execute
    monkeypatch.setattr(hip.SpsPlan, 'execute',
                        lambda self, x, n_in, out, n: (calls.append((n_in, n)), execute(self, x, n_in, out, n))[1])
    chunks = [(b0, min(nb, b0 + per)) for b0 in range(0, nb, per)]
    launches = [(min(case.N, b1 * case.n + halo) - b0 * case.n, b1 - b0) for b0, b1 in chunks]
    if name == 'ragged':
        assert launches == [(5 * 61 + 31, 5)] * 4 + [(1495 - 20 * 61, 4)]
    else:
        assert launches[0] == (4200, 7) and launches[-1] == (4200 - 63 * 64, 2) and len(launches) == 10
    for cls in (bt.HostStream, bt.DeviceStream):
        bs = _task(case, 'noise', cls, samples_per_frame=nb)
        bs.sps_budget = 3 * halo * row + per * (3 * case.n * row + 3 * row)   # `per` blocks a launch
        del calls[:]
        assert same_bits(bs.read(), want)
        assert calls == launches
        info = bs._plan.info()
        assert info['scratch_bytes'] == min(-(-case.K // info['fuse']) - 1, 2) * launches[0][0] * row
        bs.sps_budget = 1                                                      # (never less than a block)
        bs.invalidate_cache()
        bs.seek(nb - 3)
        del calls[:]
        assert same_bits(bs.read(3), want[-3:])
        assert [c[1] for c in calls] == [1] * nb                               # (the frame is the whole stream)
        bs.close()
    for spf in (1, 7, nb):
        bs = _task(case, 'noise', bt.DeviceStream, samples_per_frame=spf)
        assert bs.samples_per_frame == spf
        for start, count in [(0, 1), (6, 2), (7, 7), (2, nb - 3), (nb - 1, 1), (0, nb)]:
            bs.seek(start)
            assert same_bits(bs.read(count), want[start:start + count])
            assert bs.tell() == start + count
        bs.seek(3)
        assert same_bits(bs.read_device(9).to_host(), want[3:12])
        # by time: block 11 of the output
        bs.seek(bs.start_time + 11 * case.n / RATE)
        assert bs.tell() == 11 and same_bits(bs.read(5), want[11:16])
        bs.close()


# -- special values -------------------------------------------------------------------------------------------
def test_nan_and_inf_reach_exactly_the_windows_that_cross_them():
    case = sps_cases.by_name('ragged')
    n, halo = case.n, 2 ** (case.K - 1) - 1
    x = sps_cases.data(case, 'noise').copy()
    t_nan, t_inf = 700, 915                                   # (915 = 15 * 61: the first sample of block 15)
    x[t_nan, 3] = np.nan
    x[t_inf, 5] = np.inf
    x[:, 7] = np.nan
    x[:, 9] = -0.
    want = search.boxcar_search_samples(x, n, case.K)
    got = _task(case, x=x, cls=bt.DeviceStream).read()
    assert same_bits(got, want)
    clean = sps_cases.expected(case, 'noise')
    nb = got.shape[0]
    first = np.arange(nb) * n                                  # a block's windows cover [first, first + n - 1 + halo]
    for t, e in ((t_nan, 3), (t_inf, 5)):
        reached = (first <= t) & (t <= first + n - 1 + halo)
        assert reached.sum() == 2                              # the block that holds it and the one in front
        assert same_bits(got[~reached, :, e], clean[~reached, :, e])
    # a NaN never wins
    assert not np.isnan(got).any()
    # the Inf wins wherever a window crosses it, at the smallest width that reaches it, then the earliest start
    assert got[15, :, 5].tolist() == [np.inf, 0., 0.]
    assert got[14, :, 5].tolist() == [np.inf, n - 1., 1.]      # (start 914, width 2)
    assert np.isfinite(got[np.r_[0:14, 16:nb], SNR, 5]).all()
    # nothing but NaN: (-inf, 0, 0); a column of -0 gives what the twin gives: -0 at the first start, width 1
    assert (got[:, SNR, 7] == -np.inf).all() and not got[:, 1:, 7].any()
    assert (got[:, SNR, 9].view(np.uint32) == 0x80000000).all() and not got[:, 1:, 9].any()


# -- a planted pulse ----------------------------------------------------------------------------------------------
def test_a_planted_pulse_is_recovered_with_its_width_and_start():
    case = sps_cases.by_name('wide')
    x = np.zeros((case.N,) + case.s, np.float32)
    x[300:308, 123, 2] = 3.
    bs = _task(case, x=x, cls=bt.DeviceStream)
    best = bs.read()
    assert best.shape == (4, 3, 300, 4)
    assert best[1, :, 123, 2].tolist() == [24 * search.BOXCAR_SCALES[3], 300 - 256, 3.]
    others = best[:, SNR].copy()
    others[1, 123, 2] = -np.inf
    assert others.max() < best[1, SNR, 123, 2]
    cands = search.boxcar_candidates(best.reshape(4, 3, 1200), case.n, 7.)
    assert len(cands) == 1
    assert (cands['sample'][0], cands['trial'][0], cands['width'][0]) == (300, 123 * 4 + 2, 8)
    assert cands['snr'][0] == best[1, SNR, 123, 2]
    assert abs((bs.start_time + (cands['sample'][0] // case.n) * case.n / RATE) - (T0 + 256 / RATE)) < 1e-9


# -- a chain that never leaves HBM -----------------------------------------------------------------------------------
def test_search_chain_on_the_device():
    nh = bt.DeviceNoiseGenerator((64 * 8 * 600,), T0, 10e6, 64 * 8 * 50, dtype=np.complex64, seed=5,
                                 frequency=600e6, sideband=1)
    dt = bt.DMTrials(bt.Integrate(bt.Square(bt.Channelize(nh, 64)), 8), [0., 5., 20., 12.5])
    st = bt.Standardize(dt, 64)
    bs = bt.BoxcarSearch(st, 16, n_widths=5)
    stage = bs
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    assert produces_on_device(stage)
    n_plane = dt.shape[0]
    assert st.shape == (n_plane // 64 * 64, 4) and bs.shape == (st.shape[0] // 16, 3, 4)
    assert bs.frequency == dt.frequency and abs(bs.start_time - dt.start_time) < 1e-9
    got = bs.read_device().to_host()
    dt.seek(0)
    upstream = dt.read()
    z = search.standardize_samples(upstream, 64)
    st.seek(0)
    assert same_bits(st.read(), z)
    assert same_bits(got, search.boxcar_search_samples(z, 16, 5))
    assert np.isfinite(got).all() and got[:, SNR].max() > 2.
    bs.seek(5)
    assert same_bits(bs.read(10), got[5:15])
    cands = search.boxcar_candidates(got, 16, 3.)
    assert cands.dtype == search.CANDIDATE_DTYPE and (np.diff(cands['snr']) <= 0).all()


# -- what the plan refuses ------------------------------------------------------------------------------------------------
def test_plan_refuses_bad_sizes_and_short_inputs_before_any_launch():
    for k in (0, 14):
        with pytest.raises(hip.HipError, match='n_widths'):
            hip.SpsPlan(10, k, 3)
    for n in (0, hip.SPS_MAX_N + 1):
        with pytest.raises(hip.HipError, match='block'):
            hip.SpsPlan(n, 3, 3)
    with pytest.raises(hip.HipError, match='elements'):
        hip.SpsPlan(10, 3, 0)
    plan = hip.SpsPlan(10, 3, 2)
    x = hip.DeviceArray.from_host(np.ones((40, 2), np.float32))
    out = hip.DeviceArray.from_host(np.full((4, 3, 2), 5., np.float32))
    with pytest.raises(hip.HipError, match='shorter'):
        plan.execute(x, 39, out, 4)                            # one sample short for 4 blocks
    with pytest.raises(hip.HipError, match='no output'):
        plan.execute(x, 40, out, 0)
    with pytest.raises(ValueError):
        plan.execute(x, 41, out, 4)                            # (more samples than the array holds)
    hip.synchronize()
    assert (out.to_host() == 5.).all()                         # nothing ran
    assert plan.info()['scratch_bytes'] == 0
    plan.execute(x, 40, out, 4)
    got = out.to_host()
    # ones: the widest window that fits wins, 4 * c_2 = 2, at the first start; the last block has 10 samples left
    assert got[:, SNR].tolist() == [[2., 2.]] * 4 and not got[:, OFFSET].any() and (got[:, WIDTH] == 2.).all()
    plan.close()
    # Standardize: a block of 1
    xs = hip.DeviceArray.from_host(np.ones((8, 2), np.float32))
    with pytest.raises(ValueError):
        hip.sps_standardize(xs, 1, 2)
    with pytest.raises(ValueError):
        hip.sps_standardize(xs, 4, 2, out=hip.DeviceArray((7, 2), np.float32))
    with pytest.raises(TypeError):
        hip.sps_standardize(hip.DeviceArray((8, 2), np.complex64), 4, 2)
