"""`Whiten` and `HarmonicSearch` on the GPU against their NumPy twins (`periodicity.whiten_samples`,
`periodicity.harmonic_search_samples`), bit for bit: a block's mean is one float64 sum in a fixed
order, a harmonic sum is one float32 accumulator with the bins added in a fixed order and the winner
is the maximum of a total order, so a value has one correct result whatever the tiling or the
chunking.  The shared cases of hsum_cases.py (test_hsum_host.py proves the twins), tilings, chunks,
frames, NaN / Inf, the planted comb, a device chain from noise to candidates, and the plan's
refusals."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity
from baseband_tasks_amd.device_task import produces_on_device
from baseband_tasks_amd.periodicity import LEVEL, OFFSET, SNR

import hsum_cases
from hsum_cases import CASES, IDS, KINDS, same_bits

pytestmark = pytest.mark.gpu

T0 = bt.Time(hsum_cases.T0)


def _task(case, kind='int', cls=None, x=None, **kwargs):
    return bt.HarmonicSearch(hsum_cases.stream(case, kind, cls, x), case.n, case.K, hsum_cases.AVERAGED, case.lo,
                             **kwargs)


def _plan_run(x, n, K, lo, averaged=1.):
    n_elem = int(np.prod(x.shape[2:], dtype=int))
    plan = hip.HsumPlan(x.shape[1], n, K, lo, n_elem, periodicity.harmonic_scales(averaged))
    out = hip.DeviceArray((x.shape[0], plan.n_blocks, 3) + x.shape[2:], np.float32)
    plan.execute(hip.DeviceArray.from_host(x), x.shape[0], out)
    got = out.to_host()
    plan.close()
    return got


# -- the shared cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_task_and_plan_equal_the_twin(case, kind):
    want = hsum_cases.expected(case, kind)
    got = _task(case, kind).read()
    assert got.dtype == np.float32 and same_bits(got, want)
    dev = _task(case, kind, bt.DeviceStream)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), want)
    assert same_bits(_plan_run(hsum_cases.data(case, kind), case.n, case.K, case.lo), want)


@pytest.mark.parametrize('width, split', hsum_cases.TILINGS)
@pytest.mark.parametrize('name', ['ragged', 'rfft', 'wide'])
def test_no_value_depends_on_the_tiling(name, width, split, monkeypatch):
    """BBT_HSUM_WIDTH and BBT_HSUM_SPLIT reshape the workgroups, from the smallest to the largest; the
    order of the adds and the total order are the contract, so every bit stays."""
    case = hsum_cases.by_name(name)
    monkeypatch.setenv('BBT_HSUM_WIDTH', str(width))
    monkeypatch.setenv('BBT_HSUM_SPLIT', str(split))
    info = hip.hsum_info()
    assert (info['width'], info['split']) == (width, split)
    for kind in KINDS:
        assert same_bits(_task(case, kind, bt.DeviceStream).read(), hsum_cases.expected(case, kind))


# -- Whiten -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('skip', hsum_cases.WH_SKIPS)
@pytest.mark.parametrize('m', hsum_cases.WH_BLOCKS)
def test_whiten_equals_its_twin(m, skip):
    want = hsum_cases.wh_expected(m, skip)
    got = bt.Whiten(hsum_cases.wh_stream(), m, skip).read()
    assert got.dtype == np.float32 and same_bits(got, want)
    dev = bt.Whiten(hsum_cases.wh_stream(bt.DeviceStream), m, skip)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), want)
    x = hsum_cases.wh_data()
    out = hip.hsum_whiten(hip.DeviceArray.from_host(x), x.shape[1], x.shape[2], m, skip)
    assert same_bits(out.to_host().reshape(want.shape), want)
    # the degenerate columns are +0 throughout, and so is everything below skip
    special = [hsum_cases.ZERO, hsum_cases.MINUS_ZERO, hsum_cases.NEGATIVE, hsum_cases.TINY]
    assert not got[:, :, special].view(np.uint32).any() and not got[:, :skip].view(np.uint32).any()
    assert np.isfinite(got).all()


@pytest.mark.parametrize('rows', [1, 8, 16])
def test_whiten_does_not_depend_on_the_tiling(rows, monkeypatch):
    monkeypatch.setenv('BBT_HSUM_ROWS', str(rows))
    assert hip.hsum_info()['rows'] == rows
    for m in hsum_cases.WH_BLOCKS:
        for skip in hsum_cases.WH_SKIPS:
            got = bt.Whiten(hsum_cases.wh_stream(bt.DeviceStream), m, skip).read()
            assert same_bits(got, hsum_cases.wh_expected(m, skip))


def test_whiten_chunks_and_frames(monkeypatch):
    m, skip = 33, 5
    want = hsum_cases.wh_expected(m, skip)
    n_spec, nbin, n_elem = want.shape
    calls = []
    run = hip.hsum_whiten
    monkeypatch.setattr(hip, 'hsum_whiten', lambda x, nbin_, e, m_, s_, out=None:
                        (calls.append(x.size // (nbin_ * e)), run(x, nbin_, e, m_, s_, out=out))[1])
    for cls in (bt.HostStream, bt.DeviceStream):
        for per, launches in ((1, [1, 1, 1]), (2, [2, 1]), (3, [3])):
            wh = bt.Whiten(hsum_cases.wh_stream(cls), m, skip)
            assert wh.samples_per_frame == n_spec                             # everything in one frame
            wh.whiten_budget = per * nbin * n_elem * 4
            del calls[:]
            assert same_bits(wh.read(), want)
            assert calls == launches
        wh.whiten_budget = 1                                                  # (never less than a spectrum)
        wh.invalidate_cache()
        wh.seek(2)
        del calls[:]
        assert same_bits(wh.read(1), want[2:])
        assert calls == [1, 1, 1]
    wh = bt.Whiten(hsum_cases.wh_stream(bt.DeviceStream, samples_per_frame=1), m, skip)
    assert wh.samples_per_frame == 1
    for start, count in [(1, 1), (0, 2), (2, 1), (0, 3)]:
        wh.seek(start)
        assert same_bits(wh.read(count), want[start:start + count])
    wh.seek(1)
    assert same_bits(wh.read_device(2).to_host(), want[1:3])


# -- chunks and frames ------------------------------------------------------------------------------------
def test_search_chunks_and_frames(monkeypatch):
    case = hsum_cases.by_name('single_bin_blocks')                            # four spectra
    want = hsum_cases.expected(case, 'noise')
    row = int(np.prod(case.s)) * 4
    nb = want.shape[1]
    calls = []
    execute = hip.HsumPlan.execute
    monkeypatch.setattr(hip.HsumPlan, 'execute',
                        lambda self, x, n_spec, out: (calls.append(n_spec), execute(self, x, n_spec, out))[1])
    for cls in (bt.HostStream, bt.DeviceStream):
        for per, launches in ((1, [1] * 4), (2, [2, 2]), (4, [4])):
            hs = _task(case, 'noise', cls)
            assert hs.samples_per_frame == case.N
            hs.hsum_budget = per * (case.nbin + 3 * nb) * row
            del calls[:]
            assert same_bits(hs.read(), want)
            assert calls == launches
            hs.close()
    for spf in (1, 3, case.N):
        hs = _task(case, 'noise', bt.DeviceStream, samples_per_frame=spf)
        assert hs.samples_per_frame == spf
        for start, count in [(0, 1), (1, 2), (3, 1), (0, 4)]:
            hs.seek(start)
            assert same_bits(hs.read(count), want[start:start + count])
            assert hs.tell() == start + count
        hs.seek(hs.start_time + 2 / hsum_cases.RATE)
        assert hs.tell() == 2 and same_bits(hs.read_device(2).to_host(), want[2:4])
        hs.close()


# -- special values -----------------------------------------------------------------------------------------
def test_nan_and_inf_reach_exactly_the_cells_whose_gathers_reach_them():
    case = hsum_cases.by_name('ragged')
    n, K, lo = case.n, case.K, case.lo
    x = hsum_cases.data(case, 'noise').copy()
    at_nan, at_inf = (1, 700, 3), (2, 305, 5)                 # (305 = 5 * 61: the first bin of block 5)
    x[at_nan] = np.nan
    x[at_inf] = np.inf
    x[0, :, 7] = np.nan
    want = periodicity.harmonic_search_samples(x, n, K, 1., lo)
    got = _task(case, x=x, cls=bt.DeviceStream).read()
    assert same_bits(got, want)
    clean = hsum_cases.expected(case, 'noise')
    nb = got.shape[1]
    # the (L, j) that gather bin t, by the rule itself
    j = np.arange(case.nbin)
    for (s, t, e), special in ((at_nan, 'nan'), (at_inf, 'inf')):
        reached = np.zeros((K, case.nbin), bool)
        hit = j == t
        for L in range(K):
            for i in range(1, 1 << L, 2):
                hit = hit | (((j * i + (1 << (L - 1))) >> L) == t)
            reached[L] = hit & (((j + ((1 << L) >> 1)) >> L) >= lo)
        blocks = np.unique(j[reached.any(axis=0)] // n)
        assert len(blocks) > 3 and blocks[0] == t // n
        others = np.setdiff1d(np.arange(nb), blocks)
        # every other cell of the column, and every other column and spectrum, is what it was
        assert same_bits(got[s, others, :, e], clean[s, others, :, e])
        keep = np.ones(got.shape[0], bool)
        keep[s] = False
        assert same_bits(got[keep][..., e], clean[keep][..., e])
        if special == 'inf':
            # the Inf wins every block that reaches it, at the smallest level, then the smallest j, that does
            assert (got[s, blocks, SNR, e] == np.inf).all()
            assert got[s, t // n, :, e].tolist() == [np.inf, 0., 0.]
            for b in blocks:
                in_block = reached[:, b * n:(b + 1) * n]
                L = int(np.nonzero(in_block.any(axis=1))[0][0])
                assert got[s, b, LEVEL, e] == L and got[s, b, OFFSET, e] == np.nonzero(in_block[L])[0][0]
            assert np.isfinite(got[s, others, SNR, e]).all()
    # a NaN never wins; a spectrum of nothing else gives (-inf, 0, 0)
    assert not np.isnan(got).any()
    assert (got[0, :, SNR, 7] == -np.inf).all() and not got[0, :, 1:, 7].any()
    assert np.isfinite(got[1:, :, SNR, 7]).all()


# -- the planted comb ------------------------------------------------------------------------------------------
def test_the_planted_comb_is_recovered():
    p = hsum_cases.comb()
    sh = bt.DeviceStream(p, T0, hsum_cases.RATE, samples_per_frame=1)
    best = bt.HarmonicSearch(sh, 64, 6).read()
    c = periodicity.harmonic_scales()
    assert best.shape == (1, 17, 3, 6)
    assert best[0, 5, :, 2].tolist() == [24 * c[3], 3., 3.]
    others = best[0, :, SNR].copy()
    others[5, 2] = -np.inf
    assert others.max() == 6.0
    assert not best[0, :, SNR][:, [0, 1, 3, 4, 5]].any()
    cands = periodicity.harmonic_candidates(best[0], 64, 7., bin_width=2.)
    assert len(cands) == 1
    assert (cands['bin'][0], cands['trial'][0], cands['harmonics'][0]) == (40.375, 2, 8)
    assert cands['snr'][0] == best[0, 5, SNR, 2] and cands['frequency'][0] == 80.75
    assert same_bits(best, periodicity.harmonic_search_samples(p, 64, 6))


# -- a chain that never leaves HBM ----------------------------------------------------------------------------
def test_periodicity_chain_on_the_device():
    nh = bt.DeviceNoiseGenerator((64 * 8 * 600,), T0, 10e6, 64 * 8 * 50, dtype=np.complex64, seed=5,
                                 frequency=600e6, sideband=1)
    dt = bt.DMTrials(bt.Integrate(bt.Square(bt.Channelize(nh, 64)), 8), [0., 5., 20., 12.5])
    sp = bt.periodicity.fluctuation_spectra(dt, 64, stack=2)
    wh = bt.Whiten(sp, 8)
    hs = bt.HarmonicSearch(wh, 8, n_levels=4, averaged=2)
    stage = hs
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    assert produces_on_device(stage)
    n_spec = dt.shape[0] // 128
    assert n_spec >= 2 and sp.shape == (n_spec, 33, 4) and wh.shape == sp.shape and hs.shape == (n_spec, 5, 3, 4)
    assert sp.bin_width == dt.sample_rate / 64
    assert abs(hs.start_time - dt.start_time) < 1e-9 and hs.sample_rate == sp.sample_rate
    with pytest.raises(AttributeError):
        hs.frequency
    got = hs.read_device().to_host()
    sp.seek(0)
    spectra = sp.read()
    assert spectra.dtype == np.float32 and np.isfinite(spectra).all() and (spectra[:, 1:] > 0).all()
    z = periodicity.whiten_samples(spectra, 8)
    wh.seek(0)
    assert same_bits(wh.read(), z)
    assert same_bits(got, periodicity.harmonic_search_samples(z, 8, 4, 2., 1))
    assert np.isfinite(got).all() and got[:, :, SNR].max() > 1.
    hs.seek(1)
    assert same_bits(hs.read(1), got[1:2])
    cands = periodicity.harmonic_candidates(got[0], 8, 1., sp.bin_width)
    assert len(cands) and (np.diff(cands['snr']) <= 0).all()
    assert (cands['frequency'] == cands['bin'] * sp.bin_width).all()


# -- what the plan refuses ------------------------------------------------------------------------------------
def test_plan_refuses_bad_sizes_before_any_launch():
    scales = periodicity.harmonic_scales()
    for k in (0, 7):
        with pytest.raises(hip.HipError, match='n_levels'):
            hip.HsumPlan(40, 10, k, 1, 2, scales)
    for n in (0, hip.HSUM_MAX_N + 1):
        with pytest.raises(hip.HipError, match='search block'):
            hip.HsumPlan(40, n, 3, 1, 2, scales)
    with pytest.raises(hip.HipError, match='lo'):
        hip.HsumPlan(40, 10, 3, 40, 2, scales)
    with pytest.raises(hip.HipError, match='elements'):
        hip.HsumPlan(40, 10, 3, 1, 0, scales)
    plan = hip.HsumPlan(40, 10, 3, 1, 2, scales)
    x = hip.DeviceArray.from_host(np.ones((2, 40, 2), np.float32))
    out = hip.DeviceArray.from_host(np.full((2, 4, 3, 2), 5., np.float32))
    with pytest.raises(hip.HipError, match='no spectra'):
        plan.execute(x, 0, out)
    with pytest.raises(ValueError):
        plan.execute(x, 3, out)                                # (more spectra than the arrays hold)
    with pytest.raises(ValueError):
        plan.execute(hip.DeviceArray((2, 40, 2), np.complex64), 2, out)
    # a misaligned pointer, straight through the C ABI
    lib = hip.lib()
    assert lib.bbt_hsum_execute(plan._h, x.ptr + 2, 1, out.ptr, None) != 0 and b'aligned' in lib.bbt_last_error()
    assert lib.bbt_hsum_execute(plan._h, None, 1, out.ptr, None) != 0 and b'null' in lib.bbt_last_error()
    assert lib.bbt_hsum_whiten(x.ptr, out.ptr + 1, 1, 8, 2, 2, 1, None) != 0 and b'aligned' in lib.bbt_last_error()
    assert lib.bbt_hsum_whiten(x.ptr, out.ptr, 1, 8, 2, 1, 1, None) != 0 and b'whitening block' in lib.bbt_last_error()
    assert lib.bbt_hsum_whiten(x.ptr, out.ptr, 1, 8, 2, 2, 8, None) != 0 and b'skip' in lib.bbt_last_error()
    hip.synchronize()
    assert (out.to_host() == 5.).all()                         # nothing ran
    plan.execute(x, 2, out)
    got = out.to_host()
    # ones: every sum equals its mean, S/N 0 everywhere; the first present (L, j) wins: level 0 at the block's
    # first bin, which in block 0 is bin lo = 1
    assert not got[:, :, SNR].any() and not got[:, :, LEVEL].any()
    assert got[:, :, OFFSET].tolist() == [[[1., 1.], [0., 0.], [0., 0.], [0., 0.]]] * 2
    plan.close()
    # Whiten through the wrapper
    xs = hip.DeviceArray.from_host(np.ones((2, 8, 2), np.float32))
    for m, skip in ((1, 1), (65537, 1), (4, 8), (4, -1)):
        with pytest.raises(ValueError):
            hip.hsum_whiten(xs, 8, 2, m, skip)
    with pytest.raises(ValueError):
        hip.hsum_whiten(xs, 8, 2, 4, 1, out=hip.DeviceArray((2, 7, 2), np.float32))
    with pytest.raises(ValueError):
        hip.hsum_whiten(xs, 7, 2, 4, 1)
    with pytest.raises(TypeError):
        hip.hsum_whiten(hip.DeviceArray((2, 8, 2), np.complex64), 8, 2, 4, 1)
    got = hip.hsum_whiten(xs, 8, 2, 4, 1).to_host()
    assert not got[:, 0].any() and (got[:, 1:] == 1.).all()
