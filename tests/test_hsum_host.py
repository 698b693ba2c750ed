"""Host side of `fluctuation_spectra`, `Whiten`, `HarmonicSearch` and `harmonic_candidates` (no GPU):
the NumPy twins against brute-force restatements with the gather and the tie rule spelt out in loops
and against float64 within the bound their order implies, the scales, the planted comb, the candidate
rule on a hand-made plane, construction, metadata and the argument checks of the tasks, and the
kernels' tiling (csrc/hsum_geo.hpp) walked on the host by a stand-alone program under sanitizers."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity
from baseband_tasks_amd.periodicity import LEVEL, OFFSET, SNR

import hsum_cases
from hsum_cases import CASES, IDS, RATE, T0
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


# -- the search twin --------------------------------------------------------------------------------------
def _brute(x, n, K, lo, averaged=1.):
    """One spectrum ``(nbin, cols)`` of integers: the int64 sum of the 2^L listed bins round_half_up(j i /
    2^L), i = 1 ... 2^L, the float32 S/N (the sum and 2^L are exact in float32: one subtract, one multiply),
    the winner by the key (snr, -L, -j) among the (L, j) whose fundamental's bin is at least lo."""
    nbin, cols = x.shape
    nb = -(-nbin // n)
    ints = x.astype(np.int64)
    out = np.empty((nb, 3, cols), np.float32)
    scales = [np.float32(np.sqrt(averaged / 2. ** L)) for L in range(K)]
    for e in range(cols):
        col = ints[:, e].tolist()
        for b in range(nb):
            win = None
            for L in range(K):
                h = 1 << L
                for j in range(b * n, min((b + 1) * n, nbin)):
                    fundamental = (2 * j + h) // (2 * h)                      # round_half_up(j / 2^L)
                    if fundamental < lo:
                        continue
                    total = sum(col[(2 * j * i + h) // (2 * h)] for i in range(1, h + 1))
                    snr = (np.float32(total) - np.float32(h)) * scales[L]
                    key = (float(snr), -L, -j)
                    if win is None or key > win:
                        win = key
            out[b, :, e] = (-np.inf, 0, 0) if win is None else (win[0], -win[2] - b * n, -win[1])
    return out


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_is_the_brute_force_rule_on_integers(case):
    x = hsum_cases.data(case)
    got = hsum_cases.expected(case)
    nb = -(-case.nbin // case.n)
    assert got.dtype == np.float32 and got.shape == (case.N, nb, 3) + case.s
    flat = x.reshape(case.N, case.nbin, -1)
    cols = min(flat.shape[2], 3 if case.nbin > 2000 else 7)   # (the loops are slow: a few columns)
    spectra = range(case.N) if case.nbin < 2000 else (0,)
    for s in spectra:
        want = _brute(flat[s, :, :cols], case.n, case.K, case.lo)
        np.testing.assert_array_equal(got[s].reshape(nb, 3, -1)[:, :, :cols], want)
    assert (got[:, :, LEVEL] < case.K).all() and (got[:, :, OFFSET] < case.n).all()
    assert not np.isnan(got).any()
    if case.K > 1 and got[:, :, LEVEL].size > 50:
        assert len(np.unique(got[:, :, LEVEL])) > 1            # (winners at more than one level)


@pytest.mark.parametrize('kind', hsum_cases.KINDS)
@pytest.mark.parametrize('name', hsum_cases.EVERY_LEVEL_WINS)
def test_every_level_wins_in_the_cases_that_pin_an_instantiation(name, kind):
    """The two- and the three-level case are the only ones that reach their instantiation of the search
    kernel: their data must exercise every level of it, behind a ragged last block, a prime element count
    above a wave and a lo that cuts off another first j at every level."""
    case = hsum_cases.by_name(name)
    got = hsum_cases.expected(case, kind)
    assert case.K in (2, 3) and sorted(np.unique(got[:, :, LEVEL]).tolist()) == list(range(case.K))
    assert 0 < case.nbin % case.n < case.n and int(np.prod(case.s)) == 67 and np.isfinite(got).all()
    first = [min(j for j in range(case.n) if (j + ((1 << L) >> 1)) >> L >= case.lo) for L in range(case.K)]
    assert len(set(first)) == case.K and first[0] == case.lo


def test_brute_force_agrees_on_the_prototype_shape():
    rng = np.random.default_rng(11)
    x = rng.integers(0, 9, size=(2, 1501, 7)).astype(np.float32)
    got = periodicity.harmonic_search_samples(x, 61, 5, 1., 3)
    for s in range(2):
        np.testing.assert_array_equal(got[s], _brute(x[s], 61, 5, 3))


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_sums_on_noise_within_the_bound_of_their_adds(case):
    """T_L is 2^L - 1 rounded adds, each off by at most half an ulp of a partial sum that is at most sum
    |p|: |error| <= (2^L - 1) 2^-24 sum |p| over the same bins.  A bound, not a measurement; checked on every
    level, rebuilt as the twin builds it, against the float64 sum (whose own error, a few 2^-53 sum |p|,
    is allowed for)."""
    x = hsum_cases.data(case, 'noise')
    x64 = x.astype(np.float64)
    j = np.arange(case.nbin)
    acc, want, mag = x.copy(), x64.copy(), np.abs(x64)
    differs = False
    for L in range(1, case.K):
        for i in range(1, 1 << L, 2):
            idx = (j * i + (1 << (L - 1))) >> L
            assert idx.max() <= case.nbin - 1 and (idx <= j).all()
            acc = acc + x[:, idx]
            want = want + x64[:, idx]
            mag = mag + np.abs(x64[:, idx])
        assert acc.dtype == np.float32
        assert (np.abs(acc - want) <= (((1 << L) - 1) * 2. ** -24 + 2. ** -48) * mag).all()
        differs = differs or bool((acc != want.astype(np.float32)).any())
    if case.K > 3:
        assert differs                                         # (so the order does matter for these data)
    # finite wherever a block has a bin at or above lo (its level 0 is present), (-inf, 0, 0) in front of that
    got = hsum_cases.expected(case, 'noise')
    first = -(-(case.lo + 1) // case.n) - 1
    assert np.isfinite(got[:, first:]).all()
    assert (got[:, :first, SNR] == -np.inf).all() and not got[:, :first, 1:].any()


def test_twin_winner_is_the_level_sum_less_its_mean_times_the_scale():
    case = hsum_cases.by_name('ragged')
    x = hsum_cases.data(case, 'noise')
    got = hsum_cases.expected(case, 'noise')
    c = periodicity.harmonic_scales(1.)
    for s, b, e in ((0, 0, 0), (1, 7, 33), (2, got.shape[1] - 1, 66), (0, 1, 5)):
        snr, off, L = got[s, b, :, e]
        j, L = b * case.n + int(off), int(L)
        t = x[s, j, e]
        for lev in range(1, L + 1):
            for i in range(1, 1 << lev, 2):
                t = t + x[s, (j * i + (1 << (lev - 1))) >> lev, e]
        assert snr == (t - np.float32(1 << L)) * c[L]
        assert ((j + ((1 << L) >> 1)) >> L) >= case.lo


def test_ties_nan_inf_and_the_lo_rule():
    c = periodicity.harmonic_scales(1.)
    # two equal peaks in one block: the smaller j
    x = np.ones((1, 16, 1), np.float32)
    x[0, 5, 0] = x[0, 9, 0] = 3.
    out = periodicity.harmonic_search_samples(x, 16, 1, 1., 1)
    assert out[0, 0, :, 0].tolist() == [2., 5., 0.]
    # a tie across levels: the smaller L
    c2 = periodicity.harmonic_scales(4.)                       # 2, sqrt(2), 1: exact at levels 0 and 2
    assert c2[0] == 2. and c2[2] == 1.
    y = np.ones((1, 16, 1), np.float32)
    y[0, 13, 0] = 2.                                           # level 0 at j = 13: (2 - 1) * 2 = 2
    y[0, [2, 4, 6, 8], 0] = 1.5                                # level 2 at j = 8 gathers 2, 4, 6, 8: (6 - 4) * 1 = 2
    out = periodicity.harmonic_search_samples(y, 16, 3, 4., 1)
    assert out[0, 0, :, 0].tolist() == [2., 13., 0.]           # the smaller L although the larger j
    y[0, 13, 0] = 1.
    out = periodicity.harmonic_search_samples(y, 16, 3, 4., 1)
    assert out[0, 0, SNR, 0] == 2. and out[0, 0, LEVEL, 0] == 2.
    assert out[0, 0, OFFSET, 0] == 8.                          # the smallest j whose four bins are 2, 4, 6, 8
    # a NaN never wins; it spoils exactly the (L, j) that gather it; an Inf wins where it is gathered
    z = np.ones((1, 32, 1), np.float32)
    z[0, 7, 0] = np.nan
    z[0, 20, 0] = np.inf
    out = periodicity.harmonic_search_samples(z, 8, 2, 1., 1)
    assert not np.isnan(out).any()
    assert out[0, 0, :, 0].tolist() == [0., 1., 0.]            # block 0: bins 1 ... 6 are plain, 7 is NaN; bin 0 is below lo
    assert out[0, 1, :, 0].tolist() == [0., 0., 0.]            # block 1: j = 8 at level 0
    assert out[0, 2, :, 0].tolist() == [np.inf, 4., 0.]        # j = 20 itself
    # nothing but NaN: (-inf, 0, 0); -inf may win over nothing
    v = np.full((1, 6, 1), np.nan, np.float32)
    v[0, 4, 0] = -np.inf
    out = periodicity.harmonic_search_samples(v, 3, 1, 1., 0)
    assert out[0, 0, :, 0].tolist() == [-np.inf, 0., 0.] and out[0, 1, :, 0].tolist() == [-np.inf, 1., 0.]
    # lo per level: with lo = 3 level 0 needs j >= 3, level 1 (j + 1) >> 1 >= 3, level 2 (j + 2) >> 2 >= 3
    out = periodicity.harmonic_search_samples(np.ones((1, 12, 1), np.float32), 3, 1, 1., 3)
    assert [tuple(r) for r in out[0, :2, :, 0].tolist()] == [(-np.inf, 0, 0), (0, 0, 0)]
    ramp = np.arange(12, dtype=np.float32).reshape(1, 12, 1) + 1.       # larger j: larger sums at every level
    out = periodicity.harmonic_search_samples(ramp, 12, 3, 1., 3)
    snr, off, L = out[0, 0, :, 0]
    assert (off, L) == (11., 2.)                               # bins 3, 6, 8, 11: (4 + 7 + 9 + 12 - 4) / 2
    assert snr == (np.float32(4 + 7 + 9 + 12) - np.float32(4)) * c[2]
    # p = 2 everywhere: snr_L = 2^L c_L grows with L, so with one bin per block the winner of block j is the
    # highest level present at j, the highest L whose fundamental's bin round_half_up(j / 2^L) reaches lo
    twos = np.full((1, 40, 1), 2., np.float32)
    for lo in (0, 1, 3, 4):
        got = periodicity.harmonic_search_samples(twos, 1, 4, 1., lo)[0, :, :, 0]
        for j in range(40):
            present = [L for L in range(4) if (2 * j + (1 << L)) // (2 << L) >= lo]
            if present:
                assert got[j].tolist() == [np.float32(1 << present[-1]) * c[present[-1]], 0., present[-1]]
            else:
                assert got[j].tolist() == [-np.inf, 0., 0.]


def test_scales():
    c = periodicity.harmonic_scales()
    assert c.dtype == np.float32 and c.shape == (6,) and (SNR, OFFSET, LEVEL) == (0, 1, 2)
    for L in range(6):
        assert c[L] == np.float32(np.sqrt(1. / 2. ** L))
    assert c[1].view(np.uint32) == 0x3F3504F3
    c8 = periodicity.harmonic_scales(8)
    assert c8[1] == 2. and c8[3] == 1. and c8[5] == .5
    for bad in (0., -1., np.nan, np.inf, 1e-100):
        with pytest.raises(ValueError):
            periodicity.harmonic_scales(bad)


def test_planted_comb():
    p = hsum_cases.comb()
    j = 323
    assert tuple(sorted({(j * i + 4) >> 3 for i in range(1, 9)})) == hsum_cases.COMB_BINS
    best = periodicity.harmonic_search_samples(p, 64, 6)
    c = periodicity.harmonic_scales()
    assert best.shape == (1, 17, 3, 6)
    assert best[0, 5, :, 2].tolist() == [24 * c[3], 3., 3.]
    others = best[0, :, SNR].copy()
    others[5, 2] = -np.inf
    assert others.max() == 6.0
    assert not best[0, :, SNR][:, [0, 1, 3, 4, 5]].any()
    cands = periodicity.harmonic_candidates(best[0], 64, 7.)
    assert len(cands) == 1 and cands.dtype.names == ('bin', 'trial', 'harmonics', 'snr')
    assert (cands['bin'][0], cands['trial'][0], cands['harmonics'][0]) == (40.375, 2, 8)
    assert cands['snr'][0] == 24 * c[3]
    cands = periodicity.harmonic_candidates(best[0], 64, 7., bin_width=0.5)
    assert cands.dtype.names[-1] == 'frequency' and cands['frequency'][0] == 40.375 * 0.5


def test_twin_refusals():
    x = np.ones((2, 20, 2), np.float32)
    for fn, args in ((periodicity.harmonic_search_samples, (5, 3)), (periodicity.whiten_samples, (5,))):
        with pytest.raises(TypeError):
            fn(x.astype(np.float64), *args)
        with pytest.raises(TypeError):
            fn(x.astype(np.complex64), *args)
        with pytest.raises(TypeError):
            fn(x[0, :, 0], *args)
    for n, k, lo in ((0, 3, 1), (65537, 3, 1), (5, 0, 1), (5, 7, 1), (5, 3, 20), (5, 3, -1)):
        with pytest.raises(ValueError):
            periodicity.harmonic_search_samples(x, n, k, 1., lo)
    with pytest.raises(ValueError):
        periodicity.harmonic_search_samples(x, 5, 3, 0.)
    assert periodicity.harmonic_search_samples(x, 65536, 6, 1., 19).shape == (2, 1, 3, 2)
    for m, skip in ((1, 1), (65537, 1), (5, 20), (5, -1)):
        with pytest.raises(ValueError):
            periodicity.whiten_samples(x, m, skip)
    assert periodicity.whiten_samples(x, 65536, 19).shape == x.shape


# -- the whiten twin --------------------------------------------------------------------------------------
@pytest.mark.parametrize('skip', hsum_cases.WH_SKIPS)
@pytest.mark.parametrize('m', hsum_cases.WH_BLOCKS)
def test_whiten_twin_against_float64(m, skip):
    x = hsum_cases.wh_data()
    got = hsum_cases.wh_expected(m, skip)
    assert got.dtype == np.float32 and got.shape == x.shape
    assert not got[:, :skip].view(np.uint32).any()             # +0 below skip
    nbin = x.shape[1]
    edges = list(range(skip, nbin, m)) + [nbin]
    assert edges[-1] - edges[-2] >= 1
    noise = np.arange(6, 67)
    for j0, j1 in zip(edges[:-1], edges[1:]):
        blk = x[:, j0:j1].astype(np.float64)
        z = got[:, j0:j1]
        if j1 - j0 >= 31:
            want = blk[:, :, noise] / blk[:, :, noise].mean(axis=1, keepdims=True)
            assert (np.abs(z[:, :, noise] - want) <= 1e-6 * np.abs(want)).all()
        # the degenerate columns: +0 throughout for all zero, -0, a negative mean, a denormal mean
        for col in (hsum_cases.ZERO, hsum_cases.MINUS_ZERO, hsum_cases.NEGATIVE, hsum_cases.TINY):
            assert not z[:, :, col].view(np.uint32).any()
        # a NaN or an Inf: +0 for the block of the spectrum that holds it, and only that one
        for col, (s, at) in ((hsum_cases.NAN, hsum_cases.NAN_AT), (hsum_cases.INF, hsum_cases.INF_AT)):
            for spec in range(x.shape[0]):
                zero = not z[spec, :, col].view(np.uint32).any()
                assert zero == (spec == s and j0 <= at < j1)
    assert np.isfinite(got).all()
    if m >= 31:
        z64 = got[:, skip:, noise].astype(np.float64)
        assert abs(z64.mean() - 1.) < 1e-6


def test_whiten_twin_step_by_step():
    """One block of 70 bins by hand after two skipped ones, then a last block of 5: three segments (32,
    32, 6), each step rounded once."""
    rng = np.random.default_rng(3)
    x = (2. * rng.standard_exponential((1, 77, 1))).astype(np.float32)
    got = periodicity.whiten_samples(x, 70, 2)
    assert not got[0, :2, 0].view(np.uint32).any()
    for j0, ln in ((2, 70), (72, 5)):
        d = x[0, j0:j0 + ln, 0].astype(np.float64)
        s1 = 0.
        for t0 in range(0, ln, 32):
            a = 0.
            for v in d[t0:t0 + 32]:
                a = a + v
            s1 = s1 + a
        r = np.float32(1. / (s1 / float(ln)))
        want = x[0, j0:j0 + ln, 0] * r
        assert want.dtype == np.float32
        assert (got[0, j0:j0 + ln, 0].view(np.uint32) == want.view(np.uint32)).all()
    # the order matters for a long block: the plain float64 sum in bin order differs somewhere
    y = (2. * rng.standard_exponential((4, 2000, 50))).astype(np.float32)
    z = periodicity.whiten_samples(y, 2000, 0)
    seq = np.zeros((4, 50))
    for t in range(2000):
        seq = seq + y[:, t]
    plain = y * (1. / (seq / 2000.)).astype(np.float32)[:, np.newaxis]
    assert np.abs(z / plain - 1.).max() < 3e-7


# -- candidates -----------------------------------------------------------------------------------------
def _best(snr, off=None, level=None):
    snr = np.asarray(snr, np.float32)
    best = np.zeros((snr.shape[0], 3, snr.shape[1]), np.float32)
    best[:, SNR] = snr
    best[:, OFFSET] = 0 if off is None else off
    best[:, LEVEL] = 0 if level is None else level
    return best


def test_candidates_on_a_hand_made_plane():
    snr = np.zeros((5, 6))
    snr[0, 5] = 9.                       # an edge cell (a corner): 3 neighbours
    snr[2, 1:4] = 8.                     # a plateau of three equal cells: the first in raster order
    snr[3, 2] = 8.                       # ... which also touches the plateau from the next row
    snr[4, 5] = 7.                       # exactly the threshold
    snr[4, 0] = 6.999                    # just below
    off = np.arange(30).reshape(5, 6) % 10
    level = (np.arange(30).reshape(5, 6) % 4)
    cands = periodicity.harmonic_candidates(_best(snr, off, level), 10, 7., bin_width=0.25)
    assert cands.dtype.names == ('bin', 'trial', 'harmonics', 'snr', 'frequency')
    assert cands['bin'].dtype == np.float64 and cands['snr'].dtype == np.float32
    assert cands['snr'].tolist() == [9., 8., 7.]
    assert cands['trial'].tolist() == [5, 1, 5]
    assert cands['harmonics'].tolist() == [2 ** (5 % 4), 2 ** (13 % 4), 2 ** (29 % 4)]
    assert cands['bin'].tolist() == [(0 * 10 + 5) / 2, (2 * 10 + 3) / 2, (4 * 10 + 9) / 2]
    assert cands['frequency'].tolist() == [b * 0.25 for b in cands['bin'].tolist()]
    # the threshold is inclusive; above every value nothing is left
    assert len(periodicity.harmonic_candidates(_best(snr), 10, 6.999)) == 4
    assert len(periodicity.harmonic_candidates(_best(snr), 10, 9.5)) == 0
    # equal candidates sort by bin, then trial
    two = np.zeros((4, 4))
    two[3, 0] = two[0, 3] = two[0, 0] = 5.
    c = periodicity.harmonic_candidates(_best(two), 3, 1.)
    assert list(zip(c['bin'].tolist(), c['trial'].tolist())) == [(0., 0), (0., 3), (9., 0)]
    # a plateau that fills the plane has one candidate, its first cell
    c = periodicity.harmonic_candidates(_best(np.full((3, 3), 4.)), 2, 4.)
    assert len(c) == 1 and (c['bin'][0], c['trial'][0]) == (0., 0)
    # the same rule as boxcar_candidates, cell for cell
    rng = np.random.default_rng(5)
    plane = _best(rng.integers(0, 4, size=(9, 8)))
    a = periodicity.harmonic_candidates(plane, 1, 2.)
    b = bt.search.boxcar_candidates(plane, 1, 2.)
    assert sorted(zip(a['bin'].astype(int).tolist(), a['trial'].tolist())) == \
        sorted(zip(b['sample'].tolist(), b['trial'].tolist()))
    with pytest.raises(ValueError):
        periodicity.harmonic_candidates(np.zeros((4, 2, 3), np.float32), 2, 1.)
    with pytest.raises(ValueError):
        periodicity.harmonic_candidates(np.zeros((4, 3), np.float32), 2, 1.)


# -- construction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_search_stream_surface(case):
    sh = hsum_cases.stream(case)
    hs = bt.HarmonicSearch(sh, case.n, case.K, 1., case.lo)
    nb = -(-case.nbin // case.n)
    assert hs.shape == (case.N, nb, 3) + case.s and hs.dtype == np.float32
    assert hs.sample_rate == RATE and hs.samples_per_frame == case.N
    assert abs(hs.start_time - bt.Time(T0)) < 1e-9
    assert (hs.n, hs.n_levels, hs.lo, hs.averaged) == (case.n, case.K, case.lo, 1.)
    assert hs.scales.view(np.uint32).tolist() == periodicity.harmonic_scales().view(np.uint32).tolist()
    assert bt.HarmonicSearch(sh, case.n, samples_per_frame=1).samples_per_frame == 1
    text = repr(hs)
    assert text.startswith('HarmonicSearch(ih') and 'ih: HostStream' in text
    assert hs._input_span(0, 1) == (sh, 0, case.N)
    hs.hsum_budget = 1                                         # (never less than a spectrum)
    assert hs._chunk_size() == 1 and (hs._input_span(0, 1) is None) == (case.N > 1)
    hs.close()
    assert hs.closed
    default = bt.HarmonicSearch(sh, case.n)
    assert (default.n_levels, default.lo, default.averaged) == (5, 1, 1.)


def test_whiten_stream_surface():
    sh = hsum_cases.wh_stream(samples_per_frame=2)
    for m in hsum_cases.WH_BLOCKS:
        wh = bt.Whiten(sh, m)
        assert wh.shape == hsum_cases.WH_SHAPE and wh.dtype == np.float32
        assert wh.sample_rate == RATE and abs(wh.start_time - bt.Time(T0)) < 1e-9
        assert wh.samples_per_frame == 2 and (wh.m, wh.skip) == (m, 1)
        assert repr(wh).startswith('Whiten(ih')
    wh = bt.Whiten(sh, 50, 5, samples_per_frame=3)
    assert wh.samples_per_frame == 3 and wh.skip == 5
    assert wh._input_span(0, 1) == (sh, 0, 3)
    wh.whiten_budget = 2 * 2100 * 67 * 4
    assert wh._chunk_size() == 2 and wh._input_span(0, 1) is None


def test_metadata():
    """Metadata that vary along the bin axis are dropped by the search and kept by Whiten; those that
    do not are kept; a lone frequency is passed on."""
    x = np.ones((4, 30, 3), np.float32)
    per_bin = np.linspace(4e8, 8e8, 30).reshape(30, 1)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=per_bin, sideband=1,
                       polarization=np.array(['X', 'Y', 'X']))
    wh = bt.Whiten(sh, 8)
    np.testing.assert_array_equal(wh.frequency, sh.frequency)
    assert wh.sideband == 1
    hs = bt.HarmonicSearch(wh, 7, 2)
    assert hs.shape == (4, 5, 3, 3)
    for attr in ('frequency', 'sideband'):
        with pytest.raises(AttributeError):
            getattr(hs, attr)
    np.testing.assert_array_equal(np.broadcast_to(hs.polarization, (5, 3, 3))[4, 2], ['X', 'Y', 'X'])
    # per element: kept, with the sideband
    el = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=np.array([1e8, 2e8, 3e8]),
                       sideband=np.array([1, -1, 1]), polarization=np.arange(30).reshape(30, 1) % 2)
    hs = bt.HarmonicSearch(el, 7, 2)
    np.testing.assert_array_equal(np.broadcast_to(hs.frequency, (5, 3, 3))[1, 1], [1e8, 2e8, 3e8])
    np.testing.assert_array_equal(np.broadcast_to(hs.sideband, (5, 3, 3))[0, 2], [1, -1, 1])
    with pytest.raises(AttributeError):
        hs.polarization
    # a lone frequency, as the plane of DMTrials has
    src = bt.HostStream(np.zeros((300, 4), np.float32), bt.Time(T0), 1e4, pin=False,
                        frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(src, [0., .1, .2])
    wh = bt.Whiten(plane, 2, 0)                                # (the trials as "bins": only the labels matter here)
    assert wh.frequency == plane.frequency
    with pytest.raises(AttributeError):
        wh.sideband
    hs = bt.HarmonicSearch(plane, 2, 1, 1., 0)
    assert hs.frequency == plane.frequency and hs.shape == (plane.shape[0], 2, 3)
    with pytest.raises(AttributeError):
        hs.sideband


def test_fluctuation_spectra_on_a_plane():
    src = bt.HostStream(np.zeros((2000, 4), np.float32), bt.Time(T0), 1e4, pin=False,
                        frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(src, [0., .1, .2])
    with pytest.raises(TypeError):
        bt.Channelize(plane, 64)                               # (what the helper is for: a frequency and no sideband)
    for n, stack in ((64, 1), (64, 4), (256, 2)):
        sp = bt.periodicity.fluctuation_spectra(plane, n, stack)
        assert sp.dtype == np.float32
        assert sp.shape == (plane.shape[0] // n // stack, n // 2 + 1, 3)
        assert sp.sample_rate == pytest.approx(1e4 / (n * stack), rel=1e-12)
        assert sp.bin_width == 1e4 / n
        assert abs(sp.start_time - plane.start_time) < 1e-9
        hs = bt.HarmonicSearch(bt.Whiten(sp, 8), 8, 3, averaged=stack)
        assert hs.shape == (sp.shape[0], -(-(n // 2 + 1) // 8), 3, 3)
        with pytest.raises(AttributeError):
            hs.frequency
    # a stream that has its sideband is used as it is
    sp = bt.fluctuation_spectra(src, 64, 2)
    assert sp.shape == (2000 // 128, 33, 4) and sp.ih.ih.ih is src
    with pytest.raises(TypeError):
        bt.fluctuation_spectra(bt.HostStream(np.zeros((200, 2), np.complex64), bt.Time(T0), 1e4, pin=False), 64)
    with pytest.raises(ValueError):
        bt.fluctuation_spectra(src, 64, 0)


def test_what_is_refused():
    x = np.ones((4, 100, 3), np.float32)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False)
    z = bt.HostStream(x.astype(np.complex64), bt.Time(T0), RATE, pin=False)
    f64 = bt.HostStream(x.astype(np.float64), bt.Time(T0), RATE, pin=False)
    flat = bt.HostStream(x[:, :, 0].ravel(), bt.Time(T0), RATE, pin=False)
    for cls, args in ((bt.Whiten, (10,)), (bt.HarmonicSearch, (10, 3))):
        with pytest.raises(TypeError, match='Square'):
            cls(z, *args)
        with pytest.raises(TypeError, match='float32'):
            cls(f64, *args)
        with pytest.raises(ValueError, match='bin axis'):
            cls(flat, *args)
        with pytest.raises(TypeError):
            cls(sh, 10.5)
    for m in (1, 65537, 0):
        with pytest.raises(ValueError, match='whitening block'):
            bt.Whiten(sh, m)
    bt.Whiten(sh, 2), bt.Whiten(sh, 65536), bt.Whiten(sh, 10, 0), bt.Whiten(sh, 10, 99)
    for skip in (-1, 100):
        with pytest.raises(ValueError, match='skip'):
            bt.Whiten(sh, 10, skip)
    for n in (0, 65537):
        with pytest.raises(ValueError, match='search block'):
            bt.HarmonicSearch(sh, n)
    bt.HarmonicSearch(sh, 1), bt.HarmonicSearch(sh, 65536, 6, lo=99)
    for k in (0, 7, -1):
        with pytest.raises(ValueError, match='n_levels'):
            bt.HarmonicSearch(sh, 10, k)
    for lo in (-1, 100):
        with pytest.raises(ValueError, match='lo'):
            bt.HarmonicSearch(sh, 10, 3, lo=lo)
    for averaged in (0., -2., np.nan):
        with pytest.raises(ValueError, match='averaged'):
            bt.HarmonicSearch(sh, 10, 3, averaged)
    assert (hip.HSUM_MIN_M, hip.HSUM_MAX_M, hip.HSUM_MAX_N, hip.HSUM_MAX_LEVELS, hip.HSUM_MAX_NBIN) == \
        (2, 65536, 65536, 6, 1 << 24)


def test_library_exports_the_periodicity_search():
    lib = hip.lib()
    assert lib.bbt_version() >= 165
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_hsum_whiten', 'bbt_hsum_plan_create', 'bbt_hsum_plan_destroy', 'bbt_hsum_plan_info',
                 'bbt_hsum_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'hsum_geo.hpp')).read()
    assert f'#define BBT_HSUM_MAX_M {hip.HSUM_MAX_M}' in geo and f'#define BBT_HSUM_MAX_N {hip.HSUM_MAX_N}' in geo
    assert f'#define BBT_HSUM_MAX_LEVELS {hip.HSUM_MAX_LEVELS}' in geo and '#define BBT_HSUM_MAX_NBIN (1 << 24)' in geo
    assert f'#define BBT_HSUM_SEG {periodicity.SEGMENT}' in geo and f'#define BBT_HSUM_MIN_M {hip.HSUM_MIN_M}' in geo
    assert bt.periodicity is periodicity
    assert all(name in periodicity.__all__ and hasattr(bt, name) for name in
               ('fluctuation_spectra', 'Whiten', 'whiten_samples', 'HarmonicSearch', 'harmonic_search_samples',
                'harmonic_candidates'))
    # the tiling and a plan's scales need no device to ask
    info = hip.hsum_info()
    assert (info['width'], info['split'], info['rows']) == (64, 16, 8) and not info['scales'].any()
    scales = periodicity.harmonic_scales(8.)
    plan = hip.HsumPlan(100, 10, 4, 1, 3, scales)
    assert plan.n_blocks == 10
    got = plan.info()['scales']
    assert got[:4].view(np.uint32).tolist() == scales[:4].view(np.uint32).tolist() and not got[4:].any()
    plan.close()
    for args, what in (((0, 10, 4, 0, 3), 'spectrum'), (((1 << 24) + 1, 10, 4, 1, 3), 'spectrum'),
                       ((100, 0, 4, 1, 3), 'search block'), ((100, 65537, 4, 1, 3), 'search block'),
                       ((100, 10, 0, 1, 3), 'n_levels'), ((100, 10, 7, 1, 3), 'n_levels'),
                       ((100, 10, 4, 100, 3), 'lo'), ((100, 10, 4, -1, 3), 'lo'), ((100, 10, 4, 1, 0), 'elements')):
        with pytest.raises(hip.HipError, match=what):
            hip.HsumPlan(*args, np.ones(6, np.float32))
    with pytest.raises(hip.HipError, match='scales'):
        hip.HsumPlan(100, 10, 4, 1, 3, np.array([1., 1., 0., 1.], np.float32))
    with pytest.raises(hip.HipError, match='scales'):
        hip.HsumPlan(100, 10, 2, 1, 3, np.array([1., np.inf], np.float32))
    with pytest.raises(ValueError):
        hip.HsumPlan(100, 10, 4, 1, 3, np.ones(3, np.float32))


# -- the tiling, on the host ----------------------------------------------------------------------------
def _geo_shapes():
    """(kind, ...): every shared case under every tiling the GPU tests walk and cut into the launches
    they make (1 and 2 spectra), the limits, and spectra of 2^24 bins."""
    shapes = []
    for case in CASES:
        e = int(np.prod(case.s, dtype=int))
        for width, split in [(0, 0)] + hsum_cases.TILINGS:
            for n_spec in sorted({case.N, 1, min(2, case.N)}):
                shapes.append((0, n_spec, case.nbin, case.n, case.K, case.lo, e, width, split))
    shapes += [(0, 1, 1025, 64, 6, 1, 6, 0, 0), (0, 7, 33, 8, 4, 1, 4, 0, 0),
               (0, 1, 1, 1, 1, 0, 1, 0, 0), (0, 1, 1, 65536, 6, 0, 1, 16, 16), (0, 3, 70000, 65536, 6, 69999, 3, 64, 16),
               (0, 1, 1 << 24, 65536, 6, 1, 1, 0, 0), (0, 2, 1 << 24, 4096, 6, (1 << 24) - 1, 70, 16, 16),
               (0, 1, 1 << 24, 1000, 5, 1, 2, 32, 1),
               # more than 2^31 values in the chunk
               (0, 64, 8193, 64, 5, 1, 4100, 64, 4)]
    e = hsum_cases.WH_SHAPE[2]
    for m in hsum_cases.WH_BLOCKS:
        for skip in hsum_cases.WH_SKIPS:
            for rows in (0, 1, 8, 16):
                for n_spec in (3, 1, 2):
                    shapes.append((1, n_spec, hsum_cases.WH_SHAPE[1], e, m, skip, rows, 0, 0))
    shapes += [(1, 1, 1, 1, 2, 0, 0, 0, 0), (1, 1, 65, 300, 65536, 64, 16, 0, 0), (1, 4, 33, 4, 8, 1, 0, 0, 0),
               (1, 64, 8193, 512, 128, 1, 8, 0, 0), (1, 1, 1 << 24, 2, 65536, 1, 2, 0, 0),
               (1, 64, 8193, 4100, 128, 1, 8, 0, 0)]
    return shapes


def test_kernel_tiling_on_the_host(tmp_path):
    """Every (spectrum, block, part, element tile) owned by exactly one row of threads, every gathered
    index inside its spectrum, the whitening blocks tiling the bins, the limits and refusals: the
    program exits non-zero otherwise, and the sanitizers abort it on a wild index or an overflow of its
    own."""
    exe = compile_check('hsum_geo_check', tmp_path)
    shapes = _geo_shapes()
    plans = run_check(exe, shapes)
    for shape, g in zip(shapes, plans):
        assert g['walk'] == 0, (shape, g)
        if shape[0] == 0:
            _, n_spec, nbin, n, K, lo, e, width, split = shape
            assert g['nb'] == -(-nbin // n) and g['n_pair'] == n_spec * g['nb']
            assert g['nx'] == (width or 64) and g['nx'] * g['ny'] == 256 and g['sub'] * g['nz'] == g['ny']
            assert g['sub'] == min(g['ny'], split or 16, 2 ** (n.bit_length() - 1))
            assert g['n_tile'] == -(-e // g['nx']) and g['n_wg'] == -(-g['n_pair'] // g['nz']) * g['n_tile']
        else:
            _, n_spec, nbin, e, m, skip, rows = shape[:7]
            assert g['ny'] == (rows or 8) and g['nx'] * g['ny'] == 256
            assert g['n_blk'] == -(-(nbin - skip) // m) + (skip > 0)
            assert g['n_tile'] == -(-e // g['nx']) and g['n_wg'] == n_spec * g['n_blk'] * g['n_tile']
    assert sum(1 for s in shapes if s[0] == 0 and s[2] == 1 << 24) == 3
    # what the library refuses: no spectra, too many bins, a block of 0 and of 65537, n_levels 0 and 7, lo = nbin,
    # no elements, bad tilings; whiten: m = 1, skip = nbin, no spectra, bad rows
    bad = run_raw(exe, '0 0 100 10 1 1 3 0 0  0 1 16777217 10 1 1 3 0 0  0 2 100 0 1 1 3 0 0 '
                       '0 2 100 65537 1 1 3 0 0  0 2 100 10 0 1 3 0 0  0 2 100 10 7 1 3 0 0 '
                       '0 2 100 10 1 100 3 0 0  0 2 100 10 1 1 0 0 0  0 2 100 10 1 1 3 48 0 '
                       '0 2 100 10 1 1 3 0 3  1 3 100 5 1 1 0 0 0  1 3 100 5 2 100 0 0 0 '
                       '1 0 100 5 2 1 0 0 0  1 3 100 5 2 1 3 0 0')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 14
    assert 'no spectra' in errors[0] and '2^24' in errors[1] and '65536' in errors[2] and '65536' in errors[3]
    assert 'n_levels' in errors[4] and 'n_levels' in errors[5] and 'lo' in errors[6] and 'elements' in errors[7]
    assert 'width' in errors[8] and 'split' in errors[9] and '2 ... 65536' in errors[10] and 'skip' in errors[11]
    assert 'no spectra' in errors[12] and 'rows' in errors[13]
