"""Host side of `FFASearch` and its helpers (no GPU): the NumPy twin against a brute-force restatement with
int64 profile sums from the closed-form shifts and the tie rule spelt out in loops, the transform row by row,
the bound on the shifts, the scales, hand-made ties, special values, the candidate rule, the ladder of
`ffa_plan`, construction, metadata and refusals, the agreement of header, bindings and library, and the
kernels' tiling (csrc/ffa_geo.hpp) walked on the host by a stand-alone program under sanitizers."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import ffa, hip
from baseband_tasks_amd.ffa import PHASE, SHIFT, SNR, WIDTH

import ffa_cases
from ffa_cases import CASES, IDS, RATE, T0
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


# -- the twin ---------------------------------------------------------------------------------------------
def _brute(x, p, K):
    """One block ``x`` (n, columns) of integers at one base period: int64 profile sums from `ffa_shift` by loops,
    the S/N rounded as the rule says (the integer sum is the float32 sum: everything is exact), the winner found
    with loops in (t, k, j) order so that ties keep the earlier."""
    n, cols = x.shape
    m, M = ffa.ffa_rows(n, p)
    xi = x.astype(np.int64)
    scales = [np.float32(np.sqrt(np.float64(p) / np.float64((1 << k) * (p - (1 << k)) * m))) for k in range(K)]
    out = np.empty((4, cols), np.float64)
    for e in range(cols):
        col = xi[:, e]
        total = np.float64(int(col[:m * p].sum()))
        c = [np.float32(total * np.float64(1 << k) / np.float64(p)) for k in range(K)]
        win = None
        for t in range(M):
            prof = np.zeros(p, np.int64)
            for r in range(m):
                s = ffa.ffa_shift(r, t, M)
                prof += np.roll(col[r * p:(r + 1) * p], -s)
            for k in range(K):
                w = 1 << k
                box = sum(np.roll(prof, -i) for i in range(w))
                for j in range(p):
                    snr = (np.float32(box[j]) - c[k]) * scales[k]
                    assert snr.dtype == np.float32
                    if win is None or snr > win[0]:
                        win = (snr, t, k, j)
        out[:, e] = win
    return out


BRUTE_COLUMNS = {'long_fold': [0, 4], 'wide': [0, 77]}
BRUTE_PERIODS = {'long_fold': [9], 'wide': [31]}


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_is_the_brute_force_rule_on_integers(case):
    x = ffa_cases.data(case)
    got = ffa_cases.expected(case)
    p_lo, p_hi = case.periods
    assert got.dtype == np.float32 and got.shape == (case.N // case.n, p_hi - p_lo, 4) + case.s
    n_elem = int(np.prod(case.s))
    flat, out = x.reshape(case.N, n_elem), got.reshape(got.shape[:3] + (n_elem,))
    cols = BRUTE_COLUMNS.get(case.name, list(range(min(n_elem, 3))))
    periods = BRUTE_PERIODS.get(case.name, [p_lo, p_hi - 1] if case.name == 'ragged' else list(range(p_lo, p_hi))[:3])
    if case.name == 'long_fold':
        # (M = 8192 rows of 4444 folds each by loops is minutes: the rows around the winner and the ends)
        for p in periods:
            m, M = ffa.ffa_rows(case.n, p)
            for e in cols:
                snr, t, k, j = out[0, p - p_lo, :, e]
                rows = ffa.ffa_transform_samples(np.concatenate(
                    [flat[:m * p, e].reshape(m, p), np.zeros((M - m, p), np.float32)]))
                for tt in sorted({0, 1, int(t), M // 2, M - 1}):
                    prof = sum(np.roll(flat[r * p:(r + 1) * p, e].astype(np.int64), -ffa.ffa_shift(r, tt, M))
                               for r in range(m))
                    np.testing.assert_array_equal(rows[tt], prof.astype(np.float32))
        return
    for b in range(got.shape[0]):
        for p in periods:
            want = _brute(flat[b * case.n:(b + 1) * case.n][:, cols], p, case.K)
            np.testing.assert_array_equal(out[b, p - p_lo][:, cols], want.astype(np.float32))
    # the winners are inside their ranges
    assert np.isfinite(got[:, :, SNR]).all() and (got[:, :, WIDTH] < case.K).all()
    for i, p in enumerate(range(p_lo, p_hi)):
        assert (got[:, i, PHASE] < p).all() and (got[:, i, SHIFT] < ffa.ffa_rows(case.n, p)[1]).all()


def test_long_fold_winner_is_the_level_sum_times_the_scale():
    """The winner of the longest fold, rebuilt from the transform: its value is the twin's own level at its own
    cell, and no cell of that column beats it."""
    case = ffa_cases.by_name('long_fold')
    x, got = ffa_cases.data(case), ffa_cases.expected(case)
    p = 10
    m, M = ffa.ffa_rows(case.n, p)
    assert (m, M) == (4000, 4096) and ffa.ffa_rows(case.n, 9) == (4444, 8192)
    d = np.zeros((M, p, 5), np.float32)
    d[:m] = x[:m * p].reshape(m, p, 5)
    level = ffa.ffa_transform_samples(d)
    scales = ffa.ffa_scales(p, m, case.K)
    total = x[:m * p].astype(np.float64).sum(axis=0)                     # (integers: any order)
    every = []
    for k in range(case.K):
        c = (total * 2. ** k / p).astype(np.float32)
        every.append((level - c) * scales[k])
        level = level + np.roll(level, -(1 << k), axis=1)
    for e in range(5):
        snr, t, k, j = got[0, 1, :, e]
        assert snr == every[int(k)][int(t), int(j), e]
        assert snr == max(v[:, :, e].max() for v in every)


@pytest.mark.parametrize('M, p', [(1, 5), (2, 4), (8, 7), (32, 9), (64, 5)])
def test_transform_rows_are_the_closed_form_shifts(M, p):
    rng = np.random.default_rng(M + p)
    d = rng.integers(-4, 5, size=(M, p, 2)).astype(np.float32)
    got = ffa.ffa_transform_samples(d)
    assert got.dtype == np.float32 and got.shape == d.shape
    for t in range(M):
        want = sum(np.roll(d[r], -ffa.ffa_shift(r, t, M), axis=0) for r in range(M))
        np.testing.assert_array_equal(got[t], want)
    # the rule itself, stage by stage, with roll
    out = d
    G = 2
    while G <= M:
        new = np.empty_like(out)
        for g in range(0, M, G):
            a, b = out[g:g + G // 2], out[g + G // 2:g + G]
            for t in range(G):
                new[g + t] = a[t >> 1] + np.roll(b[t >> 1], -((t + 1) >> 1), axis=0)
        out, G = new, G * 2
    assert ffa_cases.same_bits(got, out)
    with pytest.raises(ValueError):
        ffa.ffa_transform_samples(np.zeros((3, 4), np.float32))
    with pytest.raises(TypeError):
        ffa.ffa_transform_samples(np.zeros((4, 4), np.float64))


def test_transform_on_noise_is_the_tree_not_the_running_sum():
    rng = np.random.default_rng(5)
    d = rng.standard_normal((64, 11)).astype(np.float32)
    got = ffa.ffa_transform_samples(d)
    running = np.zeros((64, 11), np.float32)
    for t in range(64):
        for r in range(64):
            running[t] = running[t] + np.roll(d[r], -ffa.ffa_shift(r, t, 64))
    assert (got != running).any()                                        # (so the order does matter)
    exact = np.array([sum(np.roll(d[r].astype(np.float64), -ffa.ffa_shift(r, t, 64)) for r in range(64)) for t in range(64)])
    # 6 levels of adds, each off by half an ulp of a partial sum of at most sum |d|
    assert (np.abs(got - exact) <= 6 * 2. ** -24 * np.abs(d).sum(axis=0).max()).all()


@pytest.mark.parametrize('M', [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024])
def test_shift_bound(M):
    """6 |shift (M - 1) - r t| <= log2(M) (M - 1), in integers, for every (r, t); shift(M - 1, t) = t; the shifts
    do not decrease with r."""
    r, t = np.arange(M)[:, np.newaxis], np.arange(M)[np.newaxis, :]
    s = ffa.ffa_shift(r, t, M)
    assert s.shape == (M, M) and s.dtype == np.int64
    log2 = M.bit_length() - 1
    assert (6 * np.abs(s * (M - 1) - r * t) <= log2 * (M - 1)).all()
    assert (s[M - 1] == np.arange(M)).all() and (s[0] == 0).all() and (s[:, 0] == 0).all()
    assert (np.diff(s, axis=0) >= 0).all()
    assert isinstance(ffa.ffa_shift(M - 1, M - 1, M), int) and ffa.ffa_shift(M - 1, M - 1, M) == M - 1
    # the recursion as the rule states it
    if M > 1:
        h = M // 2
        lower = ffa.ffa_shift(np.arange(h)[:, np.newaxis], t >> 1, h)
        assert (s[:h] == lower).all() and (s[h:] == lower + ((t + 1) >> 1)).all()
    with pytest.raises(ValueError):
        ffa.ffa_shift(0, 0, 3)


def test_scales_and_periods():
    for p, m, K in ((8, 12, 1), (17, 2, 2), (1024, 5, 10), (511, 513, 6), (4, 65536, 2)):
        a = ffa.ffa_scales(p, m, K)
        assert a.dtype == np.float32 and a.shape == (K,)
        for k in range(K):
            w = 2 ** k
            exact = np.sqrt(p / (w * (p - w) * m))
            assert a[k] == np.float32(exact) and abs(float(a[k]) / exact - 1.) < 2. ** -24
            # the correlation with a zero-mean unit-norm top-hat: h = (1 - w / p) on w bins, -w / p elsewhere
            h = np.full(p, -w / p)
            h[:w] += 1.
            assert abs(1. / np.sqrt((h * h).sum() * m) - exact) < 1e-12 * exact
    assert (ffa.SNR, ffa.SHIFT, ffa.WIDTH, ffa.PHASE) == (0, 1, 2, 3)
    assert ffa.ffa_rows(700, 21) == (33, 64) and ffa.ffa_rows(700, 22) == (31, 32) and ffa.ffa_rows(544, 17) == (32, 32)
    assert ffa.ffa_rows(120, 25) == (4, 4) and ffa.ffa_rows(50, 25) == (2, 2)
    assert ffa.ffa_period(31, 102, 6000) == 31 + 102 / 255 and ffa.ffa_period(17, 0, 544) == 17.
    np.testing.assert_array_equal(ffa.ffa_period(17, np.array([0, 31]), 544), [17., 18.])


# -- ties and special values ------------------------------------------------------------------------------
def _one(x, n, periods, K):
    out = ffa.ffa_search_samples(np.asarray(x, np.float32).reshape(-1, 1), n, periods, K)
    return out[0, :, :, 0]


def test_ties_go_to_the_smaller_shift_then_width_then_phase():
    # phase: a pulse train at exactly the base period with two equal peaks: straight in row 0 only, where bins 2
    # and 5 are equal, and the smaller bin wins
    x = np.zeros(64)
    x[2::8] = 1.
    x[5::8] = 1.
    out = _one(x, 64, (8, 9), 1)
    assert out[0, SNR] > 0 and out[0, 1:].tolist() == [0., 0., 2.]
    # shift: one sample in the last row, r = 7 of M = 8: every row t sees it once, at bin (3 - shift(7, t)) mod 8 =
    # (3 - t) mod 8, with the same height, so all eight rows tie and the smallest t wins, at its own bin
    y = np.zeros(64)
    y[8 * 7 + 3] = 2.
    out = _one(y, 64, (8, 9), 1)
    assert out[0, 1:].tolist() == [0., 0., 3.]
    y[8 * 7 + 3] = 0.
    y[8 * 3 + 3] = 2.                                           # r = 3: shift(3, t, 8) = 0 for t = 0, 1 and 1 for t = 2
    assert [ffa.ffa_shift(3, t, 8) for t in range(4)] == [0, 0, 1, 1]
    assert _one(y, 64, (8, 9), 1)[0, 1:].tolist() == [0., 0., 3.]
    # width: p = 10, m = 4: a_1 / a_0 = sqrt(9 / 16), and float32(3) a_0 == float32(4) a_1 as floats.  The profile
    # 3, 1, 0, 0, 0, -4, 0 ... (T = 0, so c_k = 0) in row 0 alone is the same in every row t: S_0 peaks with 3 at bin
    # 0, S_1 with 4 at bin 0, the two S/N are the same float, and the smaller k is kept
    a = ffa.ffa_scales(10, 4, 2)
    assert np.float32(3.) * a[0] == np.float32(4.) * a[1]
    z = np.zeros(40)
    z[0], z[1], z[5] = 3., 1., -4.
    out = _one(z, 40, (10, 11), 2)
    assert out[0].tolist() == [float(np.float32(3.) * a[0]), 0., 0., 0.]
    # ... while S_0 = 2 against S_1 = 3 is decided by the value: the wider one
    z[0], z[5] = 2., -3.
    out = _one(z, 40, (10, 11), 2)
    assert out[0].tolist() == [float(np.float32(3.) * a[1]), 0., 1., 0.]
    # everything equal: the first cell
    assert _one(np.ones(64), 64, (8, 9), 2)[0, 1:].tolist() == [0., 0., 0.]
    assert _one(np.zeros(16), 16, (8, 9), 3)[0].tolist() == [0., 0., 0., 0.]


def test_winner_is_the_first_maximum_of_the_rebuilt_levels():
    """Small integers, so that maxima are shared: the S/N of every (t, k, j) rebuilt by the rule's own steps, and
    the winner is the first maximum in (t, k, j) order."""
    rng = np.random.default_rng(12)
    x = rng.integers(-1, 2, size=(96, 4)).astype(np.float32)
    out = ffa.ffa_search_samples(x, 96, (6, 8), 2)
    shared = 0
    for i, p in enumerate((6, 7)):
        m, M = ffa.ffa_rows(96, p)
        d = np.zeros((M, p, 4), np.float32)
        d[:m] = x[:m * p].reshape(m, p, 4)
        level = ffa.ffa_transform_samples(d)
        total = x[:m * p].astype(np.float64).sum(axis=0)
        a = ffa.ffa_scales(p, m, 2)
        snr = np.empty((M, 2, p, 4), np.float32)
        for k in range(2):
            snr[:, k] = (level - (total * 2. ** k / p).astype(np.float32)) * a[k]
            level = level + np.roll(level, -(1 << k), axis=1)
        for e in range(4):
            col = snr[..., e]
            ties = np.argwhere(col == col.max())
            shared += len(ties) > 1
            assert out[0, i, :, e].tolist() == [col.max()] + ties[0].tolist()
    assert shared


def test_nan_inf_and_zeros():
    n, periods, K = 100, (7, 10), 2
    rng = np.random.default_rng(9)
    x = rng.standard_normal((100, 8)).astype(np.float32)
    clean = ffa.ffa_search_samples(x, n, periods, K)
    y = x.copy()
    y[97, 1] = np.nan          # used by p = 7 (98 samples) only: p = 8 uses 96, p = 9 uses 99 -> 7 and 9
    y[99, 2] = np.inf          # in the dropped tail of every p
    y[50, 3] = np.inf
    y[:, 4] = np.nan
    y[:, 5] = -0.
    y[:, 6] = 0.
    y[10, 7] = -np.inf
    out = ffa.ffa_search_samples(y, n, periods, K)
    assert ffa_cases.same_bits(out[..., 0], clean[..., 0]) and ffa_cases.same_bits(out[..., 2], clean[..., 2])
    # the NaN spoils exactly the periods whose used samples hold it: everything there is NaN, nothing wins
    assert out[0, :, :, 1].tolist()[0] == [-np.inf, 0., 0., 0.] and out[0, 2, :, 1].tolist() == [-np.inf, 0., 0., 0.]
    assert ffa_cases.same_bits(out[0, 1, :, 1], clean[0, 1, :, 1])
    # +inf: T is +inf, so c is +inf and every S/N is NaN or -inf
    assert (out[0, :, SNR, 3] == -np.inf).all()
    assert (out[0, :, :, 4] == np.array([-np.inf, 0., 0., 0.], np.float32)).all()
    # -0: x + (+0) turns the padded sums into +0 only where a padded row is added to -0 first ... whatever the
    # tree gives; T = -0, c = -0, S - c = S + 0 = +0 or -0 - (-0) = +0; times a: +0
    assert (out[0, :, :, 5] == 0.).all() and (out[0, :, :, 6] == 0.).all()
    assert not out[0, :, SNR, 6].view(np.uint32).any()
    # -inf: T = -inf, c = -inf, S - c = +inf or NaN (where S is -inf): +inf wins at the first cell that has it
    assert (out[0, :, SNR, 7] == np.inf).all()
    assert not np.isnan(out).any()


def test_twin_refusals():
    x = np.zeros((100, 2), np.float32)
    with pytest.raises(TypeError):
        ffa.ffa_search_samples(x.astype(np.float64), 100, (8, 9), 1)
    with pytest.raises(TypeError):
        ffa.ffa_search_samples(x.astype(np.complex64), 100, (8, 9), 1)
    for n, periods, K in ((100, (3, 9), 1), (100, (8, 8), 1), (100, (9, 8), 1), (100, (8, 1026), 1), (100, (8, 52), 1),
                          (101, (8, 9), 1), (100, (8, 9), 0), (100, (8, 9), 11), (100, (8, 9), 5), (100, (8,), 1),
                          (4 * 65537, (4, 5), 1)):
        with pytest.raises(ValueError):
            ffa.ffa_search_samples(np.zeros((max(n, 100), 2), np.float32) if n != 101 else x, n, periods, K)
    assert ffa.ffa_search_samples(x, 100, (8, 51), 1).shape == (1, 43, 4, 2)       # n // 50 = 2
    assert ffa.ffa_search_samples(x, 100, (9, 10), 4).shape == (1, 1, 4, 2)        # 2^3 = 8 is shorter than 9
    with pytest.raises(ValueError):
        ffa.ffa_search_samples(x, 100, (8, 9), 4)


# -- candidates and the ladder --------------------------------------------------------------------------------
def _best(snr, shift=0, k=0, j=0):
    snr = np.asarray(snr, np.float32)
    best = np.zeros((snr.shape[0], 4, snr.shape[1]), np.float32)
    best[:, SNR], best[:, SHIFT], best[:, WIDTH], best[:, PHASE] = snr, shift, k, j
    return best


def test_candidates_on_a_hand_made_plane():
    snr = np.zeros((5, 6))
    snr[0, 5] = 9.                       # a corner
    snr[2, 1:4] = 8.                     # a plateau: the first in raster order
    snr[3, 2] = 8.
    snr[4, 5] = 7.                       # exactly the threshold
    snr[4, 0] = 6.999
    shift = np.arange(30).reshape(5, 6)
    c = ffa.ffa_candidates(_best(snr, shift, 2, 3), 1000, (20, 25), 7., 100.)
    assert c.dtype == ffa.CANDIDATE_DTYPE
    assert c.dtype.names == ('period', 'bins', 'shift', 'trial', 'width', 'phase', 'snr')
    assert c['snr'].tolist() == [9., 8., 7.] and c['bins'].tolist() == [20, 22, 24] and c['trial'].tolist() == [5, 1, 5]
    assert c['shift'].tolist() == [5, 13, 29] and (c['width'] == 4).all() and (c['phase'] == 3).all()
    for row in c:
        M = ffa.ffa_rows(1000, row['bins'])[1]
        assert row['period'] == (row['bins'] + row['shift'] / (M - 1)) / 100.
    assert len(ffa.ffa_candidates(_best(snr), 1000, (20, 25), 6.999)) == 4
    assert len(ffa.ffa_candidates(_best(snr), 1000, (20, 25), 9.5)) == 0
    c = ffa.ffa_candidates(_best(np.full((3, 3), 4.)), 1000, (20, 23), 4.)
    assert len(c) == 1 and (c['bins'][0], c['trial'][0]) == (20, 0)
    with pytest.raises(ValueError):
        ffa.ffa_candidates(np.zeros((4, 4, 3), np.float32), 1000, (20, 25), 1.)
    with pytest.raises(ValueError):
        ffa.ffa_candidates(np.zeros((5, 3, 3), np.float32), 1000, (20, 25), 1.)


def test_planted_pulsar_in_the_twin():
    c = ffa_cases.PLANTED
    out = ffa_cases.planted_expected()
    assert out.shape == (1, 6, 4, 5)
    snr, shift, k, j = out[0, 31 - 29, :, c['column']]
    assert abs(shift - 102) <= 3 and snr > 18.9 / 2 and 2 ** k == c['width']
    others = out[0, :, SNR].copy()
    others[:, c['column']] = 0.
    assert others.max() < 5.5 and out[0, :, SNR].argmax() == (31 - 29) * 5 + c['column']
    cands = ffa.ffa_candidates(out[0], c['n'], c['periods'], 8., RATE)
    assert len(cands) == 1 and cands['bins'][0] == 31 and cands['trial'][0] == c['column']
    assert abs(cands['period'][0] * RATE - c['period']) < 3 / 255 + 1e-9


@pytest.mark.parametrize('lo, hi, rate, bins', [(0.1, 5., 1e4, 256), (0.001, 0.1, 1e5, 64), (0.5, 0.6, 1e3, 512),
                                                (0.0123, 31.7, 65536., 100), (4e-4, 1e-3, 1e4, 256)])
def test_plan_covers_the_periods_without_a_gap(lo, hi, rate, bins):
    steps = ffa.ffa_plan(lo, hi, rate, bins)
    end = None
    for factor, p_lo, p_hi in steps:
        assert isinstance(factor, int) and factor >= 1 and 4 <= p_lo < p_hi <= 1025 and p_hi <= 2 * p_lo
        assert factor == 1 or p_lo >= bins
        if end is not None:
            assert p_lo * factor <= end                        # starts at or below where the one before ends
            assert p_hi * factor > end                         # ... and gets further
        end = p_hi * factor
    assert steps[0][1] * steps[0][0] <= lo * rate and end >= hi * rate
    assert (steps[-1][2] - 1) * steps[-1][0] < hi * rate or steps[-1][2] == steps[-1][1] + 1      # (no step too many)
    for bad in ((0., 1., 1e4, 256), (1., 1., 1e4, 256), (2., 1., 1e4, 256), (1e-4, 1., 1e4, 256), (0.1, 1., 1e4, 3),
                (0.1, 1., 1e4, 513)):
        with pytest.raises(ValueError):
            ffa.ffa_plan(*bad)


# -- construction -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stream_surface(case):
    sh = ffa_cases.stream(case)
    p_lo, p_hi = case.periods
    fs = bt.FFASearch(sh, case.n, case.periods, case.K)
    assert fs.shape == (case.N // case.n, p_hi - p_lo, 4) + case.s and fs.dtype == np.float32
    assert fs.sample_rate == RATE / case.n and fs.samples_per_frame == 1
    assert abs(fs.start_time - bt.Time(T0)) < 1e-9
    assert fs.n == case.n and fs.periods == case.periods and fs.n_widths == case.K
    assert fs.frequency == 600e6 and fs.sideband == 1
    assert bt.FFASearch(sh, case.n, case.periods, case.K, samples_per_frame=2 if case.N >= 2 * case.n else 1)
    text = repr(fs)
    assert text.startswith('FFASearch(ih') and 'ih: HostStream' in text
    # what the uploader is told: the one block of a frame
    assert fs._input_span(0, 1) == (sh, 0, case.n)
    nb = case.N // case.n
    assert fs._input_span(nb - 1, nb) == (sh, (nb - 1) * case.n, case.n)
    assert fs.ffa_budget == 1 << 29 and fs._chunks() == [(0, int(np.prod(case.s)), p_lo, p_hi)]
    fs.close()
    assert fs.closed
    if 2 ** 5 < p_lo:
        assert bt.FFASearch(sh, case.n, case.periods).n_widths == 6


def test_chunks_follow_the_budget():
    """The budget holds the block, then per column the scratch (a float64 per segment of 32 samples and one more, the
    10 c_k and two buffers of the largest M p) and
    per column and base period 16 bytes of output: the columns are cut first, then the base periods."""
    case = ffa_cases.by_name('ragged')
    fs = bt.FFASearch(ffa_cases.stream(case), case.n, case.periods, case.K)
    block = case.n * 67 * 4
    column = (2 * (case.n // 32 + 1) + 10 + 2 * max(ffa.ffa_rows(case.n, p)[1] * p for p in range(16, 23))) * 4
    assert column == (2 * 22 + 10 + 2 * 64 * 21) * 4
    # room for 20 columns of one base period, and no more
    fs.ffa_budget = block + 20 * (column + 16) + 15
    chunks = fs._chunks()
    assert chunks[:8] == [(0, 20, p, p + 1) for p in range(16, 23)] + [(20, 20, 16, 17)]
    # (the last 7 columns leave room for every base period at once)
    assert chunks[-1] == (60, 7, 16, 23) and len(chunks) == 3 * 7 + 1
    # four base periods of 19 columns fit where 20 columns of one do not
    fs.ffa_budget = block + 19 * column + 19 * 16 * 4 + 100
    assert fs._chunks()[:3] == [(0, 19, 16, 20), (0, 19, 20, 23), (19, 19, 16, 20)]
    fs.ffa_budget = 1
    assert fs._chunks() == [(e, 1, p, p + 1) for e in range(67) for p in range(16, 23)]


def test_metadata_of_a_plane_without_a_sideband_is_passed_on():
    x = np.zeros((300, 4), np.float32)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(sh, [0., .1, .2])
    assert plane.shape[1:] == (3,)
    fs = bt.FFASearch(bt.Standardize(plane, 50), 100, (10, 14), 3)
    assert fs.frequency == plane.frequency and fs.shape == (plane.shape[0] // 50 * 50 // 100, 4, 4, 3)
    with pytest.raises(AttributeError):
        fs.sideband
    pol = np.array(['X', 'Y', 'X', 'Y'])
    ph = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=np.linspace(4e8, 8e8, 4),
                       sideband=np.array([1, -1, 1, -1]), polarization=pol)
    fs = bt.FFASearch(ph, 100, (10, 12), 2)
    np.testing.assert_array_equal(np.broadcast_to(fs.frequency, (2, 4, 4))[1, 2], np.linspace(4e8, 8e8, 4))
    np.testing.assert_array_equal(np.broadcast_to(fs.sideband, (2, 4, 4))[0, 1], [1, -1, 1, -1])
    np.testing.assert_array_equal(np.broadcast_to(fs.polarization, (2, 4, 4))[0, 0], pol)


def test_what_is_refused():
    x = np.zeros((100, 3), np.float32)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False)
    z = bt.HostStream(x.astype(np.complex64), bt.Time(T0), RATE, pin=False)
    f64 = bt.HostStream(x.astype(np.float64), bt.Time(T0), RATE, pin=False)
    with pytest.raises(TypeError, match='Square'):
        bt.FFASearch(z, 100, (8, 9), 1)
    with pytest.raises(TypeError, match='float32'):
        bt.FFASearch(f64, 100, (8, 9), 1)
    with pytest.raises(ValueError, match='less than one block'):
        bt.FFASearch(sh, 101, (8, 9), 1)
    bt.FFASearch(sh, 100, (8, 9), 1)
    for periods in ((3, 9), (8, 8), (9, 8), (8, 1026)):
        with pytest.raises(ValueError, match='p_lo'):
            bt.FFASearch(sh, 100, periods, 1)
    with pytest.raises(ValueError, match='two rows'):
        bt.FFASearch(sh, 100, (8, 52), 1)
    bt.FFASearch(sh, 100, (8, 51), 1)
    big = bt.HostStream(np.zeros((4 * 65537, 1), np.float32), bt.Time(T0), RATE, pin=False)
    with pytest.raises(ValueError, match='65536 rows'):
        bt.FFASearch(big, 4 * 65537, (4, 5), 1)
    bt.FFASearch(big, 4 * 65536 + 3, (4, 5), 1)
    for k in (0, 11, -1):
        with pytest.raises(ValueError, match='n_widths'):
            bt.FFASearch(sh, 100, (8, 9), k)
    with pytest.raises(ValueError, match='widest'):
        bt.FFASearch(sh, 100, (8, 9), 5)
    bt.FFASearch(sh, 100, (9, 10), 4)
    with pytest.raises(ValueError, match='periods'):
        bt.FFASearch(sh, 100, 8, 1)
    with pytest.raises(TypeError):
        bt.FFASearch(sh, 100.5, (8, 9), 1)
    assert (hip.FFA_MIN_P, hip.FFA_MAX_P, hip.FFA_MAX_ROWS, hip.FFA_MAX_WIDTHS) == (4, 1025, 65536, 10)


def test_library_exports_the_search():
    lib = hip.lib()
    assert lib.bbt_version() >= 169
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_ffa_plan_create', 'bbt_ffa_plan_destroy', 'bbt_ffa_plan_info', 'bbt_ffa_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'ffa_geo.hpp')).read()
    for name, value in (('MIN_P', hip.FFA_MIN_P), ('MAX_P', hip.FFA_MAX_P), ('MAX_ROWS', hip.FFA_MAX_ROWS),
                        ('MAX_WIDTHS', hip.FFA_MAX_WIDTHS), ('SEG', ffa.SEGMENT)):
        assert f'#define BBT_FFA_{name} {value} ' in geo or f'#define BBT_FFA_{name} {value}\n' in geo
    assert f'#define BBT_FFA_MAX_LANE (1 << 30)' in geo and hip.FFA_MAX_LANE == 1 << 30
    assert all(name in bt.ffa.__all__ and hasattr(bt, name) for name in
               ('FFASearch', 'ffa_search_samples', 'ffa_transform_samples', 'ffa_shift', 'ffa_scales', 'ffa_period',
                'ffa_candidates', 'ffa_plan'))
    info = hip.ffa_info()
    assert (info['fuse'], info['width']) == (2, 16) and info['scratch_bytes'] == 0
    # the library's scales and rows are the twin's (no device needed to make a plan and ask)
    for n, periods, K in ((700, (16, 23), 3), (5200, (1020, 1025), 10), (262144, (256, 512), 6)):
        plan = hip.FfaPlan(n, periods, K, 3)
        for p in (periods[0], periods[1] - 1):
            info = plan.info(p)
            m, M = ffa.ffa_rows(n, p)
            assert (info['m'], info['M']) == (m, M)
            want = np.zeros(10, np.float32)
            want[:K] = ffa.ffa_scales(p, m, K)
            assert info['scales'].view(np.uint32).tolist() == want.view(np.uint32).tolist()
        assert info['column_floats'] == 2 * (n // 32 + 1) + 10 + 2 * max(ffa.ffa_rows(n, p)[1] * p for p in range(*periods))
        with pytest.raises(hip.HipError, match='period'):
            plan.info(periods[1])
        plan.close()
    for args, word in (((100, (3, 9), 1, 1), 'p_lo'), ((100, (8, 52), 1, 1), 'two rows'), ((100, (8, 9), 11, 1), 'n_widths'),
                       ((100, (8, 9), 5, 1), 'widest'), ((100, (8, 9), 1, 0), 'elements'),
                       ((4 * 65537, (4, 5), 1, 1), '65536 rows')):
        with pytest.raises(hip.HipError, match=word):
            hip.FfaPlan(*args)


# -- the tiling, on the host ----------------------------------------------------------------------------------
def _geo_shapes():
    """Ten numbers each: every shared case at its first and last base period and where M changes, under every
    tiling the tests walk, whole and cut into the column chunks the tests make; the limits; launches of more
    than 2^31 values."""
    shapes = []
    for case in CASES:
        e = int(np.prod(case.s, dtype=int))
        p_lo, p_hi = case.periods
        periods = sorted({p_lo, p_hi - 1} | {p for p in range(p_lo + 1, p_hi)
                                            if ffa.ffa_rows(case.n, p)[1] != ffa.ffa_rows(case.n, p - 1)[1]})
        for fuse, width in [(0, 0)] + ffa_cases.TILINGS:
            for p in periods:
                shapes.append((case.n, p_lo, p_hi, p, case.K, e, 0, e, fuse, width))
                if e > 2:
                    shapes.append((case.n, p_lo, p_hi, p, case.K, e, e - 2, 2, fuse, width))
                    shapes.append((case.n, p_lo, p_hi, p, case.K, e, 1, 1, fuse, width))
    shapes += [(8, 4, 5, 4, 1, 1, 0, 1, 0, 0), (2048, 1024, 1025, 1024, 10, 1, 0, 1, 3, 4),
               (4 * 65536 + 3, 4, 5, 4, 2, 7, 3, 4, 3, 32), (65536 * 4, 4, 8, 7, 2, 3, 0, 3, 1, 4),
               # more than 2^31 values in a buffer; the widest lane
               (1 << 18, 256, 512, 511, 6, 20000, 100, 16000, 2, 16), (1 << 20, 256, 512, 256, 6, 4096, 0, 4096, 3, 32),
               (2048, 1000, 1025, 1024, 10, 2000000, 7, 1048575, 0, 0)]
    return shapes


def test_kernel_tiling_on_the_host(tmp_path):
    """Every output row of every pass written once, every read inside the block or the buffer, the fused
    rotations composing to the closed-form shifts, every (row, column) of the S/N pass held once inside the
    LDS buffer, the partial winners inside the spare buffer, the result cells inside the result: the program
    exits non-zero otherwise, and the sanitizers abort it on a wild index or an overflow of its own."""
    exe = compile_check('ffa_geo_check', tmp_path)
    shapes = _geo_shapes()
    plans = run_check(exe, shapes)
    for shape, g in zip(shapes, plans):
        assert g.get('walk') == 0, (shape, g)
        n, p_lo, p_hi, p, K, pitch, e0, ne, fuse, width = shape
        m, M = ffa.ffa_rows(n, p)
        assert (g['m'], g['M'], 1 << g['L']) == (m, M, M) and g['lane'] == p * ne and g['buf'] == M * p * ne
        assert g['fuse'] == (fuse or 2) and g['n_pass'] == -(-g['L'] // g['fuse'])
        assert g['ex'] <= (width or 16) and g['ex'] * p <= 8192 and (g['ex'] == (width or 16) or 2 * g['ex'] * p > 8192)
        assert g['nr'] == min(M, 8192 // (p * g['ex'])) and g['n_et'] == -(-ne // g['ex']) and g['n_rg'] == -(-M // g['nr'])
        assert g['scales'] == ffa.ffa_scales(p, m, K).view(np.uint32).tolist()
    big = [g for g in plans if g['buf'] > 2 ** 31]
    assert len(big) >= 2
    # what the library refuses
    bad = run_raw(exe, '100 3 9 8 1 3 0 3 0 0  100 8 52 8 1 3 0 3 0 0  100 8 9 8 11 3 0 3 0 0  100 8 9 8 5 3 0 3 0 0 '
                       '100 8 9 9 1 3 0 3 0 0  100 8 9 8 1 3 1 3 0 0  100 8 9 8 1 3 0 0 0 0  100 8 9 8 1 3 -1 2 0 0 '
                       '100 8 9 8 1 3 0 3 4 0  100 8 9 8 1 3 0 3 0 5  2048 1000 1025 1024 1 2000000 0 1048576 0 0 '
                       '262148 4 5 4 1 3 0 3 0 0  262144 256 512 511 6 20000 100 16500 2 16')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 13
    assert 'p_lo' in errors[0] and 'two rows' in errors[1] and 'n_widths' in errors[2] and 'widest' in errors[3]
    assert "plan's" in errors[4] and all('columns' in e for e in errors[5:8]) and 'stages' in errors[8]
    assert 'width' in errors[9] and 'too many columns' in errors[10] and '65536 rows' in errors[11]
    # 512 rows of 32936 workgroups: more than 2^24 of them in the widest fold pass
    assert 'too many tiles' in errors[12]
