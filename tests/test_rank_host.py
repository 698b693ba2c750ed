"""The block median / MAD rule on the host: the NumPy twins (`search.block_median_mad_samples`,
`search.robust_standardize_samples`, `periodicity.median_whiten_samples`) against independent
restatements, the planted columns, `median_ratio`, what the robust statistics buy on a bright pulse,
the surface of `RobustStandardize` and `MedianWhiten`, the library's exports, and the tiling and the
digit descent of the kernels walked by a sanitized host program.  No GPU."""
import json
import math
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity, search

import rank_cases
from rank_cases import RATE, T0, same_bits
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


def _blocks(x, n):
    nb = x.shape[0] // n
    return x[:nb * n].reshape((nb, n) + x.shape[1:])


# -- the twins are the rule -----------------------------------------------------------------------------
@pytest.mark.parametrize('n', rank_cases.BLOCKS)
def test_twins_are_the_rule_on_noise(n):
    x = rank_cases.noise()
    med, mad, z = rank_cases.expected('noise', n)
    xb = _blocks(x, n)
    assert med.dtype == mad.dtype == z.dtype == np.float32 and med.shape == mad.shape == (x.shape[0] // n, x.shape[1])
    # the median: numpy's own, of the float64 copy, rounded once
    assert same_bits(med, np.median(xb.astype(np.float64), axis=1).astype(np.float32))
    # the MAD: |x - med| in float32, its two middle values by partition, averaged in float64
    d = np.abs(xb - med[:, np.newaxis])
    assert d.dtype == np.float32
    part = np.partition(d, ((n - 1) // 2, n // 2), axis=1)
    want = ((part[:, (n - 1) // 2].astype(np.float64) + part[:, n // 2].astype(np.float64)) * 0.5).astype(np.float32)
    assert same_bits(mad, want) and (mad > 0).all()
    # z from them, with the three stated operations
    r32 = (1. / (mad.astype(np.float64) * 1.482602218505602)).astype(np.float32)
    rebuilt = (xb - med[:, np.newaxis]) * r32[:, np.newaxis]
    assert rebuilt.dtype == np.float32 and same_bits(z, rebuilt.reshape(z.shape))
    assert z.shape == (x.shape[0] // n * n, x.shape[1])


def test_keys_order_the_values():
    values = np.array([-np.inf, -3e38, -1., -1e-45, -0., 0., 1e-45, 1., 3e38, np.inf], np.float32)
    keys = search._rank_keys(values)
    assert keys.dtype == np.uint32 and (np.diff(keys.astype(np.int64)) > 0).all()
    assert int(keys[5]) - int(keys[4]) == 1                                  # -0 just before +0
    assert same_bits(search._rank_values(keys), values)
    bits = np.random.default_rng(3).integers(0, 2 ** 32, 10000, dtype=np.uint64).astype(np.uint32)
    assert (search._rank_values(search._rank_keys(bits.view(np.float32))).view(np.uint32) == bits).all()


@pytest.mark.parametrize('n', rank_cases.PLANT_BLOCKS)
def test_planted_columns(n):
    c = rank_cases
    x = c.planted(n)
    med, mad, z = c.expected('planted', n)
    zb, xb = _blocks(z, n), _blocks(x, n)
    assert med.shape == (3, c.PLANT_COLUMNS) and z.shape == (3 * n, c.PLANT_COLUMNS)

    def zeros(col, blocks=slice(None)):
        return not zb[blocks, :, col].view(np.uint32).any()
    # constant, all zero, all -0: mad = 0, a block of +0
    assert (med[:, c.CONST] == 2.5).all() and not mad[:, c.CONST].any() and zeros(c.CONST)
    assert not med[:, c.ZERO].view(np.uint32).any() and zeros(c.ZERO)
    assert (med[:, c.MINUS_ZERO].view(np.uint32) == 0x80000000).all() and zeros(c.MINUS_ZERO)
    # which zero is selected: x - med of the zeros of the column tells
    for col, minus in ((c.MED_PLUS_ZERO, False), (c.MED_MINUS_ZERO, True)):
        want = 0x80000000 if minus else 0
        assert (med[:, col].view(np.uint32) == want).all()
        diff = xb[:, :, col] - med[:, np.newaxis, col]
        is_zero = xb[:, :, col] == 0
        minus_zero = is_zero & np.signbit(xb[:, :, col])
        assert is_zero.sum() == 9 and minus_zero.sum() == (6 if minus else 3)
        if minus:               # x - (-0) = x + 0: +0 for either zero
            assert not np.signbit(diff[is_zero]).any()
        else:                   # x - (+0): -0 stays -0
            assert np.signbit(diff[minus_zero]).all() and not np.signbit(diff[is_zero & ~minus_zero]).any()
        assert (mad[:, col] > 0).all() and not zeros(col)
        # ... and z keeps that sign: a zero times a positive float32(r)
        assert same_bits(zb[:, :, col][is_zero], diff[is_zero])
    # a NaN, an Inf: the block is flagged, the others are not
    assert np.isnan(med[1, c.NAN]) and np.isnan(mad[1, c.NAN]) and zeros(c.NAN, 1)
    assert np.isfinite(med[[0, 2], c.NAN]).all() and not zeros(c.NAN, 0) and not zeros(c.NAN, 2)
    assert np.isnan(med[[0, 2], c.INF]).all() and zeros(c.INF, 0) and zeros(c.INF, 2) and not zeros(c.INF, 1)
    # more than half equal: mad = 0 and +0; exactly half equal (even n): not flagged
    assert (med[:, c.MOST_EQUAL] == 7.).all() and not mad[:, c.MOST_EQUAL].any() and zeros(c.MOST_EQUAL)
    assert (mad[:, c.HALF_EQUAL] > 0).all() and not zeros(c.HALF_EQUAL)
    if n % 2 == 0:
        assert ((xb[:, :, c.HALF_EQUAL] == 7.).sum(axis=1) == n // 2).all() and (med[:, c.HALF_EQUAL] > 7.).all()
    # ties, the last mantissa bit, denormals, the largest float: the twin is the sorted float64 rule
    for col in (c.INTS, c.LAST_BIT, c.DENORMAL, c.HUGE, c.HALF_EQUAL):
        s = np.sort(xb[:, :, col].astype(np.float64), axis=1)
        with np.errstate(over='ignore'):
            assert same_bits(med[:, col], ((s[:, (n - 1) // 2] + s[:, n // 2]) * 0.5).astype(np.float32))
    assert (med[:, c.HUGE].view(np.uint32) == c.HUGE_BITS).all() and not mad[:, c.HUGE].any() and zeros(c.HUGE)
    assert (xb[:, :, c.DENORMAL] < 0).any() and (np.abs(xb[:, :, c.DENORMAL]) < 1e-40).any()
    assert np.isfinite(z).all()
    # two values of the largest float, alone: no overflow
    two = np.full((2, 1), c.HUGE_BITS, np.uint32).view(np.float32)
    m2, d2 = search.block_median_mad_samples(two, 2)
    assert m2.view(np.uint32).tolist() == [[c.HUGE_BITS]] and not d2.any()


@pytest.mark.parametrize('m, skip', rank_cases.WH_CUTS)
def test_median_whiten_twin(m, skip):
    c = rank_cases
    x = c.wh_data()
    z = c.wh_expected(m, skip)
    assert z.dtype == np.float32 and z.shape == x.shape and not z[:, :skip].view(np.uint32).any()
    nbin = x.shape[1]
    for j0 in range(skip, nbin, m):
        j1 = min(j0 + m, nbin)
        block = x[:, j0:j1].astype(np.float64)
        with np.errstate(all='ignore'):
            med = np.median(block, axis=1).astype(np.float32)
            r32 = (1. / (med.astype(np.float64) / c.WH_RATIO)).astype(np.float32)
            want = x[:, j0:j1] * r32[:, np.newaxis]
        bad = ~np.isfinite(block).all(axis=1) | ~(med > 0)
        want[np.broadcast_to(bad[:, np.newaxis], want.shape)] = 0.
        assert same_bits(z[:, j0:j1], want)
    assert (nbin - skip) % m == (1 if m == 60 else (nbin - skip) - (nbin - skip) // m * m)
    # the planted columns: all zero; the NaN's and the Inf's block +0, their neighbours not
    assert not z[:, :, c.WH_ZERO].view(np.uint32).any()
    b = skip + (707 - skip) // m * m
    assert not z[1, b:b + m, c.WH_NAN].any() and z[1, b - 1, c.WH_NAN] > 0 and z[0, 707, c.WH_NAN] > 0
    last = skip + (nbin - 1 - skip) // m * m
    assert not z[2, last:, c.WH_INF].any() and z[2, last - 1, c.WH_INF] > 0
    assert np.isfinite(z).all()
    # noise comes out at unit mean: the median of a block is ratio times the mean, to the scatter of m values
    # (the data are exponential powers, ratio log 2; the cases whiten them with the ratio of 4 averaged powers)
    if m == 61 and skip == 1:
        unit = periodicity.median_whiten_samples(x, m, skip)
        assert abs(unit[:, skip:, 3:].mean() - 1.) < 0.05
        assert abs(z[:, skip:, 3:].mean() - c.WH_RATIO / math.log(2)) < 0.07
    # the statistics, block by block
    med, mad = c.spectra_stats(x, m, skip)
    assert med.shape == mad.shape == (3, -(-(nbin - skip) // m), 7)


def test_median_ratio():
    assert periodicity.median_ratio() == periodicity.median_ratio(1) == math.log(2) == periodicity.LN2
    for k, want in ((2, 0.8391734950083302), (8, 0.9586561803126001), (64, 0.994796516744751)):
        assert abs(periodicity.median_ratio(k) - want) < 1e-12
    assert periodicity.median_ratio(2.) == periodicity.median_ratio(2) == periodicity.median_ratio(np.int64(2))
    for bad in (1.5, 0, -3, 2.5, np.nan, periodicity.MAX_AVERAGED + 1, 1e30):
        with pytest.raises(ValueError, match='ratio='):
            periodicity.median_ratio(bad)


def test_median_ratio_of_long_stacks():
    """Beyond k = 709 the unscaled sum of x^j / j! overflows float64: the terms are formed in log space.  The
    references are the roots of the regularised incomplete gamma function to 20 digits; the series is the
    asymptotic expansion of the gamma median, k - 1/3 + 8 / (405 k) + 184 / (25515 k^2) + 2248 / (3444525 k^3)."""
    assert periodicity.MAX_AVERAGED == hip.LSPEC_MAX_STACK == 1 << 20
    for k, want in ((700, None), (709, None), (710, None), (720, None), (1024, 0.99967449801139462823),
                    (4096, 0.99991862096914730858), (1 << 20, 0.99999968210857916325)):
        got = periodicity.median_ratio(k)
        series = (k - 1. / 3. + 8. / (405. * k) + 184. / (25515. * k ** 2) + 2248. / (3444525. * k ** 3)) / k
        print(k, repr(got), got - series)
        assert abs(got - series) < 1e-12
        assert want is None or abs(got - want) < 1e-12
        assert 1. - 1. / (3. * k) - 1e-12 < got < 1.                  # (the gamma median lies in (k - 1/3, k))
    ratios = [periodicity.median_ratio(k) for k in (2, 8, 64, 512, 700, 720, 1024, 4096, 65536)]
    assert (np.diff(ratios) > 0).all()                                      # towards 1, monotonically
    sh = rank_cases.stream(rank_cases.wh_data())
    assert bt.MedianWhiten(sh, 50, averaged=1024).ratio == periodicity.median_ratio(1024)
    with pytest.raises(ValueError, match='ratio='):
        bt.MedianWhiten(sh, 50, averaged=(1 << 20) + 1)


def test_twin_refusals():
    x = np.ones((10, 3), np.float32)
    for fn in (search.block_median_mad_samples, search.robust_standardize_samples):
        for n in (1, 65537, 0):
            with pytest.raises(ValueError, match='block'):
                fn(x, n)
        with pytest.raises(TypeError):
            fn(x.astype(np.float64), 2)
        with pytest.raises(TypeError):
            fn(x, 2.5)
    assert search.robust_standardize_samples(x, 4).shape == (8, 3)
    assert search.block_median_mad_samples(x, 11)[0].shape == (0, 3)
    s = np.ones((2, 10, 3), np.float32)
    for m in (1, 65537):
        with pytest.raises(ValueError, match='whitening block'):
            periodicity.median_whiten_samples(s, m)
    for skip in (-1, 10):
        with pytest.raises(ValueError, match='skip'):
            periodicity.median_whiten_samples(s, 4, skip)
    for ratio in (0., -1., np.inf, np.nan):
        with pytest.raises(ValueError, match='ratio'):
            periodicity.median_whiten_samples(s, 4, 1, ratio)
    with pytest.raises(TypeError):
        periodicity.median_whiten_samples(s[0, :, 0], 4)
    z = periodicity.median_whiten_samples(s, 4)
    assert not z[:, 0].any() and same_bits(z[:, 1:], np.full((2, 9, 3), np.float32(1.) * np.float32(math.log(2)), np.float32))


# -- what it buys -------------------------------------------------------------------------------------------
def test_a_bright_pulse_does_not_lower_its_own_snr():
    x, clean = rank_cases.pulse_plane()
    med, mad = search.block_median_mad_samples(x, 1024)
    scale = 1.4826 * mad[0].astype(np.float64)
    true = clean.astype(np.float64).std(axis=0)
    ratio = scale / true
    print('robust scale / pulse-free scale:', ratio.min(), ratio.max())
    assert (ratio < 1.2).all() and (ratio > 1 / 1.2).all()
    plain = x.astype(np.float64).std(axis=0)
    print('plain standard deviation:', plain.min(), plain.max())
    assert (plain > 10.).all()
    robust = search.boxcar_search_samples(search.robust_standardize_samples(x, 1024), 1024, 8)
    naive = search.boxcar_search_samples(search.standardize_samples(x, 1024), 1024, 8)
    # the width-64 boxcar on the pulse
    zr = search.robust_standardize_samples(x, 1024)[400:464].astype(np.float64).sum(axis=0) / 8.
    zs = search.standardize_samples(x, 1024)[400:464].astype(np.float64).sum(axis=0) / 8.
    print('width-64 S/N: robust', zr.min(), 'plain', zs.max())
    assert (zr > 5. * zs).all() and zr.min() > 300. and zs.max() < 35.
    # and the search finds it there, at that width
    assert (robust[0, search.OFFSET] == 400.).all() and (robust[0, search.WIDTH] == 6.).all()
    assert (robust[0, search.SNR] > 5. * naive[0, search.SNR]).all()


# -- the tasks ------------------------------------------------------------------------------------------------
def test_robust_standardize_surface():
    x = rank_cases.noise()
    sh = rank_cases.stream(x, samples_per_frame=100)
    for n in rank_cases.BLOCKS:
        rs = bt.RobustStandardize(sh, n)
        length = x.shape[0] // n * n
        assert rs.shape == (length, 67) and rs.dtype == np.float32 and rs.n == n
        assert rs.sample_rate == RATE and abs(rs.start_time - bt.Time(T0)) < 1e-9
        assert rs.samples_per_frame == min(-(-100 // n) * n, length)
        assert repr(rs).startswith(f'RobustStandardize(ih, n={n})')
    rs = bt.RobustStandardize(sh, 50, samples_per_frame=150)
    assert rs.samples_per_frame == 150 and 'samples_per_frame=150' in repr(rs)
    assert rs._input_span(0, 1) == (sh, 0, 150) and rs._input_span(1, 3) == (sh, 150, 300)
    assert bt.RobustStandardize.robust_budget == 1 << 29
    rs.robust_budget = 3 * 50 * 67 * 4
    assert rs._chunk_size() == 150 and rs._input_span(0, 1) == (sh, 0, 150) and rs._input_span(0, 2) is None
    rs.robust_budget = 1
    assert rs._chunk_size() == 50
    flat = bt.RobustStandardize(rank_cases.stream(x[:, 0].copy()), 64)
    assert flat.shape == (2048,)


def test_median_whiten_surface():
    x = rank_cases.wh_data()
    sh = rank_cases.stream(x, samples_per_frame=2)
    for m, skip in rank_cases.WH_CUTS:
        wh = bt.MedianWhiten(sh, m, skip)
        assert wh.shape == x.shape and wh.dtype == np.float32 and (wh.m, wh.skip) == (m, skip)
        assert wh.sample_rate == RATE and abs(wh.start_time - bt.Time(T0)) < 1e-9
        assert wh.samples_per_frame == 2 and wh.ratio == math.log(2)
        assert repr(wh).startswith('MedianWhiten(ih') and 'ratio' not in repr(wh) and 'averaged' not in repr(wh)
    wh = bt.MedianWhiten(sh, 50, averaged=8, samples_per_frame=3)
    assert wh.skip == 1 and wh.ratio == periodicity.median_ratio(8) and wh.samples_per_frame == 3
    assert 'averaged=8' in repr(wh) and 'ratio' not in repr(wh)
    assert wh._input_span(0, 1) == (sh, 0, 3)
    wh.whiten_budget = 2 * 1501 * 7 * 4
    assert wh._chunk_size() == 2 and wh._input_span(0, 1) is None
    wh = bt.MedianWhiten(sh, 50, 0, ratio=0.9)
    assert wh.ratio == 0.9 and 'ratio=0.9' in repr(wh)
    for kwargs in (dict(averaged=2, ratio=0.8), dict(averaged=1.5), dict(averaged=0), dict(ratio=0.), dict(ratio=-1.),
                   dict(ratio=np.inf), dict(ratio=np.nan)):
        with pytest.raises(ValueError):
            bt.MedianWhiten(sh, 50, **kwargs)
    bt.MedianWhiten(sh, 50, averaged=1, ratio=0.7)                     # (the default averaged says nothing)


def test_metadata():
    x = np.ones((4, 30, 3), np.float32)
    per_bin = np.linspace(4e8, 8e8, 30).reshape(30, 1)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=per_bin, sideband=1,
                       polarization=np.array(['X', 'Y', 'X']))
    for task in (bt.MedianWhiten(sh, 8), bt.RobustStandardize(sh, 2)):
        np.testing.assert_array_equal(task.frequency, sh.frequency)
        assert task.sideband == 1
        np.testing.assert_array_equal(task.polarization, sh.polarization)
    # a lone frequency, as the plane of DMTrials has
    src = bt.HostStream(np.zeros((300, 4), np.float32), bt.Time(T0), 1e4, pin=False,
                        frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(src, [0., .1, .2])
    for task in (bt.MedianWhiten(plane, 2, 0), bt.RobustStandardize(plane, 16)):
        assert task.frequency == plane.frequency
        with pytest.raises(AttributeError):
            task.sideband
    rs = bt.RobustStandardize(plane, 16)
    assert rs.shape == (plane.shape[0] // 16 * 16, 3) and abs(rs.start_time - plane.start_time) < 1e-12
    # the searches take them as they are
    assert bt.BoxcarSearch(rs, 16, 3).shape == (rs.shape[0] // 16, 3, 3)
    sp = bt.fluctuation_spectra(plane, 64, 2)
    hs = bt.HarmonicSearch(bt.MedianWhiten(sp, 8, averaged=2), 8, 3, averaged=2)
    assert hs.shape == (sp.shape[0], 5, 3, 3)


def test_what_is_refused():
    x = np.ones((40, 10, 3), np.float32)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False)
    z = bt.HostStream(x.astype(np.complex64), bt.Time(T0), RATE, pin=False)
    f64 = bt.HostStream(x.astype(np.float64), bt.Time(T0), RATE, pin=False)
    flat = bt.HostStream(x[:, 0, 0].copy(), bt.Time(T0), RATE, pin=False)
    for cls, args in ((bt.MedianWhiten, (4,)), (bt.RobustStandardize, (4,))):
        with pytest.raises(TypeError, match='Square'):
            cls(z, *args)
        with pytest.raises(TypeError, match='float32'):
            cls(f64, *args)
        with pytest.raises(TypeError):
            cls(sh, 4.5)
    with pytest.raises(ValueError, match='bin axis'):
        bt.MedianWhiten(flat, 4)
    for m in (1, 65537, 0):
        with pytest.raises(ValueError, match='whitening block'):
            bt.MedianWhiten(sh, m)
        with pytest.raises(ValueError, match='block'):
            bt.RobustStandardize(sh, m)
    bt.MedianWhiten(sh, 2), bt.MedianWhiten(sh, 65536), bt.MedianWhiten(sh, 4, 0), bt.MedianWhiten(sh, 4, 9)
    for skip in (-1, 10):
        with pytest.raises(ValueError, match='skip'):
            bt.MedianWhiten(sh, 4, skip)
    with pytest.raises(ValueError, match='less than one block'):
        bt.RobustStandardize(sh, 41)
    for spf in (3, 6, 0):
        with pytest.raises(ValueError, match='multiple'):
            bt.RobustStandardize(sh, 4, samples_per_frame=spf)
    bt.RobustStandardize(sh, 40), bt.RobustStandardize(flat, 2)


def test_library_exports_the_rank_entries():
    lib = hip.lib()
    assert lib.bbt_version() >= 168 and hip.MIN_LIB_VERSION >= 168
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_rank_stats', 'bbt_rank_standardize', 'bbt_rank_whiten', 'bbt_rank_info'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'rank_geo.hpp')).read()
    assert f'#define BBT_RANK_MIN_N {hip.RANK_MIN_N}' in geo and f'#define BBT_RANK_MAX_N {hip.RANK_MAX_N}' in geo
    assert f'#define BBT_RANK_LDS_BYTES {hip.RANK_LDS_BYTES}' in geo and f'#define BBT_RANK_MISC_BYTES {hip.RANK_MISC_BYTES}' in geo
    assert f'#define BBT_RANK_MAD_SCALE {hip.RANK_MAD_SCALE!r}' in geo and search.MAD_SCALE == hip.RANK_MAD_SCALE
    assert 2 * hip.RANK_LDS_BYTES <= 160 * 1024
    # 1 / (sqrt(2) erfinv(1/2)) = 1 / Phi^-1(3/4)
    assert abs(hip.RANK_MAD_SCALE - 1.482602218505602) == 0. and abs(math.erf(1. / (hip.RANK_MAD_SCALE * math.sqrt(2.))) - 0.5) < 1e-15
    assert (search.MAX_N, periodicity.MAX_M) == (hip.RANK_MAX_N, hip.RANK_MAX_N)
    for name in ('RobustStandardize', 'robust_standardize_samples', 'block_median_mad_samples'):
        assert name in search.__all__ and getattr(bt, name) is getattr(search, name)
    for name in ('MedianWhiten', 'median_whiten_samples', 'median_ratio'):
        assert name in periodicity.__all__ and getattr(bt, name) is getattr(periodicity, name)


def test_rank_info_needs_no_device(monkeypatch):
    for name in ('BBT_RANK_ROUTE', 'BBT_RANK_DIGIT', 'BBT_RANK_WIDTH'):
        monkeypatch.delenv(name, raising=False)
    info = hip.rank_info()
    rows = info['lds_rows']
    assert rows == {w: (hip.RANK_LDS_BYTES - hip.RANK_MISC_BYTES - 16 * w * 4) // (4 * w) for w in (16, 32, 64)}
    assert rows[64] >= 128                                               # MedianWhiten's usual block, 64 columns wide
    # the automatic rule: the widest tile whose block fits the LDS, on 4-bit digits; else global, 16 wide, 8-bit
    assert hip.rank_info(64, 8193, 512, 128, 1) == dict(route='lds', digit=4, width=64, lds_rows=rows,
                                                        lds_bytes=16 * 64 * 4 + 1024 + 128 * 64 * 4)
    got = hip.rank_info(1, 1 << 16, 512, 256, 0)
    assert (got['route'], got['width']) == ('lds', 64)
    got = hip.rank_info(1, 1 << 16, 512, 4096, 0)
    assert (got['route'], got['digit'], got['width'], got['lds_bytes']) == ('global', 8, 16, 256 * 16 * 4 + 1024)
    assert hip.rank_info(1, 1000, 3, rows[16], 0)['route'] == 'lds'
    assert hip.rank_info(1, 1000, 3, rows[16] + 1, 0)['route'] == 'global' if rows[16] < 1000 else True
    assert hip.rank_info(1, rows[16] + 1, 3, rows[16] + 1, 0)['route'] == 'global'
    for route, digit, width in rank_cases.TILINGS:
        rank_cases.set_tiling(monkeypatch, route, digit, width)
        got = hip.rank_info(1, 2100, 67, 20, 0)
        assert (got['route'], got['digit'], got['width']) == (route, digit, width)
        # lds is "wherever it fits": a block too long for it goes the other way
        too_long = got['lds_rows'][width] + 1
        assert hip.rank_info(1, 70000, 67, too_long, 0)['route'] == 'global'
    monkeypatch.setenv('BBT_RANK_ROUTE', 'auto')
    monkeypatch.setenv('BBT_RANK_DIGIT', '5')
    monkeypatch.setenv('BBT_RANK_WIDTH', '48')
    got = hip.rank_info(1, 2100, 67, 20, 0)
    assert (got['route'], got['digit'], got['width']) == ('lds', 4, 64)
    for args, what in (((1, 100, 3, 1, 0), 'block'), ((1, 100, 3, 65537, 0), 'block'), ((0, 100, 3, 4, 0), 'rows'),
                       ((1, 100, 0, 4, 0), 'elements'), ((1, 100, 3, 4, 100), 'skip'), ((1, 100, 3, 4, -1), 'skip'),
                       ((1, (1 << 40) + 1, 3, 4, 0), '2\\^40'), ((1, 1 << 40, 3, 2, 0), 'tiles')):
        with pytest.raises(hip.HipError, match=what):
            hip.rank_info(*args)


# -- the tiling and the descent, on the host ---------------------------------------------------------------------
def _geo_shapes():
    """Every shared shape under the automatic rule and under every (route, digit, width) the GPU tests
    force: (n_spec, nbin, n_elem, m, skip, width, digit, route)."""
    routes = {'lds': 1, 'global': 2}
    shapes = []
    for shape in rank_cases.geo_shapes():
        shapes.append(shape + (0, 0, 0))
        for route, digit, width in rank_cases.TILINGS:
            shapes.append(shape + (width, digit, routes[route]))
    # the bench shapes, and more than 2^31 values in a chunk
    shapes += [(1, 1 << 16, 512, 256, 0, 0, 0, 0), (1, 1 << 16, 512, 4096, 0, 0, 0, 0), (1, 1 << 16, 512, 65536, 0, 0, 0, 0),
               (64, 8193, 512, 128, 1, 0, 0, 0), (64, 8193, 4100, 128, 1, 0, 0, 0), (1, 1 << 22, 600, 65536, 0, 0, 0, 2)]
    return shapes


def test_kernel_tiling_and_descent_on_the_host(tmp_path):
    """The limits and refusals, the key map and the digit descent against sorted keys on a few thousand
    blocks (65536 equal values among them), and for every shape every (block, element tile) owned once,
    every row inside its spectrum, the skip rows zeroed once, the LDS within the budget: the program
    exits non-zero otherwise, and the sanitizers abort it on a wild index or an overflow of its own."""
    exe = compile_check('rank_geo_check', tmp_path)
    shapes = _geo_shapes()
    plans = run_check(exe, shapes)
    seen_routes = set()
    for shape, g in zip(shapes, plans):
        n_spec, nbin, e, m, skip, width, digit, route = shape
        assert g['walk'] == 0, (shape, g)
        len_max = min(m, nbin - skip)
        assert g['nx'] * g['ny'] == 256 and g['nblk'] == -(-(nbin - skip) // m) and g['len_max'] == len_max
        assert g['n_tile'] == -(-e // g['nx']) and g['n_wg'] == n_spec * g['nblk'] * g['n_tile']
        if width:
            assert g['nx'] == width
        else:
            assert g['nx'] <= max(16, min(64, 1 << (e - 1).bit_length()))
        hist = (1 << g['digit']) * g['nx'] * 4
        fits = len_max <= (hip.RANK_LDS_BYTES - hip.RANK_MISC_BYTES - (1 << (digit or 4)) * g['nx'] * 4) // (4 * g['nx'])
        assert g['route'] == (1 if fits and route != 2 else 2)
        assert g['digit'] == (digit or (4 if g['route'] == 1 else 8))
        assert g['lds_bytes'] == hist + hip.RANK_MISC_BYTES + (len_max * g['nx'] * 4 if g['route'] == 1 else 0)
        assert g['lds_bytes'] <= hip.RANK_LDS_BYTES
        seen_routes.add((g['route'], g['digit'], g['nx']))
    assert len(seen_routes) == 12                                  # both routes, both digits, every width
    # what the library refuses: a block of 1 and of 65537, no rows, no elements, a skip of nbin, 2^40 rows and
    # one, too many tiles, and bad tilings
    bad = run_raw(exe, '1 100 3 1 0 0 0 0  1 100 3 65537 0 0 0 0  0 100 3 4 0 0 0 0  1 100 0 4 0 0 0 0 '
                       '1 100 3 4 100 0 0 0  1 1099511627777 3 4 0 0 0 0  1 1099511627776 3 2 0 0 0 0 '
                       '1 100 3 4 0 48 0 0  1 100 3 4 0 0 5 0  1 100 3 4 0 0 0 3')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 10
    assert 'block' in errors[0] and 'block' in errors[1] and 'rows' in errors[2] and 'elements' in errors[3]
    assert 'skip' in errors[4] and '2^40' in errors[5] and 'tiles' in errors[6]
    assert 'width' in errors[7] and 'digit' in errors[8] and 'route' in errors[9]
