"""`hip.rank_stats`, `RobustStandardize` and `MedianWhiten` on the GPU against their NumPy twins
(`search.block_median_mad_samples`, `search.robust_standardize_samples`,
`periodicity.median_whiten_samples`), bit for bit: a median is an exact selection, so a value has one
correct result whatever the route, the digit width, the tile width or the chunking.  The shared cases
of rank_cases.py (test_rank_host.py proves the twins), both routes, both digits and every tile width,
the route boundary, the counter width, chunks, frames and seeks, guard bands, a chain on the device,
and the refusals."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity, search
from baseband_tasks_amd.device_task import produces_on_device

import rank_cases
from guard_bands import POISONS, SKEWS, Guarded, check_all
from rank_cases import HOST_CASES, HOST_IDS, TILINGS, same_bits, set_tiling, stream

pytestmark = pytest.mark.gpu

F32 = np.dtype(np.float32)


def _stats(x, n, nbin=None, skip=0, mad=True):
    """`hip.rank_stats` of host ``x``: time-domain blocks of ``n`` (``nbin`` None) or spectra."""
    if nbin is None:
        nb = x.shape[0] // n
        x = x[:nb * n]
        n_elem = int(np.prod(x.shape[1:], dtype=int))
        got = hip.rank_stats(hip.DeviceArray.from_host(x), nb * n, n_elem, n, 0, mad=mad)
        shape = (nb,) + x.shape[1:]
    else:
        n_elem = int(np.prod(x.shape[2:], dtype=int))
        got = hip.rank_stats(hip.DeviceArray.from_host(x), nbin, n_elem, n, skip, mad=mad)
        shape = (x.shape[0], -(-(nbin - skip) // n)) + x.shape[2:]
    return tuple(a.to_host().reshape(shape) for a in (got if mad else (got,)))


def _standardize(x, n):
    n_elem = int(np.prod(x.shape[1:], dtype=int))
    nb = x.shape[0] // n
    return hip.rank_standardize(hip.DeviceArray.from_host(x[:nb * n]), n, n_elem).to_host().reshape((nb * n,) + x.shape[1:])


# -- the shared cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind, n', HOST_CASES, ids=HOST_IDS)
def test_stats_entry_and_task_equal_the_twins(kind, n):
    x = rank_cases.data(kind, n)
    med, mad, z = rank_cases.expected(kind, n)
    got_med, got_mad = _stats(x, n)
    assert same_bits(got_med, med) and same_bits(got_mad, mad)
    assert same_bits(_stats(x, n, mad=False)[0], med)
    assert same_bits(_standardize(x, n), z)
    got = bt.RobustStandardize(stream(x), n).read()
    assert got.dtype == np.float32 and same_bits(got, z)
    dev = bt.RobustStandardize(stream(x, bt.DeviceStream), n)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), z)


@pytest.mark.parametrize('m, skip', rank_cases.WH_CUTS)
def test_median_whiten_equals_its_twin(m, skip):
    x = rank_cases.wh_data()
    want = rank_cases.wh_expected(m, skip)
    got = bt.MedianWhiten(stream(x), m, skip, averaged=4).read()
    assert got.dtype == np.float32 and same_bits(got, want)
    dev = bt.MedianWhiten(stream(x, bt.DeviceStream), m, skip, ratio=rank_cases.WH_RATIO)
    assert produces_on_device(dev) and same_bits(dev.read_device().to_host(), want)
    out = hip.rank_whiten(hip.DeviceArray.from_host(x), x.shape[1], x.shape[2], m, skip, rank_cases.WH_RATIO)
    assert same_bits(out.to_host().reshape(want.shape), want)
    # the default ratio: exponential powers
    got = bt.MedianWhiten(stream(x, bt.DeviceStream), m, skip).read()
    assert same_bits(got, periodicity.median_whiten_samples(x, m, skip))
    # the statistics of the ragged blocks, the single bin included
    med, mad = rank_cases.spectra_stats(x, m, skip)
    got_med, got_mad = _stats(x, m, x.shape[1], skip)
    assert same_bits(got_med, med) and same_bits(got_mad, mad)


@pytest.mark.parametrize('shape', [(67,), (300, 4), (1,), ()], ids=str)
def test_sample_shapes(shape):
    rng = np.random.default_rng(19)
    x = rng.normal(5., 3., (600,) + shape).astype(np.float32)
    for n in (2, 64, 75, 600):
        assert same_bits(bt.RobustStandardize(stream(x, bt.DeviceStream), n).read(), search.robust_standardize_samples(x, n))
        med, mad = search.block_median_mad_samples(x, n)
        got_med, got_mad = _stats(x, n)
        assert same_bits(got_med, med) and same_bits(got_mad, mad)
    s = (4. * rng.standard_exponential((3, 1501) + shape)).astype(np.float32)
    for skip in (0, 1, 7):
        got = bt.MedianWhiten(stream(s, bt.DeviceStream), 61, skip).read()
        assert same_bits(got, periodicity.median_whiten_samples(s, 61, skip))
    got = bt.MedianWhiten(stream(s, bt.DeviceStream), 60, 0, averaged=2).read()          # a last block of one bin
    assert same_bits(got, periodicity.median_whiten_samples(s, 60, 0, periodicity.median_ratio(2)))


# -- both routes, both digits, every tile width -------------------------------------------------------------
@pytest.mark.parametrize('route, digit, width', TILINGS)
def test_no_value_depends_on_the_route_the_digit_or_the_width(route, digit, width, monkeypatch):
    """BBT_RANK_ROUTE, BBT_RANK_DIGIT and BBT_RANK_WIDTH reshape the work; the selection is exact, so every
    bit stays.  A block too long for the LDS at this width and digit goes the global way under 'lds' too."""
    set_tiling(monkeypatch, route, digit, width)
    fits = hip.rank_info()['lds_rows'][width]
    for kind, n in (('noise', 2), ('noise', 33), ('noise', 257), ('noise', 1000), ('planted', 8), ('planted', 9)):
        x = rank_cases.data(kind, n)
        info = hip.rank_info(1, x.shape[0] // n * n, x.shape[1], n, 0)
        assert (info['digit'], info['width']) == (digit, width)
        assert info['route'] == (route if n <= fits else 'global')
        med, mad, z = rank_cases.expected(kind, n)
        got_med, got_mad = _stats(x, n)
        assert same_bits(got_med, med) and same_bits(got_mad, mad)
        assert same_bits(bt.RobustStandardize(stream(x, bt.DeviceStream), n).read(), z)
    x = rank_cases.wh_data()
    for m, skip in rank_cases.WH_CUTS + ((20, 1),):
        assert hip.rank_info(3, 1501, 7, m, skip)['route'] == (route if m <= fits else 'global')
        want = periodicity.median_whiten_samples(x, m, skip, rank_cases.WH_RATIO)
        got = bt.MedianWhiten(stream(x, bt.DeviceStream), m, skip, averaged=4).read()
        assert same_bits(got, want)
        med, mad = rank_cases.spectra_stats(x, m, skip)
        got_med, got_mad = _stats(x, m, 1501, skip)
        assert same_bits(got_med, med) and same_bits(got_mad, mad)


def test_the_route_boundary(monkeypatch):
    """On 'auto': a block of exactly the largest length the lds route takes, and one a row longer."""
    for name in ('BBT_RANK_ROUTE', 'BBT_RANK_DIGIT', 'BBT_RANK_WIDTH'):
        monkeypatch.delenv(name, raising=False)
    L = hip.rank_info(1, 4, 3, 2, 0)['lds_rows'][16]
    assert hip.rank_info(1, 2 * L, 3, L, 0)['route'] == 'lds' and hip.rank_info(1, 2 * L + 2, 3, L + 1, 0)['route'] == 'global'
    rng = np.random.default_rng(23)
    for n, route in ((L, 'lds'), (L + 1, 'global')):
        x = rng.normal(0., 1., (2 * n, 3)).astype(np.float32)
        x[5, 1] = np.nan
        info = hip.rank_info(1, 2 * n, 3, n, 0)
        assert (info['route'], info['width']) == (route, 16) and info['lds_bytes'] <= hip.RANK_LDS_BYTES
        med, mad = search.block_median_mad_samples(x, n)
        got_med, got_mad = _stats(x, n)
        assert same_bits(got_med, med) and same_bits(got_mad, mad)
        assert same_bits(_standardize(x, n), search.robust_standardize_samples(x, n))
        s = np.abs(x).reshape(2, n, 3) + np.float32(0.5)
        want = periodicity.median_whiten_samples(s, n, 0)
        got = hip.rank_whiten(hip.DeviceArray.from_host(s), n, 3, n, 0).to_host().reshape(s.shape)
        assert same_bits(got, want)


@pytest.mark.parametrize('route', ['lds', 'global'])
@pytest.mark.parametrize('n', [65536, 'lds_rows'])
def test_counter_width(n, route, monkeypatch):
    """A block of equal values puts all of them into one counter at every digit; one more than half
    equal is mad = 0 by one value; a permutation of distinct values is the other extreme.  65536 is the
    longest block (it never fits the LDS: 'lds' takes the global route there); the longest the lds route
    takes is run too."""
    set_tiling(monkeypatch, route)
    if n == 'lds_rows':
        n = hip.rank_info(1, 4, 2, 2, 0)['lds_rows'][16] // 2 * 2
        assert hip.rank_info(1, n, 2, n, 0)['route'] == route
    else:
        assert hip.rank_info(1, n, 2, n, 0)['route'] == 'global'
    rng = np.random.default_rng(29)
    equal = np.full((n, 2), 2.5, np.float32)
    equal[:, 1] = -0.
    most = np.full((n, 2), 7., np.float32)
    spots = rng.permutation(n)[:n // 2 - 1]
    most[spots, 0] = 8. + np.arange(n // 2 - 1, dtype=np.float32)
    most[spots, 1] = -8. - np.arange(n // 2 - 1, dtype=np.float32)
    assert (most[:, 0] == 7.).sum() == n // 2 + 1
    distinct = np.stack([rng.permutation(n), -rng.permutation(n)], axis=1).astype(np.float32) - np.float32(30000.)
    for x, flat in ((equal, True), (most, True), (distinct, False)):
        med, mad = search.block_median_mad_samples(x, n)
        got_med, got_mad = _stats(x, n)
        assert same_bits(got_med, med) and same_bits(got_mad, mad)
        z = _standardize(x, n)
        assert same_bits(z, search.robust_standardize_samples(x, n))
        assert flat == (not z.view(np.uint32).any()) and flat == (not mad.any())


# -- chunks, frames and seeks ---------------------------------------------------------------------------------
def test_standardize_chunks_frames_and_seeks(monkeypatch):
    x, n = rank_cases.noise(), 100
    want = rank_cases.expected('noise', n)[2]                          # 21 blocks
    calls = []
    run = hip.rank_standardize
    monkeypatch.setattr(hip, 'rank_standardize', lambda x_, n_, e, out=None:
                        (calls.append(x_.size // (n_ * e)), run(x_, n_, e, out=out))[1])
    for cls in (bt.HostStream, bt.DeviceStream):
        for per, launches in ((1, [1] * 21), (8, [8, 8, 5]), (21, [21])):
            rs = bt.RobustStandardize(stream(x, cls), n)
            assert rs.samples_per_frame == 2100
            rs.robust_budget = per * n * 67 * 4
            del calls[:]
            assert same_bits(rs.read(), want)
            assert calls == launches
        rs.robust_budget = 1                                           # (never less than a block)
        rs.invalidate_cache()
        rs.seek(1900)
        del calls[:]
        assert same_bits(rs.read(), want[1900:])
        assert calls == [1] * 21
    for spf in (100, 700):                                             # one block a frame, and several
        rs = bt.RobustStandardize(stream(x, bt.DeviceStream, samples_per_frame=50), n, samples_per_frame=spf)
        assert rs.samples_per_frame == spf
        for start, count in [(0, 100), (250, 333), (1999, 101), (0, 2100)]:
            rs.seek(start)
            assert same_bits(rs.read(count), want[start:start + count])
            assert rs.tell() == start + count
        rs.seek(1050)                                                  # into the middle, to the end
        assert same_bits(rs.read_device().to_host(), want[1050:])


def test_whiten_chunks_frames_and_seeks(monkeypatch):
    m, skip = 61, 7
    x = rank_cases.wh_data()
    want = rank_cases.wh_expected(m, skip)
    n_spec, nbin, n_elem = want.shape
    calls = []
    run = hip.rank_whiten
    monkeypatch.setattr(hip, 'rank_whiten', lambda x_, nbin_, e, m_, s_, r_, out=None:
                        (calls.append(x_.size // (nbin_ * e)), run(x_, nbin_, e, m_, s_, r_, out=out))[1])
    for cls in (bt.HostStream, bt.DeviceStream):
        for per, launches in ((1, [1, 1, 1]), (2, [2, 1]), (3, [3])):
            wh = bt.MedianWhiten(stream(x, cls), m, skip, averaged=4)
            assert wh.samples_per_frame == n_spec
            wh.whiten_budget = per * nbin * n_elem * 4
            del calls[:]
            assert same_bits(wh.read(), want)
            assert calls == launches
        wh.whiten_budget = 1                                           # (never less than a spectrum)
        wh.invalidate_cache()
        wh.seek(2)
        del calls[:]
        assert same_bits(wh.read(1), want[2:])
        assert calls == [1, 1, 1]
    wh = bt.MedianWhiten(stream(x, bt.DeviceStream, samples_per_frame=1), m, skip, averaged=4)
    assert wh.samples_per_frame == 1
    for start, count in [(1, 1), (0, 2), (2, 1), (0, 3)]:
        wh.seek(start)
        assert same_bits(wh.read(count), want[start:start + count])
    wh.seek(1)
    assert same_bits(wh.read_device().to_host(), want[1:])


# -- guard bands ------------------------------------------------------------------------------------------------
both_skews = pytest.mark.parametrize('skew', SKEWS, ids=['aligned16', 'off4'])
both_poisons = pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))
both_routes = pytest.mark.parametrize('route', ['lds', 'global'])


def _words_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@both_poisons
@both_skews
@both_routes
def test_guard_bands_stats(route, skew, poison, monkeypatch):
    """The data are free of NaN and Inf: a poison read as data would flag a block or win a rank."""
    set_tiling(monkeypatch, route)
    x = rank_cases.wh_data()[:, :, 3:]                                 # (3, 1501, 4): noise only
    m, skip = 61, 7                                                   # a ragged last block behind the skipped bins
    med, mad = rank_cases.spectra_stats(x, m, skip)
    assert hip.rank_info(3, 1501, 4, m, skip)['route'] == route
    gx = Guarded.load(x, poison, skew)
    gm, gd = Guarded(med.shape, F32, poison, skew), Guarded(mad.shape, F32, poison, skew)
    hip.rank_stats(gx.array, 1501, 4, m, skip, out=(gm.array, gd.array))
    got_x, got_med, got_mad = check_all([gx, gm, gd], f'rank_stats {route}')
    assert same_bits(got_med, med) and same_bits(got_mad, mad) and _words_equal(got_x, x)
    assert np.isfinite(got_med).all() and np.isfinite(got_mad).all()


@both_poisons
@both_skews
@both_routes
def test_guard_bands_standardize(route, skew, poison, monkeypatch):
    set_tiling(monkeypatch, route)
    n = 33
    x = rank_cases.noise()[:20 * n]                                    # 20 blocks of 67 elements: two ragged tiles
    want = search.robust_standardize_samples(x, n)
    assert hip.rank_info(1, 20 * n, 67, n, 0)['route'] == route
    gx, go = Guarded.load(x, poison, skew), Guarded(want.shape, F32, poison, skew)
    hip.rank_standardize(gx.array, n, 67, out=go.array)
    got_x, got = check_all([gx, go], f'rank_standardize {route}')
    assert same_bits(got, want) and _words_equal(got_x, x) and np.isfinite(got).all() and got.any()


@both_poisons
@both_skews
@both_routes
def test_guard_bands_whiten(route, skew, poison, monkeypatch):
    set_tiling(monkeypatch, route)
    x = rank_cases.wh_data()[:, :, 3:]
    m, skip = 60, 0                                                   # the last block is the last bin alone
    want = periodicity.median_whiten_samples(x, m, skip, 0.9)
    gx, go = Guarded.load(x, poison, skew), Guarded(want.shape, F32, poison, skew)
    hip.rank_whiten(gx.array, 1501, 4, m, skip, 0.9, out=go.array)
    got_x, got = check_all([gx, go], f'rank_whiten {route}')
    assert same_bits(got, want) and _words_equal(got_x, x) and np.isfinite(got).all() and (got > 0).all()
    m, skip = 61, 7
    want = periodicity.median_whiten_samples(x, m, skip, 0.9)
    go = Guarded(want.shape, F32, poison, skew)
    hip.rank_whiten(gx.array, 1501, 4, m, skip, 0.9, out=go.array)
    got_x, got = check_all([gx, go], f'rank_whiten {route} skip')
    assert same_bits(got, want) and _words_equal(got_x, x) and not got[:, :skip].view(np.uint32).any()


# -- a chain that never leaves HBM ---------------------------------------------------------------------------------
def test_single_pulse_chain_on_the_device():
    rng = np.random.default_rng(31)
    x = rng.standard_normal((4096, 8)).astype(np.float32)
    x[1424:1424 + 64, 3] += np.float32(50.)                             # block 1 of 1024; start 144 of search block 5
    plane = stream(x, bt.DeviceStream, samples_per_frame=1024)
    robust = bt.BoxcarSearch(bt.RobustStandardize(plane, 1024), 256, n_widths=8)
    naive = bt.BoxcarSearch(bt.Standardize(plane, 1024), 256, n_widths=8)
    stage = robust
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    got, ref = robust.read_device().to_host(), naive.read()
    assert got.shape == ref.shape == (16, 3, 8)
    assert same_bits(got, search.boxcar_search_samples(search.robust_standardize_samples(x, 1024), 256, 8))
    assert got[5, :, 3].tolist()[1:] == [144., 6.] and ref[5, :, 3].tolist()[1:] == [144., 6.]
    print('S/N of the pulse: robust', got[5, search.SNR, 3], 'plain', ref[5, search.SNR, 3])
    assert got[5, search.SNR, 3] > 5. * ref[5, search.SNR, 3] and got[5, search.SNR, 3] > 300.
    cands = search.boxcar_candidates(got, 256, 20.)
    assert (cands['sample'][0], cands['trial'][0], cands['width'][0]) == (1424, 3, 64)


def test_periodicity_chain_on_the_device():
    rng = np.random.default_rng(37)
    x = rng.standard_normal((4096, 8)).astype(np.float32)
    x[::32, 5] += np.float32(6.)                                       # a pulse train of period 32 samples
    plane = stream(x, bt.DeviceStream, samples_per_frame=1024, frequency=np.float64(6e8), sideband=1)
    sp = bt.fluctuation_spectra(plane, 1024, stack=4)
    wh = bt.MedianWhiten(sp, 64, averaged=4)
    hs = bt.HarmonicSearch(wh, 32)
    stage = hs
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    assert sp.shape == (1, 513, 8) and wh.shape == sp.shape and hs.shape == (1, 17, 3, 8)
    got = hs.read_device().to_host()
    sp.seek(0)
    spectra = sp.read()
    z = periodicity.median_whiten_samples(spectra, 64, 1, periodicity.median_ratio(4))
    wh.seek(0)
    assert same_bits(wh.read(), z)
    assert same_bits(got, periodicity.harmonic_search_samples(z, 32, 5, 1., 1))
    assert np.isfinite(got).all()
    # the train's fundamental is bin 32: the winner of the column is a sum of harmonics of it
    snr = got[0, :, periodicity.SNR]
    assert snr[:, 5].max() == snr.max() and snr[:, 5].max() > 3. * np.delete(snr, 5, axis=1).max()


# -- what is refused ------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    lib = hip.lib()
    x = hip.DeviceArray.from_host(np.ones((2, 8, 2), np.float32))
    out = hip.DeviceArray.from_host(np.full((2, 8, 2), 5., np.float32))
    st = hip.DeviceArray.from_host(np.full((2, 4, 2), 5., np.float32))

    def refused(rc, what):
        return rc != 0 and what in lib.bbt_last_error()
    assert refused(lib.bbt_rank_stats(None, st.ptr, None, 2, 8, 2, 2, 0, None), b'null')
    assert refused(lib.bbt_rank_stats(x.ptr, None, None, 2, 8, 2, 2, 0, None), b'null')
    assert refused(lib.bbt_rank_stats(x.ptr + 2, st.ptr, None, 2, 8, 2, 2, 0, None), b'aligned')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, st.ptr + 1, 2, 8, 2, 2, 0, None), b'aligned')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, None, 2, 8, 2, 1, 0, None), b'block')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, None, 2, 8, 2, 65537, 0, None), b'block')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, None, 2, 8, 2, 2, 8, None), b'skip')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, None, 0, 8, 2, 2, 0, None), b'rows')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, None, 2, 8, 0, 2, 0, None), b'elements')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, None, 1, (1 << 40) + 1, 2, 2, 0, None), b'2^40')
    assert refused(lib.bbt_rank_stats(x.ptr, st.ptr, None, 1, 1 << 40, 2, 2, 0, None), b'tiles')
    assert refused(lib.bbt_rank_standardize(None, out.ptr, 2, 8, 2, None), b'null')
    assert refused(lib.bbt_rank_standardize(x.ptr, out.ptr + 2, 2, 8, 2, None), b'aligned')
    assert refused(lib.bbt_rank_standardize(x.ptr, out.ptr, 16, 1, 2, None), b'block')
    assert refused(lib.bbt_rank_standardize(x.ptr, out.ptr, 1, 65537, 2, None), b'block')
    assert refused(lib.bbt_rank_standardize(x.ptr, out.ptr, 0, 8, 2, None), b'whole block')
    assert refused(lib.bbt_rank_standardize(x.ptr, out.ptr, 1 << 39, 4, 2, None), b'2^40')
    assert refused(lib.bbt_rank_whiten(x.ptr, None, 2, 8, 2, 2, 1, 0.7, None), b'null')
    assert refused(lib.bbt_rank_whiten(x.ptr + 1, out.ptr, 2, 8, 2, 2, 1, 0.7, None), b'aligned')
    assert refused(lib.bbt_rank_whiten(x.ptr, out.ptr, 2, 8, 2, 1, 1, 0.7, None), b'block')
    assert refused(lib.bbt_rank_whiten(x.ptr, out.ptr, 2, 8, 2, 2, 8, 0.7, None), b'skip')
    for ratio in (0., -1., float('inf'), float('nan')):
        assert refused(lib.bbt_rank_whiten(x.ptr, out.ptr, 2, 8, 2, 2, 1, ratio, None), b'ratio')
    hip.synchronize()
    assert (out.to_host() == 5.).all() and (st.to_host() == 5.).all()      # nothing ran
    # through the wrappers
    for m, skip in ((1, 1), (65537, 1), (4, 8), (4, -1)):
        with pytest.raises(ValueError):
            hip.rank_whiten(x, 8, 2, m, skip)
        with pytest.raises(ValueError):
            hip.rank_stats(x, 8, 2, m, skip)
    for ratio in (0., float('nan')):
        with pytest.raises(ValueError, match='ratio'):
            hip.rank_whiten(x, 8, 2, 4, 1, ratio)
    with pytest.raises(ValueError):
        hip.rank_whiten(x, 8, 2, 4, 1, out=hip.DeviceArray((2, 7, 2), np.float32))
    with pytest.raises(ValueError):
        hip.rank_whiten(x, 7, 2, 4, 1)
    with pytest.raises(ValueError):
        hip.rank_stats(x, 8, 2, 4, 0, out=(st,))
    with pytest.raises(ValueError):
        hip.rank_standardize(x, 1, 2)
    with pytest.raises(ValueError):
        hip.rank_standardize(x, 4, 3)
    with pytest.raises(ValueError):
        hip.rank_standardize(x, 4, 2, out=hip.DeviceArray((15, 2), np.float32))
    z = hip.DeviceArray((2, 8, 2), np.complex64)
    for call in (lambda: hip.rank_whiten(z, 8, 2, 4, 1), lambda: hip.rank_stats(z, 8, 2, 4), lambda: hip.rank_standardize(z, 4, 2)):
        with pytest.raises(TypeError):
            call()
    zs = bt.DeviceStream(np.ones((16, 8, 2), np.complex64), bt.Time(rank_cases.T0), rank_cases.RATE)
    for cls in (bt.RobustStandardize, bt.MedianWhiten):
        with pytest.raises(TypeError, match='Square'):
            cls(zs, 4)
    # and what is not refused runs: ones whiten to ratio, standardize to +0 (mad = 0)
    got = hip.rank_whiten(x, 8, 2, 4, 1, 0.5).to_host()
    assert not got[:, 0].any() and (got[:, 1:] == 0.5).all()
    assert not hip.rank_standardize(x, 4, 2).to_host().view(np.uint32).any()
    med, mad = hip.rank_stats(x, 8, 2, 4, 0)
    assert (med.to_host() == 1.).all() and not mad.to_host().any()
