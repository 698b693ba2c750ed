"""Host side of `Standardize`, `BoxcarSearch` and `boxcar_candidates` (no GPU): the NumPy twins against
brute-force restatements with the tie rule spelt out in loops and against float64 within the bound
their order implies, the scales, the candidate rule on a hand-made plane, construction, metadata,
framing and the argument checks of both tasks, and the kernels' tiling (csrc/sps_geo.hpp) walked on
the host by a stand-alone program under sanitizers."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, search
from baseband_tasks_amd.search import OFFSET, SNR, WIDTH

import sps_cases
from sps_cases import CASES, IDS, RATE, T0
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


# -- the boxcar twin ------------------------------------------------------------------------------------
def _brute(x, n, K):
    """int64 window sums by cumulative sum, float64 S/N (an integer below 2^24 times a float32 scale is
    exact in float64), the winner found with loops and the tie rule spelt out: larger S/N, then smaller k,
    then smaller i; only windows that fit the stream."""
    N = x.shape[0]
    nb = N // n
    cols = x.reshape(N, -1).astype(np.int64)
    csum = np.concatenate([np.zeros((1, cols.shape[1]), np.int64), np.cumsum(cols, axis=0)])
    assert np.abs(np.diff(csum, axis=0)).max() <= 4
    out = np.empty((nb, 3, cols.shape[1]), np.float64)
    for e in range(cols.shape[1]):
        c = csum[:, e].tolist()
        for b in range(nb):
            win = None
            for k in range(K):
                w = 1 << k
                scale = float(np.float32(2.0 ** (-k / 2)))
                for i in range(b * n, (b + 1) * n):
                    if i + w > N:
                        break
                    snr = (c[i + w] - c[i]) * scale
                    if win is None or snr > win[0]:                       # (k, i ascending: ties keep the earlier)
                        win = (snr, i - b * n, k)
            out[b, :, e] = win
    return out.reshape((nb, 3) + x.shape[1:])


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_is_the_brute_force_rule_on_integers(case):
    x = sps_cases.data(case)
    got = sps_cases.expected(case)
    assert got.dtype == np.float32 and got.shape == (case.N // case.n, 3) + case.s
    cols = x if case.name != 'wide' else x[:, :7]             # (the loops are slow: a few columns of the widest)
    want = _brute(cols, case.n, case.K)
    # (the float64 S/N is exact; the twin's is that, rounded once to float32)
    np.testing.assert_array_equal(got[(slice(None),) * 2 + (slice(0, cols.shape[1]),)], want.astype(np.float32))
    # the data do have ties to break, and windows that do not fit
    snr = got[:, SNR]
    assert np.isfinite(snr).all() and (got[:, WIDTH] < case.K).all() and (got[:, OFFSET] < case.n).all()
    i = got[:, OFFSET] + (np.arange(got.shape[0]) * case.n).reshape((-1,) + (1,) * len(case.s))
    assert (i + 2. ** got[:, WIDTH] <= case.N).all()


def test_ties_go_to_the_smaller_width_then_the_earlier_start():
    x = np.zeros((16, 1), np.float32)
    x[3, 0] = x[9, 0] = 2.                                     # two equal peaks, too far apart to share a window
    out = search.boxcar_search_samples(x, 16, 3)
    assert out[0, :, 0].tolist() == [2., 3., 0.]
    # S_2 * c_2 = 4 * 0.5 = 2 equals a single 2 at k = 0: k = 0 wins although it starts later
    y = np.zeros((16, 1), np.float32)
    y[0:4, 0] = 1.
    y[10, 0] = 2.
    out = search.boxcar_search_samples(y, 16, 3)
    assert out[0, :, 0].tolist() == [2., 10., 0.]
    # ... and without the single sample the window of 4 is found at its start
    y[10, 0] = 0.
    out = search.boxcar_search_samples(y, 16, 3)
    assert out[0, :, 0].tolist() == [2., 0., 2.]
    # windows may run into the next block and the dropped tail, but not past the stream
    z = np.zeros((11, 1), np.float32)
    z[4:11, 0] = 1.
    out = search.boxcar_search_samples(z, 5, 3)
    assert out.shape == (2, 3, 1)
    assert out[0, :, 0].tolist() == [2., 4., 2.]               # starts in block 0 at 4, covers 4 ... 7
    assert out[1, :, 0].tolist() == [2., 0., 2.]               # 5 ... 8; the last start that fits is 7
    # NaN never wins, -inf may, a block of NaN gives (-inf, 0, 0)
    v = np.full((6, 1), np.nan, np.float32)
    v[4, 0] = -np.inf
    out = search.boxcar_search_samples(v, 3, 2)
    assert out[0, :, 0].tolist() == [-np.inf, 0., 0.] and out[1, :, 0].tolist() == [-np.inf, 1., 0.]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_twin_sums_on_noise_within_the_bound_of_a_tree(case):
    """S_k is 2^k - 1 rounded adds, each off by at most half an ulp of a partial sum that is at most sum
    |x|: |error| <= (2^k - 1) 2^-24 sum |x|.  A bound, not a measurement; checked on every level, rebuilt as
    the twin builds it, against the window summed in float64 (whose own error, a few 2^-53 sum |x|, is
    allowed for)."""
    x = sps_cases.data(case, 'noise')
    x64 = x.astype(np.float64)
    s = x
    differs = False
    for k in range(case.K):
        w = 1 << k
        if x.shape[0] < w:
            break
        windows = np.lib.stride_tricks.sliding_window_view(x64, w, axis=0)
        want, mag = windows.sum(axis=-1), np.abs(windows).sum(axis=-1)
        assert s.shape == want.shape
        assert (np.abs(s - want) <= ((w - 1) * 2. ** -24 + 2. ** -48) * mag).all()
        differs = differs or bool((s != want.astype(np.float32)).any())
        if s.shape[0] <= w:
            break
        s = s[:-w] + s[w:]
    if case.K > 3:
        assert differs                                         # (so the order does matter for these data)
    assert np.isfinite(sps_cases.expected(case, 'noise')).all()


def test_twin_winner_is_the_level_sum_times_the_scale():
    case = sps_cases.by_name('ragged')
    x = sps_cases.data(case, 'noise')
    got = sps_cases.expected(case, 'noise')
    levels = [x]
    for k in range(case.K - 1):
        levels.append(levels[-1][:-(1 << k)] + levels[-1][1 << k:])
    for b in (0, 7, got.shape[0] - 1):
        for e in (0, 33, 66):
            snr, off, k = got[b, :, e]
            i = b * case.n + int(off)
            assert snr == levels[int(k)][i, e] * search.BOXCAR_SCALES[int(k)]
            every = [lv[b * case.n:(b + 1) * case.n, e] * search.BOXCAR_SCALES[j] for j, lv in enumerate(levels)]
            assert snr == max(v.max() for v in every)


def test_scales():
    c = search.BOXCAR_SCALES
    assert c.dtype == np.float32 and c.shape == (13,) and (search.SNR, search.OFFSET, search.WIDTH) == (0, 1, 2)
    for k in range(0, 13, 2):
        assert c[k] == 2. ** (-(k // 2))                       # exact for even k
    for k in range(13):
        assert c[k] == np.float32(2.0 ** (-k / 2))
        assert abs(float(c[k]) ** 2 * 2 ** k - 1.) < 2. ** -23
    assert c[1].view(np.uint32) == 0x3F3504F3


def test_twin_refusals():
    x = np.zeros((20, 2), np.float32)
    with pytest.raises(TypeError):
        search.boxcar_search_samples(x.astype(np.float64), 5, 3)
    with pytest.raises(TypeError):
        search.boxcar_search_samples(x.astype(np.complex64), 5, 3)
    for n, k in ((0, 3), (65537, 3), (5, 0), (5, 14), (21, 3)):
        with pytest.raises(ValueError):
            search.boxcar_search_samples(x, n, k)
    assert search.boxcar_search_samples(x, 20, 13).shape == (1, 3, 2)       # (levels beyond the stream: none fit)
    with pytest.raises(TypeError):
        search.standardize_samples(x.astype(np.float64), 5)
    for n in (1, 65537):
        with pytest.raises(ValueError):
            search.standardize_samples(x, n)


# -- the standardize twin ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sps_cases.STD_BLOCKS)
def test_standardize_twin_against_float64(n):
    x = sps_cases.std_data()
    got = sps_cases.std_expected(n)
    nb = sps_cases.STD_N // n
    assert got.dtype == np.float32 and got.shape == (nb * n,) + sps_cases.STD_S
    blocks = x[:nb * n].astype(np.float64).reshape(nb, n, -1)
    with np.errstate(all='ignore'):
        mean, sd = blocks.mean(axis=1, keepdims=True), blocks.std(axis=1, keepdims=True)
        want = (blocks - mean) / sd
    z = got.reshape(nb, n, -1)
    noise = np.arange(6, 67)
    # 1e-6 relative to the value's own scale, 1 + |want|: the two float32 roundings and that of 1 / sd are a few
    # 2^-24 of it.  The mean is rounded to float32 too, which moves every value of the block by up to 2^-24
    # |mean| / sd: nothing for a long block, but a block of two nearly equal samples has an sd as small as
    # one likes, so that term of the number format is allowed for by name.
    with np.errstate(all='ignore'):
        slack = 2. ** -24 * np.abs(mean) / sd
    off = np.abs(z[:, :, noise] - want[:, :, noise])
    assert (off <= 1e-6 * (1. + np.abs(want[:, :, noise])) + slack[:, :, noise]).all()
    if n >= 31:
        assert (off <= 1e-6 * (1. + np.abs(want[:, :, noise]))).all()
        z64 = z[:, :, noise].astype(np.float64)
        assert abs(z64.mean()) < 1e-6 and abs(z64.std() - 1.) < 1e-6
    # the degenerate blocks: constant, all zero, -0 -> +0; a NaN or an Inf -> +0 for that block only
    for col in (0, 1, 4):
        assert not z[:, :, col].view(np.uint32).any()
    nan_blocks = {7 // n, 1500 // n} & set(range(nb))
    for b in range(nb):
        zero = not z[b, :, 2].view(np.uint32).any()
        assert zero == (b in nan_blocks)
        assert (not z[b, :, 3].view(np.uint32).any()) == (b == 40 // n)
    assert np.isfinite(got).all()
    # a constant that is no dyadic fraction: whatever the rule gives, which is +0 or finite
    assert np.isfinite(z[:, :, 5]).all()


def test_standardize_twin_step_by_step():
    """One block of 70 samples by hand: three segments (32, 32, 6), each step rounded once."""
    rng = np.random.default_rng(3)
    x = (2. + rng.standard_normal((70, 1))).astype(np.float32)
    d = x[:, 0].astype(np.float64)
    s1 = s2 = 0.
    for t0 in (0, 32, 64):
        a1 = a2 = 0.
        for v in d[t0:t0 + 32]:
            a1 = a1 + v
            a2 = a2 + v * v
        s1, s2 = s1 + a1, s2 + a2
    mean = s1 / 70.
    var = s2 / 70. - mean * mean
    r = 1. / np.sqrt(var)
    want = (x[:, 0] - np.float32(mean)) * np.float32(r)
    got = search.standardize_samples(x, 70)
    assert got.dtype == np.float32 and (got[:, 0].view(np.uint32) == want.view(np.uint32)).all()
    # a tail is dropped
    assert search.standardize_samples(np.concatenate([x, x[:5]]), 70).shape == (70, 1)


# -- candidates -------------------------------------------------------------------------------------------
def _best(snr, off=None, k=None):
    snr = np.asarray(snr, np.float32)
    best = np.zeros((snr.shape[0], 3, snr.shape[1]), np.float32)
    best[:, SNR] = snr
    best[:, OFFSET] = 0 if off is None else off
    best[:, WIDTH] = 0 if k is None else k
    return best


def test_candidates_on_a_hand_made_plane():
    snr = np.zeros((5, 6))
    snr[0, 5] = 9.                       # an edge cell (a corner): 3 neighbours
    snr[2, 1:4] = 8.                     # a plateau of three equal cells: the first in raster order
    snr[3, 2] = 8.                       # ... which also touches the plateau from the next row
    snr[4, 5] = 7.                       # exactly the threshold
    snr[4, 0] = 6.999                    # just below
    off = np.arange(30).reshape(5, 6) % 10
    k = (np.arange(30).reshape(5, 6) % 4)
    cands = search.boxcar_candidates(_best(snr, off, k), 10, 7.)
    assert cands.dtype.names == ('sample', 'trial', 'width', 'snr')
    assert cands['sample'].dtype == np.int64 and cands['snr'].dtype == np.float32
    assert cands['snr'].tolist() == [9., 8., 7.]
    assert cands['trial'].tolist() == [5, 1, 5]
    assert cands['sample'].tolist() == [0 * 10 + 5, 2 * 10 + 3, 4 * 10 + 9]
    assert cands['width'].tolist() == [2 ** (5 % 4), 2 ** (13 % 4), 2 ** (29 % 4)]
    # the threshold is inclusive; above every value nothing is left
    assert len(search.boxcar_candidates(_best(snr), 10, 6.999)) == 4
    assert len(search.boxcar_candidates(_best(snr), 10, 9.5)) == 0
    # equal candidates sort by sample, then trial
    two = np.zeros((4, 4))
    two[3, 0] = two[0, 3] = two[0, 0] = 5.
    c = search.boxcar_candidates(_best(two), 3, 1.)
    assert list(zip(c['sample'].tolist(), c['trial'].tolist())) == [(0, 0), (0, 3), (9, 0)]
    # a plateau that fills the plane has one candidate, its first cell
    c = search.boxcar_candidates(_best(np.full((3, 3), 4.)), 2, 4.)
    assert len(c) == 1 and (c['sample'][0], c['trial'][0]) == (0, 0)
    with pytest.raises(ValueError):
        search.boxcar_candidates(np.zeros((4, 2, 3), np.float32), 2, 1.)
    with pytest.raises(ValueError):
        search.boxcar_candidates(np.zeros((4, 3), np.float32), 2, 1.)


def test_candidates_of_a_twin_result():
    x = np.zeros((1024, 9), np.float32)
    x[300:308, 4] = 3.
    best = search.boxcar_search_samples(x, 256, 8)
    c = search.boxcar_candidates(best, 256, 7.)
    assert len(c) == 1
    assert (c['sample'][0], c['trial'][0], c['width'][0]) == (300, 4, 8) and c['snr'][0] == 24 * search.BOXCAR_SCALES[3]


# -- construction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_boxcar_stream_surface(case):
    sh = sps_cases.stream(case)
    bs = bt.BoxcarSearch(sh, case.n, case.K)
    assert bs.shape == (case.N // case.n, 3) + case.s and bs.dtype == np.float32
    assert bs.sample_rate == RATE / case.n and bs.samples_per_frame == 1
    assert abs(bs.start_time - bt.Time(T0)) < 1e-9
    assert bs.n == case.n and bs.n_widths == case.K
    assert bs.frequency == 600e6 and bs.sideband == 1
    assert bt.BoxcarSearch(sh, case.n, case.K, samples_per_frame=3).samples_per_frame == 3
    text = repr(bs)
    assert text.startswith('BoxcarSearch(ih') and 'ih: HostStream' in text
    # what the uploader is told: the blocks of the frames and the halo, cut at the end of the stream
    halo = 2 ** (case.K - 1) - 1
    assert bs._input_span(0, 1) == (sh, 0, min(case.N, case.n + halo))
    nb = case.N // case.n
    assert bs._input_span(nb - 1, nb) == (sh, (nb - 1) * case.n, min(case.N, nb * case.n + halo) - (nb - 1) * case.n)
    bs.close()
    assert bs.closed
    assert bt.BoxcarSearch(sh, case.n).n_widths == 13


def test_standardize_stream_surface():
    sh = sps_cases.std_stream(samples_per_frame=100)
    for n in sps_cases.STD_BLOCKS:
        st = bt.Standardize(sh, n)
        assert st.shape == (sps_cases.STD_N // n * n,) + sps_cases.STD_S and st.dtype == np.float32
        assert st.sample_rate == RATE and abs(st.start_time - bt.Time(T0)) < 1e-9
        assert st.samples_per_frame == -(-100 // n) * n
        assert st.frequency == 600e6 and st.sideband == 1 and st.n == n
        assert repr(st).startswith('Standardize(ih')
    assert bt.Standardize(sh, 50, samples_per_frame=150).samples_per_frame == 150
    # the default frame is never longer than the output
    long_frames = sps_cases.std_stream(samples_per_frame=sps_cases.STD_N)
    assert bt.Standardize(long_frames, 1000).samples_per_frame == 2000
    for bad in (75, 25, 0):
        with pytest.raises(ValueError, match='multiple'):
            bt.Standardize(sh, 50, samples_per_frame=bad)


def test_metadata_of_a_plane_without_a_sideband_is_passed_on():
    """The plane of `DMTrials` has a frequency and no sideband; both tasks stack on it directly, and
    metadata that vary along the sample shape broadcast over the new axis."""
    x = np.zeros((300, 4), np.float32)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(sh, [0., .1, .2])
    assert plane.shape[1:] == (3,)
    st = bt.Standardize(plane, 50)
    bs = bt.BoxcarSearch(st, 25, 4)
    for task in (st, bs):
        assert task.frequency == plane.frequency
        with pytest.raises(AttributeError):
            task.sideband
    assert bs.shape == (st.shape[0] // 25, 3, 3)
    pol = np.array(['X', 'Y', 'X', 'Y'])
    ph = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=np.linspace(4e8, 8e8, 4), sideband=np.array([1, -1, 1, -1]),
                       polarization=pol)
    bs = bt.BoxcarSearch(ph, 10, 2)
    np.testing.assert_array_equal(np.broadcast_to(bs.frequency, (3, 4))[2], np.linspace(4e8, 8e8, 4))
    np.testing.assert_array_equal(np.broadcast_to(bs.sideband, (3, 4))[1], [1, -1, 1, -1])
    np.testing.assert_array_equal(np.broadcast_to(bs.polarization, (3, 4))[0], pol)


def test_what_is_refused():
    x = np.zeros((100, 3), np.float32)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False)
    z = bt.HostStream(x.astype(np.complex64), bt.Time(T0), RATE, pin=False)
    f64 = bt.HostStream(x.astype(np.float64), bt.Time(T0), RATE, pin=False)
    for cls, args in ((bt.Standardize, (10,)), (bt.BoxcarSearch, (10, 3))):
        with pytest.raises(TypeError, match='Square'):
            cls(z, *args)
        with pytest.raises(TypeError, match='float32'):
            cls(f64, *args)
        with pytest.raises(ValueError, match='less than one block'):
            cls(sh, 101, *args[1:])
        cls(sh, 100, *args[1:])
        with pytest.raises(ValueError, match='block'):
            cls(sh, 65537, *args[1:])
    with pytest.raises(ValueError, match='block'):
        bt.Standardize(sh, 1)
    with pytest.raises(ValueError, match='block'):
        bt.BoxcarSearch(sh, 0)
    bt.BoxcarSearch(sh, 1)
    for k in (0, 14, -1):
        with pytest.raises(ValueError, match='n_widths'):
            bt.BoxcarSearch(sh, 10, k)
    with pytest.raises(TypeError):
        bt.BoxcarSearch(sh, 10.5)
    assert (hip.SPS_MAX_N, hip.SPS_MAX_WIDTHS) == (65536, 13)


def test_library_exports_the_search():
    lib = hip.lib()
    assert lib.bbt_version() >= 164
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_sps_standardize', 'bbt_sps_plan_create', 'bbt_sps_plan_destroy', 'bbt_sps_plan_info',
                 'bbt_sps_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'sps_geo.hpp')).read()
    assert f'#define BBT_SPS_MAX_N {hip.SPS_MAX_N}' in geo and f'#define BBT_SPS_MAX_WIDTHS {hip.SPS_MAX_WIDTHS}' in geo
    assert f'#define BBT_SPS_SEG {search.SEGMENT}' in geo
    assert all(name in bt.search.__all__ and hasattr(bt, name) for name in
               ('Standardize', 'BoxcarSearch', 'standardize_samples', 'boxcar_search_samples', 'boxcar_candidates'))
    # the library's scales are the twin's (no device needed to ask)
    info = hip.sps_info()
    assert info['scales'].view(np.uint32).tolist() == search.BOXCAR_SCALES.view(np.uint32).tolist()
    assert (info['width'], info['fuse'], info['split'], info['std_rows']) == (64, 2, 16, 8)


# -- the tiling, on the host ----------------------------------------------------------------------------------
def _geo_shapes():
    """(kind, ...): every shared case under every tiling the tests walk and cut into the chunks the
    tests make, the limits, and chunks of more than 2^31 values."""
    shapes = []
    for case in CASES:
        e = int(np.prod(case.s, dtype=int))
        nb = case.N // case.n
        halo = 2 ** (case.K - 1) - 1
        for width, fuse, split in [(0, 0, 0)] + sps_cases.TILINGS:
            shapes.append((0, case.N, nb, case.n, case.K, e, width, fuse, split))
            # a chunk in the middle (its halo is all there) and the last one (cut by the stream)
            if nb > 3:
                shapes.append((0, min(case.N, 3 * case.n + halo), 3, case.n, case.K, e, width, fuse, split))
                shapes.append((0, case.N - (nb - 1) * case.n, 1, case.n, case.K, e, width, fuse, split))
    shapes += [(0, 1, 1, 1, 1, 1, 0, 0, 0), (0, 1, 1, 1, 13, 1, 0, 0, 0), (0, 70000, 1, 65536, 13, 3, 64, 3, 16),
               (0, 65536, 1, 65536, 13, 1, 16, 1, 16), (0, 5000, 5000, 1, 13, 2, 16, 1, 1),
               # more than 2^31 values in the chunk and in each scratch
               (0, (1 << 16) * 64 + 4095, 1 << 16, 64, 13, 1024, 64, 2, 4), (0, 1 << 22, 1 << 14, 256, 10, 515, 32, 3, 8)]
    for n in sps_cases.STD_BLOCKS:
        for rows in (0, 1, 2, 4, 8, 16):
            shapes.append((1, sps_cases.STD_N // n, n, 67, rows, 0, 0, 0, 0))
    shapes += [(1, 1, 2, 1, 0, 0, 0, 0, 0), (1, 1, 65536, 300, 16, 0, 0, 0, 0), (1, 1 << 14, 256, 1024, 8, 0, 0, 0, 0)]
    return shapes


def test_kernel_tiling_on_the_host(tmp_path):
    """Every (block, part, element tile) owned by exactly one row of threads in every pass, every read
    inside [0, n_in) of the chunk and inside what the pass before stored, every level stored on exactly
    the rows it is defined on, the limits and refusals: the program exits non-zero otherwise, and the
    sanitizers abort it on a wild index or an overflow of its own."""
    exe = compile_check('sps_geo_check', tmp_path)
    shapes = _geo_shapes()
    plans = run_check(exe, shapes)
    scales = search.BOXCAR_SCALES.view(np.uint32).tolist()
    for shape, g in zip(shapes, plans):
        assert g['walk'] == 0, (shape, g)
        if shape[0] == 0:
            _, n_in, nb, n, K, e, width, fuse, split = shape
            assert g['n_in'] == min(n_in, nb * n + 2 ** (K - 1) - 1) and g['nbv'] == -(-g['n_in'] // n)
            assert g['nx'] == (width or 64) and g['fuse'] == (fuse or 2) and g['n_pass'] == -(-K // g['fuse'])
            assert g['nx'] * g['ny'] == 256 and g['sub'] * g['nz'] == g['ny']
            assert g['sub'] == min(g['ny'], split or 16, 2 ** (n.bit_length() - 1))
            assert g['n_tile'] == -(-e // g['nx']) and g['scratch'] == min(g['n_pass'] - 1, 2) * g['n_in'] * e
            assert g['scales'] == scales
        else:
            _, n_block, n, e, rows = shape[:5]
            assert g['ny'] == (rows or 8) and g['nx'] * g['ny'] == 256
            assert g['n_tile'] == -(-e // g['nx']) and g['n_wg'] == n_block * g['n_tile']
    big = [g for s, g in zip(shapes, plans) if s[0] == 0 and s[1] * s[5] > 2 ** 31]
    assert len(big) == 2 and all(g['scratch'] > 2 ** 32 for g in big)
    # what the library refuses: one sample short, no blocks, n_widths 0 and 14, a block of 0 and of 65537, bad tilings
    bad = run_raw(exe, '0 99 10 10 1 3 0 0 0  0 100 0 10 1 3 0 0 0  0 100 10 10 0 3 0 0 0  0 100 10 10 14 3 0 0 0 '
                       '0 100 10 0 1 3 0 0 0  0 99999 1 65537 1 3 0 0 0  0 100 10 10 1 3 48 0 0 '
                       '0 100 10 10 1 3 0 4 0  0 100 10 10 1 3 0 0 3  1 3 1 5 0 0 0 0 0  1 0 2 5 0 0 0 0 0 '
                       '1 3 2 5 3 0 0 0 0')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 12
    assert 'shorter' in errors[0] and 'no output' in errors[1] and 'n_widths' in errors[2] and 'n_widths' in errors[3]
    assert '65536' in errors[4] and '65536' in errors[5] and 'width' in errors[6] and 'levels' in errors[7]
    assert 'split' in errors[8] and '2 ... 65536' in errors[9] and 'no whole block' in errors[10] and 'rows' in errors[11]
