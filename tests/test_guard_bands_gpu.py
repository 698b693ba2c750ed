"""The search-chain kernels between guard bands (tests/guard_bands.py): Modulate, SpectralKurtosis / Excise,
DMTrials, Standardize / BoxcarSearch, Whiten / HarmonicSearch, LongSpectra and Accelerate, each entry point
or plan called directly with EVERY device array it takes -- inputs, outputs, side tables -- inside bands of
poison, 16-byte aligned and 4 bytes off, under a NaN and under +inf.  Every run compares its payloads with
the family's twin under the family's own rule, then checks all bands; the run that is 4 bytes off must also
give the bits of the aligned one.  The cases are the ragged ones of the shared tables.

What stays outside: the scratch buffers the DMTrials, BoxcarSearch and LongSpectra plans own, and the run
and piece tables `hip.modulate_runs` / `hip.modulate_pieces` upload themselves."""
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, periodicity
from baseband_tasks_amd.fold_table import plan_pieces

import accel_cases
import dmt_cases
import hsum_cases
import lspec_cases
import sk_cases
import sps_cases
from guard_bands import INF_POISON, NAN_POISON, PAD, POISONS, SKEWS, Guarded, check_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLYCO = os.path.join(ROOT, 'tests', 'golden', 'B1937_polyco.dat')
F32, C64 = np.dtype(np.float32), np.dtype(np.complex64)

#: (skew varies fastest: the aligned run of a case is followed at once by the one 4 bytes off)
both_skews = pytest.mark.parametrize('skew', SKEWS, ids=['aligned16', 'off4'])
both_poisons = pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))

# the payloads of the latest aligned run, for the run 4 bytes off that follows it
_aligned = {}


def _words_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _across_skews(key, skew, run, same):
    """``run(skew)`` returns the payloads of one guarded run, already held to the twin and to its bands.  The
    run 4 bytes off is held to the aligned one (made here, if it is not the one that just ran)."""
    got = run(skew)
    if skew == 0:
        _aligned.clear()
        _aligned[key] = got
        return
    ref = _aligned.pop(key, None)
    if ref is None:
        ref = run(0)
    assert len(ref) == len(got)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert same(a, b), f'{key}: payload {i} of the run 4 bytes off differs from the aligned run'


# -- the helper itself ----------------------------------------------------------------------------------------
@both_poisons
@both_skews
@pytest.mark.parametrize('shape, dtype', [((5, 7), F32), ((3, 2, 2), C64), ((9, 4), np.dtype(np.uint8)), ((1,), F32)])
def test_helper_catches_a_word_on_either_side(shape, dtype, skew, poison):
    """No kernel of the project runs: plain copies inside the allocation stand for the stray store."""
    _helper_catches(shape, dtype, skew, poison)


#: skews that are multiples of the item size and not of 4 (the gather plans' one- and two-byte elements), and 8 / 12
ELEMENT_SKEWS = [((9, 4), np.dtype(np.uint8), 1), ((9, 4), np.dtype(np.uint8), 2), ((9, 4), np.dtype(np.uint8), 3),
                 ((9, 4), np.dtype(np.uint8), 13), ((5, 2), np.dtype(np.int16), 2), ((5, 2), np.dtype(np.int16), 6),
                 ((5, 2), np.dtype(np.int16), 14), ((5, 7), F32, 8), ((5, 7), F32, 12), ((3, 2, 2), C64, 8),
                 ((1,), F32, 12), ((2, 3), np.dtype(np.complex128), 8)]


@both_poisons
@pytest.mark.parametrize('shape, dtype, skew', ELEMENT_SKEWS, ids=[f'{d.name}-off{s}' for _, d, s in ELEMENT_SKEWS])
def test_helper_catches_a_word_at_element_skews(shape, dtype, skew, poison):
    """The same at every other kind of skew `Guarded` takes; the band before the payload ends with a whole word."""
    _helper_catches(shape, dtype, skew, poison)
    g = Guarded(shape, dtype, poison, skew)
    assert g.front_bytes == 4 * g.front + skew % 4 and g.array.ptr - g.base.ptr == g.front_bytes
    before = g.base.to_host()[g.front_bytes - 4:g.front_bytes].view(np.uint32)[0]
    assert before == (0xa5a5a5a5 if dtype.itemsize == 1 else poison)
    with pytest.raises(AssertionError):
        Guarded(shape, dtype, poison, skew + 1 if dtype.itemsize > 1 else 16)


def _helper_catches(shape, dtype, skew, poison):
    g = Guarded(shape, dtype, poison, skew)
    assert g.array.ptr % 16 == skew and g.array.shape == shape and g.array.dtype == dtype
    assert min(g.front, g.back) * 4 >= g.row_bytes + 4 * PAD
    fresh = g.check('fresh')
    assert fresh.shape == shape and fresh.dtype == dtype
    filled = 0xa5a5a5a5 if dtype.itemsize == 1 else poison
    assert (fresh.reshape(-1).view(np.uint8)[:g.nbytes // 4 * 4].view(np.uint32) == filled).all()
    n = -(-g.nbytes // 4)                                   # words of the payload (the last one may be partial)
    # n + 1 words from the payload's first: one word past the end
    hip.DeviceArray((n + 1,), np.uint32, ptr=g.array.ptr, owner=g.base).copy_from_host(np.zeros(n + 1, np.uint32))
    with pytest.raises(AssertionError, match=rf'past the payload: word {n}\b'):
        g.check('one past')
    # and one word before it
    g = Guarded(shape, dtype, poison, skew)
    hip.DeviceArray((n + 1,), np.uint32, ptr=g.array.ptr - 4, owner=g.base).copy_from_host(np.zeros(n + 1, np.uint32))
    with pytest.raises(AssertionError, match=r'before the payload: word -1, row -1\b'):
        g.check('one before')
    # a whole row beyond the end is still inside the band
    g = Guarded(shape, dtype, poison, skew)
    row = -(-g.row_bytes // 4)
    at = g.array.ptr + 4 * (n + row)
    hip.DeviceArray((1,), np.uint32, ptr=at, owner=g.base).copy_from_host(np.zeros(1, np.uint32))
    with pytest.raises(AssertionError, match=rf'past the payload: word {n + row}\b'):
        g.check('a row past')
    # loading data that hold the poison is refused, unless the caller says how often they plant it
    data = np.zeros(shape, dtype)
    if dtype.itemsize == 1:
        data.reshape(-1)[-1] = 0xa5
    else:
        data.reshape(-1).view(np.uint32)[-1] = poison
    with pytest.raises(AssertionError, match='holds the poison'):
        Guarded.load(data, poison, skew)
    g = Guarded.load(data, poison, skew, planted=1)
    assert _words_equal(g.check('loaded'), data)


# -- Modulate -------------------------------------------------------------------------------------------------
#: (dtype, sample shape, samples): some 12300 floats each, three tiles of 16-byte accesses or twelve of 4-byte
#: ones; float counts 0, 1, 2 and 3 modulo 4 (the tail that goes with the last tile); 1, 3 and 5 x 2 elements
MOD_CASES = [(F32, (), 12289), (F32, (), 12290), (F32, (), 12291), (F32, (), 12292), (F32, (3,), 4099),
             (F32, (3,), 4101), (C64, (), 6147), (C64, (3,), 2050), (C64, (3,), 2051), (F32, (5, 2), 1231),
             (F32, (5, 2), 1230), (C64, (5, 2), 615)]
MOD_IDS = [f'{d.name}-{"x".join(map(str, s)) or "scalar"}-{n}' for d, s, n in MOD_CASES]
MOD_PHASES = 7
assert sorted({n * int(np.prod(s, dtype=int)) * (2 if d == C64 else 1) % 4 for d, s, n in MOD_CASES}) == [0, 1, 2, 3]


def _mod_data(dtype, sample_shape, n, seed=41):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n,) + sample_shape).astype(np.float32)
    if dtype == C64:
        x = (x + 1j * rng.standard_normal(x.shape).astype(np.float32)).astype(np.complex64)
    return x


def _mod_gain(per_element, n_phase, sample_shape, seed=43):
    """(profile for the twin, gains for the device): a gain per bin, or per bin and element."""
    rng = np.random.default_rng(seed)
    n_elem = int(np.prod(sample_shape, dtype=int))
    if not per_element:
        profile = rng.uniform(-2., 2., n_phase).astype(np.float32)
        return profile, profile
    profile = rng.uniform(-2., 2., (n_phase,) + sample_shape).astype(np.float32)
    return profile, profile.reshape(n_phase, n_elem)


def _mod_runs(n, fps):
    """Runs that tile [0, n): 1 ... 7 samples long in the first twentieth and the last quarter, and one run
    over the 70 % between, which holds a whole tile whatever the access width."""
    rng = np.random.default_rng(n)
    a, b = n // 20, n - n // 4
    assert (b - a) * fps >= 2 * 4 * 1024                      # (two tiles of 1024 accesses of 4 floats)
    head = np.cumsum(rng.integers(1, 8, a))
    tail = b + np.cumsum(rng.integers(1, 8, n - b))
    begin = np.concatenate([[0], head[head < a], [a], [b], tail[tail < n]]).astype(np.int64)
    assert begin[0] == 0 and (np.diff(begin) > 0).all() and begin[-1] < n
    return begin, rng.integers(0, MOD_PHASES, begin.shape[0]).astype(np.int64)


def _mod_run(entry, x, profile, gain, bins, poison, skew, what):
    gx, gg = Guarded.load(x, poison, skew), Guarded.load(gain, poison, skew)
    go = Guarded(x.shape, x.dtype, poison, skew)
    entry(gx.array, go.array, gg.array)
    got_x, got, got_g = check_all([gx, go, gg], what)
    np.testing.assert_array_equal(got, bt.modulate_samples(x, profile, bins))
    assert _words_equal(got_x, x) and _words_equal(got_g, gain)
    return (got,)


@both_poisons
@both_skews
@pytest.mark.parametrize('per_element', [False, True], ids=['per_bin', 'per_element'])
@pytest.mark.parametrize('case', MOD_CASES, ids=MOD_IDS)
def test_modulate_runs(case, per_element, skew, poison):
    dtype, sample_shape, n = case
    x = _mod_data(dtype, sample_shape, n)
    n_elem = int(np.prod(sample_shape, dtype=int))
    profile, gain = _mod_gain(per_element, MOD_PHASES, sample_shape)
    begin, run_bin = _mod_runs(n, n_elem * (2 if dtype == C64 else 1))
    bins = np.repeat(run_bin, np.diff(np.append(begin, n)))

    def run(s):
        return _mod_run(lambda i, o, g: hip.modulate_runs(i, o, n_elem, g, begin, run_bin), x, profile, gain, bins,
                        poison, s, f'modulate_runs {MOD_IDS[MOD_CASES.index(case)]}')
    _across_skews(('modulate_runs', case, per_element, poison), skew, run, _words_equal)


@both_poisons
@both_skews
@pytest.mark.parametrize('per_element', [False, True], ids=['per_bin', 'per_element'])
@pytest.mark.parametrize('case', [MOD_CASES[i] for i in (0, 2, 5, 7, 8, 11)], ids=[MOD_IDS[i] for i in (0, 2, 5, 7, 8, 11)])
def test_modulate_pieces(case, per_element, skew, poison):
    """The pieces plan made as `Modulate` makes it, from a polyco whose closest entry changes half a second
    into the stream: two pieces."""
    dtype, sample_shape, n = case
    x = _mod_data(dtype, sample_shape, n, seed=47)
    n_elem, n_phase = int(np.prod(sample_shape, dtype=int)), 64
    profile, gain = _mod_gain(per_element, n_phase, sample_shape)
    pp = bt.phases.PolycoPhase(POLYCO)
    sh = bt.HostStream(x, bt.Time('2018-05-06T22:57:35.5'), float(n), samples_per_frame=n, pin=False)
    mh = bt.Modulate(sh, profile, pp)
    assert len(pp.fold_pieces(mh.start_time, mh.sample_rate, 0, n)) == 2
    edges = mh._frame_edges(0, n)
    plan = plan_pieces(edges, mh._row_pieces(edges), n_phase, 0, n)[2]
    bins = mh.bins(0, n)
    assert len(plan['row']) == 2 and len(set(bins.tolist())) == n_phase

    def run(s):
        return _mod_run(lambda i, o, g: hip.modulate_pieces(i, o, n_elem, g, plan), x, profile, gain, bins, poison, s,
                        f'modulate_pieces {MOD_IDS[MOD_CASES.index(case)]}')
    _across_skews(('modulate_pieces', case, per_element, poison), skew, run, _words_equal)


# -- SpectralKurtosis / Excise --------------------------------------------------------------------------------
SK_NAMES = ['narrow_pol_pairs', 'odd_width_f32', 'above_a_segment', 'columns_not_a_tile', 'prime_width_f32',
            'group_of_three', 'minimum_n']


@both_poisons
@both_skews
@pytest.mark.parametrize('name', SK_NAMES)
def test_sk_estimate_and_excise(name, skew, poison):
    case = sk_cases.CASES[sk_cases.IDS.index(name)]
    n_block, n_elem = case.samples // case.n, int(np.prod(case.sample_shape, dtype=int))
    group = int(np.prod(case.sample_shape[len(case.sample_shape) - case.join:], dtype=int))
    x = sk_cases.data(case)[:n_block * case.n]
    sk, flags, out = sk_cases.expected(case)

    def run(s):
        # complex64 samples must be aligned to their elements (include/bbt_hip.h): 8 bytes off, not 4
        sx = 2 * s if case.dtype == C64 else s
        gx, go = Guarded.load(x, poison, sx), Guarded(x.shape, x.dtype, poison, sx)
        gsk = Guarded((n_block, n_elem), F32, poison, s)
        gflags = Guarded((n_block, n_elem // group), np.uint8, poison, s)
        gest = Guarded((n_block, n_elem), F32, poison, s)
        assert gx.array.ptr % 16 == go.array.ptr % 16 == sx
        hip.sk_excise(gx.array, go.array, case.n, n_elem, sk_cases.limits_of(case), case.averaged, group,
                      sk=gsk.array, flags=gflags.array)
        hip.sk_estimate(gx.array, case.n, n_elem, case.averaged, out=gest.array)
        got_x, got, got_sk, got_flags, got_est = check_all([gx, go, gsk, gflags, gest], f'sk {name}')
        assert sk_cases.same_bits(got, out) and _words_equal(got_x, x)
        assert sk_cases.same_bits(got_sk.reshape(sk.shape), sk) and sk_cases.same_bits(got_est.reshape(sk.shape), sk)
        np.testing.assert_array_equal(got_flags.reshape(flags.shape), flags.astype(np.uint8))
        return got, got_sk, got_flags, got_est
    _across_skews(('sk', name, poison), skew, run, sk_cases.same_bits)


# -- DMTrials -------------------------------------------------------------------------------------------------
@both_poisons
@both_skews
@pytest.mark.parametrize('name', ['narrow', 'tile_edges', 'wide_span', 'many_dm', 'trailing'])
def test_dmt_plan(name, skew, poison):
    """The input is exactly n_out + span rows long: the last output row reads the last input row."""
    case = dmt_cases.by_name(name)
    x, want = dmt_cases.data(case, 'noise'), dmt_cases.expected(case, 'noise')
    shifts = dmt_cases.shifts(case)
    plan = hip.DmtPlan(shifts.max() - shifts, int(np.prod(case.rest, dtype=int)))
    n_out = x.shape[0] - plan.span
    assert want.shape == (n_out, len(case.dms)) + case.rest and plan.span == int(np.ptp(shifts))

    def run(s):
        gx, go = Guarded.load(x, poison, s), Guarded(want.shape, F32, poison, s)
        plan.execute(gx.array, x.shape[0], go.array, n_out)
        got_x, got = check_all([gx, go], f'dmt {name}')
        assert dmt_cases.same_bits(got, want) and _words_equal(got_x, x)
        return (got,)
    _across_skews(('dmt', name, poison), skew, run, dmt_cases.same_bits)
    plan.close()


# -- Standardize / BoxcarSearch -------------------------------------------------------------------------------
@both_poisons
@both_skews
@pytest.mark.parametrize('n', [31, 33, 1000])
def test_sps_standardize(n, skew, poison):
    x, want = sps_cases.std_data(), sps_cases.std_expected(n)

    def run(s):
        gx = Guarded.load(x, poison, s, planted=int(poison == INF_POISON))      # (std_data plants one Inf)
        go = Guarded(want.shape, F32, poison, s)
        hip.sps_standardize(gx.array, n, x.shape[1], out=go.array)
        got_x, got = check_all([gx, go], f'standardize {n}')
        assert sps_cases.same_bits(got, want) and _words_equal(got_x, x)
        return (got,)
    _across_skews(('standardize', n, poison), skew, run, sps_cases.same_bits)


@both_poisons
@both_skews
@pytest.mark.parametrize('kind', sps_cases.KINDS)
@pytest.mark.parametrize('tiling', [None, (16, 3, 16)], ids=['default', '16-3-16'])
@pytest.mark.parametrize('name', ['ragged', 'long_halo', 'just_fits', 'single_sample_blocks'])
def test_sps_plan(name, tiling, kind, skew, poison, monkeypatch):
    case = sps_cases.by_name(name)
    if tiling is not None:
        for key, value in zip(('BBT_SPS_WIDTH', 'BBT_SPS_FUSE', 'BBT_SPS_SPLIT'), tiling):
            monkeypatch.setenv(key, str(value))
    x, want = sps_cases.data(case, kind), sps_cases.expected(case, kind)
    plan = hip.SpsPlan(case.n, case.K, int(np.prod(case.s, dtype=int)))
    info = plan.info()
    assert tiling is None or (info['width'], info['fuse'], info['split']) == tiling
    nb = case.N // case.n

    def run(s):
        gx, go = Guarded.load(x, poison, s), Guarded(want.shape, F32, poison, s)
        plan.execute(gx.array, case.N, go.array, nb)
        got_x, got = check_all([gx, go], f'boxcar {name}')
        assert sps_cases.same_bits(got, want) and _words_equal(got_x, x)
        return (got,)
    _across_skews(('boxcar', name, tiling, kind, poison), skew, run, sps_cases.same_bits)
    plan.close()


# -- Whiten / HarmonicSearch ----------------------------------------------------------------------------------
@both_poisons
@both_skews
@pytest.mark.parametrize('skip', [0, 5])
@pytest.mark.parametrize('m', [31, 33, 1000])
def test_hsum_whiten(m, skip, skew, poison):
    x, want = hsum_cases.wh_data(), hsum_cases.wh_expected(m, skip)

    def run(s):
        gx = Guarded.load(x, poison, s, planted=int(poison == INF_POISON))      # (wh_data plants one Inf)
        go = Guarded(want.shape, F32, poison, s)
        hip.hsum_whiten(gx.array, x.shape[1], x.shape[2], m, skip, out=go.array)
        got_x, got = check_all([gx, go], f'whiten {m} {skip}')
        assert hsum_cases.same_bits(got, want) and _words_equal(got_x, x)
        return (got,)
    _across_skews(('whiten', m, skip, poison), skew, run, hsum_cases.same_bits)


#: k_hsum_search<5>, <6>, <5>, and the two cases that alone reach <2> and <3>
HSUM_NAMES = ['ragged', 'rfft', 'single_bin_blocks', 'two_levels', 'three_levels']


@both_poisons
@both_skews
@pytest.mark.parametrize('kind', hsum_cases.KINDS)
@pytest.mark.parametrize('name', HSUM_NAMES)
def test_hsum_plan(name, kind, skew, poison):
    case = hsum_cases.by_name(name)
    assert (hsum_cases.by_name('two_levels').K, hsum_cases.by_name('three_levels').K) == (2, 3)
    x, want = hsum_cases.data(case, kind), hsum_cases.expected(case, kind)
    plan = hip.HsumPlan(case.nbin, case.n, case.K, case.lo, int(np.prod(case.s, dtype=int)),
                        periodicity.harmonic_scales(hsum_cases.AVERAGED))
    assert want.shape == (case.N, plan.n_blocks, 3) + case.s

    def run(s):
        gx, go = Guarded.load(x, poison, s), Guarded(want.shape, F32, poison, s)
        plan.execute(gx.array, case.N, go.array)
        got_x, got = check_all([gx, go], f'hsum {name}')
        assert hsum_cases.same_bits(got, want) and _words_equal(got_x, x)
        return (got,)
    _across_skews(('hsum', name, kind, poison), skew, run, hsum_cases.same_bits)
    plan.close()


# -- LongSpectra ----------------------------------------------------------------------------------------------
@both_poisons
@both_skews
@pytest.mark.parametrize('name, budget', [('2^15x1', 0), ('2^16x5', 0), ('2^15x6_stack3', 0), ('2^15x6_stack3', 1)])
def test_lspec_plan(name, budget, skew, poison):
    """A lone column with a zero partner; an odd count; and a stack of three (the last pass adds to `out` in
    place) with a dropped tail, under the default budget and one column pair a launch."""
    case = lspec_cases.by_name(name)
    x, want = lspec_cases.data(case), lspec_cases.expected(case)
    n = 1 << case.log2n
    plan = hip.LongSpectraPlan(n, case.stack, case.n_elem)
    assert budget == 0 or plan.info(budget)['pairs_per_launch'] == 1
    assert x.shape[0] == case.nspec * case.stack * n + case.tail

    def run(s):
        gx, go = Guarded.load(x, poison, s), Guarded(want.shape, F32, poison, s)
        plan.execute(gx.array, case.nspec, go.array, budget)
        got_x, got = check_all([gx, go], f'lspec {name}')
        lspec_cases.assert_close(got, want, f'{name}, budget {budget}, {s} bytes off')
        assert _words_equal(got_x, x)
        return (got,)
    # a value depends on the samples of its column pair only: the same bits wherever the arrays lie
    _across_skews(('lspec', name, budget, poison), skew, run, lspec_cases.same_bits)
    plan.close()


# -- Accelerate -----------------------------------------------------------------------------------------------
#: with the rows wider than a tile: k_accel<unsigned, false> on grid.y = 2 (seg_scalar, at either offset) and
#: on grid.y = 5 (seg_wide, 4 bytes off), k_accel<uint4, false> on grid.y = 2 (seg_wide, aligned), and the
#: fence post of exactly one tile of 16-byte units, which may still take the window
ACCEL_NAMES = ['n64', 'n500', 'n512', 'n256_wide', 'seg_scalar', 'seg_wide', 'one_seg_wide']
#: under BBT_ACCEL_ROUTE 1 and 2; a segmented row goes direct whatever is asked (asserted below), so asking for
#: the window there would launch the same kernel again: these three cases are most of this file's time
ACCEL_RUNS = [(name, route) for name in ACCEL_NAMES for route in (1, 2)
              if route == 2 or name not in accel_cases.SEGMENTED]


@both_poisons
@both_skews
@pytest.mark.parametrize('name, route', ACCEL_RUNS)
def test_accel_plan(name, route, skew, poison, monkeypatch):
    monkeypatch.setenv('BBT_ACCEL_ROUTE', str(route))
    case = accel_cases.by_name(name)
    x, want = accel_cases.data(case), accel_cases.expected(case)
    n_elem, rows = int(np.prod(case.shape, dtype=int)), case.length // case.n * case.n
    plan = hip.AccelPlan(case.n, n_elem, case.factors)
    if name in accel_cases.SEGMENTED + (accel_cases.FENCE_POST,):
        assert plan.info(0, rows)['rows'] == 1
    if name in accel_cases.SEGMENTED:
        assert plan.info(0, rows)['route'] == 2
        assert -(-len(case.factors) * (n_elem // 4 if n_elem % 4 == 0 else n_elem) // hip.ACCEL_TILE_UNITS) == 2
    if name == accel_cases.FENCE_POST:
        assert len(case.factors) * n_elem // 4 == hip.ACCEL_TILE_UNITS

    def run(s):
        gx = Guarded.load(x, poison, s, planted=None)          # (accel_cases.SPECIALS holds +inf on purpose)
        go = Guarded(want.shape, F32, poison, s)
        plan.execute(gx.array, 0, case.length, go.array, 0, rows, n_rows=case.length)
        got_x, got = check_all([gx, go], f'accel {name}')
        assert accel_cases.same_words(got, want) and _words_equal(got_x, x)
        return (got,)
    _across_skews(('accel', name, route, poison), skew, run, accel_cases.same_words)
    plan.close()


@both_poisons
@both_skews
@pytest.mark.parametrize('route', [1, 2])
def test_accel_exact_window(route, skew, poison, monkeypatch):
    """A chunk that starts in the middle of a block, fed exactly the window `plan.info` reports for it: poison
    lies immediately before the first and after the last row a trial may read."""
    monkeypatch.setenv('BBT_ACCEL_ROUTE', str(route))
    case = accel_cases.by_name('n64')
    x, n = accel_cases.data(case), case.n
    first, count = n + 20, 30
    plan = hip.AccelPlan(n, 3, case.factors)
    info = plan.info(first, count)
    table = periodicity.accelerate_rows(n, case.factors)[:, 20:50]
    lo, hi = int(table.min()), int(table.max())
    assert (info['window_first'], info['window_rows']) == (n + lo, hi + 1 - lo) and lo < 20 and hi > 49
    piece = x[n + lo:n + hi + 1]
    want = accel_cases.expected(case)[first:first + count]

    def run(s):
        gx = Guarded.load(piece, poison, s, planted=None)
        go = Guarded(want.shape, F32, poison, s)
        plan.execute(gx.array, n + lo, hi + 1 - lo, go.array, first, count)
        got_x, got = check_all([gx, go], 'accel window')
        assert accel_cases.same_words(got, want) and _words_equal(got_x, piece)
        return (got,)
    _across_skews(('accel window', route, poison), skew, run, accel_cases.same_words)
    plan.close()


def test_the_poisons_are_what_they_are_named_for():
    assert np.isnan(np.array([NAN_POISON], np.uint32).view(np.float32)[0])
    assert np.array([INF_POISON], np.uint32).view(np.float32)[0] == np.inf
    assert NAN_POISON not in accel_cases.SPECIALS.tolist() and INF_POISON in accel_cases.SPECIALS.tolist()
