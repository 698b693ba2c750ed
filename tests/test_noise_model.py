"""tools/noise_model.py (the CPU restatement of csrc/noise_kernels.hpp) against NumPy, the
committed ziggurat tables against the running NumPy, and what the inputs of test_noise_gpu.py
exercise: the streams of noise_cases.CASES, and the frames with an explicit counter and the batch
under a finite guard that tools/noise_find_cases.py found."""
import os
import sys

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_model as nm            # noqa: E402
import make_zig_tables as mzt       # noqa: E402
import noise_cases as nc            # noqa: E402


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize('spf', [1, 7, 4096, 20000])
@pytest.mark.parametrize('sample_shape', [(), (2,), (3, 2)])
@pytest.mark.parametrize('dtype', [np.float32, np.complex64])
@pytest.mark.parametrize('seed', [0, 1, 12345])
def test_model_equals_noise_generator(seed, dtype, sample_shape, spf):
    far = 2**40 // spf                                   # a frame far into the stream
    frames = [0, far]
    got, flags = nm.stream_frames(seed, spf, sample_shape, dtype, frames)
    gen = bt.NoiseGenerator(((far + 1) * spf,) + sample_shape, nc.START, 1. * u.MHz, spf, dtype=dtype, seed=seed)
    for k, f in enumerate(frames):
        gen.seek(f * spf)
        assert same_bytes(got[k], gen.read(spf)), f'frame {f}'
    assert not flags.any()


def test_words_are_numpys():
    bg = np.random.Philox(5)
    st = bg.state
    st['state']['counter'][:] = [2**64 - 3, 77, 2**64 - 1, 5]       # (the carry runs through word 0)
    bg.state = st
    want = bg.random_raw(64)
    got = nm.philox_words(st['state']['key'], st['state']['counter'], 64)
    assert np.array_equal(got, want)


def test_word_count_formula():
    for n in (1, 7, 4096, 6006, 1 << 22):
        assert nm.word_count(n) == 4 * int(np.ceil((1.03 * n + 256) / 4 - 1e-9))
        assert nm.word_count(n) == bt.hip.noise_word_count(n)


def test_committed_tables_are_numpys_wi():
    assert same_bytes(nm.WI, mzt.probe_wi())


def test_committed_tables_are_numpys_ki():
    """ki[idx] is the smallest rabs that is not accepted at once: bisect on whether a second word
    was taken (buffer_pos after the call)."""
    for idx in range(256):
        lo, hi = 0, (1 << 52) - 1                        # (not direct at hi: every ki is below 2^52 - 1)
        assert mzt.probe_word(idx | hi << 9)[1] > 1
        while lo < hi:
            mid = (lo + hi) // 2
            if mzt.probe_word(idx | mid << 9)[1] > 1:
                hi = mid
            else:
                lo = mid + 1
        assert lo == int(nm.KI[idx]), idx


def test_committed_header_is_what_the_recipe_makes():
    ki, wi, fi, _ = mzt.find_tables()
    with open(mzt.HEADER) as f:
        assert f.read() == mzt.render(ki, wi, fi)


def test_shortfall_doubles_the_words():
    key = np.random.Philox(3).state['state']['key']
    full, total, flag = nm.frame(key, [0, 0, 0, 0], 5000)
    short, total_s, flag_s = nm.frame(key, [0, 0, 0, 0], 5000, n_words=4096)
    assert total >= 5000 and total_s < 5000 and not flag and not flag_s
    assert same_bytes(short[:total_s], full[:total_s])
    again, flags = nm.frames(key, [[0, 0, 0, 0]], 5000, n_words=4096)
    assert same_bytes(again[0], full)


def test_guard_flags_what_it_should():
    """An infinite guard calls every wedge and tail comparison ambiguous; the default one none of
    the inputs used on the GPU."""
    _, flags = nm.stream_frames(0, 4096, (), np.float32, [0, 1], guard=np.inf)
    assert flags.all()


@pytest.fixture(scope='module')
def case_paths():
    out = []
    for seed, spf, sample_shape, dtype, length in nc.CASES:
        stats = {}
        got, flags = nm.stream_frames(seed, spf, sample_shape, dtype, list(range(-(-length // spf))), stats=stats)
        out.append((got, flags, stats))
    return out


def test_gpu_inputs_match_numpy_and_raise_no_flag(case_paths):
    for case, (got, flags, _) in zip(nc.CASES, case_paths):
        length = case[4]
        want = nc.make(bt.NoiseGenerator, case).read()
        assert same_bytes(got.reshape((-1,) + got.shape[2:])[:length], want)
        assert not flags.any()


def test_gpu_inputs_exercise_every_path(case_paths):
    for expected, (_, _, stats) in zip(nc.EXPECTED_PATHS, case_paths):
        print(stats)
        assert {k: stats[k] for k in expected} == expected
    assert case_paths[0][2]['last_kinds'] == nc.EXPECTED_LAST_KINDS_CASE0
    total = {k: sum(e[k] for e in nc.EXPECTED_PATHS) for k in nc.EXPECTED_PATHS[0]}
    assert total['tail'] >= 1 and total['tail_reject'] >= 1 and total['wedge_straddle'] >= 1
    # frames span at least three tiles of words with n no multiple of 4
    assert any((spf * int(np.prod(ss, dtype=int)) * (2 if np.dtype(dt).kind == 'c' else 1)) % 4 != 0
               and nm.word_count(spf * int(np.prod(ss, dtype=int)) * (2 if np.dtype(dt).kind == 'c' else 1)) > 3 * nm.TILE
               for _, spf, ss, dt, _ in nc.CASES)


# ---------------------------------------------------------------------------------------------
# frames with an explicit counter (noise_cases.COUNTER_CASES) and the finite guard (GUARD_CASE)
import noise_find_cases as finder   # noqa: E402

CASE_NAMES = [c['name'] for c in nc.COUNTER_CASES]


@pytest.fixture(scope='module')
def counter_runs():
    """name -> (values, total, flag, stats) of the model, run once."""
    out = {}
    for c in nc.COUNTER_CASES:
        stats = {}
        got, total, flag = nm.frame(c['key'], c['counter'], c['n'], c['n_words'], stats=stats)
        out[c['name']] = (got, total, flag, stats)
    return out


def test_numpy_frame_is_the_stream_of_a_set_state():
    bg = np.random.Philox(5)
    st = bg.state
    st['state']['counter'][:] = [2**64 - 3, 77, 2**64 - 1, 5]
    bg.state = st
    want = np.random.Generator(bg).normal(size=100).astype(np.float32)
    assert same_bytes(nm.numpy_frame(st['state']['key'], st['state']['counter'], 100), want)
    # and, from counter 0 of a seed's key, the first frame of NoiseGenerator
    key = np.random.Philox(3).state['state']['key']
    gen = bt.NoiseGenerator((64,), nc.START, 1. * u.MHz, 64, dtype=np.float32, seed=3)
    assert same_bytes(nm.numpy_frame(key, [0, 0, 0, 0], 64), gen.read())


@pytest.mark.parametrize('name', CASE_NAMES)
def test_counter_case_equals_numpy_without_a_flag(name, counter_runs):
    c = nc.counter_case(name)
    got, total, flag, _ = counter_runs[name]
    assert same_bytes(got, nm.numpy_frame(c['key'], c['counter'], c['n']))
    assert not flag
    assert total >= c['n']                                 # the default number of words suffices: no second run


@pytest.mark.parametrize('name', CASE_NAMES)
def test_counter_case_stats_are_the_recorded_ones(name, counter_runs):
    stats = counter_runs[name][3]
    expected = nc.counter_case(name)['stats']
    print(stats)
    assert {k: stats[k] for k in expected} == expected
    assert set(stats) - set(expected) == set(finder.NOT_RECORDED)


def _entered(stats, state):
    """Tile 1 is the only tile entered in another state than START, and it is entered in `state`."""
    return stats['tile_entry'][state] == 1 and sum(stats['tile_entry'][1:]) == 1


#: what the recorded stats of a case must show for it to deserve its name
SHOWS = {
    'entry_tail1_pos': lambda s: _entered(s, nm.TAIL1) and s['tail'] == 1 and s['tail_reject'] == 0,
    'entry_tail1_neg': lambda s: _entered(s, nm.TAIL1 + 1) and s['tail'] == 1 and s['tail_reject'] == 0,
    'entry_tail2_pos': lambda s: (_entered(s, nm.TAIL2) and s['tail'] == 1 and s['tail_reject'] == 0 and
                                  s['tail_pair_across_tiles'] == dict(accepted=1, rejected=0)),
    'entry_tail2_neg': lambda s: (_entered(s, nm.TAIL2 + 1) and s['tail'] == 1 and s['tail_reject'] == 0 and
                                  s['tail_pair_across_tiles'] == dict(accepted=1, rejected=0)),
    # (one tail in the frame, entered across the tiles: the rejected pair is its first)
    'entry_tail1_pos_rejected': lambda s: _entered(s, nm.TAIL1) and s['tail'] == 1 and s['tail_reject'] >= 1,
    'entry_tail1_neg_rejected': lambda s: _entered(s, nm.TAIL1 + 1) and s['tail'] == 1 and s['tail_reject'] >= 1,
    'entry_tail2_pos_rejected': lambda s: (_entered(s, nm.TAIL2) and s['tail'] == 1 and
                                           s['tail_pair_across_tiles'] == dict(accepted=0, rejected=1)),
    'entry_tail2_neg_rejected': lambda s: (_entered(s, nm.TAIL2 + 1) and s['tail'] == 1 and
                                           s['tail_pair_across_tiles'] == dict(accepted=0, rejected=1)),
    'reject_run': lambda s: s['tail_reject_runs'] >= 2,
    'last_is_tail': lambda s: s['last_kind'] == 'tail',
    'last_is_straddled_tail': lambda s: s['last_kind'] == 'tail_straddled' and sum(s['tile_entry'][2:]) == 1,
    'round_entry_wedge': lambda s: s['n_tile'] > 256 and s['round_entry'] == [nm.WEDGE],
    'round_entry_tail': lambda s: s['n_tile'] > 256 and len(s['round_entry']) == 1 and s['round_entry'][0] >= nm.TAIL1,
    'carry_host': lambda s: s['host_carry'] == 3,
    'carry_mid_tile': lambda s: 0 < s['wrap_block'] < nm.TILE // 4 - 1 and s['n_tile'] >= 2,
    'carry_at_tile': lambda s: s['wrap_block'] == nm.TILE // 4 and s['n_tile'] >= 2,
}


def test_counter_cases_show_what_their_names_say():
    assert sorted(SHOWS) == sorted(CASE_NAMES)
    for c in nc.COUNTER_CASES:
        assert SHOWS[c['name']](c['stats']), c['name']
        small = not c['name'].startswith(('round_', 'last_'))
        assert c['n'] == (260000 if c['name'].startswith('round_') else 1500 if small else c['n'])
    for name, counter in (('carry_host', (2**64 - 1, 2**64 - 1, 2**64 - 1, 7)),):
        assert nc.counter_case(name)['counter'] == counter
    for name in ('carry_mid_tile', 'carry_at_tile'):
        assert nc.counter_case(name)['counter'][1:3] == (2**64 - 1, 2**64 - 1)


def test_counter_cases_cover_what_the_finder_claims():
    stats = [c['stats'] for c in nc.COUNTER_CASES]
    entered = np.sum([s['tile_entry'] for s in stats], axis=0)
    assert (entered[nm.TAIL1:] >= 1).all()                 # TAIL1 +, TAIL1 -, TAIL2 +, TAIL2 -
    assert sum(s['tail_pair_across_tiles']['accepted'] for s in stats) >= 1
    assert sum(s['tail_pair_across_tiles']['rejected'] for s in stats) >= 1
    assert max(s['tail_reject_runs'] for s in stats) >= 2
    assert any(r != nm.START for s in stats for r in s['round_entry'])
    assert {'tail', 'tail_straddled'} <= {s['last_kind'] for s in stats}


def test_old_inputs_never_enter_a_tile_in_a_tail(case_paths):
    """What the frames with a counter add: the streams of CASES show none of it."""
    for _, _, stats in case_paths:
        assert sum(stats['tile_entry'][nm.TAIL1:]) == 0
        assert stats['tail_pair_across_tiles'] == dict(accepted=0, rejected=0)
        assert all(s['n_tile'] <= 256 and s['wrap_block'] is None and s['host_carry'] == 0 for s in stats['per_frame'])


@pytest.fixture(scope='module')
def guard_runs():
    """The model on the frames of GUARD_CASE under its guard: (values, flags, walks)."""
    g = nc.GUARD_CASE
    stats = {}
    got, flags = nm.stream_frames(g['seed'], g['samples_per_frame'], (), np.float32, list(range(g['n_frame'])),
                                  stats=stats, guard=2.0 ** g['guard_log2'])
    return got, flags, [s['walk'] for s in stats['per_frame']]


def test_finder_reproduces_the_committed_cases(guard_runs):
    assert finder.find_counter_cases() == nc.COUNTER_CASES
    g = nc.GUARD_CASE
    assert finder.find_guard_case(g['seed'], g['samples_per_frame'], g['n_frame'], walks=guard_runs[2]) == g
    with open(nc.__file__) as f:
        text = f.read()
    committed = text[text.index(finder.BEGIN) + len(finder.BEGIN):text.index(finder.END)]
    assert committed == finder.render(nc.COUNTER_CASES, g)


def test_guard_case_is_off_the_guards_doorstep(guard_runs):
    """Some frames are flagged and some are not, and no decision that bears on any of them lies
    within a factor of 4 of the guard: the device's exp and log1p, a few units in the last place
    (1e-16) from the host's, cannot turn a flag."""
    got, flags, walks = guard_runs
    g = nc.GUARD_CASE
    guard = 2.0 ** g['guard_log2']
    assert guard <= 2.0 ** -10 and len(flags) == g['n_frame'] == 64
    assert [int(f) for f in flags] == g['flags']
    assert 0 < sum(g['flags']) < len(flags)
    for f, walk in enumerate(walks):
        counts = [nm.ambiguous_at(walk, x) for x in (guard / 4, guard, 4 * guard)]
        print(f, counts)
        assert counts[0] == counts[1] == counts[2], f     # (ambiguous at a guard: at every larger one too)
        assert (counts[1] > 0) == bool(flags[f])
    # frames that are not flagged are NumPy's
    gen = bt.NoiseGenerator((g['n_frame'] * g['samples_per_frame'],), nc.START, 1. * u.MHz, g['samples_per_frame'],
                            dtype=np.float32, seed=g['seed'])
    want = gen.read().reshape(g['n_frame'], -1)
    keep = ~flags
    assert same_bytes(got[keep], want[keep])
