"""tools/noise_model.py (the CPU restatement of csrc/noise_kernels.hpp) against NumPy, the
committed ziggurat tables against the running NumPy, and what the inputs of test_noise_gpu.py
exercise."""
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
