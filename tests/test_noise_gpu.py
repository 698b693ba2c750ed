"""DeviceNoiseGenerator on the GPU: bit for bit `NoiseGenerator` (inputs: noise_cases.py, whose
paths through the sampler test_noise_model.py records), and `hip.philox_normal` on frames with an
explicit counter: bit for bit NumPy from that key and counter (`noise_model.numpy_frame`)."""
import os
import sys

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, units as u

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import noise_cases as nc            # noqa: E402
import noise_model as nm            # noqa: E402

pytestmark = pytest.mark.gpu


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope='module')
def host_streams():
    """What NumPy makes of each case (made once; never written to)."""
    out = []
    for case in nc.CASES:
        x = nc.make(bt.NoiseGenerator, case).read()
        x.flags.writeable = False
        out.append(x)
    return out


@pytest.mark.parametrize('k', range(len(nc.CASES)))
def test_whole_stream_equals_numpy(k, host_streams):
    gen = nc.make(bt.DeviceNoiseGenerator, nc.CASES[k])
    got = gen.read()                                   # several frames in one call, the last one cut
    assert same_bytes(got, host_streams[k])
    assert gen.host_frames == 0
    assert gen.tell() == gen.shape[0]


@pytest.mark.parametrize('k', range(len(nc.CASES)))
def test_pieces_in_scrambled_order(k, host_streams):
    want = host_streams[k]
    gen = nc.make(bt.DeviceNoiseGenerator, nc.CASES[k])
    spf, length = gen.samples_per_frame, gen.shape[0]
    # (start, count): inside a frame, across frames and ending inside one, one sample, the end
    pieces = [(spf + 5, 2 * spf - 9), (0, 3), (length - 7, 7), (spf - 1, 2), (2 * spf, spf), (17, spf // 2),
              (3, length - 3)]
    for start, count in pieces:
        gen.seek(start)
        assert same_bytes(gen.read(count), want[start:start + count]), (start, count)
        assert gen.tell() == start + count
    out = np.empty((spf,) + want.shape[1:], want.dtype)
    gen.seek(11)
    assert gen.read(out=out) is out and same_bytes(out, want[11:11 + spf])
    assert same_bytes(gen._read_frame(1), want[spf:2 * spf])
    assert gen.host_frames == 0


def test_a_prefix_generates_only_what_it_needs(host_streams):
    gen = nc.make(bt.DeviceNoiseGenerator, nc.CASES[2])
    spf = gen.samples_per_frame
    gen.seek(spf)
    view = gen.read_device(10)
    assert isinstance(view, hip.DeviceArray) and view.shape == (10, 2)
    assert gen._cache.shape[0] == 10                   # not the whole frame
    assert same_bytes(view.to_host(), host_streams[2][spf:spf + 10])


def test_bounded_cache_and_piecewise_reads(host_streams):
    gen = nc.make(bt.DeviceNoiseGenerator, nc.CASES[1])
    gen.max_frames_per_call = 1
    gen.seek(5)
    got = gen.read_device(gen.shape[0] - 5)            # more than the cache may hold: a fresh array
    assert same_bytes(got.to_host(), host_streams[1][5:])
    assert gen.host_frames == 0


def test_two_generators_interleaved(host_streams):
    a = nc.make(bt.DeviceNoiseGenerator, nc.CASES[0])
    b = nc.make(bt.DeviceNoiseGenerator, nc.CASES[3])
    got_a, got_b = [], []
    for _ in range(3):
        va = a.read_device(1500)
        vb = b.read_device(1700)
        got_b.append(vb.to_host())
        got_a.append(va.to_host())
    assert same_bytes(np.concatenate(got_a), host_streams[0][:4500])
    assert same_bytes(np.concatenate(got_b), host_streams[3][:5100])
    assert a.host_frames == 0 and b.host_frames == 0


def test_seed_none_draws_entropy_once():
    gen = bt.DeviceNoiseGenerator((4000,), nc.START, 1. * u.MHz, 1000, dtype=np.float32)
    first = gen.read()
    gen.seek(0)
    assert same_bytes(gen.read(), first)
    gen._host.seek(0)
    assert same_bytes(gen._host.read(), first)
    other = bt.DeviceNoiseGenerator((4000,), nc.START, 1. * u.MHz, 1000, dtype=np.float32)
    assert not same_bytes(other.read(), first)


def pipeline(source):
    return bt.Channelize(bt.Dedisperse(source, 30.), 64)


def test_feeds_dedisperse_and_channelize():
    n, spf = 6 * 2**14, 2**14
    kwargs = dict(frequency=1400 * u.MHz, sideband=1)
    host = bt.NoiseGenerator((n, 2), nc.START, 16 * u.MHz, spf, seed=12345, **kwargs)
    dev = bt.DeviceNoiseGenerator((n, 2), nc.START, 16 * u.MHz, spf, seed=12345, **kwargs)
    want = pipeline(bt.DeviceStream(host, nc.START, 16 * u.MHz, **kwargs)).read()
    got = pipeline(dev).read()
    assert same_bytes(got, want)
    assert dev.host_frames == 0


def test_device_stream_of_a_device_source(host_streams):
    case = nc.CASES[1]
    a = bt.DeviceStream(nc.make(bt.DeviceNoiseGenerator, case), nc.START, 1. * u.MHz)
    b = bt.DeviceStream(nc.make(bt.NoiseGenerator, case), nc.START, 1. * u.MHz)
    assert a.shape == b.shape and a.samples_per_frame == b.samples_per_frame
    assert same_bytes(a.read(), b.read())
    assert same_bytes(a.read_device(0).to_host(), b.read_device(0).to_host())


def test_too_few_words_are_doubled(host_streams):
    seed, spf, _, _, _ = nc.CASES[0]
    state = np.random.Philox(seed).state['state']
    counters = np.tile(state['counter'], (2, 1))
    counters[1, 1] = spf
    out = hip.DeviceArray((2, spf), np.float32)
    flags, reruns = hip.philox_normal(out, state['key'], counters, n_words=2048)      # 4096 normals need ~4190
    assert reruns == 4 and not flags.any()                 # each frame: 2048 -> 4096 -> 8192 words
    assert same_bytes(out.to_host().reshape(-1), host_streams[0][:2 * spf])
    flags, reruns = hip.philox_normal(out, state['key'], counters)
    assert reruns == 0 and not flags.any()
    assert same_bytes(out.to_host().reshape(-1), host_streams[0][:2 * spf])


def test_flagged_frames_are_made_by_numpy(host_streams):
    gen = nc.make(bt.DeviceNoiseGenerator, nc.CASES[0])
    gen._guard = np.inf                                    # every wedge or tail comparison is "too close"
    got = gen.read()
    assert same_bytes(got, host_streams[0])
    assert gen.host_frames == 4                            # 3 whole frames and the cut one


# ---------------------------------------------------------------------------------------------
# frames with an explicit counter (noise_cases.COUNTER_CASES: what each one reaches is recorded
# there and proven by test_noise_model.py), against NumPy itself

@pytest.fixture(scope='module')
def counter_wants():
    """name -> NumPy's normals of the frame (made once; never written to)."""
    out = {}
    for c in nc.COUNTER_CASES:
        out[c['name']] = nm.numpy_frame(c['key'], c['counter'], c['n'])
        out[c['name']].flags.writeable = False
    return out


@pytest.mark.parametrize('name', [c['name'] for c in nc.COUNTER_CASES])
def test_counter_case_equals_numpy(name, counter_wants):
    c = nc.counter_case(name)
    out = hip.DeviceArray((1, c['n']), np.float32)
    flags, reruns = hip.philox_normal(out, c['key'], [c['counter']], n=c['n'], n_words=c['n_words'])
    assert same_bytes(out.to_host()[0], counter_wants[name])
    assert not flags.any() and reruns == 0


def test_counter_cases_as_frames_of_one_call(counter_wants):
    """The carries (and a tile entered in a tail) in frames 1 to 4 of a call: each frame's counter
    is its own."""
    names = ['entry_tail1_pos', 'carry_host', 'carry_mid_tile', 'carry_at_tile', 'entry_tail2_neg_rejected']
    cases = [nc.counter_case(name) for name in names]
    assert all(c['n'] == 1500 and c['key'] == nc.KEY for c in cases)
    out = hip.DeviceArray((len(cases), 1500), np.float32)
    flags, reruns = hip.philox_normal(out, nc.KEY, [c['counter'] for c in cases])
    got = out.to_host()
    for k, name in enumerate(names):
        assert same_bytes(got[k], counter_wants[name]), name
    assert not flags.any() and reruns == 0


def stream_counters(seed, spf, n_frame):
    """(key, counters) of the frames of NoiseGenerator(seed=seed, samples_per_frame=spf)."""
    state = np.random.Philox(seed).state['state']
    counters = np.tile(state['counter'], (n_frame, 1))
    counters[:, 1] = spf * np.arange(n_frame, dtype=np.uint64)
    return state['key'], counters


@pytest.mark.parametrize('stride', [1031, 1032])
def test_rows_longer_than_the_frame_keep_their_remainder(stride):
    """n < stride: rows that start 4-byte (1031) and 16-byte (1032) aligned."""
    n, n_frame = 1001, 3
    sentinel = np.full((n_frame, stride), 0x7fc0beef, np.uint32).view(np.float32)
    out = hip.DeviceArray.from_host(sentinel)
    key, counters = stream_counters(7, n, n_frame)
    flags, reruns = hip.philox_normal(out, key, counters, n=n)
    got = out.to_host()
    for f in range(n_frame):
        assert same_bytes(got[f, :n], nm.numpy_frame(key, counters[f], n)), f
    assert same_bytes(got[:, n:], sentinel[:, n:])
    assert not flags.any() and reruns == 0


def test_65535_frames_of_one_sample_in_one_call():
    n_frame = 65535
    key, counters = stream_counters(11, 1, n_frame)
    out = hip.DeviceArray((n_frame, 1), np.float32)
    flags, reruns = hip.philox_normal(out, key, counters, n=1)
    want = bt.NoiseGenerator((n_frame,), nc.START, 1. * u.MHz, 1, dtype=np.float32, seed=11).read()
    assert same_bytes(out.to_host().reshape(-1), want)
    assert not flags.any() and reruns == 0


def test_more_frames_than_one_call_takes():
    """65540 frames of one sample through the task: a run of 65535 frames and one of 5."""
    args = ((65540,), nc.START, 1. * u.MHz, 1)
    gen = bt.DeviceNoiseGenerator(*args, dtype=np.float32, seed=3)
    want = bt.NoiseGenerator(*args, dtype=np.float32, seed=3).read()
    assert same_bytes(gen.read(), want)
    assert gen.host_frames == 0


def test_long_frames_take_three_rounds_of_the_scan():
    """524288 normals per frame: 528 tiles of words, so the scan over a frame's tiles carries its
    state and offset through three rounds of 256.  Two whole frames and a cut one."""
    spf = 2**17
    args = ((2 * spf + 1000, 2), nc.START, 1. * u.MHz, spf)
    assert -(-hip.noise_word_count(4 * spf) // 1024) == 528
    gen = bt.DeviceNoiseGenerator(*args, dtype=np.complex64, seed=5)
    want = bt.NoiseGenerator(*args, dtype=np.complex64, seed=5).read()
    assert same_bytes(gen.read(), want)
    gen = bt.DeviceNoiseGenerator(*args, dtype=np.complex64, seed=5)
    gen.seek(spf + 12345)                                  # starts inside frame 1, ends with the cut one
    assert same_bytes(gen.read(), want[spf + 12345:])
    assert gen.host_frames == 0


def test_a_frame_far_into_a_long_stream():
    """Beyond sample 2^40 of a stream of more than 2^41: word 1 of the counter is above 2^32."""
    spf = 4096
    args = ((2**41 + 5 * spf, 2), nc.START, 1. * u.MHz, spf)
    gen = bt.DeviceNoiseGenerator(*args, dtype=np.complex64, seed=12345)
    host = bt.NoiseGenerator(*args, dtype=np.complex64, seed=12345)
    for start, count in ((2**40 + 3 * spf, spf), (2**41 + spf + 5, 2 * spf)):
        gen.seek(start)
        host.seek(start)
        assert same_bytes(gen.read(count), host.read(count)), start
    assert gen.host_frames == 0


def test_a_finite_guard_flags_the_frames_the_model_flags():
    """64 frames under a guard of 2^-22, from which every decision that bears on them is at least a
    factor of 4 away (test_noise_model.py): the device's exp and log1p differ from the host's by
    1e-16 or so, so its flags are the model's exactly."""
    g = nc.GUARD_CASE
    spf, n_frame, guard = g['samples_per_frame'], g['n_frame'], 2.0 ** g['guard_log2']
    model_flags = np.array(g['flags'], bool)
    args = ((n_frame * spf,), nc.START, 1. * u.MHz, spf)
    want = bt.NoiseGenerator(*args, dtype=np.float32, seed=g['seed']).read()
    key, counters = stream_counters(g['seed'], spf, n_frame)
    out = hip.DeviceArray((n_frame, spf), np.float32)
    flags, reruns = hip.philox_normal(out, key, counters, guard=guard)
    assert flags.tolist() == model_flags.tolist()
    assert same_bytes(out.to_host()[~model_flags], want.reshape(n_frame, spf)[~model_flags])
    gen = bt.DeviceNoiseGenerator(*args, dtype=np.float32, seed=g['seed'])
    gen._guard = guard
    assert same_bytes(gen.read(), want)
    assert gen.host_frames == int(model_flags.sum())


def test_wrapper_checks_its_arguments():
    out = hip.DeviceArray((2, 16), np.float32)
    with pytest.raises(ValueError):
        hip.philox_normal(out, [1, 2], np.zeros((3, 4), np.uint64))
    with pytest.raises(ValueError):
        hip.philox_normal(out, [1, 2], np.zeros((2, 4), np.uint64), n=17)
    with pytest.raises(TypeError):
        hip.philox_normal(hip.DeviceArray((2, 16), np.complex64), [1, 2], np.zeros((2, 4), np.uint64))
    with pytest.raises(hip.HipError):
        hip.philox_normal(out, [1, 2], np.zeros((2, 4), np.uint64), n_words=6)


@pytest.mark.parametrize('dtype', [np.float64, np.complex128, np.int8])
def test_unsupported_dtypes_raise(dtype):
    with pytest.raises(TypeError):
        bt.DeviceNoiseGenerator((1000,), nc.START, 1. * u.MHz, 100, dtype=dtype)
