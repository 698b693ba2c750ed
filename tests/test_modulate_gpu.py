"""`Modulate` on the GPU against its NumPy twin (`modulate_samples` on `Modulate.bins`), bit for
bit: a float32 product has one correct rounding.  Runs route and pieces route, reads in pieces,
several chunks per read, the closed loop with `Fold`, and device sources and consumers."""
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u
from baseband_tasks_amd.device_task import produces_on_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLYCO = os.path.join(ROOT, 'tests', 'golden', 'B1937_polyco.dat')
T0 = bt.Time('2010-11-12T13:14:15')
RATE = 1e4


def _data(n, sample_shape, dtype, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n,) + sample_shape).astype(np.float32)
    if np.dtype(dtype).kind == 'c':
        x = (x + 1j * rng.standard_normal(x.shape).astype(np.float32)).astype(np.complex64)
    return x


def _profile(kind, n_phase, sample_shape, seed=2):
    rng = np.random.default_rng(seed)
    shape = {'shared': (), 'element': sample_shape, 'middle': sample_shape[:-1] + (1,),
             'trailing': sample_shape[-1:]}[kind]
    return rng.uniform(-2., 2., (n_phase,) + shape)


def _linear(per_bin, n_phase, offset=0.123):
    f = 1. / (per_bin * n_phase)
    return lambda t: offset + f * (t - T0) * RATE


class TwoPart:
    def __init__(self, cycles):
        self.int = np.round(cycles)
        self.frac = cycles - self.int


def _check(mh, x, profile):
    n = x.shape[0]
    want = bt.modulate_samples(x, profile, mh.bins(0, n))
    mh.seek(0)
    got = mh.read()
    assert got.dtype == x.dtype and got.shape == x.shape
    np.testing.assert_array_equal(got, want)
    return got


# (sample shape, dtype, samples, samples per frame, n_phase, samples per bin, profile)
RUN_CASES = [
    ((), np.float32, 65533, 4099, 64, 1, 'shared'),
    ((), np.float32, 65533, 4099, 7, 2.5, 'shared'),
    ((), np.complex64, 65533, 4099, 1024, 3000, 'shared'),
    ((), np.float32, 65533, 8192, 7, 3000, 'element'),
    ((2,), np.complex64, 65533, 4099, 1024, 1, 'element'),
    ((2,), np.float32, 65533, 4099, 64, 2.5, 'element'),
    ((2,), np.complex64, 40001, 40001, 1, 2.5, 'shared'),
    ((3,), np.float32, 65533, 4099, 7, 2.5, 'element'),
    ((3,), np.complex64, 65533, 4099, 64, 1, 'shared'),
    ((3,), np.float32, 50001, 50001, 64, 5000, 'element'),
    ((5, 2), np.complex64, 20001, 1531, 7, 1, 'middle'),
    ((5, 2), np.float32, 20001, 1531, 64, 2.5, 'element'),
    ((5, 2), np.complex64, 20001, 20001, 1024, 3000, 'trailing'),
    ((1024, 2), np.complex64, 41, 16, 7, 1, 'shared'),
    ((1024, 2), np.complex64, 41, 16, 64, 2.5, 'element'),
    ((1024, 2), np.float32, 41, 41, 1024, 2.5, 'middle'),
    ((1024, 2), np.float32, 41, 16, 7, 3000, 'trailing'),
]


@pytest.mark.parametrize('case', RUN_CASES, ids=lambda c: f'{c[0]}-{np.dtype(c[1]).name}-{c[4]}bins-{c[5]}per-{c[6]}')
def test_runs_route_equals_twin(case):
    sample_shape, dtype, n, spf, n_phase, per_bin, kind = case
    x = _data(n, sample_shape, dtype)
    profile = _profile(kind, n_phase, sample_shape)
    sh = bt.HostStream(x, T0, RATE, samples_per_frame=spf, pin=False)
    mh = bt.Modulate(sh, profile, _linear(per_bin, n_phase))
    _check(mh, x, profile)
    bins = mh.bins(0, n)
    if per_bin == 1:
        assert np.all(np.diff(bins[:spf]) % n_phase == (1 % n_phase))     # (exactly one sample per bin)
    if per_bin >= 3000 and n > 10000:
        assert np.max(np.diff(np.flatnonzero(np.diff(bins)))) > 2048          # (runs longer than a tile)


@pytest.mark.parametrize('two_part', [False, True])
def test_negative_and_two_part_phases(two_part):
    n, n_phase = 30011, 64
    x = _data(n, (2,), np.complex64, seed=5)
    profile = _profile('element', n_phase, (2,))
    lin = _linear(2.5, n_phase, offset=-7.31)
    phase = (lambda t: TwoPart(lin(t))) if two_part else lin
    mh = bt.Modulate(bt.HostStream(x, T0, RATE, samples_per_frame=1000, pin=False), profile, phase)
    assert float(np.ravel(lin(T0 + np.zeros(1)))[0]) < 0
    _check(mh, x, profile)


@pytest.mark.parametrize('sample_shape,dtype', [((), np.float32), ((3,), np.complex64), ((2,), np.float32)])
def test_reads_in_pieces_with_seeks(sample_shape, dtype):
    # from a stream resident in HBM: a read that starts at an odd sample hands the kernel an
    # input that is not 16-byte aligned
    n, spf, n_phase = 20000, 1024, 64
    x = _data(n, sample_shape, dtype, seed=7)
    profile = _profile('element', n_phase, sample_shape)
    mh = bt.Modulate(bt.DeviceStream(x, T0, RATE, samples_per_frame=spf), profile, _linear(2.5, n_phase),
                     samples_per_frame=spf)
    want = bt.modulate_samples(x, profile, mh.bins(0, n))
    for start, count in [(1021, 7), (1023, 3000), (4023, 2049), (3, 1), (19999, 1), (5119, 1025), (0, 20000)]:
        mh.seek(start)
        np.testing.assert_array_equal(mh.read(count), want[start:start + count])
        assert mh.tell() == start + count
    mh.seek(2047)
    d = mh.read_device(3)
    np.testing.assert_array_equal(d.to_host(), want[2047:2050])
    mh.max_frames_per_call = 2                     # (a long read assembled from several runs of frames)
    mh.seek(1)
    np.testing.assert_array_equal(mh.read_device(n - 2).to_host(), want[1:n - 1])


@pytest.mark.parametrize('sample_shape,dtype,per', [((5, 2), np.complex64, 7001), ((3,), np.float32, 7001),
                                                     ((), np.float32, 6001)])
def test_small_budget_takes_several_chunks(sample_shape, dtype, per, monkeypatch):
    n, n_phase = 20001, 64
    x = _data(n, sample_shape, dtype, seed=9)
    profile = _profile('shared', n_phase, sample_shape)
    mh = bt.Modulate(bt.HostStream(x, T0, RATE, samples_per_frame=n, pin=False), profile, _linear(700, n_phase))
    mh.modulate_budget = per * x[0].nbytes
    calls = []
    real = bt.hip.modulate_runs
    monkeypatch.setattr(bt.hip, 'modulate_runs', lambda *a: (calls.append(a[0].shape[0]), real(*a))[1])
    _check(mh, x, profile)
    assert len(calls) >= 3 and sum(calls) == n and max(calls) == per


# -- pieces route ---------------------------------------------------------------------------
def _polyco_stream(x, wide):
    # the closest polyco entry changes at 22:57:36, half a second in: inside the first frame
    rate = 64. if wide else 5e4
    spf = 48 if wide else 32768
    return bt.DeviceStream(x, bt.Time('2018-05-06T22:57:35.5'), rate, samples_per_frame=spf)


@pytest.mark.parametrize('wide', [False, True])
@pytest.mark.parametrize('kind', ['shared', 'element'])
def test_pieces_route_device_equals_host_equals_twin(wide, kind):
    pp = bt.phases.PolycoPhase(POLYCO)
    sample_shape, dtype, n = (((1024, 2), np.float32, 96) if wide else ((2,), np.complex64, 65536))
    x = _data(n, sample_shape, dtype, seed=11)
    profile = _profile(kind, 1024, sample_shape)
    out = {}
    for route in ('device', 'host'):
        mh = bt.Modulate(_polyco_stream(x, wide), profile, pp)
        mh.table_route = route
        spf = mh.samples_per_frame
        assert len(pp.fold_pieces(mh.start_time, mh.sample_rate, 0, spf)) == 2       # (two entries in frame 0)
        out[route] = _check(mh, x, profile)
        mh.seek(spf - 5)                                                        # (a read across the frame edge)
        np.testing.assert_array_equal(mh.read(11), out[route][spf - 5:spf + 6])
    np.testing.assert_array_equal(out['device'], out['host'])


# -- closed loop with Fold ----------------------------------------------------------------------
@pytest.mark.parametrize('phase_kind', ['callable', 'polyco-device', 'polyco-host'])
def test_fold_of_modulated_ones_recovers_the_profile(phase_kind):
    n, spf, n_phase = 65536, 8192, 64
    g = np.random.default_rng(13).integers(0, 32, n_phase) / 8.            # (multiples of 1/8 below 4: sums exact)
    if phase_kind == 'callable':
        ih = bt.DeviceStream(np.ones((n, 2), np.float32), T0, RATE, samples_per_frame=spf)
        phase, route = _linear(2.5, n_phase), None
    else:
        ih = bt.DeviceStream(np.ones((n, 2), np.float32), bt.Time('2018-05-06T22:57:35.5'), 1e5, samples_per_frame=spf)
        phase, route = bt.phases.PolycoPhase(POLYCO), phase_kind.split('-')[1]
    mh = bt.Modulate(ih, g, phase)
    fh = bt.Fold(mh, n_phase, phase, step=spf, average=False)
    mh.table_route = fh.table_route = route
    res = fh.read()
    assert res.shape == (n // spf, n_phase, 2)
    count = res['count']
    assert np.all(count.sum(axis=1) == spf)
    assert np.all(count[..., 0] == count[..., -1]) and np.count_nonzero(count) > 0
    np.testing.assert_array_equal(res['data'], (count * g[:, np.newaxis]).astype(np.float32))


# -- device sources and consumers ------------------------------------------------------------------
def test_device_noise_source_and_device_consumers(monkeypatch):
    n, spf, n_phase = 65536, 16384, 32
    args = ((n, 2), '2020-01-01T00:00:00', 1 * u.MHz, spf)
    kwargs = dict(seed=4321, frequency=1400 * u.MHz, sideband=1)
    g = 0.25 + np.random.default_rng(17).uniform(0., 2., n_phase)
    t0 = bt.Time('2020-01-01T00:00:00')
    phase = (lambda t: 0.4 + 30.123 * (t - t0))
    mh = bt.Modulate(bt.DeviceNoiseGenerator(*args, **kwargs), g, phase)
    assert produces_on_device(mh) and mh.samples_per_frame == spf
    noise = bt.NoiseGenerator(*args, **kwargs).read()
    want = bt.modulate_samples(noise, g, mh.bins(0, n))
    np.testing.assert_array_equal(mh.read(), want)
    # downstream device tasks take the frames in HBM: the modulated stream is never downloaded
    twin = bt.DeviceStream(want, t0, 1e6, samples_per_frame=spf, frequency=1400e6, sideband=1)
    monkeypatch.setattr(mh, 'read', lambda *a, **k: pytest.fail('the modulated stream was downloaded'))
    mh.seek(0)
    np.testing.assert_array_equal(bt.Square(mh).read(), bt.Square(twin).read())
    mh.seek(0)
    got = bt.Dedisperse(mh, 5.).read()
    ref = bt.Dedisperse(twin, 5.).read()
    assert got.shape == ref.shape and got.shape[0] > 0
    np.testing.assert_array_equal(got, ref)
    # a read_device result is this task's own cache, not the noise generator's block
    mh.seek(0)
    d = mh.read_device(100)
    src = bt.DeviceNoiseGenerator(*args, **kwargs).read_device(100)
    assert d.ptr != src.ptr and d.owner is not src.owner
    np.testing.assert_array_equal(d.to_host(), want[:100])


def test_nan_inf_and_negative_gains_pass_through_as_numpys():
    n, n_phase = 8191, 8
    profile = np.array([1., -2.5, np.nan, np.inf, 0., -0., -np.inf, 3.], np.float32)
    for dtype in (np.float32, np.complex64):
        x = _data(n, (3,), dtype, seed=19)
        mh = bt.Modulate(bt.HostStream(x, T0, RATE, samples_per_frame=n, pin=False), profile, _linear(2.5, n_phase))
        want = _check(mh, x, profile)
        bins = mh.bins(0, n)
        assert set(bins) == set(range(8)) and np.isnan(want).any() and np.isinf(want).any()
        with np.errstate(invalid='ignore'):
            numpys = x * profile[bins][:, np.newaxis]
        mh.seek(0)
        got = mh.read()
        np.testing.assert_array_equal(np.isnan(got), np.isnan(numpys))
        ok = ~np.isnan(numpys)
        np.testing.assert_array_equal(got[ok], numpys[ok])
        if dtype is np.float32:
            np.testing.assert_array_equal(np.signbit(got[ok]), np.signbit(numpys[ok]))
