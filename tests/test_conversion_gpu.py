"""`Real2Complex` on the GPU: the reference's tests (baseband_tasks/tests/test_conversion.py) in
float32, the golden vectors of the real reference (tests/golden/conversion_vectors.npz), parity of
both routes and every stream count against a float64 NumPy restatement of the reference's task
applied stream by stream, stream semantics, chains into the downstream tasks, and the C ABI."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip
from baseband_tasks_amd import units as u
from oracle import bbt_oracle as orc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conversion_vectors.npz')
T0 = bt.Time('2010-11-12T13:14:15')


def reference(x, m):
    """The reference's Real2Complex(ih, m).read() in float64, any sample shape, stream by stream:
    fft -> one-sided spectrum -> ifft -> exp(-i pi n / 2) -> [::2] per frame of 2 m samples."""
    n = 2 * m
    nf = x.shape[0] // n
    blocks = x[:nf * n].astype(np.float64).reshape((nf, n) + x.shape[1:])
    z = np.fft.fft(blocks, axis=1)
    h = np.zeros(n)
    h[0] = h[m] = 1
    h[1:m] = 2
    z = np.fft.ifft(z * h.reshape((1, n) + (1,) * (x.ndim - 1)), axis=1)
    z *= np.exp(-1j * np.pi / 2 * np.arange(n)).reshape((1, n) + (1,) * (x.ndim - 1))
    return z[:, ::2].reshape((nf * m,) + x.shape[1:])


def host(x, spf, **kw):
    return bt.HostStream(np.ascontiguousarray(x, np.float32), T0, 64 * u.kHz, samples_per_frame=spf, pin=False, **kw)


def device(x, spf, **kw):
    return bt.DeviceStream(np.ascontiguousarray(x, np.float32), T0, 64 * u.kHz, samples_per_frame=spf, **kw)


def check(out, x, m):
    ref = reference(x, m)
    assert out.shape == ref.shape and out.dtype == np.complex64
    err = rel_l2(out, ref)
    assert err <= 2e-6, err
    # the real part is the input sample itself, sign flipped on odd output samples
    nf = out.shape[0] // m
    xe = x[:nf * 2 * m:2].astype(np.float32)
    sign = np.tile((-1.) ** np.arange(m), nf).reshape((-1,) + (1,) * (x.ndim - 1)).astype(np.float32)
    assert np.array_equal(out.real, sign * xe)


# -- the reference's tests -----------------------------------------------------------------
def test_real_to_complex_delta():
    def real_delta(handle):
        d = np.zeros(handle.samples_per_frame, dtype=np.float32)
        if handle.offset == 0:
            d[0] = 1.0
        return d

    delta_fh = bt.StreamGenerator(real_delta, samples_per_frame=1024, start_time=T0, sample_rate=1. * u.kHz,
                                  frequency=400 * u.kHz, sideband=1, shape=(2048,), dtype='f4')
    real_data = delta_fh.read()
    assert real_data[0] == 1. and np.all(real_data[1:] == 0.)
    complex_delta = np.zeros(2048 // 2, dtype=np.complex64)
    complex_delta[0] = 1.0
    r2c = bt.Real2Complex(delta_fh)
    out = r2c.read()
    assert out.shape == (1024,) and np.iscomplexobj(out)
    assert np.array_equal(out, complex_delta)
    assert np.isclose(u.to_hz(r2c.frequency), 400.5e3)
    assert r2c.sideband == 1
    assert repr(r2c).startswith('Real2Complex(ih)')


def test_expected_failures():
    with pytest.raises(ValueError):
        bt.Real2Complex(bt.EmptyStreamGenerator(samples_per_frame=1024, start_time=T0, sample_rate=1. * u.kHz,
                                                shape=(2048,), dtype='c8'))
    with pytest.raises(TypeError, match='SinglePrecision'):
        bt.Real2Complex(bt.EmptyStreamGenerator(samples_per_frame=1024, start_time=T0, sample_rate=1. * u.kHz,
                                                shape=(2048,), dtype='f8'))


@pytest.mark.parametrize('f_nyquist', (0.75, 0.5, 0.25, 0.125, 0.5 + 1 / 32))
def test_real_to_complex_sine(f_nyquist):
    def real_sine(handle):
        return np.sin(f_nyquist * np.pi * np.arange(handle.samples_per_frame)).astype(np.float32)

    sine_fh = bt.StreamGenerator(real_sine, samples_per_frame=1024, start_time=T0, sample_rate=1. * u.kHz,
                                 frequency=400 * u.kHz, sideband=-1, shape=(2048,), dtype='f4')
    f_complex = f_nyquist - 0.5
    complex_dc = np.exp(2j * np.pi * (-0.25 + np.arange(2048 // 2) * f_complex))
    r2c = bt.Real2Complex(sine_fh)
    out = r2c.read()
    assert out.shape == (1024,) and np.iscomplexobj(out)
    np.testing.assert_allclose(out, complex_dc, atol=1e-5)
    assert np.isclose(u.to_hz(r2c.frequency), 399.5e3)
    assert r2c.sideband == -1


# -- golden vectors of the real reference -----------------------------------------------------
def golden_cases():
    d = np.load(GOLDEN)
    return [(json.loads(str(d[k])), d[k[:-4] + 'input'], d[k[:-4] + 'output'])
            for k in sorted(d.files) if k.endswith('/meta')]


@pytest.mark.parametrize('multi', [False, True])
def test_golden_vectors(multi, monkeypatch):
    monkeypatch.setattr(bt.Real2Complex, 'MULTI_LEVEL', multi)
    for meta, raw, want in golden_cases():
        m = meta['M']
        x = raw.astype(np.float32)
        kw = {} if meta.get('frequency') is None else dict(frequency=meta['frequency'], sideband=meta['sideband'])
        ih = host(x, meta['ih_samples_per_frame'], **kw)
        r2c = bt.Real2Complex(ih) if meta.get('default') else bt.Real2Complex(ih, samples_per_frame=m)
        out = r2c.read()
        assert out.shape == want.shape
        err = rel_l2(out, want)
        assert err <= 2e-6, (m, multi, err)
        nf = meta['frames']
        assert np.array_equal(out.real, np.tile((-1.) ** np.arange(m), nf).astype(np.float32) * x[:nf * 2 * m:2])
        if meta['out_frequency'] is not None:
            assert u.to_hz(r2c.frequency) == meta['out_frequency']
        r2c.close()


# -- routes, lengths and stream counts ------------------------------------------------------
ONE_PASS = [256, 4096, 8192, 6174, 1215, 7]
MULTI = [16384, 10000, 1 << 17]


@pytest.mark.parametrize('m', ONE_PASS + MULTI)
@pytest.mark.parametrize('shape', [(), (2,), (3,), (8,), (2, 4)])
def test_streams_and_lengths(m, shape):
    rng = np.random.default_rng(m + len(shape))
    frames = 3 if m <= 16384 else 2
    x = rng.standard_normal((2 * m * frames + 5,) + shape).astype(np.float32)
    r2c = bt.Real2Complex(host(x, 2 * m))
    assert r2c.one_pass == (m <= 8192 or m == 16384)
    check(r2c.read(), x, m)


@pytest.mark.parametrize('frames', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('m', [1024, 6174, 10000])
def test_one_stream_frame_counts(m, frames):
    x = np.random.default_rng(frames).standard_normal(2 * m * frames).astype(np.float32)
    check(bt.Real2Complex(host(x, 2 * m)).read(), x, m)


@pytest.mark.parametrize('m', [1 << 19, 1 << 20])
def test_long_frames(m):
    x = np.random.default_rng(20).standard_normal((2 * m * 2, 2)).astype(np.float32)
    r2c = bt.Real2Complex(device(x, 2 * m))
    assert not r2c.one_pass
    check(r2c.read(), x, m)


@pytest.mark.parametrize('m', [7, 1024, 6174, 8192, 16384])
@pytest.mark.parametrize('shape', [(), (3,), (8,)])
def test_one_pass_matches_multi_level(m, shape, monkeypatch):
    x = np.random.default_rng(m).standard_normal((2 * m * 3,) + shape).astype(np.float32)
    a = bt.Real2Complex(device(x, 2 * m))
    assert a.one_pass
    monkeypatch.setattr(bt.Real2Complex, 'MULTI_LEVEL', True)
    b = bt.Real2Complex(device(x, 2 * m))
    assert not b.one_pass
    ya, yb = a.read(), b.read()
    assert np.array_equal(ya.real, yb.real)
    assert rel_l2(ya, yb) <= 2e-6
    check(yb, x, m)


# -- stream semantics ---------------------------------------------------------------------------
def test_seek_read_device_host_device_and_repeats():
    m = 1000
    x = np.random.default_rng(3).standard_normal((2 * m * 7 + 11, 2, 3)).astype(np.float32)
    want = reference(x, m)
    r = bt.Real2Complex(host(x, 2 * m))
    full = r.read()
    check(full, x, m)
    # partial reads across frame boundaries
    for start, count in [(0, 1), (999, 2), (1500, 2000), (3999, 1001), (6990, 10)]:
        r.seek(start)
        piece = r.read(count)
        assert np.array_equal(piece, full[start:start + count])
        assert rel_l2(piece, want[start:start + count]) <= 2e-6
    r.seek(2500)
    assert np.array_equal(r.read_device(1700).to_host(), full[2500:4200])
    # host-resident and device-resident input: the same bits; and again
    d = bt.Real2Complex(device(x, 2 * m))
    assert np.array_equal(d.read(), full)
    d.seek(0)
    assert np.array_equal(d.read(), full)
    assert np.array_equal(bt.Real2Complex(host(x, 2 * m)).read(), full)


def test_task_on_a_host_frame():
    m = 512
    x = np.random.default_rng(4).standard_normal((2 * m * 2, 3)).astype(np.float32)
    r = bt.Real2Complex(host(x, 2 * m))
    out = r.task(x[:2 * m])
    assert out.shape == (m, 3)
    check(out, x[:2 * m], m)


# -- chains -------------------------------------------------------------------------------
def test_vdif_dedisperse_channelize_chain():
    from baseband_tasks_amd import ingest
    rng = np.random.default_rng(5)
    spf, n = 20000, 20000 * 6
    levels = np.asarray([-3.3359, -1., 1., 3.3359], dtype=np.float32)
    data = rng.choice(levels, size=(n, 1, 2))
    fs = 64e6
    raw = ingest.encode_vdif_frames(data, 2, seconds=100, ref_epoch=41, frame_nr0=0,
                                    frames_per_second=int(fs) // spf, samples_per_frame=spf, edv=3, sample_rate=fs)
    fh = bt.open_vdif(raw, frequency=300 * u.MHz, sideband=1)
    data = data.reshape(n, 2)            # (one thread: the stream's samples are (2,))
    assert fh.dtype == np.float32 and np.array_equal(fh.read(), data)
    fh.seek(0)
    r2c = bt.Real2Complex(fh)
    assert r2c.samples_per_frame == 10000 and not r2c.one_pass
    z = reference(data, 10000)
    check(r2c.read(), data, 10000)
    dm = 0.001
    dd = bt.Dedisperse(r2c, dm)
    ch = bt.Channelize(dd, 1024)
    got = ch.read()
    want_dd, _ = orc.dedisperse(z.astype(np.complex64), fs / 2, 300. + fs / 2 / 1e6, 1, dm,
                                ih_samples_per_frame=10000)
    want = orc.channelize(want_dd, 1024)
    assert got.shape == want.shape
    assert rel_l2(got, want) <= 1e-5


def test_power_integrate_two_polarizations():
    m = 2048
    x = np.random.default_rng(6).standard_normal((2 * m * 4, 2)).astype(np.float32)
    ih = host(x, 2 * m, polarization=np.array(['X', 'Y']))
    r2c = bt.Real2Complex(ih)
    ip = bt.Integrate(bt.Power(r2c), 64)
    got = ip.read()
    z = reference(x, m)
    zx, zy = z[:, 0], z[:, 1]
    pw = np.stack([np.abs(zx) ** 2, np.abs(zy) ** 2, (zx * zy.conj()).real, (zx * zy.conj()).imag], axis=-1)
    want = pw[:(pw.shape[0] // 64) * 64].reshape(-1, 64, 4).mean(1)
    assert got.shape == want.shape
    assert rel_l2(got, want) <= 1e-5


# -- the C ABI ------------------------------------------------------------------------------
def test_c_abi():
    lib = hip.lib()
    m, s, frames = 12, 3, 2
    x = np.random.default_rng(7).standard_normal((2 * m * frames, s)).astype(np.float32)
    plan = C.c_void_p()
    assert lib.bbt_r2c_plan_create(C.byref(plan), m, s) == 0
    one, ws = C.c_int(), C.c_int64()
    assert lib.bbt_r2c_plan_info(plan, C.byref(one), C.byref(ws)) == 0 and one.value == 1
    xin = hip.DeviceArray.from_host(x)
    out = hip.DeviceArray((m * frames, s), np.complex64)
    assert lib.bbt_r2c_execute(plan, xin.ptr, out.ptr, frames, None) == 0
    assert lib.bbt_stream_sync(None) == 0
    check(out.to_host(), x, m)
    assert lib.bbt_r2c_plan_destroy(plan) == 0
    bad = C.c_void_p()
    assert lib.bbt_r2c_plan_create(C.byref(bad), 11, 1) != 0
    assert b'n_out=11' in lib.bbt_last_error()


def test_overlapping_buffers_are_refused():
    lib = hip.lib()
    m, s, frames = 16, 2, 2
    plan = hip.R2CPlan(m, s)
    buf = hip.DeviceArray((frames * 2 * m * s,), np.float32)
    rc = lib.bbt_r2c_execute(plan._h, buf.ptr, buf.ptr, frames, None)
    assert rc != 0 and b'must not overlap' in lib.bbt_last_error()
    plan.close()
