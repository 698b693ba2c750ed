"""Host side of `Real2Complex` (no GPU): metadata, refusals and the golden file's metadata
(tests/golden/conversion_vectors.npz, made by make_conversion_golden.py from the real reference),
the identity the kernels compute against a float64 restatement of the reference's task, and a
hipRTC compile for gfx950 of the one-pass kernel's translation unit."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u
from baseband_tasks_amd.conversion import check_r2c_length, r2c_response

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conversion_vectors.npz')
T0 = bt.Time('2010-11-12T13:14:15')


def reference_task(x):
    """The reference's Real2Complex.task (conversion.py:77-96) in float64, along axis 0."""
    n = x.shape[0]
    z = np.fft.fft(x.astype(np.complex128), axis=0)
    h = np.zeros(n)
    if n % 2 == 0:
        h[0] = h[n // 2] = 1
        h[1:n // 2] = 2
    else:
        h[0] = 1
        h[1:(n + 1) // 2] = 2
    z = np.fft.ifft(z * h.reshape((-1,) + (1,) * (x.ndim - 1)), axis=0)
    z *= np.exp(-1j * np.pi / 2 * np.arange(n)).reshape((-1,) + (1,) * (x.ndim - 1))
    return z[::2]


def identity(x):
    """out[m] = (-1)^m (x[2m] + i (g (*) x_o)[m]) with two real streams per complex transform."""
    m = x.shape[0] // 2
    g = r2c_response(m)
    s = (-1.) ** np.arange(m)
    y = np.fft.ifft(np.fft.fft(x[1::2, 0] + 1j * x[1::2, 1]) * g)
    return np.stack([s * (x[0::2, 0] + 1j * y.real), s * (x[0::2, 1] + 1j * y.imag)], axis=1)


def stream(shape, spf, dtype=np.float32, **kw):
    return bt.HostStream(np.zeros(shape, dtype), T0, 64 * u.kHz, samples_per_frame=spf, pin=False, **kw)


# -- the identity ---------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 2, 3, 5, 7, 8, 15, 500, 1000, 1024, 1215, 6174, 16000])
def test_identity_matches_the_reference_task(m):
    rng = np.random.default_rng(m)
    x = rng.standard_normal((2 * m, 2))
    ref = reference_task(x)
    fast = identity(x)
    assert np.abs(fast - ref).max() <= 1e-10 * max(1., np.abs(ref).max())
    assert np.array_equal(fast.real, (-1.) ** np.arange(m)[:, None] * x[0::2])


@pytest.mark.parametrize('m', [2, 3, 7, 10, 1000, 1215])
def test_response_is_hermitian(m):
    g = r2c_response(m)
    assert g[0] == 0
    j = np.arange(1, m)
    assert np.allclose(np.conj(g[m - j]), g[j], rtol=0, atol=1e-14)
    assert np.abs(np.fft.ifft(g).imag).max() < 1e-14


# -- metadata -------------------------------------------------------------------------
def test_shape_rate_dtype_and_repr():
    ih = stream((20037, 2, 3), 2000)
    r = bt.Real2Complex(ih)
    assert r.shape == (10 * 1000, 2, 3) and r.sample_shape == (2, 3)
    assert r.samples_per_frame == 1000 and r.dtype == np.complex64
    assert u.to_hz(r.sample_rate) == 32e3
    assert r.start_time == ih.start_time
    assert repr(r).startswith('Real2Complex(ih)')
    r2 = bt.Real2Complex(ih, samples_per_frame=500)
    assert r2.shape == (20 * 500, 2, 3) and r2.samples_per_frame == 500
    assert 'samples_per_frame=500' in repr(r2)


def test_frequency_and_sideband():
    ih = stream((4000,), 2000, frequency=1400e6, sideband=-1)
    r = bt.Real2Complex(ih)
    assert np.isclose(u.to_hz(r.frequency), 1400e6 - 32e3, rtol=0, atol=1e-3)
    assert r.sideband == -1
    assert repr(r).startswith('Real2Complex(ih)')
    freqs = np.array([100e6, 200e6, 300e6])
    ih = stream((4000, 3), 2000, frequency=freqs, sideband=np.array([1, -1, 1]))
    r = bt.Real2Complex(ih)
    assert np.allclose(u.to_hz(r.frequency), freqs + 32e3 * np.array([1, -1, 1]), rtol=0, atol=1e-3)
    assert np.array_equal(r.sideband, [1, -1, 1])
    assert getattr(bt.Real2Complex(stream((4000,), 2000)), 'frequency', None) is None


def test_polarization_passes_through():
    ih = stream((4000, 2), 2000, polarization=np.array(['X', 'Y']))
    r = bt.Real2Complex(ih)
    assert list(r.polarization) == ['X', 'Y']


# -- refusals -------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(ValueError, match='Stream should be real'):
        bt.Real2Complex(stream((4000,), 2000, dtype=np.complex64))
    with pytest.raises(ValueError, match='Stream should be real'):
        bt.Real2Complex(stream((4000,), 2000, dtype=np.complex128))
    with pytest.raises(TypeError, match='SinglePrecision'):
        bt.Real2Complex(stream((4000,), 2000, dtype=np.float64))
    with pytest.raises(ValueError, match='even number'):
        bt.Real2Complex(stream((4000,), 1001))
    for m in (1, 11, 8191, 2 * 8192 * 11):
        with pytest.raises(ValueError, match='2 <= n <= 8192'):
            bt.Real2Complex(stream((4 * m,), 2 * m), samples_per_frame=m)


def test_accepted_lengths():
    for m in (2, 3, 7, 500, 1215, 8192, 10000, 16384, 1 << 17, 1 << 20, 1 << 24, 8192 * 8192):
        check_r2c_length(m)
    for m in (1, 0, 13, 8192 * 8192 * 2, 8191 * 2):
        with pytest.raises(ValueError):
            check_r2c_length(m)


# -- the golden file's metadata -----------------------------------------------------------
def golden_cases():
    d = np.load(GOLDEN)
    return [(json.loads(str(d[k])), d[k[:-4] + 'input'], d[k[:-4] + 'output'])
            for k in sorted(d.files) if k.endswith('/meta')]


def test_golden_metadata():
    cases = golden_cases()
    assert sorted(c[0]['M'] for c in cases) == [2, 3, 7, 500, 1000, 1024, 1215, 4096, 6174, 10000, 16384]
    for meta, x, out in cases:
        m = meta['M']
        ih = bt.HostStream(x.astype(np.float32), T0, 64 * u.kHz, samples_per_frame=meta['ih_samples_per_frame'],
                           pin=False, **({} if meta.get('frequency') is None else
                                         dict(frequency=meta['frequency'], sideband=meta['sideband'])))
        r = bt.Real2Complex(ih) if meta.get('default') else bt.Real2Complex(ih, samples_per_frame=m)
        assert list(r.shape) == meta['shape'] == [m * meta['frames']] == list(out.shape)
        assert u.to_hz(r.sample_rate) == meta['sample_rate']
        assert r.samples_per_frame == meta['samples_per_frame']
        assert str(r.dtype) == meta['dtype'] == str(out.dtype)
        assert repr(r).startswith('Real2Complex(ih') and meta['repr'].startswith('Real2Complex(ih')
        assert (f'samples_per_frame={m}' in repr(r)) == (f'samples_per_frame={m}' in meta['repr'])
        if meta['out_frequency'] is None:
            assert getattr(r, 'frequency', None) is None
        else:
            assert u.to_hz(r.frequency) == meta['out_frequency'] and r.sideband == meta['out_sideband']
        # the host restatement of the identity reproduces the reference's output
        n = 2 * m
        xf = x[:meta['frames'] * n].astype(np.float64).reshape(meta['frames'], n)
        ours = np.concatenate([identity(np.stack([f, f], axis=1))[:, 0] for f in xf])
        err = np.linalg.norm(ours - out) / np.linalg.norm(out)
        assert err < 1e-6, (m, err)


# -- the one-pass kernel through hipRTC -----------------------------------------------------
def _hiprtc():
    for name in ('libhiprtc.so.7', 'libhiprtc.so', '/opt/rocm/lib/libhiprtc.so'):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    return None


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('r2c') / 'gen2_plan_dump')
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-I', CSRC, os.path.join(ROOT, 'tests', 'gen2_plan_dump.cpp'),
                           '-o', exe])
    return exe


@pytest.mark.parametrize('w', [0, 4])
@pytest.mark.parametrize('m', [7, 1215, 4096])
def test_one_pass_kernel_compiles_through_hiprtc(dump, m, w):
    """The translation unit bbt_r2c_plan_create writes for a one-pass length (the geometry traits
    of the length and its reversal, and the BBT_G2_KERNEL_R2C entry point), compiled as csrc/rtc.hpp
    compiles it, for gfx950: both launch-bound variants (W = 4 at most 128 registers, for workgroups of
    448 threads and more)."""
    rtc = _hiprtc()
    if rtc is None:
        pytest.skip('libhiprtc.so not found')
    src = subprocess.check_output([dump, 'source', str(m)], text=True)
    traits = ''.join(line + '\n' for line in src.splitlines() if line.startswith(('#include', 'BBT_G2_TRAIT')))
    src = traits + f'BBT_G2_KERNEL_R2C(k_r2c, GA, GB, {w})\n'     # (4: the bound plans of 448 threads and more take)
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b'bbt_g2.hip', 0, None, None) == 0
    opts = [b'--offload-arch=gfx950', b'-I' + CSRC.encode(), b'-O3', b'-std=c++17', b'-Wno-unused-value',
            b'-mllvm', b'-simplifycfg-sink-common=false']
    rc = rtc.hiprtcCompileProgram(prog, len(opts), (C.c_char_p * len(opts))(*opts))
    n = C.c_size_t()
    rtc.hiprtcGetProgramLogSize(prog, C.byref(n))
    log = C.create_string_buffer(n.value + 1)
    rtc.hiprtcGetProgramLog(prog, log)
    assert rc == 0, log.value.decode(errors='replace')[-2000:]
    assert rtc.hiprtcGetCodeSize(prog, C.byref(n)) == 0 and n.value > 10000
    code = C.create_string_buffer(n.value)
    assert rtc.hiprtcGetCode(prog, code) == 0
    rtc.hiprtcDestroyProgram(C.byref(prog))
    assert b'k_r2c' in code.raw
