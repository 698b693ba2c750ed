"""PSRFITS fold-mode coding on the GPU: `hip.psrfits_encode` / `hip.psrfits_decode` against the NumPy
restatement `psrfits.encode_rows` / `decode_rows` byte for byte, the reader on the reference's real
archive against psrchive's read-out, and a fold streamed into an archive through
``read(out=writer)`` and read back."""
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, psrfits
from baseband_tasks_amd import units as u
import psrfits_cases as pc
from test_psrfits_host import ARCHIVE, READ_OUT, profiles

pytestmark = pytest.mark.gpu

#: (rows, bins, chan, pol), from tests/psrfits_cases.py, where the host tests prove which instantiations
#: and edges of the tiling they reach
SHAPES = pc.FOLD_SHAPES
SHIFTED = pc.FOLD_SHIFTED            # as a view 4 bytes into an allocation: the unaligned path
SHIFTED_CODES = pc.FOLD_SHIFTED_CODES    # codes 2 bytes into their allocation, the floats aligned
#: (in the order in which the tests got their names)
PARAMS = pc.FOLD_OLD + [SHIFTED] + pc.FOLD_NEW


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


def shifted(a, by=4):
    """``a`` in HBM as a view that starts ``by`` bytes into its allocation."""
    flat = np.ascontiguousarray(a).ravel()
    per = by // flat.dtype.itemsize
    room = hip.DeviceArray((flat.size + per,), flat.dtype)
    view = room[per:]
    view.copy_from_host(flat)
    assert view.ptr % 16 == by
    return view.reshape(a.shape)


@pytest.fixture(scope='module')
def cases():
    """shape -> (profiles, what `encode_rows` makes of them), made once."""
    out = {}
    for shape in SHAPES + [SHIFTED]:
        x = profiles(shape, seed=sum(shape))
        out[shape] = x, psrfits.encode_rows(x)
    return out


def same_bytes(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.nonzero((got.view(np.uint8) != want.view(np.uint8)).ravel())[0]
    assert bad.size == 0, (bad.size, bad[:8])


@pytest.mark.parametrize('shape', PARAMS)
def test_encode_is_byte_exact(cases, shape):
    x, want = cases[shape]
    dev = shifted(x) if shape == SHIFTED else hip.DeviceArray.from_host(x)
    got = hip.psrfits_encode(dev)
    assert got[0].dtype == np.dtype('>i2') and got[0].shape == (shape[0], shape[3], shape[2], shape[1])
    for g, w in zip(got, want):
        same_bytes(g.to_host(), np.ascontiguousarray(w))


def test_encode_into_codes_off_a_dword(cases):
    """Aligned profiles, through the C ABI into codes that start 2 bytes into their allocation: a shape
    that has float4 loads and dword stores otherwise runs the scalar kernel because of that pointer
    alone; nothing is stored before the first code or after the last."""
    x, want = cases[SHIFTED_CODES]
    n_row, n_bin, n_chan, n_pol = SHIFTED_CODES
    dev = hip.DeviceArray.from_host(x)
    room = hip.DeviceArray((want[0].size + 2,), np.dtype('>i2'))
    room.copy_from_host(np.full(room.size, 0x5a5a, np.dtype('>i2')))
    scl, offs = hip.DeviceArray(want[1].shape, np.float32), hip.DeviceArray(want[2].shape, np.float32)
    n_finite = hip.DeviceArray(want[3].shape, np.int32)
    assert dev.ptr % 16 == 0 and (room.ptr + 2) % 4 == 2
    hip.check(hip.lib().bbt_psrfits_encode(dev.ptr, room.ptr + 2, scl.ptr, offs.ptr, n_finite.ptr, n_row, n_bin,
                                           n_chan, n_pol, None))
    back = room.to_host()
    assert back[0] == 0x5a5a and back[-1] == 0x5a5a
    got = back[1:-1].reshape(want[0].shape), scl.to_host(), offs.to_host(), n_finite.to_host()
    for g, w in zip(got, want):
        same_bytes(g, np.ascontiguousarray(w))


def test_decode_of_codes_off_a_dword(cases):
    """The same the other way: codes 2 bytes into their allocation, ``out`` aligned."""
    shape = SHIFTED_CODES
    _, (codes, scl, offs, _) = cases[shape]
    d_codes, d_scl, d_offs = shifted(codes, 2), hip.DeviceArray.from_host(scl), hip.DeviceArray.from_host(offs)
    got = hip.psrfits_decode(d_codes, d_scl, d_offs)
    assert got.ptr % 16 == 0
    same_bytes(got.to_host(), psrfits.decode_rows(codes, scl, offs))
    wts = np.random.default_rng(3).integers(0, 3, (shape[0], shape[2])).astype(np.float32) * np.float32(0.7)
    out = hip.DeviceArray((shape[0] * shape[1] * shape[2] * shape[3] + 1,), np.float32)
    view = out[:out.size - 1]
    res = hip.psrfits_decode(d_codes, d_scl, d_offs, hip.DeviceArray.from_host(wts), zero_off=0.5, out=view)
    assert res.ptr == view.ptr and res.ptr % 16 == 0
    same_bytes(res.to_host().reshape(shape), psrfits.decode_rows(codes, scl, offs, wts, zero_off=0.5))


@pytest.mark.parametrize('shape', PARAMS)
def test_decode_is_exact(cases, shape):
    _, (codes, scl, offs, _) = cases[shape]
    up = shifted if shape == SHIFTED else hip.DeviceArray.from_host
    d_codes, d_scl, d_offs = up(codes), hip.DeviceArray.from_host(scl), hip.DeviceArray.from_host(offs)
    same_bytes(hip.psrfits_decode(d_codes, d_scl, d_offs).to_host(), psrfits.decode_rows(codes, scl, offs))
    wts = np.random.default_rng(3).integers(0, 3, (shape[0], shape[2])).astype(np.float32) * np.float32(0.7)
    out = hip.DeviceArray((shape[0] * shape[1] * shape[2] * shape[3] + 1,), np.float32)
    view = out[1:] if shape == SHIFTED else out[:out.size - 1]
    res = hip.psrfits_decode(d_codes, d_scl, d_offs, hip.DeviceArray.from_host(wts), zero_off=0.5, out=view)
    assert res.ptr == view.ptr
    same_bytes(res.to_host().reshape(shape), psrfits.decode_rows(codes, scl, offs, wts, zero_off=0.5))


def test_argument_checks():
    x = hip.DeviceArray((2, 4, 3), np.float32)
    assert [a.shape for a in hip.psrfits_encode(x)] == [(2, 1, 3, 4), (2, 1, 3), (2, 1, 3), (2, 1, 3)]
    assert hip.psrfits_encode(hip.DeviceArray((0, 4), np.float32))[0].shape == (0, 1, 1, 4)
    with pytest.raises(TypeError):
        hip.psrfits_encode(hip.DeviceArray((2, 4), np.complex64))
    with pytest.raises(ValueError):
        hip.psrfits_encode(hip.DeviceArray((4,), np.float32))
    codes, scl, offs, _ = hip.psrfits_encode(x)
    with pytest.raises(TypeError):
        hip.psrfits_decode(scl, scl, offs)
    with pytest.raises(ValueError):
        hip.psrfits_decode(codes, scl, offs, out=hip.DeviceArray((5,), np.float32))
    lib = hip.lib()
    assert lib.bbt_psrfits_encode(None, None, None, None, None, 1, 1, 1, 1, None) != 0
    assert b'null' in lib.bbt_last_error()
    assert lib.bbt_psrfits_encode(x.ptr, codes.ptr, scl.ptr, offs.ptr, offs.ptr, 1, 0, 1, 1, None) != 0
    assert b'bins' in lib.bbt_last_error()
    assert lib.bbt_psrfits_decode(codes.ptr + 1, scl.ptr, offs.ptr, None, 0., x.ptr, 1, 4, 3, 1, None) != 0
    assert b'aligned' in lib.bbt_last_error()


# -- the reader on the reference's archive ---------------------------------------------------
def test_reader_gives_psrchives_read_out():
    want = np.load(READ_OUT)['data'].reshape(1, 2048, 1, 1)
    with psrfits.open(ARCHIVE, weighted=False) as fh:
        got = fh.read()
        assert got.dtype == np.float32 and np.all(got == want)
        with pytest.raises(EOFError):
            fh.read(1)
        fh.seek(0)
        dev = fh.read_device(1)
        assert isinstance(dev, hip.DeviceArray) and np.all(dev.to_host() == want)
    with psrfits.open(ARCHIVE) as fh:                                      # weighted
        assert np.all(fh.read() == want * np.float32(70412.96))
        # a task on top runs on the device stream
        summed = bt.Integrate(fh, 1).read()
        assert np.all(summed == want * np.float32(70412.96))


# -- a fold into an archive and back --------------------------------------------------------------
T0 = bt.Time('2020-01-01T00:00:00') + 0.25
RATE = 1. * u.MHz
F0 = 1000. / 3.


def phase(t):
    return F0 * (t - T0)


@pytest.fixture(scope='module')
def folded():
    rng = np.random.default_rng(11)
    z = (rng.standard_normal((1 << 16, 2)) + 1j * rng.standard_normal((1 << 16, 2))).astype(np.complex64)
    sh = bt.DeviceStream(hip.DeviceArray.from_host(z), T0, RATE, samples_per_frame=1 << 12,
                         frequency=400. * u.MHz, sideband=1, polarization=['X', 'Y'])
    power = bt.Power(bt.Channelize(sh, 16))
    fold = bt.Fold(power, 8, phase, step=1 << 10)
    assert fold.shape == (4, 8, 16, 4)
    return power, fold, fold.read()


def test_fold_streams_into_an_archive(folded, tmp_path):
    power, fold, profiles4 = folded
    name, host_name = str(tmp_path / 'fold.fits'), str(tmp_path / 'host.fits')
    fold.seek(0)
    with psrfits.open(name, 'w', template=fold, primary={'TELESCOP': 'nowhere'}) as fw:
        fold.read(out=fw)
        assert fw.tell() == 4
    with psrfits.open(host_name, 'w', template=fold, primary={'TELESCOP': 'nowhere'}) as fw:
        fw.write(profiles4[:3])
        fw.write(profiles4[3:])
    with open(name, 'rb') as a, open(host_name, 'rb') as b:
        assert a.read() == b.read()
    with psrfits.open(name) as fh:
        assert fh.shape == fold.shape and fh.dtype == fold.dtype
        assert abs(fh.sample_rate / fold.sample_rate - 1) < 1e-15
        assert abs(fh.start_time - fold.start_time) < 1e-9
        want_f = np.broadcast_to(fold.frequency, fold.sample_shape)
        assert np.allclose(np.broadcast_to(fh.frequency, fh.sample_shape), want_f, rtol=1e-15, atol=0)
        assert np.all(np.broadcast_to(fh.sideband, fh.sample_shape) == np.broadcast_to(fold.sideband, fold.sample_shape))
        assert np.all(np.broadcast_to(fh.polarization, fh.sample_shape)
                      == np.broadcast_to(fold.polarization, fold.sample_shape))
        assert fh.primary['TELESCOP'] == 'nowhere'
        back = fh.read()
    # half a code step, and the roundings of coder and decoder: tests/test_psrfits_host.py
    scl = psrfits.encode_rows(profiles4)[1].astype(np.float64).transpose(0, 2, 1)      # (row, chan, pol)
    bound = 0.51 * scl + 4 * 2. ** -23 * np.abs(profiles4).max(axis=1)
    err = np.abs(back.astype(np.float64) - profiles4).max(axis=1)
    assert np.all(np.isfinite(profiles4)) and np.all(err <= bound), (err / bound).max()


def test_full_stokes_fold_of_few_channels_streams_into_an_archive(tmp_path):
    """5 channels x 4 polarizations with 64 phase bins: 20 columns, so one thread owns the four
    columns of a tile and 256 threads run along the bins (<4,vec>), under the writer."""
    rng = np.random.default_rng(12)
    z = (rng.standard_normal((1 << 15, 5, 2)) + 1j * rng.standard_normal((1 << 15, 5, 2))).astype(np.complex64)
    sh = bt.DeviceStream(hip.DeviceArray.from_host(z), T0, RATE, samples_per_frame=1 << 12,
                         frequency=(400. + np.arange(5))[:, None] * u.MHz, sideband=1, polarization=['X', 'Y'])
    fold = bt.Fold(bt.Power(sh), 64, phase, step=1 << 13)             # (2.7 turns a row: no empty bin)
    assert fold.shape == (4, 64, 5, 4)
    profiles4 = fold.read()
    name, host_name = str(tmp_path / 'fold.fits'), str(tmp_path / 'host.fits')
    fold.seek(0)
    with psrfits.open(name, 'w', template=fold) as fw:
        fold.read(out=fw)
        assert fw.tell() == 4
    with psrfits.open(host_name, 'w', template=fold) as fw:
        fw.write(profiles4[:3])
        fw.write(profiles4[3:])
    with open(name, 'rb') as a, open(host_name, 'rb') as b:
        assert a.read() == b.read()
    codes, scl, offs, _ = psrfits.encode_rows(profiles4)
    with psrfits.open(name, weighted=False) as fh:
        assert fh.shape == fold.shape and fh.dtype == fold.dtype
        back = fh.read()
    same_bytes(back, psrfits.decode_rows(codes, scl, offs))
    # half a code step, and the roundings of coder and decoder: tests/test_psrfits_host.py
    bound = 0.51 * scl.astype(np.float64).transpose(0, 2, 1) + 4 * 2. ** -23 * np.abs(profiles4).max(axis=1)
    err = np.abs(back.astype(np.float64) - profiles4).max(axis=1)
    assert np.all(np.isfinite(profiles4)) and np.all(err <= bound), (err / bound).max()


def test_writer_refuses_complex_and_counted_streams(folded, tmp_path):
    power, fold, _ = folded
    name = str(tmp_path / 'no.fits')
    with pytest.raises(TypeError, match='complex'):
        psrfits.open(name, 'w', template=power.ih)
    with pytest.raises(TypeError, match='average'):
        psrfits.open(name, 'w', template=bt.Fold(power, 8, phase, step=1 << 10, average=False))
    with pytest.raises(TypeError, match='uniform'):
        psrfits.open(name, 'w', template=bt.PulseStack(power, 8, phase))
    assert not os.path.exists(name)
