"""Compact HDF5 payloads on the GPU: `hip.pack` (bbt_pack) against the codes of
`ingest.encode_vdif_frames`, `hip.to_half` / `hip.from_half` against ``astype``, files written from
device pieces against files written from host pieces, the decoding reader, and a task chain that
writes through ``read(out=writer)`` and reads a coded file back.  Everything is compared bit for bit
(one rel-L2 guard excepted, where two `Dedisperse` plans run on equal inputs)."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hdf5, hip, ingest
from baseband_tasks_amd import units as u
from conftest import rel_l2
from test_hdf5_coded_host import TIES_8, decode_words, keywords, levels, noise, stored, ties

pytestmark = pytest.mark.gpu

T0 = '2020-01-01T00:00:00'
BITS = (1, 2, 4, 8, 16)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


def pack_input():
    rng = np.random.default_rng(2024)
    hand = np.concatenate([
        np.array([-2., 0., 2., -0., 0.], np.float32),                       # every threshold, +-0
        ties(2.95, 8., range(15)), ties(35.5, 127.5, TIES_8),
        np.array([1000.5, 1001.5, -32768.5, 32766.5, 40000., -40000.], np.float32),      # 16-bit ties and ends
        np.array([1e9, -1e9, 3e38, -3e38, np.inf, -np.inf], np.float32)])   # far outside, +-inf
    return np.concatenate([rng.standard_normal(4096 + 37).astype(np.float32), hand])


def yardstick_words(comp, bits):
    """NumPy packing of the codes of `ingest.encode_vdif_frames`: the array padded with zeros to
    whole 64-bit words goes through the encoder itself; the padding's codes are cleared after."""
    n = comp.shape[0]
    per = 32 // bits
    padded = np.zeros(-(-n // 64) * 64, np.float32)
    padded[:n] = comp
    words = np.frombuffer(ingest.encode_vdif_frames(padded.reshape(-1, 1, 1), bits), '<u4')[8:].copy()
    words = words[:-(-n // per)]
    if n % per:
        words[-1] &= np.uint32((1 << (n % per) * bits) - 1)
    return words


@pytest.fixture(scope='module')
def packed():
    """The pack input, in HBM and on the host, and the yardstick's words for every width."""
    comp = pack_input()
    return comp, hip.DeviceArray.from_host(comp), {bits: yardstick_words(comp, bits) for bits in BITS}


@pytest.mark.parametrize('bits', BITS)
def test_pack_is_bit_exact(packed, bits):
    comp, dev, want = packed
    got = hip.pack(dev, bits)
    assert got.dtype == np.uint32 and got.shape == (-(-comp.shape[0] * bits // 32),)
    got = got.to_host()
    bad = np.nonzero(got != want[bits])[0]
    assert bad.size == 0, (bits, bad[:8], got[bad[:8]], want[bits][bad[:8]])
    # complex samples are (re, im) pairs of the same components
    pairs = hip.DeviceArray.from_host(comp[:4000].view(np.complex64))
    assert np.array_equal(hip.pack(pairs, bits).to_host(), yardstick_words(comp[:4000], bits))


@pytest.mark.parametrize('bits', BITS)
def test_pack_on_many_blocks_views_and_into_out(bits):
    """More than one workgroup at every width (a workgroup makes 256 to 1024 words), a ragged end,
    a view that is not 16-byte aligned (the scalar kernel) and a caller's output array."""
    rng = np.random.default_rng(bits)
    comp = (2. * rng.standard_normal(3 * 8192 + 32 * 5 + 3)).astype(np.float32)
    dev = hip.DeviceArray.from_host(comp)
    assert np.array_equal(hip.pack(dev, bits).to_host(), yardstick_words(comp, bits))
    view = dev[1:]
    assert view.ptr % 16 == 4
    out = hip.DeviceArray((-(-(comp.shape[0] - 1) * bits // 32) + 1,), np.uint32)
    res = hip.pack(view, bits, out=out[1:])
    assert res.ptr == out.ptr + 4
    assert np.array_equal(res.to_host(), yardstick_words(comp[1:], bits))
    nan = hip.DeviceArray.from_host(np.full(64, np.nan, np.float32))
    assert hip.pack(nan, bits).to_host().shape == (2 * bits,)              # (anything, without a fault)
    assert hip.pack(hip.DeviceArray((0,), np.float32), bits).shape == (0,)


def test_pack_and_half_argument_checks():
    x = hip.DeviceArray((64,), np.float32)
    with pytest.raises(ValueError, match='bits'):
        hip.pack(x, 3)
    with pytest.raises(TypeError, match='float32 or complex64'):
        hip.pack(hip.DeviceArray((64,), np.float64), 2)
    with pytest.raises(TypeError, match='DeviceArray'):
        hip.pack(np.zeros(64, np.float32), 2)
    with pytest.raises(ValueError, match='make 4'):
        hip.pack(x, 2, out=hip.DeviceArray((5,), np.uint32))
    with pytest.raises(TypeError, match='uint32'):
        hip.pack(x, 2, out=hip.DeviceArray((4,), np.int32))
    with pytest.raises(TypeError, match='float16'):
        hip.to_half(x, out=hip.DeviceArray((64,), np.float32))
    with pytest.raises(ValueError, match='63 values'):
        hip.to_half(x, out=hip.DeviceArray((63,), np.float16))
    h = hip.DeviceArray((64,), np.float16)
    with pytest.raises(TypeError, match='float16'):
        hip.from_half(x, np.float32)
    with pytest.raises(TypeError, match='float32 or complex64'):
        hip.from_half(h, np.float64)
    with pytest.raises(ValueError, match='last axis of 2'):
        hip.from_half(h, np.complex64)
    with pytest.raises(ValueError, match='halves'):
        hip.from_half(h, np.float32, out=hip.DeviceArray((32,), np.float32))
    lib = hip.lib()
    assert lib.bbt_pack(None, None, 8, 2, 0, None) != 0 and b'null' in lib.bbt_last_error()
    assert lib.bbt_pack(x.ptr, x.ptr, 8, 3, 0, None) != 0 and b'bits per component' in lib.bbt_last_error()
    assert lib.bbt_pack(x.ptr, x.ptr, 8, 2, 1, None) != 0 and b'code' in lib.bbt_last_error()
    assert lib.bbt_pack(x.ptr, x.ptr, -1, 2, 0, None) != 0
    assert lib.bbt_to_half(None, x.ptr, 8, None) != 0 and lib.bbt_from_half(x.ptr, None, 8, None) != 0


def half_input():
    rng = np.random.default_rng(7)
    normals = (rng.standard_normal(2048) * np.exp(4 * rng.standard_normal(2048))).astype(np.float32)
    subnormal = np.exp(rng.uniform(np.log(1e-8), np.log(6e-5), 2048)).astype(np.float32)      # the subnormal half range
    subnormal[::2] *= -1
    hand = np.array([65504., 65520., 1e6, 0., -0.], np.float32)            # largest half, the overflow tie, overflow, +-0
    x = np.concatenate([normals, subnormal, hand])
    # exact rounding ties, to even both ways; the smallest subnormal's tie; values that round to inf
    x[:8] = [1 + 2.**-11, 1 + 3 * 2.**-11, -(1 + 2.**-11), 2.**-25, 3 * 2.**-25, 65519.996, -65520., 2.**-24]
    assert x.shape == (4096 + 5,)
    return x


def test_half_conversions_are_bit_exact():
    x = half_input()
    with np.errstate(over='ignore'):
        want = x.astype('<f2')
    dev = hip.DeviceArray.from_host(x)
    h = hip.to_half(dev)
    assert h.dtype == np.float16 and h.shape == x.shape
    got = h.to_host()
    bad = np.nonzero(got.view(np.uint16) != want.view(np.uint16))[0]
    assert bad.size == 0, (bad[:8], x[bad[:8]], got[bad[:8]], want[bad[:8]])
    assert np.isinf(got[-5 + 1]) and np.isinf(got[-5 + 2]) and got[-5] == 65504. and np.signbit(got[-1])
    # back: exact, subnormal halves included -- every finite half there is, and the infinities
    every = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    every = every[~np.isnan(every)]
    back = hip.from_half(hip.DeviceArray.from_host(every), np.float32).to_host()
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), every.astype('<f4').view(np.uint32))
    assert np.array_equal(hip.from_half(h, np.float32).to_host().view(np.uint32), want.astype('<f4').view(np.uint32))
    # a NaN stays a NaN, both ways
    nan = hip.DeviceArray.from_host(np.array([np.nan, 1., -np.nan, 2.] * 2, np.float32))
    n16 = hip.to_half(nan)
    assert np.array_equal(np.isnan(n16.to_host()), [True, False, True, False] * 2)
    assert np.array_equal(np.isnan(hip.from_half(n16).to_host()), [True, False, True, False] * 2)
    # views that are not 16-byte aligned (the scalar kernels), complex pairs
    assert np.array_equal(hip.to_half(dev[3:]).to_host().view(np.uint16), want[3:].view(np.uint16))
    assert np.array_equal(hip.from_half(h[1:]).to_host(), want[1:].astype('<f4'))
    z = hip.DeviceArray.from_host(x[:4096].view(np.complex64).reshape(1024, 2))
    hz = hip.to_half(z)
    assert hz.shape == (1024, 2, 2) and np.array_equal(hz.to_host().ravel().view(np.uint16), want[:4096].view(np.uint16))
    assert np.array_equal(hip.from_half(hz, np.complex64).to_host(),
                          want[:4096].astype('<f4').view(np.complex64).reshape(1024, 2))


@pytest.mark.parametrize('bits', [2, 4, 8])
def test_pack_then_unpack_gives_the_level_of_each_code(packed, bits):
    comp, dev, want = packed
    n = comp.shape[0]
    words = hip.pack(dev, bits)
    out = hip.DeviceArray((n,), np.float32)
    # the payload as one headerless frame of n one-component samples
    hip.check(hip.lib().bbt_unpack(words.ptr, out.ptr, 1, words.nbytes, 0, bits, n, 1, 1, 0, hip.get_stream()))
    per = 32 // bits
    codes = ((want[bits][:, None] >> (np.arange(per, dtype=np.uint32) * np.uint32(bits)))
             & np.uint32((1 << bits) - 1)).ravel()[:n]
    assert np.array_equal(out.to_host(), levels(codes, bits))


# --------------------------------------------------------------------------- files
CASES = [('complex', dict(bps=2)), ('complex', dict(bps=8)), ('complex', dict(encoded_dtype='c4')),
         ('real', dict(encoded_dtype='f2')), ('real', dict(bps=4))]
META = dict(frequency=np.array([1000e6, 1001e6]), sideband=np.array([1, -1]), polarization=np.array(['X', 'Y']))


def samples(kind):
    return noise((2048, 2), np.complex64) if kind == 'complex' else noise((2048,), np.float32)


def write(name, x, how, pieces, device):
    dev = hip.DeviceArray.from_host(x) if device else None
    with hdf5.open(name, 'w', **keywords(x, meta=x.ndim > 1), **how) as fw:
        for a, b in zip(pieces[:-1], pieces[1:]):
            fw[a:b] = dev[a:b] if device else x[a:b]
    return name


def decoded(x, how):
    """What a reader must return: the level of every code / the samples rounded to half precision."""
    comp = x.view(np.float32).ravel()
    if 'bps' in how:
        bits = how['bps']
        got = decode_words(hdf5.encode_words(x, bits), bits, comp.shape[0])
    else:
        got = comp.astype('<f2').astype('<f4')
    return got.view(x.dtype).reshape(x.shape)


@pytest.mark.parametrize('kind, how', CASES)
def test_device_and_host_pieces_give_identical_files(tmp_path, kind, how):
    x = samples(kind)
    # (device pieces: one that starts off a 16-byte boundary for the real half-precision file)
    cuts = [0, 1001, 2048] if 'encoded_dtype' in how else [0, 1000, 2048]
    a = write(str(tmp_path / 'device.h5'), x, how, cuts, device=True)
    b = write(str(tmp_path / 'host.h5'), x, how, [0, 512, 2048], device=False)
    with open(a, 'rb') as fa, open(b, 'rb') as fb:
        assert fa.read() == fb.read()
    items, data, shape, elem, cls = stored(a)
    want = hdf5.encode_words(x, how['bps']) if 'bps' in how else x.view(np.float32).astype('<f2')
    assert data == want.tobytes()


@pytest.mark.parametrize('kind, how', CASES)
def test_round_trip_through_the_reader(tmp_path, kind, how):
    x = samples(kind)
    name = write(str(tmp_path / 'a.h5'), x, how, [0, 1000, 2048], device=True)
    want = decoded(x, how)
    fr = hdf5.open(name)
    assert isinstance(fr, hdf5.HDF5EncodedStreamReader) and fr.samples_per_frame == 2048
    assert fr.shape == x.shape and fr.dtype == x.dtype and fr.sample_rate == 16e6
    assert fr.start_time == bt.Time('2020-01-01T00:00:00.5')
    if kind == 'complex':
        assert np.array_equal(np.ravel(fr.frequency), [1000e6, 1001e6]) and list(np.ravel(fr.sideband)) == [1, -1]
        assert [str(p) for p in np.ravel(fr.polarization)] == ['X', 'Y']
    got = fr.read()
    assert got.dtype == x.dtype and np.array_equal(got.view(np.float32), want.view(np.float32))
    fr.close()
    # frames of 512 samples: a read that starts inside a frame and crosses into the next
    fr = hdf5.open(name, samples_per_frame=512)
    assert fr.samples_per_frame == 512
    fr.seek(1000)
    assert np.array_equal(fr.read(100), want[1000:1100])
    fr.seek(0)
    assert np.array_equal(fr.read(), want)
    fr.close()


def test_a_shorter_last_frame_and_a_partial_last_word(tmp_path):
    """2045 real samples at 4 bits in frames of 512: the last frame is short and ends inside a word."""
    x = noise((2045,), np.float32)
    name = write(str(tmp_path / 'a.h5'), x, dict(bps=4), [0, 1000, 2045], device=True)
    want = decoded(x, dict(bps=4))
    fr = hdf5.open(name, samples_per_frame=512)
    assert fr.granule == 8 and np.array_equal(fr.read(), want)
    fr.seek(2000)
    assert np.array_equal(fr.read(45), want[2000:])
    with pytest.raises(ValueError, match='granule'):
        hdf5.open(name, samples_per_frame=100)
    # decoded and coded again on the GPU, piece by piece: the same words (512 is a multiple of the granule)
    fr.seek(0)
    fr.max_frames_per_call = 1
    with hdf5.open(str(tmp_path / 'b.h5'), 'w', template=fr, bps=4) as fw:
        fr.read(out=fw)
    assert stored(str(tmp_path / 'b.h5'))[1] == stored(name)[1]


# --------------------------------------------------------------------------- task chains
class CountingWriter(hdf5.HDF5StreamWriter):
    device_pieces = host_pieces = 0

    def write(self, data):
        if isinstance(data, hip.DeviceArray):
            self.device_pieces += 1
        else:
            self.host_pieces += 1
        super().write(data)


def stream(n=2**15):
    x = noise((n, 2), np.complex64, seed=5)
    return x, dict(frequency=400 * u.MHz, sideband=np.array([1, -1]))


def test_a_pipeline_writes_half_precision_from_device_pieces(tmp_path):
    x, meta = stream()
    ds = bt.DeviceStream(x, T0, 1 * u.MHz, **meta)
    ch = bt.Channelize(bt.Dedisperse(ds, 10.), 64)
    plain = ch.read()
    assert plain.shape[1:] == (64, 2) and plain.shape[0] >= 256
    ch.seek(0)
    ch.max_frames_per_call = 100                                # (several pieces)
    name = str(tmp_path / 'a.h5')
    with CountingWriter(name, template=ch, encoded_dtype='c4') as fw:
        assert ch.read(out=fw) is fw
        assert fw.device_pieces >= 2 and fw.host_pieces == 0 and fw.tell() == plain.shape[0]
    items, data, shape, elem, cls = stored(name)
    assert shape == plain.shape and items['encoded_dtype'] == '<c4'
    assert data == plain.view(np.float32).astype('<f2').tobytes()
    # other targets of read(out=...) see host arrays, as before
    ch.seek(0)
    out = np.empty(plain.shape, plain.dtype)
    assert np.array_equal(ch.read(out=out), plain)


def test_a_coded_file_feeds_a_task(tmp_path):
    x, meta = stream()
    name = str(tmp_path / 'a.h5')
    with hdf5.open(name, 'w', shape=x.shape, start_time=T0, sample_rate=1e6, dtype=x.dtype, bps=8,
                   frequency=np.array([400e6, 400e6]), sideband=np.array([1, -1])) as fw:
        fw.write(hip.DeviceArray.from_host(x))
    want_in = decoded(x, dict(bps=8))
    fr = hdf5.open(name, samples_per_frame=512)
    ds = bt.DeviceStream(want_in, T0, 1 * u.MHz, samples_per_frame=512, frequency=np.array([400e6, 400e6]),
                         sideband=np.array([1, -1]))
    pad = (lambda d: d._pad_start + d._pad_end)(bt.Dedisperse(ds, 10.))
    assert 0 < pad < 4096
    spf = 8192 - pad                                            # (blocks of 2^13 samples, several of them)
    got = bt.Dedisperse(fr, 10., samples_per_frame=spf).read()
    want = bt.Dedisperse(ds, 10., samples_per_frame=spf).read()
    assert got.shape == want.shape and got.shape[0] > 2**14
    err = rel_l2(got, want)
    print(f'coded file -> Dedisperse: rel-L2 {err:.3e}, equal {np.array_equal(got, want)}')
    # (two routes over equal inputs, as the fused / unfused comparisons of tests/test_gpu_parity.py)
    assert err < 3e-7
