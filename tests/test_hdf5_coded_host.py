"""Compact payloads of the HDF5 sink (baseband_tasks_amd/hdf5.py; reference io/hdf5/header.py:227-307,
payload.py:121-178): ``bps``-coded words and half-precision ('<f2' / '<c4') samples.  CPU tests: the
header text, the payload sizes, the NumPy encoders against `ingest.encode_vdif_frames` and against a
NumPy decode of the bytes found in the file, the argument errors -- and the datatypes as the REAL h5py
read them once (tests/golden/compact_h5py.json), the writer held to the bytes it read."""
import hashlib
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hdf5, ingest

HERE = os.path.dirname(os.path.abspath(__file__))
REQUIRED = ['sample_rate', 'sample_shape', 'samples_per_frame', 'time']
OPTIONAL = ['frequency', 'polarization', 'sideband']


def noise(shape, dtype, seed=11):
    rng = np.random.default_rng(seed)
    x = (1.5 * rng.standard_normal(tuple(shape) + (2,))).astype(np.float32)
    return x.view(np.complex64)[..., 0] if np.dtype(dtype).kind == 'c' else np.ascontiguousarray(x[..., 0])


def keywords(x, meta=True):
    kw = dict(shape=x.shape, start_time='2020-01-01T00:00:00.5', sample_rate=16e6, dtype=x.dtype)
    if meta:
        kw.update(frequency=np.array([1000e6, 1001e6]), sideband=np.array([1, -1]), polarization=np.array(['X', 'Y']))
    return kw


def stored(name):
    """(header items, payload bytes, payload shape, element size, datatype class) through `hdf5._File`."""
    raw = np.memmap(name, mode='r')
    f = hdf5._File(raw)
    links = f.links(f.root)
    items = hdf5.parse_header(f.text(links['header']))
    address, size, shape, elem, cls, inline = f.dataset(links['payload'])
    assert inline is None and address + size == raw.shape[0]
    return items, bytes(raw[address:address + size]), tuple(shape), elem, cls


def decode_words(words, bps, n_comp):
    """NumPy restatement of `unpack_level` (csrc/bbt_kernels.hpp), code 0: the first component in the
    least significant bits."""
    words = np.frombuffer(words, '<u4') if isinstance(words, bytes) else np.asarray(words, '<u4')
    per = 32 // bps
    shifts = (np.arange(per, dtype=np.uint32) * np.uint32(bps))
    codes = ((words[:, None] >> shifts) & np.uint32((1 << bps) - 1)).ravel()[:n_comp]
    return levels(codes, bps)


def levels(codes, bps):
    v = codes.astype(np.float32)
    if bps == 1:
        return np.where(codes != 0, np.float32(1), np.float32(-1))
    if bps == 2:
        return np.array([-3.3359, -1., 1., 3.3359], np.float32)[codes]
    if bps == 4:
        return (v - np.float32(8)) / np.float32(2.95)
    if bps == 8:
        return (v - np.float32(127.5)) / np.float32(35.5)
    return v - np.float32(32768)


def vdif_words(x, bps):
    """The payload words `ingest.encode_vdif_frames` (the yardstick) makes of samples whose components
    fill whole 64-bit words."""
    comp = x.view(np.float32).reshape(-1)
    frames = ingest.encode_vdif_frames(comp.reshape(-1, 1, 1), bps)
    return np.frombuffer(frames, '<u4')[8:]


#: 8-bit codes whose lower tie (k + 0.5 - 127.5) / 35.5 a fused multiply-add rounds the other way
#: (found with `fused_codes` below), and a few that it does not
TIES_8 = (0, 2, 3, 4, 5, 6, 13, 14, 15, 16, 100, 200, 254)


def ties(scale, offset, codes):
    """float32 inputs whose float32 product and sum land on (or right beside) code + 0.5."""
    return np.array([(k + 0.5 - offset) / scale for k in codes], np.float32)


# --------------------------------------------------------------------------- header text
@pytest.mark.parametrize('how', ['bps', 'c4', 'f2'])
def test_header_text_has_the_references_keys(tmp_path, how):
    x = noise((64, 2), np.float32 if how == 'f2' else np.complex64)
    extra = dict(bps=2) if how == 'bps' else dict(encoded_dtype=how)
    with hdf5.open(str(tmp_path / 'a.h5'), 'w', **keywords(x), **extra) as fw:
        text = fw.header_text
        fw.write(x)
    items = hdf5.parse_header(text)
    if how == 'bps':
        assert sorted(items) == sorted(['bps', 'complex_data'] + REQUIRED + OPTIONAL)
        assert items['bps'] == 2 and items['complex_data'] is True and 'dtype' not in items
    else:
        assert sorted(items) == sorted(['dtype', 'encoded_dtype'] + REQUIRED + OPTIONAL)
        assert items['dtype'] == ('float32' if how == 'f2' else 'complex64')
        assert items['encoded_dtype'] == ('<f2' if how == 'f2' else '<c4')
    assert items['sample_shape'] == (2,) and items['samples_per_frame'] == 64 and items['sample_rate'] == 16e6
    assert items['time'] == bt.Time('2020-01-01T00:00:00.5')
    assert np.array_equal(items['frequency'], [1000e6, 1001e6]) and list(items['sideband']) == [1, -1]
    # and the text in the file is that text
    assert stored(str(tmp_path / 'a.h5'))[0].keys() == items.keys()


def test_raw_header_is_unchanged(tmp_path):
    """A file written without the new keywords has the header it always had."""
    x = noise((10, 2), np.complex64)
    with hdf5.open(str(tmp_path / 'a.h5'), 'w', **keywords(x)) as fw:
        fw.write(x)
        assert fw.bps is None and fw.encoded_dtype is None and fw.granule == 1
    kw = keywords(x)
    want = hdf5.header_yaml((2,), 10, 16e6, kw['start_time'], x.dtype, frequency_hz=kw['frequency'],
                            sideband=kw['sideband'], polarization=kw['polarization'])
    raw = np.memmap(str(tmp_path / 'a.h5'), mode='r')
    f = hdf5._File(raw)
    assert f.text(f.links(f.root)['header']) == want and want.startswith('dtype: <c8\n')
    assert sorted(hdf5.parse_header(want)) == sorted(['dtype'] + REQUIRED + OPTIONAL)


# --------------------------------------------------------------------------- payload sizes
def test_coded_payload_sizes(tmp_path):
    x = noise((1000, 3), np.complex64)                   # 6000 components at 2 bits: 375 words
    name = str(tmp_path / 'a.h5')
    with hdf5.open(name, 'w', **keywords(x, meta=False), bps=2) as fw:
        assert fw.granule == 8                           # 6 components x 2 bits: 8 samples fill 3 words
        fw.write(x)
    items, data, shape, elem, cls = stored(name)
    assert shape == (375,) and elem == 4 and cls == 0 and len(data) == 1500
    y = noise((7,), np.float32)                          # 7 components at 4 bits: one partial word
    name = str(tmp_path / 'b.h5')
    with hdf5.open(name, 'w', **keywords(y, meta=False), bps=4) as fw:
        assert fw.granule == 8
        fw.write(y)
    items, data, shape, elem, cls = stored(name)
    assert shape == (1,) and len(data) == 4
    word = int(np.frombuffer(data, '<u4')[0])
    assert word >> 28 == 0                               # the unused high bits are zero
    assert np.array_equal(decode_words(data, 4, 7), levels(np.clip(np.rint(y * 2.95 + 8.), 0, 15).astype(np.uint32), 4))


def test_half_payload_sizes(tmp_path):
    x = noise((100, 2), np.complex64)
    name = str(tmp_path / 'a.h5')
    with hdf5.open(name, 'w', **keywords(x), encoded_dtype='complex32') as fw:
        fw.write(x)
    items, data, shape, elem, cls = stored(name)
    assert shape == (100, 2) and elem == 4 and cls == 6 and len(data) == 800
    y = noise((33,), np.float32)
    name = str(tmp_path / 'b.h5')
    with hdf5.open(name, 'w', **keywords(y, meta=False), encoded_dtype='<f2') as fw:
        fw.write(y)
    items, data, shape, elem, cls = stored(name)
    assert shape == (33,) and elem == 2 and cls == 1 and len(data) == 66


# --------------------------------------------------------------------------- the NumPy encoders
@pytest.mark.parametrize('bps', [1, 2, 4, 8, 16])
def test_encode_words_makes_the_yardsticks_words(bps):
    x = noise((512,), np.float32, seed=bps)
    if bps == 16:
        x *= 3000
    x[:12] = [-2, 0, 2, -0., 1e9, -1e9, np.inf, -np.inf, 0.5 / 2.95, 1.5 / 2.95, 0.5 / 35.5, 1.]
    words = hdf5.encode_words(x, bps)
    assert words.dtype == np.dtype('<u4') and np.array_equal(words, vdif_words(x, bps))
    z = noise((256,), np.complex64, seed=bps)
    assert np.array_equal(hdf5.encode_words(z, bps), vdif_words(z, bps))
    # a ragged count: the words of the padded array with the padding's codes cleared
    n = 512 - 37
    ragged = hdf5.encode_words(x[:n], bps)
    per = 32 // bps
    assert ragged.shape == (-(-n // per),)
    assert np.array_equal(ragged[:n // per], words[:n // per])
    if n % per:
        assert ragged[-1] == words[n // per] & np.uint32((1 << (n % per) * bps) - 1)
    assert hdf5.encode_words(np.array([np.nan], np.float32), bps)[0] == 0


@pytest.mark.parametrize('how', [dict(bps=2), dict(bps=8), dict(encoded_dtype='c4')])
def test_host_pieces_round_trip_at_the_byte_level(tmp_path, how):
    """Files written from ndarray pieces, decoded with NumPy from the bytes `hdf5._File` finds."""
    x = noise((2048, 2), np.complex64)
    name = str(tmp_path / 'a.h5')
    with hdf5.open(name, 'w', **keywords(x), **how) as fw:
        fw.write(x[:1024])
        fw[1024:1536] = x[1024:1536]
        fw.write(x[1536:])
        with pytest.raises(EOFError):
            fw.write(x[:8])
    items, data, shape, elem, cls = stored(name)
    comp = x.view(np.float32).ravel()
    if 'bps' in how:
        bps = how['bps']
        assert shape == (8192 * bps // 32,)
        codes = (np.searchsorted(np.array([-2., 0., 2.]), comp) if bps == 2
                 else np.clip(np.rint(comp * 35.5 + 127.5), 0, 255)).astype(np.uint32)
        assert np.array_equal(decode_words(data, bps, 8192), levels(codes, bps))
    else:
        got = np.frombuffer(data, hdf5.DTYPE_C4).reshape(shape)
        assert np.array_equal(got['real'], x.real.astype('<f2')) and np.array_equal(got['imag'], x.imag.astype('<f2'))


@pytest.mark.parametrize('how', [dict(bps=4), dict(encoded_dtype='f2')])
def test_real_host_pieces_round_trip_at_the_byte_level(tmp_path, how):
    x = noise((2045,), np.float32)
    name = str(tmp_path / 'a.h5')
    # half precision: pieces end anywhere; 4 bits: on multiples of the granule, 8, but for the last
    cuts = [0, 1000, 2040, 2045] if 'bps' in how else [0, 1001, 2043, 2045]
    with hdf5.open(name, 'w', **keywords(x, meta=False), **how) as fw:
        for a, b in zip(cuts[:-1], cuts[1:]):
            fw[a:b] = x[a:b]
    items, data, shape, elem, cls = stored(name)
    if 'bps' in how:
        assert shape == (256,)
        codes = np.clip(np.rint(x * 2.95 + 8.), 0, 15).astype(np.uint32)
        assert np.array_equal(decode_words(data, 4, 2045), levels(codes, 4))
        assert int(np.frombuffer(data, '<u4')[-1]) >> 20 == 0          # 5 codes in the last word
    else:
        assert np.array_equal(np.frombuffer(data, '<f2'), x.astype('<f2'))


def test_short_file_keeps_its_promised_size(tmp_path):
    x = noise((1024,), np.float32)
    name = str(tmp_path / 'a.h5')
    with hdf5.open(name, 'w', **keywords(x, meta=False), bps=8) as fw:
        fw.write(x[:512])
    items, data, shape, elem, cls = stored(name)
    assert shape == (256,) and len(data) == 1024 and data[512:] == b'\0' * 512


# --------------------------------------------------------------------------- what the GPU test's ties guard
def fused_codes(x, scale, offset, top):
    """The codes a kernel would make that rounds x * scale + offset ONCE (a fused multiply-add)."""
    exact = np.float64(x) * np.float64(np.float32(scale)) + offset
    return np.clip(np.rint(np.float32(exact)), 0, top)


def test_the_ties_tell_a_fused_multiply_add_from_two_roundings():
    """(NumPy alone.)  Without this the bit-exactness test below would not guard the kernel's
    two separately rounded operations."""
    x4, x8 = ties(2.95, 8., range(15)), ties(35.5, 127.5, TIES_8)
    two4, two8 = np.clip(np.rint(x4 * 2.95 + 8.), 0, 15), np.clip(np.rint(x8 * 35.5 + 127.5), 0, 255)
    assert (x4 * 2.95).dtype == np.float32
    # one rounding of the product with the kernel's float32 constants
    assert np.any(fused_codes(x4, 2.95, 8., 15) != two4) and np.any(fused_codes(x8, 35.5, 127.5, 255) != two8)
    # and in the plainer form, the constants in double precision
    lit4 = np.clip(np.rint(np.float32(np.float64(x4) * 2.95 + 8)), 0, 15)
    lit8 = np.clip(np.rint(np.float32(np.float64(x8) * 35.5 + 127.5)), 0, 255)
    assert np.any(lit4 != two4) or np.any(lit8 != two8)


# --------------------------------------------------------------------------- argument errors
def test_argument_errors(tmp_path):
    z, x = noise((64, 2), np.complex64), noise((64,), np.float32)
    name = str(tmp_path / 'a.h5')
    with pytest.raises(ValueError, match='excludes'):
        hdf5.open(name, 'w', **keywords(z), bps=2, encoded_dtype='c4')
    with pytest.raises(ValueError, match='excludes'):
        hdf5.open(name, 'w', **keywords(z), complex_data=True, encoded_dtype='c4')
    with pytest.raises(ValueError, match="'c4' is for complex"):
        hdf5.open(name, 'w', **keywords(x, meta=False), encoded_dtype='c4')
    with pytest.raises(ValueError, match="'f2' for real"):
        hdf5.open(name, 'w', **keywords(z), encoded_dtype='f2')
    for integer in ('i1', 'i2'):
        with pytest.raises(TypeError, match='out of scope'):
            hdf5.open(name, 'w', **keywords(z), encoded_dtype=integer)
    with pytest.raises(ValueError, match='contradicts'):
        hdf5.open(name, 'w', **keywords(z), bps=2, complex_data=False)
    with pytest.raises(ValueError, match='bps must be'):
        hdf5.open(name, 'w', **keywords(z), bps=3)
    with pytest.raises(TypeError, match='float32 or complex64'):
        hdf5.open(name, 'w', shape=(8,), start_time='2020-01-01T00:00:00', sample_rate=1e6, dtype=np.float64, bps=8)
    with hdf5.open(name, 'w', **keywords(x, meta=False), bps=4) as fw:           # granule 8
        fw.write(x[:16])
        with pytest.raises(ValueError, match='granule, 8 samples'):
            fw.write(x[16:21])
        assert fw.tell() == 16
        fw.write(x[16:])                                                     # the last piece may end anywhere
    with hdf5.open(name, 'w', **keywords(x[:61], meta=False), bps=4) as fw:
        fw.write(x[:56])
        fw.write(x[56:61])


def test_the_writer_takes_the_new_keywords(tmp_path):
    """(Raises TypeError on a writer without compact payloads.)"""
    x = noise((64, 2), np.complex64)
    fw = hdf5.HDF5StreamWriter(str(tmp_path / 'a.h5'), **keywords(x), bps=2)
    assert fw.bps == 2 and fw.granule == 4 and fw.accepts_device is True
    fw.close()


# --------------------------------------------------------------------------- reader errors (no GPU needed)
def _rewrite_header(name, old, new):
    """Patch the header text of a file in place (same length)."""
    assert len(old) == len(new)
    with open(name, 'r+b') as f:
        blob = f.read()
        at = blob.index(old)
        f.seek(at)
        f.write(new)


def test_reader_refuses_what_it_cannot_decode(tmp_path):
    x = noise((1024,), np.float32)
    name = str(tmp_path / 'a.h5')
    with hdf5.open(name, 'w', **keywords(x, meta=False), bps=8) as fw:
        fw.write(x)
    with open(name, 'r+b') as f:                         # truncated
        f.truncate(os.path.getsize(name) - 4)
    with pytest.raises(OSError, match='not an HDF5 stream file this reader understands'):
        hdf5.open(name)
    with hdf5.open(name, 'w', **keywords(x, meta=False), bps=8) as fw:
        fw.write(x)
    _rewrite_header(name, b'bps: 8\n', b'bps: 3\n')
    with pytest.raises(OSError, match='bps = 3'):
        hdf5.open(name)
    _rewrite_header(name, b'bps: 3\n', b'bps: 4\n')        # the word count no longer matches
    with pytest.raises(OSError, match='128 32-bit words'):
        hdf5.open(name)
    with pytest.raises(TypeError):
        hdf5.open(name, frames=3)


# --------------------------------------------------------------------------- the real h5py
GOLDEN = os.path.join(HERE, 'golden')
H5PY_CASES = {'c4': dict(encoded_dtype='c4'), 'f2': dict(encoded_dtype='f2'), 'bps8': dict(bps=8)}


def golden_samples(how):
    """The stream of tests/golden/check_hdf5_compact.py."""
    x = (((np.arange(400) * 37) % 101 - 50) / 7).astype(np.float32)
    return x[:200].reshape(100, 2) if how == 'f2' else x.view(np.complex64).reshape(100, 2)


@pytest.mark.parametrize('how', sorted(H5PY_CASES))
def test_h5py_read_the_compact_datatypes(tmp_path, how):
    """The 2-byte float, the {'real', 'imag'} compound of two of them (the reference's DTYPE_C4:
    io/hdf5/payload.py:18-20) and the '<u4' words as the real h5py saw them: tests/golden/
    compact_<how>.h5 is a file of this writer, compact_h5py.json what h5py 3.3.0 read in it
    (tests/golden/check_hdf5_compact.py).  The writer still makes that file byte for byte, and what
    h5py read are the values that went in."""
    x = golden_samples(how)
    name = str(tmp_path / 'a.h5')
    with hdf5.open(name, 'w', **keywords(x), **H5PY_CASES[how]) as fw:
        fw.write(x)
    with open(name, 'rb') as f, open(os.path.join(GOLDEN, f'compact_{how}.h5'), 'rb') as g:
        assert f.read() == g.read()
    with open(os.path.join(GOLDEN, 'compact_h5py.json')) as f:
        record = json.load(f)
    assert record['h5py'] == '3.3.0'
    seen = record[how]
    if how == 'c4':
        assert seen['names'] == ['real', 'imag'] and seen['offsets'] == [0, 2] and seen['shape'] == [100, 2]
        assert seen['dtype'] == str(np.dtype([('real', '<f2'), ('imag', '<f2')]))
        want = x.view(np.float32).astype('<f2').tobytes()
    elif how == 'f2':
        assert seen['dtype'] == 'float16' and seen['names'] == [] and seen['shape'] == [100, 2]
        want = x.astype('<f2').tobytes()
    else:
        assert seen['dtype'] == 'uint32' and seen['names'] == [] and seen['shape'] == [100]
        want = hdf5.encode_words(x, 8).tobytes()
    assert seen['sha256'] == hashlib.sha256(want).hexdigest()


# --------------------------------------------------------------------------- which reader opens what
def test_open_picks_the_reader_and_the_classes_refuse_the_other_kind(tmp_path):
    x = noise((64, 2), np.complex64)
    raw, coded = str(tmp_path / 'raw.h5'), str(tmp_path / 'coded.h5')
    for name, extra in ((raw, {}), (coded, dict(bps=8))):
        with hdf5.open(name, 'w', **keywords(x), **extra) as fw:
            fw.write(x)
    fr = hdf5.open(raw, samples_per_frame=16)
    assert type(fr) is hdf5.HDF5StreamReader and fr.samples_per_frame == 16
    assert np.array_equal(fr.read(), x)
    with pytest.raises(OSError, match='coded or half-precision payload'):
        hdf5.HDF5StreamReader(coded)
    with pytest.raises(OSError, match='raw payload'):
        hdf5.HDF5EncodedStreamReader(raw)


def test_a_frame_is_bounded_in_components_too(tmp_path):
    """An explicit frame length is held to what one frame of bbt_unpack takes (2^24 components),
    like the default: refused when the file is opened, not by the library at the first read."""
    x = np.zeros((8, 1 << 14), np.float32)                  # 2^14 components a sample: 1024 samples a frame
    name = str(tmp_path / 'wide.h5')
    with hdf5.open(name, 'w', **keywords(x, meta=False), bps=1) as fw:
        fw.write(x)
    assert hdf5.open(name).samples_per_frame == 8
    with pytest.raises(ValueError, match='up to 1024'):
        hdf5.open(name, samples_per_frame=2048)


def test_compact_pieces_may_be_lists(tmp_path):
    """What the raw path takes through np.ascontiguousarray the compact paths take too."""
    x = noise((32,), np.float32)
    for extra in (dict(bps=8), dict(encoded_dtype='f2')):
        a, b = str(tmp_path / 'a.h5'), str(tmp_path / 'b.h5')
        with hdf5.open(a, 'w', **keywords(x, meta=False), **extra) as fw:
            fw.write(x)
        with hdf5.open(b, 'w', **keywords(x, meta=False), **extra) as fw:
            fw.write(x.tolist())
        with open(a, 'rb') as f, open(b, 'rb') as g:
            assert f.read() == g.read()
