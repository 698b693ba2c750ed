"""Sink (and matching source) for the reference's intermediate HDF5 format.

SURVEY 8(f) rank 3, the downstream side: `baseband_tasks.io.hdf5` stores a
stream as one HDF5 file with two datasets -- ``header``, a YAML text holding
``sample_shape, samples_per_frame, sample_rate, time, dtype`` and the optional
``frequency, sideband, polarization`` (io/hdf5/header.py:23-130, written with
astropy's YAML dumper), and ``payload``, the samples as a plain array
(io/hdf5/payload.py:121-178; complex numbers as h5py stores them, a compound
of two floats ``r`` and ``i``) -- and copies a stream into it through
``fw.write(data)`` / ``fw[a:b] = data`` (io/hdf5/base.py:102-126, which is
what `integration.Integrate` and friends write through).

Neither h5py nor astropy is available where this package runs, so the file is
written directly: the subset of the HDF5 file format needed for those two
datasets (version-2 superblock, version-2 object headers with compact links,
contiguous layouts, Jenkins lookup3 checksums), the YAML text in the tags
astropy's loader resolves (``!astropy.units.Quantity``, ``!astropy.time.Time``,
``!numpy.ndarray``).  tests/test_hdf5.py reads such files back with the real
h5py + astropy YAML loader (in the build container's second interpreter, the
way the reference's ``HDF5Header.fromfile`` does); the reference's own reader
class cannot be run here (it imports `baseband`).  `open(name, 'r')` reads the
files this module writes AND the files the reference's own writer produces
(h5py with default settings: superblock 0, symbol-table groups, version-1
object headers, the header as a variable-length string; tests/golden/
reference_style.h5 is such a file, made by the real h5py + astropy) -- raw,
contiguous payloads; not HDF5 files in general (no chunking, no filters).

Compact payloads (io/hdf5/header.py:227-307, payload.py:121-178): a stream may be stored raw in a
narrower ``encoded_dtype`` -- '<f2', or the reference's '<c4', a compound of two '<f2' members
``real`` and ``imag`` -- or coded, when the header has ``bps`` and ``complex_data``: a 1-d '<u4'
array of ``ceil(bps * components / 32)`` words in VDIF coding.  The writer encodes
`hip.DeviceArray` pieces in HBM (`hip.pack`, `hip.to_half`) and copies down the encoded bytes only;
the reader uploads the stored bytes and decodes them in HBM (`HDF5EncodedStreamReader`).  The 2-byte
float datatype, the ``real`` / ``imag`` compound and the '<u4' words were read once with h5py 3.3.0
(libhdf5 1.10.6): tests/golden/compact_*.h5 are files of this writer, compact_h5py.json is what
h5py saw in them (tests/golden/check_hdf5_compact.py), and tests/test_hdf5_coded_host.py holds the
writer to those bytes.  The reference's own `HDF5Payload` classes have not been run on these files
(they import `baseband`).
"""
import base64
import math
import os
import struct

import numpy as np

from . import hip
from . import units as u
from .base import Base
from .device_task import DeviceTaskMixin
from .units import Time

__all__ = ['open', 'HDF5StreamWriter', 'HDF5StreamReader', 'HDF5EncodedStreamReader', 'header_yaml', 'lookup3',
           'DTYPE_C4', 'encode_words', 'encode_half']

_UNDEF = 0xFFFFFFFFFFFFFFFF
_SIGNATURE = b'\x89HDF\r\n\x1a\n'
_M = 0xFFFFFFFF


# --------------------------------------------------------------------------- checksums
def _rot(x, k):
    return ((x << k) | (x >> (32 - k))) & _M


def lookup3(data, initval=0):
    """Bob Jenkins' lookup3 `hashlittle`, the metadata checksum of the HDF5 format."""
    data = bytes(data)
    length = len(data)
    a = b = c = (0xdeadbeef + length + initval) & _M
    i = 0
    while length > 12:
        a = (a + int.from_bytes(data[i:i + 4], 'little')) & _M
        b = (b + int.from_bytes(data[i + 4:i + 8], 'little')) & _M
        c = (c + int.from_bytes(data[i + 8:i + 12], 'little')) & _M
        a = (a - c) & _M; a ^= _rot(c, 4); c = (c + b) & _M
        b = (b - a) & _M; b ^= _rot(a, 6); a = (a + c) & _M
        c = (c - b) & _M; c ^= _rot(b, 8); b = (b + a) & _M
        a = (a - c) & _M; a ^= _rot(c, 16); c = (c + b) & _M
        b = (b - a) & _M; b ^= _rot(a, 19); a = (a + c) & _M
        c = (c - b) & _M; c ^= _rot(b, 4); b = (b + a) & _M
        i += 12
        length -= 12
    if length == 0:
        return c
    tail = data[i:] + b'\0' * (12 - length)
    a = (a + int.from_bytes(tail[0:4], 'little')) & _M
    b = (b + int.from_bytes(tail[4:8], 'little')) & _M
    c = (c + int.from_bytes(tail[8:12], 'little')) & _M
    c ^= b; c = (c - _rot(b, 14)) & _M
    a ^= c; a = (a - _rot(c, 11)) & _M
    b ^= a; b = (b - _rot(a, 25)) & _M
    c ^= b; c = (c - _rot(b, 16)) & _M
    a ^= c; a = (a - _rot(c, 4)) & _M
    b ^= a; b = (b - _rot(a, 14)) & _M
    c ^= b; c = (c - _rot(b, 24)) & _M
    return c


# --------------------------------------------------------------------------- HDF5 structures
def _message(kind, data, flags=0):
    return struct.pack('<BHB', kind, len(data), flags) + data


def _object_header(messages, room=0):
    body = b''.join(messages)
    if room:
        body += _message(0, b'\0' * room)                   # NIL message: space for later growth
    head = b'OHDR' + struct.pack('<BBI', 2, 0x02, len(body))   # version 2, 4-byte chunk size, no times
    blob = head + body
    return blob + struct.pack('<I', lookup3(blob))


_FLOAT_TYPES = {2: (bytes([0x11, 0x20, 15, 0]), struct.pack('<HHBBBBI', 0, 16, 10, 5, 0, 10, 15)),
                4: (bytes([0x11, 0x20, 31, 0]), struct.pack('<HHBBBBI', 0, 32, 23, 8, 0, 23, 127)),
                8: (bytes([0x11, 0x20, 63, 0]), struct.pack('<HHBBBBI', 0, 64, 52, 11, 0, 52, 1023))}

#: The reference's half-precision complex element (io/hdf5/payload.py:18-20): not a NumPy number.
DTYPE_C4 = np.dtype([('real', '<f2'), ('imag', '<f2')])


def _datatype(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == 'f' and dtype.itemsize in _FLOAT_TYPES:
        head, props = _FLOAT_TYPES[dtype.itemsize]
        return head + struct.pack('<I', dtype.itemsize) + props
    if dtype.kind == 'c' and dtype.itemsize in (8, 16):
        part = _datatype(np.dtype('<f%d' % (dtype.itemsize // 2)))
        members = b'r\0' + bytes([0]) + part + b'i\0' + bytes([dtype.itemsize // 2]) + part
        return bytes([0x36, 2, 0, 0]) + struct.pack('<I', dtype.itemsize) + members
    if dtype == DTYPE_C4:
        part = _datatype(np.dtype('<f2'))
        members = b'real\0' + bytes([0]) + part + b'imag\0' + bytes([2]) + part
        return bytes([0x36, 2, 0, 0]) + struct.pack('<I', 4) + members
    if dtype.kind == 'i' or dtype.kind == 'u':
        signed = 0x08 if dtype.kind == 'i' else 0
        return (bytes([0x10, signed, 0, 0]) + struct.pack('<I', dtype.itemsize)
                + struct.pack('<HH', 0, 8 * dtype.itemsize))
    if dtype.kind == 'S':
        return bytes([0x13, 0x01, 0, 0]) + struct.pack('<I', dtype.itemsize)       # null-padded ASCII
    raise TypeError(f"no HDF5 datatype for {dtype}")


def _dataset_header(shape, dtype, address, nbytes):
    rank = len(shape)
    space = struct.pack('<BBBB', 2, rank, 0, 1 if rank else 0) + b''.join(struct.pack('<Q', d) for d in shape)
    layout = struct.pack('<BBQQ', 3, 1, address, nbytes)
    return _object_header([_message(0x01, space), _message(0x03, _datatype(dtype), 1),
                           _message(0x05, bytes([3, 0x0a]), 1), _message(0x08, layout)])


def _link(name, address):
    name = name.encode()
    return _message(0x06, struct.pack('<BBB', 1, 0, len(name)) + name + struct.pack('<Q', address))


def _layout(header_text, shape, dtype):
    """The file's metadata for the two datasets: (bytes, payload address, end of file)."""
    text = header_text.encode()
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    pos_root = 48
    root_size = len(_object_header([_message(0x02, b''), _message(0x0A, b''), _link('header', 0),
                                    _link('payload', 0)])) + 18 + 2        # (message bodies added below)
    pos_h = pos_root + root_size
    oh_h = _dataset_header((), np.dtype('S%d' % len(text)), 0, len(text))
    pos_p = pos_h + len(oh_h)
    oh_p = _dataset_header(shape, dtype, 0, nbytes)
    data_h = pos_p + len(oh_p)
    data_p = -(-(data_h + len(text)) // 4096) * 4096                       # payload on a page boundary
    eof = data_p + nbytes
    root = _object_header([_message(0x02, struct.pack('<BBQQ', 0, 0, _UNDEF, _UNDEF)),
                           _message(0x0A, bytes([0, 0]), 1), _link('header', pos_h), _link('payload', pos_p)])
    assert len(root) == root_size
    oh_h = _dataset_header((), np.dtype('S%d' % len(text)), data_h, len(text))
    oh_p = _dataset_header(shape, dtype, data_p, nbytes)
    sb = _SIGNATURE + struct.pack('<BBBBQQQQ', 2, 8, 8, 0, 0, _UNDEF, eof, pos_root)
    sb += struct.pack('<I', lookup3(sb))
    meta = sb + root + oh_h + oh_p + text
    return meta + b'\0' * (data_p - len(meta)), data_p, eof


# --------------------------------------------------------------------------- YAML header
def _yaml_array(a, indent):
    a = np.ascontiguousarray(a)
    pad = ' ' * indent
    inner = base64.b64encode(a.tobytes())
    text = base64.b64encode(inner).decode()
    lines = [text[i:i + 76] for i in range(0, len(text), 76)] or ['']
    out = '!numpy.ndarray\n' + pad + 'buffer: !!binary |\n'
    out += ''.join(pad + '  ' + ln + '\n' for ln in lines)
    out += pad + f'dtype: {a.dtype.name if a.dtype.kind in "fiub" else a.dtype.str}\n'
    out += pad + 'order: C\n'
    out += pad + 'shape: !!python/tuple [' + ', '.join(str(d) for d in a.shape) + ']\n'
    return out


def _yaml_quantity(value, unit, indent):
    pad = ' ' * indent
    out = '!astropy.units.Quantity\n' + pad + 'unit: !astropy.units.Unit {unit: ' + unit + '}\n'
    if np.ndim(value) == 0:
        return out + pad + f'value: {float(value)!r}\n'
    return out + pad + 'value: ' + _yaml_array(np.asarray(value, dtype=np.float64), indent + 2)


def header_yaml(sample_shape, samples_per_frame, sample_rate_hz, start_time, dtype, frequency_hz=None,
                sideband=None, polarization=None, bps=None, complex_data=None, encoded_dtype=None):
    """The ``header`` dataset: the reference's header keywords (io/hdf5/header.py:44-45, 215-216)
    as YAML in the tags of astropy's dumper; rates and frequencies in Hz.  With ``bps`` the header
    of a coded payload (``bps`` and ``complex_data`` in place of ``dtype``: header.py:290-307), with
    ``encoded_dtype`` ('<f2' / '<c4') that of a half-precision one (header.py:227-287)."""
    t = Time(start_time)
    jd1, jd2 = t.jd1_jd2()
    if bps is not None:
        items = {'bps': f'{int(bps)}', 'complex_data': 'true' if complex_data else 'false'}
    elif encoded_dtype is not None:
        items = {'dtype': np.dtype(dtype).name, 'encoded_dtype': str(encoded_dtype)}
    else:
        items = {'dtype': np.dtype(dtype).str}
    if frequency_hz is not None:
        items['frequency'] = _yaml_quantity(frequency_hz, 'Hz', 2)
    if polarization is not None:
        pol = np.asarray(polarization)
        items['polarization'] = _yaml_array(pol.astype('<U%d' % max(1, pol.dtype.itemsize // (4 if pol.dtype.kind == 'U' else 1))), 2)
    items['sample_rate'] = _yaml_quantity(sample_rate_hz, 'Hz', 2)
    items['sample_shape'] = '!!python/tuple [' + ', '.join(str(d) for d in sample_shape) + ']\n'
    items['samples_per_frame'] = f'{int(samples_per_frame)}\n'
    if sideband is not None:
        items['sideband'] = _yaml_array(np.asarray(sideband, dtype=np.int8), 2)
    items['time'] = ("!astropy.time.Time {format: isot, in_subfmt: '*', jd1: %r, jd2: %r,\n"
                     "  out_subfmt: '*', precision: 9, scale: utc}\n" % (jd1, jd2))
    out = ''
    for key in sorted(items):
        value = items[key]
        out += f'{key}: {value}' if value.endswith('\n') else f'{key}: {value}\n'
    return out


# --------------------------------------------------------------------------- compact payloads
#: bits per component of a coded payload (the widths of `hip.pack` / bbt_unpack code 0)
CODED_BITS = (1, 2, 4, 8, 16)
_HALF_NAMES = {'f2': '<f2', '<f2': '<f2', 'float16': '<f2', 'c4': '<c4', '<c4': '<c4', 'complex32': '<c4'}


def _granule(bps, components):
    """Fewest samples of ``components`` components at ``bps`` bits that fill whole 32-bit words."""
    return 32 // math.gcd(32, bps * components)


def _components_of(data):
    """float32 / complex64 array -> its float32 components, flat (complex: re, im adjacent)."""
    data = np.ascontiguousarray(data)
    if data.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
        raise TypeError(f"compact payloads hold float32 or complex64 samples, not {data.dtype}")
    return data.view(np.float32).ravel()


def encode_words(data, bps):
    """NumPy restatement of `hip.pack`: float32 / complex64 samples -> '<u4' words in VDIF coding
    (the codes of `ingest.encode_vdif_frames`; first component in the least significant bits, a
    last partial word zero in its unused bits)."""
    if bps not in CODED_BITS:
        raise ValueError(f"bps must be one of {CODED_BITS}, not {bps!r}")
    comp = _components_of(data)
    if bps == 1:
        codes = (comp > 0).astype(np.uint32)
    elif bps == 2:
        # (the thresholds strictly below x, as np.searchsorted counts them; a NaN is above none)
        codes = (comp > -2).astype(np.uint32) + (comp > 0) + (comp > 2)
    else:
        with np.errstate(invalid='ignore'):
            if bps == 4:
                level = comp * 2.95 + 8.
            elif bps == 8:
                level = comp * 35.5 + 127.5
            else:
                level = comp + 32768.
            level = np.clip(np.rint(level), 0, (1 << bps) - 1)
            codes = np.where(np.isnan(level), 0, level).astype(np.uint32)
    per_word = 32 // bps
    n_words = -(-codes.shape[0] // per_word)
    full = np.zeros(n_words * per_word, np.uint32)
    full[:codes.shape[0]] = codes
    full = full.reshape(n_words, per_word)
    words = np.zeros(n_words, np.uint32)
    for k in range(per_word):
        words |= full[:, k] << np.uint32(k * bps)
    return words.astype('<u4')


def encode_half(data):
    """NumPy restatement of `hip.to_half`: float32 / complex64 samples -> '<f2' components (the
    bytes of a '<f2' / '<c4' payload)."""
    with np.errstate(over='ignore'):
        return _components_of(data).astype('<f2')


# --------------------------------------------------------------------------- stream writer / reader
class HDF5StreamWriter:
    """Write a stream of known length into an HDF5 file of the reference's layout.

    ``template`` supplies shape, start time, sample rate, dtype and the optional
    frequency / sideband / polarization (any stream of this package or one
    with the same attributes); keywords override it.  Like the reference's
    writer (io/hdf5/base.py:102-126) it takes samples in order, through
    ``write(data)`` or ``fw[a:b] = data``.

    Compact payloads (reference io/hdf5/header.py:227-307, payload.py:121-178; float32 /
    complex64 streams), one of:

    ``bps`` (1, 2, 4, 8 or 16), with ``complex_data`` defaulting from the stream's dtype: a
    coded payload, ``ceil(bps * components / 32)`` '<u4' words in VDIF coding.

    ``encoded_dtype``: 'f2' / '<f2' for real, 'c4' / '<c4' / 'complex32' for complex streams:
    the samples as IEEE half precision (complex: a compound of 'real' and 'imag').

    A `hip.DeviceArray` piece of such a file is encoded in HBM and only the encoded bytes come
    down (`accepts_device`: a task's ``read(out=writer)`` hands over its device pieces); an
    ndarray piece is encoded with NumPy, to the same bytes.  Pieces of a half-precision file
    may end anywhere.  Every piece of a coded file but the last must end on a 32-bit word, i.e.
    hold a multiple of `granule` samples: the writer raises ValueError otherwise, it does not
    buffer.  ``read(out=writer)`` hands over whole frames (runs of frames, and what is left of the
    frame the pointer is in), so reading a stream from its start meets this whenever the
    task's ``samples_per_frame`` is a multiple of the granule -- any power of two from 32 on.
    Raw files take device pieces too; those are copied down first.
    """
    #: ``read(out=writer)`` of a device task may assign `hip.DeviceArray` pieces
    accepts_device = True

    def __init__(self, name, template=None, *, shape=None, start_time=None, sample_rate=None, dtype=None,
                 frequency=None, sideband=None, polarization=None, bps=None, complex_data=None,
                 encoded_dtype=None):
        get = lambda key, given: given if given is not None else getattr(template, key, None)
        shape = tuple(get('shape', shape))
        self.shape = shape
        self.sample_shape = shape[1:]
        self.dtype = np.dtype(get('dtype', dtype))
        self.bps, self.encoded_dtype, self.granule = None, None, 1
        if encoded_dtype is not None and (bps is not None or complex_data is not None):
            raise ValueError("encoded_dtype excludes bps and complex_data: a payload is coded or raw.")
        if complex_data is not None and bool(complex_data) != (self.dtype.kind == 'c'):
            raise ValueError(f"complex_data={bool(complex_data)} contradicts the stream's dtype {self.dtype}.")
        if bps is not None or encoded_dtype is not None:
            if encoded_dtype is not None and str(encoded_dtype) not in _HALF_NAMES:
                try:
                    other = np.dtype(encoded_dtype)
                except TypeError:
                    raise TypeError(f"encoded_dtype {encoded_dtype!r} is not understood.") from None
                if other == self.dtype:
                    encoded_dtype = None                   # (stored as it is: a plain raw file)
                else:
                    raise TypeError(f"encoded_dtype {other.str!r} is out of scope: only half precision "
                                    "('f2', 'c4') is written; integer payloads are not.")
        if bps is not None or encoded_dtype is not None:
            if self.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
                raise TypeError(f"compact payloads are written from float32 or complex64 streams, not {self.dtype}.")
        self._components = int(np.prod(self.sample_shape, dtype=np.int64)) * (2 if self.dtype.kind == 'c' else 1)
        if bps is not None:
            if isinstance(bps, bool) or int(bps) != bps or int(bps) not in CODED_BITS:
                raise ValueError(f"bps must be one of {CODED_BITS}, not {bps!r}.")
            self.bps = int(bps)
            self.granule = _granule(self.bps, self._components)
        elif encoded_dtype is not None:
            self.encoded_dtype = _HALF_NAMES[str(encoded_dtype)]
            if (self.encoded_dtype == '<c4') != (self.dtype.kind == 'c'):
                raise ValueError(f"encoded_dtype {self.encoded_dtype!r} does not fit a stream of {self.dtype}: "
                                 "'c4' is for complex, 'f2' for real streams.")
        self.sample_rate = u.to_hz(get('sample_rate', sample_rate))
        self.start_time = Time(get('start_time', start_time))
        self.frequency = get('frequency', frequency)
        self.sideband = get('sideband', sideband)
        self.polarization = get('polarization', polarization)
        freq = None if self.frequency is None else np.asarray(u.to_hz(self.frequency), dtype=np.float64)
        text = header_yaml(self.sample_shape, shape[0], self.sample_rate, self.start_time, self.dtype,
                           frequency_hz=freq, sideband=self.sideband, polarization=self.polarization,
                           bps=self.bps, complex_data=self.dtype.kind == 'c', encoded_dtype=self.encoded_dtype)
        self.header_text = text
        if self.bps is not None:
            stored_shape, stored = (-(-self.bps * self._components * shape[0] // 32),), np.dtype('<u4')
        elif self.encoded_dtype is not None:
            stored_shape, stored = shape, (DTYPE_C4 if self.encoded_dtype == '<c4' else np.dtype('<f2'))
        else:
            stored_shape, stored = shape, self.dtype
        meta, self._data_at, self._eof = _layout(text, stored_shape, stored)
        self._fh = builtins_open(name, 'wb')
        self._fh.write(meta)
        self.offset = 0
        self.closed = False

    def tell(self):
        return self.offset

    def _encode(self, data):
        """The bytes of a piece of a compact payload: a device piece is encoded in HBM and the
        encoded bytes are copied down, a host piece is encoded with NumPy."""
        if isinstance(data, hip.DeviceArray) and data.dtype == self.dtype:
            coded = hip.pack(data, self.bps) if self.bps is not None else hip.to_half(data)
            return coded.to_host()
        if hasattr(data, 'to_host'):
            data = data.to_host()
        data = np.ascontiguousarray(data, dtype=self.dtype)
        return encode_words(data, self.bps) if self.bps is not None else encode_half(data)

    def write(self, data):
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        compact = self.bps is not None or self.encoded_dtype is not None
        if not compact and hasattr(data, 'to_host'):
            data = data.to_host()
        if not hasattr(data, 'to_host'):                   # (a device piece of a compact file stays where it is)
            data = np.ascontiguousarray(data, dtype=self.dtype)
        assert tuple(data.shape[1:]) == self.sample_shape, f"'data' must have trailing shape {self.sample_shape}"
        n = data.shape[0]
        if self.offset + n > self.shape[0]:
            raise EOFError("cannot write beyond the length given in the header.")
        if self.bps is not None and n % self.granule and self.offset + n != self.shape[0]:
            raise ValueError(f"a piece of {n} samples does not end on a 32-bit word: every piece of a coded "
                             f"payload but the last must hold a multiple of the granule, {self.granule} samples.")
        if compact:
            data = self._encode(data)
        self._fh.write(data.tobytes())
        self.offset += n

    def __setitem__(self, item, value):
        start, stop, step = item.indices(self.shape[0])
        assert start == self.offset, 'Can only assign right following pointer.'
        assert step == 1, 'unity step size only is supported'
        assert len(value) == stop - start, 'number of samples should match.'
        self.write(value)

    def close(self):
        if not self.closed:
            self.closed = True
            if self.offset < self.shape[0]:            # (a short file still has the promised size)
                self._fh.truncate(self._eof)
            self._fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# --------------------------------------------------------------------------- the YAML header
_SI = {'': 1., 'k': 1e3, 'M': 1e6, 'G': 1e9, 'T': 1e12, 'm': 1e-3, 'u': 1e-6, 'n': 1e-9}


def _unit_in_hz(unit):
    """Factor that turns a value in ``unit`` (astropy's string for a frequency unit: Hz with an SI
    prefix, or one over a time unit) into Hz."""
    unit = unit.strip()
    if unit.endswith('Hz') and unit[:-2] in _SI:
        return _SI[unit[:-2]]
    if unit.startswith('1 / ') and unit.endswith('s') and unit[4:-1] in _SI:
        return 1. / _SI[unit[4:-1]]
    raise OSError(f"header: cannot interpret the unit {unit!r} as a frequency.")


class _Quantity:
    def __init__(self, value, unit):
        self.value, self.unit = value, unit

    def hz(self):
        return np.asarray(self.value, dtype=np.float64) * _unit_in_hz(self.unit)


def parse_header(text):
    """The header dict of a 'header' dataset: astropy's YAML (io/hdf5/header.py:66-81: dumped and
    loaded with astropy.io.misc.yaml) read with PyYAML and constructors for the four tags that
    occur -- units, quantities, times, arrays -- astropy itself being absent where this runs.
    Quantities come back in Hz (float or array), the time as `units.Time`."""
    import yaml

    class Loader(yaml.SafeLoader):
        pass

    def unit(loader, node):
        m = loader.construct_mapping(node, deep=True)
        return str(m.get('unit', ''))

    def quantity(loader, node):
        m = loader.construct_mapping(node, deep=True)
        return _Quantity(m['value'], m['unit'])

    def time(loader, node):
        m = loader.construct_mapping(node, deep=True)
        if str(m.get('scale', 'utc')).lower() != 'utc':
            raise OSError(f"header: time scale {m.get('scale')!r} is not supported (utc only).")
        return Time.from_jd(float(m['jd1']), float(m['jd2']))

    def ndarray(loader, node):
        m = loader.construct_mapping(node, deep=True)
        raw = m['buffer']
        raw = base64.b64decode(raw if isinstance(raw, bytes) else raw.encode())   # (astropy encodes, then YAML does)
        order = 'F' if str(m.get('order', 'C')).upper().startswith('F') else 'C'
        return np.frombuffer(raw, dtype=np.dtype(str(m['dtype']))).reshape(tuple(m['shape']), order=order).copy()

    Loader.add_constructor('!astropy.units.Unit', unit)
    Loader.add_constructor('!astropy.units.Quantity', quantity)
    Loader.add_constructor('!astropy.time.Time', time)
    Loader.add_constructor('!numpy.ndarray', ndarray)
    Loader.add_constructor('tag:yaml.org,2002:python/tuple', lambda loader, node: tuple(loader.construct_sequence(node)))
    items = yaml.load(text, Loader=Loader)
    if not isinstance(items, dict) or not {'sample_shape', 'samples_per_frame', 'sample_rate', 'time'} <= set(items):
        raise OSError("header: sample_shape, samples_per_frame, sample_rate and time are required "
                      "(io/hdf5/header.py:58-60).")
    for key in ('sample_rate', 'frequency'):
        if isinstance(items.get(key), _Quantity):
            items[key] = items[key].hz()
    return items


# --------------------------------------------------------------------------- the file structure
class _File:
    """The little of the HDF5 format needed to find two datasets in the root group, in both
    generations of the on-disk structures: what this module writes (superblock 2, version-2 object
    headers, compact links) and what h5py / libhdf5 write by default, i.e. what the reference's
    own writer produces (superblock 0, symbol-table group: B-tree + local heap, version-1 object
    headers with continuation blocks, variable-length strings in the global heap)."""

    def __init__(self, raw):
        self.raw = raw
        head = bytes(raw[:96])
        if head[:8] != _SIGNATURE:
            raise OSError("not an HDF5 file (signature).")
        version = head[8]
        if version in (2, 3):
            if lookup3(head[:44]) != struct.unpack('<I', head[44:48])[0]:
                raise OSError("superblock checksum.")
            if head[9] != 8 or head[10] != 8:
                raise OSError("only 8-byte offsets and lengths are supported.")
            self.root = struct.unpack('<Q', head[36:44])[0]
        elif version in (0, 1):
            if head[13] != 8 or head[14] != 8:
                raise OSError("only 8-byte offsets and lengths are supported.")
            base = 24 + (4 if version == 1 else 0)
            if struct.unpack('<Q', head[base:base + 8])[0] != 0:
                raise OSError("a non-zero base address is not supported.")
            # root group symbol table entry: link name offset, object header address, ...
            self.root = struct.unpack('<Q', head[base + 40:base + 48])[0]
        else:
            raise OSError(f"superblock version {version} is not supported.")

    def bytes(self, addr, n):
        return bytes(self.raw[addr:addr + n])

    # -- object headers
    def messages(self, addr):
        """(type, data) of every message of the object header at ``addr``."""
        if self.bytes(addr, 4) == b'OHDR':
            yield from self._messages_v2(addr)
        elif self.raw[addr] == 1:
            yield from self._messages_v1(addr)
        else:
            raise OSError("object header version not supported by this reader.")

    def _messages_v2(self, addr):
        head = self.bytes(addr, 16)
        if head[4] != 2:
            raise OSError("object header version not supported by this reader.")
        flags = head[5]
        pos = addr + 6 + (16 if flags & 0x20 else 0) + (4 if flags & 0x10 else 0)
        width = 1 << (flags & 3)
        size = int.from_bytes(self.bytes(pos, width), 'little')
        pos += width
        blocks = [(pos, pos + size)]
        while blocks:
            pos, end = blocks.pop(0)
            while pos + 4 <= end:
                kind, n, _ = struct.unpack('<BHB', self.bytes(pos, 4))
                pos += 4 + (2 if flags & 0x04 else 0)
                data = self.bytes(pos, n)
                pos += n
                if kind == 0x10:                           # continuation: 'OCHK' block
                    off, length = struct.unpack('<QQ', data[:16])
                    blocks.append((off + 4, off + length - 4))
                else:
                    yield kind, data

    def _messages_v1(self, addr):
        _, _, count, _, size = struct.unpack('<BBHII', self.bytes(addr, 12))
        blocks = [(addr + 16, addr + 16 + size)]           # (the prefix is padded to 8 bytes)
        while blocks and count > 0:
            pos, end = blocks.pop(0)
            while pos + 8 <= end and count > 0:
                kind, n, _ = struct.unpack('<HHB', self.bytes(pos, 5))
                data = self.bytes(pos + 8, n)
                pos += 8 + n
                count -= 1
                if kind == 0x10:
                    off, length = struct.unpack('<QQ', data[:16])
                    blocks.append((off, off + length))
                else:
                    yield kind, data

    # -- groups
    def links(self, addr):
        """name -> object header address of the group whose object header is at ``addr``."""
        out = {}
        for kind, data in self.messages(addr):
            if kind == 0x06 and data[0] == 1:              # link message (new-style groups)
                flags = data[1]
                pos = 2 + (1 if flags & 0x08 else 0) + (8 if flags & 0x04 else 0) + (1 if flags & 0x10 else 0)
                width = 1 << (flags & 3)
                n = int.from_bytes(data[pos:pos + width], 'little')
                pos += width
                name = data[pos:pos + n].decode()
                if not flags & 0x08 or data[2] == 0:       # hard link
                    out[name] = struct.unpack('<Q', data[pos + n:pos + n + 8])[0]
            elif kind == 0x11:                             # symbol table message (old-style groups)
                btree, heap = struct.unpack('<QQ', data[:16])
                out.update(self._symbol_table(btree, heap))
        return out

    def _symbol_table(self, btree, heap):
        h = self.bytes(heap, 32)
        if h[:4] != b'HEAP':
            raise OSError("local heap signature.")
        segment = struct.unpack('<Q', h[24:32])[0]

        def name(offset):
            end = offset
            while self.raw[segment + end] != 0:
                end += 1
            return self.bytes(segment + offset, end - offset).decode()

        out = {}
        nodes = [btree]
        while nodes:
            node = nodes.pop()
            head = self.bytes(node, 24)
            if head[:4] == b'TREE':
                if head[4] != 0:
                    raise OSError("group B-tree node type.")
                used = struct.unpack('<H', head[6:8])[0]
                for i in range(used):                      # key 0, child 0, key 1, child 1, ...
                    nodes.append(struct.unpack('<Q', self.bytes(node + 24 + 8 + 16 * i, 8))[0])
            elif head[:4] == b'SNOD':
                count = struct.unpack('<H', head[6:8])[0]
                for i in range(count):
                    off, obj = struct.unpack('<QQ', self.bytes(node + 8 + 40 * i, 16))
                    out[name(off)] = obj
            else:
                raise OSError("symbol table node signature.")
        return out

    # -- datasets
    def dataset(self, addr):
        """(data address, bytes, shape, element size, datatype class, inline data) of a dataset."""
        shape, address, size, inline = (), None, None, None
        elem, cls = None, None
        for kind, data in self.messages(addr):
            if kind == 0x01:                               # dataspace
                rank = data[1]
                first = 8 if data[0] == 1 else 4
                shape = tuple(struct.unpack('<Q', data[first + 8 * i:first + 8 + 8 * i])[0] for i in range(rank))
            elif kind == 0x03:                             # datatype
                cls = data[0] & 0x0F
                elem = struct.unpack('<I', data[4:8])[0]
            elif kind == 0x08:                             # layout
                if data[0] not in (3, 4):
                    raise OSError(f"data layout message version {data[0]} is not supported.")
                if data[1] == 1:
                    address, size = struct.unpack('<QQ', data[2:18])
                elif data[1] == 0:
                    n = struct.unpack('<H', data[2:4])[0]
                    inline = data[4:4 + n]
                else:
                    raise OSError("dataset is not stored contiguously (chunked or virtual layouts are not read).")
        if address is None and inline is None:
            raise OSError("dataset has no data layout.")
        if address == _UNDEF:
            raise OSError("dataset has no storage allocated (it was never written).")
        return address, size, shape, elem, cls, inline

    def text(self, addr):
        """The string a scalar string dataset holds: fixed length in place, or variable length in
        the global heap (what ``create_dataset('header', data=str)`` of h5py makes)."""
        address, size, shape, elem, cls, inline = self.dataset(addr)
        body = inline if inline is not None else self.bytes(address, size)
        if cls == 9:                                       # variable length: (length, heap address, index)
            length, heap, index = struct.unpack('<IQI', body[:16])
            head = self.bytes(heap, 16)
            if head[:4] != b'GCOL':
                raise OSError("global heap signature.")
            end = heap + struct.unpack('<Q', head[8:16])[0]
            pos = heap + 16
            while pos + 16 <= end:
                idx, _, _, n = struct.unpack('<HHIQ', self.bytes(pos, 16))
                if idx == index:
                    return self.bytes(pos + 16, min(n, length)).decode()
                if idx == 0:
                    break
                pos += 16 + (n + 7) // 8 * 8
            raise OSError("global heap object not found.")
        return body.split(b'\0', 1)[0].decode()


class _Structure:
    """What the readers need of a file: the header items and where the payload lies.  The checks of
    compact payloads (``bps``, the word count, the half-precision datatypes, a truncated file) are
    made here, for those files only; a raw file is checked by `HDF5StreamReader` as it always was."""

    def __init__(self, name):
        raw = np.memmap(name, mode='r')
        try:
            f = _File(raw)
            links = f.links(f.root)
            if not {'header', 'payload'} <= set(links):
                raise OSError("no 'header' and 'payload' datasets.")
            text = f.text(links['header'])
            items = parse_header(text)
            address, size, shape, elem, cls, inline = f.dataset(links['payload'])
            if inline is not None:
                raise OSError("compact payloads are not supported.")
            sample_shape = tuple(int(d) for d in items['sample_shape'])
            self.items, self.half = items, None
            if 'bps' in items:
                self._coded(items, sample_shape, shape, elem, cls)
            else:
                enc = items.get('encoded_dtype')
                enc = None if enc is None else _HALF_NAMES.get(str(enc), str(enc))
                if enc in ('<f2', '<c4'):
                    self._half(items, enc, elem, cls)
            if self.encoded and address + size > raw.shape[0]:
                raise OSError(f"the payload needs {address + size} bytes, the file has {raw.shape[0]} (truncated).")
        except OSError as exc:
            raise OSError(f"{name}: not an HDF5 stream file this reader understands ({exc})") from None
        self.raw, self.text, self.items = raw, text, items
        self.address, self.size, self.shape, self.elem, self.cls = address, size, tuple(shape), elem, cls
        self.sample_shape = sample_shape

    @property
    def encoded(self):
        return self.half is not None or 'bps' in self.items

    def _coded(self, items, sample_shape, shape, elem, cls):
        bps, complex_data = items['bps'], items.get('complex_data', False)
        if isinstance(bps, bool) or not isinstance(bps, int) or bps not in CODED_BITS:
            raise OSError(f"encoded payloads with bps = {bps!r} are not supported (bps is one of {CODED_BITS}).")
        if not isinstance(complex_data, bool):
            raise OSError(f"header: complex_data must be true or false, not {complex_data!r}.")
        n = int(items['samples_per_frame'])
        self.components = int(np.prod(sample_shape, dtype=np.int64)) * (2 if complex_data else 1)
        n_words = -(-bps * self.components * n // 32)
        if cls != 0 or elem != 4 or tuple(shape) != (n_words,):
            raise OSError(f"a coded payload of {n} samples of {self.components} components at {bps} bits is "
                          f"{n_words} 32-bit words; the payload has shape {tuple(shape)} of {elem}-byte elements.")
        self.dtype = np.dtype(np.complex64 if complex_data else np.float32)
        self.stream_shape = (n,) + sample_shape

    def _half(self, items, enc, elem, cls):
        dtype = np.dtype(str(items.get('dtype', 'c8' if enc == '<c4' else 'f4')))
        want = np.dtype(np.complex64 if enc == '<c4' else np.float32)
        if dtype != want:
            raise OSError(f"header: encoded_dtype {enc!r} goes with dtype {want.name}, not {dtype.name}.")
        if (enc == '<c4' and (cls != 6 or elem != 4)) or (enc == '<f2' and (cls != 1 or elem != 2)):
            raise OSError(f"header encoded_dtype {enc!r} does not match the {elem}-byte payload elements.")
        self.half, self.dtype = enc, dtype


class HDF5StreamReader(Base):
    """Read a stream in the reference's intermediate HDF5 format (io/hdf5/base.py:129-222 with
    ``mode='r'``): a file with a 'header' (YAML) and a 'payload' dataset in its root group, written
    by this module OR by the reference itself (h5py with default settings; tests/golden/
    reference_style.h5 was made that way).  Raw payloads (float32 / float64 / complex64 /
    complex128, stored contiguously) come through a memory map; ``bps``-coded and half-precision
    payloads (io/hdf5/payload.py:121-178) are read by `HDF5EncodedStreamReader`, a device stream:
    `open` picks the class, this one refuses such a file.
    ``samples_per_frame``: the stream's frame length (default: up to 2^20 samples)."""

    def __init__(self, name, samples_per_frame=None, *, _structure=None):
        st = _Structure(name) if _structure is None else _structure
        if st.encoded:
            raise OSError(f"{name}: a coded or half-precision payload; hdf5.open(name) reads it "
                          "(as HDF5EncodedStreamReader).")
        items, shape, elem, cls = st.items, st.shape, st.elem, st.cls
        dtype = np.dtype(str(items.get('dtype', 'c8' if (cls == 6 and elem == 8) else 'f4')))
        if dtype.itemsize != elem:
            raise OSError(f"{name}: header dtype {dtype} does not match the {elem}-byte payload elements.")
        if tuple(shape[1:]) != st.sample_shape:
            raise OSError(f"{name}: payload shape {shape} does not match sample_shape {st.sample_shape}.")
        self._text = st.text
        self._data = np.ndarray(shape, dtype, buffer=st.raw, offset=st.address)
        if samples_per_frame is None:
            samples_per_frame = min(shape[0], 1 << 20) if shape[0] else 1
        super().__init__(shape=tuple(shape), start_time=items['time'], sample_rate=float(items['sample_rate']),
                         samples_per_frame=samples_per_frame, dtype=dtype, **_meta(items))

    def host_view(self, start, count):
        return None

    def read(self, count=None, out=None):
        count = self._prepare_read(count, out)
        piece = self._data[self.offset:self.offset + count]
        self.offset += count
        if out is None:
            return np.array(piece)
        out[...] = piece
        return out

    def _read_frame(self, frame_index):
        start = frame_index * self.samples_per_frame
        return np.array(self._data[start:min(start + self.samples_per_frame, self.shape[0])])

    def close(self):
        super().close()
        self._data = None


def _meta(items):
    return {key: items[key] for key in ('frequency', 'sideband', 'polarization') if items.get(key) is not None}


class HDF5EncodedStreamReader(DeviceTaskMixin, HDF5StreamReader):
    """A coded (``bps``) or half-precision ('<f2' / '<c4') payload as a device stream: the bytes of
    the memory map are uploaded as they are and decoded in HBM (coded words by bbt_unpack, every
    frame a headerless sampler frame; half precision by `hip.from_half`), so
    ``Dedisperse(hdf5.open(name), dm)`` moves the stored bytes over PCIe.  ``read()`` returns
    float32 or complex64.  ``samples_per_frame`` is a multiple of the granule of a coded payload
    (whole 32-bit words; at most 2^20 samples and 2^24 components, what one frame of bbt_unpack
    holds), with a possibly shorter last frame."""
    #: samples x components one frame may hold (bounds a frame of bbt_unpack)
    _FRAME_COMPONENTS = 1 << 24

    def __init__(self, name, samples_per_frame=None, *, _structure=None):
        st = _Structure(name) if _structure is None else _structure
        if not st.encoded:
            raise OSError(f"{name}: a raw payload; hdf5.open(name) reads it (as HDF5StreamReader).")
        items = st.items
        self._text = st.text
        self._bps = items.get('bps')
        row = int(np.prod(st.sample_shape, dtype=np.int64)) * (2 if st.dtype.kind == 'c' else 1)
        if self._bps is not None:
            shape = st.stream_shape
            granule = _granule(self._bps, row)
            self._stored = np.ndarray(st.shape, '<u4', buffer=st.raw, offset=st.address)
        else:
            shape = st.shape
            if tuple(shape[1:]) != st.sample_shape:
                raise OSError(f"{name}: payload shape {shape} does not match sample_shape {st.sample_shape}.")
            granule = 1
            self._stored = np.ndarray((shape[0] * row,), '<f2', buffer=st.raw, offset=st.address)
        self.granule, self._row = granule, row
        n = shape[0]
        most = min(1 << 20, max(self._FRAME_COMPONENTS // max(row, 1), granule))
        if samples_per_frame is None:
            samples_per_frame = min(n, most) if n else 1
            if samples_per_frame < n:
                samples_per_frame = max(samples_per_frame // granule * granule, granule)
        samples_per_frame = int(samples_per_frame)
        if samples_per_frame < 1 or samples_per_frame > most or (samples_per_frame < n and samples_per_frame % granule):
            raise ValueError(f"samples_per_frame must be a multiple of the granule ({granule} samples) up to {most} "
                             f"(2^20 samples, 2^24 components), not {samples_per_frame}.")
        Base.__init__(self, shape=tuple(shape), start_time=items['time'], sample_rate=float(items['sample_rate']),
                      samples_per_frame=samples_per_frame, dtype=st.dtype, **_meta(items))

    def _compute_frames(self, first, last, out):
        s0, s1 = self._frame_span(first, last)
        row, spf = self._row, self.samples_per_frame
        if self._bps is None:
            stored = hip.DeviceArray.from_host(np.ascontiguousarray(self._stored[s0 * row:s1 * row]).view(np.float16))
            hip.from_half(stored, np.float32, out=_as_float32(out))
            return
        bps = self._bps
        w0, w1 = s0 * row * bps // 32, -(-s1 * row * bps // 32)        # (frames start on whole words)
        words = hip.DeviceArray.from_host(np.ascontiguousarray(self._stored[w0:w1]).view(np.uint32))
        n_full, rest = divmod(s1 - s0, spf)
        frame_bytes = spf * row * bps // 8
        lib, stream = hip.lib(), hip.get_stream()
        src, dst = words.ptr, out.ptr
        if n_full:
            hip.check(lib.bbt_unpack(src, dst, n_full, frame_bytes, 0, bps, spf, 1, row, 0, stream))
        if rest:                                                       # the stream's last, shorter frame
            hip.check(lib.bbt_unpack(src + n_full * frame_bytes, dst + n_full * spf * row * 4, 1,
                                     -(-rest * row * bps // 32) * 4, 0, bps, rest, 1, row, 0, stream))

    def close(self):
        Base.close(self)
        self._drop_cache()
        self._stored = None


def _as_float32(x):
    """float32 / complex64 `DeviceArray` -> the same memory as flat float32 components."""
    return hip.DeviceArray((x.size * (2 if x.dtype.kind == 'c' else 1),), np.float32, x.ptr, x.owner)


builtins_open = open


def open(name, mode='r', **kwargs):
    """Open an HDF5 file of the reference's intermediate format as a stream
    (reference io/hdf5/base.py:129-222): ``mode='w'`` with ``template=`` (and /
    or the header values as keywords) gives a writer, ``'r'`` a reader for
    files written by this module or by the reference's own writer:
    `HDF5StreamReader` for a raw payload, `HDF5EncodedStreamReader` (a device
    stream) for a coded or half-precision one.  ``samples_per_frame`` sets the
    reader's frame length, of either kind; a raw file is otherwise read and
    checked as it was before compact payloads were added (their checks, a
    truncated file among them, apply to compact files only)."""
    if mode == 'w':
        return HDF5StreamWriter(name, **kwargs)
    if mode == 'r':
        if set(kwargs) - {'samples_per_frame'}:
            raise TypeError("no keywords for reading but samples_per_frame.")
        structure = _Structure(name)
        reader = HDF5EncodedStreamReader if structure.encoded else HDF5StreamReader
        return reader(name, _structure=structure, **kwargs)
    raise ValueError("mode must be 'r' or 'w'.")
