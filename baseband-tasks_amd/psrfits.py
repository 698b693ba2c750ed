"""PSRFITS files: fold-mode archives (the product of a fold) and search-mode files (a dynamic
spectrum), written and read with the data coded in HBM.  Fold mode first; search mode is at the end.

The reference has this as `baseband_tasks.io.psrfits` (core.py: ``open``, `PSRFITSReader`,
`PSRFITSWriter`; hdu.py: the header wrappers, on top of astropy.io.fits).  Astropy is not available
where this package runs, so the file layer is written here, as in `hdf5`: the little of FITS that a
PSRFITS archive needs -- 2880-byte blocks of 80-character cards, the primary HDU, ``BINTABLE``
extensions with the column codes ``A B I J E D`` -- and nothing else; extensions other than
``SUBINT`` (``HISTORY``, ``PSRPARAM``, ``POLYCO``, ...) are stepped over by their size, as the
reference skips them (core.py:107-113).

A fold-mode row stores its profiles as big-endian int16 in (npol, nchan, nbin) order with one
float scale and one float offset per (polarization, channel); a fold makes float32 in (nbin,
nchan, npol) order.  `hip.psrfits_encode` / `hip.psrfits_decode` do that coding in HBM
(csrc/psrfits_kernels.hpp); `encode_rows` / `decode_rows` restate the arithmetic in NumPy, give
the same bytes, and are what the kernels are held to (tests/test_psrfits_gpu.py).

The coding rule (float32, every operation rounded on its own), per (row, pol, chan): ``mn, mx``
over the finite bins; ``offs = 0.5 mn + 0.5 mx``; ``scl = (0.5 mx - 0.5 mn) / 32767``, 1 where that
is not > 0; ``code = clip(rint((x - offs) / scl), -32767, 32767)``, 0 for a bin that is not finite;
without a finite bin ``offs = 0, scl = 1``.  Decoding is psrchive's:
``((float)code - ZERO_OFF) * scl + offs``, then times the channel's ``DAT_WTS`` if asked.

Differences from the reference: this writer scales (the reference stores the float profiles into
the int16 column unscaled: core.py "FIXME add scaling"); ``primary`` is a mapping of header cards,
not an astropy-backed HDU object, and there is no ``PSRFITSPrimaryHDU`` class; ``npol > 1`` works
(``DAT_SCL`` / ``DAT_OFFS`` are indexed ``pol * nchan + chan``, as the format says; the reference
multiplies (npol, nchan, nbin) data by an (npol * nchan, 1) scale); writing past the end raises
EOFError, as `hdf5.HDF5StreamWriter` does; frequencies are in Hz, times are `units.Time`, and leap
seconds are ignored, as `units.Time` does.

Search mode (``OBS_MODE = 'SEARCH'``; `open_search`, `PSRFITSSearchWriter`, `PSRFITSSearchReader`) is
not in the reference; the layout is the PSRFITS definition's and the coding rule is this package's.
A row holds ``NSBLK`` samples of a float32 stream ``(nchan[, npol])`` as unsigned codes of ``NBITS`` =
8, 4, 2 or 1 bits in ``[sample][pol][chan]`` order, channel fastest, the first channel of a byte in
its most significant bits (``TDIM = (NCHAN, NPOL, NSBLK * NBITS / 8)``), with ``DAT_SCL`` and
``DAT_OFFS`` per (pol, chan) and ``DAT_WTS`` per channel; ``NBIN = 1``, ``TBIN = 1 / sample_rate``,
``ZERO_OFF = 0``.  `hip.psrsearch_encode` / `hip.psrsearch_decode` do the coding in HBM
(csrc/psrsearch_kernels.hpp); `encode_search_rows` / `decode_search_rows` restate it in NumPy and are
what the kernels are held to (tests/test_psrfits_search_gpu.py).

The search-mode rule, per (row, pol, chan) over the row's finite samples, in float64 with every
operation rounded on its own: ``n``, ``S1 = sum x``, ``S2 = sum x * x`` (samples in order); ``mean =
S1 / n``; ``std = sqrt(max(S2 / n - mean * mean, 0))``; with ``k = nsigma`` and ``L = 2**nbits``:
``offs = float32(mean - k std)``, ``scl = float32((2 k) std / (L - 1))``; where ``n = 0`` or ``scl``
is not > 0: ``scl = 1``, ``offs = float32(mean)`` (0 when ``n = 0``).  In float32: ``code =
clip(rint((x - offs) / scl), 0, L - 1)``; a sample that is not finite takes the code of
``float32(mean)``.  Reading: ``(code - ZERO_OFF) * DAT_SCL + DAT_OFFS``, times ``DAT_WTS`` if asked.
"""
import re

import numpy as np

from . import hip
from . import units as u
from .base import Base
from .device_task import DeviceTaskMixin
from .units import Time

__all__ = ['open', 'PSRFITSReader', 'PSRFITSWriter', 'encode_rows', 'decode_rows', 'read_hdus', 'card',
           'header_block', 'open_search', 'PSRFITSSearchReader', 'PSRFITSSearchWriter', 'encode_search_rows',
           'decode_search_rows', 'pack_codes', 'unpack_codes']

BLOCK = 2880
CARD = 80
_MJD_UNIX = 40587                     # MJD of 1970-01-01
_F32 = np.float32
_WIDTH = {'A': 1, 'B': 1, 'I': 2, 'J': 4, 'E': 4, 'D': 8}
_NUMPY = {'B': 'u1', 'I': '>i2', 'J': '>i4', 'E': '>f4', 'D': '>f8'}

builtins_open = open


# --------------------------------------------------------------------------- FITS cards
def card(key, value=None, comment=''):
    """One 80-character header card in FITS fixed format: logicals and numbers end in column 30,
    strings are quoted from column 11 and padded to eight characters; ``value=None`` makes a
    commentary card (``COMMENT``, ``END``)."""
    key = str(key).upper()
    if len(key) > 8:
        raise ValueError(f"FITS keyword {key!r} is longer than eight characters.")
    if value is None:
        text = f'{key:<8}' + (('  ' + comment) if comment else '')
        return f'{text[:CARD]:<80}'
    if isinstance(value, (bool, np.bool_)):
        field = f"{'T' if value else 'F':>20}"
    elif isinstance(value, (int, np.integer)):
        field = f'{int(value):>20d}'
    elif isinstance(value, (float, np.floating)):
        value = float(value)
        if not np.isfinite(value):
            raise ValueError(f"FITS card {key}: {value} cannot be written as a number.")
        text = repr(value).upper()
        if '.' not in text and 'E' not in text:
            text += '.'
        elif 'E' in text and '.' not in text:
            text = text.replace('E', '.E')
        field = f'{text:>20}'
    elif isinstance(value, _Fixed):
        field = f'{value.text:>20}'
    else:
        text = str(value).replace("'", "''")
        field = "'" + f'{text:<8}' + "'"
        field = f'{field:<20}'
    text = f'{key:<8}= {field}'
    if comment:
        text += ' / ' + comment
    if len(text) > CARD:
        if len(f'{key:<8}= {field}') > CARD:
            raise ValueError(f"FITS card {key}: the value does not fit 80 characters.")
        text = text[:CARD]
    return f'{text:<80}'


class _Fixed:
    """A number with its text chosen by the writer (``STT_OFFS`` with 15 decimals)."""

    def __init__(self, text):
        self.text = text


def header_block(cards):
    """Cards plus ``END``, padded with blanks to whole 2880-byte blocks."""
    text = ''.join(cards) + card('END')
    text += ' ' * (-len(text) % BLOCK)
    return text.encode('ascii')


_NUMBER = re.compile(r'^[+-]?(\d+\.?\d*|\.\d+)([EeDd][+-]?\d+)?$')


def parse_card(text):
    """(keyword, value, comment) of a card; value None for commentary cards, else bool, int,
    float or str (trailing blanks stripped)."""
    key = text[:8].strip()
    if text[8:10] != '= ':
        return key, None, text[8:].strip()
    body = text[10:]
    stripped = body.lstrip()
    if stripped.startswith("'"):
        out, i = [], 1
        while i < len(stripped):
            ch = stripped[i]
            if ch == "'":
                if stripped[i + 1:i + 2] == "'":
                    out.append("'")
                    i += 2
                    continue
                break
            out.append(ch)
            i += 1
        rest = stripped[i + 1:]
        comment = rest.split('/', 1)[1].strip() if '/' in rest else ''
        return key, ''.join(out).rstrip(), comment
    token, _, comment = body.partition('/')
    token, comment = token.strip(), comment.strip()
    if token == 'T':
        return key, True, comment
    if token == 'F':
        return key, False, comment
    if _NUMBER.match(token):
        if re.match(r'^[+-]?\d+$', token):
            return key, int(token), comment
        return key, float(token.replace('D', 'E').replace('d', 'e')), comment
    return key, token, comment


class Header(dict):
    """The cards of one HDU as a mapping keyword -> value (commentary cards are left out; the
    first card of a repeated keyword counts).  ``comments`` maps keyword -> comment."""

    def __init__(self, cards=()):
        super().__init__()
        self.comments = {}
        for text in cards:
            key, value, comment = parse_card(text)
            if value is not None and key and key not in self:
                self[key] = value
                self.comments[key] = comment


class HDU:
    """Where one header-data unit lies in a file: its `Header`, the offset and size of its data."""

    def __init__(self, header, data_offset, data_size):
        self.header, self.data_offset, self.data_size = header, data_offset, data_size

    @property
    def name(self):
        return 'PRIMARY' if 'SIMPLE' in self.header else str(self.header.get('EXTNAME', '')).strip()


def read_hdus(raw):
    """The HDUs of a FITS file given as bytes (or a memory map): headers parsed, data located by
    ``BITPIX``, ``NAXISn``, ``PCOUNT`` and ``GCOUNT`` and not looked at."""
    hdus, pos, size = [], 0, len(raw)
    while pos < size:
        cards, done = [], False
        while not done:
            block = bytes(raw[pos:pos + BLOCK])
            if len(block) < BLOCK:
                if not cards and not block.strip(b'\0 '):
                    return hdus                             # (trailing padding)
                raise OSError("not a FITS file: a header ends inside a block.")
            pos += BLOCK
            try:
                text = block.decode('ascii')
            except UnicodeDecodeError:
                raise OSError("not a FITS file: a header holds bytes that are not ASCII.") from None
            for i in range(0, BLOCK, CARD):
                one = text[i:i + CARD]
                if one[:8] == 'END     ':
                    done = True
                    break
                cards.append(one)
        header = Header(cards)
        if not hdus and header.get('SIMPLE') is not True:
            raise OSError("not a FITS file: the first card is not SIMPLE = T.")
        if hdus and 'XTENSION' not in header:
            raise OSError("not a FITS file: an extension without XTENSION.")
        naxis = int(header.get('NAXIS', 0))
        nbytes = 0
        if naxis:
            nbytes = abs(int(header['BITPIX'])) // 8
            for k in range(1, naxis + 1):
                nbytes *= int(header[f'NAXIS{k}'])
            nbytes = (nbytes + int(header.get('PCOUNT', 0))) * int(header.get('GCOUNT', 1))
        hdus.append(HDU(header, pos, nbytes))
        pos += -(-nbytes // BLOCK) * BLOCK
    return hdus


def _tform(text):
    m = re.match(r'^\s*(\d*)([A-Z])', str(text))
    if not m or m.group(2) not in _WIDTH:
        raise OSError(f"TFORM {text!r}: only the codes {''.join(_WIDTH)} with a repeat count are read.")
    return (int(m.group(1)) if m.group(1) else 1), m.group(2)


def table_dtype(header):
    """The rows of a ``BINTABLE`` as a NumPy record dtype (big-endian, packed)."""
    names, formats = [], []
    for k in range(1, int(header['TFIELDS']) + 1):
        repeat, code = _tform(header[f'TFORM{k}'])
        names.append(str(header.get(f'TTYPE{k}', f'COL{k}')).strip())
        formats.append(f'S{repeat}' if code == 'A' else (_NUMPY[code], (repeat,)))
    dtype = np.dtype({'names': names, 'formats': formats})
    if dtype.itemsize != int(header['NAXIS1']):
        raise OSError(f"NAXIS1 = {header['NAXIS1']} is not the sum of the TFORM widths, {dtype.itemsize}.")
    return dtype


# --------------------------------------------------------------------------- the coding, in NumPy
def _as_rows(x):
    x = np.asarray(x)
    if not 2 <= x.ndim <= 4:
        raise ValueError(f"profiles have shape (row, bin[, chan[, pol]]), not {x.shape}")
    return np.ascontiguousarray(x, dtype=_F32).reshape(x.shape + (1,) * (4 - x.ndim))


def encode_rows(x):
    """NumPy restatement of `hip.psrfits_encode`: float32 profiles ``(n_row, n_bin[, n_chan[,
    n_pol]])`` -> ``(codes, scl, offs, n_finite)``: '>i2' ``(n_row, n_pol, n_chan, n_bin)`` and
    float32, float32, int32 ``(n_row, n_pol, n_chan)``.  The rule is in the module's docstring."""
    xt = _as_rows(x).transpose(0, 3, 2, 1)                          # (row, pol, chan, bin)
    finite = np.isfinite(xt)
    n_finite = finite.sum(-1, dtype=np.int32)
    some = n_finite > 0
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        mn = np.where(finite, xt, _F32(np.inf)).min(-1)
        mx = np.where(finite, xt, _F32(-np.inf)).max(-1)
        a, b = _F32(0.5) * mn, _F32(0.5) * mx
        offs = np.where(some, a + b, _F32(0.)).astype(_F32)
        scl = (b - a) / _F32(32767.)
        scl = np.where(some & (scl > 0), scl, _F32(1.)).astype(_F32)
        v = (np.where(finite, xt, _F32(0.)) - offs[..., None]) / scl[..., None]
        v = np.clip(np.rint(v), _F32(-32767.), _F32(32767.))
        codes = np.where(finite, v, _F32(0.)).astype(np.int16).astype(hip.PSRFITS_CODE)
    # (reductions over the transposed view come back in its memory order: make them C arrays)
    return tuple(np.ascontiguousarray(a) for a in (codes, scl, offs, n_finite))


def decode_rows(codes, scl, offs, wts=None, zero_off=0.):
    """NumPy restatement of `hip.psrfits_decode`: codes ``(n_row, n_pol, n_chan, n_bin)``, ``scl``
    and ``offs (n_row, n_pol, n_chan)``, optional weights ``(n_row, n_chan)`` -> float32 ``(n_row,
    n_bin, n_chan, n_pol)``; subtraction, product and sum each rounded to float32."""
    codes = np.asarray(codes)
    n_row, n_pol, n_chan, n_bin = codes.shape
    scl = np.asarray(scl, dtype=_F32).reshape(n_row, n_pol, n_chan, 1)
    offs = np.asarray(offs, dtype=_F32).reshape(n_row, n_pol, n_chan, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        t = codes.astype(_F32) - _F32(zero_off)
        t = t * scl
        t = t + offs
        if wts is not None:
            t = t * np.asarray(wts, dtype=_F32).reshape(n_row, 1, n_chan, 1)
    return np.ascontiguousarray(t.transpose(0, 3, 2, 1))


# --------------------------------------------------------------------------- times
def _stt(time):
    """(STT_IMJD, STT_SMJD, STT_OFFS as written, what of the fraction the text leaves out)."""
    days, sec = divmod(int(time.sec), 86400)
    text = '%.15f' % time.frac
    if text.startswith('1'):                                # (cannot happen for frac < 1 - 5e-16; be safe)
        text = '0.999999999999999'
    return days + _MJD_UNIX, sec, text, time.frac - float(text)


def _from_stt(imjd, smjd, offs, extra=0.):
    whole = np.floor(extra)
    return Time((int(imjd) - _MJD_UNIX) * 86400 + int(smjd) + int(whole), float(offs) + float(extra - whole))


def _number(value, default=None):
    """A header value as a float; ``default`` when it is '*' or otherwise not a number."""
    if isinstance(value, (bool, np.bool_)) or value is None:
        return default
    try:
        return float(value)
    except (TypeError, ValueError):
        return default


# --------------------------------------------------------------------------- reader
def _open_subint(name):
    """A PSRFITS file with one ``SUBINT`` table: (memory map, HDUs, primary header, the table's HDU,
    ``OBS_MODE``)."""
    raw = np.memmap(name, mode='r')
    try:
        hdus = read_hdus(raw)
    except OSError as exc:
        raise OSError(f"{name}: {exc}") from None
    primary = hdus[0].header
    if str(primary.get('FITSTYPE', '')).strip() != 'PSRFITS':
        raise ValueError(f"{name}: the primary header is not that of a PSRFITS file (FITSTYPE).")
    subints = [h for h in hdus[1:] if h.name == 'SUBINT']
    if len(subints) != 1:
        raise RuntimeError(f"{name}: {len(subints)} SUBINT extensions; exactly one can be read.")
    return raw, hdus, primary, subints[0], str(primary.get('OBS_MODE', '')).strip().upper()


def _subint_meta(name, header, rows, nchan, npol):
    """``frequency``, ``sideband`` and ``polarization`` of a stream, from ``DAT_FREQ``, ``CHAN_BW``
    and ``POL_TYPE``, where the table has them."""
    meta = {}
    chan_bw = _number(header.get('CHAN_BW'))
    if 'DAT_FREQ' in rows.dtype.names and len(rows) and chan_bw:
        freq = np.asarray(rows['DAT_FREQ'], dtype=np.float64)
        if not np.array_equiv(freq[0], freq):
            raise ValueError(f"{name}: the frequencies are not the same for all rows.")
        meta['frequency'] = freq[0].reshape(nchan, 1) * u.MHz
        meta['sideband'] = np.int8(1 if chan_bw > 0 else -1)
    pol_type = str(header.get('POL_TYPE', '')).strip()
    per = len(pol_type) // npol
    if per and pol_type != '*':
        meta['polarization'] = np.array([pol_type[k * per:(k + 1) * per] for k in range(npol)])
    return meta


class PSRFITSReader(DeviceTaskMixin, Base):
    """The ``SUBINT`` table of a PSRFITS fold-mode archive as a device stream (reference
    core.py:180-222 and hdu.py:258-566): one sample per row, of shape ``(nbin, nchan, npol)``,
    float32.  A read uploads the stored big-endian int16 codes of a run of rows as they are, with
    their scales, offsets and weights, and decodes them in HBM: ``read_device`` (and so a task on
    top: ``Integrate(psrfits.open(name), n)``) never has float profiles on the host.

    ``weighted``: multiply by ``DAT_WTS`` (default True, as in the reference).
    ``primary`` and ``header`` are the cards of the primary and the ``SUBINT`` HDU, as mappings."""

    def __init__(self, name, weighted=True):
        raw, self.hdus, primary, hdu, mode = _open_subint(name)
        if mode != 'PSR':
            raise ValueError(f"{name}: '{mode}' is not a mode this reader has (fold mode, 'PSR', only).")
        header = hdu.header
        self.primary, self.header, self.weighted = primary, header, bool(weighted)
        nrow = int(header['NAXIS2'])
        nbin, nchan, npol = int(header['NBIN']), int(header['NCHAN']), int(header['NPOL'])
        dtype = table_dtype(header)
        if hdu.data_offset + nrow * dtype.itemsize > raw.shape[0]:
            raise OSError(f"{name}: the SUBINT table needs {hdu.data_offset + nrow * dtype.itemsize} bytes, "
                          f"the file has {raw.shape[0]} (truncated).")
        rows = np.ndarray((nrow,), dtype, buffer=raw, offset=hdu.data_offset)
        for column in ('TSUBINT', 'DAT_SCL', 'DAT_OFFS', 'DATA'):
            if column not in dtype.names:
                raise OSError(f"{name}: the SUBINT table has no {column} column.")
        if (dtype['DATA'].base != hip.PSRFITS_CODE or dtype['DATA'].shape != (nbin * nchan * npol,)
                or dtype['DAT_SCL'].shape != (nchan * npol,) or dtype['DAT_OFFS'].shape != (nchan * npol,)):
            raise OSError(f"{name}: DATA, DAT_SCL or DAT_OFFS do not match NBIN, NCHAN, NPOL = {nbin}, {nchan}, {npol} "
                          "(16-bit fold-mode profiles only).")
        self._rows, self._raw = rows, raw
        self._dims = (nbin, nchan, npol)
        self._has_wts = 'DAT_WTS' in dtype.names and dtype['DAT_WTS'].shape == (nchan,)
        self.zero_off = _number(header.get('ZERO_OFF'), 0.)
        tsubint = np.asarray(rows['TSUBINT'], dtype=np.float64).reshape(nrow)
        extra = 0.
        if 'OFFS_SUB' in dtype.names and nrow:
            extra = float(rows['OFFS_SUB'][0, 0]) - float(tsubint[0]) / 2.
        start = _from_stt(primary['STT_IMJD'], primary['STT_SMJD'], _number(primary.get('STT_OFFS'), 0.), extra)
        meta = _subint_meta(name, header, rows, nchan, npol)
        Base.__init__(self, shape=(nrow, nbin, nchan, npol), start_time=start,
                      sample_rate=1. / float(tsubint.mean()) if nrow else 1., samples_per_frame=1,
                      dtype=np.float32, **meta)

    def _compute_frames(self, first, last, out):
        s0, s1 = self._frame_span(first, last)
        nbin, nchan, npol = self._dims
        rows = self._rows[s0:s1]
        n = s1 - s0
        codes = hip.DeviceArray.from_host(np.ascontiguousarray(rows['DATA']).reshape(n, npol, nchan, nbin))
        scl = hip.DeviceArray.from_host(rows['DAT_SCL'].astype(np.float32).reshape(n, npol, nchan))
        offs = hip.DeviceArray.from_host(rows['DAT_OFFS'].astype(np.float32).reshape(n, npol, nchan))
        wts = None
        if self.weighted and self._has_wts:
            wts = hip.DeviceArray.from_host(rows['DAT_WTS'].astype(np.float32).reshape(n, nchan))
        hip.psrfits_decode(codes, scl, offs, wts, self.zero_off, out=out)

    def close(self):
        Base.close(self)
        self._drop_cache()
        self._rows = self._raw = None


# --------------------------------------------------------------------------- writer
_FIXED_PRIMARY = ('SIMPLE', 'BITPIX', 'NAXIS', 'EXTEND', 'FITSTYPE', 'OBS_MODE')


def _per_bin_free(value, sample_shape, dims, what):
    """A metadata value of the stream, which broadcasts against its sample shape, as an
    ``(nchan, npol)`` array; it may not depend on the bin."""
    full = np.broadcast_to(np.asarray(value), sample_shape)
    if full.strides[0] != 0 and full.shape[0] > 1 and not np.all(full == full[:1]):
        raise ValueError(f"{what} differs between bins: a SUBINT row holds one per channel.")
    return np.array(full[0]).reshape(dims[1:])


def _per_channel(value, sample_shape, dims, what):
    """As `_per_bin_free`, one value per channel: it may not depend on the polarization either."""
    per = _per_bin_free(value, sample_shape, dims, what)
    if not np.all(per == per[:, :1]):
        raise ValueError(f"{what} differs between polarizations: a SUBINT row holds one per channel.")
    return per[:, 0]


def _real_float32(template, dtype):
    """The dtype of a stream a writer takes, float32; what it cannot store raises TypeError."""
    dtype = np.dtype(np.float32 if dtype is None else dtype)
    if dtype.kind == 'c':
        raise TypeError("fold-mode archives hold real profiles: a complex stream cannot be written "
                        "(detect it first: Square, Power).")
    if dtype.names is not None:
        raise TypeError("a structured stream (average=False: sums and counts) cannot be written; "
                        "fold with average=True.")
    if dtype != np.dtype(np.float32):
        raise TypeError(f"fold-mode archives are written from float32 streams, not {dtype}.")
    if getattr(template, '_time_from_offsets', False):
        raise TypeError("the samples of this stream are not uniform in time (PulseStack, phase-binned "
                        "Integrate): its rows cannot be given one TSUBINT.")
    return dtype


def _primary_cards(mode, start_time, frequency, sideband, sample_shape, dims, chan_bw, primary):
    """The primary HDU of a file in ``mode`` ('PSR', 'SEARCH') as keyword -> (value, comment), with
    the channel frequencies (MHz), the signed channel width (MHz; None without frequencies) and
    what of the start time ``STT_OFFS`` leaves out.  ``dims`` is ``(nbin, nchan, npol)`` and
    ``sample_shape`` what frequency and sideband broadcast against."""
    nchan = dims[1]
    imjd, smjd, offs_text, offs_rest = _stt(start_time)
    cards = {'SIMPLE': (True, 'file does conform to FITS standard'), 'BITPIX': (8, 'number of bits per data pixel'),
             'NAXIS': (0, 'number of data axes'), 'EXTEND': (True, 'FITS dataset may contain extensions'),
             'HDRVER': ('5.4', 'Header version'), 'FITSTYPE': ('PSRFITS', 'FITS definition for pulsar data files'),
             'OBS_MODE': (mode, '(PSR, CAL, SEARCH)')}
    freq_mhz = np.zeros(nchan)
    width = None
    if frequency is not None:
        freq_mhz = _per_channel(u.to_hz(frequency), sample_shape, dims, 'frequency') / u.MHz
        side = _per_channel(sideband, sample_shape, dims, 'sideband')
        if not np.all(side == side[0]):
            raise ValueError("sideband differs between channels: CHAN_BW has one sign.")
        side = 1. if side[0] > 0 else -1.
        if chan_bw is not None:
            width = abs(u.to_hz(chan_bw)) / u.MHz
        elif nchan > 1:
            width = abs(float(freq_mhz[1] - freq_mhz[0]))
        else:
            raise ValueError("a single channel does not tell its width: pass chan_bw (Hz).")
        # OBSFREQ, OBSBW, OBSNCHAN as the reference sets them (hdu.py:154-166, 172-175): channel 0
        # put back below the first, the centre is channel (nchan + 1) // 2 of the padded band
        step = float(freq_mhz[1] - freq_mhz[0]) if nchan > 1 else side * width
        padded = np.insert(freq_mhz, 0, freq_mhz[0] - step)
        cards['OBSFREQ'] = (float(padded[(nchan + 1) // 2]), '[MHz] Centre frequency for observation')
        cards['OBSBW'] = (side * float(np.ptp(padded)), '[MHz] Bandwidth for observation')
        cards['OBSNCHAN'] = (nchan, 'Number of frequency channels (original)')
        width = side * width
    cards['STT_IMJD'] = (imjd, 'Start MJD (UTC days) (J - long integer)')
    cards['STT_SMJD'] = (smjd, '[s] Start time (sec past UTC 00h) (J)')
    cards['STT_OFFS'] = (_Fixed(offs_text), '[s] Start time offset (D)')
    cards['DATE-OBS'] = (start_time.isot[:23], 'Date of observation (YYYY-MM-DDThh:mm:ss UTC)')
    for key, value in dict(primary or {}).items():
        key = str(key).upper()
        if key in _FIXED_PRIMARY:
            raise ValueError(f"the primary card {key} is the writer's own.")
        cards[key] = value if isinstance(value, tuple) else (value, '')
    return cards, freq_mhz, width, offs_rest


def _pol_type(polarization, sample_shape, dims):
    """``POL_TYPE``: the stream's labels joined, or the usual name for the number of polarizations."""
    if polarization is not None:
        labels = _per_bin_free(polarization, sample_shape, dims, 'polarization')[0]
        return ''.join(str(p) for p in labels)
    return {1: 'INTEN', 2: 'AABB', 4: 'IQUV'}.get(dims[2], '*')


def _subint_cards(columns, nrow, tdim, tdim_comment, pol_type, dims, width, tbin, nbits, nsblk):
    """The cards of a ``SUBINT`` header with ``columns`` (name, TFORM, unit, comment), the last of
    them ``DATA`` with ``TDIM = tdim``, and the bytes of a row."""
    nbin, nchan, npol = dims
    row_bytes = sum(_tform(form)[0] * _WIDTH[_tform(form)[1]] for _, form, _, _ in columns)
    sub = [card('XTENSION', 'BINTABLE', '***** Subintegration data  *****'), card('BITPIX', 8, 'N/A'),
           card('NAXIS', 2, '2-dimensional binary table'), card('NAXIS1', row_bytes, 'width of table in bytes'),
           card('NAXIS2', nrow, 'Number of rows in table (NSUBINT)'),
           card('PCOUNT', 0, 'size of special data area'), card('GCOUNT', 1, 'one data group (required keyword)'),
           card('TFIELDS', len(columns), 'Number of fields per row')]
    for k, (ttype, form, unit, comment) in enumerate(columns, start=1):
        sub += [card(f'TTYPE{k}', ttype, comment), card(f'TFORM{k}', form)]
        if unit:
            sub.append(card(f'TUNIT{k}', unit, 'Units of field'))
    sub += [card(f'TDIM{len(columns)}', tdim, tdim_comment),
            card('EXTNAME', 'SUBINT', 'name of this binary table extension'),
            card('INT_TYPE', 'TIME', 'Time axis (TIME, BINPHSPERI, BINLNGASC, etc)'),
            card('INT_UNIT', 'SEC', 'Unit of time axis (SEC, PHS (0-1), DEG)'),
            card('POL_TYPE', pol_type, 'Polarisation identifier (e.g., AABBCRCI, AA+BB)'),
            card('NPOL', npol, 'Nr of polarisations'), card('NBIN', nbin, 'Nr of bins (PSR/CAL mode; else 1)'),
            card('NCHAN', nchan, 'Number of channels/sub-bands in this file'),
            card('CHAN_BW', float(width) if width is not None else '*', '[MHz] Channel/sub-band width'),
            card('TBIN', float(tbin) if tbin is not None else '*', '[s] Time per bin or sample'),
            card('NBITS', nbits, 'Nr of bits/datum (SEARCH mode data, else 1)'),
            card('NSBLK', nsblk, 'Samples/row (SEARCH mode, else 1)'),
            card('ZERO_OFF', 0, 'Zero offset for SEARCH-mode data')]
    return sub, row_bytes


class _SubintWriter:
    """What the writers of the two modes share: samples go in order, the file keeps its promised size."""
    accepts_device = True

    def tell(self):
        return self.offset

    def __setitem__(self, item, value):
        start, stop, step = item.indices(self.shape[0])
        assert start == self.offset, 'Can only assign right following pointer.'
        assert step == 1, 'unity step size only is supported'
        assert len(value) == stop - start, 'number of samples should match.'
        self.write(value)

    def close(self):
        if not self.closed:
            self.closed = True
            self._fh.truncate(self._eof)           # (pads to a whole block; a short file keeps the promised size)
            self._fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class PSRFITSWriter(_SubintWriter):
    """Write a stream of folded profiles into a PSRFITS fold-mode archive: a primary HDU and one
    ``SUBINT`` table, one row per sample (reference core.py:225-278, whose writer does not scale).

    ``template`` is a `~baseband_tasks_amd.integration.Fold` or any float32 stream of uniform rate
    with sample shape ``(nbin,)``, ``(nbin, nchan)`` or ``(nbin, nchan, npol)``; it supplies
    ``shape, start_time, sample_rate, frequency, sideband, polarization``, and keywords of those
    names override it.  ``primary`` maps further primary-header keywords (``TELESCOP``,
    ``SRC_NAME``, ``RA``, ``DEC``, ``ANT_X``, ...) to values (or ``(value, comment)``), written as
    given.  ``chan_bw`` (Hz): the channel width, by default the spacing of the frequencies; a
    single channel with a frequency needs it.  ``tbin`` (s): the ``TBIN`` card, the time per bin
    of the fold, which a stream does not tell ('*' when not given).

    Samples go in order through ``write(data)`` or ``fw[a:b] = data``.  A `hip.DeviceArray` piece
    is coded in HBM (`hip.psrfits_encode`) and only codes, scales, offsets and counts come down
    (`accepts_device`: ``Fold(...).read(out=writer)`` streams a fold into the archive); an ndarray
    piece goes through `encode_rows`, to the same bytes.  ``DAT_WTS`` of a channel is 0 when none
    of its polarizations has a finite bin in the row, else 1.  The header is written on opening,
    ``close()`` pads to a whole block, and a short file keeps the promised size."""
    def __init__(self, name, template=None, primary=None, *, shape=None, start_time=None, sample_rate=None,
                 frequency=None, sideband=None, polarization=None, dtype=None, chan_bw=None, tbin=None):
        get = lambda key, given: given if given is not None else getattr(template, key, None)
        dtype = _real_float32(template, get('dtype', dtype))
        shape = get('shape', shape)
        if shape is None:
            raise TypeError("'shape' should either be defined by the template or passed in.")
        shape = tuple(int(d) for d in shape)
        if not 2 <= len(shape) <= 4 or min(shape[1:]) < 1 or shape[0] < 0:
            raise ValueError(f"a fold-mode stream has shape (nrow, nbin[, nchan[, npol]]), not {shape}.")
        self.shape, self.sample_shape, self.dtype = shape, shape[1:], dtype
        nbin, nchan, npol = shape[1:] + (1,) * (4 - len(shape))
        self._dims = (nbin, nchan, npol)
        rate, start = get('sample_rate', sample_rate), get('start_time', start_time)
        if rate is None or start is None:
            raise TypeError("'sample_rate' and 'start_time' should either be defined by the template or passed in.")
        self.sample_rate, self.start_time = u.to_hz(rate), Time(start)
        self.frequency, self.sideband = get('frequency', frequency), get('sideband', sideband)
        self.polarization = get('polarization', polarization)
        if (self.frequency is None) != (self.sideband is None):
            raise ValueError('frequency and sideband should both be passed in.')

        cards, freq_mhz, width, offs_rest = _primary_cards('PSR', self.start_time, self.frequency, self.sideband,
                                                           self.sample_shape, self._dims, chan_bw, primary)
        self.primary = {key: value for key, (value, _) in cards.items()}
        head = header_block([card(key, value, comment) for key, (value, comment) in cards.items()])

        pol_type = _pol_type(self.polarization, self.sample_shape, self._dims)
        columns = [('TSUBINT', '1D', 's', 'Length of subintegration'),
                   ('OFFS_SUB', '1D', 's', 'Offset from Start of subint centre'),
                   ('DAT_FREQ', f'{nchan}D', 'MHz', '[MHz] Centre frequency for each channel'),
                   ('DAT_WTS', f'{nchan}E', None, 'Weights for each channel'),
                   ('DAT_OFFS', f'{nchan * npol}E', None, 'Data offset for each channel'),
                   ('DAT_SCL', f'{nchan * npol}E', None, 'Data scale factor (outval=dataval*scl + offs)'),
                   ('DATA', f'{nbin * nchan * npol}I', None, 'Subint data table')]
        sub, self.row_bytes = _subint_cards(columns, shape[0], f'({nbin},{nchan},{npol})', '(NBIN,NCHAN,NPOL)',
                                            pol_type, self._dims, width, tbin, 1, 1)
        head += header_block(sub)
        self._data_at = len(head)
        self._eof = self._data_at + -(-shape[0] * self.row_bytes // BLOCK) * BLOCK
        self._tsubint = 1. / self.sample_rate
        self._offs0 = offs_rest                               # (start - STT: what STT_OFFS' 15 decimals leave out)
        self._freq = np.asarray(freq_mhz, dtype='>f8').tobytes()
        self._fh = builtins_open(name, 'wb')
        self._fh.write(head)
        self.offset = 0
        self.closed = False

    def _encode(self, data):
        n = data.shape[0]
        if isinstance(data, hip.DeviceArray) and data.dtype == self.dtype:
            return [a.to_host() for a in hip.psrfits_encode(data.reshape((n,) + self._dims))]
        if hasattr(data, 'to_host'):
            data = data.to_host()
        return encode_rows(np.ascontiguousarray(data, dtype=self.dtype).reshape((n,) + self._dims))

    def write(self, data):
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        if not hasattr(data, 'to_host'):
            data = np.asarray(data)
        assert tuple(data.shape[1:]) == self.sample_shape, f"'data' must have trailing shape {self.sample_shape}"
        n = data.shape[0]
        if self.offset + n > self.shape[0]:
            raise EOFError("cannot write beyond the length given in the header.")
        if n == 0:
            return
        codes, scl, offs, n_finite = self._encode(data)
        wts = (n_finite.sum(axis=1) > 0).astype('>f4')                  # (row, chan)
        scl, offs = scl.astype('>f4'), offs.astype('>f4')
        codes = np.ascontiguousarray(codes, dtype=hip.PSRFITS_CODE)
        for k in range(n):
            sub = self._offs0 + (self.offset + k + 0.5) * self._tsubint
            self._fh.write(np.array([self._tsubint, sub], '>f8').tobytes() + self._freq + wts[k].tobytes()
                           + offs[k].tobytes() + scl[k].tobytes())
            self._fh.write(codes[k].data)
        self.offset += n


def open(name, mode='r', **kwargs):
    """Open a PSRFITS fold-mode archive as a stream (reference io/psrfits/core.py:16-89):
    ``mode='r'`` (with ``weighted=True``) gives a `PSRFITSReader`, a device stream of the one
    ``SUBINT`` table; ``mode='w'`` with ``template=`` (and / or ``shape, start_time, sample_rate,
    frequency, sideband, polarization`` as keywords) and an optional mapping ``primary`` of further
    primary-header cards gives a `PSRFITSWriter`."""
    if mode == 'w':
        return PSRFITSWriter(name, **kwargs)
    if mode == 'r':
        if set(kwargs) - {'weighted'}:
            raise TypeError("no keywords for reading but weighted.")
        return PSRFITSReader(name, **kwargs)
    raise ValueError(f"Unknown mode '{mode}'. Currently only modes 'r' and 'w' are supported.")


# --------------------------------------------------------------------------- search mode
#: ``nsigma`` by ``nbits``: the coded range is mean +- nsigma std.  Policy, not measurement: 8 and 4
#: bits leave room for signal above the noise; 2 bits put the four levels 1 std apart, close to the
#: optimal four-level quantiser of normal noise; 1 bit has its threshold at the mean and decodes
#: to mean +- std.
SEARCH_NSIGMA = {8: 6.0, 4: 3.0, 2: 1.5, 1: 1.0}
#: samples of a row (``NSBLK``) unless given
SEARCH_NSBLK = 4096


def _search_bits(nbits, nsigma=None):
    if isinstance(nbits, (bool, np.bool_)) or nbits not in SEARCH_NSIGMA:
        raise ValueError(f"nbits must be one of 1, 2, 4, 8, not {nbits!r}.")
    nsigma = float(SEARCH_NSIGMA[nbits] if nsigma is None else nsigma)
    if not 0. < nsigma < np.inf:
        raise ValueError(f"nsigma must be positive and finite, not {nsigma}.")
    return int(nbits), nsigma


def pack_codes(codes, nbits):
    """Codes below ``2**nbits`` along the last axis -> bytes, ``8 / nbits`` codes a byte, the
    first in the most significant bits (4 bits: 1, 2, 3, 4 -> 0x12 0x34)."""
    nbits, _ = _search_bits(nbits)
    codes = np.asarray(codes, dtype=np.uint8)
    per = 8 // nbits
    if codes.shape[-1] % per:
        raise ValueError(f"{codes.shape[-1]} codes of {nbits} bits do not fill whole bytes.")
    groups = codes.reshape(codes.shape[:-1] + (codes.shape[-1] // per, per))
    shifts = (nbits * (per - 1 - np.arange(per))).astype(np.uint8)
    return np.bitwise_or.reduce(groups << shifts, axis=-1).astype(np.uint8)


def unpack_codes(data, nbits):
    """The inverse of `pack_codes`: bytes along the last axis -> ``8 / nbits`` codes each."""
    nbits, _ = _search_bits(nbits)
    data = np.asarray(data, dtype=np.uint8)
    per = 8 // nbits
    shifts = (nbits * (per - 1 - np.arange(per))).astype(np.uint8)
    codes = (data[..., None] >> shifts) & np.uint8((1 << nbits) - 1)
    return codes.reshape(data.shape[:-1] + (data.shape[-1] * per,))


def _search_rows(x, nsblk):
    x = np.asarray(x)
    if not 2 <= x.ndim <= 3:
        raise ValueError(f"samples have shape (n, chan[, pol]), not {x.shape}")
    nsblk = int(nsblk)
    if nsblk < 1 or x.shape[0] % nsblk:
        raise ValueError(f"{x.shape[0]} samples are not a whole number of rows of {nsblk}.")
    x = np.ascontiguousarray(x, dtype=_F32)
    return x.reshape((x.shape[0] // nsblk, nsblk) + x.shape[1:] + (1,) * (3 - x.ndim))


def encode_search_rows(x, nsblk, nbits=8, nsigma=None, scl=None, offs=None):
    """NumPy restatement of `hip.psrsearch_encode`: float32 samples ``(n, n_chan[, n_pol])``, ``n``
    a whole number of rows of ``nsblk`` -> ``(codes, scl, offs, n_finite)``: uint8 ``(n_row, nsblk,
    n_pol, n_chan * nbits / 8)`` and float32, float32, int32 ``(n_row, n_pol, n_chan)``.  The rule
    is in the module's docstring; the sums run over the samples in order.  With ``scl`` and
    ``offs`` given (``(n_row, n_pol, n_chan)``), the samples are coded with those."""
    nbits, k = _search_bits(nbits, nsigma)
    xr = _search_rows(x, nsblk)                                      # (row, sample, chan, pol)
    n_row, nsblk, n_chan, n_pol = xr.shape
    if n_chan * nbits % 8:
        raise ValueError(f"{n_chan} channels of {nbits} bits do not fill whole bytes.")
    top = (1 << nbits) - 1
    s1 = np.zeros((n_row, n_chan, n_pol), np.float64)
    s2 = np.zeros((n_row, n_chan, n_pol), np.float64)
    n = np.zeros((n_row, n_chan, n_pol), np.int32)
    for s in range(nsblk):
        ok = np.isfinite(xr[:, s])
        d = np.where(ok, xr[:, s], _F32(0.)).astype(np.float64)
        s1 = s1 + d
        s2 = s2 + d * d
        n += ok
    some = n > 0
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        dn = np.where(some, n, 1).astype(np.float64)
        mean = s1 / dn
        var = s2 / dn - mean * mean
        std = np.sqrt(np.where(var > 0., var, 0.))
        fill = np.where(some, mean, 0.).astype(_F32)
        own_offs = (mean - k * std).astype(_F32)
        own_scl = ((2. * k) * std / float(top)).astype(_F32)
        flat = ~(some & (own_scl > 0))
        own_scl = np.where(flat, _F32(1.), own_scl)
        own_offs = np.where(flat, fill, own_offs)
        if scl is None:
            scl_c, offs_c = own_scl, own_offs
        else:
            scl_c = np.asarray(scl, dtype=_F32).reshape(n_row, n_pol, n_chan).transpose(0, 2, 1)
            offs_c = np.asarray(offs, dtype=_F32).reshape(n_row, n_pol, n_chan).transpose(0, 2, 1)
        v = np.where(np.isfinite(xr), xr, fill[:, None])
        v = (v - offs_c[:, None]) / scl_c[:, None]
        v = np.clip(np.rint(v), _F32(0.), _F32(top))
        codes = np.where(np.isnan(v), _F32(0.), v).astype(np.uint8)
    data = pack_codes(codes.transpose(0, 1, 3, 2), nbits)              # (row, sample, pol, chan) -> bytes
    return (np.ascontiguousarray(data),) + tuple(
        np.ascontiguousarray(a.transpose(0, 2, 1)) for a in (scl_c.astype(_F32), offs_c.astype(_F32), n))


def decode_search_rows(codes, scl, offs, wts=None, zero_off=0., nbits=8):
    """NumPy restatement of `hip.psrsearch_decode`: bytes ``(n_row, nsblk, n_pol, n_chan * nbits /
    8)``, ``scl`` and ``offs (n_row, n_pol, n_chan)``, optional weights ``(n_row, n_chan)`` ->
    float32 ``(n_row * nsblk, n_chan, n_pol)``; subtraction, product and sum each rounded to
    float32."""
    codes = unpack_codes(codes, nbits)
    n_row, nsblk, n_pol, n_chan = codes.shape
    scl = np.asarray(scl, dtype=_F32).reshape(n_row, 1, n_pol, n_chan)
    offs = np.asarray(offs, dtype=_F32).reshape(n_row, 1, n_pol, n_chan)
    with np.errstate(invalid='ignore', over='ignore'):
        t = codes.astype(_F32) - _F32(zero_off)
        t = t * scl
        t = t + offs
        if wts is not None:
            t = t * np.asarray(wts, dtype=_F32).reshape(n_row, 1, 1, n_chan)
    return np.ascontiguousarray(t.transpose(0, 1, 3, 2)).reshape(n_row * nsblk, n_chan, n_pol)


class PSRFITSSearchWriter(_SubintWriter):
    """Write a dynamic spectrum into a PSRFITS search-mode file: a primary HDU with ``OBS_MODE =
    'SEARCH'`` and one ``SUBINT`` table whose rows hold ``nsblk`` samples each, as unsigned codes
    of ``nbits`` = 8, 4, 2 or 1 bits with a scale, an offset and a weight per channel and row.

    ``template`` is any float32 stream of uniform rate with sample shape ``(nchan,)`` or ``(nchan,
    npol)`` (``Integrate(Power(Channelize(...)), n)``); it supplies ``shape, start_time,
    sample_rate, frequency, sideband, polarization``, and keywords of those names override it.
    ``primary`` and ``chan_bw`` are `PSRFITSWriter`'s.  ``nsigma``: the coded range is mean +-
    nsigma std of the row (default by ``nbits``: `SEARCH_NSIGMA`).  The length must be a whole
    number of rows and ``nchan * nbits`` and ``nsblk * nbits`` multiples of 8.

    Samples go in order through ``write(data)`` or ``fw[a:b] = data``, in pieces that are whole
    rows: a multiple of `granule` = ``nsblk`` samples (the writer does not buffer; it raises
    ValueError otherwise).  ``read(out=writer)`` hands over runs of the stream's frames, so a
    stream whose ``samples_per_frame`` is a multiple of ``nsblk`` meets this.  A `hip.DeviceArray`
    piece is coded in HBM (`hip.psrsearch_encode`) and only bytes, scales, offsets and counts come
    down; an ndarray piece goes through `encode_search_rows`, to the same layout.  ``DAT_WTS`` of
    a channel is 0 when none of its polarizations has a finite sample in the row, else 1.  The
    header is written on opening, ``close()`` pads to a whole block."""
    def __init__(self, name, template=None, primary=None, *, nbits=8, nsblk=SEARCH_NSBLK, nsigma=None, shape=None,
                 start_time=None, sample_rate=None, frequency=None, sideband=None, polarization=None, dtype=None,
                 chan_bw=None):
        get = lambda key, given: given if given is not None else getattr(template, key, None)
        dtype = _real_float32(template, get('dtype', dtype))
        self.nbits, self.nsigma = _search_bits(nbits, nsigma)
        shape = get('shape', shape)
        if shape is None:
            raise TypeError("'shape' should either be defined by the template or passed in.")
        shape = tuple(int(d) for d in shape)
        if not 2 <= len(shape) <= 3 or min(shape[1:]) < 1 or shape[0] < 0:
            raise ValueError(f"a search-mode stream has shape (nsample, nchan[, npol]), not {shape}.")
        self.shape, self.sample_shape, self.dtype = shape, shape[1:], dtype
        nchan, npol = shape[1:] + (1,) * (3 - len(shape))
        nsblk = int(nsblk)
        if nsblk < 1:
            raise ValueError(f"nsblk must be positive, not {nsblk}.")
        if nchan * self.nbits % 8:
            raise ValueError(f"{nchan} channels of {self.nbits} bits do not fill whole bytes: nchan * nbits "
                             "must be a multiple of 8.")
        if nsblk * self.nbits % 8:
            raise ValueError(f"nsblk * nbits = {nsblk * self.nbits} must be a multiple of 8 (TDIM counts bytes).")
        if shape[0] % nsblk:
            near = max(int(round(shape[0] / nsblk)), 1) * nsblk
            raise ValueError(f"{shape[0]} samples are not a whole number of rows of nsblk = {nsblk}: "
                             f"the nearest length that is, is {near}.")
        self.nsblk = self.granule = nsblk
        self._dims = (1, nchan, npol)
        self.nrow = shape[0] // nsblk
        rate, start = get('sample_rate', sample_rate), get('start_time', start_time)
        if rate is None or start is None:
            raise TypeError("'sample_rate' and 'start_time' should either be defined by the template or passed in.")
        self.sample_rate, self.start_time = u.to_hz(rate), Time(start)
        self.frequency, self.sideband = get('frequency', frequency), get('sideband', sideband)
        self.polarization = get('polarization', polarization)
        if (self.frequency is None) != (self.sideband is None):
            raise ValueError('frequency and sideband should both be passed in.')

        binned = (1,) + self.sample_shape                     # (the helpers take a leading bin axis)
        cards, freq_mhz, width, offs_rest = _primary_cards('SEARCH', self.start_time, self.frequency, self.sideband,
                                                           binned, self._dims, chan_bw, primary)
        self.primary = {key: value for key, (value, _) in cards.items()}
        head = header_block([card(key, value, comment) for key, (value, comment) in cards.items()])
        pol_type = _pol_type(self.polarization, binned, self._dims)
        self._data_bytes = nsblk * npol * nchan * self.nbits // 8
        columns = [('TSUBINT', '1D', 's', 'Length of subintegration'),
                   ('OFFS_SUB', '1D', 's', 'Offset from Start of subint centre'),
                   ('DAT_FREQ', f'{nchan}D', 'MHz', '[MHz] Centre frequency for each channel'),
                   ('DAT_WTS', f'{nchan}E', None, 'Weights for each channel'),
                   ('DAT_OFFS', f'{nchan * npol}E', None, 'Data offset for each channel'),
                   ('DAT_SCL', f'{nchan * npol}E', None, 'Data scale factor (outval=dataval*scl + offs)'),
                   ('DATA', f'{self._data_bytes}B', None, 'Subint data table')]
        self._tbin = 1. / self.sample_rate
        sub, self.row_bytes = _subint_cards(columns, self.nrow, f'({nchan},{npol},{nsblk * self.nbits // 8})',
                                            '(NCHAN,NPOL,NSBLK*NBITS/8)', pol_type, self._dims, width, self._tbin,
                                            self.nbits, nsblk)
        sub += [card('SIGNINT', 0, '1 for signed ints in SEARCH-mode data, else 0'),
                card('NSTOT', shape[0], 'Total number of samples (SEARCH mode, else 1)')]
        head += header_block(sub)
        self._data_at = len(head)
        self._eof = self._data_at + -(-self.nrow * self.row_bytes // BLOCK) * BLOCK
        self._tsubint = nsblk * self._tbin
        self._offs0 = offs_rest
        self._freq = np.asarray(freq_mhz, dtype='>f8').tobytes()
        self._fh = builtins_open(name, 'wb')
        self._fh.write(head)
        self.offset = 0
        self.closed = False

    def _encode(self, data):
        if isinstance(data, hip.DeviceArray) and data.dtype == self.dtype:
            return [a.to_host() for a in hip.psrsearch_encode(data, self.nsblk, self.nbits, self.nsigma)]
        if hasattr(data, 'to_host'):
            data = data.to_host()
        return encode_search_rows(data, self.nsblk, self.nbits, self.nsigma)

    def write(self, data):
        if self.closed:
            raise ValueError("I/O operation on closed stream.")
        if not hasattr(data, 'to_host'):
            data = np.asarray(data)
        assert tuple(data.shape[1:]) == self.sample_shape, f"'data' must have trailing shape {self.sample_shape}"
        n = data.shape[0]
        if self.offset + n > self.shape[0]:
            raise EOFError("cannot write beyond the length given in the header.")
        if n % self.granule:
            raise ValueError(f"a piece of {n} samples does not end on a row: every piece must hold a multiple "
                             f"of the granule, nsblk = {self.granule} samples.")
        if n == 0:
            return
        codes, scl, offs, n_finite = self._encode(data)
        wts = (n_finite.sum(axis=1) > 0).astype('>f4')                  # (row, chan)
        scl, offs = scl.astype('>f4'), offs.astype('>f4')
        first = self.offset // self.nsblk
        for k in range(n // self.nsblk):
            sub = self._offs0 + (first + k + 0.5) * self._tsubint
            self._fh.write(np.array([self._tsubint, sub], '>f8').tobytes() + self._freq + wts[k].tobytes()
                           + offs[k].tobytes() + scl[k].tobytes())
            self._fh.write(codes[k].data)
        self.offset += n


class PSRFITSSearchReader(DeviceTaskMixin, Base):
    """The ``SUBINT`` table of a PSRFITS search-mode file as a device stream of shape ``(nrow *
    nsblk, nchan, npol)``, float32, with ``sample_rate = 1 / TBIN`` and one row a frame.  A read
    uploads the stored bytes of a run of rows as they are, with their scales, offsets and weights,
    and decodes them in HBM (`hip.psrsearch_decode`).

    ``weighted``: multiply by ``DAT_WTS`` (default True).  ``primary`` and ``header`` are the
    cards of the primary and the ``SUBINT`` HDU, as mappings.  Unsigned codes of 1, 2, 4 or 8 bits
    are read (``SIGNINT`` must be 0 or absent)."""

    def __init__(self, name, weighted=True):
        raw, self.hdus, primary, hdu, mode = _open_subint(name)
        if mode != 'SEARCH':
            raise ValueError(f"{name}: '{mode}' is not search mode ('SEARCH'); psrfits.open reads fold mode.")
        header = hdu.header
        self.primary, self.header, self.weighted = primary, header, bool(weighted)
        nrow = int(header['NAXIS2'])
        nsblk, nchan, npol, nbits = (int(header[key]) for key in ('NSBLK', 'NCHAN', 'NPOL', 'NBITS'))
        if nbits not in SEARCH_NSIGMA or _number(header.get('SIGNINT'), 0.) != 0.:
            raise OSError(f"{name}: unsigned codes of 1, 2, 4 or 8 bits are read, not NBITS = {nbits}, "
                          f"SIGNINT = {header.get('SIGNINT')}.")
        dtype = table_dtype(header)
        if hdu.data_offset + nrow * dtype.itemsize > raw.shape[0]:
            raise OSError(f"{name}: the SUBINT table needs {hdu.data_offset + nrow * dtype.itemsize} bytes, "
                          f"the file has {raw.shape[0]} (truncated).")
        rows = np.ndarray((nrow,), dtype, buffer=raw, offset=hdu.data_offset)
        for column in ('TSUBINT', 'DAT_SCL', 'DAT_OFFS', 'DATA'):
            if column not in dtype.names:
                raise OSError(f"{name}: the SUBINT table has no {column} column.")
        if (nchan * nbits % 8 or dtype['DATA'].base != np.dtype('u1')
                or dtype['DATA'].shape != (nsblk * npol * nchan * nbits // 8,)
                or dtype['DAT_SCL'].shape != (nchan * npol,) or dtype['DAT_OFFS'].shape != (nchan * npol,)):
            raise OSError(f"{name}: DATA, DAT_SCL or DAT_OFFS do not match NSBLK, NCHAN, NPOL, NBITS = {nsblk}, "
                          f"{nchan}, {npol}, {nbits}.")
        self._rows, self._raw = rows, raw
        self._dims, self.nbits = (nsblk, nchan, npol), nbits
        self._has_wts = 'DAT_WTS' in dtype.names and dtype['DAT_WTS'].shape == (nchan,)
        self.zero_off = _number(header.get('ZERO_OFF'), 0.)
        tbin = _number(header.get('TBIN'))
        if not tbin or not tbin > 0:
            raise OSError(f"{name}: TBIN = {header.get('TBIN')} does not give the sample rate.")
        extra = 0.
        if 'OFFS_SUB' in dtype.names and nrow:
            # (the first row's centre less half a row of nsblk * TBIN: TSUBINT is not trusted with it)
            extra = float(rows['OFFS_SUB'][0, 0]) - nsblk * tbin / 2.
        start = _from_stt(primary['STT_IMJD'], primary['STT_SMJD'], _number(primary.get('STT_OFFS'), 0.), extra)
        meta = _subint_meta(name, header, rows, nchan, npol)
        Base.__init__(self, shape=(nrow * nsblk, nchan, npol), start_time=start, sample_rate=1. / tbin,
                      samples_per_frame=nsblk, dtype=np.float32, **meta)

    def _compute_frames(self, first, last, out):
        nsblk, nchan, npol = self._dims
        rows = self._rows[first:last]
        n = last - first
        codes = hip.DeviceArray.from_host(np.ascontiguousarray(rows['DATA']))
        scl = hip.DeviceArray.from_host(rows['DAT_SCL'].astype(np.float32).reshape(n, npol, nchan))
        offs = hip.DeviceArray.from_host(rows['DAT_OFFS'].astype(np.float32).reshape(n, npol, nchan))
        wts = None
        if self.weighted and self._has_wts:
            wts = hip.DeviceArray.from_host(rows['DAT_WTS'].astype(np.float32).reshape(n, nchan))
        hip.psrsearch_decode(codes, scl, offs, wts, self.zero_off, self.nbits, self._dims, out=out)

    def close(self):
        Base.close(self)
        self._drop_cache()
        self._rows = self._raw = None


def open_search(name, mode='r', **kwargs):
    """Open a PSRFITS search-mode file as a stream: ``mode='r'`` (with ``weighted=True``) gives a
    `PSRFITSSearchReader`; ``mode='w'`` with ``template=`` (and / or the keywords of
    `PSRFITSSearchWriter`: ``nbits, nsblk, nsigma, shape, start_time, ...``) gives a
    `PSRFITSSearchWriter`."""
    if mode == 'w':
        return PSRFITSSearchWriter(name, **kwargs)
    if mode == 'r':
        if set(kwargs) - {'weighted'}:
            raise TypeError("no keywords for reading but weighted.")
        return PSRFITSSearchReader(name, **kwargs)
    raise ValueError(f"Unknown mode '{mode}'. Currently only modes 'r' and 'w' are supported.")
