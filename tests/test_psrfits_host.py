"""`bt.psrfits` without a GPU: the FITS layer on the reference's real archive (tests/golden/
B1855+09.430.PUPPI.11y.x.sum.sm, with psrchive's read-out of it in B1855_nano.npz: the data of the
reference's own test_psrfits_read.py), the NumPy coding `encode_rows` / `decode_rows` that the
kernels are held to, the bytes of a file written from host pieces, found with a card walker of
this test's own, the tiling of the kernels (csrc/psrfits_geo.hpp) walked on the host by a stand-alone
program under sanitizers, and the ledger of which instantiations and edges of that tiling the GPU
cases of tests/psrfits_cases.py reach."""
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import psrfits
from baseband_tasks_amd import units as u
import psrfits_cases as pc
from geo_check import compile_check, run_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCHIVE = os.path.join(ROOT, 'tests', 'golden', 'B1855+09.430.PUPPI.11y.x.sum.sm')
READ_OUT = os.path.join(ROOT, 'tests', 'golden', 'B1855_nano.npz')
F32 = np.float32


def mjd(time):
    return (time.sec / 86400 + 40587) + time.frac / 86400.


# -- the fixture ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def archive():
    raw = np.fromfile(ARCHIVE, np.uint8)
    hdus = psrfits.read_hdus(raw)
    sub = [h for h in hdus if h.name == 'SUBINT'][0]
    rows = np.ndarray((int(sub.header['NAXIS2']),), psrfits.table_dtype(sub.header), buffer=raw,
                      offset=sub.data_offset)
    return hdus, sub, rows, np.load(READ_OUT)


def test_fits_layer_finds_the_extensions(archive):
    hdus, sub, rows, _ = archive
    assert [h.name for h in hdus] == ['PRIMARY', 'HISTORY', 'PSRPARAM', 'POLYCO', 'SUBINT']
    assert len(hdus) - 1 == 4
    assert hdus[-1] is sub and sub.data_size == 4216 and sub.header['TFORM20'] == '2048I'
    assert sub.data_offset + 2880 * 2 == os.path.getsize(ARCHIVE)
    p = hdus[0].header
    assert p['SIMPLE'] is True and p['OBSNCHAN'] == 64 and p['TELESCOP'] == 'Arecibo'
    assert p['STT_OFFS'] == 6.3664629124105e-11 and p['SCANLEN'] == '*' and p['FD_HAND'] == -1
    assert p.comments['OBSBW'] == '[MHz] Bandwidth for observation'
    assert rows.dtype.names[-1] == 'DATA' and rows['DATA'].shape == (1, 2048)


def test_decode_rows_is_psrchives_read_out(archive):
    _, _, rows, want = archive
    got = psrfits.decode_rows(rows['DATA'].reshape(1, 1, 1, 2048), rows['DAT_SCL'], rows['DAT_OFFS'])
    assert got.dtype == np.float32 and got.shape == (1, 2048, 1, 1)
    assert np.all(got == want['data'].reshape(1, 2048, 1, 1))


def test_reader_metadata(archive):
    """(No read: the profiles are decoded on the GPU; tests/test_psrfits_gpu.py.)"""
    want = archive[3]
    with psrfits.open(ARCHIVE) as fh:
        assert fh.shape == (1, 2048, 1, 1) and fh.sample_shape == (2048, 1, 1)
        assert fh.samples_per_frame == 1 and fh.dtype == np.float32 and fh.weighted
        assert np.isclose(fh.frequency / u.MHz, 433.12399292, rtol=1e-11, atol=0).all()
        # ((nchan, 1) as given; `Base` drops the axes along which a value does not change)
        assert np.broadcast_to(fh.frequency, fh.sample_shape).shape == (2048, 1, 1) and np.all(fh.sideband == 1)
        assert fh.primary['OBSNCHAN'] == 64 and fh.primary['TELESCOP'] == 'Arecibo'
        assert fh.header['NBIN'] == 2048 and fh.header['EXTNAME'] == 'SUBINT'
        assert list(fh.polarization.ravel()) == ['INTEN']
        assert np.isclose(mjd(fh.start_time), want['t'][0])
        # 56374 d 41930 s + 6.4e-11 s + OFFS_SUB - TSUBINT / 2
        assert abs((fh.start_time - bt.Time('2013-03-23T11:38:50')) - (1498.95940172 - 3004.287 / 2)) < 1e-6
        assert np.isclose(fh.sample_rate, 1 / 3004.287, rtol=1e-7)
        assert fh.zero_off == 0.
    assert fh.closed


# -- the coding --------------------------------------------------------------------------
def profiles(shape, seed=5):
    """Seeded normal profiles (row, bin, chan, pol) with, where there is room, a column with NaN
    and inf bins, a constant column and a channel that is all NaN."""
    rng = np.random.default_rng(seed)
    x = (3. * rng.standard_normal(shape) + 7.).astype(F32)
    n_row, n_bin, n_chan, n_pol = shape
    if n_bin > 2:
        x[0, 1, 0, 0] = np.nan
        x[0, n_bin - 1, 0, 0] = np.inf
        x[0, 2, 0, 0] = -np.inf
    if n_chan > 1:
        x[-1, :, 1, n_pol - 1] = 2.5
    if n_chan > 2:
        x[0, :, 2, :] = np.nan
    return x


def test_extremes_get_the_end_codes():
    ramp = np.linspace(-3., 1e4, 257).astype(F32)
    rng = np.random.default_rng(1)
    x = np.stack([ramp, rng.permutation(ramp), 1e-3 * rng.standard_normal(257).astype(F32)], axis=1)[None]
    codes, scl, offs, n_finite = psrfits.encode_rows(x.reshape(1, 257, 3, 1))
    assert codes.dtype == np.dtype('>i2') and codes.shape == (1, 1, 3, 257)
    assert scl.dtype == offs.dtype == np.float32 and n_finite.dtype == np.int32 and np.all(n_finite == 257)
    for c in range(3):
        col = x[0, :, c]
        assert codes[0, 0, c, np.argmax(col)] == 32767 and codes[0, 0, c, np.argmin(col)] == -32767
        assert np.abs(codes[0, 0, c]).max() == 32767
    assert offs[0, 0, 0] == F32(0.5) * F32(-3.) + F32(0.5) * F32(1e4)
    assert scl[0, 0, 0] == (F32(0.5) * F32(1e4) - F32(0.5) * F32(-3.)) / F32(32767.)


@pytest.mark.parametrize('shape', [(1, 257, 3, 1), (2, 64, 5, 2), (1, 2048, 1, 1)])
def test_round_trip_is_within_half_a_step(shape):
    """|decode(encode(x)) - x| <= 0.51 scl + 4 * 2^-23 max|x| per column: half a code step, under
    0.006 of a step from the two float32 roundings of (x - offs) / scl at magnitude 32767, and the
    decoder's two roundings (product and sum, each below 2^-24 of a magnitude <= 2 max|x|)."""
    x = profiles(shape)
    x[0, :, 0, 0] = np.linspace(-3., 1e4, shape[1]).astype(F32)
    codes, scl, offs, n_finite = psrfits.encode_rows(x)
    back = psrfits.decode_rows(codes, scl, offs)
    assert back.shape == x.shape
    finite = np.isfinite(x)
    top = np.where(finite, np.abs(x), 0).max(axis=1)                       # (row, chan, pol)
    bound = 0.51 * scl.transpose(0, 2, 1).astype(np.float64) + 4 * 2. ** -23 * top
    err = np.where(finite, np.abs(back.astype(np.float64) - np.where(finite, x, 0)), 0).max(axis=1)
    assert np.all(err <= bound), (err / bound).max()
    assert np.all(n_finite.transpose(0, 2, 1) == finite.sum(axis=1))


def test_constant_nan_and_empty_columns():
    x = profiles((2, 33, 4, 2))
    codes, scl, offs, n_finite = psrfits.encode_rows(x)
    # a constant column: scale 1, codes 0, exact
    assert scl[1, 1, 1] == 1. and offs[1, 1, 1] == 2.5 and np.all(codes[1, 1, 1] == 0)
    assert np.all(psrfits.decode_rows(codes, scl, offs)[1, :, 1, 1] == 2.5)
    # bins that are not finite: left out of scale and offset, coded 0, counted out
    clean = x.copy()
    clean[0, (1, 2, 32), 0, 0] = clean[0, 5, 0, 0]
    c2, s2, o2, n2 = psrfits.encode_rows(clean)
    assert scl[0, 0, 0] == s2[0, 0, 0] and offs[0, 0, 0] == o2[0, 0, 0]
    assert np.all(codes[0, 0, 0, [1, 2, 32]] == 0) and n_finite[0, 0, 0] == 30 and n2[0, 0, 0] == 33
    keep = np.setdiff1d(np.arange(33), [1, 2, 32])
    assert np.array_equal(codes[0, 0, 0, keep], c2[0, 0, 0, keep])
    # nothing finite: offs 0, scl 1, codes 0
    assert np.all(n_finite[0, :, 2] == 0) and np.all(scl[0, :, 2] == 1.) and np.all(offs[0, :, 2] == 0.)
    assert np.all(codes[0, :, 2] == 0)
    # underflow of the scale: a column whose spread is below 32767 denormal steps
    tiny = np.zeros((1, 4, 1, 1), F32)
    tiny[0, 1] = 1e-45
    c, s, o, _ = psrfits.encode_rows(tiny)
    assert s[0, 0, 0] == 1. and np.all(c == 0)
    # weights and ZERO_OFF in the decoder
    w = np.array([[1., 0., 2., 1.], [1., 1., 1., .5]], F32)
    plain = psrfits.decode_rows(codes, scl, offs)
    assert np.array_equal(psrfits.decode_rows(codes, scl, offs, w), plain * w[:, None, :, None], equal_nan=True)
    shifted = psrfits.decode_rows(codes, scl, offs, zero_off=0.5)
    want = (codes.astype(F32) - F32(0.5)) * scl[..., None] + offs[..., None]
    assert np.array_equal(shifted, want.transpose(0, 3, 2, 1))


# -- a written file, read by a walker of this test's own --------------------------------------
WIDTHS = {'A': 1, 'B': 1, 'I': 2, 'J': 4, 'E': 4, 'D': 8}


def walk(raw):
    """[(cards, data offset)] of a FITS file: keyword -> value text (quotes and comment removed)."""
    out, pos = [], 0
    while pos < len(raw):
        cards, end = {}, False
        while not end:
            block = raw[pos:pos + 2880].decode('ascii')
            assert len(block) == 2880
            pos += 2880
            for i in range(0, 2880, 80):
                line = block[i:i + 80]
                if line.startswith('END' + ' ' * 77):
                    end = True
                    break
                if line[8:10] == '= ':
                    value = line[10:]
                    if value.lstrip().startswith("'"):
                        value = value.lstrip()[1:].split("'")[0]
                    else:
                        value = value.split('/')[0]
                    cards[line[:8].strip()] = value.strip()
        out.append((cards, pos))
        size = 0
        if int(cards['NAXIS']):
            size = int(cards['NAXIS1']) * int(cards['NAXIS2']) + int(cards.get('PCOUNT', 0))
        pos += -(-size // 2880) * 2880
    return out


class Template:
    """What a writer needs of a stream."""
    shape = (3, 5, 3, 2)
    dtype = np.dtype(np.float32)
    start_time = bt.Time('2021-03-04T05:06:07') + 0.123456789012
    sample_rate = 1. / 7.5
    frequency = np.array([400., 401.5, 403.])[:, None] * u.MHz
    sideband = np.int8(-1)
    polarization = np.array(['LL', 'RR'])


@pytest.fixture(scope='module')
def written(tmp_path_factory):
    name = str(tmp_path_factory.mktemp('psrfits') / 'host.fits')
    x = profiles(Template.shape, seed=9)
    with psrfits.open(name, 'w', template=Template, primary={'TELESCOP': 'GBT', 'SRC_NAME': ('B0000+00', 'Source'),
                                                           'ANT_X': 882589.65}) as fw:
        assert fw.accepts_device and fw.shape == Template.shape and fw.tell() == 0
        fw.write(x[:1])
        fw[1:3] = x[1:]
        assert fw.tell() == 3
        with pytest.raises(EOFError):
            fw.write(x[:1])
    return name, x


def test_written_file_layout(written):
    name, x = written
    raw = np.fromfile(name, np.uint8).tobytes()
    assert len(raw) % 2880 == 0
    (primary, _), (sub, at) = walk(raw)
    assert primary['SIMPLE'] == 'T' and primary['BITPIX'] == '8' and primary['NAXIS'] == '0' and primary['EXTEND'] == 'T'
    assert primary['FITSTYPE'] == 'PSRFITS' and primary['OBS_MODE'] == 'PSR' and 'HDRVER' in primary
    assert primary['TELESCOP'] == 'GBT' and primary['SRC_NAME'] == 'B0000+00' and float(primary['ANT_X']) == 882589.65
    # reference hdu.py:154-166: channel 0 padded below, centre channel (3 + 1) // 2 of the padded band
    assert float(primary['OBSFREQ']) == 401.5 and float(primary['OBSBW']) == -4.5 and primary['OBSNCHAN'] == '3'
    assert primary['DATE-OBS'].startswith('2021-03-04T05:06:07.123')
    assert sub['XTENSION'] == 'BINTABLE' and sub['EXTNAME'] == 'SUBINT' and sub['NAXIS'] == '2'
    assert sub['INT_TYPE'] == 'TIME' and sub['INT_UNIT'] == 'SEC' and sub['POL_TYPE'] == 'LLRR'
    assert (sub['NPOL'], sub['NBIN'], sub['NCHAN'], sub['NBITS'], sub['NSBLK']) == ('2', '5', '3', '1', '1')
    assert float(sub['ZERO_OFF']) == 0. and float(sub['CHAN_BW']) == -1.5 and 'TBIN' in sub
    n_field = int(sub['TFIELDS'])
    names = [sub[f'TTYPE{k}'] for k in range(1, n_field + 1)]
    assert names == ['TSUBINT', 'OFFS_SUB', 'DAT_FREQ', 'DAT_WTS', 'DAT_OFFS', 'DAT_SCL', 'DATA']
    forms = [sub[f'TFORM{k}'] for k in range(1, n_field + 1)]
    assert forms == ['1D', '1D', '3D', '3E', '6E', '6E', '30I']
    widths = [int(f[:-1]) * WIDTHS[f[-1]] for f in forms]
    assert int(sub['NAXIS1']) == sum(widths) and int(sub['NAXIS2']) == 3
    assert sub['TDIM7'] == '(5,3,2)'
    assert len(raw) == at + 2880 * -(-3 * sum(widths) // 2880)
    codes, scl, offs, n_finite = psrfits.encode_rows(x)
    starts = np.concatenate([[0], np.cumsum(widths)])
    stt = (int(primary['STT_IMJD']) - 40587) * 86400 + int(primary['STT_SMJD'])
    for k in range(3):
        row = raw[at + k * sum(widths):at + (k + 1) * sum(widths)]
        field = lambda i, dtype: np.frombuffer(row[starts[i]:starts[i + 1]], dtype)
        assert field(6, '>i2').tobytes() == codes[k].astype('>i2').tobytes()        # (pol, chan, bin)
        assert np.array_equal(field(5, '>f4'), scl[k].ravel()) and np.array_equal(field(4, '>f4'), offs[k].ravel())
        assert np.array_equal(field(2, '>f8'), [400., 401.5, 403.])
        assert np.array_equal(field(3, '>f4'), (n_finite[k].sum(0) > 0).astype(F32))
        tsubint, offs_sub = field(0, '>f8')[0], field(1, '>f8')[0]
        assert tsubint == 7.5
        # the row's centre, less half a row, less k rows, is the start: within 1e-9 s (a double
        # OFFS_SUB below a day resolves 1.5e-11 s)
        start = bt.Time(stt, float(primary['STT_OFFS'])) + (offs_sub - (k + 0.5) * tsubint)
        assert abs(start - Template.start_time) < 1e-9
    assert np.all(np.frombuffer(raw[at + 3 * sum(widths):], np.uint8) == 0)
    # the all-NaN channel of row 0 has weight 0, every other weight is 1
    wts = np.frombuffer(raw[at + starts[3]:at + starts[4]], '>f4')
    assert list(wts) == [1., 1., 0.]


def test_written_file_reopens(written):
    name, x = written
    with psrfits.open(name) as fh:
        assert fh.shape == Template.shape and fh.sample_rate == 1 / 7.5
        assert abs(fh.start_time - Template.start_time) < 1e-9
        assert fh.frequency.shape == (3, 1) and np.array_equal(fh.frequency, Template.frequency)
        assert np.all(fh.sideband == -1)
        assert list(fh.polarization.ravel()) == ['LL', 'RR']
        assert fh.primary['TELESCOP'] == 'GBT' and fh.header['TDIM7'] == '(5,3,2)'


def test_short_file_keeps_its_size_and_fewer_axes(tmp_path):
    name = str(tmp_path / 'short.fits')
    with psrfits.open(name, 'w', shape=(4, 6), start_time='2020-01-01T00:00:00', sample_rate=2.) as fw:
        fw.write(np.arange(6, dtype=F32)[None])
    raw = np.fromfile(name, np.uint8).tobytes()
    (_, _), (sub, at) = walk(raw)
    assert len(raw) == at + 2880 and int(sub['NAXIS1']) * 4 <= 2880 and sub['TDIM7'] == '(6,1,1)'
    assert sub['POL_TYPE'] == 'INTEN' and sub['CHAN_BW'] == '*'
    with psrfits.open(name) as fh:
        assert fh.shape == (4, 6, 1, 1)
        with pytest.raises(AttributeError):
            fh.frequency


# -- errors ------------------------------------------------------------------------------------
def test_writer_refuses_what_it_cannot_store(tmp_path):
    name = str(tmp_path / 'no.fits')
    keys = dict(start_time='2020-01-01T00:00:00', sample_rate=1.)
    with pytest.raises(TypeError, match='complex'):
        psrfits.open(name, 'w', shape=(2, 8, 2), dtype=np.complex64, **keys)
    counted = np.dtype([('data', np.float32), ('count', int)])          # (what average=False makes)
    with pytest.raises(TypeError, match='average'):
        psrfits.open(name, 'w', shape=(2, 8, 2), dtype=counted, **keys)
    with pytest.raises(TypeError, match='float32'):
        psrfits.open(name, 'w', shape=(2, 8, 2), dtype=np.float64, **keys)
    with pytest.raises(ValueError, match='shape'):
        psrfits.open(name, 'w', shape=(2,), **keys)
    with pytest.raises(ValueError, match='chan_bw'):
        psrfits.open(name, 'w', shape=(2, 8), frequency=400 * u.MHz, sideband=1, **keys)
    with pytest.raises(ValueError, match='own'):
        psrfits.open(name, 'w', shape=(2, 8), primary={'OBS_MODE': 'SEARCH'}, **keys)
    with pytest.raises(ValueError, match='mode'):
        psrfits.open(name, 'a')
    with pytest.raises(TypeError):
        psrfits.open(ARCHIVE, 'r', verify=True)
    assert not os.path.exists(name)


def test_reader_refuses_two_subints_and_search_mode(written, tmp_path):
    name, _ = written
    raw = np.fromfile(name, np.uint8).tobytes()
    (_, at0), (_, at) = walk(raw)
    twice = str(tmp_path / 'twice.fits')
    with open(twice, 'wb') as f:
        f.write(raw + raw[at0:])
    with pytest.raises(RuntimeError, match='SUBINT'):
        psrfits.open(twice)
    search = str(tmp_path / 'search.fits')
    old = psrfits.card('OBS_MODE', 'PSR', '(PSR, CAL, SEARCH)').encode()
    assert raw.count(old) == 1
    with open(search, 'wb') as f:
        f.write(raw.replace(old, psrfits.card('OBS_MODE', 'SEARCH', '(PSR, CAL, SEARCH)').encode()))
    with pytest.raises(ValueError, match='SEARCH'):
        psrfits.open(search)
    with open(search, 'wb') as f:
        f.write(raw[:at0])
    with pytest.raises(RuntimeError, match='0 SUBINT'):
        psrfits.open(search)
    with pytest.raises(OSError, match='FITS'):
        psrfits.open(READ_OUT)


# -- the kernels' tiling, on the host ------------------------------------------------------------
@pytest.fixture(scope='module')
def geo_check(tmp_path_factory):
    return compile_check('psrfits_geo_check', tmp_path_factory.mktemp('psrfits_geo'))


def geo_shape(run):
    _, (_, n_bin, n_chan, n_pol), x_aligned, codes_aligned = run
    return n_bin, n_chan, n_pol, x_aligned, codes_aligned


def test_kernel_tiling_on_the_host(geo_check):
    """Every LDS index inside its array, the tree reading written cells only, every float and every
    code touched once a pass, no vector access across the end of a row or off its alignment: the
    program exits non-zero otherwise, and the sanitizers abort it on a wild index of its own.  On
    what the GPU tests launch, and on a sweep over the edges of both tilings: every column count
    to 70 with the bin counts around 1, a bin tile of the wide kernels (128), two, and one of the
    narrow kernels (1024); every bin count to 260 and from 1020 to 1030 with the column counts
    around a thread's four, a tile (32) and two."""
    shapes = [geo_shape(run) for run in pc.fold_runs()]
    edge_bins = [b for b in range(1, 1031) if min(abs(b - e) for e in (1, 128, 256, 1024)) <= 3]
    edge_cols = [c for c in range(1, 71) if min(abs(c - e) for e in (4, 32, 64)) <= 3]
    for bins in list(range(1, 261)) + list(range(1020, 1031)):
        for cols in range(1, 71):
            if bins not in edge_bins and cols not in edge_cols:
                continue
            n_pol = next(p for p in (4, 3, 2, 1) if cols % p == 0)
            shapes.append((bins, cols // n_pol, n_pol, 1, 1))
            if bins % 2 == 0 and cols % 4 == 0:              # (else the aligned run is scalar already)
                shapes += [(bins, cols // n_pol, n_pol, 0, 1), (bins, cols // n_pol, n_pol, 1, 0)]
    plans = run_check(geo_check, shapes, through_stdin=True)
    for (n_bin, n_chan, n_pol, x_aligned, codes_aligned), g in zip(shapes, plans):
        assert g['walk'] == 0, (n_bin, n_chan, n_pol, x_aligned, codes_aligned, g)
        assert g['tc'] == (32 if n_chan * n_pol >= 32 else 4) and g['n_tile'] == -(-n_chan * n_pol // g['tc'])
        assert g['vec'] == int(x_aligned and codes_aligned and n_chan * n_pol % 4 == 0 and n_bin % 2 == 0)
        assert g['tb'] * g['tc'] == 4096 and g['nx'] * g['ny'] == 256 and g['nx'] * (4 if g['vec'] else 1) == g['tc']
        assert g['enc_pitch'] == g['tb'] // 2 + 1 and g['dec_pitch'] == g['tb'] + 1
    assert plans[4] == {'tc': 32, 'vec': 1, 'n_tile': 64, 'tb': 128, 'nx': 8, 'ny': 32, 'enc_pitch': 65,
                        'dec_pitch': 129, 'walk': 0}
    # what the library refuses, given as arguments
    errors = run_check(geo_check, [(0, 1, 1, 1, 1), (4, 1 << 16, 1 << 16, 1, 1)])
    assert 'empty' in errors[0]['error'] and '2^31' in errors[1]['error']


# -- which paths of the kernels the GPU cases take -------------------------------------------------
@pytest.fixture(scope='module')
def geo(geo_check):
    """(bins, chan, pol, floats aligned, codes aligned) -> the launcher's geometry, for every GPU run
    and its aligned twin."""
    shapes = sorted({s for run in pc.fold_runs() for s in (geo_shape(run), geo_shape(run)[:3] + (1, 1))})
    plans = dict(zip(shapes, run_check(geo_check, shapes)))
    assert all(g['walk'] == 0 for g in plans.values())
    return plans.__getitem__


def test_gpu_cases_take_every_path(geo):
    """The ledger: every (tc, vec) instantiation, ragged last column tiles of the wide kernels with
    float4 and with scalar accesses, and 1, 2, odd, fewer than a tile's, a multiple of a tile's and
    more than a tile's bins, the even ones with vector accesses."""
    took = pc.fold_ledger(pc.fold_runs(), geo)
    for path, names in took.items():
        print(f'{path}: {", ".join(names)}')
    assert pc.uncovered(took) == []


def test_every_new_gpu_case_is_needed(geo):
    """Without any one of the cases added for the ledger, a path is left uncovered."""
    for shape in pc.FOLD_NEW:
        rest = pc.fold_runs([s for s in pc.FOLD_SHAPES if s != shape])
        assert pc.uncovered(pc.fold_ledger(rest, geo)), shape
    assert pc.uncovered(pc.fold_ledger(pc.fold_runs(shifted_codes=False), geo))
