"""Shared cases of the block median / MAD tests (test_rank_host.py proves the twins, test_rank_gpu.py
holds the kernels to them bit for bit): noise blocks at and around every power of two the tilings cut
at, planted columns whose outcome the rule states, whitening spectra with ragged last blocks, the
routes, digits and tile widths, and the shapes the geometry check walks."""
import functools

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import periodicity, search

from dmt_cases import same_bits  # noqa: F401  (shared helper)

T0 = '2010-11-12T13:14:15'
RATE = 10.

#: blocks of the noise plane: the smallest, odd and even, around 32 / 64 / 256 (a row of threads, a tile's
#: rows), and one of many rounds
NOISE_SHAPE = (2100, 67)
BLOCKS = (2, 3, 31, 32, 33, 64, 255, 256, 257, 1000)
#: blocks of the planted plane: even and odd
PLANT_BLOCKS = (8, 9)
(CONST, ZERO, MINUS_ZERO, MED_PLUS_ZERO, MED_MINUS_ZERO, NAN, INF, MOST_EQUAL, HALF_EQUAL, INTS, LAST_BIT, DENORMAL,
 HUGE) = range(13)
PLANT_COLUMNS = 17
HUGE_BITS = 0x7f7fffff

#: every way to run one rule: (BBT_RANK_ROUTE, BBT_RANK_DIGIT, BBT_RANK_WIDTH)
TILINGS = [(route, digit, width) for route in ('lds', 'global') for digit in (4, 8) for width in (16, 32, 64)]


def set_tiling(monkeypatch, route, digit=None, width=None):
    monkeypatch.setenv('BBT_RANK_ROUTE', route)
    for name, value in (('BBT_RANK_DIGIT', digit), ('BBT_RANK_WIDTH', width)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


@functools.lru_cache(maxsize=None)
def noise():
    """(2100, 67) float32 normal noise of mean 5 and deviation 3, read-only."""
    x = np.random.default_rng(41).normal(5., 3., NOISE_SHAPE).astype(np.float32)
    x.setflags(write=False)
    return x


def _spread(rng, parts):
    """The values of ``parts`` in one shuffled float32 column."""
    col = np.concatenate([np.asarray(p, np.float32).ravel() for p in parts])
    return col[rng.permutation(col.shape[0])]


@functools.lru_cache(maxsize=None)
def planted(n):
    """(3 n + 1, 17) float32: three blocks of ``n`` (and a tail that is dropped), the columns named above
    planted block by block, the others noise.  Read-only."""
    rng = np.random.default_rng(100 + n)
    x = rng.normal(5., 3., (3 * n + 1, PLANT_COLUMNS)).astype(np.float32)
    odd = n & 1
    for b in range(3):
        rows = slice(b * n, (b + 1) * n)
        pos = np.arange(1, n + 1, dtype=np.float32) + np.float32(0.25 * b)
        x[rows, CONST] = 2.5
        x[rows, ZERO] = 0.
        x[rows, MINUS_ZERO] = -0.
        a = (n - 1) // 2 - 1                                   # ranks a + 1 and a + 2 hold +0: lo and hi
        x[rows, MED_PLUS_ZERO] = _spread(rng, [-pos[:a], [-0.], [0., 0.], pos[:n - a - 3]])
        a = (n - 1) // 2 - odd                                 # ranks a and a + 1 hold -0: lo and hi
        x[rows, MED_MINUS_ZERO] = _spread(rng, [-pos[:a], [-0., -0.], [0.], pos[:n - a - 3]])
        x[rows, MOST_EQUAL] = _spread(rng, [np.full(n // 2 + 1, 7.), 7. + pos[:n - n // 2 - 1]])
        x[rows, HALF_EQUAL] = _spread(rng, [np.full(n // 2, 7.), 9. + pos[:n - n // 2]])
        x[rows, INTS] = rng.integers(-4, 5, n).astype(np.float32)
        x[rows, LAST_BIT] = (np.float32(1.).view(np.uint32) + rng.integers(0, 4, n).astype(np.uint32)).view(np.float32)
        tiny = (rng.integers(1, 100, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
        x[rows, DENORMAL] = np.where(rng.random(n) < 0.4, -pos, tiny)
        huge = np.full(n - (n - 1) // 2, HUGE_BITS, np.uint32).view(np.float32)
        x[rows, HUGE] = _spread(rng, [pos[:(n - 1) // 2], huge])
    x[n + 2, NAN] = np.nan
    x[1, INF] = -np.inf
    x[2 * n + 3, INF] = np.inf
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def pulse_plane():
    """(1024, 67) standard-normal float32 from default_rng(5) with 50 added to samples 400 ... 463, and the
    plane without the pulse."""
    clean = np.random.default_rng(5).standard_normal((1024, 67)).astype(np.float32)
    x = clean.copy()
    x[400:464] += np.float32(50.)
    x.setflags(write=False)
    clean.setflags(write=False)
    return x, clean


# -- whitening ------------------------------------------------------------------------------------------------
WH_SHAPE = (3, 1501, 7)
#: (m, skip): a ragged last block behind skip 0, 1 and 7, and a last block of a single bin (1501 = 25 * 60 + 1)
WH_CUTS = ((61, 0), (61, 1), (61, 7), (60, 0))
WH_ZERO, WH_NAN, WH_INF = 0, 1, 2
WH_RATIO = periodicity.median_ratio(4)


@functools.lru_cache(maxsize=None)
def wh_data():
    """(3, 1501, 7) float32 exponential noise of mean 4: column 0 all zero, column 1 a NaN at bin 707 of
    spectrum 1, column 2 an Inf at bin 1500 (the last) of spectrum 2.  Read-only."""
    x = (4. * np.random.default_rng(78).standard_exponential(WH_SHAPE)).astype(np.float32)
    x[:, :, WH_ZERO] = 0.
    x[1, 707, WH_NAN] = np.nan
    x[2, 1500, WH_INF] = np.inf
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def wh_expected(m, skip, ratio=WH_RATIO):
    out = periodicity.median_whiten_samples(wh_data(), m, skip, ratio)
    out.setflags(write=False)
    return out


def spectra_stats(x, m, skip):
    """The twin of `hip.rank_stats` on spectra ``(N, nbin) + s``: ``(med, mad)``, each ``(N, ceil((nbin - skip) / m))
    + s``, NaN where flagged -- block by block through `search.block_median_mad_samples`."""
    nbin = x.shape[1]
    meds, mads = [], []
    for j0 in range(skip, nbin, m):
        block = x[:, j0:min(j0 + m, nbin)]
        if block.shape[1] == 1:                               # (a lone bin is its own median, its MAD is 0)
            flagged = ~np.isfinite(block[:, 0])
            med = np.where(flagged, np.float32(np.nan), block[:, 0])
            mad = np.where(flagged, np.float32(np.nan), np.float32(0.))
        else:
            med, mad = search.block_median_mad_samples(np.moveaxis(block, 1, 0).reshape((block.shape[1], -1)),
                                                       block.shape[1])
            med, mad = med.reshape(block[:, 0].shape), mad.reshape(block[:, 0].shape)
        meds.append(med)
        mads.append(mad)
    return np.stack(meds, axis=1).astype(np.float32), np.stack(mads, axis=1).astype(np.float32)


# -- expected values, computed once ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(kind, n):
    """``(med, mad, z)`` of the twins on 'noise' or 'planted' data with blocks of ``n``, read-only."""
    x = noise() if kind == 'noise' else planted(n)
    med, mad = search.block_median_mad_samples(x, n)
    z = search.robust_standardize_samples(x, n)
    for a in (med, mad, z):
        a.setflags(write=False)
    return med, mad, z


def data(kind, n):
    return noise() if kind == 'noise' else planted(n)


HOST_CASES = [('noise', n) for n in BLOCKS] + [('planted', n) for n in PLANT_BLOCKS]
HOST_IDS = [f'{kind}-{n}' for kind, n in HOST_CASES]


def stream(x, cls=None, **kwargs):
    """``x`` as a stream: a `HostStream` that is not page-locked, or ``cls`` (`DeviceStream`)."""
    kwargs.setdefault('samples_per_frame', x.shape[0])
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(x, bt.Time(T0), RATE, **kwargs)


# -- the shapes rank_geo_check.cpp walks: n_spec nbin n_elem m skip ------------------------------------------------
def geo_shapes():
    shapes = []
    for n in BLOCKS:
        shapes.append((1, NOISE_SHAPE[0] // n * n, NOISE_SHAPE[1], n, 0))
    for n in PLANT_BLOCKS:
        shapes.append((1, 3 * n, PLANT_COLUMNS, n, 0))
    for m, skip in WH_CUTS:
        shapes.append(WH_SHAPE + (m, skip))
    shapes += [(1, 67, 1, 67, 0), (1, 300, 4, 100, 0), (1, 2, 1, 2, 0),           # the sample shapes (67,), (300, 4), (1,)
               (1, 65536, 2, 65536, 0), (2, 1121, 3, 1120, 0), (1, 1121, 3, 1121, 0),     # the counter blocks, the boundary
               (4, 33, 8, 64, 1), (3, 10, 200, 4, 9)]                                 # a block longer than the spectrum; one bin left
    return shapes
