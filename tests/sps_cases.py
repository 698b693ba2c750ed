"""Cases shared by test_boxcar_host.py (which proves, without a GPU, that the NumPy twins are the
rules they claim to be) and test_boxcar_gpu.py (which runs them on the device): `BoxcarSearch` and
`Standardize` (csrc/sps_kernels.hpp) against `search.boxcar_search_samples` and
`search.standardize_samples`.

All streams have a 10 kHz sample rate, a 600 MHz frequency and an upper sideband.  Each boxcar case
has two data sets: integers in [-4, 4] stored as float32, so that every window sum is exact (at most
4096 * 4 < 2^24) and ties are plentiful, and float32 noise, for which only the tree order of the
sums gives the twin's bits."""
import functools
from collections import namedtuple

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import search

from dmt_cases import same_bits  # noqa: F401  (shared helper)

Case = namedtuple('Case', 'name s N n K seed')

T0 = '2010-11-12T13:14:15'
RATE = 1e4

CASES = [
    # the output is the block maximum itself
    Case('one_width', (3,), 100, 10, 1, 1),
    # a prime element count above a wave, a block that is no multiple of anything, a dropped tail
    Case('ragged', (67,), 1501, 61, 6, 2),
    # a halo far longer than a block; most windows of width 4096 do not fit
    Case('long_halo', (5,), 4200, 64, 13, 3),
    # exactly one window of the top width
    Case('just_fits', (2,), 4096, 4096, 13, 4),
    # trailing axes, more elements than a tile
    Case('wide', (300, 4), 1024, 256, 8, 5),
    # one-sample blocks
    Case('single_sample_blocks', (16,), 700, 1, 5, 6),
]
IDS = [c.name for c in CASES]
KINDS = ('int', 'noise')

#: every tiling the environment can ask for, from the smallest to the largest: (BBT_SPS_WIDTH,
#: BBT_SPS_FUSE, BBT_SPS_SPLIT)
TILINGS = [(16, 1, 1), (16, 3, 16), (32, 2, 4), (64, 1, 2), (64, 3, 1), (32, 3, 8), (64, 2, 4)]


def by_name(name):
    return CASES[IDS.index(name)]


@functools.lru_cache(maxsize=None)
def data(case, kind='int'):
    """The samples of a case, (N,) + s float32, read-only: 'int' or 'noise'."""
    rng = np.random.default_rng(case.seed + (0 if kind == 'int' else 1000))
    shape = (case.N,) + case.s
    if kind == 'int':
        x = rng.integers(-4, 5, size=shape).astype(np.float32)
    else:
        x = rng.standard_normal(shape).astype(np.float32)
    x.setflags(write=False)
    return x


def stream(case, kind='int', cls=None, x=None, **kwargs):
    """The case as a stream: a `HostStream` that is not page-locked, or ``cls`` (`DeviceStream`)."""
    x = data(case, kind) if x is None else x
    kwargs.setdefault('samples_per_frame', x.shape[0])
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(x, bt.Time(T0), RATE, frequency=600e6, sideband=1, **kwargs)


@functools.lru_cache(maxsize=None)
def expected(case, kind='int'):
    """The NumPy twin on the case's data, read-only."""
    out = search.boxcar_search_samples(data(case, kind), case.n, case.K)
    out.setflags(write=False)
    return out


# -- Standardize ---------------------------------------------------------------------------------------
STD_S, STD_N = (67,), 2100
#: blocks at and around the segment of 32 of the two-level sums, and one of many segments
STD_BLOCKS = (2, 31, 32, 33, 1000)


@functools.lru_cache(maxsize=None)
def std_data():
    """(2100, 67) float32 noise of mean 5 and deviation 3 with, for every block length: column 0 constant
    (2.5: its variance is exactly 0), column 1 all zero, column 2 a NaN at samples 7 and 1500, column 3 an
    Inf at sample 40, column 4 all -0, column 5 constant 0.1 (whatever rounding makes of it)."""
    rng = np.random.default_rng(77)
    x = (5. + 3. * rng.standard_normal((STD_N,) + STD_S)).astype(np.float32)
    x[:, 0] = 2.5
    x[:, 1] = 0.
    x[7, 2] = x[1500, 2] = np.nan
    x[40, 3] = np.inf
    x[:, 4] = -0.
    x[:, 5] = 0.1
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def std_expected(n):
    out = search.standardize_samples(std_data(), n)
    out.setflags(write=False)
    return out


def std_stream(cls=None, x=None, **kwargs):
    x = std_data() if x is None else x
    kwargs.setdefault('samples_per_frame', x.shape[0])
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(x, bt.Time(T0), RATE, frequency=600e6, sideband=1, **kwargs)
