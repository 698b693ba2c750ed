"""Cases shared by test_hsum_host.py (which proves, without a GPU, that the NumPy twins are the
rules they claim to be) and test_hsum_gpu.py (which runs them on the device): `HarmonicSearch` and
`Whiten` (csrc/hsum_kernels.hpp) against `periodicity.harmonic_search_samples` and
`periodicity.whiten_samples`.

All streams have a 10 Hz sample rate: a sample is one stack of spectra.  Each search case has two
data sets: integers 0 ... 8 stored as float32, so that every harmonic sum is exact (at most 32 * 8)
and ties are plentiful, and float32 exponential noise of unit mean, for which only the order of the
adds gives the twin's bits."""
import functools
from collections import namedtuple

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import periodicity

from dmt_cases import same_bits  # noqa: F401  (shared helper)

Case = namedtuple('Case', 'name s nbin N n K lo seed')

T0 = '2010-11-12T13:14:15'
RATE = 10.
AVERAGED = 1.

CASES = [
    # a single level: the output is the block maximum of p - 1 itself
    Case('one_level', (3,), 100, 2, 10, 1, 1, 1),
    # a prime element count above a wave, a short last block, lo cutting into level-dependent j
    Case('ragged', (67,), 1501, 3, 61, 5, 3, 2),
    # the real chain's shape; the last block is the Nyquist bin alone
    Case('rfft', (5,), 8193, 1, 64, 6, 1, 3),
    # one block per spectrum
    Case('one_block', (2,), 4096, 2, 4096, 6, 1, 4),
    # trailing axes, more elements than a tile
    Case('wide', (300, 4), 513, 2, 128, 4, 0, 5),
    # one bin per block
    Case('single_bin_blocks', (16,), 700, 4, 1, 5, 3, 6),
    # two and three levels, the only depths no other case has (k_hsum_search<2> and <3>): a prime element
    # count above a wave, a short last block (777 = 59 * 13 + 10), lo cutting into level-dependent j.  Blocks
    # of 13 bins, since among 61 integers 0 ... 8 some pair always beats the best single bin and level 0 never wins
    Case('two_levels', (67,), 777, 2, 13, 2, 2, 7),
    Case('three_levels', (67,), 777, 2, 13, 3, 2, 8),
]
IDS = [c.name for c in CASES]
KINDS = ('int', 'noise')
#: the cases that pin an instantiation by name: test_hsum_host.py holds the twin to winners at every level
EVERY_LEVEL_WINS = ('two_levels', 'three_levels')

#: tilings from the smallest to the largest: (BBT_HSUM_WIDTH, BBT_HSUM_SPLIT)
TILINGS = [(16, 1), (16, 16), (32, 4), (64, 2), (64, 16)]


def by_name(name):
    return CASES[IDS.index(name)]


@functools.lru_cache(maxsize=None)
def data(case, kind='int'):
    """The spectra of a case, (N, nbin) + s float32, read-only: 'int' or 'noise'."""
    rng = np.random.default_rng(case.seed + (0 if kind == 'int' else 1000))
    shape = (case.N, case.nbin) + case.s
    if kind == 'int':
        x = rng.integers(0, 9, size=shape).astype(np.float32)
    else:
        x = rng.standard_exponential(shape).astype(np.float32)
    x.setflags(write=False)
    return x


def stream(case, kind='int', cls=None, x=None, **kwargs):
    """The case as a stream: a `HostStream` that is not page-locked, or ``cls`` (`DeviceStream`)."""
    x = data(case, kind) if x is None else x
    kwargs.setdefault('samples_per_frame', x.shape[0])
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(x, bt.Time(T0), RATE, **kwargs)


@functools.lru_cache(maxsize=None)
def expected(case, kind='int'):
    """The NumPy twin on the case's data, read-only."""
    out = periodicity.harmonic_search_samples(data(case, kind), case.n, case.K, AVERAGED, case.lo)
    out.setflags(write=False)
    return out


# -- Whiten --------------------------------------------------------------------------------------------
WH_SHAPE = (3, 2100, 67)
#: blocks at and around the segment of 32 of the two-level sums, and one of many segments
WH_BLOCKS = (2, 31, 32, 33, 1000)
WH_SKIPS = (0, 1, 5)
#: the special columns
ZERO, NAN, INF, MINUS_ZERO, NEGATIVE, TINY = range(6)
NAN_AT, INF_AT = (1, 1207), (2, 40)                    # (spectrum, bin)


@functools.lru_cache(maxsize=None)
def wh_data():
    """(3, 2100, 67) float32 exponential noise of mean 4 with: column 0 all zero, column 1 a NaN at bin
    1207 of spectrum 1, column 2 an Inf at bin 40 of spectrum 2, column 3 all -0, column 4 of negative
    mean (the noise negated), column 5 constant 1e-42 (a denormal, whose reciprocal is no float32)."""
    rng = np.random.default_rng(78)
    x = (4. * rng.standard_exponential(WH_SHAPE)).astype(np.float32)
    x[:, :, ZERO] = 0.
    x[NAN_AT + (NAN,)] = np.nan
    x[INF_AT + (INF,)] = np.inf
    x[:, :, MINUS_ZERO] = -0.
    x[:, :, NEGATIVE] *= -1.
    x[:, :, TINY] = 1e-42
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def wh_expected(m, skip):
    out = periodicity.whiten_samples(wh_data(), m, skip)
    out.setflags(write=False)
    return out


def wh_stream(cls=None, x=None, **kwargs):
    x = wh_data() if x is None else x
    kwargs.setdefault('samples_per_frame', x.shape[0])
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(x, bt.Time(T0), RATE, **kwargs)


# -- the planted comb ------------------------------------------------------------------------------------
COMB_BINS = (40, 81, 121, 162, 202, 242, 283, 323)


def comb():
    """p = 1 on (1, 1025, 6) with 3 added in column 2 at the bins the rule gathers for (L, j) = (3, 323)."""
    p = np.ones((1, 1025, 6), np.float32)
    p[0, list(COMB_BINS), 2] += 3.
    return p
