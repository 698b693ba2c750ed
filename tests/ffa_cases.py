"""Cases shared by test_ffa_host.py (which proves, without a GPU, that the NumPy twin is the rule it claims to
be), test_ffa_gpu.py and test_ffa_guard_gpu.py (which run it on the device): `FFASearch`
(csrc/ffa_kernels.hpp) against `ffa.ffa_search_samples`.

All streams have a 10 kHz sample rate, a 600 MHz frequency and an upper sideband.  Each case has two data
sets: integers in [-4, 4] stored as float32, so that every fold and boxcar sum is exact (at most 8192 * 4 <
2^24) and ties are plentiful, and float32 noise, for which only the tree order of the sums gives the twin's
bits."""
import functools
from collections import namedtuple

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import ffa

from dmt_cases import same_bits  # noqa: F401  (shared helper)

Case = namedtuple('Case', 'name s N n periods K seed')

T0 = '2010-11-12T13:14:15'
RATE = 1e4

CASES = [
    # the smallest run
    Case('tiny', (3,), 100, 100, (8, 9), 1, 1),
    # m = 2 (M = 2), two blocks and a tail
    Case('two_rows', (2,), 120, 50, (17, 26), 2, 2),
    # m = 43 ... 30: M = 64 and 32, with m = 33 padded to 64 and m = 31 to 32; a prime column count above a wave
    Case('ragged', (67,), 1501, 700, (16, 23), 3, 3),
    # m = M = 32: no padded row
    Case('exact_rows', (5,), 544, 544, (17, 18), 3, 4),
    # M = 8192, 13 stages: every fuse remainder
    Case('long_fold', (5,), 40000, 40000, (9, 11), 3, 5),
    # p = 1024, m = 5, M = 8, the widest boxcar 512
    Case('wide_bins', (2,), 5200, 5200, (1020, 1025), 10, 6),
    # a tile that spans several elements and trailing axes
    Case('wide', (300, 4), 2048, 1024, (30, 34), 4, 7),
]
IDS = [c.name for c in CASES]
KINDS = ('int', 'noise')

#: every tiling the environment can ask for: (BBT_FFA_FUSE, BBT_FFA_WIDTH)
TILINGS = [(1, 4), (1, 32), (2, 8), (2, 16), (3, 4), (3, 16), (3, 32)]


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
    out = ffa.ffa_search_samples(data(case, kind), case.n, case.periods, case.K)
    out.setflags(write=False)
    return out


# -- the planted pulsar ------------------------------------------------------------------------------------
PLANTED = dict(n=6000, periods=(29, 35), K=4, period=31.4, width=2, amplitude=1., columns=5, column=3, seed=11)


@functools.lru_cache(maxsize=None)
def planted_data():
    """(6000, 5) float32 unit noise with, in column 3, a pulsar of period 31.4 samples, width 2 and amplitude 1:
    sample i is in the pulse if (i mod 31.4) < 2.  Ideal S/N: amplitude sqrt(n width / period) (1 - width /
    period)^(1/2) = 18.9."""
    c = PLANTED
    rng = np.random.default_rng(c['seed'])
    x = rng.standard_normal((c['n'], c['columns'])).astype(np.float32)
    i = np.arange(c['n'])
    on = np.mod(i, c['period']) < c['width']
    x[on, c['column']] += np.float32(c['amplitude'])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def planted_expected():
    c = PLANTED
    out = ffa.ffa_search_samples(planted_data(), c['n'], c['periods'], c['K'])
    out.setflags(write=False)
    return out
