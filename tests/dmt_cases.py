"""Cases shared by test_dmtrials_host.py (which proves, without a GPU, that the shift rule is that
of `DedisperseSamples`, that each case has the geometry it is named for and that the NumPy twin sums
exactly) and test_dmtrials_gpu.py (which runs them on the device): `DMTrials`
(csrc/dmt_kernels.hpp) against `search.dm_trials_samples`.

All streams have a 10 kHz sample rate and, unless a case says otherwise, channel frequencies spread
linearly over 400.3 ... 799.1 MHz, upper sideband.  Each case has two data sets: small integers in
[-8, 8] stored as float32, so that every sum is exact in any order (at most 1030 channels: below
2^24), and float32 noise, for which only the ascending order gives the twin's bits."""
import functools
from collections import namedtuple

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import search

Case = namedtuple('Case', 'name nchan band sideband dms reference n rest hi lo seed')

T0 = '2010-11-12T13:14:15'
RATE = 1e4
BAND = (400.3e6, 799.1e6)

#: hi, lo: the largest and smallest shift of the table (None: not pinned), worked out with the plain
#: formula and the package's delay constant; test_dmtrials_host.py holds `dm_trial_shifts` to them.
CASES = [
    # a plain channel sum, no padding
    Case('zero_dm', 5, BAND, 1, (0.,), None, 100, (), 0, 0, 1),
    # both signs, a tiny table
    Case('narrow', 3, (600e6, 610e6), 1, (0.3, 1.7), None, 200, (), 3, -3, 2),
    # a prime channel count above a wave, ragged trial and time tiles
    Case('tile_edges', 67, BAND, 1, tuple(np.linspace(0., 3.1, 13)), None, 1500, (), None, None, 3),
    # a sweep far longer than any time tile, adjacent channels up to 965 samples apart
    Case('wide_span', 16, BAND, 1, (0., 17.3, 30.9), None, 8000, (), 1557, -4436, 4),
    # one-sided tables: the reference at the top of the band, above it and below it
    Case('ref_top', 16, BAND, 1, (0., 2.3, 5.9), 800e6, 2500, (), 0, None, 5),
    Case('ref_above', 16, BAND, 1, (0., 2.3, 5.9), 1500e6, 2500, (), 0, None, 6),
    Case('ref_below', 16, BAND, 1, (0., 2.3, 5.9), 300e6, 2500, (), None, 0, 7),
    # a negative trial, the order kept as given
    Case('neg_unsorted', 16, BAND, 1, (4.1, -2.3, 0., 1.9), None, 2000, (), None, None, 8),
    # channel order is index order, not frequency order
    Case('descending', 16, BAND[::-1], -1, (0., 2.3, 5.9), None, 2000, (), None, None, 9),
    # more trials than a tile and than a register block
    Case('many_dm', 16, BAND, 1, tuple(np.arange(300) * 0.0137), None, 1600, (), None, None, 10),
    # a channel loop longer than anything staged; exact sums still below 2^24
    Case('many_chan', 1030, BAND, 1, (0., 1.3, 2.9), None, 1200, (), None, None, 11),
    # per-product planes stay separate
    Case('trailing', 16, BAND, 1, (0., 2.3), None, 1000, (4,), None, None, 12),
]
IDS = [c.name for c in CASES]

#: span = hi - lo of the cases that pin it
SPANS = dict(zero_dm=0, narrow=6, tile_edges=601, wide_span=5993, neg_unsorted=919, descending=1144, many_dm=794,
             many_chan=562)


def by_name(name):
    return CASES[IDS.index(name)]


def frequency(case):
    """Channel frequencies in Hz, shaped to broadcast against the sample shape."""
    f = np.linspace(case.band[0], case.band[1], case.nchan)
    return f.reshape((case.nchan,) + (1,) * len(case.rest))


@functools.lru_cache(maxsize=None)
def data(case, kind='int'):
    """The samples of a case, (n, nchan) + rest float32, read-only: 'int' or 'noise'."""
    rng = np.random.default_rng(case.seed + (0 if kind == 'int' else 1000))
    shape = (case.n, case.nchan) + case.rest
    if kind == 'int':
        x = rng.integers(-8, 9, size=shape).astype(np.float32)
    else:
        x = rng.standard_normal(shape).astype(np.float32)
    x.setflags(write=False)
    return x


def stream(case, kind='int', cls=None, x=None, **kwargs):
    """The case as a stream: a `HostStream` that is not page-locked, or ``cls`` (`DeviceStream`)."""
    x = data(case, kind) if x is None else x
    kwargs.setdefault('samples_per_frame', case.n)
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(x, bt.Time(T0), RATE, frequency=frequency(case), sideband=case.sideband, **kwargs)


@functools.lru_cache(maxsize=None)
def shifts(case):
    s = search.dm_trial_shifts(stream(case), case.dms, case.reference)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected(case, kind='int'):
    """The NumPy twin on the case's data, read-only."""
    out = search.dm_trials_samples(data(case, kind), shifts(case))
    out.setflags(write=False)
    return out


def same_bits(a, b):
    """Equal as bit patterns (so -0 is not +0), except that a NaN equals any NaN: the sign and
    payload of a NaN made by Inf - Inf are not fixed by IEEE 754, and the CPU's differs from the
    GPU's."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype != np.float32:
        return False
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
