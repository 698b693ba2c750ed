"""Cases shared by test_lspec_host.py (no GPU: the yardstick, the task's surface, the index maps) and
test_lspec_gpu.py (the kernels): `LongSpectra` (csrc/lspec_kernels.hpp) against
`periodicity.long_spectra_samples`, the float64 ``rfft`` yardstick.

THE TOLERANCE.  The project bounds transform amplitudes by REL_L2_TOL = 1e-6 and MAX_TOL = 1e-5
(tests/test_gpu_parity.py; round trips through 2^24-sample transforms meet them).  A power is the
square of an amplitude, so its relative error doubles: per column, against the yardstick,

    rel_l2 = |got - want|_2 / |want|_2 <= 2e-6        max |got - want| / max(want) <= 2e-5.

Per column, so that one wrong column of a wide plane cannot hide in the norm.  The columns of one
case have equal variance: with columns paired into one complex stream, a column's error scales with
the larger norm of the pair."""
import functools
from collections import namedtuple

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import periodicity

from dmt_cases import same_bits  # noqa: F401  (shared helper)

REL_L2_TOL = 2e-6
MAX_TOL = 2e-5

T0 = '2010-11-12T13:14:15'
RATE = 1000.

Case = namedtuple('Case', 'name log2n n_elem stack nspec tail seed')

#: every length, with element counts at the seams: one column (a zero partner alone), more pairs than
#: one, an odd count, more pairs than a last-pass tile holds (66 columns: 33 pairs, tiles of 8), and a
#: stack with two output spectra and a tail that is dropped
NOISE = [
    Case('2^15x1', 15, 1, 1, 1, 0, 1),
    Case('2^15x6', 15, 6, 1, 1, 0, 2),
    Case('2^16x5', 16, 5, 1, 1, 0, 3),
    Case('2^17x2', 17, 2, 1, 1, 0, 4),
    Case('2^18x66', 18, 66, 1, 1, 0, 5),
    Case('2^19x4', 19, 4, 1, 1, 0, 6),
    Case('2^20x4', 20, 4, 1, 1, 0, 7),
    Case('2^21x2', 21, 2, 1, 1, 0, 8),
    Case('2^22x4', 22, 4, 1, 1, 0, 9),
    Case('2^15x6_stack3', 15, 6, 3, 2, 1000, 10),
]
NOISE_IDS = [c.name for c in NOISE]


def by_name(name):
    return NOISE[NOISE_IDS.index(name)]


@functools.lru_cache(maxsize=2)
def data(case):
    """(nspec * stack * n + tail, n_elem) float32 noise of unit variance, read-only."""
    rng = np.random.default_rng(case.seed)
    x = rng.standard_normal((case.nspec * case.stack * (1 << case.log2n) + case.tail, case.n_elem), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=2)
def expected(case):
    want = periodicity.long_spectra_samples(data(case), 1 << case.log2n, case.stack)
    want.setflags(write=False)
    return want


def stream(x, cls=None, **kwargs):
    """``x`` as a stream: a `HostStream` that is not page-locked, or ``cls`` (`DeviceStream`)."""
    kwargs.setdefault('samples_per_frame', min(x.shape[0], 1 << 15))
    if cls is None or cls is bt.HostStream:
        cls = bt.HostStream
        kwargs['pin'] = False
    return cls(np.asarray(x), bt.Time(T0), RATE, **kwargs)


def column_errors(got, want):
    """Per column (everything but the first two axes flattened): rel-L2 and max |diff| / max want."""
    got = np.asarray(got, np.float64).reshape(got.shape[0] * got.shape[1], -1)
    want = np.asarray(want, np.float64).reshape(got.shape)
    diff = got - want
    rel = np.sqrt((diff ** 2).sum(axis=0) / (want ** 2).sum(axis=0))
    peak = np.abs(diff).max(axis=0) / want.max(axis=0)
    return rel, peak


def assert_close(got, want, what=''):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    rel, peak = column_errors(got, want)
    print(f"{what}: worst column rel-L2 {rel.max():.3g} (<= {REL_L2_TOL}), max/max {peak.max():.3g} (<= {MAX_TOL})")
    assert (rel <= REL_L2_TOL).all() and (peak <= MAX_TOL).all(), (what, rel.max(), peak.max())


def tone_bins(n, n1):
    """The fence posts of the partner map k <-> n - k of a split n = n1 n2, k = k1 + n1 k2: the first bin,
    either side of the first row boundary, a multiple of n1 (the row k1 = 0), n / 4, and the last two
    bins; None: a constant column (bin 0)."""
    return [1, n1 - 1, n1, n1 + 1, 5 * n1, n // 4, n // 2 - 1, n // 2, None]


def tones(n, n1):
    """Column c holds cos(2 pi j_c t / n) (the last one a constant): float32 (n, 9)."""
    t = np.arange(n, dtype=np.int64)
    cols = [np.ones(n) if j is None else np.cos(2. * np.pi * ((j * t) % n) / n) for j in tone_bins(n, n1)]
    return np.stack(cols, axis=1).astype(np.float32)
