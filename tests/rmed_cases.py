"""Shared cases of the sliding-median tests (test_rmed_host.py proves the twins, test_rmed_gpu.py and
test_rmed_guard_gpu.py hold the kernels to them bit for bit): the noise plane of rank_cases under every
width and scrunch the tilings cut at, a planted plane whose outcome the rule states, the selection
methods and tile widths, and the shapes the geometry check walks."""
import functools

import numpy as np

import baseband_tasks_amd as bt
from baseband_tasks_amd import search

import rank_cases
from rank_cases import RATE, T0, noise, same_bits, stream  # noqa: F401  (shared helpers)

#: (width, scrunch) on the (2100, 67) noise plane: 67 columns leave a ragged last tile at every tile width,
#: 2100 rows put several runs of workgroups and both clipped ends into every case; scrunches 32, 33 and
#: 100 cross a segment of 32, and R = 21 under width 255 clips every window on both sides
PLAIN = [(w, 1) for w in (3, 5, 31, 33, 65, 255, 1023)]
SCRUNCHED = [(w, s) for w in (3, 33, 255) for s in (2, 3, 8, 32, 33, 100)]
CASES = PLAIN + SCRUNCHED
IDS = [f'w{w}-s{s}' for w, s in CASES]

#: every way to run one rule: (BBT_RMED_SELECT, BBT_RMED_TILE, BBT_RMED_ROWS)
TILINGS = [(select, tile, rows) for select in (1, 2) for tile in (16, 32, 64) for rows in (None, 16)]
#: the cases every tiling runs: a narrow and a wide window on the samples, and a scrunched one
TILING_CASES = [(33, 1), (255, 1), (33, 8)]

# -- the planted plane -------------------------------------------------------------------------------------------
PLANT_ROWS = 1203                                # 150 rows of 8 and a tail of 3
(CONST, RAMP, STEP, SPIKE, ZEROS, EQUAL, DENORMAL, HUGE, NAN, INF, MINUS_NAN) = range(11)
PLANT_COLUMNS = 13
HUGE_BITS = 0x7f7fffff
NAN_AT, INF_AT, MINUS_NAN_AT = 500, 700, 900
SPIKE_AT = 600
STEP_AT = 640
#: (width, scrunch) the planted plane runs under
PLANT_CASES = [(9, 1), (33, 1), (9, 8), (5, 3)]


@functools.lru_cache(maxsize=None)
def planted():
    """(1203, 13) float32, read-only: the columns named above, the others noise."""
    rng = np.random.default_rng(77)
    n = PLANT_ROWS
    x = rng.normal(5., 3., (n, PLANT_COLUMNS)).astype(np.float32)
    x[:, CONST] = 2.5
    x[:, RAMP] = np.float32(-3.) + np.float32(0.125) * np.arange(n, dtype=np.float32)       # strictly monotone, exact
    x[:, STEP] = np.where(np.arange(n) < STEP_AT, np.float32(1.5), np.float32(-4.25))
    x[SPIKE_AT, SPIKE] = 1e6
    x[:, ZEROS] = np.where(rng.random(n) < 0.5, np.float32(0.), np.float32(-0.))
    x[:, EQUAL] = np.where(rng.random(n) < 0.6, np.float32(7.), rng.integers(5, 10, n).astype(np.float32))
    tiny = (rng.integers(1, 100, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32)
    x[:, DENORMAL] = tiny
    x[:, HUGE] = np.where(rng.random(n) < 0.6, np.array([HUGE_BITS], np.uint32).view(np.float32)[0],
                          rng.normal(0., 1., n).astype(np.float32))
    x[NAN_AT, NAN] = np.nan
    x[INF_AT, INF] = np.inf
    x[:, MINUS_NAN].view(np.uint32)[MINUS_NAN_AT] = 0xffc00001                                # a negative NaN with a payload
    x.setflags(write=False)
    return x


def data(kind):
    return noise() if kind == 'noise' else planted()


@functools.lru_cache(maxsize=None)
def expected(kind, width, scrunch):
    """``(b, z)`` of the twins, `running_median_samples` and `detrend_samples`, read-only."""
    x = data(kind)
    b, z = search.running_median_samples(x, width, scrunch), search.detrend_samples(x, width, scrunch)
    b.setflags(write=False)
    z.setflags(write=False)
    return b, z


def set_tiling(monkeypatch, select=None, tile=None, rows=None):
    for name, value in (('BBT_RMED_SELECT', select), ('BBT_RMED_TILE', tile), ('BBT_RMED_ROWS', rows)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def flagged_samples(n_samples, width, scrunch, bad_sample):
    """The samples of a stream that the rule zeroes for one bad sample: those whose baseline uses, as the
    interpolation's integers say, a median whose window holds the bad sample's scrunch row."""
    s, h, rows = scrunch, width // 2, n_samples // scrunch
    bad_row = bad_sample // s
    i = np.arange(rows * s)
    if rows == 1:
        return np.full(s, True)
    j = 2 * i + 1 - s
    r0 = np.clip(np.floor_divide(j, 2 * s), 0, rows - 2)
    q = j - 2 * s * r0

    def holds(r):
        return np.abs(r - bad_row) <= h
    return np.where(q <= 0, holds(r0), np.where(q >= 2 * s, holds(r0 + 1), holds(r0) | holds(r0 + 1)))


# -- the shapes rmed_geo_check.cpp walks: width scrunch n_elem n_samples tile rows method chunk ------------------------
def geo_shapes():
    shapes = []
    for w, s in CASES:
        shapes.append((w, s, 67, 2100, 0, 0, 0, 0))
    for w, s in TILING_CASES:
        for select, tile, rows in TILINGS:
            shapes.append((w, s, 67, 2100, tile, rows or 0, select, 0))
    for w, s in PLANT_CASES:
        shapes.append((w, s, PLANT_COLUMNS, PLANT_ROWS, 0, 0, 0, 0))
    shapes += [(33, 1, 1, 2100, 0, 0, 0, 0), (33, 8, 15, 600, 0, 0, 0, 0),               # one column; a (3, 5) sample shape
               (33, 8, 67, 2100, 0, 0, 0, 8), (33, 8, 67, 2100, 0, 0, 0, 704),           # chunks of one scrunch row; three chunks
               (33, 1, 67, 2100, 0, 0, 0, 1), (33, 1, 67, 2100, 0, 0, 0, 700),
               (1023, 1, 67, 2100, 64, 0, 0, 0), (1023, 1, 67, 2100, 32, 16, 1, 0),       # a forced tile too wide for the window
               (9, 2, 3, 37, 0, 0, 0, 0), (9, 2, 3, 37, 0, 0, 0, 4), (5, 1, 3, 23, 0, 0, 0, 8),      # the guard-band shapes
               (129, 1, 512, 1 << 20, 0, 0, 0, 0), (65, 16, 512, 1 << 20, 0, 0, 0, 0), (129, 8, 512, 1 << 20, 0, 0, 0, 1 << 17),
               (1023, 1, 64, 1 << 18, 0, 0, 0, 0), (1023, 1, 2, 1 << 22, 0, 0, 0, 0), (3, 4096, 2, 1 << 22, 0, 0, 0, 0)]
    return shapes
