"""The sliding-median rule on the host: the NumPy twins (`search.running_median_samples`,
`search.detrend_samples`) against independent restatements, the planted columns, the edges, what the
running baseline buys `FFASearch` on red data, the surface of `RunningMedian` and `Detrend`, the library's
exports, and the tiling and the two selection methods of the kernels walked by a sanitized host program.
No GPU."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import device_task, hip, search

import rmed_cases
from rmed_cases import RATE, T0, same_bits
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


def _median(window):
    return np.median(window.astype(np.float64), axis=0).astype(np.float32)


def _two_level(x, s):
    """c of the rule by a plain loop: float64, segments of 32 in order, the segment sums in order."""
    rows = x.shape[0] // s
    c = np.empty((rows,) + x.shape[1:], np.float32)
    for r in range(rows):
        total = np.zeros(x.shape[1:], np.float64)
        for t0 in range(0, s, 32):
            a = np.zeros(x.shape[1:], np.float64)
            for t in range(t0, min(t0 + 32, s)):
                a += x[r * s + t].astype(np.float64)
            total += a
        c[r] = (total / np.float64(s)).astype(np.float32)
    return c


def _lerp(m, s):
    """b of the rule from the medians, sample by sample integers, three float32 operations."""
    rows = m.shape[0]
    if rows == 1:
        return np.repeat(m, s, axis=0)
    b = np.empty((rows * s,) + m.shape[1:], np.float32)
    for i in range(rows * s):
        j = 2 * i + 1 - s
        r0 = min(max(j // (2 * s), 0), rows - 2)
        q = j - 2 * s * r0
        if q <= 0:
            b[i] = m[r0]
        elif q >= 2 * s:
            b[i] = m[r0 + 1]
        else:
            f = np.float32(np.float64(q) / np.float64(2 * s))
            d = m[r0 + 1] - m[r0]
            p = d * f
            b[i] = m[r0] + p
    return b


# -- the twins are the rule -----------------------------------------------------------------------------
@pytest.mark.parametrize('w', [3, 33, 129, 1023])
def test_twin_is_the_plain_median_on_the_samples(w):
    x = rmed_cases.noise()
    b = search.running_median_samples(x, w)
    assert b.dtype == np.float32 and b.shape == x.shape
    h, n = w // 2, x.shape[0]
    windows = np.lib.stride_tricks.sliding_window_view(x, w, axis=0)               # interior rows h ... n - h - 1
    step = 1 if w < 200 else 7
    rows = np.arange(h, n - h, step)
    assert same_bits(b[rows], np.median(windows[rows - h].astype(np.float64), axis=-1).astype(np.float32))
    for r in list(range(0, h, max(1, h // 40))) + list(range(n - h, n, max(1, h // 40))) + [h - 1, n - 1]:
        assert same_bits(b[r], _median(x[max(0, r - h):r + h + 1])), r             # the clipped window, odd or even
    z = search.detrend_samples(x, w)
    assert z.dtype == np.float32 and same_bits(z, x - b)


@pytest.mark.parametrize('w, s', [(3, 2), (33, 3), (33, 8), (255, 32), (33, 33), (3, 100)])
def test_twin_is_the_rule_scrunched(w, s):
    x = rmed_cases.noise()
    rows, h = x.shape[0] // s, w // 2
    c = _two_level(x, s)
    got_c, bad = search._scrunch(np.ascontiguousarray(x[:rows * s]), s)
    assert same_bits(got_c, c) and not bad.any()
    m = np.stack([_median(c[max(0, r - h):r + h + 1]) for r in range(rows)])
    b = search.running_median_samples(x, w, s)
    assert b.shape == (rows * s, 67) and same_bits(b, _lerp(m, s))
    z = search.detrend_samples(x, w, s)
    assert same_bits(z, x[:rows * s] - b)
    # the medians stand at the centres of their rows: an odd scrunch has a sample there
    if s % 2:
        assert same_bits(b[s // 2::s], m)
    assert same_bits(b[:(s + 1) // 2], np.broadcast_to(m[0], ((s + 1) // 2, 67)))   # flat before the first centre
    assert same_bits(b[-((s + 1) // 2):], np.broadcast_to(m[-1], ((s + 1) // 2, 67)))    # and after the last


# -- planted columns ---------------------------------------------------------------------------------------
def _zero_bits(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


def test_planted_columns_on_the_samples():
    c = rmed_cases
    x = c.planted()
    n = x.shape[0]
    for w in (9, 33):
        h = w // 2
        b, z = c.expected('planted', w, 1)
        inner = slice(h, n - h)
        assert _zero_bits(z[:, c.CONST]) and (b[:, c.CONST] == 2.5).all()
        # a strictly monotone ramp is its own median where the window is whole, and not at the clipped ends
        assert same_bits(b[inner, c.RAMP], x[inner, c.RAMP]) and _zero_bits(z[inner, c.RAMP])
        assert (z[:h, c.RAMP] != 0).all() and (z[n - h:, c.RAMP] != 0).all()
        # a step is reproduced exactly
        assert same_bits(b[:, c.STEP], x[:, c.STEP]) and _zero_bits(z[:, c.STEP])
        # a spike changes no median: against the column with a merely large value in its place
        y = x.copy()
        y[c.SPIKE_AT, c.SPIKE] = 100.
        assert x[c.SPIKE_AT, c.SPIKE] == 1e6 and y[:, c.SPIKE].max() == 100.
        assert same_bits(search.running_median_samples(y[:, c.SPIKE], w), b[:, c.SPIKE])
        assert z[c.SPIKE_AT, c.SPIKE] > 9e5
        # ties of +0 and -0, many equal values, denormals and the largest float: selected by the key rule
        for col in (c.ZEROS, c.EQUAL, c.DENORMAL, c.HUGE):
            keys = search._rank_keys(x[:, col])
            for r in (0, 3, h, 600, 601, n - 2, n - 1):
                win = np.sort(keys[max(0, r - h):r + h + 1])
                lo, hi = search._rank_values(win[[(len(win) - 1) // 2]]), search._rank_values(win[[len(win) // 2]])
                want = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(np.float32)
                assert same_bits(b[r, col], want[0]), (col, r)
        assert set(b[h:n - h, c.ZEROS].view(np.uint32).tolist()) == {0, 0x80000000}
        assert (b[inner, c.HUGE].view(np.uint32) == c.HUGE_BITS).sum() > n // 2 and np.isfinite(b).all()
        assert (np.abs(b[:, c.DENORMAL]) < 1e-40).all() and (b[:, c.EQUAL] == 7.).sum() > n // 2
        # a NaN, an Inf, a negative NaN: +0 in exactly the rows whose window holds it, in both outputs
        for col, at in ((c.NAN, c.NAN_AT), (c.INF, c.INF_AT), (c.MINUS_NAN, c.MINUS_NAN_AT)):
            hit = np.abs(np.arange(n) - at) <= h
            assert np.array_equal(hit, c.flagged_samples(n, w, 1, at))
            assert _zero_bits(z[hit, col]) and _zero_bits(b[hit, col])
            assert (b[~hit, col] != 0).all() and same_bits(z[~hit, col], x[~hit, col] - b[~hit, col])
        assert np.isfinite(z).all()


@pytest.mark.parametrize('w, s', [(9, 8), (5, 3)])
def test_planted_columns_scrunched(w, s):
    c = rmed_cases
    x = c.planted()
    rows = x.shape[0] // s
    b, z = c.expected('planted', w, s)
    assert b.shape == z.shape == (rows * s, c.PLANT_COLUMNS)
    assert _zero_bits(z[:, c.CONST]) and (b[:, c.CONST] == 2.5).all()
    for col, at in ((c.NAN, c.NAN_AT), (c.INF, c.INF_AT), (c.MINUS_NAN, c.MINUS_NAN_AT)):
        hit = c.flagged_samples(x.shape[0], w, s, at)
        # between the centres of two rows both medians are used; the samples at and beyond a centre use one
        assert hit.sum() in ((w + 1) * s, (w + 1) * s - 1) and hit[at]
        assert _zero_bits(z[hit, col]) and _zero_bits(b[hit, col])
        assert (b[~hit, col] != 0).all() and (z[~hit, col] != 0).all() and np.isfinite(z[:, col]).all()
    assert np.isfinite(z).all() and np.isfinite(b).all()
    # the spike moves the mean of its row, and a median of rows shrugs that off
    assert abs(b[:, c.SPIKE]).max() < 20. and z[c.SPIKE_AT, c.SPIKE] > 9e5


# -- edges ---------------------------------------------------------------------------------------------------
def test_edges():
    rng = np.random.default_rng(9)
    x = rng.normal(0., 1., (205, 3)).astype(np.float32)
    # R = 1: one median, a flat baseline; R = 2; R < w: every window clipped on both sides
    b = search.running_median_samples(x, 5, 205)
    assert b.shape == (205, 3) and same_bits(b, np.broadcast_to(_two_level(x, 205)[0], (205, 3)))
    b = search.running_median_samples(x[:7], 3, 1)
    assert same_bits(b[0], _median(x[:2])) and same_bits(b[6], _median(x[5:7])) and same_bits(b[3], _median(x[2:5]))
    for s in (100, 102):
        c = _two_level(x, s)
        assert c.shape[0] == 2
        m = _median(c)                                          # both windows hold both rows
        assert same_bits(search.running_median_samples(x, 3, s), np.broadcast_to(m, (2 * s, 3)))
    c = _two_level(x, 10)                                       # R = 20 < w = 255
    m = np.stack([_median(c) for _ in range(20)])
    assert same_bits(search.running_median_samples(x, 255, 10), _lerp(m, 10))
    c = _two_level(x, 20)                                       # R = 10, w = 5
    m = np.stack([_median(c[max(0, r - 2):r + 3]) for r in range(10)])
    assert same_bits(search.running_median_samples(x, 5, 20), _lerp(m, 20))
    # the tail of N % S samples is dropped
    for s in (1, 2, 3, 32, 33, 100):
        z = search.detrend_samples(x, 3, s)
        assert z.shape == (205 // s * s, 3)
        assert same_bits(z, search.detrend_samples(x[:205 // s * s], 3, s))
    # widths 3 and 1023
    long = rng.normal(0., 1., 1500).astype(np.float32)
    b = search.running_median_samples(long, 1023)
    assert same_bits(b[[0, 511, 700, 1499]], np.array([_median(long[:512]), _median(long[:1023]), _median(long[189:1212]),
                                                       _median(long[988:])], np.float32))
    b = search.running_median_samples(long, 3)
    assert same_bits(b[1:-1], np.median(np.lib.stride_tricks.sliding_window_view(long, 3).astype(np.float64), axis=-1).astype(np.float32))


def test_twin_refusals():
    x = np.ones((10, 3), np.float32)
    for fn in (search.running_median_samples, search.detrend_samples):
        for w in (1, 4, 1025, 0, -3):
            with pytest.raises(ValueError, match='width'):
                fn(x, w)
        for s in (0, 4097, -1):
            with pytest.raises(ValueError, match='scrunch'):
                fn(x, 3, s)
        with pytest.raises(ValueError, match='scrunch row'):
            fn(x, 3, 11)
        with pytest.raises(TypeError):
            fn(x.astype(np.float64), 3)
        with pytest.raises(TypeError):
            fn(x, 3.5)
        with pytest.raises(TypeError):
            fn(x, 3, 2.5)
        assert fn(x, 3, 4).shape == (8, 3) and fn(x, 1023, 10).shape == (10, 3)
    assert _zero_bits(search.detrend_samples(x, 3)) and (search.running_median_samples(x, 3, 4) == 1.).all()


# -- what it buys -------------------------------------------------------------------------------------------
def test_a_running_baseline_keeps_the_snr_of_a_slow_pulsar_on_red_data():
    rng = np.random.default_rng(7)
    n = 2 ** 15
    noise = rng.standard_normal((n, 2))
    t = np.arange(n)[:, np.newaxis]
    drift = 4 * np.sin(2 * np.pi * t / 3000) + 0.03 * np.cumsum(rng.standard_normal((n, 2)), axis=0)
    pulse = np.zeros((n, 2))
    pulse[:, 0] = 1.2 * ((np.arange(n) / 301.37) % 1 < 4 / 301.37)
    clean, red = (noise + pulse).astype(np.float32), (noise + drift + pulse).astype(np.float32)

    def best(z):
        snr = bt.ffa_search_samples(z, n, (290, 312), 5)[0, :, 0]
        return snr.max(axis=0), 290 + snr.argmax(axis=0)
    reference, at = best(search.standardize_samples(clean, 4096))
    print('no drift:', reference, at)
    assert at[0] == 301
    for w, s in ((65, 8), (513, 1)):
        got, at = best(search.standardize_samples(search.detrend_samples(red, w, s), 4096))
        print(f'Detrend({w}, {s}):', got, at)
        assert at[0] == 301 and got[0] >= 0.9 * reference[0] and got[1] < 6.
    got, at = best(search.standardize_samples(red, 4096))
    print('Standardize alone:', got, at)
    assert at[0] == 301 and got[0] <= 0.5 * reference[0]


# -- the tasks ------------------------------------------------------------------------------------------------
def test_surface():
    x = rmed_cases.noise()
    sh = rmed_cases.stream(x, samples_per_frame=100)
    for cls in (bt.Detrend, bt.RunningMedian):
        for w, s in ((3, 1), (65, 16), (255, 100), (1023, 33)):
            task = cls(sh, w, s)
            length = x.shape[0] // s * s
            assert task.shape == (length, 67) and task.dtype == np.float32 and (task.width, task.scrunch) == (w, s)
            assert task.sample_rate == RATE and abs(task.start_time - bt.Time(T0)) < 1e-9
            assert task.samples_per_frame == min(-(-100 // s) * s, length)
            assert ' '.join(repr(task).split()).startswith(f'{cls.__name__}(ih, width={w}' + (f', scrunch={s})' if s > 1 else ')'))
        task = cls(sh, 9, scrunch=4, samples_per_frame=200)
        assert task.samples_per_frame == 200 and 'samples_per_frame=200' in repr(task)
        assert cls.detrend_budget == 1 << 29
        flat = cls(rmed_cases.stream(x[:, 0].copy()), 33, 8)
        assert flat.shape == (2096,)
        three = cls(rmed_cases.stream(np.ones((40, 3, 5), np.float32)), 5, 3)
        assert three.shape == (39, 3, 5) and three._n_elem == 15
    assert isinstance(bt.Detrend(sh, 3), device_task.ChunkedDeviceTask) and bt.Detrend.__mro__[1] is bt.RunningMedian.__mro__[1]


def test_metadata():
    x = np.ones((40, 30, 3), np.float32)
    per_bin = np.linspace(4e8, 8e8, 30).reshape(30, 1)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False, frequency=per_bin, sideband=1,
                       polarization=np.array(['X', 'Y', 'X']))
    for task in (bt.Detrend(sh, 5, 2), bt.RunningMedian(sh, 5)):
        np.testing.assert_array_equal(task.frequency, sh.frequency)
        assert task.sideband == 1
        np.testing.assert_array_equal(task.polarization, sh.polarization)
    # a lone frequency, as the plane of DMTrials has
    src = bt.HostStream(np.zeros((300, 4), np.float32), bt.Time(T0), 1e4, pin=False,
                        frequency=np.linspace(4e8, 8e8, 4), sideband=1)
    plane = bt.DMTrials(src, [0., .1, .2])
    for task in (bt.Detrend(plane, 9, 4), bt.RunningMedian(plane, 9)):
        assert task.frequency == plane.frequency
        with pytest.raises(AttributeError):
            task.sideband
        assert abs(task.start_time - plane.start_time) < 1e-12 and task.sample_rate == plane.sample_rate
    dt = bt.Detrend(plane, 9, 4)
    assert dt.shape == (plane.shape[0] // 4 * 4, 3)
    # the next stages take it as it is
    z = bt.Standardize(dt, 16)
    assert bt.BoxcarSearch(z, 16, 3).shape == (z.shape[0] // 16, 3, 3)


def test_what_is_refused():
    x = np.ones((40, 10, 3), np.float32)
    sh = bt.HostStream(x, bt.Time(T0), RATE, pin=False)
    z = bt.HostStream(x.astype(np.complex64), bt.Time(T0), RATE, pin=False)
    f64 = bt.HostStream(x.astype(np.float64), bt.Time(T0), RATE, pin=False)
    for cls in (bt.Detrend, bt.RunningMedian):
        with pytest.raises(TypeError, match='Square'):
            cls(z, 3)
        with pytest.raises(TypeError, match='float32'):
            cls(f64, 3)
        with pytest.raises(TypeError):
            cls(sh, 3.5)
        with pytest.raises(TypeError):
            cls(sh, 3, 1.5)
        for w in (1, 2, 4, 1024, 1025, 0, -5):
            with pytest.raises(ValueError, match='width'):
                cls(sh, w)
        for s in (0, 4097, -2):
            with pytest.raises(ValueError, match='scrunch'):
                cls(sh, 3, s)
        with pytest.raises(ValueError, match='less than one scrunch row'):
            cls(sh, 3, 41)
        for spf in (3, 6, 0, 2):
            with pytest.raises(ValueError, match='multiple'):
                cls(sh, 3, 4, samples_per_frame=spf)
        cls(sh, 3, 40), cls(sh, 1023, 4, samples_per_frame=4), cls(sh, 3, 1, samples_per_frame=7)


class _PlanLog:
    """Stands in for `hip.RmedPlan`: keeps what every call was told."""
    made = []

    def __init__(self, *args):
        self.args, self.calls = args, []
        _PlanLog.made.append(self)

    def execute(self, x, in_first, n_in, out, out_first, n_out, n_rows, detrend=True):
        assert x == (in_first, n_in) and out.shape[0] == n_out
        self.calls.append((in_first, n_in, out_first, n_out, n_rows, detrend))

    def close(self):
        pass


def test_chunking_hooks(monkeypatch):
    """`_chunk_input` is rmed_need of csrc/rmed_geo.hpp (through `hip.rmed_info`, which needs no device), a
    tiny budget gives chunks of one scrunch row, and the loop hands the plan where in the stream every
    chunk lies."""
    x = rmed_cases.noise()
    sh = rmed_cases.stream(x, samples_per_frame=100)
    for w, s in ((33, 8), (33, 1), (255, 100), (3, 2), (1023, 1)):
        task = bt.Detrend(sh, w, s)
        rows, h = 2100 // s, w // 2
        for r0, r1 in ((0, 1), (0, rows), (rows - 1, rows), (rows // 2, rows // 2 + 3), (1, 2), (h + 1, h + 2)):
            if r1 > rows or r0 >= r1:
                continue
            info = hip.rmed_info(w, s, 67, rows, r0 * s, (r1 - r0) * s)
            assert task._chunk_input(r0 * s, r1 * s) == (info['in_first'], info['in_count'])
            near = 1 if s > 1 else 0
            lo, hi = max(0, max(0, r0 - near) - h), min(rows, min(rows, r1 + near) + h)
            assert (info['in_first'], info['in_count']) == (lo * s, (hi - lo) * s)
    task = bt.Detrend(sh, 33, 8, samples_per_frame=2096)
    assert task._chunk_size() % 8 == 0 and task._chunk_size() >= 2096 and task._input_span(0, 1) == (sh, 0, 2096)
    task.detrend_budget = 1
    assert task._chunk_size() == 8 and task._input_span(0, 1) is None
    row = 67 * 4
    task.detrend_budget = 34 * (8 * row + row) + 704 // 8 * (2 * 8 * row + 2 * row)
    assert task._chunk_size() == 704
    plain = bt.RunningMedian(sh, 33, samples_per_frame=2100)
    plain.detrend_budget = 34 * row + 700 * 2 * row
    assert plain._chunk_size() == 700
    # the loop
    monkeypatch.setattr(hip, 'RmedPlan', _PlanLog)
    monkeypatch.setattr(device_task, 'fetch_device', lambda ih, start, count: (start, count))
    del _PlanLog.made[:]
    task._compute_frames(0, 1, np.empty((2096, 67), np.float32))
    plain._compute_frames(0, 1, np.empty((2100, 67), np.float32))
    plan, plan1 = _PlanLog.made
    assert plan.args == (33, 8, 67) and plan1.args == (33, 1, 67)
    assert plan.calls == [(0, (88 + 17) * 8, 0, 704, 262, True), ((88 - 17) * 8, (88 + 34) * 8, 704, 704, 262, True),
                          ((176 - 17) * 8, 2096 - (176 - 17) * 8, 1408, 688, 262, True)]
    assert plan1.calls == [(0, 716, 0, 700, 2100, False), (684, 732, 700, 700, 2100, False), (1384, 716, 1400, 700, 2100, False)]
    task.detrend_budget = 1
    del plan.calls[:]
    task._compute_frames(0, 1, np.empty((2096, 67), np.float32))
    assert len(plan.calls) == 262 and plan.calls[100] == ((100 - 17) * 8, 35 * 8, 800, 8, 262, True)
    assert plan.calls[0] == (0, 18 * 8, 0, 8, 262, True) and plan.calls[261] == ((261 - 17) * 8, 18 * 8, 2088, 8, 262, True)


# -- the library ----------------------------------------------------------------------------------------------
def test_library_exports_the_rmed_entries():
    lib = hip.lib()
    assert lib.bbt_version() >= 170 and hip.MIN_LIB_VERSION >= 170
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_rmed_plan_create', 'bbt_rmed_plan_destroy', 'bbt_rmed_info', 'bbt_rmed_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'rmed_geo.hpp')).read()
    assert f'#define BBT_RMED_MIN_WIDTH {hip.RMED_MIN_WIDTH}' in geo and f'#define BBT_RMED_MAX_WIDTH {hip.RMED_MAX_WIDTH}' in geo
    assert f'#define BBT_RMED_MAX_SCRUNCH {hip.RMED_MAX_SCRUNCH}' in geo
    assert (hip.RMED_MAX_WIDTH, hip.RMED_MAX_SCRUNCH) == (1023, 4096) == (search.MAX_WIDTH, search.MAX_SCRUNCH)
    assert f'#define BBT_RMED_SEG {search.SEGMENT}' in geo
    for name in ('RunningMedian', 'Detrend', 'running_median_samples', 'detrend_samples'):
        assert name in search.__all__ and getattr(bt, name) is getattr(search, name)
    assert callable(hip.RmedPlan.execute) and callable(hip.RmedPlan.info) and callable(hip.RmedPlan.close)


def test_rmed_info_needs_no_device(monkeypatch):
    rmed_cases.set_tiling(monkeypatch)
    # the automatic rule, from the measured sweep: 16 elements and 128 medians a workgroup, fewer where the 72 KiB
    # leave less beside the halo
    for w, s, e in ((65, 16, 512), (129, 1, 512), (255, 1, 512), (897, 1, 512), (899, 1, 64), (1023, 1, 64), (3, 1, 16), (3, 1, 33)):
        tile = 16
        info = hip.rmed_info(w, s, e, 1 << 20, 0, s << 16)
        assert (info['method'], info['tile']) == ('walk', tile)
        assert info['rows'] == min(128, hip.RANK_LDS_BYTES // (4 * tile) - (w - 1)) and info['lds_bytes'] == (info['rows'] + w - 1) * 64
        near = 1 if s > 1 else 0
        assert (info['in_first'], info['in_count']) == (0, ((1 << 16) + near + w // 2) * s)
        assert info['scratch_bytes'] == (((1 << 16) + near + w // 2) + (1 << 16) + near) * e * 4 * near
    info = hip.rmed_info(33, 8, 67, 262)                                       # one scrunch row by default
    assert (info['in_first'], info['in_count'], info['rows']) == (0, 18 * 8, 2)
    for select, tile, rows in rmed_cases.TILINGS:
        rmed_cases.set_tiling(monkeypatch, select, tile, rows)
        info = hip.rmed_info(33, 8, 67, 262, 0, 2096)
        assert (info['method'], info['tile'], info['rows']) == (hip.RMED_METHODS[select], tile, rows or 128)
    # a forced tile too wide for the window is halved until 16 rows are left for the run
    rmed_cases.set_tiling(monkeypatch, tile=64)
    assert hip.rmed_info(273, 1, 67, 2100, 0, 2100)['tile'] == 64 and hip.rmed_info(275, 1, 67, 2100, 0, 2100)['tile'] == 32
    assert hip.rmed_info(1023, 1, 67, 2100, 0, 2100)['tile'] == 16
    monkeypatch.setenv('BBT_RMED_TILE', '48')
    monkeypatch.setenv('BBT_RMED_SELECT', '3')
    monkeypatch.setenv('BBT_RMED_ROWS', '17')
    info = hip.rmed_info(33, 8, 67, 262, 0, 2096)
    assert (info['method'], info['tile'], info['rows']) == ('walk', 16, 128)
    for args, what in (((4, 1, 1, 10), 'width'), ((1, 1, 1, 10), 'width'), ((1025, 1, 1, 10), 'width'), ((3, 0, 1, 10), 'scrunch'),
                       ((3, 4097, 1, 10), 'scrunch'), ((3, 1, 0, 10), 'elements'), ((3, 1, 1, 0), 'rows'),
                       ((3, 2, 1, (1 << 39) + 1), '2\\^40'), ((3, 2, 1, 10, 1, 2), 'whole scrunch rows'),
                       ((3, 2, 1, 10, 0, 3), 'whole scrunch rows'), ((3, 2, 1, 10, 20, 2), 'beyond'), ((3, 2, 1, 10, 0, 22), 'beyond')):
        with pytest.raises(hip.HipError, match=what):
            hip.rmed_info(*args)


# -- the tiling and the selection, on the host ---------------------------------------------------------------------
def test_kernel_tiling_and_selection_on_the_host(tmp_path):
    """The limits and refusals, the interpolation's integers, both selection methods against sorted windows
    on some ten thousand windows, ties and NaN included, and for every shape of the GPU tests and the bench
    every median owned once, every staged row inside the stream and the input, every window inside the
    staged rows, the LDS within the budget, the input span per call as stated: the program exits non-zero
    otherwise, and the sanitizers abort it on a wild index or an overflow of its own."""
    exe = compile_check('rmed_geo_check', tmp_path)
    shapes = rmed_cases.geo_shapes()
    plans = run_check(exe, shapes)
    seen = set()
    for shape, g in zip(shapes, plans):
        w, s, e, n, tile, rows, method, chunk = shape
        assert g['walk'] == 0, (shape, g)
        assert g['nx'] * g['ny'] == 256 and g['n_rows'] == n // s and g['n_tile'] == -(-e // g['nx'])
        assert g['calls'] == (-(-(n // s * s) // chunk) if chunk else 1)
        if tile and hip.RANK_LDS_BYTES // (4 * tile) - (w - 1) >= 16:
            assert g['nx'] == tile
        assert g['method'] == (method or 2)
        assert 1 <= g['run'] <= hip.RANK_LDS_BYTES // (4 * g['nx']) - (w - 1) and (not rows or g['run'] <= rows)
        assert g['lds_bytes'] == (g['run'] + w - 1) * g['nx'] * 4 <= hip.RANK_LDS_BYTES
        seen.add((g['method'], g['nx']))
    assert len(seen) == 6                                            # both methods, every tile width
    bad = run_raw(exe, '4 1 1 10 0 0 0 0  1025 1 1 10 0 0 0 0  3 0 1 10 0 0 0 0  3 4097 1 10 0 0 0 0  3 1 0 10 0 0 0 0 '
                       '3 4 1 3 0 0 0 0  3 1 1 10 48 0 0 0  3 1 1 10 0 0 3 0')
    assert bad.returncode == 0
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 8
    assert 'width' in errors[0] and 'width' in errors[1] and 'scrunch' in errors[2] and 'scrunch' in errors[3]
    assert 'elements' in errors[4] and 'rows' in errors[5] and 'tile' in errors[6] and 'method' in errors[7]
