"""Host side of `Fold`, `PulseStack` and ``Integrate(phase=...)`` (no GPU): array-valued
times, the run tables of fold_table.py against per-sample evaluation, shapes,
times and counts against the real reference's golden vectors
(tests/golden/fold_vectors.npz, made by make_fold_golden.py), and the argument
checks of the bbt_fold_runs entry point."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip
from baseband_tasks_amd.fold_table import bin_runs, fold_table, unwrapped_bin, sample_times

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'fold_vectors.npz')
T0 = bt.Time('2010-11-12T13:14:15')
RATE = 1e4


# -- array-valued Time --------------------------------------------------------------
def test_array_time_matches_scalar_time():
    offsets = np.array([-1.5, -1e-9, 0., 0.25, 1.75, 86399.5, 1e6 + 0.123456789])
    ta = T0 + offsets
    assert ta.shape == offsets.shape and not ta.isscalar
    t1 = bt.Time('2010-11-12T13:14:16.5')
    for i, off in enumerate(offsets):
        ts = T0 + float(off)
        assert ta[i] == ts
        assert (ta - t1)[i] == ts - t1
        assert ta.unix[i] == ts.unix
        assert tuple(np.array(ta.jd1_jd2())[:, i]) == ts.jd1_jd2()
    assert np.array_equal((ta - 0.5).unix, (T0 + (offsets - 0.5)).unix)


def test_scalar_time_unchanged():
    t = T0 + 1.25
    assert isinstance(t.sec, int) and isinstance(t.frac, float) and t.isscalar
    assert t - T0 == 1.25 and (t - 0.25) - T0 == 1.0
    assert repr(t) == "Time('2010-11-12T13:14:16.250000000')"


def test_reference_style_phase_callable():
    f0 = 80.
    ph = (lambda t: f0 * (t - T0))
    got = ph(T0 + np.arange(5) / RATE)
    np.testing.assert_allclose(got, f0 * np.arange(5) / RATE, rtol=0, atol=1e-15)


# -- run tables -----------------------------------------------------------------------
def _phase(kind, per_bin, n_phase, n):
    f = 1. / (per_bin * n_phase)          # cycles per sample
    if kind == 'linear':
        return lambda t: 0.123 + f * (t - T0) * RATE
    if kind == 'spindown':
        return lambda t: 0.123 + f * (t - T0) * RATE - 0.2 * f * ((t - T0) * RATE) ** 2 / n
    # sinusoidal modulation, still monotonic
    return lambda t: (0.123 + f * (t - T0) * RATE
                      + 0.4 * f * n / (2 * np.pi * 3) * np.sin(2 * np.pi * 3 * (t - T0) * RATE / n))


def _per_sample(phase_at, n_phase, lo, hi):
    n = np.arange(lo, hi, dtype=np.int64)
    k = unwrapped_bin(phase_at(n), n_phase)
    edge = np.flatnonzero(np.diff(k)) + 1
    return (np.concatenate(([lo], n[edge])), np.concatenate((n[edge], [hi])),
            k[np.concatenate(([0], edge))])


@pytest.mark.parametrize('kind', ['linear', 'spindown', 'sinusoidal'])
@pytest.mark.parametrize('per_bin', [0.3, 1, 2, 16, 1e4])
def test_bin_runs_equal_per_sample(kind, per_bin):
    n, n_phase = 200000, 37
    times = sample_times(T0 + 0.5 / RATE, 17, RATE)
    ph = _phase(kind, per_bin, n_phase, n)
    phase_at = (lambda s: ph(times(s)))
    got = bin_runs(phase_at, n_phase, 17, n - 3)
    want = _per_sample(phase_at, n_phase, 17, n - 3)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_chunk_edges_inside_runs():
    n, n_phase = 60000, 64
    ph = _phase('spindown', 40., n_phase, n)
    edges = np.array([0, 7001, 23456, 60000])

    def row_phase(r):
        times = sample_times(T0 + edges[r] / RATE, edges[r], RATE)
        return lambda s: ph(times(s))
    total = np.zeros((3, n_phase), np.int64)
    sums = np.zeros((3, n_phase))
    x = np.random.default_rng(1).standard_normal(n)
    for c0, c1 in [(0, 3333), (3333, 7002), (7002, 40001), (40001, 60000)]:
        r0, n_row, sp, rb, re, cnt = fold_table(edges, row_phase, n_phase, c0, c1)
        flat = total.reshape(-1)
        flat[r0 * n_phase:r0 * n_phase + len(cnt)] += cnt
        for j in range(len(sp) - 1):
            for r in range(sp[j], sp[j + 1]):
                sums.reshape(-1)[r0 * n_phase + j] += x[c0 + rb[r]:c0 + re[r]].sum()
    want = np.zeros((3, n_phase), np.int64)
    want_sum = np.zeros((3, n_phase))
    for r in range(3):
        s = np.arange(edges[r], edges[r + 1])
        b = unwrapped_bin(row_phase(r)(s), n_phase) % n_phase
        want[r] = np.bincount(b, minlength=n_phase)
        want_sum[r] = np.bincount(b, x[s], minlength=n_phase)
    np.testing.assert_array_equal(total, want)
    np.testing.assert_allclose(sums, want_sum, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('per_bin', [16, 100])
def test_phase_called_for_few_samples(per_bin):
    n, n_phase = 100000, 32
    ph = _phase('linear', per_bin, n_phase, n)
    asked = [0]

    def counting(t):
        asked[0] += t.shape[0]
        return ph(t)
    data = np.zeros((n, 1), np.float32)
    fh = bt.Fold(bt.HostStream(data, T0, RATE, pin=False), n_phase, counting)
    asked[0] = 0
    cnt = fh._counts(0, 1)
    assert cnt.sum() == n
    assert asked[0] < n / 4, asked[0]


# -- shapes, times and errors (the reference's test_times_wrong) ------------------------
@pytest.fixture(scope='module')
def pulsar():
    data = np.repeat(np.where(np.arange(16000) % 125 == 0, 10., 0.125)[:, None], 2, axis=1)
    return bt.HostStream(data.astype(np.float32), T0, RATE, samples_per_frame=200, pin=False)


def test_times_wrong(pulsar):
    ph = (lambda t: 80. * (t - T0))
    with pytest.raises(ValueError):
        bt.Fold(pulsar, 8, ph, start=T0 - 1.)
    with pytest.raises(ValueError):
        bt.Fold(pulsar, 8, ph, start=T0 + 3.)
    with pytest.raises(AssertionError):
        bt.Fold(pulsar, 8, ph, step=3600.)


def test_repr_and_dtype(pulsar):
    ph = (lambda t: 80. * (t - T0))
    fh = bt.Fold(pulsar, 8, ph, 0.01, average=False)
    r = repr(fh)
    assert r.startswith('Fold(ih') and 'n_phase=8' in r and 'step=0.01' in r and 'average=False' in r
    with pytest.raises(TypeError):
        bt.Fold(pulsar, 8, ph, dtype=np.float64)
    assert bt.Fold(pulsar, 8, ph, dtype=np.float32).dtype == np.float32
    ip = bt.Integrate(pulsar, 1. / 25, ph)
    assert ip.sample_rate == 25 and ip.shape == (3200, 2)


def test_non_integer_step_without_phase_still_refused(pulsar):
    with pytest.raises(NotImplementedError):
        bt.Integrate(pulsar, 2.5)


# -- golden vectors of the real reference -------------------------------------------------
def golden_task(g, case):
    """Rebuild golden case ``case`` with this package; returns (task, expected)."""
    meta = json.loads(str(g[f'{case}/meta']))
    data = g[f"stream/{meta['stream']}"]
    sh = bt.HostStream(np.ascontiguousarray(data), T0, RATE, samples_per_frame=200, pin=False)
    if 'slice_input' in meta:
        sh = sh[meta['slice_input'][0]:meta['slice_input'][1]]
    p = meta['phase']

    def ph(t):
        dt = t - T0
        return p['phi0'] + p['f0'] * dt + 0.5 * p['f1'] * dt * dt
    start = meta['start']
    if isinstance(start, dict):
        start = T0 + start['time']
    kind = meta['kind']
    if kind == 'fold':
        step = meta['step']
        task = bt.Fold(sh, meta['n_phase'], ph, step, start=start, average=meta['average'])
    elif kind == 'integrate':
        task = bt.Integrate(sh, meta['step'], ph, start=start, average=meta['average'])
    else:
        task = bt.PulseStack(sh, meta['n_phase'], ph, start=start, average=meta['average'])
        if 'slice_output' in meta:
            task = task[meta['slice_output'][0]:meta['slice_output'][1]]
        elif kind == 'integrate_stack':
            task = bt.Integrate(task, meta['n'])
    if f'{case}/count' in g.files:
        expected = np.empty(g[f'{case}/data'].shape, [('data', g[f'{case}/data'].dtype), ('count', int)])
        expected['data'] = g[f'{case}/data']
        expected['count'] = g[f'{case}/count']
    else:
        expected = g[f'{case}/data']
    return task, expected


def _cases():
    with np.load(GOLDEN, allow_pickle=False) as g:
        return sorted({k.split('/')[0] for k in g.files if k.startswith('case')})


@pytest.mark.parametrize('case', _cases())
def test_golden_geometry_and_counts(case):
    with np.load(GOLDEN, allow_pickle=False) as g:
        meta = json.loads(str(g[f'{case}/meta']))
        assert meta['bin_margin'] >= 1e-6 and meta['offset_margin'] >= 2e-3
        task, expected = golden_task(g, case)
        assert task.shape == tuple(meta['shape']) == expected.shape
        assert abs(task.start_time - bt.Time(meta['start_time'])) < 1e-9
        assert abs(task.stop_time - bt.Time(meta['stop_time'])) < 1e-9
        assert abs(task.sample_rate - meta['sample_rate']) < 1e-9 * meta['sample_rate']
        if f'{case}/count' in g.files:
            count = g[f'{case}/count']
            got = task._counts(0, task.shape[0])
            got = got.reshape(got.shape + (1,) * (count.ndim - got.ndim))
            np.testing.assert_array_equal(np.broadcast_to(got, count.shape), count)
        if meta['kind'] == 'integrate' and not meta['average']:
            np.testing.assert_array_equal(np.diff(task.edges), g[f'{case}/count'][:, 0])


# -- the C entry point's argument checks (no kernel runs) ---------------------------------
def test_fold_runs_argument_validation():
    lib = hip.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    sp = np.array([0, 1], np.int64).ctypes.data
    assert lib.bbt_fold_runs(None, p, 1, 1, 2, sp, sp, sp, 1, None, 0, None, 0, None) != 0
    assert b'null' in lib.bbt_last_error()
    assert lib.bbt_fold_runs(p, p, -1, 1, 2, sp, sp, sp, 1, None, 0, None, 0, None) != 0
    assert b'bad sizes' in lib.bbt_last_error()
    assert lib.bbt_fold_runs(p, p, 1, 1, 3, sp, sp, sp, 1, None, 0, None, 0, None) != 0
    assert b'mode' in lib.bbt_last_error()
    assert lib.bbt_fold_runs(p, p, 1, 3, 1, sp, sp, sp, 1, None, 0, None, 0, None) != 0
    assert b'pairs' in lib.bbt_last_error()
    assert lib.bbt_fold_runs(p, p, 1, 1, 2, sp, sp, sp, 1, None, 2, None, 0, None) != 0
    assert b'accumulate' in lib.bbt_last_error()
    assert lib.bbt_fold_runs(p, p, 1, 1, 2, sp, sp, sp, 1, None, 0, None, 16, None) != 0
    assert b'work' in lib.bbt_last_error()
    assert lib.bbt_fold_runs(p + 4, p, 1, 2, 1, sp, sp, sp, 1, None, 0, None, 0, None) != 0
    assert b'aligned' in lib.bbt_last_error()
    assert lib.bbt_version() >= 153


def test_fold_runs_wrapper_checks_tables():
    x = hip.DeviceArray.__new__(hip.DeviceArray)      # (never dereferenced: checks come first)
    x.shape, x.dtype = (10, 2), np.dtype(np.float32)
    out = hip.DeviceArray.__new__(hip.DeviceArray)
    out.shape, out.dtype = (1, 2), np.dtype(np.float32)
    with pytest.raises(ValueError):
        hip.fold_runs(x, out, 2, 2, [0, 1], [0], [11])            # run past the input
    with pytest.raises(ValueError):
        hip.fold_runs(x, out, 2, 2, [0, 2], [0], [5])             # slot_ptr vs runs
    with pytest.raises(ValueError):
        hip.fold_runs(x, out, 4, 2, [0, 1], [0], [5])             # input width
