"""Fold tables made on the GPU from polynomial phases (bbt_phase_runs) against the host
table of the same pieces, and `Fold`, `PulseStack` and ``Integrate(phase=...)`` driven by a
`PolycoPhase` against the real reference (tests/golden/phases_vectors.npz)."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip
from baseband_tasks_amd.fold_table import piece_table, plan_pieces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')
FILES = {'B1937': 'B1937_polyco.dat', 'B1957': 'B1957_polyco.dat'}
GOLDEN = os.path.join(GOLDEN_DIR, 'phases_vectors.npz')


def polyco_phase(name):
    return bt.phases.PolycoPhase(os.path.join(GOLDEN_DIR, FILES[name]))


# -- 4. the device table is the host table -------------------------------------------------
# (name, start, rate, n_phase, row edges, c0, c1); B1937 spins at 641.9 Hz, B1957 at 622.1 Hz
TABLE_CASES = {
    # 0.3 samples per bin: most bins empty, every sample a run
    'sub_sample_bins': ('B1937', '2018-05-06T22:20:00', 197200., 1024, [0, 30000], 0, 30000),
    # 3 samples per bin, many rows, the chunk starts and ends inside rows
    'three_per_bin_rows': ('B1937', '2018-05-06T22:20:00', 123250., 64, list(range(5, 120000, 2113)), 1000, 101000),
    # 16 samples per bin at 1024 bins, one row
    'sixteen_per_bin': ('B1937', '2018-05-06T22:21:00', 10.517e6, 1024, [0, 300000], 0, 300000),
    # 1000 samples per bin
    'thousand_per_bin': ('B1957', '2014-06-09T22:00:00', 39.8e6, 64, [0, 100000, 250000], 0, 250000),
    # a single bin: one run per turn
    'one_bin': ('B1957', '2014-06-09T22:00:00', 1e5, 1, [0, 5000, 20000, 20001, 40000], 2500, 39000),
    # 100 bins, rows shorter than a period
    'short_rows': ('B1957', '2014-06-10T01:00:00', 1e6, 100, list(range(0, 60001, 500)), 250, 59750),
    # rows over the instant where the closest polyco entry changes (22:57:36)
    'two_entries': ('B1937', '2018-05-06T22:57:35', 1e5, 256, [0, 70000, 150000, 260000], 100, 259000),
    # c0 and c1 inside one row
    'inside_a_row': ('B1937', '2018-05-06T22:40:00', 1e6, 1024, [0, 1000000], 123457, 654321),
}


@pytest.mark.parametrize('case', sorted(TABLE_CASES))
def test_device_table_equals_host_table(case):
    name, start, rate, n_phase, edges, c0, c1 = TABLE_CASES[case]
    pp = polyco_phase(name)
    t0 = bt.Time(start)
    edges = np.array(edges, np.int64)

    def row_pieces(r, lo, hi):
        return pp.fold_pieces(t0 + int(edges[r]) / rate, rate, lo - int(edges[r]), hi - int(edges[r]))
    r0, n_row, sp, rb, re, cnt = piece_table(edges, row_pieces, n_phase, c0, c1)
    r0d, n_rowd, plan = plan_pieces(edges, row_pieces, n_phase, c0, c1)
    assert (r0d, n_rowd) == (r0, n_row)
    if case == 'two_entries':
        assert len(plan['row']) == n_row + 1                      # (one row is two pieces)
    sp_d, rb_d, re_d, n_run, cnt_d = hip.phase_runs(plan, n_phase)
    print(f'{case}: {c1 - c0} samples, {n_run} runs ({(c1 - c0) / max(n_run, 1):.2f} samples each), '
          f'capacity {plan["run_cap"]}, grid {int((plan["n_cycle"] * n_phase).sum())} cells')
    assert n_run == len(rb)
    np.testing.assert_array_equal(sp_d.to_host(), sp)
    np.testing.assert_array_equal(rb_d.to_host(), rb)
    np.testing.assert_array_equal(re_d.to_host(), re)
    np.testing.assert_array_equal(cnt_d, cnt)
    assert cnt.sum() == min(c1, edges[-1]) - max(c0, edges[0])
    # with a slot offset, as a chunk in the middle of an output has it
    sp_o, rb_o, re_o, n_run_o, cnt_o = hip.phase_runs(plan, n_phase, slot0=3, n_slot=n_row * n_phase + 7)
    np.testing.assert_array_equal(sp_o.to_host(), np.concatenate((np.zeros(3, np.int64), sp, np.full(4, sp[-1]))))
    np.testing.assert_array_equal(rb_o.to_host(), rb)
    # twice the same
    again = hip.phase_runs(plan, n_phase)
    np.testing.assert_array_equal(again[1].to_host(), rb)
    np.testing.assert_array_equal(again[4], cnt)


def test_decreasing_phase_is_refused():
    pp = polyco_phase('B1937')
    t0, rate = bt.Time('2018-05-06T22:20:00'), 1e5
    edges = np.array([0, 20000], np.int64)

    def row_pieces(r, lo, hi):
        return pp.fold_pieces(t0, rate, lo, hi)
    _, _, plan = plan_pieces(edges, row_pieces, 64, 0, 20000)
    plan['n_cycle'][:] = 1                  # (a grid too small for the bins: as if the phase ran off)
    with pytest.raises(ValueError):
        hip.phase_runs(plan, 64)


# -- 5. against the reference ----------------------------------------------------------------
def _cases():
    if not os.path.exists(GOLDEN):
        return []
    with np.load(GOLDEN, allow_pickle=False) as g:
        return sorted({k.split('/')[0] for k in g.files if k.startswith('case')})


def golden_task(g, case, route=None):
    meta = json.loads(str(g[f'{case}/meta']))
    t0 = bt.Time(int(meta['t0'][0]), float(meta['t0'][1]))
    sh = bt.HostStream(g['stream'], t0, meta['rate'], samples_per_frame=1000, pin=False,
                       polarization=np.array(['X', 'Y']))
    src = bt.Power(sh)
    pp = polyco_phase(meta['psr'])
    if meta['kind'] == 'fold':
        task = bt.Fold(src, meta['n_phase'], pp, meta['step'], start=meta['start'], average=meta['average'])
        task.table_route = route
    elif meta['kind'] == 'pulsestack':
        task = bt.PulseStack(src, meta['n_phase'], pp, start=meta['start'], average=meta['average'])
    else:
        task = bt.Integrate(src, meta['step'], pp, start=meta['start'], average=meta['average'])
    return meta, task


@pytest.mark.parametrize('case', _cases())
def test_against_reference(case):
    """Tolerance of the existing fold goldens (tests/test_fold_gpu.py::test_golden): float32 sums
    against the reference's, rtol 1e-5 with 1e-5 of the largest value as floor; counts equal."""
    with np.load(GOLDEN, allow_pickle=False) as g:
        meta, task = golden_task(g, case)
        assert list(task.shape) == meta['shape']
        if meta['kind'] == 'fold':
            assert meta['differing'] <= 1e-6 * meta['samples']       # (counted by the recipe)
        got = task.read()
        expected = g[f'{case}/data']
        if meta['average']:
            np.testing.assert_array_equal(np.isnan(got), np.isnan(expected))
            np.testing.assert_allclose(got, expected, rtol=1e-5, equal_nan=True,
                                       atol=1e-5 * np.nanmax(np.abs(expected)))
        else:
            np.testing.assert_array_equal(got['count'], g[f'{case}/count'])
            np.testing.assert_allclose(got['data'], expected, rtol=1e-5, atol=1e-5 * np.abs(expected).max())


# -- 6. routes and repeats -------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in _cases() if c in ('case00', 'case01', 'case02', 'case03')])
def test_device_route_equals_host_route(case, monkeypatch):
    def bits(a):
        if a.dtype.names:
            return np.concatenate((a['data'].view(np.uint32).ravel(), a['count'].astype(np.uint32).ravel()))
        return a.view(np.uint32)
    with np.load(GOLDEN, allow_pickle=False) as g:
        _, dev = golden_task(g, case, 'device')
        _, host = golden_task(g, case, 'host')
        assert dev._route() == 'device' and host._route() == 'host'
        a, b = dev.read(), host.read()
        np.testing.assert_array_equal(bits(a), bits(b))
        # two reads, and a second task
        dev.invalidate_cache()
        dev.seek(0)
        np.testing.assert_array_equal(bits(dev.read()), bits(a))
        _, dev2 = golden_task(g, case)
        assert dev2._route() == 'device'                               # (the default)
        np.testing.assert_array_equal(bits(dev2.read()), bits(a))
        # the environment's switch, and many chunks
        monkeypatch.setenv('BBT_FOLD_TABLE', 'host')
        _, env = golden_task(g, case)
        assert env._route() == 'host'
        monkeypatch.delenv('BBT_FOLD_TABLE')
        _, small = golden_task(g, case, 'device')
        small.fold_budget = 3001 * 16
        c = small.read()
        if c.dtype.names:
            np.testing.assert_array_equal(c['count'], a['count'])
            np.testing.assert_allclose(c['data'], a['data'], rtol=1e-5, atol=1e-4)
        else:
            np.testing.assert_allclose(c, a, rtol=1e-5, atol=1e-5, equal_nan=True)


def test_lambda_phases_go_on_as_before():
    with np.load(GOLDEN, allow_pickle=False) as g:
        meta, task = golden_task(g, 'case00')
        pp = task.phase
        plain = bt.Fold(task.ih, meta['n_phase'], lambda t: pp(t), meta['step'])
        assert not hasattr(plain.phase, 'fold_pieces')
        np.testing.assert_allclose(plain.read(), task.read(), rtol=1e-5, atol=1e-5, equal_nan=True)
