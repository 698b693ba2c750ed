"""The correlator on the host: the order of the baselines, `correlate_samples` against a plain double loop,
the surface of `Correlate` (shapes, rate, start time, metadata kept and dropped, refusals), how it cuts a
read into fetches, the library's exports, and the cutting of the kernels into segments, groups, tiles and
lanes walked by a sanitized host program.  No GPU."""
import json
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import correlation, hip

import corr_cases
from corr_cases import BY_NAME, RATE, SEG, T0, same_bits
from geo_check import compile_check, run_check, run_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'baseband-tasks_amd', 'csrc')


# -- the table ---------------------------------------------------------------------------------------------
def test_the_table_covers_what_it_says():
    cases = corr_cases.CASES
    assert 20 <= len(cases) <= 26
    assert {corr_cases.n_inputs(c) for c in cases} == {2, 3, 4, 5, 8, 15, 16, 17, 32, 33, 64}
    assert {corr_cases.n_elem(c) for c in cases} >= {1, 3, 7, 9, 40}
    assert {c.n for c in cases} == {1, 2, 3, 7, 1023, 1024, 1025, 2051, 3072}
    assert {c.blocks for c in cases} == {1, 2, 3} and {bool(c.tail) for c in cases} == {False, True}
    assert sum(c.axis % len(c.sample_shape) != len(c.sample_shape) - 1 for c in cases) >= 1
    for a in {corr_cases.n_inputs(c) for c in cases}:
        mine = [c.n for c in cases if corr_cases.n_inputs(c) == a]
        assert any(n % 2 for n in mine) and any(n >= SEG - 1 for n in mine), a     # an odd n and a segment edge
    for c in cases:
        assert corr_cases.n_samples(c) * int(np.prod(c.sample_shape)) < 1 << 22
    for name in corr_cases.DISTINCT:
        x = corr_cases.integer_data(name)
        flat = x.reshape(x.shape[0], -1)
        assert all(len(set(row.tolist())) == flat.shape[1] for row in flat)
    x = corr_cases.integer_data(corr_cases.IDS[0])
    assert np.abs(x.real).max() == 7 and np.abs(x.imag).max() == 7 and np.array_equal(x.real, np.rint(x.real))


# -- the order of the baselines and the values -----------------------------------------------------------------
def test_baseline_pairs():
    assert bt.baseline_pairs(2).tolist() == [[0, 0], [0, 1], [1, 1]]
    assert bt.baseline_pairs(3).tolist() == [[0, 0], [0, 1], [0, 2], [1, 1], [1, 2], [2, 2]]
    for a in (2, 5, 17, 64):
        pairs = bt.baseline_pairs(a)
        assert pairs.shape == (a * (a + 1) // 2, 2) and pairs.dtype.kind == 'i'
        assert pairs.tolist() == [[i, j] for i in range(a) for j in range(i, a)]
    for a in (1, 0, 65, -3):
        with pytest.raises(ValueError, match='inputs'):
            bt.baseline_pairs(a)
    with pytest.raises(TypeError):
        bt.baseline_pairs(2.5)


@pytest.mark.parametrize('average', [True, False])
@pytest.mark.parametrize('shape, axis', [((11, 2, 3), -1), ((11, 3, 2), 0), ((11, 2, 3, 2), 1), ((7, 4), -1)])
def test_correlate_samples_is_the_double_loop(shape, axis, average):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    n = 3
    got = bt.correlate_samples(x, n, axis, average=average)
    ax = 1 + axis % (len(shape) - 1)
    a = shape[ax]
    nb = shape[0] // n
    want_shape = (nb,) + shape[1:ax] + (a * (a + 1) // 2,) + shape[ax + 1:]
    assert got.shape == want_shape and got.dtype == np.complex64
    y = np.moveaxis(x, ax, -1).astype(np.complex128)
    g = np.moveaxis(got, ax, -1)
    for blk in range(nb):
        b = 0
        for i in range(a):
            for j in range(i, a):
                total = np.zeros(y.shape[1:-1], np.complex128)
                for t in range(blk * n, (blk + 1) * n):
                    total += y[t, ..., i] * np.conj(y[t, ..., j])
                if average:
                    total = total / n
                assert np.allclose(g[blk, ..., b], total, rtol=1e-6, atol=1e-6), (blk, i, j)
                if i == j:
                    assert not np.ascontiguousarray(g[blk, ..., b].imag).view(np.uint32).any()
                b += 1
    # exact on integers, and the convention of Power: X Y*
    z = np.array([[1 + 2j, 3 - 1j]], np.complex64)
    assert bt.correlate_samples(z, 1).tolist() == [[5 + 0j, (1 + 2j) * (3 + 1j), 10 + 0j]]
    for name in ('a8-e7-n7-b2', 'axis1-a4-e15-n7-b2-t1', 'a17-e3-n1025-b2-t7'):
        c = BY_NAME[name]
        for avg in (True, False):
            assert same_bits(bt.correlate_samples(corr_cases.integer_data(name), c.n, c.axis, average=avg),
                             corr_cases.integer_expected(name, avg))


# -- the task's surface -----------------------------------------------------------------------------------------
def test_correlate_surface():
    x = corr_cases.integer_data('a2-e40-n1024-b3-t5')
    freq = np.linspace(400e6, 800e6, 40).reshape(40, 1)
    sh = bt.HostStream(x, bt.Time(T0), RATE, samples_per_frame=100, pin=False, frequency=freq, sideband=1,
                       polarization=np.array(['X', 'Y']))
    task = bt.Correlate(sh, 1024)
    assert task.shape == (3, 40, 3) and task.sample_shape == (40, 3) and task.dtype == np.complex64
    assert task.sample_rate == RATE / 1024 and abs(task.start_time - sh.start_time) < 1e-9
    assert task.samples_per_frame == 1 and task.n == 1024 and task.n_inputs == 2 and task.average is True
    assert task.baselines.tolist() == [[0, 0], [0, 1], [1, 1]]
    assert np.array_equal(task.frequency, freq) and np.all(task.sideband == 1)
    with pytest.raises(AttributeError):
        task.polarization                                     # varies along the inputs: dropped
    assert bt.Correlate(sh, 1024, samples_per_frame=2).samples_per_frame == 2
    assert bt.Correlate(sh, 1024, average=False).average is False
    assert bt.Correlate(sh, 3077).shape == (1, 40, 3)
    # the inputs on another axis: (time, A, elements)
    y = np.ascontiguousarray(np.swapaxes(x, 1, 2))
    pol = np.array(['X', 'Y']).reshape(2, 1)
    sy = bt.HostStream(y, bt.Time(T0), RATE, samples_per_frame=100, pin=False, frequency=freq.reshape(40), sideband=1,
                       polarization=pol)
    ty = bt.Correlate(sy, 1024, axis=0)
    assert ty.shape == (3, 3, 40) and ty.axis == 0 and ty._inner == 40 and ty._n_elem == 40
    assert np.array_equal(np.broadcast_to(ty.frequency, (3, 40)), np.broadcast_to(freq.reshape(40), (3, 40)))
    with pytest.raises(AttributeError):
        ty.polarization
    assert isinstance(ty._src, bt.Transpose) and ty._src.shape == (3077, 40, 2) and task._src is sh
    # a polarization that does not vary along the inputs is kept
    keep = bt.HostStream(y, bt.Time(T0), RATE, samples_per_frame=100, pin=False, polarization=np.array(['X'] * 40))
    assert np.all(bt.Correlate(keep, 7, axis=0).polarization == 'X')
    # the refusals
    with pytest.raises(TypeError, match='complex64'):
        bt.Correlate(bt.HostStream(x.astype(np.complex128), bt.Time(T0), RATE, pin=False), 4)
    with pytest.raises(TypeError, match='complex64'):
        bt.Correlate(bt.HostStream(x.real.copy(), bt.Time(T0), RATE, pin=False), 4)
    for n in (0, -1, (1 << 24) + 1):
        with pytest.raises(ValueError, match='n must be'):
            bt.Correlate(sh, n)
    with pytest.raises(TypeError):
        bt.Correlate(sh, 2.5)
    with pytest.raises(ValueError, match='less than one integration'):
        bt.Correlate(sh, 3078)
    one = bt.HostStream(x[:, :, :1].copy(), bt.Time(T0), RATE, pin=False)
    with pytest.raises(ValueError, match='inputs'):
        bt.Correlate(one, 4)
    wide = bt.HostStream(np.zeros((8, 65), np.complex64), bt.Time(T0), RATE, pin=False)
    with pytest.raises(ValueError, match='inputs'):
        bt.Correlate(wide, 4)
    with pytest.raises(ValueError, match='axis'):
        bt.Correlate(sh, 4, axis=2)
    with pytest.raises(ValueError, match='sample shape'):
        bt.Correlate(bt.HostStream(np.zeros(8, np.complex64), bt.Time(T0), RATE, pin=False), 4)
    for name in ('Correlate', 'correlate_samples', 'baseline_pairs'):
        assert name in correlation.__all__ and getattr(bt, name) is getattr(correlation, name)


class _PlanLog:
    """Stands in for `hip.CorrPlan`: keeps what every call was told."""
    made = []

    def __init__(self, *args):
        self.args, self.calls = args, []
        _PlanLog.made.append(self)

    def execute(self, x, first, count, out, out_block0, n_out_blocks):
        assert x == (first, count) and out.shape[0] == n_out_blocks
        self.calls.append((first, count, out_block0, n_out_blocks))

    def close(self):
        pass


def test_fetches_are_whole_blocks_or_whole_segments(monkeypatch):
    x = corr_cases.integer_data('a16-e9-n2051-b2')
    sh = corr_cases.stream(x)
    row = 16 * 9 * 8
    task = bt.Correlate(sh, 2051, samples_per_frame=2)
    assert bt.Correlate.correlate_budget == 1 << 29
    assert task._chunk_size() == (1 << 29) // (2051 * row) and task._piece_size() == task._chunk_size() * 2051
    assert task._input_span(0, 1) == (sh, 0, 4102)
    monkeypatch.setattr(hip, 'CorrPlan', _PlanLog)
    monkeypatch.setattr(correlation, 'fetch_device', lambda ih, start, count: (start, count))
    del _PlanLog.made[:]
    out = np.empty((2, 9, 136), np.complex64)
    task._compute_frames(0, 1, out)
    plan, = _PlanLog.made
    assert plan.args == (16, 9, 2051, 1, True) and plan.calls == [(0, 4102, 0, 2)]
    del plan.calls[:]
    task.correlate_budget = 2051 * row                          # a block per fetch
    assert task._piece_size() == 2051 and task._input_span(0, 1) is None
    task._compute_frames(0, 1, out)
    assert plan.calls == [(0, 2051, 0, 1), (2051, 2051, 1, 1)]
    del plan.calls[:]
    task.correlate_budget = 2 * SEG * row + 5                   # two segments per fetch: a block takes two fetches
    assert task._chunk_size() == 1 and task._piece_size() == 2 * SEG
    task._compute_frames(0, 1, out)
    assert plan.calls == [(0, 2048, 0, 1), (2048, 3, 0, 1), (2051, 2048, 1, 1), (4099, 3, 1, 1)]
    del plan.calls[:]
    task.correlate_budget = 1                                    # one segment at least
    task._compute_frames(0, 1, out)
    assert plan.calls == [(0, 1024, 0, 1), (1024, 1024, 0, 1), (2048, 3, 0, 1),
                          (2051, 1024, 1, 1), (3075, 1024, 1, 1), (4099, 3, 1, 1)]
    for first, count, _, _ in plan.calls:                        # every piece is one the library accepts
        assert hip.corr_info(16, 9, 2051, first, count)['n_seg'] == -(-count // SEG)
    # the transposed stream is what is fetched when the inputs are not the last axis
    c = BY_NAME['axis1-a4-e15-n7-b2-t1']
    t2 = bt.Correlate(corr_cases.stream(corr_cases.integer_data(c.name)), c.n, c.axis)
    assert t2._input_span(0, 2)[0] is t2._src and t2._src.shape == (15, 3, 5, 4) and t2._inner == 5
    del _PlanLog.made[:]
    t2._compute_frames(0, 2, np.empty((2, 3, 10, 5), np.complex64))
    assert _PlanLog.made[0].args == (4, 15, 7, 5, True) and _PlanLog.made[0].calls == [(0, 14, 0, 2)]


# -- the library ----------------------------------------------------------------------------------------------
def test_library_exports_the_corr_entries():
    lib = hip.lib()
    assert lib.bbt_version() >= 171 and hip.MIN_LIB_VERSION >= 171
    header = open(os.path.join(ROOT, 'include', 'bbt_hip.h')).read()
    for name in ('bbt_corr_plan_create', 'bbt_corr_plan_destroy', 'bbt_corr_info', 'bbt_corr_execute'):
        assert name in hip.SIGNATURES and hasattr(lib, name) and name in header
    geo = open(os.path.join(CSRC, 'corr_geo.hpp')).read()
    assert f'#define BBT_CORR_SEG {hip.CORR_SEG}' in geo and correlation.SEG == hip.CORR_SEG == SEG
    assert f'#define BBT_CORR_MIN_INPUTS {hip.CORR_MIN_INPUTS}' in geo and f'#define BBT_CORR_MAX_INPUTS {hip.CORR_MAX_INPUTS}' in geo
    assert hip.CORR_MAX_N == 1 << 24 and '#define BBT_CORR_MAX_N (1ll << 24)' in geo
    main = open(os.path.join(CSRC, 'bbt_hip.hip')).read()
    assert '#include "corr_kernels.hpp"' in main and '#include "corr_geo.hpp"' in open(os.path.join(CSRC, 'corr_kernels.hpp')).read()
    assert callable(hip.CorrPlan.execute) and callable(hip.CorrPlan.info) and callable(hip.CorrPlan.close)


def test_corr_info_needs_no_device(monkeypatch):
    corr_cases.set_tiling(monkeypatch)
    for a, pack, tiles in ((2, 8, 1), (3, 5, 1), (4, 4, 1), (5, 3, 1), (8, 2, 1), (15, 1, 1), (16, 1, 1), (17, 1, 3), (32, 1, 3),
                           (33, 1, 6), (48, 1, 6), (49, 1, 10), (64, 1, 10)):
        info = hip.corr_info(a, 40, 2051, 0, 2 * 2051)
        assert (info['pack'], info['tiles'], info['waves'], info['n_seg']) == (pack, tiles, 4, 6), (a, info)
        assert info['lds_bytes'] == 4 * 32 * 33 * 4 and info['scratch_bytes'] == 6 * 40 * (a * (a + 1) // 2) * 8
    assert hip.corr_info(16, 1024, 1024)['n_seg'] == 1                       # one block by default
    for pack, waves in corr_cases.tilings(3):
        corr_cases.set_tiling(monkeypatch, pack, waves)
        info = hip.corr_info(3, 7, 1025)
        assert (info['pack'], info['waves']) == (pack, waves)
    corr_cases.set_tiling(monkeypatch, 6, 3)                                  # what the shape cannot take leaves the default
    info = hip.corr_info(3, 7, 1025)
    assert (info['pack'], info['waves']) == (5, 4)
    corr_cases.set_tiling(monkeypatch, 2, 8)
    assert hip.corr_info(17, 7, 1025)['pack'] == 1 and hip.corr_info(17, 7, 1025)['waves'] == 4
    corr_cases.set_tiling(monkeypatch)
    for args, what in (((1, 1, 1), 'n_inputs'), ((65, 1, 1), 'n_inputs'), ((2, 0, 1), 'n_elem'), ((2, 1, 0), 'n must'),
                       ((2, 1, (1 << 24) + 1), 'n must'), ((4, 3, 2051, 0, 1000), 'whole segments'),
                       ((4, 3, 2051, 5, 1024), 'whole segments'), ((4, 3, 2051, 0, 0), 'samples'), ((4, 3, 2051, -1024, 1024), 'samples')):
        with pytest.raises(hip.HipError, match=what):
            hip.corr_info(*args)
    with pytest.raises(hip.HipError, match='inner'):
        hip.CorrPlan(4, 15, 7, inner=4)
    for args in ((1, 1, 1), (65, 1, 1), (2, 0, 1), (2, 1, 0)):
        with pytest.raises(hip.HipError):
            hip.CorrPlan(*args)
    plan = hip.CorrPlan(4, 15, 7, inner=5, average=False)
    assert plan.n_baselines == 10 and plan.info(0, 14)['n_seg'] == 2
    plan.close()


# -- the cutting, on the host ----------------------------------------------------------------------------------
def test_kernel_cutting_on_the_host(tmp_path):
    """For every case, under every tiling the geometry accepts and cut into pieces three ways, and for the
    bench rows: every (block, segment, element, baseline) owned once through the tiles' cells, every lane's
    load inside the piece or a declared zero, every scratch and output cell written once, the LDS as
    stated: the program exits non-zero otherwise, and the sanitizers abort it on a wild index or an
    overflow of its own."""
    exe = compile_check('corr_geo_check', tmp_path)
    shapes = corr_cases.geo_shapes()
    plans = run_check(exe, shapes)
    seen = set()
    for shape, g in zip(shapes, plans):
        a, e, n, blocks, tail, pack, waves, piece = shape
        assert g['walk'] == 0, (shape, g)
        most = 32 // (2 * a) if a <= 16 else 1
        assert g['pack'] == (pack or most) and g['waves'] == (waves or 4)
        assert g['T'] == -(-g['pack'] * 2 * a // 32) and g['n_tile'] == g['T'] * (g['T'] + 1) // 2
        assert g['n_group'] == -(-e // g['pack']) and g['spb'] == -(-n // SEG) and g['n_seg'] == blocks * g['spb']
        assert g['lds_bytes'] == g['waves'] * 32 * 33 * 4
        want = 1 if piece == 0 else -(-blocks // -piece) if piece < 0 else blocks * -(-n // piece)
        assert g['pieces'] == want
        seen.add(g['n_tile'])
    assert seen == {1, 3, 6, 10}
    bad = run_raw(exe, '1 1 1 1 0 0 0 0  65 1 1 1 0 0 0 0  2 0 1 1 0 0 0 0  2 1 0 1 0 0 0 0  2 1 16777217 1 0 0 0 0  2 1 1 0 0 0 0 0')
    assert bad.returncode == 0, bad.stderr[-2000:]
    errors = [json.loads(line)['error'] for line in bad.stdout.splitlines()]
    assert len(errors) == 6
    assert 'n_inputs' in errors[0] and 'n_inputs' in errors[1] and 'n_elem' in errors[2] and 'n must' in errors[3]
    assert 'n must' in errors[4] and 'one block' in errors[5]
