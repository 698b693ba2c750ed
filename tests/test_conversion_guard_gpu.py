"""`bbt_r2c_execute` between guard bands (tests/guard_bands.py, tests/r2c_cases.py): every kernel of
Real2Complex at the stream counts and pointer offsets that choose its access width, the three-step route in
several batches, and its work buffers growing.  Until now every array came from the pool, 16-byte aligned, with
1, 2, 3 or 8 streams, and the three-step route ran in one batch.

Each run holds, in this order: Re out to (-1)^m x[2m] bit for bit; EVERY slot (frame, stream) to the float64
reference of test_conversion_gpu.py at a relative L2 of 2e-6 -- the project's figure for the operation, which
the older tests apply once over the whole output; all bands to their poison and the input to what it was; and
the run whose pointers are off 16 to the bits of the aligned run.  By name:

  compiled     `BBT_G2_KERNEL_R2C` at vec 4 (S = 4, 12), 2 (S = 2, 6) and 1 (S = 1, 3, 5, and every S off 16)
  gen          `k_r2c_gen`, the fall-back, in a child process with BBT_RTC=0: S = 4, 6 and 2, aligned and off
  big          `k_r2c_big<16384, 4 | 2 | 1>`; (16384, 4, 1) off 16 is VEC = 1 on four live neighbouring streams
  three_steps  `k_r2c_gather` / `k_r2c_combine` with BBT_R2C_WORK_KIB set for two groups and five groups a
               call: batches of 2, 2, 1 (g0 > 0, a ragged last batch whose group has 1, 2 or 3 dead slots)
  regrow       one plan, calls of 1, 5 and 1 groups: the buffers are freed and allocated again, then kept
  unequal      streams scaled 1, 2^-10, 1, 2^-10 on each route: a quiet slot shares a complex transform with a
               loud one and is held to 2e-6 of its GROUP's norm (the crosstalk scales with the partner)

What stays outside: the work buffers the plan owns.

Measured on an MI355X, 2026-10-21: no band touched; every run off 16 gave the bits of the aligned run, `k_r2c_big`
included.  The largest per-slot relative L2 is 3.0e-7 (compiled, M = 8192; `k_r2c_gen` 2.0e-7, `k_r2c_big` 1.8e-7,
three steps 2.4e-7) against the 2e-6 allowed.  A quiet slot's error over its OWN norm is 1.6e-4 (M = 1215), 9.7e-5
(16384) and 1.5e-4 (10000, three steps): 1.5e-7, 0.9e-7 and 1.4e-7 of its group's norm.  """
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from baseband_tasks_amd import hip

import r2c_cases as rc
from guard_bands import POISONS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
both_poisons = pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))

# the output of the latest aligned run, for the skewed runs that follow it
_aligned = {}


def _expand(route, cases, skews=rc.SKEWS):
    """(case, skew) pairs, the skew fastest and the aligned run first, with ids that name the path."""
    pairs = [(c, s) for c in cases for s in skews]
    return pytest.mark.parametrize('case, skew', pairs, ids=[rc.case_id(route, *c, s) for c, s in pairs])


def _held_to_aligned(key, skew, run):
    """`run(skew)` is one guarded run, already held to the reference and its bands; a skewed one must give the
    bits of the aligned run (made here, if it is not the one that ran last)."""
    out = run(skew)[0]
    if skew == (0, 0):
        _aligned.clear()
        _aligned[key] = out
        return
    ref = _aligned.get(key)
    if ref is None:
        ref = run((0, 0))[0]
        _aligned.clear()
        _aligned[key] = ref
    assert rc.same_bits(out, ref), (f'{key}: {np.count_nonzero(out != ref)} of {out.size} samples of the run at {skew} '
                                    f'differ from the aligned run')


def _one_pass(route, case, skew, poison):
    M, S, frames = case
    x, ref = rc.data(M, S, frames)
    plan = hip.R2CPlan(M, S)
    try:
        assert plan.info()['one_pass']
        _held_to_aligned((route, case, poison), skew,
                         lambda sk: rc.run(plan, x, ref, poison, sk, rc.case_id(route, M, S, frames, sk)))
    finally:
        plan.close()


@_expand('compiled', rc.COMPILED)
@both_poisons
def test_compiled_kernel(case, skew, poison):
    _one_pass('compiled', case, skew, poison)


@_expand('big', rc.BIG)
@both_poisons
def test_k_r2c_big(case, skew, poison):
    """The three widths are three instantiations: equal bits are expected (the same operations on the same
    values in the same order) and were found, so they are required here too."""
    _one_pass('big', case, skew, poison)


# -- the fall-back kernel, in a process of its own that compiles nothing ---------------------------------------
def child(arg):
    """In the child process (BBT_RTC=0): every fall-back case at both skews under both poisons; the first failure
    ends it."""
    assert os.environ.get('BBT_RTC') == '0'
    for M, S, frames in json.loads(arg):
        x, ref = rc.data(M, S, frames)
        plan = hip.R2CPlan(M, S)
        for name, poison in POISONS.items():
            outs = [rc.run(plan, x, ref, poison, sk, f'{name} ' + rc.case_id('gen', M, S, frames, sk))
                    for sk in rc.FALLBACK_SKEWS]
            assert rc.same_bits(outs[0][0], outs[1][0]), (M, S, frames, name)
            print(f'CASE {M} {S} {frames} {name} {max(o[1] for o in outs):.3e}', flush=True)
        plan.close()
    assert hip.rtc_info()['modules'] == 0, 'a kernel was compiled: this was not the fall-back'
    print('DONE', flush=True)


def test_k_r2c_gen_fallback_in_a_child():
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_conversion_guard_gpu as t; t.child(sys.argv[1])"
            % (ROOT, os.path.join(ROOT, 'tests')))
    out = subprocess.run([sys.executable, '-c', code, json.dumps(rc.FALLBACK)], env=dict(os.environ, BBT_RTC='0'),
                         capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    assert out.stdout.count('CASE ') == 2 * len(rc.FALLBACK) and out.stdout.rstrip().endswith('DONE')


# -- three steps --------------------------------------------------------------------------------------------
def _three_step_plan(M, S):
    plan = hip.R2CPlan(M, S, multi_level=True)
    info = plan.info()
    assert not info['one_pass']
    return plan, info['workspace_bytes']          # (nothing allocated yet: the overlap-save plan's own)


BATCHED = [((M, S, frames), sk) for M in rc.BATCHED_M for S, frames in rc.BATCHED for sk in rc.SKEWS]


@pytest.mark.parametrize('case, skew', BATCHED, ids=[rc.case_id('three_steps', *c, s) + '-batches221' for c, s in BATCHED])
@both_poisons
def test_three_steps_in_three_batches(case, skew, poison, monkeypatch):
    M, S, frames = case
    monkeypatch.setenv('BBT_R2C_WORK_KIB', rc.work_kib(M))
    x, ref = rc.data(M, S, frames)
    plan, own = _three_step_plan(M, S)
    try:
        _held_to_aligned(('three_steps', case, poison), skew,
                         lambda sk: rc.run(plan, x, ref, poison, sk, rc.case_id('three_steps', M, S, frames, sk)))
        # two groups were allocated, for a call of five
        assert plan.info()['workspace_bytes'] == 2 * 2 * M * 16 + own
    finally:
        plan.close()


@both_poisons
@pytest.mark.parametrize('skew', [(0, 0), (4, 8)], ids=['in0out0', 'in4out8'])
@pytest.mark.parametrize('M', [1024, 10000])
def test_work_buffers_regrow(M, skew, poison, monkeypatch):
    """One plan with the default budget: 1 group, then 5 (free and allocate again), then 1 (kept)."""
    monkeypatch.delenv('BBT_R2C_WORK_KIB', raising=False)
    S = 3
    plan, own = _three_step_plan(M, S)
    try:
        held = []
        for frames, groups in ((1, 1), (6, 5), (1, 5)):
            x, ref = rc.data(M, S, frames)
            out, _ = rc.run(plan, x, ref, poison, skew, f'regrow-M{M}-f{frames}-in{skew[0]}out{skew[1]}')
            assert plan.info()['workspace_bytes'] == 2 * groups * M * 16 + own
            held.append(out)
        assert rc.same_bits(held[0], held[2])
    finally:
        plan.close()


# -- a quiet stream beside a loud one ---------------------------------------------------------------------------
@both_poisons
@pytest.mark.parametrize('skew', [(0, 0), (4, 8)], ids=['in0out0', 'in4out8'])
@pytest.mark.parametrize('route, M', rc.UNEQUAL, ids=[f'{r}-M{m}' for r, m in rc.UNEQUAL])
def test_quiet_streams_beside_loud_ones(route, M, skew, poison):
    S, frames = 4, 2
    x, ref = rc.data(M, S, frames, unequal=True)
    plan = hip.R2CPlan(M, S, multi_level=route == 'three_steps')
    try:
        assert plan.info()['one_pass'] == (route != 'three_steps')
        rc.run(plan, x, ref, poison, skew, f'unequal-{rc.case_id(route, M, S, frames, skew)}', unequal=True)
    finally:
        plan.close()


# -- the stated alignment -------------------------------------------------------------------------------------
@pytest.mark.parametrize('multi', [False, True], ids=['one_pass', 'three_steps'])
def test_misaligned_pointers_are_refused(multi):
    """By return code only: nothing is launched."""
    lib = hip.lib()
    M, S, frames = 1024, 2, 2
    plan = hip.R2CPlan(M, S, multi_level=multi)
    xin = hip.DeviceArray((frames * 2 * M * S + 4,), np.float32)
    out = hip.DeviceArray((frames * M * S + 2,), np.complex64)
    for d_in, d_out, which in ((2, 0, b'in_dev'), (1, 0, b'in_dev'), (0, 4, b'out_dev'), (0, 2, b'out_dev'),
                               (4, 12, b'out_dev')):
        rc_ = lib.bbt_r2c_execute(plan._h, xin.ptr + d_in, out.ptr + d_out, frames, None)
        msg = lib.bbt_last_error()
        assert rc_ != 0 and b'aligned' in msg and which in msg, (d_in, d_out, msg)
    plan.close()
