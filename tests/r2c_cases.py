"""Cases and helpers of test_conversion_guard_gpu.py: `hip.R2CPlan` called directly on guarded arrays
(tests/guard_bands.py), so that the test, not the pool, decides the low bits of the two pointers.

ARRAYS.  The guarded input is shaped (n_frames, 2 M S) float32 and the guarded output (n_frames, M S)
complex64, poisoned throughout: a band is then a whole frame plus 64 words, and the store of a slot that does
not exist -- a dead slot of the last group lands exactly one frame past the end -- is still inside it.  A NaN
or +inf LOADED from beyond the input spreads through the whole transform it enters, so the per-slot comparison
shows stray loads as well as stray stores.

SKEWS (input, output) modulo 16.  `bbt_r2c_execute` asks for 4 and 8 bytes; its one-pass kernels take 16 bytes
an access where S % 4 == 0, 8 where S % 2 == 0, and only if both pointers are 16-byte aligned.

CASES (M, S, frames): the smallest at which each path exists.  S = 5 has groups that straddle a frame on the
one-float path, S = 6 groups whose second pair lies in the next frame at a stream other than 0 on the 8-byte
path, S = 4 and 12 the 16-byte path -- and, off 16, four live neighbouring streams one float at a time."""
import functools

import numpy as np

from guard_bands import Guarded, check_all
from test_conversion_gpu import reference

#: (input, output): the payloads' addresses modulo 16
SKEWS = [(0, 0), (4, 8), (8, 0), (0, 8)]
#: the project's figure for this operation (test_conversion_gpu.check), here per slot
TOL = 2e-6

#: one pass on the kernel compiled for the length (`BBT_G2_KERNEL_R2C`), or with BBT_RTC=0 on `k_r2c_gen`
COMPILED = [(7, 1, 5), (7, 3, 3), (7, 4, 1), (7, 5, 1), (7, 6, 3), (7, 12, 2), (1215, 2, 3), (1215, 6, 1),
            (8192, 1, 3), (8192, 4, 1)]
#: `k_r2c_big<16384, VEC>`
BIG = [(16384, 1, 3), (16384, 2, 3), (16384, 4, 1), (16384, 6, 1)]
#: the cases of COMPILED that run again on the fall-back kernel, and their skews
FALLBACK = [(7, 4, 1), (7, 6, 3), (1215, 2, 3)]
FALLBACK_SKEWS = [(0, 0), (4, 8)]
#: three steps with a budget of two groups and five groups a call: batches of 2, 2 and 1, the last one with
#: 3, 2, 2 and 1 dead slots (n_slot = 17, 18, 18, 19)
BATCHED_M = [7, 1024, 10000]
BATCHED = [(1, 17), (3, 6), (6, 3), (1, 19)]
assert sorted({s * f % 4 for s, f in BATCHED}) == [1, 2, 3] and all((s * f + 3) // 4 == 5 for s, f in BATCHED)
#: one per route at S = 4: streams scaled 1, 2^-10, 1, 2^-10 (slots 0, 1 and 2, 3 are re and im of one transform)
UNEQUAL = [('compiled', 1215), ('big', 16384), ('three_steps', 10000)]
UNEQUAL_SCALE = np.array([1., 2. ** -10, 1., 2. ** -10], np.float32)


def vec_of(S, skew):
    """The access width `bbt_r2c_execute` picks on the one-pass route."""
    aligned = skew == (0, 0)
    return 4 if S % 4 == 0 and aligned else 2 if S % 2 == 0 and aligned else 1


def case_id(route, M, S, frames, skew):
    width = '' if route == 'three_steps' else f'-vec{vec_of(S, skew)}'
    return f'{route}-M{M}-S{S}-f{frames}-in{skew[0]}out{skew[1]}{width}'


def work_kib(M, groups=2):
    """BBT_R2C_WORK_KIB for work buffers of exactly `groups` groups of 16 M bytes."""
    return repr(groups * M * 16 / 1024.)


@functools.lru_cache(maxsize=None)
def data(M, S, frames, unequal=False):
    """(x, float64 reference), shaped (frames, 2 M, S) and (frames, M, S); made once per case."""
    rng = np.random.default_rng(1000 * S + frames + M)
    x = rng.standard_normal((frames, 2 * M, S)).astype(np.float32)
    if unequal:
        x *= UNEQUAL_SCALE
    ref = reference(x.reshape(frames * 2 * M, S), M).reshape(frames, M, S)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def slot_errors(out, ref):
    """||out - ref|| and ||ref|| per slot (frame, stream), in float64."""
    d = out.astype(np.complex128) - ref
    return np.sqrt((np.abs(d) ** 2).sum(1)), np.sqrt((np.abs(ref) ** 2).sum(1))


def run(plan, x, ref, poison, skew, what, unequal=False):
    """One guarded call of `plan` on x (frames, 2 M, S), held to what every run is held to, in this order: the
    real part bit for bit, every slot against the float64 reference, the bands and the input.  Returns the
    output (frames, M, S) and the worst per-slot ratio."""
    frames, M2, S = x.shape
    M = M2 // 2
    gx = Guarded.load(x.reshape(frames, 2 * M * S), poison, skew[0])
    go = Guarded((frames, M * S), np.complex64, poison, skew[1])
    plan.execute(gx.array, go.array, frames)
    out = go.array.to_host().reshape(frames, M, S)
    # 1. Re out is (-1)^m x[2m], bit for bit
    sign = ((-1.) ** np.arange(M)).astype(np.float32).reshape(1, M, 1)
    want_re = np.ascontiguousarray(sign * x[:, ::2])
    got_re = np.ascontiguousarray(out.real)
    assert got_re.view(np.uint32).tobytes() == want_re.view(np.uint32).tobytes(), \
        f'{what}: Re out differs from the signed even samples in {np.count_nonzero(got_re.view(np.uint32) != want_re.view(np.uint32))} places'
    # 2. per slot
    err, norm = slot_errors(out, ref)
    ratio = err / norm
    worst = float(np.nanmax(ratio)) if np.isfinite(ratio).any() else float('nan')
    print(f'{what}: worst per-slot relative L2 {worst:.3e}')
    if unequal:
        assert S == 4
        # the group's four odd-row slots: crosstalk between re and im of a transform scales with the partner
        group = np.sqrt((x[:, 1::2].astype(np.float64) ** 2).sum((1, 2)))          # (frames,)
        quiet = ratio[:, 1::2].max()
        print(f'{what}: quiet-slot error over quiet-slot norm {quiet:.3e}, over its group\'s norm '
              f'{(err[:, 1::2] / group[:, None]).max():.3e}')
        assert (err <= TOL * group[:, None]).all(), (what, err / group[:, None])
        assert (ratio[:, 0::2] <= TOL).all(), (what, ratio)
    else:
        assert (ratio <= TOL).all(), f'{what}: slots (frame, stream) {np.argwhere(~(ratio <= TOL)).tolist()[:8]} miss {TOL}: {ratio}'
    # 3. bands, and the input as it was
    got_x, got_o = check_all([gx, go], what)
    assert got_x.tobytes() == x.tobytes(), f'{what}: the input changed'
    assert got_o.tobytes() == out.tobytes()
    return out, (ratio[:, 1::2].max() if unequal else worst)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()
