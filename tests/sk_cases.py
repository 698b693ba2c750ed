"""Cases shared by test_sk_host.py (which proves, without a GPU, that the NumPy twin follows the
two-level order and that every case flags some blocks, keeps some and has no estimator on a
limit's doorstep) and test_sk_gpu.py (which runs them on the device): `SpectralKurtosis` and
`Excise` (csrc/sk_kernels.hpp) against `rfi.spectral_kurtosis` / `rfi.excise_samples`."""
import functools
from collections import namedtuple

import numpy as np

from baseband_tasks_amd import rfi

Case = namedtuple('Case', 'name sample_shape dtype n samples averaged join limits seed')

C64, F32 = np.dtype(np.complex64), np.dtype(np.float32)

#: the smallest shapes at which each path of the kernels can go wrong.  Explicit limits where the
#: default band cannot flag anything from below (n = 16: its lower edge is negative) or at all
#: (n = 2: the estimator never leaves it).
CASES = [
    Case('scalar_shared_columns_tail', (), C64, 16, 1003, 1., 0, (0.4, 1.9), 1),
    Case('narrow_pol_pairs', (2,), C64, 100, 2050, 1., 1, None, 2),
    Case('odd_width_f32', (3,), F32, 256, 2600, 1., 0, None, 3),
    Case('below_a_segment', (7,), C64, 31, 9 * 31, 1., 0, None, 4),
    Case('one_segment', (7,), C64, 32, 9 * 32, 1., 0, None, 5),
    Case('above_a_segment', (7,), C64, 33, 9 * 33, 1., 0, None, 6),
    Case('minimum_n', (64,), C64, 2, 130, 1., 0, (0.5, 2.0), 7),
    Case('columns_not_a_tile', (96, 2), C64, 64, 640, 1., 1, None, 8),
    Case('prime_width_f32', (1031,), F32, 100, 333, 1., 0, None, 9),
    Case('workload_layout', (1024, 2), C64, 256, 1024, 1., 1, None, 10),
    Case('group_of_three', (5, 3), C64, 1000, 3000, 1., 1, None, 11),
    Case('many_segments', (2,), C64, 4096, 3 * 4096 + 5, 1., 0, None, 12),
    Case('averaged_four_f32', (16,), F32, 128, 1280, 4., 0, None, 13),
    Case('averaged_half_f32', (16,), F32, 128, 1280, 0.5, 0, None, 14),
]
IDS = [c.name for c in CASES]


def limits_of(case):
    return rfi.sk_limits(case.n, 3., case.averaged) if case.limits is None else tuple(np.float32(v) for v in case.limits)


def _noise(rng, case, shape):
    """Gaussian noise: complex voltages, or powers that are the sum of `averaged` complex-voltage
    powers (0.5: the square of one real voltage)."""
    if case.dtype == C64:
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    if case.averaged == 0.5:
        return (rng.standard_normal(shape) ** 2).astype(np.float32)
    k = int(case.averaged)
    z = rng.standard_normal((2 * k,) + shape)
    return (z * z).sum(0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def kinds(case):
    """What each (block, element) holds: 0 noise, 1 a constant-amplitude tone (sk far below 1),
    2 noise whose first max(n // 16, 1) samples are 6 times stronger (sk far above 1)."""
    rng = np.random.default_rng(1000 + case.seed)
    n_block = case.samples // case.n
    k = rng.choice(3, size=(n_block,) + case.sample_shape, p=[0.7, 0.15, 0.15])
    flat = k.reshape(-1)
    flat[:3] = [1, 0, 2]
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def data(case):
    """The samples of a case, (samples,) + sample_shape, read-only."""
    rng = np.random.default_rng(case.seed)
    n, n_block = case.n, case.samples // case.n
    x = _noise(rng, case, (case.samples,) + case.sample_shape)
    body = x[:n_block * n].reshape((n_block, n) + case.sample_shape)
    kind = kinds(case)
    # the tone
    t = np.arange(n).reshape((1, n) + (1,) * len(case.sample_shape))
    phase0 = rng.uniform(0., 2. * np.pi, kind.shape)[:, np.newaxis]
    cycles = rng.uniform(0.05, 0.45, kind.shape)[:, np.newaxis]
    if case.dtype == C64:
        tone = (2. * np.exp(1j * (phase0 + 2. * np.pi * cycles * t))).astype(np.complex64)
    else:
        tone = np.broadcast_to(np.float32(4. * case.averaged) * (1. + cycles), body.shape).astype(np.float32)
    is_tone = np.broadcast_to((kind == 1)[:, np.newaxis], body.shape)
    body[is_tone] = tone[is_tone]
    # the burst
    gain = np.ones((1, n) + (1,) * len(case.sample_shape), np.float32)
    gain[:, :max(n // 16, 1)] = 6. if case.dtype == C64 else 36.
    burst = np.broadcast_to((kind == 2)[:, np.newaxis], body.shape)
    body[burst] = (body * gain)[burst]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(case):
    """(sk, flags, excised) of the NumPy twin, read-only."""
    x = data(case)
    sk = rfi.spectral_kurtosis(x, case.n, case.averaged)
    flags = rfi.excise_flags(sk, limits_of(case), case.join)
    out = rfi.excise_samples(x, case.n, limits_of(case), case.averaged, case.join)
    for a in (sk, flags, out):
        a.setflags(write=False)
    return sk, flags, out


def same_bits(a, b):
    """Equal as bit patterns (so -0 is not +0), except that a NaN equals any NaN: 0 / 0 has no
    sign or payload that IEEE 754 fixes, and the CPU's differs from the GPU's."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == 'c':
        a, b = a.view(a.real.dtype), b.view(b.real.dtype)
    if a.dtype.kind != 'f':
        return np.array_equal(a, b)
    bits = np.dtype(f'u{a.dtype.itemsize}')
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))
