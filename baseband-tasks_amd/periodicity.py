"""Periodicity search on the (time, DM) plane: the fluctuation spectrum of every trial, made in
stacks of short transforms by tasks the package has already or, from 2^15 to 2^22 points, by
`LongSpectra` (`fluctuation_spectra` routes), whitened block by block (`Whiten`), the sums of 1, 2, 4, ... 32 harmonics formed and the best S/N kept per block of
frequency bins (`HarmonicSearch`), the local maxima of which are the candidates
(`harmonic_candidates`, on the host).

The reference has no such tasks, so the rules are this package's, restated in NumPy here
(`whiten_samples`, `harmonic_search_samples`) and computed by csrc/hsum_kernels.hpp.  A block's mean
is one float64 sum in a fixed two-level order; a harmonic sum is ONE float32 accumulator per top
harmonic, the gathered bins added in a fixed order; the winner of a block is the maximum of a total
order.  So every value has one correct bit pattern, whatever the tiling or the chunking.  `LongSpectra`
is the exception: a float32 transform has no single correct rounding, so `long_spectra_samples` is a
float64 yardstick its values are near, and what is exact is that they do not depend on the chunking.
`MedianWhiten` divides by the block median over `median_ratio` instead of the mean, an exact selection
(csrc/rank_kernels.hpp; the twin is `median_whiten_samples`) that lines in the block do not raise.

For pulsars in binaries `Accelerate` goes in front of the spectra: per trial acceleration every block of the
time series is resampled along a parabola, nearest sample, by one integer rule (`accelerate_rows`; the twin is
`accelerate_samples`, csrc/accel_kernels.hpp computes it), and `acceleration_candidates` takes the maxima over
(block, acceleration, trial)."""
import functools
import math
import operator

import numpy as np

from . import hip
from .base import META_ATTRIBUTES, BaseTaskBase, SetAttribute, _stream_rate, check_broadcast_to, simplify_shape
from .channelize import Channelize
from .fourier import check_transform_length
from .device_task import ChunkedDeviceTask
from .functions import Square
from .integration import Integrate
from .search import (_block_median, _check_plane, _check_plane_stream, _init_with_band_of, _local_maxima,
                     _local_maxima_3d, _lone_frequency, _prod)

__all__ = ['fluctuation_spectra', 'LongSpectra', 'long_spectra_samples', 'Whiten', 'whiten_samples', 'MedianWhiten',
           'median_whiten_samples', 'median_ratio', 'LN2', 'HarmonicSearch', 'harmonic_search_samples',
           'harmonic_scales', 'harmonic_candidates', 'Accelerate', 'accelerate_samples', 'accelerate_rows',
           'acceleration_factors', 'acceleration_grid', 'acceleration_candidates', 'SNR', 'OFFSET', 'LEVEL']

#: rows of `HarmonicSearch`'s output: the best S/N of a block, its top harmonic's bin relative to the
#: block, its level L (2^L harmonics)
SNR, OFFSET, LEVEL = 0, 1, 2

SEGMENT = 32          # bins of a segment of Whiten's two-level sums (BBT_HSUM_SEG)
MIN_M, MAX_M = hip.HSUM_MIN_M, hip.HSUM_MAX_M
MAX_N, MAX_LEVELS, MAX_NBIN = hip.HSUM_MAX_N, hip.HSUM_MAX_LEVELS, hip.HSUM_MAX_NBIN
#: the transform lengths of `LongSpectra`: 2^15 ... 2^22
LONG_LENGTHS = tuple(1 << k for k in range(hip.LSPEC_MIN_LOG2, hip.LSPEC_MAX_LOG2 + 1))
_LONG_RANGE = f"a power of two from 2^{hip.LSPEC_MIN_LOG2} = {LONG_LENGTHS[0]} to 2^{hip.LSPEC_MAX_LOG2} = {LONG_LENGTHS[-1]}"


# -- the spectra ----------------------------------------------------------------------------------------
def fluctuation_spectra(plane, n, stack=1):
    """Stacked power spectra of every column of a float32 stream, float32 ``(nspec, n // 2 + 1) +
    plane.sample_shape`` at ``plane.sample_rate / (n * stack)``, every value the average of ``stack``
    consecutive power spectra of ``n`` samples; it never leaves the device.

    For the ``n`` that `Channelize` takes -- up to 8192, and 16384 -- it is ``Integrate(Square(Channelize(
    plane, n)), stack)``, nothing else: the transform of a real stream is an ``rfft`` per element.  For ``n`` a
    power of two from 2^15 to 2^22 it is `LongSpectra`, the same unnormalised transform and the same mean
    over the stack.  Any other ``n`` is a ``ValueError``.

    ``plane`` is usually the (time, DM) plane of `DMTrials`, which has a frequency and no sideband; such
    a stream is relabelled with ``sideband=1`` first on the short route, as the base classes take the two
    together.  Bin ``j`` is fluctuation frequency ``j * bin_width`` with ``bin_width = plane.sample_rate / n``
    in Hz, an attribute of the task returned.  The ``frequency`` `Channelize` attaches to the bins on the
    short route -- the plane's own plus the bin's -- is meaningless here: `HarmonicSearch` drops it.
    `LongSpectra` attaches none."""
    if np.dtype(plane.dtype) != np.dtype(np.float32):
        raise TypeError(f"fluctuation_spectra works on a float32 stream; got {plane.dtype}.")
    n, stack = operator.index(n), operator.index(stack)
    if stack < 1:
        raise ValueError(f"stack must be at least 1, not {stack}.")
    if n in LONG_LENGTHS:
        return LongSpectra(plane, n, stack)
    try:
        check_transform_length(n)
    except ValueError as exc:
        raise ValueError(f"{exc}  Longer spectra (LongSpectra) take n {_LONG_RANGE}.") from None
    if _lone_frequency(plane):
        plane = SetAttribute(plane, frequency=plane.frequency, sideband=1)
    spectra = Integrate(Square(Channelize(plane, n)), stack)
    spectra.bin_width = _stream_rate(plane) / n
    return spectra


def _check_long(n, stack):
    n, stack = operator.index(n), operator.index(stack)
    if n not in LONG_LENGTHS:
        raise ValueError(f"LongSpectra transforms n samples with n {_LONG_RANGE}, not {n}.")
    if not 1 <= stack <= hip.LSPEC_MAX_STACK:
        raise ValueError(f"stack must be 1 ... {hip.LSPEC_MAX_STACK}, not {stack}.")
    return n, stack


def _long_spectra(data, n, stack):
    data = np.asarray(data)
    if data.dtype != np.float32 or data.ndim < 1:
        raise TypeError(f"long_spectra_samples: data must be float32 (N, ...), not {data.dtype} {data.shape}.")
    nspec = data.shape[0] // (n * stack)
    if nspec < 1:
        raise ValueError(f"{data.shape[0]} samples are less than one stack of {stack} transforms of {n}.")
    out = np.empty((nspec, n // 2 + 1) + data.shape[1:], np.float32)
    scale = np.float64(np.float32(1. / stack))
    with np.errstate(all='ignore'):
        for m in range(nspec):
            acc = 0.
            for q in range(stack):
                x = data[(m * stack + q) * n:(m * stack + q + 1) * n].astype(np.float64)
                z = np.fft.rfft(x, axis=0)
                acc = acc + (z.real ** 2 + z.imag ** 2)
            out[m] = acc * scale if stack > 1 else acc
    return out


def long_spectra_samples(data, n, stack=1):
    """NumPy yardstick of `LongSpectra`: float32 ``data`` of shape ``(N,) + s`` gives float32 ``(N // (n *
    stack), n // 2 + 1) + s``; per output spectrum ``m``, bin ``j`` and element ::

        p_q[j] = | sum_t data[(m * stack + q) * n + t] * exp(-2 pi i j t / n) |^2     (np.fft.rfft in float64)
        out[j] = p_0[j]  for stack == 1,  else  (p_0 + ... + p_{stack-1}) * float32(1 / stack)

    all in float64 and rounded to float32 once at the end; a tail shorter than ``n * stack`` is dropped.
    It is the yardstick, not a bit-for-bit twin: a float32 transform has no single correct rounding."""
    n, stack = _check_long(n, stack)
    return _long_spectra(data, n, stack)


# -- the NumPy twins ------------------------------------------------------------------------------------
def _check_spectra(data, who):
    data = np.asarray(data)
    if data.dtype != np.float32 or data.ndim < 2:
        raise TypeError(f"{who}: spectra must be float32 (N, nbin, ...), not {data.dtype} {data.shape}.")
    return data


def _check_m(m):
    m = operator.index(m)
    if not MIN_M <= m <= MAX_M:
        raise ValueError(f"a whitening block must have {MIN_M} ... {MAX_M} bins, not {m}.")
    return m


def _check_skip(skip, nbin, what='skip'):
    skip = operator.index(skip)
    if not 0 <= skip < nbin:
        raise ValueError(f"{what} must be 0 ... {nbin - 1} for spectra of {nbin} bins, not {skip}.")
    return skip


def _whiten_blocks(x):
    """``x``: float32 ``(N, blocks, len) + s``, every ``x[:, b]`` one block."""
    ln = x.shape[2]
    s1 = np.zeros(x.shape[:2] + x.shape[3:], np.float64)
    with np.errstate(all='ignore'):
        for t0 in range(0, ln, SEGMENT):
            a = np.zeros_like(s1)
            for t in range(t0, min(t0 + SEGMENT, ln)):
                a = a + x[:, :, t].astype(np.float64)
            s1 = s1 + a
        mean = s1 / np.float64(ln)
        r = 1. / mean
        r32 = r.astype(np.float32)
        ok = np.isfinite(mean) & (mean > 0.) & np.isfinite(r32)
        z = x * r32[:, :, np.newaxis]
    assert z.dtype == np.float32
    z[np.broadcast_to(~ok[:, :, np.newaxis], z.shape)] = 0.
    return z


def whiten_samples(data, m, skip=1):
    """NumPy restatement of the `Whiten` kernel.

    ``data``: float32 ``(N, nbin) + s``.  Bins below ``skip`` come out ``+0``; from ``skip`` on the bins are
    cut into blocks of ``m``, the last one whatever is left.  Per spectrum, block and element, in float64
    with every step rounded once: ``S1 = sum x`` in the two-level order of `search.standardize_samples`
    -- segments of 32 bins summed in bin order from the block's first bin, the segment sums added in
    segment order -- then ::

        mean = S1 / len;  r = 1 / mean;  z = x * float32(r)          (float32: one multiply)

    A block whose ``mean`` is not finite or not ``> 0``, or whose ``float32(r)`` is not finite -- all zero,
    holding a NaN or an Inf, of negative mean, of a denormal mean -- is ``+0`` throughout."""
    data, m = _check_spectra(data, 'whiten_samples'), _check_m(m)
    nbin = data.shape[1]
    skip = _check_skip(skip, nbin)
    out = np.zeros(data.shape, np.float32)
    n_full = (nbin - skip) // m
    if n_full:
        x = data[:, skip:skip + n_full * m].reshape((data.shape[0], n_full, m) + data.shape[2:])
        out[:, skip:skip + n_full * m] = _whiten_blocks(x).reshape((data.shape[0], n_full * m) + data.shape[2:])
    if skip + n_full * m < nbin:
        out[:, skip + n_full * m:] = _whiten_blocks(data[:, np.newaxis, skip + n_full * m:])[:, 0]
    return out


#: the median of an exponential distribution of unit mean
LN2 = math.log(2.)


#: the most averaged powers `median_ratio` computes the median for: the longest stack of `LongSpectra`
MAX_AVERAGED = hip.LSPEC_MAX_STACK


@functools.lru_cache(maxsize=64)
def _erlang_median_ratio(k):
    """``x / k`` with ``x`` the root of the Erlang CDF ``1 - sum_{j<k} exp(j log x - x - log j!) = 1/2``.  Every
    term is formed in log space, so nothing overflows however large ``k``; the exponents, up to 1.4e7 for
    ``k`` = 2^20 and needed to 1e-12, are formed in extended precision (`numpy.longdouble`).  Terms more than
    40 sqrt(k) below the peak at ``j = x`` are below ``exp(-800)`` of it and are left out.  The median of a
    gamma distribution of shape ``k`` lies in ``(k - 1/3, k)``, so 64 bisections of ``[k - 1, k]`` end at
    neighbouring float64.  One step is one vectorised pass over at most ``40 sqrt(k)`` terms."""
    first = max(0, int(k - 1 - 40. * math.sqrt(k)))
    j = np.arange(k, dtype=np.longdouble)
    log_fact = np.concatenate([[np.longdouble(0.)], np.cumsum(np.log(j[1:]))])[first:]
    j = j[first:]

    def cdf(x):
        x = np.longdouble(x)
        return 1. - float(np.exp(j * np.log(x) - x - log_fact).sum())

    lo, hi = k - 1., float(k)
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        if cdf(mid) < 0.5:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi) / k


def median_ratio(averaged=1):
    """The median, in units of the mean, of the average of ``averaged`` exponential powers -- what
    ``stack=averaged`` of `fluctuation_spectra` makes of noise: ``log(2)`` for 1, and for an integer ``k`` from 2
    to `MAX_AVERAGED` = 2^20 ``x / k`` with ``x`` the root of ``1 - exp(-x) sum_{j<k} x^j / j! = 1/2`` (the Erlang
    distribution), found by 64 bisections of ``[k - 1, k]`` with the terms formed in log space, in extended
    precision (64 passes over at most ``40 sqrt(k)`` terms; results are remembered).  For anything else -- a
    fraction, more powers -- pass ``ratio=`` to `MedianWhiten` yourself; ``1 - 1 / (3 k)`` is within ``8 / (405
    k^2)`` of it."""
    try:
        k = operator.index(averaged)
    except TypeError:
        value = float(averaged)
        if not math.isfinite(value) or value != int(value):
            raise ValueError(f"median_ratio knows the median for a whole number of averaged powers, not "
                             f"{averaged}: pass ratio= yourself.") from None
        k = int(value)
    if not 1 <= k <= MAX_AVERAGED:
        raise ValueError(f"averaged must be 1 ... {MAX_AVERAGED}, not {averaged}: pass ratio= yourself.")
    return LN2 if k == 1 else _erlang_median_ratio(k)


def _check_ratio(ratio):
    ratio = float(ratio)
    if not 0. < ratio < math.inf:
        raise ValueError(f"ratio must be finite and > 0, not {ratio}.")
    return ratio


def _median_whiten_blocks(x, ratio):
    """``x``: float32 ``(N, blocks, len) + s``, every ``x[:, b]`` one block."""
    flat = x.reshape((x.shape[0] * x.shape[1],) + x.shape[2:])
    med = _block_median(flat).reshape(x.shape[:2] + x.shape[3:])
    flagged = ~np.isfinite(x).all(axis=2)
    with np.errstate(all='ignore'):
        mean = med.astype(np.float64) / np.float64(ratio)
        r32 = (1. / mean).astype(np.float32)
        ok = ~flagged & np.isfinite(mean) & (mean > 0.) & np.isfinite(r32)
        z = x * r32[:, :, np.newaxis]
    assert z.dtype == np.float32
    z[np.broadcast_to(~ok[:, :, np.newaxis], z.shape)] = 0.
    return z


def median_whiten_samples(data, m, skip=1, ratio=LN2):
    """NumPy restatement of the `MedianWhiten` kernel.

    ``data``: float32 ``(N, nbin) + s``.  Bins below ``skip`` come out ``+0``; from ``skip`` on the bins are
    cut into blocks of ``m``, the last one whatever is left, exactly as `whiten_samples` cuts them.  Per
    spectrum, block and element, with ``med`` the median of the block by the rule of
    `search.block_median_mad_samples` (the keys sorted; the two middle values averaged in float64) ::

        mean = float64(med) / ratio;  r = 1 / mean;  z = x * float32(r)          (float32: one multiply)

    A block that holds a NaN or an Inf, one whose ``mean`` is not finite or not ``> 0``, and one whose
    ``float32(r)`` is not finite are ``+0`` throughout."""
    data, m = _check_spectra(data, 'median_whiten_samples'), _check_m(m)
    nbin = data.shape[1]
    skip, ratio = _check_skip(skip, nbin), _check_ratio(ratio)
    out = np.zeros(data.shape, np.float32)
    n_full = (nbin - skip) // m
    if n_full:
        x = data[:, skip:skip + n_full * m].reshape((data.shape[0], n_full, m) + data.shape[2:])
        out[:, skip:skip + n_full * m] = _median_whiten_blocks(x, ratio).reshape((data.shape[0], n_full * m) + data.shape[2:])
    if skip + n_full * m < nbin:
        out[:, skip + n_full * m:] = _median_whiten_blocks(data[:, np.newaxis, skip + n_full * m:], ratio)[:, 0]
    return out


def _check_search(n, n_levels):
    n, n_levels = operator.index(n), operator.index(n_levels)
    if not 1 <= n <= MAX_N:
        raise ValueError(f"a search block must have 1 ... {MAX_N} bins, not {n}.")
    if not 1 <= n_levels <= MAX_LEVELS:
        raise ValueError(f"n_levels must be 1 ... {MAX_LEVELS} (up to {1 << (MAX_LEVELS - 1)} harmonics), not "
                         f"{n_levels}.")
    return n, n_levels


def harmonic_scales(averaged=1.):
    """``c_L = float32(sqrt(averaged / 2^L))`` for ``L < 6``: the square root in float64, rounded once.
    The sum of ``2^L`` values that are each the average of ``averaged`` exponential powers of unit mean
    has mean ``2^L`` and standard deviation ``sqrt(2^L / averaged)``."""
    averaged = float(averaged)
    with np.errstate(all='ignore'):
        c = np.sqrt(np.float64(averaged) / 2. ** np.arange(MAX_LEVELS)).astype(np.float32)
    if not (averaged > 0. and np.all(np.isfinite(c)) and np.all(c > 0.)):
        raise ValueError(f"averaged must be > 0 (and its scales finite float32), not {averaged}.")
    return c


def harmonic_search_samples(data, n, n_levels, averaged=1., lo=1):
    """NumPy restatement of the `HarmonicSearch` kernel.

    ``data``: float32 ``(N, nbin) + s``.  Per spectrum and element there is one float32 accumulator per
    ``j``: ``T_0[j] = p[j]`` and, level by level, ``T_L[j] = T_{L-1}[j] + p[(j i + 2^(L-1)) >> L]`` for ``i =
    1, 3, ... 2^L - 1`` in ascending order, one rounded add each; ``snr_L[j] = (T_L[j] - float32(2^L)) *
    c_L`` with ``c = harmonic_scales(averaged)``, one rounded subtract and one rounded multiply.  ``(L, j)``
    is present iff its fundamental's bin -- ``j`` for ``L = 0``, ``(j + 2^(L-1)) >> L`` otherwise -- is at least
    ``lo``.  For block ``b`` of ``n`` bins (the last may be short) the winner over the present ``(L, j)`` with
    ``L < n_levels`` and ``j`` in the block is the largest S/N, among equals the smaller ``L``, then the smaller
    ``j``; a NaN never wins.  Returns float32 ``(N, ceil(nbin / n), 3) + s``: row `SNR` the winner's S/N, row
    `OFFSET` its ``j - b n``, row `LEVEL` its ``L``; ``(-inf, 0, 0)`` where a block has nothing present that
    is not NaN."""
    data = _check_spectra(data, 'harmonic_search_samples')
    n, n_levels = _check_search(n, n_levels)
    N, nbin = data.shape[:2]
    if not 1 <= nbin <= MAX_NBIN:
        raise ValueError(f"a spectrum must have 1 ... {MAX_NBIN} bins, not {nbin}.")
    lo = _check_skip(lo, nbin, 'lo')
    c = harmonic_scales(averaged)
    rest = data.shape[2:]
    nb = -(-nbin // n)
    j = np.arange(nbin)
    best = np.full((N, nb) + rest, -np.inf, np.float32)
    offset = np.zeros((N, nb) + rest, np.int64)
    level = np.zeros((N, nb) + rest, np.int64)
    have = np.zeros((N, nb) + rest, bool)
    acc = data.copy()
    absent = np.full((N, nb * n - nbin) + rest, np.nan, np.float32)
    with np.errstate(all='ignore'):
        for L in range(n_levels):
            half = (1 << L) >> 1
            for i in range(1, 1 << L, 2):
                acc = acc + data[:, (j * i + half) >> L]
            snr = (acc - np.float32(1 << L)) * c[L]
            assert snr.dtype == np.float32
            present = ((j + half) >> L) >= lo
            snr[:, ~present] = np.nan                      # (absent: never a winner)
            snr = np.concatenate([snr, absent], axis=1).reshape((N, nb, n) + rest)
            valid = ~np.isnan(snr)
            filled = np.where(valid, snr, np.float32(-np.inf))
            top = filled.max(axis=2)
            first = (valid & (filled == top[:, :, np.newaxis])).argmax(axis=2)    # the smallest j among equals
            value = np.take_along_axis(snr, first[:, :, np.newaxis], axis=2)[:, :, 0]
            better = valid.any(axis=2) & (~have | (value > best))                # (not >=: the smaller L stays)
            best = np.where(better, value, best)
            offset = np.where(better, first, offset)
            level = np.where(better, L, level)
            have |= better
    out = np.empty((N, nb, 3) + rest, np.float32)
    out[:, :, SNR], out[:, :, OFFSET], out[:, :, LEVEL] = best, offset, level
    return out


def harmonic_candidates(best, n, threshold, bin_width=None):
    """The local maxima of one spectrum's `HarmonicSearch` result above a threshold (host, NumPy).

    ``best``: ``(blocks, 3, ndm)``, one sample as read from ``HarmonicSearch(spectra, n, ...)``.  A cell ``(b,
    d)`` is a candidate if its S/N is ``>= threshold``, none of its up to 8 neighbours in (block, trial) has
    a larger S/N, and no neighbour with an equal S/N comes before it in ``(b, d)`` raster order: the rule
    of `search.boxcar_candidates`.  Returns a structured array with fields ``bin`` (float64: ``(b n +
    offset) / 2^L``, the fundamental in bins of the spectrum), ``trial``, ``harmonics`` (``2^L``), ``snr`` and,
    if ``bin_width`` (Hz) is given, ``frequency = bin * bin_width``; sorted by descending ``snr``, then ``bin``,
    then ``trial``.  Nothing is merged across trials or harmonics."""
    best = np.asarray(best)
    n = _check_search(n, 1)[0]
    if best.ndim != 3 or best.shape[1] != 3:
        raise ValueError(f"best must be (blocks, 3, ndm), one sample of HarmonicSearch, not {best.shape}.")
    snr = best[:, SNR].astype(np.float32)
    b, d = _local_maxima(snr, threshold)
    fields = [('bin', np.float64), ('trial', np.int64), ('harmonics', np.int64), ('snr', np.float32)]
    if bin_width is not None:
        fields.append(('frequency', np.float64))
    out = np.empty(b.shape[0], np.dtype(fields))
    harmonics = np.int64(1) << best[b, LEVEL, d].astype(np.int64)
    out['bin'] = (b * n + best[b, OFFSET, d].astype(np.int64)) / harmonics
    out['trial'] = d
    out['harmonics'] = harmonics
    out['snr'] = snr[b, d]
    if bin_width is not None:
        out['frequency'] = out['bin'] * float(bin_width)
    return out[np.lexsort((out['trial'], out['bin'], -out['snr'].astype(np.float64)))]


# -- acceleration trials: the rule in NumPy ------------------------------------------------------------------
#: the speed of light, m / s
C_LIGHT = 299792458.
ACCEL_MIN_N, ACCEL_MAX_N, ACCEL_MAX_TRIALS = hip.ACCEL_MIN_N, hip.ACCEL_MAX_N, hip.ACCEL_MAX_TRIALS


def acceleration_factors(accelerations, sample_rate):
    """``k_j = a_j / (2. * 299792458. * sample_rate)``, float64, evaluated in exactly this order:
    ``accelerations`` in m / s^2 and ``sample_rate`` in Hz give the factors of `accelerate_rows` in 1 / sample."""
    a = np.array(accelerations, dtype=np.float64, ndmin=1)
    if a.ndim != 1 or not 1 <= a.shape[0] <= ACCEL_MAX_TRIALS:
        raise ValueError(f"the trial accelerations must be a 1-D sequence of 1 ... {ACCEL_MAX_TRIALS} values.")
    if not np.all(np.isfinite(a)):
        raise ValueError("the trial accelerations must be finite.")
    rate = float(sample_rate)
    if not (np.isfinite(rate) and rate > 0.):
        raise ValueError(f"the sample rate must be positive and finite, not {sample_rate}.")
    return a / (2. * C_LIGHT * rate)


def _check_accel(n, factors):
    n = operator.index(n)
    if not ACCEL_MIN_N <= n <= ACCEL_MAX_N:
        raise ValueError(f"a block of Accelerate must have {ACCEL_MIN_N} ... 2^24 samples, not {n}.")
    k = np.array(factors, dtype=np.float64, ndmin=1)
    if k.ndim != 1 or not 1 <= k.shape[0] <= ACCEL_MAX_TRIALS:
        raise ValueError(f"there must be 1 ... {ACCEL_MAX_TRIALS} trials in a 1-D sequence.")
    bad = ~np.isfinite(k) | ~(np.abs(k) * np.float64(n) <= .25)
    if bad.any():
        j = int(np.argmax(bad))
        raise ValueError(f"trial {j}: the factor {k[j]} is beyond |k| n <= 1/4 for n = {n} (|a| T / 2c <= 1/4).")
    return n, k


def _accel_src(n, k, i):
    """The rule for one row: python ints and one float64 product."""
    return i + int(np.rint(np.float64(k) * np.float64(i * (i - n))))


def _accel_window(n, k_min, k_max, g0, g1):
    """The input rows ``[lo, hi]`` (global, inclusive) that output rows ``g0 <= g1`` need over all trials."""
    q0, q1 = g0 // n, g1 // n
    return q0 * n + _accel_src(n, k_max, g0 - q0 * n), q1 * n + _accel_src(n, k_min, g1 - q1 * n)


def accelerate_rows(n, factors):
    """The input row of every output row of a block: int64 ``(A, n)`` ::

        src[j, i] = i + int64(rint(factors[j] * float64(i * (i - n))))

    ``i * (i - n)`` in int64 (exact), ONE float64 multiply, round half to even, an integer add.  The parabola
    is zero at both ends of the block.  ``|factors[j]| * n <= 1/4`` or ``ValueError``: then ``src`` stays in ``[0,
    n - 1]``, does not decrease with ``i``, steps by 0, 1 or 2, and for a fixed ``i`` does not increase with the
    factor."""
    n, k = _check_accel(n, factors)
    i = np.arange(n, dtype=np.int64)
    p = (i * (i - n)).astype(np.float64)
    return i + np.rint(k[:, np.newaxis] * p).astype(np.int64)


def accelerate_samples(data, factors, n):
    """NumPy twin of `Accelerate`, bit for bit: float32 ``data`` of shape ``(N,) + s`` gives float32 ``(N // n *
    n, A) + s`` with ``out[q n + i, j] = data[q n + accelerate_rows(n, factors)[j, i]]``, the 32 bits copied; a
    tail shorter than ``n`` is dropped."""
    data = _check_plane(data, 'accelerate_samples')
    src = accelerate_rows(n, factors)
    n = src.shape[1]
    nb = data.shape[0] // n
    if nb < 1:
        raise ValueError(f"{data.shape[0]} samples are less than one block of {n}.")
    bits = np.ascontiguousarray(data[:nb * n]).view(np.uint32).reshape((nb, n) + data.shape[1:])
    out = bits[:, src.T]                                         # (nb, n, A) + s
    return out.reshape((nb * n, src.shape[0]) + data.shape[1:]).view(np.float32)


def acceleration_grid(a_max, n, sample_rate, tol=1.):
    """The symmetric grid of trial accelerations ``j * da``, ``|j| <= ceil(a_max / da)``, with ``da = 8 c
    sample_rate tol / n^2`` (m / s^2): neighbouring trials then differ by ``tol`` samples in the middle of a
    block of ``n``, as ``dk n^2 / 4 = tol``.  ``ValueError`` if that is more than 4096 trials."""
    n = operator.index(n)
    a_max, rate, tol = float(a_max), float(sample_rate), float(tol)
    if not (ACCEL_MIN_N <= n <= ACCEL_MAX_N and np.isfinite(a_max) and a_max >= 0. and np.isfinite(rate) and rate > 0.
            and np.isfinite(tol) and tol > 0.):
        raise ValueError("acceleration_grid needs n = 2 ... 2^24, a_max >= 0, sample_rate > 0 and tol > 0.")
    step = 8. * C_LIGHT * rate * tol / (float(n) * float(n))
    reach = int(np.ceil(a_max / step))
    if 2 * reach + 1 > ACCEL_MAX_TRIALS:
        raise ValueError(f"{2 * reach + 1} trials of {step} m/s^2 up to {a_max}: more than {ACCEL_MAX_TRIALS}.")
    return np.arange(-reach, reach + 1, dtype=np.float64) * step


def acceleration_candidates(best, n, threshold, bin_width=None, accelerations=None):
    """The local maxima of one spectrum's `HarmonicSearch` result over acceleration trials (host, NumPy).

    ``best``: ``(blocks, 3, A, ndm)``, one sample as read from ``HarmonicSearch(... Accelerate(plane, ...) ...,
    n, ...)``.  A cell ``(b, a, d)`` is a candidate if its S/N is ``>= threshold``, none of its up to 26
    neighbours in (block, acceleration, trial) has a larger S/N, and no neighbour with an equal S/N comes
    before it in ``(b, a, d)`` raster order: the rule of `harmonic_candidates` with one more axis.  Returns a
    structured array with the fields of `harmonic_candidates` -- ``bin``, ``trial``, ``harmonics``, ``snr`` and, if
    ``bin_width`` (Hz) is given, ``frequency`` -- then ``acc``, the index of the acceleration trial, and, if
    ``accelerations`` (the ``A`` trial values) are given, ``acceleration``; sorted by descending ``snr``, then
    ``bin``, then ``acc``, then ``trial``.  Nothing is merged across trials or harmonics."""
    best = np.asarray(best)
    n = _check_search(n, 1)[0]
    if best.ndim != 4 or best.shape[1] != 3:
        raise ValueError(f"best must be (blocks, 3, A, ndm), one sample of HarmonicSearch, not {best.shape}.")
    if accelerations is not None:
        accelerations = np.asarray(accelerations, dtype=np.float64)
        if accelerations.shape != (best.shape[2],):
            raise ValueError(f"{best.shape[2]} trials need as many accelerations, not {accelerations.shape}.")
    snr = best[:, SNR].astype(np.float32)
    b, a, d = _local_maxima_3d(snr, threshold)
    fields = [('bin', np.float64), ('trial', np.int64), ('harmonics', np.int64), ('snr', np.float32)]
    if bin_width is not None:
        fields.append(('frequency', np.float64))
    fields.append(('acc', np.int64))
    if accelerations is not None:
        fields.append(('acceleration', np.float64))
    out = np.empty(b.shape[0], np.dtype(fields))
    harmonics = np.int64(1) << best[b, LEVEL, a, d].astype(np.int64)
    out['bin'] = (b * n + best[b, OFFSET, a, d].astype(np.int64)) / harmonics
    out['trial'] = d
    out['harmonics'] = harmonics
    out['snr'] = snr[b, a, d]
    if bin_width is not None:
        out['frequency'] = out['bin'] * float(bin_width)
    out['acc'] = a
    if accelerations is not None:
        out['acceleration'] = accelerations[a]
    return out[np.lexsort((out['trial'], out['acc'], out['bin'], -out['snr'].astype(np.float64)))]


# -- the tasks ------------------------------------------------------------------------------------------
def _check_spectra_stream(ih, who):
    _check_plane_stream(ih, who)
    if len(ih.shape) < 2:
        raise ValueError(f"{who} needs a bin axis: samples of shape (nbin, ...).")


class _BlockWhiten(ChunkedDeviceTask, BaseTaskBase):
    """What `Whiten` and `MedianWhiten` share: blocks of ``m`` bins from bin ``skip`` on, chunks of whole
    spectra.  A subclass launches its kernel."""

    #: input bytes fetched at most per `fetch_device` call and launch (assignable); a chunk is a
    #: whole number of spectra, one at least
    whiten_budget = 1 << 29

    def __init__(self, ih, m, skip=1, *, samples_per_frame=None):
        _check_spectra_stream(ih, type(self).__name__)
        self.m = _check_m(m)
        self._nbin = ih.shape[1]
        self.skip = _check_skip(skip, self._nbin)
        self._n_elem = _prod(ih.shape[2:])
        if samples_per_frame is None:
            samples_per_frame = max(min(operator.index(ih.samples_per_frame), ih.shape[0]), 1)
        _init_with_band_of(self, ih, samples_per_frame=operator.index(samples_per_frame), dtype=np.float32)

    def _chunk_size(self):
        return max(1, int(self.whiten_budget) // (self._nbin * self._n_elem * 4))


class Whiten(_BlockWhiten):
    """Divide every block of ``m`` frequency bins of every spectrum by its own mean, per element.

    Parameters
    ----------
    ih : stream
        float32 spectra of shape ``(N, nbin) + s``: the bin axis is the first sample axis -- usually
        `fluctuation_spectra` of the (time, DM) plane.
    m : int
        Bins of a block, 2 ... 65536, counted from bin ``skip``; the last block is whatever is left.
    skip : int, optional
        Bins below it come out ``+0``: the DC bin by default.  ``0 <= skip < nbin``.
    samples_per_frame : int, optional
        Spectra per frame.  Default: that of ``ih``.

    Shape, sample rate, start time and metadata are those of ``ih``.  The mean is the plain mean of
    the block, summed in float64 in a fixed order, and the values equal `whiten_samples` bit for
    bit.  A block that is all zero, holds a NaN or an Inf, or has a negative or a denormal mean comes
    out as +0.  There is no median and no running fit: a bright line raises the mean of its own block,
    and red noise steeper than a block is not flattened inside it.  `MedianWhiten` is the median-based
    counterpart."""

    def _launch(self, x, start, count, out, c0, c1):
        hip.hsum_whiten(x, self._nbin, self._n_elem, self.m, self.skip, out=out)


class MedianWhiten(_BlockWhiten):
    """Divide every block of ``m`` frequency bins of every spectrum by the noise mean its own median
    implies, per element: `Whiten` with an estimate the pulsar's harmonics and birdies cannot raise.

    Parameters
    ----------
    ih : stream
        float32 spectra of shape ``(N, nbin) + s``: the bin axis is the first sample axis -- usually
        `fluctuation_spectra` of the (time, DM) plane.
    m : int
        Bins of a block, 2 ... 65536, counted from bin ``skip``; the last block is whatever is left.
    skip : int, optional
        Bins below it come out ``+0``: the DC bin by default.  ``0 <= skip < nbin``.
    averaged : int, optional
        Power spectra averaged into every value (``stack`` of `fluctuation_spectra`): it fixes the ratio
        of the noise's median to its mean, `median_ratio`.  Default 1: exponential powers, ``log(2)``.
    ratio : float, optional
        That ratio itself, finite and ``> 0``, for any other noise; not together with ``averaged``.
    samples_per_frame : int, optional
        Spectra per frame.  Default: that of ``ih``.

    Shape, sample rate, start time and metadata are those of ``ih``.  Per block ``mean = float64(med) /
    ratio`` with ``med`` the block's median, an exact selection on the GPU (the mean of the two middle
    values for an even count), and ``z = x * float32(1 / mean)``: the values equal `median_whiten_samples`
    bit for bit, whatever the route, the tiling or the chunking.  A block that holds a NaN or an Inf, or
    whose median is not ``> 0`` or denormal, comes out as +0.  There is no running median and no fit: red
    noise steeper than a block is not flattened inside it."""

    def __init__(self, ih, m, skip=1, *, averaged=1, ratio=None, samples_per_frame=None):
        super().__init__(ih, m, skip, samples_per_frame=samples_per_frame)
        if ratio is not None and averaged != 1:
            raise ValueError("give averaged or ratio, not both: ratio is what averaged stands for.")
        self.ratio = median_ratio(averaged) if ratio is None else _check_ratio(ratio)
        self._ratio_given = ratio is not None
        self.averaged = averaged

    def _launch(self, x, start, count, out, c0, c1):
        hip.rank_whiten(x, self._nbin, self._n_elem, self.m, self.skip, self.ratio, out=out)

    def _repr_item(self, key, default, value=None):
        if key == 'ratio' and not self._ratio_given:
            return None
        return super()._repr_item(key, default, value)


class HarmonicSearch(ChunkedDeviceTask, BaseTaskBase):
    """The best harmonic-sum S/N in every block of ``n`` frequency bins, per spectrum and element: a
    pulsar's narrow pulse spreads its power over many harmonics, so sums of 1, 2, 4, ... harmonics are
    formed and the best one kept.

    Parameters
    ----------
    ih : stream
        float32 spectra of shape ``(N, nbin) + s``, ideally of unit mean -- usually ``Whiten(
        fluctuation_spectra(plane, ...), m)``.  ``nbin`` is 1 ... 2^24.
    n : int
        Bins folded into one output block, 1 ... 65536; the last block of a spectrum may be short.
    n_levels : int, optional
        ``K``, 1 ... 6: sums of ``2^L`` harmonics for ``L < K``, up to 32.  Default 5.
    averaged : float, optional
        ``Nd > 0``: the independent powers averaged into each value (``stack`` of `fluctuation_spectra`).
    lo : int, optional
        Lowest bin a fundamental may lie in, ``0 <= lo < nbin``.  Default 1: not the DC bin.
    samples_per_frame : int, optional
        Spectra per frame.  Default: that of ``ih``.

    The output is float32 ``(N, ceil(nbin / n), 3) + s`` with the rate, start time and framing of
    ``ih``.  With ``j`` the bin of the highest harmonic, ``T_0[j] = ih[j]`` and ``T_L[j] = T_{L-1}[j] + ih[(j i +
    2^(L-1)) >> L]`` for ``i = 1, 3, ... 2^L - 1`` -- the bins ``round_half_up(j i / 2^L)``, ``i = 1 ... 2^L``, of the
    harmonics of a fundamental at ``j / 2^L`` bins, all at most ``j`` -- and ``snr_L[j] = (T_L[j] - 2^L) * c_L``
    with ``c_L = float32(sqrt(averaged / 2^L))`` (`harmonic_scales`).  For block ``b`` row `SNR` is the largest
    ``snr_L[j]`` over the levels and the bins ``b n <= j < (b + 1) n`` whose fundamental's bin (``j`` for ``L = 0``,
    ``(j + 2^(L-1)) >> L`` otherwise) is at least ``lo``, row `OFFSET` is ``j - b n`` and row `LEVEL` is ``L`` of that
    winner, as floats.  Among equal S/N the smaller ``L`` wins, then the smaller ``j``; a NaN never wins; a
    block with nothing else gives ``(-inf, 0, 0)``.  Every sum is one float32 accumulator, the bins added in
    ascending ``i`` level by level, so values equal `harmonic_search_samples` bit for bit whatever the
    tiling or the chunking.

    The S/N is ``(sum - mean) / sd`` of the sum for noise of unit mean, NOT a Gaussian significance: for
    unstacked exponential noise a single bin exceeds ``x`` with probability ``exp(-(x + 1))``, far more
    often than a normal deviate, and only sums of many powers approach the normal tail.

    Metadata that vary along the bin axis are dropped -- the per-bin ``frequency`` and with it the
    ``sideband``, a per-bin ``polarization`` -- and those that do not are kept.  `harmonic_candidates` turns
    one sample of this task into a candidate list.  Nothing leaves HBM: one kernel gathers the harmonics
    of each ``j`` straight from the spectrum, with no scratch."""

    #: bytes of input and output at most per `fetch_device` call and launch (assignable); a chunk is a
    #: whole number of spectra, one at least
    hsum_budget = 1 << 29

    def __init__(self, ih, n, n_levels=5, averaged=1., lo=1, *, samples_per_frame=None):
        _check_spectra_stream(ih, 'HarmonicSearch')
        self.n, self.n_levels = _check_search(n, n_levels)
        self._nbin = nbin = ih.shape[1]
        if not 1 <= nbin <= MAX_NBIN:
            raise ValueError(f"a spectrum must have 1 ... {MAX_NBIN} bins, not {nbin}.")
        self.lo = _check_skip(lo, nbin, 'lo')
        self.averaged = float(averaged)
        self.scales = harmonic_scales(self.averaged)
        rest = tuple(ih.shape[2:])
        self._n_elem = _prod(rest)
        self._nb = -(-nbin // self.n)
        if samples_per_frame is None:
            samples_per_frame = max(min(operator.index(ih.samples_per_frame), ih.shape[0]), 1)
        kept = {}
        for attr in META_ATTRIBUTES:
            value = getattr(ih, attr, None)
            if value is not None:
                full = check_broadcast_to(value, tuple(ih.shape[1:]))
                if np.all(full == full[:1]):                      # (the same in every bin)
                    kept[attr] = simplify_shape(np.asanyarray(full[0]))
        if 'frequency' not in kept:
            kept.pop('sideband', None)
        _init_with_band_of(self, ih, shape=(ih.shape[0], self._nb, 3) + rest,
                           samples_per_frame=operator.index(samples_per_frame), dtype=np.float32)
        if kept:
            self.meta['__attributes__'] = kept
        else:
            self.meta.pop('__attributes__', None)

    def _check_shape(self, value):
        # (the inherited metadata describe the bins; they are replaced once the stream is set up)
        return simplify_shape(np.asanyarray(value))

    def _chunk_size(self):
        row = self._n_elem * 4
        return max(1, int(self.hsum_budget) // ((self._nbin + 3 * self._nb) * row))

    def _make_plan(self):
        return hip.HsumPlan(self._nbin, self.n, self.n_levels, self.lo, self._n_elem, self.scales)

    def _launch(self, x, start, count, out, c0, c1):
        self._plan.execute(x, count, out)


class LongSpectra(ChunkedDeviceTask, BaseTaskBase):
    """Power spectra of ``n`` = 2^15 ... 2^22 samples of every column of a float32 stream: the whole
    pointing in one coherent transform, where `Channelize` stops at 16384 points.

    Parameters
    ----------
    ih : stream
        float32 of shape ``(N,) + s`` -- usually the (time, DM) plane of `DMTrials`, `Standardize`d or
        not.  A plane with a frequency and no sideband is taken as it is.
    n : int
        Samples of a transform: a power of two, 2^15 ... 2^22.
    stack : int, optional
        Consecutive spectra averaged into one output spectrum.  ``N >= n * stack``.
    samples_per_frame : int, optional
        Output spectra per frame.  Default 1.

    The output is float32 ``(N // (n * stack), n // 2 + 1) + s`` at ``ih.sample_rate / (n * stack)`` from the
    start time of ``ih``; a tail shorter than ``n * stack`` is dropped.  Per output spectrum ``m``, bin ``j`` and
    element, ``p_q[j] = |sum_t ih[(m stack + q) n + t] exp(-2 pi i j t / n)|^2`` and ``out = (p_0 + ... +
    p_{stack-1}) * float32(1 / stack)``, float32 adds in ascending ``q`` (no scaling for ``stack == 1``): the
    unnormalised transform and the mean of `fluctuation_spectra`'s short route.  Bin ``j`` is fluctuation
    frequency ``j * bin_width``, ``bin_width = ih.sample_rate / n`` in Hz (an attribute).  Metadata of ``ih``
    describe ``s`` and are kept; no per-bin ``frequency`` is attached.  `Whiten`, `HarmonicSearch` and
    `harmonic_candidates` take the result as it is.

    How it is made (csrc/lspec_kernels.hpp): columns ``2c, 2c + 1`` are one complex stream, transformed by
    a four-step transform ``n = n1 n2`` in two passes through a scratch of ``8 n`` bytes per column pair, and
    untangled, detected and stacked in the second pass; the complex spectra are never stored and an odd
    last column pairs with zeros.  A launch takes as many pairs as fit `spectra_budget`, one at least; the
    pairing is fixed, so no value depends on the budget, on the framing or on where a read starts.  Values
    are those of a float32 transform with twiddles from float64 tables: near `long_spectra_samples`, not
    bit-equal to it.  Two consequences of the pairing: the rounding error of a column scales with the
    larger of its and its partner's norm (about 1e-7 of that per bin, so a column 1000 times fainter than
    its neighbour keeps 1e-4 of its own); and a NaN or an Inf in a column makes that column's spectrum
    and its partner's non-finite, and changes no other column by a bit.

    What it costs: the first pass of a long transform touches every sample, so the ``n * stack`` samples
    of ALL elements behind one output spectrum are fetched in one piece: ``4 n n_elem`` bytes resident per
    transform, 8 GiB for 2^22 x 512, beside the scratch and the output."""

    #: bytes of scratch a launch may use (assignable): 8 n bytes per column pair, one pair at least
    spectra_budget = hip.LSPEC_BUDGET

    def __init__(self, ih, n, stack=1, *, samples_per_frame=1):
        _check_plane_stream(ih, 'LongSpectra')
        self.n, self.stack = _check_long(n, stack)
        if ih.shape[0] < self.n * self.stack:
            raise ValueError(f"the stream has {ih.shape[0]} samples: less than one stack of {self.stack} "
                             f"transforms of {self.n}.")
        rest = tuple(ih.shape[1:])
        self._n_elem = _prod(rest)
        if self._n_elem < 1:
            raise ValueError("LongSpectra needs at least one element per sample.")
        rate = _stream_rate(ih)
        _init_with_band_of(self, ih, shape=(ih.shape[0] // (self.n * self.stack), self.n // 2 + 1) + rest,
                           sample_rate=rate / (self.n * self.stack),
                           samples_per_frame=operator.index(samples_per_frame), dtype=np.float32)
        self.bin_width = rate / self.n

    def _chunk_size(self):
        return 1                                # (the samples behind one output spectrum are fetched in one piece)

    def _chunk_input(self, c0, c1):
        per = self.n * self.stack
        return c0 * per, (c1 - c0) * per

    def _make_plan(self):
        return hip.LongSpectraPlan(self.n, self.stack, self._n_elem)

    def _launch(self, x, start, count, out, c0, c1):
        self._plan.execute(x, c1 - c0, out, max(int(self.spectra_budget), 1))


class Accelerate(ChunkedDeviceTask, BaseTaskBase):
    """Acceleration trials: resample every block of ``n`` samples of a dedispersed time series along a
    parabola, once per trial acceleration, so that a pulsar whose apparent spin frequency drifts at that
    rate -- one in a binary -- becomes strictly periodic and `LongSpectra`, `Whiten` and `HarmonicSearch`
    find it as they are.

    Parameters
    ----------
    ih : stream
        float32 of shape ``(N,) + s`` with at least one element per sample -- usually a slice of the
        standardized (time, DM) plane.  A plane with a frequency and no sideband is taken as it is.
    accelerations : sequence of float
        The ``A`` trial line-of-sight accelerations in m / s^2, 1 ... 4096 of them, finite: any order, any
        sign, repeats allowed (`acceleration_grid` makes a grid).
    n : int
        Samples of a block, 2 ... 2^24, counted from sample 0 of ``ih``, not necessarily a power of two:
        the coherent transform of the `LongSpectra` that follows.  ``N >= n``.
    samples_per_frame : int, optional
        Of the output.  Default: that of ``ih``, at most the length of the output.

    The output is float32 ``(N // n * n, A) + s`` at the sample rate and start time of ``ih``; a tail
    shorter than ``n`` is dropped, as `LongSpectra` drops it.  With ``factors = acceleration_factors(
    accelerations, ih.sample_rate)``, that is ``k_j = a_j / (2 c sample_rate)`` in float64, row ``q n + i`` of
    trial ``j`` is ::

        out[q n + i, j] = ih[q n + i + int64(rint(k_j * float64(i * (i - n))))]

    -- ``i (i - n)`` in integers, one float64 multiply, round half to even, an integer add -- the 32 bits
    copied, NaN payloads and -0 included: `accelerate_rows` is the table and `accelerate_samples` the twin,
    bit for bit.  The parabola is zero at both ends of a block, so blocks do not mix and a trial of 0 is the
    identity.  Sign: a trial ``a > 0`` makes periodic a signal whose apparent frequency falls as ``f(t) = f0 (1 -
    a (t - T / 2) / c)`` over a block of length ``T``.  It is a nearest-sample resampling, on purpose: that keeps
    the stage exact.  Every trial must satisfy ``|k_j| n <= 1/4`` (``|a| T / 2c <= 1/4``: far beyond any binary)
    or the task raises ``ValueError``; under that bound the source row stays inside the block, never steps
    back, and moves at most ``n / 16`` rows -- ``max_shift`` is the largest move of this task.  Metadata of
    ``ih`` describe ``s`` and are kept; they broadcast over the new trial axis.  Attributes: ``accelerations``,
    ``factors``, ``n``, ``max_shift``.

    What it costs: the output is ``A`` times the input, and `LongSpectra` behind it holds ``4 n A n_elem`` bytes
    per transform -- 8.6 GB for 2^22 samples x 64 trials x 8 DMs.  So give it a slice of the plane, the DMs
    that are worth it: ``bt.Accelerate(bt.Standardize(plane, 4096)[:, 40:48], accs, n)``.  A chunk of
    `accel_budget` output bytes fetches only the input rows its own window needs -- for rows ``i0 ... i1`` of a
    block, ``[src(i0, k_max), src(i1, k_min)]`` -- and one kernel (csrc/accel_kernels.hpp) writes every output
    row as one contiguous run.  No value depends on the budget, on the framing or on a seek."""

    #: output bytes at most per `fetch_device` call and launch (assignable); a chunk is a whole number
    #: of rows, one at least
    accel_budget = hip.ACCEL_BUDGET

    def __init__(self, ih, accelerations, n, *, samples_per_frame=None):
        _check_plane_stream(ih, 'Accelerate')
        self.accelerations = np.array(accelerations, dtype=np.float64, ndmin=1)
        factors = acceleration_factors(self.accelerations, _stream_rate(ih))
        self.n, self.factors = _check_accel(n, factors)
        n = self.n
        if ih.shape[0] < n:
            raise ValueError(f"the stream has {ih.shape[0]} samples: less than one block of {n}.")
        rest = tuple(ih.shape[1:])
        self._n_elem = _prod(rest)
        if self._n_elem < 1:
            raise ValueError("Accelerate needs at least one element per sample.")
        if self._n_elem * len(self.factors) > hip.ACCEL_MAX_WIDTH:
            raise ValueError(f"an output sample of {len(self.factors)} trials x {self._n_elem} elements has more "
                             f"than 2^28 values.")
        self._k_min, self._k_max = float(self.factors.min()), float(self.factors.max())
        mid = n // 2
        self.max_shift = int(np.rint(np.abs(self.factors).max() * np.float64(mid * (n - mid))))
        length = ih.shape[0] // n * n
        if samples_per_frame is None:
            samples_per_frame = max(min(operator.index(ih.samples_per_frame), length), 1)
        _init_with_band_of(self, ih, shape=(length, len(self.factors)) + rest,
                           samples_per_frame=operator.index(samples_per_frame), dtype=np.float32)

    def _chunk_size(self):
        return max(1, int(self.accel_budget) // (4 * len(self.factors) * self._n_elem))

    def _chunk_input(self, c0, c1):
        """The input samples output rows [c0, c1) need: (first, count)."""
        lo, hi = _accel_window(self.n, self._k_min, self._k_max, c0, c1 - 1)
        return lo, hi + 1 - lo

    def _make_plan(self):
        return hip.AccelPlan(self.n, self._n_elem, self.factors)

    def _launch(self, x, start, count, out, c0, c1):
        self._plan.execute(x, start, count, out, c0, c1 - c0, n_rows=self.shape[0])
