"""Radio-frequency interference found and zeroed on the GPU: the spectral kurtosis estimator
over blocks of a stream (`SpectralKurtosis`) and the excision of the blocks it condemns (`Excise`).

The reference has no such task, so the rule is this package's, restated in NumPy here
(`spectral_kurtosis`, `excise_samples`) and computed by csrc/sk_kernels.hpp.  The estimator is
that of Nita & Gary (2010, MNRAS 406, L60), generalised to inputs that are sums of ``averaged``
complex-voltage powers."""
import operator

import numpy as np

from . import hip
from .base import BaseTaskBase, _stream_rate
from .device_task import ChunkedDeviceTask

__all__ = ['SpectralKurtosis', 'Excise', 'sk_limits', 'spectral_kurtosis', 'excise_flags', 'excise_samples']

SEGMENT = 32          # samples of a segment of the two-level sums (BBT_SK_SEG)
MAX_N = hip.SK_MAX_N
MAX_GROUP = hip.SK_MAX_GROUP


def _prod(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _check_n(n):
    n = operator.index(n)
    if not 2 <= n <= MAX_N:
        raise ValueError(f"a block must have 2 ... {MAX_N} samples, not {n}.")
    return n


def _check_averaged(averaged):
    averaged = float(averaged)
    if not 0. < averaged <= 1e9:
        raise ValueError(f"averaged must be positive, not {averaged}.")
    return averaged


def _group(sample_shape, join):
    """Elements that share a flag: the product of the last ``join`` axes of a sample."""
    join = operator.index(join)
    if not 0 <= join <= len(sample_shape):
        raise ValueError(f"join must be 0 ... {len(sample_shape)} (the sample axes), not {join}.")
    g = _prod(sample_shape[len(sample_shape) - join:])
    if not 1 <= g <= MAX_GROUP:
        raise ValueError(f"join={join} makes groups of {g} elements; at most {MAX_GROUP} can share a flag.")
    return g


def sk_limits(n, nsigma=3., averaged=1.):
    """The band ``(1 - nsigma * sigma, 1 + nsigma * sigma)``, float32, inside which the spectral
    kurtosis of ``n`` samples of noise is kept, with the estimator's variance for ``M = n`` and ``Nd
    = averaged`` (Nita & Gary 2010, from the second moment, the ratio of Gamma functions written
    out)::

        sigma^2 = 2 Nd (Nd + 1) M^2 / ((M - 1) (M Nd + 2) (M Nd + 3))

    The symmetric band is a policy default, not a measurement: the estimator's distribution is
    skewed, and a 3 sigma band flags 0.4 % (M = 1024) to 1.8 % (M = 16) of pure noise rather than
    a Gaussian's 0.27 %.  Pass explicit ``limits`` to `Excise` where that matters; for small ``n``
    the lower edge is below 0 and only the upper one can flag anything."""
    m, nd, nsigma = float(_check_n(n)), _check_averaged(averaged), float(nsigma)
    if not nsigma > 0.:
        raise ValueError(f"nsigma must be positive, not {nsigma}.")
    var = 2. * nd * (nd + 1.) * m * m / ((m - 1.) * (m * nd + 2.) * (m * nd + 3.))
    sigma = np.sqrt(var)
    return np.float32(1. - nsigma * sigma), np.float32(1. + nsigma * sigma)


def _check_limits(limits):
    lo, hi = (np.float32(v) for v in limits)
    if not lo <= hi:
        raise ValueError(f"the limits must be an ordered pair, not {(lo, hi)}.")
    return lo, hi


def _powers(data, n):
    """float64 powers of the whole blocks of ``data``, (n_block, n) + sample_shape."""
    data = np.asarray(data)
    if data.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
        raise TypeError(f"samples must be float32 (powers) or complex64, not {data.dtype}.")
    n_block = data.shape[0] // n
    data = data[:n_block * n].reshape((n_block, n) + data.shape[1:])
    if data.dtype.kind == 'c':
        re, im = data.real.astype(np.float64), data.imag.astype(np.float64)
        return re * re + im * im                   # (both products exact: one rounding)
    return data.astype(np.float64)


def spectral_kurtosis(data, n, averaged=1.):
    """NumPy restatement of the spectral kurtosis kernels.

    ``data``: (samples,) + sample_shape, float32 powers or complex64 voltages (``p = re^2 + im^2``);
    a tail shorter than ``n`` is dropped.  Per block of ``n`` samples and element, in float64:
    ``S1 = sum p`` and ``S2 = sum p^2`` in a fixed two-level order -- segments of 32 consecutive
    samples (the last may be shorter) each summed in sample order from 0, the segment sums added
    in segment order from 0 -- and, with ``M = n`` and ``Nd = averaged``, step by step ::

        c = (M Nd + 1) / (M - 1);  t = S1 * S1;  r = S2 / t;  r = M * r;  r = r - 1;  sk = float32(c * r)

    ``averaged`` is the number of complex-voltage powers summed into each input value: 1 for
    ``|z|^2``, N after ``Integrate(Square(...), N)`` (the estimator is free of scale, so averages
    and sums serve alike), 0.5 for the square of one real-sampled voltage.  Returns float32
    ``(samples // n,) + sample_shape``; an all-zero block or one with a NaN or Inf gives NaN."""
    n, nd = _check_n(n), _check_averaged(averaged)
    p = _powers(data, n)
    s1 = np.zeros(p.shape[:1] + p.shape[2:], np.float64)
    s2 = np.zeros_like(s1)
    with np.errstate(all='ignore'):
        for t0 in range(0, n, SEGMENT):
            a1 = np.zeros_like(s1)
            a2 = np.zeros_like(s1)
            for t in range(t0, min(t0 + SEGMENT, n)):
                q = p[:, t]
                a1 = a1 + q
                a2 = a2 + q * q
            s1 = s1 + a1
            s2 = s2 + a2
        m = np.float64(n)
        c = (m * nd + 1.) / (m - 1.)
        t = s1 * s1
        r = s2 / t
        r = m * r
        r = r - 1.
        return (c * r).astype(np.float32)


def excise_flags(sk, limits, join=0):
    """Which (block, group) the kernels zero: ``not (lo <= sk <= hi)`` in float32 (so a NaN is
    flagged), OR-ed over the last ``join`` axes.  bool, ``sk.shape`` less those axes."""
    lo, hi = _check_limits(limits)
    sk = np.asarray(sk, dtype=np.float32)
    _group(sk.shape[1:], join)
    with np.errstate(invalid='ignore'):
        bad = ~((sk >= lo) & (sk <= hi))
    if join:
        bad = bad.reshape(bad.shape[:bad.ndim - join] + (-1,)).any(-1)
    return bad


def excise_samples(data, n, limits, averaged=1., join=0):
    """NumPy restatement of `Excise`: the whole blocks of ``data``, with every (block, group of
    elements that differ only in the last ``join`` axes) set to +0 in which an element's
    `spectral_kurtosis` lies outside ``limits``; all other samples bit for bit."""
    data = np.asarray(data)
    n = _check_n(n)
    bad = excise_flags(spectral_kurtosis(data, n, averaged), limits, join)
    n_block = data.shape[0] // n
    out = data[:n_block * n].copy().reshape((n_block, n) + data.shape[1:])
    bad = bad.reshape(bad.shape + (1,) * join)
    out[np.broadcast_to(bad[:, np.newaxis], out.shape)] = 0
    return out.reshape((n_block * n,) + data.shape[1:])


def _check_stream(ih, n, who):
    in_dtype = np.dtype(ih.dtype)
    if in_dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
        raise TypeError(f"{who} handles float32 (powers) and complex64; got {in_dtype}.")
    n = _check_n(n)
    if ih.shape[0] < n:
        raise ValueError(f"the stream has {ih.shape[0]} samples: less than one block of {n}.")
    return n


class SpectralKurtosis(ChunkedDeviceTask, BaseTaskBase):
    """The spectral kurtosis estimator of every block of ``n`` samples, per element of a sample.

    Parameters
    ----------
    ih : stream
        float32 powers or complex64 voltages, any sample shape -- usually channelized.
    n : int
        Samples of a block, 2 ... 65536.  Block ``b`` is samples ``b * n ... b * n + n - 1`` of
        ``ih``; a tail shorter than ``n`` is dropped.
    averaged : float, optional
        Complex-voltage powers summed into each input value (see `spectral_kurtosis`).
    samples_per_frame : int, optional
        Of the output (blocks).  Default 1.

    The output is float32, ``(len // n,) + sample_shape``, at ``sample_rate / n`` from ``ih``'s
    start time; ``frequency``, ``sideband`` and ``polarization`` are passed on.  Noise gives
    values around 1 with the variance of `sk_limits`; a steady carrier pulls them down, impulsive
    power pushes them up.  Values equal `spectral_kurtosis` bit for bit."""

    #: input bytes fetched at most per `fetch_device` call and launch (assignable)
    sk_budget = 1 << 29

    def __init__(self, ih, n, *, averaged=1., samples_per_frame=1):
        self.n = _check_stream(ih, n, 'SpectralKurtosis')
        self.averaged = _check_averaged(averaged)
        self._n_elem = _prod(ih.shape[1:])
        super().__init__(ih, shape=(ih.shape[0] // self.n,) + tuple(ih.shape[1:]),
                         sample_rate=_stream_rate(ih) / self.n, samples_per_frame=samples_per_frame,
                         dtype=np.float32)

    def _chunk_size(self):
        block_bytes = self.n * self._n_elem * np.dtype(self.ih.dtype).itemsize
        return max(1, int(self.sk_budget) // block_bytes)

    def _chunk_input(self, c0, c1):
        return c0 * self.n, (c1 - c0) * self.n

    def _launch(self, x, start, count, out, c0, c1):
        hip.sk_estimate(x, self.n, self._n_elem, self.averaged, out=out)


class Excise(ChunkedDeviceTask, BaseTaskBase):
    """Zero every block of ``n`` samples of an element whose spectral kurtosis is not that of noise.

    Parameters
    ----------
    ih : stream
        float32 powers or complex64 voltages, any sample shape -- usually channelized, e.g.
        ``Excise(Channelize(stream, 1024), 1024, join=1)`` ahead of `Power` or `Fold`.
    n : int
        Samples of a block, 2 ... 65536, counted from sample 0 of ``ih``; a tail shorter than
        ``n`` is dropped.
    limits : (lo, hi), optional
        Keep a block where ``lo <= sk <= hi`` (float32).  Default: ``sk_limits(n, nsigma,
        averaged)``, a symmetric band that is a policy, not a measurement (see `sk_limits`).
    nsigma : float, optional
        Half-width of the default band in standard deviations of the estimator.  Default 3.
    averaged : float, optional
        Complex-voltage powers summed into each input value (see `spectral_kurtosis`).
    join : int, optional
        The elements that differ only in the last ``join`` sample axes share the OR of their
        flags: ``join=1`` on ``(nchan, npol)`` zaps both polarizations if either is bad.  At most
        64 elements can share a flag.  Default 0.
    samples_per_frame : int, optional
        A multiple of ``n``.  Default: the smallest one that is at least ``ih.samples_per_frame``.

    Dtype, sample rate, start time and metadata are those of ``ih``; the length is ``(len // n)
    * n``.  A flagged (block, element) comes out as +0, everything else bit for bit
    (`excise_samples`); a block that is all zero or holds a NaN or Inf is flagged.  The attribute
    ``limits`` holds the float32 pair in use.  Nothing leaves HBM: one kernel makes the
    estimator of a block and rewrites the block while it is still in cache."""

    #: input bytes fetched at most per `fetch_device` call and launch (assignable); a chunk is a
    #: whole number of blocks
    excise_budget = 1 << 29

    def __init__(self, ih, n, limits=None, *, nsigma=3., averaged=1., join=0, samples_per_frame=None):
        self.n = n = _check_stream(ih, n, 'Excise')
        self.averaged = _check_averaged(averaged)
        self.nsigma = float(nsigma)
        self.join = operator.index(join)
        self._group = _group(tuple(ih.shape[1:]), join)
        self._limits_given = limits is not None
        self.limits = _check_limits(limits) if limits is not None else sk_limits(n, nsigma, self.averaged)
        self._n_elem = _prod(ih.shape[1:])
        if samples_per_frame is None:
            samples_per_frame = -(-operator.index(ih.samples_per_frame) // n) * n
        samples_per_frame = operator.index(samples_per_frame)
        if samples_per_frame < n or samples_per_frame % n:
            raise ValueError(f"samples_per_frame must be a multiple of the block, {n}; got {samples_per_frame}.")
        super().__init__(ih, shape=(ih.shape[0] // n * n,) + tuple(ih.shape[1:]),
                         samples_per_frame=samples_per_frame)

    def _chunk_size(self):
        block_bytes = self.n * self._n_elem * np.dtype(self.dtype).itemsize
        return max(1, int(self.excise_budget) // block_bytes) * self.n

    def _launch(self, x, start, count, out, c0, c1):
        hip.sk_excise(x, out, self.n, self._n_elem, self.limits, self.averaged, self._group)

    def _repr_item(self, key, default, value=None):
        if key == 'limits':
            return f"limits=({self.limits[0]}, {self.limits[1]})" if self._limits_given else None
        if key == 'samples_per_frame' and default is None:
            default = -(-self._ih_samples_per_frame // self.n) * self.n
        return super()._repr_item(key, default, value)
