"""Fast-folding period search on the (time, DM) plane on the GPU (`FFASearch`): every block of ``n`` samples
of every column is folded coherently at every trial period between two base periods (the radix-2 fast
folding algorithm of Staelin 1969), every folded profile is matched-filtered with circular boxcars of
widths 1, 2, 4, ... bins, and the best S/N per (block, base period, column) is kept; its local maxima are the
candidates (`ffa_candidates`, on the host).  `ffa_plan` lays out the ladder of downsampling factors and
base periods that covers a range of periods.

The reference has no such task, so the rule is this package's, restated in NumPy here (`ffa_search_samples`,
`ffa_transform_samples`, `ffa_shift`, `ffa_scales`) and computed by csrc/ffa_kernels.hpp.  A folded bin is a
fixed binary tree of float32 adds over its rows, a boxcar a fixed tree over its bins, and the winner the
maximum of a total order: the GPU equals the twin bit for bit whatever the tiling or the chunking."""
import math
import operator

import numpy as np

from . import hip
from .base import BaseTaskBase, _stream_rate
from .device_task import ChunkedDeviceTask
from .search import _check_plane, _check_plane_stream, _init_with_band_of, _local_maxima, _prod

__all__ = ['FFASearch', 'ffa_search_samples', 'ffa_transform_samples', 'ffa_shift', 'ffa_scales', 'ffa_period',
           'ffa_rows', 'ffa_candidates', 'ffa_plan', 'SNR', 'SHIFT', 'WIDTH', 'PHASE']

#: rows of `FFASearch`'s output: the best S/N, the row t of the transform, the level k, the first bin j
SNR, SHIFT, WIDTH, PHASE = 0, 1, 2, 3

SEGMENT = 32          # samples of a segment of the two-level sum T (BBT_FFA_SEG)
MIN_P, MAX_P, MAX_ROWS, MAX_WIDTHS = hip.FFA_MIN_P, hip.FFA_MAX_P, hip.FFA_MAX_ROWS, hip.FFA_MAX_WIDTHS

CANDIDATE_DTYPE = np.dtype([('period', np.float64), ('bins', np.int64), ('shift', np.int64), ('trial', np.int64),
                            ('width', np.int64), ('phase', np.int64), ('snr', np.float32)])


def _check_sizes(n, periods, n_widths):
    n = operator.index(n)
    try:
        p_lo, p_hi = (operator.index(p) for p in periods)
    except (TypeError, ValueError):
        raise ValueError("periods must be two whole numbers of samples, (p_lo, p_hi).") from None
    n_widths = operator.index(n_widths)
    if not MIN_P <= p_lo < p_hi <= MAX_P:
        raise ValueError(f"the periods must obey {MIN_P} <= p_lo < p_hi <= {MAX_P}, not ({p_lo}, {p_hi}).")
    if n < 1 or n // (p_hi - 1) < 2:
        raise ValueError(f"a block of {n} samples does not hold two rows of the longest period, {p_hi - 1}.")
    if n // p_lo > MAX_ROWS:
        raise ValueError(f"a block of {n} samples holds more than {MAX_ROWS} rows of the shortest period, {p_lo}.")
    if not 1 <= n_widths <= MAX_WIDTHS:
        raise ValueError(f"n_widths must be 1 ... {MAX_WIDTHS} (widths up to {1 << (MAX_WIDTHS - 1)}), not {n_widths}.")
    if 1 << (n_widths - 1) >= p_lo:
        raise ValueError(f"n_widths = {n_widths}: the widest boxcar, {1 << (n_widths - 1)} bins, is not shorter than the "
                         f"shortest period, {p_lo}.")
    return n, p_lo, p_hi, n_widths


def ffa_rows(n, p):
    """``(m, M)``: the rows of data ``n // p`` of a block of ``n`` samples folded at ``p``, and the power of two they
    are padded to, ``M / 2 < m <= M``."""
    m = int(n) // int(p)
    M = 1
    while M < m:
        M *= 2
    return m, M


def ffa_shift(r, t, M):
    """The bins by which row ``r`` is rotated in row ``t`` of the transform of ``M`` rows (a power of two):
    ``shift(r, t, M) = shift(r, t >> 1, M / 2)`` for ``r < M / 2``, else ``shift(r - M / 2, t >> 1, M / 2) + ((t + 1) >>
    1)``; 0 for ``M = 1``.  ``r`` and ``t`` may be integer arrays (broadcast)."""
    M = operator.index(M)
    if M < 1 or M & (M - 1):
        raise ValueError(f"M must be a power of two, not {M}.")
    r, t = np.broadcast_arrays(np.asarray(r, dtype=np.int64), np.asarray(t, dtype=np.int64))
    r, t = r.copy(), t.copy()
    s = np.zeros(r.shape, np.int64)
    while M > 1:
        h = M // 2
        upper = r >= h
        s += np.where(upper, (t + 1) >> 1, 0)
        r -= np.where(upper, h, 0)
        t >>= 1
        M = h
    return s if s.ndim else int(s)


def ffa_period(p, shift, n):
    """The period, in samples, of row ``shift`` of the transform of a block of ``n`` samples at the base period
    ``p``: ``p + shift / (M - 1)``."""
    _, M = ffa_rows(n, p)
    return p + np.asarray(shift, dtype=np.float64) / (M - 1) if M > 1 else np.float64(p)


def ffa_scales(p, m, n_widths):
    """``a_k = float32(sqrt(p / (2^k (p - 2^k) m)))`` for ``k < n_widths``, formed in float64 (the denominator is an
    exact integer): what the sum of ``2^k`` of ``p`` bins, less its share of the total, is scaled by so that
    samples of unit variance folded over ``m`` rows give unit variance."""
    p, m = int(p), int(m)
    out = np.empty(int(n_widths), np.float32)
    for k in range(out.shape[0]):
        w = 1 << k
        out[k] = np.float32(np.sqrt(np.float64(p) / np.float64(w * (p - w) * m)))
    return out


def ffa_transform_samples(d):
    """NumPy restatement of the fold stages: ``d`` float32 ``(M, p) + s``, ``M`` a power of two.  For ``G = 2, 4, ...
    M`` every group of ``G`` consecutive rows is replaced by ``out[g + t] = A[t >> 1] + roll(B[t >> 1], -((t + 1) >>
    1))``, ``t < G``, with ``A`` and ``B`` the transformed lower and upper half of the group and ``roll(v, -c)[j] =
    v[(j + c) mod p]``: one rounded float32 add each.  Row ``t`` of the result is ``sum over r of d[r, (j +
    ffa_shift(r, t, M)) mod p]``, added as a fixed binary tree."""
    d = np.asarray(d)
    if d.dtype != np.float32 or d.ndim < 2:
        raise TypeError(f"ffa_transform_samples: rows must be float32 (M, p, ...), not {d.dtype} {d.shape}.")
    M, p = d.shape[:2]
    if M < 1 or M & (M - 1):
        raise ValueError(f"the number of rows must be a power of two, not {M}.")
    rest = d.shape[2:]
    out = d
    bins = np.arange(p)
    G = 2
    with np.errstate(all='ignore'):
        while G <= M:
            h = G // 2
            pairs = out.reshape((M // G, 2, h, p) + rest)
            a, b = pairs[:, 0], pairs[:, 1]
            u = np.arange(h)
            new = np.empty((M // G, h, 2, p) + rest, np.float32)
            for odd in (0, 1):
                at = (bins[np.newaxis, :] + (u[:, np.newaxis] + odd)) % p           # (h, p): t = 2 u + odd
                new[:, :, odd] = a + b[:, u[:, np.newaxis], at]
            out = new.reshape((M, p) + rest)
            G *= 2
    return out


def _block_totals(x):
    """The float64 sum along axis 0 in the two-level order: segments of 32 in order, then the segments."""
    total = np.zeros(x.shape[1:], np.float64)
    for t0 in range(0, x.shape[0], SEGMENT):
        a = np.zeros_like(total)
        for t in range(t0, min(t0 + SEGMENT, x.shape[0])):
            a = a + x[t].astype(np.float64)
        total = total + a
    return total


def _search_block(x, p, K):
    """One block ``x`` ``(n,) + s`` at one base period: the four rows ``(4,) + s``."""
    n, rest = x.shape[0], x.shape[1:]
    m, M = ffa_rows(n, p)
    d = np.zeros((M, p) + rest, np.float32)
    d[:m] = x[:m * p].reshape((m, p) + rest)
    rows = ffa_transform_samples(d)
    total = _block_totals(x[:m * p])
    scales = ffa_scales(p, m, K)
    snr = np.empty((M, K, p) + rest, np.float32)
    level = rows
    for k in range(K):
        c = ((total * np.float64(1 << k)) / np.float64(p)).astype(np.float32)
        snr[:, k] = (level - c) * scales[k]
        if k + 1 < K:
            level = level + np.roll(level, -(1 << k), axis=1)
    flat = snr.reshape((M * K * p,) + rest)
    valid = ~np.isnan(flat)
    filled = np.where(valid, flat, np.float32(-np.inf))
    top = filled.max(axis=0)
    first = (valid & (filled == top)).argmax(axis=0)                  # the smallest (t, k, j) among equals
    value = np.take_along_axis(flat, first[np.newaxis], axis=0)[0]
    have = valid.any(axis=0)
    out = np.empty((4,) + rest, np.float32)
    out[SNR] = np.where(have, value, np.float32(-np.inf))
    out[SHIFT] = np.where(have, first // (K * p), 0)
    out[WIDTH] = np.where(have, first // p % K, 0)
    out[PHASE] = np.where(have, first % p, 0)
    return out


def ffa_search_samples(data, n, periods, n_widths=6):
    """NumPy restatement of the `FFASearch` kernels.

    ``data``: float32 ``(N,) + s``, ``N >= n``; blocks of ``n`` samples from sample 0, a shorter tail dropped.  Per
    block, column and base period ``p_lo <= p < p_hi``: ``m = n // p`` rows ``d[r, j] = x[r p + j]`` padded with +0 to
    ``M`` rows (`ffa_rows`), transformed by `ffa_transform_samples`; ``S_0`` = row ``t``, ``S_{k+1}[j] = S_k[j] +
    S_k[(j + 2^k) mod p]`` (one rounded float32 add); with ``T`` the float64 sum of the ``m p`` used samples in the
    two-level order of `search.standardize_samples`, ``c_k = float32((T 2^k) / p)`` and ``a_k`` of `ffa_scales`,
    ``snr_k[t, j] = (S_k[t, j] - c_k) * a_k`` (one rounded float32 subtract, one rounded multiply).  The winner
    over all ``(t, k, j)`` is the largest S/N, among equals the smaller ``t``, then ``k``, then ``j``; a NaN never
    wins.  Returns float32 ``(N // n, p_hi - p_lo, 4) + s``: rows `SNR`, `SHIFT`, `WIDTH`, `PHASE` = ``snr, t, k, j``;
    ``(-inf, 0, 0, 0)`` where there is nothing but NaN."""
    data = _check_plane(data, 'ffa_search_samples')
    n, p_lo, p_hi, K = _check_sizes(n, periods, n_widths)
    if data.shape[0] < n:
        raise ValueError(f"{data.shape[0]} samples are less than one block of {n}.")
    nb = data.shape[0] // n
    out = np.empty((nb, p_hi - p_lo, 4) + data.shape[1:], np.float32)
    with np.errstate(all='ignore'):
        for b in range(nb):
            x = data[b * n:(b + 1) * n]
            for p in range(p_lo, p_hi):
                out[b, p - p_lo] = _search_block(x, p, K)
    return out


def ffa_candidates(best, n, periods, threshold, sample_rate=1.):
    """The local maxima of one block of an `FFASearch` result above a threshold (host, NumPy).

    ``best``: ``(p_hi - p_lo, 4, ndm)``, one output sample of ``FFASearch(plane, n, periods, ...)``.  A cell ``(base
    period, trial)`` is a candidate if its S/N is ``>= threshold``, none of its up to 8 neighbours has a larger S/N
    and no neighbour with an equal S/N comes before it in raster order (the rule of `search.boxcar_candidates`).
    Returns a structured array with fields ``period`` (seconds: `ffa_period` over ``sample_rate`` in Hz), ``bins``
    (the base period), ``shift``, ``trial``, ``width`` (``2^k`` bins), ``phase`` (the first bin) and ``snr``, sorted by
    descending ``snr``, then ``bins``, then ``trial``.  Nothing is merged across base periods or trials."""
    best = np.asarray(best)
    n = operator.index(n)
    p_lo, p_hi = (operator.index(p) for p in periods)
    if best.ndim != 3 or best.shape[:2] != (p_hi - p_lo, 4):
        raise ValueError(f"best must be ({p_hi - p_lo}, 4, ndm), one block as FFASearch makes it, not {best.shape}.")
    snr = best[:, SNR].astype(np.float32)
    i, d = _local_maxima(snr, threshold)
    out = np.empty(i.shape[0], CANDIDATE_DTYPE)
    out['bins'] = p_lo + i
    out['shift'] = best[i, SHIFT, d].astype(np.int64)
    out['trial'] = d
    out['width'] = np.int64(1) << best[i, WIDTH, d].astype(np.int64)
    out['phase'] = best[i, PHASE, d].astype(np.int64)
    out['snr'] = snr[i, d]
    rate = float(sample_rate)
    out['period'] = [float(ffa_period(p, s, n)) / rate for p, s in zip(out['bins'], out['shift'])]
    return out[np.lexsort((out['trial'], out['bins'], -out['snr'].astype(np.float64)))]


def ffa_plan(period_min, period_max, sample_rate, bins_min=256):
    """The ladder of searches that covers the periods ``period_min ... period_max`` (seconds) of a plane sampled at
    ``sample_rate`` (Hz): a list of ``(factor, p_lo, p_hi)`` with whole downsampling factors and ``p_hi <= 2 p_lo``, so
    that ``FFASearch(Standardize(Integrate(plane, factor), ...), n, (p_lo, p_hi))`` folds at the periods ``p_lo factor
    / sample_rate ... p_hi factor / sample_rate``.  Each step starts at or below the period where the one before
    ends, with ``bins_min`` (4 ... 512) bins or more across the period wherever the plane's own sampling allows
    it."""
    bins_min = operator.index(bins_min)
    if not MIN_P <= bins_min <= (MAX_P - 1) // 2:
        raise ValueError(f"bins_min must be {MIN_P} ... {(MAX_P - 1) // 2}, not {bins_min}.")
    rate = float(sample_rate)
    lo, hi = float(period_min) * rate, float(period_max) * rate              # in samples of the plane
    if not (math.isfinite(lo) and math.isfinite(hi) and MIN_P <= lo < hi):
        raise ValueError(f"the periods must obey {MIN_P} samples <= period_min < period_max; got {lo} and {hi} samples.")
    steps = []
    start = lo
    while True:
        factor = max(1, int(start // bins_min))
        p_lo = int(start // factor)
        p_hi = min(2 * p_lo, MAX_P)
        if p_hi * factor >= hi:
            p_hi = max(p_lo + 1, min(p_hi, math.ceil(hi / factor)))
            steps.append((factor, p_lo, p_hi))
            return steps
        steps.append((factor, p_lo, p_hi))
        start = float(p_hi * factor)


class FFASearch(ChunkedDeviceTask, BaseTaskBase):
    """The best fold of every block of ``n`` samples at every base period, per element of a sample: a pulsar of
    unknown period and duty cycle is folded coherently at every trial period and its profile matched-filtered
    with circular boxcars of widths 1, 2, 4, ... bins.

    Parameters
    ----------
    ih : stream
        float32, any sample shape, of zero mean and unit variance -- usually ``Standardize(Integrate(DMTrials(...),
        factor), ...)``.
    n : int
        Samples of a block, counted from sample 0 of ``ih``; a shorter tail is dropped.
    periods : (int, int)
        The base periods ``p_lo <= p < p_hi`` in whole samples: ``4 <= p_lo < p_hi <= 1025``, ``n // (p_hi - 1) >= 2``,
        ``n // p_lo <= 65536``.
    n_widths : int, optional
        ``K``, 1 ... 10 with ``2^(K-1) < p_lo``: widths ``2^k`` bins for ``k < K``.  Default 6.
    samples_per_frame : int, optional
        Of the output (blocks).  Default 1.

    The output is float32 ``(len // n, p_hi - p_lo, 4) + sample_shape`` at ``sample_rate / n`` from ``ih``'s start time.
    Per block and base period ``p`` the ``m = n // p`` whole rows of ``p`` samples (the last ``n - m p`` samples are not
    used) are padded with zero rows to a power of two ``M`` and transformed by the radix-2 fast folding algorithm:
    row ``t < M`` is the fold at a period of ``p + t / (M - 1)`` samples (`ffa_period`).  Row `SNR` is the largest
    ``(S_k[t, j] - c_k) * a_k`` over all rows ``t``, levels ``k`` and bins ``j`` -- the sum of the ``2^k`` bins from ``j`` on,
    circularly, less its share of the block's total, in units of the noise for input of unit variance -- and rows
    `SHIFT`, `WIDTH`, `PHASE` are ``t``, ``k`` and ``j`` of that winner, as floats.  Among equal S/N the smaller ``t`` wins,
    then the smaller ``k``, then the smaller ``j``; a NaN never wins; nothing else gives ``(-inf, 0, 0, 0)``.  A NaN or
    an Inf spoils its own (block, column) for the base periods whose used samples hold it.  Every add is one
    rounded float32 add in a fixed tree, so values equal `ffa_search_samples` bit for bit whatever the tiling or
    the chunking.  Metadata are those of ``ih``, broadcast over the new axes.  `ffa_candidates` turns one output
    sample into a candidate list, `ffa_plan` lays out a ladder of searches.  Nothing leaves HBM: the stages are
    made pass by pass through two scratch buffers the plan owns.

    Not done: row counts that are no power of two without padding, downsampling by other than whole factors,
    widths other than powers of two, the full periodogram as output, merging candidates across base periods
    and DMs, folding the candidates."""

    #: bytes of a block's input, the scratch and the output per launch (assignable): the columns, then the base
    #: periods, are cut into chunks to stay within it
    ffa_budget = 1 << 29

    def __init__(self, ih, n, periods, n_widths=6, *, samples_per_frame=1):
        _check_plane_stream(ih, 'FFASearch')
        self.n, p_lo, p_hi, self.n_widths = _check_sizes(n, periods, n_widths)
        self.periods = (p_lo, p_hi)
        if ih.shape[0] < self.n:
            raise ValueError(f"the stream has {ih.shape[0]} samples: less than one block of {self.n}.")
        self._n_elem = _prod(ih.shape[1:])
        self._max_mp = max(ffa_rows(self.n, p)[1] * p for p in range(p_lo, p_hi))
        _init_with_band_of(self, ih, shape=(ih.shape[0] // self.n, p_hi - p_lo, 4) + tuple(ih.shape[1:]),
                           sample_rate=_stream_rate(ih) / self.n, samples_per_frame=samples_per_frame,
                           dtype=np.float32)

    def _chunks(self):
        """The launches of one block: a list of ``(e0, ne, pa, pb)``."""
        p_lo, p_hi = self.periods
        left = int(self.ffa_budget) - self.n * self._n_elem * 4
        # bytes of scratch per column: the running segment sums (float64), the c_k, two buffers of the largest M p
        column = (2 * (self.n // SEGMENT + 1) + hip.FFA_MAX_WIDTHS + 2 * self._max_mp) * 4
        cell = 4 * 4                                                      # bytes of output per column and period
        ne = min(max(1, left // (column + cell)), self._n_elem, (hip.FFA_MAX_LANE - 1) // (p_hi - 1))
        launches = []
        for e0 in range(0, self._n_elem, ne):
            cols = min(ne, self._n_elem - e0)
            per = min(max(1, (left - cols * column) // (cols * cell)), p_hi - p_lo)
            launches += [(e0, cols, pa, min(p_hi, pa + per)) for pa in range(p_lo, p_hi, per)]
        return launches

    def _chunk_size(self):
        return 1                                # (one block per fetch; `_chunks` cuts it into launches)

    def _chunk_input(self, c0, c1):
        return c0 * self.n, (c1 - c0) * self.n

    def _make_plan(self):
        return hip.FfaPlan(self.n, self.periods, self.n_widths, self._n_elem)

    def _launch(self, x, start, count, out, c0, c1):
        for e0, ne, pa, pb in self._chunks():
            self._plan.execute(x, out, e0, ne, pa, pb)
