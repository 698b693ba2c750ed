"""Incoherent dedispersion over many trial DMs on the GPU: a detected filterbank swept along the
dispersion curve of every trial and summed over frequency, giving the (time, DM) plane in which a
pulse of unknown DM stands out (`DMTrials`); and the single-pulse search on that plane: every
column brought to zero mean and unit variance per block (`Standardize`), matched-filtered with
boxcars of widths 1, 2, ... 4096 and the best S/N kept per block of start times (`BoxcarSearch`),
the local maxima of which are the candidates (`boxcar_candidates`, on the host).

The reference has no such tasks, so the rules are this package's, restated in NumPy here
(`dm_trial_shifts`, `dm_trials_samples`, `standardize_samples`, `boxcar_search_samples`) and
computed by csrc/dmt_kernels.hpp and csrc/sps_kernels.hpp.  The shifts are those of
`DedisperseSamples`, to the bit; the trial sum is one float32 accumulator per output element, the
channels added in ascending index; a boxcar sum is a fixed binary tree over its own samples.

`RobustStandardize` is `Standardize` with the block median and the median absolute deviation, both
exact selections (csrc/rank_kernels.hpp; the twins are `block_median_mad_samples` and
`robust_standardize_samples`): a bright pulse does not lower its own S/N.

`Detrend` subtracts a running baseline -- the sliding median over ``width`` points of the series
scrunched by ``scrunch``, interpolated back to the samples -- and `RunningMedian` is that baseline
(csrc/rmed_kernels.hpp; the twins are `detrend_samples` and `running_median_samples`): on red data a
block baseline leaves a step at every block edge, which `FFASearch` folds and `BoxcarSearch` reads
as a wide pulse."""
import operator

import numpy as np

from . import hip
from .base import BaseTaskBase, _stream_rate, _stream_start, check_broadcast_to, simplify_shape
from .device_task import ChunkedDeviceTask
from .dispersion import dispersion_sample_delays, with_band
from .dm import DispersionMeasure

__all__ = ['DMTrials', 'dm_trial_shifts', 'dm_trials_samples', 'Standardize', 'standardize_samples',
           'RobustStandardize', 'robust_standardize_samples', 'block_median_mad_samples',
           'RunningMedian', 'Detrend', 'running_median_samples', 'detrend_samples',
           'BoxcarSearch', 'boxcar_search_samples', 'boxcar_candidates', 'SNR', 'OFFSET', 'WIDTH']

MAX_NCHAN, MAX_NDM = hip.DMT_MAX_NCHAN, hip.DMT_MAX_NDM
MAX_REST, MAX_SPAN = hip.DMT_MAX_REST, hip.DMT_MAX_SPAN


def _prod(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _check_dms(dms):
    try:
        values = [float(DispersionMeasure(dm)) for dm in dms]
    except TypeError:
        raise ValueError("dms must be a 1-D sequence of trial DMs.") from None
    dm = np.array(values, dtype=np.float64)
    if dm.ndim != 1 or dm.shape[0] < 1:
        raise ValueError("dms must be a 1-D sequence of at least one trial DM.")
    if dm.shape[0] > MAX_NDM:
        raise ValueError(f"at most {MAX_NDM} trial DMs in one task, not {dm.shape[0]}.")
    return dm


def _channel_rows(value, sample_shape, what):
    """``value`` broadcast to the sample shape and cut to its channel axis, the first; ValueError
    if it varies along any other."""
    full = check_broadcast_to(value, sample_shape)
    rows = full.reshape(full.shape[0], -1)
    if not np.all(rows == rows[:, :1]):
        raise ValueError(f"{what} may vary along the channel axis (the first sample axis) only.")
    return rows[:, 0]


def dm_trial_shifts(ih, dms, reference_frequency=None):
    """The whole-sample shift of every channel of ``ih`` at every trial DM: int ``(ndm, nchan)``.

    Row ``d`` is exactly the ``_shift`` of ``DedisperseSamples(ih, dms[d],
    reference_frequency=reference_frequency)``: the dispersive delay at the channel's frequency
    relative to the reference frequency (default: the mean over the channels), negated, times the
    sample rate, rounded as `numpy.round` does.  Like that task it takes the frequency of a stream
    that is not complex to be ``ih.frequency + ih.sideband * ih.sample_rate / 2``; for detected
    power, whose ``frequency`` usually is the channel centre already, this moves every channel by
    half a channel sample rate -- negligible, but real.  Relabel the stream (``frequency=`` of
    `DMTrials`, or `SetAttribute`) where other frequencies are wanted."""
    dm = _check_dms(dms)
    if len(ih.shape) < 2:
        raise ValueError("the stream needs a channel axis: samples of shape (nchan, ...).")
    delays, _ = dispersion_sample_delays(ih, [-DispersionMeasure(v) for v in dm], reference_frequency)
    sample_shape = tuple(ih.shape[1:])
    return np.stack([_channel_rows(np.round(delay).astype(int), sample_shape, "the frequency")
                     for delay in delays])


def dm_trials_samples(data, shifts):
    """NumPy restatement of the trial-DM kernel.

    ``data``: float32 ``(N, nchan) + rest``; ``shifts``: int ``(ndm, nchan)``.  With ``hi =
    shifts.max()``, ``span = hi - shifts.min()`` and ``offsets = hi - shifts`` ::

        out[i, d, r] = sum over c of data[i + offsets[d, c], c, r]

    float32 ``(N - span, ndm) + rest``: one float32 accumulator per output element, started at +0,
    the channels added in ascending ``c`` with one rounded float32 add each.  A NaN or Inf lands in
    exactly the outputs whose sweep crosses it."""
    data = np.asarray(data)
    if data.dtype != np.float32 or data.ndim < 2:
        raise TypeError(f"samples must be float32 (N, nchan, ...), not {data.dtype} {data.shape}.")
    shifts = np.asarray(shifts)
    if shifts.ndim != 2 or shifts.shape[1] != data.shape[1] or shifts.dtype.kind not in 'iu':
        raise ValueError(f"shifts must be an integer array (ndm, {data.shape[1]}).")
    hi = int(shifts.max())
    span = hi - int(shifts.min())
    n_out = data.shape[0] - span
    if n_out < 1:
        raise ValueError(f"{data.shape[0]} samples are not more than the span of the shifts, {span}.")
    offsets = hi - shifts
    out = np.zeros((n_out, shifts.shape[0]) + data.shape[2:], np.float32)
    with np.errstate(all='ignore'):
        for d in range(shifts.shape[0]):
            acc = out[:, d]
            for c in range(data.shape[1]):
                o = int(offsets[d, c])
                acc += data[o:o + n_out, c]
    return out


class DMTrials(ChunkedDeviceTask, BaseTaskBase):
    """Dedisperse a detected stream incoherently at many trial DMs and sum over frequency.

    Parameters
    ----------
    ih : stream
        float32 powers of shape ``(N, nchan) + rest``: the channel axis is the first sample axis,
        ``rest`` may be empty or, say, the 4 products of `Power`.  For example
        ``Integrate(Square(Channelize(...)), n)`` or a `psrfits.PSRFITSSearchReader`.
    dms : sequence of float or `DispersionMeasure`
        The ``ndm`` trial DMs in pc / cm^3: any order, any sign, repeats allowed.
    reference_frequency : float, optional
        Frequency (Hz) whose arrival time the output keeps.  Default: the mean over the channels.
    samples_per_frame : int, optional
        Of the output.  Default: that of ``ih``, at most the length of the output.
    frequency, sideband : optional
        Override / provide the stream's metadata (frequency in Hz), as for `DedisperseSamples`.

    With ``shifts = dm_trial_shifts(ih, dms, reference_frequency)`` (the attribute ``shifts``),
    ``hi = shifts.max()``, ``span = hi - shifts.min()`` and ``offsets = hi - shifts`` ::

        out[i, d, r] = sum over c of ih[i + offsets[d, c], c, r]

    float32 of shape ``(N - span, ndm) + rest`` at the sample rate of ``ih``, starting ``hi``
    samples after it.  Row ``d`` of ``shifts`` is the ``_shift`` of ``DedisperseSamples(ih,
    dms[d], ...)`` to the bit, so for every trial ``out[i, d]`` equals that task's output at sample
    ``i + hi - shifts[d].max()``, summed over the channel axis: all trials on one time grid.  The
    shift rule, including the half-channel offset it gives the frequencies of a stream that is not
    complex, is described in `dm_trial_shifts`.

    The sum is ONE float32 accumulator per output element, started at +0, the channels added in
    ascending index with one rounded add each: values equal `dm_trials_samples` bit for bit, NaN
    and Inf included, whatever the tiling or the chunking.  The attribute ``dm`` holds the trials
    (float64), ``reference_frequency`` the reference; the output's ``frequency`` is that scalar,
    ``sideband`` is not passed on, and ``polarization`` is where it does not vary with the channel.
    (The base classes take ``frequency`` and ``sideband`` together, so a task stacked on the plane
    wants it relabelled: ``Integrate(SetAttribute(plane, frequency=plane.frequency, sideband=1), n)``.)
    Nothing leaves HBM: per chunk the input is transposed to time-fastest once and swept by one
    kernel with lanes along time and a block of trials in the registers of each thread."""

    #: bytes of input plus output at most per `fetch_device` call and launch (assignable)
    dmt_budget = 1 << 29

    def __init__(self, ih, dms, *, reference_frequency=None, samples_per_frame=None,
                 frequency=None, sideband=None):
        in_dtype = np.dtype(ih.dtype)
        if in_dtype.kind == 'c':
            raise TypeError("DMTrials sums detected power; make a complex stream float32 with Square "
                            "or Power first.")
        if in_dtype != np.dtype(np.float32):
            raise TypeError(f"DMTrials handles float32 streams; got {in_dtype}.")
        self._band_given = dict(frequency=frequency, sideband=sideband)
        ih = with_band(ih, frequency, sideband)
        self.dm = _check_dms(dms)
        self.shifts = shifts = dm_trial_shifts(ih, self.dm, reference_frequency)
        _, self.reference_frequency = dispersion_sample_delays(ih, [], reference_frequency)
        nchan, rest = ih.shape[1], tuple(ih.shape[2:])
        self._n_rest = _prod(rest)
        if nchan > MAX_NCHAN or self._n_rest > MAX_REST:
            raise ValueError(f"at most {MAX_NCHAN} channels of {MAX_REST} elements each; got {nchan} of "
                             f"{self._n_rest}.")
        hi = int(shifts.max())
        self._span = span = hi - int(shifts.min())
        if span > MAX_SPAN:
            raise ValueError(f"the shifts span {span} samples; at most {MAX_SPAN} can.")
        if ih.shape[0] <= span:
            raise ValueError(f"the stream has {ih.shape[0]} samples: not more than the span of the "
                             f"shifts, {span}.")
        self._offsets = (hi - shifts).astype(np.int32)
        polarization = getattr(ih, 'polarization', None)
        if polarization is not None:
            # kept where every channel has the same: one label per element of `rest`
            full = check_broadcast_to(polarization, (nchan,) + rest)
            polarization = full[0] if np.all(full == full[:1]) else None
        if samples_per_frame is None:
            # (that of `ih`; never more than the stream holds, which tasks on top would refuse)
            samples_per_frame = min(max(int(ih.samples_per_frame), 1), ih.shape[0] - span)
        super().__init__(ih, shape=(ih.shape[0] - span, len(self.dm)) + rest,
                         start_time=_stream_start(ih) + hi / _stream_rate(ih),
                         samples_per_frame=samples_per_frame, dtype=np.float32)
        # the band is summed over: what is left is the reference frequency, and no sideband
        attributes = {'frequency': np.array(self.reference_frequency, dtype=float)}
        if polarization is not None:
            attributes['polarization'] = simplify_shape(np.asanyarray(polarization))
        self.meta['__attributes__'] = attributes

    def _check_shape(self, value):
        # (the inherited metadata describe the channels; they are replaced once the stream is set up)
        return simplify_shape(np.asanyarray(value))

    def _chunk_size(self):
        row_in = self.shifts.shape[1] * self._n_rest * 4
        row_out = self.shifts.shape[0] * self._n_rest * 4
        return max(1, (int(self.dmt_budget) - self._span * row_in) // (row_in + row_out))

    def _chunk_input(self, c0, c1):
        return c0, c1 - c0 + self._span

    def _make_plan(self):
        return hip.DmtPlan(self._offsets, self._n_rest)

    def _launch(self, x, start, count, out, c0, c1):
        self._plan.execute(x, count, out, c1 - c0)

    def _repr_item(self, key, default, value=None):
        if key == 'dms':
            return f"dms={np.array2string(self.dm, threshold=6)}".replace('\n', ',')
        if key in ('frequency', 'sideband'):
            given = self._band_given[key]
            return None if given is None else f"{key}={given}".replace('\n', ',')
        return super()._repr_item(key, default, value)


# -- the single-pulse search on the plane ------------------------------------------------------------------
#: rows of `BoxcarSearch`'s output: the best S/N of a block, its start relative to the block, its level k
SNR, OFFSET, WIDTH = 0, 1, 2

SEGMENT = 32          # samples of a segment of Standardize's two-level sums (BBT_SPS_SEG)
MAX_N, MAX_WIDTHS = hip.SPS_MAX_N, hip.SPS_MAX_WIDTHS
#: c_k = float32(2 ** (-k / 2)): what a sum over 2^k samples of unit variance is scaled by
BOXCAR_SCALES = np.array([2.0 ** (-k / 2) for k in range(MAX_WIDTHS)]).astype(np.float32)
BOXCAR_SCALES.setflags(write=False)

CANDIDATE_DTYPE = np.dtype([('sample', np.int64), ('trial', np.int64), ('width', np.int64), ('snr', np.float32)])


def _check_block(n, least):
    n = operator.index(n)
    if not least <= n <= MAX_N:
        raise ValueError(f"a block must have {least} ... {MAX_N} samples, not {n}.")
    return n


def _check_widths(n_widths):
    n_widths = operator.index(n_widths)
    if not 1 <= n_widths <= MAX_WIDTHS:
        raise ValueError(f"n_widths must be 1 ... {MAX_WIDTHS} (widths up to {1 << (MAX_WIDTHS - 1)}), not {n_widths}.")
    return n_widths


def _check_plane(data, who):
    data = np.asarray(data)
    if data.dtype != np.float32 or data.ndim < 1:
        raise TypeError(f"{who}: samples must be float32 (N, ...), not {data.dtype} {data.shape}.")
    return data


def standardize_samples(data, n):
    """NumPy restatement of the `Standardize` kernel.

    ``data``: float32 ``(N,) + s``; a tail shorter than ``n`` is dropped.  Per block of ``n`` samples and
    element, in float64 with every step rounded once: ``S1 = sum x`` and ``S2 = sum x * x`` (the product of
    two float32 is exact) in the two-level order of `rfi.spectral_kurtosis` -- segments of 32 samples
    summed in sample order from 0, the segment sums added in segment order from 0 -- then ::

        mean = S1 / n;  q = S2 / n;  t = mean * mean;  var = q - t;  sd = sqrt(var);  r = 1 / sd
        z[i] = (x[i] - float32(mean)) * float32(r)          (float32: one subtract, one multiply)

    A block whose ``var`` is not finite or not ``> 0`` -- constant, all zero, holding a NaN or an Inf -- is
    ``+0`` throughout.  Returns float32 ``((N // n) * n,) + s``."""
    data, n = _check_plane(data, 'standardize_samples'), _check_block(n, 2)
    nb = data.shape[0] // n
    x = data[:nb * n].reshape((nb, n) + data.shape[1:])
    s1 = np.zeros((nb,) + data.shape[1:], np.float64)
    s2 = np.zeros_like(s1)
    with np.errstate(all='ignore'):
        for t0 in range(0, n, SEGMENT):
            a1 = np.zeros_like(s1)
            a2 = np.zeros_like(s1)
            for t in range(t0, min(t0 + SEGMENT, n)):
                q = x[:, t].astype(np.float64)
                a1 = a1 + q
                a2 = a2 + q * q
            s1 = s1 + a1
            s2 = s2 + a2
        m = np.float64(n)
        mean = s1 / m
        q = s2 / m
        t = mean * mean
        var = q - t
        sd = np.sqrt(var)
        r = 1. / sd
        ok = np.isfinite(var) & (var > 0.)
        m32, r32 = mean.astype(np.float32), r.astype(np.float32)
        z = x - m32[:, np.newaxis]
        z = z * r32[:, np.newaxis]
    assert z.dtype == np.float32
    z[np.broadcast_to(~ok[:, np.newaxis], z.shape)] = 0.
    return z.reshape((nb * n,) + data.shape[1:])


#: sd = mad * this for normal noise: 1 / (sqrt(2) erfinv(1/2)) (BBT_RANK_MAD_SCALE)
MAD_SCALE = hip.RANK_MAD_SCALE
_SIGN = np.uint32(0x80000000)


def _rank_keys(x):
    """The monotone integer keys of float32 ``x``: ``bits ^ 0xffffffff`` where the sign bit is set, ``bits |
    0x80000000`` otherwise, so that -0 comes just before +0."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(bits & _SIGN != 0, ~bits, bits | _SIGN)


def _rank_values(keys):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    return np.where(keys & _SIGN != 0, keys & ~_SIGN, ~keys).astype(np.uint32).view(np.float32)


def _block_median(x):
    """``x``: float32 ``(a, L) + s``, every ``x[i]`` one block: float32 ``(a,) + s``, the median by the rule."""
    ln = x.shape[1]
    keys = np.sort(_rank_keys(x), axis=1)
    lo, hi = _rank_values(keys[:, (ln - 1) // 2]), _rank_values(keys[:, ln // 2])
    with np.errstate(all='ignore'):
        return ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(np.float32)


def _block_median_mad(x):
    """``x``: float32 ``(a, L) + s``: ``(med, mad, flagged)``, each ``(a,) + s``."""
    flagged = ~np.isfinite(x).all(axis=1)
    med = _block_median(x)
    with np.errstate(all='ignore'):
        d = np.abs(x - med[:, np.newaxis])
    assert d.dtype == np.float32
    return med, _block_median(d), flagged


def block_median_mad_samples(data, n):
    """NumPy restatement of the selection of `RobustStandardize`: the median and the median absolute
    deviation of every block of ``n`` samples, per element.

    ``data``: float32 ``(N,) + s``; a tail shorter than ``n`` is dropped.  Values are ordered by the monotone
    integer key of their bits (`_rank_keys`: -0 just before +0), and the keys are what is sorted.  With ``lo``
    the value of rank ``(n - 1) // 2`` and ``hi`` that of rank ``n // 2`` (0-based), ``med = float32((float64(lo)
    + float64(hi)) * 0.5)``; ``mad`` is the same median of ``d[i] = |x[i] - med|`` (one rounded float32 subtract,
    the sign cleared).  Returns ``(med, mad)``, float32 ``(N // n,) + s``, NaN in both where the block holds
    a NaN or an Inf."""
    data, n = _check_plane(data, 'block_median_mad_samples'), _check_block(n, 2)
    nb = data.shape[0] // n
    x = data[:nb * n].reshape((nb, n) + data.shape[1:])
    med, mad, flagged = _block_median_mad(x)
    med[flagged] = np.nan
    mad[flagged] = np.nan
    return med, mad


def robust_standardize_samples(data, n):
    """NumPy restatement of the `RobustStandardize` kernel.

    ``data``: float32 ``(N,) + s``; a tail shorter than ``n`` is dropped.  Per block of ``n`` samples and
    element, with ``med`` and ``mad`` of `block_median_mad_samples` ::

        sd = float64(mad) * 1.482602218505602;  r = 1 / sd
        z[i] = (x[i] - med) * float32(r)                    (float32: one subtract, one multiply)

    A block that holds a NaN or an Inf, one whose ``mad`` is not ``> 0`` -- more than half of its values
    equal -- and one whose ``float32(r)`` is not finite are ``+0`` throughout.  Returns float32 ``((N // n) *
    n,) + s``."""
    data, n = _check_plane(data, 'robust_standardize_samples'), _check_block(n, 2)
    nb = data.shape[0] // n
    x = data[:nb * n].reshape((nb, n) + data.shape[1:])
    med, mad, flagged = _block_median_mad(x)
    with np.errstate(all='ignore'):
        sd = mad.astype(np.float64) * MAD_SCALE
        r32 = (1. / sd).astype(np.float32)
        ok = ~flagged & (mad > 0.) & np.isfinite(r32)
        z = x - med[:, np.newaxis]
        z = z * r32[:, np.newaxis]
    assert z.dtype == np.float32
    z[np.broadcast_to(~ok[:, np.newaxis], z.shape)] = 0.
    return z.reshape((nb * n,) + data.shape[1:])


# -- the sliding-median baseline -------------------------------------------------------------------------------
MIN_WIDTH, MAX_WIDTH, MAX_SCRUNCH = hip.RMED_MIN_WIDTH, hip.RMED_MAX_WIDTH, hip.RMED_MAX_SCRUNCH


def _check_window(width, scrunch):
    width, scrunch = operator.index(width), operator.index(scrunch)
    if not MIN_WIDTH <= width <= MAX_WIDTH or not width & 1:
        raise ValueError(f"the width must be odd, {MIN_WIDTH} ... {MAX_WIDTH} points of the scrunched series, not {width}.")
    if not 1 <= scrunch <= MAX_SCRUNCH:
        raise ValueError(f"scrunch must be 1 ... {MAX_SCRUNCH}, not {scrunch}.")
    return width, scrunch


def _scrunch(x, scrunch):
    """``x``: float32 ``(R * scrunch,) + s``: ``(c, bad)``, the scrunched series float32 ``(R,) + s`` and its bad
    rows."""
    rows = x.reshape((x.shape[0] // scrunch, scrunch) + x.shape[1:])
    bad = (rows.view(np.uint32) & np.uint32(0x7f800000) == np.uint32(0x7f800000)).any(axis=1)
    if scrunch == 1:
        return rows[:, 0], bad
    total = np.zeros((rows.shape[0],) + x.shape[1:], np.float64)
    with np.errstate(all='ignore'):
        for t0 in range(0, scrunch, SEGMENT):
            a = np.zeros_like(total)
            for t in range(t0, min(t0 + SEGMENT, scrunch)):
                a = a + rows[:, t].astype(np.float64)
            total = total + a
        return (total / np.float64(scrunch)).astype(np.float32), bad


def _running_median(c, bad, width):
    """``(m, flagged)`` of the scrunched series ``c``, float32 ``(R,) + s``, with bad rows ``bad``."""
    nrow, h = c.shape[0], width // 2
    m = np.empty_like(c)
    first_full, end_full = h, nrow - h                            # rows [h, R - h) have the whole window
    if end_full > first_full:
        keys = _rank_keys(c)
        windows = np.lib.stride_tricks.sliding_window_view(keys, width, axis=0)         # (R - 2 h,) + s + (width,)
        per = max(1, (1 << 26) // (width * max(_prod(c.shape[1:]), 1) * 4))
        for r0 in range(0, windows.shape[0], per):
            mid = np.partition(windows[r0:r0 + per], h, axis=-1)[..., h]
            value = _rank_values(mid)
            m[first_full + r0:first_full + r0 + value.shape[0]] = _block_median(np.stack([value, value], axis=1))
    for r in list(range(min(first_full, nrow))) + list(range(max(end_full, first_full, 0), nrow)):
        m[r] = _block_median(c[np.newaxis, max(0, r - h):r + h + 1])[0]
    count = np.concatenate([np.zeros((1,) + bad.shape[1:], np.int64), np.cumsum(bad, axis=0, dtype=np.int64)])
    rows = np.arange(nrow)
    flagged = count[np.minimum(rows + h + 1, nrow)] - count[np.maximum(rows - h, 0)] > 0
    return m, flagged


def _baseline(data, width, scrunch, who):
    """``(x, b, flagged)``: the samples that count, their baseline and where it is flagged."""
    data = _check_plane(data, who)
    width, scrunch = _check_window(width, scrunch)
    nrow = data.shape[0] // scrunch
    if nrow < 1:
        raise ValueError(f"{who}: {data.shape[0]} samples are less than one scrunch row of {scrunch}.")
    x = np.ascontiguousarray(data[:nrow * scrunch])
    c, bad = _scrunch(x, scrunch)
    m, flagged = _running_median(c, bad, width)
    if nrow == 1:
        r0 = np.zeros(scrunch, np.int64)
        q = np.zeros(scrunch, np.int64)
        r1 = r0
    else:
        j = 2 * np.arange(nrow * scrunch, dtype=np.int64) + 1 - scrunch
        r0 = np.clip(j // (2 * scrunch), 0, nrow - 2)
        q = j - 2 * scrunch * r0
        r1 = r0 + 1
    f = (q.astype(np.float64) / np.float64(2 * scrunch)).astype(np.float32)
    shape = (-1,) + (1,) * (x.ndim - 1)
    below, above = (q <= 0).reshape(shape), (q >= 2 * scrunch).reshape(shape)
    lo, hi = m[r0], m[r1]
    with np.errstate(all='ignore'):
        d = hi - lo
        p = d * f.reshape(shape)
        between = lo + p
    assert between.dtype == np.float32
    b = np.where(below, lo, np.where(above, hi, between))
    flagged = np.where(below, flagged[r0], np.where(above, flagged[r1], flagged[r0] | flagged[r1]))
    return x, b, flagged


def running_median_samples(data, width, scrunch=1):
    """NumPy restatement of the `RunningMedian` kernels: the sliding-median baseline of every element.

    ``data``: float32 ``(N,) + s``.  With ``S = scrunch``, ``w = width`` (odd), ``h = w // 2`` and ``R = N // S`` (the
    tail of ``N % S`` samples is dropped):

    1. ``c[r] = x[r]`` for ``S = 1``; else ``c[r] = float32(T / S)`` with ``T`` the float64 sum of ``x[r S ... r S + S -
       1]`` in the two-level order of `standardize_samples` (segments of 32 summed in order, the segment sums
       added in order).  Row ``r`` is bad if one of its samples is a NaN or an Inf.
    2. ``m[r]`` is the median, by the rule of `block_median_mad_samples`, of ``c[max(0, r - h) ... min(R - 1, r +
       h)]``: clipped at the two ends of the stream, where it is shorter and can be even.  It is flagged if the
       window holds a bad row.
    3. With ``j = 2 i + 1 - S``: ``b[i] = m[0]`` if ``R = 1``; else ``r0 = clip(j // 2 S, 0, R - 2)``, ``q = j - 2 S r0``, and
       ``b[i] = m[r0]`` if ``q <= 0``, ``m[r0 + 1]`` if ``q >= 2 S``, else ``m[r0] + (m[r0 + 1] - m[r0]) * float32(float64(q) /
       float64(2 S))``, three rounded float32 operations: the medians stand at the centres of their rows
       and are joined by straight lines; before the first centre and after the last the baseline is flat.
       ``b[i]`` is flagged if an ``m`` it used is.

    Returns ``b``, float32 ``(R S,) + s``, +0 where flagged."""
    x, b, flagged = _baseline(data, width, scrunch, 'running_median_samples')
    b[flagged] = 0.
    return b


def detrend_samples(data, width, scrunch=1):
    """NumPy restatement of the `Detrend` kernels: ``x[i] - b[i]`` with the baseline of `running_median_samples`
    before its flags are applied, one rounded float32 subtract; +0 where the baseline is flagged.  Returns
    float32 ``((N // scrunch) * scrunch,) + s``."""
    x, b, flagged = _baseline(data, width, scrunch, 'detrend_samples')
    with np.errstate(all='ignore'):
        z = x - b
    assert z.dtype == np.float32
    z[flagged] = 0.
    return z


def boxcar_search_samples(data, n, n_widths=MAX_WIDTHS):
    """NumPy restatement of the `BoxcarSearch` kernels.

    ``data``: float32 ``(N,) + s``, ``N >= n``.  With ``S_0 = x`` and, level by level, ``S_{k+1}[i] = S_k[i]
    + S_k[i + 2^k]`` (one rounded float32 add; defined where ``i + 2^(k+1) <= N``), ``snr_k[i] = S_k[i] *
    BOXCAR_SCALES[k]`` (one rounded multiply).  For block ``b`` of ``n`` start times the winner over all ``(k,
    i)`` with ``k < n_widths``, ``b n <= i < (b + 1) n`` and ``i + 2^k <= N`` is the largest S/N, among equals
    the smaller ``k``, then the smaller ``i``; a NaN never wins.  Returns float32 ``(N // n, 3) + s``: row
    `SNR` the winner's S/N, row `OFFSET` its ``i - b n``, row `WIDTH` its ``k``; ``(-inf, 0, 0)`` where a
    block has nothing but NaN."""
    data = _check_plane(data, 'boxcar_search_samples')
    n, n_widths = _check_block(n, 1), _check_widths(n_widths)
    if data.shape[0] < n:
        raise ValueError(f"{data.shape[0]} samples are less than one block of {n}.")
    rest = data.shape[1:]
    nb = data.shape[0] // n
    best = np.full((nb,) + rest, -np.inf, np.float32)
    offset = np.zeros((nb,) + rest, np.int64)
    level = np.zeros((nb,) + rest, np.int64)
    have = np.zeros((nb,) + rest, bool)
    s = data
    with np.errstate(all='ignore'):
        for k in range(n_widths):
            w = 1 << k
            snr = s[:nb * n] * BOXCAR_SCALES[k]
            if snr.shape[0] < nb * n:              # (start times whose window runs past the stream: absent)
                snr = np.concatenate([snr, np.full((nb * n - snr.shape[0],) + rest, np.nan, np.float32)])
            snr = snr.reshape((nb, n) + rest)
            valid = ~np.isnan(snr)
            filled = np.where(valid, snr, np.float32(-np.inf))
            top = filled.max(axis=1)
            first = (valid & (filled == top[:, np.newaxis])).argmax(axis=1)       # the smallest i among equals
            value = np.take_along_axis(snr, first[:, np.newaxis], axis=1)[:, 0]
            better = valid.any(axis=1) & (~have | (value > best))                # (not >=: the smaller k stays)
            best = np.where(better, value, best)
            offset = np.where(better, first, offset)
            level = np.where(better, k, level)
            have |= better
            if k + 1 == n_widths or s.shape[0] <= w:
                break
            s = s[:-w] + s[w:]
    out = np.empty((nb, 3) + rest, np.float32)
    out[:, SNR], out[:, OFFSET], out[:, WIDTH] = best, offset, level
    return out


def _local_maxima(snr, threshold):
    """The cells ``(b, d)`` of a float32 plane ``snr`` that are ``>= threshold``, have no larger value among
    their up to 8 neighbours and no equal one before them in raster order: two index arrays."""
    nb, nd = snr.shape
    padded = np.full((nb + 2, nd + 2), np.nan, np.float32)             # (a NaN compares False: no neighbour)
    padded[1:-1, 1:-1] = snr
    with np.errstate(invalid='ignore'):
        keep = snr >= np.float32(threshold)
        for db in (-1, 0, 1):
            for dd in (-1, 0, 1):
                if db == 0 and dd == 0:
                    continue
                other = padded[1 + db:1 + db + nb, 1 + dd:1 + dd + nd]
                keep &= ~(other > snr)
                if (db, dd) < (0, 0):
                    keep &= ~(other == snr)
    return np.nonzero(keep)


def _local_maxima_3d(snr, threshold):
    """`_local_maxima` for a float32 cube ``snr`` of cells ``(b, a, d)``: ``>= threshold``, no larger value
    among the up to 26 neighbours and no equal one before the cell in raster order: three index arrays."""
    nb, na, nd = snr.shape
    padded = np.full((nb + 2, na + 2, nd + 2), np.nan, np.float32)     # (a NaN compares False: no neighbour)
    padded[1:-1, 1:-1, 1:-1] = snr
    with np.errstate(invalid='ignore'):
        keep = snr >= np.float32(threshold)
        for db in (-1, 0, 1):
            for da in (-1, 0, 1):
                for dd in (-1, 0, 1):
                    if db == 0 and da == 0 and dd == 0:
                        continue
                    other = padded[1 + db:1 + db + nb, 1 + da:1 + da + na, 1 + dd:1 + dd + nd]
                    keep &= ~(other > snr)
                    if (db, da, dd) < (0, 0, 0):
                        keep &= ~(other == snr)
    return np.nonzero(keep)


def boxcar_candidates(best, n, threshold):
    """The local maxima of a `BoxcarSearch` result above a threshold (host, NumPy).

    ``best``: ``(blocks, 3, ndm)`` as read from ``BoxcarSearch(plane, n, ...)``.  A cell ``(b, d)`` is a
    candidate if its S/N is ``>= threshold``, none of its up to 8 neighbours in (block, trial) has a larger
    S/N, and no neighbour with an equal S/N comes before it in ``(b, d)`` raster order (so a plateau yields
    its first cell, and cells that touch only diagonally-later equals still count).  Returns a structured
    array with fields ``sample`` (int64: ``b n + offset``, on the sample grid of the searched plane),
    ``trial``, ``width`` (``2^k``) and ``snr``, sorted by descending ``snr``, then ``sample``, then ``trial``.
    Nothing is merged across widths or trials."""
    best = np.asarray(best)
    n = _check_block(n, 1)
    if best.ndim != 3 or best.shape[1] != 3:
        raise ValueError(f"best must be (blocks, 3, ndm) as BoxcarSearch makes it, not {best.shape}.")
    snr = best[:, SNR].astype(np.float32)
    b, d = _local_maxima(snr, threshold)
    out = np.empty(b.shape[0], CANDIDATE_DTYPE)
    out['sample'] = b * n + best[b, OFFSET, d].astype(np.int64)
    out['trial'] = d
    out['width'] = np.int64(1) << best[b, WIDTH, d].astype(np.int64)
    out['snr'] = snr[b, d]
    return out[np.lexsort((out['trial'], out['sample'], -out['snr'].astype(np.float64)))]


def _check_plane_stream(ih, who):
    in_dtype = np.dtype(ih.dtype)
    if in_dtype.kind == 'c':
        raise TypeError(f"{who} works on detected power; make a complex stream float32 with Square or Power first.")
    if in_dtype != np.dtype(np.float32):
        raise TypeError(f"{who} handles float32 streams; got {in_dtype}.")


def _lone_frequency(ih):
    """Does ``ih`` have a frequency but no sideband, as the plane of `DMTrials` has?  The base classes
    take the two together; a task that passes such metadata on hands them a placeholder sideband and
    takes it out again."""
    return getattr(ih, 'frequency', None) is not None and getattr(ih, 'sideband', None) is None


def _init_with_band_of(task, ih, **kwargs):
    """``BaseTaskBase.__init__(task, ih, **kwargs)`` for a task that passes the metadata of ``ih`` on,
    a lone frequency included (`_lone_frequency`)."""
    lone = _lone_frequency(ih)
    BaseTaskBase.__init__(task, ih, **kwargs, **(dict(sideband=1) if lone else {}))
    if lone:
        del task.meta['__attributes__']['sideband']


class _BlockStandardize(ChunkedDeviceTask, BaseTaskBase):
    """What `Standardize` and `RobustStandardize` share: blocks of ``n`` samples, frames and chunks of
    whole blocks.  A subclass names its budget attribute (``_budget``) and launches its kernel."""
    _budget = None

    def __init__(self, ih, n, *, samples_per_frame=None):
        _check_plane_stream(ih, type(self).__name__)
        self.n = n = _check_block(n, 2)
        if ih.shape[0] < n:
            raise ValueError(f"the stream has {ih.shape[0]} samples: less than one block of {n}.")
        self._n_elem = _prod(ih.shape[1:])
        length = ih.shape[0] // n * n
        if samples_per_frame is None:
            samples_per_frame = min(-(-operator.index(ih.samples_per_frame) // n) * n, length)
        samples_per_frame = operator.index(samples_per_frame)
        if samples_per_frame < n or samples_per_frame % n:
            raise ValueError(f"samples_per_frame must be a multiple of the block, {n}; got {samples_per_frame}.")
        _init_with_band_of(self, ih, shape=(length,) + tuple(ih.shape[1:]), samples_per_frame=samples_per_frame,
                           dtype=np.float32)

    def _chunk_size(self):
        block_bytes = self.n * self._n_elem * 4
        return max(1, int(getattr(self, self._budget)) // block_bytes) * self.n

    def _repr_item(self, key, default, value=None):
        if key == 'samples_per_frame' and default is None:
            default = min(-(-self._ih_samples_per_frame // self.n) * self.n, self.shape[0])
        return super()._repr_item(key, default, value)


class Standardize(_BlockStandardize):
    """Bring every block of ``n`` samples to zero mean and unit variance, per element of a sample.

    Parameters
    ----------
    ih : stream
        float32, any sample shape -- usually the (time, DM) plane of `DMTrials`.
    n : int
        Samples of a block, 2 ... 65536, counted from sample 0 of ``ih``; a tail shorter than ``n`` is
        dropped.
    samples_per_frame : int, optional
        A multiple of ``n``.  Default: the smallest one that is at least ``ih.samples_per_frame``, at
        most the length of the output.

    Sample rate, start time and metadata are those of ``ih``; the length is ``(len // n) * n``.  The
    statistics are the plain mean and variance of the block, summed in float64 in a fixed order, and
    the values equal `standardize_samples` bit for bit.  A block that is constant, all zero (what
    `Excise` leaves) or holds a NaN or an Inf comes out as +0.  There is no median / MAD, no running
    baseline, and a pulse's own power is not clipped from the estimate: a bright pulse in a short
    block lowers its own S/N.  Choose blocks much longer than the widest boxcar.  `RobustStandardize` is
    the median / MAD counterpart.  Where the baseline drifts within a block, put `Detrend` in front."""

    #: input bytes fetched at most per `fetch_device` call and launch (assignable); a chunk is a
    #: whole number of blocks
    standardize_budget = 1 << 29
    _budget = 'standardize_budget'

    def _launch(self, x, start, count, out, c0, c1):
        hip.sps_standardize(x, self.n, self._n_elem, out=out)


class RobustStandardize(_BlockStandardize):
    """Bring every block of ``n`` samples to zero median and unit robust scale (1.4826 MAD), per element
    of a sample: `Standardize` with statistics a bright pulse or residual RFI in the block cannot move.

    Parameters
    ----------
    ih : stream
        float32, any sample shape -- usually the (time, DM) plane of `DMTrials`.
    n : int
        Samples of a block, 2 ... 65536, counted from sample 0 of ``ih``; a tail shorter than ``n`` is
        dropped.
    samples_per_frame : int, optional
        A multiple of ``n``.  Default: the smallest one that is at least ``ih.samples_per_frame``, at
        most the length of the output.

    Sample rate, start time and metadata are those of ``ih``; the length is ``(len // n) * n``.  Per block
    and element ``med`` is the median and ``mad`` the median of ``|x - med|``, both exact selections on the
    GPU (the mean of the two middle values for even ``n``), and ``z = (x - med) * float32(1 / (mad *
    1.482602218505602))``: the values equal `robust_standardize_samples` bit for bit, whatever the
    route, the tiling or the chunking.  A block that holds a NaN or an Inf, or in which more than half
    of the values are equal (``mad = 0``: constant, all zero, what `Excise` leaves) comes out as +0.  The
    scale is that of normal noise; there is no clipping and re-estimation, no running median, and no
    percentile other than the median.  The running median is `Detrend`, which goes in front of this task."""

    #: input bytes fetched at most per `fetch_device` call and launch (assignable); a chunk is a
    #: whole number of blocks
    robust_budget = 1 << 29
    _budget = 'robust_budget'

    def _launch(self, x, start, count, out, c0, c1):
        hip.rank_standardize(x, self.n, self._n_elem, out=out)


class _SlidingMedian(ChunkedDeviceTask, BaseTaskBase):
    """What `RunningMedian` and `Detrend` share, which differ in what the last kernel writes (``_detrend``):
    frames and chunks of whole scrunch rows, and per chunk the rows of the stream its windows reach."""
    _detrend = None

    #: bytes of input, scratch and output at most per `fetch_device` call and launch (assignable); a chunk
    #: is a whole number of scrunch rows
    detrend_budget = 1 << 29

    def __init__(self, ih, width, scrunch=1, *, samples_per_frame=None):
        _check_plane_stream(ih, type(self).__name__)
        self.width, self.scrunch = width, scrunch = _check_window(width, scrunch)
        if ih.shape[0] < scrunch:
            raise ValueError(f"the stream has {ih.shape[0]} samples: less than one scrunch row of {scrunch}.")
        self._n_elem = _prod(ih.shape[1:])
        self._n_rows = ih.shape[0] // scrunch
        length = self._n_rows * scrunch
        if samples_per_frame is None:
            samples_per_frame = min(-(-operator.index(ih.samples_per_frame) // scrunch) * scrunch, length)
        samples_per_frame = operator.index(samples_per_frame)
        if samples_per_frame < scrunch or samples_per_frame % scrunch:
            raise ValueError(f"samples_per_frame must be a multiple of scrunch, {scrunch}; got {samples_per_frame}.")
        _init_with_band_of(self, ih, shape=(length,) + tuple(ih.shape[1:]), samples_per_frame=samples_per_frame,
                           dtype=np.float32)

    def _chunk_size(self):
        s, row = self.scrunch, self._n_elem * 4
        per_row = 2 * s * row + (2 * row if s > 1 else 0)             # input and output; c and m
        halo = (self.width + 1) * (s * row + (row if s > 1 else 0))   # the w - 1 rows the windows reach, the 2 neighbours
        return max(1, (int(self.detrend_budget) - halo) // per_row) * s

    def _chunk_input(self, c0, c1):
        """The input samples output samples [c0, c1) need (whole scrunch rows): (first, count) -- the rows
        the windows of their medians reach, the interpolation's neighbours included (rmed_need in
        csrc/rmed_geo.hpp)."""
        s, h, rows = self.scrunch, self.width // 2, self._n_rows
        near = 1 if s > 1 else 0
        first = max(0, max(0, c0 // s - near) - h)
        last = min(rows, min(rows, c1 // s + near) + h)
        return first * s, (last - first) * s

    def _make_plan(self):
        return hip.RmedPlan(self.width, self.scrunch, self._n_elem)

    def _launch(self, x, start, count, out, c0, c1):
        self._plan.execute(x, start, count, out, c0, c1 - c0, self._n_rows, detrend=self._detrend)

    def _repr_item(self, key, default, value=None):
        if key == 'samples_per_frame' and default is None:
            default = min(-(-self._ih_samples_per_frame // self.scrunch) * self.scrunch, self.shape[0])
        return super()._repr_item(key, default, value)


class RunningMedian(_SlidingMedian):
    """The running baseline of a stream: the sliding median over ``width`` points of the series scrunched by
    ``scrunch``, interpolated back to the samples, per element of a sample.  `Detrend` is the stream minus it.

    Parameters
    ----------
    ih : stream
        float32, any sample shape -- usually the (time, DM) plane of `DMTrials`.
    width : int
        Points of the scrunched series in a window: odd, 3 ... 1023.  The window spans ``width * scrunch``
        samples; choose it a few times longer than the widest pulse that is to survive.
    scrunch : int, optional
        Samples averaged into one point of the series the median runs over, 1 ... 4096, counted from sample
        0 of ``ih``; a tail shorter than ``scrunch`` is dropped.  The cost grows with ``width`` per scrunched
        point, so a long window is a moderate ``width`` on a scrunched series: 2 s at 1 ms sampling is
        ``width=125, scrunch=16``, not a width of 2001.  Default 1.
    samples_per_frame : int, optional
        A multiple of ``scrunch``.  Default: the smallest one that is at least ``ih.samples_per_frame``, at
        most the length of the output.

    Sample rate, start time and metadata are those of ``ih``; the length is ``(len // scrunch) * scrunch``.
    The windows are clipped at the two ends of the stream (never at a frame or a chunk), the medians stand
    at the centres of their scrunch rows and are joined by straight lines, flat before the first centre and
    after the last.  A NaN or an Inf makes +0 of every output whose baseline has it in a window.  The rule
    is stated in full in `running_median_samples`; a median is an exact selection and the scrunch and the
    interpolation fix their order, so the values equal that function bit for bit, whatever the selection
    method, the tiling, the budget, the framing or the seek.  There are no reflected or extrapolated ends,
    no clipping of a pulse out of the window, no running MAD, and no percentile other than the median."""
    _detrend = False


class Detrend(_SlidingMedian):
    """Subtract the running baseline of `RunningMedian` from a stream, per element of a sample: what goes in
    front of `Standardize` and the searches where the data are red -- a block baseline leaves a step at
    every block edge and the drift inside a block, which `FFASearch` folds coherently and `BoxcarSearch` reads
    as a wide pulse.

    Parameters
    ----------
    ih : stream
        float32, any sample shape -- usually the (time, DM) plane of `DMTrials`.
    width : int
        Points of the scrunched series in a window: odd, 3 ... 1023.
    scrunch : int, optional
        Samples averaged into one point of the series the median runs over, 1 ... 4096; a tail shorter
        than ``scrunch`` is dropped.  Default 1.
    samples_per_frame : int, optional
        A multiple of ``scrunch``.  Default: the smallest one that is at least ``ih.samples_per_frame``, at
        most the length of the output.

    ``out[i] = ih[i] - b[i]`` with ``b`` the baseline of `RunningMedian` (see there for the parameters and the
    ends), one rounded float32 subtract, and +0 where the baseline is flagged.  Sample rate, start time and
    metadata are those of ``ih``.  The values equal `detrend_samples` bit for bit, whatever the selection
    method, the tiling, the budget, the framing or the seek.  For ``scrunch=1`` one kernel reads ``ih`` once and
    writes the result once; otherwise the scrunched series and its medians pass through a scratch the plan
    owns.  The scale is left alone: ``Standardize(Detrend(plane, 65, scrunch=16), 4096)``."""
    _detrend = True


class BoxcarSearch(ChunkedDeviceTask, BaseTaskBase):
    """The best boxcar S/N in every block of ``n`` start times, per element of a sample: a pulse of
    unknown width is matched-filtered with boxcars of widths 1, 2, 4, ... and the best one kept.

    Parameters
    ----------
    ih : stream
        float32, any sample shape, of zero mean and unit variance -- usually
        ``Standardize(DMTrials(...), m)``.
    n : int
        Start times folded into one output sample, 1 ... 65536, counted from sample 0 of ``ih``; the
        stream must hold one block at least.
    n_widths : int, optional
        ``K``, 1 ... 13: widths ``2^k`` for ``k < K``, up to 4096.  Default 13.
    samples_per_frame : int, optional
        Of the output (blocks).  Default 1.

    The output is float32 ``(len // n, 3) + sample_shape`` at ``sample_rate / n`` from ``ih``'s start
    time: for block ``b`` row `SNR` is the largest ``snr_k[i] = S_k[i] * float32(2^(-k/2))`` over all
    widths and all start times ``b n <= i < (b + 1) n`` whose window fits the stream (``i + 2^k <= len``; it may
    run into later blocks and into the dropped tail), row `OFFSET` is ``i - b n`` and row `WIDTH` is ``k`` of
    that winner, as floats.  Among equal S/N the smaller ``k`` wins, then the smaller ``i``; a NaN never
    wins; a block of nothing else gives ``(-inf, 0, 0)``.  ``S_k[i]`` is the sum of ``ih[i] ... ih[i + 2^k -
    1]`` added up as a fixed binary tree (``S_{k+1}[i] = S_k[i] + S_k[i + 2^k]``, one rounded float32 add),
    so values equal `boxcar_search_samples` bit for bit whatever the tiling or the chunking.  Metadata are
    those of ``ih``, broadcast over the new axis.  `boxcar_candidates` turns a read of this task into a
    candidate list.  Nothing leaves HBM: the levels are made pass by pass through a scratch the plan owns,
    the running winner living in the output."""

    #: bytes of input, partial sums (twice the input at most) and output per `fetch_device` call and
    #: launch (assignable)
    sps_budget = 1 << 29

    def __init__(self, ih, n, n_widths=MAX_WIDTHS, *, samples_per_frame=1):
        _check_plane_stream(ih, 'BoxcarSearch')
        self.n = n = _check_block(n, 1)
        self.n_widths = _check_widths(n_widths)
        if ih.shape[0] < n:
            raise ValueError(f"the stream has {ih.shape[0]} samples: less than one block of {n}.")
        self._n_elem = _prod(ih.shape[1:])
        self._halo = (1 << (self.n_widths - 1)) - 1
        _init_with_band_of(self, ih, shape=(ih.shape[0] // n, 3) + tuple(ih.shape[1:]),
                           sample_rate=_stream_rate(ih) / n, samples_per_frame=samples_per_frame, dtype=np.float32)

    def _chunk_size(self):
        row = self._n_elem * 4
        return max(1, (int(self.sps_budget) - 3 * self._halo * row) // (3 * self.n * row + 3 * row))

    def _chunk_input(self, b0, b1):
        """The input samples blocks [b0, b1) need: (first, count)."""
        start = b0 * self.n
        return start, min(self.ih.shape[0], b1 * self.n + self._halo) - start

    def _make_plan(self):
        return hip.SpsPlan(self.n, self.n_widths, self._n_elem)

    def _launch(self, x, start, count, out, c0, c1):
        self._plan.execute(x, count, out, c1 - c0)
