"""Incoherent dedispersion over many trial DMs on the GPU: a detected filterbank swept along the
dispersion curve of every trial and summed over frequency, giving the (time, DM) plane in which a
pulse of unknown DM stands out (`DMTrials`).

The reference has no such task, so the rule is this package's, restated in NumPy here
(`dm_trial_shifts`, `dm_trials_samples`) and computed by csrc/dmt_kernels.hpp.  The shifts are those
of `DedisperseSamples`, to the bit; the sum is one float32 accumulator per output element, the
channels added in ascending index."""
import numpy as np

from . import hip
from .base import BaseTaskBase, _stream_rate, _stream_start, check_broadcast_to, simplify_shape
from .device_task import DeviceTaskMixin, fetch_device
from .dispersion import dispersion_sample_delays, with_band
from .dm import DispersionMeasure

__all__ = ['DMTrials', 'dm_trial_shifts', 'dm_trials_samples']

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


class DMTrials(DeviceTaskMixin, BaseTaskBase):
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
        self._plan = None
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

    def _chunk_samples(self):
        row_in = self.shifts.shape[1] * self._n_rest * 4
        row_out = self.shifts.shape[0] * self._n_rest * 4
        return max(1, (int(self.dmt_budget) - self._span * row_in) // (row_in + row_out))

    def _input_span(self, first, last):
        a, b = self._frame_span(first, last)
        return (self.ih, a, b - a + self._span) if b - a <= self._chunk_samples() else None     # (one fetch only)

    def _compute_frames(self, first, last, out):
        if self._plan is None:
            self._plan = hip.DmtPlan(self._offsets, self._n_rest)
        a, b = self._frame_span(first, last)
        per = self._chunk_samples()
        for c0 in range(a, b, per):
            c1 = min(b, c0 + per)
            n_in = c1 - c0 + self._span
            x = fetch_device(self.ih, c0, n_in)
            self._plan.execute(x, n_in, out[c0 - a:c1 - a], c1 - c0)

    def _repr_item(self, key, default, value=None):
        if key == 'dms':
            return f"dms={np.array2string(self.dm, threshold=6)}".replace('\n', ',')
        if key in ('frequency', 'sideband'):
            given = self._band_given[key]
            return None if given is None else f"{key}={given}".replace('\n', ',')
        return super()._repr_item(key, default, value)

    def close(self):
        super().close()
        self._drop_cache()
        if self._plan is not None:
            self._plan.close()
            self._plan = None
