"""Stepwise integration, folding and pulse stacks on the GPU (reference
baseband_tasks/integration.py: `Integrate` 52-303, `Fold` 306-395, `PulseStack`
398-478)."""
import operator
import os
import warnings

import numpy as np

from . import hip
from . import units as u
from .base import BaseTaskBase, _stream_rate, _stream_start
from .device_task import DeviceTaskMixin, fetch_device
from .fold_table import (contiguous_table, fold_table, phase_difference, piece_table, plan_pieces,
                         sample_times)
from .functions import _DetectTask
from .units import Time

__all__ = ['Integrate', 'Fold', 'PulseStack']


def _prod(shape):
    n = 1
    for d in shape:
        n *= d
    return n


class Integrate(DeviceTaskMixin, BaseTaskBase):
    """Integrate a stream over ``step`` consecutive samples.

    Parameters
    ----------
    ih : stream
        float32 (e.g. the output of `Square` / `Power`) or complex64.
    step : int or float, optional
        Input samples per output sample; default: everything from ``start``.
        With ``phase``, the width of an output sample in cycles (e.g. ``1/25``).
        (Integration over time intervals, a non-integer step without ``phase``,
        is outside the accelerated path.)
    phase : callable, optional
        Pulse phase of the input (see `Fold`): the output samples are bins of
        ``step`` cycles; output sample ``k`` sums the contiguous input samples
        between the offsets at which the phase (relative to the start) reaches
        ``k * step`` and ``(k + 1) * step`` (found as in the reference,
        integration.py:174-228).
    start : int or `~baseband_tasks_amd.units.Time`
        Offset (or time, rounded to the nearest sample) of the first sample.
    average : bool
        True: averages.  False: like the reference, `read` returns a structured
        array with the sums in ``'data'`` and the number of samples summed in
        ``'count'`` (the task's ``dtype`` is that structured type; the frames in
        HBM hold the sums).
    samples_per_frame : int
        Output samples per frame (framing only).
    dtype : optional, must equal the input dtype.

    When ``ih`` is a GPU `Square` or `Power`, detection and integration run as
    one kernel on the undetected stream (the detected stream is never stored).
    """
    max_frames_per_call = 1 << 16

    def __new__(cls, ih, step=None, phase=None, *, start=0, average=True, samples_per_frame=1,
                dtype=None):
        # with a phase callable: integration in pulse-phase bins (a task of its own).  (The
        # signature is __init__'s: repr reads the constructor's parameters from it.)
        if cls is Integrate and phase is not None:
            return _PhaseIntegrate(ih, step, phase, start=start, average=average,
                                   samples_per_frame=samples_per_frame, dtype=dtype)
        return super().__new__(cls)

    def __init__(self, ih, step=None, phase=None, *, start=0, average=True,
                 samples_per_frame=1, dtype=None):
        if phase is not None:
            raise NotImplementedError("integration in pulse phase is outside the accelerated path.")
        ih_start = ih.seek(start)
        ih_n = ih.shape[0] - ih_start
        if ih_start < 0 or ih_n < 0:
            raise ValueError("'start' is not within the underlying stream.")
        if step is None:
            step = ih_n
        try:
            if isinstance(step, float) and step.is_integer():
                step = int(step)                # (3.0 samples is 3 samples)
            step = operator.index(step)
        except TypeError:
            raise NotImplementedError("integration over time intervals (non-integer step) is "
                                      "outside the accelerated path.") from None
        in_dtype = np.dtype(ih.dtype)
        if in_dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
            raise TypeError(f"the accelerated Integrate handles float32/complex64; got {in_dtype}.")
        if dtype is not None and np.dtype(dtype) != in_dtype:
            raise TypeError("the accelerated Integrate keeps the input dtype.")
        n_out = int(ih_n / step + 0.5 / step)
        assert n_out >= 1, "time per frame larger than total time in stream"
        rate = _stream_rate(ih)
        self._start = start
        self._step, self._ih_start = step, ih_start
        self.average = bool(average)
        self._sum_dtype = in_dtype
        out_dtype = in_dtype if average else np.dtype([('data', in_dtype), ('count', int)])
        super().__init__(ih, shape=(n_out,) + tuple(ih.shape[1:]), sample_rate=rate / step,
                         samples_per_frame=samples_per_frame,
                         start_time=_stream_start(ih) + ih_start / rate, dtype=out_dtype)

    @property
    def _device_dtype(self):
        return self._sum_dtype

    @property
    def _time_from_offsets(self):
        # on top of pulse-phase bins (`PulseStack`), times are those of the input
        return bool(getattr(self.__dict__.get('ih'), '_time_from_offsets', False))

    def _tell_time(self, offset):
        if self._time_from_offsets:
            return self.ih._tell_time(self._ih_start + offset * self._step)
        return super()._tell_time(offset)

    def read(self, count=None, out=None):
        if self.average:
            return super().read(count, out)
        if out is not None:
            raise NotImplementedError("average=False: read() makes its own structured output.")
        count = self._prepare_read(count, None)
        sums = super().read(count, np.empty((count,) + tuple(self.sample_shape), self._sum_dtype))
        result = np.empty(sums.shape, self.dtype)
        result['data'] = sums
        result['count'] = self._step
        return result

    def _repr_item(self, key, default, value=None):
        # 'step' as given (None = everything), 'start' as given
        if key == 'step' and self._step == self.ih.shape[0] - self._ih_start and self.shape[0] == 1:
            return None
        return super()._repr_item(key, default, value)

    def _compute_frames(self, first, last, out):
        a, b = self._frame_span(first, last)
        n_out, step = b - a, self._step
        src = self.ih
        if isinstance(src, _DetectTask) and not src.closed:
            # a channelizer on top of an overlap-save task detects and sums in
            # that task's last pass: neither stream is ever stored
            fused = getattr(src.ih, '_compute_detected', None)
            if (fused is not None and not src._real and getattr(src, '_inner', 1) == 1
                    and not getattr(src.ih, 'closed', False)
                    and fused(self._ih_start + a * step, n_out, step, src._mode, self.average, out)):
                return
            x = fetch_device(src.ih, self._ih_start + a * step, n_out * step)
            src._detect(x, n_out, step, out, self.average)
            return
        x = fetch_device(src, self._ih_start + a * step, n_out * step)
        n_float = _prod(self.sample_shape) * (2 if self._sum_dtype.kind == 'c' else 1)
        hip.detect_integrate(x, out, n_out, step, n_float, 2, self.average)

    def close(self):
        super().close()
        self._drop_cache()


# ---------------------------------------------------------------------------
# folding: shared machinery
def _is_index(n):
    if isinstance(n, (bool, float)):
        return False
    try:
        operator.index(n)
    except TypeError:
        return False
    return True


def _array_time(t):
    """Scalar `Time` -> array-valued time of one element (what the phase callable gets)."""
    return Time(t) + np.zeros(1)


class _RunTableTask(DeviceTaskMixin, BaseTaskBase):
    """A task whose output slots each sum runs of input samples (after detection), computed
    by `hip.fold_runs` from run tables built on the host from the sample times alone."""

    #: input bytes fetched at most per `fetch_device` call (assignable)
    fold_budget = 1 << 29

    def _init_source(self, ih, dtype, average):
        in_dtype = np.dtype(ih.dtype)
        if in_dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
            raise TypeError(f"the accelerated {type(self).__name__} handles float32/complex64; "
                            f"got {in_dtype}.")
        if dtype is not None and np.dtype(dtype) != in_dtype:
            raise TypeError(f"the accelerated {type(self).__name__} keeps the input dtype.")
        self._sum_dtype = in_dtype
        self.average = bool(average)
        return in_dtype if average else np.dtype([('data', in_dtype), ('count', int)])

    @property
    def _device_dtype(self):
        return self._sum_dtype

    def _source(self):
        """(stream to fetch, detection mode, n_elem) -- a GPU `Square` / `Power` in the fast
        layout is read undetected and detected in the fold kernel."""
        src = self.ih
        if (isinstance(src, _DetectTask) and not src.closed and not src._real
                and getattr(src, '_inner', 1) == 1 and not getattr(src.ih, 'closed', False)):
            return src.ih, src._mode, _prod(src.ih.shape[1:])
        n = _prod(src.shape[1:]) * (2 if np.dtype(src.dtype).kind == 'c' else 1)
        return src, 2, n

    def _run_fold(self, in0, in1, n_slot, table, out):
        """Sum input samples [in0, in1) into the ``n_slot`` rows of DeviceArray ``out``;
        ``table(c0, c1)`` -> (first slot, slot_ptr, run_begin, run_end, counts) for a chunk.
        Returns the counts per slot (int64)."""
        src, mode, n_elem = self._source()
        rows = out.reshape(n_slot, -1)
        rows.fill_bytes(0)
        counts = np.zeros(n_slot, np.int64)
        sample_bytes = _prod(src.shape[1:]) * np.dtype(src.dtype).itemsize
        per = max(1, int(self.fold_budget) // max(sample_bytes, 1))
        c0 = in0
        while True:
            c1 = min(in1, c0 + per)
            s0, sp, rb, re, cnt = table(c0, c1)
            on_device = isinstance(sp, hip.DeviceArray)        # (made there; slot_ptr is complete)
            if not on_device:
                full = np.empty(n_slot + 1, np.int64)
                full[:s0 + 1] = 0
                full[s0:s0 + len(sp)] = sp
                full[s0 + len(sp):] = sp[-1]
            counts[s0:s0 + len(cnt)] += cnt
            last = c1 >= in1
            scale = None
            if last and self.average:
                with np.errstate(divide='ignore'):
                    scale = np.where(counts > 0, 1. / np.maximum(counts, 1), np.nan).astype(np.float32)
            if len(rb) or scale is not None:
                x = fetch_device(src, c0, c1 - c0) if c1 > c0 else hip.DeviceArray((1,) + tuple(src.shape[1:]), src.dtype)
                if on_device:
                    hip.fold_runs_device(x, rows, n_elem, mode, sp, rb, re, scale=scale, accumulate=True)
                else:
                    hip.fold_runs(x, rows, n_elem, mode, full, rb, re, scale=scale, accumulate=True)
            if last:
                return counts
            c0 = c1

    def read(self, count=None, out=None):
        if self.average:
            return super().read(count, out)
        if out is not None:
            raise NotImplementedError("average=False: read() makes its own structured output.")
        count = self._prepare_read(count, None)
        first = self.offset
        sums = super().read(count, np.empty((count,) + tuple(self.sample_shape), self._sum_dtype))
        result = np.empty(sums.shape, self.dtype)
        result['data'] = sums
        cnt = self._counts(first, first + count)
        result['count'] = cnt.reshape(cnt.shape + (1,) * (sums.ndim - cnt.ndim))
        return result

    def close(self):
        super().close()
        self._drop_cache()


class Fold(_RunTableTask):
    """Fold pulse profiles in fixed time intervals (reference integration.py:306-395).

    Parameters
    ----------
    ih : stream
        float32 (e.g. the output of `Square` / `Power`) or complex64 (summed as is).
    n_phase : int
        Phase bins per pulse period.
    phase : callable
        Pulse phase for given times: receives the times of the samples it needs as one
        array-valued `~baseband_tasks_amd.units.Time`, returns cycles (a float array,
        anything with ``to_value('cycle')``, or a two-part phase with ``.int`` and
        ``.frac``).  ``lambda t: F0 * (t - t0)`` works.  Must increase with time.
        A phase that offers polynomial pieces (``fold_pieces``, as
        `~baseband_tasks_amd.phases.PolycoPhase` does) has its run tables made on the
        GPU; see `table_route`.
    step : int or float, optional
        Input samples (int) or seconds (float) per profile; default: everything.
    start : int or `~baseband_tasks_amd.units.Time`
    average : bool
        True: averages (empty bins NaN).  False: `read` returns a structured array
        with the sums in ``'data'`` and the counts in ``'count'``.
    samples_per_frame : int
        Profiles per frame.  Framing only: unlike the reference (which with
        ``samples_per_frame > 1`` counts the first input sample of a profile
        after the first in a frame into the profile before it), the output does
        not depend on it.
    dtype : optional, must equal the input dtype (as in the reference, not a conversion).

    The input sample at ``t`` goes to bin ``int((phase(t) % 1) * n_phase)``, with
    ``t`` the time of the first sample of its profile plus its offset in it
    (integration.py:389-391).  The data never leave HBM: the host builds a run
    table per chunk from the times alone (`fold_table`), and one kernel sums the
    runs (detecting a GPU `Square` / `Power` input on the way).
    """

    def __init__(self, ih, n_phase, phase, step=None, *, start=0, average=True,
                 samples_per_frame=1, dtype=None):
        n_phase = operator.index(n_phase)
        if n_phase < 1:
            raise ValueError("n_phase must be positive.")
        self._start, self._step = start, step
        ih_start = ih.seek(start)
        ih_n = ih.shape[0] - ih_start
        if ih_start < 0 or ih_n < 0:
            raise ValueError("'start' is not within the underlying stream.")
        rate = _stream_rate(ih)
        t_start = ih.time
        ih_start_f = float(ih_start)
        if u.is_time(start):
            # (the start need not be at a sample)
            ih_start_f += (Time(start) - t_start) * rate
            t_start = Time(start)
        if step is None:
            step = ih_n
        if _is_index(step):
            step = operator.index(step)
            sample_rate = rate / step
            n_sample = ih_n / step
        else:
            step_s = u.to_seconds(step)
            sample_rate = 1. / step_s
            n_sample = (ih.stop_time - t_start) * sample_rate
        self._mean_offset_size = n_sample / ih_n if ih_n else 1.
        n_out = int(n_sample + 0.5 * self._mean_offset_size)
        assert n_out >= 1, "time per frame larger than total time in stream"
        self._ih_start = ih_start_f
        self.n_phase = n_phase
        self.phase = phase
        out_dtype = self._init_source(ih, dtype, average)
        super().__init__(ih, shape=(n_out, n_phase) + tuple(ih.shape[1:]), sample_rate=sample_rate,
                         samples_per_frame=samples_per_frame, start_time=t_start, dtype=out_dtype)

    def _get_offsets(self, samples):
        """Input offsets of output rows (integration.py:184-186)."""
        return np.around(np.asarray(samples) / self._mean_offset_size + self._ih_start).astype(np.int64)

    def _row_phase(self, edges):
        ih, rate = self.ih, _stream_rate(self.ih)
        phase = self.phase

        def row(r):
            # (the times the reference gives a row: its first sample's, plus offsets)
            n_ref = int(edges[r])
            t_ref = ih._tell_time(n_ref) if hasattr(ih, '_tell_time') else _stream_start(ih) + n_ref / rate
            times = sample_times(t_ref, n_ref, rate)
            return lambda n: phase(times(n))
        return row

    #: where the run tables of a phase that offers polynomial pieces (``fold_pieces``, see
    #: INTEGRATION.md) are made: 'device' (the table kernel), 'host' (NumPy, every sample), or
    #: None: the environment's BBT_FOLD_TABLE, else 'device'.  Both give the same table, and both
    #: refuse (ValueError) a phase whose bin steps back inside a row.
    table_route = None

    def _route(self):
        route = self.table_route or os.environ.get('BBT_FOLD_TABLE', '') or 'device'
        if route not in ('device', 'host'):
            raise ValueError(f"table route {route!r}: must be 'device' or 'host'")
        return route

    def _row_pieces(self, edges):
        ih, rate = self.ih, _stream_rate(self.ih)
        fold_pieces = self.phase.fold_pieces

        def pieces(r, lo, hi):
            n_ref = int(edges[r])
            t_ref = ih._tell_time(n_ref) if hasattr(ih, '_tell_time') else _stream_start(ih) + n_ref / rate
            return fold_pieces(t_ref, rate, lo - n_ref, hi - n_ref)
        return pieces

    def _tables(self, a, b):
        """Row edges and the chunk table function for rows [a, b)."""
        edges = self._get_offsets(np.arange(a, b + 1))
        n_phase = self.n_phase
        if hasattr(self.phase, 'fold_pieces'):
            row_pieces = self._row_pieces(edges)
            n_slot = (b - a) * n_phase

            def host_table(c0, c1):
                r0, n_row, sp, rb, re, cnt = piece_table(edges, row_pieces, n_phase, c0, c1)
                return r0 * n_phase, sp, rb, re, cnt

            def device_table(c0, c1):
                r0, n_row, plan = plan_pieces(edges, row_pieces, n_phase, c0, c1)
                if plan is None:
                    return host_table(c0, c1)              # (no samples: an empty table)
                sp, rb, re, n_run, cnt = hip.phase_runs(plan, n_phase, r0 * n_phase, n_slot)
                return r0 * n_phase, sp, rb, re, cnt
            return edges, (device_table if self._route() == 'device' else host_table)
        row_phase = self._row_phase(edges)

        def table(c0, c1):
            r0, n_row, sp, rb, re, cnt = fold_table(edges, row_phase, n_phase, c0, c1)
            return r0 * n_phase, sp, rb, re, cnt
        return edges, table

    def _compute_frames(self, first, last, out):
        a, b = self._frame_span(first, last)
        edges, table = self._tables(a, b)
        self._run_fold(int(edges[0]), int(edges[-1]), (b - a) * self.n_phase, table, out)

    def _counts(self, a, b):
        edges, table = self._tables(a, b)
        _, sp, rb, re, cnt = table(int(edges[0]), int(edges[-1]))      # (on either route, counts on the host)
        out = np.zeros((b - a) * self.n_phase, np.int64)
        out[:len(cnt)] = cnt
        return out.reshape(b - a, self.n_phase)


class _PhaseIntegrate(_RunTableTask):
    """``Integrate(ih, step, phase)``: output sample ``k`` sums the contiguous input samples
    [off(k), off(k+1)) with the offsets found by the reference's iterative solve
    (integration.py:174-228).  The task's times are those of the input at the offsets."""

    _time_from_offsets = True

    def __init__(self, ih, step=None, phase=None, *, start=0, average=True,
                 samples_per_frame=1, dtype=None):
        assert not _is_index(step), 'cannot pass in phase and integer step'
        self._start, self._step = start, step
        ih_start = ih.seek(start)
        ih_n = ih.shape[0] - ih_start
        if ih_start < 0 or ih_n < 0:
            raise ValueError("'start' is not within the underlying stream.")
        rate = _stream_rate(ih)
        t_start = ih.time
        ih_start_f = float(ih_start)
        if u.is_time(start):
            ih_start_f += (Time(start) - t_start) * rate
            t_start = Time(start)
        step_c = float(step.to_value('cycle')) if hasattr(step, 'to_value') else float(step)
        self._phase = phase
        self._sample_start = phase(_array_time(t_start))
        stop_phase = phase(_array_time(ih.stop_time))
        n_sample = float(phase_difference(stop_phase, self._sample_start)[0]) / step_c
        self._mean_offset_size = n_sample / ih_n if ih_n else 1.
        self._ih_start = ih_start_f
        self._step_c = step_c
        n_out = int(n_sample + 0.5 * self._mean_offset_size)
        assert n_out >= 1, "time per frame larger than total time in stream"
        out_dtype = self._init_source(ih, dtype, average)
        super().__init__(ih, shape=(n_out,) + tuple(ih.shape[1:]), sample_rate=1. / step_c,
                         samples_per_frame=samples_per_frame, start_time=t_start, dtype=out_dtype)
        self._edges = None

    @property
    def phase(self):
        return self._phase

    def _get_offsets(self, samples, precision=1.e-3, max_iter=10):
        """Input offsets nearest to the output samples (the reference's solve)."""
        phase = np.ravel(samples) / self.sample_rate
        ih_mean_phase_size = self._mean_offset_size / self.sample_rate
        offsets = phase / ih_mean_phase_size
        all_offsets = np.hstack((0, offsets, self.ih.shape[0] - self._ih_start))
        all_ih_phase = all_offsets * ih_mean_phase_size
        all_offsets += self._ih_start
        offsets = all_offsets[1:-1]
        ih_phase = all_ih_phase[1:-1]
        mask = np.ones(offsets.shape, bool)
        ih_t0 = Time(self.ih.start_time)
        rate = _stream_rate(self.ih)
        it = 0
        while np.any(mask) and it < max_iter:
            old_offsets = offsets[mask]
            ih_time = ih_t0 + old_offsets / rate
            ih_phase[mask] = phase_difference(self._phase(ih_time), self._sample_start)
            offsets[mask] = np.interp(phase[mask], all_ih_phase, all_offsets)
            mask[mask] = abs(offsets[mask] - old_offsets) > precision
            it += 1
        if it >= max_iter:  # pragma: no cover
            warnings.warn('offset calculation did not converge. This should not happen!')
        shape = getattr(samples, 'shape', ())
        return offsets.round().astype(np.int64).reshape(shape)

    @property
    def edges(self):
        """Input offsets of output samples 0 .. n (solved once, for all of them)."""
        if self._edges is None:
            self._edges = self._get_offsets(np.arange(self.shape[0] + 1))
        return self._edges

    def _tell_time(self, offset):
        return self.ih._tell_time(int(self.edges[offset]))

    def _fold_samples(self, a, b, out):
        edges = self.edges[a:b + 1]

        def table(c0, c1):
            r0, n, sp, rb, re, cnt = contiguous_table(edges, c0, c1)
            return r0, sp, rb, re, cnt
        return self._run_fold(int(edges[0]), int(edges[-1]), b - a, table, out)

    def _compute_frames(self, first, last, out):
        a, b = self._frame_span(first, last)
        self._fold_samples(a, b, out)

    def _counts(self, a, b):
        return np.diff(self.edges[a:b + 1])

    def _repr_item(self, key, default, value=None):
        if key == 'phase':
            return f"phase={self._phase!r}"
        return super()._repr_item(key, default, value)


class PulseStack(_RunTableTask):
    """Pulse stacks: ``Integrate(ih, 1 / n_phase cycle, phase)`` reshaped to
    ``(cycles, n_phase) + sample_shape``; an incomplete last cycle is dropped
    (reference integration.py:398-478).  Parameters as for `Fold`; ``phase`` must
    include the cycle count."""

    _time_from_offsets = True

    def __init__(self, ih, n_phase, phase, *, start=0, average=True, samples_per_frame=1,
                 dtype=None):
        n_phase = operator.index(n_phase)
        phased = Integrate(ih, 1. / n_phase, phase, start=start, average=average,
                           samples_per_frame=samples_per_frame * n_phase, dtype=dtype)
        self._phased = phased
        self.n_phase = n_phase
        self._start = start
        self._init_source(ih, dtype, average)
        n_cycle = phased.shape[0] // n_phase
        assert n_cycle >= 1, "less than one pulse period in the stream"
        super().__init__(ih, shape=(n_cycle, n_phase) + tuple(ih.shape[1:]),
                         sample_rate=phased.sample_rate / n_phase, samples_per_frame=samples_per_frame,
                         start_time=phased.start_time, dtype=phased.dtype)

    @property
    def phase(self):
        return self._phased.phase

    def _tell_time(self, offset):
        return self._phased._tell_time(offset * self.n_phase)

    def _compute_frames(self, first, last, out):
        a, b = self._frame_span(first, last)
        self._phased._fold_samples(a * self.n_phase, b * self.n_phase, out)

    def _counts(self, a, b):
        return self._phased._counts(a * self.n_phase, b * self.n_phase).reshape(b - a, self.n_phase)
