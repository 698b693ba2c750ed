"""Modulation of a stream by a pulse profile on the GPU: `Modulate`, the mirror image of
`~baseband_tasks_amd.integration.Fold` (the reference modulates through its generic ``Task``
with a callable per frame: baseband_tasks/tests/test_simulate.py, ``TestModulation`` and
``TestCyclicModulation``)."""
import os

import numpy as np

from . import hip
from .base import BaseTaskBase, _stream_rate, check_broadcast_to
from .device_task import ChunkedDeviceTask
from .fold_table import PIECE, bin_runs, plan_pieces, polynomial_bins, sample_times, unwrapped_bin

__all__ = ['Modulate', 'modulate_samples']


def _prod(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def modulate_samples(data, profile, bins):
    """NumPy restatement of the modulation kernels: ``data[n] * profile[bins[n]]``.

    ``data``: (n,) + sample_shape, float32 or complex64; ``profile``: real, (n_phase,) + s with
    ``s`` broadcastable to the sample shape, rounded to float32; ``bins``: (n,) wrapped phase
    bins.  A complex sample times a real gain is two float32 products, as on the GPU (and as
    NumPy's complex product for finite data)."""
    data = np.asarray(data)
    gain = np.asarray(profile).astype(np.float32)[np.asarray(bins, dtype=np.int64)]
    gain = gain.reshape(gain.shape[:1] + (1,) * (data.ndim - gain.ndim) + gain.shape[1:])
    if data.dtype.kind == 'c':
        out = np.empty(data.shape, np.complex64)
        out.real = data.real.astype(np.float32) * gain
        out.imag = data.imag.astype(np.float32) * gain
        return out
    return data.astype(np.float32) * gain


def _time_ordered(starts, ks, n_phase, c0):
    """Run starts (absolute) and unwrapped bins, frame by frame -> (run_begin relative to c0,
    wrapped bins), int64."""
    return (np.concatenate(starts) - c0).astype(np.int64), (np.concatenate(ks) % n_phase).astype(np.int64)


class Modulate(ChunkedDeviceTask, BaseTaskBase):
    """Multiply a stream by a pulse profile: every sample by the gain of its phase bin.

    Parameters
    ----------
    ih : stream
        float32 or complex64, any sample shape.
    profile : array
        Real gains, rounded once to float32: shape ``(n_phase,)`` (one gain per phase bin for
        all elements of a sample) or ``(n_phase,) + s`` with ``s`` broadcastable to the sample
        shape (a gain per bin and element).  The gain multiplies amplitudes: for an intensity
        profile ``I`` pass ``sqrt(I)``.
    phase : callable
        Pulse phase for given times, as for `~baseband_tasks_amd.integration.Fold`: a callable
        on an array-valued `~baseband_tasks_amd.units.Time` that returns cycles (a float array,
        anything with ``to_value('cycle')``, or a two-part phase with ``.int`` and ``.frac``),
        or an object that offers polynomial pieces (``fold_pieces``, as
        `~baseband_tasks_amd.phases.PolycoPhase` does).  Must increase with time.
    samples_per_frame : int, optional
        Default: that of ``ih``.

    Shape, dtype, sample rate, start time, ``frequency``, ``sideband`` and ``polarization`` are
    those of ``ih``.  Output sample ``n`` is ::

        out[n, ...] = in[n, ...] * profile[b(n), ...],   b(n) = int((phase(t_n) % 1) * n_phase)

    (``b`` clipped to ``n_phase - 1``): `Fold`'s bin rule (`fold_table.unwrapped_bin`,
    `fold_table.polynomial_bins`), wrapped.  ``t_n`` is the time of the first sample of the
    output frame that holds ``n`` plus the offset of ``n`` in that frame, the expression
    `Fold` evaluates for a profile whose first sample is the frame's: a `Fold` of this stream
    with the same ``phase``, the same start and an integer ``step`` equal to this task's
    ``samples_per_frame`` puts every sample into the bin whose gain it got, and so recovers
    ``count * profile`` exactly.

    The bins depend on the framing only through rounding at bin edges: ``t_n`` is the same
    instant whatever the frame, but it reaches the phase callable as (frame start) + (offset),
    and a float64 phase of a time split differently can differ in its last bits, which moves
    a sample that lies within that rounding of a bin edge into the neighbouring bin.

    Nothing leaves HBM: host callables give a table of runs of constant bin per call
    (`fold_table.bin_runs` per frame) that one kernel applies; a phase with ``fold_pieces``
    has its bins evaluated in the kernel itself (`table_route`).  Unlike the reference's
    ``Task``-based modulation, which applies one gain per frame (that of the frame's centre),
    the gain here is per phase bin and per sample, whatever the framing.
    """

    #: input bytes fetched at most per `fetch_device` call and launch (assignable)
    modulate_budget = 1 << 29

    #: where the bins of a phase that offers polynomial pieces (``fold_pieces``) are found:
    #: 'device' (in the modulation kernel, from the pieces), 'host' (NumPy, every sample, as
    #: runs), or None: the environment's BBT_FOLD_TABLE, else 'device'.  Both give the same
    #: output bit for bit.
    table_route = None

    def __init__(self, ih, profile, phase, *, samples_per_frame=None):
        in_dtype = np.dtype(ih.dtype)
        if in_dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
            raise TypeError(f"the accelerated Modulate handles float32/complex64; got {in_dtype}.")
        profile = np.asarray(profile)
        if profile.dtype.kind == 'c':
            raise TypeError("the profile must be real (a gain per phase bin).")
        profile = profile.astype(np.float32)
        if profile.ndim < 1 or profile.shape[0] < 1:
            raise ValueError("the profile needs at least one phase bin along its first axis.")
        sample_shape = tuple(ih.shape[1:])
        check_broadcast_to(profile[0], sample_shape)
        self.profile = profile
        self.n_phase = profile.shape[0]
        self.phase = phase
        self._n_elem = _prod(sample_shape)
        if all(d == 1 for d in profile.shape[1:]):
            self._gain_host = np.ascontiguousarray(profile.reshape(self.n_phase))
        else:
            aligned = profile.reshape((self.n_phase,) + (1,) * (len(sample_shape) - profile.ndim + 1)
                                      + profile.shape[1:])
            self._gain_host = np.ascontiguousarray(
                np.broadcast_to(aligned, (self.n_phase,) + sample_shape)).reshape(self.n_phase, self._n_elem)
        self._gain = None
        super().__init__(ih, samples_per_frame=samples_per_frame)

    # -- bins ---------------------------------------------------------------------
    def _route(self):
        route = self.table_route or os.environ.get('BBT_FOLD_TABLE', '') or 'device'
        if route not in ('device', 'host'):
            raise ValueError(f"table route {route!r}: must be 'device' or 'host'")
        return route

    def _frame_edges(self, c0, c1):
        """Edges of the output frames that meet samples [c0, c1)."""
        spf = self.samples_per_frame
        edges = np.arange(c0 // spf, (c1 - 1) // spf + 2, dtype=np.int64) * spf
        return np.minimum(edges, self.shape[0])

    def _row_phase(self, edges):
        # (as Fold._row_phase, for rows that are this task's frames)
        rate, phase = _stream_rate(self), self.phase

        def row(r):
            n_ref = int(edges[r])
            times = sample_times(self._tell_time(n_ref), n_ref, rate)
            return lambda n: phase(times(n))
        return row

    def _row_pieces(self, edges):
        # (as Fold._row_pieces)
        rate, fold_pieces = _stream_rate(self), self.phase.fold_pieces

        def pieces(r, lo, hi):
            n_ref = int(edges[r])
            return fold_pieces(self._tell_time(n_ref), rate, lo - n_ref, hi - n_ref)
        return pieces

    def _runs(self, c0, c1):
        """The time-ordered run table of samples [c0, c1) made on the host: (run_begin relative
        to c0, wrapped bin of each run), from `bin_runs` per frame for a callable and from
        `polynomial_bins` of every sample for a phase with pieces."""
        edges = self._frame_edges(c0, c1)
        n_phase = self.n_phase
        starts, ks = [], []
        if hasattr(self.phase, 'fold_pieces'):
            row_pieces = self._row_pieces(edges)
            for r in range(len(edges) - 1):
                lo, hi = max(c0, int(edges[r])), min(c1, int(edges[r + 1]))
                n_ref = int(edges[r])
                for (m0, m1, coeff, dt0, step, ref_int, ref_frac) in row_pieces(r, lo, hi):
                    for a in range(m0, m1, PIECE):
                        m = np.arange(a, min(m1, a + PIECE), dtype=np.int64)
                        k = polynomial_bins(coeff, dt0, step, ref_int, ref_frac, m, n_phase)
                        new = np.concatenate((np.ones(1, bool), k[1:] != k[:-1]))
                        starts.append(m[new] + n_ref)
                        ks.append(k[new])
        else:
            row_phase = self._row_phase(edges)
            for r in range(len(edges) - 1):
                lo, hi = max(c0, int(edges[r])), min(c1, int(edges[r + 1]))
                b, e, k = bin_runs(row_phase(r), n_phase, lo, hi)
                starts.append(b)
                ks.append(k)
        return _time_ordered(starts, ks, n_phase, c0)

    def bins(self, first, count):
        """The wrapped phase bin of samples ``first .. first + count - 1``, evaluated for every
        sample on the host (what the kernels are checked against)."""
        c0, c1 = int(first), int(first) + int(count)
        if not 0 <= c0 <= c1 <= self.shape[0]:
            raise ValueError("samples outside the stream.")
        out = np.empty(c1 - c0, np.int64)
        if c1 == c0:
            return out
        edges = self._frame_edges(c0, c1)
        by_pieces = hasattr(self.phase, 'fold_pieces')
        rows = self._row_pieces(edges) if by_pieces else self._row_phase(edges)
        for r in range(len(edges) - 1):
            lo, hi = max(c0, int(edges[r])), min(c1, int(edges[r + 1]))
            if by_pieces:
                n_ref = int(edges[r])
                for (m0, m1, coeff, dt0, step, ref_int, ref_frac) in rows(r, lo, hi):
                    m = np.arange(m0, m1, dtype=np.int64)
                    out[m0 + n_ref - c0:m1 + n_ref - c0] = polynomial_bins(coeff, dt0, step, ref_int, ref_frac, m,
                                                                            self.n_phase) % self.n_phase
            else:
                out[lo - c0:hi - c0] = unwrapped_bin(rows(r)(np.arange(lo, hi, dtype=np.int64)),
                                                     self.n_phase) % self.n_phase
        return out

    # -- frames ---------------------------------------------------------------------
    def _chunk_size(self):
        sample_bytes = self._n_elem * np.dtype(self.dtype).itemsize
        return max(1, int(self.modulate_budget) // max(sample_bytes, 1))

    def _launch(self, x, start, count, out, c0, c1):
        if self._gain is None:
            self._gain = hip.DeviceArray.from_host(self._gain_host)
        if hasattr(self.phase, 'fold_pieces') and self._route() == 'device':
            edges = self._frame_edges(c0, c1)
            plan = plan_pieces(edges, self._row_pieces(edges), self.n_phase, c0, c1)[2]
            hip.modulate_pieces(x, out, self._n_elem, self._gain, plan)
        else:
            run_begin, run_bin = self._runs(c0, c1)
            hip.modulate_runs(x, out, self._n_elem, self._gain, run_begin, run_bin)

    def _repr_item(self, key, default, value=None):
        if key == 'phase':
            return f"phase={self.phase!r}"
        return super()._repr_item(key, default, value)

    def close(self):
        super().close()
        self._gain = None
