"""Cross-correlation on the GPU: the visibilities of up to 64 inputs of one stream.

`Correlate` multiplies every input of a complex64 stream by the conjugate of every other and of itself
and integrates the products over blocks of ``n`` samples, in HBM.  It is what `TimeDelay`, `Stack` and
`Channelize` lead up to: ``Correlate(Channelize(Stack([...], axis=1), nchan), n)`` gives the visibilities per
channel.  The reference has no correlator; `Power` is the one for exactly two inputs along a polarization
axis, and this task follows its convention (``x_i conj(x_j)``).  `correlate_samples` restates the values in
NumPy, in float64: it is the reference for the values, not a bit-for-bit twin.
"""
import operator

import numpy as np

from . import hip
from .base import META_ATTRIBUTES, BaseTaskBase, _stream_rate, check_broadcast_to, simplify_shape
from .device_task import ChunkedDeviceTask, fetch_device
from .search import _init_with_band_of
from .shaping import Transpose

__all__ = ['Correlate', 'correlate_samples', 'baseline_pairs']

#: samples of a segment of the summation rule (BBT_CORR_SEG in csrc/corr_geo.hpp): a constant of the rule
SEG = hip.CORR_SEG


def _prod(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def _check_inputs(a):
    a = operator.index(a)
    if not hip.CORR_MIN_INPUTS <= a <= hip.CORR_MAX_INPUTS:
        raise ValueError(f"the correlated axis must hold {hip.CORR_MIN_INPUTS} ... {hip.CORR_MAX_INPUTS} inputs, not {a}.")
    return a


def _check_n(n):
    n = operator.index(n)
    if not 1 <= n <= hip.CORR_MAX_N:
        raise ValueError(f"n must be 1 ... 2^24 samples, not {n}.")
    return n


def _sample_axis(axis, ndim):
    """``axis`` of a sample shape of ``ndim`` axes as a non-negative index."""
    axis = operator.index(axis)
    if not -ndim <= axis < ndim:
        raise ValueError(f"axis {axis} is out of bounds for a sample shape of {ndim} axes.")
    return axis % ndim


def baseline_pairs(n_inputs):
    """The baselines of `Correlate` in its order: an int array ``(B, 2)`` of ``(i, j)``, ``i <= j``, row-major --
    ``(0,0), (0,1), ..., (0,A-1), (1,1), ...`` -- with ``B = A (A + 1) / 2``."""
    a = _check_inputs(n_inputs)
    i, j = np.triu_indices(a)
    return np.stack([i, j], axis=1).astype(np.int64)


def correlate_samples(x, n, axis=-1, average=True):
    """What `Correlate` computes, in NumPy and float64, rounded once to complex64 at the end.

    ``x``: ``(N,) + sample_shape``, complex; ``axis`` counts the axes of the sample shape, as for `Correlate`.
    Returns ``(N // n,) + s'``, ``s'`` the sample shape with ``axis`` replaced by the baselines of `baseline_pairs`:
    ``sum_t x_i(t) conj(x_j(t))`` over each block of ``n`` samples, divided by ``n`` if ``average``."""
    x = np.asarray(x)
    n = _check_n(n)
    if x.ndim < 2:
        raise ValueError("x must be (N,) + sample_shape with an axis of inputs.")
    ax = _sample_axis(axis, x.ndim - 1)
    pairs = baseline_pairs(x.shape[1 + ax])
    nb = x.shape[0] // n
    y = np.moveaxis(x[:nb * n], 1 + ax, -1).astype(np.complex128)
    y = y.reshape((nb, n) + y.shape[1:])
    vis = np.einsum('bt...i,bt...j->b...ij', y, y.conj())[..., pairs[:, 0], pairs[:, 1]]
    if average:
        vis = vis / np.float64(n)
    return np.ascontiguousarray(np.moveaxis(vis, -1, 1 + ax)).astype(np.complex64)


class Correlate(ChunkedDeviceTask, BaseTaskBase):
    """Cross-products of the inputs of a stream, integrated over blocks of ``n`` samples: the visibilities.

    Parameters
    ----------
    ih : stream
        complex64, any sample shape.
    n : int
        Samples of an integration, 1 ... 2^24, counted from sample 0 of ``ih``; a tail shorter than ``n`` is
        dropped.
    axis : int, optional
        The axis of the SAMPLE shape that holds the inputs, ``A = ih.sample_shape[axis]``, 2 ... 64.  Default
        -1, the fast layout (inputs adjacent): what ``Channelize(Stack([...], axis=1), nchan)`` makes.  Another
        axis is brought last by a `Transpose` inside the task.
    average : bool, optional
        Divide the sums by ``n`` (default); otherwise the sums themselves, as complex64.
    samples_per_frame : int, optional
        Of the output (integrations).  Default 1.

    The output is complex64 ``(len // n,) + s'`` at ``sample_rate / n`` from ``ih``'s start time, ``s'`` the sample
    shape with ``axis`` replaced by the ``B = A (A + 1) / 2`` baselines ``(i, j)``, ``i <= j``, in the order of
    `baseline_pairs` (also ``.baselines``); a value is ``sum_t x_i(t) conj(x_j(t))``, `Power`'s convention -- for
    ``A = 2`` the rows are XX, XY, YY.  Metadata that vary along ``axis`` (usually ``polarization``) are dropped,
    the others pass through.

    The rule: a block is cut into segments of 1024 samples from its first sample; per segment and baseline
    four float32 chains run in sample order, one fused multiply-add per sample (``rr += re_i re_j``, ``ii += im_i
    im_j``, ``ir += im_i re_j``, ``ri += re_i im_j``), then ``Re = rr + ii`` and ``Im = ir - ri``; the segment values are
    added in float64 in order, divided by ``n`` in float64, and rounded once to float32.  So no value depends
    on the budget, the framing, a seek or the tiling, and the imaginary part of an autocorrelation is
    exactly +0.  `correlate_samples` gives the values in float64; the kernel stays within ``(min(n, 1024) + 4)
    2^-24 sum |a b|`` of it.  The chains run on the matrix cores (``v_mfma_f32_32x32x2_f32``, exact float32).  There
    is no structured output with counts, no selection of autos or crosses, no second stream, no weights."""

    #: input bytes fetched at most per `fetch_device` call and launch (assignable): whole blocks where one
    #: fits, else whole segments of one block, one segment at least
    correlate_budget = 1 << 29

    def __init__(self, ih, n, axis=-1, *, average=True, samples_per_frame=1):
        if np.dtype(ih.dtype) != np.dtype(np.complex64):
            raise TypeError(f"Correlate handles complex64 streams; got {np.dtype(ih.dtype)}.")
        sample_shape = tuple(ih.shape[1:])
        if not sample_shape:
            raise ValueError("Correlate needs a sample shape with an axis of inputs.")
        self.axis = ax = _sample_axis(axis, len(sample_shape))
        self.n_inputs = a = _check_inputs(sample_shape[ax])
        self.n = n = _check_n(n)
        self.average = bool(average)
        if ih.shape[0] < n:
            raise ValueError(f"the stream has {ih.shape[0]} samples: less than one integration of {n}.")
        self.baselines = baseline_pairs(a)
        nbl = self.baselines.shape[0]
        self._n_elem = _prod(sample_shape) // a
        self._inner = _prod(sample_shape[ax + 1:])
        # metadata that do not vary along the inputs pass through, with that axis of length 1
        kept = {}
        for attr in META_ATTRIBUTES:
            value = getattr(ih, attr, None)
            if value is not None:
                full = check_broadcast_to(value, sample_shape)
                first = full[(slice(None),) * ax + (slice(0, 1),)]
                if np.all(full == first):
                    kept[attr] = simplify_shape(np.asanyarray(first))
        if 'frequency' not in kept:
            kept.pop('sideband', None)
        elif 'sideband' not in kept and getattr(ih, 'sideband', None) is not None:
            del kept['frequency']                                     # (the two go together)
        _init_with_band_of(self, ih, shape=(ih.shape[0] // n,) + sample_shape[:ax] + (nbl,) + sample_shape[ax + 1:],
                           sample_rate=_stream_rate(ih) / n, samples_per_frame=operator.index(samples_per_frame),
                           dtype=np.complex64)
        if kept:
            self.meta['__attributes__'] = kept
        else:
            self.meta.pop('__attributes__', None)
        # the inputs adjacent: the stream itself, or its transpose
        nd = len(sample_shape)
        self._src = ih if ax == nd - 1 else Transpose(ih, tuple(k + 1 for k in range(nd) if k != ax) + (ax + 1,))

    def _check_shape(self, value):
        # (the inherited metadata describe the inputs' axis; they are replaced once the stream is set up)
        return simplify_shape(np.asanyarray(value))

    def _sample_bytes(self):
        return self._n_elem * self.n_inputs * 8

    def _chunk_size(self):
        return max(1, int(self.correlate_budget) // (self.n * self._sample_bytes()))

    def _piece_size(self):
        """The samples of a fetch at most: whole blocks, or whole segments of one block."""
        row = self._sample_bytes()
        if self.n * row <= int(self.correlate_budget):
            return self._chunk_size() * self.n
        return max(1, int(self.correlate_budget) // (SEG * row)) * SEG

    def _chunk_input(self, b0, b1):
        return b0 * self.n, (b1 - b0) * self.n

    def _input_span(self, first, last):
        a, b = self._frame_span(first, last)
        start, count = self._chunk_input(a, b)
        return (self._src, start, count) if count <= self._piece_size() else None     # (one fetch only)

    def _make_plan(self):
        return hip.CorrPlan(self.n_inputs, self._n_elem, self.n, self._inner, self.average)

    def _compute_frames(self, first, last, out):
        if not self._plan_made:
            self._plan, self._plan_made = self._make_plan(), True
        a, b = self._frame_span(first, last)
        per, piece = self._chunk_size(), self._piece_size()
        for c0 in range(a, b, per):
            c1 = min(b, c0 + per)
            start, count = self._chunk_input(c0, c1)
            # (a chunk of more than one piece is one block, so every piece begins at a segment of it)
            for p0 in range(start, start + count, piece):
                pc = min(piece, start + count - p0)
                x = fetch_device(self._src, p0, pc)
                self._plan.execute(x, p0, pc, out[c0 - a:c1 - a], c0, c1 - c0)

    def close(self):
        src = self.__dict__.pop('_src', None)
        if src is not None and src is not self.__dict__.get('ih'):
            src.close()
        super().close()
