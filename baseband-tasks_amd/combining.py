"""Combining streams on the GPU (reference baseband_tasks/combining.py).

Stacking or concatenating streams moves samples and computes nothing: each
element of an output sample is a copy of one element of one input stream's
sample at the same time.  As in `~baseband_tasks_amd.shaping`, ``task`` is
applied once, to label arrays, and the index map that comes back is executed
by one gather plan (libbbt_hip: bbt_gather_*) on the streams where they are,
in HBM: one kernel launch per run of frames, whatever the number of streams.

Differences from the reference: the callable of `CombineStreams` must be a
rearrangement (``np.stack``, ``np.concatenate``, indexing, ...; one that
computes is refused with `TypeError`), and it is called on label arrays at
construction rather than on data at every frame.  At most 64 streams.
"""
import numpy as np

from . import hip
from . import units as u
from .base import Task, TaskBase, META_ATTRIBUTES, _stream_rate
from .device_task import DeviceTaskMixin, cache_producer, fetch_device, views_to_keep
from .hip import DeviceArray
from .shaping import index_map, _prod

__all__ = ['CombineStreamsBase', 'CombineStreams', 'Concatenate', 'Stack']


class CombineStreamsBase(DeviceTaskMixin, TaskBase):
    """Base class for combining streams (reference combining.py:11-137).

    A subclass defines ``task(data)``, with ``data`` a list of arrays that
    share the time axis, one per stream.  This class checks that the streams
    can be combined, finds their common time span, and combines their
    ``frequency``, ``sideband`` and ``polarization`` in the same way (on the
    host).

    Parameters
    ----------
    ihs : tuple of task or stream readers
        Input data streams: same ``sample_rate`` and ``dtype``; the output
        covers the time from the latest start to the earliest stop.  Streams
        that are not on the device are uploaded as for every other task.
        Streams that reach the same device task (the same task twice, windows
        or relabelled copies of one task) are read one after the other, and the
        view each read hands over lives until the next read of that task: all
        but the last are copied (one device-to-device copy each); streams with
        distinct producers are gathered from where they are.
    atol : float (seconds) or time quantity, optional
        Tolerance within which streams should be considered aligned.  By
        default, the lesser of 1 ns and 0.01 sample.
    samples_per_frame : int, optional
        By default the number of the first stream.
    **kwargs
        Additional arguments to be passed on to the base class.
    """
    _plan = None
    _keep = None
    #: Route of the gather plan: 'auto', or 'run_copy', 'tile', 'direct' to force one (tests).
    ROUTE = 'auto'

    def __init__(self, ihs, *, atol=None, samples_per_frame=None, **kwargs):
        try:
            ih0 = ihs[0]
        except (TypeError, IndexError) as exc:
            exc.args += ("Need an iterable containing at least one stream.",)
            raise
        ihs = list(ihs)
        if len(ihs) > 64:
            raise ValueError(f"at most 64 streams can be combined in one task; got {len(ihs)}.")
        rate = _stream_rate(ih0)
        start_time = u.Time(ih0.start_time)
        stop_time = u.Time(ih0.stop_time)
        for ih in ihs[1:]:
            assert _stream_rate(ih) == rate
            assert ih.dtype == ih0.dtype
            start_time = max(start_time, u.Time(ih.start_time))
            stop_time = min(stop_time, u.Time(ih.stop_time))
        # First sample of each stream in the common span, and how well they are aligned.
        firsts, n, max_offset = [], None, 0.
        for ih in ihs:
            t0 = u.Time(ih.start_time)
            first = int(round((start_time - t0) * rate))
            stop = int(round((stop_time - t0) * rate))
            firsts.append(first)
            n = stop - first if n is None else min(n, stop - first)
            max_offset = max(max_offset, abs((t0 + first / rate) - start_time))
        if atol is None:
            atol = min(1e-9, 0.01 / rate)
        else:
            atol = u.to_seconds(atol)
        if max_offset > atol:
            raise ValueError(f"streams only aligned to {max_offset} s, "
                             f"not within {atol} s.")
        # Check that the stream samples can be combined.
        fakes = [np.empty((7,) + tuple(ih.sample_shape), ih.dtype) for ih in ihs]
        try:
            a = self.task(fakes)
        except Exception as exc:
            exc.args += ("streams with sample shapes {} cannot be combined "
                         "as required".format([f.shape[1:] for f in fakes]),)
            raise
        if a.shape[0] != 7:
            raise ValueError("combination affected the sample axis (0).")
        out_shape, self._map_src, self._map_elem = index_map(
            self.task, [tuple(ih.sample_shape) for ih in ihs], combine=True)
        assert tuple(out_shape) == tuple(a.shape[1:])
        self.ihs = ihs
        self._firsts = firsts
        for attr in META_ATTRIBUTES:
            if attr not in kwargs:
                kwargs[attr] = self._combine_attr(attr)
        super().__init__(ih0, start_time=start_time, shape=(n,) + tuple(a.shape[1:]),
                         samples_per_frame=samples_per_frame, **kwargs)

    def _combine_attr(self, attr):
        """Combine the given attribute from all streams: None if all are None."""
        values = [getattr(ih, attr, None) for ih in self.ihs]
        if all(value is None for value in values):
            return None
        values = [np.broadcast_to(value, (1,) + tuple(ih.sample_shape), subok=True)
                  for value, ih in zip(values, self.ihs)]
        try:
            result = self.task(values)
        except Exception as exc:
            exc.args += ("the {} attribute of the streams cannot be combined "
                         "as required".format(attr),)
            raise
        return result[0]

    def _get_plan(self):
        if self._plan is None:
            self._plan = hip.GatherPlan([_prod(ih.sample_shape) for ih in self.ihs], self._map_src,
                                        self._map_elem, np.dtype(self.dtype).itemsize, route=self.ROUTE)
        return self._plan

    @property
    def route(self):
        """Route of the gather plan ('run_copy', 'tile' or 'direct')."""
        return self._get_plan().info()['route']

    def _input_span(self, first, last):
        start, stop = self._frame_span(first, last)
        return self.ihs[0], self._firsts[0] + start, stop - start

    def _compute_frames(self, first, last, out):
        start, stop = self._frame_span(first, last)
        used = set(np.unique(self._map_src).tolist())
        if self._keep is None:
            # (inputs that share a producer: the next fetch from it may refill the frame cache
            # that the view of this one lies in)
            self._keep = views_to_keep([cache_producer(ih) if k in used else None
                                        for k, ih in enumerate(self.ihs)])
        xs = []
        for k, (ih, f) in enumerate(zip(self.ihs, self._firsts)):
            x = fetch_device(ih, f + start, stop - start) if k in used else None
            if self._keep[k]:
                x = DeviceArray(x.shape, x.dtype).copy_from_device(x)
            xs.append(x)
        self._get_plan().execute(xs, out, stop - start)

    def close(self):
        super().close()
        self._drop_cache()
        if self._plan is not None:
            self._plan.close()
            self._plan = None
        for ih in self.ihs[1:]:
            ih.close()

    def _repr_item(self, key, default, value=None):
        if key == 'ihs':
            return 'ihs'
        return super()._repr_item(key, default=default, value=value)

    def __repr__(self):
        extra = f"\nihs: {len(self.ihs)} streams of which the first is:\n    "
        return super().__repr__().replace('\nih: ', extra)


class CombineStreams(Task, CombineStreamsBase):
    """Combining streams using a callable (reference combining.py:140-172).

    Parameters
    ----------
    ihs : tuple of task or stream readers
        Input data streams.
    task : callable
        The function or method-like callable, taking a list of arrays.  It
        must work with any number of samples and only rearrange elements
        (``np.stack``, ``np.concatenate``, indexing, ...).  It is called on
        integer label arrays when the stream is made, not on the data, and on
        the ``frequency``, ``sideband`` and ``polarization`` of the streams.
    method : bool, optional
        Whether ``task`` is a method (two arguments) or a function (one
        argument).  Default: inferred by inspection.
    atol, samples_per_frame : as for `CombineStreamsBase`.
    """
    # Override init just to change name of ih to ihs.
    def __init__(self, ihs, task, method=None, *, atol=None, samples_per_frame=None):
        super().__init__(ihs, task, method=method, atol=atol, samples_per_frame=samples_per_frame)


class Concatenate(CombineStreamsBase):
    """Concatenate streams along an existing axis (reference combining.py:175-210).

    Parameters
    ----------
    ihs : tuple of task or stream readers
        Input data streams.
    axis : int
        Axis along which to combine the samples.  Should be a sample axis and
        thus cannot be 0.
    atol, samples_per_frame : as for `CombineStreamsBase`.
    """

    def __init__(self, ihs, axis=1, *, atol=None, samples_per_frame=None):
        self.axis = axis
        super().__init__(ihs, atol=atol, samples_per_frame=samples_per_frame)

    def task(self, data):
        """Concatenate the pieces of data together."""
        return np.concatenate(data, axis=self.axis)


class Stack(CombineStreamsBase):
    """Stack streams along a new axis (reference combining.py:213-248).

    Parameters
    ----------
    ihs : tuple of task or stream readers
        Input data streams.
    axis : int
        New axis along which to stack the samples.  Should be a sample axis
        and thus cannot be 0.
    atol, samples_per_frame : as for `CombineStreamsBase`.
    """

    def __init__(self, ihs, axis=1, *, atol=None, samples_per_frame=None):
        self.axis = axis
        super().__init__(ihs, atol=atol, samples_per_frame=samples_per_frame)

    def task(self, data):
        """Stack the pieces of data."""
        return np.stack(data, axis=self.axis)
