"""Sample-shape tasks on the GPU (reference baseband_tasks/shaping.py).

None of these tasks computes: every element of an output sample is a copy of
one element of the input sample at the same time offset.  So where the
reference applies ``task`` to every frame, here ``task`` is applied once, when
the task is built, to an array of *labels* (``arange`` over the input sample),
and what comes back is the index map that one gather plan (libbbt_hip:
bbt_gather_*, csrc/gather_kernels.hpp) then executes on the samples in HBM.
`index_map` is shared with `~baseband_tasks_amd.combining`.

Differences from the reference: the callable of `ChangeSampleShape` must be a
rearrangement (indexing, reshaping, transposing, ...: anything that only moves
elements; one that computes is refused with `TypeError`), and it is called on
label arrays at construction rather than on data at every frame.
"""
import numpy as np

from . import hip
from .base import Task, TaskBase, check_broadcast_to, simplify_shape, _stream_rate, _stream_start
from .device_task import DeviceTaskMixin, fetch_device, produces_on_device

__all__ = ['ChangeSampleShapeBase', 'ChangeSampleShape', 'Reshape', 'Transpose',
           'ReshapeAndTranspose', 'GetItem', 'GetSlice', 'index_map', 'map_runs']


def _prod(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def index_map(task, sample_shapes, combine=False):
    """The index map of a rearranging ``task``: ``(out_sample_shape, map_src, map_elem)``.

    ``task`` is called twice on label arrays of shape ``(1,) + sample_shape`` (a list of them, one
    per stream, if ``combine``): once with labels ``i`` and once with ``2 i + 1``, where ``i``
    counts the elements of all input samples.  A rearrangement returns an integer array of valid
    labels both times, and the two results agree element for element; anything else computes
    and is refused with `TypeError`.  (Labels are not negative, so a function that only differs
    from a rearrangement on negative numbers, such as ``abs``, passes as one.)  A result whose first axis is not 1 changed the time axis:
    `ValueError`.
    """
    sizes = [_prod(s) for s in sample_shapes]
    bases = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(bases[-1])

    def probe(scale, shift):
        labels = [((np.arange(n, dtype=np.int64) + b) * scale + shift).reshape((1,) + tuple(s))
                  for n, b, s in zip(sizes, bases[:-1], sample_shapes)]
        return task(labels if combine else labels[0])

    first, second = probe(1, 0), probe(2, 1)
    what = "the callable does not only rearrange the elements of the samples (it {}); the " \
           "accelerated shaping and combining tasks copy elements, they do not compute"
    for r in (first, second):
        if not isinstance(r, np.ndarray) or r.dtype.kind not in 'iu':
            raise TypeError(what.format("returns " + (f"dtype {r.dtype}" if isinstance(r, np.ndarray)
                                                     else type(r).__name__) + " for integer input"))
    if first.shape != second.shape:
        raise TypeError(what.format("returns shapes that depend on the values"))
    if first.ndim < 1 or first.shape[0] != 1:
        raise ValueError("shape change affected the sample axis (0).")
    out_shape = first.shape[1:]
    first = first.astype(np.int64).ravel()
    second = second.astype(np.int64).ravel()
    if first.size and (first.min() < 0 or first.max() >= total):
        raise TypeError(what.format("produces values that are not among its input"))
    if not np.array_equal(second, 2 * first + 1):
        raise TypeError(what.format("produces values that depend on the input values"))
    src = (np.searchsorted(bases, first, side='right') - 1).astype(np.int32)
    return out_shape, src, first - bases[src]


def map_runs(map_src, map_elem):
    """Run compression of an index map, as the library does it: ``(out_start, src, elem, length)``
    for every maximal stretch where the source stays and the element advances by one."""
    map_src = np.asarray(map_src).ravel()
    map_elem = np.asarray(map_elem).ravel()
    if map_src.size == 0:
        return []
    brk = np.flatnonzero((np.diff(map_src) != 0) | (np.diff(map_elem) != 1)) + 1
    starts = np.concatenate([[0], brk])
    stops = np.concatenate([brk, [map_src.size]])
    return [(int(a), int(map_src[a]), int(map_elem[a]), int(b - a)) for a, b in zip(starts, stops)]


class ChangeSampleShapeBase(DeviceTaskMixin, TaskBase):
    """Base class for sample shape operations (reference shaping.py:12-58).

    A subclass defines ``task(data)``, which changes the shape of the samples
    but not the time axis.  ``task`` is applied to a label array when the
    stream is made (see the module docstring) and to the ``frequency``,
    ``sideband`` and ``polarization`` of the input, on the host; the samples
    are rearranged in HBM by one kernel launch per run of frames.

    Where the rearrangement keeps every element in place (a `Reshape`, a
    `GetItem` that keeps everything, an identity `Transpose`) no bytes move:
    ``read_device`` hands on the upstream device array under its new shape
    (same device pointer, no launch).  Like every ``read_device`` result that
    is a view, it lives until the next read of the task it came from; the
    combining tasks copy inputs that share a producer.

    Parameters
    ----------
    ih : task or stream reader
        Input data stream.
    **kwargs
        Possible further arguments; see `~baseband_tasks_amd.base.TaskBase`.
    """
    _plan = None
    _start = 0          # (GetSlice: first input sample)
    #: Route of the gather plan: 'auto', or 'run_copy', 'tile', 'direct' to force one (tests).
    ROUTE = 'auto'

    def __init__(self, ih, **kwargs):
        # Check operation is possible (as the reference does, on a fake array)
        a = np.empty((7,) + tuple(ih.sample_shape), dtype='?')
        try:
            a = self.task(a)
        except Exception as exc:
            exc.args += ("stream samples with shape {} cannot be changed "
                         "as required".format(tuple(ih.sample_shape)),)
            raise
        if a.shape[0] != 7:
            raise ValueError("shape change affected the sample axis (0).")
        out_shape, self._map_src, self._map_elem = index_map(self.task, [tuple(ih.sample_shape)])
        assert tuple(out_shape) == tuple(a.shape[1:])
        n_in = _prod(ih.sample_shape)
        self._identity = (self._map_elem.size == n_in
                          and np.array_equal(self._map_elem, np.arange(n_in)))
        super().__init__(ih, shape=tuple(ih.shape[:1]) + tuple(a.shape[1:]), **kwargs)

    def _check_shape(self, value):
        """Broadcast value to the input sample shape and apply the shape change; axes in which
        all values are identical are then removed (reference shaping.py:44-58)."""
        broadcast = check_broadcast_to(value, (1,) + tuple(self.ih.sample_shape))
        value = self.task(broadcast)[0, ...]
        return simplify_shape(value)

    @property
    def index_map(self):
        """Input element (flat index in the input sample) of every output element."""
        return self._map_elem.reshape(self.sample_shape)

    def _get_plan(self):
        if self._plan is None:
            self._plan = hip.GatherPlan([_prod(self.ih.sample_shape)], self._map_src, self._map_elem,
                                        np.dtype(self.dtype).itemsize, route=self.ROUTE)
        return self._plan

    @property
    def route(self):
        """Route of the gather plan ('run_copy', 'tile' or 'direct'); None for a pure view."""
        return None if self._identity else self._get_plan().info()['route']

    def _input_span(self, first, last):
        start, stop = self._frame_span(first, last)
        return self.ih, self._start + start, stop - start

    def _compute_frames(self, first, last, out):
        start, stop = self._frame_span(first, last)
        x = fetch_device(self.ih, self._start + start, stop - start)
        if self._identity:
            out.copy_from_device(x)
        else:
            self._get_plan().execute([x], out, stop - start)

    @property
    def _view_source(self):
        return self.ih if self._identity and produces_on_device(self.ih) else None

    def read_device(self, count=None):
        """As `DeviceTaskMixin.read_device`; where no element moves, the upstream device array
        under the new shape, which lives until the next read of the task it came from."""
        if not (self._identity and produces_on_device(self.ih)):
            return super().read_device(count)
        count = self._prepare_read(count, None)
        self.ih.seek(self._start + self.offset)
        x = self.ih.read_device(count)
        self.offset += count
        return x.reshape((count,) + tuple(self.sample_shape))

    def read(self, count=None, out=None):
        if not self._identity or out is not None:
            return super().read(count, out)
        count = self._prepare_read(count, None)
        self.ih.seek(self._start + self.offset)
        x = self.ih.read(count)
        self.offset += count
        return x.reshape((count,) + tuple(self.sample_shape))

    def close(self):
        super().close()
        self._drop_cache()
        if self._plan is not None:
            self._plan.close()
            self._plan = None


class ChangeSampleShape(Task, ChangeSampleShapeBase):
    """Change sample shape using a callable (reference shaping.py:61-110).

    Parameters
    ----------
    ih : task or stream reader
        Input data stream.
    task : callable
        The function or method-like callable.  It must work with any number of
        samples and only rearrange the elements of the samples (index, reshape,
        transpose, ``swapaxes``, ``moveaxis``, ...).  It is called on integer
        label arrays when the stream is made, not on the data, and on the
        ``frequency``, ``sideband`` and ``polarization`` of the input stream.
    method : bool, optional
        Whether ``task`` is a method (two arguments) or a function (one
        argument).  Default: inferred by inspection.

    Raises
    ------
    TypeError
        If ``task`` computes rather than rearranges.
    ValueError
        If ``task`` changes the time axis.
    """


class Reshape(ChangeSampleShapeBase):
    """Reshapes the sample shape of a stream (reference shaping.py:113-167).  No bytes move:
    ``read_device`` is the upstream array under the new shape.

    Parameters
    ----------
    ih : task or stream reader
        Input data stream.
    sample_shape : tuple of int
        Output sample shape.
    """

    def __init__(self, ih, sample_shape):
        self._new_shape = (-1,) + tuple(sample_shape)
        super().__init__(ih)

    def task(self, data):
        """Reshape the data."""
        return data.reshape(self._new_shape)

    def _repr_item(self, key, default, value=None):
        if key == 'sample_shape':
            value = self._new_shape[1:]
        return super()._repr_item(key, default=default, value=value)


class Transpose(ChangeSampleShapeBase):
    """Reshapes the axes of the samples of a stream (reference shaping.py:170-224).

    Parameters
    ----------
    ih : task or stream reader
        Input data stream.
    sample_axes : tuple of int
        Where the input sample shape axes should end up in the output sample
        shape (as for `~numpy.transpose`).  Should contain all axes of the
        sample shape, starting at ``1`` (time axis 0 always stays in place).
    """

    def __init__(self, ih, sample_axes):
        self._sample_axes = tuple(sample_axes)
        self._axes = (0,) + tuple(sample_axes)
        super().__init__(ih)

    def task(self, data):
        """Transpose the axes of data."""
        return data.transpose(self._axes)


class ReshapeAndTranspose(Reshape):
    """Reshapes the sample shape of a stream and transposes its axes, in one pass (reference
    shaping.py:227-293).

    Parameters
    ----------
    ih : task or stream reader
        Input data stream.
    sample_shape : tuple of int
        Output sample shape (before the transpose).
    sample_axes : tuple of int
        As for `Transpose`.
    """

    def __init__(self, ih, sample_shape, sample_axes):
        self._sample_shape = tuple(sample_shape)
        self._sample_axes = tuple(sample_axes)
        self._axes = (0,) + tuple(sample_axes)
        super().__init__(ih, sample_shape=sample_shape)

    def task(self, data):
        """Reshape and transpose the axes of data."""
        return data.reshape(self._new_shape).transpose(self._axes)

    def _repr_item(self, key, default, value=None):
        if key == 'sample_shape':
            value = self._sample_shape
        return super()._repr_item(key, default=default, value=value)


class GetItem(ChangeSampleShapeBase):
    """Index or slice the samples of a stream (reference shaping.py:296-347).

    Parameters
    ----------
    ih : task or stream reader
        Input data stream.
    item : int, slice, list of int, or array of int, or a tuple of these
        Anything that can index a numpy array.  Should only attempt to index
        the samples, not the time axis.  An item that keeps everything moves
        no bytes (see `ChangeSampleShapeBase`).
    """

    def __init__(self, ih, item):
        if isinstance(item, tuple):
            self._task_item = (slice(None),) + item
        else:
            self._task_item = (slice(None), item)
        super().__init__(ih)
        self._item = item

    def task(self, data):
        """Get the preset item from the data."""
        return data[self._task_item]


class GetSlice(ChangeSampleShapeBase):
    """Slice a stream and index or slice its samples (reference shaping.py:350-423).

    Parameters
    ----------
    ih : task or stream reader
        Input data stream.
    item : slice or tuple of slice, int, or array of int
        Anything that can index a numpy array.  Should be a slice for the
        time axis, with step 1 and a length that is not zero.

    Raises
    ------
    AssertionError
        For a time item that is not a slice, has a step, or is empty (as the
        reference, which asserts).
    """

    def __init__(self, ih, item):
        self._item = item
        if isinstance(item, tuple):
            if any(not (isinstance(i, slice) and i == slice(None)) for i in item[1:]):
                # Override task to also take sample items.
                self._task_item = (slice(None),) + item[1:]
                self.task = lambda data: data[self._task_item]
            item = item[0]
        assert isinstance(item, slice), "only support slice for time axis"
        start, stop, step = item.indices(ih.shape[0])
        assert step == 1, "do not support step for time slice"
        assert stop > start, "empty time slice"
        super().__init__(ih)
        self._start = start
        self._shape = (stop - start,) + tuple(self.shape[1:])
        # (streams whose samples are not evenly spaced in time tell the time of every offset themselves)
        self._time_from_ih = hasattr(ih, '_tell_time')
        if not self._time_from_ih:
            self._start_time = _stream_start(ih) + start / _stream_rate(ih)

    def _tell_time(self, offset):
        if self._time_from_ih:
            return self.ih._tell_time(self._start + offset)
        return super()._tell_time(offset)

    def task(self, data):
        """No-op task for the default case of no sample slicing (overridden in the initializer
        if the samples are indexed too)."""
        return data
