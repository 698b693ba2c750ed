"""Synthetic sources (reference baseband_tasks/generators.py) plus
`DeviceStream`, a source whose samples already live in HBM."""
import numpy as np

from .base import Base
from . import hip
from .hip import DeviceArray, as_device_array

__all__ = ['StreamGenerator', 'EmptyStreamGenerator', 'Noise', 'NoiseGenerator', 'HostStream',
           'DeviceStream', 'DeviceNoiseGenerator']


class StreamGenerator(Base):
    """Frames produced by ``function(stream)``; the stream pointer is at the
    start of the frame when the function is called and it must return
    ``samples_per_frame`` samples (reference generators.py:16-90)."""

    def __init__(self, function, shape, start_time, sample_rate, samples_per_frame=1,
                 dtype=np.complex64, **kwargs):
        super().__init__(shape=shape, start_time=start_time, sample_rate=sample_rate,
                         samples_per_frame=samples_per_frame, dtype=dtype, **kwargs)
        self._function = function

    def _read_frame(self, frame_index):
        return self._function(self)


class EmptyStreamGenerator(Base):
    """Uninitialised frames, to be filled by a `Task` (reference generators.py:93-151)."""

    def _read_frame(self, frame_index):
        return np.empty((self.samples_per_frame,) + self.sample_shape, self.dtype)


class Noise:
    """Reproducible Gaussian noise frames: the Philox counter is re-seeded per
    frame with the frame's sample offset (reference generators.py:154-190), so
    any frame can be regenerated bit-for-bit in any order."""

    def __init__(self, seed=None):
        self.seed = seed
        self._bit_generator = np.random.Philox(seed)
        self._rng = np.random.Generator(self._bit_generator)
        self._state0 = self._bit_generator.state

    def __call__(self, sh):
        state = self._state0
        state['state']['counter'][1] = sh.tell()
        self._bit_generator.state = state
        shape = (sh.samples_per_frame,) + tuple(sh.sample_shape)
        if sh.complex_data:
            shape = shape[:-1] + (shape[-1] * 2,)
        numbers = self._rng.normal(size=shape)
        if sh.complex_data:
            numbers = numbers.view(np.complex128)
        return numbers.astype(sh.dtype, copy=False)


class NoiseGenerator(StreamGenerator):
    """Stream of unit-variance (per component) normal noise; choose
    ``samples_per_frame`` large (reference generators.py:193-245)."""

    def __init__(self, shape, start_time, sample_rate, samples_per_frame,
                 dtype=np.complex64, seed=None, **kwargs):
        super().__init__(function=Noise(seed), shape=shape, start_time=start_time,
                         sample_rate=sample_rate, samples_per_frame=samples_per_frame,
                         dtype=dtype, **kwargs)


class HostStream(Base):
    """A stream whose samples sit in a NumPy array (or memory map) on the host:
    the host-side counterpart of `DeviceStream`, for data that does not come
    from a file reader.  ``read(out=...)`` is one copy; a device task on top
    uploads straight from the array when its memory is page-locked (``pin``:
    lock it in place with hipHostRegister -- on by default for C-contiguous
    arrays; arrays from `host_pipeline.pinned_empty` are pinned already), run
    m + 1 going up while run m is transformed (host_pipeline.py)."""

    def __init__(self, data, start_time, sample_rate, samples_per_frame=None, *, pin=True, **kwargs):
        self._data = data if isinstance(data, np.ndarray) else np.asarray(data)
        if samples_per_frame is None:
            samples_per_frame = min(self._data.shape[0], 1 << 20)
        self._pinned = None
        self._pin = bool(pin)
        super().__init__(shape=self._data.shape, start_time=start_time, sample_rate=sample_rate,
                         samples_per_frame=samples_per_frame, dtype=self._data.dtype, **kwargs)

    def host_view(self, start, count):
        """The samples [start, start + count) as a view of the array if it is
        C-contiguous and page-locked, else None."""
        if self._pinned is None:
            from . import host_pipeline
            self._pinned = bool(self._data.flags.c_contiguous and
                                (host_pipeline.is_pinned(self._data) or
                                 (self._pin and host_pipeline.pin_array(self._data))))
        return self._data[start:start + count] if self._pinned else None

    def read(self, count=None, out=None):
        count = self._prepare_read(count, out)
        piece = self._data[self.offset:self.offset + count]
        self.offset += count
        if out is None:
            return piece.copy()
        out[...] = piece
        return out

    def _read_frame(self, frame_index):
        start = frame_index * self.samples_per_frame
        return self._data[start:min(start + self.samples_per_frame, self.shape[0])].copy()

    def close(self):
        super().close()
        self._data = None


class DeviceStream(Base):
    """A stream resident in HBM.

    ``data`` is a `hip.DeviceArray`, a torch tensor on the GPU, or a host
    array / stream of this package (which is uploaded once).  ``read_device``
    returns zero-copy views, so a task chain on top never touches the host.
    """
    _produces_on_device = True
    #: any range of the stream is there for the taking: a task that reads straight from it need
    #: not bound how much it asks for at once (`DeviceTaskMixin.read_device`)
    _resident = True

    def __init__(self, data, start_time, sample_rate, samples_per_frame=None, **kwargs):
        if isinstance(data, np.ndarray):
            data = DeviceArray.from_host(data)
        elif isinstance(data, Base):
            source = data
            old = source.tell()
            source.seek(0)
            dev = DeviceArray(source.shape, source.dtype)
            step = max(source.samples_per_frame, 1 << 20)
            on_device = bool(getattr(source, '_produces_on_device', False))
            for start in range(0, source.shape[0], step):
                n = min(step, source.shape[0] - start)
                if on_device:
                    dev[start:start + n].copy_from_device(source.read_device(n))   # (stays in HBM)
                else:
                    dev[start:start + n].copy_from_host(source.read(n))
            source.seek(old)
            if samples_per_frame is None:
                samples_per_frame = source.samples_per_frame
            for key in ('frequency', 'sideband', 'polarization'):
                if key not in kwargs and getattr(source, key, None) is not None:
                    kwargs[key] = getattr(source, key)
            data = dev
        self._data = as_device_array(data)
        if samples_per_frame is None:
            samples_per_frame = min(self._data.shape[0], 1 << 20)
        super().__init__(shape=self._data.shape, start_time=start_time,
                         sample_rate=sample_rate, samples_per_frame=samples_per_frame,
                         dtype=self._data.dtype, **kwargs)

    def read_device(self, count=None):
        count = self._prepare_read(count, None)
        view = self._data[self.offset:self.offset + count]
        self.offset += count
        return view

    def read(self, count=None, out=None):
        count = self._prepare_read(count, out)
        view = self._data[self.offset:self.offset + count]
        self.offset += count
        return view.to_host(out)

    def _read_frame(self, frame_index):
        start = frame_index * self.samples_per_frame
        return self._data[start:min(start + self.samples_per_frame, self.shape[0])].to_host()


class DeviceNoiseGenerator(Base):
    """`NoiseGenerator`, with the samples made on the GPU: the same arguments, and bit for bit
    the same stream (NumPy's Philox-4x64 counter generator re-seeded per frame, through NumPy's
    ziggurat normal sampler: csrc/noise_kernels.hpp), for float32 and complex64.

    A device source like `DeviceStream`: ``read_device`` returns a view of a cache of frames in
    HBM (consume it before reading again), ``read`` downloads.  Comparisons of the sampler that
    this device's and the host's math library might decide differently are detected on the device;
    the frame concerned is then made by NumPy and uploaded (``host_frames`` counts them; expect none
    in 10^12 samples)."""
    _produces_on_device = True
    #: a cache fill takes a new block of the pool, so a view handed out earlier stays what it was
    #: (`device_task.cache_producer`)
    _views_keep_their_block = True
    #: relative margin of the comparisons left to NumPy (`hip.philox_normal`)
    _guard = hip.NOISE_GUARD
    _max_frames_per_call = None

    def __init__(self, shape, start_time, sample_rate, samples_per_frame,
                 dtype=np.complex64, seed=None, **kwargs):
        if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.complex64)):
            raise TypeError(f"DeviceNoiseGenerator makes float32 or complex64 samples, not {np.dtype(dtype)}")
        super().__init__(shape=shape, start_time=start_time, sample_rate=sample_rate,
                         samples_per_frame=samples_per_frame, dtype=dtype, **kwargs)
        # the host twin: draws the entropy of seed=None (once), holds the key, makes flagged frames
        self._host = NoiseGenerator(shape, start_time, sample_rate, samples_per_frame,
                                    dtype=dtype, seed=seed, **kwargs)
        state0 = self._host._function._state0
        self.seed = seed
        self._key = np.array(state0['state']['key'], dtype=np.uint64)
        self._counter = np.array(state0['state']['counter'], dtype=np.uint64)
        self._per_sample = (2 if self.complex_data else 1) * int(np.prod(self.sample_shape, dtype=np.int64))
        #: frames that were made by NumPy on the host because the device flagged them
        self.host_frames = 0
        self._cache = None
        self._cache_start = self._cache_stop = 0

    @property
    def max_frames_per_call(self):
        """Upper bound on the frames generated into the cache by one call: as many as make 512 MiB,
        32 at least (as for the device tasks).  Assignable."""
        if self._max_frames_per_call is not None:
            return self._max_frames_per_call
        frame = max(int(self.samples_per_frame) * self._per_sample * 4, 1)
        return max(32, min((1 << 29) // frame, 1 << 18))

    @max_frames_per_call.setter
    def max_frames_per_call(self, value):
        self._max_frames_per_call = None if value is None else int(value)

    def _generate(self, start, stop, out):
        """Samples [start, stop) into DeviceArray ``out``; start is the start of a frame.  Whole
        frames go in one call; a last frame that is cut short is made only as far as needed."""
        spf, per = self.samples_per_frame, self._per_sample
        n_full = (stop - start) // spf
        runs = []                                   # (first sample, frames, samples per frame made)
        for f0 in range(0, n_full, 65535):
            runs.append((start + f0 * spf, min(65535, n_full - f0), spf))
        if start + n_full * spf < stop:
            runs.append((start + n_full * spf, 1, stop - start - n_full * spf))
        for s0, frames, length in runs:
            piece = out[s0 - start:s0 - start + frames * length]
            normals = DeviceArray((frames, length * per), np.float32, piece.ptr, piece)
            counters = np.tile(self._counter, (frames, 1))
            counters[:, 1] = s0 + spf * np.arange(frames, dtype=np.uint64)
            flags, _ = hip.philox_normal(normals, self._key, counters, guard=self._guard)
            for f in np.nonzero(flags)[0]:
                self._host.seek(s0 + int(f) * spf)
                piece[int(f) * length:(int(f) + 1) * length].copy_from_host(self._host.read(length))
                self.host_frames += 1

    def _fetch(self, count):
        """View of (or fresh array with) samples [offset, offset + count) in HBM; moves the pointer."""
        if count == 0:
            return DeviceArray((0,) + tuple(self.sample_shape), self.dtype)
        spf = self.samples_per_frame
        begin, end = self.offset, self.offset + count
        if not (self._cache is not None and self._cache_start <= begin and end <= self._cache_stop):
            start = begin // spf * spf
            if end - start > (self.max_frames_per_call + 2) * spf:
                # too much for the cache: a fresh array, filled run by run
                out = DeviceArray((count,) + tuple(self.sample_shape), self.dtype)
                if begin > start:
                    head = min(start + spf, end)
                    tmp = DeviceArray((head - start,) + tuple(self.sample_shape), self.dtype)
                    self._generate(start, head, tmp)
                    out[:head - begin].copy_from_device(tmp[begin - start:])
                    start = head
                step = self.max_frames_per_call * spf
                while start < end:
                    stop = min(start + step, end)
                    self._generate(start, stop, out[start - begin:stop - begin])
                    start = stop
                self.offset = end
                return out
            # (a new block of the pool every time: whoever still reads the last view keeps its block)
            self._cache = None
            base = DeviceArray((end - start,) + tuple(self.sample_shape), self.dtype)
            self._generate(start, end, base)
            self._cache, self._cache_start, self._cache_stop = base, start, end
        view = self._cache[begin - self._cache_start:end - self._cache_start]
        self.offset = end
        return view

    def read_device(self, count=None):
        return self._fetch(self._prepare_read(count, None))

    def read(self, count=None, out=None):
        return self._fetch(self._prepare_read(count, out)).to_host(out)

    def _read_frame(self, frame_index):
        start = frame_index * self.samples_per_frame
        stop = min(start + self.samples_per_frame, self.shape[0])
        dev = DeviceArray((stop - start,) + tuple(self.sample_shape), self.dtype)
        self._generate(start, stop, dev)
        return dev.to_host()

    def close(self):
        super().close()
        self._host.close()
        self._cache = None
