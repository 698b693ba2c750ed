"""Real-sampled streams to complex baseband on the GPU (reference
baseband_tasks/conversion.py:10-101).

Per frame of ``N = 2 M`` real samples the reference takes the analytic signal
(fft, one-sided spectrum, ifft), shifts it down by a quarter of the sample rate
(``exp(-i pi n / 2)``) and keeps every second sample.  With ``x_e[m] = x[2m]``
and ``x_o[m] = x[2m + 1]`` that is exactly

    out[m] = (-1)^m (x_e[m] + i (g (*) x_o)[m]),   fft(g) = G,
    G[0] = 0,  G[j] = -1j exp(-1j pi j / M)  (0 < j < M),

a circular convolution of length ``M`` with a real ``g`` (``G`` is Hermitian):
the real part is the input sample itself, and two real streams share one
complex transform of ``M`` points where the reference transforms ``2 M`` points
per stream (libbbt_hip: bbt_r2c_*, include/bbt_hip.h).
"""
import operator

import numpy as np

from . import hip
from .base import TaskBase, _stream_rate
from .device_task import DeviceTaskMixin, fetch_device
from .fourier import MAX_WG_FFT_LEN, is_fast_len

__all__ = ['Real2Complex', 'check_r2c_length', 'r2c_response']


def _prod(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def _splits(n):
    """n = n1 * n2 with both factors <= MAX_WG_FFT_LEN (the two-level overlap-save plans)?"""
    d = 1
    while d * d <= n:
        if n % d == 0 and n // d <= MAX_WG_FFT_LEN:
            return True
        d += 1
    return False


def check_r2c_length(n):
    """Output frame lengths the kernels take: any 2^a 3^b 5^c 7^d from 2 to 8192, and 16384, in one
    pass, and the longer ones of the overlap-save plans (two factors of at most 8192; powers of two up to
    2^24 among them)."""
    if n < 2 or not is_fast_len(n) or not (n <= MAX_WG_FFT_LEN or _splits(n)):
        raise ValueError(f"the hip engine handles Real2Complex output frames of n = 2^a 3^b 5^c 7^d "
                         f"samples with 2 <= n <= {MAX_WG_FFT_LEN}, or that split into two such "
                         f"factors; got {n}.")


def r2c_response(n):
    """G of the identity above for output frames of ``n`` samples: FFT-natural order, unscaled,
    complex128."""
    j = np.arange(n)
    g = -1j * np.exp(-1j * np.pi * j / n)
    g[0] = 0
    return g


class Real2Complex(DeviceTaskMixin, TaskBase):
    """Convert a real baseband signal to complex baseband at half the sample rate
    (reference conversion.py:10-101).

    Every input frame of ``2 * samples_per_frame`` samples is transformed on its
    own, circularly, as the reference does: the analytic signal (negative
    frequencies dropped), shifted by ``-sample_rate / 4`` and decimated by two.
    Trailing input that does not fill a frame is dropped.

    Parameters
    ----------
    ih : task or stream reader
        Real (float32) input stream, time as the first axis.  Unlike the
        reference, which broadcasts its filter against the last axis and so
        works on one-dimensional streams only, any sample shape is transformed
        along the time axis, stream by stream.
    samples_per_frame : int, optional
        Complete output samples per frame, ``M``.  Default: half the input's
        ``samples_per_frame`` (which must then be even).  Any 2^a 3^b 5^c 7^d
        up to 8192, and 16384, runs in one pass; longer lengths that split into two such
        factors (powers of two up to 2^24 among them) run in three steps.

    Raises
    ------
    ValueError
        If ``ih`` has complex data, or for frame lengths the kernels do not take.
    TypeError
        For float64 input (wrap the stream in `SinglePrecision`).
    """
    #: Take the three-step (multi-level) route for every length, also where one pass would do.
    MULTI_LEVEL = False
    _plan = None

    def __init__(self, ih, samples_per_frame=None):
        if ih.complex_data:
            raise ValueError("Stream should be real.")
        if np.dtype(ih.dtype) != np.dtype(np.float32):
            raise TypeError("the accelerated Real2Complex handles float32 streams; "
                            f"got {ih.dtype} (wrap the stream in SinglePrecision(...)).")
        if samples_per_frame is None:
            if ih.samples_per_frame % 2:
                raise ValueError("need even number of input samples")
            samples_per_frame = ih.samples_per_frame // 2
        samples_per_frame = operator.index(samples_per_frame)
        check_r2c_length(samples_per_frame)
        rate = _stream_rate(ih)
        frequency = getattr(ih, 'frequency', None)
        sideband = getattr(ih, 'sideband', None)
        if frequency is not None:
            frequency = frequency + rate / 2 * sideband
        self._n_stream = _prod(ih.shape[1:])
        super().__init__(ih, samples_per_frame=samples_per_frame, sample_rate=rate / 2,
                         frequency=frequency, sideband=sideband, dtype=np.complex64)

    def _get_plan(self):
        if self._plan is None:
            self._plan = hip.R2CPlan(self.samples_per_frame, self._n_stream, multi_level=self.MULTI_LEVEL)
        return self._plan

    @property
    def one_pass(self):
        """Does this task run on the one-pass kernels?"""
        return self._get_plan().info()['one_pass']

    def _input_span(self, first, last):
        n = self._ih_samples_per_frame
        return self.ih, first * n, (last - first) * n

    def _compute_frames(self, first, last, out):
        n_frames = last - first
        x = fetch_device(self.ih, first * self._ih_samples_per_frame, n_frames * self._ih_samples_per_frame)
        self._get_plan().execute(x, out, n_frames)

    def task(self, data):
        """Convert one frame (or several whole frames) given on the host (reference
        conversion.py:77-96)."""
        data = np.ascontiguousarray(data, dtype=np.float32)
        n = self._ih_samples_per_frame
        if data.shape[0] % n or data.shape[1:] != tuple(self.ih.shape[1:]):
            raise ValueError(f"need whole frames of {n} samples of shape {tuple(self.ih.shape[1:])}; "
                             f"got {data.shape}.")
        n_frames = data.shape[0] // n
        x = hip.DeviceArray.from_host(data.reshape(n_frames * n, self._n_stream))
        y = hip.DeviceArray((n_frames * self.samples_per_frame, self._n_stream), np.complex64)
        self._get_plan().execute(x, y, n_frames)
        return y.to_host().reshape((n_frames * self.samples_per_frame,) + tuple(self.sample_shape))

    def _repr_item(self, key, default, value=None):
        if key not in ('ih', 'samples_per_frame'):
            return None          # (the metadata follow from the input: not arguments here)
        if key == 'samples_per_frame' and default is None:
            default = self.ih.samples_per_frame // 2
        return super()._repr_item(key, default=default, value=value)

    def close(self):
        super().close()
        self._drop_cache()
        if self._plan is not None:
            self._plan.close()
            self._plan = None
