"""ctypes binding of libbbt_hip.so (C ABI: include/bbt_hip.h) and thin device
helpers.  There is deliberately NO fallback: if the library is missing or a
call fails, an exception is raised.
"""
import ctypes as C
import importlib.util
import os
import sys
import threading
import weakref

import numpy as np

__all__ = ['HipError', 'HipLibraryMissing', 'lib', 'available', 'DeviceArray',
           'OsmPlan', 'ChanPlan', 'PfbPlan', 'set_stream', 'get_stream',
           'synchronize', 'Event', 'device_count', 'set_device', 'pack', 'to_half', 'from_half',
           'psrfits_encode', 'psrfits_decode', 'psrsearch_encode', 'psrsearch_decode', 'philox_normal']

_HERE = os.path.dirname(os.path.abspath(__file__))
# BBT_HIP_LIB points at another build of the same library (the sanitizer build
# of tools/build_sanitize.sh); never at a different implementation.
LIB_PATH = os.environ.get('BBT_HIP_LIB') or os.path.join(_HERE, 'lib', 'libbbt_hip.so')


class HipError(RuntimeError):
    """A call into libbbt_hip.so failed."""


class HipLibraryMissing(ImportError):
    """libbbt_hip.so has not been built (run ``python __graft_entry__.py``)."""


_vp, _i64, _i32, _int, _sz = C.c_void_p, C.c_int64, C.c_int32, C.c_int, C.c_size_t
_pvp = C.POINTER(C.c_void_p)
_pi64, _pi32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)

# name -> argtypes ; every entry point declared in include/bbt_hip.h
SIGNATURES = {
    'bbt_version': [],
    'bbt_rtc_info': [C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)],
    'bbt_tune_scratch': [C.c_int, C.POINTER(C.c_int64)],
    'bbt_device_count': [C.POINTER(_int)],
    'bbt_set_device': [_int],
    'bbt_get_device': [C.POINTER(_int)],
    'bbt_device_name': [C.c_char_p, _int],
    'bbt_malloc': [_pvp, _sz],
    'bbt_free': [_vp],
    'bbt_pool_set_stream': [_vp],
    'bbt_pool_trim': [],
    'bbt_pool_info': [C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    'bbt_host_alloc': [_pvp, _sz],
    'bbt_host_free': [_vp],
    'bbt_memset': [_vp, _int, _sz, _vp],
    'bbt_memcpy_h2d': [_vp, _vp, _sz, _vp],
    'bbt_memcpy_d2h': [_vp, _vp, _sz, _vp],
    'bbt_memcpy_d2d': [_vp, _vp, _sz, _vp],
    'bbt_memcpy2d': [_vp, _sz, _vp, _sz, _sz, _sz, _int, _vp],
    'bbt_pad_streams': [_vp, _vp, _i64, _int, _int, _int, _vp],
    'bbt_detect_power_axis': [_vp, _vp, _i64, _i64, _int, _int, _int, _vp],
    'bbt_stream_create': [_pvp],
    'bbt_stream_destroy': [_vp],
    'bbt_stream_sync': [_vp],
    'bbt_device_sync': [],
    'bbt_event_create': [_pvp],
    'bbt_event_create_ordering': [_pvp],
    'bbt_event_destroy': [_vp],
    'bbt_event_record': [_vp, _vp],
    'bbt_event_sync': [_vp],
    'bbt_event_query': [_vp, C.POINTER(C.c_int)],
    'bbt_stream_wait_event': [_vp, _vp],
    'bbt_host_register': [_vp, _sz],
    'bbt_host_unregister': [_vp],
    'bbt_event_elapsed_ms': [_vp, _vp, C.POINTER(C.c_float)],
    'bbt_osm_plan_create': [_pvp, _i64, _int, _int, _vp, _int, _pi32],
    'bbt_osm_plan_destroy': [_vp],
    'bbt_osm_plan_info': [_vp, _pi64, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int)],
    'bbt_osm_plan_fusable': [_vp, _int],
    'bbt_osm_plan_defer': [_vp, _vp],
    'bbt_osm_execute': [_vp, _vp, _vp, _i64, _pi64, _pi64, _pi32, _pi32, _vp],
    'bbt_osm_execute_flat': [_vp, _vp, _vp, _i64, _pi64, _pi64, _pi32, _i32, _pi32, _vp],
    'bbt_osm_plan_set_layout': [_vp, _i64, _i64],
    'bbt_osm_execute_channelized': [_vp, _vp, _vp, _i64, _pi64, _pi64, _pi32, _pi32, _int, _i64,
                                    _i64, _vp],
    'bbt_osm_execute_channelized_detect': [_vp, _vp, _vp, _i64, _pi64, _pi64, _pi32, _pi32, _int,
                                           _i64, _i64, _int, _int, _int, _vp],
    'bbt_osm_detect_bins_max': [_vp, _int, _int],
    'bbt_osm_execute_regular': [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp],
    'bbt_osm_timing_enable': [_vp, _int],
    'bbt_osm_timing_read': [_vp, C.POINTER(C.c_double), _pi64],
    'bbt_osm_timing_read_passes': [_vp, C.POINTER(C.c_double), _pi64, _pi64],
    'bbt_chan_plan_create': [_pvp, _int, _int, _int],
    'bbt_chan_plan_destroy': [_vp],
    'bbt_chan_execute': [_vp, _vp, _vp, _i64, _vp],
    'bbt_pfb_plan_create': [_pvp, _int, _int, _int, C.POINTER(C.c_float)],
    'bbt_pfb_plan_destroy': [_vp],
    'bbt_pfb_execute': [_vp, _vp, _vp, _i64, _vp],
    'bbt_detect_integrate': [_vp, _vp, _i64, _i64, _i64, _int, _int, _vp],
    'bbt_fold_runs': [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _i64, _vp, _int, _vp, _i64, _vp],
    'bbt_phase_runs_work': [_i64, _i64, _i64, _pi64],
    'bbt_phase_runs': [_vp, _i64, _int, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp,
                       _vp, _i64, _pi64, _vp],
    'bbt_modulate_runs': [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _vp],
    'bbt_modulate_pieces': [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _int, _vp],
    'bbt_sk_estimate': [_vp, _vp, _i64, _i64, _i64, _int, C.c_double, _vp],
    'bbt_sk_excise': [_vp, _vp, _i64, _i64, _i64, _int, C.c_double, C.c_float, C.c_float, _i64, _vp, _vp, _vp],
    'bbt_philox_normal_work': [_i64, _i64, _pi64],
    'bbt_philox_normal': [_vp, _vp, _i64, _i64, _i64, C.c_double, _vp, _i64, _vp, _i64, _pi64, _pi64, _vp],
    'bbt_shift_plan_create': [_pvp, _int, _int, _pi32],
    'bbt_shift_plan_destroy': [_vp],
    'bbt_shift_execute': [_vp, _vp, _vp, _i64, _vp],
    'bbt_dmt_plan_create': [_pvp, _pi32, _i64, _i64, _i64],
    'bbt_dmt_plan_destroy': [_vp],
    'bbt_dmt_plan_info': [_vp, _pi64, C.POINTER(_int), C.POINTER(_int), _pi64],
    'bbt_dmt_execute': [_vp, _vp, _i64, _vp, _i64, _vp],
    'bbt_sps_standardize': [_vp, _vp, _i64, _i64, _i64, _vp],
    'bbt_sps_plan_create': [_pvp, _i64, _i64, _i64],
    'bbt_sps_plan_destroy': [_vp],
    'bbt_sps_plan_info': [_vp, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), _pi64,
                          C.POINTER(C.c_float)],
    'bbt_sps_execute': [_vp, _vp, _i64, _vp, _i64, _vp],
    'bbt_ffa_plan_create': [_pvp, _i64, _i64, _i64, _i64, _i64],
    'bbt_ffa_plan_destroy': [_vp],
    'bbt_ffa_plan_info': [_vp, _i64, C.POINTER(_int), C.POINTER(_int), _pi64, _pi64, _pi64, _pi64, C.POINTER(C.c_float)],
    'bbt_ffa_execute': [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp],
    'bbt_hsum_whiten': [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp],
    'bbt_hsum_plan_create': [_pvp, _i64, _i64, _i64, _i64, _i64, C.POINTER(C.c_float)],
    'bbt_hsum_plan_destroy': [_vp],
    'bbt_hsum_plan_info': [_vp, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), C.POINTER(C.c_float)],
    'bbt_hsum_execute': [_vp, _vp, _i64, _vp, _vp],
    'bbt_lspec_plan_create': [_pvp, _i64, _i64, _i64],
    'bbt_lspec_plan_destroy': [_vp],
    'bbt_lspec_plan_info': [_vp, _i64, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), C.POINTER(_int),
                            C.POINTER(_int), _pi64, _pi64],
    'bbt_lspec_execute': [_vp, _vp, _i64, _vp, _i64, _i64, _vp],
    'bbt_accel_plan_create': [_pvp, _i64, _i64, C.POINTER(C.c_double), _i64],
    'bbt_accel_plan_destroy': [_vp],
    'bbt_accel_plan_info': [_vp, _i64, _i64, C.POINTER(_int), C.POINTER(_int), _pi64, _pi64, _pi64, C.POINTER(_int)],
    'bbt_accel_execute': [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp],
    'bbt_rank_stats': [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp],
    'bbt_rank_standardize': [_vp, _vp, _i64, _i64, _i64, _vp],
    'bbt_rank_whiten': [_vp, _vp, _i64, _i64, _i64, _i64, _i64, C.c_double, _vp],
    'bbt_rank_info': [_i64, _i64, _i64, _i64, _i64, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), _pi64, _pi64],
    'bbt_rmed_plan_create': [_pvp, _i64, _i64, _i64],
    'bbt_rmed_plan_destroy': [_vp],
    'bbt_rmed_info': [_i64, _i64, _i64, _i64, _i64, _i64, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), _pi64, _pi64,
                      _pi64, _pi64],
    'bbt_rmed_execute': [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _int, _vp],
    'bbt_corr_plan_create': [_pvp, _i64, _i64, _i64, _i64, _int],
    'bbt_corr_plan_destroy': [_vp],
    'bbt_corr_info': [_i64, _i64, _i64, _i64, _i64, C.POINTER(_int), C.POINTER(_int), C.POINTER(_int), _pi64, _pi64, _pi64],
    'bbt_corr_execute': [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp],
    'bbt_fir_plan_create': [_pvp, _int, _int, _vp],
    'bbt_fir_plan_destroy': [_vp],
    'bbt_fir_execute': [_vp, _vp, _vp, _i64, _vp],
    'bbt_r2c_plan_create': [_pvp, _i64, _int],
    'bbt_r2c_plan_create_ex': [_pvp, _i64, _int, _int],
    'bbt_r2c_plan_destroy': [_vp],
    'bbt_r2c_plan_info': [_vp, C.POINTER(_int), _pi64],
    'bbt_r2c_execute': [_vp, _vp, _vp, _i64, _vp],
    'bbt_gather_plan_create': [_pvp, _int, _pi64, _i64, C.POINTER(C.c_int32), _pi64, _int],
    'bbt_gather_plan_create_ex': [_pvp, _int, _pi64, _i64, C.POINTER(C.c_int32), _pi64, _int, _int],
    'bbt_gather_plan_destroy': [_vp],
    'bbt_gather_plan_info': [_vp, C.POINTER(_int), _pi64, C.POINTER(_int), C.POINTER(_int)],
    'bbt_gather_execute': [_vp, C.POINTER(_vp), _pi64, _vp, _i64, _vp],
    'bbt_real_op': [_vp, _vp, _int, _i64, _int, _int, _vp],
    'bbt_chirp': [_vp, _i64, _int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                  C.c_double, C.c_double, C.c_double, _vp],
    'bbt_scale_streams': [_vp, _vp, _i64, _int, _vp, _vp],
    'bbt_unpack': [_vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _int, _vp],
    'bbt_unpack_masked': [_vp, _vp, _i64, _int, _int, _int, _int, _int, _int, _int, _vp, _vp],
    'bbt_pack': [_vp, _vp, _i64, _int, _int, _vp],
    'bbt_to_half': [_vp, _vp, _i64, _vp],
    'bbt_from_half': [_vp, _vp, _i64, _vp],
    'bbt_psrfits_encode': [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp],
    'bbt_psrfits_decode': [_vp, _vp, _vp, _vp, C.c_float, _vp, _i64, _i64, _i64, _i64, _vp],
    'bbt_psrsearch_encode': [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _int, C.c_double, _vp],
    'bbt_psrsearch_decode': [_vp, _vp, _vp, _vp, C.c_float, _vp, _i64, _i64, _i64, _i64, _int, _vp],
    'bbt_comm_unique_id': [_vp, _sz],
    'bbt_comm_init': [_pvp, _int, _int, _vp, _sz],
    'bbt_comm_destroy': [_vp],
    'bbt_bcast_chirp': [_vp, _vp, _i64, _int, _vp],
    'bbt_gather_output': [_vp, _vp, _vp, _i64, _vp],
}

#: oldest libbbt_hip.so whose entry points and argument meanings this binding assumes
MIN_LIB_VERSION = 171

_lib = None
_lock = threading.Lock()


_torch_lib_dir = None      # set when PyTorch's bundled ROCm runtime was preloaded


def _preload_torch_runtime(name='libamdhip64.so'):
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own
    libamdhip64 / libhsa-runtime64 / librccl; libbbt_hip.so is linked against
    the system's.  If this library is loaded first it pulls in the system
    runtime, and a later ``import torch`` brings a second one that finds no GPU
    ("No HIP GPUs are available", measured on the MI355X box).  So when torch is
    installed but not imported yet, its copy is loaded first, globally: this
    library and torch then share it whatever the import order (the same sonames;
    it is what `bench.py`, which imports torch first, runs on anyway).
    BBT_HIP_RUNTIME=system skips this."""
    global _torch_lib_dir
    if os.environ.get('BBT_HIP_RUNTIME', '') == 'system':
        return
    if _torch_lib_dir is None:
        if 'torch' in sys.modules and name == 'libamdhip64.so':
            return                       # already in the process
        try:
            spec = importlib.util.find_spec('torch')
        except (ImportError, ValueError):
            spec = None
        where = list(getattr(spec, 'submodule_search_locations', None) or [])
        if not where or not os.path.exists(os.path.join(where[0], 'lib', 'libamdhip64.so')):
            return
        _torch_lib_dir = os.path.join(where[0], 'lib')
    path = os.path.join(_torch_lib_dir, name)
    if os.path.exists(path):
        C.CDLL(path, mode=C.RTLD_GLOBAL)


# ROCm maps the HIP streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4), and a
# process of this package can have more streams than that (a plan's lanes and tail, the stream of
# every one-kernel plan of a chain, upload, download, the caller's); streams that share a queue
# take turns.  Rounds 4-5 set the variable to 16 here when it was unset, for the host path (an
# upload and a download that share a queue: 2.38 instead of 2.57 Gsamples/s host to host).  Measured
# at the end of round 5 (profiles/r05_hw_queues.txt, alternating runs in one box): with 8 or 16
# queues reads of device-resident chains are SLOWER -- `Dedisperse` on 160 blocks 38 against 47 G,
# `Power(Channelize(Dedisperse))` 35 against 44 G, `Resample` 133 against 154 G -- and the headline
# (768 blocks per call) does not care (51.3-51.9 G either way).  The resident path is the product,
# so the package leaves ROCm's default alone (the host path of the final round-5 run read 2.53
# Gsamples/s with 4 queues: profiles/r05_bench_final.json).


def lib():
    """The loaded library (loads on first use; raises if it is not built)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                _preload_torch_runtime()
                _preload_torch_runtime('libhiprtc.so')     # (csrc/rtc.hpp opens it by soname)
                if not os.path.exists(LIB_PATH):
                    raise HipLibraryMissing(
                        f"{LIB_PATH} not found: build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
                handle = C.CDLL(LIB_PATH)
                handle.bbt_last_error.restype = C.c_char_p
                handle.bbt_last_error.argtypes = []
                # (the version first: an older library lacks entry points the table below names)
                if handle.bbt_version() < MIN_LIB_VERSION:
                    raise HipLibraryMissing(
                        f"{LIB_PATH} is version {handle.bbt_version()}, this package needs "
                        f">= {MIN_LIB_VERSION}: rebuild it (python -c 'import __graft_entry__ as g; g.build()').")
                for name, argtypes in SIGNATURES.items():
                    fn = getattr(handle, name)
                    fn.argtypes = argtypes
                    fn.restype = _int
                _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        raise HipError(lib().bbt_last_error().decode(errors='replace'))


def device_count():
    n = _int(0)
    check(lib().bbt_device_count(C.byref(n)))
    return n.value


def available():
    """True if the library loads and sees at least one GPU."""
    try:
        return device_count() > 0
    except (HipError, HipLibraryMissing, OSError):
        return False


def set_device(index):
    check(lib().bbt_set_device(int(index)))


def get_device():
    index = _int(0)
    check(lib().bbt_get_device(C.byref(index)))
    return index.value


def rtc_info():
    """Run-time specialisation of the kernels for lengths that are not powers of two
    (include/bbt_hip.h: bbt_rtc_info): dict(mode, modules, seconds)."""
    mode, modules, seconds = _int(0), _i64(0), C.c_double(0)
    check(lib().bbt_rtc_info(C.byref(mode), C.byref(modules), C.byref(seconds)))
    return dict(mode=('off', 'on', 'required')[mode.value], modules=modules.value, seconds=seconds.value)


def tuning_scratch(release=False):
    """Bytes of scratch device memory the library keeps on the current device for plans that time
    their candidate kernels when they are made (include/bbt_hip.h: bbt_tune_scratch);
    ``release=True`` frees them."""
    held = _i64(0)
    check(lib().bbt_tune_scratch(int(bool(release)), C.byref(held)))
    return held.value


def device_name():
    buf = C.create_string_buffer(256)
    check(lib().bbt_device_name(buf, 256))
    return buf.value.decode()


# The stream all work of this package is queued on (a hipStream_t as int;
# None / 0 = the default stream).  bench.py points it at torch's stream.
_stream = None
_NO_STREAM = object()


def set_stream(stream):
    """Queue all further work of this package on ``stream`` (a hipStream_t as
    int; None / 0 = the default stream).  Also becomes the stream the device
    memory pool orders the reuse of freed blocks by (include/bbt_hip.h)."""
    global _stream
    _stream = int(stream) if stream else None
    check(lib().bbt_pool_set_stream(_stream))


def get_stream():
    return _stream


def synchronize():
    check(lib().bbt_stream_sync(_stream))


class Event:
    def __init__(self):
        self._h = C.c_void_p()
        check(lib().bbt_event_create(C.byref(self._h)))

    def record(self):
        check(lib().bbt_event_record(self._h, _stream))
        return self

    def synchronize(self):
        check(lib().bbt_event_sync(self._h))

    def elapsed_ms(self, later):
        ms = C.c_float()
        check(lib().bbt_event_elapsed_ms(self._h, later._h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if self._h:
                lib().bbt_event_destroy(self._h)
        except Exception:
            pass


def pool_trim():
    """Return every idle block of the device memory pool to the driver."""
    check(lib().bbt_pool_trim())


def pool_info():
    """(idle bytes kept for reuse, bytes in use) of the device memory pool."""
    cached, live = C.c_int64(), C.c_int64()
    check(lib().bbt_pool_info(C.byref(cached), C.byref(live)))
    return cached.value, live.value


#: Plan calls whose output this package owns are issued with a deferred join
#: (include/bbt_hip.h: bbt_osm_plan_defer): the stream is not ordered after the plan's lanes, so
#: consecutive calls -- a reader taking run after run of frames -- flow into each other without
#: a drain at the call boundary; the completion event travels with the output's allocation and
#: is waited for by whatever touches that memory next (`DeviceArray.ptr`).  ``BBT_DEFER=0``:
#: every call joins its stream (round 3's behaviour).
DEFER_JOIN = os.environ.get('BBT_DEFER', '1') != '0'


class _EventPool:
    """Completion events of deferred plan calls: ordering events (no timing, no system-scope fence
    -- streams wait for them, the host never does).  An event goes back to the pool as soon as the
    wait for it has been queued: a stream's wait refers to the record that preceded it."""

    def __init__(self):
        self._idle = []
        self._lock = threading.Lock()

    def take(self):
        with self._lock:
            if self._idle:
                return self._idle.pop()
        h = C.c_void_p()
        check(lib().bbt_event_create_ordering(C.byref(h)))
        return h

    def give(self, h):
        with self._lock:
            self._idle.append(h)


_events = _EventPool()


class _Done:
    """The completion event of one deferred plan call, shared by the allocations the call reads
    and writes; back to the pool once each of them has queued its wait."""
    __slots__ = ('event', 'refs')

    def __init__(self, event, refs):
        self.event = event
        self.refs = refs

    def release(self):
        self.refs -= 1
        if self.refs == 0:
            _events.give(self.event)


class _Pending:
    """What a deferred plan call still owes an allocation -- it is writing it, or reading it --:
    the event that marks the call's end and the objects (the input, the plan) that must outlive
    the call."""
    __slots__ = ('done', 'keep')

    def __init__(self, done, keep):
        self.done = done
        self.keep = keep


def _prune(owed):
    """Let go of the leading entries of a list of deferred READERS whose calls have finished
    (`bbt_event_query`: never blocks): each keeps its plan -- and through the plan its streams and
    work buffers -- alive, and a task that was dropped long ago would otherwise be destroyed (a
    device-wide wait: hipFree) in the middle of whatever read happens to push its entry out, 64
    calls later.  Found with tools/chain_host_probe.py: `Dedisperse(Resample(x))` after other chains
    on the same tensor, two calls of every read blocked 2.5-3 ms in `bbt_osm_plan_destroy` (18.6
    instead of 29 G).  Readers only: a finished reader leaves nothing to make visible.  Returns
    what is left (a tuple for a tuple, the list itself, shortened, for a list)."""
    n, done = 0, C.c_int(0)
    while n < len(owed):
        if lib().bbt_event_query(owed[n].done.event, C.byref(done)) != 0 or not done.value:
            break
        n += 1
    if not n:
        return owed
    gone = owed[:n]
    if isinstance(owed, list):
        del owed[:n]
    else:
        owed = owed[n:]
    for p in gone:
        p.done.release()
    return owed


class _Allocation:
    """Owns one block of the device memory pool, and the calls it is still owed: deferred plan
    calls that are WRITING somewhere in it (`writes`) or READING it (`reads`).  A later reader
    must come after the writes, a later writer -- or the return of the block to the pool -- after
    both; calls that only read may share it, and so may calls that write regions the caller knows
    to be disjoint (`DeviceArray.fresh`: the runs of one big read)."""
    writes = ()
    reads = ()

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        check(lib().bbt_malloc(C.byref(self.ptr), max(self.nbytes, 1)))

    @property
    def pending(self):
        return bool(self.writes or self.reads)

    _MAX_OWED = 64

    def owe(self, pending, write):
        """Note a deferred call that writes (reads) this block.  The lists stay short: beyond
        _MAX_OWED entries the oldest is waited for on the current stream (it finished long ago:
        the wait costs nothing) and let go."""
        owed = (self.writes if write else _prune(self.reads)) + (pending,)
        if len(owed) > self._MAX_OWED:
            old, owed = owed[0], owed[1:]
            check(lib().bbt_stream_wait_event(_stream, old.done.event))
            old.done.release()
        if write:
            self.writes = owed
        else:
            self.reads = owed

    def settle(self, stream=_NO_STREAM, reads=True):
        """Order ``stream`` (default: the package's current stream) after the deferred calls that
        still write this block and -- unless ``reads`` is False: the caller only wants to read --
        after those that still read it."""
        owed = self.writes + (self.reads if reads else ())
        if not owed:
            return
        self.writes = ()
        if reads:
            self.reads = ()
        target = _stream if stream is _NO_STREAM else stream
        for p in owed:
            check(lib().bbt_stream_wait_event(target, p.done.event))
            p.done.release()

    def __del__(self):
        try:
            if self.ptr:
                # (reuse of a freed block is ordered by the pool stream: it must come after the
                # deferred writer too; the writer's inputs are released after this block)
                self.settle()
                lib().bbt_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


# Deferred plan calls that still READ memory this package does not own (a torch tensor handed in
# as a stream's samples): id(owner) -> (weak reference to the owner, [_Pending, ...]).  The owner
# has no `_Allocation` to carry the events, so whoever is about to OVERWRITE such memory in place
# asks `wait_for_readers` first (include/bbt_hip.h: a deferred call's input stays untouched until
# its completion event).
_foreign_reads = {}
_FOREIGN_MAX = 64


def _owe_foreign_read(owner, pending):
    key = id(owner)
    entry = _foreign_reads.get(key)
    if entry is None or entry[0]() is not owner:
        try:
            ref = weakref.ref(owner, lambda _r, k=key: _drop_foreign(k))
        except TypeError:
            return False
        entry = _foreign_reads[key] = (ref, [])
    _prune(entry[1])
    entry[1].append(pending)
    if len(entry[1]) > _FOREIGN_MAX:
        old = entry[1].pop(0)
        check(lib().bbt_stream_wait_event(_stream, old.done.event))
        old.done.release()
    return True


def _drop_foreign(key):
    entry = _foreign_reads.pop(key, None)
    if entry is not None:
        for p in entry[1]:
            try:
                p.done.release()
            except Exception:
                pass


def wait_for_readers(array, stream=_NO_STREAM):
    """Order ``stream`` (default: the package's current stream) after every deferred plan call
    that still reads ``array`` -- a `DeviceArray`, or the foreign object (a torch tensor) that was
    handed to `DeviceStream` / `as_device_array`.  Call it before refilling such an input in
    place on that stream; memory of this package needs no call (`DeviceArray.ptr` waits)."""
    owner = array.owner if isinstance(array, DeviceArray) else array
    if owner.__class__ is _Allocation:
        owner.settle(stream)
        return
    entry = _foreign_reads.get(id(owner))
    if entry is None or entry[0]() is not owner:
        return
    target = _stream if stream is _NO_STREAM else stream
    owed, entry[1][:] = list(entry[1]), []
    for p in owed:
        check(lib().bbt_stream_wait_event(target, p.done.event))
        p.done.release()


class DeviceArray:
    """C-contiguous array in HBM: (ptr, shape, dtype); leading-axis slices are
    zero-copy views.  ``owner`` keeps the allocation (or a foreign object such
    as a torch tensor) alive."""

    def __init__(self, shape, dtype=np.complex64, ptr=None, owner=None):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        if ptr is None:
            owner = _Allocation(self.nbytes)
            ptr = owner.ptr.value
        self._ptr = int(ptr) if ptr else 0
        # (a view of a view is kept alive by -- and shares the pending state of -- the root)
        self.owner = owner.owner if isinstance(owner, DeviceArray) else owner

    @property
    def ptr(self):
        """Device address.  Asking for it is the announcement of a use: if a deferred plan call
        still owes this memory (`_Allocation.pending`), the current stream is first ordered after
        that call -- every binding, copy and interop path goes through here."""
        o = self.owner
        if o.__class__ is _Allocation and (o.writes or o.reads):
            o.settle()
        return self._ptr

    def ptr_to_read(self):
        """The address for a use that only READS the array: ordered after the deferred calls that
        still write its allocation, not after those that merely read it too."""
        o = self.owner
        if o.__class__ is _Allocation and o.writes:
            o.settle(reads=False)
        return self._ptr

    #: Set by a caller that hands this view to a plan call as output and KNOWS that no call still
    #: owed to the allocation touches the view's region (the consecutive runs of one big read fill
    #: disjoint slices of a fresh array): the call is then not ordered after those calls.
    fresh = False

    @property
    def pending(self):
        """Is a deferred plan call still writing or reading this array's allocation (nobody has
        waited for it yet)?"""
        o = self.owner
        return o.__class__ is _Allocation and bool(o.writes or o.reads)

    @property
    def size(self):
        n = 1
        for d in self.shape:
            n *= d
        return n

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def row_bytes(self):
        n = self.dtype.itemsize
        for d in self.shape[1:]:
            n *= d
        return n

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, item):
        if not isinstance(item, slice):
            raise TypeError("DeviceArray supports only leading-axis slices")
        start, stop, step = item.indices(self.shape[0])
        if step != 1:
            raise ValueError("DeviceArray slices must be contiguous")
        stop = max(stop, start)
        view = DeviceArray((stop - start,) + self.shape[1:], self.dtype,
                           self._ptr + start * self.row_bytes, self.owner)
        if self.fresh:
            view.fresh = True              # (part of a region nobody is owed is such a region)
        return view

    def reshape(self, *shape):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        shape = list(shape)
        if -1 in shape:
            known = 1
            for d in shape:
                if d != -1:
                    known *= d
            shape[shape.index(-1)] = self.size // known if known else 0
        out = DeviceArray(shape, self.dtype, self._ptr, self.owner)
        if out.size != self.size:
            raise ValueError(f"cannot reshape {self.shape} into {tuple(shape)}")
        if self.fresh:
            out.fresh = True
        return out

    @classmethod
    def from_host(cls, array, dtype=None):
        array = np.ascontiguousarray(array, dtype=dtype)
        out = cls(array.shape, array.dtype)
        out.copy_from_host(array)
        return out

    def copy_from_host(self, array):
        array = np.ascontiguousarray(array, dtype=self.dtype)
        if array.nbytes != self.nbytes:
            raise ValueError("size mismatch in host to device copy")
        if array.nbytes:
            check(lib().bbt_memcpy_h2d(self.ptr, array.ctypes.data, array.nbytes, _stream))
            # pageable host memory: make sure the source may be released
            check(lib().bbt_stream_sync(_stream))
        return self

    def copy_from_device(self, other):
        if other.nbytes != self.nbytes:
            raise ValueError("size mismatch in device to device copy")
        if self.nbytes:
            # (the source is only read: after the calls that still write it, beside those that read it too)
            check(lib().bbt_memcpy_d2d(self.ptr, other.ptr_to_read(), self.nbytes, _stream))
        return self

    def to_host(self, out=None):
        if out is None:
            out = np.empty(self.shape, self.dtype)
        elif (not isinstance(out, np.ndarray) or out.dtype != self.dtype
              or not out.flags.c_contiguous or out.shape != self.shape):
            tmp = self.to_host()
            out[...] = tmp
            return out
        if self.nbytes:
            check(lib().bbt_memcpy_d2h(out.ctypes.data, self.ptr_to_read(), self.nbytes, _stream))
            check(lib().bbt_stream_sync(_stream))
        return out

    def fill_bytes(self, value):
        if self.nbytes:
            check(lib().bbt_memset(self.ptr, int(value), self.nbytes, _stream))
        return self

    @property
    def __cuda_array_interface__(self):
        return dict(shape=self.shape, typestr=self.dtype.str, data=(self.ptr, False),
                    version=3, strides=None)

    def __repr__(self):
        return f"<DeviceArray shape={self.shape} dtype={self.dtype} ptr=0x{self._ptr:x}>"


def as_device_array(obj):
    """DeviceArray view of a DeviceArray or a torch tensor on the GPU."""
    if isinstance(obj, DeviceArray):
        return obj
    if hasattr(obj, 'data_ptr') and hasattr(obj, 'is_contiguous'):   # torch
        if not obj.is_contiguous():
            raise ValueError("tensor must be contiguous")
        import torch
        dt = {torch.complex64: np.complex64, torch.float32: np.float32,
              torch.complex128: np.complex128, torch.float64: np.float64}[obj.dtype]
        return DeviceArray(tuple(obj.shape), dt, obj.data_ptr(), obj)
    raise TypeError(f"cannot interpret {type(obj)} as a device array")


def copy_2d(dst, dst_pitch, src, src_pitch, src_offset, width, rows):
    """Device-to-device copy of ``rows`` runs of ``width`` bytes: run r goes
    from src + src_offset + r * src_pitch to dst + r * dst_pitch."""
    if rows and width:
        check(lib().bbt_memcpy2d(dst.ptr, int(dst_pitch), src.ptr_to_read() + int(src_offset), int(src_pitch),
                                 int(width), int(rows), 2, _stream))
    return dst


def pad_streams_to_even(dev, n_stream):
    """(n, S) complex64 with odd S -> (n, S+1) with a zero stream appended."""
    n = dev.size // n_stream
    out = DeviceArray((n, n_stream + 1), dev.dtype)
    check(lib().bbt_pad_streams(dev.ptr_to_read(), out.ptr, n, n_stream, n_stream + 1, dev.dtype.itemsize, _stream))
    return out


def strip_stream_pad(dev_padded, n_rows, n_stream, out):
    """inverse of pad_streams_to_even for rows of (S+1) -> S elements."""
    isz = dev_padded.dtype.itemsize
    if n_rows:
        check(lib().bbt_memcpy2d(out.ptr, n_stream * isz, dev_padded.ptr_to_read(), (n_stream + 1) * isz,
                                 n_stream * isz, n_rows, 2, _stream))
    return out


def detect_integrate(in_dev, out_dev, n_out, step, n_elem, mode, average=True):
    """Square (mode 0) / Power (1) / plain sum (2) over ``step`` samples."""
    check(lib().bbt_detect_integrate(in_dev.ptr_to_read(), out_dev.ptr, int(n_out), int(step), int(n_elem),
                                     int(mode), int(bool(average)), _stream))


#: shares a slot of `fold_runs` may be split into (bounds its work area)
FOLD_MAX_SPLIT = 64


def fold_runs(in_dev, out_dev, n_elem, mode, slot_ptr, run_begin, run_end, scale=None,
              accumulate=False):
    """Sum (after detection ``mode``, as `detect_integrate`) the input samples of every run of
    every slot into rows of ``out_dev`` (see bbt_fold_runs in include/bbt_hip.h).

    ``slot_ptr`` (n_slot + 1), ``run_begin`` / ``run_end`` are host int64 arrays (checked
    against the input here, then uploaded); ``scale`` an optional float32 array (n_slot)."""
    slot_ptr = np.ascontiguousarray(slot_ptr, dtype=np.int64)
    run_begin = np.ascontiguousarray(run_begin, dtype=np.int64)
    run_end = np.ascontiguousarray(run_end, dtype=np.int64)
    n_slot = len(slot_ptr) - 1
    n_in = in_dev.shape[0] if in_dev.shape else 0
    if n_slot < 0 or run_begin.shape != run_end.shape or slot_ptr[0] != 0 or slot_ptr[-1] != len(run_begin):
        raise ValueError("fold_runs: slot_ptr does not describe the runs")
    if n_slot == 0:
        return out_dev
    if np.any(np.diff(slot_ptr) < 0):
        raise ValueError("fold_runs: slot_ptr must not decrease")
    if len(run_begin) and (run_begin.min() < 0 or run_end.max() > n_in or np.any(run_end < run_begin)):
        raise ValueError("fold_runs: runs outside the input")
    n_out_f = 2 * int(n_elem) if mode == 1 else int(n_elem)
    if out_dev.size * (2 if out_dev.dtype.kind == 'c' else 1) != n_slot * n_out_f:
        raise ValueError("fold_runs: output is not n_slot rows of the mode's width")
    if in_dev.size * (2 if in_dev.dtype.kind == 'c' else 1) != n_in * int(n_elem) * (1 if mode == 2 else 2):
        raise ValueError("fold_runs: input is not n_in samples of n_elem elements")
    n_runs = len(run_begin)
    table = DeviceArray.from_host(np.concatenate([slot_ptr, run_begin, run_end]))
    tptr = table.ptr
    return _fold_launch(in_dev, out_dev, n_in, n_elem, mode, tptr, tptr + 8 * (n_slot + 1),
                        tptr + 8 * (n_slot + 1 + n_runs), n_slot, n_out_f, scale, accumulate)


def _fold_launch(in_dev, out_dev, n_in, n_elem, mode, sp_ptr, rb_ptr, re_ptr, n_slot, n_out_f, scale, accumulate):
    sc = DeviceArray.from_host(np.ascontiguousarray(scale, dtype=np.float32)) if scale is not None else None
    work_floats = min(FOLD_MAX_SPLIT * n_slot * n_out_f, 1 << 24)
    work = DeviceArray((work_floats,), np.float32) if work_floats >= 2 * n_slot * n_out_f else None
    check(lib().bbt_fold_runs(in_dev.ptr_to_read(), out_dev.ptr, int(n_in), int(n_elem), int(mode),
                              sp_ptr, rb_ptr, re_ptr,
                              int(n_slot), sc.ptr if sc is not None else None, int(bool(accumulate)),
                              work.ptr if work is not None else None,
                              int(work_floats) if work is not None else 0, _stream))
    return out_dev


def fold_runs_device(in_dev, out_dev, n_elem, mode, slot_ptr, run_begin, run_end, scale=None,
                     accumulate=False):
    """`fold_runs` with the table already in HBM (int64 `DeviceArray`s, as `phase_runs` makes
    them; the kernel clips runs to the input)."""
    n_slot = slot_ptr.shape[0] - 1
    if n_slot <= 0:
        return out_dev
    n_in = in_dev.shape[0] if in_dev.shape else 0
    n_out_f = 2 * int(n_elem) if mode == 1 else int(n_elem)
    if out_dev.size * (2 if out_dev.dtype.kind == 'c' else 1) != n_slot * n_out_f:
        raise ValueError("fold_runs: output is not n_slot rows of the mode's width")
    if in_dev.size * (2 if in_dev.dtype.kind == 'c' else 1) != n_in * int(n_elem) * (1 if mode == 2 else 2):
        raise ValueError("fold_runs: input is not n_in samples of n_elem elements")
    return _fold_launch(in_dev, out_dev, n_in, n_elem, mode, slot_ptr.ptr_to_read(), run_begin.ptr_to_read(),
                        run_end.ptr_to_read(), n_slot, n_out_f, scale, accumulate)


def _piece_words(plan):
    """The 8-byte words of the pieces of a plan (`~baseband_tasks_amd.fold_table.plan_pieces`),
    as bbt_phase_runs and bbt_modulate_pieces read them."""
    return np.concatenate([plan['lo'].astype(np.int64).view(np.float64), plan['m0'].astype(np.int64).view(np.float64),
                           plan['row'].astype(np.int64).view(np.float64), plan['dt0'], plan['step'], plan['ref_int'],
                           plan['ref_frac'], plan['coeff'].ravel()]).astype(np.float64, copy=False)


def phase_runs(plan, n_phase, slot0=0, n_slot=None):
    """Run table of a chunk from polynomial phases, made on the GPU (bbt_phase_runs).

    ``plan``: what `~baseband_tasks_amd.fold_table.plan_pieces` returns.  Returns (slot_ptr,
    run_begin, run_end) as int64 `DeviceArray`s -- slot_ptr has ``n_slot + 1`` entries, the
    chunk's rows starting at slot ``slot0``; run_begin / run_end hold ``n_run`` runs -- then
    ``n_run`` and the samples per slot of the chunk's rows (host int64)."""
    n_piece, n_row = len(plan['row']), len(plan['k0'])
    n_chunk_slot = n_row * int(n_phase)
    n_slot = n_chunk_slot + slot0 if n_slot is None else int(n_slot)
    n_coeff = plan['coeff'].shape[1]
    pieces = DeviceArray.from_host(_piece_words(plan))
    cell0 = np.concatenate(([0], np.cumsum(plan['n_cycle'] * int(n_phase))))
    n_cell = int(cell0[-1])
    rows = DeviceArray.from_host(np.concatenate([plan['k0'], plan['n_cycle'], cell0[:-1]]).astype(np.int64))
    s_begin, s_end, run_cap = int(plan['lo'][0]), int(plan['lo'][-1]), int(plan['run_cap'])
    need = C.c_int64()
    check(lib().bbt_phase_runs_work(s_end - s_begin, n_cell, run_cap, C.byref(need)))
    work = DeviceArray((need.value,), np.uint8)                  # (exactly: no slack for the layout to lean on)
    slot_ptr = DeviceArray((n_slot + 1,), np.int64)
    runs = DeviceArray((2, run_cap), np.int64)
    counts = DeviceArray((n_chunk_slot,), np.int64)
    info = (C.c_int64 * 2)()
    check(lib().bbt_phase_runs(pieces.ptr, n_piece, n_coeff, s_begin, s_end, int(n_phase), rows.ptr, n_row, n_cell,
                               int(slot0), n_slot, run_cap, slot_ptr.ptr, runs.ptr, runs.ptr + 8 * run_cap,
                               counts.ptr, work.ptr, work.nbytes, info, _stream))
    if info[1] != 0:
        raise ValueError("phase_runs: the phase does not increase with time (or the plan does not "
                         f"describe it): status {info[1]}, {info[0]} runs for a capacity of {run_cap}")
    n_run = int(info[0])
    return slot_ptr, runs[0:1].reshape(run_cap)[:n_run], runs[1:2].reshape(run_cap)[:n_run], n_run, counts.to_host()


def _modulate_sizes(who, in_dev, out_dev, n_elem, gain):
    """Checks shared by `modulate_runs` and `modulate_pieces`: (n_in, floats per sample, n_phase,
    gain stride)."""
    n_elem = int(n_elem)
    n_in = in_dev.shape[0] if in_dev.shape else 0
    if in_dev.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)) or out_dev.dtype != in_dev.dtype:
        raise TypeError(f"{who}: input and output must both be float32 or both complex64")
    if n_elem < 1 or n_in < 1 or in_dev.size != n_in * n_elem:
        raise ValueError(f"{who}: input is not n_in >= 1 samples of n_elem elements")
    if out_dev.size != in_dev.size:
        raise ValueError(f"{who}: output is not the size of the input")
    if gain.dtype != np.dtype(np.float32) or len(gain.shape) not in (1, 2) or gain.shape[0] < 1:
        raise ValueError(f"{who}: the gains must be float32, (n_phase,) or (n_phase, n_elem)")
    if len(gain.shape) == 2 and gain.shape[1] != n_elem:
        raise ValueError(f"{who}: gains of {gain.shape[1]} elements for samples of {n_elem}")
    n_float = n_elem * (2 if in_dev.dtype.kind == 'c' else 1)
    return n_in, n_float, gain.shape[0], (n_elem if len(gain.shape) == 2 else 0)


def modulate_runs(in_dev, out_dev, n_elem, gain, run_begin, run_bin):
    """``out[n, e] = in[n, e] * gain[bin(n), e]`` (or ``gain[bin(n)]`` for gains of shape
    (n_phase,)), with ``bin(n) = run_bin[r]`` for the run ``r`` that holds sample ``n`` (see
    bbt_modulate_runs in include/bbt_hip.h).

    ``gain`` is a float32 `DeviceArray`; ``run_begin`` / ``run_bin`` are host int64 arrays in time
    order (checked here, then uploaded): the runs tile [0, n_in), the bins lie in [0, n_phase)."""
    n_in, n_float, n_phase, stride = _modulate_sizes('modulate_runs', in_dev, out_dev, n_elem, gain)
    run_begin = np.ascontiguousarray(run_begin, dtype=np.int64)
    run_bin = np.ascontiguousarray(run_bin, dtype=np.int64)
    if run_begin.ndim != 1 or run_begin.shape != run_bin.shape or len(run_begin) < 1:
        raise ValueError("modulate_runs: run_begin and run_bin must be 1-d, of one length >= 1")
    if run_begin[0] != 0 or run_begin[-1] >= n_in or np.any(np.diff(run_begin) <= 0):
        raise ValueError("modulate_runs: the runs do not tile the input")
    if run_bin.min() < 0 or run_bin.max() >= n_phase:
        raise ValueError("modulate_runs: bins outside the profile")
    n_run = len(run_begin)
    table = DeviceArray.from_host(np.concatenate([run_begin, run_bin]))
    tptr = table.ptr
    check(lib().bbt_modulate_runs(in_dev.ptr_to_read(), out_dev.ptr, n_in, n_float, gain.ptr_to_read(), n_phase,
                                  stride, tptr, tptr + 8 * n_run, n_run, _stream))
    return out_dev


def modulate_pieces(in_dev, out_dev, n_elem, gain, plan):
    """`modulate_runs` with the bins evaluated on the GPU from polynomial pieces
    (bbt_modulate_pieces): ``plan`` is what `~baseband_tasks_amd.fold_table.plan_pieces` returns
    for the input's samples, whose pieces must tile [0, n_in)."""
    n_in, n_float, n_phase, stride = _modulate_sizes('modulate_pieces', in_dev, out_dev, n_elem, gain)
    lo = np.asarray(plan['lo'], dtype=np.int64)
    n_piece = len(plan['row'])
    if n_piece < 1 or len(lo) != n_piece + 1 or lo[0] != 0 or lo[-1] != n_in or np.any(np.diff(lo) <= 0):
        raise ValueError("modulate_pieces: the pieces do not tile the input")
    pieces = DeviceArray.from_host(_piece_words(plan))
    check(lib().bbt_modulate_pieces(in_dev.ptr_to_read(), out_dev.ptr, n_in, n_float, gain.ptr_to_read(), n_phase,
                                    stride, pieces.ptr, n_piece, int(plan['coeff'].shape[1]), _stream))
    return out_dev


#: bounds of the spectral-kurtosis entry points (csrc/sk_geo.hpp)
SK_MAX_N, SK_MAX_GROUP = 65536, 64


def _sk_sizes(who, x, n, n_elem, averaged):
    """Checks shared by `sk_estimate` and `sk_excise`: (n_block, n, n_elem, is_complex, averaged)."""
    if not isinstance(x, DeviceArray):
        raise TypeError(f"{who}: the input must be a DeviceArray, not {type(x).__name__}")
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
        raise TypeError(f"{who}: the input must be float32 or complex64, not {x.dtype}")
    n, n_elem, averaged = int(n), int(n_elem), float(averaged)
    if not 2 <= n <= SK_MAX_N:
        raise ValueError(f"{who}: n must be 2 ... {SK_MAX_N}, not {n}")
    if not 0. < averaged <= 1e9:
        raise ValueError(f"{who}: averaged must be positive, not {averaged}")
    n_in = x.shape[0] if x.shape else 0
    if n_elem < 1 or n_in < 1 or x.size != n_in * n_elem or n_in % n:
        raise ValueError(f"{who}: the input is not whole blocks of {n} samples of {n_elem} elements "
                         f"(shape {tuple(x.shape)})")
    return n_in // n, n, n_elem, int(x.dtype.kind == 'c'), averaged


def sk_estimate(x, n, n_elem, averaged=1., out=None):
    """Spectral kurtosis of every block of ``n`` samples and every element of a float32 (powers) or
    complex64 `DeviceArray` ``x`` of ``n_block * n`` samples of ``n_elem`` elements
    (bbt_sk_estimate in include/bbt_hip.h; `rfi.spectral_kurtosis` is the NumPy restatement).
    Returns float32 ``(n_block, n_elem)`` (``out`` if given)."""
    n_block, n, n_elem, cplx, averaged = _sk_sizes('sk_estimate', x, n, n_elem, averaged)
    if out is None:
        out = DeviceArray((n_block, n_elem), np.float32)
    elif not isinstance(out, DeviceArray) or out.dtype != np.dtype(np.float32) or out.size != n_block * n_elem:
        raise ValueError(f"sk_estimate: out must be a float32 DeviceArray of {n_block * n_elem} values")
    check(lib().bbt_sk_estimate(x.ptr_to_read(), out.ptr, n_block, n, n_elem, cplx, averaged, _stream))
    return out


def sk_excise(x, out, n, n_elem, limits, averaged=1., group=1, sk=None, flags=None):
    """``out`` = ``x`` with every (block of ``n`` samples, group of ``group`` adjacent elements)
    zeroed in which an element's spectral kurtosis lies outside ``limits = (lo, hi)``, float32
    (bbt_sk_excise; `rfi.excise_samples` is the NumPy restatement).  ``sk``, ``flags``: None, or
    `DeviceArray`s that receive the estimator, float32 ``(n_block, n_elem)``, and the flags,
    uint8 ``(n_block, n_elem / group)``.  Returns ``out``."""
    n_block, n, n_elem, cplx, averaged = _sk_sizes('sk_excise', x, n, n_elem, averaged)
    if not isinstance(out, DeviceArray) or out.dtype != x.dtype or out.size != x.size:
        raise ValueError("sk_excise: the output must be a DeviceArray of the input's dtype and size")
    group = int(group)
    if not 1 <= group <= SK_MAX_GROUP or n_elem % group:
        raise ValueError(f"sk_excise: a group of {group} elements must divide {n_elem} and be at most {SK_MAX_GROUP}")
    lo, hi = (float(np.float32(v)) for v in limits)
    if not lo <= hi:
        raise ValueError(f"sk_excise: the limits must be ordered, not {(lo, hi)}")
    for name, arr, dtype, size in (('sk', sk, np.float32, n_block * n_elem),
                                   ('flags', flags, np.uint8, n_block * (n_elem // group))):
        if arr is not None and (not isinstance(arr, DeviceArray) or arr.dtype != np.dtype(dtype) or arr.size != size):
            raise ValueError(f"sk_excise: {name} must be a {np.dtype(dtype)} DeviceArray of {size} values")
    check(lib().bbt_sk_excise(x.ptr_to_read(), out.ptr, n_block, n, n_elem, cplx, averaged, lo, hi, group,
                              None if sk is None else sk.ptr, None if flags is None else flags.ptr, _stream))
    return out


#: relative margin inside which a comparison of the normal sampler that goes through exp / log1p is
#: left to NumPy (see bbt_philox_normal in include/bbt_hip.h)
NOISE_GUARD = 2.0 ** -46


def noise_word_count(n):
    """Words of the Philox stream examined first for n normals: 4 * ceil((1.03 n + 256) / 4)
    (the sampler takes 1.022 words per normal on average)."""
    return 4 * (-(-(103 * int(n) + 25600) // 400))


def philox_normal(out, key, counters, n=None, n_words=None, guard=NOISE_GUARD):
    """NumPy's normals on the GPU (bbt_philox_normal): row f of ``out`` (a float32 `DeviceArray`
    of shape (n_frame, stride)) gets the first ``n`` (default: stride) values, rounded to float32,
    that ``Generator(Philox).normal`` gives for a state with this ``key`` (two uint64), counter
    ``counters[f]`` (four uint64) and an empty buffer.

    ``n_words`` words of the stream are examined per frame (default `noise_word_count`); frames
    whose words hold fewer than n normals are run again with the number doubled, until they do.
    Returns (flags, reruns): flags[f] is True if a decision of frame f was too close to call
    between this device's and the host's math library -- its row is then to be made with NumPy --
    and reruns counts the runs of a frame that had to be repeated with more words."""
    if out.dtype != np.float32 or len(out.shape) != 2:
        raise TypeError("philox_normal: out must be a float32 DeviceArray of shape (n_frame, stride)")
    n_frame, stride = out.shape
    n = stride if n is None else int(n)
    key = np.ascontiguousarray(key, dtype=np.uint64)
    counters = np.ascontiguousarray(counters, dtype=np.uint64)
    if key.shape != (2,) or counters.shape != (n_frame, 4):
        raise ValueError("philox_normal: key must hold 2 and counters (n_frame, 4) uint64")
    if not 1 <= n <= stride:
        raise ValueError("philox_normal: n must be between 1 and the row length of out")
    n_words = noise_word_count(n) if n_words is None else int(n_words)
    flags = np.zeros(n_frame, bool)
    todo = np.arange(n_frame)
    reruns = 0
    while len(todo):
        # (runs of consecutive frames share a call; after a shortfall usually one frame is left)
        first = int(todo[0])
        count = 1
        while count < len(todo) and todo[count] == first + count and count < 65535:
            count += 1
        need = C.c_int64()
        check(lib().bbt_philox_normal_work(count, n_words, C.byref(need)))
        work = DeviceArray((need.value // 8 + 2,), np.int64)
        totals = np.zeros(count, np.int64)
        flagged = np.zeros(count, np.int64)
        piece = out[first:first + count]
        ctr = counters[first:first + count]
        check(lib().bbt_philox_normal(key.ctypes.data, ctr.ctypes.data, count, n, n_words, float(guard),
                                      piece.ptr, stride, work.ptr, work.nbytes,
                                      totals.ctypes.data_as(_pi64), flagged.ctypes.data_as(_pi64), _stream))
        flags[first:first + count] = flagged != 0
        short = first + np.nonzero((totals < n) & (flagged == 0))[0]
        todo = todo[count:]
        for f in short:
            sub_flags, again = philox_normal(out[int(f):int(f) + 1], key, counters[f:f + 1], n, 2 * n_words, guard)
            flags[f] = sub_flags[0]
            reruns += 1 + again
    return flags, reruns


def detect_power_axis(in_dev, out_dev, n_out, step, outer, inner, average=True):
    """Power (mode 1 of `detect_integrate`) for samples (outer, 2, inner)."""
    check(lib().bbt_detect_power_axis(in_dev.ptr_to_read(), out_dev.ptr, int(n_out), int(step), int(outer), int(inner),
                                      int(bool(average)), _stream))


def real_to_complex(x):
    """float32 DeviceArray -> complex64 with zero imaginary part (same shape)."""
    out = DeviceArray(x.shape, np.complex64)
    check(lib().bbt_real_op(x.ptr_to_read(), out.ptr, 0, out.size, 0, 0, _stream))
    return out


def real_part(z, out=None):
    """complex64 DeviceArray -> its real part (float32)."""
    if out is None:
        out = DeviceArray(z.shape, np.float32)
    check(lib().bbt_real_op(z.ptr_to_read(), out.ptr, 1, out.size, 0, 0, _stream))
    return out


def half_to_full_spectrum(z, n_chan, n_stream):
    """(n_spec, n_chan/2+1, n_stream) complex64 -> Hermitian (n_spec, n_chan, n_stream)."""
    n_spec = z.size // ((n_chan // 2 + 1) * n_stream)
    out = DeviceArray((n_spec, n_chan, n_stream), np.complex64)
    check(lib().bbt_real_op(z.ptr_to_read(), out.ptr, 2, out.size, int(n_chan), int(n_stream), _stream))
    return out


def keep_half_spectrum(z, n_chan, n_stream, out):
    """(n_spec, n_chan, n_stream) -> first n_chan/2+1 channels of every spectrum."""
    n_spec = z.size // (n_chan * n_stream)
    half = n_chan // 2 + 1
    if n_spec:
        check(lib().bbt_memcpy2d(out.ptr, half * n_stream * 8, z.ptr_to_read(), n_chan * n_stream * 8,
                                 half * n_stream * 8, n_spec, 2, _stream))
    return out


def split_real_pair_spectra(z, n_chan, n_stream, out, padded=False):
    """Spectra ``(n_spec, n_chan, n_stream/2)`` of complex streams z = a + i b
    -> half spectra ``(n_spec, n_chan/2+1, n_stream)`` of the real streams.
    ``padded``: z carries one more, unused, complex stream."""
    check(lib().bbt_real_op(z.ptr_to_read(), out.ptr, 6 if padded else 4, out.size, int(n_chan), int(n_stream),
                            _stream))
    return out


def merge_real_pair_spectra(z_half, n_chan, n_stream, out):
    """Half spectra ``(n_spec, n_chan/2+1, n_stream)`` of real streams ->
    ``(n_spec, n_chan, n_stream/2)`` spectra of the complex streams a + i b."""
    check(lib().bbt_real_op(z_half.ptr_to_read(), out.ptr, 5, out.size, int(n_chan), int(n_stream), _stream))
    return out


def square_real(x, out):
    check(lib().bbt_real_op(x.ptr_to_read(), out.ptr, 3, out.size, 0, 0, _stream))
    return out


def scale_streams(x, out, n_samples, n_elem, factor_dev):
    """out[i, e] = x[i, e] * factor[e] (complex64)."""
    check(lib().bbt_scale_streams(x.ptr_to_read(), out.ptr, int(n_samples), int(n_elem), factor_dev.ptr, _stream))


#: widths `pack` encodes (and `bbt_unpack` code 0 decodes)
PACK_BITS = (1, 2, 4, 8, 16)


def _components(x, who):
    """Number of float32 components of a float32 / complex64 `DeviceArray`."""
    if not isinstance(x, DeviceArray):
        raise TypeError(f"{who}: the input must be a DeviceArray, not {type(x).__name__}")
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
        raise TypeError(f"{who}: the input must be float32 or complex64, not {x.dtype}")
    return x.size * (2 if x.dtype.kind == 'c' else 1)


def pack(x, bits, out=None):
    """Encode a float32 / complex64 `DeviceArray` (complex: re, im adjacent) into VDIF-coded
    little-endian 32-bit words, the first component in the least significant bits (bbt_pack in
    include/bbt_hip.h; the codes of `ingest.encode_vdif_frames`).  Returns a uint32 `DeviceArray`
    of ``ceil(components * bits / 32)`` words (``out`` if given)."""
    n_comp = _components(x, 'pack')
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or int(bits) not in PACK_BITS:
        raise ValueError(f"pack: bits must be one of {PACK_BITS}, not {bits!r}")
    bits = int(bits)
    n_words = -(-n_comp * bits // 32)
    if out is None:
        out = DeviceArray((n_words,), np.uint32)
    elif not isinstance(out, DeviceArray):
        raise TypeError(f"pack: out must be a DeviceArray, not {type(out).__name__}")
    elif out.dtype != np.dtype(np.uint32):
        raise TypeError(f"pack: out must be uint32, not {out.dtype}")
    elif out.size != n_words:
        raise ValueError(f"pack: out holds {out.size} words; {n_comp} components at {bits} bits make {n_words}")
    if n_comp:
        check(lib().bbt_pack(x.ptr_to_read(), out.ptr, n_comp, bits, 0, _stream))
    return out


def to_half(x, out=None):
    """float32 / complex64 `DeviceArray` -> IEEE binary16 components (bbt_to_half): a float16
    `DeviceArray` of ``x``'s shape, with a last axis of 2 (re, im) added for complex input."""
    n = _components(x, 'to_half')
    shape = x.shape + ((2,) if x.dtype.kind == 'c' else ())
    if out is None:
        out = DeviceArray(shape, np.float16)
    elif not isinstance(out, DeviceArray):
        raise TypeError(f"to_half: out must be a DeviceArray, not {type(out).__name__}")
    elif out.dtype != np.dtype(np.float16):
        raise TypeError(f"to_half: out must be float16, not {out.dtype}")
    elif out.size != n:
        raise ValueError(f"to_half: out holds {out.size} values for {n} components")
    if n:
        check(lib().bbt_to_half(x.ptr_to_read(), out.ptr, n, _stream))
    return out


def from_half(h, dtype=np.float32, out=None):
    """float16 `DeviceArray` -> float32, or complex64 from (re, im) pairs along the last axis
    (bbt_from_half; exact)."""
    if not isinstance(h, DeviceArray):
        raise TypeError(f"from_half: the input must be a DeviceArray, not {type(h).__name__}")
    if h.dtype != np.dtype(np.float16):
        raise TypeError(f"from_half: the input must be float16, not {h.dtype}")
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
        raise TypeError(f"from_half: dtype must be float32 or complex64, not {dtype}")
    if dtype.kind == 'c':
        if not h.shape or h.shape[-1] != 2:
            raise ValueError(f"from_half: complex64 needs a last axis of 2 (re, im), not shape {h.shape}")
        shape = h.shape[:-1]
    else:
        shape = h.shape
    if out is None:
        out = DeviceArray(shape, dtype)
    elif not isinstance(out, DeviceArray):
        raise TypeError(f"from_half: out must be a DeviceArray, not {type(out).__name__}")
    elif out.dtype != dtype:
        raise TypeError(f"from_half: out must be {dtype}, not {out.dtype}")
    elif out.size * (2 if dtype.kind == 'c' else 1) != h.size:
        raise ValueError(f"from_half: out holds {out.size} {dtype} for {h.size} halves")
    if h.size:
        check(lib().bbt_from_half(h.ptr_to_read(), out.ptr, h.size, _stream))
    return out


#: the stored type of a fold-mode profile: int16, big-endian
PSRFITS_CODE = np.dtype('>i2')


def _rows_shape(shape, who):
    """(n_row, n_bin, n_chan, n_pol) of profiles of shape (n_row, n_bin[, n_chan[, n_pol]])."""
    if not 2 <= len(shape) <= 4:
        raise ValueError(f"{who}: profiles have shape (row, bin[, chan[, pol]]), not {tuple(shape)}")
    shape = tuple(shape) + (1,) * (4 - len(shape))
    if min(shape[1:]) < 1:
        raise ValueError(f"{who}: an empty axis in {shape}")
    return shape


def psrfits_encode(x):
    """Code float32 profiles ``(n_row, n_bin[, n_chan[, n_pol]])`` in HBM as the rows of a PSRFITS
    fold-mode table (bbt_psrfits_encode in include/bbt_hip.h; `psrfits.encode_rows` is the NumPy
    restatement).  Returns `DeviceArray`s ``(codes, scl, offs, n_finite)``: big-endian int16
    ``(n_row, n_pol, n_chan, n_bin)``, and float32, float32, int32 ``(n_row, n_pol, n_chan)``."""
    if not isinstance(x, DeviceArray):
        raise TypeError(f"psrfits_encode: the input must be a DeviceArray, not {type(x).__name__}")
    if x.dtype != np.dtype(np.float32):
        raise TypeError(f"psrfits_encode: the input must be float32, not {x.dtype}")
    n_row, n_bin, n_chan, n_pol = _rows_shape(x.shape, 'psrfits_encode')
    codes = DeviceArray((n_row, n_pol, n_chan, n_bin), PSRFITS_CODE)
    scl = DeviceArray((n_row, n_pol, n_chan), np.float32)
    offs = DeviceArray((n_row, n_pol, n_chan), np.float32)
    n_finite = DeviceArray((n_row, n_pol, n_chan), np.int32)
    if n_row:
        check(lib().bbt_psrfits_encode(x.ptr_to_read(), codes.ptr, scl.ptr, offs.ptr, n_finite.ptr,
                                       n_row, n_bin, n_chan, n_pol, _stream))
    return codes, scl, offs, n_finite


def psrfits_decode(codes, scl, offs, wts=None, zero_off=0., out=None):
    """Decode rows of a PSRFITS fold-mode table in HBM (bbt_psrfits_decode): big-endian int16
    ``codes (n_row, n_pol, n_chan, n_bin)``, float32 ``scl`` and ``offs (n_row, n_pol, n_chan)``
    and optional float32 weights ``wts (n_row, n_chan)`` -> float32 ``(n_row, n_bin, n_chan,
    n_pol)``: ``((float)code - zero_off) * scl + offs``, times the weight (``out`` if given)."""
    for name, a, dtype in (('codes', codes, PSRFITS_CODE), ('scl', scl, np.float32), ('offs', offs, np.float32),
                           ('wts', wts, np.float32)):
        if a is None and name == 'wts':
            continue
        if not isinstance(a, DeviceArray):
            raise TypeError(f"psrfits_decode: {name} must be a DeviceArray, not {type(a).__name__}")
        if a.dtype != np.dtype(dtype):
            raise TypeError(f"psrfits_decode: {name} must be {np.dtype(dtype).str}, not {a.dtype.str}")
    if len(codes.shape) != 4 or min(codes.shape[1:]) < 1:
        raise ValueError(f"psrfits_decode: codes have shape (row, pol, chan, bin), not {codes.shape}")
    n_row, n_pol, n_chan, n_bin = codes.shape
    if scl.size != n_row * n_pol * n_chan or offs.size != scl.size:
        raise ValueError(f"psrfits_decode: scl and offs hold {scl.size} and {offs.size} values for "
                         f"{n_row * n_pol * n_chan} profiles")
    if wts is not None and wts.size != n_row * n_chan:
        raise ValueError(f"psrfits_decode: wts holds {wts.size} values for {n_row} rows of {n_chan} channels")
    zero_off = float(zero_off)
    if zero_off != zero_off:
        raise ValueError("psrfits_decode: zero_off is not a number")
    if out is None:
        out = DeviceArray((n_row, n_bin, n_chan, n_pol), np.float32)
    elif not isinstance(out, DeviceArray):
        raise TypeError(f"psrfits_decode: out must be a DeviceArray, not {type(out).__name__}")
    elif out.dtype != np.dtype(np.float32):
        raise TypeError(f"psrfits_decode: out must be float32, not {out.dtype}")
    elif out.size != codes.size:
        raise ValueError(f"psrfits_decode: out holds {out.size} values for {codes.size} codes")
    if n_row:
        check(lib().bbt_psrfits_decode(codes.ptr_to_read(), scl.ptr_to_read(), offs.ptr_to_read(),
                                       wts.ptr_to_read() if wts is not None else None, zero_off, out.ptr,
                                       n_row, n_bin, n_chan, n_pol, _stream))
    return out


#: widths of a search-mode code
PSRSEARCH_BITS = (1, 2, 4, 8)
#: columns (channels x polarizations) of a row from which bbt_psrsearch_encode adds a column's
#: samples in order (BBT_PSRSEARCH_MANY in csrc/psrsearch_geo.hpp)
PSRSEARCH_MANY_COLUMNS = 64


def _search_dims(nsblk, n_chan, n_pol, nbits, who):
    if isinstance(nbits, bool) or nbits not in PSRSEARCH_BITS:
        raise ValueError(f"{who}: nbits must be one of {PSRSEARCH_BITS}, not {nbits!r}")
    nsblk, n_chan, n_pol = int(nsblk), int(n_chan), int(n_pol)
    if min(nsblk, n_chan, n_pol) < 1:
        raise ValueError(f"{who}: an empty axis in (nsblk, nchan, npol) = {(nsblk, n_chan, n_pol)}")
    if n_pol > 32:
        raise ValueError(f"{who}: {n_pol} polarizations; at most 32 are coded")
    if n_chan * nbits % 8:
        raise ValueError(f"{who}: {n_chan} channels of {nbits} bits do not fill whole bytes "
                         "(nchan * nbits must be a multiple of 8)")
    return nsblk, n_chan, n_pol, int(nbits)


def psrsearch_encode(x, nsblk, nbits, nsigma):
    """Code float32 samples ``(n, n_chan[, n_pol])``, ``n`` a whole number of rows of ``nsblk``
    samples, in HBM as the rows of a PSRFITS search-mode table (bbt_psrsearch_encode in
    include/bbt_hip.h; `psrfits.encode_search_rows` is the NumPy restatement).  Returns
    `DeviceArray`s ``(codes, scl, offs, n_finite)``: uint8 ``(n_row, nsblk, n_pol, n_chan * nbits
    / 8)``, and float32, float32, int32 ``(n_row, n_pol, n_chan)``."""
    if not isinstance(x, DeviceArray):
        raise TypeError(f"psrsearch_encode: the input must be a DeviceArray, not {type(x).__name__}")
    if x.dtype != np.dtype(np.float32):
        raise TypeError(f"psrsearch_encode: the input must be float32, not {x.dtype}")
    if not 2 <= len(x.shape) <= 3:
        raise ValueError(f"psrsearch_encode: samples have shape (n, chan[, pol]), not {tuple(x.shape)}")
    n, n_chan, n_pol = tuple(x.shape) + (1,) * (3 - len(x.shape))
    nsblk, n_chan, n_pol, nbits = _search_dims(nsblk, n_chan, n_pol, nbits, 'psrsearch_encode')
    if n % nsblk:
        raise ValueError(f"psrsearch_encode: {n} samples are not a whole number of rows of {nsblk}")
    nsigma = float(nsigma)
    if not 0. < nsigma < np.inf:
        raise ValueError(f"psrsearch_encode: nsigma must be positive and finite, not {nsigma}")
    n_row = n // nsblk
    codes = DeviceArray((n_row, nsblk, n_pol, n_chan * nbits // 8), np.uint8)
    scl = DeviceArray((n_row, n_pol, n_chan), np.float32)
    offs = DeviceArray((n_row, n_pol, n_chan), np.float32)
    n_finite = DeviceArray((n_row, n_pol, n_chan), np.int32)
    if n_row:
        check(lib().bbt_psrsearch_encode(x.ptr_to_read(), codes.ptr, scl.ptr, offs.ptr, n_finite.ptr,
                                         n_row, nsblk, n_chan, n_pol, nbits, nsigma, _stream))
    return codes, scl, offs, n_finite


def psrsearch_decode(codes, scl, offs, wts, zero_off, nbits, dims, out=None):
    """Decode rows of a PSRFITS search-mode table in HBM (bbt_psrsearch_decode): uint8 ``codes``
    holding ``(n_row, nsblk, n_pol, n_chan * nbits / 8)`` bytes, float32 ``scl`` and ``offs (n_row,
    n_pol, n_chan)`` and float32 weights ``wts (n_row, n_chan)`` or None, with ``dims = (nsblk,
    n_chan, n_pol)`` -> float32 ``(n_row * nsblk, n_chan, n_pol)``: ``((float)code - zero_off) *
    scl + offs``, times the weight (``out`` if given)."""
    for name, a, dtype in (('codes', codes, np.uint8), ('scl', scl, np.float32), ('offs', offs, np.float32),
                           ('wts', wts, np.float32)):
        if a is None and name == 'wts':
            continue
        if not isinstance(a, DeviceArray):
            raise TypeError(f"psrsearch_decode: {name} must be a DeviceArray, not {type(a).__name__}")
        if a.dtype != np.dtype(dtype):
            raise TypeError(f"psrsearch_decode: {name} must be {np.dtype(dtype).str}, not {a.dtype.str}")
    if len(tuple(dims)) != 3:
        raise ValueError(f"psrsearch_decode: dims are (nsblk, nchan, npol), not {dims!r}")
    nsblk, n_chan, n_pol, nbits = _search_dims(*dims, nbits, 'psrsearch_decode')
    if offs.size != scl.size or scl.size % (n_chan * n_pol):
        raise ValueError(f"psrsearch_decode: scl and offs hold {scl.size} and {offs.size} values for rows of "
                         f"{n_chan} channels and {n_pol} polarizations")
    n_row = scl.size // (n_chan * n_pol)
    row_bytes = nsblk * n_pol * n_chan * nbits // 8
    if codes.size != n_row * row_bytes:
        raise ValueError(f"psrsearch_decode: codes hold {codes.size} bytes for {n_row} rows of {row_bytes}")
    if wts is not None and wts.size != n_row * n_chan:
        raise ValueError(f"psrsearch_decode: wts holds {wts.size} values for {n_row} rows of {n_chan} channels")
    zero_off = float(zero_off)
    if zero_off != zero_off:
        raise ValueError("psrsearch_decode: zero_off is not a number")
    if out is None:
        out = DeviceArray((n_row * nsblk, n_chan, n_pol), np.float32)
    elif not isinstance(out, DeviceArray):
        raise TypeError(f"psrsearch_decode: out must be a DeviceArray, not {type(out).__name__}")
    elif out.dtype != np.dtype(np.float32):
        raise TypeError(f"psrsearch_decode: out must be float32, not {out.dtype}")
    elif out.size != n_row * nsblk * n_chan * n_pol:
        raise ValueError(f"psrsearch_decode: out holds {out.size} values for {n_row * nsblk * n_chan * n_pol} codes")
    if n_row:
        check(lib().bbt_psrsearch_decode(codes.ptr_to_read(), scl.ptr_to_read(), offs.ptr_to_read(),
                                         wts.ptr_to_read() if wts is not None else None, zero_off, out.ptr,
                                         n_row, nsblk, n_chan, n_pol, nbits, _stream))
    return out


class _Plan:
    _destroy = None

    def __init__(self):
        self._h = C.c_void_p()

    def close(self):
        if getattr(self, '_h', None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def chirp(n, frequency_hz, sideband, reference_hz, rate_hz, d_dm, offset_s=0.):
    """(n_col, n) complex64 dispersion chirps made on the GPU in float64 (bbt_chirp): one
    column per entry of the equal-length 1-d arrays ``frequency_hz, sideband, reference_hz``."""
    f = np.ascontiguousarray(frequency_hz, dtype=np.float64).ravel()
    sb = np.ascontiguousarray(sideband, dtype=np.float64).ravel()
    fr = np.ascontiguousarray(reference_hz, dtype=np.float64).ravel()
    assert f.shape == sb.shape == fr.shape
    out = DeviceArray((f.shape[0], int(n)), np.complex64)
    pd = C.POINTER(C.c_double)
    check(lib().bbt_chirp(out.ptr, int(n), f.shape[0], f.ctypes.data_as(pd), sb.ctypes.data_as(pd),
                          fr.ctypes.data_as(pd), float(rate_hz), float(d_dm), float(offset_s), _stream))
    return out


class OsmPlan(_Plan):
    """ifft(fft(block) * response)[valid] for overlap-save blocks."""
    _destroy = 'bbt_osm_plan_destroy'

    def __init__(self, n_fft, n_stream, response, response_index=None):
        super().__init__()
        self.n_fft, self.n_stream = int(n_fft), int(n_stream)
        if isinstance(response, DeviceArray):
            resp_ptr, on_dev, n_resp = response.ptr, 1, response.shape[0]
            assert response.dtype == np.complex64 and response.shape[1] == n_fft
        else:
            response = np.ascontiguousarray(response, dtype=np.complex64)
            assert response.ndim == 2 and response.shape[1] == n_fft
            resp_ptr, on_dev, n_resp = response.ctypes.data, 0, response.shape[0]
        idx = None
        if response_index is not None:
            idx_arr = np.ascontiguousarray(response_index, dtype=np.int32)
            assert idx_arr.shape == (n_stream,)
            idx = idx_arr.ctypes.data_as(_pi32)
        check(lib().bbt_osm_plan_create(C.byref(self._h), self.n_fft, self.n_stream, n_resp,
                                        resp_ptr, on_dev, idx))

    def info(self):
        ws, chunk, n1, n2 = _i64(), _int(), _int(), _int()
        check(lib().bbt_osm_plan_info(self._h, C.byref(ws), C.byref(chunk), C.byref(n1),
                                      C.byref(n2)))
        return dict(workspace_bytes=ws.value, chunk_blocks=chunk.value, n1=n1.value, n2=n2.value)

    def set_layout(self, in_plane=0, out_plane=0):
        """Pair-planar hand-over between two plans (see bbt_osm_plan_set_layout); 0, 0: interleaved."""
        check(lib().bbt_osm_plan_set_layout(self._h, int(in_plane), int(out_plane)))

    def fusable(self, n_chan):
        """Can `execute_channelized` take Channelize(n_chan) into the row pass?"""
        return bool(lib().bbt_osm_plan_fusable(self._h, int(n_chan)))

    def _call(self, fn, in_dev, out_dev, *args):
        """One execute entry point of the C ABI on (in_dev, out_dev).  When this package owns the
        output's allocation the call is issued with a deferred join (plans with lanes leave the
        lanes running; one-kernel plans run on a stream of their own beside the caller's)
        (`DEFER_JOIN`): its completion event is left with the output's allocation."""
        owner = out_dev.owner
        defer = DEFER_JOIN and owner.__class__ is _Allocation
        # the input is read: after the calls that still write it; the output is written: after
        # every call still owed to its allocation -- unless the caller vouches for the region
        src = in_dev.ptr_to_read()
        dst = out_dev._ptr if (defer and out_dev.fresh) else out_dev.ptr
        if not defer:
            check(fn(self._h, src, dst, *args, _stream))
            return
        ev = _events.take()
        check(lib().bbt_osm_plan_defer(self._h, ev))
        try:
            check(fn(self._h, src, dst, *args, _stream))
        except Exception:
            lib().bbt_osm_plan_defer(self._h, None)         # (if the call never took it)
            check(lib().bbt_event_record(ev, _stream))
            _events.give(ev)
            raise
        # The call's end is owed to the output (it is being written) and to the input (it is being
        # read: whoever overwrites it next -- the upstream task filling its cache again -- or frees
        # it must come after the lanes).  The input of a foreign owner (a torch tensor) is the
        # caller's to keep untouched, as include/bbt_hip.h says.
        src_owner = in_dev.owner
        shared = src_owner.__class__ is _Allocation and src_owner is not owner
        foreign = src_owner is not None and src_owner.__class__ is not _Allocation
        done = _Done(ev, 2 if (shared or foreign) else 1)
        owner.owe(_Pending(done, (src_owner, self)), write=True)
        if shared:
            src_owner.owe(_Pending(done, (self,)), write=False)
        elif foreign and not _owe_foreign_read(src_owner, _Pending(done, (self,))):
            done.release()              # (an owner that cannot be weakly referenced: not tracked)
        out_dev.fresh = False           # (from now on the region IS owed a call)

    @staticmethod
    def _descriptors(in_off, out_off, valid_start, valid_count):
        in_off = np.ascontiguousarray(in_off, dtype=np.int64)
        out_off = np.ascontiguousarray(out_off, dtype=np.int64)
        valid_start = np.ascontiguousarray(valid_start, dtype=np.int32)
        valid_count = np.ascontiguousarray(valid_count, dtype=np.int32)
        n = in_off.shape[0]
        assert out_off.shape == valid_start.shape == valid_count.shape == (n,)
        return (n, in_off.ctypes.data_as(_pi64), out_off.ctypes.data_as(_pi64),
                valid_start.ctypes.data_as(_pi32), valid_count.ctypes.data_as(_pi32)), \
            (in_off, out_off, valid_start, valid_count)

    def execute(self, in_dev, out_dev, in_off, out_off, valid_start, valid_count):
        desc, _alive = self._descriptors(in_off, out_off, valid_start, valid_count)
        self._call(lib().bbt_osm_execute, in_dev, out_dev, *desc)

    def execute_flat(self, in_dev, out_dev, in_off, out_elem_off, valid_start, first_elem, valid_elems):
        """`execute` with the kept range in elements of the (row, stream) matrix (plans of one
        kernel: power-of-two n_fft <= 4096): see bbt_osm_execute_flat."""
        (n, io, oo, vs, ve), _alive = self._descriptors(in_off, out_elem_off, valid_start, valid_elems)
        self._call(lib().bbt_osm_execute_flat, in_dev, out_dev, n, io, oo, vs, int(first_elem), ve)

    def execute_channelized(self, in_dev, out_dev, in_off, out_off, valid_start, valid_count,
                            n_chan, first_spectrum, n_spectra):
        """Fused Channelize: spectra [first_spectrum, +n_spectra) of the stream
        the blocks would produce (``out_off`` absolute in that stream)."""
        desc, _alive = self._descriptors(in_off, out_off, valid_start, valid_count)
        self._call(lib().bbt_osm_execute_channelized, in_dev, out_dev, *desc, int(n_chan),
                   int(first_spectrum), int(n_spectra))

    def detect_bins_max(self, n_chan, step):
        """Integration bins one workgroup of the last pass would touch (<= 64
        for the fused detection)."""
        return int(lib().bbt_osm_detect_bins_max(self._h, int(n_chan), int(step)))

    def execute_channelized_detect(self, in_dev, out_dev, in_off, out_off, valid_start, valid_count,
                                   n_chan, first_spectrum, n_bins, step, mode, average=True):
        """Fused Channelize + Square/Power + Integrate(step): float32 bins."""
        desc, _alive = self._descriptors(in_off, out_off, valid_start, valid_count)
        self._call(lib().bbt_osm_execute_channelized_detect, in_dev, out_dev, *desc, int(n_chan),
                   int(first_spectrum), int(n_bins), int(step), int(mode), int(bool(average)))

    def execute_regular(self, in_dev, out_dev, n_blocks, in_off0, out_off0, hop, valid_start):
        self._call(lib().bbt_osm_execute_regular, in_dev, out_dev, int(n_blocks), int(in_off0),
                   int(out_off0), int(hop), int(valid_start))

    def timing_enable(self, enable=True):
        """False/0 off, True/1 time the normal (two-lane) schedule, 2 isolated
        passes on a single lane."""
        check(lib().bbt_osm_timing_enable(self._h, int(enable)))

    def timing_read(self):
        ms = (C.c_double * 3)()
        n = _i64()
        check(lib().bbt_osm_timing_read(self._h, ms, C.byref(n)))
        return list(ms), n.value

    def timing_read_passes(self):
        """Per pass: accumulated ms, timed launches, overlap-save blocks those launches covered."""
        ms = (C.c_double * 3)()
        launches, blocks = (_i64 * 3)(), (_i64 * 3)()
        check(lib().bbt_osm_timing_read_passes(self._h, ms, launches, blocks))
        return list(ms), list(launches), list(blocks)


class ChanPlan(_Plan):
    """FFT over groups of n_chan complete samples."""
    _destroy = 'bbt_chan_plan_destroy'

    def __init__(self, n_chan, n_stream, direction=-1):
        super().__init__()
        self.n_chan, self.n_stream = int(n_chan), int(n_stream)
        check(lib().bbt_chan_plan_create(C.byref(self._h), self.n_chan, self.n_stream,
                                         int(direction)))

    def execute(self, in_dev, out_dev, n_spectra):
        check(lib().bbt_chan_execute(self._h, in_dev.ptr_to_read(), out_dev.ptr, int(n_spectra), _stream))


class R2CPlan(_Plan):
    """Real2Complex of frames of 2 n_out float32 samples of n_stream streams into n_out complex64
    samples each (bbt_r2c_*)."""
    _destroy = 'bbt_r2c_plan_destroy'

    def __init__(self, n_out, n_stream, multi_level=False):
        """multi_level: the three-step route for any length (BBT_R2C_MULTI_LEVEL)."""
        super().__init__()
        self.n_out, self.n_stream = int(n_out), int(n_stream)
        check(lib().bbt_r2c_plan_create_ex(C.byref(self._h), self.n_out, self.n_stream, 1 if multi_level else 0))

    def info(self):
        one, ws = _int(), _i64()
        check(lib().bbt_r2c_plan_info(self._h, C.byref(one), C.byref(ws)))
        return dict(one_pass=bool(one.value), workspace_bytes=ws.value)

    def execute(self, in_dev, out_dev, n_frames):
        """in_dev: (n_frames * 2 n_out, n_stream) float32 -> out_dev: (n_frames * n_out, n_stream) complex64."""
        check(lib().bbt_r2c_execute(self._h, in_dev.ptr_to_read(), out_dev.ptr, int(n_frames), _stream))


class GatherPlan(_Plan):
    """An index map over the elements of a sample (bbt_gather_*): element j of an output sample is
    element ``map_elem[j]`` of the sample at the same time offset of source ``map_src[j]``."""
    _destroy = 'bbt_gather_plan_destroy'
    ROUTES = {'auto': 0, 'run_copy': 1, 'tile': 2, 'direct': 3}

    def __init__(self, src_row_elems, map_src, map_elem, elem_bytes, route='auto'):
        super().__init__()
        rows = np.ascontiguousarray(src_row_elems, dtype=np.int64).ravel()
        self.map_src = np.ascontiguousarray(map_src, dtype=np.int32).ravel()
        self.map_elem = np.ascontiguousarray(map_elem, dtype=np.int64).ravel()
        if self.map_src.shape != self.map_elem.shape:
            raise ValueError("map_src and map_elem must have the same length")
        self.n_src, self.elem_bytes = len(rows), int(elem_bytes)
        self.src_row_elems, self.out_row_elems = rows, len(self.map_src)
        check(lib().bbt_gather_plan_create_ex(
            C.byref(self._h), self.n_src, rows.ctypes.data_as(_pi64), self.out_row_elems,
            self.map_src.ctypes.data_as(C.POINTER(C.c_int32)), self.map_elem.ctypes.data_as(_pi64),
            self.elem_bytes, self.ROUTES[route]))

    def info(self):
        route, runs, tile, lds = _int(), _i64(), _int(), _int()
        check(lib().bbt_gather_plan_info(self._h, C.byref(route), C.byref(runs), C.byref(tile), C.byref(lds)))
        names = {v: k for k, v in self.ROUTES.items()}
        return dict(route=names[route.value], n_runs=runs.value, tile_samples=tile.value, lds_bytes=lds.value)

    def execute(self, sources, out_dev, n_samples, first_samples=None):
        """sources: one DeviceArray per source (None for a source the map does not use), source k
        holding rows of ``src_row_elems[k]`` elements from sample ``first_samples[k]`` (default 0)
        on; out_dev: ``n_samples`` rows of ``out_row_elems`` elements."""
        if len(sources) != self.n_src:
            raise ValueError(f"the plan has {self.n_src} sources; got {len(sources)}")
        ptrs = (_vp * self.n_src)(*[None if s is None else s.ptr_to_read() for s in sources])
        first = np.zeros(self.n_src, np.int64) if first_samples is None else \
            np.ascontiguousarray(first_samples, dtype=np.int64)
        check(lib().bbt_gather_execute(self._h, ptrs, first.ctypes.data_as(_pi64), out_dev.ptr,
                                       int(n_samples), _stream))


class PfbPlan(_Plan):
    """n_tap FIR across blocks followed by the channelizer FFT."""
    _destroy = 'bbt_pfb_plan_destroy'

    def __init__(self, taps, n_stream):
        super().__init__()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.n_tap, self.n_chan = taps.shape
        self.n_stream = int(n_stream)
        check(lib().bbt_pfb_plan_create(C.byref(self._h), self.n_tap, self.n_chan, self.n_stream,
                                        taps.ctypes.data_as(C.POINTER(C.c_float))))

    def execute(self, in_dev, out_dev, n_spectra):
        check(lib().bbt_pfb_execute(self._h, in_dev.ptr_to_read(), out_dev.ptr, int(n_spectra), _stream))


class FirPlan(_Plan):
    """Time-domain convolution with a short response ``(n_tap, n_stream)``:
    out[i] = sum_k response[k] * in[i + n_tap - 1 - k] (what Convolve keeps)."""
    _destroy = 'bbt_fir_plan_destroy'

    def __init__(self, response):
        super().__init__()
        response = np.ascontiguousarray(response, dtype=np.complex64)
        assert response.ndim == 2
        self.n_tap, self.n_stream = response.shape
        check(lib().bbt_fir_plan_create(C.byref(self._h), self.n_tap, self.n_stream,
                                        response.ctypes.data_as(C.c_void_p)))

    def execute(self, in_dev, out_dev, n_out):
        check(lib().bbt_fir_execute(self._h, in_dev.ptr_to_read(), out_dev.ptr, int(n_out), _stream))


class ShiftPlan(_Plan):
    """out[i, e] = in[i + offsets[e], e] (per-element integer sample shifts)."""
    _destroy = 'bbt_shift_plan_destroy'

    def __init__(self, offsets, elem_bytes):
        super().__init__()
        offsets = np.ascontiguousarray(offsets, dtype=np.int32).ravel()
        check(lib().bbt_shift_plan_create(C.byref(self._h), offsets.shape[0], int(elem_bytes),
                                          offsets.ctypes.data_as(_pi32)))

    def execute(self, in_dev, out_dev, n_out):
        check(lib().bbt_shift_execute(self._h, in_dev.ptr_to_read(), out_dev.ptr, int(n_out), _stream))


#: bounds of the trial-DM plan (csrc/dmt_geo.hpp)
DMT_MAX_NCHAN, DMT_MAX_NDM, DMT_MAX_REST, DMT_MAX_SPAN = 16384, 4096, 64, 1 << 24


class DmtPlan(_Plan):
    """out[i, d, r] = sum over c, ascending, of in[i + offsets[d, c], c, r]: incoherent dedispersion
    over ``ndm`` trial DMs, one float32 accumulator per output element (bbt_dmt_* in
    include/bbt_hip.h; `search.dm_trials_samples` is the NumPy restatement).  ``offsets``: int
    ``(ndm, nchan)``, all >= 0; the plan's ``span`` is the largest."""
    _destroy = 'bbt_dmt_plan_destroy'

    def __init__(self, offsets, n_rest=1):
        super().__init__()
        offsets = np.asarray(offsets)
        if offsets.ndim != 2 or offsets.dtype.kind not in 'iu':
            raise ValueError("DmtPlan: offsets must be an integer array (ndm, nchan)")
        if offsets.size and (offsets.min() < -(1 << 31) or offsets.max() >= (1 << 31)):
            raise ValueError("DmtPlan: offsets must fit 32 bits")
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        self.ndm, self.nchan = offsets.shape
        self.n_rest = int(n_rest)
        check(lib().bbt_dmt_plan_create(C.byref(self._h), offsets.ctypes.data_as(_pi32), self.ndm, self.nchan,
                                        self.n_rest))
        self.span = self.info()['span']

    def info(self):
        """span of the table, the tiling the next call will use (BBT_DMT_TILE, BBT_DMT_TRIALS) and
        the bytes of scratch the plan holds."""
        span, scratch, tile, trials = _i64(0), _i64(0), _int(0), _int(0)
        check(lib().bbt_dmt_plan_info(self._h, C.byref(span), C.byref(tile), C.byref(trials), C.byref(scratch)))
        return dict(span=span.value, tile=tile.value, trials=trials.value, scratch_bytes=scratch.value)

    def execute(self, in_dev, n_in, out_dev, n_out):
        """``in_dev``: float32, at least ``n_in * nchan * n_rest`` values; ``out_dev``: float32, at
        least ``n_out * ndm * n_rest``; ``n_in >= n_out + span``."""
        n_in, n_out = int(n_in), int(n_out)
        row_in, row_out = self.nchan * self.n_rest, self.ndm * self.n_rest
        if (in_dev.dtype != np.float32 or out_dev.dtype != np.float32 or n_in < 0 or n_out < 0
                or in_dev.size < n_in * row_in or out_dev.size < n_out * row_out):
            raise ValueError("DmtPlan.execute: float32 DeviceArrays of n_in * nchan * n_rest and "
                             "n_out * ndm * n_rest values are needed")
        check(lib().bbt_dmt_execute(self._h, in_dev.ptr_to_read(), n_in, out_dev.ptr, n_out, _stream))


#: bounds of the single-pulse search (csrc/sps_geo.hpp)
SPS_MAX_N, SPS_MAX_WIDTHS = 65536, 13


def sps_info(plan=None):
    """The tiling the next call will use (BBT_SPS_WIDTH, BBT_SPS_FUSE, BBT_SPS_SPLIT, BBT_SPS_STD_ROWS),
    the library's 13 scales c_k and, for a plan, the bytes of scratch it holds."""
    width, fuse, split, rows, scratch = _int(0), _int(0), _int(0), _int(0), _i64(0)
    scales = (C.c_float * SPS_MAX_WIDTHS)()
    check(lib().bbt_sps_plan_info(plan._h if plan is not None else None, C.byref(width), C.byref(fuse),
                                  C.byref(split), C.byref(rows), C.byref(scratch), scales))
    return dict(width=width.value, fuse=fuse.value, split=split.value, std_rows=rows.value,
                scratch_bytes=scratch.value, scales=np.array(scales[:], dtype=np.float32))


def sps_standardize(x, n, n_elem, out=None):
    """Every whole block of ``n`` samples of float32 ``x`` (samples of ``n_elem`` elements) brought to
    zero mean and unit variance per element (bbt_sps_standardize in include/bbt_hip.h;
    `search.standardize_samples` is the NumPy restatement).  Returns ``out``, float32 of ``(x.size //
    n_elem // n) * n * n_elem`` values."""
    n, n_elem = int(n), int(n_elem)
    if x.dtype != np.float32:
        raise TypeError(f"sps_standardize: x must be float32, not {x.dtype}")
    if n_elem < 1 or x.size % n_elem:
        raise ValueError(f"sps_standardize: {x.size} values are not samples of {n_elem} elements")
    if not 2 <= n <= SPS_MAX_N:
        raise ValueError(f"sps_standardize: n must be 2 ... {SPS_MAX_N}, not {n}")
    n_block = x.size // n_elem // n
    if out is None:
        out = DeviceArray((n_block * n, n_elem), np.float32)
    elif out.dtype != np.float32 or out.size != n_block * n * n_elem:
        raise ValueError(f"sps_standardize: out must be a float32 DeviceArray of {n_block * n * n_elem} values")
    check(lib().bbt_sps_standardize(x.ptr_to_read(), out.ptr, n_block, n, n_elem, _stream))
    return out


class SpsPlan(_Plan):
    """best[b, :, e] = (snr, offset, level) of the best boxcar of widths 1, 2, ... 2^(n_widths - 1) that
    starts in block ``b`` of ``n`` samples (bbt_sps_* in include/bbt_hip.h; `search.boxcar_search_samples`
    is the NumPy restatement).  The plan owns the scratch of the partial sums."""
    _destroy = 'bbt_sps_plan_destroy'

    def __init__(self, n, n_widths, n_elem=1):
        super().__init__()
        self.n, self.n_widths, self.n_elem = int(n), int(n_widths), int(n_elem)
        check(lib().bbt_sps_plan_create(C.byref(self._h), self.n, self.n_widths, self.n_elem))

    def info(self):
        """The tiling the next call will use and the bytes of scratch the plan holds (`sps_info`)."""
        return sps_info(self)

    def execute(self, in_dev, n_in, out_dev, n_blocks):
        """``in_dev``: float32, at least ``n_in * n_elem`` values, ``n_in >= n_blocks * n``; ``out_dev``:
        float32, at least ``n_blocks * 3 * n_elem``."""
        n_in, n_blocks = int(n_in), int(n_blocks)
        if (in_dev.dtype != np.float32 or out_dev.dtype != np.float32 or n_in < 0 or n_blocks < 0
                or in_dev.size < n_in * self.n_elem or out_dev.size < n_blocks * 3 * self.n_elem):
            raise ValueError("SpsPlan.execute: float32 DeviceArrays of n_in * n_elem and n_blocks * 3 * n_elem "
                             "values are needed")
        check(lib().bbt_sps_execute(self._h, in_dev.ptr_to_read(), n_in, out_dev.ptr, n_blocks, _stream))


#: bounds of the fast-folding search (csrc/ffa_geo.hpp)
FFA_MIN_P, FFA_MAX_P, FFA_MAX_ROWS, FFA_MAX_WIDTHS, FFA_MAX_LANE = 4, 1025, 65536, 10, 1 << 30


def ffa_info(plan=None, period=0):
    """The tiling the next call will use (BBT_FFA_FUSE, BBT_FFA_WIDTH) and, for a plan, the bytes of scratch it
    holds and the floats of scratch it needs per column; for a base period of the plan also its rows of data
    ``m``, its rows ``M`` and the library's 10 scales a_k (0 beyond ``n_widths``)."""
    fuse, width, rows, padded, scratch, column = _int(0), _int(0), _i64(0), _i64(0), _i64(0), _i64(0)
    scales = (C.c_float * FFA_MAX_WIDTHS)()
    check(lib().bbt_ffa_plan_info(plan._h if plan is not None else None, int(period), C.byref(fuse), C.byref(width),
                                  C.byref(rows), C.byref(padded), C.byref(scratch), C.byref(column), scales))
    return dict(fuse=fuse.value, width=width.value, m=rows.value, M=padded.value, scratch_bytes=scratch.value,
                column_floats=column.value, scales=np.array(scales[:], dtype=np.float32))


class FfaPlan(_Plan):
    """best[p - p_lo, :, e] = (snr, shift, level, phase) of the best boxcar over every fold of a block of ``n``
    samples at the base period ``p`` (bbt_ffa_* in include/bbt_hip.h; `ffa.ffa_search_samples` is the NumPy
    restatement).  The plan owns the scratch of the fold stages."""
    _destroy = 'bbt_ffa_plan_destroy'

    def __init__(self, n, periods, n_widths, n_elem=1):
        super().__init__()
        self.n, self.n_widths, self.n_elem = int(n), int(n_widths), int(n_elem)
        self.p_lo, self.p_hi = (int(p) for p in periods)
        check(lib().bbt_ffa_plan_create(C.byref(self._h), self.n, self.p_lo, self.p_hi, self.n_widths, self.n_elem))

    def info(self, period=0):
        """The tiling the next call will use, the scratch, and the rows and scales of a base period (`ffa_info`)."""
        return ffa_info(self, period)

    def execute(self, in_dev, out_dev, e0=0, ne=None, pa=None, pb=None):
        """``in_dev``: float32, one block of ``n * n_elem`` values at least; ``out_dev``: float32, ``(p_hi - p_lo) * 4
        * n_elem``.  Only the columns ``e0 ... e0 + ne`` and the base periods ``pa ... pb`` are searched and
        written (default: all)."""
        e0 = int(e0)
        ne = self.n_elem - e0 if ne is None else int(ne)
        pa = self.p_lo if pa is None else int(pa)
        pb = self.p_hi if pb is None else int(pb)
        if (in_dev.dtype != np.float32 or out_dev.dtype != np.float32 or in_dev.size < self.n * self.n_elem
                or out_dev.size < (self.p_hi - self.p_lo) * 4 * self.n_elem):
            raise ValueError("FfaPlan.execute: float32 DeviceArrays of n * n_elem and (p_hi - p_lo) * 4 * n_elem "
                             "values are needed")
        check(lib().bbt_ffa_execute(self._h, in_dev.ptr_to_read(), out_dev.ptr, e0, ne, pa, pb, _stream))


#: bounds of the periodicity search (csrc/hsum_geo.hpp)
HSUM_MIN_M, HSUM_MAX_M, HSUM_MAX_N, HSUM_MAX_LEVELS, HSUM_MAX_NBIN = 2, 65536, 65536, 6, 1 << 24


def hsum_info(plan=None):
    """The tiling the next call will use (BBT_HSUM_WIDTH, BBT_HSUM_SPLIT, BBT_HSUM_ROWS) and, for a
    plan, the 6 scales c_L it holds (0 beyond its levels)."""
    width, split, rows = _int(0), _int(0), _int(0)
    scales = (C.c_float * HSUM_MAX_LEVELS)()
    check(lib().bbt_hsum_plan_info(plan._h if plan is not None else None, C.byref(width), C.byref(split),
                                   C.byref(rows), scales))
    return dict(width=width.value, split=split.value, rows=rows.value,
                scales=np.array(scales[:], dtype=np.float32))


def hsum_whiten(x, nbin, n_elem, m, skip=1, out=None):
    """Every block of ``m`` bins, counted from bin ``skip``, of every spectrum of float32 ``x`` (spectra of
    ``nbin`` bins of ``n_elem`` elements) divided by its own mean, the bins below ``skip`` +0
    (bbt_hsum_whiten in include/bbt_hip.h; `periodicity.whiten_samples` is the NumPy restatement).
    Returns ``out``, float32 of the size of ``x``."""
    nbin, n_elem, m, skip = int(nbin), int(n_elem), int(m), int(skip)
    if x.dtype != np.float32:
        raise TypeError(f"hsum_whiten: x must be float32, not {x.dtype}")
    if n_elem < 1 or nbin < 1 or x.size % (nbin * n_elem) or x.size == 0:
        raise ValueError(f"hsum_whiten: {x.size} values are not spectra of {nbin} bins of {n_elem} elements")
    if not HSUM_MIN_M <= m <= HSUM_MAX_M:
        raise ValueError(f"hsum_whiten: m must be {HSUM_MIN_M} ... {HSUM_MAX_M}, not {m}")
    if not 0 <= skip < nbin:
        raise ValueError(f"hsum_whiten: skip must be 0 ... {nbin - 1}, not {skip}")
    n_spec = x.size // (nbin * n_elem)
    if out is None:
        out = DeviceArray((n_spec, nbin, n_elem), np.float32)
    elif out.dtype != np.float32 or out.size != x.size:
        raise ValueError(f"hsum_whiten: out must be a float32 DeviceArray of {x.size} values")
    check(lib().bbt_hsum_whiten(x.ptr_to_read(), out.ptr, n_spec, nbin, n_elem, m, skip, _stream))
    return out


class HsumPlan(_Plan):
    """best[s, b, :, e] = (snr, offset, level) of the best sum of 1, 2, ... 2^(n_levels - 1) harmonics whose
    top harmonic lies in block ``b`` of ``n`` bins of spectrum ``s`` (bbt_hsum_* in include/bbt_hip.h;
    `periodicity.harmonic_search_samples` is the NumPy restatement).  ``scales``: the ``n_levels`` float32
    ``c_L`` the S/N is formed with."""
    _destroy = 'bbt_hsum_plan_destroy'

    def __init__(self, nbin, n, n_levels, lo, n_elem, scales):
        super().__init__()
        self.nbin, self.n, self.n_levels, self.lo, self.n_elem = int(nbin), int(n), int(n_levels), int(lo), int(n_elem)
        scales = np.ascontiguousarray(scales, dtype=np.float32).ravel()
        if scales.shape[0] < min(max(self.n_levels, 0), HSUM_MAX_LEVELS):
            raise ValueError(f"HsumPlan: {self.n_levels} levels need as many scales, not {scales.shape[0]}")
        self.n_blocks = -(-self.nbin // self.n) if self.n > 0 else 0
        check(lib().bbt_hsum_plan_create(C.byref(self._h), self.nbin, self.n, self.n_levels, self.lo, self.n_elem,
                                         scales.ctypes.data_as(C.POINTER(C.c_float))))

    def info(self):
        """The tiling the next call will use and the plan's scales (`hsum_info`)."""
        return hsum_info(self)

    def execute(self, in_dev, n_spec, out_dev):
        """``in_dev``: float32, at least ``n_spec * nbin * n_elem`` values; ``out_dev``: float32, at least
        ``n_spec * n_blocks * 3 * n_elem``."""
        n_spec = int(n_spec)
        if (in_dev.dtype != np.float32 or out_dev.dtype != np.float32 or n_spec < 0
                or in_dev.size < n_spec * self.nbin * self.n_elem
                or out_dev.size < n_spec * self.n_blocks * 3 * self.n_elem):
            raise ValueError("HsumPlan.execute: float32 DeviceArrays of n_spec * nbin * n_elem and n_spec * "
                             "n_blocks * 3 * n_elem values are needed")
        check(lib().bbt_hsum_execute(self._h, in_dev.ptr_to_read(), n_spec, out_dev.ptr, _stream))


#: bounds of the long fluctuation spectra (csrc/lspec_geo.hpp)
LSPEC_MIN_LOG2, LSPEC_MAX_LOG2, LSPEC_MAX_STACK, LSPEC_BUDGET = 15, 22, 1 << 20, 1 << 29
LSPEC_LDS_CELLS, LSPEC_MAX_COLS, LSPEC_MAX_PAIRS = 8192, 32, 16


class LongSpectraPlan(_Plan):
    """out[m, k, e] = the mean over ``stack`` consecutive transforms of ``|sum_t in[(m stack + q) n + t, e]
    exp(-2 pi i k t / n)|^2``, ``k <= n / 2``, for ``n`` a power of two from 2^15 to 2^22 (bbt_lspec_* in
    include/bbt_hip.h; `periodicity.long_spectra_samples` is the NumPy yardstick)."""
    _destroy = 'bbt_lspec_plan_destroy'

    def __init__(self, n, stack, n_elem):
        super().__init__()
        self.n, self.stack, self.n_elem = int(n), int(stack), int(n_elem)
        self.nbin = self.n // 2 + 1
        check(lib().bbt_lspec_plan_create(C.byref(self._h), self.n, self.stack, self.n_elem))

    def info(self, budget=0):
        """The split ``n1 x n2``, the columns of a first-pass and the column pairs of a last-pass
        workgroup, its threads (BBT_LSPEC_THREADS), and what a call under ``budget`` bytes of scratch (0: the default, 512 MiB) takes: the
        pairs of a launch and the scratch bytes."""
        n1, n2, cols, pairs, threads = _int(0), _int(0), _int(0), _int(0), _int(0)
        per, scratch = C.c_int64(0), C.c_int64(0)
        check(lib().bbt_lspec_plan_info(self._h, int(budget), C.byref(n1), C.byref(n2), C.byref(cols), C.byref(pairs),
                                        C.byref(threads), C.byref(per), C.byref(scratch)))
        return dict(n1=n1.value, n2=n2.value, cols=cols.value, pairs=pairs.value, threads=threads.value,
                    pairs_per_launch=per.value,
                    scratch_bytes=scratch.value)

    def execute(self, in_dev, n_spec, out_dev, budget=0):
        """``in_dev``: float32, at least ``n_spec * stack * n * n_elem`` values; ``out_dev``: float32, at least
        ``n_spec * (n // 2 + 1) * n_elem``.  ``budget``: bytes of scratch a launch may use (0: the default)."""
        n_spec = int(n_spec)
        if in_dev.dtype != np.float32 or out_dev.dtype != np.float32:
            raise TypeError("LongSpectraPlan.execute: float32 DeviceArrays are needed")
        if (n_spec < 1 or in_dev.size < n_spec * self.stack * self.n * self.n_elem
                or out_dev.size < n_spec * self.nbin * self.n_elem):
            raise ValueError("LongSpectraPlan.execute: float32 DeviceArrays of n_spec * stack * n * n_elem and "
                             "n_spec * (n // 2 + 1) * n_elem values are needed, n_spec >= 1")
        check(lib().bbt_lspec_execute(self._h, in_dev.ptr_to_read(), in_dev.size // self.n_elem, out_dev.ptr, n_spec,
                                      int(budget), _stream))


#: bounds of the acceleration trials (csrc/accel_geo.hpp)
ACCEL_MIN_N, ACCEL_MAX_N, ACCEL_MAX_TRIALS, ACCEL_BUDGET = 2, 1 << 24, 4096, 1 << 29
ACCEL_LDS_BYTES, ACCEL_TILE_UNITS, ACCEL_MAX_ROWS, ACCEL_MAX_WIDTH = 32768, 16384, 256, 1 << 28


class AccelPlan(_Plan):
    """out[q n + i, j, e] = in[q n + i + rint(k_j * float64(i * (i - n))), e]: every block of ``n`` rows of a
    float32 stream resampled along a parabola for each of the float64 ``factors`` k_j, ``|k_j| n <= 1/4``, the
    32 bits copied (bbt_accel_* in include/bbt_hip.h; `periodicity.accelerate_samples` is the NumPy twin)."""
    _destroy = 'bbt_accel_plan_destroy'

    def __init__(self, n, n_elem, factors):
        super().__init__()
        self.n, self.n_elem = int(n), int(n_elem)
        factors = np.ascontiguousarray(factors, dtype=np.float64)
        if factors.ndim != 1:
            raise ValueError("AccelPlan: factors must be a 1-D sequence of float64")
        self.factors = factors
        self.n_acc = factors.shape[0]
        check(lib().bbt_accel_plan_create(C.byref(self._h), self.n, self.n_elem,
                                          factors.ctypes.data_as(C.POINTER(C.c_double)), self.n_acc))

    def info(self, out_first=0, n_out=1):
        """For output rows ``[out_first, out_first + n_out)``: the route a launch takes now (BBT_ACCEL_ROUTE;
        1: the window wherever it fits, 2: direct), the rows of a tile, the LDS bytes the window kernel
        declares, the input rows the run needs and whether they would fit that LDS as one tile."""
        route, rows, fits = _int(0), _int(0), _int(0)
        lds, first, count = _i64(0), _i64(0), _i64(0)
        check(lib().bbt_accel_plan_info(self._h, int(out_first), int(n_out), C.byref(route), C.byref(rows),
                                        C.byref(lds), C.byref(first), C.byref(count), C.byref(fits)))
        return dict(route=route.value, rows=rows.value, lds_bytes=lds.value, window_first=first.value,
                    window_rows=count.value, fits=bool(fits.value))

    def execute(self, in_dev, in_first, n_in, out_dev, out_first, n_out, n_rows=None):
        """``in_dev``: float32, at least ``n_in * n_elem`` values, global rows ``[in_first, in_first + n_in)`` of
        the stream; ``out_dev``: float32, at least ``n_out * n_acc * n_elem``, for global rows ``[out_first,
        out_first + n_out)``.  ``n_rows``: the length of the stream, if known: rows beyond its last whole block
        are refused."""
        in_first, n_in, out_first, n_out = int(in_first), int(n_in), int(out_first), int(n_out)
        if in_dev.dtype != np.float32 or out_dev.dtype != np.float32:
            raise TypeError("AccelPlan.execute: float32 DeviceArrays are needed")
        if (n_in < 1 or n_out < 1 or in_first < 0 or out_first < 0 or in_dev.size < n_in * self.n_elem
                or out_dev.size < n_out * self.n_acc * self.n_elem):
            raise ValueError("AccelPlan.execute: float32 DeviceArrays of n_in * n_elem and n_out * n_acc * n_elem "
                             "values are needed, n_in >= 1, n_out >= 1")
        if n_rows is not None and out_first + n_out > int(n_rows) // self.n * self.n:
            raise ValueError(f"AccelPlan.execute: rows {out_first} ... {out_first + n_out - 1} run beyond the last "
                             f"whole block of {self.n} of a stream of {n_rows}")
        check(lib().bbt_accel_execute(self._h, in_dev.ptr_to_read(), in_first, n_in, out_dev.ptr, out_first, n_out,
                                      _stream))


#: bounds of the block median / MAD (csrc/rank_geo.hpp)
RANK_MIN_N, RANK_MAX_N, RANK_LDS_BYTES, RANK_MISC_BYTES = 2, 65536, 73728, 1024
RANK_MAD_SCALE = 1.482602218505602
RANK_ROUTES = {1: 'lds', 2: 'global'}


def rank_info(n_spec=1, nbin=2, n_elem=1, m=2, skip=0):
    """For a launch of these sizes: the route it takes now (BBT_RANK_ROUTE; 'lds' or 'global'), the bits of a
    digit (BBT_RANK_DIGIT), the elements of a workgroup (BBT_RANK_WIDTH), the LDS bytes of a workgroup and
    ``lds_rows``: per width 16, 32, 64 the longest block the lds route takes.  No device is needed."""
    route, digit, width, lds = _int(0), _int(0), _int(0), _i64(0)
    rows = (_i64 * 3)()
    check(lib().bbt_rank_info(int(n_spec), int(nbin), int(n_elem), int(m), int(skip), C.byref(route), C.byref(digit),
                              C.byref(width), C.byref(lds), rows))
    return dict(route=RANK_ROUTES[route.value], digit=digit.value, width=width.value, lds_bytes=lds.value,
                lds_rows={16: rows[0], 32: rows[1], 64: rows[2]})


def _rank_sizes(who, x, nbin, n_elem, m, skip):
    if x.dtype != np.float32:
        raise TypeError(f"{who}: x must be float32, not {x.dtype}")
    if n_elem < 1 or nbin < 1 or x.size % (nbin * n_elem) or x.size == 0:
        raise ValueError(f"{who}: {x.size} values are not spectra of {nbin} rows of {n_elem} elements")
    if not RANK_MIN_N <= m <= RANK_MAX_N:
        raise ValueError(f"{who}: a block must have {RANK_MIN_N} ... {RANK_MAX_N} values, not {m}")
    if not 0 <= skip < nbin:
        raise ValueError(f"{who}: skip must be 0 ... {nbin - 1}, not {skip}")
    return x.size // (nbin * n_elem)


def rank_stats(x, nbin, n_elem, m, skip=0, mad=True, out=None):
    """The median -- and, with ``mad``, the median absolute deviation from it -- of every block of ``m`` rows,
    counted from row ``skip``, the last block whatever is left, of every spectrum of float32 ``x`` (spectra of
    ``nbin`` rows of ``n_elem`` elements), by exact selection (bbt_rank_stats in include/bbt_hip.h;
    `search.block_median_mad_samples` is the NumPy restatement).  Returns float32 DeviceArrays ``(n_spec,
    ceil((nbin - skip) / m), n_elem)``: ``(med, mad)`` or ``med``; NaN where a block holds a NaN or an Inf.
    ``out``: the arrays to fill, ``(med, mad)`` or ``(med,)``."""
    nbin, n_elem, m, skip = int(nbin), int(n_elem), int(m), int(skip)
    n_spec = _rank_sizes('rank_stats', x, nbin, n_elem, m, skip)
    shape = (n_spec, -(-(nbin - skip) // m), n_elem)
    if out is None:
        out = tuple(DeviceArray(shape, np.float32) for _ in range(2 if mad else 1))
    size = shape[0] * shape[1] * shape[2]
    if len(out) != (2 if mad else 1) or any(a.dtype != np.float32 or a.size != size for a in out):
        raise ValueError(f"rank_stats: out must be {2 if mad else 1} float32 DeviceArrays of {size} values")
    med, dev = out[0], (out[1] if mad else None)
    check(lib().bbt_rank_stats(x.ptr_to_read(), med.ptr, dev.ptr if mad else None, n_spec, nbin, n_elem, m, skip,
                               _stream))
    return (med, dev) if mad else med


def rank_standardize(x, n, n_elem, out=None):
    """Every whole block of ``n`` samples of float32 ``x`` (samples of ``n_elem`` elements) brought to zero
    median and unit ``1.4826 MAD`` per element (bbt_rank_standardize in include/bbt_hip.h;
    `search.robust_standardize_samples` is the NumPy restatement).  Returns ``out``, float32 of ``(x.size //
    n_elem // n) * n * n_elem`` values."""
    n, n_elem = int(n), int(n_elem)
    if x.dtype != np.float32:
        raise TypeError(f"rank_standardize: x must be float32, not {x.dtype}")
    if n_elem < 1 or x.size % n_elem:
        raise ValueError(f"rank_standardize: {x.size} values are not samples of {n_elem} elements")
    if not RANK_MIN_N <= n <= RANK_MAX_N:
        raise ValueError(f"rank_standardize: n must be {RANK_MIN_N} ... {RANK_MAX_N}, not {n}")
    n_block = x.size // n_elem // n
    if out is None:
        out = DeviceArray((n_block * n, n_elem), np.float32)
    elif out.dtype != np.float32 or out.size != n_block * n * n_elem:
        raise ValueError(f"rank_standardize: out must be a float32 DeviceArray of {n_block * n * n_elem} values")
    check(lib().bbt_rank_standardize(x.ptr_to_read(), out.ptr, n_block, n, n_elem, _stream))
    return out


def rank_whiten(x, nbin, n_elem, m, skip=1, ratio=0.6931471805599453, out=None):
    """Every block of ``m`` bins, counted from bin ``skip``, of every spectrum of float32 ``x`` (spectra of
    ``nbin`` bins of ``n_elem`` elements) divided by its own median over ``ratio``, the bins below ``skip`` +0
    (bbt_rank_whiten in include/bbt_hip.h; `periodicity.median_whiten_samples` is the NumPy restatement).
    Returns ``out``, float32 of the size of ``x``."""
    nbin, n_elem, m, skip, ratio = int(nbin), int(n_elem), int(m), int(skip), float(ratio)
    n_spec = _rank_sizes('rank_whiten', x, nbin, n_elem, m, skip)
    if not 0. < ratio < float('inf'):
        raise ValueError(f"rank_whiten: ratio must be finite and > 0, not {ratio}")
    if out is None:
        out = DeviceArray((n_spec, nbin, n_elem), np.float32)
    elif out.dtype != np.float32 or out.size != x.size:
        raise ValueError(f"rank_whiten: out must be a float32 DeviceArray of {x.size} values")
    check(lib().bbt_rank_whiten(x.ptr_to_read(), out.ptr, n_spec, nbin, n_elem, m, skip, ratio, _stream))
    return out


#: bounds of the sliding median (csrc/rmed_geo.hpp)
RMED_MIN_WIDTH, RMED_MAX_WIDTH, RMED_MAX_SCRUNCH = 3, 1023, 4096
RMED_METHODS = {1: 'radix', 2: 'walk'}
RMED_BASELINE, RMED_DETREND = 0, 1


def rmed_info(width, scrunch=1, n_elem=1, n_rows=1, out_first=0, n_out=None):
    """For the call that makes output samples ``[out_first, out_first + n_out)`` (default: one scrunch row) of
    a stream of ``n_rows`` scrunch rows: the selection method it takes now (BBT_RMED_SELECT; 'radix' or 'walk'),
    the elements and the medians of a workgroup (BBT_RMED_TILE, BBT_RMED_ROWS), the LDS bytes of a workgroup,
    the scratch bytes of the call and the input samples it needs, ``(in_first, in_count)``.  No device is
    needed."""
    method, tile, rows = _int(0), _int(0), _int(0)
    lds, scratch, first, count = _i64(0), _i64(0), _i64(0), _i64(0)
    n_out = int(scrunch) if n_out is None else int(n_out)
    check(lib().bbt_rmed_info(int(width), int(scrunch), int(n_elem), int(n_rows), int(out_first), n_out, C.byref(method),
                              C.byref(tile), C.byref(rows), C.byref(lds), C.byref(scratch), C.byref(first),
                              C.byref(count)))
    return dict(method=RMED_METHODS[method.value], tile=tile.value, rows=rows.value, lds_bytes=lds.value,
                scratch_bytes=scratch.value, in_first=first.value, in_count=count.value)


class RmedPlan(_Plan):
    """The sliding-median baseline of a float32 stream of samples of ``n_elem`` elements: the median over
    ``width`` points of the series scrunched by ``scrunch``, interpolated back to the samples, or the stream
    minus it (bbt_rmed_* in include/bbt_hip.h; `search.running_median_samples` and `search.detrend_samples`
    are the NumPy twins).  The plan owns the scratch of the scrunched series and its medians."""
    _destroy = 'bbt_rmed_plan_destroy'

    def __init__(self, width, scrunch=1, n_elem=1):
        super().__init__()
        self.width, self.scrunch, self.n_elem = int(width), int(scrunch), int(n_elem)
        check(lib().bbt_rmed_plan_create(C.byref(self._h), self.width, self.scrunch, self.n_elem))

    def info(self, n_rows=1, out_first=0, n_out=None):
        """`rmed_info` for a call of this plan."""
        return rmed_info(self.width, self.scrunch, self.n_elem, n_rows, out_first, n_out)

    def execute(self, in_dev, in_first, n_in, out_dev, out_first, n_out, n_rows, detrend=True):
        """``in_dev``: float32, at least ``n_in * n_elem`` values, samples ``[in_first, in_first + n_in)`` of the
        stream; ``out_dev``: float32, at least ``n_out * n_elem``, for samples ``[out_first, out_first + n_out)``,
        whole scrunch rows; ``n_rows``: the scrunch rows of the whole stream, at whose ends alone the windows
        are clipped.  ``detrend``: the stream minus the baseline, else the baseline."""
        in_first, n_in, out_first, n_out, n_rows = int(in_first), int(n_in), int(out_first), int(n_out), int(n_rows)
        if in_dev.dtype != np.float32 or out_dev.dtype != np.float32:
            raise TypeError("RmedPlan.execute: float32 DeviceArrays are needed")
        if (n_in < 1 or n_out < 1 or in_first < 0 or out_first < 0 or in_dev.size < n_in * self.n_elem
                or out_dev.size < n_out * self.n_elem):
            raise ValueError("RmedPlan.execute: float32 DeviceArrays of n_in * n_elem and n_out * n_elem values are "
                             "needed, n_in >= 1, n_out >= 1")
        check(lib().bbt_rmed_execute(self._h, in_dev.ptr_to_read(), in_first, n_in, out_dev.ptr, out_first, n_out,
                                     n_rows, RMED_DETREND if detrend else RMED_BASELINE, _stream))


#: bounds of the correlator and the segment of its rule (csrc/corr_geo.hpp)
CORR_MIN_INPUTS, CORR_MAX_INPUTS, CORR_MAX_N, CORR_SEG = 2, 64, 1 << 24, 1024


def corr_info(n_inputs, n_elem=1, n=1, first=0, count=None):
    """For the piece ``[first, first + count)`` (default: one block) of a stream correlated in blocks of ``n``:
    the elements that share a tile now (BBT_CORR_PACK), the tiles a wave holds, the waves of a workgroup
    (BBT_CORR_WAVES), the LDS bytes of a workgroup, the scratch bytes and the segments of the piece.  No
    device is needed."""
    pack, tiles, waves = _int(0), _int(0), _int(0)
    lds, scratch, n_seg = _i64(0), _i64(0), _i64(0)
    count = int(n) if count is None else int(count)
    check(lib().bbt_corr_info(int(n_inputs), int(n_elem), int(n), int(first), count, C.byref(pack), C.byref(tiles),
                              C.byref(waves), C.byref(lds), C.byref(scratch), C.byref(n_seg)))
    return dict(pack=pack.value, tiles=tiles.value, waves=waves.value, lds_bytes=lds.value,
                scratch_bytes=scratch.value, n_seg=n_seg.value)


class CorrPlan(_Plan):
    """The cross-products ``x_i conj(x_j)``, ``i <= j``, of the ``n_inputs`` adjacent inputs of a complex64 stream
    of samples of ``n_elem`` elements, integrated over blocks of ``n`` samples (bbt_corr_* in
    include/bbt_hip.h; `correlation.correlate_samples` restates the values in NumPy).  ``inner``: the elements
    of a sample that lie behind the baselines in the output.  The plan owns the scratch of the segment
    values and the float64 carry of a block that a piece leaves unfinished."""
    _destroy = 'bbt_corr_plan_destroy'

    def __init__(self, n_inputs, n_elem, n, inner=1, average=True):
        super().__init__()
        self.n_inputs, self.n_elem, self.n, self.inner = int(n_inputs), int(n_elem), int(n), int(inner)
        self.average = bool(average)
        self.n_baselines = self.n_inputs * (self.n_inputs + 1) // 2
        check(lib().bbt_corr_plan_create(C.byref(self._h), self.n_inputs, self.n_elem, self.inner, self.n,
                                         int(self.average)))

    def info(self, first=0, count=None):
        """`corr_info` for a piece of this plan."""
        return corr_info(self.n_inputs, self.n_elem, self.n, first, count)

    def execute(self, in_dev, first, count, out_dev, out_block0, n_out_blocks):
        """``in_dev``: complex64, at least ``count * n_elem * n_inputs`` values, samples ``[first, first + count)`` of
        the stream, whole segments; ``out_dev``: complex64, ``n_out_blocks * n_elem * n_baselines`` values at least,
        for blocks ``[out_block0, out_block0 + n_out_blocks)``, of which those that end in the piece are written."""
        first, count, out_block0, n_out_blocks = int(first), int(count), int(out_block0), int(n_out_blocks)
        if in_dev.dtype != np.complex64 or out_dev.dtype != np.complex64:
            raise TypeError("CorrPlan.execute: complex64 DeviceArrays are needed")
        if (count < 1 or first < 0 or n_out_blocks < 0 or in_dev.size < count * self.n_elem * self.n_inputs
                or out_dev.size < n_out_blocks * self.n_elem * self.n_baselines):
            raise ValueError("CorrPlan.execute: complex64 DeviceArrays of count * n_elem * n_inputs and n_out_blocks * "
                             "n_elem * n_baselines values are needed, count >= 1")
        check(lib().bbt_corr_execute(self._h, in_dev.ptr_to_read(), first, count, out_dev.ptr, out_block0,
                                     n_out_blocks, _stream))


COMM_ID_BYTES = 128


def comm_unique_id():
    """The id rank 0 creates and hands to the other ranks (bytes)."""
    lib()
    if _torch_lib_dir is not None:
        _preload_torch_runtime('librccl.so')         # the RCCL that goes with the preloaded runtime
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(lib().bbt_comm_unique_id(buf, COMM_ID_BYTES))
    return buf.raw


class Comm(_Plan):
    """RCCL communicator behind the C ABI (one process per GPU; call after
    `set_device`).  ``uid``: the bytes of `comm_unique_id()` made on rank 0."""
    _destroy = 'bbt_comm_destroy'

    def __init__(self, n_ranks, rank, uid):
        super().__init__()
        self.n_ranks, self.rank = int(n_ranks), int(rank)
        lib()
        if _torch_lib_dir is not None:
            _preload_torch_runtime('librccl.so')
        uid = bytes(uid)
        check(lib().bbt_comm_init(C.byref(self._h), self.n_ranks, self.rank, uid, len(uid)))

    def bcast_chirp(self, resp_dev, root=0):
        """In-place broadcast of a complex64 DeviceArray from ``root``."""
        assert resp_dev.dtype == np.complex64
        check(lib().bbt_bcast_chirp(self._h, resp_dev.ptr, resp_dev.size, int(root), _stream))
        return resp_dev

    def gather_output(self, local, out=None):
        """All-gather equally sized DeviceArrays along axis 0, in rank order."""
        if out is None:
            out = DeviceArray((self.n_ranks * local.shape[0],) + local.shape[1:], local.dtype)
        check(lib().bbt_gather_output(self._h, local.ptr, out.ptr, local.nbytes, _stream))
        return out
