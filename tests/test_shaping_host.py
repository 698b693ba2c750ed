"""Shaping and combining tasks, the parts that need no GPU: index maps and their run compression
against NumPy, the route a plan picks, metadata and refusals against the real reference's golden
cases (tests/golden/shaping_vectors.npz) and its own test expectations (the reference's
tests/test_shaping.py and tests/test_combining.py, with generated streams in place of the VDIF sample
file), and the C ABI's argument refusals.  Samples are only moved, so every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, units as u
from baseband_tasks_amd.base import _TimeSlice
from baseband_tasks_amd.shaping import index_map, map_runs

import shaping_cases as sc

CASES = sc.load()
T0 = '2020-01-01T00:00:00'


def noise(shape, spf=64, start=T0, rate=1e6, dtype=np.complex64, seed=1, **kw):
    return bt.NoiseGenerator(shape, start, rate, spf, dtype=dtype, seed=seed, **kw)


def apply_map(datas, src, elem, out_shape):
    """NumPy model of the kernels: out[t, j] = datas[src[j]][t].ravel()[elem[j]]."""
    n = datas[0].shape[0]
    flat = [d.reshape(n, -1) for d in datas]
    out = np.empty((n, len(src)), datas[0].dtype)
    for k, f in enumerate(flat):
        sel = src == k
        out[:, sel] = f[:, elem[sel]]
    return out.reshape((n,) + tuple(out_shape))


def model_runs(src, elem):
    runs = []
    for j, (s, e) in enumerate(zip(src.tolist(), elem.tolist())):
        if runs and runs[-1][1] == s and runs[-1][2] + runs[-1][3] == e:
            runs[-1][3] += 1
        else:
            runs.append([j, s, e, 1])
    return [tuple(r) for r in runs]


# ---------------------------------------------------------------------------------------------
# index maps
@pytest.mark.parametrize('key,meta,inputs,want', CASES, ids=[c[0] + '-' + c[1]['cls'] for c in CASES])
def test_golden_maps_and_metadata(key, meta, inputs, want):
    streams = [sc.host_stream(meta, k, x) for k, x in enumerate(inputs)]
    task = sc.build(meta, streams)
    sc.check_metadata(task, meta)
    # the map applied to the aligned inputs is the reference's output
    if meta['cls'] in sc.SHAPING:
        start = getattr(task, '_start', 0)
        datas = [inputs[0][start:start + task.shape[0]]]
    else:
        datas = [x[f:f + task.shape[0]] for x, f in zip(inputs, task._firsts)]
    got = apply_map(datas, task._map_src, task._map_elem, task.sample_shape)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert map_runs(task._map_src, task._map_elem) == model_runs(task._map_src, task._map_elem)


shapes = st.lists(st.integers(1, 5), min_size=1, max_size=4).map(tuple)


@settings(max_examples=60, deadline=None)
@given(shape=shapes, data=st.data())
def test_random_transposes_items_and_reshapes(shape, data):
    rng = np.random.default_rng(data.draw(st.integers(0, 2**31)))
    x = rng.integers(-1000, 1000, size=(5,) + shape).astype(np.int16)
    perm = data.draw(st.permutations(range(1, len(shape) + 1)))
    item = tuple(data.draw(st.one_of(
        st.integers(-d, d - 1), st.slices(d), st.lists(st.integers(-d, d - 1), min_size=1, max_size=4)))
        for d in shape[:data.draw(st.integers(1, len(shape)))])
    lists = [k for k, i in enumerate(item) if isinstance(i, list)]
    if lists:
        # (NumPy moves the axes of index arrays that a slice separates to the front, the time axis
        # with them: keep one list, and no integers beside it)
        item = tuple(i if k == lists[0] else slice(i[0], i[0] + 1 or None) if isinstance(i, list)
                     else slice(i, i + 1 or None) if isinstance(i, int) else i for k, i in enumerate(item))
    for task in (lambda d: d.transpose((0,) + tuple(perm)), lambda d: d[(slice(None),) + item],
                 lambda d: d.reshape(d.shape[0], -1)[:, ::-1], lambda d: np.moveaxis(d, 1, -1)):
        want = task(x)
        if want.size == 0:
            continue
        out_shape, src, elem = index_map(task, [shape])
        assert tuple(out_shape) == want.shape[1:]
        assert np.array_equal(apply_map([x], src, elem, out_shape), want)
        runs = map_runs(src, elem)
        assert runs == model_runs(src, elem)
        assert sum(r[3] for r in runs) == len(src)


@settings(max_examples=40, deadline=None)
@given(shape=shapes, n=st.integers(1, 5), data=st.data())
def test_random_stacks_and_concatenations(shape, n, data):
    rng = np.random.default_rng(data.draw(st.integers(0, 2**31)))
    xs = [rng.integers(-1000, 1000, size=(4,) + shape).astype(np.int16) for _ in range(n)]
    axis = data.draw(st.integers(1, len(shape)))
    for task in (lambda d: np.stack(d, axis=axis), lambda d: np.stack(d, axis=-1),
                 lambda d: np.concatenate(d, axis=axis), lambda d: np.concatenate(d[::-1], axis=-1)):
        want = task(xs)
        out_shape, src, elem = index_map(task, [shape] * n, combine=True)
        assert np.array_equal(apply_map(xs, src, elem, out_shape), want)
        assert map_runs(src, elem) == model_runs(src, elem)


def test_random_permutation_is_all_single_runs_or_fewer():
    rng = np.random.default_rng(5)
    perm = rng.permutation(4096)
    out_shape, src, elem = index_map(lambda d: d[:, perm], [(4096,)])
    assert np.array_equal(elem, perm) and not src.any()
    assert map_runs(src, elem) == model_runs(src, elem)


def test_large_rows_index_in_64_bits():
    """The host model of the kernels' flat index: n_samples * row passes 2^31 (the element count
    one launch covers is not limited by 32 bits)."""
    row, n = 3 * 2**20, 2**11 + 5
    g = np.int64(n) * row - 1
    assert g > 2**31 and g // row == n - 1 and g % row == row - 1


# ---------------------------------------------------------------------------------------------
# refusals
def test_computing_callables_are_refused():
    ih = noise((1000, 4, 2))
    for task in (lambda d: d[:, 0] + d[:, 1], lambda d: d * 2, lambda d: d * 1.0, lambda d: d + 1,
                 lambda d: d.sum(1), lambda d: np.zeros_like(d)):
        with pytest.raises(TypeError, match='rearrange'):
            bt.ChangeSampleShape(ih, task)
    with pytest.raises(TypeError, match='rearrange'):
        bt.CombineStreams([ih, noise((1000, 4, 2), seed=2)], lambda d: d[0] + d[1])
    with pytest.raises(ValueError, match='sample axis'):
        bt.ChangeSampleShape(ih, lambda d: d.reshape(-1, 2))
    with pytest.raises(ValueError, match='sample axis'):
        bt.ChangeSampleShape(ih, lambda d: d.swapaxes(0, 1))


def test_reference_shaping_expectations():
    """Ported from the reference's tests/test_shaping.py (metadata of an 8-thread stream)."""
    freq = 311.25e6 + (np.arange(8.) // 2) * 16e6
    pol = np.tile(['L', 'R'], 4)
    fh = noise((4000, 8), frequency=freq, sideband=1, polarization=pol)
    rt = bt.Reshape(fh, (4, 2))
    assert rt.shape == (4000, 4, 2) and rt.sample_shape == (4, 2)
    assert rt.start_time == fh.start_time and rt.sample_rate == fh.sample_rate
    assert np.array_equal(rt.frequency, freq[::2].reshape(4, 1))
    assert np.array_equal(rt.polarization, pol[:2]) and np.all(rt.sideband == 1)
    assert rt.sideband.shape == ()
    tt = bt.Transpose(rt, (2, 1))
    assert tt.shape == (4000, 2, 4)
    assert np.array_equal(tt.frequency, freq[::2]) and np.array_equal(tt.polarization, pol[:2].reshape(2, 1))
    rtt = bt.ReshapeAndTranspose(fh, (4, 2), (2, 1))
    assert rtt.shape == tt.shape
    assert np.array_equal(rtt.index_map, np.arange(8).reshape(4, 2).T)
    assert np.array_equal(rtt.frequency, tt.frequency) and np.array_equal(rtt.polarization, tt.polarization)
    gi = bt.GetItem(fh, slice(0, 6))
    assert gi.shape == (4000, 6) and np.array_equal(gi.frequency, freq[:6])
    assert np.array_equal(gi.polarization, pol[:6])
    sh = bt.ChangeSampleShape(fh, lambda data: data.reshape(-1, 4, 2)[:, :3])
    assert sh.shape == (4000, 3, 2) and np.array_equal(sh.frequency, freq[:6:2].reshape(3, 1))
    gs = bt.GetSlice(fh, slice(10, -10))
    assert gs.shape == (3980, 8) and abs(gs.start_time - (fh.start_time + 10 / 1e6)) < 1e-12
    assert abs(gs.stop_time - (fh.stop_time - 10 / 1e6)) < 1e-12
    gs2 = fh[10:-10, 2:4]
    assert isinstance(gs2, bt.GetSlice) and gs2.shape == (3980, 2)
    assert np.array_equal(np.broadcast_to(gs2.frequency, (2,)), freq[2:4]) and np.array_equal(gs2.polarization, pol[2:4])
    # wrong arguments carry the reference's extra message
    with pytest.raises(ValueError, match='cannot be changed'):
        bt.Reshape(fh, (4, 4))
    with pytest.raises(ValueError, match='cannot be changed'):
        bt.Transpose(rt, (1, 0))
    with pytest.raises(IndexError, match='cannot be changed'):
        bt.GetItem(fh, 8)
    # GetSlice asserts like the reference
    for item in (5, slice(0, 100, 2), slice(10, 10)):
        with pytest.raises(AssertionError):
            bt.GetSlice(fh, item)


def test_reference_combining_expectations():
    """Ported from the reference's tests/test_combining.py."""
    freq = 311.25e6 + np.arange(4.) * 16e6
    a = noise((4000, 4), frequency=freq, sideband=1, polarization='L', seed=1)
    b = noise((4000, 4), frequency=freq, sideband=1, polarization='R', seed=2)
    st_ = bt.Stack([a, b], axis=2)
    assert st_.shape == (4000, 4, 2) and st_.start_time == a.start_time
    assert np.array_equal(st_.frequency, freq.reshape(4, 1)) and np.array_equal(st_.polarization, ['L', 'R'])
    assert st_.sideband.shape == () and st_.samples_per_frame == a.samples_per_frame
    assert 'ihs: 2 streams' in repr(st_)
    cc = bt.Concatenate([a, b], axis=-1, samples_per_frame=100)
    assert cc.shape == (4000, 8) and cc.samples_per_frame == 100
    assert np.array_equal(cc.frequency, np.concatenate([freq, freq]))
    assert np.array_equal(cc.polarization, np.repeat(['L', 'R'], 4))
    cs = bt.CombineStreams([a, b], lambda d: np.stack(d, axis=1))
    assert cs.shape == (4000, 2, 4) and np.array_equal(cs.polarization, [['L'], ['R']])
    # no metadata anywhere stays None
    plain = bt.Stack([noise((100,)), noise((100,), seed=3)], axis=-1)
    assert getattr(plain, 'frequency', None) is None and getattr(plain, 'polarization', None) is None
    # different start times: the common span, offsets by whole samples
    meta = dict(frequency=freq, sideband=1, polarization='R')
    late = noise((4000, 4), start=u.Time(T0) + 25e-6, seed=4, **meta)
    both = bt.Stack([a, late], samples_per_frame=50)
    assert both.shape == (3975, 2, 4) and abs(both.start_time - late.start_time) < 1e-12
    assert both._firsts == [25, 0]
    off = noise((4000, 4), start=u.Time(T0) + 25.3e-6, seed=4, **meta)
    with pytest.raises(ValueError, match='streams only aligned to'):
        bt.Stack([a, off])
    assert bt.Stack([a, off], atol=0.4e-6).shape[0] == 3975
    with pytest.raises(ValueError, match='cannot be combined'):
        bt.Concatenate([a, noise((4000, 4, 2))])
    with pytest.raises(ValueError, match='sample axis'):
        bt.Stack([a, b], axis=0)
    with pytest.raises(ValueError, match='sample axis'):
        bt.Concatenate([a, b], axis=0)
    with pytest.raises(AssertionError):
        bt.Stack([a, noise((4000, 4), rate=2e6)])
    with pytest.raises(AssertionError):
        bt.Stack([a, noise((4000, 4), dtype=np.float32)])
    with pytest.raises((TypeError, IndexError), match='at least one stream'):
        bt.Stack([])
    st_.close()
    assert b.closed and not a.closed


def test_time_slices_are_what_they_were():
    fh = noise((1000, 2))
    ts = fh[10:20]
    assert type(ts) is _TimeSlice and ts.shape == (10, 2) and ts._first == 10
    assert type(fh[10:20, ]) is _TimeSlice
    with pytest.raises(NotImplementedError):
        fh[::2]
    with pytest.raises(NotImplementedError):
        fh[::2, 0]
    with pytest.raises(NotImplementedError):
        fh[5]
    gs = fh[10:20, 0]
    assert isinstance(gs, bt.GetSlice) and gs.shape == (10,) and gs._start == 10


# ---------------------------------------------------------------------------------------------
# routes (a plan is made, and its route read, without a device)
def plan_of(task, shapes, eb, route='auto', combine=False):
    _, src, elem = index_map(task, shapes, combine=combine)
    return hip.GatherPlan([int(np.prod(s, dtype=int)) for s in shapes], src, elem, eb, route=route)


def test_route_choice():
    two = [(), ()]
    assert plan_of(lambda d: np.stack(d, -1), two, 8, combine=True).info()['route'] == 'tile'
    assert plan_of(lambda d: np.stack(d, -1), [()] * 8, 8, combine=True).info()['route'] == 'tile'
    wide = [(1024, 2)] * 2
    p = plan_of(lambda d: np.concatenate(d, 1), wide, 8, combine=True)
    assert p.info()['route'] == 'run_copy' and p.info()['n_runs'] == 2
    assert plan_of(lambda d: np.stack(d, 1), wide, 8, combine=True).info()['route'] == 'run_copy'
    t = plan_of(lambda d: d.transpose(0, 2, 1), [(1024, 2)], 8)
    assert t.info()['route'] == 'tile' and t.info()['n_runs'] == 2048
    # (rows of 16 KiB and one 8-byte granule per 256 bytes: 16896 bytes a sample, three in 64 KiB)
    assert t.info()['tile_samples'] == 3 and 3 * 16896 <= t.info()['lds_bytes'] <= 65536
    assert plan_of(lambda d: d[:, 100:356], [(1024, 2)], 8).info()['route'] == 'run_copy'
    assert plan_of(lambda d: d[:, ::2], [(1024, 2)], 8).info()['route'] == 'run_copy'      # (runs of two: 16 bytes)
    assert plan_of(lambda d: d[:, ::2], [(1024,)], 8).info()['route'] == 'tile'
    assert plan_of(lambda d: d[:, ::2], [(1024,)], 16).info()['route'] == 'run_copy'
    # a row too large for a tile, and an index array with no structure over a wide row
    assert plan_of(lambda d: d.transpose(0, 2, 1), [(8192, 2)], 8).info()['route'] == 'direct'
    pick = np.random.default_rng(1).permutation(65536)[:64]
    assert plan_of(lambda d: d[:, pick], [(65536,)], 4).info()['route'] == 'direct'
    # every map may be forced onto the direct route; the others only where their conditions hold
    assert plan_of(lambda d: np.concatenate(d, 1), wide, 8, 'direct', True).info()['route'] == 'direct'
    assert plan_of(lambda d: np.concatenate(d, 1), [(8, 2)] * 2, 8, 'tile', True).info()['route'] == 'tile'
    with pytest.raises(hip.HipError, match='16-byte'):
        plan_of(lambda d: np.stack(d, -1), two, 8, 'run_copy', True)
    with pytest.raises(hip.HipError, match='tile'):
        plan_of(lambda d: d.transpose(0, 2, 1), [(8192, 2)], 8, 'tile')


def test_abi_refusals():
    lib = hip.lib()
    plan = C.c_void_p()
    rows = np.array([4, 4], np.int64)
    src = np.array([0, 1, 0, 1], np.int32)
    elem = np.array([0, 0, 1, 1], np.int64)
    pi64, pi32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)

    def create(n_src=2, rows=rows, src=src, elem=elem, eb=8, route=0):
        return lib.bbt_gather_plan_create_ex(C.byref(plan), n_src, rows.ctypes.data_as(pi64), len(src),
                                             src.ctypes.data_as(pi32), elem.ctypes.data_as(pi64), eb, route)
    assert create(eb=3) != 0 and b'elem_bytes' in lib.bbt_last_error()
    assert create(eb=32) != 0
    assert create(n_src=65, rows=np.full(65, 4, np.int64)) != 0 and b'n_src' in lib.bbt_last_error()
    assert create(n_src=0) != 0
    assert create(src=np.array([0, 2, 0, 1], np.int32)) != 0 and b'out of range' in lib.bbt_last_error()
    assert create(elem=np.array([0, 0, 4, 1], np.int64)) != 0 and b'out of range' in lib.bbt_last_error()
    assert create(elem=np.array([0, -1, 1, 1], np.int64)) != 0
    assert create(route=7) != 0
    assert lib.bbt_gather_plan_create(None, 2, rows.ctypes.data_as(pi64), 4, src.ctypes.data_as(pi32),
                                      elem.ctypes.data_as(pi64), 8) != 0
    assert create() == 0 and plan.value
    # an output that overlaps a source, null and misaligned pointers (refused before anything runs)
    ptrs = (C.c_void_p * 2)(0x10000, 0x20000)
    first = np.zeros(2, np.int64)
    ex = lib.bbt_gather_execute
    assert ex(plan, ptrs, first.ctypes.data_as(pi64), C.c_void_p(0x10000 + 64), 100, None) != 0
    assert b'overlaps source 0' in lib.bbt_last_error()
    assert ex(plan, ptrs, first.ctypes.data_as(pi64), C.c_void_p(0x20000 - 64), 100, None) != 0
    assert b'overlaps source 1' in lib.bbt_last_error()
    assert ex(plan, ptrs, first.ctypes.data_as(pi64), C.c_void_p(0x30004), 100, None) != 0
    assert b'aligned' in lib.bbt_last_error()
    assert ex(plan, ptrs, first.ctypes.data_as(pi64), None, 100, None) != 0
    assert ex(plan, ptrs, first.ctypes.data_as(pi64), C.c_void_p(0x30000), -1, None) != 0
    first[1] = -1
    assert ex(plan, ptrs, first.ctypes.data_as(pi64), C.c_void_p(0x30000), 100, None) != 0
    assert ex(None, ptrs, None, C.c_void_p(0x30000), 100, None) != 0
    assert lib.bbt_gather_plan_info(None, None, None, None, None) != 0
    assert lib.bbt_gather_plan_destroy(plan) == 0 and lib.bbt_gather_plan_destroy(None) == 0
    with pytest.raises(hip.HipError, match='elem_bytes'):
        hip.GatherPlan([4], [0], [0], 3)


# ---------------------------------------------------------------------------------------------
# whose frame cache a ``read_device`` result lies in (device_task.cache_producer): the combining
# tasks copy the views of inputs that share one
def empty(shape=(640, 2, 3), spf=64, **kw):
    return bt.EmptyStreamGenerator(shape, T0, 1e6, samples_per_frame=spf, **kw)


def test_cache_producer_walks_through_the_wrappers_that_hand_views_on():
    from baseband_tasks_amd.device_task import cache_producer, produces_on_device
    host = empty(frequency=np.full((2, 3), 1e9), sideband=1)
    assert cache_producer(host) is None and cache_producer(host[10:20]) is None      # (uploads: the caller's)
    t = bt.Transpose(host, (2, 1))                      # moves elements: a device task with a frame cache
    assert t.route == 'tile' and t._view_source is None and cache_producer(t) is t
    wrappers = [t[64:200], t[64:200, :], bt.GetSlice(t, slice(64, 200)), bt.Reshape(t[64:200], (3, 2)),
                bt.Reshape(t[64:200], (6,)), bt.Reshape(t, (2, 3)), bt.GetItem(t, slice(None)),
                bt.GetItem(t[3:], (slice(0, 3), slice(None))), bt.Transpose(t[:128], (1, 2)),
                bt.SetAttribute(t[64:192], frequency=np.full((3, 2), 2e9), sideband=-1),
                bt.SetAttribute(t, start_time=bt.Time(T0) - 1e-3)[0:100]]
    for w in wrappers:
        assert produces_on_device(w) and w._view_source is not None, w
        assert getattr(w, 'route', None) is None
        assert cache_producer(w) is t, w
    # mixed chains, several deep
    deep = bt.SetAttribute(bt.Reshape(bt.GetItem(t[5:500], slice(None))[7:300, :], (6,)), polarization='X')[1:]
    assert cache_producer(deep) is t
    # a wrapper that moves elements, or over a host stream, owns the cache its views lie in
    for own in (bt.GetItem(t, 0), t[64:200, 1], bt.Transpose(t[64:200], (2, 1)), bt.Reshape(host, (6,)),
                bt.Stack([t, t]), bt.Stack([t, t])[3:9].ih):
        assert cache_producer(own) is own and own is not t
    assert cache_producer(bt.GetItem(t, 0)[1:5]).ih is t
    # a SetAttribute that changes the framing reads on the host: its result is an upload
    assert cache_producer(bt.SetAttribute(t, samples_per_frame=32)) is None
    # distinct producers stay distinct, under whatever wrappers
    t2 = bt.Transpose(host, (2, 1))
    assert cache_producer(t2[:100]) is t2 and cache_producer(t2[:100]) is not cache_producer(t[:100])


def test_cache_producer_exempts_resident_streams_and_fresh_blocks():
    from baseband_tasks_amd.device_task import cache_producer

    class Source(bt.EmptyStreamGenerator):
        _produces_on_device = True

    class Resident(Source):
        _resident = True

    assert bt.DeviceStream._resident and bt.DeviceNoiseGenerator._views_keep_their_block
    args = ((64, 2), T0, 1e6)
    other = Source(*args)
    assert cache_producer(other) is other and cache_producer(other[3:9]) is other     # (unknown: its own)
    assert cache_producer(Resident(*args)) is None and cache_producer(Resident(*args)[3:9]) is None
    noise_dev = bt.DeviceNoiseGenerator((640, 2), T0, 1e6, 64, seed=1)
    assert cache_producer(noise_dev) is None and cache_producer(bt.Reshape(noise_dev[5:], (2, 1))) is None


def test_views_to_keep_marks_all_but_the_last_fetch_from_a_producer():
    from baseband_tasks_amd.device_task import cache_producer, views_to_keep
    a, b = object(), object()
    assert views_to_keep([]) == []
    assert views_to_keep([a]) == [False] and views_to_keep([None, None, None]) == [False] * 3
    assert views_to_keep([a, b]) == [False, False]
    assert views_to_keep([a, a]) == [True, False] and views_to_keep([a, a, a]) == [True, True, False]
    assert views_to_keep([a, b, a, None, b, a]) == [True, True, True, False, False, False]
    # as a combining task sees its inputs
    host = empty()
    t, t2 = bt.Transpose(host, (2, 1)), bt.Transpose(host, (2, 1))
    ins = [t[0:100], host[0:100], t2[0:100], bt.Reshape(t[50:150], (3, 2)), t2[1:101, :]]
    assert views_to_keep([cache_producer(ih) for ih in ins]) == [True, False, True, False, False]
    assert not any(views_to_keep([cache_producer(ih) for ih in (t, t2, host, host)]))
