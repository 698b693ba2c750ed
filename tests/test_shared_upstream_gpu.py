"""Task graphs in which several branches reach ONE upstream device task: windows of one task combined
by `Stack` / `Concatenate` / `CombineStreams` (lagged copies of a stream, on- and off-pulse ranges of a
fold), and diamonds of two consumers read in turn.

``read_device`` of a device task hands out a view of the task's frame cache, and time slices,
relabellings (`SetAttribute`) and shaping tasks that keep every element in place hand that view on as
it is.  The next read of the task may refill the cache, so a combining task, which fetches all its
inputs before it launches its one gather, has to make the views of inputs that share a producer its own
(`device_task.cache_producer`, `views_to_keep`).  Every case here builds such a graph and compares it,
bit for bit, with branches that were built a second time from the same host array and read alone, put
together by NumPy.

Geometry, in frames of the shared task (``spf`` samples): every window is 2.75 frames long and the
windows sit at 0, d, 2d with d one of

* ``inside``   0.2 frames: the second window lies in the frames the first fetch cached (the control),
* ``miss``     1.25 frames: its frames are not all cached and it does not start on the last cached one,
* ``straddle`` 2.25 frames: it starts on the last cached frame (the ``reuse`` path of `_ensure_frames`),

which every test asserts by replaying the cache rule on the frame numbers (`fetch_relations`).  A
combining task lines its inputs up by their times and keeps the span they share, so a bare
``Stack([t[0:n], t[d:n + d]])`` reads the SAME range of ``t`` twice (see
`test_bare_windows_are_lined_up_by_time`); windows become lagged copies by setting the clock of ``t``
back by the lag first (`relabelled`), which is one more wrapper that hands views on.

Measured once on an MI355X with the copies switched off (what the tree did before), 145 cases: 101
failed, 44 passed.

* A: all ``inside`` cases passed, with three windows too (the third window leaves the cached run, but the
  refill starts on the same frame and puts the same samples in the same place).  All ``miss`` and
  ``straddle`` cases failed for every upstream but `Dedisperse`: its ``miss`` cases passed with two AND
  with three windows (a deferred call is owed, so the cache alternates between two buffers, and the
  third fetch needs one frame more than the first, which is a new allocation); its ``straddle`` cases failed.
* B: every wrapper failed at both lags, the bare task with a wrapped window of it as well.
* C: `Stack`, `Concatenate` and the reversed callable failed; the callable that leaves one of three inputs
  out passed (its second fetch needs a larger buffer: a new allocation); ``Stack([t, t])`` and the bare
  windows passed (one range read twice).
* D: every pattern failed over `Square`; over `Dedisperse` the whole read, ``read_device``, the seek back
  (two and three windows), and with two windows the upstream run frame by frame and one piecewise read
  passed, the other ten failed.
* E: all passed: the diamonds without a combiner, and the stacks of `Dedisperse` branches over one
  `Real2Complex` (each branch owns its cache; the shared one is guarded by its deferred readers).
* The copy counts: none for distinct producers, before and after; none for shared ones before.
"""
import functools

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hdf5, hip, ingest, psrfits
from baseband_tasks_amd import units as u
from baseband_tasks_amd.device_task import cache_producer, produces_on_device

pytestmark = pytest.mark.gpu

T0 = bt.Time('2020-01-01T00:00:00') + 0.25
RATE = 1e6
BAND = dict(frequency=np.array([400e6, 400e6]), sideband=np.array([1, -1]))
KINDS = ('inside', 'miss', 'straddle')


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


# -- helpers ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noise(shape, dtype='c8', seed=1):
    """Seeded normal samples on the host; every private copy of a chain starts from the same array."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == 'c':
        x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    else:
        x = (8. * rng.standard_normal(shape)).astype(np.float32)
    x.setflags(write=False)
    return x


def device_stream(x, spf, rate=RATE, **kw):
    return bt.DeviceStream(hip.DeviceArray.from_host(x), T0, rate, samples_per_frame=spf, **kw)


def same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    row = max(got.nbytes // max(got.shape[0], 1), 1)
    bad = np.flatnonzero(got.view(np.uint8).ravel() != want.view(np.uint8).ravel())
    assert bad.size == 0, f'{bad.size} of {got.nbytes} bytes differ, the first in sample {bad[0] // row} of {got.shape[0]}'


def geometry(spf, kind):
    """(window length, lag) in samples for frames of ``spf`` samples: 2.75 frames, and 0.2 / 1.25 / 2.25."""
    return -(-11 * spf // 4), {'inside': spf // 5, 'miss': 5 * spf // 4, 'straddle': 2 * spf + spf // 4}[kind]


def frames(start, count, spf):
    return start // spf, (start + count - 1) // spf + 1


def relation(cached, wanted):
    """What `DeviceTaskMixin._ensure_frames` does for frames ``wanted`` with frames ``cached`` in the cache."""
    (c0, c1), (w0, w1) = cached, wanted
    if c0 <= w0 and w1 <= c1:
        return 'inside'
    if w0 == c1 - 1 and w1 > w0 + 1:
        return 'straddle'
    return 'miss'


def fetch_relations(starts, count, spf):
    """The relation of every fetch after the first to what the fetches before it left in the cache."""
    cached, out = frames(starts[0], count, spf), []
    for start in starts[1:]:
        wanted = frames(start, count, spf)
        out.append(relation(cached, wanted))
        if out[-1] != 'inside':
            cached = wanted
    return out


def check_geometry(kind, starts, count, spf):
    got = fetch_relations(starts, count, spf)
    assert got[0] == kind, (kind, got, spf)
    if kind != 'inside':                      # (at 0.2 frames the third window leaves the cached run)
        assert all(r == kind for r in got), (kind, got, spf)
    return got


def relabelled(t, lag, start=None, **kw):
    """``t`` with its clock set back by ``lag`` samples: ``relabelled(t, a)[a:]`` starts when ``t`` does
    (or at ``start``).  A `SetAttribute` that hands the views of ``t`` on."""
    start = bt.Time(t.start_time if start is None else start)
    out = bt.SetAttribute(t, start_time=start - lag / u.to_hz(t.sample_rate), **kw)
    assert produces_on_device(out) and out._view_source is t
    return out


def window(t, a, n, start=None):
    w = relabelled(t, a, start)[a:a + n]
    assert w.shape[0] == n and produces_on_device(w) and cache_producer(w) is cache_producer(t)
    return w


def alone(make, a, n, wrap=None):
    """Samples [a, a + n) of a privately built chain, through the same wrappers, read alone."""
    w = window(make(), a, n)
    return (w if wrap is None else wrap(w)).read()


# -- the upstream tasks: name -> function of tmp_path that returns a maker of private copies -----------
def phase(t):
    return 62500. * (t - T0)


def up_square(tmp_path):
    return lambda: bt.Square(device_stream(noise((4096, 2)), 256))


def up_power(tmp_path):
    return lambda: bt.Power(device_stream(noise((4096, 2)), 256, polarization=['X', 'Y']))


def channelized(n=4096, spf=256):
    ds = device_stream(noise((n, 2)), spf, frequency=400e6, sideband=1, polarization=['X', 'Y'])
    return bt.Channelize(ds, 16, samples_per_frame=16)


def up_channelize(tmp_path):
    return lambda: channelized()


def dedisperse_frame(ds, dm=10.):
    pad = (lambda d: d._pad_start + d._pad_end)(bt.Dedisperse(ds, dm))
    assert 0 < pad < 4096
    return 8192 - pad                           # (blocks of 2^13 samples)


def up_dedisperse(tmp_path):
    def make():
        ds = device_stream(noise((1 << 16, 2)), 512, **BAND)
        return bt.Dedisperse(ds, 10., samples_per_frame=dedisperse_frame(ds))
    return make


def up_real2complex(tmp_path):
    return lambda: bt.Real2Complex(device_stream(noise((8192, 2), 'f4'), 512, frequency=300e6, sideband=1),
                                   samples_per_frame=256)


def up_transpose(tmp_path):
    def make():
        t = bt.Transpose(device_stream(noise((4096, 2, 3)), 256), (2, 1))
        assert t.route is not None and t._view_source is None
        return t
    return make


def up_integrate(tmp_path):
    return lambda: bt.Integrate(bt.Power(channelized()), 4)


def up_fold(tmp_path):
    return lambda: bt.Fold(bt.Square(device_stream(noise((4096, 2)), 256)), 8, phase, step=128)


def up_hdf5(tmp_path):
    x = noise((4096, 2))
    name = str(tmp_path / 'coded.h5')
    with hdf5.open(name, 'w', shape=x.shape, start_time=T0, sample_rate=RATE, dtype=x.dtype, bps=8, **BAND) as fw:
        fw.write(hip.DeviceArray.from_host(x))
    return lambda: hdf5.open(name, samples_per_frame=512)


def fits_source():
    return device_stream(noise((1 << 16, 2)), 1 << 12, frequency=400. * u.MHz, sideband=1, polarization=['X', 'Y'])


def up_psrfits_search(tmp_path):
    name = str(tmp_path / 'search.fits')
    stream = bt.Integrate(bt.Power(bt.Channelize(fits_source(), 16)), 4)
    assert stream.shape == (1024, 16, 4)
    with psrfits.open_search(name, 'w', template=stream, nbits=8, nsblk=64) as fw:
        stream.read(out=fw)
    return lambda: psrfits.open_search(name)


def up_psrfits_fold(tmp_path):
    name = str(tmp_path / 'fold.fits')
    fold = bt.Fold(bt.Power(bt.Channelize(fits_source(), 16)), 8, lambda t: 1000. / 3. * (t - T0), step=1 << 9)
    assert fold.shape == (8, 8, 16, 4)
    with psrfits.open(name, 'w', template=fold) as fw:
        fold.read(out=fw)
    return lambda: psrfits.open(name)


def up_vdif(tmp_path):
    rng = np.random.default_rng(2)
    n, spf, fs = 8 * 640, 640, 32e6
    levels = np.array([-3.3359, -1., 1., 3.3359], np.float32)
    data = rng.choice(levels, size=(n, 2, 8)).view(np.complex64)
    raw = ingest.encode_vdif_frames(data, 2, seconds=100, ref_epoch=41, frame_nr0=49998, frames_per_second=50000,
                                    samples_per_frame=spf, edv=3, sample_rate=fs)
    return lambda: bt.open_vdif(raw, frequency=300 * u.MHz, sideband=1)


UPSTREAMS = {'Square': (up_square, 256), 'Power': (up_power, 256), 'Channelize': (up_channelize, 16),
             'Dedisperse': (up_dedisperse, None), 'Real2Complex': (up_real2complex, 256),
             'Transpose': (up_transpose, 256), 'Integrate': (up_integrate, 1), 'Fold': (up_fold, 1),
             'hdf5': (up_hdf5, 512), 'psrfits-search': (up_psrfits_search, 64), 'psrfits-fold': (up_psrfits_fold, 1),
             'vdif': (up_vdif, 640)}


def upstream(name, tmp_path):
    factory, spf = UPSTREAMS[name]
    make = factory(tmp_path)
    t = make()
    assert produces_on_device(t) and cache_producer(t) is t, name      # (a task with a frame cache of its own)
    assert spf is None or t.samples_per_frame == spf, (name, t.samples_per_frame)
    return make, t, t.samples_per_frame


# -- A. every upstream, through t[a:b], into Stack of two and of three windows ---------------------------
@pytest.mark.parametrize('n_win', [2, 3])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', list(UPSTREAMS))
def test_stack_of_windows_of_every_upstream(name, kind, n_win, tmp_path):
    make, t, spf = upstream(name, tmp_path)
    n, d = geometry(spf, kind)
    starts = [k * d for k in range(n_win)]
    check_geometry(kind, starts, n, spf)
    st = bt.Stack([window(t, a, n) for a in starts], axis=1)
    assert st.shape[0] == n and st._firsts == [0] * n_win
    want = np.stack([alone(make, a, n) for a in starts], axis=1)
    same(st.read(), want)


def test_bare_windows_are_lined_up_by_time(tmp_path):
    """``Stack([t[0:n], t[d:n + d]])`` as it stands: the streams are lined up by their times, so both
    inputs are the span the windows share and one range of ``t`` is fetched twice (a cache hit)."""
    make, t, spf = upstream('Square', tmp_path)
    n, d = geometry(spf, 'miss')
    st = bt.Stack([t[0:n], t[d:n + d]], axis=1)
    assert st.shape[0] == n - d and st._firsts == [d, 0]
    whole = make().read()
    same(st.read(), np.stack([whole[d:n], whole[d:n]], axis=1))


# -- B. every wrapper that hands views on, over Square ---------------------------------------------------
def square4(tmp_path=None):
    return bt.Square(device_stream(noise((4096, 2, 2)), 256, frequency=400e6, sideband=1))


WRAPPERS = {
    'time-slice': lambda t, a, n: relabelled(t, a)[a:a + n],
    'getslice-all': lambda t, a, n: relabelled(t, a)[a:a + n, :],
    'getslice-all-axes': lambda t, a, n: relabelled(t, a)[a:a + n, :, :],
    'reshape-same': lambda t, a, n: bt.Reshape(window(t, a, n), (2, 2)),
    'reshape-flat': lambda t, a, n: bt.Reshape(window(t, a, n), (4,)),
    'getitem-all': lambda t, a, n: bt.GetItem(window(t, a, n), (slice(None), slice(0, 2))),
    'transpose-identity': lambda t, a, n: bt.Transpose(window(t, a, n), (1, 2)),
    'setattribute': lambda t, a, n: relabelled(t, a, frequency=np.array([[1e9, 2e9]]), sideband=-1)[a:a + n],
    'three-deep': lambda t, a, n: bt.Reshape(bt.GetItem(relabelled(t[a:], 0, t.start_time)[:n, :], slice(None)), (4,)),
}


def check_hands_views_on(w, t):
    assert produces_on_device(w) and cache_producer(w) is t
    if isinstance(w, bt.ChangeSampleShapeBase):
        assert w.route is None
    assert w._view_source is not None


@pytest.mark.parametrize('kind', KINDS[1:])
@pytest.mark.parametrize('wrapper', list(WRAPPERS))
def test_every_wrapper_that_hands_views_on(wrapper, kind):
    wrap = WRAPPERS[wrapper]
    t = square4()
    n, d = geometry(256, kind)
    check_geometry(kind, [0, d], n, 256)
    ws = [wrap(t, a, n) for a in (0, d)]
    for w in ws:
        check_hands_views_on(w, t)
    st = bt.Stack(ws, axis=1)
    assert st.shape[0] == n
    want = np.stack([wrap(square4(), a, n).read() for a in (0, d)], axis=1)
    same(st.read(), want)


@pytest.mark.parametrize('kind', KINDS[1:])
def test_bare_task_with_a_wrapped_window_of_it(kind):
    """One input is ``t`` itself, the other ``t[d:]`` under a reshape."""
    t = square4()
    n, d = geometry(256, kind)
    stop = None if kind == 'miss' else d + n         # (t[d:] to the end; for the straddle, a window's length)
    length = (t.shape[0] if stop is None else stop) - d
    check_geometry(kind, [0, d], length, 256)
    w = bt.Reshape(relabelled(t, d)[d:stop], (2, 2))
    check_hands_views_on(w, t)
    st = bt.Stack([t, w], axis=1)
    assert st.shape[0] == length and st._firsts == [0, 0]
    whole = square4().read()
    same(st.read(), np.stack([whole[:length], whole[d:d + length]], axis=1))


# -- C. every combiner ---------------------------------------------------------------------------------------
def reverse(data):
    return np.stack(data[::-1], axis=1)


def outer_two(data):
    return np.stack([data[0], data[2]], axis=-1)


COMBINERS = {
    'Stack': (2, lambda ws: bt.Stack(ws, axis=1), lambda xs: np.stack(xs, axis=1)),
    'Stack-last-axis': (3, lambda ws: bt.Stack(ws, axis=-1), lambda xs: np.stack(xs, axis=-1)),
    'Concatenate': (2, lambda ws: bt.Concatenate(ws, axis=1), lambda xs: np.concatenate(xs, axis=1)),
    'CombineStreams-reversed': (3, lambda ws: bt.CombineStreams(ws, reverse), reverse),
    'CombineStreams-one-unused': (3, lambda ws: bt.CombineStreams(ws, outer_two), outer_two),
}


@pytest.mark.parametrize('combiner', list(COMBINERS))
def test_every_combiner(combiner, tmp_path):
    n_win, build, numpy_twin = COMBINERS[combiner]
    make, t, spf = upstream('Square', tmp_path)
    n, d = geometry(spf, 'miss')
    starts = [k * d for k in range(n_win)]
    fetched = starts if combiner != 'CombineStreams-one-unused' else starts[::2]
    assert 'inside' not in fetch_relations(fetched, n, spf)
    if fetched is starts:
        check_geometry('miss', starts, n, spf)
    task = build([window(t, a, n) for a in starts])
    assert task.shape[0] == n
    same(task.read(), numpy_twin([alone(make, a, n) for a in starts]))


def test_the_same_task_twice(tmp_path):
    make, t, spf = upstream('Square', tmp_path)
    whole = make().read()
    same(bt.Stack([t, t], axis=1).read(), np.stack([whole, whole], axis=1))
    same(bt.Concatenate([t, t[:], t], axis=1).read(), np.concatenate([whole] * 3, axis=1))


# -- D. read patterns on the combined task -----------------------------------------------------------------
def read_whole(st, t, n, spf):
    return st.read()


def read_pieces(st, t, n, spf):
    step = max(6 * spf // 10, 1)
    return np.concatenate([st.read(min(step, n - at)) for at in range(0, n, step)])


def read_on_device(st, t, n, spf):
    return st.read_device().to_host()


def read_again_after_a_seek(st, t, n, spf):
    first = st.read(n // 2 + 1)
    st.seek(spf // 3)
    rest = st.read(n - spf // 3)
    same(first[spf // 3:], rest[:first.shape[0] - spf // 3])
    st.seek(-(n // 3), 2)
    same(st.read(), rest[-(n // 3):])
    st.seek(0)
    return np.concatenate([st.read(spf // 3), rest])


def read_frame_by_frame(st, t, n, spf):
    st.max_frames_per_call = 1
    return st.read()


def read_upstream_frame_by_frame(st, t, n, spf):
    t.max_frames_per_call = 1
    return st.read()


def read_piecewise(st, t, n, spf):
    """More than ``max_frames_per_call + 2`` frames in one request: `read_device` assembles a fresh array
    run by run."""
    st.max_frames_per_call = 1
    assert frames(0, n, st.samples_per_frame)[1] > st.max_frames_per_call + 2
    return st.read_device().to_host()


#: name -> (reader, samples per frame of the combining task: None for the upstream's, or a function of
#: the upstream's that gives a number it is no multiple of)
PATTERNS = {'whole': (read_whole, None), 'pieces': (read_pieces, None), 'read_device': (read_on_device, None),
            'seek-back': (read_again_after_a_seek, None),
            'frames-of-700': (read_pieces, lambda spf: 700 if spf % 700 else 701),
            'combine-frame-by-frame': (read_frame_by_frame, None),
            'upstream-frame-by-frame': (read_upstream_frame_by_frame, None),
            'piecewise': (read_piecewise, lambda spf: spf // 2 + 1),
            'piecewise-frames-of-700': (read_piecewise, lambda spf: 700 if spf > 2800 else 100)}
_expected = {}


def expected_stack(name, make, starts, n):
    """The NumPy stack of privately built branches read alone: made once for every pattern."""
    key = (name, len(starts))
    if key not in _expected:
        _expected[key] = np.stack([alone(make, a, n) for a in starts], axis=1)
    return _expected[key]


@pytest.mark.parametrize('n_win', [2, 3])
@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('name', ['Square', 'Dedisperse'])
def test_read_patterns(name, pattern, n_win, tmp_path):
    reader, frame = PATTERNS[pattern]
    make, t, spf = upstream(name, tmp_path)
    n, d = geometry(spf, 'miss')
    starts = [k * d for k in range(n_win)]
    check_geometry('miss', starts, n, spf)
    frame = frame(spf) if callable(frame) else frame
    assert frame is None or spf % frame
    st = bt.Stack([window(t, a, n) for a in starts], axis=1, samples_per_frame=frame)
    assert st.shape[0] == n
    same(reader(st, t, n, spf), expected_stack(name, make, starts, n))


# -- E. diamonds: two consumers of one task, read in turn --------------------------------------------------
def read_in_turn(streams, wants, seed):
    """Uneven pieces of the streams in turn, with seeks, on the host and on the device."""
    rng = np.random.default_rng(seed)
    for k in range(16):
        which = (k + (k % 5 == 4)) % len(streams)
        s, want = streams[which], wants[which]
        assert s.shape == want.shape
        if k % 3 == 2 or s.tell() == s.shape[0]:
            s.seek(int(rng.integers(0, s.shape[0] - 1)))
        at = s.tell()
        count = min(s.shape[0] - at, max(1, int(s.shape[0] * rng.uniform(0.03, 0.3))))
        got = s.read(count) if k % 4 else s.read_device(count).to_host()
        same(got, want[at:at + count])


def test_diamond_of_power_and_a_channel_range():
    ch = channelized(1 << 14)
    pair = [bt.Power(ch), ch[:, 3:11]]
    assert pair[1].route is not None and cache_producer(pair[1]) is pair[1]
    wants = [bt.Power(channelized(1 << 14)).read(), channelized(1 << 14)[:, 3:11].read()]
    assert wants[0].shape == (1024, 16, 4) and wants[1].shape == (1024, 8, 2)
    read_in_turn(pair, wants, 1)


def test_diamond_of_fold_and_integrate():
    def branches(ch_a, ch_b):
        return [bt.Fold(bt.Square(ch_a), 8, lambda t: 62500. / 16. * (t - T0), step=64), bt.Integrate(bt.Power(ch_b), 4)]
    ch = channelized(1 << 14)
    wants = [b.read() for b in branches(channelized(1 << 14), channelized(1 << 14))]
    assert wants[0].shape == (16, 8, 16, 2) and wants[1].shape == (256, 16, 4)
    read_in_turn(branches(ch, ch), wants, 2)


def real_to_complex():
    ds = device_stream(noise((1 << 17, 2), 'f4'), 8192, frequency=300e6, sideband=1)
    return bt.Real2Complex(ds, samples_per_frame=4096)


def dedispersed(r, dm):
    return bt.Dedisperse(r, dm, samples_per_frame=dedisperse_frame(r, dm))


def test_diamond_of_two_dedispersions():
    r = real_to_complex()
    assert r.shape == (1 << 16, 2)
    wants = [dedispersed(real_to_complex(), dm).read() for dm in (10., 7.)]
    assert wants[0].shape != wants[1].shape
    read_in_turn([dedispersed(r, 10.), dedispersed(r, 7.)], wants, 3)


@pytest.mark.parametrize('kind', KINDS)
def test_stack_of_three_dedispersions_of_one_task(kind):
    """Every branch has a deferred call that reads the shared `Real2Complex` cache while the next
    branch refills it; the branches' own caches are distinct (no copies)."""
    r = real_to_complex()
    branches = [dedispersed(r, 10.) for _ in range(3)]
    spf = branches[0].samples_per_frame
    n, d = geometry(spf, kind)
    starts = [0, d, 2 * d]
    check_geometry(kind, starts, n, spf)
    st = bt.Stack([window(b, a, n) for b, a in zip(branches, starts)], axis=1)
    assert st.shape[0] == n
    want = np.stack([alone(lambda: dedispersed(real_to_complex(), 10.), a, n) for a in starts], axis=1)
    same(st.read(), want)
    st.seek(0)
    same(read_pieces(st, None, n, spf), want)


def test_stack_of_two_dispersion_measures_of_one_task():
    r = real_to_complex()
    pair = [dedispersed(r, 10.), dedispersed(r, 7.)]
    spf = pair[0].samples_per_frame
    n, d = geometry(spf, 'miss')
    st = bt.Stack([window(pair[0], 0, n), window(pair[1], d, n, start=pair[0].start_time)], axis=1)
    assert st.shape[0] == n and st._firsts == [0, 0]
    want = np.stack([alone(lambda: dedispersed(real_to_complex(), 10.), 0, n),
                     alone(lambda: dedispersed(real_to_complex(), 7.), d, n)], axis=1)
    same(st.read(), want)


# -- copies are made where a producer is shared, and only there ----------------------------------------
@pytest.fixture
def copies(monkeypatch):
    made = []
    plain = hip.DeviceArray.copy_from_device

    def counted(self, other):
        made.append(self.nbytes)
        return plain(self, other)
    monkeypatch.setattr(hip.DeviceArray, 'copy_from_device', counted)
    return made


def test_inputs_with_distinct_producers_are_not_copied(copies, tmp_path):
    make, t, spf = upstream('Square', tmp_path)
    n, d = geometry(spf, 'miss')
    others = [make(), make()]
    ds = device_stream(noise((4096, 2), 'f4', seed=5), 256)
    ins = [window(t, 0, n), window(others[0], d, n), window(others[1], 2 * d, n),
           window(ds, d, n), window(ds, 2 * d, n)]          # (and a resident stream twice: nothing to guard)
    st = bt.Stack(ins, axis=1)
    assert st._keep is None
    del copies[:]
    got = st.read()
    assert copies == [] and st._keep == [False] * 5
    st.seek(0)
    view = st.read_device()
    assert copies == []
    whole, flat = make().read(), noise((4096, 2), 'f4', seed=5)
    want = np.stack([whole[0:n], whole[d:d + n], whole[2 * d:2 * d + n], flat[d:d + n], flat[2 * d:2 * d + n]], axis=1)
    same(got, want)
    same(view.to_host(), want)


@pytest.mark.parametrize('n_win', [2, 3])
def test_inputs_that_share_a_producer_are_copied_but_for_the_last(copies, n_win, tmp_path):
    make, t, spf = upstream('Square', tmp_path)
    n, d = geometry(spf, 'miss')
    starts = [k * d for k in range(n_win)]
    st = bt.Stack([window(t, a, n) for a in starts], axis=1)
    del copies[:]
    got = st.read()
    assert st._keep == [True] * (n_win - 1) + [False]
    assert copies == [n * 2 * 4] * (n_win - 1)              # (whole windows of two float32 a sample)
    same(got, np.stack([alone(make, a, n) for a in starts], axis=1))
