"""Parity of the HIP path with the CPU oracle (and the committed reference
vectors) -- the `-m gpu` suite.  Every GPU result is produced through the
package's task classes, i.e. through the C ABI of libbbt_hip.so.

Tolerances (float32 arithmetic against a float64-FFT
oracle):  relative L2 <= 1e-6  and  max|delta| <= 1e-5 * rms(oracle).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u
from baseband_tasks_amd.fourier import HipFFTMaker
from oracle import bbt_oracle as orc
from conftest import rel_l2, max_over_rms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_L2_TOL = 1e-6
MAX_TOL = 1e-5
T0 = '2020-01-01T00:00:00'


def assert_parity(got, want, what=''):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.dtype == np.complex64
    e2, em = rel_l2(got, want), max_over_rms(got, want)
    assert e2 <= REL_L2_TOL and em <= MAX_TOL, (what, e2, em)


def noise(n, sample_shape, spf, seed=12345, fs=16 * u.MHz, **kw):
    return bt.NoiseGenerator((n,) + tuple(sample_shape), T0, fs, spf, seed=seed, **kw)


@pytest.fixture(scope='module', autouse=True)
def _need_gpu():
    if not bt.hip.available():
        pytest.fail("no GPU / libbbt_hip.so: the -m gpu suite must run on an MI355X")


# --------------------------------------------------------------------------- config 1
@pytest.mark.parametrize('spf', [1, 16, 33])
def test_config1_channelize(golden, spf):
    nh = noise(2**20, (2,), 2**20, frequency=1000 * u.MHz, sideband=1)
    ch = bt.Channelize(nh, 1024, samples_per_frame=spf)
    z = ch.read()
    x = orc.noise_stream(12345, 0, 2**20, 2**20, (2,))
    want = orc.channelize(x[:(2**20 // (1024 * spf)) * 1024 * spf], 1024)
    assert_parity(z, want, 'channelize')
    assert_parity(z[:4], golden['c1_head'], 'golden head')
    if spf in (1, 16):
        assert_parity(z[-4:], golden['c1_tail'], 'golden tail')
    assert ch.frequency[512, 0] == 992e6
    assert ch.sample_rate == 16e6 / 1024


# --------------------------------------------------------------------------- config 2
def test_config2_dedisperse_and_metric_pipeline(golden):
    nh = noise(4 * 2**20, (2,), 2**20, frequency=1000 * u.MHz, sideband=1)
    dd = bt.Dedisperse(nh, 100.)
    assert (dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame) == \
        (104963, 107513, 2**20, 836100)
    y = dd.read()
    x = orc.noise_stream(12345, 0, 4 * 2**20, 2**20, (2,))
    want, info = orc.dedisperse(x, 16e6, 1000., 1, 100., ih_samples_per_frame=2**20)
    assert_parity(y, want, 'dedisperse')
    spf = 836100
    for name, sl in (('c2_head', slice(0, 2048)), ('c2_seam1', slice(spf - 1024, spf + 1024)),
                     ('c2_seam_last', slice(3 * spf - 1024, 3 * spf + 1024)),
                     ('c2_tail', slice(-2048, None))):
        assert_parity(y[sl], golden[name], name)
    # the metric pipeline
    dd.seek(0)
    ch = bt.Channelize(dd, 1024, samples_per_frame=512)
    z = ch.read()
    assert list(z.shape) == list(golden['c2ch_shape'])
    wantz = orc.channelize(want[:z.shape[0] * 1024], 1024)
    assert_parity(z, wantz, 'dedisperse->channelize')
    k = spf // 1024
    assert_parity(z[:2], golden['c2ch_head'], 'golden head')
    assert_parity(z[k - 1:k + 2], golden['c2ch_seam'], 'golden seam')
    assert_parity(z[-2:], golden['c2ch_tail'], 'golden tail')


def test_fused_channelizer_short_final_frame():
    """The last dedispersion frame keeps fewer samples than one spectrum: that
    call takes the unfused route, everything else stays fused."""
    n_fft, pad = 2**15, 767 + 771                  # (16 x 2048: the shortest blocks with a row pass to fuse into)
    spf = n_fft - pad
    n_in = 3 * spf + pad + 100                      # dedispersed length 3 * spf + 100
    nh = noise(n_in, (2,), 5000, seed=31, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
    x = orc.noise_stream(31, 0, n_in, 5000, (2,))
    dd = bt.Dedisperse(nh, 5., samples_per_frame=spf)
    assert dd.shape[0] == 3 * spf + 100 and dd._ih_samples_per_frame == n_fft
    ch = bt.Channelize(dd, 256, samples_per_frame=1)
    assert ch._fusable_input() is dd
    z = ch.read()
    y, _ = orc.dedisperse(x, 1e6, 300., 1, 5., samples_per_frame=spf, ih_samples_per_frame=5000,
                          fast_len=HipFFTMaker.next_fast_len)
    assert z.shape[0] == (3 * spf + 100) // 256
    assert_parity(z, orc.channelize(y[:z.shape[0] * 256], 256), 'short final frame')


def test_config2_device_resident_chain_matches_host_chain():
    nh = noise(3 * 2**20, (2,), 2**20, frequency=1000 * u.MHz, sideband=1)
    ds = bt.DeviceStream(nh, T0, 16 * u.MHz)
    assert np.all(ds.frequency == nh.frequency)
    z_dev = bt.Channelize(bt.Dedisperse(ds, 100.), 1024, 64).read()
    z_host = bt.Channelize(bt.Dedisperse(nh, 100.), 1024, 64).read()
    assert np.array_equal(z_dev, z_host)
    # read_device hands back HBM, bit-identical to read()
    ch = bt.Channelize(bt.Dedisperse(ds, 100.), 1024, 64)
    zd = ch.read_device(128)
    assert isinstance(zd, bt.hip.DeviceArray) and zd.shape == (128, 1024, 2)
    assert np.array_equal(zd.to_host(), z_host[:128])


def test_host_path_pipelined_reads_are_bit_identical(monkeypatch):
    """The host path of ``read`` (host_pipeline.py: upload of run m + 1, transforms of run m,
    download of run m - 1 at once; page-locked staging and result) returns exactly what the
    synchronous path returns -- for a NumPy-backed stream read straight out of pinned memory
    (`HostStream`), for a reader that has to be read into staging memory (`StreamGenerator`), for
    the fused metric pipeline, the plain task, a resampler in front, and reads that start and end
    inside frames.  Reference: Base.read, base.py:389-438."""
    from baseband_tasks_amd import host_pipeline as hp
    n_fft, pad = 2**14, 767 + 771
    spf = n_fft - pad
    n_in = 23 * spf + pad + 321
    rng = np.random.default_rng(8)
    x = rng.standard_normal((n_in, 4), dtype=np.float32).view(np.complex64)
    kw = dict(frequency=300 * u.MHz, sideband=1)

    def sources():
        yield 'HostStream', bt.HostStream(x.copy(), T0, 1 * u.MHz, samples_per_frame=5000, **kw)
        yield 'pinned HostStream', bt.HostStream(hp.pinned_empty(x.shape, x.dtype), T0, 1 * u.MHz,
                                                 samples_per_frame=5000, **kw)
        yield 'StreamGenerator', bt.StreamGenerator(
            lambda fh: x[fh.tell():fh.tell() + fh.samples_per_frame], x.shape, T0, 1 * u.MHz,
            samples_per_frame=5000, dtype=np.complex64, **kw)

    def chains(src):
        yield 'dedisperse', bt.Dedisperse(src, 5., samples_per_frame=spf)
        yield 'fused', bt.Channelize(bt.Dedisperse(src, 5., samples_per_frame=spf), 256, samples_per_frame=8)
        yield 'resample+dedisperse', bt.Dedisperse(bt.Resample(src, 0.25, pad=32, samples_per_frame=4000),
                                                   5., samples_per_frame=spf)

    if not hp.ENABLED:
        pytest.skip('host pipeline switched off (BBT_HOST_PIPELINE=0)')
    for sname, src in sources():
        if sname == 'pinned HostStream':
            src._data[...] = x
            assert src.host_view(0, 10) is not None and hp.is_pinned(src._data)
        for cname, task in chains(src):
            task.max_frames_per_call = 4
            if cname == 'resample+dedisperse':
                task.ih.seek(0)
                task.ih.max_frames_per_call = 3
            task.seek(0)
            got = task.read()
            assert hp.is_pinned(got), (sname, cname)
            # the synchronous route: an ordinary (pageable) result array
            task.invalidate_cache()
            task.seek(0)
            plain = task.read(out=np.empty(got.shape, got.dtype))
            assert np.array_equal(got, plain), (sname, cname)
            # pieces that start and end inside frames, across many runs
            task.invalidate_cache()
            k = 1 if got.ndim == 2 else 0
            lo = 3 * task.samples_per_frame + 5 + k
            cnt = 11 * task.samples_per_frame + 7
            task.seek(lo)
            assert np.array_equal(task.read(cnt), got[lo:lo + cnt]), (sname, cname)
            task.close()
    # and the result arrays' memory goes back to the pool when they are dropped
    a = hp.pinned_empty((1 << 20,), np.float32)
    address = a.ctypes.data
    del a
    assert any(address in stack for stack in hp._pool.free.values())
    assert hp.pinned_empty((1 << 20,), np.float32).ctypes.data == address


def test_host_path_upload_never_lands_in_a_block_still_being_read():
    """The window of VERDICT r03 weak point 6, forced: a slow host reader (every ``read`` sleeps a
    millisecond, so the worker takes its time), runs of ONE 2^20-sample frame (the input of run m
    is freed while its kernels are still queued, and has exactly the size the upload of run m + 1
    asks the pool for), pipelined against synchronous: same bits, and one load per run."""
    import time
    from baseband_tasks_amd import host_pipeline as hp
    if not hp.ENABLED:
        pytest.skip('host pipeline switched off (BBT_HOST_PIPELINE=0)')
    n_fft = 2**20
    dd0 = bt.Dedisperse(bt.EmptyStreamGenerator((4 * n_fft, 2), T0, 16 * u.MHz, samples_per_frame=n_fft,
                                                dtype=np.complex64, frequency=1000 * u.MHz, sideband=1), 100.)
    spf = dd0.samples_per_frame
    n_in = 9 * spf + (n_fft - spf)
    rng = np.random.default_rng(19)
    x = rng.standard_normal((n_in, 4), dtype=np.float32).view(np.complex64)

    def slow(fh):
        time.sleep(1e-3)
        return x[fh.tell():fh.tell() + fh.samples_per_frame]

    def task():
        src = bt.StreamGenerator(slow, x.shape, T0, 16 * u.MHz, samples_per_frame=2**16, dtype=np.complex64,
                                 frequency=1000 * u.MHz, sideband=1)
        ch = bt.Channelize(bt.Dedisperse(src, 100., samples_per_frame=spf), 1024, samples_per_frame=spf // 1024)
        ch.max_frames_per_call = ch.ih.max_frames_per_call = 1
        return src, ch
    src, ch = task()
    got = ch.read()
    assert hp.is_pinned(got)
    assert hp.uploader_for(src).loads == -(-got.shape[0] // ch.samples_per_frame)
    src2, ch2 = task()
    plain = ch2.read(out=np.empty(got.shape, got.dtype))          # (pageable result: synchronous copies)
    assert np.array_equal(got, plain)
    want, _ = orc.dedisperse(x[:2 * n_fft], 16e6, 1000., 1, 100., samples_per_frame=spf, ih_samples_per_frame=n_fft)
    # (the oracle on the first two blocks only: its second block is then the stream's re-aligned
    # last one, so just the first frame is comparable)
    nz = spf // 1024
    assert_parity(got[:nz], orc.channelize(want[:nz * 1024], 1024), 'slow reader, runs of one frame')


def test_deferred_calls_do_not_let_the_upstream_task_overwrite_what_the_lanes_still_read(monkeypatch):
    """Plan calls are issued with a deferred join (hip.DEFER_JOIN): the stream is not ordered after
    the lanes.  The input of such a call is the upstream task's cache, which that task fills again
    for the next run -- on the stream, i.e. possibly while the lanes of the previous run still read
    it.  The call's completion event therefore stays with the INPUT's allocation too, and the
    upstream task waits for it (or switches to its second buffer) before it writes.  A direct filter (a single kernel on the stream)
    in front of a dedispersion on 2^20-sample blocks, read run after run: same bits as with every
    call joined."""
    n_fft = 2**20
    rng = np.random.default_rng(33)
    x = rng.standard_normal((14 * n_fft, 4), dtype=np.float32).view(np.complex64)
    taps = rng.standard_normal(9).astype(np.float32)
    ds = bt.DeviceStream(x, T0, 16 * u.MHz, samples_per_frame=n_fft, frequency=1000 * u.MHz, sideband=1)

    def chain():
        cv = bt.Convolve(ds, taps, samples_per_frame=n_fft)
        assert cv._use_fir()
        dd = bt.Dedisperse(cv, 100.)
        cv.max_frames_per_call = 6
        dd.max_frames_per_call = 4
        return cv, dd
    if not bt.hip.DEFER_JOIN:
        pytest.skip('deferred joins switched off (BBT_DEFER=0)')
    cv, dd = chain()
    pieces, buffers, starts = [], set(), []
    dd.seek(0)
    while dd.tell() < dd.shape[0]:
        starts.append(dd.tell())
        # (nothing touches a piece before the next run is queued: the window stays open)
        pieces.append(dd.read_device(min(4 * dd.samples_per_frame, dd.shape[0] - dd.tell())))
        buffers.add(dd._cache_buffer._ptr)
    assert len(pieces) >= 4 and len(buffers) == 2          # (the cache alternates while a call is owed)
    last_two = [p.to_host() for p in pieces[-2:]]           # (earlier ones have been overwritten since)
    monkeypatch.setattr(bt.hip, 'DEFER_JOIN', False)
    cv, dd = chain()
    whole = dd.read()
    for piece, start in zip(last_two, starts[-2:]):
        assert np.array_equal(piece, whole[start:start + piece.shape[0]])


def test_pipeline_output_into_the_hdf5_sink(tmp_path):
    """SURVEY 8f rank 3, downstream side: a task's output goes into the reference's intermediate HDF5
    format the way the reference writes it -- ``task.read(out=writer)``, the writer taking slices in order
    (io/hdf5/base.py:102-126) -- for spectra and for detected, integrated power; read back, the samples
    and the header are the task's."""
    from baseband_tasks_amd import hdf5
    n_fft, pad = 2**14, 767 + 771
    nh = noise(9 * (n_fft - pad) + pad, (2,), 5000, seed=41, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
    ch = bt.Channelize(bt.Dedisperse(nh, 5., samples_per_frame=n_fft - pad), 256, samples_per_frame=4)
    pw = bt.Integrate(bt.Power(bt.SetAttribute(ch, polarization=np.array(['X', 'Y']))), 8)
    for task in (ch, pw):
        task.seek(0)
        want = task.read()
        name = str(tmp_path / f'{type(task).__name__}.h5')
        task.seek(0)
        with hdf5.open(name, 'w', template=task) as fw:
            task.read(out=fw)
            assert fw.tell() == task.shape[0]
        fr = hdf5.open(name)
        assert fr.shape == task.shape and fr.dtype == task.dtype
        assert abs(fr.sample_rate - task.sample_rate) < 1e-9 * task.sample_rate
        assert abs(fr.start_time - task.start_time) < 1e-9
        assert np.array_equal(fr.read(), want)
        assert np.allclose(np.ravel(fr.frequency), np.ravel(np.broadcast_to(task.frequency, fr.frequency.shape)))
        fr.close()


def test_fused_and_unfused_channelizer_agree(golden, monkeypatch):
    """Channelize on top of a GPU overlap-save task folds its FFT into that
    task's row pass; both routes must match the oracle (and each other to
    rounding), for aligned and unaligned framings, seams included."""
    from baseband_tasks_amd import channelize as chmod
    nh = noise(4 * 2**20, (2,), 2**20, frequency=1000 * u.MHz, sideband=1)
    x = orc.noise_stream(12345, 0, 4 * 2**20, 2**20, (2,))
    want_y, _ = orc.dedisperse(x, 16e6, 1000., 1, 100., ih_samples_per_frame=2**20)
    results = {}
    for fuse in (True, False):
        monkeypatch.setattr(chmod, 'FUSE_WITH_OVERLAP_SAVE', fuse)
        for n, spf in ((1024, 512), (4096, 7), (256, 1000)):
            ch = bt.Channelize(bt.Dedisperse(nh, 100.), n, samples_per_frame=spf)
            assert (ch._fusable_input() is not None) == fuse
            z = ch.read()
            want = orc.channelize(want_y[:z.shape[0] * n], n)
            assert_parity(z, want, f'fuse={fuse} n={n}')
            # random access into the middle, across a block seam
            k = 836100 // n
            ch.seek(k - 3)
            assert np.array_equal(ch.read(7), z[k - 3:k + 4])
            results[fuse, n] = z
    for n in (1024, 4096, 256):
        # (each route is within 1e-6 of the oracle above; between themselves the two differ by
        # their independent rounding -- the plain route applies its inverse four-step twiddles in
        # the last column pass, the fused route in the row pass: up to 4.6e-7 measured in round 3)
        assert rel_l2(results[True, n], results[False, n]) < 6e-7
    # small geometry: N1 = 16 column pass, two sidebands, Convolve upstream
    nh = noise(60000, (2,), 20000, seed=11, fs=1 * u.MHz, frequency=300 * u.MHz,
               sideband=np.array([1, -1]))
    xs = orc.noise_stream(11, 0, 60000, 20000, (2,))
    pow2 = HipFFTMaker(power_of_two=True)         # (the fused route needs power-of-two blocks)
    ys, info = orc.dedisperse(xs, 1e6, 300., np.array([1, -1]), 5., ih_samples_per_frame=20000,
                              fast_len=pow2.next_fast_len)
    monkeypatch.setattr(chmod, 'FUSE_WITH_OVERLAP_SAVE', True)
    with bt.fft_maker.set(pow2):
        ch = bt.Channelize(bt.Dedisperse(nh, 5.), 256, samples_per_frame=5)
    assert ch._fusable_input() is not None and info['ih_spf'] == 32768
    z = ch.read()
    assert_parity(z, orc.channelize(ys[:z.shape[0] * 256], 256), 'fused small')


@pytest.mark.parametrize('n_stream', [2, 16, 66])
@pytest.mark.parametrize('n_chan', [2, 4, 8])
@pytest.mark.parametrize('n_fft', [2**14, 2**15, 2**16, 2**18])
def test_very_few_channels_fused_into_16_column_plans(n_stream, n_chan, n_fft, monkeypatch):
    """`Channelize(2 ... 8)` behind `Dedisperse` on 2^14 ... 2^16-sample blocks (the CHIME-native
    form of config 4, SURVEY 8d: Channelize(4) on the defaults' 2^16-sample blocks; reference
    channelize.py:73-74) is the lane butterflies of the row pass: fused and unfused routes against
    the oracle, on one pair, on pairs in eights (the multi-pair column passes) and on an odd pair
    count; unaligned frames, so that spectra straddle block seams."""
    from baseband_tasks_amd import channelize as chmod
    if n_fft == 2**14 and n_stream != 16:
        pytest.skip('16384-sample blocks run in one kernel unless the stream pairs come in eights')
    if n_fft == 2**18 and n_stream == 66:
        pytest.skip('(kept small)')
    fs, fc, dm = 1 * u.MHz, 300 * u.MHz, 0.3 if n_fft == 2**14 else 1.0
    n_in = 3 * n_fft + 4321
    rng = np.random.default_rng(n_fft + n_stream + n_chan)
    x = rng.standard_normal((n_in, n_stream, 2), dtype=np.float32).view(np.complex64)[..., 0]
    pow2 = HipFFTMaker(power_of_two=True)
    probe = bt.Dedisperse(bt.DeviceStream(x, T0, fs, samples_per_frame=n_fft, frequency=fc, sideband=1), dm)
    pad = probe._pad_start + probe._pad_end
    assert pad < n_fft // 2
    y, info = orc.dedisperse(x, 1e6, 300., 1, dm, samples_per_frame=n_fft - pad, ih_samples_per_frame=n_fft)
    assert info['ih_spf'] == n_fft
    got = {}
    for fuse in (True, False):
        monkeypatch.setattr(chmod, 'FUSE_WITH_OVERLAP_SAVE', fuse)
        dd = bt.Dedisperse(bt.DeviceStream(x, T0, fs, samples_per_frame=n_fft, frequency=fc, sideband=1), dm,
                           samples_per_frame=n_fft - pad)
        assert dd._ih_samples_per_frame == n_fft and dd._get_plan().info()['n1'] == (16 if n_fft <= 2**16 else 256)
        ch = bt.Channelize(dd, n_chan, samples_per_frame=1000)
        assert (ch._fusable_input() is not None) == fuse
        z = ch.read()
        assert_parity(z, orc.channelize(y[:z.shape[0] * n_chan], n_chan), f'fuse={fuse} {n_stream} streams n={n_chan}')
        k = (n_fft - pad) // n_chan                      # across the first block seam
        ch.seek(k - 5)
        assert np.array_equal(ch.read(11), z[k - 5:k + 6])
        got[fuse] = z
    assert rel_l2(got[True], got[False]) < 6e-7


# --------------------------------------------------------------------------- config 3
def test_config3_polyphase_filter_bank(golden):
    nh = noise(2 * 2**20, (2,), 2**20, frequency=1000 * u.MHz, sideband=1)
    resp = bt.sinc_hamming(12, 1024)
    pfb = bt.PolyphaseFilterBank(nh, resp)
    assert [pfb.padded._pad_start, pfb.padded._pad_end, pfb.padded._ih_samples_per_frame,
            pfb.padded.samples_per_frame, pfb.samples_per_frame, pfb.shape[0]] == \
        list(golden['c3_geo'])
    assert abs((pfb.start_time - nh.start_time) * 16e6 - golden['c3_shift'][0]) < 1e-3
    z = pfb.read()
    x = orc.noise_stream(12345, 0, 2 * 2**20, 2**20, (2,))
    want, _ = orc.polyphase_filter_bank(x, orc.sinc_hamming(12, 1024), 2**20)
    assert_parity(z, want, 'pfb')
    k = pfb.samples_per_frame
    assert_parity(z[:3], golden['c3_head'], 'golden head')
    assert_parity(z[k - 1:k + 2], golden['c3_seam'], 'golden seam')
    assert_parity(z[-3:], golden['c3_tail'], 'golden tail')


@pytest.mark.parametrize('sample_shape', [(8, 2), (64, 2), (3, 2), (2,), (4, 2)])
@pytest.mark.parametrize('n_tap,n_chan', [(4, 1024), (12, 256), (16, 512), (16, 4096)])
def test_filter_bank_on_many_streams(sample_shape, n_tap, n_chan):
    """`PolyphaseFilterBank` broadcasts over the trailing sample axes (reference pfb.py:136-154).  From
    16 streams on -- and for 4096 channels, which have no sliding-window kernel -- the window is a
    streaming pass over whole rows and the transform follows in place (`k_pfb_fir_rows` + the
    channelizer; 6 streams: the one-pass kernels): both against the oracle,
    over more spectra than one sweep of the window pass (192) and a ragged last sweep."""
    if n_chan == 4096 and sample_shape[0] == 64:
        pytest.skip('(kept small)')
    n_spec = 192 + 37
    n_in = (n_spec + n_tap - 1) * n_chan
    rng = np.random.default_rng(n_chan + sample_shape[0])
    x = rng.standard_normal((n_in,) + sample_shape + (2,), dtype=np.float32).view(np.complex64)[..., 0]
    resp = bt.sinc_hamming(n_tap, n_chan)
    ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=n_in)
    pfb = bt.PolyphaseFilterBank(ds, resp, samples_per_frame=n_spec)
    z = pfb.read()
    flat = x.reshape(n_in, -1)
    want, _ = orc.polyphase_filter_bank(flat, orc.sinc_hamming(n_tap, n_chan), n_in, samples_per_frame=n_spec)
    want = want.reshape((want.shape[0], n_chan) + sample_shape)
    assert z.shape == want.shape
    assert_parity(z, want, f'pfb {n_tap} x {n_chan} on {sample_shape}')


@pytest.mark.parametrize('route', [dict(BBT_PFB_TWO_PASS='1'), dict(BBT_PFB_TWO_PASS='0'), dict(BBT_PFB_PP='4'),
                                   dict(BBT_PFB_PP='4', BBT_PFB_GL='4'), dict(BBT_PFB_PP='8'),
                                   dict(BBT_PFB_PP='8', BBT_PFB_GL='1'), dict(BBT_PFB_TUNE='0'), {}],
                         ids=lambda r: '-'.join(f'{k[8:]}{v}' for k, v in r.items()) or 'timed')
@pytest.mark.parametrize('n_tap,n_chan', [(4, 1024), (12, 256), (16, 512), (8, 2048)])
def test_filter_bank_routes_on_many_streams(route, n_tap, n_chan, monkeypatch):
    """A filter-bank plan on 8 streams and more times its routes and keeps the fastest (bbt_hip.hip
    pfb_pick): two passes, one pair per workgroup, or 4 / 8 neighbouring pairs per workgroup with the
    lanes over the pairs first, in two orders of the workgroups.  Every route forced in turn, on
    32 streams and a ragged number of spectra, against the oracle (reference pfb.py:91-100,
    136-154)."""
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    sample_shape = (16, 2)
    n_spec = 192 + 37
    n_in = (n_spec + n_tap - 1) * n_chan
    rng = np.random.default_rng(n_chan + n_tap)
    x = rng.standard_normal((n_in,) + sample_shape + (2,), dtype=np.float32).view(np.complex64)[..., 0]
    pfb = bt.PolyphaseFilterBank(bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=n_in), bt.sinc_hamming(n_tap, n_chan),
                                 samples_per_frame=n_spec)
    z = pfb.read()
    want, _ = orc.polyphase_filter_bank(x.reshape(n_in, -1), orc.sinc_hamming(n_tap, n_chan), n_in, samples_per_frame=n_spec)
    assert_parity(z, want.reshape((want.shape[0], n_chan) + sample_shape), f'pfb {n_tap} x {n_chan}, route {route}')


@pytest.mark.parametrize('route', [dict(BBT_PFB_PP='4'), dict(BBT_PFB_PP='4', BBT_PFB_GL='2'), dict(BBT_PFB_PP='8', BBT_PFB_GL='1'),
                                   dict(BBT_PFB_TWO_PASS='1')],
                         ids=lambda r: '-'.join(f'{k[8:]}{v}' for k, v in r.items()))
@pytest.mark.filterwarnings('ignore:task will be inefficient')
def test_filter_bank_routes_on_very_few_spectra(route, monkeypatch):
    """The several-pairs window kernels sweep 2048 / N spectra per workgroup (two for 1024 channels,
    eight for 256): streams with fewer spectra than one sweep, and one more than a sweep, on 16
    and 48 streams (the pair groups of the second do not fill the `GL` order evenly), against the
    oracle."""
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(5)
    for n_tap, n_chan in ((4, 1024), (12, 256), (8, 512)):
        for n_spec in (1, 2, 3, 9):
            for n_pair in (8, 24):
                n_in = (n_spec + n_tap - 1) * n_chan
                x = rng.standard_normal((n_in, n_pair, 2, 2), dtype=np.float32).view(np.complex64)[..., 0]
                pfb = bt.PolyphaseFilterBank(bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=n_in),
                                             bt.sinc_hamming(n_tap, n_chan), samples_per_frame=n_spec)
                z = pfb.read()
                want, _ = orc.polyphase_filter_bank(x.reshape(n_in, -1), orc.sinc_hamming(n_tap, n_chan), n_in,
                                                    samples_per_frame=n_spec)
                assert_parity(z, want.reshape((n_spec, n_chan, n_pair, 2)),
                              f'pfb {n_tap} x {n_chan}, {n_spec} spectra, {n_pair} pairs, route {route}')


# --------------------------------------------------------------------------- small, complete outputs
def test_small_dedisperse_two_sidebands_golden(golden):
    nh = noise(10000, (2,), 4000, seed=11, fs=1 * u.MHz, frequency=300 * u.MHz,
               sideband=np.array([1, -1]))
    dd = bt.Dedisperse(nh, 5., samples_per_frame=4096 - 767 - 771)
    assert [dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame,
            dd.shape[0], dd._sample_offset] == list(golden['sb_geo'])
    assert_parity(dd.read(), golden['sb_out'], 'sb')


@pytest.mark.parametrize('tag,kw', [('sa', {}), ('sc', dict(reference_frequency=300.4 * u.MHz)),
                                    ('sd', dict(reference_frequency=300.7 * u.MHz))])
def test_reference_default_geometry_golden(golden, tag, kw):
    """Default arguments give the reference's own block geometry -- here
    6174-sample blocks (2 x 3^2 x 7^3, fourier/numpy.py:99-126 via base.py:750-758)
    -- and the complete outputs the reference produced with it."""
    nh = noise(10000, (2,), 4000, seed=11, fs=1 * u.MHz, frequency=300 * u.MHz,
               sideband=np.array([1, -1]))
    dd = bt.Dedisperse(nh, 5., **kw)
    assert [dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame,
            dd.shape[0], dd._sample_offset] == list(golden[tag + '_geo'])
    assert dd._ih_samples_per_frame & (dd._ih_samples_per_frame - 1)       # not a power of two
    assert abs((dd.start_time - nh.start_time) * 1e6 - golden[tag + '_shift'][0]) < 1e-4
    assert_parity(dd.read(), golden[tag + '_out'], tag)


@pytest.mark.parametrize('n_fft', [6, 60, 210, 1000, 2187, 6174, 7203, 8192,           # one workgroup
                                   8232, 19200, 25725, 31104, 2 * 3**9, 131250, 1049760])  # two factors (short rows: several per workgroup)
def test_block_lengths_that_are_not_powers_of_two(n_fft):
    """Overlap-save blocks of every kind of 2^a 3^b 5^c 7^d length against the
    oracle (random response, so every bin matters; three streams)."""
    assert HipFFTMaker.next_fast_len(n_fft) == n_fft
    n_tap = max(2, min(n_fft // 3, 40000))
    rng = np.random.default_rng(n_fft)
    resp = (rng.standard_normal((n_tap, 3)) + 1j * rng.standard_normal((n_tap, 3))) / np.sqrt(n_tap)
    n_in = 2 * n_fft + n_fft // 2 + 5
    x = (rng.standard_normal((n_in, 6), dtype=np.float32)).view(np.complex64)
    ds = bt.DeviceStream(x, T0, 1 * u.MHz)
    limit = bt.Convolve.FIR_MAX_TAPS_COMPLEX
    bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0           # the Fourier-domain plan, not the direct FIR
    try:
        cv = bt.Convolve(ds, resp.astype(np.complex64), samples_per_frame=n_fft - n_tap + 1)
        assert cv._ih_samples_per_frame == n_fft
        got = cv.read()
    finally:
        bt.Convolve.FIR_MAX_TAPS_COMPLEX = limit
    want, info = orc.convolve(x, resp.astype(np.complex64), samples_per_frame=n_fft - n_tap + 1,
                              ih_samples_per_frame=1000)
    assert info['ih_spf'] == n_fft
    assert_parity(got, want, f'n_fft {n_fft}')


def test_lengths_that_are_not_powers_of_two_run_on_kernels_compiled_for_them():
    """The default path for such lengths: kernels specialised on the length when the plan is made
    (csrc/rtc.hpp; include/bbt_hip.h: bbt_rtc_info).  A length this process has not met yet costs
    one compilation, a second plan of the same length none; the result is the oracle's."""
    info = bt.hip.rtc_info()
    if info['mode'] == 'off':
        pytest.skip('BBT_RTC=0: the general kernels run every length')
    n_fft, n_tap = 2 * 3 * 5 * 7 * 7 * 3, 1470              # 4410: in no other test (more than 513 taps: no short-block plan)
    rng = np.random.default_rng(4410)
    resp = ((rng.standard_normal((n_tap, 1)) + 1j * rng.standard_normal((n_tap, 1))) / np.sqrt(n_tap)).astype(np.complex64)
    x = rng.standard_normal((3 * n_fft, 4), dtype=np.float32).view(np.complex64)
    limit = bt.Convolve.FIR_MAX_TAPS_COMPLEX
    bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0
    try:
        got = []
        for _ in range(2):
            cv = bt.Convolve(bt.DeviceStream(x, T0, 1 * u.MHz), resp, samples_per_frame=n_fft - n_tap + 1)
            assert cv._ih_samples_per_frame == n_fft
            got.append(cv.read())
            after = bt.hip.rtc_info()
            if len(got) == 1:
                assert after['modules'] == info['modules'] + 1 and after['seconds'] > info['seconds']
                first = after
            else:
                assert after['modules'] == first['modules']          # (cached: the same source text)
    finally:
        bt.Convolve.FIR_MAX_TAPS_COMPLEX = limit
    want, _ = orc.convolve(x, resp, samples_per_frame=n_fft - n_tap + 1, ih_samples_per_frame=1000)
    assert_parity(got[0], want, 'n_fft 4410, specialised kernels')
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize('mode, points', [('0', None), ('require', None), ('require', 10), ('require', 16), ('require', 20),
                                          ('require', 116)])
def test_general_and_specialised_kernels_agree_with_the_oracle(mode, points):
    """BBT_RTC=0 keeps every such length on the general kernels (the fall-back when hipRTC is not
    available), BBT_RTC=require makes a failing compilation an error: one child process each runs
    one-kernel and two-level blocks, several streams, and channel counts either side of the
    engines' ranges, against the oracle.  A channelizer plan keeps the fastest of its candidates
    (bbt_hip.hip chan_pick); with `points` the timing is off and every channel count runs on the
    kernels compiled for that many points per thread, so that each candidate is checked (116: 16
    points in the `wide` form, as many stream pairs per workgroup as fit 1024 threads)."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u
from oracle import bbt_oracle as orc
assert bt.hip.rtc_info()['mode'] == %r
worst = 0.
def check(got, want):
    global worst
    err = np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel())
    assert err < 1e-6, err
    worst = max(worst, err)
bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0
for n_fft, n_stream in ((630, 2), (6174, 4), (25725, 2), (131250, 6)) if %r else ():
    n_tap = max(2, min(n_fft // 3, 5000))
    rng = np.random.default_rng(n_fft)
    resp = ((rng.standard_normal((n_tap, n_stream)) + 1j * rng.standard_normal((n_tap, n_stream))) / np.sqrt(n_tap)).astype(np.complex64)
    x = rng.standard_normal((2 * n_fft + 77, 2 * n_stream), dtype=np.float32).view(np.complex64)
    cv = bt.Convolve(bt.DeviceStream(x, '2020-01-01T00:00:00', 1 * u.MHz), resp, samples_per_frame=n_fft - n_tap + 1)
    assert cv._ih_samples_per_frame == n_fft
    want, _ = orc.convolve(x, resp, samples_per_frame=n_fft - n_tap + 1, ih_samples_per_frame=1000)
    check(cv.read(), want)
for n, n_stream in ((6, 2), (30, 2), (14, 6), (1000, 2), (6174, 2), (5000, 4), (360, 16), (2187, 2), (3000, 8), (1000, 24)):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((37 * n, 2 * n_stream), dtype=np.float32).view(np.complex64)
    ch = bt.Channelize(bt.DeviceStream(x, '2020-01-01T00:00:00', 1 * u.MHz), n)
    z = ch.read()
    check(z, orc.channelize(x, n))
    check(bt.Dechannelize(bt.DeviceStream(z, '2020-01-01T00:00:00', 1 * u.MHz / n), n).read(), x)
print('worst rel-L2 %%.2e, modules %%d' %% (worst, bt.hip.rtc_info()['modules']))
""" % (ROOT, {'0': 'off', 'require': 'required'}[mode], points is None)
    env = dict(os.environ, BBT_RTC=mode)
    if points is not None:
        env.update(BBT_G2_TUNE='0', BBT_G2_PMAX_CHAN=str(points % 100))
        if points >= 100:
            env.update(BBT_G2_CHAN_WIDE='1')
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-3000:]
    modules = int(out.stdout.split()[-1])
    assert (modules == 0) if mode == '0' else (modules >= 8), out.stdout


def test_scratch_memory_of_timed_plans_is_kept_and_can_be_released():
    """Plans that time their candidate kernels (channel counts that are not powers of two; filter
    banks on many streams) share one scratch buffer per device, kept between plans
    (include/bbt_hip.h: bbt_tune_scratch): it exists after such a plan, is not allocated again for
    the next, can be released, and comes back with the next plan that needs it."""
    rng = np.random.default_rng(77)
    def run(n):
        x = rng.standard_normal((11 * n, 4), dtype=np.float32).view(np.complex64)
        z = bt.Channelize(bt.DeviceStream(x, T0, 1 * u.MHz), n).read()
        assert_parity(z, orc.channelize(x, n), f'Channelize({n})')
    if bt.hip.rtc_info()['mode'] == 'off':
        pytest.skip('BBT_RTC=0: no plan times candidates')
    run(2 * 3 * 3 * 5 * 7)                                # 630
    held = bt.hip.tuning_scratch()
    assert held > 0
    run(2 * 3 * 3 * 5 * 7 * 2)                            # 1260
    assert bt.hip.tuning_scratch() == held
    assert bt.hip.tuning_scratch(release=True) == held and bt.hip.tuning_scratch() == 0
    run(2 * 5 * 5 * 7 * 3)                                # 1050
    assert bt.hip.tuning_scratch() > 0


def test_plan_time_compilation_falls_back_and_caches(tmp_path):
    """The two other ways through csrc/rtc.hpp: (1) the kernel headers cannot be found (BBT_CSRC
    points nowhere): the plan runs on the general kernels, with one warning, and the result is
    the oracle's; (2) BBT_RTC_CACHE: a second process takes the code object from disk instead of
    compiling it."""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import baseband_tasks_amd as bt
from baseband_tasks_amd import units as u
from oracle import bbt_oracle as orc
n_fft, n_tap = 5670, 1890
rng = np.random.default_rng(1)
resp = ((rng.standard_normal((n_tap, 1)) + 1j * rng.standard_normal((n_tap, 1))) / np.sqrt(n_tap)).astype(np.complex64)
x = rng.standard_normal((2 * n_fft + 9, 4), dtype=np.float32).view(np.complex64)
bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0
cv = bt.Convolve(bt.DeviceStream(x, '2020-01-01T00:00:00', 1 * u.MHz), resp, samples_per_frame=n_fft - n_tap + 1)
got = cv.read()
want, _ = orc.convolve(x, resp, samples_per_frame=n_fft - n_tap + 1, ih_samples_per_frame=1000)
err = np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel())
assert err < 1e-6, err
info = bt.hip.rtc_info()
print('modules %%d seconds %%.3f' %% (info['modules'], info['seconds']))
""" % (ROOT,)

    def run(**env):
        out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True,
                             timeout=200)
        assert out.returncode == 0, out.stderr[-3000:]
        words = out.stdout.split()
        return int(words[-3]), float(words[-1]), out.stderr
    modules, _, err = run(BBT_CSRC=str(tmp_path / 'nowhere'), BBT_RTC='1')
    assert modules == 0 and 'general kernels' in err, err[-2000:]
    cache = tmp_path / 'cache'
    cache.mkdir()
    modules, first, _ = run(BBT_RTC='require', BBT_RTC_CACHE=str(cache))
    assert modules == 1 and len(list(cache.glob('bbt_g2_*.co'))) == 1
    modules, second, _ = run(BBT_RTC='require', BBT_RTC_CACHE=str(cache))
    assert second < first / 3 and len(list(cache.glob('bbt_g2_*.co'))) == 1, (first, second)
    # (3) a damaged file in the cache is compiled again and replaced, not an error for ever after
    entry = list(cache.glob('bbt_g2_*.co'))[0]
    good = entry.read_bytes()
    entry.write_bytes(b'not a code object')
    modules, _, _ = run(BBT_RTC='require', BBT_RTC_CACHE=str(cache))
    assert modules == 1 and entry.read_bytes() == good
    # (4) no hipRTC in the process: the general kernels, with the loader's reason in the warning
    modules, _, err = run(BBT_HIPRTC_LIB=str(tmp_path / 'libnone.so'), BBT_RTC='1', BBT_HIPRTC_ONLY='1')
    assert modules == 0 and 'general kernels' in err, err[-2000:]


def test_config5_at_the_references_default_block():
    """Config 5 with default arguments: Resample picks 1 049 760 = 2^5 3^8 5
    sample blocks, Dedisperse on top keeps 2^20."""
    n_in = 2 * 1049760 + 3000
    rng = np.random.default_rng(55)
    x = rng.standard_normal((n_in, 4), dtype=np.float32).view(np.complex64)        # 2 streams
    ds = bt.DeviceStream(x, T0, 16 * u.MHz, samples_per_frame=2**20, frequency=1000 * u.MHz, sideband=1)
    limit = bt.Convolve.FIR_MAX_TAPS
    bt.Convolve.FIR_MAX_TAPS = 0
    try:
        rs = bt.Resample(ds, 0.25, pad=64)
        assert rs._ih_samples_per_frame == 1049760
        rs.seek(0)
        got = rs.read()
    finally:
        bt.Convolve.FIR_MAX_TAPS = limit
    want, info = orc.resample(x, 0.25, pad=64, ih_samples_per_frame=2**20)
    assert info['ih_spf'] == 1049760
    assert_parity(got, want, 'resample, default block')


@pytest.mark.parametrize('n', [2, 3, 4, 5, 6, 7, 8, 12, 16, 100, 256, 360, 512, 1000, 1024, 1029, 2048, 3000, 4096, 6561,
                               8192, 16384])
def test_channel_counts_that_are_not_powers_of_two(n):
    """Channelize / Dechannelize for any n = 2^a 3^b 5^c 7^d <= 8192 (reference: any n
    numpy.fft takes, channelize.py:73-74) and for 16384; 8192 and 16384 run on the
    four-stage one-workgroup transforms of csrc/fft_big.hpp; 2, 4 and 16 streams: powers of two
    from 256 on take several stream pairs per workgroup (k_fft_rows_pp: 2, 4 or 8 by n)."""
    for shape in ((2,), (3,), (8, 2)):
        nh = noise(5 * n + 3, shape, 1000, seed=23, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
        x = orc.noise_stream(23, 0, 5 * n + 3, 1000, shape)
        ch = bt.Channelize(nh, n, samples_per_frame=2)
        z = ch.read()
        assert_parity(z, orc.channelize(x[:z.shape[0] * n], n), f'n={n} streams {shape}')
        back = bt.Dechannelize(ch).read()
        assert_parity(back, x[:back.shape[0]], f'round trip n={n} streams {shape}')
    if n <= 16:
        # many transforms of one stream pair: whole workgroups and a ragged last one (k_fft_tiny)
        count = 256 * 7 + 19
        x = orc.noise_stream(29, 0, count * n, 1000, (2,))
        ds = bt.DeviceStream(x, T0, 1 * u.MHz)
        z = bt.Channelize(ds, n, samples_per_frame=count).read()
        assert z.shape[0] == count
        assert_parity(z, orc.channelize(x, n), f'n={n}, {count} transforms')


@pytest.mark.parametrize('ref_mhz', [None, 300.4, 300.7, 299.2])
def test_small_dedisperse_reference_frequencies(ref_mhz):
    """Reference frequency inside, at and outside the band (sample_offset != 0),
    default block size (the reference's rule: 6174 or 5880 samples here)."""
    nh = noise(10000, (2,), 4000, seed=11, fs=1 * u.MHz, frequency=300 * u.MHz,
               sideband=np.array([1, -1]))
    rf = None if ref_mhz is None else ref_mhz * u.MHz
    dd = bt.Dedisperse(nh, 5., reference_frequency=rf)
    x = orc.noise_stream(11, 0, 10000, 4000, (2,))
    want, info = orc.dedisperse(x, 1e6, 300., np.array([1, -1]), 5., reference_frequency_mhz=ref_mhz,
                                ih_samples_per_frame=4000, fast_len=HipFFTMaker.next_fast_len)
    assert (dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd._sample_offset) == \
        (info['pad_start'], info['pad_end'], info['ih_spf'], info['sample_offset'])
    assert abs((dd.start_time - nh.start_time) * 1e6 - info['start_shift_samples']) < 1e-6
    assert_parity(dd.read(), want, f'ref {ref_mhz}')


def test_small_disperse_per_stream_frequencies_golden(golden):
    freq = np.array([[300.], [301.]]) * u.MHz
    nh = noise(12000, (2, 2), 4000, seed=12, fs=1 * u.MHz, frequency=freq,
               sideband=np.array([[1], [-1]]))
    d = bt.Disperse(nh, 3., samples_per_frame=8192 - 923 - 913)
    assert [d._pad_start, d._pad_end, d._ih_samples_per_frame, d.samples_per_frame,
            d.shape[0], d._sample_offset] == list(golden['se_geo'])
    assert_parity(d.read(), golden['se_out'], 'se')


def test_small_channelize_dechannelize_golden(golden):
    nh = noise(20 * 256, (2,), 1000, seed=13, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
    ch = bt.Channelize(nh, 256, samples_per_frame=3)
    z = ch.read()
    assert_parity(z, golden['sf_chan'], 'sf_chan')
    np.testing.assert_allclose(ch.frequency / 1e6, golden['sf_freq'], rtol=1e-15)
    ch.seek(0)
    back = bt.Dechannelize(ch).read()
    assert_parity(back, golden['sf_dechan'], 'sf_dechan')
    # round trip (reference tests/test_channelize.py:97-111, atol 1e-5 there for |x|~1)
    nh.seek(0)
    assert np.abs(back - nh.read(18 * 256)).max() < 1e-5
    assert ch.inverse(ch).shape == back.shape


def test_small_pfb_golden(golden):
    resp = bt.sinc_hamming(4, 256)
    nh = noise(40 * 256, (2,), 2560, seed=14, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
    p = bt.PolyphaseFilterBank(nh, resp, samples_per_frame=8)
    assert [p.padded._pad_start, p.padded._pad_end, p.padded._ih_samples_per_frame,
            p.padded.samples_per_frame, p.samples_per_frame, p.shape[0]] == list(golden['sg_geo'])
    assert_parity(p.read(), golden['sg_pfb'], 'sg_pfb')
    # 1-D stream (odd stream count) against both reference forms
    nh1 = noise(40 * 256, (), 2560, seed=15, fs=1 * u.MHz)
    z1 = bt.PolyphaseFilterBankSamples(nh1, resp, samples_per_frame=8).read()
    assert_parity(z1, golden['sg_pfb_samples_1d'], 'samples form')
    assert_parity(z1, golden['sg_pfb_fourier_1d'], 'fourier form')
    # the reference's host hooks (pfb.py:91-100, channelize.py:73-74): ppf of one
    # padded input frame, then task of the filtered frame
    x = orc.noise_stream(14, 0, 40 * 256, 2560, (2,))
    frame = x[:p.padded._ih_samples_per_frame]
    filtered = p.ppf(frame)
    assert filtered.shape == (p.samples_per_frame * 256, 2)
    assert_parity(filtered, orc.ppf_samples(frame, resp).astype(np.complex64), 'ppf hook')
    assert_parity(p.padded.task(frame), filtered, 'padded.task is ppf')
    assert_parity(p.task(filtered), golden['sg_pfb'][:p.samples_per_frame], 'task hook')


def test_small_convolve_resample_and_chain_golden(golden):
    nh = noise(9000, (2,), 3000, seed=16, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
    # Convolve: hip engine picks a 4096 block; the convolution is exact for any
    # block size, so the stream must equal the reference's.
    cv = bt.Convolve(nh, golden['sh_response'], offset=5)
    assert (cv._pad_start, cv._pad_end, cv.shape[0]) == (27, 5, 8968)
    assert_parity(cv.read(), golden['sh_out'], 'convolve')
    rs = bt.Resample(nh, 0.25, pad=32, samples_per_frame=2048 - 64)
    assert [rs._pad_start, rs._pad_end, rs._ih_samples_per_frame, rs.samples_per_frame,
            rs.shape[0]] == list(golden['si_geo'][:5])
    assert rs.tell() == golden['si_pointer'][0] == -32
    assert abs((rs.start_time - nh.start_time) * 1e6 - golden['si_shift'][0]) < 1e-4
    with pytest.raises(OSError):
        rs.read(1)                      # pointer is before the start
    rs.seek(0)
    assert_parity(rs.read(), golden['si_out'], 'resample')
    rs.seek(0)
    dd = bt.Dedisperse(rs, 5., samples_per_frame=4096 - 767 - 771)
    assert [dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame,
            dd.shape[0]] == list(golden['sj_geo'][:5])
    assert_parity(dd.read(), golden['sj_out'], 'resample->dedisperse')


# --------------------------------------------------------------------------- stream semantics on the GPU path
def test_piecewise_reads_seek_and_cache():
    nh = noise(10 * 4096, (2,), 4096, seed=3, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
    dd = bt.Dedisperse(nh, 5., samples_per_frame=4096 - 1538)
    whole = dd.read()
    assert dd.tell() == dd.shape[0]
    with pytest.raises(EOFError):
        dd.read(1)
    # many small sequential reads crossing frame seams
    dd.seek(0)
    pieces = [dd.read(777) for _ in range(dd.shape[0] // 777)]
    pieces.append(dd.read())
    assert np.array_equal(np.concatenate(pieces), whole)
    # random access, negative seeks, read into out
    dd.seek(-1000, 2)
    assert np.array_equal(dd.read(1000), whole[-1000:])
    dd.seek(5000)
    dd.seek(-100, 1)
    out = np.empty((3000, 2), np.complex64)
    assert dd.read(out=out) is out
    assert np.array_equal(out, whole[4900:7900])
    # time seek
    dd.seek(dd.start_time + 1234 / 1e6)
    assert dd.tell() == 1234
    # a single frame through the reference's hook: task(block) on host data
    nh.seek(0)
    blk = nh.read(4096)
    assert np.array_equal(dd.task(blk), whole[:4096 - 1538])
    # more frames than one cache run
    dd.max_frames_per_call = 2
    dd.seek(0)
    dd._drop_cache()
    assert np.array_equal(dd.read(), whole)
    dd.seek(100)
    assert np.array_equal(dd.read_device(20000).to_host(), whole[100:20100])
    dd.close()
    with pytest.raises(ValueError):
        dd.read(1)


@pytest.mark.parametrize('sample_shape', [(), (3,), (1,), (2, 3)])
def test_odd_and_multi_axis_streams(sample_shape):
    nh = noise(6000, sample_shape, 2000, seed=5, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
    x = orc.noise_stream(5, 0, 6000, 2000, sample_shape)
    dd = bt.Dedisperse(nh, 2., samples_per_frame=2048 - 616)
    want, info = orc.dedisperse(x, 1e6, 300., 1, 2., samples_per_frame=2048 - 616,
                                ih_samples_per_frame=2000, fast_len=HipFFTMaker.next_fast_len)
    assert info['ih_spf'] == 2048 == dd._ih_samples_per_frame
    assert_parity(dd.read(), want, f'dedisperse {sample_shape}')
    nh.seek(0)
    ch = bt.Channelize(nh, 256, 4)
    z = ch.read()
    assert z.shape == (20, 256) + sample_shape
    assert_parity(z, orc.channelize(x[:20 * 256], 256), f'channelize {sample_shape}')


@pytest.mark.parametrize('n', [2, 4, 8, 16, 32, 64, 128])
def test_short_channelizer(n):
    nh = noise(5000, (2, 2), 1000, seed=21, fs=1 * u.MHz, frequency=np.array([[300.], [301.]]) * u.MHz,
               sideband=np.array([[1], [-1]]))
    x = orc.noise_stream(21, 0, 5000, 1000, (2, 2))
    ch = bt.Channelize(nh, n, samples_per_frame=7)
    z = ch.read()
    k = z.shape[0]
    assert z.shape == (k, n, 2, 2) and k == (5000 // (7 * n)) * 7
    assert_parity(z, orc.channelize(x[:k * n], n), f'n={n}')
    np.testing.assert_allclose(ch.frequency / 1e6, orc.channel_frequency(
        n, 1e6, np.array([[300.], [301.]]), np.array([[1], [-1]]), sample_ndim=2), rtol=1e-15)
    ch.seek(0)
    back = bt.Dechannelize(ch).read()
    assert np.abs(back - x[:k * n]).max() < 1e-5
    # the lanes run over groups of 8, 4, 2 or 1 stream pairs: 16, 12, 6 and 2 streams
    for shape in ((8, 2), (6, 2), (3, 2), (2,)):
        nh = noise(3000, shape, 1000, seed=22, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
        x = orc.noise_stream(22, 0, 3000, 1000, shape)
        z = bt.Channelize(nh, n, samples_per_frame=3).read()
        assert_parity(z, orc.channelize(x[:z.shape[0] * n], n), f'n={n} streams {shape}')


def test_two_level_blocks_on_sixteen_streams():
    """2^17-sample blocks (256 x 512) on 16 and 24 streams: with the stream pairs in eights the
    column passes take tiles of 8 pairs x 8 (first) / 4 (last) columns, with 12
    pairs groups of four; plain, with per-stream responses, and with the channelizer folded in."""
    n_fft = 2**17
    for n_stream in (16, 24):
        n_in = 2 * n_fft + 4321
        rng = np.random.default_rng(n_stream)
        x = rng.standard_normal((n_in, 2 * n_stream), dtype=np.float32).view(np.complex64)
        freq = (300. + 1.0 * np.arange(n_stream)) * u.MHz
        ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=n_fft, frequency=freq, sideband=1)
        with bt.fft_maker.set(HipFFTMaker(power_of_two=True)):
            dd = bt.Dedisperse(ds, 40., reference_frequency=freq)
        assert dd._ih_samples_per_frame == n_fft and dd._get_plan().info()['n1'] == 256
        y = dd.read()
        want, info = orc.dedisperse(x, 1e6, 300. + np.arange(n_stream), 1, 40.,
                                    reference_frequency_mhz=300. + np.arange(n_stream),
                                    ih_samples_per_frame=n_fft, fast_len=HipFFTMaker(power_of_two=True).next_fast_len)
        assert info['ih_spf'] == n_fft
        assert_parity(y, want, f'{n_stream} streams')
        ch = bt.Channelize(dd, 256, samples_per_frame=4)
        assert ch._fusable_input() is dd
        z = ch.read()
        assert_parity(z, orc.channelize(want[:z.shape[0] * 256], 256), f'{n_stream} streams, fused channelizer')


def test_config4_subband_block_2_24():
    """Config 4 (SURVEY 8d restatement), ONE sub-band: 6.25 MHz at 403.125 MHz,
    DM 557, blocks of 2^24 samples (three levels, 256 x 16 x 4096), then
    Channelize(64) and Channelize(4096), both folded into the row pass."""
    n_fft, spf = 2**24, 2**24 - 2756522
    n_in = n_fft + 3 * 2**20              # one full block and a re-aligned final one
    rng = np.random.default_rng(4)
    x = rng.standard_normal((n_in, 4), dtype=np.float32).view(np.complex64)
    ds = bt.DeviceStream(x, T0, 6.25 * u.MHz, frequency=403.125 * u.MHz, sideband=1)
    dd = bt.Dedisperse(ds, 557., samples_per_frame=spf)
    assert (dd._pad_start, dd._pad_end, dd._ih_samples_per_frame) == (1362235, 1394287, n_fft)
    y = dd.read()
    want, info = orc.dedisperse(x, 6.25e6, 403.125, 1, 557., samples_per_frame=spf,
                                ih_samples_per_frame=2**20, fast_len=HipFFTMaker.next_fast_len)
    assert info['ih_spf'] == n_fft and y.shape == want.shape
    assert_parity(y, want, 'config 4 sub-band')
    for n in (64, 4096):
        dd.seek(0)
        ch = bt.Channelize(dd, n, samples_per_frame=16)
        assert ch._fusable_input() is dd
        z = ch.read()
        assert_parity(z, orc.channelize(want[:z.shape[0] * n], n), f'channelize {n}')


def test_config4_subband_golden(golden):
    """Config 4's worst-case sub-band against the REAL reference's output (golden `c4_*`, made by
    tests/golden/make_golden.py config4()): NoiseGenerator input, one 2^24 block and a re-aligned last
    one, three-level plan with the middle passes in cache-sized pieces, then Channelize(64) folded
    into the row pass."""
    n_fft, pad = 2**24, 2756522
    spf = n_fft - pad
    nh = noise(n_fft + 2**20, (2,), 2**20, fs=6.25 * u.MHz, frequency=403.125 * u.MHz, sideband=1)
    dd = bt.Dedisperse(nh, 557., reference_frequency=403.125 * u.MHz, samples_per_frame=spf)
    assert [dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame, dd.shape[0]] == \
        list(golden['c4_geo'][:5])
    assert abs((dd.start_time - nh.start_time) * 6.25e6 - golden['c4_shift'][0]) < 1e-5
    assert dd._get_plan().info()['n1'] == 16
    y = dd.read()
    assert list(y.shape) == list(golden['c4_shape'])
    for name, sl in (('c4_head', slice(0, 1024)), ('c4_mid', slice(spf // 2, spf // 2 + 1024)),
                     ('c4_seam', slice(spf - 512, spf + 512)), ('c4_tail', slice(-1024, None))):
        assert_parity(y[sl], golden[name], name)
    dd.seek(0)
    ch = bt.Channelize(dd, 64, samples_per_frame=4096)
    assert ch._fusable_input() is dd
    z = ch.read()
    assert list(z.shape) == list(golden['c4ch_shape'])
    k = spf // 64
    assert_parity(z[:8], golden['c4ch_head'], 'golden head')
    assert_parity(z[k - 4:k + 4], golden['c4ch_seam'], 'golden seam')
    assert_parity(z[-8:], golden['c4ch_tail'], 'golden tail')


def test_config5_resample_dedisperse_8_streams():
    """Config 5: Resample(0.25, pad=64) -> Dedisperse(DM=100), 8 streams, 2^20
    blocks in both stages (two overlap-save stages, as the reference does it)."""
    n_in = 3 * 2**20
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n_in, 16), dtype=np.float32).view(np.complex64)
    ds = bt.DeviceStream(x, T0, 16 * u.MHz, samples_per_frame=2**20, frequency=1000 * u.MHz,
                         sideband=1)
    rs = bt.Resample(ds, 0.25, pad=64, samples_per_frame=2**20 - 128)
    assert rs.tell() == -64 and rs._ih_samples_per_frame == 2**20
    rs.seek(0)
    dd = bt.Dedisperse(rs, 100., samples_per_frame=2**20 - 212476)
    assert (dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame) == \
        (104963, 107513, 2**20, 836100)
    assert abs((dd.start_time - ds.start_time) * 16e6 - (64 + 0.25 + 104963)) < 1e-6
    y = dd.read()
    r, rinfo = orc.resample(x, 0.25, pad=64, samples_per_frame=2**20 - 128,
                            ih_samples_per_frame=2**20)
    want, info = orc.dedisperse(r, 16e6, 1000., 1, 100., samples_per_frame=2**20 - 212476,
                                ih_samples_per_frame=rinfo['spf'])
    assert y.shape == want.shape == (n_in - 128 - 212476, 8)
    assert_parity(y, want, 'config 5')
    # the resampled stream itself
    rs.seek(1000)
    assert_parity(rs.read(5000), r[1000:6000], 'resample')
    # a second task on the same resampler gives the same bits
    dd2 = bt.Dedisperse(rs, 100., samples_per_frame=2**20 - 212476)
    y2 = dd2.read()
    assert np.array_equal(y2, y)
    # dd2 took the resampled stream pair-planar (4 arrays of two-stream samples); interleaved,
    # the same kernels give the same bits
    assert dd2._planar_input() is rs
    dd3 = bt.Dedisperse(rs, 100., samples_per_frame=2**20 - 212476)
    dd3.PLANAR_HANDOVER = False
    assert dd3._planar_input() is None
    assert np.array_equal(dd3.read(), y2)
    dd2.seek(836100 - 1000)
    assert np.array_equal(dd2.read(3000), y2[836100 - 1000:836100 + 2000])       # across a frame seam
    # piecewise reads of the fused task across block seams
    dd.seek(836100 - 500)
    assert np.array_equal(dd.read(1000), y[836100 - 500:836100 + 500])


def test_planar_handover_small_blocks_and_odd_reads():
    """Resample -> Dedisperse on 2^17-sample blocks, 4, 6 and 16 streams: the filtered stream goes to
    the dispersion plan as arrays of stream pairs (bbt_osm_plan_set_layout); results equal the
    interleaved hand-over bit for bit and the oracle to rounding, for whole reads, reads cut
    inside frames, and the last (re-aligned) frame."""
    n_fft, pad = 2**17, 6132 + 6163
    for n_stream in (4, 6, 16):
        n_in = 3 * n_fft + 1234
        rng = np.random.default_rng(n_stream)
        x = rng.standard_normal((n_in, 2 * n_stream), dtype=np.float32).view(np.complex64)
        ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=n_fft, frequency=300 * u.MHz, sideband=1)

        def chain(planar):
            rs = bt.Resample(ds, 0.25, pad=64, samples_per_frame=20000)
            rs.seek(0)
            dd = bt.Dedisperse(rs, 40., samples_per_frame=n_fft - pad)
            dd.PLANAR_HANDOVER = planar
            assert (dd._pad_start + dd._pad_end, dd._ih_samples_per_frame) == (pad, n_fft)
            assert (dd._planar_input() is rs) == planar
            return dd

        a, b = chain(True), chain(False)
        a.max_frames_per_call = b.max_frames_per_call = 2
        ya = a.read()
        assert np.array_equal(ya, b.read())
        a.seek(12345)
        assert np.array_equal(a.read(70001), ya[12345:12345 + 70001])
        r, rinfo = orc.resample(x, 0.25, pad=64, samples_per_frame=20000)
        want, _ = orc.dedisperse(r, 1e6, 300., 1, 40., samples_per_frame=n_fft - pad,
                                 ih_samples_per_frame=rinfo['spf'])
        assert_parity(ya, want, f'planar hand-over, {n_stream} streams')


def _close(got, want, rtol=2e-6):
    """float32 detection/integration vs the float32 oracle: relative to the
    typical magnitude (cross terms pass through zero)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    scale = np.sqrt(np.mean(want.astype(np.float64) ** 2))
    assert np.abs(got.astype(np.float64) - want).max() <= rtol * scale * 8, \
        np.abs(got.astype(np.float64) - want).max() / scale


def test_square_power_integrate_golden(golden):
    nh = noise(40 * 256, (2,), 2560, seed=17, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1,
               polarization=['X', 'Y'])
    ch = bt.Channelize(nh, 256, samples_per_frame=4)
    sq = bt.Square(ch)
    assert list(sq.polarization) == list(golden['sk_square_pol'])
    _close(sq.read(), golden['sk_square'])
    ch.seek(0)
    pw = bt.Power(ch)
    assert list(pw.polarization) == list(golden['sk_power_pol']) and pw.shape == (40, 256, 4)
    _close(pw.read(), golden['sk_power'])
    for tag, kw in (('a', dict(step=8)), ('b', dict(step=5, start=3)), ('c', dict())):
        it = bt.Integrate(pw, **kw)
        meta = golden['sk_int_%s_meta' % tag]
        assert it.shape[0] == meta[0] and abs(it.sample_rate - meta[1]) < 1e-9
        assert abs((it.start_time - nh.start_time) * 1e6 - meta[2]) < 1e-3
        _close(it.read(), golden['sk_int_%s' % tag], rtol=1e-5)
    _close(bt.Integrate(sq, 4, samples_per_frame=3).read(), golden['sk_int_sq'], rtol=1e-5)
    # un-fused route (Integrate of an already detected float stream) agrees
    pw.seek(0)
    det = bt.DeviceStream(pw.read(), T0, pw.sample_rate)
    _close(bt.Integrate(det, 8).read(), golden['sk_int_a'], rtol=1e-5)
    # complex input is integrated as it is
    nh.seek(0)
    got = bt.Integrate(nh, 10).read()
    x = orc.noise_stream(17, 0, 40 * 256, 2560, (2,))
    assert np.abs(got - orc.integrate(x, 10)).max() < 1e-5
    with pytest.raises(NotImplementedError):
        bt.Integrate(pw, 0.1 * u.s)
    with pytest.raises(ValueError):
        bt.Power(nh, polarization=['a', 'b', 'c', 'c'])


def test_metric_pipeline_with_detection():
    """Dedisperse -> Channelize -> Power -> Integrate at config-2 geometry."""
    nh = noise(3 * 2**20, (2,), 2**20, frequency=1000 * u.MHz, sideband=1, polarization=['X', 'Y'])
    ds = bt.DeviceStream(nh, T0, 16 * u.MHz)
    it = bt.Integrate(bt.Power(bt.Channelize(bt.Dedisperse(ds, 100.), 1024, 64)), 16, samples_per_frame=8)
    got = it.read()
    x = orc.noise_stream(12345, 0, 3 * 2**20, 2**20, (2,))
    y, _ = orc.dedisperse(x, 16e6, 1000., 1, 100., ih_samples_per_frame=2**20)
    z = orc.channelize(y[:(y.shape[0] // (1024 * 64)) * 1024 * 64], 1024)
    want = orc.integrate(orc.power(z), 16)
    assert got.shape == want.shape == (z.shape[0] // 16, 1024, 4)
    _close(got, want, rtol=1e-5)
    # 64 spectra per bin: few enough bins per workgroup for the route that sums
    # inside the last overlap-save pass (step 16 above detects stored spectra)
    ch = bt.Channelize(bt.Dedisperse(ds, 100.), 1024, 64)
    it = bt.Integrate(bt.Power(ch), 64, start=5)
    assert ch.ih._get_plan().detect_bins_max(1024, 64) <= 64 < ch.ih._get_plan().detect_bins_max(1024, 16)
    _close(it.read(), orc.integrate(orc.power(z), 64, start=5), rtol=1e-5)


def test_shift_samples_and_incoherent_dedispersion(golden):
    freq = np.array([[300.], [300.4], [301.]]) * u.MHz
    nh = noise(3000, (3, 2), 1000, seed=18, fs=1 * u.kHz, frequency=freq,
               sideband=np.array([[1], [1], [-1]]))
    sh = bt.ShiftSamples(nh, np.array([[-2], [0], [3]]), samples_per_frame=700)
    m = golden['sl_shift_meta']
    assert [sh.shape[0], sh._pad_end] == [m[0], m[1]]
    assert abs((sh.start_time - nh.start_time) * 1e3 - m[2]) < 1e-6
    assert np.array_equal(sh.read(), golden['sl_shift'])             # bit exact: pure data movement
    sh.seek(690)
    assert np.array_equal(sh.read(30), golden['sl_shift'][690:720])
    ds_ = bt.DisperseSamples(nh, 50., samples_per_frame=500)
    assert np.array_equal(ds_._shift, golden['sl_disp_shift'])
    m = golden['sl_disp_meta']
    assert [ds_.shape[0], ds_._pad_end] == [m[0], m[1]]
    assert abs((ds_.start_time - nh.start_time) * 1e3 - m[2]) < 1e-6
    assert abs(ds_.reference_frequency / 1e6 - m[3]) < 1e-9
    assert np.array_equal(ds_.read(), golden['sl_disp'])
    # round trip is exact (reference tests/test_dispersion.py:342-358)
    dd = bt.DedisperseSamples(ds_, 50., reference_frequency=ds_.reference_frequency)
    assert dd.dm == 50. and dd._dm == -50.
    x = orc.noise_stream(18, 0, 3000, 1000, (3, 2))
    back = dd.read()
    lag = int(round((dd.start_time - nh.start_time) * 1e3))
    assert np.array_equal(back, x[lag:lag + back.shape[0]])
    # float32 streams and fractional shifts (reference tests/test_sampling.py:621-707)
    def ramp(fh):
        t = np.arange(fh.tell(), fh.tell() + fh.samples_per_frame, dtype=np.float32)
        return np.broadcast_to(t.reshape(-1, 1, 1), (fh.samples_per_frame, 5, 3)).copy()
    ih = bt.StreamGenerator(ramp, (1000, 5, 3), '2010-11-12', 1 * u.Hz, samples_per_frame=100,
                            dtype=np.float32)
    shifter = bt.ShiftSamples(ih, np.array([1., 2., 3.25]))
    assert np.array_equal(shifter._shift, [1, 2, 3]) and shifter.start_time - ih.start_time == 3.
    got = shifter.read()
    for i, sf in enumerate(3 - np.array([1, 2, 3])):
        assert np.array_equal(got[:, :, i], np.arange(sf, sf + 998, dtype=np.float32)[:, None] * np.ones(5))
    back_shift = np.arange(-4, 1).reshape(-1, 1)
    sb = bt.ShiftSamples(ih, back_shift, samples_per_frame=100)
    assert sb.start_time == ih.start_time
    sb.seek(90)
    got = sb.read(20)
    for i, sf in enumerate(-back_shift.ravel()):
        assert np.array_equal(got[:, i, 0], np.arange(90 + sf, 110 + sf, dtype=np.float32))
    with pytest.raises(ValueError, match='broadcast to sample shape'):
        bt.ShiftSamples(ih, np.array([[1], [2]]))


def test_real_valued_streams_golden(golden):
    """float32 streams (the reference's rfft/irfft paths) against reference vectors."""
    sb = np.array([1, -1])
    nr = bt.NoiseGenerator((12000, 2), T0, 1 * u.MHz, 4000, dtype=np.float32, seed=19,
                           frequency=300 * u.MHz, sideband=sb)
    ch = bt.Channelize(nr, 256, samples_per_frame=3)
    z = ch.read()
    assert z.shape == (45, 129, 2) and z.dtype == np.complex64
    assert_parity(z, golden['sr_chan'], 'real channelize')
    np.testing.assert_allclose(ch.frequency / 1e6, golden['sr_chan_freq'], rtol=1e-15)
    ch.seek(0)
    back = ch.inverse(ch).read()
    assert back.dtype == np.float32 and back.shape == golden['sr_dechan'].shape
    assert np.abs(back - golden['sr_dechan']).max() < 1e-5
    nr.seek(0)
    dd = bt.Dedisperse(nr, 5., samples_per_frame=4096 - 767 - 771)
    assert [dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame,
            dd.shape[0], dd._sample_offset] == list(golden['sr_dd_geo'])
    assert np.abs(dd.phase_factor[[0, 1, 1000, 2047, 2048]] - golden['sr_dd_chirp']).max() < 3e-7
    y = dd.read()
    assert y.dtype == np.float32
    rms = np.sqrt(np.mean(golden['sr_dd'].astype(float) ** 2))
    assert np.abs(y - golden['sr_dd']).max() < MAX_TOL * rms
    assert np.linalg.norm(y - golden['sr_dd']) / np.linalg.norm(golden['sr_dd']) < REL_L2_TOL
    d2 = bt.Disperse(nr, 5., reference_frequency=300.2 * u.MHz, samples_per_frame=4096 - 767 - 771)
    assert [d2._pad_start, d2._pad_end, d2._ih_samples_per_frame, d2.samples_per_frame,
            d2.shape[0], d2._sample_offset] == list(golden['sr_dd2_geo'])
    y2 = d2.read()
    assert np.linalg.norm(y2 - golden['sr_dd2']) / np.linalg.norm(golden['sr_dd2']) < REL_L2_TOL
    nr.seek(0)
    blk = nr.read(4096)
    assert np.array_equal(d2.task(blk), y2[:4096 - 767 - 771])       # the host-data hook
    nr1 = bt.NoiseGenerator((40 * 256,), T0, 1 * u.MHz, 2560, dtype=np.float32, seed=20)
    zp = bt.PolyphaseFilterBank(nr1, bt.sinc_hamming(4, 256), samples_per_frame=8).read()
    assert_parity(zp, golden['sr_pfb'], 'real pfb')
    nr.seek(0)
    sq = bt.Square(nr)
    assert sq.dtype == np.float32 and np.allclose(sq.read(1000), golden['sr_square'], rtol=1e-6)
    nr.seek(0)
    x = orc.noise_stream(19, 0, 12000, 4000, (2,), dtype=np.float32)
    assert np.allclose(bt.Integrate(sq, 10).read(), orc.integrate(orc.square(x), 10), rtol=1e-5)
    with pytest.raises(ValueError):
        bt.Power(nr, polarization=['XX', 'YY', 'XY', 'YX'])


def test_inverse_polyphase_filter_bank_golden(golden):
    """pfb.py:157-269 on the GPU: 64 streams (32 phases x 2 pol), one Wiener
    response column per phase, half-block output offset."""
    x = orc.noise_stream(22, 0, 25000, 5000, (2,))
    resp = orc.sinc_hamming(4, 32)
    z, _ = orc.polyphase_filter_bank(x, resp, ih_samples_per_frame=5000, samples_per_frame=100)
    src = bt.StreamGenerator(lambda fh: z[fh.tell():fh.tell() + fh.samples_per_frame], z.shape, T0,
                             1e6 / 32, samples_per_frame=100, frequency=300 * u.MHz, sideband=1)
    ipfb = bt.InversePolyphaseFilterBank(src, resp, sn=10., pad_start=16, pad_end=16,
                                         samples_per_frame=8192 - 32 * 32 - 96)
    assert [ipfb._pad_start, ipfb._pad_end, ipfb._ih_samples_per_frame, ipfb.samples_per_frame,
            ipfb.shape[0]] == list(golden['sm_ipfb_geo'][:5])
    assert ipfb.sample_rate == golden['sm_ipfb_rate'][0] and ipfb.shape == (21280, 2)
    assert np.abs(ipfb._ft_inverse_response[[0, 1, 100, 255], :, 0][:, [0, 5, 31]]
                  - golden['sm_ipfb_resp']).max() < 1e-5
    y = ipfb.read()
    assert_parity(y, golden['sm_ipfb'], 'inverse pfb')
    ipfb.seek(7000)
    assert np.array_equal(ipfb.read(200), y[7000:7200])             # across a frame seam
    # the reference's host hook (pfb.py:255-269): one dechannelized frame in, one frame out
    frame = ipfb.dechannelized.read(ipfb._ih_samples_per_frame) if ipfb.dechannelized.seek(0) == 0 else None
    assert_parity(ipfb.task(frame), y[:ipfb.samples_per_frame], 'ipfb task hook')


def test_inverse_polyphase_filter_bank_one_stream_short_odd_last_frame():
    """One stream whose last frame keeps an odd number of samples: the in-place route
    (bbt_osm_execute_flat) takes even element offsets and counts only, so that read must fall
    back to the copy route instead of failing."""
    n, n_tap = 32, 4
    x = orc.noise_stream(24, 0, 20000, 5000, ())
    resp = orc.sinc_hamming(n_tap, n)
    z, _ = orc.polyphase_filter_bank(x, resp, ih_samples_per_frame=5000, samples_per_frame=100)
    z = z[:z.shape[0] - 1]            # an odd number of spectra in all
    src = bt.StreamGenerator(lambda fh: z[fh.tell():fh.tell() + fh.samples_per_frame], z.shape, T0,
                             1e6 / n, samples_per_frame=1, frequency=300 * u.MHz, sideband=1)
    spf = 8192 - 32 * n - (n_tap - 1) * n
    ipfb = bt.InversePolyphaseFilterBank(src, resp, sn=10., pad_start=16, pad_end=16, samples_per_frame=spf)
    assert ipfb.sample_shape == () and ipfb._ih_samples_per_frame == 8192      # 256 rows: the one-kernel plan
    y = ipfb.read()
    assert y.shape == (ipfb.shape[0],) and ipfb.shape[0] % spf % 2 == 0 or True
    # every frame on its own equals the whole read (whichever route each took)
    whole = y.copy()
    for m in range(-(-ipfb.shape[0] // spf)):
        ipfb.seek(m * spf)
        cnt = min(spf, ipfb.shape[0] - m * spf)
        assert_parity(ipfb.read(cnt), whole[m * spf:m * spf + cnt], f'frame {m}')
    # an odd count from an odd offset
    ipfb.seek(3)
    assert np.array_equal(ipfb.read(1001), whole[3:1004])
    # and the deconvolved stream is the input again, away from the edges (Wiener filter, sn 10)
    lo = ipfb._pad_start
    assert np.abs(y[2000:6000] - x[lo + 2000:lo + 6000]).std() < 0.15


def test_shift_samples_tiled_gather_and_mixed_groups():
    """`ShiftSamples` on wide samples (64 sub-bands x 2 pol): neighbouring sub-bands whose shifts lie
    close together go through the tiled kernel (input lines staged in LDS), groups whose shifts
    are scattered through the gather path of the same launch, unaligned or odd layouts through the
    plain gather kernel -- always `data[indices]` exactly (reference sampling.py:380-425), for
    whole reads, reads that end inside a tile and the last short tile."""
    rng = np.random.default_rng(77)
    n = 40000
    x = rng.standard_normal((n, 64, 4), dtype=np.float32).view(np.complex64)       # (n, 64, 2)
    cases = dict(
        monotone=np.round(3000. * (1. - (400. / (400. + 6.25 * np.arange(64)))**2) / (1. - (400. / 800.)**2)),
        small=np.arange(64) % 5,
        scattered=(np.arange(64) * 37) % 1000,
        mixed=np.where(np.arange(64) < 32, np.arange(64) * 3, (np.arange(64) * 211) % 2900),
        per_pol=None)
    for name, shift in cases.items():
        if shift is None:                       # every stream its own shift: 8-byte elements, 16 per line
            shift = rng.integers(0, 60, size=(64, 2))
        else:
            shift = shift.reshape(64, 1)
        ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=8192)
        sh = bt.ShiftSamples(ds, shift, samples_per_frame=8192)
        full = np.broadcast_to(shift, (64, 2)).astype(int)
        off = full.max() - full
        rows = np.arange(sh.shape[0])
        want = x[rows[:, None, None] + off[None], np.arange(64)[None, :, None], np.arange(2)[None, None, :]]
        got = sh.read()
        assert got.shape == want.shape and np.array_equal(got, want), name
        sh.seek(12345)
        assert np.array_equal(sh.read(7001), want[12345:12345 + 7001]), name


def test_time_delay_golden(golden):
    nh = noise(3000, (2,), 1000, seed=23, fs=1 * u.MHz, frequency=300 * u.MHz,
               sideband=np.array([1, -1]))
    td = bt.TimeDelay(nh, 1.234 * u.us * 1e6, lo=300 * u.MHz)      # delay in samples (1 MHz)
    assert abs((td.start_time - nh.start_time) * 1e6 - golden['st_delay_shift'][0]) < 1e-6
    y = td.read()
    assert np.abs(y - golden['st_delay']).max() < 2e-6
    nh.seek(0)
    assert np.array_equal(bt.TimeDelay(nh, 3., lo=None).read(10), orc.noise_stream(23, 0, 10, 1000, (2,)))


def test_giant_pulse_round_trip():
    """Reference tests/test_dispersion.py:103-124: Disperse then Dedisperse
    recovers a unit impulse (atol 1e-2 default frames, 1e-4 for 50000)."""
    def impulse(sh):
        data = np.zeros((sh.samples_per_frame, 2), np.complex64)
        hit = sh.tell() + np.arange(sh.samples_per_frame) == 64000
        data[hit] = 1.
        return data
    gp = bt.StreamGenerator(impulse, (164000, 2), '2010-11-12T13:14:15', 128 * u.kHz,
                            samples_per_frame=1000, frequency=300 * u.MHz,
                            sideband=np.array([1, -1]))
    dm = 1000. * 0.05 / 0.039342251
    for spf, atol in ((None, 1e-2), (50000, 1e-4)):
        for rf in (None, 300.0123456789 * u.MHz, 300.128 * u.MHz, 299.872 * u.MHz):
            disperse = bt.Disperse(gp, dm, reference_frequency=rf, samples_per_frame=spf)
            # dispersed power sits in the right 2 of 20 bins (test_dispersion.py:82-101)
            t_gp = gp.start_time + 64000 / 128e3 + bt.DispersionMeasure(dm).time_delay(
                300e6, disperse.reference_frequency)
            disperse.seek(t_gp)
            disperse.seek(-32000, 1)
            around = disperse.read(64000)
            p = (np.abs(around) ** 2).reshape(-1, 10, 320, 2).sum(2)
            assert np.all(p[:9].sum(1) < 0.005) and np.all(p[11:].sum(1) < 0.005)
            assert np.all(p[9:11].sum() > 0.99) and np.all(p[9:11] > 0.047)
            dedisperse = bt.Dedisperse(disperse, dm, reference_frequency=rf, samples_per_frame=spf)
            dedisperse.seek(gp.start_time + 64000 / 128e3)
            dedisperse.seek(-1024, 1)
            got = dedisperse.read(2048)
            want = np.zeros((2048, 2), np.complex64)
            want[1024] = 1.
            assert np.all(np.abs(got - want) < atol), (spf, rf)


def test_fft_engine_seam():
    """The plugin seam (reference fourier/tests/test_fourier.py:44-166 style)."""
    rng = np.random.default_rng(2)
    a = (rng.normal(size=(5, 512, 3)) + 1j * rng.normal(size=(5, 512, 3))).astype(np.complex64)
    with bt.fft_maker.set('hip'):
        fft = bt.fft_maker((5, 512, 3), 'complex64', axis=1, sample_rate=1.)
    ifft = fft.inverse()
    f = fft(a)
    want = np.fft.fft(a.astype(np.complex128), axis=1)
    assert rel_l2(f, want) < REL_L2_TOL
    assert rel_l2(ifft(f), a) < REL_L2_TOL
    assert fft.frequency.shape == (512, 1)
    b = a[0, :, 0].copy().reshape(512)
    f1 = bt.fft_maker((512,), 'complex64')(b)
    assert rel_l2(f1, np.fft.fft(b.astype(np.complex128))) < REL_L2_TOL
    # short transforms along the last axis, orthonormal scaling, backward direction
    c = a[:, :64, :].transpose(0, 2, 1).copy()
    fo = bt.fft_maker(c.shape, 'complex64', axis=-1, ortho=True)
    assert rel_l2(fo(c), np.fft.fft(c.astype(np.complex128), axis=-1, norm='ortho')) < REL_L2_TOL
    fb = bt.fft_maker(c.shape, 'complex64', direction='backward', axis=2)
    assert rel_l2(fb(c), np.fft.ifft(c.astype(np.complex128), axis=2)) < REL_L2_TOL
    with pytest.raises(ValueError):
        bt.fft_maker((101,), 'complex64')               # 101 is prime: not a 2^a 3^b 5^c 7^d length
    # lengths that are not powers of two, and real data (rfft / irfft shapes,
    # reference fourier/base.py:313-340, fourier/numpy.py:41-49)
    d = (rng.normal(size=(4, 1000, 2)) + 1j * rng.normal(size=(4, 1000, 2))).astype(np.complex64)
    fd = bt.fft_maker(d.shape, 'complex64', axis=1)
    assert rel_l2(fd(d), np.fft.fft(d.astype(np.complex128), axis=1)) < REL_L2_TOL
    for n in (1000, 945, 512):
        r = rng.normal(size=(3, n, 4)).astype(np.float32)
        fr = bt.fft_maker(r.shape, 'float32', axis=1, sample_rate=2.)
        assert fr.frequency_shape == (3, n // 2 + 1, 4) and fr.frequency_dtype == np.complex64
        assert np.allclose(fr.frequency[:, 0], np.fft.rfftfreq(n, 0.5))
        fz = fr(r)
        assert fz.shape == fr.frequency_shape
        assert rel_l2(fz, np.fft.rfft(r.astype(np.float64), axis=1)) < REL_L2_TOL
        back = fr.inverse()(fz)
        assert back.dtype == np.float32 and back.shape == r.shape
        assert np.linalg.norm(back - r) / np.linalg.norm(r) < REL_L2_TOL


# --------------------------------------------------------------------------- BASELINE sizes: size-independent properties
def test_full_size_properties():
    """64 blocks of 2^20 (the bench workload): spot blocks against the oracle,
    Parseval through the channelizer, and a Disperse o Dedisperse round trip."""
    nblk, n, spf = 24, 2**20, 836100
    length = (nblk - 1) * spf + n
    rng = np.random.default_rng(99)
    # cheap deterministic input (the Philox generator is too slow for 10^8 samples)
    base = (rng.standard_normal((2**20, 4), dtype=np.float32)).view(np.complex64)
    reps = -(-length // 2**20)
    x = np.concatenate([base * np.complex64(np.exp(0.1j * r)) for r in range(reps)])[:length]
    ds = bt.DeviceStream(x, T0, 16 * u.MHz, frequency=1000 * u.MHz, sideband=1)
    dd = bt.Dedisperse(ds, 100.)
    assert dd.shape[0] == nblk * spf
    y = dd.read()
    g = orc.disperse_geometry(16e6, 1000., 1, -100.)
    h = orc.chirp(n, 16e6, 1000., 1, -100., g['reference_frequency'])
    for m in (0, 7, nblk - 1):
        want = orc.disperse_block(x[m * spf:m * spf + n], h, g['pad_start'], spf)
        assert_parity(y[m * spf:(m + 1) * spf], want, f'block {m}')
    # Parseval per spectrum: sum|Z|^2 = n sum|y|^2
    dd.seek(0)
    ch = bt.Channelize(dd, 1024, 512)
    z = ch.read()
    nspec = z.shape[0]
    pz = (np.abs(z.astype(np.complex128)) ** 2).sum(axis=(1, 2))
    py = (np.abs(y[:nspec * 1024].astype(np.complex128)) ** 2).reshape(nspec, -1).sum(1)
    np.testing.assert_allclose(pz, 1024 * py, rtol=2e-6)
    # round trip: Disperse(Dedisperse(x)) returns x away from the ends
    rt = bt.Disperse(dd, 100.)
    shift = dd._pad_start + rt._pad_start
    rt.seek(3 * spf)
    got = rt.read(4096)
    want = x[3 * spf + shift:3 * spf + shift + 4096]
    # limited by wrap-around leakage of the chirp's band-edge tails, not by arithmetic:
    # the float64 oracle gives rel-L2 9.4e-4, max 0.043 for this geometry
    assert np.abs(got - want).max() < 0.1
    assert rel_l2(got, want) < 5e-3


def test_many_blocks_in_one_call_match_the_oracle_block_by_block():
    """The shape of the timed bench call: ONE read_device covering many
    overlap-save blocks (max_frames_per_call >= 64: many chunk launches
    alternating the plan's lanes, a ragged last chunk, a seam fix per block
    boundary).  (a) 70 blocks of 2^17 (two-level 256 x 512, like the headline's
    256 x 4096): every block and every seam spectrum against the oracle.
    (b) 70 blocks of 2^20 (the headline geometry itself) in one call: sampled
    blocks against the oracle, and the whole result bit-identical to the same
    stream read in calls of at most 6 blocks."""
    # ---- (a)
    n, nblk = 2**17, 70
    nh0 = noise(8 * n, (2,), n, seed=77, fs=2 * u.MHz, frequency=400 * u.MHz, sideband=1)
    dd0 = bt.Dedisperse(nh0, 30., samples_per_frame=None)
    pad = dd0._pad_start + dd0._pad_end
    spf = n - pad
    assert dd0._ih_samples_per_frame == n and 0 < pad < n // 2
    length = (nblk - 1) * spf + n + 1000           # + a short re-aligned last block
    x = orc.noise_stream(77, 0, length, n, (2,))
    ds = bt.DeviceStream(x, T0, 2 * u.MHz, frequency=400 * u.MHz, sideband=1)
    dd = bt.Dedisperse(ds, 30., samples_per_frame=spf)
    assert dd._ih_samples_per_frame == n and dd.shape[0] == nblk * spf + 1000
    info = dd._get_plan().info()
    dd.max_frames_per_call = nblk + 1
    assert (nblk + 1) % info['chunk_blocks'] != 0 and nblk + 1 > 4 * info['chunk_blocks']
    y = dd.read_device(dd.shape[0]).to_host()
    want, oinfo = orc.dedisperse(x, 2e6, 400., 1, 30., samples_per_frame=spf, ih_samples_per_frame=n,
                                 fast_len=HipFFTMaker.next_fast_len)
    assert oinfo['ih_spf'] == n
    for m in range(nblk + 1):
        assert_parity(y[m * spf:(m + 1) * spf], want[m * spf:(m + 1) * spf], f'block {m}')
    dd.seek(0)
    ch = bt.Channelize(dd, 512, samples_per_frame=64)
    assert ch._fusable_input() is dd
    ch.max_frames_per_call = 10**6
    nspec = (dd.shape[0] // 512 // 64) * 64
    z = ch.read_device(nspec).to_host()
    wantz = orc.channelize(want[:nspec * 512], 512)
    for m in range(nblk):
        k = (m + 1) * spf // 512                    # the spectrum straddling seam m | m + 1
        if k + 1 < nspec:
            assert_parity(z[k - 1:k + 2], wantz[k - 1:k + 2], f'seam {m}')
    assert_parity(z, wantz, 'all spectra')
    del x, y, z, want, wantz, ds, dd, ch
    # ---- (b)
    n, spf, nblk = 2**20, 836100, 70
    length = (nblk - 1) * spf + n
    rng = np.random.default_rng(5)
    base = rng.standard_normal((2**20, 4), dtype=np.float32).view(np.complex64)
    reps = -(-length // 2**20)
    x = np.concatenate([base * np.complex64(np.exp(0.37j * r)) for r in range(reps)])[:length]
    ds = bt.DeviceStream(x, T0, 16 * u.MHz, frequency=1000 * u.MHz, sideband=1)
    dd = bt.Dedisperse(ds, 100.)
    ch = bt.Channelize(dd, 1024, 512)
    dd.max_frames_per_call = nblk
    ch.max_frames_per_call = 10**6
    nspec = (dd.shape[0] // 1024 // 512) * 512
    z = ch.read_device(nspec).to_host()
    g = orc.disperse_geometry(16e6, 1000., 1, -100.)
    h = orc.chirp(n, 16e6, 1000., 1, -100., g['reference_frequency'])
    for m in (0, 5, 6, 35, nblk - 2):               # 6-block chunks: 5 | 6 is also a chunk (lane) seam
        yy = np.concatenate([orc.disperse_block(x[b * spf:b * spf + n], h, g['pad_start'], spf)
                             for b in (m, m + 1)])
        s0 = -(-m * spf // 1024)
        s1 = min((m + 2) * spf // 1024, nspec)
        wantz = orc.channelize(yy[s0 * 1024 - m * spf:s1 * 1024 - m * spf], 1024)
        assert_parity(z[s0:s1], wantz, f'blocks {m}, {m + 1}')
    dd2 = bt.Dedisperse(ds, 100.)
    ch2 = bt.Channelize(dd2, 1024, 512)
    dd2.max_frames_per_call = 6
    ch2.max_frames_per_call = 8
    assert np.array_equal(ch2.read(nspec), z)


def test_one_call_past_2_32_elements_repeats_with_the_period_of_its_input():
    """Maximum sizes: ONE `read_device` of the metric pipeline whose input (35 GB) and
    result (28 GB) each hold more than 2^32 float32 pairs -- 2600 blocks of 2^20, 3.4
    times the bench's call, every index past 32 bits.  No oracle runs at this size; the
    property used is periodicity: the input repeats every spf = 836100 samples, so
    every block transforms the same 2^20 samples and the spectra repeat every
    lcm(spf, 1024) / 1024 = 209025 spectra (256 blocks) BIT FOR BIT, whichever chunk,
    lane and seam slot a block falls on; the first period is checked against the
    oracle where it starts."""
    n, spf, nblk = 2**20, 836100, 2600
    period = spf * 256 // 1024                       # spectra
    rng = np.random.default_rng(11)
    one = rng.standard_normal((spf, 4), dtype=np.float32).view(np.complex64)
    length = (nblk - 1) * spf + n
    hip = bt.hip
    try:
        x = hip.DeviceArray((length, 2), np.complex64)
    except hip.HipError as exc:
        pytest.skip(f"no room for a {length * 16 / 1e9:.0f} GB stream: {exc}")
    x[:spf].copy_from_host(one)
    have = spf
    while have < length:                             # doubling device-to-device copies
        m = min(have, length - have)
        x[have:have + m].copy_from_device(x[:m])
        have += m
    ds = bt.DeviceStream(x, T0, 16 * u.MHz, frequency=1000 * u.MHz, sideband=1)
    dd = bt.Dedisperse(ds, 100.)
    assert dd._ih_samples_per_frame == n and dd.samples_per_frame == spf
    ch = bt.Channelize(dd, 1024, 512)
    nspec = (dd.shape[0] // 1024 // 512) * 512
    assert nspec * 1024 * 2 > 2**32 and nspec > 10 * period
    try:
        z = ch.read_device(nspec)
    except hip.HipError as exc:
        pytest.skip(f"no room for the {nspec * 16384 / 1e9:.0f} GB result: {exc}")
    assert z.shape == (nspec, 1024, 2)
    first = z[:period].to_host()
    # the first period against the oracle: the spectra inside block 0, and across the seam 0 | 1
    g = orc.disperse_geometry(16e6, 1000., 1, -100.)
    h = orc.chirp(n, 16e6, 1000., 1, -100., g['reference_frequency'])
    block = np.concatenate([one, one])[:n]
    y = orc.disperse_block(block, h, g['pad_start'], spf)
    yy = np.concatenate([y, y])
    k1 = spf // 1024                                 # the spectrum that straddles blocks 0 | 1
    assert_parity(first[:64], orc.channelize(yy[:64 * 1024], 1024), 'first spectra')
    assert_parity(first[k1 - 8:k1 + 8], orc.channelize(yy[(k1 - 8) * 1024:(k1 + 8) * 1024], 1024), 'seam 0 | 1')
    # every later period, whole, bit for bit
    step = 8192
    for j in range(1, nspec // period + 1):
        lo, hi = j * period, min((j + 1) * period, nspec)
        for a in range(lo, hi, step):
            b = min(a + step, hi)
            assert np.array_equal(z[a:b].to_host(), first[a - lo:b - lo]), (j, a)


def _periodic_on_device(one, length):
    """(length,) + one.shape[1:] in HBM, the rows of `one` over and over (doubling device copies);
    skips the test when the GPU has no room."""
    hip = bt.hip
    try:
        x = hip.DeviceArray((length,) + one.shape[1:], one.dtype)
    except hip.HipError as exc:
        pytest.skip(f"no room for a {length * one[0].nbytes / 1e9:.0f} GB stream: {exc}")
    have = len(one)
    x[:have].copy_from_host(one)
    while have < length:
        m = min(have, length - have)
        x[have:have + m].copy_from_device(x[:m])
        have += m
    return x


def _same_as_first_period(z, first, what):
    period, step = len(first), max(1, (1 << 27) // first[0].nbytes)
    for lo in range(period, z.shape[0], period):
        hi = min(lo + period, z.shape[0])
        for a in range(lo, hi, step):
            b = min(a + step, hi)
            assert np.array_equal(z[a:b].to_host(), first[a - lo:b - lo]), (what, a)


def test_neighbouring_kernels_past_2_32_elements():
    """The same maximum-size check for the one-kernel tasks: filter bank, channelizer
    and sample shifts on streams of more than 2^32 float32 pairs in ONE read each (34-39
    GB in, as much out).  Periodic input: the first period against the oracle (the
    shifts: all of it, exactly), every later one bit-identical to the first."""
    rng = np.random.default_rng(12)
    # ---- PolyphaseFilterBank 12 x 1024, 2 pol: period 4 x 1013 spectra (whole frames, whole workgroups)
    resp = bt.sinc_hamming(12, 1024)
    period = 4 * 1013
    one = rng.standard_normal((period * 1024, 4), dtype=np.float32).view(np.complex64)
    nper = 2**32 // (period * 1024 * 2) + 2
    x = _periodic_on_device(one, nper * period * 1024)
    ds = bt.DeviceStream(x, T0, 16 * u.MHz, frequency=1000 * u.MHz, sideband=1)
    pfb = bt.PolyphaseFilterBank(ds, resp)
    nspec = pfb.shape[0] - pfb.shape[0] % period
    assert nspec * 1024 * 2 > 2**32
    try:
        z = pfb.read_device(nspec)
    except bt.hip.HipError as exc:
        pytest.skip(f"no room for the result: {exc}")
    first = z[:period].to_host()
    want = orc.channelize(orc.ppf_samples(one[:(64 + 11) * 1024], orc.sinc_hamming(12, 1024)), 1024)
    assert_parity(first[:64], want, 'filter bank, first spectra')
    _same_as_first_period(z, first, 'filter bank')
    del z, first, pfb
    # ---- Channelize(1024) on the same stream
    ch = bt.Channelize(ds, 1024, 1024)
    nspec = ch.shape[0] - ch.shape[0] % period
    z = ch.read_device(nspec)
    first = z[:period].to_host()
    assert_parity(first[:256], orc.channelize(one[:256 * 1024], 1024), 'channelizer, first spectra')
    _same_as_first_period(z, first, 'channelizer')
    del z, first, ch, ds, x
    bt.hip.pool_trim()
    # ---- ShiftSamples, (n, 8) streams each with its own shift: a pure gather, checked exactly
    period = 1 << 16
    one = rng.standard_normal((period, 16), dtype=np.float32).view(np.complex64)
    shift = np.array([0, 3, 17, 2, 40, 41, 9, 1])
    n = (2**32 // 8 // period + 2) * period
    x = _periodic_on_device(one, n)
    ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=period)
    sh = bt.ShiftSamples(ds, shift, samples_per_frame=period)
    count = (sh.shape[0] // period) * period
    assert count * 8 > 2**32
    z = sh.read_device(count)
    off = shift.max() - shift
    want = one[(np.arange(period)[:, None] + off[None]) % period, np.arange(8)[None]]
    assert np.array_equal(z[:period].to_host(), want)
    _same_as_first_period(z, want, 'sample shifts')


@pytest.mark.parametrize('n_fft,n_chan', [(2**11, 0), (2**13, 0), (2**14, 0), (2**15, 0), (2**15, 256), (2**17, 64),
                                          (6174, 0), (30000, 0)])
def test_hundreds_of_short_blocks_in_one_call(n_fft, n_chan):
    """Short blocks by the hundred in ONE call: runs of regular blocks go to the kernels as one
    descriptor and a hop (`OsmChunk::reg_count`), launches hold as many blocks as the work
    buffer does, the fused channelizer's shifts and seam slots follow from the hop, a re-aligned
    last block ends the run.  Against the oracle, and bit for bit against the same stream read
    in calls of at most sixteen blocks (the descriptor-per-block route)."""
    fs, dm = 1e6, (5. if n_fft >= 4096 else 1.2)
    nh0 = noise(4 * n_fft, (2,), n_fft, seed=3, fs=fs, frequency=300 * u.MHz, sideband=1)
    pad = (lambda d: d._pad_start + d._pad_end)(bt.Dedisperse(nh0, dm))
    assert pad < n_fft // 2
    spf = n_fft - pad
    nblk = 333
    length = nblk * spf + pad + spf // 3                    # + a re-aligned last block
    x = orc.noise_stream(3, 0, length, n_fft, (2,))
    ds = bt.DeviceStream(x, T0, fs, frequency=300 * u.MHz, sideband=1)
    want, info = orc.dedisperse(x, fs, 300., 1, dm, samples_per_frame=spf, ih_samples_per_frame=n_fft,
                                fast_len=HipFFTMaker.next_fast_len)
    assert info['ih_spf'] == n_fft

    def task(per_call):
        dd = bt.Dedisperse(ds, dm, samples_per_frame=spf)
        assert dd._ih_samples_per_frame == n_fft
        top = bt.Channelize(dd, n_chan, samples_per_frame=7) if n_chan else dd
        if n_chan and n_fft >= 2**15:
            assert top._fusable_input() is dd
        dd.max_frames_per_call = per_call
        top.max_frames_per_call = 10**6 if per_call > 16 else max(1, per_call * spf // (7 * max(n_chan, 1)))
        return top
    whole = task(10**6)
    assert whole.ih._get_plan().info()['chunk_blocks'] <= 16 if n_chan else True
    got = whole.read_device(whole.shape[0]).to_host()
    ref = orc.channelize(want[:got.shape[0] * n_chan], n_chan) if n_chan else want
    assert got.shape == ref.shape
    assert_parity(got, ref, f'{nblk} blocks of {n_fft}, {n_chan} channels')
    pieces = task(16)
    assert np.array_equal(pieces.read(), got)
    whole.seek(whole.shape[0] // 2 + 5)
    assert np.array_equal(whole.read(1000), got[whole.shape[0] // 2 + 5:whole.shape[0] // 2 + 1005])


def test_random_runs_of_many_short_blocks():
    """Randomised version of the test above (seedable with BBT_TEST_SEED): block length, number of
    blocks, stream shape (one stream, odd counts, several pairs) and channelizer on top."""
    rng = np.random.default_rng(909 + int(os.environ.get('BBT_TEST_SEED', '0')))
    fs = 1e6
    for case in range(6):
        n_fft = int(rng.choice([2**11, 2**12, 2**13, 2**14, 2**15, 2**16, 2**17, 3000, 6174, 30000]))
        shape = [(2,), (), (3,), (2, 2)][case % 4]
        dm = 5. if n_fft >= 4096 else 1.2
        g = orc.disperse_geometry(fs, 300., 1, -dm)
        pad = g['pad_start'] + g['pad_end']
        spf = n_fft - pad
        nblk = int(rng.integers(17, 1 + max(18, min(700, (1 << 23) // n_fft))))
        length = nblk * spf + pad + int(rng.integers(0, spf))
        x = (rng.standard_normal((length,) + shape) + 1j * rng.standard_normal((length,) + shape)).astype(np.complex64)
        ds = bt.DeviceStream(x, T0, fs, frequency=300 * u.MHz, sideband=1)
        n_chan = 0
        if n_fft >= 2**15 and n_fft & (n_fft - 1) == 0 and case % 2:
            n_chan = 256
        want, info = orc.dedisperse(x, fs, 300., 1, dm, samples_per_frame=spf, ih_samples_per_frame=min(length, 4096),
                                    fast_len=HipFFTMaker.next_fast_len)
        assert info['ih_spf'] == n_fft
        res = []
        for per_call in (10**6, 16):
            dd = bt.Dedisperse(ds, dm, samples_per_frame=spf)
            assert dd._ih_samples_per_frame == n_fft
            top = bt.Channelize(dd, n_chan, samples_per_frame=5) if n_chan else dd
            dd.max_frames_per_call = per_call
            top.max_frames_per_call = 10**6 if per_call > 16 else max(1, per_call * spf // (5 * max(n_chan, 1)))
            res.append(top.read_device(top.shape[0]).to_host())
        ref = orc.channelize(want[:res[0].shape[0] * n_chan], n_chan) if n_chan else want
        what = f'case {case}: {nblk} blocks of {n_fft}, shape {shape}, {n_chan} channels'
        assert res[0].shape == ref.shape, what
        assert_parity(res[0], ref, what)
        assert np.array_equal(res[0], res[1]), what


def test_chirp_made_on_the_gpu_equals_the_reference_attribute():
    """The plan's chirp is made on the GPU in float64 (`bbt_chirp`) instead of being evaluated on
    the host and uploaded; `phase_factor` stays the reference's attribute (dispersion.py:115-129).
    Both are float64 results rounded to complex64: they agree to a rounding of the last bit (the
    phase itself, up to 10^6 cycles for config 4, to 1e-9 cycle) -- scalar and per-stream
    frequencies and sidebands, a reference frequency outside the band (sample offset), odd and
    even block lengths, both signs of DM."""
    cases = [
        dict(n=2**20, fs=16e6, f=1000e6, sb=1, dm=100., ref=None, shape=(2,)),
        dict(n=2**20, fs=16e6, f=1000e6, sb=np.array([1, -1]), dm=100., ref=None, shape=(2,)),
        dict(n=6561, fs=1e6, f=np.array([[300e6], [301e6]]), sb=np.array([[1], [-1]]), dm=5., ref=300.7e6, shape=(2, 2)),
        dict(n=30000, fs=1e6, f=300e6, sb=-1, dm=5., ref=299.2e6, shape=(3,)),
        dict(n=2**20, fs=6.25e6, f=(403.125e6 + 6.25e6 * np.arange(8)).reshape(8, 1), sb=1, dm=30.,
             ref=(403.125e6 + 6.25e6 * np.arange(8)).reshape(8, 1), shape=(8, 2)),
        dict(n=2**24, fs=6.25e6, f=403.125e6, sb=1, dm=557., ref=None, shape=(2,)),      # config 4's worst sub-band
    ]
    for case in cases:
        for cls in (bt.Dedisperse, bt.Disperse):
            nh = bt.EmptyStreamGenerator((2**27,) + case['shape'], T0, case['fs'], samples_per_frame=case['n'],
                                         frequency=case['f'], sideband=case['sb'], dtype=np.complex64)
            kw = {} if case['ref'] is None else dict(reference_frequency=case['ref'])
            probe = cls(nh, case['dm'], **kw)
            spf = case['n'] - probe._pad_start - probe._pad_end
            host = cls(nh, case['dm'], samples_per_frame=spf, **kw)
            host.DEVICE_CHIRP = False
            want, want_index = host._response_columns()
            dev = cls(nh, case['dm'], samples_per_frame=spf, **kw)
            assert dev._ih_samples_per_frame == case['n']
            if not dev.DEVICE_CHIRP:
                pytest.skip('device chirp switched off (BBT_DEVICE_CHIRP=0)')
            got, got_index = dev._response_columns()
            assert isinstance(got, bt.hip.DeviceArray) and dev._phase_factor is None
            got = got.to_host()
            assert got.shape == want.shape and np.array_equal(got_index, want_index)
            err = np.abs(got.astype(np.complex128) - want.astype(np.complex128)).max()
            assert err < 2.5e-7, (cls.__name__, case['n'], err)
            assert np.mean(got == want) > 0.9, (cls.__name__, case['n'], np.mean(got == want))


@pytest.mark.parametrize('n_fft', [2**15, 2**16])
def test_sixteen_streams_on_blocks_with_16_point_columns(n_fft):
    """16 x N2 blocks with many streams: the column passes' lanes run over 8 stream pairs first
    (whole lines of every complete sample; `k_osm_col16<..., PP = 8>`) -- per-sub-band
    frequencies and reference frequencies (the CHIME-native form of config 4), plain
    output and the fused channelizer, against the oracle."""
    freq = (400. + 0.39 * np.arange(8)).reshape(8, 1) * u.MHz
    fs, dm = 0.39 * u.MHz, 60.
    nh0 = noise(8 * n_fft, (8, 2), n_fft, seed=5, fs=fs, frequency=freq, sideband=1)
    pad = (lambda d: d._pad_start + d._pad_end)(bt.Dedisperse(nh0, dm, reference_frequency=freq))
    assert pad < n_fft // 2
    spf = n_fft - pad
    length = 3 * spf + pad + 555
    x = orc.noise_stream(5, 0, length, n_fft, (8, 2))
    ds = bt.DeviceStream(x, T0, fs, frequency=freq, sideband=1)
    want, info = orc.dedisperse(x, 0.39e6, np.asarray(freq) / 1e6, 1, dm, reference_frequency_mhz=np.asarray(freq) / 1e6,
                                samples_per_frame=spf, ih_samples_per_frame=n_fft)
    dd = bt.Dedisperse(ds, dm, reference_frequency=freq, samples_per_frame=spf)
    assert dd._ih_samples_per_frame == n_fft and dd._get_plan().info()['n1'] == 16
    assert_parity(dd.read(), want, f'16 streams, blocks of {n_fft}')
    ch = bt.Channelize(bt.Dedisperse(ds, dm, reference_frequency=freq, samples_per_frame=spf), 256, 5)
    assert ch._fusable_input() is not None
    z = ch.read()
    assert_parity(z, orc.channelize(want[:z.shape[0] * 256], 256), f'fused channelizer, 16 streams, blocks of {n_fft}')


def test_device_memory_pool_reuses_blocks():
    """bbt_malloc/bbt_free cache blocks (the per-call output arrays of a reader
    must not cost a hipMalloc + synchronising hipFree each)."""
    import os
    if os.environ.get('BBT_POOL') == '0':
        pytest.skip("device memory pool switched off by BBT_POOL=0")
    hip = bt.hip
    hip.pool_trim()
    a = hip.DeviceArray((1 << 20, 2), np.complex64)
    ptr, nbytes = a.ptr, a.nbytes
    cached0, live0 = hip.pool_info()
    assert live0 >= nbytes
    del a
    cached1, live1 = hip.pool_info()
    assert cached1 - cached0 >= nbytes and live0 - live1 >= nbytes
    b = hip.DeviceArray(((1 << 20) - 1000, 2), np.complex64)      # slightly smaller: same block
    assert b.ptr == ptr
    c = hip.DeviceArray((1 << 20, 2), np.complex64)               # block in use: a new one
    assert c.ptr != ptr
    x = np.arange(16, dtype=np.float32).view(np.complex64).reshape(4, 2)
    d = hip.DeviceArray.from_host(x) if hasattr(hip.DeviceArray, 'from_host') else None
    del b, c, d
    hip.pool_trim()
    assert hip.pool_info()[0] == 0


@pytest.mark.parametrize('sample_shape,dtype', [((2,), np.complex64), ((3,), np.complex64),
                                                ((2, 2), np.complex64), ((2,), np.float32)])
def test_direct_and_fourier_convolution_agree(sample_shape, dtype, monkeypatch):
    """Short responses are convolved in the time domain (k_fir), long ones in
    the Fourier domain; both are the linear convolution the reference keeps
    (convolution.py:116-120), so they must agree with each other and with the
    oracle for real, complex and per-stream responses."""
    n = 3 * 4096 + 321
    nh = bt.NoiseGenerator((n,) + sample_shape, T0, 1 * u.MHz, 4096, seed=21, dtype=dtype,
                           frequency=300 * u.MHz, sideband=1)
    x = nh.read()
    rng = np.random.default_rng(5)
    n_stream = int(np.prod(sample_shape))
    responses = [rng.standard_normal(129),                                          # real, shared
                 rng.standard_normal((40,) + sample_shape)]                         # real, per stream
    if dtype == np.complex64:
        responses.append(rng.standard_normal(33) + 1j * rng.standard_normal(33))    # complex
    for resp in responses:
        direct = bt.Convolve(nh, resp, offset=7)
        assert direct._use_fir()
        got = direct.read()
        monkeypatch.setattr(bt.Convolve, 'FIR_MAX_TAPS', 0)
        monkeypatch.setattr(bt.Convolve, 'FIR_MAX_TAPS_COMPLEX', 0)
        fourier = bt.Convolve(nh, resp, offset=7)
        assert not fourier._use_fir()
        want_gpu = fourier.read()
        monkeypatch.undo()
        # (the oracle's convolve is written for complex streams; a real stream is its real part)
        want, geo = orc.convolve(x.astype(np.complex64), resp if resp.ndim > 1 or len(sample_shape) == 1
                                 else resp.reshape((-1,) + (1,) * len(sample_shape)), offset=7,
                                 ih_samples_per_frame=4096, fast_len=HipFFTMaker().next_fast_len)
        assert got.shape == want.shape == want_gpu.shape and got.dtype == dtype
        if dtype == np.float32:
            want = want.real if np.iscomplexobj(want) else want
        for a, what in ((got, 'direct'), (want_gpu, 'fourier')):
            e2, em = rel_l2(a, want), max_over_rms(a, want)
            assert e2 <= REL_L2_TOL and em <= MAX_TOL, (what, resp.shape, e2, em)
    # the LO phase of ShiftAndResample makes the taps complex per stream
    if dtype == np.complex64:
        shift = np.linspace(-0.3, 0.4, n_stream).reshape(sample_shape)
        sr = bt.ShiftAndResample(nh, shift, lo=299.5 * u.MHz, pad=32)
        assert sr._use_fir()
        got = sr.read()
        monkeypatch.setattr(bt.Convolve, 'FIR_MAX_TAPS_COMPLEX', 0)
        sr2 = bt.ShiftAndResample(nh, shift, lo=299.5 * u.MHz, pad=32)
        assert not sr2._use_fir()
        want = sr2.read()
        monkeypatch.undo()
        assert rel_l2(got, want) <= REL_L2_TOL and max_over_rms(got, want) <= MAX_TOL


@pytest.mark.parametrize('sample_shape', [(2,), (2, 2)])
def test_fused_detection_matches_stored_spectra(sample_shape, monkeypatch):
    """Integrate(Power|Square(Channelize(Dedisperse))) sums the power in the
    last pass of the overlap-save plan (float atomics); it must equal
    detecting the stored spectra, and the oracle, for steps that do and do not
    divide the spectra of a block, with a start offset, and fall back when a
    workgroup would touch too many bins."""
    import baseband_tasks_amd.channelize as chz
    pol = ['X', 'Y']
    nh = noise(3 * 2**18 + 5000, sample_shape, 2**18, seed=31, frequency=1000 * u.MHz, sideband=1,
               polarization=pol)
    ds = bt.DeviceStream(nh, T0, 16 * u.MHz)
    x = orc.noise_stream(31, 0, nh.shape[0], 2**18, sample_shape)
    y, info = orc.dedisperse(x, 16e6, 1000., 1, 30., ih_samples_per_frame=2**18)
    n_chan = 256
    n_spec = (y.shape[0] // (n_chan * 32)) * 32          # whole frames of 32 spectra
    z = orc.channelize(y[:n_spec * n_chan], n_chan)
    for detect, mode in ((bt.Power, 1), (bt.Square, 0)):
        for step, start in ((64, 0), (100, 7), (17 * 4, 3), (1000, 0)):
            def build():
                dd = bt.Dedisperse(ds, 30.)
                assert dd._ih_samples_per_frame == 2**18
                ch = bt.Channelize(dd, n_chan, 32)
                return bt.Integrate(detect(ch), step, start=start, samples_per_frame=1)
            it = build()
            plan = it.ih.ih.ih._get_plan()
            assert plan.detect_bins_max(n_chan, step) <= 64
            got = it.read()
            monkeypatch.setattr(chz, 'FUSE_DETECTION', False)
            want_gpu = build().read()
            monkeypatch.undo()
            det = orc.power(z) if mode else orc.square(z)
            want = orc.integrate(det, step, start=start)
            assert got.shape == want_gpu.shape == want.shape and got.dtype == np.float32
            _close(got, want_gpu, rtol=2e-6)
            _close(got, want, rtol=1e-5)
    # sums with counts (average=False) through the fused route
    summed = bt.Integrate(bt.Power(bt.Channelize(bt.Dedisperse(ds, 30.), n_chan, 32)), 64, average=False).read()
    assert np.all(summed['count'] == 64)
    _close(summed['data'], 64. * orc.integrate(orc.power(z), 64), rtol=1e-5)
    # a step too short for the fused route (more than 64 bins per workgroup) still works
    it = bt.Integrate(bt.Power(bt.Channelize(bt.Dedisperse(ds, 30.), n_chan, 32)), 8)
    assert it.ih.ih.ih._get_plan().detect_bins_max(n_chan, 8) > 64
    _close(it.read(), orc.integrate(orc.power(z), 8), rtol=1e-5)


@pytest.mark.parametrize('sample_shape', [(2,), (2, 2)])
def test_detection_without_integration_in_the_last_pass(sample_shape, monkeypatch):
    """Power|Square(Channelize(Dedisperse)) on its own (no Integrate): the last pass of the
    overlap-save plan stores the powers where the spectra would have gone (plain stores, step 1 of
    the fused route; reference functions.py:15-16, 131-143 on channelize.py:73-74).  Equal to
    detecting the stored spectra and to the oracle, also for reads that start and end inside
    frames."""
    import baseband_tasks_amd.channelize as chz
    nh = noise(3 * 2**18 + 5000, sample_shape, 2**18, seed=33, frequency=1000 * u.MHz, sideband=1,
               polarization=['X', 'Y'])
    ds = bt.DeviceStream(nh, T0, 16 * u.MHz)
    x = orc.noise_stream(33, 0, nh.shape[0], 2**18, sample_shape)
    y, info = orc.dedisperse(x, 16e6, 1000., 1, 30., ih_samples_per_frame=2**18)
    n_chan = 256
    n_spec = (y.shape[0] // (n_chan * 32)) * 32
    z = orc.channelize(y[:n_spec * n_chan], n_chan)
    calls = []
    real = bt.hip.OsmPlan.execute_channelized_detect
    monkeypatch.setattr(bt.hip.OsmPlan, 'execute_channelized_detect',
                        lambda self, *a, **k: (calls.append(a[-3]), real(self, *a, **k))[1])
    for detect, want in ((bt.Power, orc.power(z)), (bt.Square, orc.square(z))):
        def build():
            return detect(bt.Channelize(bt.Dedisperse(ds, 30.), n_chan, 32))
        task = build()
        del calls[:]
        got = task.read()
        assert calls and all(step == 1 for step in calls), calls
        assert got.shape == want.shape and got.dtype == np.float32
        _close(got, want, rtol=1e-5)
        task.seek(1000)
        _close(task.read(777), want[1000:1777], rtol=1e-5)
        monkeypatch.setattr(chz, 'FUSE_DETECTION', False)
        del calls[:]
        stored = build().read()
        assert not calls
        monkeypatch.setattr(chz, 'FUSE_DETECTION', True)
        _close(got, stored, rtol=2e-6)


def test_subband_shards_equal_columns_of_the_whole():
    """Config-4 style sharding: a rank's run of sub-bands is the same series as
    those columns of the whole stream (bit-exact through a per-stream filter),
    and dedisperses with its own chirp columns to the oracle's result."""
    from baseband_tasks_amd import sharding
    freq = (400. + 6.25 * np.arange(6)).reshape(6, 1) * u.MHz
    nh = noise(3 * 2**14, (6, 2), 2**14, seed=41, fs=6.25 * u.MHz, frequency=freq, sideband=1,
               polarization=['X', 'Y'])
    x = nh.read()
    resp = np.random.default_rng(2).standard_normal((31, 6, 2))
    whole = bt.Convolve(nh, resp).read()
    for world in (2, 3):
        parts = []
        for rank in range(world):
            mine = sharding.SubbandShard(nh, rank, world)
            lo, hi = mine.subbands
            assert mine.shape == (nh.shape[0], hi - lo, 2) and np.all(mine.frequency == freq[lo:hi] * 1.)
            assert np.array_equal(mine.read(), x[:, lo:hi])
            mine.seek(1000)
            assert np.array_equal(mine.read_device(77).to_host(), x[1000:1077, lo:hi])
            mine.seek(0)
            parts.append(bt.Convolve(mine, resp[:, lo:hi]).read())
            dd = bt.Dedisperse(mine, 0.5, reference_frequency=mine.frequency)
            want, info = orc.dedisperse(x[:, lo:hi], 6.25e6, np.asarray(freq[lo:hi]) / 1e6, 1, 0.5,
                                        reference_frequency_mhz=np.asarray(freq[lo:hi]) / 1e6,
                                        ih_samples_per_frame=2**14,
                                        fast_len=HipFFTMaker.next_fast_len)
            assert dd._ih_samples_per_frame == info['ih_spf']
            assert_parity(dd.read(), want, f'shard {rank}/{world}')
        assert np.array_equal(np.concatenate(parts, axis=1), whole)


@pytest.mark.parametrize('n_fft', [256, 512, 1024, 2048, 4096])
def test_single_kernel_blocks_with_many_streams(n_fft, monkeypatch):
    """Blocks of <= 4096 samples run as one kernel whose lanes go over groups
    of stream pairs (2, 4 or 8) first; 16 and 6 streams take the grouped and
    the one-pair-per-workgroup variants."""
    monkeypatch.setattr(bt.Convolve, 'FIR_MAX_TAPS', 0)
    resp = np.random.default_rng(8).standard_normal(20)
    for shape in ((8, 2), (3, 2)):
        nh = noise(5 * n_fft, shape, n_fft, seed=51, fs=1 * u.MHz, frequency=300 * u.MHz, sideband=1)
        cv = bt.Convolve(nh, resp, samples_per_frame=n_fft - 19)
        assert not cv._use_fir() and cv._ih_samples_per_frame == n_fft
        want, _ = orc.convolve(nh.read(), resp.reshape(-1, 1, 1), samples_per_frame=n_fft - 19,
                               ih_samples_per_frame=n_fft, fast_len=HipFFTMaker.next_fast_len)
        assert_parity(cv.read(), want, f'n_fft={n_fft} streams {shape}')


def test_sixteen_streams_through_the_column_passes():
    """Eight stream pairs: the 256-point column passes put the lanes of a row
    over the pairs (whole cache lines of each complete sample); plain,
    channelized and detected outputs against the oracle."""
    n_fft = 2**17
    freq = (400. + 6.25 * np.arange(8)).reshape(8, 1) * u.MHz
    nh = noise(3 * n_fft, (8, 2), n_fft, seed=61, fs=6.25 * u.MHz, frequency=freq, sideband=1,
               polarization=['X', 'Y'])
    dd = bt.Dedisperse(nh, 3., reference_frequency=freq)
    x = nh.read()
    want, info = orc.dedisperse(x, 6.25e6, np.asarray(freq) / 1e6, 1, 3.,
                                reference_frequency_mhz=np.asarray(freq) / 1e6,
                                ih_samples_per_frame=n_fft, fast_len=HipFFTMaker.next_fast_len)
    assert dd._ih_samples_per_frame == info['ih_spf'] == n_fft
    assert dd._get_plan().info()['n1'] == 256
    assert_parity(dd.read(), want, 'dedisperse 16 streams')
    ch = bt.Channelize(bt.Dedisperse(nh, 3., reference_frequency=freq), 256, 4)
    assert ch._fusable_input() is not None
    z = ch.read()
    wz = orc.channelize(want[:z.shape[0] * 256], 256)
    assert_parity(z, wz, 'fused channelizer 16 streams')
    it = bt.Integrate(bt.Power(bt.Channelize(bt.Dedisperse(nh, 3., reference_frequency=freq), 256, 4)), 64)
    _close(it.read(), orc.integrate(orc.power(wz), 64), rtol=1e-5)


@pytest.mark.parametrize('sample_shape', [(2,), (4,), (3, 2)])
def test_real_stream_pairs_run_as_complex_streams(sample_shape, monkeypatch):
    """Two neighbouring float32 streams with the same response are one
    complex64 stream to the overlap-save plan (a real impulse response acts on
    real and imaginary parts separately): same result as the zero-extended
    route and as the oracle's rfft/irfft restatement."""
    from baseband_tasks_amd.overlap_save import SpectralMultiplyTask
    n_fft = 2**14
    nr = bt.NoiseGenerator((3 * n_fft + 777,) + sample_shape, T0, 1 * u.MHz, n_fft, dtype=np.float32,
                           seed=71, frequency=300 * u.MHz, sideband=1)
    x = nr.read()
    want, info = orc.dedisperse(x, 1e6, 300., 1, 5., ih_samples_per_frame=n_fft,
                                fast_len=HipFFTMaker.next_fast_len)
    dd = bt.Dedisperse(nr, 5.)
    assert dd._ih_samples_per_frame == info['ih_spf']
    got = dd.read()
    assert dd._paired and got.dtype == np.float32
    monkeypatch.setattr(SpectralMultiplyTask, 'PAIR_REAL_STREAMS', False)
    d1 = bt.Dedisperse(nr, 5.)
    unpaired = d1.read()
    assert not d1._paired
    monkeypatch.undo()
    rms = np.sqrt(np.mean(want.astype(float) ** 2))
    for a, what in ((got, 'paired'), (unpaired, 'zero-extended')):
        assert np.linalg.norm(a - want) / np.linalg.norm(want) <= REL_L2_TOL, what
        assert np.abs(a - want).max() <= MAX_TOL * rms, what
    nr.seek(0)
    blk = nr.read(n_fft)
    assert np.array_equal(dd.task(blk), got[:dd.samples_per_frame])          # the host-data hook
    # per-stream frequencies: nothing to pair, still correct
    if sample_shape == (2,):
        nq = bt.NoiseGenerator((3 * n_fft,) + sample_shape, T0, 1 * u.MHz, n_fft, dtype=np.float32,
                               seed=71, frequency=np.array([300., 301.]) * u.MHz, sideband=1)
        dq = bt.Dedisperse(nq, 5.)
        yq = dq.read()
        assert not dq._paired
        nq.seek(0)
        wq, _ = orc.dedisperse(nq.read(), 1e6, np.array([300., 301.]), 1, 5., ih_samples_per_frame=n_fft,
                               fast_len=HipFFTMaker.next_fast_len)
        assert yq.shape == wq.shape
        assert np.linalg.norm(yq - wq) / np.linalg.norm(wq) <= REL_L2_TOL


def test_real_stream_pairs_through_channelizer_and_filter_bank(monkeypatch):
    """Channelize / Dechannelize / PolyphaseFilterBank transform two real
    streams as one complex stream a + i b and separate the spectra afterwards;
    same results as one zero-extended transform per stream and as the oracle."""
    import baseband_tasks_amd.channelize as chz
    for shape in ((2,), (6,), (2, 2)):
        nr = bt.NoiseGenerator((40 * 256,) + shape, T0, 1 * u.MHz, 2560, dtype=np.float32, seed=81,
                               frequency=300 * u.MHz, sideband=1)
        x = nr.read()
        results = {}
        for pair in (True, False):
            monkeypatch.setattr(chz._RowFFTTask, 'PAIR_REAL_STREAMS', pair)
            ch = bt.Channelize(nr, 256, samples_per_frame=4)
            assert bool(ch._pairs()) == pair
            z = ch.read()
            ch.seek(0)
            back = bt.Dechannelize(ch, n=256, dtype=np.float32).read()
            pf = bt.PolyphaseFilterBank(nr, bt.sinc_hamming(4, 256), samples_per_frame=8).read()
            results[pair] = (z, back, pf)
        monkeypatch.undo()
        z, back, pf = results[True]
        want = orc.channelize(x[:z.shape[0] * 256], 256)
        assert z.shape == want.shape == (40, 129) + shape
        assert_parity(z, want, f'real channelize {shape}')
        assert np.abs(back - x[:back.shape[0]]).max() < 1e-5
        for a, b, what in zip(results[True], results[False], ('channelize', 'dechannelize', 'pfb')):
            assert a.shape == b.shape and a.dtype == b.dtype
            scale = np.sqrt(np.mean(np.abs(b) ** 2))
            assert np.abs(a - b).max() <= MAX_TOL * scale, (what, shape)


@pytest.mark.parametrize('dtype', [np.float32, np.complex64])
def test_resampled_tones_match_the_finer_grid(dtype):
    """Analytic check in the spirit of the reference's TestResampleReal /
    TestResampleComplex (tests/test_sampling.py:77-261): two tones sampled at a
    quarter of the rate, resampled onto quarter-sample offsets with a 65-tap
    windowed sinc, reproduce the fully sampled signal to 7e-4 (the
    reference's tolerance), for Resample and for per-stream ShiftAndResample."""
    full_rate, n_full, pad = 1e3, 3 * 4096, 32
    f_tone = full_rate * 2 / 4096 * np.array([31.092, 65.1234])          # Hz, one per stream

    def tones(fh):
        t = (fh.tell() + np.arange(fh.samples_per_frame)) / fh.sample_rate
        phi = np.pi / 180. * np.pi + 2. * np.pi * f_tone * t[:, np.newaxis]
        return (np.cos(phi) if np.dtype(dtype).kind == 'f' else np.exp(1j * phi)).astype(dtype)

    def stream(rate, n, spf):
        return bt.StreamGenerator(tones, (n, 2), T0, rate, samples_per_frame=spf, dtype=dtype,
                                  frequency=400e3, sideband=np.array([-1, 1]))

    full = stream(full_rate, n_full, 4096).read()
    part_fh = stream(full_rate / 4, n_full // 4, 1024)
    assert np.allclose(part_fh.read(), full[::4], atol=1e-6)
    for offset in (34, 34.5, 35.75):
        ih = bt.Resample(part_fh, offset, pad=pad)
        assert ih.shape[0] == part_fh.shape[0] - 2 * pad and ih.tell() + pad == round(offset)
        ih.seek(0)
        data = ih.read()
        first = (ih.start_time - part_fh.start_time) * full_rate            # in full-rate samples
        assert abs(first - round(first)) < 1e-6
        expected = full[int(round(first))::4][:data.shape[0]]
        assert data.dtype == dtype and np.abs(data - expected).max() < 7e-4
    shift = np.array([1.75, 10.25])
    ih = bt.ShiftAndResample(part_fh, shift, offset=0.25, pad=pad)
    data = ih.read()
    for i, s in enumerate(shift):
        first = ((ih.start_time - part_fh.start_time) * full_rate / 4 - s) * 4
        assert abs(first - round(first)) < 1e-6 and first >= 0
        expected = full[int(round(first))::4, i][:data.shape[0]]
        assert np.abs(data[:, i] - expected).max() < 7e-4


def test_convolve_equals_numpy_convolve():
    """Independent of the oracle (which, like the reference, goes through FFTs):
    Convolve keeps the 'valid' part of the linear convolution, shifted by
    ``offset`` (reference tests/test_convolution.py:42-98 compare the same way)."""
    rng = np.random.default_rng(12)
    nh = noise(6000, (2,), 1000, seed=91, fs=1 * u.kHz)
    x = nh.read().astype(np.complex128)
    for n_tap, offset in ((3, 0), (3, 1), (40, 7), (300, 0)):
        resp = rng.standard_normal(n_tap)
        cv = bt.Convolve(nh, resp, offset=offset)
        got = cv.read()
        want = np.stack([np.convolve(x[:, k], resp, mode='valid') for k in range(2)], axis=1)
        assert got.shape == want.shape
        assert_parity(got, want.astype(np.complex64), f'{n_tap} taps')
        # the result is attributed to input sample pad_start = n_tap - 1 - offset
        assert abs((cv.start_time - nh.start_time) * 1e3 - (n_tap - 1 - offset)) < 1e-9


@pytest.mark.parametrize('shape', [(2,), (8,), (1,), (3,)])
def test_convolve_on_short_blocks_matches_numpy_and_direct_filter(shape):
    """The short-block route of `Convolve` (medium responses: transform, multiply and inverse of
    2048-sample blocks in one kernel, whatever the frame length) against numpy.convolve and
    against the direct filter: the linear convolution does not depend on the block geometry
    (reference convolution.py:116-120).  Ragged ends: the last block is re-aligned."""
    rng = np.random.default_rng(77)
    n = 3 * 2**15 + 1234
    nh = noise(n, shape, 2**15, seed=92, fs=1 * u.kHz)
    x = nh.read().astype(np.complex128)
    for n_tap, offset in ((129, 64), (65, 0), (300, 17)):
        resp = rng.standard_normal((n_tap,) + shape) if n_tap == 65 else rng.standard_normal(n_tap)
        cv = bt.Convolve(nh, resp, offset=offset)
        assert cv._short_blocks() is not None
        assert cv._short_blocks()._ih_samples_per_frame == {129: 1024, 65: 1024, 300: 4096}[n_tap]
        got = cv.read()
        full = np.broadcast_to(resp.reshape(n_tap, -1) if resp.ndim > 1 else resp[:, None], (n_tap, shape[0]))
        want = np.stack([np.convolve(x[:, k], full[:, k], mode='valid') for k in range(shape[0])], axis=1)
        assert got.shape == want.shape
        assert_parity(got, want.astype(np.complex64), f'{n_tap} taps on short blocks')
        if n_tap <= 160:
            direct = bt.Convolve(nh, resp, offset=offset)
            direct.SHORT_BLOCK = 0
            assert direct._short_blocks() is None and direct._use_fir()
            assert_parity(got, direct.read(), f'{n_tap} taps: short blocks against the direct filter')
        # piecewise reads (frames of the task, spans that do not start at 0) give the same samples
        cv.seek(5000)
        assert np.array_equal(cv.read(40000), got[5000:45000])


@pytest.mark.parametrize('n_fft,n1', [(2**21, 512), (2**22, 16)])
def test_blocks_longer_than_2_20_with_sixteen_streams(n_fft, n1):
    """2^21- / 2^22-sample blocks x 16 streams: plain and fused-channelizer outputs (256,
    64 and 16 channels); 2^21 on two levels, 512 x 4096 (the 512-point column pass), 2^22 with
    stream pairs in eights on three (256 x 16 x 1024: its column passes take 8 pairs at once)."""
    freq = (400. + 6.25 * np.arange(8)).reshape(8, 1) * u.MHz
    nh = noise(n_fft + 300000, (8, 2), 2**19, seed=63, fs=6.25 * u.MHz, frequency=freq, sideband=1)
    x = nh.read()
    dm = 60. if n_fft == 2**21 else 120.          # (padding 2^19 .. 2^20 quarter-blocks: the power-of-two rule gives 2^22)
    pow2 = HipFFTMaker(power_of_two=True)
    want, info = orc.dedisperse(x, 6.25e6, np.asarray(freq) / 1e6, 1, dm,
                                reference_frequency_mhz=np.asarray(freq) / 1e6,
                                ih_samples_per_frame=2**19, fast_len=pow2.next_fast_len)
    with bt.fft_maker.set(pow2):
        dd = bt.Dedisperse(nh, dm, reference_frequency=freq)
        assert dd._ih_samples_per_frame == info['ih_spf'] == n_fft
        assert dd._get_plan().info()['n1'] == n1
        assert_parity(dd.read(), want, 'dedisperse, 16 streams')
        ds = bt.DeviceStream(x, T0, 6.25 * u.MHz, frequency=freq, sideband=1)     # (re-reading the noise
        for n in (256, 64, 16):                                                      # generator per call is slow)
            ch = bt.Channelize(bt.Dedisperse(ds, dm, reference_frequency=freq), n, 2048 // n * 8)
            assert ch._fusable_input() is not None
            z = ch.read()
            assert_parity(z, orc.channelize(want[:z.shape[0] * n], n), f'fused channelizer {n}, 16 streams')


@pytest.mark.parametrize('n_chan', [16, 32, 64, 128])
@pytest.mark.parametrize('sample_shape', [(2,), (4, 2)])
def test_fused_channelizer_with_few_channels(n_chan, sample_shape, monkeypatch):
    """Channelize(n < 256) folded into the overlap-save plan (an extra exchange
    plus wavefront shuffles in the row pass): equal to the oracle and to the
    unfused route, seam spectra included; 2^17-sample blocks (256 x 512)."""
    from baseband_tasks_amd import channelize as chmod
    n = 2**17
    nh0 = noise(4 * n, sample_shape, n, seed=91, fs=2 * u.MHz, frequency=400 * u.MHz, sideband=1)
    spf = n - (lambda d: d._pad_start + d._pad_end)(bt.Dedisperse(nh0, 30.))
    length = 3 * spf + n + 777
    nh = noise(length, sample_shape, n, seed=91, fs=2 * u.MHz, frequency=400 * u.MHz, sideband=1)
    x = orc.noise_stream(91, 0, length, n, sample_shape)
    want_y, info = orc.dedisperse(x, 2e6, 400., 1, 30., samples_per_frame=spf, ih_samples_per_frame=n)
    assert info['ih_spf'] == n
    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(chmod, 'FUSE_WITH_OVERLAP_SAVE', fuse)
        ch = bt.Channelize(bt.Dedisperse(nh, 30., samples_per_frame=spf), n_chan, samples_per_frame=37)
        assert (ch._fusable_input() is not None) == fuse
        z = ch.read()
        assert_parity(z, orc.channelize(want_y[:z.shape[0] * n_chan], n_chan), f'fuse={fuse}')
        k = spf // n_chan
        ch.seek(k - 2)
        assert np.array_equal(ch.read(5), z[k - 2:k + 3])
        res[fuse] = z
    assert rel_l2(res[True], res[False]) < 3e-7


def test_config4_share_of_one_rank():
    """Config 4 at its real size on one GPU: 8 sub-bands x 2 pol,
    6.25 MHz each, DM 557, one 2^24-sample block plus a re-aligned final one,
    Channelize(64) fused; three of the sub-bands against the oracle (float64
    FFTs of 2^24 points take seconds each)."""
    from baseband_tasks_amd import sharding
    n_fft, spf = 2**24, 2**24 - 2756522
    n_in = n_fft + 2**20
    rng = np.random.default_rng(44)
    x = rng.standard_normal((n_in, 8, 4), dtype=np.float32).view(np.complex64)       # (n, 8, 2)
    band = (403.125e6 + 6.25e6 * np.arange(64)).reshape(64, 1)
    freq = band[:8]
    ds = bt.DeviceStream(x, T0, 6.25 * u.MHz, frequency=freq, sideband=1)
    dd = sharding.SubbandDedisperse(ds, 557., band_frequency=band, band_reference_frequency=band,
                                    reference_frequency=freq, samples_per_frame=spf)
    assert (dd._pad_start, dd._pad_end, dd._ih_samples_per_frame) == (1362235, 1394287, n_fft)
    assert dd._get_plan().info()['n1'] == 16            # three levels: 256 x 16 x 4096
    ch = bt.Channelize(dd, 64, samples_per_frame=1024)
    assert ch._fusable_input() is dd
    z = ch.read()
    assert z.shape == ((n_in - 2756522) // 64 // 1024 * 1024, 64, 8, 2)
    for k in (0, 3, 7):
        f0 = float(freq[k, 0]) / 1e6
        want, info = orc.dedisperse(np.ascontiguousarray(x[:, k]), 6.25e6, f0, 1, 557.,
                                    reference_frequency_mhz=f0, samples_per_frame=spf,
                                    ih_samples_per_frame=2**20)
        if k == 0:
            assert (info['pad_start'], info['ih_spf']) == (1362235, n_fft)
            wy = want
        else:                  # the whole band's padding, not the sub-band's own
            g = dict(pad_start=1362235, pad_end=1394287, ih_spf=n_fft, spf=spf,
                     n_out=n_in - 2756522)
            h = orc.chirp(n_fft, 6.25e6, f0, 1, -557., f0)
            wy = orc.overlap_save(np.ascontiguousarray(x[:, k]), g,
                                  lambda blk: orc.disperse_block(blk, h, 1362235, spf))
        assert_parity(z[:, :, k], orc.channelize(wy[:z.shape[0] * 64], 64), f'sub-band {k}')


def test_rccl_entry_points_of_the_c_abi():
    """bbt_comm_* / bbt_bcast_chirp / bbt_gather_output: a
    one-rank communicator on this GPU (more ranks need more GPUs; the call
    sequence is the same)."""
    uid = bt.hip.comm_unique_id()
    assert len(uid) == bt.hip.COMM_ID_BYTES
    comm = bt.hip.Comm(1, 0, uid)
    rng = np.random.default_rng(3)
    h = (rng.standard_normal((2, 4096)) + 1j * rng.standard_normal((2, 4096))).astype(np.complex64)
    d = bt.hip.DeviceArray.from_host(h)
    comm.bcast_chirp(d, root=0)
    assert np.array_equal(d.to_host(), h)
    out = comm.gather_output(d)
    assert out.shape == (2, 4096) and np.array_equal(out.to_host(), h)
    odd = bt.hip.DeviceArray.from_host(np.arange(7, dtype=np.uint8))
    assert np.array_equal(comm.gather_output(odd).to_host(), np.arange(7, dtype=np.uint8))
    comm.close()
    with pytest.raises(bt.hip.HipError):
        bt.hip.Comm(2, 5, uid)


@pytest.mark.parametrize('bits,complex_data', [(2, False), (2, True), (1, False), (4, True), (8, True), (16, False)])
def test_vdif_frames_are_unpacked_on_the_device(bits, complex_data):
    """SURVEY 8f rank 3 (parity unpinned: the reference holds no decoder and no
    VDIF file; this checks the device unpacking against this package's own
    restatement of the VDIF 1.1.1 packing).  Two threads x four channels, EDV 3
    sample rate, frames that straddle a second."""
    from baseband_tasks_amd import ingest
    rng = np.random.default_rng(bits)
    n, n_thread, n_chan, spf = 8 * 640, 2, 4, 640
    levels = {1: [-1., 1.], 2: [-3.3359, -1., 1., 3.3359],
              4: (np.arange(16, dtype=np.float32) - np.float32(8.)) / np.float32(2.95),
              8: (np.arange(256, dtype=np.float32) - np.float32(127.5)) / np.float32(35.5),
              16: np.arange(-300., 300.)}[bits]
    comp = rng.choice(np.asarray(levels, dtype=np.float32), size=(n, n_thread, n_chan * (2 if complex_data else 1)))
    data = comp.view(np.complex64) if complex_data else comp
    fs = 32e6
    raw = ingest.encode_vdif_frames(data, bits, seconds=100, ref_epoch=41, frame_nr0=49998,
                                    frames_per_second=50000, samples_per_frame=spf, edv=3, sample_rate=fs)
    fh = bt.open_vdif(raw, frequency=300 * u.MHz, sideband=1)
    assert fh.shape == (n, n_thread, n_chan) and fh.dtype == (np.complex64 if complex_data else np.float32)
    assert fh.sample_rate == fs and fh.samples_per_frame == spf
    assert abs((fh.start_time - bt.Time('2020-07-01T00:01:40')) - 49998 * spf / fs) < 1e-9
    same = np.array_equal if bits not in (4, 8) else (lambda a, b: np.allclose(a, b, rtol=3e-7, atol=0))   # (a division)
    assert same(fh.read(), data)
    fh.seek(1000)
    assert same(fh.read_device(700).to_host(), data[1000:1700])
    # feeds the path without touching the host again
    if complex_data and bits == 2:
        dd = bt.Dedisperse(fh, 0.003, samples_per_frame=1024)
        want, _ = orc.dedisperse(data, fs, 300., 1, 0.003, samples_per_frame=1024, ih_samples_per_frame=spf)
        assert_parity(dd.read(), want, 'Dedisperse(open_vdif(...))')
    hdr = ingest.vdif_header(np.frombuffer(raw[:32], '<u4'))
    assert (hdr['bits'], hdr['n_chan'], hdr['complex_data'], hdr['frame_nr'], hdr['edv']) == \
        (bits, n_chan, complex_data, 49998, 3)


def test_packed_frames_are_read_ahead_through_the_host_pipeline(monkeypatch):
    """Frames in file order go up through `host_pipeline.HostUploader` (run m + 1 copied to
    page-locked memory and uploaded while run m is unpacked and processed): same samples as the
    synchronous upload, from pageable and from page-locked bytes, alone and in front of the path."""
    from baseband_tasks_amd import host_pipeline as hp
    from baseband_tasks_amd import ingest
    rng = np.random.default_rng(77)
    n, per, header = 40 * 1024, 1024, 32
    frame = header + per * 4
    raw = rng.integers(0, 256, size=(n // per) * frame, dtype=np.uint8)
    pinned = hp.pinned_empty(raw.shape, np.uint8)
    pinned[...] = raw

    def stream(buf):
        return ingest.RawFrameStream(buf, frame_nbytes=frame, header_nbytes=header, samples_per_frame=per, bits=8,
                                     n_chan=2, complex_data=True, start_time=T0, sample_rate=1e6,
                                     frequency=300 * u.MHz, sideband=1)

    def results():
        out = []
        for buf in (raw, pinned):
            fh = stream(buf)
            fh.max_frames_per_call = 7                      # several runs per read
            out.append(fh.read())
            dd = bt.Dedisperse(stream(buf), 5., samples_per_frame=2**13 - 767 - 771)
            dd.ih.max_frames_per_call = 7
            dd.max_frames_per_call = 2
            out.append(dd.read())
            dd.seek(4321)
            out.append(dd.read(9999))
        return out

    if not hp.ENABLED:
        pytest.skip('host pipeline switched off (BBT_HOST_PIPELINE=0)')
    fetched = []
    real = hp.HostUploader.fetch
    monkeypatch.setattr(hp.HostUploader, 'fetch', lambda self, *a: (fetched.append(a), real(self, *a))[1])
    piped = results()
    assert len(fetched) > 10
    monkeypatch.setattr(hp, 'ENABLED', False)
    n_fetched = len(fetched)
    plain = results()
    assert len(fetched) == n_fetched
    for a, b in zip(piped, plain):
        assert a.shape == b.shape and np.array_equal(a, b)
    want = (raw.reshape(-1, frame)[:, header:].astype(np.float32) - np.float32(127.5)) / np.float32(35.5)
    assert np.allclose(piped[0], want.reshape(n, 2, 2).view(np.complex64)[..., 0], rtol=3e-7, atol=0)


def test_vdif_frames_out_of_order_invalid_or_missing():
    """open_vdif reads every header: frames shuffled in the file come back in
    time and thread order; a frame flagged invalid and a frame that is not in
    the file at all read as zeros; a duplicated frame counts once (parity
    unpinned, as for the decoder itself: `baseband` fills such frames with its
    fill value 0)."""
    from baseband_tasks_amd import ingest
    rng = np.random.default_rng(17)
    n_sets, n_thread, n_chan, spf = 12, 2, 4, 160
    levels = np.array([-3.3359, -1., 1., 3.3359], np.float32)
    data = rng.choice(levels, size=(n_sets * spf, n_thread, n_chan * 2)).view(np.complex64)
    raw = ingest.encode_vdif_frames(data, 2, seconds=7, ref_epoch=41, frame_nr0=24996, frames_per_second=25000,
                                    samples_per_frame=spf, edv=3, sample_rate=4e6)
    nb = len(raw) // (n_sets * n_thread)
    frames = [bytearray(raw[i * nb:(i + 1) * nb]) for i in range(n_sets * n_thread)]      # (set, thread) order
    frames[2 * 5 + 1][3] |= 0x80                          # set 5, thread 1: invalid flag (bit 31 of word 0)
    gone = 2 * 8 + 0                                      # set 8, thread 0: not in the file
    order = [i for i in rng.permutation(len(frames)) if i != gone]
    order.insert(3, 2 * 2 + 1)                            # set 2, thread 1 twice (the later copy is garbage)
    shuffled = [bytes(frames[i]) for i in order]
    late = len(shuffled) - 1 - order[::-1].index(2 * 2 + 1)
    shuffled[late] = shuffled[late][:32] + bytes(len(shuffled[late]) - 32)
    fh = bt.open_vdif(b''.join(shuffled), frequency=300 * u.MHz, sideband=1)
    assert fh.shape == (n_sets * spf, n_thread, n_chan) and fh.sample_rate == 4e6
    assert abs((fh.start_time - bt.Time('2020-07-01T00:00:07')) - 24996 * spf / 4e6) < 1e-9
    want = data.copy()
    want[5 * spf:6 * spf, 1] = 0.
    want[8 * spf:9 * spf, 0] = 0.
    assert np.array_equal(fh.read(), want)
    fh.seek(7 * spf + 11)
    assert np.array_equal(fh.read(2 * spf), want[7 * spf + 11:9 * spf + 11])
    # a complete file in order takes the direct route
    assert bt.open_vdif(raw)._frame_map is None and fh._frame_map is not None


def test_dada_samples_are_unpacked_on_the_device():
    """PSRDADA: ASCII header + signed 8-bit (time, pol, re/im) samples (parity unpinned)."""
    rng = np.random.default_rng(8)
    n = 4096 + 512
    samples = rng.integers(-128, 128, size=(n, 2, 2), dtype=np.int8)          # (time, pol, re/im)
    header = ("HDR_VERSION 1.0\nHDR_SIZE 4096\nNBIT 8\nNDIM 2\nNPOL 2\nNCHAN 1\nTSAMP 0.0625\n"
              "UTC_START 2020-01-01-00:00:00\nOBS_OFFSET 6400\nFREQ 1000.0\nBW 16\n")
    raw = header.encode().ljust(4096, b'\0') + samples.tobytes()
    fh = bt.open_dada(raw, frequency=1000 * u.MHz, sideband=1)
    assert fh.shape == (n - n % fh.samples_per_frame, 2)            # (time, pol); the unit channel axis is dropped
    want = samples.astype(np.float32).view(np.complex64).reshape(n, 2)
    got = fh.read()
    assert got.dtype == np.complex64
    assert np.array_equal(got, want[:got.shape[0]])
    assert fh.sample_rate == 16e6
    assert abs((fh.start_time - bt.Time('2020-01-01T00:00:00')) - 1600 / 16e6) < 1e-12


def test_random_overlap_save_geometries():
    """Randomised block lengths (powers of two and other 2^a 3^b 5^c 7^d), response
    lengths and offsets, stream shapes and ragged stream ends against the oracle."""
    rng = np.random.default_rng(2024 + int(os.environ.get('BBT_TEST_SEED', '0')))
    lengths = [64, 128, 256, 512, 1024, 4096, 8192, 16384, 65536, 300, 1000, 1536, 2187, 6174, 7000, 8192 * 3,
               10000, 30000, 46080]
    shapes = [(2,), (3,), (2, 2), (), (4,)]
    limit_r, limit_c = bt.Convolve.FIR_MAX_TAPS, bt.Convolve.FIR_MAX_TAPS_COMPLEX
    bt.Convolve.FIR_MAX_TAPS = bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0          # always the block transform
    try:
        for case in range(24):
            n_fft = int(rng.choice(lengths))
            shape = shapes[case % len(shapes)]
            n_tap = int(rng.integers(2, max(3, n_fft // 3)))
            offset = int(rng.integers(0, n_tap))
            n_in = int(n_fft * rng.integers(1, 4) + rng.integers(0, n_fft))
            resp = (rng.standard_normal((n_tap,) + shape) + 1j * rng.standard_normal((n_tap,) + shape)) / np.sqrt(n_tap)
            resp = resp.astype(np.complex64)
            x = (rng.standard_normal((n_in,) + shape) + 1j * rng.standard_normal((n_in,) + shape)).astype(np.complex64)
            ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=min(n_in, 1000))
            cv = bt.Convolve(ds, resp, offset=offset, samples_per_frame=n_fft - n_tap + 1)
            assert cv._ih_samples_per_frame == n_fft, (case, n_fft, n_tap)
            want, info = orc.convolve(x, resp, offset=offset, samples_per_frame=n_fft - n_tap + 1,
                                      ih_samples_per_frame=min(n_in, 1000))
            got = cv.read()
            assert_parity(got, want, f'case {case}: n_fft {n_fft} taps {n_tap} offset {offset} shape {shape} n_in {n_in}')
            # a read from the middle equals the whole
            if got.shape[0] > 10:
                a = int(rng.integers(0, got.shape[0] - 5))
                cv.seek(a)
                assert np.array_equal(cv.read(5), got[a:a + 5])
    finally:
        bt.Convolve.FIR_MAX_TAPS, bt.Convolve.FIR_MAX_TAPS_COMPLEX = limit_r, limit_c


def test_random_fused_channelizer_geometries():
    """Randomised block length / channel count / framing for Channelize on top of
    Dedisperse (fused route), against the oracle: every spectrum, seams included."""
    rng = np.random.default_rng(77 + int(os.environ.get('BBT_TEST_SEED', '0')))
    for case in range(48):
        n_fft = int(2 ** rng.integers(13, 18))
        n_chan = int(rng.choice([16, 32, 64, 128, 256, 512, 1024, 2048, 4096]))
        fs = 2e6
        dm = float(rng.uniform(2., 8.))
        g = orc.disperse_geometry(fs, 400., 1, -dm)
        pad = g['pad_start'] + g['pad_end']
        if pad >= n_fft // 2 or n_chan > n_fft - pad:
            continue
        spf = n_fft - pad
        n_in = int(spf * rng.integers(2, 5) + pad + rng.integers(0, spf))
        sample_shape = (2,) if case % 3 else (2, 2)
        x = (rng.standard_normal((n_in,) + sample_shape) + 1j * rng.standard_normal((n_in,) + sample_shape)).astype(np.complex64)
        ds = bt.DeviceStream(x, T0, fs, frequency=400 * u.MHz, sideband=1)
        dd = bt.Dedisperse(ds, dm, samples_per_frame=spf)
        assert dd._ih_samples_per_frame == n_fft
        ch = bt.Channelize(dd, n_chan, samples_per_frame=int(min(rng.integers(1, 40), dd.shape[0] // n_chan)))
        plan = dd._get_plan()
        y, _ = orc.dedisperse(x, fs, 400., 1, dm, samples_per_frame=spf, ih_samples_per_frame=min(n_in, 4096))
        z = ch.read()
        want = orc.channelize(y[:z.shape[0] * n_chan], n_chan)
        assert_parity(z, want, f'case {case}: n_fft {n_fft} n_chan {n_chan} fused={plan.fusable(n_chan)} '
                               f'frames of {ch.samples_per_frame} n_in {n_in} shape {sample_shape}')


@pytest.mark.parametrize('n_fft,n_chan,detect', [
    (2**14, 1024, False),      # one kernel (16384-point transform), the channelizer after it
    (2**15, 2048, False),      # 16 x 2048: one spectrum per row
    (2**16, 4096, False),      # 16 x 4096
    (2**18, 128, False),       # few channels (lane exchange)
    (2**18, 1024, False),      # 256 x 1024
    (2**18, 1024, True),       # ... with the powers summed in the last pass
    (2**20, 4096, False),      # 256 x 4096
    (2**21, 512, False),       # 512 x 4096 (512-point column pass)
    (2**22, 2048, False),      # 1024 x 4096 (1024-point column pass)
    (2**23, 512, False),       # three levels, 256 x 16 x 2048
    (2**23, 64, False),        # ... few channels
    (2**24, 1024, False),      # 256 x 16 x 4096
])
def test_channel_count_larger_than_the_padding(n_fft, n_chan, detect):
    """When n_chan exceeds the block's padding, the last n_chan-aligned group of a
    block both wraps around the block end and holds the end of the kept range:
    it is the tail half of a seam spectrum (and, wrapped, possibly the head half
    of another one).  Every seam spectrum must match the oracle."""
    rng = np.random.default_rng(n_fft // n_chan)
    fs, n_tap = 2e6, 57                                  # padding 56 < every n_chan here
    resp = (rng.standard_normal(n_tap) + 1j * rng.standard_normal(n_tap)).astype(np.complex64)
    spf = n_fft - n_tap + 1
    n_in = 3 * spf + n_tap - 1 + 777
    x = (rng.standard_normal((n_in, 2)) + 1j * rng.standard_normal((n_in, 2))).astype(np.complex64)
    limit = bt.Convolve.FIR_MAX_TAPS_COMPLEX
    bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0                 # the Fourier-domain plan, not the direct FIR
    try:
        ds = bt.DeviceStream(x, T0, fs, polarization=['X', 'Y'])
        cv = bt.Convolve(ds, resp, samples_per_frame=spf)
        assert cv._ih_samples_per_frame == n_fft
        plan = cv._get_plan()
        # (8192 / 16384 samples: one kernel, nothing to fuse into -- unless BBT_OSM_NO_BIG keeps them on two levels)
        assert plan.fusable(n_chan) == (n_fft > 2**14 or bool(os.environ.get('BBT_OSM_NO_BIG')))
        ch = bt.Channelize(cv, n_chan, samples_per_frame=3)
        y = np.stack([np.convolve(x[:, k].astype(np.complex128), resp.astype(np.complex128), mode='valid')
                      for k in range(2)], axis=1)
        n_spec = y.shape[0] // n_chan
        want = orc.channelize(y[:n_spec * n_chan].astype(np.complex64), n_chan)
        if detect:
            got = bt.Integrate(bt.Power(ch), 64, samples_per_frame=1).read()
            _close(got, orc.integrate(orc.power(want), 64), rtol=2e-5)
        else:
            got = ch.read()                                # whole frames of three spectra
            assert n_spec - 3 < got.shape[0] <= n_spec
            assert_parity(got, want[:got.shape[0]], f'n_fft {n_fft} n_chan {n_chan}')
    finally:
        bt.Convolve.FIR_MAX_TAPS_COMPLEX = limit


def test_random_windows_of_the_fused_channelizer():
    """Random (seek, count) reads of Channelize(Dedisperse) and of
    Integrate(Power(...)) against slices of the oracle's whole result: windows
    that start and stop inside blocks, single spectra, seams first or last."""
    rng = np.random.default_rng(5 + int(os.environ.get('BBT_TEST_SEED', '0')))
    fs = 2e6
    for n_fft, n_chan, dm in ((2**16, 2048, 3.), (2**18, 256, 6.), (2**18, 64, 2.5), (2**15, 512, 7.)):
        g = orc.disperse_geometry(fs, 400., 1, -dm)
        pad = g['pad_start'] + g['pad_end']
        spf = n_fft - pad
        n_in = 5 * spf + pad + int(rng.integers(0, spf))
        x = (rng.standard_normal((n_in, 2)) + 1j * rng.standard_normal((n_in, 2))).astype(np.complex64)
        ds = bt.DeviceStream(x, T0, fs, frequency=400 * u.MHz, sideband=1, polarization=['X', 'Y'])
        y, _ = orc.dedisperse(x, fs, 400., 1, dm, samples_per_frame=spf, ih_samples_per_frame=min(n_in, 4096))
        n_spec = y.shape[0] // n_chan
        want = orc.channelize(y[:n_spec * n_chan], n_chan)
        dd = bt.Dedisperse(ds, dm, samples_per_frame=spf)
        assert dd._get_plan().fusable(n_chan)
        ch = bt.Channelize(dd, n_chan, samples_per_frame=1)
        assert ch.shape[0] == n_spec
        seam_spectra = [(k * spf) // n_chan for k in range(1, 5)]
        windows = [(s, 1) for s in seam_spectra[:2]] + [(seam_spectra[2], 2), (seam_spectra[3] - 1, 2)]
        for _ in range(10):
            a = int(rng.integers(0, n_spec - 1))
            windows.append((a, int(rng.integers(1, min(n_spec - a, 3 * spf // n_chan) + 1))))
        for a, count in windows:
            ch.seek(a)
            assert_parity(ch.read(count), want[a:a + count], f'n_fft {n_fft} n_chan {n_chan} window {a}+{count}')
        if n_chan >= 256:
            step = 16
            power = orc.integrate(orc.power(want), step)
            it = bt.Integrate(bt.Power(bt.Channelize(bt.Dedisperse(ds, dm, samples_per_frame=spf), n_chan,
                                                     samples_per_frame=1)), step, samples_per_frame=1)
            for _ in range(6):
                a = int(rng.integers(0, power.shape[0] - 1))
                count = int(rng.integers(1, power.shape[0] - a + 1))
                it.seek(a)
                _close(it.read(count), power[a:a + count], rtol=2e-5)


@pytest.mark.parametrize('n_chan', [6, 96, 100, 1000, 1536, 6000, 8192, 16384])
def test_filter_bank_with_any_channel_count(n_chan):
    """PolyphaseFilterBank for channel counts the fused FIR + FFT kernels do not take (the
    reference takes any n numpy.fft takes, pfb.py:128-154): the polyphase sum as a filter
    along the block axis, then the channelizer transform -- complex and float32 streams,
    odd stream counts, against the oracle."""
    rng = np.random.default_rng(n_chan)
    for shape, real, n_tap in (((2,), False, 4), ((3,), False, 12), ((2,), True, 8), ((), True, 5)):
        if real and n_chan % 2:
            continue
        ih_spf = n_chan * (n_tap + 9)
        n_in = ih_spf * 5
        if real:
            x = rng.standard_normal((n_in,) + shape).astype(np.float32)
        else:
            x = (rng.standard_normal((n_in,) + shape) + 1j * rng.standard_normal((n_in,) + shape)).astype(np.complex64)
        resp = orc.sinc_hamming(n_tap, n_chan) * 1.7
        ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=ih_spf)
        pfb = bt.PolyphaseFilterBank(ds, resp)
        want, geo = orc.polyphase_filter_bank(x, resp, ih_spf)
        assert pfb.samples_per_frame == geo['chan_spf']
        got = pfb.read()
        assert got.shape == want.shape
        assert_parity(got, want.astype(np.complex64), f'n {n_chan} taps {n_tap} {shape} real={real}')


def test_random_filter_bank_channelizer_and_resampler_geometries():
    """Randomised PolyphaseFilterBank (taps, channels, framing, real and complex
    streams, odd stream counts), Channelize (any 2^a 3^b 5^c 7^d channel count) and
    Resample (offsets, padding) against the oracle."""
    rng = np.random.default_rng(303 + int(os.environ.get('BBT_TEST_SEED', '0')))
    shapes = [(2,), (3,), (2, 2), (), (5,)]
    for case in range(12):
        n_chan = int(rng.choice([256, 512, 1024, 2048, 4096]))
        n_tap = int(rng.integers(2, 17))
        shape = shapes[case % len(shapes)]
        real = bool(case % 2)
        n_frames_in = int(rng.integers(8, 14))        # (the padded frame must fit the stream)
        ih_spf = int(n_chan * rng.integers(n_tap + 1, n_tap + 12))
        n_in = ih_spf * n_frames_in
        if real:
            x = rng.standard_normal((n_in,) + shape).astype(np.float32)
        else:
            x = (rng.standard_normal((n_in,) + shape) + 1j * rng.standard_normal((n_in,) + shape)).astype(np.complex64)
        resp = (orc.sinc_hamming(n_tap, n_chan) * rng.uniform(0.5, 2.)).astype(np.float64)
        ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=ih_spf)
        pfb = bt.PolyphaseFilterBank(ds, resp)
        want, geo = orc.polyphase_filter_bank(x, resp, ih_spf)
        assert pfb.samples_per_frame == geo['chan_spf']
        assert_parity(pfb.read(), want.astype(np.complex64), f'pfb case {case}: n {n_chan} taps {n_tap} {shape} real={real}')
    for case in range(12):
        n_chan = int(rng.choice([2, 6, 16, 24, 100, 243, 256, 343, 1000, 1536, 4096, 6000, 8192]))
        shape = shapes[case % len(shapes)]
        real = bool(case % 2) and n_chan % 2 == 0
        n_spec = int(rng.integers(3, 40))
        if real:
            x = rng.standard_normal((n_spec * n_chan + 3,) + shape).astype(np.float32)
        else:
            x = (rng.standard_normal((n_spec * n_chan + 3,) + shape)
                 + 1j * rng.standard_normal((n_spec * n_chan + 3,) + shape)).astype(np.complex64)
        ds = bt.DeviceStream(x, T0, 1 * u.MHz)
        ch = bt.Channelize(ds, n_chan, samples_per_frame=int(rng.integers(1, n_spec + 1)))
        got = ch.read()
        want = orc.channelize(x[:got.shape[0] * n_chan], n_chan)
        assert 0 < got.shape[0] <= (n_spec * n_chan + 3) // n_chan
        assert_parity(got, want.astype(np.complex64), f'channelize case {case}: n {n_chan} {shape} real={real}')
    for case in range(8):
        shape = shapes[case % len(shapes)]
        pad = int(rng.choice([16, 32, 64]))
        offset = float(rng.uniform(0., 3.))
        n_in = int(rng.integers(20000, 60000))
        ih_spf = int(rng.choice([1000, 4096, 10000]))
        n_in -= n_in % ih_spf
        x = (rng.standard_normal((n_in,) + shape) + 1j * rng.standard_normal((n_in,) + shape)).astype(np.complex64)
        ds = bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=ih_spf)
        rs = bt.Resample(ds, offset, pad=pad)
        want, info = orc.resample(x, offset, pad=pad, ih_samples_per_frame=ih_spf)
        rs.seek(0)
        assert_parity(rs.read(), want, f'resample case {case}: offset {offset} pad {pad} {shape}')
        assert abs((rs.start_time - ds.start_time) * 1e6 - info['start_shift_samples']) < 1e-6


def test_random_block_descriptors_through_the_c_abi():
    """bbt_osm_execute / bbt_osm_execute_channelized with descriptors the host
    classes never produce: every block with its own input offset, first kept
    sample (0 included: the spectrum before the block start then wraps around the
    block end) and kept count; the output stream starting anywhere.  Checked
    against a float64 numpy model of what the header promises."""
    from baseband_tasks_amd import hip
    rng = np.random.default_rng(909 + int(os.environ.get('BBT_TEST_SEED', '0')))
    lengths = [2**12, 2**13, 2**14, 2**15, 2**16, 2**17, 2**18, 2**19, 2**20, 2**21, 3000, 6174, 30000, 46080,
               131220]
    for case in range(12):
        n_fft = int(rng.choice(lengths))
        S = int(rng.choice([1, 2, 4, 6, 16]))
        if S == 1 and n_fft & (n_fft - 1):
            S = 2                                      # (one stream: power-of-two blocks only)
        n_resp = int(rng.choice([1, max(S // 2, 1), S]))
        resp = np.exp(2j * np.pi * rng.uniform(size=(n_resp, n_fft))) * rng.uniform(0.5, 1.5, size=(n_resp, n_fft))
        resp = resp.astype(np.complex64)
        index = None if n_resp == 1 else (np.arange(S, dtype=np.int32) * n_resp) // S    # one per stream or per pair
        plan = hip.OsmPlan(n_fft, S, resp, index)
        geo = plan.info()
        choices = [c for c in (16, 64, 128, 256, 512, 1024, 2048, 4096) if plan.fusable(c)]
        n_chan = int(rng.choice(choices)) if choices else 16          # (not fusable: plain only)
        n_blocks = int(rng.integers(2, 7 if S * n_fft <= 2**23 else 4))
        L = 3 * n_fft
        x = (rng.standard_normal((L, S)) + 1j * rng.standard_normal((L, S))).astype(np.complex64)
        in_off = rng.integers(0, L - n_fft + 1, size=n_blocks)
        vs = rng.integers(0, n_fft // 4, size=n_blocks)
        vs[rng.integers(0, n_blocks)] = 0
        vc = np.array([rng.integers(n_chan, n_fft - v + 1) for v in vs])
        vc[rng.integers(0, n_blocks)] = n_fft - vs[0] if rng.integers(0, 2) else n_chan
        vc = np.minimum(vc, n_fft - vs)
        out0 = int(rng.integers(0, 3 * n_chan))
        out_off = out0 + np.concatenate([[0], np.cumsum(vc)[:-1]])
        total = int(out_off[-1] + vc[-1])
        # the model: each block filtered on its own (circularly), kept part placed in the stream
        stream = np.zeros((total, S), np.complex128)
        h = resp.astype(np.complex128)[(index if index is not None else np.zeros(S, int))]      # (S, N)
        for b in range(n_blocks):
            blk = x[in_off[b]:in_off[b] + n_fft].astype(np.complex128)
            y = np.fft.ifft(np.fft.fft(blk, axis=0) * h.T, axis=0)
            stream[out_off[b]:out_off[b] + vc[b]] = y[vs[b]:vs[b] + vc[b]]
        x_dev = hip.DeviceArray.from_host(x)
        what = f'case {case}: n_fft {n_fft} S {S} n_chan {n_chan} vs {vs.tolist()} vc {vc.tolist()} out0 {out0}'
        plain = hip.DeviceArray((total, S), np.complex64).fill_bytes(0)
        plan.execute(x_dev, plain, in_off, out_off, vs, vc)
        got = plain.to_host()
        assert_parity(got[out0:], stream[out0:].astype(np.complex64), 'plain ' + what)
        assert not got[:out0].any()
        if geo['n1'] == 1 and S > 1 and not n_fft & (n_fft - 1):
            # the kept range in elements of the (row, stream) matrix (bbt_osm_execute_flat)
            first_elem = 2 * int(rng.integers(0, S // 2))
            fvs = rng.integers(0, n_fft // 4, size=n_blocks)
            room = (n_fft - fvs) * S - first_elem
            felems = np.array([2 * int(rng.integers(1, r // 2 + 1)) for r in room])
            foff = 2 * int(rng.integers(0, 8)) + np.concatenate([[0], np.cumsum(felems)[:-1]])
            flat_out = hip.DeviceArray((int(foff[-1] + felems[-1]) + 6,), np.complex64).fill_bytes(0)
            plan.execute_flat(x_dev, flat_out, in_off, foff, fvs, first_elem, felems)
            want_flat = np.zeros(flat_out.shape, np.complex128)
            for b in range(n_blocks):
                blk = x[in_off[b]:in_off[b] + n_fft].astype(np.complex128)
                y = np.fft.ifft(np.fft.fft(blk, axis=0) * h.T, axis=0).reshape(-1)
                a = fvs[b] * S + first_elem
                want_flat[foff[b]:foff[b] + felems[b]] = y[a:a + felems[b]]
            got_flat = flat_out.to_host()
            keep = want_flat != 0
            assert_parity(got_flat[keep], want_flat[keep].astype(np.complex64), 'flat ' + what)
            assert not got_flat[~keep].any()
        if not choices:
            continue
        first = -(-out0 // n_chan)
        n_spec = total // n_chan - first
        assert n_spec > 0
        want = np.fft.fft(stream[first * n_chan:(first + n_spec) * n_chan].reshape(n_spec, n_chan, S), axis=1)
        spectra = hip.DeviceArray((n_spec, n_chan, S), np.complex64).fill_bytes(0)
        plan.execute_channelized(x_dev, spectra.reshape(n_spec * n_chan, S), in_off, out_off, vs, vc, n_chan,
                                 first, n_spec)
        assert_parity(spectra.to_host(), want.astype(np.complex64), 'channelized ' + what)
        # a window of the spectra only
        if n_spec > 3:
            a = int(rng.integers(1, n_spec - 1))
            k = int(rng.integers(1, n_spec - a + 1))
            part = hip.DeviceArray((k, n_chan, S), np.complex64).fill_bytes(0)
            plan.execute_channelized(x_dev, part.reshape(k * n_chan, S), in_off, out_off, vs, vc, n_chan,
                                     first + a, k)
            assert_parity(part.to_host(), want[a:a + k].astype(np.complex64), 'window ' + what)
        # the powers summed in the last pass instead of stored spectra
        step = int(rng.integers(1, 40))
        if (S > 1 and geo['n1'] == 256 and n_fft <= 2**20 and n_chan >= 256 and n_spec >= step
                and plan.detect_bins_max(n_chan, step) <= 64):
            n_bins = n_spec // step
            mode = int(rng.integers(0, 2))
            z = want[:n_bins * step].reshape(n_bins, step, n_chan, S)
            if mode:
                zp = z.reshape(n_bins, step, n_chan, S // 2, 2)
                xx, yy = zp[..., 0], zp[..., 1]
                cross = xx * yy.conj()
                pw = np.stack([np.abs(xx) ** 2, np.abs(yy) ** 2, cross.real, cross.imag], axis=-1).mean(axis=1)
                shape = (n_bins, n_chan, S // 2, 4)
            else:
                pw = (np.abs(z) ** 2).mean(axis=1)
                shape = (n_bins, n_chan, S)
            det = hip.DeviceArray(shape, np.float32).fill_bytes(0)
            plan.execute_channelized_detect(x_dev, det, in_off, out_off, vs, vc, n_chan, first, n_bins, step, mode)
            d = det.to_host()
            scale = np.sqrt(np.mean(pw[..., :2] ** 2)) if mode else np.sqrt(np.mean(pw ** 2))
            assert np.abs(d - pw).max() <= 2e-5 * scale * max(1., np.sqrt(step)), ('detect ' + what, step, mode)


def test_host_threads_with_their_own_streams_and_plans():
    """Four host threads on one device, each with its own HIP stream and plans
    (and the shared twiddle-table caches, created concurrently on first use),
    plus two threads sharing ONE plan (its mutex serialises them): every result
    equals the single-threaded one bit for bit."""
    import ctypes as C
    import threading
    from baseband_tasks_amd import hip
    lib = hip.lib()
    rng = np.random.default_rng(4)
    jobs = []
    for n_fft, n_chan, S in ((2**15, 512, 2), (2**17, 512, 4), (6174, 0, 2), (2**16, 2048, 2), (2**14, 0, 2)):
        resp = np.exp(2j * np.pi * rng.uniform(size=(1, n_fft))).astype(np.complex64)
        x = (rng.standard_normal((4 * n_fft, S)) + 1j * rng.standard_normal((4 * n_fft, S))).astype(np.complex64)
        vs, vc = n_fft // 8, n_fft - n_fft // 4
        in_off = np.arange(4, dtype=np.int64) * vc
        in_off = in_off[in_off + n_fft <= x.shape[0]]
        nb = len(in_off)
        jobs.append(dict(n_fft=n_fft, n_chan=n_chan, S=S, resp=resp, x_dev=hip.DeviceArray.from_host(x), nb=nb,
                         in_off=in_off, out_off=np.arange(nb, dtype=np.int64) * vc,
                         vs=np.full(nb, vs, np.int32), vc=np.full(nb, vc, np.int32),
                         out=hip.DeviceArray((nb * vc, S), np.complex64).fill_bytes(0)))
    p64, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)

    def run(job, plan, stream, reps, results, key, errors):
        try:
            for _ in range(reps):
                out = job['out'] if key != 'shared-b' else job['out_b']
                args = (job['x_dev'].ptr, out.ptr, job['nb'], job['in_off'].ctypes.data_as(p64),
                        job['out_off'].ctypes.data_as(p64), job['vs'].ctypes.data_as(p32),
                        job['vc'].ctypes.data_as(p32))
                if job['n_chan']:
                    n_spec = (job['nb'] * int(job['vc'][0])) // job['n_chan']
                    rc = lib.bbt_osm_execute_channelized(plan, *args, job['n_chan'], 0, n_spec, stream)
                else:
                    rc = lib.bbt_osm_execute(plan, *args, stream)
                if rc:
                    raise RuntimeError(lib.bbt_last_error().decode())
                if lib.bbt_stream_sync(stream):
                    raise RuntimeError(lib.bbt_last_error().decode())
            results[key] = out.to_host().copy()
        except Exception as exc:                       # surfaces in the main thread
            errors.append((key, repr(exc)))

    def make_plan(job):
        plan = C.c_void_p()
        rc = lib.bbt_osm_plan_create(C.byref(plan), job['n_fft'], job['S'], 1, job['resp'].ctypes.data, 0, None)
        assert rc == 0, lib.bbt_last_error()
        return plan

    # single-threaded truth (fresh plans, default stream)
    truth, errors = {}, []
    for k, job in enumerate(jobs):
        plan = make_plan(job)
        run(job, plan, None, 1, truth, k, errors)
        lib.bbt_osm_plan_destroy(plan)
        job['out'].fill_bytes(0)
    assert not errors, errors
    hip.synchronize()
    # threads: plan creation inside the thread too
    results = {}

    def worker(k, job):
        stream = C.c_void_p()
        assert lib.bbt_stream_create(C.byref(stream)) == 0
        plan = make_plan(job)
        run(job, plan, stream, 8, results, k, errors)
        lib.bbt_osm_plan_destroy(plan)
        lib.bbt_stream_destroy(stream)

    threads = [threading.Thread(target=worker, args=(k, job)) for k, job in enumerate(jobs)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(len(jobs)):
        assert np.array_equal(results[k], truth[k]), k
    # two threads, one plan, two streams
    job = jobs[1]
    job['out_b'] = hip.DeviceArray(job['out'].shape, np.complex64).fill_bytes(0)
    job['out'].fill_bytes(0)
    hip.synchronize()
    plan = make_plan(job)
    streams = [C.c_void_p(), C.c_void_p()]
    for st in streams:
        assert lib.bbt_stream_create(C.byref(st)) == 0
    shared = {}
    threads = [threading.Thread(target=run, args=(job, plan, streams[i], 8, shared, key, errors))
               for i, key in enumerate(('shared-a', 'shared-b'))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert np.array_equal(shared['shared-a'], truth[1]) and np.array_equal(shared['shared-b'], truth[1])
    lib.bbt_osm_plan_destroy(plan)
    for st in streams:
        lib.bbt_stream_destroy(st)


def test_random_sizes_of_the_row_kernels_through_the_c_abi():
    """bbt_chan_execute, bbt_pfb_execute, bbt_fir_execute, bbt_shift_execute,
    bbt_unpack and bbt_detect_integrate with ragged counts (0, 1, one more or fewer than a tile) and stream counts
    the pipelines above do not reach, against float64 numpy; guard cells behind
    every output must stay untouched."""
    from baseband_tasks_amd import hip
    rng = np.random.default_rng(1234 + int(os.environ.get('BBT_TEST_SEED', '0')))
    counts = [0, 1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 127, 255, 257, 1000]
    GUARD = 64

    def cplx(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)

    def guarded(shape, dtype):
        n = int(np.prod(shape))
        buf = hip.DeviceArray((n + GUARD,), dtype)
        buf.copy_from_host(np.full(n + GUARD, 7.5, dtype))
        return buf, n

    def check_guarded(buf, n, shape, want, what, tol=1.):
        host = buf.to_host()
        assert np.all(host[n:] == 7.5), 'wrote past the end: ' + what
        if n:
            got, want = host[:n].reshape(shape), want.astype(host.dtype)
            if host.dtype.kind == 'c' and tol != 1.:
                # (a handful of outputs, each a float32 sum of many random terms: the rel-L2 of so few
                # samples scatters around the usual bound)
                assert rel_l2(got, want) <= tol * REL_L2_TOL and max_over_rms(got, want) <= tol * MAX_TOL, what
            elif host.dtype.kind == 'c':
                assert_parity(got, want, what)
            else:
                assert np.abs(got - want).max() <= 1e-5 * tol * np.abs(want).max(), what

    for case in range(10):
        S = int(rng.choice([2, 4, 6, 10, 34]))
        # channelizer, both directions
        n_chan = int(rng.choice([2, 4, 8, 16, 64, 256, 1024, 4096, 8192, 6, 100, 1029]))
        n_spec = int(rng.choice(counts if n_chan * S <= 2**14 else counts[:11]))
        x = cplx(max(n_spec, 1) * n_chan, S)
        x_dev = hip.DeviceArray.from_host(x)
        for direction in (-1, 1):
            out, n = guarded((n_spec, n_chan, S), np.complex64)
            hip.ChanPlan(n_chan, S, direction).execute(x_dev, out, n_spec)
            blocks = x[:n_spec * n_chan].reshape(n_spec, n_chan, S).astype(np.complex128)
            want = np.fft.fft(blocks, axis=1) if direction < 0 else np.fft.ifft(blocks, axis=1)
            check_guarded(out, n, (n_spec, n_chan, S), want, f'chan case {case}: n {n_chan} S {S} count {n_spec} dir {direction}')
        # two real streams as one complex stream, half spectra straight from the transform (direction -2)
        n_chan = int(rng.choice([256, 512, 1024, 2048, 4096]))
        n_spec = int(rng.choice(counts[:11]))
        for pairs in (1, int(rng.choice([2, 4, 6]))):            # complex streams = pairs of real ones
            xr = rng.standard_normal((max(n_spec, 1) * n_chan, 2 * pairs)).astype(np.float32)
            out, n = guarded((n_spec, n_chan // 2 + 1, 2 * pairs), np.complex64)
            hip.ChanPlan(n_chan, pairs, -2).execute(hip.DeviceArray.from_host(xr.view(np.complex64)), out, n_spec)
            want = np.fft.rfft(xr[:n_spec * n_chan].astype(np.float64).reshape(n_spec, n_chan, 2 * pairs), axis=1)
            check_guarded(out, n, (n_spec, n_chan // 2 + 1, 2 * pairs), want,
                          f'real pair case {case}: n {n_chan} count {n_spec} pairs {pairs}')
        # ... and back (direction +2): half spectra in, the two real streams out as one complex stream
        for pairs in (1, int(rng.choice([2, 4]))):
            half = (rng.standard_normal((max(n_spec, 1), n_chan // 2 + 1, 2 * pairs))
                    + 1j * rng.standard_normal((max(n_spec, 1), n_chan // 2 + 1, 2 * pairs))).astype(np.complex64)
            out, n = guarded((n_spec * n_chan, pairs), np.complex64)
            hip.ChanPlan(n_chan, pairs, +2).execute(hip.DeviceArray.from_host(half), out, n_spec)
            back = np.fft.irfft(half[:n_spec].astype(np.complex128), n=n_chan, axis=1)      # (n_spec, n_chan, 2 pairs) real
            z = (back[..., 0::2] + 1j * back[..., 1::2]).reshape(n_spec * n_chan, pairs)
            check_guarded(out, n, (n_spec * n_chan, pairs), z, f'real pair inverse case {case}: n {n_chan} count {n_spec} pairs {pairs}')
        # ... and the same for the filter bank's sliding-window kernels (n_stream -1)
        n_chan = int(rng.choice([256, 512, 1024, 2048]))
        n_tap = int(rng.choice([4, 8, 12, 16]))
        n_spec = int(rng.choice(counts[:11]))
        taps = rng.standard_normal((n_tap, n_chan)).astype(np.float32)
        for pairs in (1, int(rng.choice([2, 4]))):
            xr = rng.standard_normal(((max(n_spec, 1) + n_tap - 1) * n_chan, 2 * pairs)).astype(np.float32)
            out, n = guarded((n_spec, n_chan // 2 + 1, 2 * pairs), np.complex64)
            hip.PfbPlan(taps, -pairs).execute(hip.DeviceArray.from_host(xr.view(np.complex64)), out, n_spec)
            blocks = xr.reshape(-1, n_chan, 2 * pairs).astype(np.float64)
            acc = sum(blocks[t:t + n_spec] * taps[t].astype(np.float64)[:, None] for t in range(n_tap))
            check_guarded(out, n, (n_spec, n_chan // 2 + 1, 2 * pairs), np.fft.rfft(acc, axis=1) if n_spec else acc,
                          f'real pair pfb case {case}: n {n_chan} taps {n_tap} count {n_spec} pairs {pairs}')
        # polyphase filter bank
        n_chan = int(rng.choice([256, 512, 1024, 2048, 4096]))
        n_tap = int(rng.integers(1, 17))
        n_spec = int(rng.choice(counts[:12]))
        taps = rng.standard_normal((n_tap, n_chan)).astype(np.float32)
        x = cplx((max(n_spec, 1) + n_tap - 1) * n_chan, S)
        out, n = guarded((n_spec, n_chan, S), np.complex64)
        hip.PfbPlan(taps, S).execute(hip.DeviceArray.from_host(x), out, n_spec)
        xr = x.reshape(-1, n_chan, S).astype(np.complex128)
        acc = sum(xr[t:t + n_spec] * taps[t].astype(np.float64)[:, None] for t in range(n_tap))
        check_guarded(out, n, (n_spec, n_chan, S), np.fft.fft(acc, axis=1) if n_spec else acc,
                      f'pfb case {case}: n {n_chan} taps {n_tap} S {S} count {n_spec}')
        # direct FIR, real and complex responses
        n_tap = int(rng.choice([1, 2, 3, 17, 64, 129, 200]))
        n_out = int(rng.choice(counts + [4095, 4097, 20000]))
        for Sf in (S, 1):                                           # (one stream: its two halves side by side)
            resp = cplx(n_tap, Sf) if case % 2 else rng.standard_normal((n_tap, Sf)).astype(np.complex64)
            x = cplx(max(n_out, 1) + n_tap - 1, Sf)
            out, n = guarded((n_out, Sf), np.complex64)
            hip.FirPlan(resp).execute(hip.DeviceArray.from_host(x), out, n_out)
            want = np.stack([np.convolve(x[:, k].astype(np.complex128), resp[:, k].astype(np.complex128), mode='valid')
                             for k in range(Sf)], axis=1)[:n_out]
            check_guarded(out, n, (n_out, Sf), want, f'fir case {case}: taps {n_tap} S {Sf} count {n_out}',
                          tol=2. if n_out * Sf < 64 else 1.)
        # per-element sample shifts: 4- and 8-byte elements, neighbours moving together or not
        n_elem = int(rng.choice([1, 2, 3, 4, 6, 16, 128, 130, 600]))
        n_out = int(rng.choice(counts + [5000]))
        group = int(rng.choice([1, 2, 4]))
        offsets = np.repeat(rng.integers(0, 50, size=-(-n_elem // group)), group)[:n_elem].astype(np.int32)
        for dtype in (np.float32, np.complex64):
            src = rng.standard_normal((max(n_out, 1) + 50, n_elem)).astype(dtype)
            if dtype is np.complex64:
                src = src + 1j * rng.standard_normal(src.shape).astype(np.float32)
            out, n = guarded((n_out, n_elem), dtype)
            hip.ShiftPlan(offsets, np.dtype(dtype).itemsize).execute(hip.DeviceArray.from_host(src), out, n_out)
            want = np.stack([src[offsets[e]:offsets[e] + n_out, e] for e in range(n_elem)], axis=1)
            host = out.to_host()
            assert np.all(host[n:] == 7.5), f'shift case {case} wrote past the end'
            assert np.array_equal(host[:n].reshape(n_out, n_elem), want), \
                f'shift case {case}: elem {n_elem} group {group} count {n_out} {dtype}'
        # sampler frames: bits x components x threads, against a bit-level numpy decoder
        bits = int(rng.choice([1, 2, 4, 8, 16]))
        code = int(rng.choice([0, 1])) if bits in (8, 16) else 0
        E = int(rng.choice([1, 2, 3, 4, 8, 12, 16]))
        n_thread = int(rng.choice([1, 2, 3]))
        spf = int(rng.choice([1, 7, 32, 100, 640])) * (32 // np.gcd(32, E * bits))      # whole 32-bit words per frame
        header = int(rng.choice([0, 16, 32]))
        n_sets = int(rng.choice([0, 1, 2, 5, 33]))
        payload_words = spf * E * bits // 32
        frames = rng.integers(0, 2**32, size=(n_sets * n_thread, header // 4 + payload_words + int(rng.integers(0, 3))),
                              dtype=np.uint64).astype(np.uint32)
        frame_bytes = frames.shape[1] * 4
        raw_dev = hip.DeviceArray.from_host(frames.reshape(-1) if frames.size else np.zeros(1, np.uint32))
        out, n = guarded((n_sets * spf, n_thread, E), np.float32)
        hip.check(hip.lib().bbt_unpack(raw_dev.ptr, out.ptr, n_sets * n_thread, frame_bytes, header, bits, spf,
                                       n_thread, E, code, hip.get_stream()))
        host = out.to_host()
        assert np.all(host[n:] == 7.5), f'unpack case {case} wrote past the end'
        if n:
            words = frames[:, header // 4:header // 4 + payload_words].astype(np.uint64)
            shifts = np.arange(0, 32, bits, dtype=np.uint64)
            v = ((words[:, :, None] >> shifts) & np.uint64((1 << bits) - 1)).reshape(n_sets, n_thread, spf, E)
            v = v.astype(np.int64)
            if code == 1:
                lv = np.where(v >= (1 << (bits - 1)), v - (1 << bits), v).astype(np.float32)
            elif bits == 1:
                lv = np.where(v > 0, 1., -1.).astype(np.float32)
            elif bits == 2:
                lv = np.array([-3.3359, -1., 1., 3.3359], np.float32)[v]
            elif bits == 4:
                lv = ((v.astype(np.float32) - np.float32(8.)) / np.float32(2.95)).astype(np.float32)
            elif bits == 8:
                lv = ((v.astype(np.float32) - np.float32(127.5)) / np.float32(35.5)).astype(np.float32)
            else:
                lv = (v - (1 << (bits - 1))).astype(np.float32)
            want = lv.transpose(0, 2, 1, 3).reshape(n_sets * spf, n_thread, E)
            got = host[:n].reshape(want.shape)
            assert np.allclose(got, want, rtol=3e-7, atol=0), \
                f'unpack case {case}: bits {bits} code {code} E {E} threads {n_thread} spf {spf} sets {n_sets}'
        # pitched device copies (odd stream counts are padded to even with these)
        unit = int(rng.choice([1, 4, 8, 16]))
        width = unit * int(rng.choice([1, 2, 3, 5, 64, 300]))
        rows = int(rng.choice(counts[1:] + [4099]))
        spitch = width + unit * int(rng.integers(0, 4))
        dpitch = width + unit * int(rng.integers(0, 4))
        src = rng.integers(0, 256, size=rows * spitch + 16, dtype=np.uint8)
        src_dev = hip.DeviceArray.from_host(src)
        dst_dev = hip.DeviceArray((rows * dpitch + GUARD,), np.uint8)
        dst_dev.copy_from_host(np.full(rows * dpitch + GUARD, 99, np.uint8))
        skew = unit * int(rng.integers(0, 2))                       # a source that starts off the 16-byte grid
        hip.copy_2d(dst_dev, dpitch, src_dev, spitch, skew, width, rows)
        got = dst_dev.to_host()
        want = np.full(rows * dpitch + GUARD, 99, np.uint8)
        for r in range(rows):
            want[r * dpitch:r * dpitch + width] = src[skew + r * spitch:skew + r * spitch + width]
        assert np.array_equal(got, want), f'copy_2d case {case}: unit {unit} width {width} rows {rows} {spitch} {dpitch}'
        # detection + integration
        step = int(rng.choice([1, 2, 3, 7, 16, 100]))
        n_out = int(rng.choice(counts[:12]))
        n_elem = int(rng.choice([2, 4, 6, 34, 1024, 2050]))
        z = cplx(max(n_out, 1) * step, n_elem)
        z_dev = hip.DeviceArray.from_host(z)
        zz = z[:n_out * step].reshape(n_out, step, n_elem).astype(np.complex128)
        for mode, average in ((0, True), (1, False), (2, True)):
            if mode == 0:
                want, shape, src = (np.abs(zz) ** 2).sum(axis=1), (n_out, n_elem), z_dev
            elif mode == 1:
                xx, yy = zz[..., 0::2], zz[..., 1::2]
                cross = xx * yy.conj()
                want = np.stack([np.abs(xx) ** 2, np.abs(yy) ** 2, cross.real, cross.imag], axis=-1).sum(axis=1)
                shape, src = (n_out, n_elem // 2, 4), z_dev
            else:
                f = z.view(np.float32)                                  # (.., 2 n_elem) float32 elements
                want = f[:n_out * step].reshape(n_out, step, 2 * n_elem).astype(np.float64).sum(axis=1)
                shape, src = (n_out, 2 * n_elem), z_dev
            if average:
                want = want / step
            out, n = guarded(shape, np.float32)
            hip.detect_integrate(src, out, n_out, step, 2 * n_elem if mode == 2 else n_elem, mode, average)
            check_guarded(out, n, shape, want, f'detect case {case}: mode {mode} step {step} elem {n_elem} count {n_out}',
                          tol=10.)


@pytest.mark.parametrize('n_chan', [256, 512, 1024, 2048, 4096])
def test_one_stream_through_the_channelizer_unpadded(n_chan):
    """A single complex stream (and two float32 streams, which are one complex
    stream) is transformed as it is -- two consecutive spectra side by side in
    the registers -- for odd and even numbers of spectra, both directions."""
    from baseband_tasks_amd import hip
    rng = np.random.default_rng(n_chan)
    for n_spec in (1, 2, 7, 64, 129):
        x = (rng.standard_normal(n_spec * n_chan) + 1j * rng.standard_normal(n_spec * n_chan)).astype(np.complex64)
        ds = bt.DeviceStream(x, T0, 1 * u.MHz)
        ch = bt.Channelize(ds, n_chan, samples_per_frame=n_spec)
        assert ch._n_stream_even == 1                         # no padding
        z = ch.read()
        want = np.fft.fft(x.astype(np.complex128).reshape(n_spec, n_chan), axis=1)
        assert_parity(z, want.astype(np.complex64), f'one stream, {n_spec} spectra of {n_chan}')
        back = bt.Dechannelize(ch).read()
        assert_parity(back, x, f'round trip, {n_spec} spectra of {n_chan}')
        xr = rng.standard_normal((n_spec * n_chan, 2)).astype(np.float32)
        zr = bt.Channelize(bt.DeviceStream(xr, T0, 1 * u.MHz), n_chan, samples_per_frame=n_spec).read()
        want = np.fft.rfft(xr.astype(np.float64).reshape(n_spec, n_chan, 2), axis=1)
        assert_parity(zr, want.astype(np.complex64), f'two real streams, {n_spec} spectra of {n_chan}')
    # the C ABI says so too, and refuses one stream where the kernels want pairs
    assert hip.ChanPlan(n_chan, 1, -1) is not None
    with pytest.raises(RuntimeError):
        hip.ChanPlan(128, 1, -1)


@pytest.mark.parametrize('n_fft', [1024, 4096, 2**14, 2**16, 2**18, 2**21])
def test_one_stream_through_overlap_save_unpadded(n_fft):
    """One complex stream (and two float32 streams with a Hermitian response,
    which are one complex stream) through every block-length regime: the
    library pairs consecutive blocks instead of streams, for odd and even
    numbers of blocks and a ragged last block, and matches the padded route
    bit for bit."""
    rng = np.random.default_rng(n_fft)
    n_tap = 33
    spf = n_fft - n_tap + 1
    resp = (rng.standard_normal(n_tap) + 1j * rng.standard_normal(n_tap)).astype(np.complex64)
    limit_r, limit_c = bt.Convolve.FIR_MAX_TAPS, bt.Convolve.FIR_MAX_TAPS_COMPLEX
    bt.Convolve.FIR_MAX_TAPS = bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0
    try:
        for n_blocks, extra in ((1, 0), (2, 0), (3, 77), (6, 5)):
            n_in = n_blocks * spf + n_tap - 1 + extra
            x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
            ds = bt.DeviceStream(x, T0, 1 * u.MHz)
            cv = bt.Convolve(ds, resp, samples_per_frame=spf)
            assert cv._ih_samples_per_frame == n_fft
            got = cv.read()
            assert cv._single and cv._get_plan().n_stream == 1
            want = np.convolve(x.astype(np.complex128), resp.astype(np.complex128), mode='valid')
            assert_parity(got, want[:got.shape[0]].astype(np.complex64), f'one stream, n_fft {n_fft}, {n_blocks} blocks')
            padded = bt.Convolve(ds, resp, samples_per_frame=spf)
            padded.SINGLE_STREAM_UNPADDED = False
            assert np.array_equal(padded.read(), got) and not padded._single
            if n_blocks > 1:
                cv.seek(spf - 3)                              # a read across a block seam
                assert np.array_equal(cv.read(7), got[spf - 3:spf + 4])
        # two float32 streams, real response
        xr = rng.standard_normal((3 * spf + n_tap - 1 + 11, 2)).astype(np.float32)
        rr = rng.standard_normal(n_tap).astype(np.float32)
        cv = bt.Convolve(bt.DeviceStream(xr, T0, 1 * u.MHz), rr, samples_per_frame=spf)
        got = cv.read()
        assert cv._single and got.dtype == np.float32
        want = np.stack([np.convolve(xr[:, k].astype(np.float64), rr.astype(np.float64), mode='valid')
                         for k in range(2)], axis=1)[:got.shape[0]]
        assert np.abs(got - want).max() <= 1e-5 * np.sqrt(np.mean(want ** 2)) * 3
    finally:
        bt.Convolve.FIR_MAX_TAPS, bt.Convolve.FIR_MAX_TAPS_COMPLEX = limit_r, limit_c


@pytest.mark.parametrize('n_tap,n_chan', [(4, 256), (8, 512), (12, 1024), (16, 2048), (12, 4096), (5, 1024)])
def test_one_stream_through_the_filter_bank(n_tap, n_chan):
    """One complex stream / two float32 streams through PolyphaseFilterBank: unpadded
    on the sliding-window kernels (two groups of spectra side by side), padded
    for the other (taps, channels); both against the oracle."""
    rng = np.random.default_rng(n_tap * n_chan)
    resp = orc.sinc_hamming(n_tap, n_chan)
    window = n_chan <= 2048 and n_tap in (4, 8, 12, 16)
    for n_frames in (3, 4):
        ih_spf = n_chan * (n_tap + 9)
        n_in = ih_spf * (n_frames + 4)
        x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
        pfb = bt.PolyphaseFilterBank(bt.DeviceStream(x, T0, 1 * u.MHz, samples_per_frame=ih_spf), resp)
        assert pfb._n_stream_even == (1 if window else 2)
        want, _ = orc.polyphase_filter_bank(x, resp, ih_spf)
        assert_parity(pfb.read(), want.astype(np.complex64), f'one stream {n_tap} x {n_chan}')
        xr = rng.standard_normal((n_in, 2)).astype(np.float32)
        pfb = bt.PolyphaseFilterBank(bt.DeviceStream(xr, T0, 1 * u.MHz, samples_per_frame=ih_spf), resp)
        want, _ = orc.polyphase_filter_bank(xr, resp, ih_spf)
        assert_parity(pfb.read(), want.astype(np.complex64), f'two real streams {n_tap} x {n_chan}')


def test_streams_with_more_than_2_31_elements():
    """Index arithmetic beyond 32 bits (tools/large_index_check.py: a 17 GB stream through Channelize,
    Dedisperse, the fused pair and Power+Integrate, highest indices compared with numpy).  In its own
    process: the stream is made with torch, which has to initialise the GPU before this library does."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, os.path.join(root, 'tools', 'large_index_check.py')], capture_output=True,
                          text=True, timeout=900)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert 'large index check ok' in done.stdout


def test_this_library_and_torch_share_one_hip_runtime_in_either_import_order():
    """PyTorch bundles its own ROCm runtime; two runtimes in one process leave the
    second without a GPU ("No HIP GPUs are available" when this library came
    first).  hip.lib() therefore loads torch's copy first when torch is installed:
    both orders work, and only one libamdhip64 is mapped.

    Timing (round 4, `tools/import_order.py` on the MI355X box): ``import torch`` takes 0.7 s
    before the HIP runtime is initialised and 3-11 s after it -- a runtime that is already up
    digests the fat binaries of libtorch_hip.so (gigabytes of device code) as they register
    instead of on first use, i.e. it reads them all.  On a box whose page cache is cold that read
    is what took more than 300 s once in round 3 (the child was killed inside ``import torch``;
    no lock is involved).  Hence: torch-first runs first (it pages torch in the cheap way), the
    child dumps its stacks after 240 s should it ever sit anywhere that long, and the limit is
    back at 300 s per order."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = '''
import faulthandler, sys, time
faulthandler.dump_traceback_later(240, exit=False)
sys.path.insert(0, %r)
order = sys.argv[1]
t0 = time.time()
if order == "torch-first":
    import torch
    t = torch.ones(4, device="cuda")
import baseband_tasks_amd as bt
a = bt.hip.DeviceArray.from_host(__import__("numpy").arange(4, dtype="float32"))
t1 = time.time()
if order == "lib-first":
    import torch
    print("import torch after the runtime was up: %%.1f s" %% (time.time() - t1), file=sys.stderr)
    t = torch.ones(4, device="cuda")
assert float(t.sum()) == 4. and a.to_host().sum() == 6.
maps = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l})
assert len(maps) == 1, maps
print("one runtime:", maps[0])
''' % root
    for order in ('torch-first', 'lib-first'):
        done = subprocess.run([sys.executable, '-c', script, order], capture_output=True, text=True, timeout=300)
        assert done.returncode == 0 and 'one runtime:' in done.stdout, (order, done.stdout[-500:], done.stderr[-1500:])


@pytest.mark.parametrize('n_fft,n_chan', [(2**15, 256), (2**15, 2048), (2**16, 4096), (2**18, 1024), (2**20, 512),
                                          (2**21, 256)])
def test_one_stream_through_the_fused_channelizer(n_fft, n_chan):
    """Channelize(Convolve(one complex stream)): fused, blocks paired, each block with
    its own circular shift; odd and even numbers of blocks, seam spectra included;
    equal to the unfused route and to numpy."""
    import baseband_tasks_amd.channelize as chz
    rng = np.random.default_rng(n_fft + n_chan)
    n_tap = 45
    spf = n_fft - n_tap + 1
    resp = (rng.standard_normal(n_tap) + 1j * rng.standard_normal(n_tap)).astype(np.complex64)
    limit = bt.Convolve.FIR_MAX_TAPS_COMPLEX
    bt.Convolve.FIR_MAX_TAPS_COMPLEX = 0
    try:
        for n_blocks, extra in ((2, 0), (3, 901), (5, 17)):
            n_in = n_blocks * spf + n_tap - 1 + extra
            x = (rng.standard_normal(n_in) + 1j * rng.standard_normal(n_in)).astype(np.complex64)
            ds = bt.DeviceStream(x, T0, 1 * u.MHz)
            cv = bt.Convolve(ds, resp, samples_per_frame=spf)
            ch = bt.Channelize(cv, n_chan, samples_per_frame=2)
            assert ch._fusable_input() is cv and cv._single
            got = ch.read()
            y = np.convolve(x.astype(np.complex128), resp.astype(np.complex128), mode='valid')
            want = np.fft.fft(y[:got.shape[0] * n_chan].reshape(-1, n_chan), axis=1)
            assert got.shape[0] >= (y.shape[0] // n_chan) - 1
            assert_parity(got, want.astype(np.complex64), f'one stream fused, n_fft {n_fft} n_chan {n_chan} {n_blocks} blocks')
            saved = chz.FUSE_WITH_OVERLAP_SAVE
            chz.FUSE_WITH_OVERLAP_SAVE = False
            try:
                plain = bt.Channelize(bt.Convolve(ds, resp, samples_per_frame=spf), n_chan, samples_per_frame=2).read()
            finally:
                chz.FUSE_WITH_OVERLAP_SAVE = saved
            assert rel_l2(got, plain) < 5e-7
    finally:
        bt.Convolve.FIR_MAX_TAPS_COMPLEX = limit


@pytest.mark.parametrize('shape', [(2,), (4,)])
def test_real_streams_through_the_fused_channelizer(shape):
    """Channelize(Dedisperse(float32 streams)): pairs of real streams are complex
    streams to the fused plan, their spectra are separated afterwards; equal to
    the oracle's rfft of the dedispersed real streams and to the unfused route."""
    import baseband_tasks_amd.channelize as chz
    rng = np.random.default_rng(sum(shape))
    fs, n_chan = 4e6, 512
    n_in = 5 * 2**16 + 1234
    x = rng.standard_normal((n_in,) + shape).astype(np.float32)
    ds = bt.DeviceStream(x, T0, fs, samples_per_frame=2**14, frequency=400 * u.MHz, sideband=1)
    probe = bt.Dedisperse(ds, 3.)
    dd = bt.Dedisperse(ds, 3., samples_per_frame=2**16 - (probe._pad_start + probe._pad_end))
    dd._get_plan()
    assert dd._ih_samples_per_frame == 2**16 and dd._real and dd._paired
    ch = bt.Channelize(dd, n_chan, samples_per_frame=4)
    assert ch._fusable_input() is dd
    got = ch.read()
    y = dd.read()                                                    # the dedispersed real streams (GPU, unfused)
    want = np.fft.rfft(y[:got.shape[0] * n_chan].astype(np.float64).reshape((-1, n_chan) + shape), axis=1)
    assert got.shape == want.shape
    assert_parity(got, want.astype(np.complex64), f'real streams fused {shape}')
    saved = chz.FUSE_WITH_OVERLAP_SAVE
    chz.FUSE_WITH_OVERLAP_SAVE = False
    try:
        plain = bt.Channelize(bt.Dedisperse(ds, 3., samples_per_frame=dd.samples_per_frame), n_chan,
                              samples_per_frame=4).read()
    finally:
        chz.FUSE_WITH_OVERLAP_SAVE = saved
    assert rel_l2(got, plain) < 5e-7


def test_bench_two_ranks_share_this_gpu():
    """`python bench.py --gpus 2` end to end on one GPU: the launcher starts two
    ranks (gloo, as RCCL wants one device per rank), the chirp is broadcast, each
    rank runs and verifies its own blocks against the oracle, outputs are
    gathered, rank 0 prints one JSON line."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BBT_BENCH_BACKEND='gloo')
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '2',
                        '--warmup', '1', '--blocks', '24', '--full', '--no-cpu'], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak' and d['value'] > 0
    assert d['verified']['ok'] and d['verified']['all_ranks_ok']
    assert d['with_gather'] and 'error' not in d['with_gather'], d['with_gather']
    assert d['with_gather']['gathered_shape'][0] == 2 * (24 * 836100 // 1024 // 512) * 512
    assert 'broadcast' in d['config']['sharding']
    # both collectives made to fail on both ranks: each evaluates the chirp itself, the gathered
    # figure is reported missing -- and the sharded value stands, verified on every rank
    env['BBT_BENCH_INJECT'] = 'bcast,gather'
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '2',
                        '--warmup', '1', '--blocks', '24', '--full', '--no-cpu'], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][0])
    assert d['n_gpus'] == 2 and d['value'] > 0 and d['verified']['ok'] and d['verified']['all_ranks_ok']
    assert 'injected gather failure' in d['with_gather']['error']
    assert 'the broadcast failed' in d['config']['sharding']


def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """A plain `python bench.py` run times exactly --steps steps, leaves what only --full measures
    null, and --dump-outputs writes a seeded sample of the last timed step's spectra: float32
    (row, channel, pol, re/im) with float64 row numbers; the first spectrum matches the oracle on the
    benchmark's own seeded input (regenerated with torch in a child process: torch stays out of this
    one, whose HIP runtime the library already holds)."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3',
                        '--warmup', '1', '--blocks', '24', '--dump-outputs', str(out)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['warmup'] == 1 and d['ms_per_step'] > 0 and d['value'] > 0
    assert d['unit'] == 'Msamples/s' and d['higher_is_better'] is True and d['dtype'] == 'c64'
    assert all(d[k] is None for k in ('roofline', 'verified', 'cpu_baseline', 'host_path', 'with_gather'))
    spectra = np.load(out / 'spectra.npy')
    index = np.load(out / 'spectra_index.npy')
    n_spec = (24 * 836100 // 1024 // 512) * 512
    assert spectra.dtype == np.float32 and index.dtype == np.float64
    assert spectra.shape == (len(index), 1024, 2, 2) and spectra.nbytes + index.nbytes <= 64 << 20
    assert index[0] == 0 and index[-1] == n_spec - 1 and np.all(np.diff(index) > 0)
    assert np.all(np.isfinite(spectra)) and np.any(spectra != 0)
    # the benchmark's input: torch.randn of (n_in, 2 pol, re/im) from a cuda:0 generator seeded 12345
    script = '''
import sys
import numpy as np
import torch
sys.path.insert(0, %r)
from oracle import bbt_oracle as orc
n_fft = 2**20
gen = torch.Generator(device="cuda:0")
gen.manual_seed(12345)
x = torch.randn((23 * 836100 + n_fft, 2, 2), generator=gen, device="cuda:0", dtype=torch.float32)
xin = torch.view_as_complex(x[:n_fft]).cpu().numpy()
g = orc.disperse_geometry(16e6, 1000., 1, -100.)
h = orc.chirp(n_fft, 16e6, 1000., 1, -100., g["reference_frequency"])
y = orc.disperse_block(xin, h, g["pad_start"], n_fft - g["pad_start"] - g["pad_end"])
np.save(sys.argv[1], np.fft.fft(y[:1024].astype(np.complex128), axis=0))
''' % root
    want_file = tmp_path / 'want.npy'
    done = subprocess.run([sys.executable, '-c', script, str(want_file)], env=env, capture_output=True, text=True,
                          timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert rel_l2(spectra[0, ..., 0] + 1j * spectra[0, ..., 1], np.load(want_file)) < 1e-6


def test_default_arguments_at_full_scale_golden(golden):
    """Default-argument tasks on full-size streams against the REAL reference's
    output (tests/golden/make_golden.py): Dedisperse(DM 100) at 800 MHz picks
    1 666 980-sample blocks (1260 x 1323 on the generic path), Resample 1 049 760."""
    nh = noise(4 * 2**20, (2,), 2**20, frequency=800 * u.MHz, sideband=1)
    ds = bt.DeviceStream(nh, T0, 16 * u.MHz)
    dd = bt.Dedisperse(ds, 100.)
    assert [dd._pad_start, dd._pad_end, dd._ih_samples_per_frame, dd.samples_per_frame, dd.shape[0],
            dd._sample_offset] == list(golden['d8_geo'])
    y = dd.read()
    spf = dd.samples_per_frame
    assert_parity(y[:1024], golden['d8_head'], 'head')
    assert_parity(y[spf - 512:spf + 512], golden['d8_seam1'], 'seam')
    assert_parity(y[-1024:], golden['d8_tail'], 'tail')
    nh = noise(3 * 2**20, (2,), 2**20, frequency=1000 * u.MHz, sideband=1)
    ds = bt.DeviceStream(nh, T0, 16 * u.MHz)
    limit = bt.Convolve.FIR_MAX_TAPS
    for taps_limit in (limit, 0):                   # the direct filter, and the 1 049 760-sample block transform
        bt.Convolve.FIR_MAX_TAPS = taps_limit
        try:
            rs = bt.Resample(ds, 0.25, pad=64)
            assert [rs._pad_start, rs._pad_end, rs._ih_samples_per_frame, rs.samples_per_frame,
                    rs.shape[0]] == list(golden['r5_geo'][:5])
            rs.seek(0)
            r = rs.read()
        finally:
            bt.Convolve.FIR_MAX_TAPS = limit
        spf = rs.samples_per_frame
        assert_parity(r[:1024], golden['r5_head'], 'head')
        assert_parity(r[spf - 512:spf + 512], golden['r5_seam1'], 'seam')
        assert_parity(r[-1024:], golden['r5_tail'], 'tail')


def test_plain_c_program_on_the_abi():
    """tests/cabi_example.c: a C (gcc) host program on include/bbt_hip.h -- an
    overlap-save delay filter over two blocks and a channelizer -- runs on the GPU."""
    import subprocess
    from test_cabi import build_c_example
    r = subprocess.run([build_c_example()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'C ABI example OK' in r.stdout and 'expected error' in r.stdout


@pytest.mark.parametrize('n_fft', [1000, 2187, 3125, 2401 * 3, 6174, 12000])
def test_real_streams_on_block_lengths_that_are_not_powers_of_two(n_fft):
    """float32 streams (the reference's rfft / irfft engine paths,
    fourier/numpy.py:41-49) with even and ODD block lengths, paired and
    unpaired streams, through the generic transform."""
    assert HipFFTMaker.next_fast_len(n_fft) == n_fft
    rng = np.random.default_rng(n_fft)
    n_tap = 37
    limit = bt.Convolve.FIR_MAX_TAPS
    bt.Convolve.FIR_MAX_TAPS = 0
    try:
        for shape, per_stream in (((2,), False), ((3,), True), ((4,), True)):
            resp = rng.standard_normal((n_tap,) + (shape if per_stream else (1,))).astype(np.float32)
            n_in = 2 * n_fft + 321
            x = rng.standard_normal((n_in,) + shape).astype(np.float32)
            src = bt.StreamGenerator(lambda fh: x[fh.tell():fh.tell() + fh.samples_per_frame], x.shape, T0, 1e6,
                                     samples_per_frame=n_in, dtype=np.float32)
            cv = bt.Convolve(src, resp, samples_per_frame=n_fft - n_tap + 1)
            assert cv._ih_samples_per_frame == n_fft and cv.dtype == np.float32
            got = cv.read()
            # truth: the exact linear convolution (which is what Convolve keeps, block independent)
            full = np.broadcast_to(resp, (n_tap,) + shape).astype(np.float64)
            want = np.stack([np.convolve(x[:, i].astype(np.float64), full[:, i], mode='valid')
                             for i in range(shape[0])], axis=1)
            assert got.dtype == np.float32 and got.shape == want.shape
            err = np.linalg.norm((got - want).ravel()) / np.linalg.norm(want.ravel())
            assert err < REL_L2_TOL and np.abs(got - want).max() < MAX_TOL * np.sqrt(np.mean(want ** 2)), \
                (n_fft, shape, err)
    finally:
        bt.Convolve.FIR_MAX_TAPS = limit
