"""Host side of `Modulate` (no GPU): construction checks, the per-sample bins and the
time-ordered run tables against `fold_table`, the NumPy twin against a plain loop, and the
argument checks of hip.modulate_runs and of the two C entry points."""
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip
from baseband_tasks_amd.fold_table import polynomial_bins, sample_times, unwrapped_bin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLYCO = os.path.join(ROOT, 'tests', 'golden', 'B1937_polyco.dat')
T0 = bt.Time('2010-11-12T13:14:15')
RATE = 1e4


def _phase(kind, per_bin, n_phase, n):
    """The phases of tests/test_fold_host.py."""
    f = 1. / (per_bin * n_phase)          # cycles per sample
    if kind == 'linear':
        return lambda t: 0.123 + f * (t - T0) * RATE
    if kind == 'spindown':
        return lambda t: 0.123 + f * (t - T0) * RATE - 0.2 * f * ((t - T0) * RATE) ** 2 / n
    return lambda t: (0.123 + f * (t - T0) * RATE
                      + 0.4 * f * n / (2 * np.pi * 3) * np.sin(2 * np.pi * 3 * (t - T0) * RATE / n))


def _stream(n=4000, sample_shape=(2,), dtype=np.float32, spf=200, **kwargs):
    return bt.HostStream(np.zeros((n,) + sample_shape, dtype), T0, RATE, samples_per_frame=spf, pin=False,
                         **kwargs)


def _expand(run_begin, run_bin, n):
    return np.repeat(run_bin, np.diff(np.concatenate((run_begin, [n]))))


# -- construction -------------------------------------------------------------------------
def test_profile_and_dtype_checks():
    ph = _phase('linear', 2.5, 8, 4000)
    sh = _stream()
    with pytest.raises(TypeError):
        bt.Modulate(sh, np.ones(8, np.complex64), ph)
    with pytest.raises(ValueError):
        bt.Modulate(sh, np.ones((8, 3)), ph)                      # (3,) against samples of (2,)
    with pytest.raises(ValueError):
        bt.Modulate(sh, np.ones((8, 2, 2)), ph)                   # more axes than a sample has
    with pytest.raises(ValueError):
        bt.Modulate(sh, np.ones(0), ph)
    with pytest.raises(ValueError):
        bt.Modulate(sh, np.float32(2.), ph)
    with pytest.raises(TypeError, match='float32/complex64'):
        bt.Modulate(_stream(dtype=np.int16), np.ones(8), ph)
    for profile in (np.ones(8), np.ones((8, 1)), np.ones((8, 2)), np.arange(8)):
        mh = bt.Modulate(sh, profile, ph)
        assert mh.profile.dtype == np.float32 and mh.n_phase == 8
    mh = bt.Modulate(_stream(sample_shape=(5, 3, 2)), np.ones((8, 5, 1, 2)), ph)
    assert mh._gain_host.shape == (8, 30)
    g = np.arange(16.).reshape(8, 2)
    mh = bt.Modulate(_stream(sample_shape=(5, 3, 2)), g, ph)           # (trailing axes align, as in NumPy)
    np.testing.assert_array_equal(mh._gain_host.reshape(8, 5, 3, 2), np.broadcast_to(g[:, None, None, :], (8, 5, 3, 2)))
    assert bt.Modulate(sh, np.ones((8, 1)), ph)._gain_host.shape == (8,)


def test_shape_framing_metadata_and_repr():
    ph = _phase('linear', 2.5, 8, 4000)
    sh = _stream(dtype=np.complex64, frequency=np.array([300e6, 310e6]), sideband=np.array([1, -1]),
                 polarization=np.array(['X', 'Y']))
    mh = bt.Modulate(sh, np.arange(1., 9.), ph)
    assert mh.shape == sh.shape and mh.dtype == np.complex64 and mh.samples_per_frame == 200
    assert mh.sample_rate == sh.sample_rate and mh.start_time == sh.start_time
    assert mh.stop_time == sh.stop_time
    np.testing.assert_array_equal(mh.frequency, sh.frequency)
    np.testing.assert_array_equal(mh.sideband, sh.sideband)
    np.testing.assert_array_equal(mh.polarization, sh.polarization)
    assert mh._produces_on_device and mh._view_source is None
    r = repr(mh)
    assert r.startswith('Modulate(ih') and 'profile=[1. 2. 3. 4. 5. 6. 7. 8.]' in r and 'phase=' in r
    assert 'samples_per_frame' not in r.split('\nih:')[0]
    m7 = bt.Modulate(sh, np.ones((8, 2)), ph, samples_per_frame=7)
    assert m7.samples_per_frame == 7 and m7.shape == sh.shape
    assert 'samples_per_frame=7' in repr(m7)
    assert mh.seek(250) == 250 and mh.tell() == 250
    mh.close()
    assert mh.closed
    with pytest.raises(ValueError):
        mh.read(1)


def test_table_route_values(monkeypatch):
    mh = bt.Modulate(_stream(), np.ones(8), _phase('linear', 2.5, 8, 4000))
    monkeypatch.delenv('BBT_FOLD_TABLE', raising=False)
    assert mh.table_route is None and mh._route() == 'device'
    monkeypatch.setenv('BBT_FOLD_TABLE', 'host')
    assert mh._route() == 'host'
    mh.table_route = 'device'
    assert mh._route() == 'device'
    mh.table_route = 'elsewhere'
    with pytest.raises(ValueError):
        mh._route()


# -- bins and run tables ----------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['linear', 'spindown', 'sinusoidal'])
@pytest.mark.parametrize('per_bin', [1, 2.5, 700])
def test_bins_equal_per_sample_unwrapped_bin(kind, per_bin):
    n, n_phase, spf = 20000, 37, 1531
    ph = _phase(kind, per_bin, n_phase, n)
    mh = bt.Modulate(_stream(n, spf=spf), np.ones(n_phase), ph)
    first, count = 1000, 17000                       # (starts and ends inside frames, eleven edges between)
    want = np.empty(count, np.int64)
    for f in range(first // spf, (first + count - 1) // spf + 1):
        lo, hi = max(first, f * spf), min(first + count, (f + 1) * spf)
        times = sample_times(T0 + f * spf / RATE, f * spf, RATE)
        want[lo - first:hi - first] = unwrapped_bin(ph(times(np.arange(lo, hi))), n_phase) % n_phase
    assert want.min() >= 0 and want.max() < n_phase
    got = mh.bins(first, count)
    np.testing.assert_array_equal(got, want)
    # the runs handed to the kernel expand to the same bins
    run_begin, run_bin = mh._runs(first, first + count)
    assert run_begin.dtype == run_bin.dtype == np.int64
    assert run_begin[0] == 0 and np.all(np.diff(run_begin) > 0) and run_begin[-1] < count
    np.testing.assert_array_equal(_expand(run_begin, run_bin, count), want)
    if per_bin == 700:
        assert len(run_begin) < 60                    # (runs, not samples)


def test_bins_of_a_negative_and_a_two_part_phase():
    class TwoPart:
        def __init__(self, cycles):
            self.int = np.round(cycles)
            self.frac = cycles - self.int              # in [-0.5, 0.5]

    n, n_phase = 3000, 16
    lin = (lambda t: -7.31 + (t - T0) * RATE / (2.5 * n_phase))
    a = bt.Modulate(_stream(n), np.ones(n_phase), lin)
    b = bt.Modulate(_stream(n), np.ones(n_phase), lambda t: TwoPart(lin(t)))
    bins = a.bins(0, n)
    assert bins.min() == 0 and bins.max() == n_phase - 1
    times = sample_times(T0, 0, RATE)
    np.testing.assert_array_equal(bins[:200], np.floor((lin(times(np.arange(200))) % 1.) * n_phase))
    np.testing.assert_array_equal(b.bins(0, n), bins)
    np.testing.assert_array_equal(_expand(*b._runs(0, n), n), bins)


def test_polyco_bins_are_polynomial_bins_of_fold_pieces():
    pp = bt.phases.PolycoPhase(POLYCO)
    # the closest polyco entry changes at 22:57:36: sample 25000, inside the first frame
    t0, rate, n, spf, n_phase = bt.Time('2018-05-06T22:57:35.5'), 5e4, 65536, 32768, 64
    sh = bt.HostStream(np.zeros((n, 1), np.float32), t0, rate, samples_per_frame=spf, pin=False)
    mh = bt.Modulate(sh, np.ones(n_phase), pp)
    mh.table_route = 'host'
    want = np.empty(n, np.int64)
    n_piece = []
    for f in range(2):
        pieces = pp.fold_pieces(t0 + f * spf / rate, rate, 0, spf)
        n_piece.append(len(pieces))
        for (m0, m1, coeff, dt0, step, ref_int, ref_frac) in pieces:
            k = polynomial_bins(coeff, dt0, step, ref_int, ref_frac, np.arange(m0, m1), n_phase)
            want[f * spf + m0:f * spf + m1] = k % n_phase
    assert n_piece == [2, 1]
    np.testing.assert_array_equal(mh.bins(0, n), want)
    np.testing.assert_array_equal(mh.bins(20001, 30000), want[20001:50001])
    run_begin, run_bin = mh._runs(20001, 50001)
    np.testing.assert_array_equal(_expand(run_begin, run_bin, 30000), want[20001:50001])
    assert run_begin[0] == 0 and np.all(np.diff(run_begin) > 0)


# -- the NumPy twin --------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.complex64])
@pytest.mark.parametrize('profile_shape', [(5,), (5, 2), (5, 3, 1), (5, 3, 2)])
def test_modulate_samples_against_a_loop(dtype, profile_shape):
    rng = np.random.default_rng(3)
    data = rng.standard_normal((40, 3, 2)).astype(np.float32)
    if dtype is np.complex64:
        data = (data + 1j * rng.standard_normal(data.shape)).astype(np.complex64)
    profile = rng.standard_normal(profile_shape)
    bins = rng.integers(0, 5, 40)
    got = bt.modulate_samples(data, profile, bins)
    assert got.dtype == dtype and got.shape == data.shape
    full = np.broadcast_to(profile.astype(np.float32).reshape((5,) + (1,) * (3 - len(profile_shape)) + profile_shape[1:]),
                           (5, 3, 2))
    for n in range(40):
        for i in range(3):
            for j in range(2):
                g = full[bins[n], i, j]
                x = data[n, i, j]
                want = np.complex64(complex(np.float32(x.real) * g, np.float32(x.imag) * g)) if dtype is np.complex64 \
                    else np.float32(x) * g
                assert got[n, i, j] == want
    np.testing.assert_array_equal(got, data * full[bins])          # (NumPy's own product, finite data)


# -- wrapper and C entry points: refusals before any launch ------------------------------------
def _fake(shape, dtype):
    d = hip.DeviceArray.__new__(hip.DeviceArray)       # (never dereferenced: checks come first)
    d.shape, d.dtype = shape, np.dtype(dtype)
    return d


def test_modulate_runs_wrapper_checks_tables():
    x, out = _fake((10, 2), np.float32), _fake((10, 2), np.float32)
    gain, gain2 = _fake((4,), np.float32), _fake((4, 2), np.float32)
    for begin, bins in (([1, 5], [0, 1]),              # does not start at 0
                        ([0, 5, 5], [0, 1, 2]),        # not strictly increasing
                        ([0, 5, 10], [0, 1, 2]),       # a run at the end of the input
                        ([0, 5], [0, 4]),              # bin past the profile
                        ([0, 5], [-1, 0]),
                        ([0, 5], [0, 1, 2]),           # lengths differ
                        ([], [])):
        with pytest.raises(ValueError):
            hip.modulate_runs(x, out, 2, gain, begin, bins)
    with pytest.raises(ValueError):
        hip.modulate_runs(x, out, 4, gain, [0], [0])               # input width
    with pytest.raises(ValueError):
        hip.modulate_runs(x, _fake((9, 2), np.float32), 2, gain, [0], [0])
    with pytest.raises(ValueError):
        hip.modulate_runs(x, out, 2, _fake((4, 3), np.float32), [0], [0])       # gains per element
    with pytest.raises(ValueError):
        hip.modulate_runs(x, out, 2, _fake((4,), np.float64), [0], [0])
    with pytest.raises(TypeError):
        hip.modulate_runs(_fake((10, 2), np.int16), out, 2, gain2, [0], [0])
    with pytest.raises(TypeError):
        hip.modulate_runs(x, _fake((10, 2), np.complex64), 2, gain2, [0], [0])
    plan = dict(lo=np.array([0, 4, 9]), row=np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        hip.modulate_pieces(x, out, 2, gain, plan)                  # the pieces end before the input


def test_modulate_entry_points_validate_arguments():
    lib = hip.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    t = np.zeros(8, np.int64).ctypes.data
    assert lib.bbt_version() >= 161
    for args in ((None, p, 1, 1, p, 1, 0, t, t, 1, None), (p, None, 1, 1, p, 1, 0, t, t, 1, None),
                 (p, p, 1, 1, None, 1, 0, t, t, 1, None), (p, p, 1, 1, p, 1, 0, None, t, 1, None),
                 (p, p, 1, 1, p, 1, 0, t, None, 1, None)):
        assert lib.bbt_modulate_runs(*args) != 0
        assert b'bbt_modulate_runs: null' in lib.bbt_last_error()
    for args in ((p, p, 0, 1, p, 1, 0, t, t, 1, None), (p, p, 1, 0, p, 1, 0, t, t, 1, None),
                 (p, p, 1, 1, p, 0, 0, t, t, 1, None), (p, p, 1, 1, p, 1, -1, t, t, 1, None),
                 (p, p, 1, 1, p, 1, 0, t, t, 0, None), (p, p, -5, 1, p, 1, 0, t, t, 1, None),
                 (p, p, 1, 1, p, 1, 0, t, t, 2, None)):
        assert lib.bbt_modulate_runs(*args) != 0
        assert b'bad sizes' in lib.bbt_last_error()
    assert lib.bbt_modulate_runs(p, p, 4, 6, p, 1, 4, t, t, 1, None) != 0
    assert b'gain stride' in lib.bbt_last_error()
    assert lib.bbt_modulate_runs(p + 2, p, 4, 1, p, 1, 0, t, t, 1, None) != 0
    assert b'aligned' in lib.bbt_last_error()
    for args in ((None, p, 1, 1, p, 1, 0, t, 1, 1, None), (p, None, 1, 1, p, 1, 0, t, 1, 1, None),
                 (p, p, 1, 1, None, 1, 0, t, 1, 1, None), (p, p, 1, 1, p, 1, 0, None, 1, 1, None)):
        assert lib.bbt_modulate_pieces(*args) != 0
        assert b'bbt_modulate_pieces: null' in lib.bbt_last_error()
    for args in ((p, p, 0, 1, p, 1, 0, t, 1, 1, None), (p, p, 1, 0, p, 1, 0, t, 1, 1, None),
                 (p, p, 1, 1, p, 0, 0, t, 1, 1, None), (p, p, 1, 1, p, 1, 0, t, 0, 1, None),
                 (p, p, 1, 1, p, 1, 0, t, 1, 0, None), (p, p, 1, 1, p, 1, 0, t, 1, 65, None)):
        assert lib.bbt_modulate_pieces(*args) != 0
        assert b'bad sizes' in lib.bbt_last_error()
    assert lib.bbt_modulate_pieces(p, p, 1, 1, p, 1, 0, t + 4, 1, 1, None) != 0
    assert b'aligned' in lib.bbt_last_error()
