"""`SpectralKurtosis` and `Excise` on the GPU against their NumPy twin (`rfi.spectral_kurtosis`,
`rfi.excise_samples`), bit for bit: the sums are float64 in a fixed two-level order, so a value has
one correct result whatever the tiling.  The shared cases of sk_cases.py (test_sk_host.py proves
that each flags some blocks, keeps some and has no estimator on a limit's doorstep), reads in
pieces, chunks and small runs, exact small-integer data, NaN / Inf / all-zero blocks, and device
consumers."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, rfi
from baseband_tasks_amd.device_task import produces_on_device

import sk_cases
from sk_cases import CASES, IDS, same_bits

pytestmark = pytest.mark.gpu

T0 = bt.Time('2010-11-12T13:14:15')
RATE = 1e4


def _group(case):
    return int(np.prod(case.sample_shape[len(case.sample_shape) - case.join:], dtype=int))


def _noise(n, sample_shape, dtype, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n,) + sample_shape) + 1j * rng.standard_normal((n,) + sample_shape)
    if np.dtype(dtype).kind == 'c':
        return z.astype(np.complex64)
    return (z.real ** 2 + z.imag ** 2).astype(np.float32)


# -- the shared cases ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_tasks_and_entry_point_equal_the_twin(case):
    x = sk_cases.data(case)
    sk, flags, out = sk_cases.expected(case)
    sh = bt.HostStream(x, T0, RATE, samples_per_frame=case.samples, pin=False)
    kh = bt.SpectralKurtosis(sh, case.n, averaged=case.averaged)
    got_sk = kh.read()
    assert got_sk.dtype == np.float32 and same_bits(got_sk, sk)
    eh = bt.Excise(sh, case.n, case.limits, averaged=case.averaged, join=case.join)
    assert eh.limits == sk_cases.limits_of(case)
    got = eh.read()
    assert got.dtype == x.dtype and same_bits(got, out)
    # the entry point's own sk and flags
    n_block, n_elem, g = case.samples // case.n, int(np.prod(case.sample_shape, dtype=int)), _group(case)
    d_x = hip.DeviceArray.from_host(x[:n_block * case.n])
    d_out = hip.DeviceArray(d_x.shape, x.dtype)
    d_sk = hip.DeviceArray((n_block, n_elem), np.float32)
    d_flags = hip.DeviceArray((n_block, n_elem // g), np.uint8)
    hip.sk_excise(d_x, d_out, case.n, n_elem, sk_cases.limits_of(case), case.averaged, g, sk=d_sk, flags=d_flags)
    assert same_bits(d_out.to_host(), out)
    assert same_bits(d_sk.to_host().reshape(sk.shape), sk)
    np.testing.assert_array_equal(d_flags.to_host().reshape(flags.shape), flags.astype(np.uint8))
    assert same_bits(hip.sk_estimate(d_x, case.n, n_elem, case.averaged).to_host().reshape(sk.shape), sk)
    # the zero pattern is the thresholded estimator stream's, with the join applied
    zapped = rfi.excise_flags(got_sk, eh.limits, case.join)
    zapped = np.repeat(zapped, case.n, axis=0).reshape((n_block * case.n,) + zapped.shape[1:] + (1,) * case.join)
    zapped = np.broadcast_to(zapped, got.shape)
    assert not np.ascontiguousarray(got[zapped]).view(np.uint32).any()
    assert same_bits(got[~zapped], x[:n_block * case.n][~zapped])


@pytest.mark.parametrize('slab_kib', [1, 16, 65536])
@pytest.mark.parametrize('name', ['workload_layout', 'prime_width_f32', 'many_segments', 'columns_not_a_tile'])
def test_no_value_depends_on_the_tiling(name, slab_kib, monkeypatch):
    """BBT_SK_SLAB_KIB sizes the tiles for another slab (from the narrowest tile to the widest);
    the order of the sums is the contract, so every bit stays."""
    case = CASES[IDS.index(name)]
    x = sk_cases.data(case)
    sk, flags, out = sk_cases.expected(case)
    monkeypatch.setenv('BBT_SK_SLAB_KIB', str(slab_kib))
    eh = bt.Excise(bt.DeviceStream(x, T0, RATE, samples_per_frame=case.n), case.n, case.limits,
                   averaged=case.averaged, join=case.join)
    assert same_bits(eh.read(), out)


# -- framing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sample_shape, dtype, join', [((), np.float32, 0), ((3,), np.complex64, 0),
                                                       ((3,), np.float32, 1), ((5, 2), np.complex64, 1)])
def test_reads_in_pieces_with_seeks(sample_shape, dtype, join):
    # from a stream resident in HBM: a read that starts at an odd sample of an odd-width stream hands
    # the kernel an input that is not 16-byte aligned
    n, samples = 64, 64 * 37 + 11
    x = _noise(samples, sample_shape, dtype, seed=21)
    body = x[:64 * 37].reshape((37, 64) + sample_shape)
    body[::3, :4] *= 40.                                   # bursts: every third block, every element
    limits = rfi.sk_limits(n)
    want = rfi.excise_samples(x, n, limits, join=join)
    want_sk = rfi.spectral_kurtosis(x, n)
    flags = rfi.excise_flags(want_sk, limits, join)
    assert flags.any() and not flags.all()
    dh = bt.DeviceStream(x, T0, RATE, samples_per_frame=100)
    # blocks are counted from sample 0 of the stream given: a slice that starts at an odd sample
    for first in (1, 65):
        part = bt.Excise(dh[first:], n, join=join)
        assert same_bits(part.read(), rfi.excise_samples(x[first:], n, limits, join=join))
        assert same_bits(bt.SpectralKurtosis(dh[first:], n).read(), rfi.spectral_kurtosis(x[first:], n))
    eh = bt.Excise(dh, n, join=join, samples_per_frame=128)
    assert eh.shape[0] == 64 * 37
    for start, count in [(127, 3), (129, 1000), (63, 66), (5, 1), (2367, 1), (641, 1025), (0, 2368)]:
        eh.seek(start)
        assert same_bits(eh.read(count), want[start:start + count])
        assert eh.tell() == start + count
    eh.seek(191)
    assert same_bits(eh.read_device(3).to_host(), want[191:194])
    eh.max_frames_per_call = 2                             # (a long read assembled from several runs of frames)
    eh.seek(1)
    assert same_bits(eh.read_device(2366).to_host(), want[1:2367])
    eh.seek(0)
    assert same_bits(eh.read(), want)
    kh = bt.SpectralKurtosis(dh, n, samples_per_frame=4)
    for start, count in [(3, 2), (5, 30), (36, 1), (0, 37)]:
        kh.seek(start)
        assert same_bits(kh.read(count), want_sk[start:start + count])
    kh.max_frames_per_call = 2
    kh.seek(1)
    assert same_bits(kh.read_device(35).to_host(), want_sk[1:36])


@pytest.mark.parametrize('sample_shape, dtype', [((5, 2), np.complex64), ((3,), np.float32)])
def test_small_budget_takes_several_chunks(sample_shape, dtype, monkeypatch):
    n, n_block = 100, 41
    x = _noise(n * n_block + 3, sample_shape, dtype, seed=23)
    x[:n * n_block].reshape((n_block, n) + sample_shape)[::4, :5] *= 30.
    limits = rfi.sk_limits(n)
    sh = bt.HostStream(x, T0, RATE, samples_per_frame=x.shape[0], pin=False)
    eh = bt.Excise(sh, n, samples_per_frame=n * n_block)
    eh.excise_budget = 7 * n * x[0].nbytes + 5
    calls = []
    real = hip.sk_excise
    monkeypatch.setattr(hip, 'sk_excise', lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    assert same_bits(eh.read(), rfi.excise_samples(x, n, limits))
    assert len(calls) == 6 and sum(calls) == n * n_block and max(calls) == 7 * n
    kh = bt.SpectralKurtosis(sh, n, samples_per_frame=n_block)
    kh.sk_budget = 7 * n * x[0].nbytes + 5
    calls = []
    real_estimate = hip.sk_estimate
    monkeypatch.setattr(hip, 'sk_estimate', lambda *a, **k: (calls.append(a[0].shape[0]), real_estimate(*a, **k))[1])
    assert same_bits(kh.read(), rfi.spectral_kurtosis(x, n))
    assert len(calls) == 6 and max(calls) == 7 * n


# -- sums that are exact in any order -----------------------------------------------------------------------
@pytest.mark.parametrize('sample_shape, n', [((), 16), ((6,), 100), ((1024, 2), 256), ((3,), 4096)])
def test_small_integer_data_is_exact(sample_shape, n):
    """re, im in [-7, 7]: p <= 98, S2 <= 65536 * 98^2 < 2^53, so every sum is exact whatever the
    order and only the estimator's last steps round."""
    rng = np.random.default_rng(25)
    samples = 5 * n
    x = (rng.integers(-7, 8, (samples,) + sample_shape)
         + 1j * rng.integers(-7, 8, (samples,) + sample_shape)).astype(np.complex64)
    x[n:2 * n] = 3 + 4j                                    # a carrier in every element: sk = 0
    p = (x.real.astype(np.float64) ** 2 + x.imag.astype(np.float64) ** 2).reshape((5, n) + sample_shape)
    m = float(n)
    with np.errstate(all='ignore'):
        exact = (((m + 1.) / (m - 1.)) * (m * ((p * p).sum(1) / p.sum(1) ** 2) - 1.)).astype(np.float32)
    want_sk = rfi.spectral_kurtosis(x, n)
    assert same_bits(want_sk, exact) and not want_sk[1].any()
    dh = bt.DeviceStream(x, T0, RATE, samples_per_frame=n)
    assert same_bits(bt.SpectralKurtosis(dh, n).read(), exact)
    limits = (0.2, 3.0)                                    # (uniform integers are not Gaussian: their own band)
    flags = rfi.excise_flags(exact, limits)
    assert flags[1].all() and not flags.all()
    assert same_bits(bt.Excise(dh, n, limits).read(), rfi.excise_samples(x, n, limits))


# -- NaN, Inf and nothing ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.complex64, np.float32])
@pytest.mark.parametrize('sample_shape, join', [((4, 2), 1), ((3,), 0), ((300,), 0)])
def test_nan_inf_and_all_zero_blocks_are_flagged(dtype, sample_shape, join):
    n, n_block = 64, 9
    x = _noise(n * n_block, sample_shape, dtype, seed=27)
    body = x.reshape((n_block, n) + sample_shape)
    first = (0,) * len(sample_shape)
    last = tuple(d - 1 for d in sample_shape)
    body[(1, 17) + first] = np.nan
    body[(3, 63) + last] = np.inf
    body[(5, slice(None)) + first] = 0.
    body[(7, 0) + last] = -np.inf if dtype is np.float32 else complex(0., -np.inf)
    limits = (0.05, 20.)                                   # (wide: noise is never flagged, only what is not finite)
    sk = rfi.spectral_kurtosis(x, n)
    flags = rfi.excise_flags(sk, limits)
    want_flags = np.zeros(flags.shape, bool)
    for b, e in ((1, first), (3, last), (5, first), (7, last)):
        want_flags[(b,) + e] = True
        assert np.isnan(sk[(b,) + e])
    np.testing.assert_array_equal(flags, want_flags)
    want = rfi.excise_samples(x, n, limits, join=join)
    dh = bt.DeviceStream(x, T0, RATE, samples_per_frame=n)
    got = bt.Excise(dh, n, limits, join=join).read()
    assert same_bits(got, want)
    assert np.all(np.isfinite(got))
    for b in (1, 3, 5, 7):
        e = first if b in (1, 5) else last
        zero = got[(slice(b * n, (b + 1) * n),) + e]
        assert not np.ascontiguousarray(zero).view(np.uint32).any()
    # the neighbours are untouched
    for b in (0, 2, 4, 6, 8):
        assert same_bits(got[b * n:(b + 1) * n], x[b * n:(b + 1) * n])
    got_sk = bt.SpectralKurtosis(dh, n).read()
    assert same_bits(got_sk, sk)


# -- device consumers --------------------------------------------------------------------------------------------
def test_device_consumers_take_the_frames_in_hbm(monkeypatch):
    n_chan, n, n_spec = 64, 64, 64 * 6
    rng = np.random.default_rng(29)
    v = (rng.standard_normal((n_chan * n_spec, 2)) + 1j * rng.standard_normal((n_chan * n_spec, 2))).astype(np.complex64)
    t = np.arange(n_chan * n_spec // 3)
    v[:len(t), 0] += (8. * np.exp(2j * np.pi * (5. / n_chan) * t)).astype(np.complex64)     # a carrier in channel 5, X
    meta = dict(frequency=300e6, sideband=1, polarization=np.array(['X', 'Y']))
    sh = bt.DeviceStream(v, T0, 1e6, samples_per_frame=n_chan * 16, **meta)
    ch = bt.Channelize(sh, n_chan, 16)
    spectra = ch.read()
    eh = bt.Excise(bt.Channelize(sh, n_chan, 16), n, join=1)
    assert produces_on_device(eh) and eh.shape == spectra.shape and eh.samples_per_frame == n
    want = rfi.excise_samples(spectra, n, eh.limits, join=1)
    flags = rfi.excise_flags(rfi.spectral_kurtosis(spectra, n), eh.limits, join=1)
    assert flags[:2, 5].all() and not flags[2:].all() and flags.mean() < 0.2
    assert same_bits(eh.read(), want)
    twin = bt.DeviceStream(want, ch.start_time, ch.sample_rate, samples_per_frame=n, frequency=ch.frequency,
                           sideband=ch.sideband, polarization=ch.polarization)
    monkeypatch.setattr(eh, 'read', lambda *a, **k: pytest.fail('the excised stream was downloaded'))
    eh.seek(0)
    got = bt.Power(eh).read()
    ref = bt.Power(twin).read()
    assert got.shape == ref.shape == (n_spec, n_chan, 4)
    assert same_bits(got, ref)
    # a time stream: Dedisperse on top of the excised voltages
    x = sk_cases.data(CASES[1])                            # (2,) complex64, 2050 samples
    limits = rfi.sk_limits(100)
    tmeta = dict(frequency=1400e6, sideband=1)
    th = bt.Excise(bt.DeviceStream(x, T0, 1e6, samples_per_frame=500, **tmeta), 100, join=1)
    twin = bt.DeviceStream(rfi.excise_samples(x, 100, limits, join=1), T0, 1e6, samples_per_frame=500, **tmeta)
    monkeypatch.setattr(th, 'read', lambda *a, **k: pytest.fail('the excised stream was downloaded'))
    got = bt.Dedisperse(th, 0.3).read()
    ref = bt.Dedisperse(twin, 0.3).read()
    assert got.shape == ref.shape and got.shape[0] > 0
    assert same_bits(got, ref)
