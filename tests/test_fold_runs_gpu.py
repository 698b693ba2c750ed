"""bbt_fold_runs (csrc/fold_kernels.hpp) on wide rows, several column tiles and split slots,
against the NumPy fold of tests/fold_cases.py.  The cases hold integers small enough that every
float32 partial sum is exact (test_fold_runs_host.py proves it, and that the cases reach every
kernel shape of the launcher), so the comparison is bit for bit; then the same widths through
`Fold`, `PulseStack` and ``Integrate(phase=...)``."""
import os

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip

import fold_cases as fc

pytestmark = pytest.mark.gpu

GUARD = 64
T0 = bt.Time('2010-11-12T13:14:15')
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def upload_input(x, aligned):
    """The samples in HBM, on the 16-byte grid or 8 bytes off it (a flat array 8 bytes longer,
    sliced)."""
    if aligned:
        dev = hip.DeviceArray.from_host(x)
    else:
        extra = 8 // x.dtype.itemsize
        flat = hip.DeviceArray((x.size + extra,), x.dtype)
        dev = flat[extra:]
        dev.copy_from_host(x.ravel())
        dev = dev.reshape(x.shape)
    assert dev.ptr % 16 == (0 if aligned else 8)
    return dev


def guarded_output(n_slot, width, prev):
    """An output of (n_slot, width) float32 with GUARD floats of 7.5 behind it, holding ``prev``
    (or 7.5 everywhere, which a call that does not accumulate must overwrite)."""
    n = n_slot * width
    host = np.full(n + GUARD, 7.5, np.float32)
    if prev is not None:
        host[:n] = prev.ravel()
    buf = hip.DeviceArray.from_host(host)
    return buf, buf[:n].reshape(n_slot, width)


def check_exact(buf, want, what):
    host = buf.to_host()
    n = want.size
    assert np.all(host[n:] == 7.5), 'wrote past the end: ' + what
    got = host[:n].reshape(want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)


def run_both_routes(case, x, table, prev, scale, want, routes=('host', 'device')):
    d = fc.dispatch_of(case)
    x_dev = upload_input(x, case.aligned)
    slot_ptr, begin, end = table
    for route in routes:
        buf, rows = guarded_output(case.n_slot, want.shape[1], prev)
        if route == 'host':
            hip.fold_runs(x_dev, rows, case.n_elem, case.mode, slot_ptr, begin, end, scale=scale,
                          accumulate=case.accumulate)
        else:
            on_device = [hip.DeviceArray.from_host(np.ascontiguousarray(a, np.int64)) for a in table]
            hip.fold_runs_device(x_dev, rows, case.n_elem, case.mode, *on_device, scale=scale,
                                 accumulate=case.accumulate)
        check_exact(buf, want, f'{case.name}, {route} table, {d}')


@pytest.mark.parametrize('case', fc.CASES, ids=lambda case: case.name)
def test_sums_are_exact(case):
    table = fc.make_table(case)
    x, prev, scale = fc.make_input(case), fc.make_prev(case), fc.make_scale(case, table)
    total, mass = fc.fold_reference(x, case.mode, *table, prev, None)
    assert mass.max() < fc.EXACT
    run_both_routes(case, x, table, prev, scale, fc.expected_float32(total, scale))


CLIPPED = [
    # narrow, one share and split; two tiles of columns, one share and split
    fc.new_case('clip_narrow', 0, 6, 1000, 8, accumulate=True, scale='scale', empty=(3,)),
    fc.new_case('clip_narrow_split', 0, 6, 32768, 2, scale='scale', n_runs=30),
    fc.new_case('clip_two_tiles', 1, 600, 1024, 20, scale='scale', empty=(0, 19), n_runs=100),
    fc.new_case('clip_two_tiles_split', 1, 600, 1024, 2, accumulate=True, n_runs=30),
]


@pytest.mark.parametrize('case', CLIPPED, ids=lambda case: case.name)
def test_runs_outside_the_input_are_clipped(case):
    d = fc.dispatch_of(case)
    assert (d['split'] > 1) == case.name.endswith('split') and d['tiles'] == (2 if 'tiles' in case.name else 1)
    n_in = case.n_in
    slot_ptr, begin, end = (a.copy() for a in fc.make_table(case))
    # runs that stick out at either end, by a little and by more than 32 bits hold
    first, last = np.argmin(begin), np.argmax(end)
    begin[first], end[last] = -7, n_in + 1000
    mid = len(begin) // 2
    begin[mid], end[mid - 1] = -(1 << 40), 1 << 40
    # behind the runs of the last slot: runs wholly outside the input, and reversed ones
    begin = np.concatenate((begin, [n_in + 10, -50, n_in, 100, n_in + 5, 1 << 40]))
    end = np.concatenate((end, [n_in + 50, -10, n_in + 1, 40, -5, (1 << 40) + 9]))
    slot_ptr[-1] += 6
    assert begin.min() < 0 and end.max() > n_in and np.any(end < begin)
    table = (slot_ptr, begin, end)
    x, prev, scale = fc.make_input(case), fc.make_prev(case), fc.make_scale(case, table)
    total, mass = fc.fold_reference(x, case.mode, *table, prev, None)
    assert mass.max() < fc.EXACT
    run_both_routes(case, x, table, prev, scale, fc.expected_float32(total, scale), routes=('device',))


@pytest.mark.parametrize('mode, n_elem', [(1, 600), (2, 2048)])
def test_float_sums_stay_accurate_when_split_and_tiled(mode, n_elem):
    """Random float32 data, 2 slots of 8192 samples: split and (with 300 and 512 units) two tiles
    of columns.  The bound is the one of test_fold_gpu.py::test_long_bins_accuracy.
    Measured on MI355X: rel-L2 1.1e-7 (mode 1, 300 units) and 2.0e-7 (mode 2, 512 units), 64 shares each."""
    case = fc.new_case(f'float_mode{mode}', mode, n_elem, 8192, 2, n_runs=40)
    d = fc.dispatch_of(case)
    assert d['split'] > 1 and d['tiles'] == 2 and d['n_unit'] == (300 if mode == 1 else 512)
    rng = np.random.default_rng(mode)
    x = rng.standard_normal((case.n_in, n_elem * (1 if mode == 2 else 2))).astype(np.float32)
    if mode != 2:
        x = x.view(np.complex64)
    table = fc.make_table(case)
    ref, _ = fc.fold_reference(x, mode, *table)
    buf, rows = guarded_output(2, ref.shape[1], None)
    hip.fold_runs(upload_input(x, True), rows, n_elem, mode, *table)
    host = buf.to_host()
    assert np.all(host[ref.size:] == 7.5)
    err = np.linalg.norm(host[:ref.size].reshape(ref.shape) - ref) / np.linalg.norm(ref)
    print(f'mode {mode}, {d}: rel-L2 {err:.3e}')
    assert err < 1e-5, err


# -- the same widths through the tasks -----------------------------------------------------------
RATE = 1e5


def linear_phase(period):
    """A phase that includes the cycle count, one turn per ``period`` samples."""
    def ph(t):
        return 0.37 + (RATE / period) * (t - T0)
    return ph


def whole(rng, n, shape, dtype):
    if np.dtype(dtype).kind == 'c':
        parts = rng.integers(-4, 5, size=(n,) + shape + (2,)).astype(np.float32)
        return parts.view(np.complex64)[..., 0]
    return rng.integers(-4, 5, size=(n,) + shape).astype(np.float32)


def square_of(x):
    x = x.astype(np.complex128)
    return x.real ** 2 + x.imag ** 2                 # (exact for integers, which abs(x) ** 2 is not)


def power_of(x):
    X, Y = x[..., 0].astype(np.complex128), x[..., 1].astype(np.complex128)
    xy = X * Y.conj()
    return np.stack([square_of(X), square_of(Y), xy.real, xy.imag], axis=-1)


def wide_stream(kind):
    """(task to fold, what it yields in float64 / complex128, bytes per sample fetched)."""
    rng = np.random.default_rng(len(kind))
    if kind == 'power':                     # mode 1, 1024 pairs per sample: 4 tiles
        x = whole(rng, 4096, (1024, 2), np.complex64)
        ds = bt.DeviceStream(x, T0, RATE, polarization=np.array(['X', 'Y']))
        return bt.Power(ds), power_of(x), x[0].nbytes
    if kind == 'square':                    # mode 0, an odd row: one element per lane, 2 tiles
        x = whole(rng, 8192, (301,), np.complex64)
        return bt.Square(bt.DeviceStream(x, T0, RATE)), square_of(x), x[0].nbytes
    if kind == 'float':                     # mode 2, four floats per lane, 2 tiles
        x = whole(rng, 4096, (2, 1024), np.float32)
        return bt.DeviceStream(x, T0, RATE), x.astype(np.float64), x[0].nbytes
    x = whole(rng, 8192, (300,), np.complex64)     # complex, summed as it is
    return bt.DeviceStream(x, T0, RATE), x.astype(np.complex128), x[0].nbytes


def as_floats(a, n_lead):
    a = np.ascontiguousarray(a)
    return a.view(np.float32).reshape(a.shape[:n_lead] + (-1,))


def mean_of(sums, counts):
    """float32(sum) * float32(1 / count) per float, NaN where the count is 0: what `_run_fold` asks
    of the kernels for an average.  ``sums`` exact, in the task's dtype; one count per leading index."""
    with np.errstate(divide='ignore', invalid='ignore'):
        scale = np.where(counts > 0, 1. / np.maximum(counts, 1), np.nan).astype(np.float32)
        return as_floats(sums, counts.ndim) * scale[..., None]


@pytest.mark.parametrize('kind', ['power', 'square', 'float', 'complex'])
def test_wide_streams_through_the_tasks(kind):
    src, xx, sample_bytes = wide_stream(kind)
    dtype = np.complex64 if kind == 'complex' else np.float32
    n_phase, step = 16, 1024
    for period in (150, 1500):             # several runs per bin; bins without samples
        ph = linear_phase(period)
        fh = bt.Fold(src, n_phase, ph, step, average=False)
        fr = fh.read()
        edges = fh._get_offsets(np.arange(fh.shape[0] + 1))
        ref, cnt = fc.numpy_fold(xx, edges, n_phase, ph, RATE, T0)
        assert len(edges) - 1 == xx.shape[0] // step and (cnt.min() == 0) == (period == 1500)
        sums = ref.astype(dtype)
        assert np.array_equal(sums, ref)
        lead = cnt.reshape(cnt.shape + (1,) * (ref.ndim - 2))
        np.testing.assert_array_equal(fr['count'], np.broadcast_to(lead, ref.shape))
        np.testing.assert_array_equal(fr['data'], sums)
        avg = bt.Fold(src, n_phase, ph, step).read()
        np.testing.assert_array_equal(as_floats(avg, 2), mean_of(sums, cnt))
        assert np.isnan(avg).any() == (period == 1500)
        # at least five chunks, their edges inside runs: the same sums
        small = bt.Fold(src, n_phase, ph, step, average=False)
        small.fold_budget = 701 * sample_bytes
        assert xx.shape[0] // 701 >= 5
        chunked = small.read()
        np.testing.assert_array_equal(chunked['count'], fr['count'])
        np.testing.assert_array_equal(chunked['data'], fr['data'])
        small = bt.Fold(src, n_phase, ph, step)
        small.fold_budget = 701 * sample_bytes
        np.testing.assert_array_equal(as_floats(small.read(), 2), as_floats(avg, 2))


def test_wide_streams_through_the_tasks_pulse_stack_and_integrate():
    src, xx, _ = wide_stream('power')
    ph = linear_phase(150)
    n_phase = 16
    ps = bt.PulseStack(src, n_phase, ph)
    edges = ps._phased.edges[:ps.shape[0] * n_phase + 1]
    cnt = np.diff(edges)
    assert ps.shape[0] >= 20 and cnt.min() >= 1
    sums = np.array([xx[a:b].sum(0) for a, b in zip(edges[:-1], edges[1:])]).astype(np.float32)
    got = ps.read()
    np.testing.assert_array_equal(as_floats(got, 2), mean_of(sums, cnt).reshape(ps.shape[0], n_phase, -1))
    ih = bt.Integrate(src, 2.5, ph, average=False)
    edges = ih.edges
    fr = ih.read()
    sums = np.array([xx[a:b].sum(0) for a, b in zip(edges[:-1], edges[1:])]).astype(np.float32)
    assert len(sums) >= 8
    np.testing.assert_array_equal(fr['count'][:, 0, 0], np.diff(edges))
    np.testing.assert_array_equal(fr['data'], sums)


def test_wide_streams_through_the_tasks_polyco_on_both_table_routes():
    pp = bt.phases.PolycoPhase(os.path.join(GOLDEN_DIR, 'B1937_polyco.dat'))
    t0, rate, n_phase = bt.Time('2018-05-06T22:20:00'), 123250., 64
    x = whole(np.random.default_rng(1937), 4096, (600,), np.complex64)
    xx = square_of(x)
    src = bt.Square(bt.DeviceStream(x, t0, rate))
    reads = {}
    for route in ('device', 'host'):
        fh = bt.Fold(src, n_phase, pp, 1024, average=False)
        fh.table_route = route
        assert fh._route() == route
        reads[route] = fh.read()
    edges = fh._get_offsets(np.arange(fh.shape[0] + 1))
    ref, cnt = fc.numpy_fold(xx, edges, n_phase, pp, rate, t0)
    for route, fr in reads.items():
        np.testing.assert_array_equal(fr['count'][..., 0], cnt, err_msg=route)
        np.testing.assert_array_equal(fr['data'], ref.astype(np.float32), err_msg=route)
    np.testing.assert_array_equal(reads['device']['data'].view(np.uint32), reads['host']['data'].view(np.uint32))
