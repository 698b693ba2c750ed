"""`hip.RmedPlan`, `RunningMedian` and `Detrend` on the GPU against their NumPy twins
(`search.running_median_samples`, `search.detrend_samples`), bit for bit: a median is an exact selection
and the scrunch and the interpolation fix their order, so a value has one correct result whatever the
selection method, the tile, the chunking, the framing or the seek.  The shared cases of rmed_cases.py
(test_rmed_host.py proves the twins), both methods and every tile width, the tasks end to end, a chain
on the device, and the refusals."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip, search
from baseband_tasks_amd.device_task import produces_on_device

import dmt_cases
import rmed_cases
from rmed_cases import same_bits, set_tiling, stream

pytestmark = pytest.mark.gpu


def _execute(x, w, s, detrend):
    """One call of a plan over the whole of host ``x``."""
    n_elem = int(np.prod(x.shape[1:], dtype=int))
    rows = x.shape[0] // s
    plan = hip.RmedPlan(w, s, n_elem)
    out = hip.DeviceArray((rows * s, n_elem), np.float32)
    plan.execute(hip.DeviceArray.from_host(x), 0, x.shape[0], out, 0, rows * s, rows, detrend=detrend)
    got = out.to_host().reshape((rows * s,) + x.shape[1:])
    assert plan.info(rows, 0, rows * s)['scratch_bytes'] == (0 if s == 1 else (2 * rows * n_elem * 4))
    plan.close()
    return got


# -- the shared cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('w, s', rmed_cases.CASES, ids=rmed_cases.IDS)
def test_plan_equals_the_twins_on_noise(w, s):
    x = rmed_cases.noise()
    b, z = rmed_cases.expected('noise', w, s)
    assert same_bits(_execute(x, w, s, True), z)
    assert same_bits(_execute(x, w, s, False), b)


@pytest.mark.parametrize('w, s', rmed_cases.PLANT_CASES, ids=str)
def test_plan_equals_the_twins_on_the_planted_plane(w, s):
    x = rmed_cases.planted()
    b, z = rmed_cases.expected('planted', w, s)
    got_z, got_b = _execute(x, w, s, True), _execute(x, w, s, False)
    assert same_bits(got_z, z) and same_bits(got_b, b)
    assert np.isfinite(got_z).all() and np.isfinite(got_b).all()
    for col, at in ((rmed_cases.NAN, rmed_cases.NAN_AT), (rmed_cases.INF, rmed_cases.INF_AT),
                    (rmed_cases.MINUS_NAN, rmed_cases.MINUS_NAN_AT)):
        hit = rmed_cases.flagged_samples(x.shape[0], w, s, at)
        assert not got_z[hit, col].view(np.uint32).any() and not got_b[hit, col].view(np.uint32).any()
        assert (got_b[~hit, col] != 0).all()


@pytest.mark.parametrize('shape', [(), (1,), (3, 5)], ids=str)
def test_sample_shapes(shape):
    x = np.random.default_rng(19).normal(5., 3., (600,) + shape).astype(np.float32)
    for w, s in ((33, 1), (33, 8), (5, 100)):
        assert same_bits(_execute(x, w, s, True), search.detrend_samples(x, w, s))
        got = bt.Detrend(stream(x, bt.DeviceStream), w, s).read()
        assert got.shape == (600 // s * s,) + shape and same_bits(got, search.detrend_samples(x, w, s))


# -- both methods, every tile width ---------------------------------------------------------------------------
@pytest.mark.parametrize('select, tile, rows', rmed_cases.TILINGS)
def test_no_value_depends_on_the_method_or_the_tile(select, tile, rows, monkeypatch):
    """BBT_RMED_SELECT, BBT_RMED_TILE and BBT_RMED_ROWS reshape the work; the selection is exact, so every bit
    stays."""
    set_tiling(monkeypatch, select, tile, rows)
    x = rmed_cases.noise()
    for w, s in rmed_cases.TILING_CASES:
        info = hip.rmed_info(w, s, 67, 2100 // s, 0, 2100 // s * s)
        assert info['method'] == hip.RMED_METHODS[select] and info['tile'] == tile
        assert info['rows'] <= (rows or info['rows']) and info['lds_bytes'] <= hip.RANK_LDS_BYTES
        b, z = rmed_cases.expected('noise', w, s)
        assert same_bits(_execute(x, w, s, True), z)
        assert same_bits(_execute(x, w, s, False), b)
    x = rmed_cases.planted()
    b, z = rmed_cases.expected('planted', 9, 8)
    assert same_bits(_execute(x, 9, 8, True), z) and same_bits(_execute(x, 9, 8, False), b)


# -- the tasks: chunks, frames and seeks ----------------------------------------------------------------------
@pytest.mark.parametrize('w, s', [(33, 8), (33, 1)], ids=str)
def test_tasks_chunks_frames_and_seeks(w, s, monkeypatch):
    x = rmed_cases.noise()
    b, z = rmed_cases.expected('noise', w, s)
    n = z.shape[0]
    calls = []
    run = hip.RmedPlan.execute
    monkeypatch.setattr(hip.RmedPlan, 'execute', lambda self, x_, i0, ni, out, o0, no, rows, detrend=True:
                        (calls.append(no), run(self, x_, i0, ni, out, o0, no, rows, detrend=detrend))[1])
    row = 67 * 4
    third = -(-n // (3 * s)) * s                                       # three chunks, the last one shorter
    halo = (w + 1) * (s * row + (row if s > 1 else 0))
    budget3 = halo + third // s * (2 * s * row + (2 * row if s > 1 else 0))
    for cls in (bt.HostStream, bt.DeviceStream):
        budgets = [(1 << 29, [n]), (budget3, [third, third, n - 2 * third])]
        if cls is bt.DeviceStream:
            budgets.append((1, [s] * (n // s)))                        # (never less than a scrunch row)
        for budget, launches in budgets:
            dt = bt.Detrend(stream(x, cls), w, s)
            assert dt.samples_per_frame == n and produces_on_device(dt)
            dt.detrend_budget = budget
            del calls[:]
            assert same_bits(dt.read(), z)
            assert calls == launches
        dt.invalidate_cache()
        dt.seek(n - 150)
        assert same_bits(dt.read(), z[n - 150:])
    for spf in (s, None, 25 * s):                                      # one scrunch row a frame, the default, several
        src = stream(x, bt.DeviceStream, samples_per_frame=50)
        dt = bt.Detrend(src, w, s, samples_per_frame=spf)
        rm = bt.RunningMedian(src, w, s, samples_per_frame=spf)
        assert dt.samples_per_frame == (spf or -(-50 // s) * s) == rm.samples_per_frame
        for start, count in [(0, 100), (250, 333), (n - 101, 101), (1000, 7), (0, n)]:
            dt.seek(start)
            assert same_bits(dt.read(count), z[start:start + count])
            assert dt.tell() == start + count
            rm.seek(start)
            assert same_bits(rm.read(count), b[start:start + count])
        dt.seek(1050)                                                  # into the middle, to the end
        assert same_bits(dt.read_device().to_host(), z[1050:])
    # the stream minus its baseline is the detrended stream
    rm = bt.RunningMedian(stream(x, bt.DeviceStream), w, s).read()
    assert same_bits(rm, b) and same_bits(x[:n] - rm, z)


# -- a chain that never leaves HBM ---------------------------------------------------------------------------------
def test_single_pulse_chain_on_the_device():
    case = dmt_cases.by_name('zero_dm')                                # the smallest plane: 100 samples, one trial
    x = dmt_cases.data(case, 'noise')
    plane = bt.DMTrials(dmt_cases.stream(case, 'noise', bt.DeviceStream), case.dms)
    chain = bt.BoxcarSearch(bt.Standardize(bt.Detrend(plane, 9, scrunch=2), 25), 25, 3)
    stage = chain
    while hasattr(stage, 'ih'):
        assert produces_on_device(stage)
        stage = stage.ih
    got = chain.read_device().to_host()
    want = search.dm_trials_samples(x, dmt_cases.shifts(case))
    want = search.standardize_samples(search.detrend_samples(want, 9, 2), 25)
    want = search.boxcar_search_samples(want, 25, 3)
    assert got.shape == want.shape == (4, 3, 1) and same_bits(got, want)
    assert np.isfinite(got).all()


# -- what is refused ------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    lib = hip.lib()
    x = hip.DeviceArray.from_host(np.ones((20, 2), np.float32))
    out = hip.DeviceArray.from_host(np.full((20, 2), 5., np.float32))
    plan = hip.RmedPlan(5, 2, 2)

    def refused(rc, what):
        return rc != 0 and what in lib.bbt_last_error()
    h = plan._h
    assert refused(lib.bbt_rmed_execute(None, x.ptr, 0, 20, out.ptr, 0, 20, 10, 1, None), b'null')
    assert refused(lib.bbt_rmed_execute(h, None, 0, 20, out.ptr, 0, 20, 10, 1, None), b'null')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, None, 0, 20, 10, 1, None), b'null')
    assert refused(lib.bbt_rmed_execute(h, x.ptr + 2, 0, 20, out.ptr, 0, 20, 10, 1, None), b'aligned')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, out.ptr + 1, 0, 20, 10, 1, None), b'aligned')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, out.ptr, 0, 20, 10, 2, None), b'mode')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, out.ptr, 0, 20, 0, 1, None), b'rows')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, out.ptr, 1, 18, 10, 1, None), b'whole scrunch rows')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, out.ptr, 0, 19, 10, 1, None), b'whole scrunch rows')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, out.ptr, 0, 0, 10, 1, None), b'whole scrunch rows')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 20, out.ptr, 2, 20, 10, 1, None), b'beyond')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 18, out.ptr, 0, 20, 10, 1, None), b'does not hold')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 2, 18, out.ptr, 0, 4, 10, 1, None), b'does not hold')
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 0, 12, out.ptr, 0, 8, 10, 1, None), b'does not hold')     # rows 0 ... 6 are needed
    assert refused(lib.bbt_rmed_execute(h, x.ptr, 1, 19, out.ptr, 4, 4, 10, 1, None), b'begin at a scrunch row')
    made = hip.C.c_void_p()
    for args, what in (((4, 1, 1), b'width'), ((1, 1, 1), b'width'), ((1025, 1, 1), b'width'), ((3, 0, 1), b'scrunch'),
                       ((3, 4097, 1), b'scrunch'), ((3, 1, 0), b'elements')):
        assert refused(lib.bbt_rmed_plan_create(hip.C.byref(made), *args), what) and not made.value
    hip.synchronize()
    assert (out.to_host() == 5.).all()                                  # nothing ran
    # through the wrappers
    for args in ((4, 1, 1), (3, 0, 1), (3, 1, 0)):
        with pytest.raises(hip.HipError):
            hip.RmedPlan(*args)
    with pytest.raises(ValueError):
        plan.execute(x, 0, 21, out, 0, 20, 10)
    with pytest.raises(ValueError):
        plan.execute(x, 0, 20, out, 0, 22, 11)
    with pytest.raises(TypeError):
        plan.execute(hip.DeviceArray((20, 2), np.complex64), 0, 20, out, 0, 20, 10)
    zs = bt.DeviceStream(np.ones((16, 8, 2), np.complex64), bt.Time(rmed_cases.T0), rmed_cases.RATE)
    for cls in (bt.Detrend, bt.RunningMedian):
        with pytest.raises(TypeError, match='Square'):
            cls(zs, 3)
    # and what is not refused runs: ones detrend to +0, and are their own baseline
    plan.execute(x, 0, 20, out, 0, 20, 10)
    assert not out.to_host().view(np.uint32).any()
    plan.execute(x, 0, 14, out, 0, 8, 10, detrend=False)                # rows 0 ... 6 are all the first four need
    got = out.to_host()
    assert (got[:8] == 1.).all() and not got[8:].any()
    plan.close()
    plan.close()
