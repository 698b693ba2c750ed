"""`hip.CorrPlan.execute` between guard bands (tests/guard_bands.py): input and output each inside one
allocation between two bands of poison, 16-byte aligned and 8 bytes off (complex64 asks for no more),
under NaN and +inf poison, on integer data whose result is exact -- whole, and segment by segment with
every piece in a guarded array of exactly its samples.  The shapes leave ragged tiles (3 inputs: 5
elements of 6 reals in a tile of 32 rows, 7 elements in two groups; 17 and 33 inputs: 34 and 66 reals in 2
and 3 chunks) and an odd last segment of one sample, so a load beyond the group's reals or the segment
puts poison into a product, and a store past the scratch's cells or the output shows in the bands or in
the comparison.  A planted NaN or +inf must spoil exactly the baselines of its input, element and block:
zero-fed lanes and elements that share a tile do not leak (inf * 0)."""
import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip

import corr_cases
from corr_cases import BY_NAME, same_bits, set_tiling
from guard_bands import POISONS, Guarded, check_all

pytestmark = pytest.mark.gpu

C64 = np.dtype(np.complex64)
both_skews = pytest.mark.parametrize('skew', (0, 8), ids=['aligned16', 'off8'])
both_poisons = pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))
guarded_cases = pytest.mark.parametrize('name', corr_cases.GUARDED)


def _setup(name):
    case = BY_NAME[name]
    a, e, n = corr_cases.n_inputs(case), corr_cases.n_elem(case), case.n
    x = np.ascontiguousarray(corr_cases.integer_data(name)[:n * case.blocks])
    return case, a, e, n, x


def _count(x, poison):
    return int(np.count_nonzero(np.ascontiguousarray(x).reshape(-1).view(np.uint32) == poison))


def _plain(plan, x, blocks, e):
    out = hip.DeviceArray((blocks, e, plan.n_baselines), C64)
    plan.execute(hip.DeviceArray.from_host(x), 0, x.shape[0], out, 0, blocks)
    return out.to_host()


@both_poisons
@both_skews
@guarded_cases
def test_guard_bands_whole(name, skew, poison, monkeypatch):
    set_tiling(monkeypatch)
    case, a, e, n, x = _setup(name)
    plan = hip.CorrPlan(a, e, n, 1, average=False)
    want = corr_cases.integer_expected(name, False)
    assert same_bits(_plain(plan, x, case.blocks, e), want)
    gx, go = Guarded.load(x, poison, skew), Guarded(want.shape, C64, poison, skew)
    plan.execute(gx.array, 0, x.shape[0], go.array, 0, case.blocks)
    got_x, got = check_all([gx, go], f'corr whole {name}')
    assert same_bits(got, want) and same_bits(got_x, x)
    plan.close()


@both_poisons
@both_skews
@guarded_cases
def test_guard_bands_segment_by_segment(name, skew, poison, monkeypatch):
    """Every piece is one segment in a guarded array of exactly its samples: the last of a block is the
    one odd sample, beyond which nothing lies; the block goes on in the plan's float64 carry."""
    set_tiling(monkeypatch)
    case, a, e, n, x = _setup(name)
    plan = hip.CorrPlan(a, e, n, 1, average=False)
    want = corr_cases.integer_expected(name, False)
    go = Guarded(want.shape, C64, poison, skew)
    for blk in range(case.blocks):
        for p0 in range(blk * n, (blk + 1) * n, corr_cases.SEG):
            p1 = min((blk + 1) * n, p0 + corr_cases.SEG)
            gx = Guarded.load(x[p0:p1], poison, skew)
            plan.execute(gx.array, p0, p1 - p0, go.array, 0, case.blocks)
            assert same_bits(gx.check(f'corr piece [{p0}, {p1}) {name}'), x[p0:p1])
    assert p1 - p0 == 1
    assert same_bits(go.check(f'corr pieces {name}'), want)
    plan.close()


@pytest.mark.parametrize('what', ['nan', 'inf'])
@both_poisons
@guarded_cases
def test_a_planted_value_spoils_its_baselines_only(name, poison, what, monkeypatch):
    set_tiling(monkeypatch)
    case, a, e, n, x = _setup(name)
    plan = hip.CorrPlan(a, e, n, 1, average=False)
    base = corr_cases.integer_expected(name, False)
    blk, e0, i0 = case.blocks - 1, 1, a - 2
    y = x.copy()
    y[blk * n + corr_cases.SEG, e0, i0] = complex(np.nan, np.nan) if what == 'nan' else complex(np.inf, 0.)
    gy = Guarded.load(y, poison, 8, planted=_count(y, poison))
    go = Guarded(base.shape, C64, poison, 8)
    plan.execute(gy.array, 0, y.shape[0], go.array, 0, case.blocks)
    _, got = check_all([gy, go], f'corr planted {what} {name}')
    pairs = bt.baseline_pairs(a)
    spoiled = np.zeros(base.shape, bool)
    spoiled[blk, e0, (pairs[:, 0] == i0) | (pairs[:, 1] == i0)] = True
    assert spoiled.sum() == a
    # (a planted +inf gives inf or, against a zero or an opposite inf, NaN: not finite either way)
    bad = np.isnan(got) if what == 'nan' else ~np.isfinite(got)
    assert np.array_equal(bad, spoiled)
    assert same_bits(got[~spoiled], base[~spoiled])
    plan.close()
