"""`hip.FfaPlan` between guard bands (tests/guard_bands.py): the block and the result each lie inside one
allocation between two bands of poison, 16-byte aligned and 4 bytes off, under the NaN and the +inf poison.  A
load beyond the block would fold poison into a profile or into the total, a store beyond the result or a
cell never written shows in the bands or against the twin.  The scratch is the plan's own and not visible to
the caller."""
import numpy as np
import pytest

from baseband_tasks_amd import hip

import ffa_cases
from guard_bands import POISONS, SKEWS, Guarded, check_all

pytestmark = pytest.mark.gpu

F32 = np.dtype(np.float32)


@pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))
@pytest.mark.parametrize('chunked', [False, True], ids=['whole', 'chunked'])
@pytest.mark.parametrize('kind', ffa_cases.KINDS)
@pytest.mark.parametrize('name', ['ragged', 'wide_bins'])
def test_ffa_plan(name, kind, chunked, poison):
    """Each block as exactly n rows: the row after the last sample is the back band.  Chunked: the first six columns
    in launches of two columns and two base periods, the others in one launch; together they must fill every cell
    of the poisoned result, and none may touch a cell of another."""
    case = ffa_cases.by_name(name)
    x, want = ffa_cases.data(case, kind), ffa_cases.expected(case, kind)
    n_elem = int(np.prod(case.s, dtype=int))
    p_lo, p_hi = case.periods
    plan = hip.FfaPlan(case.n, case.periods, case.K, n_elem)
    aligned = None
    for skew in SKEWS:
        got = np.empty_like(want)
        for b in range(want.shape[0]):
            block = x[b * case.n:(b + 1) * case.n]
            gx, go = Guarded.load(block, poison, skew), Guarded(want.shape[1:], F32, poison, skew)
            if chunked:
                cut = min(n_elem, 6)
                for e0 in range(0, cut, 2):
                    for pa in range(p_lo, p_hi, 2):
                        plan.execute(gx.array, go.array, e0, min(2, cut - e0), pa, min(p_hi, pa + 2))
                if cut < n_elem:                                # (the other columns, every base period at once)
                    plan.execute(gx.array, go.array, cut, n_elem - cut)
            else:
                plan.execute(gx.array, go.array)
            got_x, got[b] = check_all([gx, go], f'ffa {name} block {b}')
            assert got_x.tobytes() == np.ascontiguousarray(block).tobytes()
        assert ffa_cases.same_bits(got, want)
        if aligned is not None:
            assert ffa_cases.same_bits(got, aligned), 'the run 4 bytes off differs from the aligned run'
        aligned = got
    plan.close()
