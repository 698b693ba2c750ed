"""What tests/fold_cases.py claims, proved without a GPU: its NumPy fold of a run table equals
a brute-force fold, every case sums exactly in float32, and the case list reaches every shape
of the fold launcher it says it does (as `fold_cases.fold_dispatch` restates the launcher)."""
import numpy as np
import pytest

import fold_cases as fc


# -- the reference against loops ---------------------------------------------------------------
TINY = {
    # mode: (n_elem, slot_ptr, run_begin, run_end): an empty slot, runs out of time order, a run
    # twice, runs that stick out of the input at both ends, an empty and a reversed run
    0: (3, [0, 2, 2, 5], [4, 0, 7, -3, 9], [9, 2, 7, 2, 14]),
    1: (4, [0, 1, 4, 4], [5, 0, 0, 11], [12, 3, 3, 10]),
    2: (5, [0, 0, 3, 4], [2, 3, 20, 6], [3, 8, 25, 13]),
}


@pytest.mark.parametrize('mode', sorted(TINY))
def test_reference_equals_brute_force(mode):
    n_elem, slot_ptr, begin, end = TINY[mode]
    rng = np.random.default_rng(mode)
    n_in, n_slot = 12, len(slot_ptr) - 1
    if mode == 2:
        x = rng.integers(-4, 5, size=(n_in, n_elem)).astype(np.float32)
    else:
        x = (rng.integers(-4, 5, size=(n_in, n_elem)) + 1j * rng.integers(-4, 5, size=(n_in, n_elem))).astype(np.complex64)
    width = 2 * n_elem if mode == 1 else n_elem
    prev = rng.integers(-9, 10, size=(n_slot, width)).astype(np.float32)
    scale = np.array([0.3, np.nan, 4.], np.float32)
    for p, s in ((None, None), (prev, None), (prev, scale), (None, scale)):
        got, mass = fc.fold_reference(x, mode, slot_ptr, begin, end, p, s)
        want = fc.brute_force(x, mode, slot_ptr, begin, end, p, s)
        assert got.shape == (n_slot, width)
        np.testing.assert_array_equal(got, want)
        assert np.all(mass >= np.abs(fc.fold_reference(x, mode, slot_ptr, begin, end, p, None)[0]))
    # the same data as floats that are no integers: the float64 path
    y = (x * np.float32(0.37)).astype(x.dtype)
    got, _ = fc.fold_reference(y, mode, slot_ptr, begin, end, prev, None)
    np.testing.assert_allclose(got, fc.brute_force(y, mode, slot_ptr, begin, end, prev, None), rtol=1e-12, atol=1e-12)


# -- every case is exact ---------------------------------------------------------------------
def test_the_case_list_is_small():
    assert len(fc.CASES) <= 40
    for case in fc.CASES:
        n_bytes = case.n_in * case.n_elem * (4 if case.mode == 2 else 8)
        assert n_bytes <= 20 << 20, case.name
        assert case.n_in <= (8192 if case.n_elem > 64 else 1 << 17), case.name


@pytest.mark.parametrize('case', fc.CASES, ids=lambda case: case.name)
def test_sums_of_a_case_are_exact_in_float32(case):
    table = fc.make_table(case)
    x, prev, scale = fc.make_input(case), fc.make_prev(case), fc.make_scale(case, table)
    slot_ptr, begin, end = table
    assert slot_ptr[0] == 0 and slot_ptr[-1] == len(begin) == len(end) and np.all(np.diff(slot_ptr) >= 0)
    # a table `hip.fold_runs` accepts
    assert begin.min() >= 0 and end.max() <= case.n_in and np.all(end >= begin)
    parts = x.view(np.float32)
    assert np.array_equal(parts, np.rint(parts)) and np.abs(parts).max() <= 4
    total, mass = fc.fold_reference(x, case.mode, *table, prev, None)
    assert mass.max() < fc.EXACT, mass.max()
    want = fc.expected_float32(total, scale)
    assert want.dtype == np.float32
    if scale is not None:
        # one float32 product of two float32 numbers is the rounded exact product, which float64 holds
        scaled, _ = fc.fold_reference(x, case.mode, *table, prev, scale)
        np.testing.assert_array_equal(scaled.astype(np.float32), want)
        assert np.all(np.isnan(want[np.isnan(scale)])) and not np.any(np.isnan(want[~np.isnan(scale)]))
        hollow = fc.slot_samples(*table, case.n_in) == 0
        assert not np.any(np.isnan(scale[~hollow]))


# -- the cases span the launcher's grid --------------------------------------------------------
def test_the_cases_cover_every_required_cell():
    assert fc.missing_cells(fc.CASES) == []


def test_the_dispatch_of_the_issue_example():
    """n_slot = 2, n_unit = 300, n_in = 4096: 2 tiles and 32 shares."""
    d = fc.fold_dispatch(4096, 600, 1, 2, True, fc.fold_work_floats(2, 600, 1))
    assert (d['n_unit'], d['lg_tc'], d['tt'], d['tiles'], d['split']) == (300, 8, 1, 2, 32)


def test_the_coverage_check_bites():
    """Without the only case of a cell, the cell is reported missing -- for every such cell."""
    owners = {}
    for case in fc.CASES:
        for cell in fc.cells_of(case):
            owners.setdefault(cell, []).append(case)
    alone = {cell: cases[0] for cell, cases in owners.items() if cell in fc.REQUIRED_CELLS and len(cases) == 1}
    assert ('n_unit', 1029) not in alone and ('tiles', 5) in owners      # (cells of several cases exist too)
    assert ('lg_tc', 4) in alone and ('n_unit', 128) in alone
    for cell, case in alone.items():
        rest = [c for c in fc.CASES if c is not case]
        assert cell in fc.missing_cells(rest), (cell, case.name)
