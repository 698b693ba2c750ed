"""The ledger of tests/phase_cases.py: what every case of test_phase_runs_guard_gpu.py reaches, asserted from
`plan_pieces`' plan and the `piece_table` twin alone, without a device.  A case whose claim stops holding (a
changed builder, a changed plan) fails here; it does not quietly stop testing its edge.

The figures of `LEDGER` are (runs of the twin, `run_cap` of the plan, cells of the grid, pieces); the other
claims are spelled out case by case below."""
import numpy as np
import pytest

import phase_cases
from phase_cases import BY_NAME, CASES, GROUP, STEP_BACK, TILE, facts, plan_of, sample_bins, twin

from baseband_tasks_amd.fold_table import piece_table, plan_pieces

# name: (n_run, run_cap, n_cell, n_piece)
LEDGER = {
    'tiny_1': (1, 1, 8, 1), 'tiny_2': (1, 1, 8, 1), 'tiny_3': (1, 1, 8, 1), 'tiny_4': (2, 2, 8, 1),
    'tiny_5': (2, 2, 8, 1),
    'tile_edges_1023': (1023, 1023, 3424, 5), 'tile_edges_1024': (1024, 1024, 3440, 6),
    'tile_edges_1025': (1025, 1025, 3440, 7),
    'odd_cells': (821, 821, 833, 6),
    'cell_tails_1021': (1021, 1021, 1021, 1), 'cell_tails_1023': (1023, 1023, 1023, 1),
    'cell_tails_1024': (1024, 1024, 1024, 1), 'cell_tails_1025': (1025, 1025, 1025, 1),
    'cell_tails_1027': (1027, 1027, 1027, 1),
    'wide_grid': (700, 700, 274432, 3),
    'many_sample_tiles': (264, 264, 320, 1),
    'row_only_starts': (4, 4, 192, 3),
    'many_pieces': (343, 343, 352, 257),
    'negative': (821, 821, 833, 6),
    'constant': (3, 3, 48, 3),
    'padded64': (1025, 1025, 3440, 7),
    'inside_a_row': (815, 815, 826, 3),
}


def test_the_ledger_names_every_case():
    assert sorted(LEDGER) == sorted(BY_NAME)


@pytest.mark.parametrize('name', sorted(LEDGER))
def test_figures_and_counts(name):
    case = BY_NAME[name]
    f = facts(case)
    print(name, f)
    assert (f['n_run'], f['run_cap'], f['n_cell'], f['n_piece']) == LEDGER[name]
    assert f['n_run'] <= f['run_cap'] <= f['n']
    # the twin's counts sum to the chunk's samples, its runs tile them, and every run has a cell of its own
    assert f['samples_counted'] == f['n'] == case.chunk[1] - case.chunk[0]
    slot_ptr, run_begin, run_end, counts = twin(case)
    assert slot_ptr[0] == 0 and slot_ptr[-1] == f['n_run'] and len(counts) == len(slot_ptr) - 1
    order = np.argsort(run_begin)
    assert run_begin[order][0] == 0 and run_end[order][-1] == f['n']
    np.testing.assert_array_equal(run_begin[order][1:], run_end[order][:-1])
    assert f['steps_back'] == 0 and f['distinct'] == f['n_run']


def test_tiny_is_less_than_a_group_and_one_more():
    assert [facts(BY_NAME[f'tiny_{n}'])['n'] for n in (1, 2, 3, 4, 5)] == [1, 2, 3, GROUP, GROUP + 1]
    assert facts(BY_NAME['tiny_1'])['n_run'] == 1 == facts(BY_NAME['tiny_1'])['run_cap']


def test_tile_edges():
    for n in (TILE - 1, TILE, TILE + 1):
        f = facts(BY_NAME[f'tile_edges_{n}'])
        assert f['n'] == n and f['n_run'] == f['run_cap'] == n                # (every sample a run: no spare capacity)
        assert f['sample_tiles'] == (2 if n > TILE else 1)
        assert f['one_sample_pieces'] >= 3
    # a piece edge at each offset of a thread's four samples, and one on the tile's edge
    f = facts(BY_NAME['tile_edges_1025'])
    assert f['edge_offsets'] == [0, 1, 2, 3] and f['edge_on_tile'] and f['cell_tiles'] == 4


def test_cell_counts_off_the_int4_path_and_off_a_tile():
    f = facts(BY_NAME['odd_cells'])
    assert f['n_cell_mod4'] == 1 and f['sample_tiles'] == 3 and f['edge_offsets'] == [0, 1, 2, 3]
    assert f['row_only_starts'] == 1          # (sample 1025 is 410 bins on, less one rounding: row 1 starts in row 0's last bin)
    want = {1021: (1, 1), 1023: (3, 1), 1024: (0, 1), 1025: (1, 2), 1027: (3, 2)}
    for c, (mod4, cell_tiles) in want.items():
        f = facts(BY_NAME[f'cell_tails_{c}'])
        assert (f['n_cell'], f['n_cell_mod4'], f['cell_tiles']) == (c, mod4, cell_tiles)
        assert f['n'] == 4 * c


def test_more_than_256_tiles():
    f = facts(BY_NAME['wide_grid'])
    assert f['cell_tiles'] == 268 > 256 and f['sample_tiles'] == 1            # (k_scan_tiles' second trip, for cells)
    assert f['n_run'] == 700 and f['n_cell'] > 300 * f['n_run']              # (almost all empty)
    f = facts(BY_NAME['many_sample_tiles'])
    assert f['sample_tiles'] == 258 > 256 and f['cell_tiles'] == 1            # (and for samples)
    assert f['n'] % TILE == 1 and f['n_run'] < f['n'] // 900


def test_row_only_starts_exist():
    case = BY_NAME['row_only_starts']
    f = facts(case)
    assert f['row_only_starts'] == 2 and f['one_sample_rows'] == 1
    row, k = sample_bins(case)
    assert k[499] == k[500] == k[501] and list(row[499:502]) == [0, 1, 2]
    f = facts(BY_NAME['constant'])
    assert f['n_coeff'] == 1 and f['row_only_starts'] == 2 and f['n_run'] == 3 == len(BY_NAME['constant'].edges) - 1
    plan = plan_of(BY_NAME['constant'])
    assert np.all(plan['n_cycle'] == 1)                                       # (k_first == k_last in every row)


def test_piece_search_and_widths():
    f = facts(BY_NAME['many_pieces'])
    assert f['n_piece'] == 257 and f['edge_offsets'] == [0] and f['edge_on_tile']
    f = facts(BY_NAME['padded64'])
    assert f['n_coeff'] == 64
    # the padding changes no bin
    for a, b in zip(twin(BY_NAME['padded64']), twin(BY_NAME['tile_edges_1025'])):
        np.testing.assert_array_equal(a, b)


def test_negative_bins_and_chunk_inside_a_row():
    case = BY_NAME['negative']
    f = facts(case)
    assert f['k_min'] == -3 * case.n_phase and f['k0_min'] == -3 * case.n_phase
    row, k = sample_bins(case)
    assert k.min() < 0 < k.max() and np.any(k == 0)                           # (the phase crosses 0 inside the chunk)
    # apart from the shift, odd_cells
    for a, b in zip(twin(case), twin(BY_NAME['odd_cells'])):
        np.testing.assert_array_equal(a, b)
    case = BY_NAME['inside_a_row']
    f = facts(case)
    assert f['m0_first'] == 7 > 0 and case.chunk == (7, 2041)
    assert plan_of(case)['lo'][0] == 0                                        # (lo counts from the chunk's start)
    assert f['n_cell_mod4'] == 2 and f['edge_offsets'] == [1, 2]


# -- the refusals ----------------------------------------------------------------------------------------------
def test_capacity_and_grid_refusals_have_something_to_refuse():
    for name in ('odd_cells', 'tile_edges_1025'):
        f = facts(BY_NAME[name])
        assert f['run_cap'] == f['n_run'] >= 2                                # (one less is one short)
    plan = plan_of(BY_NAME['odd_cells'])
    assert plan['n_cycle'][-1] >= 2
    row, k = sample_bins(BY_NAME['odd_cells'])
    assert (k[-1] - plan['k0'][-1]) // 7 == plan['n_cycle'][-1] - 1           # (the last cycle is in use)


@pytest.mark.parametrize('which', sorted(STEP_BACK))
def test_step_back_passes_the_plan_and_the_twin_refuses_it(which):
    case = STEP_BACK[which]
    row, k = sample_bins(case)
    assert np.count_nonzero(np.diff(k) < 0) == 1 and k[12] < k[11] and k[-1] >= k[0]
    r0, n_row, plan = plan_pieces(np.array(case.edges), phase_cases.row_pieces_of(case), case.n_phase, *case.chunk)
    assert plan['run_cap'] == 24 and list(plan['k0']) == [16]
    assert np.all((k - 16) // case.n_phase < plan['n_cycle'][0])               # (every bin inside the row's grid)
    if which == 'shared_cells':
        assert list(plan['n_cycle']) == [8] and len(np.unique(k)) == 22       # two cells get two runs each
    else:
        assert len(np.unique(k)) == 24                                        # a cell per run, out of time order
    with pytest.raises(ValueError, match='phase must increase with time'):
        piece_table(np.array(case.edges), phase_cases.row_pieces_of(case), case.n_phase, *case.chunk)
