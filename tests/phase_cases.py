"""Synthetic phases for the fold-table kernels (bbt_phase_runs, csrc/phase_kernels.hpp), shared by
test_phase_cases_host.py -- the ledger: what every case reaches, asserted from the plan and the twin alone --
and test_phase_runs_guard_gpu.py, which launches them between guard bands.

No polyco is needed: `fold_table.piece_table` (the twin: every sample's bin from `polynomial_bins`, the stated
bit-for-bit definition of the kernel's `phase_bin`) and `fold_table.plan_pieces` (the kernel's arguments) take
any ``row_pieces(r, lo, hi)`` callback.  The phases here are linear, ``coeff = [0, 1]`` with ``step = 1 /
(per_bin * n_phase)`` and ``dt0 = n_ref * step``, so that the phase is continuous over the rows, plus a
reference phase ``ref_int + ref_frac``; rows are cut into pieces at absolute sample positions, and a piece may
start a number of bins BACK from where the one before it ended (the refusals).

The tile is 1024 samples or cells (BBT_PHASE_TILE), a thread has four of either."""
import functools
from collections import namedtuple

import numpy as np

from baseband_tasks_amd import hip
from baseband_tasks_amd.fold_table import piece_table, plan_pieces, polynomial_bins

TILE = 1024
GROUP = 4

#: n samples at ``per_bin`` samples per bin of ``n_phase`` bins; ``edges`` the row edges (absolute samples);
#: ``cuts`` absolute positions that split a row into pieces; the phase of sample 0 is ``ref_int + ref_frac``;
#: ``chunk`` the samples [c0, c1) of the table; ``coeff`` None for the linear phase, else the coefficients of
#: every piece; ``width``: the coefficients padded with zeros to that many; ``back``: ((position, bins), ...),
#: the pieces from ``position`` on lie ``bins`` bins back.
Case = namedtuple('Case', 'name n per_bin n_phase edges cuts ref_int ref_frac chunk coeff width back')


def new_case(name, n, per_bin, n_phase, edges=None, cuts=(), ref_int=0, ref_frac=0., chunk=None, coeff=None,
             width=None, back=()):
    edges = (0, n) if edges is None else tuple(int(e) for e in edges)
    assert edges[0] == 0 and edges[-1] == n and all(a < b for a, b in zip(edges[:-1], edges[1:]))
    assert -0.5 <= ref_frac <= 0.5
    return Case(name, n, per_bin, n_phase, edges, tuple(cuts), ref_int, ref_frac, tuple(chunk or (0, n)),
                None if coeff is None else tuple(coeff), width, tuple(back))


def row_pieces_of(case):
    """The ``row_pieces(r, lo, hi)`` callback of a case: tuples (m_begin, m_end, coeff, dt0, step, ref_int,
    ref_frac) with m counted from the row's first sample."""
    step = 1. / (case.per_bin * case.n_phase)
    coeff = np.array([0., 1.] if case.coeff is None else case.coeff, float)
    if case.width:
        coeff = np.concatenate((coeff, np.zeros(case.width - len(coeff))))

    def row_pieces(r, lo, hi):
        n_ref = case.edges[r]
        at = [lo] + [c for c in sorted(set(case.cuts) | {p for p, _ in case.back}) if lo < c < hi] + [hi]
        pieces = []
        for a, b in zip(at[:-1], at[1:]):
            bins = sum(bins for p, bins in case.back if p <= a)
            ref = case.ref_int + case.ref_frac - bins / case.n_phase       # (exact: the cases keep it dyadic)
            ref_int = float(np.round(ref))
            pieces.append((a - n_ref, b - n_ref, coeff, n_ref * step, step, ref_int, ref - ref_int))
        return pieces
    return row_pieces


@functools.lru_cache(maxsize=None)
def twin(case):
    """`piece_table` of the case: (slot_ptr, run_begin, run_end, counts), host int64, computed once and read-only."""
    r0, n_row, *table = piece_table(np.array(case.edges), row_pieces_of(case), case.n_phase, *case.chunk)
    for a in table:
        a.setflags(write=False)
    return tuple(table)


@functools.lru_cache(maxsize=None)
def _plan(case):
    r0, n_row, plan = plan_pieces(np.array(case.edges), row_pieces_of(case), case.n_phase, *case.chunk)
    return r0, n_row, plan


def plan_of(case):
    """A copy of `plan_pieces`' plan for the case (the refusals edit theirs)."""
    plan = _plan(case)[2]
    return {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in plan.items()}


def n_rows(case):
    return _plan(case)[1]


def arguments(plan, n_phase):
    """What bbt_phase_runs reads: (the pieces' 8-byte words as float64, rows = k0 | n_cycle | cell0 as int64,
    n_cell), laid out as `hip.phase_runs` lays them out."""
    cell0 = np.concatenate(([0], np.cumsum(plan['n_cycle'] * int(n_phase))))
    rows = np.concatenate([plan['k0'], plan['n_cycle'], cell0[:-1]]).astype(np.int64)
    return hip._piece_words(plan), rows, int(cell0[-1])


def sample_bins(case):
    """(row, k) of every sample of the chunk, int64, from `polynomial_bins` piece by piece."""
    c0, c1 = case.chunk
    row, k = np.full(c1 - c0, -1, np.int64), np.zeros(c1 - c0, np.int64)
    pieces = row_pieces_of(case)
    for r in range(len(case.edges) - 1):
        lo, hi = max(c0, case.edges[r]), min(c1, case.edges[r + 1])
        if hi <= lo:
            continue
        for (a, b, *piece) in pieces(r, lo, hi):
            at = slice(a + case.edges[r] - c0, b + case.edges[r] - c0)
            row[at] = r
            k[at] = polynomial_bins(*piece, np.arange(a, b), case.n_phase)
    assert row.min() >= 0
    return row, k


def tiles(n):
    return -(-n // TILE)


def facts(case):
    """What the case reaches, from the plan and the twin alone (the ledger asserts these)."""
    plan = _plan(case)[2]
    slot_ptr, run_begin, run_end, counts = twin(case)
    row, k = sample_bins(case)
    n = len(k)
    n_cell = int((plan['n_cycle'] * case.n_phase).sum())
    inner = plan['lo'][1:-1] - plan['lo'][0]
    new_row = np.flatnonzero(row[1:] != row[:-1]) + 1
    rows_present = np.unique(row)
    per_row = [k[row == r] for r in rows_present]
    return dict(
        n=n, n_run=len(run_begin), run_cap=int(plan['run_cap']), n_cell=n_cell, n_cell_mod4=n_cell % GROUP,
        sample_tiles=tiles(n), cell_tiles=tiles(n_cell), n_piece=len(plan['row']), n_coeff=plan['coeff'].shape[1],
        edge_offsets=sorted({int(e) % GROUP for e in inner}),
        edge_on_tile=bool(np.any(inner % TILE == 0)),
        one_sample_pieces=int(np.count_nonzero(np.diff(plan['lo']) == 1)),
        row_only_starts=int(np.count_nonzero(k[new_row] == k[new_row - 1])),
        one_sample_rows=int(np.count_nonzero(np.bincount(row - row.min()) == 1)),
        k_min=int(k.min()), k0_min=int(plan['k0'].min()), m0_first=int(plan['m0'][0]),
        steps_back=int(sum(np.count_nonzero(np.diff(kr) < 0) for kr in per_row)),
        distinct=int(sum(len(np.unique(kr)) for kr in per_row)),
        samples_counted=int(counts.sum()))


# -- the cases -------------------------------------------------------------------------------------------------
def _tile_edges(n, **more):
    return dict(n=n, per_bin=0.3, n_phase=16, edges=(0, n // 2 + 1, n), cuts=(1, 2, 3, 1023, 1024), **more)


_ODD_CELLS = dict(n=2049, per_bin=2.5, n_phase=7, edges=(0, 1025, 2049), cuts=(5, 6, 7, 8))

CASES = (
    # fewer samples than a thread's four, and one more
    [new_case(f'tiny_{n}', n, 3, 8) for n in (1, 2, 3, 4, 5)]
    # every sample a run, the capacity exactly the runs; pieces of one sample; a piece edge at each offset of a
    # thread's group and on the tile's edge
    + [new_case(f'tile_edges_{n}', **_tile_edges(n)) for n in (1023, 1024, 1025)]
    # a cell count that is 1 modulo 4; three tiles of samples
    + [new_case('odd_cells', **_ODD_CELLS)]
    # n_cell = c: the last int4 of k_grid_count and its scalar tail, one off a tile of cells
    + [new_case(f'cell_tails_{c}', 4 * c, 4, 1) for c in (1021, 1023, 1024, 1025, 1027)]
    # more than 256 tiles of cells (the second trip of k_scan_tiles), almost all empty
    + [new_case('wide_grid', 700, 1. / 380., 4096, edges=(0, 234, 467, 700))]
    # more than 256 tiles of samples, few runs
    + [new_case('many_sample_tiles', 262144 + 1025, 1000, 64)]
    # runs that start because the row changes while k does not; a row of one sample
    + [new_case('row_only_starts', 1500, 1000, 64, edges=(0, 500, 501, 1500))]
    # the piece search over hundreds of pieces
    + [new_case('many_pieces', 1028, 3, 32, cuts=range(4, 1028, 4))]
    # the phase crosses 0 inside the chunk: negative k and k0
    + [new_case('negative', ref_int=-3, **_ODD_CELLS)]
    # n_coeff 1: one run per row, k_first == k_last
    + [new_case('constant', 1030, 1, 16, edges=(0, 1, 1025, 1030), coeff=(0.3,))]
    # the widest Horner loop
    + [new_case('padded64', **_tile_edges(1025, width=64))]
    # m0 > 0, lo relative to the chunk
    + [new_case('inside_a_row', chunk=(7, 2041), **_ODD_CELLS)]
)
BY_NAME = {case.name: case for case in CASES}
assert len(BY_NAME) == len(CASES)

#: Phases that step back between two pieces while the row's last bin is still at or above its first, so that
#: `plan_pieces` passes them: 3 bins a sample from k = 16; the second piece, from sample 12, starts 6 bins back
#: (on bins the first piece visited: two runs share a cell of the grid) or 5 bins back (on bins it stepped
#: over: every run has a cell of its own, out of time order).
STEP_BACK = {
    'shared_cells': new_case('step_back_shared_cells', 24, 1. / 3., 8, ref_int=2, back=((12, 6),)),
    'fresh_cells': new_case('step_back_fresh_cells', 24, 1. / 3., 8, ref_int=2, back=((12, 5),)),
}
