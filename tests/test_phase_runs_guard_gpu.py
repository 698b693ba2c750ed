"""`bbt_phase_runs` (csrc/phase_kernels.hpp: count, scan, scatter into a grid, count, scan, compact, binary
search) between guard bands (tests/guard_bands.py), on the synthetic phases of tests/phase_cases.py, whose
ledger (test_phase_cases_host.py) says which edge of the kernels each of them reaches.

The entry point is called directly, after `bbt_phase_runs_work`.  Every device array of a call is a `Guarded`:
the pieces and the rows it reads; `slot_ptr`, `run_begin`, `run_end` and `counts`, poisoned throughout; and a
work area of EXACTLY the bytes `bbt_phase_runs_work` returns, so that a word past the layout is in a band.
The int64 arrays run 0 and 8 bytes off the 16-byte grid, the work area on it (the entry point asks for that).
Everything is compared by equality with the twin, `fold_table.piece_table`: ``info == (n_run, 0)``, the table,
the counts, the capacity beyond the runs still poison word for word, the inputs unchanged, all bands clean.
A refused call (status != 0) leaves `slot_ptr` all zeros, the runs untouched and all bands clean; none of them
leaves its arrays: the kernels clamp every index they form.

The chain hands the guarded table to `hip.fold_runs_device`, with a guarded input and a guarded output of its
own: small integers as `fold_cases.make_input` makes them, so that the float32 sums are exact and equal to
`fold_cases.fold_reference` on the twin's table; a sample read outside the input is a NaN or an infinity in a
sum."""
import ctypes as C

import numpy as np
import pytest

import baseband_tasks_amd as bt
from baseband_tasks_amd import hip

import fold_cases as fc
from guard_bands import POISONS, Guarded, check_all
from phase_cases import BY_NAME, STEP_BACK, arguments, n_rows, new_case, plan_of, row_pieces_of, twin

pytestmark = pytest.mark.gpu

both_poisons = pytest.mark.parametrize('poison', list(POISONS.values()), ids=list(POISONS))
both_skews = pytest.mark.parametrize('skew', [0, 8], ids=['on16', 'off8'])
#: the cases of the variants and the refusals
FOUR = ['tile_edges_1025', 'odd_cells', 'row_only_starts', 'cell_tails_1025']


def poison64(poison):
    """An int64 of two poison words."""
    return np.array([poison, poison], '<u4').view(np.int64)[0]


class Call:
    """The guarded arrays of one call of bbt_phase_runs for ``plan``, and the call."""

    def __init__(self, plan, n_phase, poison, skew, slot0=0, n_slot=None, run_cap=None):
        self.words, self.rows, self.n_cell = arguments(plan, n_phase)
        self.n_phase, self.poison = int(n_phase), poison
        self.n_piece, self.n_coeff = len(plan['row']), plan['coeff'].shape[1]
        self.n_row = len(plan['k0'])
        self.n_chunk_slot = self.n_row * self.n_phase
        self.slot0 = slot0
        self.n_slot = self.n_chunk_slot + slot0 if n_slot is None else n_slot
        self.run_cap = int(plan['run_cap']) if run_cap is None else run_cap
        self.s_begin, self.s_end = int(plan['lo'][0]), int(plan['lo'][-1])
        need = C.c_int64()
        hip.check(hip.lib().bbt_phase_runs_work(self.s_end - self.s_begin, self.n_cell, self.run_cap, C.byref(need)))
        self.need = need.value
        assert self.need % 8 == 0
        self.pieces = Guarded.load(self.words, poison, skew)
        self.rows_dev = Guarded.load(self.rows, poison, skew)
        self.slot_ptr = Guarded((self.n_slot + 1,), np.int64, poison, skew)
        self.run_begin = Guarded((self.run_cap,), np.int64, poison, skew)
        self.run_end = Guarded((self.run_cap,), np.int64, poison, skew)
        self.counts = Guarded((self.n_chunk_slot,), np.int64, poison, skew)
        self.work = Guarded((self.need // 8,), np.int64, poison, 0)
        assert self.work.nbytes == self.need and self.work.array.ptr % 16 == 0
        self.info = None

    def launch(self):
        info = (C.c_int64 * 2)(-1, -1)
        hip.check(hip.lib().bbt_phase_runs(
            self.pieces.array.ptr, self.n_piece, self.n_coeff, self.s_begin, self.s_end, self.n_phase,
            self.rows_dev.array.ptr, self.n_row, self.n_cell, self.slot0, self.n_slot, self.run_cap,
            self.slot_ptr.array.ptr, self.run_begin.array.ptr, self.run_end.array.ptr, self.counts.array.ptr,
            self.work.array.ptr, self.need, info, hip._stream))
        self.info = (int(info[0]), int(info[1]))
        return self.info

    def download(self, what):
        """All bands clean and the inputs unchanged; (slot_ptr, run_begin, run_end, counts) on the host."""
        words, rows, slot_ptr, run_begin, run_end, counts, _ = check_all(
            [self.pieces, self.rows_dev, self.slot_ptr, self.run_begin, self.run_end, self.counts, self.work], what)
        assert words.tobytes() == self.words.tobytes(), f'{what}: the pieces changed'
        np.testing.assert_array_equal(rows, self.rows, err_msg=f'{what}: the rows changed')
        return slot_ptr, run_begin, run_end, counts

    def check_table(self, table, what):
        """The call gave the twin's table, and wrote nothing else."""
        sp, rb, re, cnt = table
        n_run = len(rb)
        print(f'{what}: info {self.info}, {n_run} runs of the twin, capacity {self.run_cap}, {self.n_cell} cells, '
              f'work area {self.need} bytes')
        slot_ptr, run_begin, run_end, counts = self.download(what)
        assert self.info == (n_run, 0), what
        tail = self.n_slot - self.slot0 - self.n_chunk_slot
        np.testing.assert_array_equal(slot_ptr, np.concatenate((np.zeros(self.slot0, np.int64), sp,
                                                                np.full(tail, n_run, np.int64))), err_msg=what)
        np.testing.assert_array_equal(counts, cnt, err_msg=what)
        np.testing.assert_array_equal(run_begin[:n_run], rb, err_msg=what)
        np.testing.assert_array_equal(run_end[:n_run], re, err_msg=what)
        assert np.all(run_begin[n_run:] == poison64(self.poison)), f'{what}: run_begin written beyond the runs'
        assert np.all(run_end[n_run:] == poison64(self.poison)), f'{what}: run_end written beyond the runs'

    def check_refused(self, what, n_run=None):
        """Status set, an empty table, the runs untouched, all bands clean."""
        print(f'{what}: info {self.info}, capacity {self.run_cap}, {self.n_cell} cells')
        slot_ptr, run_begin, run_end, counts = self.download(what)
        assert self.info[1] != 0, f'{what}: status 0, {self.info[0]} runs'
        if n_run is not None:
            assert self.info[0] == n_run, what
        assert not slot_ptr.any(), f'{what}: slot_ptr is not all zeros'
        assert np.all(run_begin == poison64(self.poison)) and np.all(run_end == poison64(self.poison)), \
            f'{what}: runs written by a refused call'


# -- every case, as the plan gives it --------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(BY_NAME))
@both_skews
@both_poisons
def test_device_table_between_bands(name, poison, skew):
    case = BY_NAME[name]
    call = Call(plan_of(case), case.n_phase, poison, skew)
    assert call.n_row == n_rows(case)
    call.launch()
    call.check_table(twin(case), name)


# -- variants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FOUR)
@both_skews
@both_poisons
def test_slot_offset(name, poison, skew):
    """Zeros in front, a flat tail: the chunk's rows in the middle of an output."""
    case = BY_NAME[name]
    call = Call(plan_of(case), case.n_phase, poison, skew, slot0=3, n_slot=n_rows(case) * case.n_phase + 7)
    call.launch()
    call.check_table(twin(case), f'{name}, slot0 3')


@pytest.mark.parametrize('name', FOUR)
@both_skews
@both_poisons
def test_larger_capacity(name, poison, skew):
    """Five more runs allowed than there are: the same table, the spare capacity untouched.  A capacity above
    the number of samples is no capacity the entry points take (every sample a run is the most there is): where
    the runs are the samples, that is what is asserted, before anything is launched."""
    case = BY_NAME[name]
    plan = plan_of(case)
    cap = int(plan['run_cap']) + 5
    if cap > case.chunk[1] - case.chunk[0]:
        assert name == 'tile_edges_1025'
        with pytest.raises(hip.HipError, match='out of range'):
            Call(plan, case.n_phase, poison, skew, run_cap=cap)
        return
    call = Call(plan, case.n_phase, poison, skew, run_cap=cap)
    call.launch()
    call.check_table(twin(case), f'{name}, capacity {cap}')


@pytest.mark.parametrize('name', FOUR)
@both_skews
@both_poisons
def test_twice_through_the_same_arrays(name, poison, skew):
    """Once more without poisoning anything again: the grid, the scalars and the counts are zeroed by the entry
    point itself."""
    case = BY_NAME[name]
    call = Call(plan_of(case), case.n_phase, poison, skew)
    first = call.launch()
    call.check_table(twin(case), f'{name}, first call')
    assert call.launch() == first
    call.check_table(twin(case), f'{name}, second call')


# -- refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['odd_cells', 'tile_edges_1025'])
@both_skews
@both_poisons
def test_capacity_one_short_is_refused(name, poison, skew):
    case = BY_NAME[name]
    n_run = len(twin(case)[1])
    call = Call(plan_of(case), case.n_phase, poison, skew, run_cap=n_run - 1)
    call.launch()
    call.check_refused(f'{name}, capacity {n_run - 1} for {n_run} runs', n_run)
    assert call.info[1] & 1


@both_skews
@both_poisons
def test_grid_one_cycle_short_is_refused(poison, skew):
    case = BY_NAME['odd_cells']
    plan = plan_of(case)
    plan['n_cycle'][-1] -= 1
    call = Call(plan, case.n_phase, poison, skew)
    call.launch()
    call.check_refused('odd_cells, the last row one cycle short', len(twin(case)[1]))
    assert call.info[1] & 2


@pytest.mark.parametrize('which', sorted(STEP_BACK))
@both_skews
@both_poisons
def test_step_back_is_refused(which, poison, skew):
    """A phase that steps back between two pieces of a row and passes `plan_pieces` (test_phase_cases_host.py):
    onto bins the row already visited, two runs share a cell of the grid, fewer cells are occupied than there
    are runs, and before status bits 4 and 8 existed the call returned status 0 with 24 runs of which only the
    22 first were written; onto bins the row stepped over, every run has its cell and only bit 8 tells."""
    case = STEP_BACK[which]
    call = Call(plan_of(case), case.n_phase, poison, skew)
    call.launch()
    call.check_refused(f'step back, {which}', 24)
    assert call.info[1] == (12 if which == 'shared_cells' else 8)


@both_skews
@both_poisons
def test_a_row_that_comes_back_is_refused(poison, skew):
    """Pieces of rows 0, 1, 0 with one bin throughout: no sample's bin is below its predecessor's in the same
    row, but the third run has the first run's cell: bit 4 alone."""
    case = new_case('rows_return', 12, 1000, 8, edges=(0, 8, 12), cuts=(4,))
    plan = plan_of(case)
    assert list(plan['row']) == [0, 0, 1] and list(plan['n_cycle']) == [1, 1]
    plan['row'][:] = [0, 1, 0]
    call = Call(plan, case.n_phase, poison, skew, run_cap=3)
    call.launch()
    call.check_refused('rows 0, 1, 0', 3)
    assert call.info[1] == 4


@pytest.mark.parametrize('route', ['device', 'host'])
def test_fold_refuses_a_phase_that_steps_back(route):
    """`Fold` on either `table_route`: both give the same table, and both refuse the same phase."""
    case = STEP_BACK['shared_cells']
    pieces = row_pieces_of(case)

    class SteppedBack:
        def fold_pieces(self, t_ref, rate, lo, hi):
            return pieces(0, lo, hi)

        def __call__(self, t):
            raise AssertionError('a phase that offers pieces is not called')
    x = np.ones((case.n, 2), np.float32)
    sh = bt.HostStream(x, bt.Time('2010-11-12T13:14:15'), 1e3, samples_per_frame=case.n, pin=False)
    fold = bt.Fold(sh, case.n_phase, SteppedBack())
    fold.table_route = route
    assert fold._route() == route
    with pytest.raises(ValueError, match='increase with time'):
        fold.read()


# -- the chain: the guarded table folds a guarded input ---------------------------------------------------------
CHAIN = [(name, mode, n_elem, skew) for name in ('odd_cells', 'row_only_starts', 'tiny_5')
         for mode, n_elem, skew in ((2, 5, 0), (2, 5, 4), (1, 4, 0))]


@pytest.mark.parametrize('name, mode, n_elem, skew', CHAIN,
                         ids=[f'{n}-mode{m}-{e}-skew{s}' for n, m, e, s in CHAIN])
@both_poisons
def test_guarded_table_folds_a_guarded_input(name, mode, n_elem, skew, poison):
    """Mode 2 at 5 floats a sample, the input on the 16-byte grid and 4 bytes off it; mode 1 at 2 (X, Y) pairs a
    sample."""
    case = BY_NAME[name]
    sp, rb, re, cnt = table = twin(case)
    n_run, n_slot = len(rb), len(cnt)
    call = Call(plan_of(case), case.n_phase, poison, 0)
    call.launch()
    call.check_table(table, name)
    n_in = case.chunk[1] - case.chunk[0]
    x = fc.make_input(fc.new_case(f'phase_{name}', mode, n_elem, n_in, n_slot))
    total, mass = fc.fold_reference(x, mode, sp, rb, re)
    assert mass.max() < fc.EXACT
    want = fc.expected_float32(total, None)
    gx = Guarded.load(x, poison, skew)
    out = Guarded(want.shape, np.float32, poison, 0)
    hip.fold_runs_device(gx.array, out.array, n_elem, mode, call.slot_ptr.array, call.run_begin.array[:n_run],
                         call.run_end.array[:n_run])
    got_x, got = check_all([gx, out], f'{name}, fold mode {mode}')
    assert got_x.tobytes() == x.tobytes()
    np.testing.assert_array_equal(got, want)
    call.check_table(table, f'{name}, after the fold')                              # (the fold only read the table)
