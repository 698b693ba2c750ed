"""Run tables for folding: which input samples go to which (row, phase bin), from
the sample times alone (host side of `Fold`, `PulseStack` and ``Integrate(phase=...)``).

Phase is monotonic in time, so the samples that share a phase bin form contiguous
runs.  A table for a chunk of input is in CSR form: slot ``j`` (``row * n_phase +
bin``) owns runs ``slot_ptr[j] .. slot_ptr[j+1]-1``, run ``r`` covers samples
``[run_begin[r], run_end[r])`` relative to the chunk start; ``counts[j]`` is the
number of samples of slot ``j`` (exact).

The bin of a sample is the reference's ``int((phase % 1 cycle) * n_phase)``
(baseband_tasks/integration.py:389-391).  Its unwrapped form ``k = floor(phase) *
n_phase + bin`` increases with time, which lets `bin_runs` find the bin edges by a
crossing search instead of calling the phase callable once per sample: ``k`` on a
grid a fraction of a bin apart, then, where it steps by one, the first sample of
the new bin from an interpolated guess checked against its neighbour (bisection if
the guess misses); where it steps by more, every sample of that interval.  For
monotonic phases the runs equal those of a per-sample evaluation exactly: every
sample's ``k`` comes from the same time expression, only fewer of them are asked.
"""
import numpy as np

__all__ = ['phase_parts', 'phase_difference', 'sample_times', 'bin_runs', 'fold_table',
           'contiguous_table', 'polynomial_bins', 'piece_table', 'plan_pieces']

#: samples handled in one piece by `bin_runs` (bounds host memory)
PIECE = 1 << 22


def _cycles(value):
    if hasattr(value, 'to_value'):
        return np.asarray(value.to_value('cycle'), dtype=float)
    return np.asarray(value, dtype=float)


def phase_parts(value):
    """Phase (cycles as an ndarray, a quantity with ``to_value('cycle')``, or a two-part
    phase with ``.int`` and ``.frac``) -> (whole cycles as int64, fraction in [0, 1))."""
    if hasattr(value, 'int') and hasattr(value, 'frac'):
        whole = _cycles(value.int)
        frac = _cycles(value.frac)
    else:
        cycles = _cycles(value)
        whole = np.floor(cycles)
        frac = cycles % 1.
    carry = np.floor(frac)
    return (whole + carry).astype(np.int64), frac - carry


def phase_difference(value, ref):
    """``value - ref`` in cycles (float64), taken part by part for two-part phases."""
    if hasattr(value, 'int') and hasattr(value, 'frac'):
        return ((_cycles(value.int) - _cycles(ref.int)) + (_cycles(value.frac) - _cycles(ref.frac)))
    return _cycles(value) - _cycles(ref)


def unwrapped_bin(value, n_phase):
    """``floor(phase) * n_phase + int((phase % 1) * n_phase)``, int64."""
    whole, frac = phase_parts(value)
    b = np.minimum((frac * n_phase).astype(np.int64), n_phase - 1)
    return whole * n_phase + b


def polynomial_bins(coeff, dt0, step, ref_int, ref_frac, m, n_phase):
    """Unwrapped bin of the samples ``m`` (int64 offsets from the row start) of a piece whose
    phase is a polynomial: ``x = dt0 + m * step``, ``phase = ref_int + ref_frac +
    sum_j coeff[j] x**j`` (``ref_int`` a whole number, ``ref_frac`` in [-0.5, 0.5]).

    This function is the definition of the bins of a phase that offers pieces (see
    `~baseband_tasks_amd.phases.PolycoPhase.fold_pieces`): the table kernel
    (csrc/phase_kernels.hpp) carries out the same float64 operations in the same order, none
    of them fused, so host and device agree bit for bit.
    """
    x = dt0 + np.asarray(m, dtype=np.int64).astype(np.float64) * step
    p = np.full(x.shape, coeff[-1], dtype=np.float64)
    for c in coeff[-2::-1]:
        p = p * x
        p = p + c
    whole = np.floor(p)
    frac = (p - whole) + ref_frac                   # in [-0.5, 1.5)
    carry = np.floor(frac)
    frac = frac - carry
    whole = whole.astype(np.int64) + carry.astype(np.int64) + np.int64(ref_int)
    b = np.minimum((frac * float(n_phase)).astype(np.int64), n_phase - 1)
    return whole * n_phase + b


def sample_times(t_ref, n_ref, sample_rate):
    """Function: int64 sample indices -> array-valued `Time` ``t_ref + (n - n_ref) / rate``."""
    def times(n):
        return t_ref + (np.asarray(n, dtype=np.int64) - n_ref) / sample_rate
    return times


def bin_runs(phase_at, n_phase, lo, hi):
    """Runs of constant unwrapped bin over samples [lo, hi).

    ``phase_at(n)``: phase of the int64 sample indices ``n`` (an array).
    Returns (begin, end, k) int64 arrays.
    """
    if hi <= lo:
        e = np.zeros(0, np.int64)
        return e, e, e
    begins, ends, ks = [], [], []
    for a in range(lo, hi, PIECE):
        b, e, k = _bin_runs_piece(phase_at, n_phase, a, min(hi, a + PIECE))
        if ks and ks[-1][-1] == k[0]:           # one run across the piece edge
            ends[-1][-1] = e[0]
            b, e, k = b[1:], e[1:], k[1:]
        begins.append(b)
        ends.append(e)
        ks.append(k)
    return np.concatenate(begins), np.concatenate(ends), np.concatenate(ks)


def _runs_from_samples(n, k):
    edge = np.flatnonzero(np.diff(k)) + 1
    starts = np.concatenate(([0], edge))
    begin = n[starts]
    end = np.concatenate((n[edge], [n[-1] + 1]))
    return begin.astype(np.int64), end.astype(np.int64), k[starts].astype(np.int64)


def _bin_runs_piece(phase_at, n_phase, lo, hi):
    n = hi - lo
    if n <= 16:
        samples = np.arange(lo, hi, dtype=np.int64)
        return _runs_from_samples(samples, unwrapped_bin(phase_at(samples), n_phase))
    ends = np.array([lo, hi - 1], np.int64)
    k_ends = unwrapped_bin(phase_at(ends), n_phase)
    if k_ends[1] == k_ends[0]:
        return (np.array([lo], np.int64), np.array([hi], np.int64), k_ends[:1].astype(np.int64))
    if k_ends[1] < k_ends[0]:
        raise ValueError("phase must increase with time")
    per_bin = (hi - 1 - lo) / float(k_ends[1] - k_ends[0])
    grid_step = int(per_bin * 0.75)
    if per_bin < 4:                                       # (a grid would cost more than it saves)
        samples = np.arange(lo, hi, dtype=np.int64)
        return _runs_from_samples(samples, unwrapped_bin(phase_at(samples), n_phase))
    grid = np.arange(lo, hi, grid_step, dtype=np.int64)
    if grid[-1] != hi - 1:
        grid = np.append(grid, np.int64(hi - 1))
    value = phase_at(grid)
    whole, frac = phase_parts(value)
    kg = whole * n_phase + np.minimum((frac * n_phase).astype(np.int64), n_phase - 1)
    xg = ((whole - whole[0]) + frac) * n_phase            # continuous bin coordinate (for guesses)
    d = np.diff(kg)
    if np.any(d < 0):
        raise ValueError("phase must increase with time")
    change_n, change_k = [], []
    # intervals where k steps by one: the first sample of the new bin is in (a, b]
    one = np.flatnonzero(d == 1)
    if one.size:
        a, b = grid[one], grid[one + 1]
        target = kg[one + 1]
        # guess from the continuous coordinate, then check m - 1 and m
        x_target = (target - whole[0] * n_phase).astype(float)
        frac_pos = (x_target - xg[one]) / np.maximum(xg[one + 1] - xg[one], 1e-300)
        m = a + np.ceil(np.clip(frac_pos, 0., 1.) * (b - a)).astype(np.int64)
        m = np.clip(m, a + 1, b)
        k_m = unwrapped_bin(phase_at(m), n_phase)
        k_m1 = unwrapped_bin(phase_at(m - 1), n_phase)
        hit = (k_m >= target) & (k_m1 < target)
        # misses: bracket (lo_, hi_] with k(lo_) < target <= k(hi_), then bisect
        lo_ = np.where(k_m < target, m, np.where(k_m1 >= target, a, m - 1))
        hi_ = np.where(k_m < target, b, np.where(k_m1 >= target, m - 1, m))
        lo_ = np.where(hit, m - 1, lo_)
        hi_ = np.where(hit, m, hi_)
        active = hi_ - lo_ > 1
        while np.any(active):
            idx = np.flatnonzero(active)
            mid = (lo_[idx] + hi_[idx]) // 2
            k_mid = unwrapped_bin(phase_at(mid), n_phase)
            up = k_mid >= target[idx]
            hi_[idx] = np.where(up, mid, hi_[idx])
            lo_[idx] = np.where(up, lo_[idx], mid)
            active = hi_ - lo_ > 1
        change_n.append(hi_)
        change_k.append(target)
    # intervals where k steps by more than one: every sample
    many = np.flatnonzero(d > 1)
    if many.size:
        lens = grid[many + 1] - grid[many]
        samples = np.concatenate([np.arange(grid[i] + 1, grid[i + 1] + 1, dtype=np.int64) for i in many])
        ks = unwrapped_bin(phase_at(samples), n_phase)
        prev = np.empty_like(ks)
        prev[1:] = ks[:-1]
        prev[np.concatenate(([0], np.cumsum(lens)[:-1]))] = kg[many]      # (k of each interval's left end)
        step = ks != prev
        change_n.append(samples[step])
        change_k.append(ks[step])
    if change_n:
        cn = np.concatenate(change_n)
        ck = np.concatenate(change_k)
        order = np.argsort(cn, kind='stable')
        cn, ck = cn[order], ck[order]
    else:
        cn = ck = np.zeros(0, np.int64)
    begin = np.concatenate(([lo], cn)).astype(np.int64)
    end = np.concatenate((cn, [hi])).astype(np.int64)
    k = np.concatenate(([kg[0]], ck)).astype(np.int64)
    return begin, end, k


def _csr(slot, begin, end, n_slot, chunk_start):
    order = np.argsort(slot, kind='stable')              # (runs of a slot stay in time order)
    slot = slot[order]
    length = (end - begin)[order]
    slot_ptr = np.zeros(n_slot + 1, np.int64)
    np.cumsum(np.bincount(slot, minlength=n_slot), out=slot_ptr[1:])
    counts = np.bincount(slot, weights=length, minlength=n_slot).astype(np.int64)
    return (slot_ptr, (begin[order] - chunk_start).astype(np.int64),
            (end[order] - chunk_start).astype(np.int64), counts)


def fold_table(row_edges, row_phase, n_phase, c0, c1):
    """Run table of input samples [c0, c1) for rows with edges ``row_edges`` (row ``r``
    covers [row_edges[r], row_edges[r+1]), absolute sample indices) and ``row_phase(r)``
    the phase function of row ``r`` (see `bin_runs`).

    Returns (first row, number of rows, slot_ptr, run_begin, run_end, counts); slots are
    numbered from the first row that meets the chunk.
    """
    row_edges = np.asarray(row_edges, dtype=np.int64)
    r0 = max(int(np.searchsorted(row_edges, c0, side='right')) - 1, 0)
    r1 = min(int(np.searchsorted(row_edges, c1, side='left')), len(row_edges) - 1)
    slots, begins, ends = [], [], []
    for r in range(r0, r1):
        lo, hi = max(c0, int(row_edges[r])), min(c1, int(row_edges[r + 1]))
        if hi <= lo:
            continue
        b, e, k = bin_runs(row_phase(r), n_phase, lo, hi)
        slots.append((r - r0) * n_phase + k % n_phase)
        begins.append(b)
        ends.append(e)
    n_row = max(r1 - r0, 0)
    if not slots:
        z = np.zeros(0, np.int64)
        return r0, n_row, np.zeros(n_row * n_phase + 1, np.int64), z, z, np.zeros(n_row * n_phase, np.int64)
    return (r0, n_row) + _csr(np.concatenate(slots), np.concatenate(begins), np.concatenate(ends),
                              n_row * n_phase, c0)


def piece_rows(row_edges, c0, c1):
    """(first row, one past the last row) of the rows that meet the chunk [c0, c1)."""
    r0 = max(int(np.searchsorted(row_edges, c0, side='right')) - 1, 0)
    r1 = min(int(np.searchsorted(row_edges, c1, side='left')), len(row_edges) - 1)
    return r0, max(r1, r0)


def piece_table(row_edges, row_pieces, n_phase, c0, c1):
    """`fold_table` for a phase given in polynomial pieces, on the host: the bin of every
    sample from `polynomial_bins`, runs where (row, bin) changes.

    ``row_pieces(r, lo, hi)``: the pieces of row ``r`` for its samples [lo, hi) (absolute
    indices), as (m_begin, m_end, coeff, dt0, step, ref_int, ref_frac) with ``m`` counted from
    ``row_edges[r]``.  A row whose unwrapped bin decreases from one run to the next is refused
    (ValueError), as the table kernel refuses it: `plan_pieces` sees the ends of a row only.
    """
    row_edges = np.asarray(row_edges, dtype=np.int64)
    r0, r1 = piece_rows(row_edges, c0, c1)
    slots, begins, ends = [], [], []
    for r in range(r0, r1):
        lo, hi = max(c0, int(row_edges[r])), min(c1, int(row_edges[r + 1]))
        if hi <= lo:
            continue
        n_ref = int(row_edges[r])
        starts, ks, prev = [], [], None
        for (m0, m1, coeff, dt0, step, ref_int, ref_frac) in row_pieces(r, lo, hi):   # (they tile [lo, hi))
            for a in range(m0, m1, PIECE):
                m = np.arange(a, min(m1, a + PIECE), dtype=np.int64)
                k = polynomial_bins(coeff, dt0, step, ref_int, ref_frac, m, n_phase)
                first = np.ones(1, bool) if prev is None else k[:1] != prev
                new = np.concatenate((first, k[1:] != k[:-1]))
                starts.append(m[new] + n_ref)
                ks.append(k[new])
                prev = k[-1]
        b = np.concatenate(starts)
        k = np.concatenate(ks)
        if np.any(k[1:] < k[:-1]):                       # (the table kernel refuses the same phases: status 8)
            raise ValueError("phase must increase with time")
        slots.append((r - r0) * n_phase + k % n_phase)
        begins.append(b)
        ends.append(np.concatenate((b[1:], [hi])).astype(np.int64))
    n_row = r1 - r0
    if not slots:
        z = np.zeros(0, np.int64)
        return r0, n_row, np.zeros(n_row * n_phase + 1, np.int64), z, z, np.zeros(n_row * n_phase, np.int64)
    return (r0, n_row) + _csr(np.concatenate(slots), np.concatenate(begins), np.concatenate(ends),
                              n_row * n_phase, c0)


def plan_pieces(row_edges, row_pieces, n_phase, c0, c1):
    """What the table kernel (`~baseband_tasks_amd.hip.phase_runs`) needs for the chunk [c0, c1):
    the pieces of its rows with sample indices relative to c0, and per row the grid of cycles its
    bins span, from `polynomial_bins` at the first and last sample of each row in the chunk.

    Returns (first row, number of rows, plan); plan is None if no row meets the chunk.
    """
    row_edges = np.asarray(row_edges, dtype=np.int64)
    r0, r1 = piece_rows(row_edges, c0, c1)
    lo, m0, row, dt0, step, ref_int, ref_frac, coeff = [], [], [], [], [], [], [], []
    k0, n_cycle, run_cap = [], [], 0
    for r in range(r0, r1):
        a, b = max(c0, int(row_edges[r])), min(c1, int(row_edges[r + 1]))
        if b <= a:
            k0.append(0)
            n_cycle.append(0)
            continue
        n_ref = int(row_edges[r])
        pieces = row_pieces(r, a, b)
        for (pa, pb, c, d0, st, ri, rf) in pieces:
            lo.append(pa + n_ref - c0)
            m0.append(pa)
            row.append(r - r0)
            dt0.append(d0)
            step.append(st)
            ref_int.append(ri)
            ref_frac.append(rf)
            coeff.append(np.asarray(c, dtype=float))
        first, last = pieces[0], pieces[-1]
        k_first = int(polynomial_bins(first[2], first[3], first[4], first[5], first[6], np.array([first[0]]), n_phase)[0])
        k_last = int(polynomial_bins(last[2], last[3], last[4], last[5], last[6], np.array([last[1] - 1]), n_phase)[0])
        if k_last < k_first:
            raise ValueError("phase must increase with time")
        base = (k_first // n_phase) * n_phase
        k0.append(base)
        n_cycle.append((k_last - base) // n_phase + 1)
        run_cap += min(b - a, k_last - k_first + 1)
    if not lo:
        return r0, r1 - r0, None
    width = max(len(c) for c in coeff)
    plan = dict(lo=np.array(lo + [min(c1, int(row_edges[r1])) - c0], np.int64), m0=np.array(m0, np.int64),
                row=np.array(row, np.int64), dt0=np.array(dt0, float), step=np.array(step, float),
                ref_int=np.array(ref_int, float), ref_frac=np.array(ref_frac, float),
                coeff=np.array([np.concatenate((c, np.zeros(width - len(c)))) for c in coeff], float),
                k0=np.array(k0, np.int64), n_cycle=np.array(n_cycle, np.int64), run_cap=run_cap)
    return r0, r1 - r0, plan


def contiguous_table(edges, c0, c1):
    """Run table for outputs that each sum one contiguous run: output ``k`` covers
    [edges[k], edges[k+1]).  Same return value as `fold_table` (one slot per output)."""
    edges = np.asarray(edges, dtype=np.int64)
    r0 = max(int(np.searchsorted(edges, c0, side='right')) - 1, 0)
    r1 = min(int(np.searchsorted(edges, c1, side='left')), len(edges) - 1)
    n = max(r1 - r0, 0)
    begin = np.clip(edges[r0:r0 + n], c0, c1)
    end = np.clip(edges[r0 + 1:r0 + n + 1], c0, c1)
    keep = end > begin
    slot = np.arange(n, dtype=np.int64)[keep]
    return (r0, n) + _csr(slot, begin[keep], end[keep], n, c0)
