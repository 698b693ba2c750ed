// Run tables for folding, made on the device from polynomial phases (the device twin of
// fold_table.piece_table / fold_table.polynomial_bins).
//
// A chunk of n input samples is tiled by pieces; piece p covers samples [lo[p], lo[p+1]) of the
// chunk, belongs to output row row[p], and gives sample i the phase
//   x = dt0[p] + (m0[p] + (i - lo[p])) * step[p];   phase = ref_int[p] + ref_frac[p] + sum_j c[p][j] x^j
// and the unwrapped bin k = floor(phase) * n_phase + int(frac(phase) * n_phase), evaluated in float64
// with exactly the operations, in exactly the order, of polynomial_bins (every one rounded on its own:
// floating-point contraction is off in phase_bin, so no product is fused into a sum).
//
// A run is a maximal stretch of samples with the same (row, k).  Phase increases with time, so the
// runs of a row have increasing k, and run (row, k) has a cell of its own in a grid laid out slot by
// slot: cell = cell0[row] + bin * n_cycle[row] + cycle, with bin = (k - k0[row]) % n_phase, cycle =
// (k - k0[row]) / n_phase (k0[row]: a multiple of n_phase at or below the row's first k; n_cycle[row]
// the cycles the row spans in the chunk; both from the host, which evaluates k at the ends of the
// rows).  The table is the grid with its empty cells squeezed out:
//   1. k_phase_count:   run starts per tile of samples
//   2. k_scan_tiles:    exclusive scan of the tile counts (one workgroup, LDS scan)
//   3. k_phase_scatter: run g (in time order) -> begin[g], slot[g]; grid[cell] = g + 1
//   4. k_grid_count / k_scan_tiles / k_grid_compact: occupied cells per tile, scan, and run g of
//      an occupied cell goes to position (occupied cells before it): run_begin, run_end (the
//      next run's begin), the slot per position; counts[slot] += length (integer atomics: the sum
//      does not depend on the order)
//   5. k_slot_ptr:      slot_ptr[j] = first position whose slot is >= j (binary search)
// Everything but the counts is a pure function of the arguments (scans and unique cells, no
// atomics); the counts are integer sums.  Status is a sum of bits, and with any of them set nothing is
// compacted or searched: the table is empty, and nothing is written out of bounds.
//   1  more runs than the caller allowed for
//   2  a k outside its row's grid (a phase that ran below the row's first bin or beyond its last)
//   4  two runs in one cell (fewer occupied cells than runs): a (row, k) that came back
//   8  a k below that of the sample before it in the same row (a phase that steps back), whether or not
//      it lands on a cell of its own: fold_table.piece_table refuses exactly these phases
#pragma once
#include <hip/hip_runtime.h>

#define BBT_PHASE_TILE 1024          // samples (cells) per workgroup: 256 threads x 4

namespace bbt {

struct PhasePieces {
    const long long* lo;             // [n_piece + 1] chunk-relative sample edges
    const long long* m0;             // [n_piece] offset of sample lo[p] from its row's start
    const long long* row;            // [n_piece] output row (relative to the first row of the chunk)
    const double* dt0;               // [n_piece]
    const double* step;              // [n_piece]
    const double* ref_int;           // [n_piece]
    const double* ref_frac;          // [n_piece]
    const double* coeff;             // [n_piece][n_coeff]
    int n_piece;
    int n_coeff;
};

// k of sample i of piece p: see polynomial_bins
__device__ __forceinline__ long long phase_bin(const PhasePieces& P, int p, long long i, long long n_phase) {
#pragma clang fp contract(off)
    const double m = (double)(P.m0[p] + (i - P.lo[p]));
    const double mx = m * P.step[p];
    const double x = P.dt0[p] + mx;
    const double* c = P.coeff + (long long)p * P.n_coeff;
    double v = c[P.n_coeff - 1];
    for (int j = P.n_coeff - 2; j >= 0; --j) {
        const double vx = v * x;
        v = vx + c[j];
    }
    const double whole = floor(v);
    const double rest = v - whole;
    double frac = rest + P.ref_frac[p];
    const double carry = floor(frac);
    frac = frac - carry;
    const long long w = (long long)whole + (long long)carry + (long long)P.ref_int[p];
    const double scaled = frac * (double)n_phase;
    long long b = (long long)scaled;
    if (b > n_phase - 1) b = n_phase - 1;
    return w * n_phase + b;
}

// last piece with lo[p] <= i (i inside [lo[0], lo[n_piece]))
__device__ __forceinline__ int phase_piece_of(const PhasePieces& P, long long i) {
    int a = 0, b = P.n_piece;
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (P.lo[mid] <= i) a = mid; else b = mid;
    }
    return a;
}

// The four samples of this thread: k, row and whether each starts a run.  Samples beyond `end`
// start nothing.  (The thread re-evaluates the sample before its first: no exchange needed.)
// Returns whether one of them has a k below that of the sample before it in the same row.
__device__ __forceinline__ bool phase_flags(const PhasePieces& P, long long base, long long begin, long long end,
                                            long long n_phase, long long k[4], int piece[4], bool start[4]) {
    long long k_prev = 0, row_prev = -1;
    int p = 0;
    bool back = false;
    if (base < end) {
        p = phase_piece_of(P, base > begin ? base - 1 : base);
        if (base > begin) {
            k_prev = phase_bin(P, p, base - 1, n_phase);
            row_prev = P.row[p];
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long i = base + t;
        start[t] = false;
        k[t] = 0;
        piece[t] = p;
        if (i >= end) continue;
        while (p + 1 < P.n_piece && P.lo[p + 1] <= i) ++p;
        piece[t] = p;
        k[t] = phase_bin(P, p, i, n_phase);
        const long long r = P.row[p];
        start[t] = r != row_prev || k[t] != k_prev;
        back = back || (r == row_prev && k[t] < k_prev);
        k_prev = k[t];
        row_prev = r;
    }
    return back;
}

__device__ __forceinline__ void phase_status(long long* status, unsigned long long bit) {
    atomicOr((unsigned long long*)status, bit);
}

// Sum of v over the 256 threads of the workgroup, and this thread's exclusive prefix.
__device__ __forceinline__ long long block_scan_256(long long v, long long* lds, long long& total) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const long long add = tid >= d ? lds[tid - d] : 0;
        __syncthreads();
        lds[tid] += add;
        __syncthreads();
    }
    total = lds[255];
    const long long excl = lds[tid] - v;
    __syncthreads();
    return excl;
}

__global__ __launch_bounds__(256) void k_phase_count(PhasePieces P, long long n_phase, long long* tile_count) {
    __shared__ long long lds[256];
    const long long begin = P.lo[0], end = P.lo[P.n_piece];
    const long long base = begin + (long long)blockIdx.x * BBT_PHASE_TILE + threadIdx.x * 4;
    long long k[4];
    int piece[4];
    bool start[4];
    phase_flags(P, base, begin, end, n_phase, k, piece, start);
    long long total;
    block_scan_256((long long)start[0] + start[1] + start[2] + start[3], lds, total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// In place: count[t] -> sum of count[0 .. t-1]; *total = the sum of all; status |= 1 if it exceeds cap.
// With `expect` (the occupied cells against the runs; every run was scattered if neither bit 1 nor
// bit 2 is set): status |= 4 if the sum is not *expect.
__global__ __launch_bounds__(256) void k_scan_tiles(long long* count, long long n, long long* total, long long cap,
                                                    const long long* expect, long long* status) {
    __shared__ long long lds[256];
    long long carry = 0;
    for (long long base = 0; base < n; base += 256) {
        const long long i = base + threadIdx.x;
        const long long v = i < n ? count[i] : 0;
        long long sum;
        const long long excl = block_scan_256(v, lds, sum);
        if (i < n) count[i] = carry + excl;
        carry += sum;
    }
    if (threadIdx.x == 0) {
        *total = carry;
        if (carry > cap) phase_status(status, 1);
        if (expect && carry != *expect && (*status & 3) == 0) phase_status(status, 4);
    }
}

__global__ __launch_bounds__(256) void k_phase_scatter(PhasePieces P, long long n_phase, const long long* tile_off,
                                                       const long long* __restrict__ k0, const long long* __restrict__ n_cycle,
                                                       const long long* __restrict__ cell0, long long n_row, long long n_cell,
                                                       long long slot0, long long run_cap, long long* begin_t,
                                                       long long* slot_t, int* grid, long long* status) {
    __shared__ long long lds[256];
    const long long begin = P.lo[0], end = P.lo[P.n_piece];
    const long long base = begin + (long long)blockIdx.x * BBT_PHASE_TILE + threadIdx.x * 4;
    long long k[4];
    int piece[4];
    bool start[4];
    if (phase_flags(P, base, begin, end, n_phase, k, piece, start)) phase_status(status, 8);
    long long total;
    long long g = tile_off[blockIdx.x] +
                  block_scan_256((long long)start[0] + start[1] + start[2] + start[3], lds, total);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!start[t]) continue;
        const long long r = P.row[piece[t]];
        const bool row_ok = r >= 0 && r < n_row;
        const long long rel = row_ok ? k[t] - k0[r] : -1;
        const long long cyc = rel >= 0 ? rel / n_phase : -1;
        if (g >= run_cap || cyc < 0 || cyc >= n_cycle[r]) {
            phase_status(status, 2);
        } else {
            const long long bin = rel - cyc * n_phase;
            const long long cell = cell0[r] + bin * n_cycle[r] + cyc;
            if (cell >= 0 && cell < n_cell) {
                begin_t[g] = base + t;
                slot_t[g] = slot0 + r * n_phase + bin;
                grid[cell] = (int)(g + 1);
            } else {
                phase_status(status, 2);
            }
        }
        ++g;
    }
}

__global__ __launch_bounds__(256) void k_grid_count(const int* __restrict__ grid, long long n_cell, long long* tile_count) {
    __shared__ long long lds[256];
    const long long base = (long long)blockIdx.x * BBT_PHASE_TILE + threadIdx.x * 4;
    long long v = 0;
    if (base + 3 < n_cell) {
        const int4 q = *(const int4*)(grid + base);           // (the grid is 16-byte aligned)
        v = (q.x != 0) + (q.y != 0) + (q.z != 0) + (q.w != 0);
    } else {
        for (long long i = base; i < n_cell; ++i) v += grid[i] != 0;
    }
    long long total;
    block_scan_256(v, lds, total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_grid_compact(const int* __restrict__ grid, long long n_cell,
                                                      const long long* __restrict__ tile_off,
                                                      const long long* __restrict__ begin_t,
                                                      const long long* __restrict__ slot_t,
                                                      const long long* __restrict__ n_run, long long run_cap,
                                                      const long long* __restrict__ status, long long end,
                                                      long long slot0, long long n_slot_chunk, long long* run_begin,
                                                      long long* run_end, long long* slot_sorted,
                                                      unsigned long long* counts) {
    __shared__ long long lds[256];
    const long long base = (long long)blockIdx.x * BBT_PHASE_TILE + threadIdx.x * 4;
    int q[4] = {0, 0, 0, 0};
    for (int t = 0; t < 4; ++t)
        if (base + t < n_cell) q[t] = grid[base + t];
    long long total;
    long long pos = tile_off[blockIdx.x] +
                    block_scan_256((long long)(q[0] != 0) + (q[1] != 0) + (q[2] != 0) + (q[3] != 0), lds, total);
    const long long R = *n_run;
    if (*status != 0 || R > run_cap) return;
    for (int t = 0; t < 4; ++t) {
        if (q[t] == 0) continue;
        const long long g = (long long)q[t] - 1;
        if (g < R && pos < run_cap) {
            const long long b = begin_t[g];
            const long long e = g + 1 < R ? begin_t[g + 1] : end;
            const long long s = slot_t[g];
            run_begin[pos] = b;
            run_end[pos] = e;
            slot_sorted[pos] = s;
            if (s >= slot0 && s < slot0 + n_slot_chunk) atomicAdd(counts + (s - slot0), (unsigned long long)(e - b));
        }
        ++pos;
    }
}

// slot_ptr[j] for j in [0, n_slot]: the first position whose slot is >= j
__global__ __launch_bounds__(256) void k_slot_ptr(const long long* __restrict__ slot_sorted,
                                                  const long long* __restrict__ n_run, long long run_cap,
                                                  const long long* __restrict__ status, long long n_slot,
                                                  long long* slot_ptr) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j > n_slot) return;
    long long R = *n_run;
    if (*status != 0 || R > run_cap) R = 0;
    long long a = 0, b = R;
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (slot_sorted[mid] < j) a = mid + 1; else b = mid;
    }
    slot_ptr[j] = a;
}

}  // namespace bbt
