// Acceleration trials: Accelerate in periodicity.py; the host twin is periodicity.accelerate_samples.
// The reference has no such task: the rule is this package's, and accel_geo.hpp holds its only C++
// definition (accel_src) and every index of this kernel.
//
//   out[q n + i][j][e] = in[q n + accel_src(n, k_j, i)][e],   the 32 bits copied.
//
// A workgroup owns tile blockIdx.x -- a run of adjacent output rows inside one block q -- and segment
// blockIdx.y of the row.  Its nx lanes run along the flattened (trial, element) axis of the output row, so
// a row is written as one contiguous run; ny rows are in flight.  A thread works out (j, e) and loads k_j
// once per column it owns and walks down the rows of the tile.
//
// WINDOW = true: if the input rows lo ... hi the tile needs -- one contiguous piece of `in` -- fit the
// LDS the kernel declares, they are staged with coalesced loads and every trial is served from there;
// a tile whose window does not fit reads global memory like WINDOW = false.  The choice is the same for
// every thread of a workgroup (it depends on the geometry and blockIdx only), so the barrier is met by
// all or by none.  Both ways go through the same accel_src: identical bits.
//
// U is unsigned (4 bytes) or uint4 (16 bytes: n_elem % 4 == 0 and both arrays 16-byte aligned; n_elem
// and W then count units of 16).  Integer types, so no bit of a NaN or a -0 can change on the way.
//
// WHY NO ACCESS LEAVES ITS BUFFER.  accel_geo refuses a launch unless the piece covers the window of the
// chunk, and under |k| n <= 1/4 the window of every tile lies inside that (accel_geo.hpp); i0 <= i < i1 are
// rows of the chunk and w < W.  The LDS index is below (hi - lo + 1) n_elem <= lds_units where it is used.
// No atomics, no scratch buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "accel_geo.hpp"

namespace bbt {

template <typename U, bool WINDOW>
__global__ __launch_bounds__(BBT_ACCEL_THREADS) void k_accel(const U* __restrict__ in, U* __restrict__ out,
                                                             const double* __restrict__ factors, AccelGeo g) {
#pragma clang fp contract(off)
    __shared__ U s_win[WINDOW ? BBT_ACCEL_LDS_BYTES / sizeof(U) : 1];

    const int tid = threadIdx.x;
    const int tx = tid & (g.nx - 1), ty = tid >> g.log2nx;
    AccelTile t;
    accel_tile(g, (long long)blockIdx.x, &t);
    long long w0, w1;
    accel_segment(g, (long long)blockIdx.y, &w0, &w1);

    const bool staged = WINDOW && accel_fits(g, t);
    if (staged) {
        const int count = (int)accel_window_units(g, t);
        const U* __restrict__ piece = in + accel_in_index(g, t.q, t.lo, 0);
        for (int u = tid; u < count; u += BBT_ACCEL_THREADS) s_win[u] = piece[u];
        __syncthreads();
    }

    const int n_elem = (int)g.n_elem;
    for (long long w = w0 + tx; w < w1; w += g.nx) {
        const int j = (int)w / n_elem, e = (int)w - j * n_elem;
        const double k = factors[j];
        for (long long i = t.i0 + ty; i < t.i1; i += g.ny) {
            const long long s = accel_src(g.n, k, i);
            const U v = staged ? s_win[accel_lds_index(g, t, s, e)] : in[accel_in_index(g, t.q, s, e)];
            out[accel_out_index(g, t.q, i, w)] = v;
        }
    }
}

}  // namespace bbt
