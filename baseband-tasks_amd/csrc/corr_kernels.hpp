// Correlate (correlation.py): the cross-products x_i conj(x_j), i <= j, of the A inputs of a complex64
// stream, integrated over blocks of n samples.  The reference has no correlator: the rule is this
// package's; the host restatement of the values is correlation.correlate_samples.  The cutting into
// segments, groups, tiles and waves is corr_geo.hpp's.
//
// THE RULE IS THE CONTRACT.  A block is cut into segments of BBT_CORR_SEG samples from its first sample.
// Per segment and baseline four float32 chains run in sample order from +0, one fused multiply-add per
// sample: rr += re_i re_j, ii += im_i im_j, ir += im_i re_j, ri += re_i im_j; then Re = rr + ii and Im = ir - ri,
// one rounded float32 operation each.  The segment values are added in float64 in segment order, divided
// by n in float64 if averaged, and each part is rounded once to float32.  k_corr_gram makes the chains as
// the k-ordered accumulation of v_mfma_f32_32x32x2_f32 (D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), k0 the even
// sample of a pair); k_corr_finish adds the segments.  The chains of G[r][c] and G[c][r] see the same
// factors in the same order, so the imaginary part of an autocorrelation is x - x = +0.
//
// LANE MAPS of the MFMA.  Operands: lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][column l & 31], one
// float each -- the same map for both, so chunk c's register serves as the rows of tile (c, *) and the
// columns of tile (*, c), and a diagonal tile takes one register twice.  Result: register `reg` of lane l
// is row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5), column l & 31.
//
// WHY NO ACCESS LEAVES ITS ARRAY.  corr_geo refuses a piece that is not whole segments, so segment s < n_seg
// lies at samples [off, off + len) of the piece, 0 <= off, off + len <= count (corr_segment).  A lane reads
// float corr_lane() < E W of samples off + t, t < len, only: rows beyond the group's reals and the second
// sample of an odd segment's last pair are zeros that form no address.  A wave whose unit does not exist
// (u >= n_unit) reads and writes nothing.  A cell is written only where corr_cell() names an element e < E and
// a baseline b < B: scratch float corr_scratch_at(s, e, b) + 1 < n_seg E B 2.  k_corr_finish: value v < 2 E B reads
// scratch[s][v], s < n_seg, the carry at v, and writes the blocks [blk0, blk1) that end in the piece, which
// the launcher has checked against the output it was given.
#pragma once
#include <hip/hip_runtime.h>

#include "corr_geo.hpp"

namespace bbt {

typedef float corr_acc __attribute__((ext_vector_type(16)));

// scratch[s][e][b] of every unit of the piece x (its first sample first).  T chunks, T (T + 1) / 2 tiles per wave.
template <int T>
__global__ __launch_bounds__(64 * BBT_CORR_MAX_WAVES) void k_corr_gram(const float* __restrict__ x, float* __restrict__ scratch,
                                                                       CorrGeo g) {
#pragma clang fp contract(off)
    constexpr int NT = T * (T + 1) / 2;
    extern __shared__ float corr_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 31, k = lane >> 5;
    const long long u = (long long)blockIdx.x * g.waves + wave;
    const bool live = u < g.n_unit;
    long long s = 0, grp = 0, blk = 0, m = 0, off = 0, len = 0;
    if (live) {
        s = u / g.n_group, grp = u - s * g.n_group;
        corr_segment(g, s, &blk, &m, &off, &len);
    }
    const long long row = g.E * g.W;                   // floats of a sample
    long long at[T];
    bool fed[T];
#pragma unroll
    for (int c = 0; c < T; ++c) {
        at[c] = live ? corr_lane(g, grp, c, i) : -1;
        fed[c] = at[c] >= 0;
    }
    corr_acc acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    const float* __restrict__ p = x + (off + k) * row;  // this lane's sample of the first pair
    const long long pairs = len / 2;
    long long sp = 0;
    for (; sp + 4 <= pairs; sp += 4) {                  // four pairs' loads in flight before their MFMAs
        float v[4][T];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < T; ++c) v[j][c] = fed[c] ? p[2 * j * row + at[c]] : 0.f;
        p += 8 * row;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int q = 0;
#pragma unroll
            for (int ti = 0; ti < T; ++ti)
#pragma unroll
                for (int tj = ti; tj < T; ++tj, ++q)
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j][ti], v[j][tj], acc[q], 0, 0, 0);
        }
    }
    for (; sp < pairs; ++sp) {
        float v[T];
#pragma unroll
        for (int c = 0; c < T; ++c) v[c] = fed[c] ? p[at[c]] : 0.f;
        p += 2 * row;
        int q = 0;
#pragma unroll
        for (int ti = 0; ti < T; ++ti)
#pragma unroll
            for (int tj = ti; tj < T; ++tj, ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[ti], v[tj], acc[q], 0, 0, 0);
    }
    if (len & 1) {                                      // the last sample alone: zeros in the second k slot
        float v[T];
#pragma unroll
        for (int c = 0; c < T; ++c) v[c] = fed[c] && k == 0 ? p[at[c]] : 0.f;
        int q = 0;
#pragma unroll
        for (int ti = 0; ti < T; ++ti)
#pragma unroll
            for (int tj = ti; tj < T; ++tj, ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[ti], v[tj], acc[q], 0, 0, 0);
    }

    // tile by tile through the wave's 32 x 32 floats of LDS: the four reals of a cell lie in two registers
    // of two lanes
    float* __restrict__ tile = corr_lds + wave * BBT_CORR_TILE_FLOATS;
    int q = 0;
#pragma unroll
    for (int ti = 0; ti < T; ++ti)
#pragma unroll
        for (int tj = ti; tj < T; ++tj, ++q) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * k) * BBT_CORR_TILE_PITCH + i] = acc[q][r];
            __syncthreads();
            if (!live) continue;
            for (int cell = lane; cell < 256; cell += 64) {
                const int il = cell >> 4, jl = cell & 15;
                long long e, b;
                if (!corr_cell(g, grp, ti, tj, il, jl, &e, &b)) continue;
                const float* __restrict__ t0 = tile + 2 * il * BBT_CORR_TILE_PITCH + 2 * jl;
                const float rr = t0[0], ri = t0[1], ir = t0[BBT_CORR_TILE_PITCH], ii = t0[BBT_CORR_TILE_PITCH + 1];
                const long long o = corr_scratch_at(g, s, e, b);
                scratch[o] = rr + ii;
                scratch[o + 1] = ir - ri;
            }
        }
}

// The segments of the piece added per value in float64 in order; out gets the blocks that end in the piece.
// carry[v]: the float64 sum of a block's segments so far, read if the piece begins inside a block, written
// if it ends inside one.
__global__ __launch_bounds__(256) void k_corr_finish(const float* __restrict__ scratch, double* __restrict__ carry,
                                                      float* __restrict__ out, CorrGeo g, long long inner, long long out_blk0,
                                                      int average) {
#pragma clang fp contract(off)
    const long long n_val = 2 * g.E * g.B;
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_val) return;
    const long long part = v & 1, eb = v >> 1, e = eb / g.B, b = eb - e * g.B;
    long long q = g.seg0;                               // the segment's index in its block
    long long blk = g.blk0;
    double sum = q ? carry[v] : 0.;
    const float* __restrict__ p = scratch + v;
    for (long long s = 0; s < g.n_seg;) {
        // the segments of this block that the piece holds: the loads sixteen at a time, the adds in order
        long long run = g.spb - q;
        if (run > g.n_seg - s) run = g.n_seg - s;
        long long k = 0;
        for (; k + 16 <= run; k += 16) {
            float f[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) f[j] = p[(k + j) * n_val];
#pragma unroll
            for (int j = 0; j < 16; ++j) sum += (double)f[j];
        }
        for (; k < run; ++k) sum += (double)p[k * n_val];
        p += run * n_val, s += run, q += run;
        if (q == g.spb) {
            const double value = average ? sum / (double)g.n : sum;
            out[corr_out_at(g, inner, out_blk0, blk, e, b) + part] = (float)value;
            q = 0, ++blk, sum = 0.;
        }
    }
    if (q) carry[v] = sum;
}

}  // namespace bbt
