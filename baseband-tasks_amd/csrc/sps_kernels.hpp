// Single-pulse search on the (time, DM) plane: Standardize and BoxcarSearch in search.py; the host
// twins are search.standardize_samples and search.boxcar_search_samples.  The reference has no such
// tasks: the rules are this package's.  The tiling is sps_geo.hpp's.
//
// THE ARITHMETIC IS THE CONTRACT.
//
// Standardize, per block of n samples and element, in float64 with contraction off:
//   S1 = sum x, S2 = sum x * x (the product of two float32 is exact in float64) in a FIXED TWO-LEVEL
//   ORDER: segments of 32 consecutive samples (the last may be shorter) are each summed in sample
//   order from 0, and the segment sums are added in segment order from 0.
//   mean = S1 / n; q = S2 / n; t = mean * mean; var = q - t; sd = sqrt(var); r = 1 / sd
//   z[i] = (x[i] - (float)mean) * (float)r  in float32: one rounded subtract, one rounded multiply;
//   a block whose var is not finite or not > 0 is +0 throughout.
// Divide and square root are the correctly rounded ones (no fast-math anywhere in this library).
// The ny threads of a column take a segment each per round; the segment sums meet in LDS (two
// buffers in turn: one barrier a round) and thread ty = 0 adds them in segment order.  Then all
// ny threads rewrite the block, which the workgroup has just pulled through cache.
//
// BoxcarSearch: S_0 = x, S_{k+1}[i] = S_k[i] + S_k[i + 2^k] (one rounded float32 add), snr_k[i] =
// S_k[i] * c_k (one rounded multiply).  A window sum is a fixed binary tree over its own samples:
// k_sps_pass<F> reads the 2^F values S_k0[i + m 2^k0] and folds neighbours F times, which IS that
// tree, whatever F is and whichever buffer S_k0 came from.  The winner of a block is the largest
// of (snr, -k, -i), a total order, NaN left out: threads, LDS and the passes may merge it in any
// order.  Between passes the running winner lives in the result itself, with level BBT_SPS_NONE
// where a block has had no value that is not NaN; the last pass turns that into (-inf, 0, 0).  A
// (block, element) is read and written by one thread per pass, and the passes are ordered by the
// stream: no atomics.
//
// WHY NO READ LEAVES THE CHUNK.  A thread walks i from b n + q < n_in - 2^k0 + 1, so i + 2^k0 <= n_in.
// It reads S_k0[i + m 2^k0], m < 2^F, only if i + (m + 1) 2^k0 <= n_in, i.e. row i + m 2^k0 <= n_in -
// 2^k0 < n_in: inside the chunk, and inside what the pass before stored, which was every row j with j +
// 2^k0 <= n_in (it walks the blocks up to ceil(n_in / n), halo and tail included).  The column is e < n_elem
// or the thread does nothing.  A level k0 + j of start time i is used -- for the winner, or stored --
// only if i + 2^(k0 + j) <= n_in, which is exactly when all the leaves it was folded from were read; the
// others are folded from zeros and dropped.  Stores go to row i < n_in of a scratch of n_in rows, and to
// block b < nb of the result.  Standardize reads and writes rows b n + t, t < n, b < n_block, of columns
// e < n_elem only.
#pragma once
#include <hip/hip_runtime.h>

#include "sps_geo.hpp"

namespace bbt {

__global__ __launch_bounds__(BBT_SPS_THREADS) void k_sps_standardize(const float* __restrict__ x,
                                                                     float* __restrict__ out, StdGeo g) {
#pragma clang fp contract(off)
    constexpr int NT = BBT_SPS_THREADS;
    __shared__ double s_s1[2][NT], s_s2[2][NT];      // segment sums of a round: [buffer][tid]
    __shared__ float s_mean[NT], s_rsd[NT];          // per column of the tile
    __shared__ unsigned char s_ok[NT];               // 0: a degenerate block

    const int tid = threadIdx.x;
    const int nx = g.nx, ny = g.ny;
    const int tx = tid % nx, ty = tid / nx;
    const long long tile = (long long)blockIdx.x % g.n_tile;
    const long long block = (long long)blockIdx.x / g.n_tile;
    const long long e = tile * nx + tx;
    const bool active = e < g.n_elem;
    const long long n = g.n, pitch = g.n_elem;
    const long long at = active ? block * n * pitch + e : 0;               // sample 0 of the column
    const float* __restrict__ xin = x + at;

    double tot1 = 0., tot2 = 0.;
    const int n_seg = (int)((n + BBT_SPS_SEG - 1) / BBT_SPS_SEG);
    const int rounds = (n_seg + ny - 1) / ny;
    for (int r = 0; r < rounds; ++r) {
        const int seg = r * ny + ty;
        double a1 = 0., a2 = 0.;
        if (active && seg < n_seg) {
            const long long t0 = (long long)seg * BBT_SPS_SEG;
            const int cnt = (int)(n - t0 < BBT_SPS_SEG ? n - t0 : BBT_SPS_SEG);
            const float* __restrict__ p = xin + t0 * pitch;
            int i = 0;
            for (; i + 8 <= cnt; i += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = p[(i + u) * pitch];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double d = (double)v[u];
                    const double dd = d * d;
                    a1 = a1 + d;
                    a2 = a2 + dd;
                }
            }
            for (; i < cnt; ++i) {
                const double d = (double)p[i * pitch];
                const double dd = d * d;
                a1 = a1 + d;
                a2 = a2 + dd;
            }
        }
        if (ny == 1) {
            tot1 = tot1 + a1, tot2 = tot2 + a2;
        } else {
            // (buffer r & 1 was last read in round r - 2, before the barrier of round r - 1)
            const int b = r & 1;
            s_s1[b][tid] = a1, s_s2[b][tid] = a2;
            __syncthreads();
            if (active && ty == 0) {
                const int have = n_seg - r * ny < ny ? n_seg - r * ny : ny;
                for (int k = 0; k < have; ++k) {
                    tot1 = tot1 + s_s1[b][tid + k * nx];
                    tot2 = tot2 + s_s2[b][tid + k * nx];
                }
            }
        }
    }

    if (active && ty == 0) {
        const double m = (double)n;
        const double mean = tot1 / m;
        const double q = tot2 / m;
        const double t = mean * mean;
        const double var = q - t;
        const double sd = sqrt(var);
        const double rs = 1. / sd;
        s_mean[tx] = (float)mean;
        s_rsd[tx] = (float)rs;
        s_ok[tx] = var > 0. && var < __builtin_inf();                       // (false for a NaN)
    }
    __syncthreads();
    if (!active) return;
    const float m32 = s_mean[tx], r32 = s_rsd[tx];
    const bool ok = s_ok[tx];
    float* __restrict__ o = out + at;
    for (long long t = ty; t < n; t += 4ll * ny) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long s = t + (long long)u * ny;
            v[u] = 0.f;
            if (ok && s < n) v[u] = xin[s * pitch];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long s = t + (long long)u * ny;
            if (s >= n) break;
            const float d = v[u] - m32;
            o[s * pitch] = ok ? d * r32 : 0.f;
        }
    }
}

// (s, k, i) beats (bs, bk, bi): larger snr, then the smaller level, then the smaller start; a NaN never does
__device__ __forceinline__ bool sps_beats(float s, int k, int i, float bs, int bk, int bi) {
    return s > bs || (s == bs && (k < bk || (k == bk && i < bi)));
}

// One pass: levels k0 ... k0 + F - 1 from src = S_k0 (rows of n_elem floats), S_{k0 + F} into dst where
// store is set.  first: the result holds no running winner yet; last: it is finished here.
template <int F>
__global__ __launch_bounds__(BBT_SPS_THREADS) void k_sps_pass(const float* __restrict__ src, float* __restrict__ dst,
                                                              float* __restrict__ best, SpsGeo g, int k0,
                                                              long long blocks, int store, int first, int last,
                                                              float c0, float c1, float c2) {
#pragma clang fp contract(off)
    constexpr int NT = BBT_SPS_THREADS;
    constexpr int M = 1 << F;
    __shared__ float s_snr[NT];
    __shared__ int s_k[NT], s_i[NT];

    const int tid = threadIdx.x;
    const int tx = tid % g.nx, ty = tid / g.nx;
    SpsOwn o;
    const bool owned = sps_own(g, (long long)blockIdx.x, ty, blocks, &o);
    const long long e = o.e0 + tx;
    const bool active = owned && e < g.n_elem;
    const bool scored = active && o.b < g.nb;                  // (a block of the result: it has a winner)
    const long long w = 1ll << k0;
    const long long n_in = g.n_in, pitch = g.n_elem;
    const int levels = g.K - k0 < F ? g.K - k0 : F;

    float bs = -__builtin_inff();
    int bk = BBT_SPS_NONE, bi = 0;
    if (active) {
        const long long t0 = o.b * g.n;
        long long t1 = t0 + g.n;
        if (t1 > n_in - w + 1) t1 = n_in - w + 1;              // i + 2^k0 <= n_in
        const float* __restrict__ col = src + e;
        for (long long i = t0 + o.q; i < t1; i += g.sub) {
            float v[M];
#pragma unroll
            for (int m = 0; m < M; ++m) {
                v[m] = 0.f;
                if (i + (m + 1) * w <= n_in) v[m] = col[(i + m * w) * pitch];
            }
#pragma unroll
            for (int j = 0; j < F; ++j) {
                // v[0] is S_{k0 + j}[i] if that is defined
                if (scored && j < levels && i + (w << j) <= n_in) {
                    const float snr = v[0] * (j == 0 ? c0 : j == 1 ? c1 : c2);     // c_{k0 + j}
                    const int off = (int)(i - t0);
                    if (sps_beats(snr, k0 + j, off, bs, bk, bi)) bs = snr, bk = k0 + j, bi = off;
                }
#pragma unroll
                for (int m = 0; m < (M >> (j + 1)); ++m) v[m] = v[2 * m] + v[2 * m + 1];
            }
            if (store && i + (w << F) <= n_in) dst[i * pitch + e] = v[0];
        }
    }

    if (g.sub > 1) {
        s_snr[tid] = bs, s_k[tid] = bk, s_i[tid] = bi;
        __syncthreads();
        if (scored && o.q == 0) {
            for (int q = 1; q < g.sub; ++q) {
                const int at = tid + q * g.nx;
                if (sps_beats(s_snr[at], s_k[at], s_i[at], bs, bk, bi)) bs = s_snr[at], bk = s_k[at], bi = s_i[at];
            }
        }
    }
    if (!scored || o.q != 0) return;
    float* __restrict__ cell = best + o.b * 3 * pitch + e;     // [b][0 ... 2][e]
    if (!first) {
        const float rs = cell[0];
        const int ri = (int)cell[pitch], rk = (int)cell[2 * pitch];
        if (!sps_beats(bs, bk, bi, rs, rk, ri)) bs = rs, bk = rk, bi = ri;
    }
    if (last && bk == BBT_SPS_NONE) bk = 0, bi = 0;            // (bs is -inf: nothing but NaN in the block)
    cell[0] = bs;
    cell[pitch] = (float)bi;
    cell[2 * pitch] = (float)bk;
}

}  // namespace bbt
