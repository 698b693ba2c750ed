// Periodicity search on the stacked fluctuation spectra of the (time, DM) plane: Whiten and
// HarmonicSearch in periodicity.py; the host twins are periodicity.whiten_samples and
// periodicity.harmonic_search_samples.  The reference has no such tasks: the rules are this
// package's.  The tiling is hsum_geo.hpp's.
//
// THE ARITHMETIC IS THE CONTRACT.
//
// Whiten, per (spectrum, block, element), in float64 with contraction off:
//   S1 = sum x in a FIXED TWO-LEVEL ORDER: segments of 32 consecutive bins (the last may be shorter)
//   are each summed in bin order from the block's first bin, and the segment sums are added in
//   segment order from 0.
//   mean = S1 / len; r = 1 / mean; z = x * (float)r  in float32: one rounded multiply;
//   the block is +0 throughout if mean is not finite, not > 0, or (float)r is not finite.
// The divides are the correctly rounded ones (no fast-math anywhere in this library).  The ny
// threads of a column take a segment each per round; the segment sums meet in LDS (two buffers in
// turn: one barrier a round) and thread ty = 0 adds them in segment order.  Then all ny threads
// rewrite the block, which the workgroup has just pulled through cache.  Bins below `skip` are a
// block of their own that is only cleared.
//
// HarmonicSearch, per spectrum and element, ONE float32 accumulator per top harmonic j:
//   T_0[j] = p[j];  T_L[j] = T_{L-1}[j] + p[(j i + 2^(L-1)) >> L] for i = 1, 3, ..., 2^L - 1 in
//   ascending order, one rounded add each;  snr_L[j] = (T_L[j] - (float)2^L) * c_L, one rounded
//   subtract and one rounded multiply, c_L from the plan's table.
// (L, j) is present iff its fundamental's bin -- j for L = 0, (j + 2^(L-1)) >> L otherwise -- is at
// least lo.  The winner of a block is the largest of (snr, -L, -j) among the present, a total order,
// NaN left out: the parts of a block merge theirs through LDS in any order.  A (pair, element) is
// written by one thread: no atomics, no scratch.
//
// WHY NO ACCESS LEAVES THE CHUNK.  A thread reads rows of its own spectrum s < n_spec only, at bins j
// with b n <= j < min((b + 1) n, nbin) and (j i + 2^(L-1)) >> L with i < 2^L, which is at most j and at
// least 0: bins in [0, nbin).  The column is e < n_elem or the thread does nothing.  The winner goes to
// best[s][b][0 ... 2][e], b < nb.  Whiten reads and writes bins j0 ... j0 + len - 1 < nbin of spectrum
// s < n_spec, columns e < n_elem, each block by one workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include "hsum_geo.hpp"

namespace bbt {

__global__ __launch_bounds__(BBT_HSUM_THREADS) void k_hsum_whiten(const float* __restrict__ x,
                                                                  float* __restrict__ out, WhitenGeo g) {
#pragma clang fp contract(off)
    constexpr int NT = BBT_HSUM_THREADS;
    __shared__ double s_s1[2][NT];                   // segment sums of a round: [buffer][tid]
    __shared__ float s_r[NT];                        // per column of the tile
    __shared__ unsigned char s_ok[NT];               // 0: a degenerate block

    const int tid = threadIdx.x;
    const int nx = g.nx, ny = g.ny;
    const int tx = tid % nx, ty = tid / nx;
    WhitenOwn o;
    hsum_whiten_own(g, (long long)blockIdx.x, &o);
    const long long e = o.e0 + tx;
    const bool active = e < g.n_elem;
    const long long n = o.len, pitch = g.n_elem;
    const long long at = active ? (o.s * g.nbin + o.j0) * pitch + e : 0;   // bin j0 of the column
    const float* __restrict__ xin = x + at;
    float* __restrict__ dst = out + at;

    if (o.zero) {                                    // (the whole workgroup: no barrier is skipped by some)
        if (active)
            for (long long t = ty; t < n; t += ny) dst[t * pitch] = 0.f;
        return;
    }

    double tot = 0.;
    const int n_seg = (int)((n + BBT_HSUM_SEG - 1) / BBT_HSUM_SEG);
    const int rounds = (n_seg + ny - 1) / ny;
    for (int r = 0; r < rounds; ++r) {
        const int seg = r * ny + ty;
        double a = 0.;
        if (active && seg < n_seg) {
            const long long t0 = (long long)seg * BBT_HSUM_SEG;
            const int cnt = (int)(n - t0 < BBT_HSUM_SEG ? n - t0 : BBT_HSUM_SEG);
            const float* __restrict__ p = xin + t0 * pitch;
            int i = 0;
            for (; i + 8 <= cnt; i += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = p[(i + u) * pitch];
#pragma unroll
                for (int u = 0; u < 8; ++u) a = a + (double)v[u];
            }
            for (; i < cnt; ++i) a = a + (double)p[i * pitch];
        }
        if (ny == 1) {
            tot = tot + a;
        } else {
            // (buffer r & 1 was last read in round r - 2, before the barrier of round r - 1)
            const int b = r & 1;
            s_s1[b][tid] = a;
            __syncthreads();
            if (active && ty == 0) {
                const int have = n_seg - r * ny < ny ? n_seg - r * ny : ny;
                for (int k = 0; k < have; ++k) tot = tot + s_s1[b][tid + k * nx];
            }
        }
    }

    if (active && ty == 0) {
        const double mean = tot / (double)n;
        const double rd = 1. / mean;
        const float r32 = (float)rd;
        s_r[tx] = r32;
        s_ok[tx] = mean > 0. && mean < __builtin_inf() && r32 < __builtin_inff();     // (false for a NaN)
    }
    __syncthreads();
    if (!active) return;
    const float r32 = s_r[tx];
    const bool ok = s_ok[tx];
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
            dst[s * pitch] = ok ? v[u] * r32 : 0.f;
        }
    }
}

// (s, k, i) beats (bs, bk, bi): larger snr, then the smaller level, then the smaller bin; a NaN never does
__device__ __forceinline__ bool hsum_beats(float s, int k, int i, float bs, int bk, int bi) {
    return s > bs || (s == bs && (k < bk || (k == bk && i < bi)));
}

// T_L[j] from acc = T_{L-1}[j]: the 2^(L-1) rows of the odd harmonics are loaded, then added in ascending i
template <int L>
__device__ __forceinline__ float hsum_level(const float* __restrict__ col, long long pitch, int j, float acc) {
#pragma clang fp contract(off)
    constexpr int H = 1 << (L - 1);
    float v[H];
#pragma unroll
    for (int u = 0; u < H; ++u) v[u] = col[(long long)hsum_bin(j, 2 * u + 1, L) * pitch];
#pragma unroll
    for (int u = 0; u < H; ++u) acc = acc + v[u];
    return acc;
}

// levels 0 ... K - 1 of every top harmonic of a block, the winner into best[s][b][0 ... 2][e]
template <int K>
__global__ __launch_bounds__(BBT_HSUM_THREADS) void k_hsum_search(const float* __restrict__ p,
                                                                  float* __restrict__ best, HsumGeo g) {
#pragma clang fp contract(off)
    constexpr int NT = BBT_HSUM_THREADS;
    __shared__ float s_snr[NT];
    __shared__ int s_k[NT], s_i[NT];

    const int tid = threadIdx.x;
    const int tx = tid % g.nx, ty = tid / g.nx;
    HsumOwn o;
    const bool owned = hsum_own(g, (long long)blockIdx.x, ty, &o);
    const long long e = o.e0 + tx;
    const bool active = owned && e < g.n_elem;
    const long long pitch = g.n_elem;

    float bs = -__builtin_inff();
    int bk = BBT_HSUM_NONE, bi = 0;
    if (active) {
        const float* __restrict__ col = p + o.s * g.nbin * pitch + e;       // bin 0 of the spectrum's column
        const int j0 = (int)(o.b * g.n);
        const int j1 = (int)(g.nbin - j0 < g.n ? g.nbin : j0 + g.n);
        const int lo = (int)g.lo;
        for (int j = j0 + o.q; j < j1; j += g.sub) {
            const int off = j - j0;
            float acc = col[(long long)j * pitch];
#define BBT_HSUM_OFFER(L)                                                                         \
    if (hsum_bin(j, 1, L) >= lo) {                                                                \
        const float d = acc - (float)(1 << (L));                                                  \
        const float snr = d * g.c[L];                                                             \
        if (hsum_beats(snr, L, off, bs, bk, bi)) bs = snr, bk = L, bi = off;                      \
    }
            BBT_HSUM_OFFER(0)
            if constexpr (K > 1) {
                acc = hsum_level<1>(col, pitch, j, acc);
                BBT_HSUM_OFFER(1)
            }
            if constexpr (K > 2) {
                acc = hsum_level<2>(col, pitch, j, acc);
                BBT_HSUM_OFFER(2)
            }
            if constexpr (K > 3) {
                acc = hsum_level<3>(col, pitch, j, acc);
                BBT_HSUM_OFFER(3)
            }
            if constexpr (K > 4) {
                acc = hsum_level<4>(col, pitch, j, acc);
                BBT_HSUM_OFFER(4)
            }
            if constexpr (K > 5) {
                acc = hsum_level<5>(col, pitch, j, acc);
                BBT_HSUM_OFFER(5)
            }
#undef BBT_HSUM_OFFER
        }
    }

    if (g.sub > 1) {
        s_snr[tid] = bs, s_k[tid] = bk, s_i[tid] = bi;
        __syncthreads();
        if (active && o.q == 0) {
            for (int q = 1; q < g.sub; ++q) {
                const int at = tid + q * g.nx;
                if (hsum_beats(s_snr[at], s_k[at], s_i[at], bs, bk, bi)) bs = s_snr[at], bk = s_k[at], bi = s_i[at];
            }
        }
    }
    if (!active || o.q != 0) return;
    if (bk == BBT_HSUM_NONE) bk = 0, bi = 0;                   // (bs is -inf: nothing present that is not NaN)
    float* __restrict__ cell = best + (o.s * g.nb + o.b) * 3 * pitch + e;     // [s][b][0 ... 2][e]
    cell[0] = bs;
    cell[pitch] = (float)bi;
    cell[2 * pitch] = (float)bk;
}

}  // namespace bbt
