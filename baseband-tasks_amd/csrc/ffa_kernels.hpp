// Fast-folding period search on the (time, DM) plane: FFASearch in ffa.py; the host twin is
// ffa.ffa_search_samples.  The reference has no such task: the rule is this package's.  The tiling is
// ffa_geo.hpp's.
//
// THE ARITHMETIC IS THE CONTRACT.
//
// Per block of n samples, column and base period p: d[r][j] = x[r p + j], r < m = n / p, and +0 for m <= r <
// M, the power of two with M / 2 < m <= M.  For G = 2, 4, ... M every group of G rows becomes out[t] = A[t >>
// 1] + roll(B[t >> 1], -((t + 1) >> 1)), A and B the transformed halves: one rounded float32 add.  So a
// final row is a FIXED BINARY TREE over its M leaves, and k_ffa_pass<LV>, which folds the 2^LV leaves of LV
// stages pairwise LV times, makes that tree whatever LV is.  A padded leaf is +0 and IS added.
// Boxcars along phase: S_0 = the row, S_{k+1}[j] = S_k[j] + S_k[(j + 2^k) mod p].
// T = the float64 sum of the m p used samples in the two-level order of k_sps_standardize (segments of 32
// samples in sample order, the segment sums in segment order; see k_ffa_segments); c_k = float32((T 2^k) / p); a_k is
// ffa_scale's; snr = (S_k - c_k) * a_k: one rounded float32 subtract, one rounded multiply, no contraction.
// The winner of a (p, column) is the largest of (snr, -t, -k, -j), a total order, NaN left out: threads,
// LDS, the row groups and k_ffa_merge may meet in any order.  A (row group, column) of the partial winners
// and a cell of the result are written by one thread; the launches are ordered by the stream: no atomics.
//
// WHY NO ACCESS LEAVES ITS ARRAY.  A thread of k_ffa_pass owns lane x < lane; a rotated lane is x + c ne with
// c < p, less lane if that is >= lane, so it is in [0, lane).  Pass 0 reads data row r only if r < m, at
// sample r p + j <= m p - 1 < n of column e0 + e < pitch.  Later passes read rows in0 + (u << s0) < M and write
// rows out0 + v < M of buffers of M lane floats.  k_ffa_snr reads rows r0 + r < M and columns ge < ne, and
// writes partial[(rg 4 + f) ne + ge], rg < n_rg <= M, which fits a buffer since 4 <= p.  k_ffa_segments reads
// samples < 32 (n / 32) <= n and writes seg[s ne + e], s < n / 32; k_ffa_prefix walks s <= n / 32 of an array of n /
// 32 + 1 rows; k_ffa_total reads pre[full], full <= n / 32, and samples < m p.
#pragma once
#include <hip/hip_runtime.h>

#include "ffa_geo.hpp"

namespace bbt {

// T is made in three steps, so that the block is read once for all base periods.  k_ffa_segments: seg[s ne + e] =
// the float64 sum of the whole segment s < n / 32 of column e, in sample order from +0.  k_ffa_prefix: in place,
// pre[s ne + e] = the segment sums before s added in segment order from +0, s <= n / 32.  k_ffa_total, per base
// period: T = pre[full] (+ the sum, in sample order from +0, of the cnt samples of the last, shorter segment), with
// m p = 32 full + cnt -- step for step the adds of the two-level order.
__global__ __launch_bounds__(BBT_FFA_THREADS) void k_ffa_segments(const float* __restrict__ x, double* __restrict__ seg,
                                                                  FfaGeo g) {
#pragma clang fp contract(off)
    const long long n_seg = g.n / BBT_FFA_SEG;
    const long long at = (long long)blockIdx.x * BBT_FFA_THREADS + threadIdx.x;      // s ne + e
    if (at >= n_seg * g.ne) return;
    const long long s = at / g.ne, e = at - s * g.ne;
    const float* __restrict__ q = x + s * BBT_FFA_SEG * g.pitch + e;
    double a = 0.;
#pragma unroll 8
    for (int i = 0; i < BBT_FFA_SEG; ++i) a = a + (double)q[i * g.pitch];
    seg[at] = a;
}

__global__ __launch_bounds__(BBT_FFA_THREADS) void k_ffa_prefix(double* __restrict__ pre, FfaGeo g) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * BBT_FFA_THREADS + threadIdx.x;
    if (e >= g.ne) return;
    const long long n_seg = g.n / BBT_FFA_SEG;
    double tot = 0.;
    for (long long s = 0; s < n_seg; ++s) {
        const double a = pre[s * g.ne + e];
        pre[s * g.ne + e] = tot;
        tot = tot + a;
    }
    pre[n_seg * g.ne + e] = tot;
}

// c[k ne + e] = float32((T 2^k) / p), k < K, for the columns e < ne of the launch
__global__ __launch_bounds__(BBT_FFA_THREADS) void k_ffa_total(const float* __restrict__ x, const double* __restrict__ pre,
                                                               float* __restrict__ c, FfaGeo g) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * BBT_FFA_THREADS + threadIdx.x;
    if (e >= g.ne) return;
    const long long used = g.m * g.p;
    const long long full = used / BBT_FFA_SEG;                                       // <= n / 32
    const int cnt = (int)(used - full * BBT_FFA_SEG);
    double tot = pre[full * g.ne + e];
    if (cnt) {
        const float* __restrict__ q = x + full * BBT_FFA_SEG * g.pitch + e;
        double a = 0.;
        for (int i = 0; i < cnt; ++i) a = a + (double)q[i * g.pitch];
        tot = tot + a;
    }
    const double pd = (double)g.p;
    for (int k = 0; k < g.K; ++k) {
        const double scaled = tot * (double)(1 << k);                                // (exact)
        const double q = scaled / pd;
        c[(long long)k * g.ne + e] = (float)q;
    }
}

// LV stages at once: groups of 2^s0 rows of src (the block itself if first) into groups of 2^(s0 + LV) of dst
template <int LV>
__global__ __launch_bounds__(BBT_FFA_THREADS) void k_ffa_pass(const float* __restrict__ src, float* __restrict__ dst,
                                                              FfaGeo g, int s0, int first) {
#pragma clang fp contract(off)
    constexpr int NL = 1 << LV;
    FfaOwn o;
    ffa_own(g, (long long)blockIdx.x, s0, LV, &o);
    const int x = o.x0 + (int)threadIdx.x;
    if (x >= g.lane) return;
    const int lane = g.lane, ne = (int)g.ne, p = (int)g.p;
#pragma unroll
    for (int v = 0; v < NL; ++v) {
        const long long t = (o.tq << LV) + v;
        float w[NL];
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int c = (int)(ffa_leaf_shift(t, u, LV) % p);
            int at = x + c * ne;                                           // (c ne < lane)
            if (at >= lane) at -= lane;
            const long long row = o.in0 + ((long long)u << s0);
            if (first)
                w[u] = row < g.m ? src[ffa_in_at(g, row, at)] : 0.f;
            else
                w[u] = src[row * lane + at];
        }
#pragma unroll
        for (int j = 0; j < LV; ++j) {
#pragma unroll
            for (int u = 0; u < (NL >> (j + 1)); ++u) w[u] = w[2 * u] + w[2 * u + 1];
        }
        dst[(o.out0 + v) * lane + x] = w[0];
    }
}

// (s, t, k, j) beats (bs, bt, bk, bj): larger snr, then the smaller row, level, bin; a NaN never does
__device__ __forceinline__ bool ffa_beats(float s, int t, int k, int j, float bs, int bt, int bk, int bj) {
    return s > bs || (s == bs && (t < bt || (t == bt && (k < bk || (k == bk && j < bj)))));
}

// The boxcar levels and the S/N of nr whole rows of ex columns; the winner of the row group per column into
// part[(rg 4 + f) ne + e], f = snr, row, level, bin; row BBT_FFA_NO_ROW where nothing but NaN was seen.
__global__ __launch_bounds__(BBT_FFA_THREADS) void k_ffa_snr(const float* __restrict__ src, const float* __restrict__ c,
                                                             float* __restrict__ part, FfaGeo g) {
#pragma clang fp contract(off)
    constexpr int NT = BBT_FFA_THREADS;
    __shared__ float s_lv[2][BBT_FFA_CAP];

    const int tid = threadIdx.x;
    const int ex = g.ex, p = (int)g.p;
    const int pe = p * ex;
    const long long tile = (long long)blockIdx.x % g.n_et, rg = (long long)blockIdx.x / g.n_et;
    const long long r0 = rg * g.nr;
    const int rows = (int)(g.M - r0 < g.nr ? g.M - r0 : g.nr);
    const int tot = rows * pe;                                             // <= BBT_FFA_CAP
    const int e = tid % ex;                                                // (ex divides NT: the same for every idx)
    const long long ge = tile * ex + e;
    const bool active = ge < g.ne;

    for (int idx = tid; idx < tot; idx += NT) {
        const int r = idx / pe, rem = idx - r * pe;
        const int j = rem / ex;
        s_lv[0][idx] = active ? src[(r0 + r) * g.lane + (long long)j * g.ne + ge] : 0.f;
    }
    __syncthreads();

    float bs = -__builtin_inff();
    int bt = BBT_FFA_NO_ROW, bk = 0, bj = 0;
    for (int k = 0; k < g.K; ++k) {
        const float* __restrict__ cur = s_lv[k & 1];
        float* __restrict__ nxt = s_lv[(k + 1) & 1];
        const float ck = active ? c[(long long)k * g.ne + ge] : 0.f;
        const float ak = g.a[k];
        const int step = ex << k;                                          // (2^k < p: step < pe)
        const bool more = k + 1 < g.K;
        for (int idx = tid; idx < tot; idx += NT) {
            const int r = idx / pe, rem = idx - r * pe;
            const float v = cur[idx];
            if (active) {
                const float d = v - ck;
                const float snr = d * ak;
                const int t = (int)r0 + r, j = rem / ex;
                if (ffa_beats(snr, t, k, j, bs, bt, bk, bj)) bs = snr, bt = t, bk = k, bj = j;
            }
            if (more) {
                int rem2 = rem + step;
                if (rem2 >= pe) rem2 -= pe;
                nxt[idx] = v + cur[r * pe + rem2];
            }
        }
        __syncthreads();
    }

    // (every level has been read: the buffers are free)
    float* s_s = s_lv[0];
    int* s_i = (int*)s_lv[1];
    s_s[tid] = bs, s_i[tid] = bt, s_i[NT + tid] = bk, s_i[2 * NT + tid] = bj;
    __syncthreads();
    if (tid >= ex || !active) return;
    for (int q = tid + ex; q < NT; q += ex)
        if (ffa_beats(s_s[q], s_i[q], s_i[NT + q], s_i[2 * NT + q], bs, bt, bk, bj))
            bs = s_s[q], bt = s_i[q], bk = s_i[NT + q], bj = s_i[2 * NT + q];
    float* __restrict__ cell = part + rg * 4 * g.ne + ge;
    cell[0] = bs;
    cell[g.ne] = (float)bt;
    cell[2 * g.ne] = (float)bk;
    cell[3 * g.ne] = (float)bj;
}

// best[f][e0 + e] (rows of out_pitch floats) = the winner over the n_rg partial winners of column e < ne.  A
// workgroup owns BBT_FFA_MERGE_NX columns; the 256 / NX threads of a column take the row groups ty, ty + NY, ... and
// meet in LDS: the order is total, so any order of meeting gives the same winner.
__global__ __launch_bounds__(BBT_FFA_THREADS) void k_ffa_merge(const float* __restrict__ part, float* __restrict__ best,
                                                               long long out_pitch, FfaGeo g) {
    constexpr int NT = BBT_FFA_THREADS, NX = BBT_FFA_MERGE_NX, NY = NT / NX;
    __shared__ float s_s[NT];
    __shared__ int s_i[3][NT];
    const int tid = threadIdx.x;
    const int tx = tid % NX, ty = tid / NX;
    const long long e = (long long)blockIdx.x * NX + tx;
    const bool active = e < g.ne;
    float bs = -__builtin_inff();
    int bt = BBT_FFA_NO_ROW, bk = 0, bj = 0;
    if (active) {
        for (long long rg = ty; rg < g.n_rg; rg += NY) {
            const float* __restrict__ cell = part + rg * 4 * g.ne + e;
            const float s = cell[0];
            const int t = (int)cell[g.ne], k = (int)cell[2 * g.ne], j = (int)cell[3 * g.ne];
            if (t != BBT_FFA_NO_ROW && ffa_beats(s, t, k, j, bs, bt, bk, bj)) bs = s, bt = t, bk = k, bj = j;
        }
    }
    s_s[tid] = bs, s_i[0][tid] = bt, s_i[1][tid] = bk, s_i[2][tid] = bj;
    __syncthreads();
    if (ty != 0 || !active) return;
    for (int q = tid + NX; q < NT; q += NX)
        if (s_i[0][q] != BBT_FFA_NO_ROW && ffa_beats(s_s[q], s_i[0][q], s_i[1][q], s_i[2][q], bs, bt, bk, bj))
            bs = s_s[q], bt = s_i[0][q], bk = s_i[1][q], bj = s_i[2][q];
    if (bt == BBT_FFA_NO_ROW) bt = 0, bk = 0, bj = 0;                       // (bs is -inf: nothing but NaN)
    best[e] = bs;
    best[out_pitch + e] = (float)bt;
    best[2 * out_pitch + e] = (float)bk;
    best[3 * out_pitch + e] = (float)bj;
}

}  // namespace bbt
