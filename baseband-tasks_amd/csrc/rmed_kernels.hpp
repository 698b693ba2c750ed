// Sliding-median baseline: RunningMedian and Detrend in search.py; the host twins are
// search.running_median_samples and search.detrend_samples.  The reference has no such tasks: the rule
// is this package's.  The tiling, the rows a call needs, the interpolation's integers and the two
// selection methods are rmed_geo.hpp's; the order of the values and the median are rank_geo.hpp's.
//
// THE RULE IS THE CONTRACT.  S = scrunch, w = width, h = w / 2, R = N / S; everything per element.
//   1. c[r] = x[r] (the 32 bits) for S = 1; else float32(T / S), T the float64 sum of x[r S ... r S + S - 1],
//      segments of 32 summed in order, the segment sums added in order.  Row r is bad if one of its
//      samples is a NaN or an Inf (rank_not_finite).
//   2. m[r] = rank_mid(lo, hi) of the window c[max(0, r - h) ... min(R - 1, r + h)], lo of rank (L - 1) / 2 and
//      hi of rank L / 2 in the order rank_key; flagged if the window holds a bad row.
//   3. sample i: (r0, q) = rmed_lerp(i); b = m[r0] if q <= 0, m[r0 + 1] if q >= 2 S, else m[r0] + (m[r0 + 1] -
//      m[r0]) * float32(float64(q) / float64(2 S)): three float32 operations, contraction off; flagged if an
//      m it used is.
//   4. RunningMedian: b; Detrend: x[i] - b, one rounded float32 subtract; +0 where flagged.
// A selection has no summation order and steps 1 and 3 fix theirs: no bit depends on the tiling, the
// method, the chunking.
//
// THE FLAGS TRAVEL IN THE VALUES.  The float64 sum of S <= 4096 finite float32 is finite and T / S is no
// larger than the largest of them, so float32(T / S) is finite; a bad row's sum is not.  k_rmed_scrunch
// writes the quiet NaN 0x7fc00000 for a bad row all the same, and k_rmed_select writes it for a flagged
// median (rank_mid of two finite values is finite): "bad" and "flagged" are rank_not_finite of the
// scratch value, and no value of a flagged window or sample is ever used.
//
// WHY NO ACCESS LEAVES ITS ARRAY.  rmed_geo refuses a call whose input does not hold scrunch rows [c0, c1)
// whole.  k_rmed_scrunch: thread idx < (c1 - c0) n_elem reads x rows (c0 + r) S + s, s < S, of the input and
// writes c[idx].  k_rmed_select: workgroup wg stages rows [st0, st0 + n_st) with c0 <= max(0, m0 - h) <= st0
// and st0 + n_st <= min(R, m1 + h) = c1 (rmed_own), n_st <= run + 2 h rows of LDS, which the launcher sized;
// a thread touches column e = e0 + tx only if e < n_elem and forms no address otherwise.  The window of
// median r is rows [max(0, r - h), min(R, r + h + 1)) of these, row0 <= r < row0 + len.  It writes m[r - m0] or,
// for S = 1 where m0 = ro0 and m1 = ro1, output row r - ro0.  k_rmed_apply: thread idx < n_out n_elem reads x
// [idx], m[r0 - m0] and, only where q > 0, m[r0 + 1 - m0]: max(0, ro - 1) <= r0 and r0 + 1 <= min(R - 1, ro + 1) < m1.
#pragma once
#include <hip/hip_runtime.h>

#include "rmed_geo.hpp"

namespace bbt {

#define BBT_RMED_NAN 0x7fc00000u

// c[r][e] for the rows r < n_c of x[r S + s][e] (x and c begin at the same scrunch row)
__global__ __launch_bounds__(BBT_RMED_THREADS) void k_rmed_scrunch(const float* __restrict__ x, unsigned* __restrict__ c,
                                                                   long long n_c, long long n_elem, int S) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * BBT_RMED_THREADS + threadIdx.x;
    if (idx >= n_c * n_elem) return;
    const long long r = idx / n_elem, e = idx - r * n_elem;
    const float* __restrict__ p = x + r * S * n_elem + e;
    double total = 0.;
    unsigned bad = 0u;
    for (int s0 = 0; s0 < S; s0 += BBT_RMED_SEG) {
        const int s1 = s0 + BBT_RMED_SEG < S ? s0 + BBT_RMED_SEG : S;
        double a = 0.;
        for (int s = s0; s < s1; ++s) {
            const float v = p[(long long)s * n_elem];
            bad |= (unsigned)rank_not_finite(__float_as_uint(v));
            a += (double)v;
        }
        total += a;
    }
    c[idx] = bad ? BBT_RMED_NAN : __float_as_uint((float)(total / (double)S));
}

// The medians of a run.  c: scrunch rows from row c_row0 of the stream on (x itself for S = 1).  FUSED (S =
// 1): out is the output of the call, row ro0 first, and gets b or x - b; else out is m, row m0 first.
template <bool FUSED>
__global__ __launch_bounds__(BBT_RMED_THREADS) void k_rmed_select(const unsigned* __restrict__ c, long long c_row0,
                                                                  float* __restrict__ out, RmedGeo g) {
#pragma clang fp contract(off)
    extern __shared__ unsigned rmed_lds[];
    const int nx = g.nx, ny = g.ny;
    const int tid = threadIdx.x;
    const int tx = tid % nx, ty = tid / nx;
    RmedOwn o;
    rmed_own(g, (long long)blockIdx.x, &o);
    const long long e = o.e0 + tx;
    const bool active = e < g.n_elem;
    const long long pitch = g.n_elem;
    if (active) {
        const unsigned* __restrict__ col = c + (o.st0 - c_row0) * pitch + e;
        for (int t = ty; t < o.n_st; t += ny) rmed_lds[t * nx + tx] = rank_key(col[(long long)t * pitch]);
    }
    __syncthreads();
    if (!active) return;
    const unsigned* s_col = rmed_lds + tx;
    auto key_at = [&](int t) -> unsigned { return s_col[t * nx]; };
    auto bad_at = [&](int t) -> int { return (int)rank_not_finite(rank_unkey(s_col[t * nx])); };

    const int h = (int)g.h, w = (int)g.w;
    const int i0 = ty * o.per, i1 = i0 + o.per < o.len ? i0 + o.per : o.len;
    float* __restrict__ dst = out + (o.row0 - (FUSED ? g.ro0 : g.m0)) * pitch + e;
    unsigned key = 0u;
    int pos = 0, nbad = 0;
    bool full_before = false;
    for (int i = i0; i < i1; ++i) {
        const long long r = o.row0 + i;
        const int a = (int)((r - h < 0 ? 0 : r - h) - o.st0);
        const int b = (int)((r + h + 1 > g.R ? g.R : r + h + 1) - o.st0);
        const bool full = b - a == w;
        unsigned lo, hi;
        if (full && full_before && g.method == BBT_RMED_SELECT_WALK) {
            nbad += bad_at(b - 1) - bad_at(a - 1);
            rmed_step(key_at, a - 1, b - 1, &key, &pos);
            lo = hi = key;
        } else {
            rmed_select(key_at, a, b, &lo, &hi, &pos);
            key = lo;
            nbad = 0;
            for (int t = a; t < b; ++t) nbad += bad_at(t);
        }
        full_before = full;
        const float med = rank_mid(__uint_as_float(rank_unkey(lo)), __uint_as_float(rank_unkey(hi)));
        float v;
        if (FUSED) {
            const float xv = __uint_as_float(rank_unkey(key_at((int)(r - o.st0))));
            v = nbad ? 0.f : (g.mode == BBT_RMED_DETREND ? xv - med : med);
        } else {
            v = nbad ? __uint_as_float(BBT_RMED_NAN) : med;
        }
        dst[(long long)i * pitch] = v;
    }
}

// S > 1: the output samples from x (the call's first output sample first) and m (row m0 first)
__global__ __launch_bounds__(BBT_RMED_THREADS) void k_rmed_apply(const float* __restrict__ x, const unsigned* __restrict__ m,
                                                                 float* __restrict__ out, RmedGeo g) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * BBT_RMED_THREADS + threadIdx.x;
    if (idx >= g.n_out * g.n_elem) return;
    const long long il = idx / g.n_elem, e = idx - il * g.n_elem;
    long long r0, q;
    rmed_lerp(g.out_first + il, g.S, g.R, &r0, &q);
    const unsigned* __restrict__ col = m + (r0 - g.m0) * g.n_elem + e;
    const unsigned lo_bits = col[0];
    float b;
    bool flagged;
    if (q <= 0) {
        b = __uint_as_float(lo_bits), flagged = rank_not_finite(lo_bits);
    } else {
        const unsigned hi_bits = col[g.n_elem];
        if (q >= 2 * g.S) {
            b = __uint_as_float(hi_bits), flagged = rank_not_finite(hi_bits);
        } else {
            const float lo = __uint_as_float(lo_bits), hi = __uint_as_float(hi_bits);
            const float f = (float)((double)q / (double)(2 * g.S));
            const float d = hi - lo;
            const float p = d * f;
            b = lo + p;
            flagged = rank_not_finite(lo_bits) || rank_not_finite(hi_bits);
        }
    }
    float v = 0.f;
    if (!flagged) v = g.mode == BBT_RMED_DETREND ? x[idx] - b : b;
    out[idx] = v;
}

}  // namespace bbt
