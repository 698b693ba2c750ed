// Fluctuation spectra of 2^15 ... 2^22 points: LongSpectra in periodicity.py; the NumPy yardstick is
// periodicity.long_spectra_samples.  The reference has no such task: the rule is this package's.  All
// index arithmetic is lspec_geo.hpp's; see there for the four-step split n = n1 n2, the pairing of
// columns (2p, 2p + 1) into one complex stream and the scratch S[k1][b][pair].
//
// k_lspec_first  reads c1 columns (b, pair) of the input, transforms them over a (n1 points) in LDS,
//                multiplies by W_n^(b k1) and writes S.
// k_lspec_last   reads rows k1 and n1 - k1 of cp pairs from S, transforms them over b (n2 points) in
//                LDS, and for every bin k <= n / 2 it owns forms A = (Z[k] + conj Z[n-k]) / 2 and B = (Z[k]
//                - conj Z[n-k]) / 2i, the spectra of the two real columns, and writes |A|^2 and |B|^2:
//                mode 0 out = p, mode 1 out = out + p, mode 2 out = (out + p) * scale -- the transforms of
//                a stack are launched in ascending order on one stream, and every out[k][e] belongs to
//                one thread: no atomics, no sum shared between workgroups.
//
// The transform in LDS (lspec_fft) is radix 2 decimation in frequency, in place, two stages fused per
// barrier (a radix-2 stage last if log2 is odd); the value of index k ends at position brev(k).  Its
// twiddles W_len^j come from a table of len / 2 entries made in float64 on the host; W_n^(b k1) is the
// product of two such table entries (the exponent b k1 < n is exact in an int).  No sine is evaluated
// on the device.  Contraction is off: a value depends on its column pair's samples only, never on how
// pairs are grouped into workgroups or launches.
//
// WHY NO ACCESS LEAVES ITS BUFFER.  Pass 1: col = wg c1 + c < n2 P because c1 divides n2 and the grid is
// n2 P / c1; so b < n2, pl < P, and the input float is (a n2 + b) n_elem + e with a n2 + b < n and e = 2 (p0
// + pl) + half < n_elem checked (the zero partner is not read); the scratch cell is k1 n2 P + col < n P.
// Pass 2: h < n1 / 2 from the grid, rows < n1, pl < P checked, so cells (row n2 + b) P + pl < n P; bins k =
// row + n1 k2 <= n / 2 by lspec_writes, columns e < n_elem checked.  LDS: positions < len, columns < c1 or
// 2 cp, and len c1 <= 8192, n2 2 cp <= 8192.  tests/lspec_geo_check.cpp walks all of it on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "lspec_geo.hpp"

namespace bbt {

__device__ __forceinline__ float2 lspec_mul(float2 a, float2 w) {
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// In-place transform of `len` = 2^lg points of each of ncol = 2^lc columns, lds[pos * ncol + col]; tw[j]
// = exp(-2 pi i j / len), j < len / 2.  Ends with a barrier.  nt threads, a multiple of ncol.
__device__ __forceinline__ void lspec_fft(float2* __restrict__ lds, const float2* __restrict__ tw, int lg, int lc,
                                          int tid, int nt) {
#pragma clang fp contract(off)
    const int len = 1 << lg;
    const int col = tid & ((1 << lc) - 1);
    const int step = nt >> lc;
    int lL = lg;                                             // log2 of the block length L of this stage
    for (; lL >= 2; lL -= 2) {
        const int lq = lL - 2, q = 1 << lq, sh = lg - lL;    // the quarter; tw index = j << sh
        for (int idx = tid >> lc; idx < (len >> 2); idx += step) {
            const int j = idx & (q - 1);
            const int base = ((((idx >> lq) << lL) + j) << lc) + col;
            const int d = q << lc;
            const float2 e0 = lds[base], e1 = lds[base + d], e2 = lds[base + 2 * d], e3 = lds[base + 3 * d];
            const float2 w1 = tw[j << sh], w2 = tw[(2 * j) << sh];
            const float2 a0 = make_float2(e0.x + e2.x, e0.y + e2.y);
            const float2 a1 = make_float2(e1.x + e3.x, e1.y + e3.y);
            const float2 a2 = lspec_mul(make_float2(e0.x - e2.x, e0.y - e2.y), w1);
            // W_L^(j + L/4) = -i W_L^j
            const float2 a3 = lspec_mul(make_float2(e1.y - e3.y, -(e1.x - e3.x)), w1);
            lds[base] = make_float2(a0.x + a1.x, a0.y + a1.y);
            lds[base + d] = lspec_mul(make_float2(a0.x - a1.x, a0.y - a1.y), w2);
            lds[base + 2 * d] = make_float2(a2.x + a3.x, a2.y + a3.y);
            lds[base + 3 * d] = lspec_mul(make_float2(a2.x - a3.x, a2.y - a3.y), w2);
        }
        __syncthreads();
    }
    if (lL == 1) {
        for (int idx = tid >> lc; idx < (len >> 1); idx += step) {
            const int base = ((2 * idx) << lc) + col;
            const float2 u = lds[base], v = lds[base + (1 << lc)];
            lds[base] = make_float2(u.x + v.x, u.y + v.y);
            lds[base + (1 << lc)] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BBT_LSPEC_MAX_THREADS) void k_lspec_first(const float* __restrict__ x,
                                                                   float2* __restrict__ scratch,
                                                                   const float2* __restrict__ tw1,
                                                                   const float2* __restrict__ tw_hi,
                                                                   const float2* __restrict__ tw_lo, LspecGeo g) {
#pragma clang fp contract(off)
    __shared__ float2 lds[BBT_LSPEC_LDS_CELLS];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int c = tid & (g.c1 - 1);
    const int step = nt >> g.log2c1;
    LspecCol o;
    lspec_col(g, (long long)blockIdx.x, c, &o);
    for (int a = tid >> g.log2c1; a < g.n1; a += step) {
        const long long i0 = lspec_in_index(g, o, a, 0), i1 = lspec_in_index(g, o, a, 1);
        lds[lspec_lds1(g, a, c)] = make_float2(x[i0], i1 >= 0 ? x[i1] : 0.f);
    }
    __syncthreads();
    lspec_fft(lds, tw1, g.log2n1, g.log2c1, tid, nt);
    for (int k1 = tid >> g.log2c1; k1 < g.n1; k1 += step) {
        const float2 v = lds[lspec_lds1(g, lspec_pos1(g, k1), c)];
        const int m = lspec_tw_exp(g, o.b, k1);
        const float2 w = lspec_mul(tw_hi[m >> BBT_LSPEC_TW_LO_LOG2], tw_lo[m & ((1 << BBT_LSPEC_TW_LO_LOG2) - 1)]);
        scratch[lspec_scratch(g, k1, o.col)] = lspec_mul(v, w);
    }
}

__global__ __launch_bounds__(BBT_LSPEC_MAX_THREADS) void k_lspec_last(const float2* __restrict__ scratch,
                                                                  float* __restrict__ out,
                                                                  const float2* __restrict__ tw2, LspecGeo g,
                                                                  int mode, float scale) {
#pragma clang fp contract(off)
    __shared__ float2 lds[BBT_LSPEC_LDS_CELLS];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int lc = g.log2cp + 1;
    const int col = tid & ((1 << lc) - 1);
    const int ri = col >> g.log2cp, s = col & (g.cp - 1);
    const int step = nt >> lc;
    const long long wg = (long long)blockIdx.x;
    const int h = lspec_h(g, wg);
    const long long pl = lspec_pl0(g, wg) + s;
    const bool valid = pl < g.P;
    const int row = lspec_row(g, h, ri);
    for (int b = tid >> lc; b < g.n2; b += step)
        lds[lspec_lds2(g, b, ri, s)] = valid ? scratch[lspec_scratch(g, row, (long long)b * g.P + pl)]
                                             : make_float2(0.f, 0.f);
    __syncthreads();
    lspec_fft(lds, tw2, g.log2n2, lc, tid, nt);
    if (!valid) return;
    for (int k2 = tid >> lc; k2 <= g.n2 / 2; k2 += step) {
        if (!lspec_writes(g, h, ri, k2)) continue;
        int rj, k2j;
        lspec_partner(g, h, ri, k2, &rj, &k2j);
        const float2 z = lds[lspec_lds2(g, lspec_pos2(g, k2), ri, s)];
        const float2 w = lds[lspec_lds2(g, lspec_pos2(g, k2j), rj, s)];
        const float ar = 0.5f * (z.x + w.x), ai = 0.5f * (z.y - w.y);      // A = (Z[k] + conj Z[n-k]) / 2
        const float br = 0.5f * (z.y + w.y), bi = -0.5f * (z.x - w.x);     // B = (Z[k] - conj Z[n-k]) / 2i
        const float p[2] = {ar * ar + ai * ai, br * br + bi * bi};
        const long long k = lspec_bin(g, h, ri, k2);
        for (int half = 0; half < 2; ++half) {
            const long long at = lspec_out_index(g, k, pl, half);
            if (at < 0) continue;
            if (mode == 0)
                out[at] = p[half];
            else if (mode == 1)
                out[at] = out[at] + p[half];
            else
                out[at] = (out[at] + p[half]) * scale;
        }
    }
}

}  // namespace bbt
