// Spectral kurtosis of blocks of n samples and the excision of the blocks it condemns
// (SpectralKurtosis and Excise in rfi.py; the host twin is rfi.spectral_kurtosis /
// rfi.excise_samples).  The reference has no such task: the rule is this package's.
//
// The stream is x[block][sample][element], float32 (a power) or complex64 (p = re^2 + im^2); the
// tiling is sk_geo.hpp's: a workgroup owns w adjacent elements of nz blocks, threads (tx, ty, tz).
//
// The arithmetic, per block and element (float64, contraction off):
//   p = (double)re * re + (double)im * im  (both products exact, one rounding)  or  (double)x
//   S1 = sum p, S2 = sum p * p  in a FIXED TWO-LEVEL ORDER: segments of 32 consecutive samples (the
//   last may be shorter) are each summed in sample order from 0, and the segment sums are added
//   in segment order from 0.  Nothing else about the launch enters a value.
//   c = (M Nd + 1) / (M - 1);  t = S1 * S1;  r = S2 / t;  r = M * r;  r = r - 1;  sk = (float)(c * r)
//   flag = !(sk >= lo && sk <= hi)       (a NaN -- an all-zero block, a NaN or Inf sample -- is flagged)
// and the g adjacent elements of a group share the OR of their flags.
//
// Pass 1: ny = 1, a thread walks its columns, segment accumulator and total in registers; ny > 1,
// the ny threads of a column take a segment each per round, the segment sums meet in LDS (two
// buffers in turn: one barrier a round) and thread ty = 0 adds them in segment order.  Eight
// loads are in flight per thread.  The flags go through LDS, where the OR over a group is taken.
// Pass 2 (k_sk_excise) walks the slab again -- the workgroup has just pulled it through cache --
// with the ny threads of a column on consecutive samples: a thread loads an access unless all its
// columns are flagged, zeroes the flagged ones and stores it itself.  No atomics; indices are
// 64-bit across the array.
#pragma once
#include <hip/hip_runtime.h>

#include "sk_geo.hpp"

namespace bbt {

struct SkArgs {
    const void* x;
    void* out;               // excise only
    float* sk;               // [n_block][n_elem] or null (estimate: never null)
    unsigned char* flags;    // [n_block][n_elem / group] or null
    long long n_block, n, n_elem;
    double averaged;
    float lo, hi;
    int group;
};

__device__ __forceinline__ float sk_value(double s1, double s2, double m, double nd) {
#pragma clang fp contract(off)
    const double c = (m * nd + 1.) / (m - 1.);
    const double t = s1 * s1;
    double r = s2 / t;
    r = m * r;
    r = r - 1.;
    return (float)(c * r);
}

// the V powers of one access, added to a1 (sum p) and a2 (sum p * p)
template <bool CPLX, int V, typename vec>
__device__ __forceinline__ void sk_add(const vec& q, double* a1, double* a2) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < V; ++j) {
        double p;
        if constexpr (CPLX) {
            const double re = (double)q[2 * j], im = (double)q[2 * j + 1];
            const double rr = re * re, ii = im * im;
            p = rr + ii;
        } else if constexpr (V == 1) {
            p = (double)q;
        } else {
            p = (double)q[j];
        }
        const double pp = p * p;
        a1[j] = a1[j] + p;
        a2[j] = a2[j] + pp;
    }
}

template <int F> struct sk_vec { using type = float __attribute__((ext_vector_type(F))); };
template <> struct sk_vec<1> { using type = float; };

// CPLX: complex64 elements; V: elements per access; EXCISE: the second pass
template <bool CPLX, int V, bool EXCISE>
__device__ __forceinline__ void sk_tile(const SkArgs& A, const SkGeo& g) {
#pragma clang fp contract(off)
    constexpr int NT = BBT_SK_THREADS;
    constexpr int F = V * (CPLX ? 2 : 1);                    // floats per access
    using vec = typename sk_vec<F>::type;
    __shared__ double s_s1[2][V * NT], s_s2[2][V * NT];      // segment sums of a round: [buffer][j * NT + tid]
    __shared__ unsigned char s_flag[V * NT];                 // [tz * w + column of the tile]
    __shared__ unsigned char s_group[V * NT];                // [tz * (w / group) + group of the tile]

    const int tid = threadIdx.x;
    const int nx = g.nx, ny = g.ny, nz = g.nz;
    const int tx = tid % nx, ty = (tid / nx) % ny, tz = tid / (nx * ny);
    const long long tile = (long long)blockIdx.x % g.n_tile;
    const long long block = ((long long)blockIdx.x / g.n_tile) * nz + tz;
    const long long e0 = tile * g.w;                         // first element of the tile
    const int wt = (int)(A.n_elem - e0 < g.w ? A.n_elem - e0 : g.w);      // its width: a multiple of V and the group
    const bool active = tz < nz && block < A.n_block && tx * V < wt;
    const long long pitch = A.n_elem / V;                    // accesses per sample
    const long long n = A.n;
    const long long at = active ? (block * n) * pitch + e0 / V + tx : 0;   // access of sample 0
    const vec* __restrict__ xin = (const vec*)A.x + at;

    // 1. S1 and S2 of every column, in the two-level order
    double tot1[V], tot2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) tot1[j] = 0., tot2[j] = 0.;
    const int n_seg = (int)((n + BBT_SK_SEG - 1) / BBT_SK_SEG);
    const int rounds = (n_seg + ny - 1) / ny;
    for (int r = 0; r < rounds; ++r) {
        const int seg = r * ny + ty;
        double a1[V], a2[V];
#pragma unroll
        for (int j = 0; j < V; ++j) a1[j] = 0., a2[j] = 0.;
        if (active && seg < n_seg) {
            const long long t0 = (long long)seg * BBT_SK_SEG;
            const int cnt = (int)(n - t0 < BBT_SK_SEG ? n - t0 : BBT_SK_SEG);
            const vec* __restrict__ p = xin + t0 * pitch;
            int i = 0;
            for (; i + 8 <= cnt; i += 8) {
                vec q[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = p[(i + u) * pitch];
#pragma unroll
                for (int u = 0; u < 8; ++u) sk_add<CPLX, V, vec>(q[u], a1, a2);
            }
            for (; i < cnt; ++i) sk_add<CPLX, V, vec>(p[i * pitch], a1, a2);
        }
        if (ny == 1) {
#pragma unroll
            for (int j = 0; j < V; ++j) tot1[j] = tot1[j] + a1[j], tot2[j] = tot2[j] + a2[j];
        } else {
            // (buffer r & 1 was last read in round r - 2, before the barrier of round r - 1)
            const int b = r & 1;
#pragma unroll
            for (int j = 0; j < V; ++j) s_s1[b][j * NT + tid] = a1[j], s_s2[b][j * NT + tid] = a2[j];
            __syncthreads();
            if (active && ty == 0) {
                const int have = n_seg - r * ny < ny ? n_seg - r * ny : ny;
                for (int k = 0; k < have; ++k) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        tot1[j] = tot1[j] + s_s1[b][j * NT + tid + k * nx];
                        tot2[j] = tot2[j] + s_s2[b][j * NT + tid + k * nx];
                    }
                }
            }
        }
    }

    // the estimator and its flag, by the thread that holds the column's sums
    if (active && ty == 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float sk = sk_value(tot1[j], tot2[j], (double)n, A.averaged);
            if (A.sk) A.sk[block * A.n_elem + e0 + tx * V + j] = sk;
            if (EXCISE) s_flag[tz * g.w + tx * V + j] = !(sk >= A.lo && sk <= A.hi);
        }
    }
    if (!EXCISE) return;
    __syncthreads();

    // the OR over every group of the tile
    const int grp = A.group;
    const int ngt = wt / grp, ngw = g.w / grp;               // groups of this tile, of a full one
    const long long n_group = A.n_elem / grp;
    for (int i = tid; i < nz * ngt; i += NT) {
        const int z = i / ngt, gi = i - z * ngt;
        const long long bz = ((long long)blockIdx.x / g.n_tile) * nz + z;
        if (bz >= A.n_block) continue;
        unsigned char f = 0;
        for (int k = 0; k < grp; ++k) f |= s_flag[z * g.w + gi * grp + k];
        s_group[z * ngw + gi] = f;
        if (A.flags) A.flags[bz * n_group + e0 / grp + gi] = f;
    }
    __syncthreads();

    // 2. the rewrite: kept columns as they are, flagged ones +0
    if (!active) return;
    bool keep[V], any = false;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        keep[j] = !s_group[tz * ngw + (tx * V + j) / grp];
        any = any || keep[j];
    }
    vec* __restrict__ out = (vec*)A.out + at;
    for (long long t = ty; t < n; t += 4ll * ny) {
        vec q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long s = t + (long long)u * ny;
            q[u] = (vec)(0.f);
            if (any && s < n) q[u] = xin[s * pitch];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long s = t + (long long)u * ny;
            if (s >= n) break;
            if constexpr (F == 1) {
                if (!keep[0]) q[u] = 0.f;
            } else {
#pragma unroll
                for (int f = 0; f < F; ++f)
                    if (!keep[f / (CPLX ? 2 : 1)]) q[u][f] = 0.f;
            }
            out[s * pitch] = q[u];
        }
    }
}

template <bool CPLX, int V>
__global__ __launch_bounds__(BBT_SK_THREADS) void k_sk_estimate(SkArgs A, SkGeo g) {
    sk_tile<CPLX, V, false>(A, g);
}

template <bool CPLX, int V>
__global__ __launch_bounds__(BBT_SK_THREADS) void k_sk_excise(SkArgs A, SkGeo g) {
    sk_tile<CPLX, V, true>(A, g);
}

}  // namespace bbt
