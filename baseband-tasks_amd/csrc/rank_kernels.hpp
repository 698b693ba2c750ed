// Block median and MAD by selection: RobustStandardize in search.py and MedianWhiten in periodicity.py;
// the host twins are search.block_median_mad_samples, search.robust_standardize_samples and
// periodicity.median_whiten_samples.  The reference has no such tasks: the rules are this package's.
// The tiling, the key map and the step of the descent are rank_geo.hpp's.
//
// THE RULE IS THE CONTRACT.  A median is an exact selection: there is no summation order to pin down.
//
// Order: float32 values are ordered by rank_key of their bits (monotone; -0 just before +0).  The
// median of L values: lo the value of rank (L - 1) / 2, hi of rank L / 2, med = float32((float64(lo) +
// float64(hi)) * 0.5).  A block that holds a NaN or an Inf is flagged.
//   RobustStandardize: d[i] = |x[i] - med| (one rounded float32 subtract, the sign cleared), mad the
//   median of d by the same rule, sd = float64(mad) * 1.482602218505602, r = 1 / sd, z[i] = (x[i] - med)
//   * float32(r): one subtract and one multiply, contraction off.  A flagged block, one whose mad is
//   not > 0 and one whose float32(r) is not finite are +0 throughout.
//   MedianWhiten: mean = float64(med) / ratio, r = 1 / mean, z = x * float32(r); +0 throughout where
//   the block is flagged, mean is not finite or not > 0, or float32(r) is not finite.
// Divide is the correctly rounded one (no fast-math anywhere in this library).
//
// The selection is a most-significant-digit radix select on the keys, digits of 4 or 8 bits.  Per
// digit the ny threads of a column count, with integer LDS atomics, the digit of every value whose key
// matches the prefix fixed so far -- counts are integers, so the order of the adds cannot matter, and
// a 32-bit counter holds the 65536 of a block of equal values -- and every thread of the column then
// walks its column's counters (rank_pick) to the digit that holds the wanted rank: all of them hold
// the prefix and the rank in registers, nothing is broadcast.  The descent is for rank lo; at its end
// the last counter says how many values equal lo, so hi = lo if the rank after lo's is still among
// them, and else hi is the smallest key above lo's: one more pass with an LDS atomicMin, made by the
// whole workgroup whenever L is even.  The MAD is the same descent over |x - med| recomputed on the
// fly.  Barriers are uniform: idle columns (e >= n_elem) count nothing and walk zeros.
//
// WHY NO READ LEAVES THE CHUNK.  A workgroup reads rows row0 + t, t < len, where rank_own gives row0 = s
// nbin + skip + b m and len = min(m, nbin - skip - b m) >= 1 for b < nblk = ceil((nbin - skip) / m): so
// row0 + len <= (s + 1) nbin <= n_spec nbin.  A thread touches column e = e0 + tx only if e < n_elem
// (`active`); an idle thread forms no address.  On the lds route the tile lives at s_x[t * nx + tx], t <
// len <= len_max, and the launcher sized the LDS for len_max rows.  Stores go to the same rows and
// columns of `out`, to rows s nbin + t, t < skip, of the spectrum (from the workgroup of block 0 only),
// and to cell (s nblk + b) n_elem + e of the statistics.  The histogram index is digit * nx + tx with
// digit < 2^BITS, the minima and flags are indexed by tx < nx <= 64.
#pragma once
#include <hip/hip_runtime.h>

#include "rank_geo.hpp"

namespace bbt {

// use(get(t)) for the rows t = ty, ty + ny, ... < len of a thread, the loads of eight rows issued before
// the first is used (on the global route they are what the walk waits for)
template <class Get, class Use>
__device__ __forceinline__ void rank_walk(int len, int ty, int ny, Get get, Use use) {
    constexpr int U = 8;
    for (int t = ty; t < len; t += U * ny) {
        unsigned v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = t + u * ny < len ? get(t + u * ny) : 0u;
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t + u * ny < len) use(v[u]);
    }
}

// The median of the `len` values of a column: x itself (DEV false) or |x - center| (DEV true).
template <int BITS, bool LDS, bool DEV>
__device__ __forceinline__ float rank_median(const float* __restrict__ col, long long pitch, const float* s_col, int nx,
                                             int ny, int tx, int ty, int tid, int len, bool active, float center,
                                             unsigned* s_hist, unsigned* s_min) {
#pragma clang fp contract(off)
    constexpr int NB = 1 << BITS;
    auto key_at = [&](int t) -> unsigned {
        float v = LDS ? s_col[t * nx] : col[(long long)t * pitch];
        if (DEV) v = fabsf(v - center);
        return rank_key(__float_as_uint(v));
    };
    unsigned prefix = 0;
    int k = (len - 1) >> 1, equal = 0;
    for (int shift = 32 - BITS; shift >= 0; shift -= BITS) {
        for (int i = tid; i < NB * nx; i += BBT_RANK_THREADS) s_hist[i] = 0u;
        __syncthreads();
        const unsigned fixed = rank_fixed_mask(shift, BITS);
        if (active)
            rank_walk(len, ty, ny, key_at, [&](unsigned key) {
                if (((key ^ prefix) & fixed) == 0u) atomicAdd(&s_hist[((key >> shift) & (NB - 1)) * nx + tx], 1u);
            });
        __syncthreads();
        const int d = rank_pick(s_hist + tx, NB, nx, &k, &equal);
        prefix |= (unsigned)d << shift;
        __syncthreads();                                   // (the counters are cleared next)
    }
    // prefix is lo's key, `equal` values have it, and lo is the k-th of them
    unsigned hi = prefix;
    if (!(len & 1)) {
        if (tid < nx) s_min[tid] = 0xffffffffu;
        __syncthreads();
        unsigned least = 0xffffffffu;
        if (active)
            rank_walk(len, ty, ny, key_at, [&](unsigned key) {
                if (key > prefix && key < least) least = key;
            });
        if (active) atomicMin(&s_min[tx], least);
        __syncthreads();
        if (k + 1 >= equal) hi = s_min[tx];
    }
    return rank_mid(__uint_as_float(rank_unkey(prefix)), __uint_as_float(rank_unkey(hi)));
}

template <int BITS, bool LDS>
__global__ __launch_bounds__(BBT_RANK_THREADS) void k_rank(const float* __restrict__ x, float* __restrict__ out,
                                                           float* __restrict__ med_out, float* __restrict__ mad_out,
                                                           RankGeo g) {
#pragma clang fp contract(off)
    extern __shared__ unsigned rank_lds[];
    constexpr int NB = 1 << BITS;
    const int nx = g.nx, ny = g.ny;
    unsigned* s_hist = rank_lds;                                   // [NB][nx]
    unsigned* s_min = s_hist + NB * nx;                            // [nx]
    unsigned* s_flag = s_min + 64;                                 // [nx]
    float* s_x = (float*)(s_hist + NB * nx + BBT_RANK_MISC_BYTES / 4);      // [len][nx], the lds route

    const int tid = threadIdx.x;
    const int tx = tid % nx, ty = tid / nx;
    RankOwn o;
    rank_own(g, (long long)blockIdx.x, &o);
    const long long e = o.e0 + tx;
    const bool active = e < g.n_elem;
    const long long pitch = g.n_elem;
    const int len = o.len;
    const float* __restrict__ col = x + (active ? o.row0 * pitch + e : 0);
    const float* s_col = s_x + tx;

    if (tid < nx) s_flag[tid] = 0u;
    __syncthreads();
    unsigned bad = 0u;
    if (active) {
        int t_at = ty;                                             // (rank_walk visits the rows in order)
        rank_walk(len, ty, ny, [&](int t) { return __float_as_uint(col[(long long)t * pitch]); },
                  [&](unsigned bits) {
                      if (LDS) s_x[t_at * nx + tx] = __uint_as_float(bits);
                      t_at += ny;
                      bad |= (unsigned)rank_not_finite(bits);
                  });
    }
    if (bad) atomicOr(&s_flag[tx], 1u);
    // (the first barrier of the descent is between these stores and every read of s_x and s_flag)

    const float med = rank_median<BITS, LDS, false>(col, pitch, s_col, nx, ny, tx, ty, tid, len, active, 0.f, s_hist, s_min);
    float mad = 0.f;
    if (g.mode == BBT_RANK_STANDARDIZE || g.with_mad)
        mad = rank_median<BITS, LDS, true>(col, pitch, s_col, nx, ny, tx, ty, tid, len, active, med, s_hist, s_min);
    if (!active) return;
    const bool flagged = s_flag[tx] != 0u;

    if (g.mode == BBT_RANK_STATS) {
        if (ty == 0) {
            const float nan = __uint_as_float(0x7fc00000u);
            med_out[o.cell * pitch + e] = flagged ? nan : med;
            if (g.with_mad) mad_out[o.cell * pitch + e] = flagged ? nan : mad;
        }
        return;
    }
    float r32;
    bool ok;
    if (g.mode == BBT_RANK_STANDARDIZE) {
        const double sd = (double)mad * BBT_RANK_MAD_SCALE;
        const double r = 1. / sd;
        r32 = (float)r;
        ok = !flagged && mad > 0.f && r32 < __builtin_inff();
    } else {
        const double mean = (double)med / g.ratio;
        const double r = 1. / mean;
        r32 = (float)r;
        ok = !flagged && mean > 0. && mean < __builtin_inf() && r32 > -__builtin_inff() && r32 < __builtin_inff();
        float* __restrict__ z0 = out + o.zero0 * pitch + e;
        for (long long t = ty; t < o.zero_rows; t += ny) z0[t * pitch] = 0.f;
    }
    const float center = g.mode == BBT_RANK_STANDARDIZE ? med : 0.f;
    float* __restrict__ z = out + o.row0 * pitch + e;
    for (int t = ty; t < len; t += ny) {
        float v = 0.f;
        if (ok) {
            const float xv = LDS ? s_col[t * nx] : col[(long long)t * pitch];
            const float d = g.mode == BBT_RANK_STANDARDIZE ? xv - center : xv;
            v = d * r32;
        }
        z[(long long)t * pitch] = v;
    }
}

}  // namespace bbt
