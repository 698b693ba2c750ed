// Coding of PSRFITS search-mode rows (OBS_MODE = 'SEARCH': the SUBINT table's DATA, DAT_SCL and
// DAT_OFFS columns; the reference reads and writes fold mode only, so the rule is this package's,
// restated in NumPy by psrfits.encode_search_rows / decode_search_rows).  A row is nsblk samples of
// float32 x[sample][chan][pol] in HBM; the file holds unsigned codes of nbits = 1, 2, 4 or 8 bits
// as bytes[sample][pol][chan * nbits / 8], the first channel of a byte in its most significant
// bits, with one float scale and offset per (pol, chan) of the row.  The tiling is psrsearch_geo.hpp's.
//
// k_psrsearch_encode: ONE WORKGROUP OWNS ct CHANNELS OF ONE ROW, ALL THEIR POLARIZATIONS AND
// SAMPLES.  Pass 1 sums the finite samples of every column in float64 with the lanes along (chan,
// pol): coalesced loads, no atomics.  From 64 columns a row a thread owns a column and adds its
// samples in order, the order of the NumPy twin; below, 256 / w threads share a column and their
// partial sums meet in a fixed tree in LDS.  Pass 2 reads the slab again -- nsblk x w floats the
// workgroup has just pulled through L2 --, codes it with the lanes still along (chan, pol), turns
// (chan, pol) -> (pol, chan) through LDS (a dword per code) and packs 8 / nbits channels a byte;
// a thread stores a dword of codes where the alignment allows (VEC), else a byte.
//
// The arithmetic, per column (float64, contraction off, finite samples only):
//   n, S1 = sum x, S2 = sum x * x;  mean = S1 / n;  var = max(S2 / n - mean * mean, 0);  std = sqrt(var)
//   offs = float(mean - k std);  scl = float((2 k) std / (2^nbits - 1))      (k = nsigma)
//   n = 0 or not scl > 0:  scl = 1, offs = float(mean) (0 when n = 0)
// and per sample (float32, contraction off):
//   code = clip(rint((x - offs) / scl), 0, 2^nbits - 1), a NaN quotient 0;
//   a sample that is not finite takes the code of float(mean) (0 when n = 0).
//
// k_psrsearch_decode: out = ((float)code - zero_off) * scl + offs, three roundings, times the
// channel's weight if weights are given; bytes are read along a polarization's channels, unpacked
// into LDS and stored along (chan, pol).
//
// Index arithmetic is 64-bit across the array.
#pragma once
#include <hip/hip_runtime.h>

#include "psrfits_kernels.hpp"
#include "psrsearch_geo.hpp"

namespace bbt {

__device__ __forceinline__ void pss_scale(double s1, double s2, int n, double k, int levels, float& scl, float& offs,
                                          float& fill) {
#pragma clang fp contract(off)
    if (n == 0) {
        scl = 1.f, offs = 0.f, fill = 0.f;
        return;
    }
    const double dn = (double)n;
    const double mean = s1 / dn;
    const double msq = mean * mean;
    double var = s2 / dn - msq;
    if (!(var > 0.)) var = 0.;
    const double sd = __dsqrt_rn(var);
    const double ks = k * sd;
    offs = (float)(mean - ks);
    const double span = (2. * k) * sd;
    scl = (float)(span / (double)(levels - 1));
    fill = (float)mean;
    if (!(scl > 0.f)) scl = 1.f, offs = fill;
}

template <int NBITS>
__device__ __forceinline__ unsigned pss_code(float x, float scl, float offs) {
#pragma clang fp contract(off)
    const float d = x - offs;
    float v = d / scl;
    v = fminf(fmaxf(rintf(v), 0.f), (float)((1 << NBITS) - 1));       // (fmaxf drops a NaN: code 0)
    return (unsigned)v;
}

__device__ __forceinline__ float pss_decode(unsigned code, float zero_off, float scl, float offs, float w,
                                            bool weighted) {
#pragma clang fp contract(off)
    float t = (float)code - zero_off;
    t = t * scl;
    t = t + offs;
    if (weighted) t = t * w;
    return t;
}

template <int NBITS, bool VEC>
__global__ __launch_bounds__(BBT_PSRSEARCH_THREADS) void k_psrsearch_encode(
    const float* __restrict__ x, unsigned char* __restrict__ codes, float* __restrict__ scl,
    float* __restrict__ offs, int* __restrict__ n_finite, long long nsblk, long long n_chan, long long n_pol,
    double nsigma, PsrSearchGeo g) {
#pragma clang fp contract(off)
    constexpr int NT = BBT_PSRSEARCH_THREADS;
    constexpr int CPB = 8 / NBITS, UNIT = VEC ? 4 * CPB : CPB, UB = UNIT / CPB;
    __shared__ unsigned s_code[BBT_PSRSEARCH_LDS];
    __shared__ double s_s1[NT], s_s2[NT];
    __shared__ int s_cnt[NT];
    __shared__ float s_scl[NT], s_offs[NT];
    __shared__ unsigned s_fill[NT];

    const int tid = threadIdx.x;
    const int npol = (int)n_pol;
    const long long n_col = n_chan * n_pol;
    const long long row = (long long)blockIdx.x / g.n_tile;
    const long long c0 = ((long long)blockIdx.x % g.n_tile) * g.ct;
    const int cte = (int)(n_chan - c0 < g.ct ? n_chan - c0 : g.ct);      // channels, columns of this tile
    const int w = cte * npol, wfull = g.ct * npol;
    const int tx = tid % wfull, ty = tid / wfull;
    const float* __restrict__ xr = x + (row * nsblk) * n_col + c0 * n_pol;

    // 1. count, sum and sum of squares of the finite samples of every column
    double s1 = 0., s2 = 0.;
    int cnt = 0;
    if (ty < g.ny && tx < w) {
#pragma unroll 8
        for (long long s = ty; s < nsblk; s += g.ny) {
            const float v = xr[s * n_col + tx];
            const bool ok = psr_finite(v);
            const double d = ok ? (double)v : 0.;
            s1 += d;
            s2 += d * d;
            cnt += ok ? 1 : 0;
        }
    }
    if (g.ny > 1) {
        s_s1[tid] = s1, s_s2[tid] = s2, s_cnt[tid] = cnt;
        __syncthreads();
        int top = 1;
        while (top < g.ny) top <<= 1;
        for (int s = top >> 1; s > 0; s >>= 1) {
            if (ty < s && ty + s < g.ny) {
                const int j = tid + s * wfull;
                s_s1[tid] += s_s1[j], s_s2[tid] += s_s2[j], s_cnt[tid] += s_cnt[j];
            }
            __syncthreads();
        }
        s1 = s_s1[tid], s2 = s_s2[tid], cnt = s_cnt[tid];
    }
    const int p = tx % npol, c = tx / npol;
    if (tid < w) {                                                       // (ty = 0: the whole column's sums)
        float sc, of, fill;
        pss_scale(s1, s2, cnt, nsigma, 1 << NBITS, sc, of, fill);
        const long long q = row * n_col + (long long)p * n_chan + c0 + c;
        scl[q] = sc, offs[q] = of, n_finite[q] = cnt;
        s_scl[tid] = sc, s_offs[tid] = of, s_fill[tid] = pss_code<NBITS>(fill, sc, of);
    }
    __syncthreads();

    // 2. the codes, ts samples at a time
    const int ny2 = NT / wfull;
    const int at = p * g.pol_pitch + c + (c >> 5);
    const int sp = npol * g.pol_pitch;
    const bool mine = ty < ny2 && tx < w;
    const float sc = mine ? s_scl[tx] : 1.f, of = mine ? s_offs[tx] : 0.f;
    const unsigned fill = mine ? s_fill[tx] : 0u;
    const int units = cte / UNIT, per_sample = npol * units;
    const long long pol_bytes = n_chan / CPB, sample_bytes = n_col / CPB;
    unsigned char* __restrict__ dst = codes + (row * nsblk) * sample_bytes + c0 / CPB;
    for (long long s0 = 0; s0 < nsblk; s0 += g.ts) {
        const int nts = (int)(nsblk - s0 < g.ts ? nsblk - s0 : g.ts);
        if (mine) {
#pragma unroll 4
            for (int t = ty; t < nts; t += ny2) {
                const float v = xr[(s0 + t) * n_col + tx];
                s_code[t * sp + at] = psr_finite(v) ? pss_code<NBITS>(v, sc, of) : fill;
            }
        }
        __syncthreads();
        for (int i = tid; i < nts * per_sample; i += NT) {
            const int u = i % units, r = i / units;
            const int pp = r % npol, t = r / npol;
            const unsigned* __restrict__ src = s_code + t * sp + pp * g.pol_pitch;
            unsigned word = 0;
#pragma unroll
            for (int b = 0; b < UB; ++b) {
                unsigned byte = 0;
#pragma unroll
                for (int k = 0; k < CPB; ++k) {
                    const int cc = u * UNIT + b * CPB + k;
                    byte = (byte << NBITS) | src[cc + (cc >> 5)];
                }
                word |= byte << (8 * b);
            }
            const long long o = (s0 + t) * sample_bytes + pp * pol_bytes + (long long)u * UB;
            if (VEC)                                        // (dst, sample_bytes, pol_bytes, c0 / CPB: multiples of 4)
                *reinterpret_cast<unsigned*>(dst + o) = word;
            else
                dst[o] = (unsigned char)word;
        }
        __syncthreads();
    }
}

template <int NBITS, bool VEC>
__global__ __launch_bounds__(BBT_PSRSEARCH_THREADS) void k_psrsearch_decode(
    const unsigned char* __restrict__ codes, const float* __restrict__ scl, const float* __restrict__ offs,
    const float* __restrict__ wts, float zero_off, float* __restrict__ out, long long nsblk, long long n_chan,
    long long n_pol, PsrSearchGeo g) {
    constexpr int NT = BBT_PSRSEARCH_THREADS;
    constexpr int CPB = 8 / NBITS, UNIT = VEC ? 4 * CPB : CPB, UB = UNIT / CPB;
    __shared__ float s_val[BBT_PSRSEARCH_LDS];
    __shared__ float s_scl[NT], s_offs[NT], s_w[NT];                     // (at pol * ct + chan of the tile)

    const int tid = threadIdx.x;
    const int npol = (int)n_pol;
    const long long n_col = n_chan * n_pol;
    const long long row = (long long)blockIdx.x / g.n_tile;
    const long long c0 = ((long long)blockIdx.x % g.n_tile) * g.ct;
    const int cte = (int)(n_chan - c0 < g.ct ? n_chan - c0 : g.ct);
    const int w = cte * npol, wfull = g.ct * npol;
    const int tx = tid % wfull, ty = tid / wfull;
    const int p = tx % npol, c = tx / npol;
    const bool weighted = wts != nullptr;
    if (tid < w) {
        const long long q = row * n_col + (long long)p * n_chan + c0 + c;
        s_scl[p * g.ct + c] = scl[q], s_offs[p * g.ct + c] = offs[q];
        s_w[p * g.ct + c] = weighted ? wts[row * n_chan + c0 + c] : 1.f;
    }
    __syncthreads();

    const int ny2 = NT / wfull;
    const int at = p * g.pol_pitch + c + (c >> 5);
    const int sp = npol * g.pol_pitch;
    const bool mine = ty < ny2 && tx < w;
    const int units = cte / UNIT, per_sample = npol * units;
    const long long pol_bytes = n_chan / CPB, sample_bytes = n_col / CPB;
    const unsigned char* __restrict__ src = codes + (row * nsblk) * sample_bytes + c0 / CPB;
    float* __restrict__ outr = out + (row * nsblk) * n_col + c0 * n_pol;
    for (long long s0 = 0; s0 < nsblk; s0 += g.ts) {
        const int nts = (int)(nsblk - s0 < g.ts ? nsblk - s0 : g.ts);
        for (int i = tid; i < nts * per_sample; i += NT) {
            const int u = i % units, r = i / units;
            const int pp = r % npol, t = r / npol;
            const long long o = (s0 + t) * sample_bytes + pp * pol_bytes + (long long)u * UB;
            const unsigned word = VEC ? *reinterpret_cast<const unsigned*>(src + o) : (unsigned)src[o];
            float* __restrict__ tile = s_val + t * sp + pp * g.pol_pitch;
#pragma unroll
            for (int b = 0; b < UB; ++b) {
                const unsigned byte = (word >> (8 * b)) & 0xffu;
#pragma unroll
                for (int k = 0; k < CPB; ++k) {
                    const int cc = u * UNIT + b * CPB + k, j = pp * g.ct + cc;
                    const unsigned code = (byte >> (NBITS * (CPB - 1 - k))) & ((1u << NBITS) - 1u);
                    tile[cc + (cc >> 5)] = pss_decode(code, zero_off, s_scl[j], s_offs[j], s_w[j], weighted);
                }
            }
        }
        __syncthreads();
        if (mine) {
#pragma unroll 4
            for (int t = ty; t < nts; t += ny2) outr[(s0 + t) * n_col + tx] = s_val[t * sp + at];
        }
        __syncthreads();
    }
}

}  // namespace bbt
