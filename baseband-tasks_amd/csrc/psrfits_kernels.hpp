// Coding of PSRFITS fold-mode rows (the SUBINT table's DATA, DAT_SCL and DAT_OFFS columns; reference
// io/psrfits/hdu.py:457-474 reads them, its writer stores unscaled floats: core.py "FIXME add
// scaling").  A folded row is float32 x[n_bin][n_chan][n_pol] in HBM; the file holds big-endian
// int16 codes[n_pol][n_chan][n_bin] with one float scale and offset per (pol, chan).  Both kernels
// turn an n_bin x (n_chan * n_pol) matrix per row, with the minor index permuted
// m = chan * n_pol + pol  <->  q = pol * n_chan + chan.
//
// k_psrfits_encode: ONE WORKGROUP OWNS TC COLUMNS OF ONE ROW, ALL THEIR BINS.  It reads the columns
// once to reduce (per thread min / max / count over its bins, then a tree over the workgroup in
// LDS: no atomics, min and max do not depend on the order, the count is an integer sum), makes
// scale and offset, and reads its slab again -- n_bin x TC floats it has just pulled through L2 --
// to code it, tile by tile of TB bins: codes go to LDS as big-endian pairs (two bins of a column
// in one dword, column pitch TB / 2 + 1 dwords: the writes of a half-wave fall on 32 banks, the
// reads run along a column) and leave as 4-byte stores along the bins.
//
// The arithmetic, in float32 with contraction off (the NumPy encoder must give the same bytes):
//   mn, mx  over the finite bins;  offs = 0.5 mn + 0.5 mx;  half = 0.5 mx - 0.5 mn;
//   scl = half / 32767, 1 if that is not > 0;  code = clip(rint((x - offs) / scl), -32767, 32767),
//   0 for a bin that is not finite;  no finite bin: offs = 0, scl = 1.
//
// k_psrfits_decode: out = ((float)code - zero_off) * scl + offs, three roundings (psrchive's
// read-out), times the channel's weight if weights are given.  Codes are read along the bins in
// pairs, turned through LDS (column pitch TB + 1 floats) and stored along (chan, pol).
//
// VEC: 16-byte loads / stores of floats (x / out 16-byte aligned, n_chan * n_pol a multiple of 4)
// and 4-byte accesses of code pairs (codes 4-byte aligned, n_bin even); otherwise scalar accesses.
// Which instantiation runs and the shape of its tile are psrfits_geo.hpp's.
// Index arithmetic is 64-bit across the array.
#pragma once
#include <hip/hip_runtime.h>

#include "psrfits_geo.hpp"

namespace bbt {

__device__ __forceinline__ bool psr_finite(float x) {
    return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}

__device__ __forceinline__ void psr_scale(float mn, float mx, int cnt, float& scl, float& offs) {
#pragma clang fp contract(off)
    if (cnt == 0) {
        scl = 1.f;
        offs = 0.f;
        return;
    }
    const float a = 0.5f * mn, b = 0.5f * mx;
    offs = a + b;
    const float half = b - a;
    scl = half / 32767.0f;
    if (!(scl > 0.f)) scl = 1.f;
}

// the code of one bin as the file's two bytes (big-endian) in the low half of the result
__device__ __forceinline__ unsigned psr_code(float x, float scl, float offs) {
#pragma clang fp contract(off)
    if (!psr_finite(x)) return 0u;
    const float d = x - offs;
    float v = d / scl;
    v = fminf(fmaxf(rintf(v), -32767.f), 32767.f);
    const unsigned c = (unsigned)(int)v & 0xffffu;
    return ((c & 0xffu) << 8) | (c >> 8);
}

__device__ __forceinline__ float psr_decode(unsigned be, float zero_off, float scl, float offs, float w,
                                            bool weighted) {
#pragma clang fp contract(off)
    const short code = (short)(((be & 0xffu) << 8) | ((be >> 8) & 0xffu));
    float t = (float)code - zero_off;
    t = t * scl;
    t = t + offs;
    if (weighted) t = t * w;
    return t;
}

template <int CPT>
__device__ __forceinline__ void psr_load(const float* __restrict__ p, long long mc, long long n_col, float (&v)[CPT]) {
    if (CPT == 4) {                        // (n_col is a multiple of 4: the four are inside or outside together)
        if (mc < n_col) {
            const float4 f = *reinterpret_cast<const float4*>(p + mc);
            v[0] = f.x, v[CPT > 1 ? 1 : 0] = f.y, v[CPT > 2 ? 2 : 0] = f.z, v[CPT - 1] = f.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            if (mc + k < n_col) v[k] = p[mc + k];
    }
}

template <int TC, bool VEC>
__global__ __launch_bounds__(BBT_PSRFITS_THREADS) void k_psrfits_encode(
    const float* __restrict__ x, unsigned short* __restrict__ codes, float* __restrict__ scl,
    float* __restrict__ offs, int* __restrict__ n_finite, long long n_bin, long long n_chan, long long n_pol,
    long long n_tile) {
    constexpr int NT = BBT_PSRFITS_THREADS;
    constexpr PsrFitsTile T = psrfits_tile(TC, VEC);
    constexpr int CPT = T.cpt;                       // columns of a thread
    constexpr int NX = T.nx, NY = T.ny;              // threads across the columns, along the bins
    constexpr int TB = T.tb, NP = T.np, PITCH = T.enc_pitch;
    static_assert(NX >= 1 && NX * NY == NT && (NY & (NY - 1)) == 0 && NP % 2 == 0, "tile shape");
    __shared__ unsigned s_tile[TC * PITCH];
    __shared__ float s_mn[NT * CPT], s_mx[NT * CPT];
    __shared__ int s_cnt[NT * CPT];
    __shared__ float s_scl[TC], s_offs[TC];
    __shared__ long long s_base[TC];

    const long long n_col = n_chan * n_pol;
    const long long row = (long long)blockIdx.x / n_tile;
    const long long m0 = ((long long)blockIdx.x % n_tile) * TC;
    const int tx = threadIdx.x % NX, ty = threadIdx.x / NX;
    const long long mc = m0 + (long long)tx * CPT;
    const float* __restrict__ xr = x + row * n_bin * n_col;

    // 1. min, max and count of the finite bins of every column
    float mn[CPT], mx[CPT];
    int cnt[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) mn[k] = INFINITY, mx[k] = -INFINITY, cnt[k] = 0;
#pragma unroll 4
    for (long long b = ty; b < n_bin; b += NY) {
        float v[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) v[k] = INFINITY;      // (outside the array: not finite)
        psr_load<CPT>(xr + b * n_col, mc, n_col, v);
#pragma unroll
        for (int k = 0; k < CPT; ++k)
            if (psr_finite(v[k])) mn[k] = fminf(mn[k], v[k]), mx[k] = fmaxf(mx[k], v[k]), ++cnt[k];
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int i = ty * TC + tx * CPT + k;
        s_mn[i] = mn[k], s_mx[i] = mx[k], s_cnt[i] = cnt[k];
    }
    __syncthreads();
    for (int s = NY / 2; s > 0; s >>= 1) {
        if (ty < s) {
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int i = ty * TC + tx * CPT + k, j = i + s * TC;
                s_mn[i] = fminf(s_mn[i], s_mn[j]), s_mx[i] = fmaxf(s_mx[i], s_mx[j]), s_cnt[i] += s_cnt[j];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < TC) {
        const int c = threadIdx.x;
        const long long m = m0 + c;
        float sc = 1.f, of = 0.f;
        long long base = 0;
        if (m < n_col) {
            psr_scale(s_mn[c], s_mx[c], s_cnt[c], sc, of);
            const long long q = (m % n_pol) * n_chan + m / n_pol;
            scl[row * n_col + q] = sc, offs[row * n_col + q] = of, n_finite[row * n_col + q] = s_cnt[c];
            base = (row * n_col + q) * n_bin;
        }
        s_scl[c] = sc, s_offs[c] = of, s_base[c] = base;
    }
    __syncthreads();

    // 2. the codes, a tile of TB bins at a time
    float sc[CPT], of[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) sc[k] = s_scl[tx * CPT + k], of[k] = s_offs[tx * CPT + k];
    for (long long b0 = 0; b0 < n_bin; b0 += TB) {
#pragma unroll 2
        for (int p = ty; p < NP; p += NY) {
            const long long b = b0 + 2 * p;
            if (b >= n_bin) break;
            float v0[CPT], v1[CPT];
#pragma unroll
            for (int k = 0; k < CPT; ++k) v0[k] = v1[k] = INFINITY;
            psr_load<CPT>(xr + b * n_col, mc, n_col, v0);
            if (b + 1 < n_bin) psr_load<CPT>(xr + (b + 1) * n_col, mc, n_col, v1);
#pragma unroll
            for (int k = 0; k < CPT; ++k)
                s_tile[(tx * CPT + k) * PITCH + p] = psr_code(v0[k], sc[k], of[k]) | (psr_code(v1[k], sc[k], of[k]) << 16);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TC * NP; i += NT) {
            const int c = i / NP, p = i % NP;
            const long long b = b0 + 2 * p;
            if (m0 + c < n_col && b < n_bin) {
                const unsigned w = s_tile[c * PITCH + p];
                const long long o = s_base[c] + b;
                if (VEC) {                                  // (n_bin and b are even: o is)
                    reinterpret_cast<unsigned*>(codes)[o >> 1] = w;
                } else {
                    codes[o] = (unsigned short)(w & 0xffffu);
                    if (b + 1 < n_bin) codes[o + 1] = (unsigned short)(w >> 16);
                }
            }
        }
        __syncthreads();
    }
}

template <int TC, bool VEC>
__global__ __launch_bounds__(BBT_PSRFITS_THREADS) void k_psrfits_decode(
    const unsigned short* __restrict__ codes, const float* __restrict__ scl, const float* __restrict__ offs,
    const float* __restrict__ wts, float zero_off, float* __restrict__ out, long long n_bin, long long n_chan,
    long long n_pol, long long n_tile) {
    constexpr int NT = BBT_PSRFITS_THREADS;
    constexpr PsrFitsTile T = psrfits_tile(TC, VEC);
    constexpr int CPT = T.cpt;
    constexpr int NX = T.nx, NY = T.ny;
    constexpr int TB = T.tb, NP = T.np, PITCH = T.dec_pitch;
    static_assert(NX >= 1 && NX * NY == NT, "tile shape");
    __shared__ float s_tile[TC * PITCH];
    __shared__ float s_scl[TC], s_offs[TC], s_w[TC];
    __shared__ long long s_base[TC];

    const long long n_col = n_chan * n_pol;
    const long long row = (long long)blockIdx.x / n_tile;
    const long long m0 = ((long long)blockIdx.x % n_tile) * TC;
    const int tx = threadIdx.x % NX, ty = threadIdx.x / NX;
    const long long mc = m0 + (long long)tx * CPT;
    const bool weighted = wts != nullptr;
    if (threadIdx.x < TC) {
        const int c = threadIdx.x;
        const long long m = m0 + c;
        float sc = 1.f, of = 0.f, w = 1.f;
        long long base = 0;
        if (m < n_col) {
            const long long chan = m / n_pol, q = (m % n_pol) * n_chan + chan;
            sc = scl[row * n_col + q], of = offs[row * n_col + q];
            if (weighted) w = wts[row * n_chan + chan];
            base = (row * n_col + q) * n_bin;
        }
        s_scl[c] = sc, s_offs[c] = of, s_w[c] = w, s_base[c] = base;
    }
    __syncthreads();
    float* __restrict__ outr = out + row * n_bin * n_col;
    for (long long b0 = 0; b0 < n_bin; b0 += TB) {
        for (int i = threadIdx.x; i < TC * NP; i += NT) {
            const int c = i / NP, p = i % NP;
            const long long b = b0 + 2 * p;
            if (m0 + c < n_col && b < n_bin) {
                const long long o = s_base[c] + b;
                unsigned w;
                if (VEC) {
                    w = reinterpret_cast<const unsigned*>(codes)[o >> 1];
                } else {
                    w = codes[o];
                    if (b + 1 < n_bin) w |= (unsigned)codes[o + 1] << 16;
                }
                s_tile[c * PITCH + 2 * p] = psr_decode(w & 0xffffu, zero_off, s_scl[c], s_offs[c], s_w[c], weighted);
                s_tile[c * PITCH + 2 * p + 1] = psr_decode(w >> 16, zero_off, s_scl[c], s_offs[c], s_w[c], weighted);
            }
        }
        __syncthreads();
        for (int bl = ty; bl < TB; bl += NY) {
            const long long b = b0 + bl;
            if (b >= n_bin) break;
            float* __restrict__ dst = outr + b * n_col;
            if (VEC) {
                if (mc < n_col) {
                    const int c = tx * CPT;
                    *reinterpret_cast<float4*>(dst + mc) =
                        make_float4(s_tile[c * PITCH + bl], s_tile[(c + (CPT > 1 ? 1 : 0)) * PITCH + bl],
                                    s_tile[(c + (CPT > 2 ? 2 : 0)) * PITCH + bl], s_tile[(c + CPT - 1) * PITCH + bl]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < CPT; ++k)
                    if (mc + k < n_col) dst[mc + k] = s_tile[(tx * CPT + k) * PITCH + bl];
            }
        }
        __syncthreads();
    }
}

}  // namespace bbt
