// Encoders for the compact payloads of the HDF5 intermediate format (reference io/hdf5/payload.py:
// 121-178): float32 components -> VDIF-coded 32-bit words (k_pack, the inverse of k_unpack code 0)
// and float32 <-> IEEE binary16 (k_to_half / k_from_half: the '<f2' / '<c4' raw payloads).  Pure
// streaming kernels: a stream leaves HBM at its stored width instead of as float32.
//
// k_pack: word w of the output holds components [w * 32 / bits, (w + 1) * 32 / bits), the first in
// the least significant bits (VDIF 1.1.1; what `ingest.encode_vdif_frames` makes on the host, the
// yardstick).  ONE THREAD OWNS EVERY WORD IT WRITES: it reads the word's components (16-byte
// loads), assembles the word in a register and stores it -- no atomics, no read-modify-write of
// the output, no word shared between threads; a last, partial word gets zeros in its unused high
// bits.  A thread makes WPT consecutive words: four (one 16-byte store) at 16 and 8 bits, where
// the output is a half and a quarter of the traffic; two at 4 bits and one at 2 and 1 bit, where
// a word alone is 64 / 128 bytes of input -- more words per thread would spread the lanes of one
// load over more cache lines than a wave's share of the vector cache holds, for stores that are
// 1/16 and 1/32 of the bytes moved.  Index arithmetic is 64-bit across the array.
//
// The codes (levels as k_unpack decodes them):
//   1 bit   x > 0
//   2 bits  number of thresholds in {-2, 0, 2} strictly below x
//   4 bits  clip(rint(x * 2.95 + 8), 0, 15)
//   8 bits  clip(rint(x * 35.5 + 127.5), 0, 255)
//   16 bits clip(rint(x + 32768), 0, 65535)
// with the product and the sum rounded to float32 SEPARATELY, as NumPy does on the host: a fused
// multiply-add rounds once and puts ties and near-ties one code off (contraction is switched off
// in pack_affine).  rint rounds half to even.  +-inf clip to the end codes; a NaN encodes as 0.
#pragma once
#include <hip/hip_runtime.h>

namespace bbt {

#define BBT_PACK_THREADS 256

// x * scale + offset in two roundings.  (`__fmul_rn` / `__fadd_rn` are plain operators inside the
// HIP headers, compiled there with contraction allowed: their results fuse again after inlining.
// The pragma covers the operators written here.)
__device__ __forceinline__ float pack_affine(float x, float scale, float offset) {
#pragma clang fp contract(off)
    const float p = x * scale;
    return p + offset;
}

template <int BITS>
__device__ __forceinline__ unsigned pack_code(float x) {
    if (BITS == 1) return x > 0.f ? 1u : 0u;
    if (BITS == 2) return (x > -2.f ? 1u : 0u) + (x > 0.f ? 1u : 0u) + (x > 2.f ? 1u : 0u);
    float v;
    if (BITS == 4) v = pack_affine(x, 2.95f, 8.f);
    else if (BITS == 8) v = pack_affine(x, 35.5f, 127.5f);
    else v = x + 32768.f;
    // (fmaxf returns the other operand for a NaN: code 0)
    v = fminf(fmaxf(rintf(v), 0.f), (float)((1u << BITS) - 1u));
    return (unsigned)(int)v;
}

// VEC: both pointers are 16-byte aligned (float4 loads, WPT-word stores); otherwise scalar
// accesses -- a view that starts inside an allocation.
template <int BITS, int WPT, bool VEC>
__global__ __launch_bounds__(BBT_PACK_THREADS) void k_pack(const float* __restrict__ in,
                                                           unsigned* __restrict__ out,
                                                           long long n_comp, long long n_words) {
    constexpr int PER = 32 / BITS;                  // components of a word
    const long long w0 = ((long long)blockIdx.x * BBT_PACK_THREADS + threadIdx.x) * WPT;
    if (w0 >= n_words) return;
    const long long c0 = w0 * PER;
    unsigned word[WPT];
    if (c0 + (long long)WPT * PER <= n_comp) {      // all WPT words are whole
        constexpr int C = WPT * PER;                // components of the thread: a multiple of 4
#pragma unroll
        for (int k = 0; k < WPT; ++k) word[k] = 0;
        if (VEC) {
#pragma unroll
            for (int j = 0; j < C / 4; ++j) {
                const float4 f = *reinterpret_cast<const float4*>(in + c0 + 4 * j);
                const float x[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    word[(4 * j + m) / PER] |= pack_code<BITS>(x[m]) << (((4 * j + m) % PER) * BITS);
            }
        } else {
#pragma unroll
            for (int q = 0; q < C; ++q) word[q / PER] |= pack_code<BITS>(in[c0 + q]) << ((q % PER) * BITS);
        }
        if (VEC && WPT == 4) {
            *reinterpret_cast<uint4*>(out + w0) = make_uint4(word[0], word[WPT > 1 ? 1 : 0], word[WPT > 2 ? 2 : 0],
                                                             word[WPT - 1]);
        } else if (VEC && WPT == 2) {
            *reinterpret_cast<uint2*>(out + w0) = make_uint2(word[0], word[WPT - 1]);
        } else {
#pragma unroll
            for (int k = 0; k < WPT; ++k) out[w0 + k] = word[k];
        }
        return;
    }
    // the ragged end of the array: component by component, zeros past the last one
#pragma unroll
    for (int k = 0; k < WPT; ++k) {
        if (w0 + k >= n_words) return;
        unsigned acc = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const long long c = c0 + k * PER + j;
            if (c < n_comp) acc |= pack_code<BITS>(in[c]) << (j * BITS);
        }
        out[w0 + k] = acc;
    }
}

// float32 -> binary16, round to nearest even, subnormals kept, overflow to +-inf (one
// v_cvt_f16_f32 per value); eight values a thread: two 16-byte loads, one 16-byte store.
#define BBT_HALF_PER 8

__device__ __forceinline__ unsigned half_pair(float a, float b) {
    const _Float16 ha = (_Float16)a, hb = (_Float16)b;
    return (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
}

template <bool VEC>
__global__ __launch_bounds__(BBT_PACK_THREADS) void k_to_half(const float* __restrict__ in,
                                                              unsigned short* __restrict__ out, long long n) {
    const long long i0 = ((long long)blockIdx.x * BBT_PACK_THREADS + threadIdx.x) * BBT_HALF_PER;
    if (i0 >= n) return;
    if (VEC && i0 + BBT_HALF_PER <= n) {
        const float4 a = *reinterpret_cast<const float4*>(in + i0);
        const float4 b = *reinterpret_cast<const float4*>(in + i0 + 4);
        *reinterpret_cast<uint4*>(out + i0) =
            make_uint4(half_pair(a.x, a.y), half_pair(a.z, a.w), half_pair(b.x, b.y), half_pair(b.z, b.w));
        return;
    }
#pragma unroll
    for (int j = 0; j < BBT_HALF_PER; ++j)
        if (i0 + j < n) out[i0 + j] = __builtin_bit_cast(unsigned short, (_Float16)in[i0 + j]);
}

__device__ __forceinline__ float half_lo(unsigned w) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu));
}
__device__ __forceinline__ float half_hi(unsigned w) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
}

template <bool VEC>
__global__ __launch_bounds__(BBT_PACK_THREADS) void k_from_half(const unsigned short* __restrict__ in,
                                                                float* __restrict__ out, long long n) {
    const long long i0 = ((long long)blockIdx.x * BBT_PACK_THREADS + threadIdx.x) * BBT_HALF_PER;
    if (i0 >= n) return;
    if (VEC && i0 + BBT_HALF_PER <= n) {
        const uint4 h = *reinterpret_cast<const uint4*>(in + i0);
        *reinterpret_cast<float4*>(out + i0) = make_float4(half_lo(h.x), half_hi(h.x), half_lo(h.y), half_hi(h.y));
        *reinterpret_cast<float4*>(out + i0 + 4) = make_float4(half_lo(h.z), half_hi(h.z), half_lo(h.w), half_hi(h.w));
        return;
    }
#pragma unroll
    for (int j = 0; j < BBT_HALF_PER; ++j)
        if (i0 + j < n) out[i0 + j] = (float)__builtin_bit_cast(_Float16, in[i0 + j]);
}

}  // namespace bbt
