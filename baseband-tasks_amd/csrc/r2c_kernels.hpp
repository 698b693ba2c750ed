// Real2Complex (reference baseband_tasks/conversion.py:77-101): a real stream to complex baseband
// at half the sample rate, frame by frame.  With x_e[m] = x[2m], x_o[m] = x[2m + 1] (m < M) of a
// frame of 2M samples, the reference's fft -> one-sided spectrum -> ifft -> exp(-i pi n / 2) ->
// [::2] is, exactly in exact arithmetic,
//
//   out[m] = (-1)^m (x_e[m] + i (g (*) x_o)[m]),   G = fft(g):  G[0] = 0,  G[j] = -i W_2M^j
//
// (g real: G is Hermitian).  So the real part is the input sample itself, and the imaginary part a
// real circular convolution of length M: pairs of real streams go through one complex transform.
//
//   k_r2c_gen       M = 2^a 3^b 5^c 7^d <= 8192: the whole frame in one workgroup (LDS Stockham
//                   engine, fft_generic.hpp; the run-time specialised twin is gen2_kernels.hpp
//                   BBT_G2_KERNEL_R2C).  Each input byte read once, each output byte written once.
//   k_r2c_big       M = 16384 in one pass likewise, on the four-stage transform of fft_big.hpp.
//   k_r2c_gather    longer M: the odd rows of four slots into one two-stream block of a work
//                   buffer, which an overlap-save plan (response G, hop M) then convolves ...
//   k_r2c_combine   ... and the even rows, the sign and the convolved odd rows into the output.
// Slots: real (frame, stream) pairs t = f S + s, four per transform (gen_functors.hpp R2cSlots).
#pragma once
#include <hip/hip_runtime.h>
#include "gen_kernels.hpp"
#include "big_kernels.hpp"

namespace bbt {

// One workgroup per four slots: n = g.n <= 8192 elements of dynamic LDS.
__global__ __launch_bounds__(BBT_GEN_MAX_THREADS) void k_r2c_gen(const float* __restrict__ in,
                                                  float2* __restrict__ out, int S, long long n_slot,
                                                  int vec, const cf* __restrict__ resp, GenGeo g,
                                                  const cf* __restrict__ wn, GenGeo gr,
                                                  const cf* __restrict__ wnr) {
    extern __shared__ f4 gen_lds[];
    const R2cSlots sl = r2c_slots(in, out, g.n, S, n_slot, blockIdx.x, vec);
    R2cOddSrc src{sl};
    GenRespMul mul{resp, resp, true};
    R2cEvenDst dst{sl};
    gen_conv_open(gen_lds, g, gr, 1, wn, wnr, threadIdx.x, blockDim.x, src, mul, dst);
}

// M = 16384: the same with the four-stage one-workgroup transform of fft_big.hpp (thread tau,
// register j: element tau + T j on input and output; 1024 threads, one workgroup per CU).  The access
// width VEC is a template parameter here: with it chosen at run time the 16 points, the table and
// the slots' addresses did not fit 128 registers (25 spilled dwords).
template <int N, int VEC>
__global__ __launch_bounds__(N / 16, 4) void k_r2c_big(const float* __restrict__ in, float2* __restrict__ out,
                                                        int S, long long n_slot,
                                                        const cf* __restrict__ resp, const cf* __restrict__ tw) {
    constexpr int T = BigGeo<N>::T;
    extern __shared__ v2 big_lds[];
    const int tau = threadIdx.x;
    const R2cSlots sl = r2c_slots(in, out, N, S, n_slot, blockIdx.x, VEC);
    c2 v[16];
    R2cOddSrc src{sl};
    src.template load<16>(tau, T, v);
    wg_fft_big<N, -1>(v, big_lds, tau, tw);
    __builtin_amdgcn_sched_barrier(0);
    apply_resp<T>(v, resp + tau, resp + tau, true);          // G / M, natural order
    __builtin_amdgcn_sched_barrier(0);
    {
        const cf* twb = tw;
        asm volatile("" : "+s"(twb));          // (as k_osm_small_big: the table is loaded again)
        wg_fft_big<N, +1>(v, big_lds, tau, twb);
    }
    R2cEvenDst dst{sl};
#pragma unroll
    for (int j = 0; j < 16; ++j) {           // (one point at a time: the even rows' loads not all hoisted)
        c2 u[1] = {v[j]};
        dst.template store<1>(tau + T * j, 0, u);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// work[(b M + m) 4 + k] = x_o of slot 4 (g0 + b) + k at row m (0 past the last slot), for the
// n_group groups from g0 on.  Element e = m * (4 n_group) + (4 b + k): neighbouring threads take
// neighbouring slots, i.e. neighbouring streams of a frame.  (One thread per slot with the rows in a
// loop was measured slower: too few threads when there are few slots.)
__global__ void k_r2c_gather(const float* __restrict__ in, float* __restrict__ work, long long M, int S,
                             long long n_slot, long long g0, long long n_group) {
    const long long width = 4 * n_group, total = M * width;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const long long m = e / width, u = e - m * width;
        const long long t = g0 * 4 + u, f = t / S, s = t - f * S;
        work[((u >> 2) * M + m) * 4 + (u & 3)] = t < n_slot ? in[(f * 2 * M + 2 * m + 1) * S + s] : 0.f;
    }
}

// out[(f M + m) S + s] = (-1)^m (x[2m], y[m]) for the live slots of groups g0 .. g0 + n_group - 1,
// y = the convolved work buffer (same layout as k_r2c_gather's)
__global__ void k_r2c_combine(const float* __restrict__ in, const float* __restrict__ work,
                              float2* __restrict__ out, long long M, int S, long long n_slot, long long g0,
                              long long n_group) {
    const long long t0 = g0 * 4, width = (n_slot - t0 < 4 * n_group ? n_slot - t0 : 4 * n_group);
    const long long total = M * width;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        const long long m = e / width, u = e - m * width;
        const long long t = t0 + u, f = t / S, s = t - f * S;
        const float sg = (m & 1) ? -1.f : 1.f;
        const float y = work[((u >> 2) * M + m) * 4 + (u & 3)];
        out[(f * M + m) * S + s] = make_float2(sg * in[(f * 2 * M + 2 * m) * S + s], sg * y);
    }
}

}  // namespace bbt
