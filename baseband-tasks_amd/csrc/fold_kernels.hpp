// Folding by a run table (reference baseband_tasks/integration.py: Fold._integrate 380-395,
// Integrate._integrate 270-303 for phase bins): output slot j owns the runs
// slot_ptr[j] .. slot_ptr[j+1]-1, run r the input samples [run_begin[r], run_end[r]), and
//   out[j, :] = (prev ? prev[j, :] : 0) + sum over its runs and samples of f(in[t, :]),
//   then times scale[j] if scale is given
// with f the detection of k_detect_integrate (0 = |z|^2, 1 = Power of (X, Y), 2 = identity).
//
// Output-stationary gather: a workgroup owns one slot, one tile of columns and one of n_split
// equal shares of the slot's samples (in run order), sums in registers and writes once -- no
// atomics, so the result depends on the arguments only.  Lanes map to columns ("units": 16 bytes
// where the row allows, one float / complex otherwise); when a row has fewer than 256 units the
// remaining lanes go across time and an LDS tree (fixed order) adds them up.  Each lane adds at
// most BBT_FOLD_BLOCK samples into a sub-sum before adding that to its total, which bounds the
// sequential float32 error for bins of millions of samples.  With n_split > 1 the shares land in
// a work area and k_fold_combine adds them in split order.
#pragma once
#include <hip/hip_runtime.h>

#define BBT_FOLD_BLOCK 1024

namespace bbt {

// Output floats per unit.
template <int MODE, int VEC>
struct FoldUnit {
    static constexpr int OUTW = MODE == 1 ? 4 : (MODE == 0 ? (VEC ? 2 : 1) : (VEC ? 4 : 1));
};

template <int MODE, int VEC>
__device__ __forceinline__ void fold_add(float4& acc, const void* __restrict__ in, long long idx) {
    if (MODE == 1) {
        const float4 z = ((const float4*)in)[idx];          // X = (x, y), Y = (z, w)
        acc.x += z.x * z.x + z.y * z.y;
        acc.y += z.z * z.z + z.w * z.w;
        acc.z += z.x * z.z + z.y * z.w;
        acc.w += z.y * z.z - z.x * z.w;
    } else if (MODE == 0 && VEC) {
        const float4 z = ((const float4*)in)[idx];          // two complex elements
        acc.x += z.x * z.x + z.y * z.y;
        acc.y += z.z * z.z + z.w * z.w;
    } else if (MODE == 0) {
        const float2 z = ((const float2*)in)[idx];
        acc.x += z.x * z.x + z.y * z.y;
    } else if (VEC) {
        const float4 z = ((const float4*)in)[idx];
        acc.x += z.x;
        acc.y += z.y;
        acc.z += z.z;
        acc.w += z.w;
    } else {
        acc.x += ((const float*)in)[idx];
    }
}

__device__ __forceinline__ void f4_add(float4& a, const float4& b) {
    a.x += b.x;
    a.y += b.y;
    a.z += b.z;
    a.w += b.w;
}

__device__ __forceinline__ long long fold_clamp(long long v, long long n) {
    return v < 0 ? 0 : (v > n ? n : v);
}

// grid: tiles x n_slot x n_split workgroups (flattened, tile fastest), 256 threads:
// 2^lg_tc lanes across units, 256 >> lg_tc across time.  dst: the output (n_split == 1,
// prev / scale applied) or the work area, share s at dst + s * split_stride.
template <int MODE, int VEC>
__global__ __launch_bounds__(256) void k_fold_gather(
    const void* __restrict__ in, float* dst, long long n_in, long long n_unit,
    int lg_tc, long long tiles, long long n_slot, int n_split, const long long* __restrict__ slot_ptr,
    const long long* __restrict__ run_begin, const long long* __restrict__ run_end,
    const float* prev, const float* __restrict__ scale, long long split_stride) {
    constexpr int OUTW = FoldUnit<MODE, VEC>::OUTW;
    __shared__ float4 red[256];
    const int tc = 1 << lg_tc, tt = 256 >> lg_tc;
    const int cx = threadIdx.x & (tc - 1), ty = threadIdx.x >> lg_tc;
    long long g = (long long)blockIdx.x;
    const long long tile = g % tiles;
    g /= tiles;
    const long long j = g % n_slot;
    const int s = (int)(g / n_slot);
    const long long u = tile * tc + cx;
    const bool live = u < n_unit;
    const long long r0 = slot_ptr[j], r1 = slot_ptr[j + 1];
    long long total = 0;
    for (long long r = r0; r < r1; ++r) {
        const long long b = fold_clamp(run_begin[r], n_in), e = fold_clamp(run_end[r], n_in);
        if (e > b) total += e - b;
    }
    const long long lo = total * s / n_split, hi = total * (s + 1) / n_split;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), sub = acc;
    int nsub = 0;
    long long pos = 0;
    for (long long r = r0; r < r1 && pos < hi; ++r) {
        const long long b = fold_clamp(run_begin[r], n_in), e = fold_clamp(run_end[r], n_in);
        if (e <= b) continue;
        const long long len = e - b;
        const long long a0 = lo - pos > 0 ? lo - pos : 0, a1 = hi - pos < len ? hi - pos : len;
        pos += len;
        if (a0 >= a1 || !live) continue;
        long long t = b + a0 + ty;
        const long long tend = b + a1;
        while (t < tend) {
            const long long left = (tend - t + tt - 1) / tt;
            const long long take = left < (long long)(BBT_FOLD_BLOCK - nsub) ? left : (long long)(BBT_FOLD_BLOCK - nsub);
            const long long tstop = t + take * tt;
#pragma unroll 4
            for (; t < tstop; t += tt) fold_add<MODE, VEC>(sub, in, t * n_unit + u);
            nsub += (int)take;
            if (nsub == BBT_FOLD_BLOCK) {
                f4_add(acc, sub);
                sub = make_float4(0.f, 0.f, 0.f, 0.f);
                nsub = 0;
            }
        }
    }
    f4_add(acc, sub);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int h = tt >> 1; h >= 1; h >>= 1) {
        if (ty < h) f4_add(red[threadIdx.x], red[threadIdx.x + (h << lg_tc)]);
        __syncthreads();
    }
    if (ty != 0 || !live) return;
    const float4 v4 = red[cx];
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    const long long base = (j * n_unit + u) * OUTW;
    float* o = dst + (long long)s * split_stride + base;
    const float sc = scale ? scale[j] : 1.0f;
#pragma unroll
    for (int c = 0; c < OUTW; ++c) {
        float x = v[c];
        if (prev) x = prev[base + c] + x;
        if (scale) x *= sc;
        o[c] = x;
    }
}

// out[j, f] = ((accumulate ? out[j, f] : 0) + sum_{s < n_split} work[s][j, f]) * (scale ? scale[j] : 1),
// the shares added in split order.
__global__ __launch_bounds__(256) void k_fold_combine(const float* __restrict__ work, float* out,
                                                      long long n_slot, long long n_out_f, int n_split,
                                                      long long split_stride, const float* __restrict__ scale,
                                                      int accumulate) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_slot * n_out_f) return;
    float v = 0.f;
    for (int s = 0; s < n_split; ++s) v += work[(long long)s * split_stride + idx];
    if (accumulate) v = out[idx] + v;
    if (scale) v *= scale[idx / n_out_f];
    out[idx] = v;
}

}  // namespace bbt
