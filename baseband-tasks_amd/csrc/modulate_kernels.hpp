// Modulation by a pulse profile: out[n, e] = in[n, e] * gain[bin(n), e] (Modulate in
// modulation.py; the host twin is modulation.modulate_samples).
//
// The stream is a flat array of floats, `fps` per sample (a complex element is two floats that
// share a gain); element-float f of sample n takes gain[bin(n) * gs + (f >> cshift)], with gs = 0
// for a gain per bin alone.  A workgroup owns a tile of 1024 accesses of W floats (W = 4: 16-byte
// loads and stores; W = 1 where the addresses do not allow them), which covers the samples
// s_lo .. s_hi.  It first finds the bin of each of those samples once, into LDS:
//   runs route    one search of the run table for s_lo, then a forward walk: the runs that begin
//                 inside the tile mark their first sample, and a running maximum over the marks
//                 (per thread over a few samples, a scan over the threads) gives every sample its
//                 run.  A run that covers the whole tile needs none of that.
//   pieces route  phase_bin of phase_kernels.hpp per sample, the piece found by one search per
//                 tile and a forward walk; k wrapped with a non-negative modulo.
// and then streams the tile: every input float is read once and every output float written once,
// by vector stores of the thread that read it.  The floats past the last whole access (at most
// three) go with the last tile, one per thread.
#pragma once
#include <hip/hip_runtime.h>
#include "phase_kernels.hpp"

#define BBT_MOD_TILE 1024            // accesses per workgroup: 256 threads x 4
#define BBT_MOD_SEG 17               // most samples per thread in the walk (odd strides: no LDS bank conflicts)
#define BBT_MOD_CAP (256 * BBT_MOD_SEG)   // >= samples a tile can meet: (4 * 1024 + 3 - 1) / 1 + 2

namespace bbt {

struct ModRuns {
    const long long* begin;          // [n_run] first sample of each run; begin[0] = 0, increasing
    const long long* bin;            // [n_run] wrapped bin of each run
    long long n_run;
};

struct ModArgs {
    const float* in;
    float* out;
    long long n_in;                  // samples
    long long n_float;               // n_in * fps
    unsigned fps;                    // floats per sample
    const float* gain;               // [n_phase][gs or 1]
    long long n_phase;
    unsigned gs;                     // gain stride: 0 or elements per sample
    int cshift;                      // 0: a gain per float; 1: per pair of floats (complex)
};

// Exclusive running maximum of v over the 256 threads of the workgroup (v >= 0).
__device__ __forceinline__ int block_excl_max_256(int v, int* wave_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl = max(incl, o);
    }
    if (lane == 63) wave_max[wave] = incl;
    int excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0;
    __syncthreads();
    for (int w = 0; w < wave; ++w) excl = max(excl, wave_max[w]);
    return excl;
}

// Bins of samples s_lo .. s_lo + ns - 1 into sbin, from the run table.  Returns true, with the bin
// in `one`, if a single run covers them all (sbin is then not written).
__device__ __forceinline__ bool mod_bins_runs(const ModRuns& R, long long s_lo, int ns, long long n_in,
                                              long long n_phase, int* sbin, int* wave_max, long long& one) {
    // last run that begins at or before s_lo (the same search in every thread): runs are about
    // evenly long, so bracket it by doubling steps from a proportional guess, then bisect -- a few
    // dependent loads instead of log2(n_run)
    long long a = min(max((long long)((double)s_lo / (double)n_in * (double)R.n_run), 0ll), R.n_run - 1);
    long long b;
    if (R.begin[a] <= s_lo) {
        long long step = 1;
        while (a + step < R.n_run && R.begin[a + step] <= s_lo) {
            a += step;
            step <<= 1;
        }
        b = min(a + step, R.n_run);
    } else {
        b = a;
        long long step = 1;
        while (b - step > 0 && R.begin[b - step] > s_lo) {
            b -= step;
            step <<= 1;
        }
        a = max(b - step, 0ll);                            // (begin[0] = 0 <= s_lo)
    }
    while (b - a > 1) {
        const long long mid = (a + b) >> 1;
        if (R.begin[mid] <= s_lo) a = mid; else b = mid;
    }
    const long long r0 = a;
    const long long next = r0 + 1 < R.n_run ? R.begin[r0 + 1] : n_in;
    if (next >= s_lo + ns || next <= s_lo) {               // (next <= s_lo: not a table; one bin, in range)
        one = min(max(R.bin[r0], 0ll), n_phase - 1);
        return true;
    }
    const int tid = threadIdx.x;
    const int seg = ((ns + 255) >> 8) | 1;                  // samples per thread: odd, <= BBT_MOD_SEG
    const int i0 = tid * seg;
    for (int i = 0; i < seg; ++i)
        if (i0 + i < ns) sbin[i0 + i] = 0;
    __syncthreads();
    for (long long r = r0 + 1 + tid; r < R.n_run; r += 256) {
        const long long rel = R.begin[r] - s_lo;
        if (rel >= ns) break;
        if (rel > 0) sbin[rel] = (int)(r - r0);             // (r - r0 <= rel < ns: fits an int)
    }
    __syncthreads();
    int m = 0;
    for (int i = 0; i < seg; ++i)
        if (i0 + i < ns) m = max(m, sbin[i0 + i]);
    int run = block_excl_max_256(m, wave_max);
    int have = -1;
    int bin = 0;
    for (int i = 0; i < seg; ++i) {
        if (i0 + i >= ns) break;
        run = max(run, sbin[i0 + i]);
        if (run != have) {
            const long long r = min(r0 + run, R.n_run - 1);
            bin = (int)min(max(R.bin[r], 0ll), n_phase - 1);
            have = run;
        }
        sbin[i0 + i] = bin;
    }
    __syncthreads();
    return false;
}

// The same from polynomial pieces: polynomial_bins' k, wrapped.
__device__ __forceinline__ void mod_bins_pieces(const PhasePieces& P, long long s_lo, int ns, long long n_phase,
                                                int* sbin) {
    const int p_lo = phase_piece_of(P, s_lo);
    for (int i = threadIdx.x; i < ns; i += 256) {
        const long long s = s_lo + i;
        int p = p_lo;
        while (p + 1 < P.n_piece && P.lo[p + 1] <= s) ++p;
        const long long k = phase_bin(P, p, s, n_phase);
        long long bin = k % n_phase;
        if (bin < 0) bin += n_phase;
        sbin[i] = (int)bin;
    }
    __syncthreads();
}

// ROUTE 0: runs, 1: pieces.  W: floats per access.  ONE: fps % W == 0 (an access lies within one
// sample, and the gains of its floats are adjacent and aligned like the access).
template <int ROUTE, int W, bool ONE>
__global__ __launch_bounds__(256) void k_modulate(ModArgs A, ModRuns R, PhasePieces P) {
    __shared__ int sbin[BBT_MOD_CAP];
    __shared__ int wave_max[4];
    const long long n_acc = A.n_float / W;                  // whole accesses
    const long long acc0 = (long long)blockIdx.x * BBT_MOD_TILE;
    const bool last = blockIdx.x == gridDim.x - 1;
    const long long f0 = acc0 * W;
    const long long f1 = last ? A.n_float : f0 + (long long)BBT_MOD_TILE * W;     // floats [f0, f1)
    if (f1 <= f0) return;
    const long long s_lo = f0 / A.fps;
    const unsigned rem0 = (unsigned)(f0 - s_lo * A.fps);
    const long long s_hi = min((f1 - 1) / A.fps, A.n_in - 1);
    const int ns = (int)min(s_hi - s_lo + 1, (long long)BBT_MOD_CAP);
    long long one = 0;
    bool uniform = false;
    if (ROUTE == 0) uniform = mod_bins_runs(R, s_lo, ns, A.n_in, A.n_phase, sbin, wave_max, one);
    else mod_bins_pieces(P, s_lo, ns, A.n_phase, sbin);
    const unsigned fps = A.fps, gs = A.gs;
    const int cs = A.cshift;
    const unsigned ubin = (unsigned)one;

    using vec = float __attribute__((ext_vector_type(W)));
    const vec* in = (const vec*)A.in;
    vec* out = (vec*)A.out;
    vec x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const long long v = acc0 + u * 256 + threadIdx.x;
        if (v < n_acc) x[u] = in[v];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const unsigned vl = u * 256 + threadIdx.x;
        const long long v = acc0 + vl;
        if (v >= n_acc) continue;
        const unsigned o = rem0 + vl * W;                   // float offset from the start of sample s_lo
        unsigned sr = o / fps;
        unsigned e = o - sr * fps;
        if (ONE) {
            const unsigned b = uniform ? ubin : (unsigned)sbin[min(sr, (unsigned)(ns - 1))];
            if (gs == 0) {
                x[u] *= A.gain[b];
            } else {
                const float* g = A.gain + (size_t)b * gs + (e >> cs);
                if (W == 1) {
                    x[u] *= g[0];
                } else if (cs == 0) {
                    x[u] *= *(const vec*)g;
                } else {
                    const float2 g2 = *(const float2*)g;
                    x[u][0] *= g2.x;
                    x[u][1] *= g2.x;
                    x[u][W > 1 ? 2 : 0] *= g2.y;
                    x[u][W > 1 ? 3 : 0] *= g2.y;
                }
            }
        } else {
            unsigned have = 0xffffffffu, b = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) {
                while (e >= fps) {
                    e -= fps;
                    ++sr;
                }
                if (sr != have) {
                    b = uniform ? ubin : (unsigned)sbin[min(sr, (unsigned)(ns - 1))];
                    have = sr;
                }
                x[u][j] *= A.gain[gs ? (size_t)b * gs + (e >> cs) : (size_t)b];
                ++e;
            }
        }
        out[v] = x[u];
    }
    // the floats past the last whole access
    if (last && W > 1) {
        const long long f = n_acc * W + threadIdx.x;
        if (f < A.n_float) {
            const unsigned o = rem0 + (unsigned)(f - f0);
            const unsigned sr = o / fps;
            const unsigned e = o - sr * fps;
            const unsigned b = uniform ? ubin : (unsigned)sbin[min(sr, (unsigned)(ns - 1))];
            A.out[f] = A.in[f] * A.gain[gs ? (size_t)b * gs + (e >> cs) : (size_t)b];
        }
    }
}

}  // namespace bbt
