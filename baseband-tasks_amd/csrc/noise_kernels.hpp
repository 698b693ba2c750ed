// NumPy's normal stream on the device: Philox-4x64-10 words through the 256-step ziggurat sampler,
// bit for bit what `Generator(Philox).normal` gives (the CPU restatement, and the specification, is
// tools/noise_model.py).
//
// The sampler consumes a variable number of words per normal, as a small automaton over the word
// stream.  In state START a word either yields a normal at once (98 %), or opens a wedge test that
// takes the next word as its uniform (WEDGE; accepted or not, the sampler starts again on the word
// after), or (idx 0) opens the tail loop that takes pairs of words (TAIL1, TAIL2) until a pair is
// accepted.  The tail's sign comes from the word that opened it, so it is part of the state: six
// states.  What a word does in each state depends on that word and the one before it only, so
// every word has a map states -> states (3 bits per state) and a flag "emits" per entry state;
// maps compose associatively.  Three passes, no atomics, words never stored (Philox is recomputed):
//   1. k_noise_count: per (frame, tile of 1024 words) the composed map and, per entry state, the
//      number of normals the tile emits
//   2. k_noise_scan:  per frame, the tiles scanned from START: entry state and output offset of
//      every tile, and the frame's total
//   3. k_noise_emit:  per tile, scan of the threads' maps from the entry state; every thread walks
//      its four words from its own entry state and stores the normals whose rank is below n
// A thread owns one Philox block (four words).  Float64 arithmetic of the decisions is not
// contracted.  Comparisons that involve exp / log1p raise the frame's flag when their sides lie
// within a relative `guard` of each other (and so does a tail value whose float32 rounding is not
// safe by that margin): the host then makes that frame with NumPy.
#pragma once
#include <hip/hip_runtime.h>

#include "zig_tables.hpp"

#define BBT_NOISE_TILE 1024          // words per workgroup: 256 threads x one Philox block

namespace bbt {

__device__ const unsigned long long zig_ki[256] = BBT_ZIG_KI;
__device__ const unsigned long long zig_wi[256] = BBT_ZIG_WI;
__device__ const unsigned long long zig_fi[256] = BBT_ZIG_FI;

typedef unsigned long long nu64;

enum { NS_START = 0, NS_WEDGE = 1, NS_TAIL1 = 2, NS_TAIL2 = 4 };      // TAIL1 + sign, TAIL2 + sign
#define BBT_NOISE_IDENTITY (0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12 | 5u << 15)
#define BBT_ZIG_R 3.6541528853610087963519472518
#define BBT_ZIG_INV_R 0.27366123732975827203338247596

struct NoiseTables {
    nu64 ki[256];
    double wi[256];
    double fi[256];
};

// a stretch of words: where each entry state ends up, and how many normals it emits on the way
struct NoiseSeg {
    unsigned map;
    unsigned cnt[6];
};

__device__ __forceinline__ unsigned noise_next(unsigned map, unsigned s) { return (map >> (3 * s)) & 7u; }

__device__ __forceinline__ unsigned noise_pick(const unsigned c[6], unsigned s) {
    return s == 0 ? c[0] : s == 1 ? c[1] : s == 2 ? c[2] : s == 3 ? c[3] : s == 4 ? c[4] : c[5];
}

// a, then b
__device__ __forceinline__ NoiseSeg noise_compose(const NoiseSeg& a, const NoiseSeg& b) {
    NoiseSeg r;
    r.map = 0;
#pragma unroll
    for (unsigned s = 0; s < 6; ++s) {
        const unsigned mid = noise_next(a.map, s);
        r.map |= noise_next(b.map, mid) << (3 * s);
        r.cnt[s] = a.cnt[s] + noise_pick(b.cnt, mid);
    }
    return r;
}

__device__ __forceinline__ void philox4x64_10(nu64 c0, nu64 c1, nu64 c2, nu64 c3, nu64 k0, nu64 k1, nu64 out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B97F4A7C15ull;
            k1 += 0xBB67AE8584CAA73Bull;
        }
        const nu64 hi0 = __umul64hi(0xD2E7470EE14C6C93ull, c0), lo0 = 0xD2E7470EE14C6C93ull * c0;
        const nu64 hi1 = __umul64hi(0xCA5A826395121157ull, c2), lo1 = 0xCA5A826395121157ull * c2;
        c0 = hi1 ^ c1 ^ k0;
        c2 = hi0 ^ c3 ^ k1;
        c1 = lo1;
        c3 = lo0;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// block `b` of a frame: the frame's counter (already one past the state's) plus b, with carries
__device__ __forceinline__ void noise_block(const nu64* __restrict__ ctr, nu64 k0, nu64 k1, nu64 b, nu64 out[4]) {
    const nu64 c0 = ctr[0] + b;
    nu64 carry = c0 < b ? 1 : 0;
    const nu64 c1 = ctr[1] + carry;
    carry = (carry && c1 == 0) ? 1 : 0;
    const nu64 c2 = ctr[2] + carry;
    carry = (carry && c2 == 0) ? 1 : 0;
    philox4x64_10(c0, c1, c2, ctr[3] + carry, k0, k1, out);
}

__device__ __forceinline__ double noise_uniform(nu64 w) { return (double)(w >> 11) * (1.0 / 9007199254740992.0); }

// the value of an initiating word
__device__ __forceinline__ double noise_x(nu64 w, const NoiseTables& T) {
    const nu64 rabs = (w >> 9) & 0x000fffffffffffffull;
    const double x = (double)rabs * T.wi[w & 0xff];
    return ((w >> 8) & 1 ? -x : x) + 0.0;              // (loc + scale * x: -0.0 becomes 0.0)
}

// word w as the uniform of the wedge test opened by wp (idx > 0)
__device__ __forceinline__ bool noise_wedge(nu64 wp, nu64 w, const NoiseTables& T, double guard, bool& amb) {
#pragma clang fp contract(off)
    const unsigned idx = (unsigned)(wp & 0xff);
    const nu64 rabs = (wp >> 9) & 0x000fffffffffffffull;
    const double x = (double)rabs * T.wi[idx];
    const double u = noise_uniform(w);
    const double d = T.fi[idx - 1] - T.fi[idx];
    const double du = d * u;
    const double lhs = du + T.fi[idx];
    const double hx = -0.5 * x;
    const double rhs = exp(hx * x);
    const double gm = guard * fmax(fabs(lhs), fabs(rhs));
    amb = !(fabs(lhs - rhs) > gm);
    return lhs < rhs;
}

// the pair of uniforms (w1, w2) of the tail loop; xx is valid unless the pair is accepted without
// a logarithm (`sure`: 2 u2 (1 - u1)^2 > (u1 / r)^2 (1 + 1e-9) implies acceptance by a margin far
// beyond rounding, since u <= -log1p(-u) <= u / (1 - u))
__device__ __forceinline__ bool noise_tail(nu64 w1, nu64 w2, double guard, bool want_xx, bool& amb, double& xx) {
#pragma clang fp contract(off)
    const double u1 = noise_uniform(w1), u2 = noise_uniform(w2);
    const double a = 1.0 - u1;
    const double b = u1 * BBT_ZIG_INV_R;
    const double a2 = a * a;
    const double b2 = b * b;
    const double l0 = (2.0 * u2) * a2;
    const double r0 = b2 * (1.0 + 1e-9);
    const bool sure = l0 > r0;
    amb = false;
    xx = 0;
    if (sure && !want_xx) return true;
    xx = (-BBT_ZIG_INV_R) * log1p(-u1);
    if (sure) return true;
    const double yy = -log1p(-u2);
    const double l = yy + yy;
    const double r = xx * xx;
    const double gm = guard * fmax(fabs(l), fabs(r));
    amb = !(fabs(l - r) > gm);
    return l > r;
}

// map (3 bits per entry state) and emit flags (1 bit per entry state) of word w behind word wp
__device__ __forceinline__ void noise_word_map(nu64 wp, nu64 w, const NoiseTables& T, unsigned& map, unsigned& emit) {
    const unsigned idx = (unsigned)(w & 0xff);
    const nu64 rabs = (w >> 9) & 0x000fffffffffffffull;
    const bool direct = rabs < T.ki[idx];
    const unsigned sign = (unsigned)((rabs >> 8) & 1);
    const unsigned from_start = direct ? NS_START : idx == 0 ? NS_TAIL1 + sign : NS_WEDGE;
    // the wedge test is evaluated only behind a word that could have opened one
    const unsigned pidx = (unsigned)(wp & 0xff);
    bool amb, wedge_ok = false;
    if (pidx != 0 && !(((wp >> 9) & 0x000fffffffffffffull) < T.ki[pidx])) wedge_ok = noise_wedge(wp, w, T, 0.0, amb);
    double xx;
    const bool tail_ok = noise_tail(wp, w, 0.0, false, amb, xx);
    map = from_start | NS_START << 3 | (NS_TAIL2 + 0) << 6 | (NS_TAIL2 + 1) << 9 |
          (tail_ok ? NS_START : NS_TAIL1 + 0) << 12 | (tail_ok ? NS_START : NS_TAIL1 + 1) << 15;
    emit = (direct ? 1u : 0u) | (wedge_ok ? 2u : 0u) | (tail_ok ? 0x30u : 0u);
}

struct NoiseShared {
    NoiseTables T;
    nu64 last[256];
    unsigned map[256];
    unsigned cnt[6][256];
};

// This thread's four words of tile `tile` (w), the word before them (wp), and the segment they
// make; words at or beyond n_words change nothing.  Leaves the tables in S.T.
__device__ __forceinline__ NoiseSeg noise_thread_seg(NoiseShared& S, const nu64* __restrict__ ctr, nu64 k0, nu64 k1,
                                                     long long tile, long long n_words, nu64 w[4], nu64& wp,
                                                     unsigned map[4], unsigned emit[4]) {
    const int tid = threadIdx.x;
    S.T.ki[tid] = zig_ki[tid];
    S.T.wi[tid] = __longlong_as_double((long long)zig_wi[tid]);
    S.T.fi[tid] = __longlong_as_double((long long)zig_fi[tid]);
    const long long block = tile * (BBT_NOISE_TILE / 4) + tid;
    noise_block(ctr, k0, k1, (nu64)block, w);
    S.last[tid] = w[3];
    __syncthreads();
    if (tid > 0) {
        wp = S.last[tid - 1];
    } else if (block > 0) {
        nu64 q[4];
        noise_block(ctr, k0, k1, (nu64)(block - 1), q);
        wp = q[3];
    } else {
        wp = 0;
    }
    nu64 before = wp;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (block * 4 + j < n_words) {
            noise_word_map(before, w[j], S.T, map[j], emit[j]);
        } else {
            map[j] = BBT_NOISE_IDENTITY;
            emit[j] = 0;
        }
        before = w[j];
    }
    NoiseSeg seg;
    seg.map = 0;
#pragma unroll
    for (unsigned s = 0; s < 6; ++s) {
        unsigned st = s, c = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c += (emit[j] >> st) & 1u;
            st = noise_next(map[j], st);
        }
        seg.map |= st << (3 * s);
        seg.cnt[s] = c;
    }
    return seg;
}

// Inclusive scan of the threads' segments (left in S.map / S.cnt); returns this thread's exclusive
// prefix.  All 256 threads call it.
__device__ __forceinline__ NoiseSeg noise_block_scan(NoiseShared& S, NoiseSeg own) {
    const int tid = threadIdx.x;
    S.map[tid] = own.map;
#pragma unroll
    for (int s = 0; s < 6; ++s) S.cnt[s][tid] = own.cnt[s];
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        NoiseSeg a;
        if (tid >= d) {
            a.map = S.map[tid - d];
#pragma unroll
            for (int s = 0; s < 6; ++s) a.cnt[s] = S.cnt[s][tid - d];
        }
        __syncthreads();
        if (tid >= d) {
            own = noise_compose(a, own);
            S.map[tid] = own.map;
#pragma unroll
            for (int s = 0; s < 6; ++s) S.cnt[s][tid] = own.cnt[s];
        }
        __syncthreads();
    }
    NoiseSeg excl;
    excl.map = BBT_NOISE_IDENTITY;
#pragma unroll
    for (int s = 0; s < 6; ++s) excl.cnt[s] = 0;
    if (tid > 0) {
        excl.map = S.map[tid - 1];
#pragma unroll
        for (int s = 0; s < 6; ++s) excl.cnt[s] = S.cnt[s][tid - 1];
    }
    return excl;
}

// grid (n_tile, n_frame).  ctr: [n_frame][4]; tile_map [n_frame][n_tile]; tile_cnt [n_frame][n_tile][6]
__global__ __launch_bounds__(256) void k_noise_count(const nu64* __restrict__ ctr, nu64 k0, nu64 k1, long long n_words,
                                                     long long n_tile, unsigned* __restrict__ tile_map,
                                                     unsigned* __restrict__ tile_cnt) {
    __shared__ NoiseShared S;
    const long long frame = blockIdx.y, tile = blockIdx.x;
    nu64 w[4], wp;
    unsigned map[4], emit[4];
    const NoiseSeg own = noise_thread_seg(S, ctr + frame * 4, k0, k1, tile, n_words, w, wp, map, emit);
    noise_block_scan(S, own);
    if (threadIdx.x < 6) tile_cnt[(frame * n_tile + tile) * 6 + threadIdx.x] = S.cnt[threadIdx.x][255];
    if (threadIdx.x == 6) tile_map[frame * n_tile + tile] = S.map[255];
}

// grid (n_frame): the frame's tiles from START
__global__ __launch_bounds__(256) void k_noise_scan(const unsigned* __restrict__ tile_map,
                                                    const unsigned* __restrict__ tile_cnt, long long n_tile,
                                                    int* __restrict__ tile_entry, long long* __restrict__ tile_off,
                                                    long long* __restrict__ total) {
    __shared__ NoiseShared S;
    const long long frame = blockIdx.x;
    const int tid = threadIdx.x;
    unsigned state = NS_START;
    long long off = 0;
    for (long long base = 0; base < n_tile; base += 256) {
        const long long t = base + tid;
        NoiseSeg own;
        own.map = BBT_NOISE_IDENTITY;
#pragma unroll
        for (int s = 0; s < 6; ++s) own.cnt[s] = 0;
        if (t < n_tile) {
            own.map = tile_map[frame * n_tile + t];
#pragma unroll
            for (int s = 0; s < 6; ++s) own.cnt[s] = tile_cnt[(frame * n_tile + t) * 6 + s];
        }
        const NoiseSeg excl = noise_block_scan(S, own);
        if (t < n_tile) {
            tile_entry[frame * n_tile + t] = (int)noise_next(excl.map, state);
            tile_off[frame * n_tile + t] = off + noise_pick(excl.cnt, state);
        }
        off += S.cnt[state][255];
        state = noise_next(S.map[255], state);
        __syncthreads();
    }
    if (tid == 0) total[frame] = off;
}

// grid (n_tile, n_frame).  out: frame f's normals at out + f * out_stride; flag[f] set to 1 when a
// decision that bears on the frame's n normals is ambiguous
__global__ __launch_bounds__(256) void k_noise_emit(const nu64* __restrict__ ctr, nu64 k0, nu64 k1, long long n_words,
                                                    long long n_tile, const int* __restrict__ tile_entry,
                                                    const long long* __restrict__ tile_off, long long n, double guard,
                                                    float* __restrict__ out, long long out_stride,
                                                    long long* __restrict__ flag) {
    __shared__ NoiseShared S;
    const long long frame = blockIdx.y, tile = blockIdx.x;
    nu64 w[4], wp;
    unsigned map[4], emit[4];
    const NoiseSeg own = noise_thread_seg(S, ctr + frame * 4, k0, k1, tile, n_words, w, wp, map, emit);
    const NoiseSeg excl = noise_block_scan(S, own);
    const unsigned entry = (unsigned)tile_entry[frame * n_tile + tile];
    unsigned st = noise_next(excl.map, entry);
    long long rank = tile_off[frame * n_tile + tile] + noise_pick(excl.cnt, entry);
    if (rank >= n) return;
    float* dst = out + frame * out_stride;
    const long long word0 = (tile * (BBT_NOISE_TILE / 4) + threadIdx.x) * 4;
    if (st == NS_START && (emit[0] & emit[1] & emit[2] & emit[3] & 1u) && rank + 3 < n &&
        (((uintptr_t)(dst + rank)) & 15) == 0) {
        // (words beyond n_words emit nothing, so all four are inside)
        *(float4*)(dst + rank) = make_float4((float)noise_x(w[0], S.T), (float)noise_x(w[1], S.T),
                                             (float)noise_x(w[2], S.T), (float)noise_x(w[3], S.T));
        return;
    }
    bool ambiguous = false;
    nu64 before = wp;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const nu64 cur = w[j];
        if (word0 + j < n_words && rank < n) {
            if (st == NS_START) {
                if (emit[j] & 1u) dst[rank++] = (float)noise_x(cur, S.T);
                st = noise_next(map[j], NS_START);
            } else if (st == NS_WEDGE) {
                bool amb;
                if (noise_wedge(before, cur, S.T, guard, amb)) dst[rank++] = (float)noise_x(before, S.T);
                ambiguous |= amb;
                st = NS_START;
            } else if (st < NS_TAIL2) {
                st += 2;
            } else {
                bool amb;
                double xx;
                if (noise_tail(before, cur, guard, true, amb, xx)) {
#pragma clang fp contract(off)
                    const double v = BBT_ZIG_R + xx;
                    const double vlo = v * (1.0 - guard);
                    const double vhi = v * (1.0 + guard);
                    ambiguous |= !((float)vlo == (float)vhi);
                    dst[rank++] = (float)(st == NS_TAIL2 + 1 ? -v : v);
                    st = NS_START;
                } else {
                    st -= 2;
                }
                ambiguous |= amb;
            }
        }
        before = cur;
    }
    if (ambiguous) flag[frame] = 1;                       // (every writer writes the same value)
}

}  // namespace bbt
