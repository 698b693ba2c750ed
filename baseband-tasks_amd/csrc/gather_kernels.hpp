// Shaping and combining tasks (reference baseband_tasks/shaping.py `task` methods, combining.py
// `_read_frame`): Reshape, Transpose, GetItem, Stack, Concatenate and every rearranging callable
// are one index map -- element j of an output sample is a copy of element e(j) of the sample at
// the same time offset of source s(j).  No arithmetic, no atomics: every output element has one
// writer.  Three kernels, chosen by the host from the runs of the map (bbt_gather_plan_create):
//
//   k_gather_map<B16>  "run copy": every run is whole, aligned 16-byte units in both rows.  The map
//                      is restated per 16-byte unit; consecutive lanes take consecutive units of the
//                      output, which inside a run are consecutive addresses of the source.
//   k_gather_tile<E>   short runs: a workgroup stages T consecutive samples of the stretch of each
//                      source row that the map uses in LDS (coalesced, 16 bytes a lane where the
//                      alignment allows) and writes the T output rows as 16-byte chunks that it
//                      assembles from LDS through the map.
//   k_gather_map<E>    "direct": one output element per lane, gathered reads.  Right for every
//                      map; the fall-back of the other two when a pointer is not 16-byte aligned.
//
// LDS layout of a tile (bytes).  Source u has a block of T rows of `pitch` bytes at `lds_base`;
// inside a row, offset r of the stretch sits at r + (r >> ROWSH) * G: one granule G (the element,
// 4 bytes at least) of padding after every bank row (256 bytes for 8- and 16-byte reads, 128 for
// the narrower ones, whose bank is (addr / 4) % 32).  A two-axis transpose (A, B) -> (B, A) reads
// with a stride of B elements: the lanes of a 32-lane half then span B bank rows, which the padding
// shifts by 0, G, 2 G, ... so they meet on no bank (B a power of two up to 32).  The rows of a block
// follow each other without gaps (pitch is the padded stretch, rounded to G only), and block u
// starts at (u mod n') * (bank row / n') past a bank row boundary, n' the power of two >= the
// number of sources: the lanes of an interleave of n sources (Stack along the last axis) read n
// stretches of 32 / n' consecutive elements that tile one bank row.
#pragma once
#include <hip/hip_runtime.h>

namespace bbt {

#define BBT_GATHER_MAX_SRC 64
#define BBT_GATHER_THREADS 256

struct alignas(8) GatherB8 { unsigned x, y; };
struct alignas(16) GatherB16 { unsigned x, y, z, w; };

// source pointers of one call: base + first sample (+ start of the stretch, tile route)
struct GatherPtrs { const char* p[BBT_GATHER_MAX_SRC]; };

// per used source, tile route (bytes)
struct GatherTileSrc {
    long long stride;     // source row
    int lds_base, pitch;  // block in LDS
    int len;              // stretch staged per sample
    int pad_;
};

template <typename E> struct GatherGeo {
    static constexpr int EB = (int)sizeof(E);
    static constexpr int G = EB < 4 ? 4 : EB;       // LDS granule
    static constexpr int ROWSH = EB >= 8 ? 8 : 7;   // log2 of the bank row of a read of E
};

// Map route.  tab[j] = (used source, byte offset in its row) for unit j of the output row of R
// units of sizeof(E) bytes; stride[u]: source rows in bytes.  Flat 64-bit index over
// n_samples * R; four independent copies in flight per lane.
template <typename E>
__global__ __launch_bounds__(BBT_GATHER_THREADS) void k_gather_map(GatherPtrs ptrs, const long long* __restrict__ stride,
                                                                    int n_used, const int2* __restrict__ tab, int R,
                                                                    E* __restrict__ out, long long n_samples) {
    __shared__ const char* sp[BBT_GATHER_MAX_SRC];
    __shared__ long long ss[BBT_GATHER_MAX_SRC];
    for (int u = 0; u < n_used; ++u)          // (uniform index: scalar loads of the kernel arguments)
        if ((int)threadIdx.x == u) {
            sp[u] = ptrs.p[u];
            ss[u] = stride[u];
        }
    __syncthreads();
    const long long total = n_samples * (long long)R;
    const long long step = (long long)gridDim.x * BBT_GATHER_THREADS;
    long long g = (long long)blockIdx.x * BBT_GATHER_THREADS + threadIdx.x;
    if (g >= total) return;
    long long t = g / R;
    int j = (int)(g - t * R);
    const long long step_t = step / R;
    const int step_j = (int)(step - step_t * R);
    while (g < total) {
        E v[4];
        long long gg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            gg[k] = g;
            if (g < total) {
                const int2 m = tab[j];
                v[k] = *(const E*)(sp[m.x] + t * ss[m.x] + m.y);
            }
            g += step;
            t += step_t;
            j += step_j;
            if (j >= R) {
                j -= R;
                ++t;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (gg[k] < total) out[gg[k]] = v[k];
    }
}

template <typename E> __device__ __forceinline__ void gather_lds_put16(char* lds, int a, const GatherB16& v) {
    constexpr int G = GatherGeo<E>::G;
    if constexpr (G == 16) {
        *(GatherB16*)(lds + a) = v;
    } else if constexpr (G == 8) {
        *(GatherB8*)(lds + a) = GatherB8{v.x, v.y};
        *(GatherB8*)(lds + a + 8) = GatherB8{v.z, v.w};
    } else {
        *(unsigned*)(lds + a) = v.x;
        *(unsigned*)(lds + a + 4) = v.y;
        *(unsigned*)(lds + a + 8) = v.z;
        *(unsigned*)(lds + a + 12) = v.w;
    }
}

// Tile route.  src[u]: the blocks; vec_mask bit u: stretch u is staged in 16-byte pieces (its
// pointer, row and length are multiples of 16), else element by element.  tab[j] = (LDS offset of
// element j of the output row in row 0 of its block, pitch of that block).  vec_out: the output
// slab of a tile starts 16-byte aligned.  Dynamic LDS: the plan's tile size.
template <typename E>
__global__ __launch_bounds__(BBT_GATHER_THREADS) void k_gather_tile(GatherPtrs ptrs, unsigned long long vec_mask,
                                                                     const GatherTileSrc* __restrict__ src, int n_used,
                                                                     const int2* __restrict__ tab, int R,
                                                                     E* __restrict__ out, long long n_samples, int T,
                                                                     int vec_out) {
    extern __shared__ GatherB16 gather_lds[];
    char* lds = (char*)gather_lds;
    constexpr int EB = GatherGeo<E>::EB, G = GatherGeo<E>::G, ROWSH = GatherGeo<E>::ROWSH;
    const long long n_tiles = (n_samples + T - 1) / T;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long long t0 = tile * T;
        const int tn = (int)((n_samples - t0) < (long long)T ? (n_samples - t0) : (long long)T);
        for (int u = 0; u < n_used; ++u) {
            const GatherTileSrc s = src[u];
            const char* p = ptrs.p[u] + t0 * s.stride;
            if ((vec_mask >> u) & 1ull) {
                const int nq = s.len >> 4, n = tn * nq;
                for (int i = threadIdx.x; i < n; i += BBT_GATHER_THREADS) {
                    const int t = i / nq, r = (i - t * nq) << 4;
                    const GatherB16 v = *(const GatherB16*)(p + t * s.stride + r);
                    gather_lds_put16<E>(lds, s.lds_base + t * s.pitch + r + (r >> ROWSH) * G, v);
                }
            } else {
                const int ne = s.len / EB, n = tn * ne;
                for (int i = threadIdx.x; i < n; i += BBT_GATHER_THREADS) {
                    const int t = i / ne, r = (i - t * ne) * EB;
                    *(E*)(lds + s.lds_base + t * s.pitch + r + (r >> ROWSH) * G) = *(const E*)(p + t * s.stride + r);
                }
            }
        }
        __syncthreads();
        E* o = out + t0 * (long long)R;
        const int n_el = tn * R;
        int done = 0;
        if (vec_out) {
            constexpr int V = 16 / EB;
            const int nch = n_el / V;
            for (int c = threadIdx.x; c < nch; c += BBT_GATHER_THREADS) {
                const int i = c * V;
                int t = i / R, j = i - t * R;
                union {
                    GatherB16 q;
                    E e[V];
                } w;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int2 m = tab[j];
                    w.e[k] = *(const E*)(lds + m.x + t * m.y);
                    if (++j == R) {
                        j = 0;
                        ++t;
                    }
                }
                ((GatherB16*)o)[c] = w.q;
            }
            done = nch * V;
        }
        for (int i = done + threadIdx.x; i < n_el; i += BBT_GATHER_THREADS) {
            const int t = i / R, j = i - t * R;
            const int2 m = tab[j];
            o[i] = *(const E*)(lds + m.x + t * m.y);
        }
        __syncthreads();
    }
}

}  // namespace bbt
