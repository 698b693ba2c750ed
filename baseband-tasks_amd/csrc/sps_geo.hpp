// How k_sps_standardize / k_sps_pass (sps_kernels.hpp) cut one chunk of Standardize and BoxcarSearch
// (search.py) into workgroups: plain C++, shared by the host launcher and the kernels (the structs
// are kernel arguments) and compiled on its own by tests/sps_geo_check.cpp.
//
// A chunk is x[t][e], t < n_in, e < n_elem, float32, element fastest: every e is a column of its own.
//
// Standardize.  Blocks of n samples; a workgroup owns nx adjacent elements of one block, threads
// (tx, ty) with ty < ny = 256 / nx.  The ny threads of a column take a segment of 32 samples each
// per round; thread ty = 0 adds the segment sums in segment order.
//
// BoxcarSearch.  S_0 = x, S_{k+1}[i] = S_k[i] + S_k[i + 2^k], defined where i + 2^(k+1) <= n_in.  The
// K levels are made in n_pass = ceil(K / fuse) launches; pass p starts from S_k0, k0 = p * fuse, read
// from global memory (the chunk itself for p = 0, else the scratch the pass before wrote), makes
// the levels k0 ... k0 + fuse - 1 of one start time i in registers from the 2^fuse values S_k0[i +
// m 2^k0], and, unless it is the last, stores S_{k0 + fuse}[i] into the other scratch.  The start
// times are cut into the blocks of n that the output folds; a workgroup owns nx adjacent elements of
// nz adjacent blocks, and `sub` threads share a (block, element): thread part q takes i = b n + q, q +
// sub, ...  Blocks at and beyond nb (the halo, and the dropped tail) are walked by the passes that
// store sums -- later levels of the blocks in front read them -- but have no winner.  Of the chunk
// only the first nb n + 2^(K-1) - 1 samples can be reached by a window that starts in a block; n_in
// is cut to that.
//
// Every index into the chunk, the scratch and the result is 64-bit; only the per-axis counts below
// are bounded.
#pragma once

#define BBT_SPS_THREADS 256
#define BBT_SPS_SEG 32                       // samples of a segment of Standardize's two-level sums
#define BBT_SPS_STD_MIN_N 2
#define BBT_SPS_MAX_N 65536                  // samples of a block, both tasks
#define BBT_SPS_MAX_WIDTHS 13                // widths 1 ... 4096
#define BBT_SPS_WIDTH 64                     // elements of a boxcar workgroup (default): 16, 32 or 64
#define BBT_SPS_FUSE 2                       // levels per pass (default): 1, 2 or 3
#define BBT_SPS_FUSE_MAX 3
#define BBT_SPS_SPLIT 16                     // threads that share a (block, element) at most (default): 1 ... 16
#define BBT_SPS_STD_ROWS 8                   // ny of Standardize (default): 1, 2, 4, 8 or 16
#define BBT_SPS_NONE 255                     // the level of "no winner yet"
#define BBT_SPS_MAX_ROWS (1ll << 40)         // samples of a chunk

// c_k = float32(2^(-k / 2)): a power of two for even k, float32(sqrt(1/2)) = 0x1.6a09e6p-1 times one for odd k
inline float sps_scale(int k) {
    float c = (k & 1) ? 0x1.6a09e6p-1f : 1.f;
    for (int j = 0; j < k / 2; ++j) c *= 0.5f;           // (exact)
    return c;
}

struct StdGeo {
    long long n_block, n, n_elem;
    int nx, ny;                  // threads along the elements, along the segments
    long long n_tile;            // workgroups along the elements
    long long n_wg;              // n_block * n_tile
};

// 0, or what is wrong with a launch.  rows: ny, 1, 2, 4, 8 or 16 (0: the default).
inline const char* sps_std_geo(long long n_block, long long n, long long n_elem, int rows, StdGeo* g) {
    if (n < BBT_SPS_STD_MIN_N || n > BBT_SPS_MAX_N) return "a block must have 2 ... 65536 samples";
    if (n_block < 1) return "no whole block";
    if (n_elem < 1) return "no elements";
    if (n_block * n > BBT_SPS_MAX_ROWS) return "more than 2^40 samples in one call";
    if (rows == 0) rows = BBT_SPS_STD_ROWS;
    if (rows != 1 && rows != 2 && rows != 4 && rows != 8 && rows != 16) return "the rows must be 1, 2, 4, 8 or 16";
    g->n_block = n_block, g->n = n, g->n_elem = n_elem;
    g->ny = rows, g->nx = BBT_SPS_THREADS / rows;
    g->n_tile = (n_elem + g->nx - 1) / g->nx;
    if (g->n_tile >= (1ll << 31) / n_block) return "too many tiles for one launch";
    g->n_wg = n_block * g->n_tile;
    return 0;
}

struct SpsGeo {
    long long n_in;              // samples of the chunk that are used: at most nb n + 2^(K-1) - 1
    long long nb, n, n_elem;     // blocks of the result, samples of a block, elements
    long long nbv;               // blocks walked by a pass that stores sums: ceil(n_in / n)
    int K, fuse, n_pass;
    int nx, ny;                  // threads along the elements, along time
    int sub, nz;                 // threads that share a (block, element); blocks of a workgroup: ny = sub nz
    long long n_tile;            // workgroups along the elements
    long long scratch;           // floats of the scratch: min(n_pass - 1, 2) buffers of n_in n_elem
    float c[BBT_SPS_MAX_WIDTHS]; // c_k
};

// 0, or what is wrong with the sizes of a plan (a static string)
inline const char* sps_sizes(long long n, long long K, long long n_elem) {
    if (n < 1 || n > BBT_SPS_MAX_N) return "a block must have 1 ... 65536 samples";
    if (K < 1 || K > BBT_SPS_MAX_WIDTHS) return "n_widths must be 1 ... 13";
    if (n_elem < 1) return "no elements";
    return 0;
}

// 0, or what is wrong with a launch.  width: 16, 32 or 64; fuse: 1, 2 or 3; split: 1, 2, 4, 8 or 16
// (each 0: the default).
inline const char* sps_geo(long long n_in, long long nb, long long n, long long K, long long n_elem, int width,
                           int fuse, int split, SpsGeo* g) {
    const char* err = sps_sizes(n, K, n_elem);
    if (err) return err;
    if (nb < 1) return "no output blocks";
    if (nb > BBT_SPS_MAX_ROWS / n) return "more than 2^40 samples in one call";
    if (n_in < nb * n) return "the input is shorter than the blocks";
    if (width == 0) width = BBT_SPS_WIDTH;
    if (fuse == 0) fuse = BBT_SPS_FUSE;
    if (split == 0) split = BBT_SPS_SPLIT;
    if (width != 16 && width != 32 && width != 64) return "the width must be 16, 32 or 64 elements";
    if (fuse < 1 || fuse > BBT_SPS_FUSE_MAX) return "the levels of a pass must be 1, 2 or 3";
    if (split != 1 && split != 2 && split != 4 && split != 8 && split != 16) return "the split must be 1, 2, 4, 8 or 16";
    const long long reach = nb * n + (1ll << (K - 1)) - 1;
    g->n_in = n_in < reach ? n_in : reach;
    g->nb = nb, g->n = n, g->n_elem = n_elem, g->K = (int)K, g->fuse = fuse;
    g->n_pass = (int)((K + fuse - 1) / fuse);
    g->nbv = (g->n_in + n - 1) / n;
    g->nx = width, g->ny = BBT_SPS_THREADS / width;
    int sub = 1;
    while (sub * 2 <= g->ny && sub * 2 <= split && sub * 2 <= n) sub *= 2;
    g->sub = sub, g->nz = g->ny / sub;
    g->n_tile = (n_elem + width - 1) / width;
    if (n_elem > (1ll << 40) / g->n_in) return "more than 2^40 values in one call";
    g->scratch = (g->n_pass - 1 < 2 ? g->n_pass - 1 : 2) * g->n_in * n_elem;
    if (g->n_tile >= (1ll << 31) / ((g->nbv + g->nz - 1) / g->nz)) return "too many tiles for one launch";
    for (int k = 0; k < BBT_SPS_MAX_WIDTHS; ++k) g->c[k] = sps_scale(k);
    return 0;
}

// Pass `p` < n_pass: its first level, whether it stores S_{k0 + fuse}, the blocks it walks and its grid.
struct SpsPass {
    int k0, levels;
    bool store;
    long long blocks, n_wg;
};
inline SpsPass sps_pass(const SpsGeo& g, int p) {
    SpsPass o;
    o.k0 = p * g.fuse;
    o.levels = g.K - o.k0 < g.fuse ? g.K - o.k0 : g.fuse;
    o.store = o.k0 + g.fuse < g.K;
    o.blocks = o.store ? g.nbv : g.nb;
    o.n_wg = (o.blocks + g.nz - 1) / g.nz * g.n_tile;
    return o;
}

// What the threads of row `ty` < ny of workgroup `wg` own in a pass that walks `blocks` blocks: block
// b, part q < sub of it, first element e0.  False if the block is beyond those walked.  The kernel
// and the host check share this.
struct SpsOwn {
    long long b, e0;
    int q;
};
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool sps_own(const SpsGeo& g, long long wg, int ty, long long blocks, SpsOwn* o) {
    o->e0 = (wg % g.n_tile) * g.nx;
    o->b = (wg / g.n_tile) * g.nz + ty / g.sub;
    o->q = ty % g.sub;
    return o->b < blocks;
}
