// How k_hsum_whiten / k_hsum_search (hsum_kernels.hpp) cut one chunk of Whiten and HarmonicSearch
// (periodicity.py) into workgroups: plain C++, shared by the host launcher and the kernels (the
// structs are kernel arguments) and compiled on its own by tests/hsum_geo_check.cpp.
//
// A chunk is p[s][j][e], s < n_spec spectra, j < nbin bins, e < n_elem, float32, element fastest:
// every (s, e) is a spectrum of its own.
//
// Whiten.  Bins below `skip` are one block that comes out +0; from `skip` on blocks of m bins, the
// last one whatever is left (at least one bin).  A workgroup owns nx adjacent elements of one
// (spectrum, block), threads (tx, ty) with ty < ny = 256 / nx.  The ny threads of a column take a
// segment of 32 bins each per round; thread ty = 0 adds the segment sums in segment order.
//
// HarmonicSearch.  The bins are cut into blocks of n (the last may be short), nb = ceil(nbin / n); the
// (spectrum, block) pairs are numbered s nb + b.  A workgroup owns nx adjacent elements of nz adjacent
// pairs, and `sub` threads share a (pair, element): thread part q takes j = b n + q, q + sub, ...  For
// level L it gathers the rows (j i + 2^(L-1)) >> L, i odd below 2^L, of its own spectrum: all at most j.
//
// Every address is 64-bit; j i stays below 2^29 (nbin <= 2^24, i < 32), so the index arithmetic of a
// spectrum is int32.
#pragma once

#define BBT_HSUM_THREADS 256
#define BBT_HSUM_SEG 32                      // bins of a segment of Whiten's two-level sums
#define BBT_HSUM_MIN_M 2
#define BBT_HSUM_MAX_M 65536                 // bins of a whitening block
#define BBT_HSUM_MAX_N 65536                 // bins of a search block
#define BBT_HSUM_MAX_LEVELS 6                // sums of 1, 2, 4, 8, 16, 32 harmonics
#define BBT_HSUM_MAX_NBIN (1 << 24)          // bins of a spectrum the search takes
#define BBT_HSUM_WIDTH 64                    // elements of a search workgroup (default): 16, 32 or 64
#define BBT_HSUM_SPLIT 16                    // threads that share a (pair, element) at most (default): 1, 2, 4, 8 or 16
#define BBT_HSUM_ROWS 8                      // ny of Whiten (default): 1, 2, 4, 8 or 16
#define BBT_HSUM_NONE 255                    // the level of "no winner yet"
#define BBT_HSUM_MAX_ROWS (1ll << 40)        // rows (spectra times bins) of a chunk

struct WhitenGeo {
    long long n_spec, nbin, n_elem, m, skip;
    int nx, ny;                  // threads along the elements, along the segments
    long long n_tile;            // workgroups along the elements
    long long n_blk;             // blocks of a spectrum, the one below `skip` (if any) included
    long long n_wg;              // n_spec * n_blk * n_tile
};

// 0, or what is wrong with a launch (a static string).  rows: ny, 1, 2, 4, 8 or 16 (0: the default).
inline const char* hsum_whiten_geo(long long n_spec, long long nbin, long long n_elem, long long m, long long skip,
                                   int rows, WhitenGeo* g) {
    if (m < BBT_HSUM_MIN_M || m > BBT_HSUM_MAX_M) return "a whitening block must have 2 ... 65536 bins";
    if (n_spec < 1) return "no spectra";
    if (nbin < 1) return "no bins";
    if (n_elem < 1) return "no elements";
    if (skip < 0 || skip >= nbin) return "skip must be 0 ... nbin - 1";
    if (nbin > BBT_HSUM_MAX_ROWS / n_spec) return "more than 2^40 bins in one call";
    if (n_elem > BBT_HSUM_MAX_ROWS / (n_spec * nbin)) return "more than 2^40 values in one call";
    if (rows == 0) rows = BBT_HSUM_ROWS;
    if (rows != 1 && rows != 2 && rows != 4 && rows != 8 && rows != 16) return "the rows must be 1, 2, 4, 8 or 16";
    g->n_spec = n_spec, g->nbin = nbin, g->n_elem = n_elem, g->m = m, g->skip = skip;
    g->ny = rows, g->nx = BBT_HSUM_THREADS / rows;
    g->n_tile = (n_elem + g->nx - 1) / g->nx;
    g->n_blk = (nbin - skip + m - 1) / m + (skip > 0 ? 1 : 0);
    if (g->n_tile >= (1ll << 31) / g->n_blk || g->n_tile * g->n_blk >= (1ll << 31) / n_spec)
        return "too many tiles for one launch";
    g->n_wg = n_spec * g->n_blk * g->n_tile;
    return 0;
}

// What workgroup `wg` owns: bins [j0, j0 + len) of spectrum s, first element e0; zero: the block below
// `skip`, which is only cleared.  The kernel and the host check share this.
struct WhitenOwn {
    long long s, j0, len, e0;
    bool zero;
};
#ifdef __HIPCC__
__host__ __device__
#endif
inline void hsum_whiten_own(const WhitenGeo& g, long long wg, WhitenOwn* o) {
    o->e0 = (wg % g.n_tile) * g.nx;
    const long long sb = wg / g.n_tile;
    o->s = sb / g.n_blk;
    long long b = sb % g.n_blk;
    o->zero = g.skip > 0 && b == 0;
    if (o->zero) {
        o->j0 = 0, o->len = g.skip;
        return;
    }
    if (g.skip > 0) --b;
    o->j0 = g.skip + b * g.m;
    o->len = g.nbin - o->j0 < g.m ? g.nbin - o->j0 : g.m;
}

struct HsumGeo {
    long long n_spec, nbin, n_elem;
    long long n, nb, lo;         // bins of a block, blocks of a spectrum, the lowest bin of a fundamental
    long long n_pair;            // n_spec * nb
    int K;
    int nx, ny;                  // threads along the elements, along the pairs and parts
    int sub, nz;                 // threads that share a (pair, element); pairs of a workgroup: ny = sub nz
    long long n_tile;            // workgroups along the elements
    long long n_wg;
    float c[BBT_HSUM_MAX_LEVELS];   // c_L = float32(sqrt(averaged / 2^L)), from the plan's table
};

// 0, or what is wrong with the sizes of a plan (a static string)
inline const char* hsum_sizes(long long nbin, long long n, long long K, long long lo, long long n_elem) {
    if (nbin < 1 || nbin > BBT_HSUM_MAX_NBIN) return "a spectrum must have 1 ... 2^24 bins";
    if (n < 1 || n > BBT_HSUM_MAX_N) return "a search block must have 1 ... 65536 bins";
    if (K < 1 || K > BBT_HSUM_MAX_LEVELS) return "n_levels must be 1 ... 6";
    if (lo < 0 || lo >= nbin) return "lo must be 0 ... nbin - 1";
    if (n_elem < 1) return "no elements";
    return 0;
}

// 0, or what is wrong with a launch.  width: 16, 32 or 64; split: 1, 2, 4, 8 or 16 (each 0: the default).
// The scales are not set here.
inline const char* hsum_geo(long long n_spec, long long nbin, long long n, long long K, long long lo, long long n_elem,
                            int width, int split, HsumGeo* g) {
    const char* err = hsum_sizes(nbin, n, K, lo, n_elem);
    if (err) return err;
    if (n_spec < 1) return "no spectra";
    if (n_spec > BBT_HSUM_MAX_ROWS / nbin) return "more than 2^40 bins in one call";
    if (n_elem > BBT_HSUM_MAX_ROWS / (n_spec * nbin)) return "more than 2^40 values in one call";
    if (width == 0) width = BBT_HSUM_WIDTH;
    if (split == 0) split = BBT_HSUM_SPLIT;
    if (width != 16 && width != 32 && width != 64) return "the width must be 16, 32 or 64 elements";
    if (split != 1 && split != 2 && split != 4 && split != 8 && split != 16) return "the split must be 1, 2, 4, 8 or 16";
    g->n_spec = n_spec, g->nbin = nbin, g->n_elem = n_elem, g->n = n, g->lo = lo, g->K = (int)K;
    g->nb = (nbin + n - 1) / n;
    g->n_pair = n_spec * g->nb;
    g->nx = width, g->ny = BBT_HSUM_THREADS / width;
    int sub = 1;
    while (sub * 2 <= g->ny && sub * 2 <= split && sub * 2 <= n) sub *= 2;
    g->sub = sub, g->nz = g->ny / sub;
    g->n_tile = (n_elem + width - 1) / width;
    const long long groups = (g->n_pair + g->nz - 1) / g->nz;
    if (g->n_tile >= (1ll << 31) / groups) return "too many tiles for one launch";
    g->n_wg = groups * g->n_tile;
    return 0;
}

// What the threads of row `ty` < ny of workgroup `wg` own: spectrum s, block b, part q < sub of it, first
// element e0.  False if the pair is beyond the last.  The kernel and the host check share this.
struct HsumOwn {
    long long s, b, e0;
    int q;
};
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool hsum_own(const HsumGeo& g, long long wg, int ty, HsumOwn* o) {
    o->e0 = (wg % g.n_tile) * g.nx;
    const long long pair = (wg / g.n_tile) * g.nz + ty / g.sub;
    o->q = ty % g.sub;
    o->s = pair / g.nb;
    o->b = pair % g.nb;
    return pair < g.n_pair;
}

// The bin that harmonic i of 2^L gathers for the top harmonic j: round_half_up(j i / 2^L); never above j
// for i <= 2^L.  j < 2^24 and i < 2^5: the product fits an int.
#ifdef __HIPCC__
__host__ __device__
#endif
inline int hsum_bin(int j, int i, int L) { return L == 0 ? j : (j * i + (1 << (L - 1))) >> L; }
