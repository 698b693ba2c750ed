// How k_rank (rank_kernels.hpp) cuts one chunk of RobustStandardize (search.py) and MedianWhiten
// (periodicity.py) into workgroups, and the integer rules of the selection itself: plain C++, shared
// by the host launcher and the kernels (RankGeo is a kernel argument) and compiled on its own by
// tests/rank_geo_check.cpp.
//
// A chunk is x[s][j][e], s < n_spec, j < nbin, e < n_elem, float32, element fastest: row s nbin + j of
// n_elem floats.  Rows below `skip` of a spectrum belong to no block; from `skip` on the rows are cut
// into nblk = ceil((nbin - skip) / m) blocks of m, the last whatever is left (down to one row).  The
// time-domain blocks of RobustStandardize are n_spec = 1, nbin = n_block n, skip = 0, m = n.
//
// A workgroup of 256 threads owns nx adjacent elements of ONE block: threads (tx, ty), ty < ny = 256 /
// nx, lanes along the elements so that every row access is nx consecutive floats, the ny threads of a
// column taking rows ty, ty + ny, ... of the block.  Workgroup wg = (s nblk + b) n_tile + tile.  The
// workgroup of block 0 also writes the +0 of the `skip` rows in front of it.
//
// Two routes over one rule.  lds: the tile's block, L rows of nx floats, is loaded into LDS once and
// both descents and the rewrite run from there.  global: the descents re-read the tile from global
// memory.  Either way the LDS of a workgroup is
//     histogram 2^digit counters x nx columns x 4 bytes  +  BBT_RANK_MISC_BYTES  (+ L nx 4 on lds)
// and is kept within BBT_RANK_LDS_BYTES = 72 KiB, so that two workgroups fit the 160 KiB of a CU (the
// widest histogram, 256 counters x 64 columns, is 64 KiB of it); the lds route takes a block if its L
// (the longest of the launch) is at most rank_lds_rows(nx, digit).
//
// Every index into the chunk is 64-bit; only the per-axis counts below are bounded.
#pragma once

#define BBT_RANK_THREADS 256
#define BBT_RANK_MIN_N 2
#define BBT_RANK_MAX_N 65536                 // rows of a block; every counter of a histogram holds it
#define BBT_RANK_MAX_ROWS (1ll << 40)        // rows of a chunk
#define BBT_RANK_LDS_BYTES 73728             // LDS of a workgroup at most: 72 KiB (two fit a CU's 160 KiB)
#define BBT_RANK_MISC_BYTES 1024             // the per-column minima and flags
#define BBT_RANK_DIGIT 0                     // bits of a digit: 4 or 8; 0: 4 on the lds route, 8 on the global one
#define BBT_RANK_DIGIT_LDS 4
#define BBT_RANK_DIGIT_GLOBAL 8
#define BBT_RANK_WIDTH 0                     // nx: 16, 32 or 64; 0: the smallest that holds n_elem, at most 64
#define BBT_RANK_ROUTE_AUTO 0
#define BBT_RANK_ROUTE_LDS 1                 // lds wherever the block fits
#define BBT_RANK_ROUTE_GLOBAL 2
#define BBT_RANK_MAD_SCALE 1.482602218505602 // sd = mad * this, for normal noise

#define BBT_RANK_STATS 0                     // what a launch writes
#define BBT_RANK_STANDARDIZE 1
#define BBT_RANK_WHITEN 2

#ifdef __HIPCC__
#define BBT_RANK_HD __host__ __device__
#else
#define BBT_RANK_HD
#endif

// The order: float32 bits -> a key whose unsigned order is the order of the values, -0 just before +0
// (and -NaN first, +NaN last: a flagged block's ranks are computed and dropped).
BBT_RANK_HD inline unsigned rank_key(unsigned bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
BBT_RANK_HD inline unsigned rank_unkey(unsigned key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }
BBT_RANK_HD inline bool rank_not_finite(unsigned bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

// Of a key, the bits above the digit at `shift` of width `bits`: the prefix the descent has fixed.
BBT_RANK_HD inline unsigned rank_fixed_mask(int shift, int bits) {
    return shift + bits >= 32 ? 0u : ~0u << (shift + bits);
}

// One step of the descent: among `nb` counters hist[d * stride], d ascending, the digit that holds rank
// *k of the matching keys.  *k becomes the rank inside that digit; returns the digit, its count in
// *count.  (If the counters hold fewer than *k + 1 keys -- an idle column -- the last digit.)
BBT_RANK_HD inline int rank_pick(const unsigned* hist, int nb, int stride, int* k, int* count) {
    int cum = 0, d = 0, c = 0;
    for (; d < nb; ++d) {
        c = (int)hist[(long long)d * stride];
        if (*k < cum + c) break;
        cum += c;
    }
    if (d == nb) d = nb - 1, cum -= c;
    *k -= cum, *count = c;
    return d;
}

// med = float32((float64(lo) + float64(hi)) * 0.5): exact in float64, rounded once
BBT_RANK_HD inline float rank_mid(float lo, float hi) { return (float)(((double)lo + (double)hi) * 0.5); }

inline long long rank_hist_bytes(int nx, int digit) { return (1ll << digit) * nx * 4; }

// rows of the longest block the lds route takes at tile width nx and this digit width (may be < 2)
inline long long rank_lds_rows(int nx, int digit) {
    const long long left = BBT_RANK_LDS_BYTES - BBT_RANK_MISC_BYTES - rank_hist_bytes(nx, digit);
    return left <= 0 ? 0 : left / (nx * 4ll);
}

struct RankGeo {
    long long n_spec, nbin, n_elem, m, skip;
    long long nblk;              // blocks of a spectrum
    long long len_max;           // rows of the longest block
    int nx, ny;                  // threads along the elements, along the rows
    int digit, route;            // 4 or 8; BBT_RANK_ROUTE_LDS or _GLOBAL
    int mode;                    // BBT_RANK_STATS, _STANDARDIZE or _WHITEN (the launcher's)
    int with_mad;                // stats: the second descent is wanted
    long long n_tile;            // workgroups along the elements
    long long n_wg;              // n_spec * nblk * n_tile
    long long lds_bytes;         // dynamic LDS of a workgroup
    double ratio;                // whiten: mean = med / ratio
};

// 0, or what is wrong with a launch.  width: 16, 32, 64; digit: 4, 8; route: BBT_RANK_ROUTE_* (each 0:
// the default / automatic).  A forced lds route falls back to global where the block does not fit.
inline const char* rank_geo(long long n_spec, long long nbin, long long n_elem, long long m, long long skip, int width,
                            int digit, int route, RankGeo* g) {
    if (m < BBT_RANK_MIN_N || m > BBT_RANK_MAX_N) return "a block must have 2 ... 65536 values";
    if (n_spec < 1 || nbin < 1) return "no rows";
    if (n_elem < 1) return "no elements";
    if (skip < 0 || skip >= nbin) return "skip must be 0 ... nbin - 1";
    if (n_spec > BBT_RANK_MAX_ROWS / nbin) return "more than 2^40 rows in one call";
    if (width != 0 && width != 16 && width != 32 && width != 64) return "the width must be 16, 32 or 64 elements";
    if (digit != 0 && digit != 4 && digit != 8) return "a digit must have 4 or 8 bits";
    if (route < 0 || route > 2) return "the route must be 0 (automatic), 1 (lds) or 2 (global)";
    g->n_spec = n_spec, g->nbin = nbin, g->n_elem = n_elem, g->m = m, g->skip = skip;
    g->nblk = (nbin - skip + m - 1) / m;
    g->len_max = nbin - skip < m ? nbin - skip : m;
    const int digit_lds = digit ? digit : BBT_RANK_DIGIT_LDS;
    if (width == 0) {
        // the widest tile, no wider than the elements need, whose block still fits the LDS; where none
        // does, the narrowest: a long block is walked by one workgroup, and narrow tiles make more of them
        const int cap = n_elem <= 16 ? 16 : n_elem <= 32 ? 32 : 64;
        width = 16;
        if (route != BBT_RANK_ROUTE_GLOBAL)
            for (int w = cap; w > 16; w /= 2)
                if (g->len_max <= rank_lds_rows(w, digit_lds)) {
                    width = w;
                    break;
                }
    }
    g->nx = width, g->ny = BBT_RANK_THREADS / width;
    const bool fits = g->len_max <= rank_lds_rows(width, digit_lds);
    g->route = (route != BBT_RANK_ROUTE_GLOBAL && fits) ? BBT_RANK_ROUTE_LDS : BBT_RANK_ROUTE_GLOBAL;
    g->digit = digit ? digit : (g->route == BBT_RANK_ROUTE_LDS ? BBT_RANK_DIGIT_LDS : BBT_RANK_DIGIT_GLOBAL);
    g->lds_bytes = rank_hist_bytes(width, g->digit) + BBT_RANK_MISC_BYTES +
                   (g->route == BBT_RANK_ROUTE_LDS ? g->len_max * width * 4 : 0);
    g->n_tile = (n_elem + width - 1) / width;
    const long long sb = n_spec * g->nblk;               // (at most 2^40: nblk <= nbin)
    if (sb >= (1ll << 31) || g->n_tile >= (1ll << 31) / sb) return "too many tiles for one launch";
    g->n_wg = sb * g->n_tile;
    g->mode = BBT_RANK_STATS, g->with_mad = 0, g->ratio = 1.;
    return 0;
}

// RobustStandardize's blocks: n_block whole blocks of n rows
inline const char* rank_std_geo(long long n_block, long long n, long long n_elem, int width, int digit, int route,
                                RankGeo* g) {
    if (n < BBT_RANK_MIN_N || n > BBT_RANK_MAX_N) return "a block must have 2 ... 65536 values";
    if (n_block < 1) return "no whole block";
    if (n_block > BBT_RANK_MAX_ROWS / n) return "more than 2^40 rows in one call";
    return rank_geo(1, n_block * n, n_elem, n, 0, width, digit, route, g);
}

// What workgroup `wg` < n_wg owns: rows [row0, row0 + len) of the chunk, elements [e0, e0 + nx) of them
// below n_elem, statistic cell `cell` (of nblk n_spec), and the rows [zero0, zero0 + zero_rows) it sets
// to +0 when whitening.  The kernel and the host check share this.
struct RankOwn {
    long long row0, e0, cell, zero0, zero_rows;
    int len;
};
BBT_RANK_HD inline void rank_own(const RankGeo& g, long long wg, RankOwn* o) {
    const long long tile = wg % g.n_tile, sb = wg / g.n_tile;
    const long long b = sb % g.nblk, s = sb / g.nblk;
    const long long left = g.nbin - g.skip - b * g.m;
    o->e0 = tile * g.nx;
    o->row0 = s * g.nbin + g.skip + b * g.m;
    o->len = (int)(left < g.m ? left : g.m);
    o->cell = sb;
    o->zero0 = s * g.nbin;
    o->zero_rows = b == 0 ? g.skip : 0;
}
