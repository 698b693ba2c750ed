// How k_lspec_first / k_lspec_last (lspec_kernels.hpp) cut one long transform of LongSpectra
// (periodicity.py) into workgroups: plain C++, shared by the host launcher and the kernels (the struct
// is a kernel argument) and compiled on its own by tests/lspec_geo_check.cpp.  ALL index arithmetic of
// the two passes lives here: the kernels only move and combine what these functions address.
//
// The input of one transform is x[t][e], t < n samples, e < n_elem, float32, element fastest.  Columns
// (2p, 2p + 1) are column pair p, one complex stream z = x[2p] + i x[2p + 1]; an odd last column pairs
// with zeros.  n = n1 n2, t = n2 a + b, k = k1 + n1 k2 (four-step).  A launch takes P adjacent pairs from
// p0 on; its scratch is S[k1][b][pl], pl < P fastest, 8 n bytes a pair.
//
// Pass 1.  The n2 P columns (b, pl) of a launch are numbered col = b P + pl; a workgroup owns c1 adjacent
// ones (c1 divides n2, so there are no ragged workgroups) and transforms them over a in LDS, in place,
// decimation in frequency: the value of k1 is left at position brev(k1).  It is multiplied by
// W_n^(b k1) and written to S[k1][col].
//
// Pass 2.  Workgroup (h, pt), h < n1 / 2, owns rows (k1, n1 - k1) = lspec_row(h, 0 / 1) -- h = 0: the two
// rows 0 and n1 / 2 that pair with themselves -- of cp adjacent pairs of the launch (the last tile may
// be ragged), transforms them over b and so holds Z[k] next to Z[n - k] (lspec_partner).  It untangles
// the two real columns, detects them and writes (or adds to) bins k <= n / 2 of out[k][e].
//
// Every global index is 64-bit; everything inside one transform of one pair (b k1 < n <= 2^22) is int.
#pragma once

#define BBT_LSPEC_THREADS 1024               // threads of a workgroup (default): 256, 512 or 1024
#define BBT_LSPEC_MAX_THREADS 1024
#define BBT_LSPEC_MIN_LOG2 15                // the shortest transform, 2^15
#define BBT_LSPEC_MAX_LOG2 22                // the longest, 2^22
#define BBT_LSPEC_LDS_CELLS 8192             // complex cells of a workgroup's LDS: 64 KiB
#define BBT_LSPEC_MAX_COLS 32                // columns of a pass-1 workgroup at most
#define BBT_LSPEC_MAX_PAIRS 16               // column pairs of a pass-2 workgroup at most
#define BBT_LSPEC_TW_LO_LOG2 11              // W_n^m = hi[m >> 11] lo[m & 2047], both tables from float64
#define BBT_LSPEC_MAX_STACK (1 << 20)
#define BBT_LSPEC_MAX_VALUES (1ll << 40)     // values of one call, in or out
#define BBT_LSPEC_BUDGET (1ll << 29)         // bytes of scratch of a launch (default)

#ifdef __HIPCC__
#define BBT_LSPEC_HD __host__ __device__
#else
#define BBT_LSPEC_HD
#endif

struct LspecGeo {
    long long n, n_elem, n_pair;       // samples of a transform; columns; ceil(n_elem / 2)
    long long p0, P;                   // the launch: pairs p0 ... p0 + P - 1
    int log2n, log2n1, log2n2, n1, n2;
    int c1, log2c1;                    // columns of a pass-1 workgroup
    int cp, log2cp;                    // pairs of a pass-2 workgroup (2 cp LDS columns)
    long long n_tile;                  // pass-2 workgroups along the pairs
    long long n_wg1, n_wg2;
};

// 0, or what is wrong with the sizes of a plan (a static string)
inline const char* lspec_sizes(long long n, long long stack, long long n_elem) {
    if (n < (1ll << BBT_LSPEC_MIN_LOG2) || n > (1ll << BBT_LSPEC_MAX_LOG2) || (n & (n - 1)))
        return "n must be a power of two, 2^15 ... 2^22";
    if (stack < 1 || stack > BBT_LSPEC_MAX_STACK) return "stack must be 1 ... 2^20";
    if (n_elem < 1) return "no elements";
    if (n_elem > BBT_LSPEC_MAX_VALUES / (n * stack)) return "more than 2^40 values in one spectrum";
    return 0;
}

// The pairs one launch takes under a scratch budget in bytes: as many as fit, one at least.
inline long long lspec_pairs_per_launch(long long n, long long n_elem, long long budget) {
    const long long n_pair = (n_elem + 1) / 2;
    long long per = budget / (8 * n);
    if (per < 1) per = 1;
    return per < n_pair ? per : n_pair;
}

inline long long lspec_n_launch(long long n_elem, long long per) { return ((n_elem + 1) / 2 + per - 1) / per; }

// 0, or what is wrong; fills the geometry of launch i of lspec_n_launch(n_elem, per)
inline const char* lspec_geo(long long n, long long n_elem, long long per, long long i, LspecGeo* g) {
    const char* err = lspec_sizes(n, 1, n_elem);
    if (err) return err;
    g->n = n, g->n_elem = n_elem, g->n_pair = (n_elem + 1) / 2;
    if (per < 1 || i < 0 || i * per >= g->n_pair) return "no such launch";
    g->p0 = i * per;
    g->P = g->n_pair - g->p0 < per ? g->n_pair - g->p0 : per;
    int lg = 0;
    while ((1ll << lg) < n) ++lg;
    g->log2n = lg, g->log2n1 = lg / 2, g->log2n2 = lg - lg / 2;
    g->n1 = 1 << g->log2n1, g->n2 = 1 << g->log2n2;
    g->c1 = BBT_LSPEC_LDS_CELLS / g->n1 < BBT_LSPEC_MAX_COLS ? BBT_LSPEC_LDS_CELLS / g->n1 : BBT_LSPEC_MAX_COLS;
    g->cp = BBT_LSPEC_LDS_CELLS / g->n2 / 2 < BBT_LSPEC_MAX_PAIRS ? BBT_LSPEC_LDS_CELLS / g->n2 / 2 : BBT_LSPEC_MAX_PAIRS;
    for (g->log2c1 = 0; (1 << g->log2c1) < g->c1;) ++g->log2c1;
    for (g->log2cp = 0; (1 << g->log2cp) < g->cp;) ++g->log2cp;
    g->n_tile = (g->P + g->cp - 1) / g->cp;
    if (g->P >= (1ll << 31) * g->c1 / g->n2 || g->n_tile >= (1ll << 31) / (g->n1 / 2)) return "too many pairs for one launch";
    g->n_wg1 = g->n2 * g->P / g->c1;
    g->n_wg2 = (long long)(g->n1 / 2) * g->n_tile;
    return 0;
}

// bits < 32 of v reversed within the low `bits` bits
BBT_LSPEC_HD inline int lspec_brev(int v, int bits) {
    unsigned x = (unsigned)v;
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    x = (x >> 16) | (x << 16);
    return (int)(x >> (32 - bits));
}

// -- pass 1 ---------------------------------------------------------------------------------------------
// Column slot c < c1 of workgroup wg: b and the launch's pair pl.
struct LspecCol {
    long long col;
    int b;
    long long pl;
};
BBT_LSPEC_HD inline void lspec_col(const LspecGeo& g, long long wg, int c, LspecCol* o) {
    o->col = wg * g.c1 + c;
    o->b = (int)(o->col / g.P);
    o->pl = o->col - (long long)o->b * g.P;
}
// The float of x (n rows of n_elem) that holds part `half` (0: real, 1: imaginary) of sample a of the
// column, or -1 for the zero partner of an odd last column.
BBT_LSPEC_HD inline long long lspec_in_index(const LspecGeo& g, const LspecCol& o, int a, int half) {
    const long long e = 2 * (g.p0 + o.pl) + half;
    return e < g.n_elem ? ((long long)a * g.n2 + o.b) * g.n_elem + e : -1;
}
// where sample a of slot c sits in LDS before the transform, and where the value of k1 sits after it
BBT_LSPEC_HD inline int lspec_lds1(const LspecGeo& g, int pos, int c) { return (pos << g.log2c1) + c; }
BBT_LSPEC_HD inline int lspec_pos1(const LspecGeo& g, int k1) { return lspec_brev(k1, g.log2n1); }
// the exponent m of the twiddle W_n^m, already below n
BBT_LSPEC_HD inline int lspec_tw_exp(const LspecGeo& g, int b, int k1) { return b * k1; }
// the scratch cell (complex) of (k1, col)
BBT_LSPEC_HD inline long long lspec_scratch(const LspecGeo& g, int k1, long long col) {
    return (long long)k1 * g.n2 * g.P + col;
}

// -- pass 2 ---------------------------------------------------------------------------------------------
// Workgroup wg: the row pair h and the first pair of the tile.
BBT_LSPEC_HD inline int lspec_h(const LspecGeo& g, long long wg) { return (int)(wg / g.n_tile); }
BBT_LSPEC_HD inline long long lspec_pl0(const LspecGeo& g, long long wg) { return (wg % g.n_tile) * g.cp; }
// the row k1 of side ri (0, 1) of row pair h
BBT_LSPEC_HD inline int lspec_row(const LspecGeo& g, int h, int ri) {
    return h == 0 ? (ri ? g.n1 / 2 : 0) : (ri ? g.n1 - h : h);
}
// LDS column of (side ri, pair slot s < cp): 2 cp columns
BBT_LSPEC_HD inline int lspec_lds2(const LspecGeo& g, int pos, int ri, int s) {
    return (((pos << 1) + ri) << g.log2cp) + s;
}
BBT_LSPEC_HD inline int lspec_pos2(const LspecGeo& g, int k2) { return lspec_brev(k2, g.log2n2); }
// The partner of k = row(h, ri) + n1 k2, that is n - k (n -> 0), as (side, k2) of the same workgroup.
BBT_LSPEC_HD inline void lspec_partner(const LspecGeo& g, int h, int ri, int k2, int* rj, int* k2j) {
    if (h == 0) {
        *rj = ri;
        *k2j = ri ? g.n2 - 1 - k2 : (g.n2 - k2) & (g.n2 - 1);
    } else {
        *rj = 1 - ri;
        *k2j = g.n2 - 1 - k2;
    }
}
// Does side ri of row pair h write bin k2 -- is k = row + n1 k2 <= n / 2?  k2 runs to n2 / 2 inclusive.
BBT_LSPEC_HD inline bool lspec_writes(const LspecGeo& g, int h, int ri, int k2) {
    return k2 < g.n2 / 2 || (k2 == g.n2 / 2 && h == 0 && ri == 0);
}
BBT_LSPEC_HD inline long long lspec_bin(const LspecGeo& g, int h, int ri, int k2) {
    return lspec_row(g, h, ri) + (long long)g.n1 * k2;
}
// the float of out (n / 2 + 1 rows of n_elem) of bin k, pair pl, part half; -1: the zero partner's
BBT_LSPEC_HD inline long long lspec_out_index(const LspecGeo& g, long long k, long long pl, int half) {
    const long long e = 2 * (g.p0 + pl) + half;
    return e < g.n_elem ? k * g.n_elem + e : -1;
}
