// The resampling rule of Accelerate (periodicity.py) and how k_accel (accel_kernels.hpp) cuts a chunk of
// output rows into workgroups: plain C++, shared by the host launcher and the kernel (the struct is a
// kernel argument) and compiled on its own by tests/accel_geo_check.cpp.  ALL index arithmetic lives
// here: the kernel only moves what these functions address.
//
// THE RULE.  The stream is x[t][e], t a global row, e < n_elem, element fastest; it is cut into blocks
// of n rows, t = q n + i.  Trial j has the factor k_j = a_j / (2 c rate), a float64 made on the host,
// and  out[q n + i][j][e] = x[q n + accel_src(n, k_j, i)][e]  with
//     accel_src(n, k, i) = i + (long long)rint(k * (double)(i * (i - n))):
// i (i - n) in 64-bit integers (exact, below 2^53 in size), ONE double multiply, round half to even, an
// integer add.  There is no floating add next to the multiply, so nothing can be fused with it.
//
// THE BOUND.  |k| n <= 1/4 (accel_factor_ok).  Under it src stays in [0, n - 1], does not decrease with i
// and steps by 0, 1 or 2; and since i (i - n) <= 0, src does not increase with k for a fixed i.  So the
// input rows that output rows i0 ... i1 of one block need, over all trials, are exactly
// [src(i0, k_max), src(i1, k_min)]: accel_window, also across blocks, the blocks between being whole.
//
// THE TILING.  A row of the output is W = n_acc n_elem units wide (a unit is 4 bytes, or 16 on the
// vector path, where n_elem counts units of 16).  Block q is cut into tiles of `rows` adjacent rows from
// its row 0, the last one ragged, so a tile lies in one block; the chunk [out_first, out_first + n_out)
// takes the tiles it touches and clips the first and the last to itself.  A row wider than
// BBT_ACCEL_TILE_UNITS is cut into segments of that many units (then rows = 1).  Workgroup (x, y) owns
// tile x and segment y; its nx lanes run along the row, ny = threads / nx rows are in flight.
// The window route stages rows [lo, hi] of the tile's own window -- one contiguous piece of x -- in LDS
// when it fits (accel_fits, per tile, the same for all threads of the workgroup); otherwise the tile
// reads global memory.  Both routes use the same accel_src, so they give the same bits.
//
// Every buffer index is 64-bit.
#pragma once
#include <cmath>

#define BBT_ACCEL_MIN_N 2
#define BBT_ACCEL_MAX_N (1 << 24)            // rows of a block at most
#define BBT_ACCEL_MAX_TRIALS 4096
#define BBT_ACCEL_MAX_WIDTH (1ll << 28)      // 4-byte values of an output row at most
#define BBT_ACCEL_MAX_VALUES (1ll << 40)     // values of one call, in or out
#define BBT_ACCEL_THREADS 256                // threads of a workgroup
#define BBT_ACCEL_LDS_BYTES 32768            // LDS the window kernel declares
#define BBT_ACCEL_TILE_UNITS 16384           // units of a tile of the output, about
#define BBT_ACCEL_MAX_ROWS 256               // rows of a tile at most
#define BBT_ACCEL_BUDGET (1ll << 29)         // output bytes of a chunk (default of the task)

#ifdef __HIPCC__
#define BBT_ACCEL_HD __host__ __device__
#else
#define BBT_ACCEL_HD
#endif

// the rule
BBT_ACCEL_HD inline long long accel_src(long long n, double k, long long i) {
    const long long p = i * (i - n);
    const double d = k * (double)p;
    return i + (long long)__builtin_rint(d);
}

inline bool accel_factor_ok(long long n, double k) { return std::isfinite(k) && std::fabs(k) * (double)n <= .25; }

// 0, or what is wrong with the sizes of a plan (a static string)
inline const char* accel_sizes(long long n, long long n_elem, long long n_acc) {
    if (n < BBT_ACCEL_MIN_N || n > BBT_ACCEL_MAX_N) return "n must be 2 ... 2^24";
    if (n_acc < 1 || n_acc > BBT_ACCEL_MAX_TRIALS) return "1 ... 4096 trials";
    if (n_elem < 1) return "no elements";
    if (n_elem > BBT_ACCEL_MAX_WIDTH / n_acc) return "an output row of more than 2^28 values";
    return 0;
}

// The input rows [*lo, *hi] (global, inclusive) that output rows g0 <= g1 (global, inclusive) need.
inline void accel_window(long long n, double k_min, double k_max, long long g0, long long g1, long long* lo,
                         long long* hi) {
    const long long q0 = g0 / n, q1 = g1 / n;
    *lo = q0 * n + accel_src(n, k_max, g0 - q0 * n);
    *hi = q1 * n + accel_src(n, k_min, g1 - q1 * n);
}

struct AccelGeo {
    long long n, n_elem, n_acc, W;     // rows of a block; units of a sample; trials; units of an output row
    long long in_first, n_in;          // the input piece: global rows in_first ... in_first + n_in - 1
    long long out_first, n_out;        // the chunk: global rows
    double k_min, k_max;
    int rows;                          // rows of a tile
    long long tpb;                     // tiles of a block
    long long tile0, n_tile;           // the first tile of the chunk (q tpb + u) and how many
    long long ws, n_seg;               // units of a segment of a row, and how many segments
    int nx, log2nx, ny;                // lanes along the row (a power of two), rows in flight
    int lds_units;                     // units the LDS of the window kernel holds
    int unit;                          // bytes of a unit: 4 or 16
};

// rows of a tile for rows of W units
inline int accel_rows(long long W) {
    const long long r = BBT_ACCEL_TILE_UNITS / W;
    return (int)(r < 1 ? 1 : r > BBT_ACCEL_MAX_ROWS ? BBT_ACCEL_MAX_ROWS : r);
}

// 0, or what is wrong; the geometry of one launch.  `unit` is 4 or 16 (bytes); n_elem4 counts 4-byte values.
inline const char* accel_geo(long long n, long long n_elem4, long long n_acc, int unit, double k_min, double k_max,
                             long long in_first, long long n_in, long long out_first, long long n_out, AccelGeo* g) {
    const char* err = accel_sizes(n, n_elem4, n_acc);
    if (err) return err;
    if (unit != 4 && !(unit == 16 && n_elem4 % 4 == 0)) return "a 16-byte unit needs n_elem % 4 == 0";
    if (!accel_factor_ok(n, k_min) || !accel_factor_ok(n, k_max) || k_min > k_max) return "a factor beyond |k| n <= 1/4";
    if (out_first < 0 || n_out < 1 || in_first < 0 || n_in < 1) return "no rows";
    if (n_out > BBT_ACCEL_MAX_VALUES / (n_elem4 * n_acc) || n_in > BBT_ACCEL_MAX_VALUES / n_elem4 ||
        out_first > BBT_ACCEL_MAX_VALUES - n_out || in_first > BBT_ACCEL_MAX_VALUES - n_in)
        return "more than 2^40 values in one call";
    long long lo, hi;
    accel_window(n, k_min, k_max, out_first, out_first + n_out - 1, &lo, &hi);
    if (lo < in_first || hi >= in_first + n_in) return "the input piece does not cover the window of the rows";
    g->n = n, g->n_elem = n_elem4 / (unit / 4), g->n_acc = n_acc, g->W = g->n_elem * n_acc;
    g->in_first = in_first, g->n_in = n_in, g->out_first = out_first, g->n_out = n_out;
    g->k_min = k_min, g->k_max = k_max;
    g->rows = accel_rows(g->W);
    g->tpb = (n + g->rows - 1) / g->rows;
    const long long q0 = out_first / n, last = out_first + n_out - 1, q1 = last / n;
    g->tile0 = q0 * g->tpb + (out_first - q0 * n) / g->rows;
    g->n_tile = q1 * g->tpb + (last - q1 * n) / g->rows - g->tile0 + 1;
    g->ws = g->W < BBT_ACCEL_TILE_UNITS ? g->W : BBT_ACCEL_TILE_UNITS;
    g->n_seg = (g->W + g->ws - 1) / g->ws;
    if (g->n_tile >= (1ll << 31) || g->n_seg > 65535) return "too many workgroups for one launch";
    for (g->log2nx = 0; (1 << g->log2nx) < BBT_ACCEL_THREADS && (1ll << g->log2nx) < g->ws;) ++g->log2nx;
    g->nx = 1 << g->log2nx, g->ny = BBT_ACCEL_THREADS / g->nx;
    g->lds_units = BBT_ACCEL_LDS_BYTES / unit, g->unit = unit;
    return 0;
}

// Tile x of the launch: its block q, its rows i0 <= i < i1 of that block, and the rows lo ... hi of the
// block that they need.
struct AccelTile {
    long long q, i0, i1, lo, hi;
};
BBT_ACCEL_HD inline void accel_tile(const AccelGeo& g, long long x, AccelTile* t) {
    const long long tile = g.tile0 + x;
    t->q = tile / g.tpb;
    const long long u = tile - t->q * g.tpb, base = t->q * g.n;
    long long i0 = u * g.rows, i1 = i0 + g.rows;
    if (i1 > g.n) i1 = g.n;
    if (i0 < g.out_first - base) i0 = g.out_first - base;
    if (i1 > g.out_first + g.n_out - base) i1 = g.out_first + g.n_out - base;
    t->i0 = i0, t->i1 = i1;
    t->lo = accel_src(g.n, g.k_max, i0);
    t->hi = accel_src(g.n, g.k_min, i1 - 1);
}
// units of the tile's window, and whether the LDS holds them
BBT_ACCEL_HD inline long long accel_window_units(const AccelGeo& g, const AccelTile& t) {
    return (t.hi - t.lo + 1) * g.n_elem;
}
BBT_ACCEL_HD inline bool accel_fits(const AccelGeo& g, const AccelTile& t) {
    return accel_window_units(g, t) <= g.lds_units;
}
// the units w0 <= w < w1 of a row that segment y holds
BBT_ACCEL_HD inline void accel_segment(const AccelGeo& g, long long y, long long* w0, long long* w1) {
    *w0 = y * g.ws;
    *w1 = *w0 + g.ws < g.W ? *w0 + g.ws : g.W;
}
// the unit of the input piece that holds element e of row s of block q
BBT_ACCEL_HD inline long long accel_in_index(const AccelGeo& g, long long q, long long s, long long e) {
    return (q * g.n + s - g.in_first) * g.n_elem + e;
}
// the LDS unit of the same, the window staged from row t.lo on
BBT_ACCEL_HD inline int accel_lds_index(const AccelGeo& g, const AccelTile& t, long long s, long long e) {
    return (int)((s - t.lo) * g.n_elem + e);
}
// the unit of the output chunk of unit w of row i of block q
BBT_ACCEL_HD inline long long accel_out_index(const AccelGeo& g, long long q, long long i, long long w) {
    return (q * g.n + i - g.out_first) * g.W + w;
}

// Does the window of the tile that holds global row r of the chunk fit the LDS?
inline bool accel_row_fits(const AccelGeo& g, long long r) {
    const long long q = r / g.n;
    AccelTile t;
    accel_tile(g, q * g.tpb + (r - q * g.n) / g.rows - g.tile0, &t);
    return accel_fits(g, t);
}

// BBT_ACCEL_ROUTE: 0 automatic, 1 the window wherever it fits, 2 direct.  What a launch runs: 1 or 2.
// A row of the input wider than half the LDS can never be staged with its neighbour, and a segment of a
// row does not know which elements it needs: direct.
// The automatic rule, from the MI355X rows of profiles/accel_bench.jsonl (times in device copies of the
// output, window | direct): samples of 32 bytes 0.45 | 0.68; samples of 8 bytes 0.82 | 0.78; samples of
// 256 bytes, whose windows do not fit where the shifts are largest, 0.72 | 0.69.  So: the window if a
// sample has at least 16 bytes AND the widest windows of the chunk -- those of the tiles nearest the
// middle of a block -- fit; else direct, which then does not pay for LDS it would not use.
inline int accel_route(int asked, const AccelGeo& g) {
    if (asked == 2 || 2 * g.n_elem > g.lds_units || g.n_seg > 1) return 2;
    if (asked == 1) return 1;
    if (g.n_elem * g.unit < 16) return 2;
    const long long last = g.out_first + g.n_out - 1, q0 = g.out_first / g.n;
    for (long long q = q0; q <= q0 + 1; ++q) {
        long long r = q * g.n + g.n / 2;                 // the middle of block q, or the chunk's row nearest to it
        if (q > q0 && r > last) break;
        r = r < g.out_first ? g.out_first : r > last ? last : r;
        if (!accel_row_fits(g, r)) return 2;
    }
    return 1;
}
