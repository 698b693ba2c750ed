// How the kernels of rmed_kernels.hpp cut one chunk of RunningMedian / Detrend (search.py) into
// workgroups, which rows of the stream a run of output needs, the integer rules of the interpolation and
// the two selection methods themselves: plain C++, shared by the host launcher and the kernels (RmedGeo
// is a kernel argument) and compiled on its own by tests/rmed_geo_check.cpp.  The order of the values
// and the median of a window are rank_geo.hpp's (rank_key, rank_not_finite, rank_mid), unchanged.
//
// The stream is x[i][e], i < N samples, e < n_elem, float32, element fastest.  S = scrunch, w = width, h =
// w / 2, R = N / S rows of the scrunched series c[r][e]; m[r][e] is the median of c[max(0, r - h) ...
// min(R - 1, r + h)][e]: windows are clipped at the two ends of the STREAM only, so a call is told where
// in the stream its rows lie.  Output sample i takes its baseline from m[r0] and m[r0 + 1] (rmed_lerp).
//
// A call makes output samples [out_first, out_first + n_out), both multiples of S: scrunch rows [ro0,
// ro1).  For S > 1 these read m[max(0, ro0 - 1) ... min(R, ro1 + 1)) -- the interpolation neighbours --
// and for S = 1 just m[ro0 ... ro1); medians [m0, m1) read c[max(0, m0 - h) ... min(R, m1 + h)) (rmed_need).
// The input of the call must hold those rows of c, whole.
//
// The selection kernel: a workgroup of 256 threads owns nx adjacent elements of a run of `run`
// consecutive medians, threads (tx, ty), ty < ny = 256 / nx, lanes along the elements.  It stages the
// keys of the run's rows and of the up to h rows on either side, [st0, st0 + n_st) of the stream, in LDS:
// s_key[(row - st0) * nx + tx], at most BBT_RANK_LDS_BYTES = 72 KiB, so that two workgroups fit a CU.
// Thread ty then walks medians row0 + ty * per ... of its column, per = ceil(len / ny).  Workgroup wg =
// run_index * n_tile + tile.
//
// Two methods, one result (a selection is exact).  radix: every median is a fresh most-significant-digit
// descent over the window's keys, digits of 2 bits, 16 passes over the window.  walk: only the first
// median of a thread and the medians of clipped windows are; between two full windows the thread keeps
// the median as the element (key, row) of rank h in the strict order (key, row), and as one element
// leaves and one enters it stays or moves to its neighbour in that order, found by one pass (rmed_step).
//
// Every index into the chunk is 64-bit; only the per-axis counts below are bounded.
#pragma once

#include "rank_geo.hpp"

#define BBT_RMED_THREADS 256
#define BBT_RMED_MIN_WIDTH 3
#define BBT_RMED_MAX_WIDTH 1023
#define BBT_RMED_MAX_SCRUNCH 4096
#define BBT_RMED_RUN 128                     // medians of a workgroup unless BBT_RMED_ROWS says otherwise
#define BBT_RMED_SEG 32                      // samples of a segment of the scrunch's two-level sum (BBT_SPS_SEG)
#define BBT_RMED_MAX_ROWS (1ll << 40)        // samples of a stream
#define BBT_RMED_SELECT_RADIX 1
#define BBT_RMED_SELECT_WALK 2
#define BBT_RMED_BASELINE 0                  // what a call writes: the baseline b
#define BBT_RMED_DETREND 1                   // x - b

// rows of keys a workgroup of tile width nx can stage
inline long long rmed_lds_rows(int nx) { return BBT_RANK_LDS_BYTES / (nx * 4ll); }

// Sample i of the stream: its baseline is m[*r0] if *q <= 0, m[*r0 + 1] if *q >= 2 S, and else m[r0] + (m[r0
// + 1] - m[r0]) * float32(double(q) / double(2 S)).  j = 2 i + 1 - S is twice the distance of the sample
// from the centre of scrunch row 0, in half samples.
BBT_RANK_HD inline void rmed_lerp(long long i, long long S, long long R, long long* r0, long long* q) {
    if (R < 2) {
        *r0 = 0, *q = 0;
        return;
    }
    const long long j = 2 * i + 1 - S, two = 2 * S;
    long long f = j >= 0 ? j / two : -((-j + two - 1) / two);      // floor
    f = f < 0 ? 0 : f > R - 2 ? R - 2 : f;
    *r0 = f, *q = j - two * f;
}

// The medians [*m0, *m1) and the scrunch rows [*c0, *c1) that output scrunch rows [ro0, ro1) need.
BBT_RANK_HD inline void rmed_need(long long S, long long h, long long R, long long ro0, long long ro1, long long* m0,
                                  long long* m1, long long* c0, long long* c1) {
    const long long nb = S > 1 ? 1 : 0;
    *m0 = ro0 - nb < 0 ? 0 : ro0 - nb;
    *m1 = ro1 + nb > R ? R : ro1 + nb;
    *c0 = *m0 - h < 0 ? 0 : *m0 - h;
    *c1 = *m1 + h > R ? R : *m1 + h;
}

// -- the selection ---------------------------------------------------------------------------------------
// (key, t): the strict order of the elements of a window, t the index of the row
typedef unsigned long long rmed_ord;
BBT_RANK_HD inline rmed_ord rmed_ord_of(unsigned key, int t) { return ((rmed_ord)key << 32) | (unsigned)t; }

// The median of the keys key_at(t), a <= t < b, b - a = L >= 1: *lo the key of rank (L - 1) / 2, *hi that of
// rank L / 2, *pos the row of the element of rank (L - 1) / 2 in the order (key, t).
template <class KeyAt>
BBT_RANK_HD inline void rmed_select(KeyAt key_at, int a, int b, unsigned* lo, unsigned* hi, int* pos) {
    const int L = b - a;
    int k = (L - 1) >> 1, cnt = L;
    unsigned prefix = 0;
    for (int shift = 30; shift >= 0; shift -= 2) {
        const unsigned fixed = rank_fixed_mask(shift, 2);
        int c0 = 0, c1 = 0, c2 = 0;
        for (int t = a; t < b; ++t) {
            const unsigned key = key_at(t);
            if (((key ^ prefix) & fixed) == 0u) {
                const unsigned d = (key >> shift) & 3u;
                c0 += d == 0u, c1 += d == 1u, c2 += d == 2u;
            }
        }
        unsigned d;
        if (k < c0) d = 0u, cnt = c0;
        else if (k < c0 + c1) d = 1u, k -= c0, cnt = c1;
        else if (k < c0 + c1 + c2) d = 2u, k -= c0 + c1, cnt = c2;
        else d = 3u, k -= c0 + c1 + c2, cnt -= c0 + c1 + c2;
        prefix |= d << shift;
    }
    // prefix is lo's key, cnt keys equal it, and lo is the k-th of them by row
    unsigned above = 0xffffffffu;
    int seen = 0, at = a;
    for (int t = a; t < b; ++t) {
        const unsigned key = key_at(t);
        if (key == prefix) {
            if (seen == k) at = t;
            ++seen;
        } else if (key > prefix && key < above) {
            above = key;
        }
    }
    *lo = prefix, *pos = at;
    *hi = (!(L & 1) && k + 1 >= cnt) ? above : prefix;
}

// The window moves from rows [a, b) to [a + 1, b + 1), b - a odd: (*key, *pos), the element of rank (b - a) / 2
// of the old window in the order (key, t), becomes that of the new one.
template <class KeyAt>
BBT_RANK_HD inline void rmed_step(KeyAt key_at, int a, int b, unsigned* key, int* pos) {
    const rmed_ord med = rmed_ord_of(*key, *pos);
    const rmed_ord out = rmed_ord_of(key_at(a), a), in = rmed_ord_of(key_at(b), b);
    int move = 0;                                  // +1: to the next element above, -1: below
    if (out == med) move = in > med ? 1 : -1;
    else if (out < med && in > med) move = 1;
    else if (out > med && in < med) move = -1;
    if (move == 0) return;
    rmed_ord best = in;                            // (the entering element is on the side the median moves to)
    if (move > 0) {
        for (int t = a + 1; t < b; ++t) {
            const rmed_ord o = rmed_ord_of(key_at(t), t);
            if (o > med && o < best) best = o;
        }
    } else {
        for (int t = a + 1; t < b; ++t) {
            const rmed_ord o = rmed_ord_of(key_at(t), t);
            if (o < med && o > best) best = o;
        }
    }
    *key = (unsigned)(best >> 32), *pos = (int)(unsigned)best;
}

// -- the tiling --------------------------------------------------------------------------------------------
struct RmedGeo {
    long long S, w, h, R, n_elem;
    long long in_first, n_in;        // the samples of the stream the input holds
    long long out_first, n_out;      // the samples of the stream the call makes
    long long ro0, ro1;              // their scrunch rows
    long long m0, m1;                // the medians they read
    long long c0, c1;                // the scrunch rows those read
    int nx, ny;                      // threads along the elements, along the rows
    int run;                         // medians of a workgroup
    int method;                      // BBT_RMED_SELECT_*
    int mode;                        // BBT_RMED_BASELINE or _DETREND (the launcher's)
    long long n_tile, n_run, n_wg;
    long long lds_bytes;             // dynamic LDS of a workgroup
    long long scratch_bytes;         // c[c0 ... c1) and m[m0 ... m1) for S > 1, else none
};

inline const char* rmed_sizes(long long width, long long scrunch, long long n_elem) {
    if (width < BBT_RMED_MIN_WIDTH || width > BBT_RMED_MAX_WIDTH || !(width & 1)) return "the width must be odd, 3 ... 1023";
    if (scrunch < 1 || scrunch > BBT_RMED_MAX_SCRUNCH) return "scrunch must be 1 ... 4096";
    if (n_elem < 1 || n_elem >= (1ll << 31)) return "no elements, or 2^31 and more";
    return 0;
}

// 0, or what is wrong with a call.  tile: 16, 32, 64 (halved while its LDS rows leave the window a run of
// less than 16); rows: the medians of a workgroup at most; method: BBT_RMED_SELECT_* (each 0: the default
// / automatic).
inline const char* rmed_geo(long long width, long long scrunch, long long n_elem, long long n_rows, long long in_first,
                            long long n_in, long long out_first, long long n_out, int tile, int rows, int method,
                            RmedGeo* g) {
    const char* err = rmed_sizes(width, scrunch, n_elem);
    if (err) return err;
    const long long S = scrunch, h = width / 2, R = n_rows;
    if (R < 1 || R > BBT_RMED_MAX_ROWS / S) return "the stream must have 1 ... 2^40 / scrunch rows";
    if (tile != 0 && tile != 16 && tile != 32 && tile != 64) return "the tile must be 16, 32 or 64 elements";
    if (rows < 0 || method < 0 || method > 2) return "the method must be 0 (automatic), 1 (radix) or 2 (walk)";
    if (out_first < 0 || n_out < S || out_first % S || n_out % S) return "the output must be whole scrunch rows, one at least";
    if (out_first > R * S - n_out) return "the output runs beyond the stream";
    if (in_first < 0 || in_first % S || n_in < 0 || n_in > BBT_RMED_MAX_ROWS) return "the input must begin at a scrunch row";
    g->S = S, g->w = width, g->h = h, g->R = R, g->n_elem = n_elem;
    g->in_first = in_first, g->n_in = n_in, g->out_first = out_first, g->n_out = n_out;
    g->ro0 = out_first / S, g->ro1 = (out_first + n_out) / S;
    rmed_need(S, h, R, g->ro0, g->ro1, &g->m0, &g->m1, &g->c0, &g->c1);
    if (g->c0 * S < in_first || g->c1 * S > in_first + n_in) return "the input does not hold the rows the output needs";
    // measured (profiles/rmed_sweep.jsonl): the narrowest tile and a run of 128 beat wider tiles and the longest
    // run the LDS holds by 1.7 times -- a small LDS footprint puts more workgroups on a CU
    if (tile == 0) tile = 16;
    while (tile > 16 && rmed_lds_rows(tile) - 2 * h < 16) tile /= 2;      // (a forced tile too wide for the window)
    g->nx = tile, g->ny = BBT_RMED_THREADS / tile;
    long long run = rmed_lds_rows(tile) - 2 * h;          // (1152 - 1022 = 130 at the least)
    if (rows == 0 && run > BBT_RMED_RUN) run = BBT_RMED_RUN;
    if (rows > 0 && rows < run) run = rows;
    if (run > g->m1 - g->m0) run = g->m1 - g->m0;
    g->run = (int)run;
    g->method = method ? method : BBT_RMED_SELECT_WALK;
    g->mode = BBT_RMED_BASELINE;
    g->n_tile = (n_elem + tile - 1) / tile;
    g->n_run = (g->m1 - g->m0 + run - 1) / run;
    if (g->n_run >= (1ll << 31) || g->n_tile >= (1ll << 31) / g->n_run) return "too many tiles for one launch";
    g->n_wg = g->n_run * g->n_tile;
    g->lds_bytes = (run + 2 * h) * tile * 4;
    if ((g->c1 - g->c0) * S > (1ll << 61) / (n_elem * 4)) return "too many values in one call";
    g->scratch_bytes = S > 1 ? ((g->c1 - g->c0) + (g->m1 - g->m0)) * n_elem * 4 : 0;
    return 0;
}

// What workgroup `wg` < n_wg owns: medians [row0, row0 + len) of the stream, elements [e0, e0 + nx) of them
// below n_elem, and the rows [st0, st0 + n_st) it stages; thread row ty walks medians [row0 + ty per,
// min(row0 + len, row0 + (ty + 1) per)).  The kernel and the host check share this.
struct RmedOwn {
    long long row0, e0, st0;
    int len, n_st, per;
};
BBT_RANK_HD inline void rmed_own(const RmedGeo& g, long long wg, RmedOwn* o) {
    const long long tile = wg % g.n_tile, ri = wg / g.n_tile;
    o->e0 = tile * g.nx;
    o->row0 = g.m0 + ri * g.run;
    const long long left = g.m1 - o->row0;
    o->len = (int)(left < g.run ? left : g.run);
    o->st0 = o->row0 - g.h < 0 ? 0 : o->row0 - g.h;
    const long long st1 = o->row0 + o->len + g.h > g.R ? g.R : o->row0 + o->len + g.h;
    o->n_st = (int)(st1 - o->st0);
    o->per = (o->len + g.ny - 1) / g.ny;
}
