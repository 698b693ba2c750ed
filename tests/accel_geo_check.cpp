// Host walk of csrc/accel_geo.hpp, the rule and the index arithmetic of Accelerate's kernel, built with
// -fsanitize=address,undefined by tests/test_accel_host.py.
//
//   accel_geo_check walk N_ROWS N N_ELEM UNIT ROUTE CHUNK A K_0 ... K_{A-1}  [N_ROWS ...]
//       A stream of N_ROWS rows of N_ELEM float32 is resampled in blocks of N with the A factors and
//       cut into launches of CHUNK output rows, as the task cuts it; every launch gets exactly the
//       window of its rows as its input piece.  UNIT is 4 or 16 (bytes a lane moves), ROUTE is
//       BBT_ACCEL_ROUTE.  One JSON line per group with the geometry of the first launch and "walk": 0 if,
//       in every launch walked (all of them if the call is small, else the first and the last; of a
//       launch too large to walk whole, its first and last two tiles), the loops of k_accel, thread by
//       thread, write every output unit exactly once, read only rows inside the tile's window, which lies
//       inside the piece, index the LDS only below what the kernel declares, and every tile lies within
//       one block.  A line with "error" for what the library refuses.
//   accel_geo_check maps N FILE K_0 ...
//       writes accel_src(N, K_j, i), i < N, as raw int64 (A, N) into FILE.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "accel_geo.hpp"

static int fail(const char* what, long long a, long long b) {
    std::fprintf(stderr, "accel_geo_check: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

struct Seen {
    long long max_in = -1, max_out = -1, staged = 0, direct = 0, tiles = 0, launches = 0;
    AccelGeo first = {};
};

static const long long WHOLE = 1ll << 25;          // units of a launch walked whole

// 0 if the launch of output rows [out_first, out_first + n_out) is sound
static int walk_launch(long long n, long long n_elem4, int unit, int asked, const std::vector<double>& k,
                       long long out_first, long long n_out, Seen* seen, const char** refused) {
    double k_min = k[0], k_max = k[0];
    for (double v : k) k_min = v < k_min ? v : k_min, k_max = v > k_max ? v : k_max;
    long long lo, hi;
    accel_window(n, k_min, k_max, out_first, out_first + n_out - 1, &lo, &hi);
    AccelGeo g = {};
    *refused = accel_geo(n, n_elem4, (long long)k.size(), unit, k_min, k_max, lo, hi - lo + 1, out_first, n_out, &g);
    if (*refused) return 0;
    if (seen->launches++ == 0) seen->first = g;
    const int route = accel_route(asked, g);
    const long long out_units = g.n_out * g.W, in_units = g.n_in * g.n_elem;
    if (g.nx * g.ny != BBT_ACCEL_THREADS || (1 << g.log2nx) != g.nx || g.rows < 1 || g.rows > BBT_ACCEL_MAX_ROWS ||
        g.ws < 1 || g.ws * g.n_seg < g.W || g.ws * (g.n_seg - 1) >= g.W || g.lds_units * unit != BBT_ACCEL_LDS_BYTES ||
        g.W != g.n_elem * g.n_acc || g.n_elem * (unit / 4) != n_elem4)
        return fail("bad geometry", g.nx, g.rows);
    const bool whole = out_units <= WHOLE;
    std::vector<unsigned char> written(whole ? (size_t)out_units : 0);
    long long rows_seen = 0, next_row = out_first;
    for (long long x = 0; x < g.n_tile; ++x) {
        if (!whole && x >= 2 && x + 2 < g.n_tile) continue;
        AccelTile t;
        accel_tile(g, x, &t);
        ++seen->tiles;
        // one block, inside the chunk, adjacent to the tile before
        if (t.i0 < 0 || t.i0 >= t.i1 || t.i1 > n || t.i1 - t.i0 > g.rows) return fail("tile outside its block", t.i0, t.i1);
        if (t.q * n + t.i0 < out_first || t.q * n + t.i1 > out_first + n_out) return fail("tile outside the chunk", x, t.q);
        if (whole || x < 2) {
            if (t.q * n + t.i0 != next_row) return fail("tiles do not follow each other", x, next_row);
            next_row = t.q * n + t.i1;
        }
        rows_seen += t.i1 - t.i0;
        // the window of the tile inside the block and inside the piece
        if (t.lo < 0 || t.hi > n - 1 || t.lo > t.hi) return fail("window outside the block", t.lo, t.hi);
        if (t.q * n + t.lo < g.in_first || t.q * n + t.hi >= g.in_first + g.n_in)
            return fail("window outside the piece", t.q * n + t.lo, t.q * n + t.hi);
        const bool staged = route == 1 && accel_fits(g, t);
        const long long count = accel_window_units(g, t);
        if (staged) {
            ++seen->staged;
            if (count < 1 || count > g.lds_units) return fail("window larger than the LDS", count, g.lds_units);
            const long long base = accel_in_index(g, t.q, t.lo, 0);
            if (base < 0 || base + count > in_units) return fail("staging outside the piece", base, count);
            if (base + count - 1 > seen->max_in) seen->max_in = base + count - 1;
        } else {
            ++seen->direct;
        }
        for (long long y = 0; y < g.n_seg; ++y) {
            long long w0, w1;
            accel_segment(g, y, &w0, &w1);
            if (w0 < 0 || w0 >= w1 || w1 > g.W) return fail("segment outside the row", w0, w1);
            for (int tid = 0; tid < BBT_ACCEL_THREADS; ++tid) {
                const int tx = tid & (g.nx - 1), ty = tid >> g.log2nx;
                const int n_elem = (int)g.n_elem;
                for (long long w = w0 + tx; w < w1; w += g.nx) {
                    const int j = (int)w / n_elem, e = (int)w - j * n_elem;
                    if (j < 0 || j >= (int)k.size() || e < 0 || e >= n_elem) return fail("column outside", j, e);
                    for (long long i = t.i0 + ty; i < t.i1; i += g.ny) {
                        const long long s = accel_src(n, k[(size_t)j], i);
                        if (s < t.lo || s > t.hi) return fail("source row outside the tile's window", s, i);
                        if (staged) {
                            const int at = accel_lds_index(g, t, s, e);
                            if (at < 0 || at >= count) return fail("LDS index outside", at, count);
                        } else {
                            const long long at = accel_in_index(g, t.q, s, e);
                            if (at < 0 || at >= in_units) return fail("input index outside", at, in_units);
                            if (at > seen->max_in) seen->max_in = at;
                        }
                        const long long to = accel_out_index(g, t.q, i, w);
                        if (to < 0 || to >= out_units) return fail("output index outside", to, out_units);
                        if (to > seen->max_out) seen->max_out = to;
                        if (whole && ++written[(size_t)to] != 1) return fail("output unit written twice", to, x);
                    }
                }
            }
        }
    }
    if (whole) {
        if (rows_seen != n_out || next_row != out_first + n_out) return fail("rows left out", rows_seen, n_out);
        for (long long u = 0; u < out_units; ++u)
            if (written[(size_t)u] != 1) return fail("output unit not written", u, out_units);
    }
    return 0;
}

static int walk(int argc, char** argv) {
    int at = 0;
    while (at < argc) {
        if (argc - at < 8) return fail("walk: N_ROWS N N_ELEM UNIT ROUTE CHUNK A K...", argc, at);
        const long long n_rows = atoll(argv[at]), n = atoll(argv[at + 1]), n_elem = atoll(argv[at + 2]);
        const int unit = atoi(argv[at + 3]), route = atoi(argv[at + 4]);
        const long long chunk = atoll(argv[at + 5]), n_acc = atoll(argv[at + 6]);
        at += 7;
        if (n_acc < 0 || n_acc > argc - at) return fail("walk: fewer factors than announced", n_acc, argc - at);
        std::vector<double> k;
        for (long long j = 0; j < n_acc; ++j) k.push_back(strtod(argv[at++], nullptr));
        const char* refused = accel_sizes(n, n_elem, n_acc);
        for (size_t j = 0; !refused && j < k.size(); ++j)
            if (!accel_factor_ok(n, k[j])) refused = "a factor beyond |k| n <= 1/4";
        if (!refused && (n_rows < n || chunk < 1)) refused = "no whole block";
        Seen seen;
        if (!refused) {
            const long long length = n_rows / n * n, W = n_elem * n_acc;
            const long long n_launch = (length + chunk - 1) / chunk;
            const bool all = length * W <= 4 * WHOLE;
            for (long long c = 0; c < n_launch && !refused; ++c) {
                if (!all && c != 0 && c != n_launch - 1) continue;
                const long long c0 = c * chunk, c1 = c0 + chunk < length ? c0 + chunk : length;
                if (walk_launch(n, n_elem, unit, route, k, c0, c1 - c0, &seen, &refused)) return 1;
            }
        }
        if (refused) {
            std::printf("{\"error\": \"%s\"}\n", refused);
            continue;
        }
        const AccelGeo& g = seen.first;
        std::printf("{\"walk\": 0, \"launches\": %lld, \"tiles\": %lld, \"staged\": %lld, \"direct\": %lld, \"rows\": %d, "
                    "\"nx\": %d, \"ny\": %d, \"ws\": %lld, \"n_seg\": %lld, \"tpb\": %lld, \"n_tile\": %lld, "
                    "\"lds_units\": %d, \"max_in\": %lld, \"max_out\": %lld}\n",
                    seen.launches, seen.tiles, seen.staged, seen.direct, g.rows, g.nx, g.ny, g.ws, g.n_seg, g.tpb,
                    g.n_tile, g.lds_units, seen.max_in, seen.max_out);
    }
    return 0;
}

static int maps(int argc, char** argv) {
    if (argc < 3) return fail("maps: N FILE K...", argc, 0);
    const long long n = atoll(argv[0]);
    if (accel_sizes(n, 1, argc - 2)) return fail("maps: sizes out of range", n, argc - 2);
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return fail("maps: cannot write the file", 0, 0);
    std::vector<long long> row((size_t)n);
    for (int j = 2; j < argc; ++j) {
        const double k = strtod(argv[j], nullptr);
        if (!accel_factor_ok(n, k)) return fail("maps: a factor beyond the bound", j - 2, n);
        for (long long i = 0; i < n; ++i) row[(size_t)i] = accel_src(n, k, i);
        if (std::fwrite(row.data(), sizeof(long long), row.size(), f) != row.size()) return fail("maps: short write", j, 0);
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "walk")) return walk(argc - 2, argv + 2);
    if (argc >= 2 && !std::strcmp(argv[1], "maps")) return maps(argc - 2, argv + 2);
    return fail("usage: accel_geo_check walk ... | maps ...", argc, 0);
}
