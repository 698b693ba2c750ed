// Walks the tiling of the sliding-median kernels (csrc/rmed_geo.hpp) on the host and runs its two
// selection methods against sorted windows, for test_rmed_host.py: built with
// -fsanitize=address,undefined, no GPU.
//
//   rmed_geo_check  width scrunch n_elem n_samples tile rows method chunk  [eight more numbers ...]
//
// Before the shapes: the limits and refusals, rmed_lerp against its statement in floor arithmetic, and
// the selection -- the very rmed_select and rmed_step the kernel calls, driven by a loop that restates
// the kernel thread's (a fresh selection for its first median and for every clipped window, a step
// between two full windows) -- on columns of random values, ties, both zeros, denormals and NaN, every
// median compared with the sorted keys of its window: lo, hi and the row of lo in the order (key, row).
// Per shape the stream of n_samples is made in calls of `chunk` output samples (0: one call), as the task
// makes it, and one JSON line gives the geometry of the first call and "walk", 0 if for every call
//   - the input span rmed_need states is exactly what the samples of the call reach: for the first and
//     the last sample of every scrunch row, the windows of the medians rmed_lerp names, clipped to [0, R),
//   - every median of [m0, m1) is owned by exactly one run of workgroups, the element tiles cover the
//     elements, the threads of a column cut the run into consecutive pieces,
//   - every staged row lies inside [c0, c1), so inside the stream and the input, every window of an owned
//     median inside the staged rows, the staged rows within the LDS bytes and those within 72 KiB,
//   - every m a sample reads lies in [m0, m1),
// and if the calls tile [0, R S).  {"error": ...} where the geometry refuses the shape.  Exit status 1 if
// any of that fails.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rmed_geo.hpp"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures < 20) {          \
                fprintf(stderr, __VA_ARGS__); \
                fputc('\n', stderr);      \
            }                             \
            ++failures;                   \
        }                                 \
    } while (0)

static unsigned as_bits(float f) {
    unsigned b;
    memcpy(&b, &f, 4);
    return b;
}

// one column of R keys walked as a kernel thread walks it, in pieces of `per` medians
static long long check_column(const std::vector<unsigned>& keys, int w, int per, int method) {
    const int R = (int)keys.size(), h = w / 2;
    auto key_at = [&](int t) -> unsigned { return keys[(size_t)t]; };             // (ASan checks t)
    long long steps = 0;
    unsigned key = 0;
    int pos = 0;
    bool full_before = false;
    for (int r = 0; r < R; ++r) {
        if (r % per == 0) full_before = false;                                   // the next thread begins
        const int a = r - h < 0 ? 0 : r - h, b = r + h + 1 > R ? R : r + h + 1;
        const bool full = b - a == w;
        unsigned lo, hi;
        if (full && full_before && method == BBT_RMED_SELECT_WALK) {
            rmed_step(key_at, a - 1, b - 1, &key, &pos);
            lo = hi = key;
            ++steps;
        } else {
            rmed_select(key_at, a, b, &lo, &hi, &pos);
            key = lo;
        }
        full_before = full;
        std::vector<rmed_ord> sorted;
        for (int t = a; t < b; ++t) sorted.push_back(rmed_ord_of(keys[(size_t)t], t));
        std::sort(sorted.begin(), sorted.end());
        const int L = b - a;
        const rmed_ord want_lo = sorted[(size_t)((L - 1) / 2)], want_hi = sorted[(size_t)(L / 2)];
        CHECK(lo == (unsigned)(want_lo >> 32) && hi == (unsigned)(want_hi >> 32) && pos == (int)(unsigned)want_lo,
              "selection: w=%d R=%d r=%d method=%d: lo %08x hi %08x pos %d, sorted %08x %08x pos %d", w, R, r, method, lo, hi,
              pos, (unsigned)(want_lo >> 32), (unsigned)(want_hi >> 32), (int)(unsigned)want_lo);
    }
    return steps;
}

static void check_selection() {
    std::mt19937 rng(12345);
    std::normal_distribution<float> normal(5.f, 3.f);
    long long windows = 0, steps = 0;
    const int widths[] = {3, 5, 31, 33, 65, 255, 1023};
    for (int kind = 0; kind < 6; ++kind)
        for (int w : widths) {
            const int R = kind == 5 ? w / 2 + 1 + (int)(rng() % 7) : w + 40 + (int)(rng() % 200);     // (kind 5: every window clipped on both sides)
            std::vector<unsigned> keys((size_t)R);
            for (int t = 0; t < R; ++t) {
                float v;
                switch (kind) {
                    case 0: v = normal(rng); break;
                    case 1: v = (float)((int)(rng() % 9) - 4); break;                                      // many ties
                    case 2: v = (rng() & 1) ? 0.f : -0.f; break;                                           // both zeros
                    case 3: v = (float)t * ((w & 2) ? 1.f : -1.f); break;                                  // a ramp, up or down
                    case 4: {
                        unsigned bits = rng() % 5 == 0 ? (0x7fc00000u | (rng() & 0x80000000u)) : (rng() % 100 + 1) | (rng() & 0x80000000u);
                        memcpy(&v, &bits, 4);                                                              // NaN of either sign, denormals
                        break;
                    }
                    default: v = rng() % 3 ? 7.f : normal(rng); break;
                }
                keys[(size_t)t] = rank_key(as_bits(v));
            }
            for (int method = 1; method <= 2; ++method)
                for (int per : {R, 7, 64}) {
                    steps += check_column(keys, w, per, method);
                    windows += R;
                }
        }
    CHECK(windows > 5000 && steps > 2000, "selection: only %lld windows, %lld steps", windows, steps);
    // the key map of the block median, unchanged: -0 just before +0
    CHECK(rank_key(0x80000000u) + 1 == rank_key(0u), "keys: -0 is not just before +0");
}

static void check_lerp() {
    for (long long S : {1ll, 2ll, 3ll, 8ll, 32ll, 33ll, 100ll, 4096ll})
        for (long long R : {1ll, 2ll, 3ll, 21ll})
            for (long long i = 0; i < R * S; ++i) {
                long long r0, q;
                rmed_lerp(i, S, R, &r0, &q);
                if (R == 1) {
                    CHECK(r0 == 0 && q == 0, "lerp: R = 1");
                    continue;
                }
                const long long j = 2 * i + 1 - S;
                long long f = j / (2 * S);
                if (f * 2 * S > j) --f;                                          // floor
                f = std::max(0ll, std::min(R - 2, f));
                CHECK(r0 == f && q == j - 2 * S * f, "lerp: S=%lld R=%lld i=%lld: r0 %lld q %lld", S, R, i, r0, q);
                const long long row = i / S;
                CHECK(r0 >= std::max(0ll, row - 1) && r0 + 1 <= std::min(R - 1, row + 1), "lerp: S=%lld R=%lld i=%lld leaves its neighbours", S, R, i);
                if (S == 1) CHECK((q == 0 && r0 == i) || (q == 2 && r0 + 1 == i), "lerp: S = 1 is not b[i] = m[i] at i=%lld", i);
            }
}

static void check_limits() {
    RmedGeo g;
    CHECK(BBT_RMED_MAX_WIDTH == 1023 && BBT_RMED_MIN_WIDTH == 3 && BBT_RMED_MAX_SCRUNCH == 4096, "limits");
    CHECK(2 * BBT_RANK_LDS_BYTES <= 160 * 1024, "two workgroups do not fit a CU");
    CHECK(rmed_lds_rows(16) - (BBT_RMED_MAX_WIDTH - 1) >= 16, "the widest window leaves no run");
    CHECK(rmed_sizes(4, 1, 1) && rmed_sizes(1, 1, 1) && rmed_sizes(1025, 1, 1) && rmed_sizes(3, 0, 1) && rmed_sizes(3, 4097, 1) &&
              rmed_sizes(3, 1, 0) && !rmed_sizes(3, 1, 1) && !rmed_sizes(1023, 4096, 1),
          "sizes");
    CHECK(rmed_geo(5, 2, 3, 10, 0, 20, 0, 20, 0, 0, 0, &g) == 0, "a plain call is refused");
    CHECK(rmed_geo(5, 2, 3, 10, 0, 20, 1, 20, 0, 0, 0, &g) != 0, "an output off the scrunch rows");
    CHECK(rmed_geo(5, 2, 3, 10, 0, 20, 0, 22, 0, 0, 0, &g) != 0, "an output beyond the stream");
    CHECK(rmed_geo(5, 2, 3, 10, 0, 18, 0, 20, 0, 0, 0, &g) != 0, "an input too short");
    CHECK(rmed_geo(5, 2, 3, 10, 2, 18, 0, 4, 0, 0, 0, &g) != 0, "an input that begins too late");
    CHECK(rmed_geo(5, 2, 3, 10, 1, 19, 4, 4, 0, 0, 0, &g) != 0, "an input off the scrunch rows");
    CHECK(rmed_geo(5, 2, 3, 0, 0, 20, 0, 20, 0, 0, 0, &g) != 0, "no rows");
    CHECK(rmed_geo(5, 2, 3, 10, 0, 20, 0, 20, 48, 0, 0, &g) != 0 && rmed_geo(5, 2, 3, 10, 0, 20, 0, 20, 0, 0, 3, &g) != 0, "knobs");
}

int main(int argc, char** argv) {
    check_limits();
    check_lerp();
    check_selection();
    for (int at = 1; at + 8 <= argc; at += 8) {
        const long long w = atoll(argv[at]), S = atoll(argv[at + 1]), E = atoll(argv[at + 2]), N = atoll(argv[at + 3]);
        const int tile = atoi(argv[at + 4]), rows = atoi(argv[at + 5]), method = atoi(argv[at + 6]);
        long long chunk = atoll(argv[at + 7]);
        const long long R = S > 0 ? N / S : 0, h = w / 2;
        if (chunk <= 0) chunk = R * S;
        const int before = failures;
        bool first = true;
        long long calls = 0;
        for (long long o0 = 0; first || o0 < R * S; o0 += chunk, first = false) {
            const long long o1 = std::min(R * S, o0 + chunk);
            long long m0 = 0, m1 = 0, c0 = 0, c1 = 0;
            if (S > 0 && R > 0) rmed_need(S, h, R, o0 / S, o1 / S, &m0, &m1, &c0, &c1);
            RmedGeo g;
            memset(&g, 0, sizeof g);
            const char* err = rmed_geo(w, S, E, R, c0 * S, (c1 - c0) * S, o0, o1 - o0, tile, rows, method, &g);
            if (err) {
                if (first) printf("{\"error\": \"%s\"}\n", err);
                else CHECK(false, "a later call is refused: %s", err);
                break;
            }
            ++calls;
            CHECK(chunk % S == 0 && g.m0 == m0 && g.m1 == m1 && g.c0 == c0 && g.c1 == c1, "the rows of the call");
            // what the samples reach
            long long reach0 = R, reach1 = 0, med0 = R, med1 = 0;
            for (long long ro = o0 / S; ro < o1 / S; ++ro)
                for (long long i : {ro * S, ro * S + S - 1}) {
                    long long r0, q;
                    rmed_lerp(i, S, R, &r0, &q);
                    const long long ma = q >= 2 * S ? r0 + 1 : r0, mb = q <= 0 ? r0 : r0 + 1;
                    med0 = std::min(med0, ma), med1 = std::max(med1, mb + 1);
                    reach0 = std::min(reach0, std::max(0ll, ma - h)), reach1 = std::max(reach1, std::min(R, mb + h + 1));
                }
            CHECK(med0 == m0 && med1 == m1 && reach0 == c0 && reach1 == c1,
                  "out [%lld, %lld): medians [%lld, %lld) rows [%lld, %lld), stated [%lld, %lld) [%lld, %lld)", o0, o1, med0, med1,
                  reach0, reach1, m0, m1, c0, c1);
            CHECK(c0 == std::max(0ll, std::max(0ll, o0 / S - (S > 1)) - h) && c1 == std::min(R, std::min(R, o1 / S + (S > 1)) + h), "the input span");
            // the tiling
            CHECK(g.nx * g.ny == BBT_RMED_THREADS && g.n_tile * g.nx >= E && (g.n_tile - 1) * g.nx < E, "element tiles");
            CHECK(g.n_wg == g.n_run * g.n_tile && g.run >= 1 && g.lds_bytes <= BBT_RANK_LDS_BYTES, "workgroups, LDS");
            CHECK(g.scratch_bytes == (S > 1 ? ((c1 - c0) + (m1 - m0)) * E * 4 : 0), "scratch");
            long long next = m0;
            for (long long ri = 0; ri < g.n_run; ++ri) {
                RmedOwn o;
                rmed_own(g, ri * g.n_tile + (g.n_tile - 1), &o);
                CHECK(o.row0 == next && o.len >= 1 && o.len <= g.run && o.e0 == (g.n_tile - 1) * g.nx, "run %lld begins at %lld, not %lld", ri, o.row0, next);
                next = o.row0 + o.len;
                CHECK(o.st0 >= c0 && o.st0 + o.n_st <= c1 && o.st0 >= 0 && o.st0 + o.n_st <= R, "run %lld stages rows outside the input", ri);
                CHECK((long long)o.n_st * g.nx * 4 <= g.lds_bytes, "run %lld stages %d rows: beyond the LDS", ri, o.n_st);
                CHECK(o.st0 <= std::max(0ll, o.row0 - h) && o.st0 + o.n_st >= std::min(R, o.row0 + o.len + h), "run %lld: a window leaves the staged rows", ri);
                CHECK(o.per >= 1 && (long long)o.per * g.ny >= o.len && (long long)(o.per - 1) * g.ny < o.len, "run %lld: the threads' pieces", ri);
            }
            CHECK(next == m1, "the runs end at %lld, not %lld", next, m1);
            if (first)
                printf("{\"width\": %lld, \"scrunch\": %lld, \"n_elem\": %lld, \"n_rows\": %lld, \"nx\": %d, \"ny\": %d, \"run\": %d, "
                       "\"method\": %d, \"n_tile\": %lld, \"n_wg\": %lld, \"lds_bytes\": %lld, \"scratch_bytes\": %lld, "
                       "\"in_first\": %lld, \"in_count\": %lld, ",
                       w, S, E, R, g.nx, g.ny, g.run, g.method, g.n_tile, g.n_wg, g.lds_bytes, g.scratch_bytes, c0 * S, (c1 - c0) * S);
        }
        if (calls) printf("\"calls\": %lld, \"walk\": %d}\n", calls, failures - before);
    }
    if (failures) fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
