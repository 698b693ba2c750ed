// Walks the tiling of the trial-DM kernels (csrc/dmt_geo.hpp) on the host, for test_dmtrials_host.py:
// built with -fsanitize=address,undefined, no GPU.
//
//   dmt_geo_check  n_in n_out nchan n_rest ndm span tile_t db  [eight more numbers ...]
//
// Per shape one JSON line: the geometry and "walk", 0 if
//   - the waves of all workgroups own every (block of 64 times, block of db trials, r) of the
//     result exactly once, and nothing beyond it,
//   - every read the sweep makes -- row e = c * n_rest + r of the scratch at t0 + lane' + offset,
//     for the extreme offsets 0 and span, lane' as the kernel sets it -- lies inside [0, n_in) of
//     that row and inside the scratch, and every offset-table read inside [0, nchan * ndm_pad),
//   - the transpose tiles cover the chunk,
// or {"error": ...} where dmt_geo refuses the shape.  Before the shapes, the table validation is
// held to: a negative offset, an offset above the span and a span beyond the limit are refused, a
// good table is not, and an input one sample short is refused.  Exit status 1 if any of that fails.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dmt_geo.hpp"

static int walk(const DmtGeo& g, long long span) {
    const long long blocks_t = (g.n_out + BBT_DMT_WAVE - 1) / BBT_DMT_WAVE;
    const long long blocks_d = (g.ndm + g.db - 1) / g.db;
    std::vector<unsigned char> seen((size_t)(blocks_t * blocks_d * g.n_rest), 0);
    const long long n_e = (long long)g.nchan * g.n_rest;
    if (g.pitch < g.n_in || g.scratch != n_e * g.pitch) return 1;
    if (g.ndm_pad < g.ndm || g.ndm_pad % BBT_DMT_DB_MAX) return 2;
    for (long long wg = 0; wg < g.n_wg; ++wg) {
        for (int w = 0; w < BBT_DMT_THREADS / BBT_DMT_WAVE; ++w) {
            DmtWave o;
            if (!dmt_wave(g, wg, w, &o)) continue;
            if (o.t0 % BBT_DMT_WAVE || o.d0 % g.db || o.r < 0 || o.r >= g.n_rest) return 3;
            if (o.t0 < 0 || o.t0 >= g.n_out || o.d0 < 0 || o.d0 >= g.ndm) return 4;
            unsigned char& s = seen[(size_t)(((o.t0 / BBT_DMT_WAVE) * blocks_d + o.d0 / g.db) * g.n_rest + o.r)];
            if (s) return 5;
            s = 1;
            // the table: entries d0 ... d0 + db - 1 of every row
            if (o.d0 + g.db > g.ndm_pad) return 6;
            // the reads: first and last lane, least and largest offset, first and last channel
            for (int lane = 0; lane < BBT_DMT_WAVE; lane += BBT_DMT_WAVE - 1) {
                const long long lt = o.t0 + lane < g.n_out ? lane : 0;
                for (long long off = 0; off <= span; off += span ? span : 1) {
                    const long long t = o.t0 + lt + off;
                    if (t < 0 || t >= g.n_in) return 7;
                    for (long long c = 0; c < g.nchan; c += g.nchan > 1 ? g.nchan - 1 : 1) {
                        const long long at = (c * g.n_rest + o.r) * g.pitch + t;
                        if (at < 0 || at >= g.scratch) return 8;
                    }
                }
            }
            // the stores: the last one
            const long long last_t = o.t0 + BBT_DMT_WAVE - 1 < g.n_out ? o.t0 + BBT_DMT_WAVE - 1 : g.n_out - 1;
            const long long last_d = o.d0 + g.db - 1 < g.ndm ? o.d0 + g.db - 1 : g.ndm - 1;
            const long long at = (last_t * g.ndm + last_d) * g.n_rest + o.r;
            if (at < 0 || at >= g.n_out * g.ndm * g.n_rest) return 9;
        }
    }
    for (unsigned char s : seen)
        if (!s) return 10;
    if (g.tr_t * BBT_DMT_TR < g.n_in || (g.tr_t - 1) * BBT_DMT_TR >= g.n_in) return 11;
    if ((long long)g.tr_e * BBT_DMT_TR < n_e || ((long long)g.tr_e - 1) * BBT_DMT_TR >= n_e) return 12;
    return 0;
}

static int validation() {
    const int good[6] = {0, 3, 7, 7, 1, 0};
    if (dmt_check_table(good, 6, 7)) return 1;
    int bad[6] = {0, 3, -1, 7, 1, 0};
    if (!dmt_check_table(bad, 6, 7)) return 2;
    bad[2] = 8;
    if (!dmt_check_table(bad, 6, 7)) return 3;
    if (dmt_check_table(bad, 6, 8)) return 4;
    if (!dmt_check_table(good, 6, (long long)BBT_DMT_MAX_SPAN + 1) || !dmt_check_table(good, 6, -1)) return 5;
    DmtGeo g;
    if (dmt_geo(100 + 7, 100, 3, 1, 2, 7, 0, 0, &g)) return 6;
    if (!dmt_geo(100 + 6, 100, 3, 1, 2, 7, 0, 0, &g)) return 7;                  // one sample short
    if (!dmt_geo(107, 0, 3, 1, 2, 7, 0, 0, &g)) return 8;
    if (!dmt_sizes(BBT_DMT_MAX_NDM + 1, 1, 1) || !dmt_sizes(1, BBT_DMT_MAX_NCHAN + 1, 1) ||
        !dmt_sizes(1, 1, BBT_DMT_MAX_REST + 1) || !dmt_sizes(0, 1, 1) || !dmt_sizes(1, 0, 1) || !dmt_sizes(1, 1, 0))
        return 9;
    if (dmt_sizes(BBT_DMT_MAX_NDM, BBT_DMT_MAX_NCHAN, BBT_DMT_MAX_REST)) return 10;
    return 0;
}

int main(int argc, char** argv) {
    const int v = validation();
    if (v) {
        printf("{\"validation\": %d}\n", v);
        return 1;
    }
    int status = 0;
    for (int i = 1; i + 8 <= argc; i += 8) {
        long long a[8];
        for (int k = 0; k < 8; ++k) a[k] = atoll(argv[i + k]);
        DmtGeo g = {};
        const char* err = dmt_geo(a[0], a[1], a[2], a[3], a[4], a[5], (int)a[6], (int)a[7], &g);
        if (err) {
            printf("{\"error\": \"%s\"}\n", err);
            continue;
        }
        const int w = walk(g, a[5]);
        if (w) status = 1;
        printf("{\"pitch\": %lld, \"scratch\": %lld, \"ndm_pad\": %d, \"db\": %d, \"tile_t\": %d, \"tile_d\": %d, "
               "\"waves_t\": %d, \"waves_d\": %d, \"n_tile_t\": %lld, \"n_tile_d\": %d, \"n_wg\": %lld, \"tr_t\": %lld, "
               "\"tr_e\": %d, \"walk\": %d}\n",
               g.pitch, g.scratch, g.ndm_pad, g.db, g.tile_t, g.tile_d, g.waves_t, g.waves_d, g.n_tile_t, g.n_tile_d,
               g.n_wg, g.tr_t, g.tr_e, w);
    }
    return status;
}
