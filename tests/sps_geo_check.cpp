// Walks the tiling of the single-pulse search kernels (csrc/sps_geo.hpp) on the host, for
// test_boxcar_host.py: built with -fsanitize=address,undefined, no GPU.
//
//   sps_geo_check  kind a b c d e f g h  [nine more numbers ...]
//
// kind 0, BoxcarSearch: n_in nb n K n_elem width fuse split.  kind 1, Standardize: n_block n n_elem rows
// and four numbers that are ignored.  Per shape one JSON line: the geometry and "walk", 0 if
//   boxcar, for every pass:
//   - every (block walked, part, element tile) is owned by exactly one row of threads of one
//     workgroup, and nothing beyond the blocks walked is; the element tiles cover the elements,
//   - every read a thread makes -- row i + m 2^k0 for the first and the last start time of its walk,
//     every m the kernel's own condition lets through -- lies inside [0, n_in) and inside what the pass
//     before stored; every store lies inside the scratch, and the rows stored are, counted over all
//     owners, exactly the rows on which the next level is defined,
//   - the winners written are those of blocks < nb, and the two scratch buffers do not overlap;
//   standardize: every (block, element tile) owned once, every row read inside [0, n_block n);
// or {"error": ...} where the geometry refuses the shape.  Before the shapes the limits are held to.
// Exit status 1 if any of that fails.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sps_geo.hpp"

static int walk_boxcar(const SpsGeo& g, long long n_in_given) {
    if (g.n_in > n_in_given || g.n_in < g.nb * g.n || g.n_in > g.nb * g.n + (1ll << (g.K - 1)) - 1) return 1;
    if (g.nx * g.ny != BBT_SPS_THREADS || g.sub * g.nz != g.ny || g.sub > g.n) return 2;
    if (g.n_tile * g.nx < g.n_elem || (g.n_tile - 1) * g.nx >= g.n_elem) return 3;
    if (g.nbv * g.n < g.n_in || (g.nbv - 1) * g.n >= g.n_in) return 4;
    if (g.n_pass != (g.K + g.fuse - 1) / g.fuse) return 5;
    const long long plane = g.n_in * g.n_elem;
    if (g.scratch != (g.n_pass - 1 < 2 ? g.n_pass - 1 : 2) * plane) return 6;
    long long stored_rows_before = g.n_in;            // rows of S_k0 that exist: those of the chunk for pass 0
    for (int p = 0; p < g.n_pass; ++p) {
        const SpsPass ps = sps_pass(g, p);
        if (ps.k0 != p * g.fuse || ps.k0 >= g.K || ps.levels < 1 || ps.k0 + ps.levels > g.K) return 10;
        if (ps.store != (p + 1 < g.n_pass)) return 11;
        if (ps.blocks < g.nb || ps.blocks > g.nbv || (ps.store && ps.blocks != g.nbv)) return 12;
        const long long w = 1ll << ps.k0, wf = w << g.fuse;
        if (stored_rows_before != g.n_in - w + 1) return 13;          // S_k0 is defined on exactly these rows
        std::vector<unsigned char> seen((size_t)(ps.blocks * g.sub * g.n_tile), 0);
        long long rows_stored = 0;
        for (long long wg = 0; wg < ps.n_wg; ++wg) {
            for (int ty = 0; ty < g.ny; ++ty) {
                SpsOwn o;
                if (!sps_own(g, wg, ty, ps.blocks, &o)) continue;
                if (o.b < 0 || o.b >= ps.blocks || o.q < 0 || o.q >= g.sub || o.e0 % g.nx || o.e0 < 0 || o.e0 >= g.n_elem)
                    return 14;
                unsigned char& s = seen[(size_t)((o.b * g.sub + o.q) * g.n_tile + o.e0 / g.nx)];
                if (s) return 15;
                s = 1;
                // the walk of this row of threads, as the kernel sets it up
                const long long t0 = o.b * g.n;
                long long t1 = t0 + g.n;
                if (t1 > g.n_in - w + 1) t1 = g.n_in - w + 1;
                const long long first = t0 + o.q;
                if (first >= t1) continue;
                const long long last = first + (t1 - 1 - first) / g.sub * g.sub;
                const long long e_last = (o.e0 + g.nx - 1 < g.n_elem ? o.e0 + g.nx - 1 : g.n_elem - 1);
                for (long long i = first;; i = last) {
                    for (long long m = 0; m < (1ll << g.fuse); ++m) {
                        if (!(i + (m + 1) * w <= g.n_in)) continue;              // (the kernel's condition)
                        const long long row = i + m * w;
                        if (row < 0 || row >= g.n_in || row >= stored_rows_before) return 16;
                        const long long at = row * g.n_elem + e_last;
                        if (at < 0 || at >= plane) return 17;
                    }
                    if (ps.store && i + wf <= g.n_in && (i < 0 || i * g.n_elem + e_last >= plane)) return 18;
                    if (i == last) break;
                }
                if (ps.store && o.e0 == 0) {
                    long long end = t0 + g.n;
                    if (end > g.n_in - wf + 1) end = g.n_in - wf + 1;
                    if (first < end) rows_stored += (end - 1 - first) / g.sub + 1;
                }
            }
        }
        for (unsigned char s : seen)
            if (!s) return 19;
        if (ps.store) {
            const long long want = g.n_in - wf + 1 > 0 ? g.n_in - wf + 1 : 0;
            if (rows_stored != want) return 20;
            stored_rows_before = g.n_in - wf + 1;
        }
        // the winners: blocks < nb, cell [b][2][e_last]
        if ((g.nb - 1) * 3 * g.n_elem + 2 * g.n_elem + g.n_elem - 1 >= g.nb * 3 * g.n_elem) return 21;
    }
    return 0;
}

static int walk_std(const StdGeo& g) {
    if (g.nx * g.ny != BBT_SPS_THREADS) return 1;
    if (g.n_tile * g.nx < g.n_elem || (g.n_tile - 1) * g.nx >= g.n_elem) return 2;
    if (g.n_wg != g.n_block * g.n_tile) return 3;
    std::vector<unsigned char> seen((size_t)g.n_wg, 0);
    for (long long wg = 0; wg < g.n_wg; ++wg) {
        const long long tile = wg % g.n_tile, block = wg / g.n_tile;
        if (block >= g.n_block) return 4;
        unsigned char& s = seen[(size_t)(block * g.n_tile + tile)];
        if (s) return 5;
        s = 1;
        const long long e_last = (tile * g.nx + g.nx - 1 < g.n_elem ? tile * g.nx + g.nx - 1 : g.n_elem - 1);
        const int n_seg = (int)((g.n + BBT_SPS_SEG - 1) / BBT_SPS_SEG);
        const long long t_last = (long long)(n_seg - 1) * BBT_SPS_SEG + (g.n - (long long)(n_seg - 1) * BBT_SPS_SEG) - 1;
        if (t_last != g.n - 1) return 6;
        const long long at = (block * g.n + t_last) * g.n_elem + e_last;
        if (at < 0 || at >= g.n_block * g.n * g.n_elem) return 7;
    }
    for (unsigned char s : seen)
        if (!s) return 8;
    return 0;
}

static int validation() {
    SpsGeo g;
    StdGeo s;
    if (sps_geo(100, 10, 10, 1, 3, 0, 0, 0, &g)) return 1;
    if (!sps_geo(99, 10, 10, 1, 3, 0, 0, 0, &g)) return 2;                       // one sample short
    if (!sps_geo(100, 0, 10, 1, 3, 0, 0, 0, &g)) return 3;                       // no blocks
    if (!sps_geo(100, 10, 10, 0, 3, 0, 0, 0, &g) || !sps_geo(100, 10, 10, 14, 3, 0, 0, 0, &g)) return 4;
    if (!sps_geo(100, 10, 0, 1, 3, 0, 0, 0, &g) || !sps_geo(1 << 20, 1, 65537, 1, 3, 0, 0, 0, &g)) return 5;
    if (sps_geo(65536, 1, 65536, 13, 1, 0, 0, 0, &g)) return 6;
    if (!sps_geo(100, 10, 10, 1, 0, 0, 0, 0, &g)) return 7;
    if (!sps_geo(100, 10, 10, 1, 3, 48, 0, 0, &g) || !sps_geo(100, 10, 10, 1, 3, 0, 4, 0, &g) ||
        !sps_geo(100, 10, 10, 1, 3, 0, 0, 3, &g))
        return 8;
    if (!sps_sizes(0, 1, 1) || !sps_sizes(1, 0, 1) || !sps_sizes(1, 14, 1) || !sps_sizes(1, 1, 0) || sps_sizes(65536, 13, 1))
        return 9;
    if (sps_std_geo(3, 2, 5, 0, &s) || !sps_std_geo(3, 1, 5, 0, &s) || !sps_std_geo(3, 65537, 5, 0, &s) ||
        !sps_std_geo(0, 2, 5, 0, &s) || !sps_std_geo(3, 2, 0, 0, &s) || !sps_std_geo(3, 2, 5, 3, &s) ||
        sps_std_geo(1, 65536, 5, 16, &s))
        return 10;
    // the scales: exact powers of two for even k, and c_k c_k = 2^-k to the last bit but one for odd k
    for (int k = 0; k < BBT_SPS_MAX_WIDTHS; k += 2) {
        float want = 1.f;
        for (int j = 0; j < k / 2; ++j) want /= 2.f;
        if (sps_scale(k) != want) return 11;
    }
    for (int k = 1; k + 2 < BBT_SPS_MAX_WIDTHS; k += 2)
        if (sps_scale(k + 2) * 2.f != sps_scale(k)) return 12;
    return 0;
}

int main(int argc, char** argv) {
    const int v = validation();
    if (v) {
        printf("{\"validation\": %d}\n", v);
        return 1;
    }
    int status = 0;
    for (int i = 1; i + 9 <= argc; i += 9) {
        long long a[9];
        for (int k = 0; k < 9; ++k) a[k] = atoll(argv[i + k]);
        if (a[0] == 0) {
            SpsGeo g = {};
            const char* err = sps_geo(a[1], a[2], a[3], a[4], a[5], (int)a[6], (int)a[7], (int)a[8], &g);
            if (err) {
                printf("{\"error\": \"%s\"}\n", err);
                continue;
            }
            const int w = walk_boxcar(g, a[1]);
            if (w) status = 1;
            printf("{\"n_in\": %lld, \"nbv\": %lld, \"n_pass\": %d, \"fuse\": %d, \"nx\": %d, \"ny\": %d, \"sub\": %d, "
                   "\"nz\": %d, \"n_tile\": %lld, \"scratch\": %lld, \"scales\": [",
                   g.n_in, g.nbv, g.n_pass, g.fuse, g.nx, g.ny, g.sub, g.nz, g.n_tile, g.scratch);
            for (int k = 0; k < BBT_SPS_MAX_WIDTHS; ++k) {
                unsigned bits;
                memcpy(&bits, &g.c[k], 4);
                printf("%s%u", k ? ", " : "", bits);
            }
            printf("], \"walk\": %d}\n", w);
        } else {
            StdGeo g = {};
            const char* err = sps_std_geo(a[1], a[2], a[3], (int)a[4], &g);
            if (err) {
                printf("{\"error\": \"%s\"}\n", err);
                continue;
            }
            const int w = walk_std(g);
            if (w) status = 1;
            printf("{\"nx\": %d, \"ny\": %d, \"n_tile\": %lld, \"n_wg\": %lld, \"walk\": %d}\n", g.nx, g.ny, g.n_tile,
                   g.n_wg, w);
        }
    }
    return status;
}
