// Walks the tiling of the periodicity-search kernels (csrc/hsum_geo.hpp) on the host, for
// test_hsum_host.py: built with -fsanitize=address,undefined, no GPU.
//
//   hsum_geo_check  kind a b c d e f g h  [nine more numbers ...]
//
// kind 0, HarmonicSearch: n_spec nbin n K lo n_elem width split.  kind 1, Whiten: n_spec nbin n_elem m skip
// rows and two numbers that are ignored.  Per shape one JSON line: the geometry and "walk", 0 if
//   search:
//   - every (spectrum, block, part, element tile) is owned by exactly one row of threads of one
//     workgroup, and nothing beyond the last pair is; the element tiles cover the elements,
//   - every index a thread gathers -- (j i + 2^(L-1)) >> L for every level, every odd i, and every j of
//     its walk (the first and the last j only for spectra of more than 2^16 bins) -- lies in [0, j],
//     so inside the spectrum, with j i below 2^29, and its address inside the chunk; the walks of the
//     parts of a block cover its bins exactly once,
//   - the winner's three cells lie inside the result;
//   whiten: every workgroup owns one (spectrum, block, element tile), the blocks of a spectrum tile
//     its bins in order with no gap -- [0, skip) first if skip > 0, then blocks of m, the last one
//     short -- and the last row read lies inside the chunk;
// or {"error": ...} where the geometry refuses the shape.  Before the shapes the limits are held to.
// Exit status 1 if any of that fails.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hsum_geo.hpp"

static int walk_search(const HsumGeo& g) {
    if (g.nx * g.ny != BBT_HSUM_THREADS || g.sub * g.nz != g.ny || g.sub > g.n || g.sub < 1) return 1;
    if (g.n_tile * g.nx < g.n_elem || (g.n_tile - 1) * g.nx >= g.n_elem) return 2;
    if (g.nb * g.n < g.nbin || (g.nb - 1) * g.n >= g.nbin) return 3;
    if (g.n_pair != g.n_spec * g.nb) return 4;
    if (g.n_wg != (g.n_pair + g.nz - 1) / g.nz * g.n_tile) return 5;
    const long long chunk = g.n_spec * g.nbin * g.n_elem, result = g.n_pair * 3 * g.n_elem;
    const bool every = g.nbin <= (1 << 16);
    std::vector<unsigned char> seen((size_t)(g.n_pair * g.sub * g.n_tile), 0);
    std::vector<long long> walked((size_t)g.n_pair, 0);              // bins walked, over the parts, for tile 0
    for (long long wg = 0; wg < g.n_wg; ++wg) {
        for (int ty = 0; ty < g.ny; ++ty) {
            HsumOwn o;
            if (!hsum_own(g, wg, ty, &o)) {
                if (((wg / g.n_tile) * g.nz + ty / g.sub) < g.n_pair) return 10;
                continue;
            }
            if (o.s < 0 || o.s >= g.n_spec || o.b < 0 || o.b >= g.nb || o.q < 0 || o.q >= g.sub || o.e0 % g.nx ||
                o.e0 < 0 || o.e0 >= g.n_elem)
                return 11;
            const long long pair = o.s * g.nb + o.b;
            unsigned char& s = seen[(size_t)((pair * g.sub + o.q) * g.n_tile + o.e0 / g.nx)];
            if (s) return 12;
            s = 1;
            // the walk of this row of threads, as the kernel sets it up
            const int j0 = (int)(o.b * g.n);
            const int j1 = (int)(g.nbin - j0 < g.n ? g.nbin : j0 + g.n);
            if (j0 < 0 || j1 > g.nbin || j1 <= j0) return 13;
            const long long e_last = (o.e0 + g.nx - 1 < g.n_elem ? o.e0 + g.nx - 1 : g.n_elem - 1);
            const int first = j0 + o.q;
            if (first < j1 && o.e0 == 0) walked[(size_t)pair] += (j1 - 1 - first) / g.sub + 1;
            if (first >= j1) continue;
            const int last = first + (j1 - 1 - first) / g.sub * g.sub;
            for (int j = first; j <= last; j += every ? g.sub : (last > first ? last - first : 1)) {
                for (int L = 0; L < g.K; ++L) {
                    for (int i = 1; i < (1 << L) || i == 1; i += 2) {
                        if ((long long)j * i >= (1ll << 29)) return 14;
                        const int idx = hsum_bin(j, i, L);
                        if (idx < 0 || idx > j || idx >= g.nbin) return 15;
                        const long long at = (o.s * g.nbin + idx) * g.n_elem + e_last;
                        if (at < 0 || at >= chunk) return 16;
                    }
                    const int f = hsum_bin(j, 1, L);                 // the fundamental's bin
                    if (f < 0 || f > j) return 17;
                }
            }
            const long long cell = pair * 3 * g.n_elem + 2 * g.n_elem + e_last;
            if (cell < 0 || cell >= result) return 18;
        }
    }
    for (unsigned char s : seen)
        if (!s) return 19;
    for (long long pair = 0; pair < g.n_pair; ++pair) {
        const long long b = pair % g.nb;
        const long long len = g.nbin - b * g.n < g.n ? g.nbin - b * g.n : g.n;
        if (walked[(size_t)pair] != len) return 20;
    }
    return 0;
}

static int walk_whiten(const WhitenGeo& g) {
    if (g.nx * g.ny != BBT_HSUM_THREADS) return 1;
    if (g.n_tile * g.nx < g.n_elem || (g.n_tile - 1) * g.nx >= g.n_elem) return 2;
    if (g.n_blk != (g.nbin - g.skip + g.m - 1) / g.m + (g.skip > 0)) return 3;
    if (g.n_wg != g.n_spec * g.n_blk * g.n_tile) return 4;
    const long long chunk = g.n_spec * g.nbin * g.n_elem;
    long long wg = 0;
    for (long long s = 0; s < g.n_spec; ++s) {
        long long next = 0;                                          // the bin the next block must start at
        for (long long b = 0; b < g.n_blk; ++b) {
            for (long long tile = 0; tile < g.n_tile; ++tile, ++wg) {
                WhitenOwn o;
                hsum_whiten_own(g, wg, &o);
                if (o.s != s || o.e0 != tile * g.nx || o.j0 != next || o.len < 1 || o.j0 + o.len > g.nbin) return 5;
                if (o.zero != (g.skip > 0 && b == 0)) return 6;
                if (o.zero ? o.len != g.skip : (o.len > g.m || (o.len < g.m && o.j0 + o.len != g.nbin))) return 7;
                if (!o.zero && (o.j0 - g.skip) % g.m) return 8;
                const long long e_last = (o.e0 + g.nx - 1 < g.n_elem ? o.e0 + g.nx - 1 : g.n_elem - 1);
                const int n_seg = (int)((o.len + BBT_HSUM_SEG - 1) / BBT_HSUM_SEG);
                const long long t_last = (long long)(n_seg - 1) * BBT_HSUM_SEG +
                                         (o.len - (long long)(n_seg - 1) * BBT_HSUM_SEG) - 1;
                if (t_last != o.len - 1) return 9;
                const long long at = (o.s * g.nbin + o.j0 + t_last) * g.n_elem + e_last;
                if (at < 0 || at >= chunk) return 10;
                if (tile + 1 == g.n_tile) next = o.j0 + o.len;
            }
        }
        if (next != g.nbin) return 11;
    }
    return wg == g.n_wg ? 0 : 12;
}

static int validation() {
    HsumGeo g;
    WhitenGeo w;
    if (hsum_geo(2, 100, 10, 1, 1, 3, 0, 0, &g)) return 1;
    if (!hsum_geo(0, 100, 10, 1, 1, 3, 0, 0, &g)) return 2;                               // no spectra
    if (!hsum_geo(2, 0, 10, 1, 0, 3, 0, 0, &g) || !hsum_geo(1, (1 << 24) + 1, 10, 1, 1, 3, 0, 0, &g)) return 3;
    if (hsum_geo(1, 1 << 24, 65536, 6, (1 << 24) - 1, 1, 0, 0, &g)) return 4;
    if (!hsum_geo(2, 100, 0, 1, 1, 3, 0, 0, &g) || !hsum_geo(2, 100, 65537, 1, 1, 3, 0, 0, &g)) return 5;
    if (!hsum_geo(2, 100, 10, 0, 1, 3, 0, 0, &g) || !hsum_geo(2, 100, 10, 7, 1, 3, 0, 0, &g)) return 6;
    if (!hsum_geo(2, 100, 10, 1, -1, 3, 0, 0, &g) || !hsum_geo(2, 100, 10, 1, 100, 3, 0, 0, &g)) return 7;
    if (hsum_geo(2, 100, 10, 1, 99, 3, 0, 0, &g) || hsum_geo(2, 1, 1, 1, 0, 1, 0, 0, &g)) return 8;
    if (!hsum_geo(2, 100, 10, 1, 1, 0, 0, 0, &g)) return 9;
    if (!hsum_geo(2, 100, 10, 1, 1, 3, 48, 0, &g) || !hsum_geo(2, 100, 10, 1, 1, 3, 0, 3, &g)) return 10;
    if (!hsum_sizes(0, 1, 1, 0, 1) || !hsum_sizes(1, 0, 1, 0, 1) || !hsum_sizes(1, 1, 0, 0, 1) ||
        !hsum_sizes(1, 1, 1, 1, 1) || !hsum_sizes(1, 1, 1, 0, 0) || hsum_sizes(1 << 24, 65536, 6, 0, 1))
        return 11;
    if (hsum_whiten_geo(3, 100, 5, 2, 1, 0, &w) || !hsum_whiten_geo(3, 100, 5, 1, 1, 0, &w) ||
        !hsum_whiten_geo(3, 100, 5, 65537, 1, 0, &w) || hsum_whiten_geo(3, 100, 5, 65536, 0, 16, &w) ||
        !hsum_whiten_geo(0, 100, 5, 2, 1, 0, &w) || !hsum_whiten_geo(3, 0, 5, 2, 0, 0, &w) ||
        !hsum_whiten_geo(3, 100, 0, 2, 1, 0, &w) || !hsum_whiten_geo(3, 100, 5, 2, -1, 0, &w) ||
        !hsum_whiten_geo(3, 100, 5, 2, 100, 0, &w) || hsum_whiten_geo(3, 100, 5, 2, 99, 0, &w) ||
        !hsum_whiten_geo(3, 100, 5, 2, 1, 3, &w) || hsum_whiten_geo(1, 1, 1, 2, 0, 1, &w))
        return 12;
    // the gathered bins of level L are round_half_up(j i / 2^L), i = 1 ... 2^L: the even i are the level below
    for (int j : {0, 1, 2, 3, 323, 1500, (1 << 24) - 1})
        for (int L = 1; L < BBT_HSUM_MAX_LEVELS; ++L)
            for (int i = 1; i <= (1 << L); ++i) {
                const long long want = ((long long)j * i * 2 + (1ll << L)) / (2ll << L);        // floor(j i / 2^L + 1/2)
                if (hsum_bin(j, i, L) != want) return 13;
                if (i % 2 == 0 && hsum_bin(j, i, L) != hsum_bin(j, i / 2, L - 1)) return 14;
            }
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
            HsumGeo g = {};
            const char* err = hsum_geo(a[1], a[2], a[3], a[4], a[5], a[6], (int)a[7], (int)a[8], &g);
            if (err) {
                printf("{\"error\": \"%s\"}\n", err);
                continue;
            }
            const int w = walk_search(g);
            if (w) status = 1;
            printf("{\"nb\": %lld, \"n_pair\": %lld, \"nx\": %d, \"ny\": %d, \"sub\": %d, \"nz\": %d, \"n_tile\": %lld, "
                   "\"n_wg\": %lld, \"walk\": %d}\n",
                   g.nb, g.n_pair, g.nx, g.ny, g.sub, g.nz, g.n_tile, g.n_wg, w);
        } else {
            WhitenGeo g = {};
            const char* err = hsum_whiten_geo(a[1], a[2], a[3], a[4], a[5], (int)a[6], &g);
            if (err) {
                printf("{\"error\": \"%s\"}\n", err);
                continue;
            }
            const int w = walk_whiten(g);
            if (w) status = 1;
            printf("{\"nx\": %d, \"ny\": %d, \"n_tile\": %lld, \"n_blk\": %lld, \"n_wg\": %lld, \"walk\": %d}\n", g.nx,
                   g.ny, g.n_tile, g.n_blk, g.n_wg, w);
        }
    }
    return status;
}
