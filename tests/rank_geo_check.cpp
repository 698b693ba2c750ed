// Walks the tiling of the block median / MAD kernels (csrc/rank_geo.hpp) on the host and runs the host
// restatement of the key map and of the digit descent against brute-force sorting, for
// test_rank_host.py: built with -fsanitize=address,undefined, no GPU.
//
//   rank_geo_check  n_spec nbin n_elem m skip width digit route  [eight more numbers ...]
//
// Before the shapes: the limits and refusals, and the descent -- the very rank_key, rank_fixed_mask,
// rank_pick and rank_mid the kernel calls, driven by a loop that restates the kernel's (a histogram per
// digit over the keys that match the prefix, the minimum above lo's key for an even count, the second
// descent over |x - med|) -- on a few thousand random and planted blocks, blocks of 65536 equal values
// among them, for both digit widths, each compared with the sorted keys bit for bit.
// Per shape one JSON line: the geometry and "walk", 0 if
//   - every (spectrum, block, element tile) is owned by exactly one workgroup, the element tiles cover
//     the elements, and the blocks of a spectrum tile its rows from `skip` on, the last one ragged,
//   - every row a workgroup reads lies inside its spectrum and so inside the chunk, every address inside
//     the arrays, the rows it zeroes are the `skip` rows of its spectrum and only block 0 has any,
//   - the LDS of a workgroup is within the budget and, on the lds route, holds the longest block,
// or {"error": ...} where the geometry refuses the shape.  Exit status 1 if any of that fails.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rank_geo.hpp"

static float as_float(unsigned bits) {
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
static unsigned as_bits(float f) {
    unsigned b;
    memcpy(&b, &f, 4);
    return b;
}

// the key of value t of a block: x itself, or |x - center| (one rounded float32 subtract, the sign cleared)
static unsigned key_of(const std::vector<unsigned>& x, size_t t, bool dev, float center) {
    unsigned bits = x[t];
    if (dev) {
        volatile float d = as_float(bits) - center;
        bits = as_bits(d) & 0x7fffffffu;
    }
    return rank_key(bits);
}

// the kernel's descent, one column
static float descent_median(const std::vector<unsigned>& x, int digit, bool dev, float center) {
    const int len = (int)x.size(), nb = 1 << digit;
    std::vector<unsigned> hist((size_t)nb);
    unsigned prefix = 0;
    int k = (len - 1) >> 1, equal = 0;
    for (int shift = 32 - digit; shift >= 0; shift -= digit) {
        std::fill(hist.begin(), hist.end(), 0u);
        const unsigned fixed = rank_fixed_mask(shift, digit);
        for (int t = 0; t < len; ++t) {
            const unsigned key = key_of(x, (size_t)t, dev, center);
            if (((key ^ prefix) & fixed) == 0u) hist[(key >> shift) & (unsigned)(nb - 1)] += 1u;
        }
        const int d = rank_pick(hist.data(), nb, 1, &k, &equal);
        prefix |= (unsigned)d << shift;
    }
    unsigned hi = prefix;
    if (!(len & 1)) {
        unsigned least = 0xffffffffu;
        for (int t = 0; t < len; ++t) {
            const unsigned key = key_of(x, (size_t)t, dev, center);
            if (key > prefix && key < least) least = key;
        }
        if (k + 1 >= equal) hi = least;
    }
    return rank_mid(as_float(rank_unkey(prefix)), as_float(rank_unkey(hi)));
}

// brute force: the keys sorted
static float sorted_median(const std::vector<unsigned>& x, bool dev, float center) {
    std::vector<unsigned> keys(x.size());
    for (size_t t = 0; t < x.size(); ++t) keys[t] = key_of(x, t, dev, center);
    std::sort(keys.begin(), keys.end());
    const size_t len = keys.size();
    const float lo = as_float(rank_unkey(keys[(len - 1) / 2])), hi = as_float(rank_unkey(keys[len / 2]));
    return (float)(((double)lo + (double)hi) * 0.5);
}

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd() {
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (unsigned)(g_state >> 24);
}

static int check_block(const std::vector<unsigned>& x) {
    for (int digit = 4; digit <= 8; digit += 4) {
        const float med = descent_median(x, digit, false, 0.f), want = sorted_median(x, false, 0.f);
        if (as_bits(med) != as_bits(want)) return 1;
        const float mad = descent_median(x, digit, true, med), want_mad = sorted_median(x, true, med);
        if (as_bits(mad) != as_bits(want_mad)) return 2;
    }
    return 0;
}

static int descents() {
    // the key map: monotone on ordered values, -0 just before +0, and its own inverse
    const float ordered[] = {-INFINITY, -3.4028235e38f, -1.f, -1e-45f, -0.f, 0.f, 1e-45f, 1.f, 3.4028235e38f, INFINITY};
    for (size_t i = 0; i + 1 < sizeof ordered / sizeof *ordered; ++i)
        if (!(rank_key(as_bits(ordered[i])) < rank_key(as_bits(ordered[i + 1])))) return 1;
    if (rank_key(as_bits(-0.f)) + 1u != rank_key(as_bits(0.f))) return 2;
    for (int i = 0; i < 100000; ++i) {
        const unsigned b = rnd();
        if (rank_unkey(rank_key(b)) != b) return 3;
    }
    if (!rank_not_finite(0x7f800000u) || !rank_not_finite(0xffc00000u) || rank_not_finite(0x7f7fffffu)) return 4;
    if (rank_fixed_mask(28, 4) != 0u || rank_fixed_mask(24, 8) != 0u || rank_fixed_mask(24, 4) != 0xf0000000u ||
        rank_fixed_mask(0, 8) != 0xffffff00u)
        return 5;
    // random and planted blocks
    std::vector<unsigned> x;
    for (int trial = 0; trial < 3000; ++trial) {
        const int len = 1 + (int)(rnd() % (trial % 10 == 0 ? 3000u : 70u));
        const int kind = trial % 7;
        x.resize((size_t)len);
        for (int t = 0; t < len; ++t) {
            switch (kind) {
                case 0: x[(size_t)t] = rnd(); break;                                         // any bits, NaN included
                case 1: x[(size_t)t] = as_bits((float)((int)(rnd() % 9u) - 4)); break;          // heavy ties
                case 2: x[(size_t)t] = as_bits(1.f) + rnd() % 4u; break;                       // the last mantissa bits
                case 3: x[(size_t)t] = (rnd() & 1u) << 31; break;                              // -0 and +0
                case 4: x[(size_t)t] = (rnd() % 100u) | ((rnd() & 1u) << 31); break;           // denormals and zeros
                case 5: x[(size_t)t] = rnd() % 3u ? 0x7f7fffffu : as_bits((float)t); break;     // the largest float
                default: x[(size_t)t] = as_bits((float)(rnd() % 100000u) * 1e-3f - 50.f); break;
            }
        }
        const int c = check_block(x);
        if (c) return 10 + c;
    }
    // the counters: 65536 equal values, 32769 of them equal, and a permutation of 65536 distinct values
    x.assign(65536, as_bits(2.5f));
    if (check_block(x)) return 20;
    for (int t = 0; t < 32767; ++t) x[(size_t)(2 * t + 1)] = as_bits(3.f + (float)t);
    if (check_block(x)) return 21;
    for (int t = 0; t < 65536; ++t) x[(size_t)t] = as_bits((float)(((unsigned)t * 40503u) % 65536u) - 30000.f);
    if (check_block(x)) return 22;
    // two values of the largest float do not overflow
    x.assign(2, 0x7f7fffffu);
    if (as_bits(descent_median(x, 8, false, 0.f)) != 0x7f7fffffu) return 23;
    return 0;
}

static int validation() {
    RankGeo g;
    if (rank_geo(1, 100, 3, 10, 0, 0, 0, 0, &g)) return 1;
    if (!rank_geo(1, 100, 3, 1, 0, 0, 0, 0, &g) || !rank_geo(1, 100, 3, 65537, 0, 0, 0, 0, &g)) return 2;
    if (rank_geo(1, 65536, 3, 65536, 0, 0, 0, 0, &g) || g.route != BBT_RANK_ROUTE_GLOBAL || g.nblk != 1) return 3;
    if (!rank_geo(0, 100, 3, 10, 0, 0, 0, 0, &g) || !rank_geo(1, 0, 3, 10, 0, 0, 0, 0, &g)) return 4;
    if (!rank_geo(1, 100, 0, 10, 0, 0, 0, 0, &g)) return 5;
    if (!rank_geo(1, 100, 3, 10, 100, 0, 0, 0, &g) || !rank_geo(1, 100, 3, 10, -1, 0, 0, 0, &g)) return 6;
    if (rank_geo(1, 100, 3, 10, 99, 0, 0, 0, &g) || g.nblk != 1 || g.len_max != 1) return 7;
    if (!rank_geo(1, (1ll << 40) + 1, 3, 10, 0, 0, 0, 0, &g) || !rank_geo(1ll << 20, (1ll << 20) + 1, 3, 10, 0, 0, 0, 0, &g))
        return 8;                                                                  // more than 2^40 rows
    if (rank_geo(1, 1ll << 40, 3, 65536, 0, 0, 0, 0, &g) || g.n_wg != (1ll << 24)) return 9;          // 2^40 rows are taken
    const char* many = rank_geo(1, 1ll << 40, 3, 2, 0, 0, 0, 0, &g);
    if (!many || strcmp(many, "too many tiles for one launch")) return 9;
    if (rank_geo(1, 1ll << 30, 16, 2, 0, 0, 0, 0, &g) || !rank_geo(1, 1ll << 31, 65, 2, 0, 0, 0, 0, &g)) return 10;
    if (!rank_geo(1, 100, 3, 10, 0, 48, 0, 0, &g) || !rank_geo(1, 100, 3, 10, 0, 0, 5, 0, &g) ||
        !rank_geo(1, 100, 3, 10, 0, 0, 0, 3, &g))
        return 11;
    if (rank_std_geo(3, 2, 5, 0, 0, 0, &g) || !rank_std_geo(3, 1, 5, 0, 0, 0, &g) || !rank_std_geo(3, 65537, 5, 0, 0, 0, &g) ||
        !rank_std_geo(0, 2, 5, 0, 0, 0, &g) || !rank_std_geo(3, 2, 0, 0, 0, 0, &g) || !rank_std_geo(1ll << 39, 4, 1, 0, 0, 0, &g))
        return 12;
    // the routes: lds wherever the block fits, forced or not; global when asked or when it does not
    for (int w = 16; w <= 64; w *= 2)
        for (int d = 4; d <= 8; d += 4) {
            const long long rows = rank_lds_rows(w, d);
            if (rows < 2) return 13;
            if (rank_geo(1, rows, 3, rows, 0, w, d, 0, &g) || g.route != BBT_RANK_ROUTE_LDS || g.lds_bytes > BBT_RANK_LDS_BYTES)
                return 14;
            if (rank_geo(1, rows + 1, 3, rows + 1, 0, w, d, 1, &g) || g.route != BBT_RANK_ROUTE_GLOBAL) return 15;
            if (rank_geo(1, rows, 3, rows, 0, w, d, 2, &g) || g.route != BBT_RANK_ROUTE_GLOBAL) return 16;
            if (BBT_RANK_MISC_BYTES / 4 < 64 + w) return 17;                   // the minima at 0, the flags at 64
        }
    if (2 * BBT_RANK_LDS_BYTES > 160 * 1024) return 18;                       // two workgroups to a CU
    // the automatic width: no wider than the elements need, the widest that still fits the LDS, else 16
    if (rank_geo(1, 128, 512, 128, 0, 0, 0, 0, &g) || g.nx != 64 || g.route != BBT_RANK_ROUTE_LDS || g.digit != 4) return 19;
    if (rank_geo(1, 300, 512, 300, 0, 0, 0, 0, &g) || g.nx != 32 || g.route != BBT_RANK_ROUTE_LDS) return 20;
    if (rank_geo(1, 4096, 512, 4096, 0, 0, 0, 0, &g) || g.nx != 16 || g.route != BBT_RANK_ROUTE_GLOBAL || g.digit != 8) return 21;
    if (rank_geo(1, 128, 3, 128, 0, 0, 0, 0, &g) || g.nx != 16) return 22;
    return 0;
}

static int walk(const RankGeo& g) {
    if (g.nx * g.ny != BBT_RANK_THREADS) return 1;
    if (g.n_tile * g.nx < g.n_elem || (g.n_tile - 1) * g.nx >= g.n_elem) return 2;
    if (g.nblk != (g.nbin - g.skip + g.m - 1) / g.m || g.n_wg != g.n_spec * g.nblk * g.n_tile) return 3;
    if (g.digit != 4 && g.digit != 8) return 4;
    const long long fixed_bytes = rank_hist_bytes(g.nx, g.digit) + BBT_RANK_MISC_BYTES;
    if (g.lds_bytes > BBT_RANK_LDS_BYTES) return 5;
    if (g.route == BBT_RANK_ROUTE_LDS) {
        if (g.lds_bytes != fixed_bytes + g.len_max * g.nx * 4 || g.len_max > rank_lds_rows(g.nx, g.digit)) return 6;
    } else if (g.route != BBT_RANK_ROUTE_GLOBAL || g.lds_bytes != fixed_bytes) {
        return 7;
    }
    const long long total = g.n_spec * g.nbin * g.n_elem, cells = g.n_spec * g.nblk * g.n_elem;
    std::vector<unsigned char> seen((size_t)g.n_wg, 0);
    std::vector<long long> rows_of((size_t)(g.n_spec * g.n_tile), 0), zeroed((size_t)(g.n_spec * g.n_tile), 0);
    for (long long wg = 0; wg < g.n_wg; ++wg) {
        RankOwn o;
        rank_own(g, wg, &o);
        if (o.e0 < 0 || o.e0 % g.nx || o.e0 >= g.n_elem) return 10;
        const long long tile = o.e0 / g.nx;
        if (o.cell < 0 || o.cell >= g.n_spec * g.nblk) return 11;
        unsigned char& s = seen[(size_t)(o.cell * g.n_tile + tile)];
        if (s) return 12;
        s = 1;
        const long long spec = o.cell / g.nblk, b = o.cell % g.nblk;
        if (o.len < 1 || o.len > g.len_max || o.len > g.m) return 13;
        if (o.row0 != spec * g.nbin + g.skip + b * g.m) return 14;
        if (o.row0 < spec * g.nbin + g.skip || o.row0 + o.len > (spec + 1) * g.nbin) return 15;      // inside its spectrum
        if (b + 1 < g.nblk && o.len != g.m) return 16;                                                 // only the last is ragged
        const long long e_last = o.e0 + g.nx - 1 < g.n_elem ? o.e0 + g.nx - 1 : g.n_elem - 1;
        const long long at = (o.row0 + o.len - 1) * g.n_elem + e_last;
        if (at < 0 || at >= total || o.row0 * g.n_elem + o.e0 < 0) return 17;
        if (o.cell * g.n_elem + e_last >= cells) return 18;
        if (o.zero_rows != (b == 0 ? g.skip : 0) || o.zero0 != spec * g.nbin) return 19;
        if (o.zero_rows && o.zero0 + o.zero_rows != o.row0) return 20;                                 // right in front of block 0
        if (g.route == BBT_RANK_ROUTE_LDS &&
            fixed_bytes + ((long long)(o.len - 1) * g.nx + g.nx - 1) * 4 + 4 > g.lds_bytes)
            return 21;
        rows_of[(size_t)(spec * g.n_tile + tile)] += o.len;
        zeroed[(size_t)(spec * g.n_tile + tile)] += o.zero_rows;
    }
    for (unsigned char s : seen)
        if (!s) return 22;
    for (size_t i = 0; i < rows_of.size(); ++i)
        if (rows_of[i] != g.nbin - g.skip || zeroed[i] != g.skip) return 23;                           // every row once
    return 0;
}

int main(int argc, char** argv) {
    const int v = validation();
    if (v) {
        printf("{\"validation\": %d}\n", v);
        return 1;
    }
    const int d = descents();
    if (d) {
        printf("{\"descent\": %d}\n", d);
        return 1;
    }
    int status = 0;
    for (int i = 1; i + 8 <= argc; i += 8) {
        long long a[8];
        for (int k = 0; k < 8; ++k) a[k] = atoll(argv[i + k]);
        RankGeo g = {};
        const char* err = rank_geo(a[0], a[1], a[2], a[3], a[4], (int)a[5], (int)a[6], (int)a[7], &g);
        if (err) {
            printf("{\"error\": \"%s\"}\n", err);
            continue;
        }
        const int w = walk(g);
        if (w) status = 1;
        printf("{\"route\": %d, \"digit\": %d, \"nx\": %d, \"ny\": %d, \"nblk\": %lld, \"len_max\": %lld, \"n_tile\": %lld, "
               "\"n_wg\": %lld, \"lds_bytes\": %lld, \"walk\": %d}\n",
               g.route, g.digit, g.nx, g.ny, g.nblk, g.len_max, g.n_tile, g.n_wg, g.lds_bytes, w);
    }
    return status;
}
