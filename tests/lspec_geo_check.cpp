// Host walk of csrc/lspec_geo.hpp, the index arithmetic of LongSpectra's two kernels, built with
// -fsanitize=address,undefined by tests/test_lspec_host.py.
//
//   lspec_geo_check walk N N_ELEM PER [N N_ELEM PER ...]
//       one JSON line per triple: the geometry of a call that takes PER column pairs a launch, and
//       "walk": 0 if, in every launch walked (all of them if the call is small, else the first
//       and the last), every input sample of the launch's columns is read exactly once, every
//       scratch cell is written once and read once, every output bin 0 ... N / 2 of every column of the
//       launch is written exactly once by the side that holds its partner N - k, every LDS cell of a
//       workgroup is filled once and every address lies inside its buffer.  A line with "error" for sizes
//       the library refuses.
//   lspec_geo_check maps N DIR
//       writes the index maps of one column pair (N_ELEM = 2, one launch) as raw int32 files into DIR,
//       for the NumPy model of the decomposition, and prints their sizes as one JSON line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lspec_geo.hpp"

static int fail(const char* what, long long a, long long b) {
    std::fprintf(stderr, "lspec_geo_check: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

struct Seen {
    long long max_in = -1, max_out = -1;
};

// 0 if launch i of the call is sound
static int walk_launch(long long n, long long n_elem, long long per, long long i, Seen* seen) {
    LspecGeo g = {};
    const char* err = lspec_geo(n, n_elem, per, i, &g);
    if (err) return fail(err, n, i);
    const long long P = g.P, nbin = n / 2 + 1;
    if (n * P > (1ll << 25)) return fail("too large a launch to walk", n, P);
    if ((long long)g.n1 * g.n2 != n || g.n1 * g.c1 > BBT_LSPEC_LDS_CELLS || g.n2 * 2 * g.cp > BBT_LSPEC_LDS_CELLS ||
        BBT_LSPEC_THREADS % g.c1 || BBT_LSPEC_THREADS % (2 * g.cp) || g.n2 % g.c1 || (1 << g.log2c1) != g.c1 ||
        (1 << g.log2cp) != g.cp || g.n_wg1 * g.c1 != g.n2 * P || g.n_wg1 >= (1ll << 31) || g.n_wg2 >= (1ll << 31))
        return fail("bad geometry", g.n1, g.n2);
    std::vector<unsigned char> c_in((size_t)(n * 2 * P)), c_w((size_t)(n * P)), c_r((size_t)(n * P)),
        c_out((size_t)(nbin * 2 * P)), lds(BBT_LSPEC_LDS_CELLS);
    const long long n_in_total = n * n_elem, n_out_total = nbin * n_elem;
    // pass 1
    for (long long wg = 0; wg < g.n_wg1; ++wg) {
        std::memset(lds.data(), 0, lds.size());
        for (int c = 0; c < g.c1; ++c) {
            LspecCol o;
            lspec_col(g, wg, c, &o);
            if (o.b < 0 || o.b >= g.n2 || o.pl < 0 || o.pl >= P) return fail("column outside the launch", wg, c);
            for (int a = 0; a < g.n1; ++a) {
                for (int half = 0; half < 2; ++half) {
                    const long long at = lspec_in_index(g, o, a, half);
                    if (at < 0) {
                        if (!(half == 1 && 2 * (g.p0 + o.pl) + 1 == n_elem)) return fail("a sample left out", wg, a);
                        continue;
                    }
                    if (at >= n_in_total) return fail("input index outside", at, n_in_total);
                    const long long t = at / n_elem, e = at % n_elem - 2 * g.p0;
                    if (t != (long long)a * g.n2 + o.b || e != 2 * o.pl + half) return fail("wrong sample", at, t);
                    ++c_in[(size_t)(t * 2 * P + e)];
                    if (at > seen->max_in) seen->max_in = at;
                }
                const int cell = lspec_lds1(g, a, c);
                if (cell < 0 || cell >= g.n1 * g.c1) return fail("LDS cell outside (first pass)", cell, a);
                ++lds[(size_t)cell];
            }
            for (int k1 = 0; k1 < g.n1; ++k1) {
                const int pos = lspec_pos1(g, k1);
                if (pos < 0 || pos >= g.n1 || lspec_brev(pos, g.log2n1) != k1) return fail("bad position", pos, k1);
                if (++lds[(size_t)lspec_lds1(g, pos, c)] != 2) return fail("LDS cell not read once", pos, c);
                const int m = lspec_tw_exp(g, o.b, k1);
                if (m < 0 || m >= n || (m >> BBT_LSPEC_TW_LO_LOG2) >= n >> BBT_LSPEC_TW_LO_LOG2 ||
                    m != (int)(((long long)o.b * k1) % n))
                    return fail("twiddle exponent outside", m, n);
                const long long cell = lspec_scratch(g, k1, o.col);
                if (cell < 0 || cell >= n * P) return fail("scratch cell outside (write)", cell, n * P);
                ++c_w[(size_t)cell];
            }
        }
    }
    // pass 2
    for (long long wg = 0; wg < g.n_wg2; ++wg) {
        std::memset(lds.data(), 0, lds.size());
        const int h = lspec_h(g, wg);
        const long long pl0 = lspec_pl0(g, wg);
        if (h < 0 || h >= g.n1 / 2 || pl0 < 0 || pl0 >= P) return fail("workgroup outside", wg, h);
        for (int ri = 0; ri < 2; ++ri)
            for (int s = 0; s < g.cp; ++s) {
                const long long pl = pl0 + s;
                const int row = lspec_row(g, h, ri);
                if (row < 0 || row >= g.n1) return fail("row outside", row, h);
                for (int b = 0; b < g.n2; ++b) {
                    const int cell = lspec_lds2(g, b, ri, s);
                    if (cell < 0 || cell >= g.n2 * 2 * g.cp) return fail("LDS cell outside (last pass)", cell, b);
                    ++lds[(size_t)cell];
                    if (pl >= P) continue;
                    const long long at = lspec_scratch(g, row, (long long)b * P + pl);
                    if (at < 0 || at >= n * P) return fail("scratch cell outside (read)", at, n * P);
                    ++c_r[(size_t)at];
                }
            }
        for (int ri = 0; ri < 2; ++ri)
            for (int s = 0; s < g.cp; ++s) {
                const long long pl = pl0 + s;
                if (pl >= P) continue;
                for (int k2 = 0; k2 <= g.n2 / 2; ++k2) {
                    if (!lspec_writes(g, h, ri, k2)) continue;
                    int rj = -1, k2j = -1;
                    lspec_partner(g, h, ri, k2, &rj, &k2j);
                    if (rj < 0 || rj > 1 || k2j < 0 || k2j >= g.n2) return fail("partner outside", rj, k2j);
                    const long long k = lspec_bin(g, h, ri, k2), kj = lspec_bin(g, h, rj, k2j);
                    if (k < 0 || k > n / 2 || (k + kj) % n != 0 || kj >= n) return fail("not the partner", k, kj);
                    const int pa = lspec_pos2(g, k2), pb = lspec_pos2(g, k2j);
                    if (pa < 0 || pa >= g.n2 || pb < 0 || pb >= g.n2 || lspec_brev(pa, g.log2n2) != k2)
                        return fail("bad position (last pass)", pa, pb);
                    if (lds[(size_t)lspec_lds2(g, pa, ri, s)] != 1 || lds[(size_t)lspec_lds2(g, pb, rj, s)] != 1)
                        return fail("reads an LDS cell nobody filled", pa, pb);
                    for (int half = 0; half < 2; ++half) {
                        const long long at = lspec_out_index(g, k, pl, half);
                        if (at < 0) {
                            if (!(half == 1 && 2 * (g.p0 + pl) + 1 == n_elem)) return fail("a bin left out", k, pl);
                            continue;
                        }
                        if (at >= n_out_total) return fail("output index outside", at, n_out_total);
                        if (at / n_elem != k || at % n_elem != 2 * (g.p0 + pl) + half) return fail("wrong bin", at, k);
                        ++c_out[(size_t)(k * 2 * P + 2 * pl + half)];
                        if (at > seen->max_out) seen->max_out = at;
                    }
                }
            }
        for (int cell = 0; cell < g.n2 * 2 * g.cp; ++cell)
            if (lds[(size_t)cell] != 1) return fail("LDS cell not filled once", cell, wg);
    }
    const bool odd_here = (n_elem & 1) && g.p0 + P == g.n_pair;
    for (long long t = 0; t < n; ++t)
        for (long long e = 0; e < 2 * P; ++e)
            if (c_in[(size_t)(t * 2 * P + e)] != ((odd_here && e == 2 * P - 1) ? 0 : 1))
                return fail("input sample not read once", t, e);
    for (long long c = 0; c < n * P; ++c)
        if (c_w[(size_t)c] != 1 || c_r[(size_t)c] != 1) return fail("scratch cell not written and read once", c, c_w[(size_t)c]);
    for (long long k = 0; k < nbin; ++k)
        for (long long e = 0; e < 2 * P; ++e)
            if (c_out[(size_t)(k * 2 * P + e)] != ((odd_here && e == 2 * P - 1) ? 0 : 1))
                return fail("output bin not written once", k, e);
    return 0;
}

static int walk(long long n, long long n_elem, long long per) {
    const char* err = lspec_sizes(n, 1, n_elem);
    LspecGeo g = {};
    if (!err) err = lspec_geo(n, n_elem, per, 0, &g);
    if (err) {
        std::printf("{\"error\": \"%s\"}\n", err);
        return 0;
    }
    const long long n_launch = lspec_n_launch(n_elem, per);
    // the launches tile the pairs
    long long next = 0;
    for (long long i = 0; i < n_launch; ++i) {
        LspecGeo l = {};
        if (lspec_geo(n, n_elem, per, i, &l) || l.p0 != next || l.P < 1 || l.P > per) return fail("launch list", i, next);
        next += l.P;
    }
    if (next != g.n_pair || lspec_geo(n, n_elem, per, n_launch, &g) == 0) return fail("launch list end", next, n_launch);
    lspec_geo(n, n_elem, per, 0, &g);
    Seen seen;
    int bad = 0;
    long long walked = 0;
    if (n * g.n_pair <= (1ll << 23)) {
        for (long long i = 0; i < n_launch && !bad; ++i, ++walked) bad = walk_launch(n, n_elem, per, i, &seen);
    } else {
        long long last = -1;
        for (long long i : {0ll, n_launch - 1}) {
            if (i == last || bad) continue;
            bad = walk_launch(n, n_elem, per, i, &seen);
            last = i, ++walked;
        }
    }
    std::printf("{\"n\": %lld, \"n_elem\": %lld, \"per\": %lld, \"n1\": %d, \"n2\": %d, \"c1\": %d, \"cp\": %d, "
                "\"n_launch\": %lld, \"walked\": %lld, \"n_wg1\": %lld, \"n_wg2\": %lld, \"max_in\": %lld, "
                "\"max_out\": %lld, \"walk\": %d}\n",
                n, n_elem, per, g.n1, g.n2, g.c1, g.cp, n_launch, walked, g.n_wg1, g.n_wg2, seen.max_in, seen.max_out, bad);
    return 0;
}

static int dump(const std::string& dir, const char* name, const std::vector<int>& v) {
    const std::string path = dir + "/" + name + ".i32";
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return fail("cannot write a map", 0, 0);
    const size_t done = std::fwrite(v.data(), sizeof(int), v.size(), f);
    std::fclose(f);
    return done == v.size() ? 0 : fail("short write", (long long)done, (long long)v.size());
}

static int maps(long long n, const std::string& dir) {
    LspecGeo g = {};
    const char* err = lspec_geo(n, 2, 1, 0, &g);
    if (err) return fail(err, n, 0);
    const int n1 = g.n1, n2 = g.n2, nk = n2 / 2 + 1;
    std::vector<int> in_t((size_t)n), pos1((size_t)n1), exp1((size_t)n), cell1((size_t)n);
    for (long long wg = 0; wg < g.n_wg1; ++wg)
        for (int c = 0; c < g.c1; ++c) {
            LspecCol o;
            lspec_col(g, wg, c, &o);
            for (int a = 0; a < n1; ++a) in_t[(size_t)o.b * n1 + a] = (int)(lspec_in_index(g, o, a, 0) / 2);
            for (int k1 = 0; k1 < n1; ++k1) {
                exp1[(size_t)k1 * n2 + o.b] = lspec_tw_exp(g, o.b, k1);
                cell1[(size_t)k1 * n2 + o.b] = (int)lspec_scratch(g, k1, o.col);
            }
        }
    for (int k1 = 0; k1 < n1; ++k1) pos1[(size_t)k1] = lspec_pos1(g, k1);
    const int nh = n1 / 2;
    std::vector<int> rows((size_t)nh * 2), cell2((size_t)nh * 2 * n2), pos2((size_t)n2), partner((size_t)nh * 2 * nk * 2),
        bin((size_t)nh * 2 * nk);
    for (int k2 = 0; k2 < n2; ++k2) pos2[(size_t)k2] = lspec_pos2(g, k2);
    for (long long wg = 0; wg < g.n_wg2; ++wg) {
        const int h = lspec_h(g, wg);
        const long long pl = lspec_pl0(g, wg);
        for (int ri = 0; ri < 2; ++ri) {
            const size_t hr = (size_t)h * 2 + ri;
            rows[hr] = lspec_row(g, h, ri);
            for (int b = 0; b < n2; ++b) cell2[hr * n2 + b] = (int)lspec_scratch(g, rows[hr], (long long)b * g.P + pl);
            for (int k2 = 0; k2 < nk; ++k2) {
                int rj = 0, k2j = 0;
                lspec_partner(g, h, ri, k2 < n2 ? k2 : 0, &rj, &k2j);
                partner[(hr * nk + k2) * 2] = rj, partner[(hr * nk + k2) * 2 + 1] = k2j;
                bin[hr * nk + k2] = lspec_writes(g, h, ri, k2) ? (int)lspec_bin(g, h, ri, k2) : -1;
            }
        }
    }
    if (dump(dir, "in_t", in_t) || dump(dir, "pos1", pos1) || dump(dir, "exp1", exp1) || dump(dir, "cell1", cell1) ||
        dump(dir, "rows", rows) || dump(dir, "cell2", cell2) || dump(dir, "pos2", pos2) || dump(dir, "partner", partner) ||
        dump(dir, "bin", bin))
        return 1;
    std::printf("{\"n\": %lld, \"n1\": %d, \"n2\": %d, \"n_wg1\": %lld, \"n_wg2\": %lld}\n", n, n1, n2, g.n_wg1, g.n_wg2);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "maps")) return maps(std::atoll(argv[2]), argv[3]);
    if (argc < 5 || std::strcmp(argv[1], "walk") || (argc - 2) % 3) {
        std::fprintf(stderr, "usage: lspec_geo_check walk N N_ELEM PER ... | maps N DIR\n");
        return 2;
    }
    for (int i = 2; i + 2 < argc; i += 3)
        if (walk(std::atoll(argv[i]), std::atoll(argv[i + 1]), std::atoll(argv[i + 2]))) return 1;
    return 0;
}
