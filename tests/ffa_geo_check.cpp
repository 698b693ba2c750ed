// Walks the tiling of the fast-folding search kernels (csrc/ffa_geo.hpp) on the host, for
// test_ffa_host.py: built with -fsanitize=address,undefined, no GPU.
//
//   ffa_geo_check  n p_lo p_hi p K pitch e0 ne fuse width  [ten more numbers ...]
//
// One launch of the plan (n, p_lo, p_hi, K, pitch elements) at base period p for the columns e0 ... e0 + ne.
// Per shape one JSON line: the geometry and "walk", 0 if
//   - the plan's scratch holds the running segment sums, the c_k and two buffers of M lane floats side by side,
//   - in every transform pass every (row, lane tile) of the output is written by exactly one workgroup,
//     every rotated lane lies in [0, lane), pass 0 reads only rows < m at samples < m p <= n of the columns
//     e0 ... e0 + ne of the block, later passes read rows < M of a buffer, and the stages add up to log2(M),
//   - for rows up to 1024 the rotations of the fused passes compose to ffa_shift(r, t, M) for every (r, t),
//   - in the S/N pass every (row, column) is held by exactly one workgroup, a tile fits the LDS buffer, a
//     boxcar step stays inside its row, every read lies in the buffer and every partial winner in the other,
//   - the cells of the result written are those of the period and the columns, inside [p_hi - p_lo][4][pitch];
// or {"error": ...} where the geometry refuses the shape.  Exit status 1 if any of that fails.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ffa_geo.hpp"

static int walk(const FfaGeo& g, long long p_lo, long long p_hi, long long e0) {
    const long long max_mp = ffa_max_mp(g.n, p_lo, p_hi);
    if (g.m != g.n / g.p || g.M < g.m || g.M / 2 >= g.m || (1ll << g.L) != g.M) return 1;
    if (g.lane != g.p * g.ne || g.buf != g.M * g.lane || g.buf > max_mp * g.ne) return 2;
    // the running segment sums: one double in front of every whole segment and the last; the one k_ffa_total reads
    if (ffa_prefix(g.n) != g.n / BBT_FFA_SEG + 1 || g.m * g.p / BBT_FFA_SEG >= ffa_prefix(g.n) || g.m * g.p > g.n) return 6;
    if (ffa_scratch(g.n, max_mp, g.ne) != (2 * ffa_prefix(g.n) + BBT_FFA_MAX_WIDTHS + 2 * max_mp) * g.ne || g.K > BBT_FFA_MAX_WIDTHS)
        return 3;
    if (g.n_pass != (g.L + g.fuse - 1) / g.fuse || g.n_pass < 1) return 4;
    if (g.n_lt * BBT_FFA_THREADS < g.lane || (g.n_lt - 1) * BBT_FFA_THREADS >= g.lane) return 5;
    const long long block = g.n * g.pitch;

    // the rotation of data row r in row t so far, for small M: sh[t * M + r]
    const bool compose = g.M <= 1024 && (g.M / 2) * g.n_lt <= (1ll << 22);      // (and every workgroup is walked)
    std::vector<long long> sh, sh_new;
    if (compose) sh.assign((size_t)(g.M * g.M), 0), sh_new.assign((size_t)(g.M * g.M), 0);

    int stages = 0;
    for (int q = 0; q < g.n_pass; ++q) {
        const FfaPass ps = ffa_pass(g, q);
        if (ps.s0 != stages || ps.lv < 1 || ps.lv > g.fuse || ps.s0 + ps.lv > g.L) return 10;
        if (ps.n_wg != (g.M >> ps.lv) * g.n_lt) return 11;
        const int nl = 1 << ps.lv;
        // (all workgroups where that is quick; else some 4000 of them, the first and the last included)
        const long long stride = ps.n_wg > (1ll << 22) ? ps.n_wg / 4099 : 1;
        const long long walked = stride == 1 ? ps.n_wg : 4100;
        std::vector<unsigned char> seen((size_t)(stride == 1 ? g.M * g.n_lt : 1), 0);
        for (long long i = 0; i < walked; ++i) {
            const long long wg = i + 1 == walked ? ps.n_wg - 1 : i * stride;
            FfaOwn o;
            ffa_own(g, wg, ps.s0, ps.lv, &o);
            if (o.x0 < 0 || o.x0 >= g.lane || o.x0 % BBT_FFA_THREADS || o.tq < 0 || o.tq >= (1ll << ps.s0)) return 12;
            const int x_last = o.x0 + BBT_FFA_THREADS - 1 < g.lane ? o.x0 + BBT_FFA_THREADS - 1 : g.lane - 1;
            for (int v = 0; v < nl; ++v) {
                const long long t = (o.tq << ps.lv) + v, out_row = o.out0 + v;
                if (out_row < 0 || out_row >= g.M) return 13;
                if (stride == 1) {
                    unsigned char& s = seen[(size_t)(out_row * g.n_lt + o.x0 / BBT_FFA_THREADS)];
                    if (s) return 14;
                    s = 1;
                }
                if (out_row * g.lane + x_last >= g.buf) return 15;
                for (int u = 0; u < nl; ++u) {
                    const long long row = o.in0 + ((long long)u << ps.s0);
                    if (row < 0 || row >= g.M) return 16;
                    const long long shift = ffa_leaf_shift(t, u, ps.lv);
                    const int c = (int)(shift % g.p);
                    if (shift < 0 || (long long)c * g.ne >= g.lane) return 17;
                    for (int x = o.x0;; x = x_last) {
                        int at = x + c * (int)g.ne;
                        if (at >= g.lane) at -= g.lane;
                        if (at < 0 || at >= g.lane) return 18;
                        if (q == 0) {
                            if (row < g.m) {
                                const long long where = e0 + ffa_in_at(g, row, at);
                                if (where < 0 || where >= block) return 19;
                                const long long sample = where / g.pitch, col = where % g.pitch;
                                if (sample >= g.m * g.p || sample != row * g.p + at / g.ne) return 20;
                                if (col < e0 || col >= e0 + g.ne || col != e0 + at % g.ne) return 21;
                            }
                        } else if (row * g.lane + at >= g.buf) {
                            return 22;
                        }
                        if (x == x_last) break;
                    }
                    if (compose && o.x0 == 0) {
                        // the leaf is row `row` of the pass before: group of 2^s0 rows, its row tq
                        const long long g0 = 1ll << ps.s0, base = row - o.tq;
                        for (long long r = 0; r < g0; ++r)
                            sh_new[(size_t)(out_row * g.M + base + r)] = sh[(size_t)(row * g.M + base + r)] + shift;
                    }
                }
            }
        }
        if (stride == 1)
            for (unsigned char s : seen)
                if (!s) return 23;
        if (compose) sh.swap(sh_new);
        stages += ps.lv;
    }
    if (stages != g.L) return 24;
    if (compose)
        for (long long t = 0; t < g.M; ++t)
            for (long long r = 0; r < g.M; ++r)
                if (sh[(size_t)(t * g.M + r)] != ffa_shift(r, t, g.M)) return 25;

    // the S/N pass
    if (g.ex < 1 || g.ex > 32 || BBT_FFA_THREADS % g.ex || g.nr < 1 || (long long)g.nr * g.p * g.ex > BBT_FFA_CAP) return 30;
    if (g.n_et * g.ex < g.ne || (g.n_et - 1) * g.ex >= g.ne || g.n_rg * g.nr < g.M || (g.n_rg - 1) * g.nr >= g.M) return 31;
    if (4 * BBT_FFA_THREADS > BBT_FFA_CAP) return 32;                     // (the winners of the threads reuse a buffer)
    long long rows_held = 0;
    for (long long rg = 0; rg < g.n_rg; ++rg) {
        const long long r0 = rg * g.nr;
        const long long rows = g.M - r0 < g.nr ? g.M - r0 : g.nr;
        if (rows < 1) return 33;
        rows_held += rows;
        const long long pe = g.p * g.ex, tot = rows * pe;
        if (tot > BBT_FFA_CAP) return 34;
        for (int k = 0; k + 1 < g.K; ++k)
            if (((long long)g.ex << k) >= pe) return 35;
        for (long long tile = 0; tile < g.n_et; tile += (g.n_et > 4 && tile == 1) ? g.n_et - 3 : 1) {
            const long long ge_last = (tile + 1) * g.ex - 1 < g.ne ? (tile + 1) * g.ex - 1 : g.ne - 1;
            if (tile * g.ex >= g.ne) return 36;
            const long long last = (r0 + rows - 1) * g.lane + (g.p - 1) * g.ne + ge_last;
            if (last >= g.buf) return 37;
            if ((rg * 4 + 3) * g.ne + ge_last >= g.buf) return 38;
        }
    }
    if (rows_held != g.M) return 39;

    // the result
    const long long cells = (p_hi - p_lo) * 4 * g.pitch;
    const long long first = (g.p - p_lo) * 4 * g.pitch + e0, last = first + 3 * g.pitch + g.ne - 1;
    if (first < 0 || last >= cells) return 40;
    return 0;
}

int main(int argc, char** argv) {
    if ((argc - 1) % 10) {
        fprintf(stderr, "ten numbers per shape\n");
        return 2;
    }
    if (BBT_FFA_CAP < BBT_FFA_MAX_P - 1 || 2 * BBT_FFA_CAP * (int)sizeof(float) > 65536) return 1;
    int bad = 0;
    for (int i = 1; i + 9 < argc; i += 10) {
        long long v[10];
        for (int j = 0; j < 10; ++j) v[j] = atoll(argv[i + j]);
        const long long n = v[0], p_lo = v[1], p_hi = v[2], p = v[3], K = v[4], pitch = v[5], e0 = v[6], ne = v[7];
        const char* err = ffa_sizes(n, p_lo, p_hi, K, pitch);
        if (!err && (p < p_lo || p >= p_hi)) err = "the period is not one of the plan's";
        FfaGeo g;
        memset(&g, 0, sizeof g);
        if (!err) err = ffa_geo(n, p, K, pitch, e0, ne, (int)v[8], (int)v[9], &g);
        if (err) {
            printf("{\"error\": \"%s\"}\n", err);
            continue;
        }
        const int w = walk(g, p_lo, p_hi, e0);
        if (w) bad = 1;
        printf("{\"m\": %lld, \"M\": %lld, \"L\": %d, \"lane\": %d, \"fuse\": %d, \"n_pass\": %d, \"ex\": %d, \"nr\": %d, "
               "\"n_et\": %lld, \"n_rg\": %lld, \"buf\": %lld, \"scales\": [",
               g.m, g.M, g.L, g.lane, g.fuse, g.n_pass, g.ex, g.nr, g.n_et, g.n_rg, g.buf);
        for (int k = 0; k < g.K; ++k) {
            unsigned bits;
            memcpy(&bits, &g.a[k], 4);
            printf("%s%u", k ? ", " : "", bits);
        }
        printf("], \"walk\": %d}\n", w);
    }
    return bad;
}
