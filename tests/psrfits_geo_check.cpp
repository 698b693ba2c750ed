// Host check of csrc/psrfits_geo.hpp, the tiling of the PSRFITS fold-mode kernels: for every shape
// given as "n_bin n_chan n_pol x_aligned16 codes_aligned4" (as arguments, or on standard input when
// there are none) it prints the geometry as a JSON line and walks the index arithmetic of
// k_psrfits_encode / k_psrfits_decode (psrfits_kernels.hpp) on the host, one row, every workgroup,
// every thread -- every s_tile, s_mn / s_mx / s_cnt and s_base index inside its array, the
// reduction tree reading only cells that were written and counting every bin of a column once,
// every float read once a pass and stored once, every code stored and loaded exactly once, no
// float4 and no dword of two codes across the end of a row, every vector access aligned.  Built by
// tests/test_psrfits_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "psrfits_geo.hpp"

namespace {

const int NT = BBT_PSRFITS_THREADS;

struct Row {
    long long n_bin, n_col;
    bool x_aligned16, codes_aligned4;
    std::vector<int> floats, codes;          // accesses of a pass: [bin * n_col + m], [q * n_bin + bin]

    // a thread's floats of bin b from column mc on; 0, or what is wrong
    int touch_floats(const PsrFitsTile& t, long long b, long long mc) {
        if (t.cpt == 4) {
            if (mc >= n_col) return 0;
            if (mc + 3 >= n_col) return 20;                                  // (a float4 across the end of the row)
            if (!x_aligned16 || (b * n_col + mc) % 4) return 21;
        }
        for (int k = 0; k < t.cpt; ++k)
            if (mc + k < n_col) ++floats[(size_t)(b * n_col + mc + k)];
        return 0;
    }
    // the pair of codes of column q from bin b on
    int touch_codes(bool vec, long long q, long long b) {
        const long long o = q * n_bin + b;
        if (vec) {
            if (b + 1 >= n_bin) return 22;                                   // (a dword across the end of the column)
            if (!codes_aligned4 || o % 2) return 23;
        }
        ++codes[(size_t)o];
        if (b + 1 < n_bin) ++codes[(size_t)(o + 1)];
        return 0;
    }
    bool all_once(std::vector<int>& v) {
        bool ok = true;
        for (int& n : v) ok &= n == 1, n = 0;
        return ok;
    }
};

int walk(long long n_bin, long long n_chan, long long n_pol, bool x_aligned16, bool codes_aligned4,
         const PsrFitsGeo& g) {
    const PsrFitsTile t = psrfits_tile(g.tc, g.vec != 0);
    const long long n_col = n_chan * n_pol;
    if ((g.tc != 32 && g.tc != 4) || t.nx < 1 || t.nx * t.cpt != g.tc || t.nx * t.ny != NT ||
        (t.ny & (t.ny - 1)) || t.tb * g.tc != BBT_PSRFITS_TILE || t.np * 2 != t.tb)
        return 1;
    if (g.n_tile * g.tc < n_col || (g.n_tile - 1) * g.tc >= n_col) return 2;
    if (g.vec && (n_col % 4 || n_bin % 2 || !x_aligned16 || !codes_aligned4)) return 3;
    Row row{n_bin, n_col, x_aligned16, codes_aligned4, std::vector<int>((size_t)(n_bin * n_col), 0),
            std::vector<int>((size_t)(n_bin * n_col), 0)};
    std::vector<int> col_enc((size_t)n_col, 0), col_dec((size_t)n_col, 0);   // scl / offs / n_finite written, read
    int rc;

    // -- k_psrfits_encode ---------------------------------------------------------------------------
    const int n_stat = NT * t.cpt, n_enc = g.tc * t.enc_pitch;
    for (long long tile = 0; tile < g.n_tile; ++tile) {
        const long long m0 = tile * g.tc;
        std::vector<long long> s_cnt((size_t)n_stat, -1), s_base((size_t)g.tc, -1);
        // 1. the statistics: s_cnt holds the bins a thread has seen of a column, -1 where nothing was written
        for (int tid = 0; tid < NT; ++tid) {
            const int tx = tid % t.nx, ty = tid / t.nx;
            const long long mc = m0 + (long long)tx * t.cpt;
            long long seen = 0;
            for (long long b = ty; b < n_bin; b += t.ny, ++seen)
                if ((rc = row.touch_floats(t, b, mc))) return rc;
            for (int k = 0; k < t.cpt; ++k) {
                const int i = ty * g.tc + tx * t.cpt + k;
                if (i >= n_stat || s_cnt[(size_t)i] != -1) return 4;
                s_cnt[(size_t)i] = seen;
            }
        }
        for (int s = t.ny / 2; s > 0; s >>= 1)
            for (int tid = 0; tid < NT; ++tid) {
                const int tx = tid % t.nx, ty = tid / t.nx;
                if (ty >= s) continue;
                for (int k = 0; k < t.cpt; ++k) {
                    const int i = ty * g.tc + tx * t.cpt + k, j = i + s * g.tc;
                    if (j >= n_stat || s_cnt[(size_t)i] < 0 || s_cnt[(size_t)j] < 0) return 5;
                    s_cnt[(size_t)i] += s_cnt[(size_t)j];
                    s_cnt[(size_t)j] = -1;                                   // (added once: not read again)
                }
            }
        for (int c = 0; c < g.tc && c < NT; ++c) {
            const long long m = m0 + c;
            long long base = 0;
            if (m < n_col) {
                if (s_cnt[(size_t)c] != n_bin) return 6;                     // (every bin of the column, once)
                const long long q = (m % n_pol) * n_chan + m / n_pol;
                if (q < 0 || q >= n_col) return 7;
                ++col_enc[(size_t)q];
                base = q * n_bin;
            }
            s_base[(size_t)c] = base;
        }
        if (g.tc > NT) return 8;
        // 2. the codes, a tile of tb bins at a time
        std::vector<long long> stamp((size_t)n_enc, -1);
        for (long long b0 = 0; b0 < n_bin; b0 += t.tb) {
            for (int tid = 0; tid < NT; ++tid) {
                const int tx = tid % t.nx, ty = tid / t.nx;
                const long long mc = m0 + (long long)tx * t.cpt;
                for (int p = ty; p < t.np; p += t.ny) {
                    const long long b = b0 + 2 * p;
                    if (b >= n_bin) break;
                    if ((rc = row.touch_floats(t, b, mc))) return rc;
                    if (b + 1 < n_bin && (rc = row.touch_floats(t, b + 1, mc))) return rc;
                    for (int k = 0; k < t.cpt; ++k) {
                        const int at = (tx * t.cpt + k) * t.enc_pitch + p;
                        if (at >= n_enc || stamp[(size_t)at] == b0) return 9;      // (inside, no two on a cell)
                        stamp[(size_t)at] = b0;
                    }
                }
            }
            for (int i = 0; i < g.tc * t.np; ++i) {
                const int c = i / t.np, p = i % t.np;
                const long long b = b0 + 2 * p;
                if (!(m0 + c < n_col && b < n_bin)) continue;
                const int at = c * t.enc_pitch + p;
                if (at >= n_enc || stamp[(size_t)at] != b0) return 10;       // (a pair coded in this round)
                if (c >= g.tc || s_base[(size_t)c] < 0) return 11;
                if ((rc = row.touch_codes(g.vec != 0, s_base[(size_t)c] / n_bin, b))) return rc;
            }
        }
    }
    for (int& n : row.floats) {                                              // (read by the statistics, and to be coded)
        if (n != 2) return 12;
        n = 0;
    }
    if (!row.all_once(row.codes)) return 13;
    for (int n : col_enc)
        if (n != 1) return 14;

    // -- k_psrfits_decode ---------------------------------------------------------------------------
    const int n_dec = g.tc * t.dec_pitch;
    for (long long tile = 0; tile < g.n_tile; ++tile) {
        const long long m0 = tile * g.tc;
        std::vector<long long> s_base((size_t)g.tc, -1), stamp((size_t)n_dec, -1);
        for (int c = 0; c < g.tc; ++c) {
            const long long m = m0 + c;
            long long base = 0;
            if (m < n_col) {
                const long long q = (m % n_pol) * n_chan + m / n_pol;
                if (q < 0 || q >= n_col) return 15;
                ++col_dec[(size_t)q];
                base = q * n_bin;
            }
            s_base[(size_t)c] = base;
        }
        for (long long b0 = 0; b0 < n_bin; b0 += t.tb) {
            for (int i = 0; i < g.tc * t.np; ++i) {
                const int c = i / t.np, p = i % t.np;
                const long long b = b0 + 2 * p;
                if (!(m0 + c < n_col && b < n_bin)) continue;
                if (c >= g.tc || s_base[(size_t)c] < 0) return 16;
                if ((rc = row.touch_codes(g.vec != 0, s_base[(size_t)c] / n_bin, b))) return rc;
                const int at = c * t.dec_pitch + 2 * p;
                if (at + 1 >= n_dec || stamp[(size_t)at] == b0 || stamp[(size_t)(at + 1)] == b0) return 17;
                stamp[(size_t)at] = stamp[(size_t)(at + 1)] = b0;
            }
            for (int tid = 0; tid < NT; ++tid) {
                const int tx = tid % t.nx, ty = tid / t.nx;
                const long long mc = m0 + (long long)tx * t.cpt;
                for (int bl = ty; bl < t.tb; bl += t.ny) {
                    const long long b = b0 + bl;
                    if (b >= n_bin) break;
                    if ((rc = row.touch_floats(t, b, mc))) return rc;
                    for (int k = 0; k < t.cpt; ++k) {
                        if (mc + k >= n_col) continue;
                        const int at = (tx * t.cpt + k) * t.dec_pitch + bl;
                        if (at >= n_dec || stamp[(size_t)at] != b0) return 18;     // (a value decoded in this round)
                    }
                }
            }
        }
    }
    if (!row.all_once(row.floats)) return 19;
    if (!row.all_once(row.codes)) return 24;
    for (int n : col_dec)
        if (n != 1) return 25;
    return 0;
}

int one(long long n_bin, long long n_chan, long long n_pol, int x_aligned, int codes_aligned) {
    PsrFitsGeo g = {};
    const char* err = psrfits_geo(n_bin, n_chan, n_pol, x_aligned != 0, codes_aligned != 0, &g);
    if (err) {
        printf("{\"error\": \"%s\"}\n", err);
        return 0;
    }
    const int rc = walk(n_bin, n_chan, n_pol, x_aligned != 0, codes_aligned != 0, g);
    const PsrFitsTile t = psrfits_tile(g.tc, g.vec != 0);
    printf("{\"tc\": %d, \"vec\": %d, \"n_tile\": %lld, \"tb\": %d, \"nx\": %d, \"ny\": %d, \"enc_pitch\": %d, "
           "\"dec_pitch\": %d, \"walk\": %d}\n", g.tc, g.vec, g.n_tile, t.tb, t.nx, t.ny, t.enc_pitch, t.dec_pitch, rc);
    return rc != 0;
}

}  // namespace

int main(int argc, char** argv) {
    int bad = 0;
    if (argc > 1) {
        for (int i = 1; i + 4 < argc; i += 5)
            bad |= one(atoll(argv[i]), atoll(argv[i + 1]), atoll(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]));
    } else {
        long long n_bin, n_chan, n_pol;
        int x_aligned, codes_aligned;
        while (scanf("%lld %lld %lld %d %d", &n_bin, &n_chan, &n_pol, &x_aligned, &codes_aligned) == 5)
            bad |= one(n_bin, n_chan, n_pol, x_aligned, codes_aligned);
    }
    return bad;
}
