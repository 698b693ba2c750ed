// Host check of csrc/psrsearch_geo.hpp, the tiling of the PSRFITS search-mode kernels: for every
// shape given as "nsblk n_chan n_pol nbits aligned4" it prints the geometry as a JSON line and
// walks the index arithmetic of k_psrsearch_encode / k_psrsearch_decode on the host -- every LDS
// index inside the tile, every thread's column inside the row, every byte of a sample stored
// exactly once.  Built by tests/test_psrfits_search_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "psrsearch_geo.hpp"

static int walk(long long nsblk, long long n_chan, long long n_pol, int nbits, const PsrSearchGeo& g) {
    const int nt = BBT_PSRSEARCH_THREADS, cpb = 8 / nbits, ub = g.unit / cpb;
    const long long pol_bytes = n_chan / cpb, sample_bytes = n_chan * n_pol / cpb;
    const int sp = (int)n_pol * g.pol_pitch, wfull = g.ct * (int)n_pol;
    if (g.ct < 1 || g.ct % g.unit || wfull > nt || g.ny < 1 || g.ny * wfull > nt || g.ts < 1) return 1;
    if ((long long)g.ts * sp > BBT_PSRSEARCH_LDS) return 2;
    if (g.vec && (pol_bytes % 4 || ub != 4)) return 3;
    std::vector<int> stored((size_t)sample_bytes, 0), column((size_t)(n_chan * n_pol), 0);
    for (long long tile = 0; tile < g.n_tile; ++tile) {
        const long long c0 = tile * g.ct;
        const int cte = (int)(n_chan - c0 < g.ct ? n_chan - c0 : g.ct), w = cte * (int)n_pol;
        if (cte < 1 || cte % g.unit) return 4;
        std::vector<int> cell((size_t)sp, 0);
        for (int tx = 0; tx < w; ++tx) {
            const int p = tx % (int)n_pol, c = tx / (int)n_pol;
            const int at = p * g.pol_pitch + c + (c >> 5);
            if (at >= sp || cell[(size_t)at]++) return 5;                     // (inside a sample, no two on a cell)
            const long long m = c0 * n_pol + tx;
            if (m >= n_chan * n_pol) return 6;
            ++column[(size_t)m];
            if (p * g.ct + c >= nt) return 7;
        }
        const int units = cte / g.unit;
        for (int pp = 0; pp < (int)n_pol; ++pp)
            for (int u = 0; u < units; ++u) {
                for (int k = 0; k < g.unit; ++k) {
                    const int cc = u * g.unit + k;
                    if (cc >= cte || cell[(size_t)(pp * g.pol_pitch + cc + (cc >> 5))] != 1) return 8;
                }
                const long long o = c0 / cpb + pp * pol_bytes + (long long)u * ub;
                if (g.vec && o % 4) return 9;
                for (int b = 0; b < ub; ++b) {
                    if (o + b >= sample_bytes) return 10;
                    ++stored[(size_t)(o + b)];
                }
            }
    }
    for (int v : stored)
        if (v != 1) return 11;
    for (int v : column)
        if (v != 1) return 12;
    (void)nsblk;
    return 0;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int i = 1; i + 4 < argc; i += 5) {
        const long long nsblk = atoll(argv[i]), n_chan = atoll(argv[i + 1]), n_pol = atoll(argv[i + 2]);
        const int nbits = atoi(argv[i + 3]), aligned = atoi(argv[i + 4]);
        PsrSearchGeo g = {};
        const char* err = psrsearch_geo(nsblk, n_chan, n_pol, nbits, aligned != 0, &g);
        if (err) {
            printf("{\"error\": \"%s\"}\n", err);
            continue;
        }
        const int rc = walk(nsblk, n_chan, n_pol, nbits, g);
        bad |= rc != 0;
        printf("{\"ct\": %d, \"unit\": %d, \"vec\": %d, \"ny\": %d, \"pol_pitch\": %d, \"ts\": %d, \"n_tile\": %lld, "
               "\"walk\": %d}\n", g.ct, g.unit, g.vec, g.ny, g.pol_pitch, g.ts, g.n_tile, rc);
    }
    return bad;
}
