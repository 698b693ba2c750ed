// Host check of csrc/sk_geo.hpp, the tiling of the spectral-kurtosis kernels: for every shape
// given as "n_block n n_elem is_complex group aligned16 slab" it prints the geometry as a JSON line
// and walks the index arithmetic of k_sk_estimate / k_sk_excise (sk_kernels.hpp) on the host --
// every access of the input read exactly once by the sums and stored exactly once by the rewrite,
// every segment sum, flag and group inside its LDS array, every sk and flag written once, every
// segment of a column added by the thread ty = 0 of that column in segment order.  Built by
// tests/test_sk_host.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sk_geo.hpp"

static int walk(long long n_block, long long n, long long n_elem, long long group, const SkGeo& g) {
    const int nt = BBT_SK_THREADS, V = g.v;
    if (V != 1 && V != 2 && V != 4) return 1;
    if (g.w < 1 || g.w % V || g.w % group || g.nx != g.w / V || g.nx < 1 || g.ny < 1 || g.nz < 1) return 2;
    if ((long long)g.nx * g.ny * g.nz > nt || g.nz * g.w > V * nt) return 3;
    if (n_elem % V) return 4;
    const long long pitch = n_elem / V, n_acc = n_block * n * pitch, n_group = n_elem / group;
    const int n_seg = (int)((n + BBT_SK_SEG - 1) / BBT_SK_SEG);
    if (g.ny > n_seg) return 5;
    const int rounds = (n_seg + g.ny - 1) / g.ny;
    std::vector<int> read((size_t)n_acc, 0), stored((size_t)n_acc, 0);
    std::vector<int> sk((size_t)(n_block * n_elem), 0), flags((size_t)(n_block * n_group), 0);
    for (long long wg = 0; wg < g.n_tile * g.n_zgroup; ++wg) {
        const long long tile = wg % g.n_tile, e0 = tile * g.w;
        const int wt = (int)(n_elem - e0 < g.w ? n_elem - e0 : g.w);
        if (wt < 1 || wt % V || wt % group) return 6;
        std::vector<int> s_flag((size_t)(V * nt), 0);
        for (int tid = 0; tid < nt; ++tid) {
            const int tx = tid % g.nx, ty = (tid / g.nx) % g.ny, tz = tid / (g.nx * g.ny);
            const long long block = (wg / g.n_tile) * g.nz + tz;
            const bool active = tz < g.nz && block < n_block && tx * V < wt;
            if (!active) continue;
            const long long at = (block * n) * pitch + e0 / V + tx;
            int next_seg = 0;                                      // (the segment thread ty = 0 adds next)
            for (int r = 0; r < rounds; ++r) {
                const int seg = r * g.ny + ty;
                if (seg < n_seg) {
                    const long long t0 = (long long)seg * BBT_SK_SEG;
                    const int cnt = (int)(n - t0 < BBT_SK_SEG ? n - t0 : BBT_SK_SEG);
                    for (int i = 0; i < cnt; ++i) {
                        const long long a = at + (t0 + i) * pitch;
                        if (a < 0 || a >= n_acc) return 7;
                        ++read[(size_t)a];
                    }
                }
                for (int j = 0; j < V; ++j)
                    if (j * nt + tid >= V * nt) return 8;
                if (g.ny > 1 && ty == 0) {
                    const int have = n_seg - r * g.ny < g.ny ? n_seg - r * g.ny : g.ny;
                    for (int k = 0; k < have; ++k) {
                        const int from = tid + k * g.nx;           // the thread (tx, k, tz)
                        if (from >= nt || from % g.nx != tx || (from / g.nx) % g.ny != k ||
                            from / (g.nx * g.ny) != tz)
                            return 9;
                        if (r * g.ny + k != next_seg++) return 10;
                    }
                } else if (g.ny == 1) {
                    if (seg != next_seg++) return 10;
                }
            }
            if (ty == 0) {
                if (next_seg != n_seg) return 11;
                for (int j = 0; j < V; ++j) {
                    const long long q = block * n_elem + e0 + tx * V + j;
                    if (q >= n_block * n_elem) return 12;
                    ++sk[(size_t)q];
                    const int f = tz * g.w + tx * V + j;
                    if (f >= V * nt || s_flag[(size_t)f]++) return 13;
                }
            }
            for (int j = 0; j < V; ++j)
                if (tz * (g.w / (int)group) + (tx * V + j) / (int)group >= V * nt) return 14;
            for (long long t = ty; t < n; t += 4ll * g.ny)
                for (int u = 0; u < 4; ++u) {
                    const long long s = t + (long long)u * g.ny;
                    if (s >= n) break;
                    const long long a = at + s * pitch;
                    if (a < 0 || a >= n_acc) return 15;
                    ++stored[(size_t)a];
                }
        }
        const int ngt = wt / (int)group, ngw = g.w / (int)group;
        for (int i = 0; i < g.nz * ngt; ++i) {
            const int z = i / ngt, gi = i - z * ngt;
            const long long bz = (wg / g.n_tile) * g.nz + z;
            if (bz >= n_block) continue;
            for (int k = 0; k < group; ++k) {
                const int f = z * g.w + gi * (int)group + k;
                if (f >= V * nt || s_flag[(size_t)f] != 1) return 16;      // (a flag that was written)
            }
            if (z * ngw + gi >= V * nt) return 17;
            const long long q = bz * n_group + e0 / group + gi;
            if (q >= n_block * n_group) return 18;
            ++flags[(size_t)q];
        }
    }
    for (int v : read)
        if (v != 1) return 19;
    for (int v : stored)
        if (v != 1) return 20;
    for (int v : sk)
        if (v != 1) return 21;
    for (int v : flags)
        if (v != 1) return 22;
    return 0;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int i = 1; i + 6 < argc; i += 7) {
        const long long n_block = atoll(argv[i]), n = atoll(argv[i + 1]), n_elem = atoll(argv[i + 2]);
        const int is_complex = atoi(argv[i + 3]);
        const long long group = atoll(argv[i + 4]);
        const int aligned = atoi(argv[i + 5]);
        const long long slab = atoll(argv[i + 6]);
        SkGeo g = {};
        const char* err = sk_geo(n_block, n, n_elem, is_complex, group, aligned != 0, slab, &g);
        if (err) {
            printf("{\"error\": \"%s\"}\n", err);
            continue;
        }
        const int rc = walk(n_block, n, n_elem, group, g);
        bad |= rc != 0;
        printf("{\"v\": %d, \"w\": %d, \"nx\": %d, \"ny\": %d, \"nz\": %d, \"n_tile\": %lld, \"n_zgroup\": %lld, "
               "\"walk\": %d}\n", g.v, g.w, g.nx, g.ny, g.nz, g.n_tile, g.n_zgroup, rc);
    }
    return bad;
}
