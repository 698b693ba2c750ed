// Walks the cutting of the correlator kernels (csrc/corr_geo.hpp) on the host, for test_corr_host.py:
// built with -fsanitize=address,undefined, no GPU.
//
//   corr_geo_check  A E n blocks tail pack waves piece  [eight more numbers ...]
//
// Before the shapes: the limits and refusals, the order of the baselines and of the tiles.  Per shape the
// blocks * n samples of a stream (the tail is dropped, as the task drops it) are handed over in pieces as
// the task cuts them -- piece = 0: all at once; piece > 0: that many samples of one block at a time; piece <
// 0: -piece blocks at a time -- and one JSON line gives the geometry and "walk", 0 if for every piece
//   - it is accepted, begins where the last one ended or at a block, and a piece that begins inside a
//     block follows the piece that ended there (the float64 carry),
//   - every segment lies inside the piece, and over all pieces every (block, segment) comes exactly once,
//   - the lanes of a unit feed every real of its group's elements exactly once and nothing else, every
//     address they form for the first and the last sample of the segment lies inside the piece, and every
//     other lane is a declared zero,
//   - every cell of every tile that names a baseline takes its rows and columns from the lanes that feed
//     that element's inputs i and j, and every (segment, element, baseline) of the scratch is written exactly
//     once, inside the scratch bytes the geometry states,
//   - every (block, element, baseline) of the output is written exactly once, by the piece in which the block
//     ends, for inner = 1, the elements' smallest factor and all elements,
//   - a wave's tile lies inside its LDS and the workgroup's LDS is what the geometry states.
// {"error": ...} where the geometry refuses the shape.  Exit status 1 if any of that fails.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "corr_geo.hpp"

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

static void check_statics() {
    CHECK(corr_sizes(1, 1, 1) && corr_sizes(65, 1, 1) && corr_sizes(2, 0, 1) && corr_sizes(2, 1, 0) &&
              corr_sizes(2, 1, BBT_CORR_MAX_N + 1) && corr_sizes(2, BBT_CORR_MAX_ELEM + 1, 1),
          "sizes out of range are not refused");
    CHECK(!corr_sizes(2, 1, 1) && !corr_sizes(64, BBT_CORR_MAX_ELEM, BBT_CORR_MAX_N), "the limits themselves are refused");
    CorrGeo g;
    // pieces that are not whole segments of their blocks, empty ones, negative ones
    CHECK(corr_geo(4, 3, 2051, 1, 2050, 0, 0, &g) && corr_geo(4, 3, 2051, 0, 1000, 0, 0, &g) && corr_geo(4, 3, 2051, 1024, 1000, 0, 0, &g) &&
              corr_geo(4, 3, 2051, 0, 0, 0, 0, &g) && corr_geo(4, 3, 2051, -1024, 2048, 0, 0, &g) && corr_geo(4, 3, 2051, 2051 + 5, 1024, 0, 0, &g),
          "a piece that is not whole segments is not refused");
    CHECK(!corr_geo(4, 3, 2051, 0, 1024, 0, 0, &g) && !corr_geo(4, 3, 2051, 2048, 3, 0, 0, &g) && !corr_geo(4, 3, 2051, 1024, 1027 + 1024, 0, 0, &g),
          "a piece of whole segments is refused");
    for (long long A = 2; A <= 64; ++A) {
        long long b = 0;
        for (long long i = 0; i < A; ++i)
            for (long long j = i; j < A; ++j, ++b) CHECK(corr_baseline(A, i, j) == b, "baseline order: A=%lld (%lld, %lld)", A, i, j);
        CHECK(b == corr_baselines(A), "baseline count: A=%lld", A);
        CHECK(corr_max_pack(A) * 2 * A <= 32 || A > 16, "pack: A=%lld", A);
    }
    for (int T = 1; T <= 4; ++T) {
        int q = 0;
        for (int ti = 0; ti < T; ++ti)
            for (int tj = ti; tj < T; ++tj, ++q) {
                int a, b;
                corr_tile(T, q, &a, &b);
                CHECK(a == ti && b == tj, "tile order: T=%d q=%d", T, q);
            }
    }
}

struct Piece {
    long long first, count;
};

static void walk(long long A, long long E, long long n, long long blocks, long long tail, int pack, int waves, long long piece) {
    (void)tail;
    CorrGeo g0;
    const char* err = corr_plan_geo(A, E, n, pack, waves, &g0);
    if (!err && blocks < 1) err = "the stream must hold one block";
    if (err) {
        printf("{\"error\": \"%s\"}\n", err);
        return;
    }
    std::vector<Piece> pieces;
    if (piece == 0) {
        pieces.push_back({0, blocks * n});
    } else if (piece < 0) {
        for (long long b = 0; b < blocks; b += -piece) pieces.push_back({b * n, ((b - piece > blocks ? blocks : b - piece) - b) * n});
    } else {
        for (long long b = 0; b < blocks; ++b)
            for (long long p0 = 0; p0 < n; p0 += piece) pieces.push_back({b * n + p0, p0 + piece > n ? n - p0 : piece});
    }
    const long long B = g0.B, W = g0.W, row = E * W, spb = g0.spb;
    std::vector<unsigned char> seg_seen((size_t)(blocks * spb), 0);
    long long inners[3] = {1, E, E};
    for (long long f = 2; f <= E; ++f)
        if (E % f == 0) {
            inners[2] = f;
            break;
        }
    std::vector<std::vector<unsigned char>> out_seen(3, std::vector<unsigned char>((size_t)(blocks * E * B), 0));
    long long carried = -1, at_end = 0, scratch_most = 0, n_seg_total = 0;
    CorrGeo g = g0;
    for (const Piece& pc : pieces) {
        err = corr_geo(A, E, n, pc.first, pc.count, pack, waves, &g);
        CHECK(!err, "piece [%lld, +%lld) refused: %s", pc.first, pc.count, err ? err : "");
        if (err) break;
        CHECK(pc.first == at_end, "piece begins at %lld, the last ended at %lld", pc.first, at_end);
        CHECK(g.seg0 == 0 || carried == pc.first, "piece at %lld begins inside a block without a carry", pc.first);
        CHECK(g.pack == g0.pack && g.T == g0.T && g.waves == g0.waves && g.n_tile == g.T * (g.T + 1) / 2, "plan geometry changed");
        CHECK(g.lds_bytes == (long long)g.waves * BBT_CORR_TILE_FLOATS * 4 && g.lds_bytes <= 65536, "lds bytes %lld", g.lds_bytes);
        CHECK((3 + 8 * 3 + 4) * BBT_CORR_TILE_PITCH + 31 < BBT_CORR_TILE_FLOATS, "a tile leaves its LDS");
        CHECK(g.scratch_bytes == g.n_seg * E * B * 8, "scratch bytes");
        CHECK(g.n_unit == g.n_seg * g.n_group && g.n_wg * g.waves >= g.n_unit && (g.n_wg - 1) * g.waves < g.n_unit, "units");
        scratch_most = g.scratch_bytes > scratch_most ? g.scratch_bytes : scratch_most;
        n_seg_total += g.n_seg;
        std::vector<unsigned char> cell_seen((size_t)(g.n_seg * E * B), 0);
        long long covered = 0;
        for (long long s = 0; s < g.n_seg; ++s) {
            long long blk, m, off, len;
            corr_segment(g, s, &blk, &m, &off, &len);
            CHECK(blk >= 0 && blk < blocks && m >= 0 && m < spb, "segment %lld: block %lld segment %lld", s, blk, m);
            CHECK(off == covered && len >= 1 && len <= BBT_CORR_SEG && off + len <= pc.count, "segment %lld: [%lld, +%lld) of %lld", s, off, len,
                  pc.count);
            CHECK(pc.first + off == blk * n + m * BBT_CORR_SEG && (len == BBT_CORR_SEG || m == spb - 1), "segment %lld is not of the rule", s);
            covered += len;
            if (blk >= 0 && blk < blocks && m >= 0 && m < spb) ++seg_seen[(size_t)(blk * spb + m)];
        }
        CHECK(covered == pc.count, "the segments cover %lld of %lld samples", covered, pc.count);
        for (long long u = 0; u < g.n_wg * g.waves; ++u) {
            if (u >= g.n_unit) continue;                       // a wave without a unit reads and writes nothing
            const long long s = u / g.n_group, grp = u - s * g.n_group;
            long long blk, m, off, len;
            corr_segment(g, s, &blk, &m, &off, &len);
            const long long e0 = grp * g.pack, e1 = e0 + g.pack > E ? E : e0 + g.pack;
            // the lanes: only the first and the last segment of the piece walk the addresses
            std::vector<int> fed((size_t)((e1 - e0) * W), 0);
            for (int c = 0; c < g.T; ++c)
                for (int i = 0; i < 32; ++i) {
                    const long long at = corr_lane(g, grp, c, i);
                    if (at < 0) continue;
                    CHECK(at >= e0 * W && at < e1 * W, "unit %lld chunk %d lane %d feeds real %lld outside its group", u, c, i, at);
                    if (at >= e0 * W && at < e1 * W) ++fed[(size_t)(at - e0 * W)];
                    CHECK(at == e0 * W + 32 * c + i, "unit %lld chunk %d lane %d: real %lld", u, c, i, at);
                    const long long lo = off * row + at, hi = (off + len - 1) * row + at;
                    CHECK(lo >= 0 && hi < pc.count * row, "unit %lld: a load at float %lld of %lld", u, hi, pc.count * row);
                }
            for (int f : fed) CHECK(f == 1, "unit %lld: a real of the group is fed %d times", u, f);
            for (int q = 0; q < g.n_tile; ++q) {
                int ti, tj;
                corr_tile(g.T, q, &ti, &tj);
                for (int il = 0; il < 16; ++il)
                    for (int jl = 0; jl < 16; ++jl) {
                        long long e, b;
                        if (!corr_cell(g, grp, ti, tj, il, jl, &e, &b)) continue;
                        CHECK(e >= e0 && e < e1 && b >= 0 && b < B, "unit %lld: cell names element %lld baseline %lld", u, e, b);
                        if (!(e >= e0 && e < e1 && b >= 0 && b < B)) continue;
                        // the inputs of baseline b
                        long long i = 0, rest = b;
                        while (rest >= A - i) rest -= A - i, ++i;
                        const long long j = i + rest;
                        CHECK(corr_lane(g, grp, ti, 2 * il) == e * W + 2 * i && corr_lane(g, grp, ti, 2 * il + 1) == e * W + 2 * i + 1 &&
                                  corr_lane(g, grp, tj, 2 * jl) == e * W + 2 * j && corr_lane(g, grp, tj, 2 * jl + 1) == e * W + 2 * j + 1,
                              "unit %lld tile (%d, %d) cell (%d, %d): not the reals of inputs %lld and %lld of element %lld", u, ti, tj, il, jl, i,
                              j, e);
                        const long long o = corr_scratch_at(g, s, e, b);
                        CHECK(o >= 0 && (o + 2) * 4 <= g.scratch_bytes && o % 2 == 0, "scratch float %lld of %lld bytes", o, g.scratch_bytes);
                        if (o >= 0 && (o + 2) * 4 <= g.scratch_bytes) ++cell_seen[(size_t)(o / 2)];
                    }
            }
        }
        for (size_t k = 0; k < cell_seen.size(); ++k)
            if (cell_seen[k] != 1) {
                CHECK(false, "piece at %lld: scratch cell %zu written %d times", pc.first, k, (int)cell_seen[k]);
                break;
            }
        // the finishing kernel: the blocks that end in the piece
        CHECK(g.blk0 == pc.first / n && g.blk1 == (pc.first + pc.count) / n, "blocks of the piece");
        for (int w = 0; w < 3; ++w)
            for (long long blk = g.blk0; blk < g.blk1; ++blk)
                for (long long e = 0; e < E; ++e)
                    for (long long b = 0; b < B; ++b) {
                        const long long o = corr_out_at(g, inners[w], g.blk0, blk, e, b);
                        CHECK(o >= 0 && o % 2 == 0 && o / 2 < (g.blk1 - g.blk0) * E * B, "output float %lld", o);
                        if (o >= 0 && o / 2 < (g.blk1 - g.blk0) * E * B) ++out_seen[(size_t)w][(size_t)(g.blk0 * E * B + o / 2)];
                    }
        at_end = pc.first + pc.count;
        carried = at_end % n ? at_end : -1;
    }
    CHECK(at_end == blocks * n && carried == -1, "the pieces end at %lld of %lld", at_end, blocks * n);
    for (size_t k = 0; k < seg_seen.size(); ++k) CHECK(seg_seen[k] == 1, "segment %zu comes %d times", k, (int)seg_seen[k]);
    for (int w = 0; w < 3; ++w)
        for (size_t k = 0; k < out_seen[(size_t)w].size(); ++k)
            if (out_seen[(size_t)w][k] != 1) {
                CHECK(false, "inner %lld: output cell %zu written %d times", inners[w], k, (int)out_seen[(size_t)w][k]);
                break;
            }
    printf("{\"A\": %lld, \"E\": %lld, \"n\": %lld, \"pack\": %d, \"T\": %d, \"n_tile\": %d, \"waves\": %d, \"n_group\": %lld, \"spb\": %lld, "
           "\"pieces\": %zu, \"n_seg\": %lld, \"lds_bytes\": %lld, \"scratch_bytes\": %lld, \"walk\": %d}\n",
           A, E, n, g0.pack, g0.T, g0.n_tile, g0.waves, g0.n_group, spb, pieces.size(), n_seg_total, g0.lds_bytes, scratch_most, failures);
}

int main(int argc, char** argv) {
    check_statics();
    if ((argc - 1) % 8) {
        fprintf(stderr, "usage: corr_geo_check A E n blocks tail pack waves piece ...\n");
        return 2;
    }
    for (int k = 1; k + 7 < argc; k += 8) {
        long long v[8];
        for (int j = 0; j < 8; ++j) v[j] = atoll(argv[k + j]);
        walk(v[0], v[1], v[2], v[3], v[4], (int)v[5], (int)v[6], v[7]);
    }
    return failures ? 1 : 0;
}
