// How the kernels of corr_kernels.hpp cut one piece of Correlate (correlation.py) into segments, tiles and
// waves: plain C++, shared by the host launcher and the kernels (CorrGeo is a kernel argument) and
// compiled on its own by tests/corr_geo_check.cpp.
//
// The stream is x[t][e][a], t < N samples, e < E elements, a < A inputs, complex64, input fastest: as
// floats R[t][e][r], r < W = 2 A, r = 2 a (real) or 2 a + 1 (imaginary).  Blocks of n samples are counted
// from sample 0; block k is cut into segments of BBT_CORR_SEG samples from its first sample, the last
// possibly shorter: spb = ceil(n / SEG) segments per block.  Per segment and element the kernel makes
// the real Gram matrix G = sum_t R R^T, W x W, as 32 x 32 tiles of `v_mfma_f32_32x32x2_f32` over pairs of
// samples, and from it the B = A (A + 1) / 2 baselines (i, j), i <= j, row-major:
//     Re = G[2i][2j] + G[2i+1][2j+1],   Im = G[2i+1][2j] - G[2i][2j+1].
//
// A UNIT is what one wave owns: one segment of one GROUP of `pack` adjacent elements.  G of the group is
// cut into T = ceil(pack W / 32) chunks of 32 rows; the wave holds the T (T + 1) / 2 tiles (ti, tj), ti <= tj,
// of the upper triangle, row-major.  For A <= 16, T = 1 and pack <= 32 / W elements share the tile, each on
// its own diagonal block (the cross-element products are never read); for A > 16, pack = 1 and T = 2, 3, 4
// give 3, 6, 10 tiles.  Lane l of the wave feeds row 32 c + (l & 31) of chunk c at sample 2 s + (l >> 5) of
// the segment: R at corr_lane() of the sample's row, or a zero where corr_lane() says -1 (beyond the
// group's reals) or the sample lies beyond an odd segment.  Unit u = segment * n_group + group; workgroup
// wg holds units wg * waves ... wg * waves + waves - 1.
//
// A PIECE is samples [first, first + count) of the stream, whole segments: it begins at a segment's
// first sample and ends at a segment's or a block's end.  Segment s of the piece writes scratch[s][e][b]
// [2] (float32); the finishing kernel adds, per value, the segments of a block in float64 in order -- a
// block that a piece leaves unfinished goes on from the plan's float64 carry -- and writes the blocks
// that end in the piece.
//
// Every index into the piece, the scratch and the output is 64-bit; only the per-axis counts are bounded.
#pragma once

#ifdef __HIPCC__
#define BBT_CORR_HD __host__ __device__
#else
#define BBT_CORR_HD
#endif

#define BBT_CORR_SEG 1024                    // samples of a segment: a constant of the rule, not a knob
#define BBT_CORR_MIN_INPUTS 2
#define BBT_CORR_MAX_INPUTS 64
#define BBT_CORR_MAX_N (1ll << 24)           // samples of a block
#define BBT_CORR_MAX_ELEM (1ll << 26)        // elements of a sample
#define BBT_CORR_MAX_SAMPLES (1ll << 44)     // samples of a stream
#define BBT_CORR_WAVES 4                     // waves of a workgroup unless BBT_CORR_WAVES says otherwise
#define BBT_CORR_MAX_WAVES 4
#define BBT_CORR_TILE_PITCH 33               // floats of a row of a wave's 32 x 32 tile in LDS
#define BBT_CORR_TILE_FLOATS (32 * BBT_CORR_TILE_PITCH)

struct CorrGeo {
    long long A, E, n, W, B;                 // inputs, elements, samples of a block, 2 A, baselines
    long long spb;                           // segments of a block
    int pack, T, n_tile, waves;              // elements of a group, chunks, tiles of a unit, waves of a workgroup
    long long n_group;                       // groups of a sample
    long long first, count;                  // the piece
    long long blk0, seg0;                    // its first segment: segment seg0 of block blk0
    long long n_seg, n_unit, n_wg;           // its segments, units and workgroups
    long long blk1;                          // blocks [blk0, blk1) end in the piece
    long long lds_bytes, scratch_bytes;
};

BBT_CORR_HD inline long long corr_baselines(long long A) { return A * (A + 1) / 2; }

// elements that can share a tile
BBT_CORR_HD inline int corr_max_pack(long long A) { return A <= 16 ? (int)(32 / (2 * A)) : 1; }

// baseline (i, j), i <= j < A, in the row-major order of the upper triangle
BBT_CORR_HD inline long long corr_baseline(long long A, long long i, long long j) { return i * A - i * (i - 1) / 2 + (j - i); }

// tile q of the T (T + 1) / 2: (ti, tj), ti <= tj, row-major
BBT_CORR_HD inline void corr_tile(int T, int q, int* ti, int* tj) {
    int i = 0;
    while (q >= T - i) q -= T - i, ++i;
    *ti = i, *tj = i + q;
}

inline const char* corr_sizes(long long A, long long E, long long n) {
    if (A < BBT_CORR_MIN_INPUTS || A > BBT_CORR_MAX_INPUTS) return "n_inputs must be 2 ... 64";
    if (E < 1 || E > BBT_CORR_MAX_ELEM) return "n_elem must be 1 ... 2^26";
    if (n < 1 || n > BBT_CORR_MAX_N) return "n must be 1 ... 2^24";
    return nullptr;
}

// The plan's part of the geometry: pack_knob and waves_knob are BBT_CORR_PACK and BBT_CORR_WAVES, 0 or a
// value the shape cannot take standing for the default (as many elements as fit a tile; 4 waves).
inline const char* corr_plan_geo(long long A, long long E, long long n, int pack_knob, int waves_knob, CorrGeo* g) {
    const char* err = corr_sizes(A, E, n);
    if (err) return err;
    *g = CorrGeo{};
    g->A = A, g->E = E, g->n = n, g->W = 2 * A, g->B = corr_baselines(A);
    g->spb = (n + BBT_CORR_SEG - 1) / BBT_CORR_SEG;
    const int most = corr_max_pack(A);
    g->pack = pack_knob >= 1 && pack_knob <= most ? pack_knob : most;
    g->T = (int)((g->pack * g->W + 31) / 32);
    g->n_tile = g->T * (g->T + 1) / 2;
    g->waves = waves_knob == 1 || waves_knob == 2 || waves_knob == 4 ? waves_knob : BBT_CORR_WAVES;
    g->n_group = (E + g->pack - 1) / g->pack;
    g->lds_bytes = (long long)g->waves * BBT_CORR_TILE_FLOATS * 4;
    return nullptr;
}

// The geometry of the piece [first, first + count), or why it is refused.
inline const char* corr_geo(long long A, long long E, long long n, long long first, long long count, int pack_knob,
                            int waves_knob, CorrGeo* g) {
    const char* err = corr_plan_geo(A, E, n, pack_knob, waves_knob, g);
    if (err) return err;
    if (first < 0 || count < 1 || first > BBT_CORR_MAX_SAMPLES || count > BBT_CORR_MAX_SAMPLES)
        return "a piece must hold 1 ... 2^44 samples of the first 2^44 of the stream";
    const long long end = first + count;
    g->first = first, g->count = count;
    g->blk0 = first / n, g->blk1 = end / n;
    const long long in0 = first - g->blk0 * n, in1 = end - g->blk1 * n;
    if (in0 % BBT_CORR_SEG || in1 % BBT_CORR_SEG) return "a piece must be whole segments of its blocks";
    g->seg0 = in0 / BBT_CORR_SEG;
    g->n_seg = (g->blk1 - g->blk0) * g->spb + in1 / BBT_CORR_SEG - g->seg0;
    if (g->n_seg > (1ll << 40) / g->n_group) return "too many segments for one launch";
    g->n_unit = g->n_seg * g->n_group;
    g->n_wg = (g->n_unit + g->waves - 1) / g->waves;
    if (g->n_wg >= (1ll << 31)) return "too many segments for one launch";
    g->scratch_bytes = g->n_seg * E * g->B * 8;
    return nullptr;
}

// Segment s < n_seg of the piece: the block it belongs to, its index in that block, its first sample
// relative to the piece's and its samples.
BBT_CORR_HD inline void corr_segment(const CorrGeo& g, long long s, long long* blk, long long* m, long long* off, long long* len) {
    const long long q = g.seg0 + s;
    *blk = g.blk0 + q / g.spb, *m = q % g.spb;
    const long long in = *m * BBT_CORR_SEG;
    *off = *blk * g.n + in - g.first;
    *len = g.n - in < BBT_CORR_SEG ? g.n - in : BBT_CORR_SEG;
}

// What lane row i < 32 of chunk c < T feeds for group grp: the offset in floats from the first float of a
// sample, or -1 for a zero (a row beyond the group's reals, which is never read from memory).
BBT_CORR_HD inline long long corr_lane(const CorrGeo& g, long long grp, int c, int i) {
    const long long e0 = grp * g.pack;
    const long long held = g.E - e0 < g.pack ? g.E - e0 : g.pack;
    const long long r = 32ll * c + i;
    return r < held * g.W ? e0 * g.W + r : -1;
}

// The cell (il, jl), il, jl < 16, of the 16 x 16 complex cells of tile (ti, tj) of group grp: false if it is
// no baseline (two different elements, below the diagonal, beyond the group), else its element and
// baseline.  Its four reals are rows 2 il, 2 il + 1 and columns 2 jl, 2 jl + 1 of the tile.
BBT_CORR_HD inline bool corr_cell(const CorrGeo& g, long long grp, int ti, int tj, int il, int jl, long long* e, long long* b) {
    const long long ci = 16ll * ti + il, cj = 16ll * tj + jl;
    const long long pe = ci / g.A;
    if (cj / g.A != pe || pe >= g.pack) return false;
    const long long i = ci - pe * g.A, j = cj - pe * g.A;
    *e = grp * g.pack + pe;
    if (i > j || *e >= g.E) return false;
    *b = corr_baseline(g.A, i, j);
    return true;
}

// where value (segment s, element e, baseline b) lies in the scratch, in floats (real; the imaginary part follows)
BBT_CORR_HD inline long long corr_scratch_at(const CorrGeo& g, long long s, long long e, long long b) {
    return ((s * g.E + e) * g.B + b) * 2;
}

// Where baseline b of element e of block blk lies in an output that begins at block out_blk0, in floats:
// the baselines stand where the inputs' axis stood, `inner` elements of the sample behind it.
BBT_CORR_HD inline long long corr_out_at(const CorrGeo& g, long long inner, long long out_blk0, long long blk, long long e,
                                         long long b) {
    const long long outer = e / inner, in = e - outer * inner;
    return ((((blk - out_blk0) * (g.E / inner) + outer) * g.B + b) * inner + in) * 2;
}
