// How k_dmt_transpose / k_dmt_sweep (dmt_kernels.hpp) cut one chunk of DMTrials (search.py) into
// tiles: plain C++, shared by the host launcher and the kernels (the struct is a kernel argument)
// and compiled on its own by tests/dmt_geo_check.cpp.
//
// A chunk is in[t][c][r], t < n_in, c < nchan, r < n_rest, float32, and a table offsets[d][c] in
// [0, span] for d < ndm; the result is out[i][d][r] = sum over c, ascending, of
// in[i + offsets[d][c]][c][r] for i < n_out, with n_in >= n_out + span.
//
// 1. The transpose writes scratch[e][t], e = c * n_rest + r, rows `pitch` floats apart (n_in
//    rounded up to a wave), in tiles of BBT_DMT_TR x BBT_DMT_TR elements through LDS.
// 2. The sweep has lanes along time.  A wave owns 64 consecutive output times of `db` consecutive
//    trials of one r; a thread holds the db accumulators of its time in registers and walks the
//    channels in ascending order.  The trial block of a wave is the same for all its lanes, so the
//    db offsets of a channel are one wave-uniform load from the device table, which is kept
//    channel-major, tab[c][ndm_pad], its rows padded to a multiple of BBT_DMT_DB_MAX with offset 0
//    (a valid offset; the padded trials are never stored).  The four waves of a workgroup are
//    `waves_t` along time by `waves_d` along the trials: tile_t = 64 * waves_t times by tile_d =
//    db * waves_d trials.  Workgroups are numbered trial tile fastest, then r, then time tile, so
//    those in flight together read the same few rows of the scratch.
//
// Every index into the chunk, the scratch and the result is 64-bit; only the per-axis counts
// below are bounded.
#pragma once

#define BBT_DMT_THREADS 256
#define BBT_DMT_WAVE 64
#define BBT_DMT_TR 64                        // edge of a transpose tile
#define BBT_DMT_DB 8                         // trials a thread holds (default)
#define BBT_DMT_DB_MAX 16
#define BBT_DMT_TILE 256                     // output times of a workgroup (default): 64, 128 or 256
#define BBT_DMT_MAX_NCHAN 16384
#define BBT_DMT_MAX_NDM 4096
#define BBT_DMT_MAX_REST 64
#define BBT_DMT_MAX_SPAN (1 << 24)
#define BBT_DMT_MAX_ROWS (1ll << 40)         // samples of a chunk

struct DmtGeo {
    long long n_in, n_out;       // samples of the chunk, of the result
    long long pitch;             // floats between rows of the scratch
    long long scratch;           // floats of the scratch: nchan * n_rest * pitch
    int nchan, n_rest, ndm, ndm_pad;
    int db;                      // trials per thread
    int waves_t, waves_d;        // waves of a workgroup along time, along the trials
    int tile_t, tile_d;          // output times, trials of a workgroup
    long long n_tile_t;          // workgroups along time
    int n_tile_d;                // workgroups along the trials
    long long n_wg;              // n_tile_d * n_rest * n_tile_t
    long long tr_t;              // transpose tiles along time (grid x)
    int tr_e;                    // transpose tiles along the elements (grid y)
};

inline int dmt_pad_ndm(int ndm) { return (ndm + BBT_DMT_DB_MAX - 1) / BBT_DMT_DB_MAX * BBT_DMT_DB_MAX; }

// 0, or what is wrong with the sizes of a table (a static string)
inline const char* dmt_sizes(long long ndm, long long nchan, long long n_rest) {
    if (ndm < 1 || ndm > BBT_DMT_MAX_NDM) return "ndm must be 1 ... 4096";
    if (nchan < 1 || nchan > BBT_DMT_MAX_NCHAN) return "nchan must be 1 ... 16384";
    if (n_rest < 1 || n_rest > BBT_DMT_MAX_REST) return "n_rest must be 1 ... 64";
    return 0;
}

// 0, or what is wrong with a table offsets[ndm * nchan]: every entry must lie in [0, span].
// This is what the kernels' reads rest on; see dmt_kernels.hpp.
inline const char* dmt_check_table(const int* offsets, long long n, long long span) {
    if (span < 0 || span > BBT_DMT_MAX_SPAN) return "the span must be 0 ... 2^24 samples";
    for (long long i = 0; i < n; ++i) {
        if (offsets[i] < 0) return "a negative offset";
        if (offsets[i] > span) return "an offset above the span";
    }
    return 0;
}

// 0, or what is wrong with a launch.  tile_t: 64, 128 or 256 (0: the default); db: 1, 2, 4, 8 or 16
// (0: the default).
inline const char* dmt_geo(long long n_in, long long n_out, long long nchan, long long n_rest, long long ndm,
                           long long span, int tile_t, int db, DmtGeo* g) {
    const char* err = dmt_sizes(ndm, nchan, n_rest);
    if (err) return err;
    if (span < 0 || span > BBT_DMT_MAX_SPAN) return "the span must be 0 ... 2^24 samples";
    if (n_out < 1) return "no output samples";
    if (n_in > BBT_DMT_MAX_ROWS) return "more than 2^40 samples in one call";
    if (n_in < n_out + span) return "the input is shorter than the output plus the span";
    if (tile_t == 0) tile_t = BBT_DMT_TILE;
    if (db == 0) db = BBT_DMT_DB;
    if (tile_t != 64 && tile_t != 128 && tile_t != 256) return "the time tile must be 64, 128 or 256";
    if (db != 1 && db != 2 && db != 4 && db != 8 && db != 16) return "the trial block must be 1, 2, 4, 8 or 16";
    g->n_in = n_in, g->n_out = n_out;
    g->nchan = (int)nchan, g->n_rest = (int)n_rest, g->ndm = (int)ndm, g->ndm_pad = dmt_pad_ndm((int)ndm);
    g->pitch = (n_in + BBT_DMT_WAVE - 1) / BBT_DMT_WAVE * BBT_DMT_WAVE;
    g->scratch = nchan * n_rest * g->pitch;
    g->db = db;
    g->tile_t = tile_t;
    g->waves_t = tile_t / BBT_DMT_WAVE;
    g->waves_d = BBT_DMT_THREADS / BBT_DMT_WAVE / g->waves_t;
    g->tile_d = db * g->waves_d;
    g->n_tile_t = (n_out + tile_t - 1) / tile_t;
    g->n_tile_d = (int)((ndm + g->tile_d - 1) / g->tile_d);
    g->n_wg = (long long)g->n_tile_d * n_rest * g->n_tile_t;
    g->tr_t = (n_in + BBT_DMT_TR - 1) / BBT_DMT_TR;
    g->tr_e = (int)((nchan * n_rest + BBT_DMT_TR - 1) / BBT_DMT_TR);
    if (g->n_wg >= (1ll << 31) || g->tr_t >= (1ll << 31) || g->tr_e > 65535) return "too many tiles for one launch";
    return 0;
}

// What a wave of the sweep owns: workgroup `wg` < n_wg, wave `w` < 4.  False if it owns nothing
// (its times or trials lie beyond the result), else its first time t0 < n_out, first trial d0 <
// ndm and r.  The kernel and the host check share this.
struct DmtWave {
    long long t0;
    int d0, r;
};
#ifdef __HIPCC__
__host__ __device__
#endif
inline bool dmt_wave(const DmtGeo& g, long long wg, int w, DmtWave* o) {
    const int td = (int)(wg % g.n_tile_d);
    wg /= g.n_tile_d;
    o->r = (int)(wg % g.n_rest);
    const long long tt = wg / g.n_rest;
    o->t0 = tt * g.tile_t + (long long)(w % g.waves_t) * BBT_DMT_WAVE;
    o->d0 = (td * g.waves_d + w / g.waves_t) * g.db;
    return o->t0 < g.n_out && o->d0 < g.ndm;
}
