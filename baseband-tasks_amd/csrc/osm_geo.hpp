// Everything an overlap-save plan (bbt_hip.hip: bbt_osm_plan_create, osm_run_all) decides from
// the block length, the stream count and the environment: how a block splits into outer x n1 x
// n2, which kernels run it, the translation unit compiled for a length that is not a power of
// two, lanes, chunk and the bytes of a lane's work buffer, and how a regular run is cut into
// launches.  Plain C++17 with no device code and no HIP header (never part of a run-time compiled
// source): tests/gen2_plan_dump.cpp prints these decisions for tests/test_osm_geo.py.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gen_host.hpp"
#include "osm_limits.hpp"

namespace bbt {

// ---- length checks -----------------------------------------------------------------------------
static inline bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }
static inline bool fft_len_ok(int64_t n) { return is_pow2(n) && n >= 256 && n <= 4096; }
static inline bool is_7smooth(int64_t n) {
    if (n < 1) return false;
    for (int r : {2, 3, 5, 7})
        while (n % r == 0) n /= r;
    return n == 1;
}

// ---- what the environment may override ---------------------------------------------------------
static inline int rtc_mode() {              // BBT_RTC: 0 off, 1 on, 2 required
    const char* e = getenv("BBT_RTC");
    if (!e || !*e) return 1;
    if (!strcmp(e, "0")) return 0;
    if (!strcmp(e, "require")) return 2;
    return 1;
}
struct OsmKnobs {
    int rtc = 1;                // BBT_RTC, as rtc_mode()
    bool no_big = false;        // BBT_OSM_NO_BIG: 8192 / 16384 samples never as one kernel
    int64_t gen_n1 = 0;         // BBT_GEN_N1 (dev): force the split of a generic length; 0: the rule
    int gen_ct = 0;             // BBT_GEN_CT (dev): upper bound of the columns per tile; 0: the rule
    int lanes = 2;              // BBT_OSM_LANES
    bool has_chunk = false;     // BBT_OSM_CHUNK is set: `chunk` blocks per launch, and no longer regular runs
    int chunk = 0;
    int timing_stride = 4;      // BBT_OSM_TIMING_STRIDE: timing events on every such chunk of a lane
    int small_cap = -1;         // BBT_SMALL_CAP (dev): pairs per workgroup of the one-kernel plans at most; -1: the rule
    int mid_mib = 128;          // BBT_OSM_MID_MIB: three levels, the piece the middle passes take at a time (osm_launch.hpp)
};
static inline OsmKnobs osm_knobs_from_env() {
    OsmKnobs k;
    k.rtc = rtc_mode();
    k.no_big = getenv("BBT_OSM_NO_BIG") != nullptr;
    if (const char* env = getenv("BBT_GEN_N1")) k.gen_n1 = atoll(env);
    if (const char* env = getenv("BBT_GEN_CT")) k.gen_ct = std::max(1, atoi(env));
    if (const char* env = getenv("BBT_OSM_LANES")) k.lanes = atoi(env);
    if (const char* env = getenv("BBT_OSM_CHUNK")) {
        k.has_chunk = true;
        k.chunk = atoi(env);
    }
    if (const char* env = getenv("BBT_OSM_TIMING_STRIDE")) k.timing_stride = std::max(1, atoi(env));
    if (const char* env = getenv("BBT_SMALL_CAP")) k.small_cap = std::max(0, atoi(env));
    if (const char* env = getenv("BBT_OSM_MID_MIB")) k.mid_mib = atoi(env);
    return k;
}

// N = N1 * N2 for a two-level plan (gen_host.hpp: gen_split); `measured` as there
static inline bool split_7smooth(int64_t n, const OsmKnobs& k, int* n1, int* n2, bool* measured = nullptr) {
    const int64_t d = k.gen_n1;
    if (d > 1 && n % d == 0 && n / d <= BBT_GEN_MAX_LEN && d <= BBT_GEN_MAX_LEN) {
        if (measured) *measured = false;
        *n1 = (int)d;
        *n2 = (int)(n / d);
        return true;
    }
    return gen_split(n, k.rtc != 0, n1, n2, measured);
}

// ---- levels ------------------------------------------------------------------------------------
struct OsmGeo {
    int64_t n = 0;
    int S = 0, npair = 0;
    bool fast = false;          // a power of two in [256, 2^24]
    bool generic = false;       // any other product of 2, 3, 5, 7 (gen_kernels.hpp, gen2_kernels.hpp)
    bool single = false;        // one stream: pairs are made of two consecutive blocks
    int outer = 1;              // 256 for three-level transforms: N = outer * n1 * n2
    int n1 = 1, n2 = 0;         // n1 == 1: one kernel, no work buffer
    // generic lengths
    bool measured = false;      // the split is the one measured for the compiled kernels (gen_split)
    GenGeo g1 = {}, g2 = {};    // stages of the general kernels (woff: filled with their tables)
    int gen_ct = 1;             // columns per tile of the column passes
    int row_ct = 1;             // rows per workgroup of the compiled row pass
    bool compiled = false;      // the kernels specialised on the length have a plan: q1 (n1 > 1), q2, q2r
    G2Plan q1, q2, q2r;         // column transform (gen_ct columns), row transform and its reversal
    // osm_buffers
    int n2p = 0;                // pitch of a row of the work buffer
    size_t per_block = 0;       // bytes of the work buffer one block takes
    int lanes = 1, chunk = 1, cap = 1;
    size_t work_bytes = 0;      // per lane
};

static inline bool osm_refuse(std::string* error, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *error = buf;
    return false;
}

// Checks the block length and the stream count and decides the levels.  False: refused, with the
// text of the error.  True with `error` set: a generic length that has no plan on the compiled
// kernels (geo->compiled is false), and why.
static inline bool osm_levels(int64_t n_fft, int n_stream, const OsmKnobs& k, OsmGeo* geo, std::string* error) {
    OsmGeo g;
    error->clear();
    g.fast = is_pow2(n_fft) && n_fft >= 256 && n_fft <= (1 << 24);
    int gn1 = 1, gn2 = 0;
    if (!(g.fast || (is_7smooth(n_fft) && n_fft >= 2 &&
                     (n_fft <= BBT_GEN_MAX_LEN || split_7smooth(n_fft, k, &gn1, &gn2, &g.measured)))))
        return osm_refuse(error,
                          "bbt_osm_plan_create: n_fft=%lld must be a power of two in [256, 2^24] or a product of "
                          "2, 3, 5, 7 that is <= 8192 or splits into two such factors",
                          (long long)n_fft);
    g.single = n_stream == 1 && g.fast;
    if (!(g.single || (n_stream >= 2 && n_stream % 2 == 0 && n_stream <= 65535 * 2)))
        return osm_refuse(error,
                          "bbt_osm_plan_create: n_stream=%d must be even and >= 2 (or 1 with a power-of-two block "
                          "length)", n_stream);
    g.n = n_fft;
    g.S = n_stream;
    g.npair = g.single ? 1 : n_stream / 2;
    if (!g.fast) {
        g.generic = true;
        g.n1 = n_fft <= BBT_GEN_MAX_LEN ? 1 : gn1;
    } else if (n_fft <= 4096 ||
               ((n_fft == 8192 || n_fft == 16384) && (g.single || (n_stream / 2) % 8 != 0) && !k.no_big)) {
        // (8192 / 16384 samples: one workgroup of 512 / 1024 threads, big_kernels.hpp -- one stream pair
        // per workgroup, 16 bytes of every complete sample: with pairs in eights the two-level plan, whose
        // 16-point column passes then move whole lines, is as fast at 8192 and faster at 16384 samples:
        // 16 / 128 / 2048 streams 113 / 109 / 84 against 84 / 88 / 58 G stream-samples/s)
        g.n1 = 1;
    } else if (n_fft <= (1 << 16)) {
        g.n1 = 16;
    } else if (n_fft <= (1 << 20)) {
        g.n1 = 256;
    } else if (n_fft == (1 << 21)) {
        // 512 x 4096: still two levels -- three streaming passes where 256 x 16 x 512 takes five.
        // (A 512-point column pass holds 8 columns in 48 KiB of exchange area, three workgroups
        // per CU; the row pass is the 4096-point one of the 2^20 blocks.)
        g.n1 = 512;
    } else if (n_fft == (1 << 22) && (g.single || (n_stream / 2) % 8 != 0)) {
        // (stream pairs in eights: three levels, whose 256-point column passes take 8 pairs per workgroup --
        // 16 / 128 streams 59.9 / 66.4 against 54.3 / 59.7 G stream-samples/s; at 2^21 two levels stay ahead)
        g.n1 = 1024;             // 1024 x 4096, likewise (8 columns: 80 KiB, two workgroups per CU)
    } else {
        g.outer = 256;           // three levels, 256 x 16 x N2
        g.n1 = 16;
        if (n_stream / 2 > 255)
            return osm_refuse(error, "bbt_osm_plan_create: blocks longer than 2^20 support at most 510 streams");
    }
    g.n2 = (int)(n_fft / g.n1 / g.outer);
    if (g.generic) {
        if (!gen_factor_7smooth(g.n2, &g.g2) || (g.n1 > 1 && !gen_factor_7smooth(g.n1, &g.g1)))
            return osm_refuse(error, "bbt_osm_plan_create: cannot factor %d x %d", g.n1, g.n2);
        // columns per tile of the column passes (gen_host.hpp: gen_col_ct_wanted)
        g.gen_ct = gen_col_ct_wanted(n_fft, g.n1, k.rtc != 0, k.gen_ct);
        // The plan of the kernels specialised on this length (fft_gen2.hpp); without one the plan
        // runs on the general ones.
        if (k.rtc) {
            // (short rows: several neighbouring rows per workgroup, gen2_host.hpp g2_row_ct)
            g.row_ct = g.n1 > 1 ? g2_row_ct(g.n2, g2_pmax(BBT_G2_KIND_ROW)) : 1;
            bool ok = g2_plan(g.n2, g.row_ct, &g.q2, g2_pmax(BBT_G2_KIND_ROW));
            if (ok) g.q2r = g2_reversed(g.q2);
            // (a column tile is one workgroup: at most 1024 threads and 64 KiB of exchange area)
            if (ok && g.n1 > 1) ok = g2_fit_col_plan(g.n1, &g.gen_ct, &g.q1);
            ok = ok && g.q2.threads() <= 1024 && std::max(g.q2.lds_elems, g.q2r.lds_elems) * 8 <= 96 * 1024;
            if (!ok) osm_refuse(error, "no stage list within a workgroup for %d x %d", g.n1, g.n2);
            g.compiled = ok;
        }
    }
    *geo = g;
    return true;
}

// ---- the compiled source -----------------------------------------------------------------------
// The translation unit of a generic length whose geo.compiled is set, and its entry points:
// k_small (one kernel), or k_row, k_first, k_last (row kernel and both column passes).
struct OsmSource {
    std::string text;
    std::vector<const char*> names;
};
static inline OsmSource osm_g2_source(const OsmGeo& g) {
    OsmSource s;
    s.text = "#include \"gen2_kernels.hpp\"\n" + g2_trait_source("GA", g.q2) + g2_trait_source("GB", g.q2r);
    // (workgroups of 7 waves or more: at most 128 registers, two of them per CU)
    const std::string w2 = g.q2.threads() >= 448 ? "4" : "0";
    if (g.n1 == 1) {
        s.text += "BBT_G2_KERNEL_OSM_SMALL(k_small, GA, GB, " + w2 + ")\n";
        s.names = {"k_small"};
    } else {
        const std::string w1 = g.q1.threads() >= 448 ? "4" : "0";
        s.text += g2_trait_source("GC", g.q1) + "BBT_G2_KERNEL_ROW(k_row, GA, GB, " + w2 + ")\n"
                  "BBT_G2_KERNEL_COL(k_first, GC, true, " + w1 + ")\nBBT_G2_KERNEL_COL(k_last, GC, false, " + w1 + ")\n";
        s.names = {"k_row", "k_first", "k_last"};
    }
    return s;
}

// ---- buffers -----------------------------------------------------------------------------------
// workspace: `lanes` work buffers of `chunk` blocks each, 192 MiB in total.
// Measured on MI355X (2-pol 2^20 blocks): 2 x 6 blocks is best; a launch of
// 6 blocks is 1536 row-pass workgroups = exactly two rounds of the 768
// resident ones, while 2 x 12 (384 MiB) falls out of the 256 MiB Infinity
// Cache and loses 6 % although every pass alone is faster.
// `rtc_ok`: the plan runs on the compiled kernels (known once they have been built).
static inline void osm_buffers(OsmGeo* g, bool rtc_ok, const OsmKnobs& k) {
    int lanes = k.lanes < 1 ? 1 : (k.lanes > BBT_MAX_LANES ? BBT_MAX_LANES : k.lanes);
    // (plans on the specialised generic kernels pad the rows of the work buffer to whole lines)
    g->n2p = rtc_ok ? (g->n2 + 7) / 8 * 8 : g->n2;
    const size_t per_block = rtc_ok ? (size_t)g->npair * g->n1 * g->n2p * 16 : (size_t)g->npair * g->n * 16;
    g->per_block = per_block;
    int chunk = (int)((192u << 20) / per_block / lanes);
    if (k.has_chunk) chunk = k.chunk;
    if (chunk < 1) chunk = 1;
    if (chunk > BBT_MAX_CHUNK) chunk = BBT_MAX_CHUNK;
    if (g->outer > 1) {                       // grid.y = blocks * pairs * 256 must fit
        while (chunk > 1 && (long long)chunk * g->npair * g->outer > 65535) --chunk;
    }
    while (chunk > 1 && (long long)chunk * g->npair > 65535) --chunk;      // grid.y of the row pass
    if ((double)chunk * per_block * lanes > 16.0 * (1u << 30)) lanes = 1;   // (config 4: 2 x 2 GiB)
    // Short blocks: sixteen descriptors are a small launch (16 x 8192 samples: 32 workgroups per
    // pass), so runs of REGULAR blocks -- equal steps of input and output, the same kept range:
    // every block of a padded task but a re-aligned last one -- go as one descriptor and a hop
    // (OsmChunk::reg_count), as many blocks as the work buffer (the same 192 MiB) holds.
    int cap = (int)std::min<size_t>((192u << 20) / per_block / lanes, 4096);
    while (cap > 1 && (long long)cap * g->npair * g->outer > 65535) --cap;
    if (cap < chunk || k.has_chunk) cap = chunk;
    if (g->single) {
        // `chunk` pairs of blocks fit the work buffer: a chunk of descriptors holds twice as many blocks
        const int pairs = chunk > BBT_MAX_CHUNK / 2 ? BBT_MAX_CHUNK / 2 : chunk;
        cap = std::max(cap, pairs);
        g->work_bytes = per_block * cap;
        chunk = 2 * pairs;
        cap = 2 * cap;
    } else {
        g->work_bytes = per_block * cap;
    }
    if (g->n1 == 1) {
        // one kernel, no work buffer and no lanes: nothing bounds a launch but the descriptor array
        if (!k.has_chunk) {
            chunk = BBT_MAX_CHUNK;
            while (chunk > 1 && (long long)chunk * g->npair >= (1ll << 31)) --chunk;
        }
        cap = (int)std::min<long long>(1 << 20, ((1ll << 31) - 1) / g->npair);   // nothing to hold
        g->work_bytes = 0;
        lanes = 1;
    }
    g->chunk = chunk;
    g->cap = cap;
    g->lanes = lanes;
}

// ---- pure predicates of the geometry -----------------------------------------------------------
// can bbt_osm_execute_channelized take Channelize(n_chan) into the row pass?
static inline bool osm_fusable(bool generic, bool single, int outer, int n1, int n2, int n_chan) {
    if (generic || (n1 == 1 && outer == 1)) return false;
    if (single)                 // one stream: blocks side by side; 256 channels and up, no detection
        return fft_len_ok(n_chan) && n_chan <= n2 && n2 % n_chan == 0;
    if (n_chan == 16 || n_chan == 32 || n_chan == 64 || n_chan == 128)       // few channels: after an
        return n1 >= 256 || outer == 256;                                   // exchange in the row pass
    if (n_chan == 2 || n_chan == 4 || n_chan == 8)       // very few: lane butterflies in the row pass,
        return outer == 1 && (n1 == 16 || n1 == 256);                    // two-level plans (2^13 ... 2^20 samples)
    return fft_len_ok(n_chan) && n_chan <= n2 && n2 % n_chan == 0;
}
// integration bins one column-pass workgroup touches: its 256 rows hold
// every (n2 / n_chan)-th of 256 * n2 / n_chan consecutive spectra
static inline int osm_detect_bins_max(int n2, int n_chan, int step) {
    if (n_chan <= 0 || step <= 0) return -1;
    const int64_t span = 255ll * (n2 / n_chan);
    return (int)(span / step) + 2;
}

// ---- run slicing (osm_run_all) -----------------------------------------------------------------
// regular runs longer than a chunk of descriptors: only where the work buffer holds more
static inline bool osm_regular_ok(int chunk, int cap) { return cap > chunk; }
// Block `b` is block `a` moved by `d` samples of input and of output (the fused channelizer's
// per-block shift follows from the hop, mask = n_chan - 1 or 0; index: the fills count blocks up).
// Block: OsmBlock of osm_chunk.hpp.
template <class Block>
static inline bool osm_follows(const Block& a, const Block& b, long long d, int mask) {
    return b.in_off - a.in_off == d && b.out_off - a.out_off == d && b.valid_start == a.valid_start &&
           b.valid_count == a.valid_count && !a.flat && !b.flat &&
           b.shift == (int)(((long long)a.shift - d) & mask);
}
// A regular run of `run` > chunk blocks goes in `parts` launches of `per` blocks (the last one
// may be shorter): launches of equal size, as few as the work buffer allows -- one per lane at
// least when each still gets more than a chunk of descriptors would hold.
static inline void osm_run_parts(int64_t run, int chunk, int cap, int lanes, bool fork, int64_t* parts, int64_t* per) {
    *parts = (run + cap - 1) / cap;
    if (fork && *parts < lanes && run >= (int64_t)lanes * 2 * chunk) *parts = lanes;
    *per = (run + *parts - 1) / *parts;
}

}  // namespace bbt
