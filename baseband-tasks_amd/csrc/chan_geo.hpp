// Everything a channelizer plan (bbt_hip.hip: bbt_chan_plan_create, chan_pick) decides from the
// channel count, the stream count, the direction and the environment: which kind of plan the
// arguments make (or the refusal), and for channel counts that are not powers of two the
// candidates on the compiled kernels -- their geometry, their source text, the list a timed plan
// compares and the choice of an untimed one.  Plain C++17 with no device code and no HIP header
// (never part of a run-time compiled source): tests/gen2_plan_dump.cpp prints these decisions for
// tests/test_tune_geo.py.
#pragma once
#include "osm_geo.hpp"

namespace bbt {

// ---- what the environment may override (read once per plan, as OsmKnobs) -----------------------
struct ChanKnobs {
    bool tune = true;           // BBT_G2_TUNE=0: no timing, g2_pmax(CHAN) points
    bool general = false;       // BBT_G2_CHAN=none: the general kernels
    bool wide = false;          // BBT_G2_CHAN_WIDE: the untimed plan in the `wide` form (tests)
    int ct_cap = 256;           // BBT_G2_CHAN_CT (dev): columns per workgroup at most
};
static inline ChanKnobs chan_knobs_from_env() {
    ChanKnobs k;
    if (const char* env = getenv("BBT_G2_TUNE")) k.tune = strcmp(env, "0") != 0;
    if (const char* env = getenv("BBT_G2_CHAN")) k.general = !strcmp(env, "none");
    k.wide = getenv("BBT_G2_CHAN_WIDE") != nullptr;
    if (const char* env = getenv("BBT_G2_CHAN_CT")) k.ct_cap = atoi(env);
    return k;
}

// ---- the arguments -----------------------------------------------------------------------------
enum ChanKind {
    CHAN_SHORT,                 // a power of two in [2, 128]
    CHAN_ROWS,                  // a power of two in [256, 4096]
    CHAN_BIG,                   // 8192 / 16384 channels: one workgroup per transform (big_kernels.hpp)
    CHAN_GENERIC                // any other product of 2, 3, 5, 7 up to 8192
};
struct ChanShape {
    ChanKind kind = CHAN_SHORT;
    bool single = false;        // one stream
    bool split_real = false;    // direction -2 / +2
    int direction = -1;         // -1 or +1
};
// False: refused, with the text of the error.
static inline bool chan_check(int n_chan, int n_stream, int direction, ChanShape* shape, std::string* error) {
    ChanShape s;
    const bool fast = is_pow2(n_chan) && n_chan >= 2 && n_chan <= 4096;
    // (8192 and 16384 channels: one workgroup of 512 / 1024 threads per transform, stream pairs, plain directions)
    const bool big = (n_chan == 8192 || n_chan == 16384) && n_stream % 2 == 0 && (direction == -1 || direction == 1);
    if (!(fast || big || (n_chan >= 2 && n_chan <= BBT_GEN_MAX_LEN && is_7smooth(n_chan))))
        return osm_refuse(error,
                          "bbt_chan_plan_create: n_chan=%d must be a power of two in [2, 16384] (above 4096: stream "
                          "pairs, directions -1 / +1) or a product of 2, 3, 5, 7 up to 8192", n_chan);
    s.single = n_stream == 1 && fast && n_chan >= 256;
    if (!(s.single || (n_stream >= 2 && n_stream % 2 == 0 && n_stream <= 65535 * 2)))
        return osm_refuse(error,
                          "bbt_chan_plan_create: n_stream=%d must be even and >= 2 (or 1 for a power-of-two n_chan "
                          "in [256, 4096])", n_stream);
    // direction -2: forward transform of ONE stream z = a + i b made of two real streams, writing their
    // half spectra (n_spectra, n_chan / 2 + 1, 2) instead of Z (Channelize of float32 streams in one pass)
    // (+2: the inverse -- half spectra of two real streams in, z = a + i b out)
    s.split_real = direction == -2 || direction == 2;
    if (s.split_real && !(fast && n_chan >= 256))
        return osm_refuse(error, "bbt_chan_plan_create: direction -2 / +2 needs a power-of-two n_chan in [256, 4096]");
    if (s.split_real) direction /= 2;
    if (!(direction == -1 || direction == 1))
        return osm_refuse(error, "bbt_chan_plan_create: direction must be -1, +1, -2 or +2");
    s.direction = direction;
    s.kind = big ? CHAN_BIG : !fast ? CHAN_GENERIC : n_chan >= 256 ? CHAN_ROWS : CHAN_SHORT;
    error->clear();
    *shape = s;
    return true;
}

// ---- candidates on the compiled kernels --------------------------------------------------------
// One candidate of a generic-length plan: columns of a workgroup = cp neighbouring stream pairs
// (up to 8: 128-byte pieces of a complete sample, as many as divide the pair count) x consecutive
// transforms while they still fit ONE wave (a transform of 100 threads gains nothing from a
// neighbour: 1000 channels 160 G alone, 128 G in twos).
// `wide` (many streams): as many pairs as fit a workgroup of 1024 threads and 144 KiB instead of 256
// threads -- whole 128-byte lines at one workgroup per CU, as k_fft_rows_pp.
// `code`: points per thread, + 100: wide -- also how a plan's choice is remembered (0: the general kernel).
struct ChanCandidate {
    int code = 0;
    int cp = 1;                 // stream pairs per workgroup; q.ct / cp transforms of each
    G2Plan q;                   // q.ct columns per workgroup
    std::string source;         // the translation unit; its entry point is k_rows
    std::string error;          // not available: why
    bool ok() const { return error.empty(); }
};
static inline ChanCandidate chan_g2_candidate(int n_chan, int npair, int direction, int pmax, bool wide, const ChanKnobs& k) {
    ChanCandidate c;
    c.code = pmax + (wide ? 100 : 0);
    G2Plan probe;
    if (!g2_plan(n_chan, 1, &probe, pmax)) {
        osm_refuse(&c.error, "no stage list for %d", n_chan);
        return c;
    }
    int cp = 1;
    while (cp < 8 && npair % (2 * cp) == 0 &&
           (wide ? probe.tj * 2 * cp <= 1024 && (int64_t)n_chan * 2 * cp * 8 <= 144 * 1024 : probe.tj * 2 * cp <= 256))
        cp *= 2;
    int ct = cp;
    while (2 * ct <= k.ct_cap && probe.tj * 2 * ct <= 64 && (int64_t)n_chan * 2 * ct * 8 <= 64 * 1024) ct *= 2;
    if (!g2_plan(n_chan, ct, &c.q, pmax) || c.q.threads() > 1024) {
        osm_refuse(&c.error, "no plan for %d x %d columns", n_chan, ct);
        return c;
    }
    c.cp = cp;
    // (workgroups of 7 waves or more: at most 128 registers, two of them per CU)
    c.source = "#include \"gen2_kernels.hpp\"\n" + g2_trait_source("GA", c.q) + "BBT_G2_KERNEL_FFT_ROWS(k_rows, GA, " +
               (direction < 0 ? "-1" : "+1") + (c.q.threads() >= 448 ? ", 4)\n" : ", 0)\n");
    return c;
}
// Two candidates run the same kernel on the same columns: stage list, threads per transform and
// columns per workgroup are equal (and with them the source text).  cp is NOT compared, and never
// was: it is an argument of the launch, and the rules above give equal tj and ct the same cp.
static inline bool chan_same_plan(const G2Plan& a, const G2Plan& b) {
    bool eq = a.nfac == b.nfac && a.tj == b.tj && a.ct == b.ct;
    for (int i = 0; eq && i < a.nfac; ++i) eq = a.fac[i] == b.fac[i];
    return eq;
}
// The candidates a timed plan compares (after the general kernel), in order: 10, 16 and 20 points
// per thread, then each `wide` on four stream pairs and more; those without a plan and those equal
// to an earlier one are left out.  An empty list: the last reason in `error`.
static inline std::vector<ChanCandidate> chan_candidates(int n_chan, int npair, int direction, const ChanKnobs& k,
                                                         std::string* error = nullptr) {
    std::vector<ChanCandidate> list;
    for (int code : {10, 16, 20, 110, 116, 120}) {
        const bool wide = code >= 100;
        if (wide && npair < 4) continue;
        ChanCandidate c = chan_g2_candidate(n_chan, npair, direction, code % 100, wide, k);
        if (!c.ok()) {
            if (error) *error = c.error;
            continue;
        }
        bool same = false;
        for (const ChanCandidate& o : list) same = same || chan_same_plan(o.q, c.q);
        if (!same) list.push_back(c);
    }
    return list;
}
// What a plan takes without timing: a remembered choice, or BBT_G2_TUNE=0 (g2_pmax(CHAN) points,
// wide only with BBT_G2_CHAN_WIDE).  -1: the candidates are to be timed.
static inline int chan_untimed_code(int remembered, const ChanKnobs& k) {
    if (remembered >= 0) return remembered;
    return k.tune ? -1 : g2_pmax(BBT_G2_KIND_CHAN) + (k.wide ? 100 : 0);
}

}  // namespace bbt
