// Everything a filter-bank plan (bbt_hip.hip: bbt_pfb_plan_create, pfb_pick) decides from taps,
// channels, streams and the environment: the argument checks, which (n_chan, n_tap) have a
// sliding-window kernel, whether several stream pairs may share a workgroup and on which
// geometry, the route -- fixed, or the candidates to time -- and the permutation of the taps the
// window kernels read.  Plain C++17 with no device code and no HIP header:
// tests/gen2_plan_dump.cpp prints these decisions for tests/test_tune_geo.py.
#pragma once
#include "osm_geo.hpp"

namespace bbt {

// ---- what the environment may override (read once per plan, as OsmKnobs) -----------------------
struct PfbKnobs {
    bool tune = true;           // BBT_PFB_TUNE=0: the round-4 rule (two passes from 16 streams on)
    int two_pass = -1;          // BBT_PFB_TWO_PASS=0 / 1 (dev): force one pass / two passes; -1: not set
    int pp = 0;                 // BBT_PFB_PP=4 / 8 (dev): force so many pairs per workgroup; 0: not set
    int gl = 0;                 // BBT_PFB_GL (dev): the order of the workgroups that goes with BBT_PFB_PP
};
static inline PfbKnobs pfb_knobs_from_env() {
    PfbKnobs k;
    if (const char* env = getenv("BBT_PFB_TUNE")) k.tune = strcmp(env, "0") != 0;
    if (const char* env = getenv("BBT_PFB_TWO_PASS")) k.two_pass = atoi(env) != 0;
    if (const char* env = getenv("BBT_PFB_PP")) k.pp = atoi(env);
    if (const char* env = getenv("BBT_PFB_GL")) k.gl = atoi(env);
    return k;
}

// sliding-window variants exist for these (n_chan, n_tap)
constexpr bool pfb_has_window(int n_chan, int n_tap) {
    return (n_chan == 256 || n_chan == 512 || n_chan == 1024 || n_chan == 2048) &&
           (n_tap == 4 || n_tap == 8 || n_tap == 12 || n_tap == 16);
}
// geometry of one pair in the several-pairs form of the window kernel: 128 threads and 2048 / N
// spectra per workgroup up to 1024 channels, 256 threads and two spectra for 2048
constexpr int pfb_pp_geometry(int n) { return n <= 1024 ? 2048 : 4096; }

// ---- the arguments -----------------------------------------------------------------------------
struct PfbShape {
    int n_tap = 0, n = 0, S = 0, npair = 0;
    bool split_real = false;    // n_stream -1 / -S: streams z = a + i b of two real streams, half spectra out
    bool window = false;        // a sliding-window kernel exists
    bool pp_ok = false;         // several stream pairs per workgroup of the window kernel are possible
    int gn = 4096;              // ... on this geometry (pfb_pp_geometry)
    bool two_ok = false;        // two passes are possible (k_pfb_fir_rows, then the channelizer in place)
    bool rule_two = false;      // ... and what the rule takes untimed
};
// False: refused, with the text of the error.
static inline bool pfb_check(int n_tap, int n_chan, int n_stream, PfbShape* shape, std::string* error) {
    PfbShape s;
    if (!fft_len_ok(n_chan))
        return osm_refuse(error, "bbt_pfb_plan_create: n_chan=%d must be a power of two in [256, 4096]", n_chan);
    if (!(n_tap >= 1 && n_tap <= 64))
        return osm_refuse(error, "bbt_pfb_plan_create: n_tap=%d must be in [1, 64]", n_tap);
    // n_stream -1: as 1, the stream being z = a + i b of two real streams; out receives their half
    // spectra (n_spectra, n_chan / 2 + 1, 2) -- the filter bank of two float32 streams in one pass
    // (a negative even n_stream -S: S such streams, in pairs)
    s.split_real = n_stream == -1 || (n_stream < 0 && n_stream % 2 == 0);
    if (s.split_real) n_stream = -n_stream;
    if (!(n_stream == 1 || (n_stream >= 2 && n_stream % 2 == 0 && n_stream <= 65535 * 2)))
        return osm_refuse(error, "bbt_pfb_plan_create: n_stream=%d must be even and >= 2", n_stream);
    s.n_tap = n_tap;
    s.n = n_chan;
    s.S = n_stream;
    s.npair = n_stream / 2;
    s.window = pfb_has_window(n_chan, n_tap);
    if ((n_stream == 1 || s.split_real) && !s.window)      // only the sliding-window kernels take one stream / split
        return osm_refuse(error,
                          "bbt_pfb_plan_create: one stream needs n_chan in 256..2048 and 4, 8, 12 or 16 taps "
                          "(got %d x %d); pad to two streams otherwise", n_tap, n_chan);
    s.pp_ok = s.window && !s.split_real && n_chan <= 2048 && s.npair % 4 == 0;
    s.gn = s.pp_ok ? pfb_pp_geometry(n_chan) : 4096;
    s.two_ok = !s.split_real && n_stream >= 2 && (n_tap == 4 || n_tap == 8 || n_tap == 12 || n_tap == 16);
    // (two passes also where no sliding-window kernel exists and every spectrum would re-read its rows:
    // 16 x 4096 on two streams 64.4 -> 84.2 G complete samples/s, 0.26 -> 0.34; with a window kernel one
    // pass wins on few streams: 8 x 2048 125 against 91, 4 x 1024 164 against 88)
    s.rule_two = s.two_ok && (n_stream >= 16 || (!s.window && n_tap >= 8));
    error->clear();
    *shape = s;
    return true;
}

// ---- the route ---------------------------------------------------------------------------------
// pp 0: two passes; 1: one pass, one pair per workgroup (the window kernel if there is one, k_pfb
// otherwise); 4 / 8: one pass of the window kernel with so many pairs per workgroup, whose
// workgroups go in order gl.
struct PfbCandidate {
    int pp = 1, gl = 0;
};
static inline bool operator==(const PfbCandidate& a, const PfbCandidate& b) { return a.pp == b.pp && a.gl == b.gl; }
// an order of the workgroups that does not divide the pair groups is order 0
static inline PfbCandidate pfb_candidate(const PfbShape& s, int pp, int gl) {
    if (pp <= 1) return {pp, 0};
    return {pp, (gl > 0 && (s.npair / pp) % gl == 0) ? gl : 0};
}
// Which route a filter-bank plan takes.  Measured on MI355X (round 5, 1024 channels, G
// stream-samples/s at 16 / 128 / 2048 streams): one pair per workgroup (16 bytes of every complete
// sample per lane) 4 taps 140 / 99 / 82, 12 taps 107 / 54 / 54; two passes (window over whole rows,
// transform in place: 33 bytes per stream-sample instead of 16) 150 / 159 / 146 and 144 / 154 / 133;
// several pairs per workgroup, lanes over the pairs first (64- or 128-byte runs): 4 taps
// 223 / 228 / 186, 12 taps 148 / 131 / 130 -- with 128 registers and at most two workgroups per CU
// its NTAP + NG - 1 row loads for NG spectra weigh more the more taps there are.  Which of them
// and which order of workgroups wins depends on taps, channels and streams, so the candidates
// are timed once on scratch memory (csrc/tune.hpp) and the choice is remembered for the process.
// BBT_PFB_TUNE=0: the round-4 rule (two passes from 16 streams on); BBT_PFB_TWO_PASS=0 / 1,
// BBT_PFB_PP=4 / 8 (+ BBT_PFB_GL) force a route (dev).
struct PfbRoute {
    bool timed = false;
    PfbCandidate fixed;                     // !timed: the route; timed: the one taken when timing is impossible
    std::vector<PfbCandidate> candidates;   // timed: compared in this order
};
static inline PfbRoute pfb_route(const PfbKnobs& k, const PfbShape& s) {
    PfbRoute r;
    if (k.pp && s.pp_ok && (k.pp == 4 || (k.pp == 8 && s.gn == 2048)) && s.npair % k.pp == 0) {
        r.fixed = pfb_candidate(s, k.pp, k.gl);
        return r;
    }
    r.fixed = {s.rule_two ? 0 : 1, 0};
    if (k.two_pass >= 0) {
        r.fixed.pp = (s.two_ok && k.two_pass) ? 0 : 1;
        return r;
    }
    if (!s.pp_ok || !k.tune || s.S < 8) return r;
    r.timed = true;
    if (s.two_ok) r.candidates.push_back({0, 0});
    if (s.S < 16) r.candidates.push_back({1, 0});
    r.candidates.push_back({4, 0});
    if ((s.npair / 4) % 4 == 0) r.candidates.push_back({4, 4});
    if (s.gn == 2048 && s.npair % 8 == 0) {
        r.candidates.push_back({8, 0});
        if (s.npair / 8 > 1) r.candidates.push_back({8, 1});
    }
    return r;
}

// ---- taps --------------------------------------------------------------------------------------
// What the window kernels read: the taps of column tau + T c, four at a time,
// quads[((c * n_tap / 4) + q) * T + tau][k] = h[4 q + k]   (T threads per pair: 256, or gn / 16 in
// the several-pairs form; n_tap a multiple of 4, n_chan of T)
static inline std::vector<float> pfb_tap_quads(const float* taps, int n_tap, int n_chan, int T) {
    const int cols = n_chan / T, quads = n_tap / 4;
    std::vector<float> perm((size_t)n_tap * n_chan);
    for (int c = 0; c < cols; ++c)
        for (int q = 0; q < quads; ++q)
            for (int tau = 0; tau < T; ++tau)
                for (int k = 0; k < 4; ++k)
                    perm[(((size_t)c * quads + q) * T + tau) * 4 + k] = taps[(size_t)(4 * q + k) * n_chan + tau + T * c];
    return perm;
}

}  // namespace bbt
