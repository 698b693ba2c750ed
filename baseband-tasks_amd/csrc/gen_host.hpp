// Host rules of the general LDS Stockham kernels (fft_generic.hpp, gen_kernels.hpp) and of the
// two-level overlap-save plans built on them: stage lists, workgroup size, how a block length
// splits into N1 x N2 and how many columns a column tile takes.  Plain C++ (no device code): the
// plan's geometry (osm_geo.hpp) is built on these rules, and tests/gen2_plan_dump.cpp prints them
// without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <map>
#include <utility>
#include <vector>

#include "gen2_host.hpp"
#include "gen_geo.hpp"

namespace bbt {

// Plan-time compilation of the kernels specialised on a length (rtc.hpp): switched off
// (BBT_RTC=0), on, or on and failed -- the plan then runs on the general kernels with the split
// and the tile that were chosen for the compiled ones.
enum { BBT_GEN_RTC_OFF = 0, BBT_GEN_RTC_ON = 1, BBT_GEN_RTC_FAILED = 2 };

static inline bool gen_factor_7smooth(int64_t n, GenGeo* g) {
    // Stages of the LDS Stockham transform: radices from {2..10, 12, 14, 15, 16} (the composite
    // ones are small Cooley-Tukey transforms on registers, fft_generic.hpp), as few as possible --
    // every stage is a round trip of the whole tile through LDS with two barriers -- and among
    // the shortest lists the one with the smallest largest radix (registers).
    if (n < 1 || n > BBT_GEN_MAX_LEN) return false;
    static const int all[] = {16, 15, 14, 12, 10, 9, 8, 7, 6, 5, 4, 3, 2};
    const int* radices = all;
    int nrad = 13;
    while (nrad > 1 && radices[0] > BBT_GEN_MAXR) {   // (the list is in descending order)
        ++radices;
        --nrad;
    }
    g->n = (int)n;
    g->nfac = 0;
    if (n == 1) return true;
    // dynamic programme over the divisors of n: best[d] = (stages, largest radix) to reach d
    std::map<int64_t, std::pair<int, int>> best;
    std::map<int64_t, int> step;
    best[1] = {0, 0};
    std::vector<int64_t> divisors;
    for (int64_t d = 1; d <= n; ++d)
        if (n % d == 0) divisors.push_back(d);
    for (int64_t d : divisors) {
        auto it = best.find(d);
        if (it == best.end()) continue;
        for (int i = 0; i < nrad; ++i) {
            const int r = radices[i];
            const int64_t e = d * r;
            if (n % e) continue;
            const std::pair<int, int> cand = {it->second.first + 1, std::max(it->second.second, r)};
            auto jt = best.find(e);
            if (jt == best.end() || cand < jt->second) {
                best[e] = cand;
                step[e] = r;
            }
        }
    }
    if (!best.count(n) || best[n].first > BBT_GEN_MAX_FACTORS) return false;
    std::vector<int> fac;
    for (int64_t d = n; d > 1; d /= step[d]) fac.push_back(step[d]);
    std::sort(fac.begin(), fac.end(), std::greater<int>());      // (large radices first: fewer twiddles)
    for (int r : fac) g->fac[g->nfac++] = r;
    return true;
}

static inline int gen_threads(int elements) {          // elements <= BBT_GEN_EPT * threads, whole waves
    int t = ((elements + BBT_GEN_EPT - 1) / BBT_GEN_EPT + 63) / 64 * 64;
    return t < 64 ? 64 : (t > 1024 ? 1024 : t);
}

// N = N1 * N2 with N1 <= N2 <= BBT_GEN_MAX_LEN: the largest N1 up to 512 (the column passes
// then hold 8 columns of N1 points in their LDS tile: 128-byte runs), else as balanced as possible.
static inline bool gen_split_balanced(int64_t n, int* n1, int* n2) {
    const int64_t prefer = 512;
    int64_t best = 0, wide = 0;
    for (int64_t d = 1; d * d <= n; ++d)
        if (n % d == 0 && n / d <= BBT_GEN_MAX_LEN) {
            best = d;
            if (d <= prefer) wide = d;
        }
    if (wide) best = wide;
    if (!best) return false;
    *n1 = (int)best;
    *n2 = (int)(n / best);
    return true;
}
// (plans on the run-time specialised kernels: the split rule measured for them; the column
// tile of the general kernels holds n1 * 8 <= 8192 elements, so n1 <= 1024 keeps the fall-back)
// `measured` (optional): whether that rule gave the split.
static inline bool gen_split(int64_t n, bool rtc, int* n1, int* n2, bool* measured = nullptr) {
    const bool m = rtc && g2_choose_split(n, 8, 1024, BBT_GEN_MAX_LEN, n1, n2);
    if (measured) *measured = m;
    return m || gen_split_balanced(n, n1, n2);
}

// Columns per tile of the column passes: a power of two (gen_stage), as many as fit the LDS tile
// up to 8 (128-byte runs of the stream and of the work buffer; measured: 8 columns 18.9, 16
// columns 18.1, 4 columns 17.3 Gsamples/s for the 1 666 980-sample block); short blocks on the
// compiled kernels: as many columns as fill a wave (gen2_host.hpp g2_col_ct).  `cap` > 0
// overrides the upper bound (dev).
static inline int gen_col_ct_wanted(int64_t n_fft, int n1, bool rtc, int cap = 0) {
    if (n1 <= 1) return 1;
    const int ct_cap = cap > 0 ? cap : (rtc && n_fft <= (1 << 17)) ? g2_col_ct(n1, g2_pmax(BBT_G2_KIND_COL)) : 8;
    int ct = 1;
    // (the doubled tile must fit: k_gen_col transforms BBT_GEN_MAX_LEN elements at most, and leaves what
    // lies beyond untransformed)
    while (ct < ct_cap && 2 * ct * n1 <= BBT_GEN_MAX_LEN) ct *= 2;
    return ct;
}
// The column plan of the compiled kernels, from `*ct` columns down: a column tile is one
// workgroup, at most 1024 threads and 64 KiB of exchange area.  False: no such plan.
static inline bool g2_fit_col_plan(int n1, int* ct, G2Plan* q1) {
    bool ok;
    while ((ok = g2_plan(n1, *ct, q1, g2_pmax(BBT_G2_KIND_COL))) && *ct > 1 &&
           (q1->threads() > 1024 || q1->lds_elems * 8 > 64 * 1024))
        *ct /= 2;
    return ok && q1->threads() <= 1024 && q1->lds_elems * 8 <= 64 * 1024;
}
// What osm_levels (osm_geo.hpp) leaves in gen_ct in each mode.  With compilation on the column plan of
// the compiled kernels may have narrowed the tile, and after a failed compilation k_gen_col runs
// with that: n1 * ct <= BBT_GEN_MAX_LEN holds in every mode.
static inline int gen_col_ct(int64_t n_fft, int n1, int mode) {
    int ct = gen_col_ct_wanted(n_fft, n1, mode != BBT_GEN_RTC_OFF);
    if (mode != BBT_GEN_RTC_OFF && n1 > 1) {
        G2Plan q1;
        g2_fit_col_plan(n1, &ct, &q1);
    }
    return ct;
}

}  // namespace bbt
