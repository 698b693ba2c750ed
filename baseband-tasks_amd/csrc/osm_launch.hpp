// What an overlap-save plan (bbt_hip.hip: osm_run_chunk) decides every time it runs a chunk: the
// kernel launches, in order, as plain data -- which instantiation, its grid, workgroup size and
// dynamic LDS bytes, and after which launches the timing events fall.  osm_dispatch (bbt_hip.hip)
// only follows the list.  Plain C++17 with no device code and no HIP header (never part of a run-time
// compiled source): tests/gen2_plan_dump.cpp prints these lists for tests/test_osm_launches.py.
#pragma once
#include "osm_geo.hpp"

namespace bbt {

// ---- exchange areas ----------------------------------------------------------------------------
// FftGeo<N>::LDS_ELEMS (fft_core.hpp) and BigGeo<N>::LDS_ELEMS (fft_big.hpp), in 8-byte elements;
// bbt_hip.hip ties them to the templates with static_assert for every instantiated N.
constexpr int fft_lds_elems(int n) {
    const int r2 = n / 256, t = n / 16;
    const int pad0 = r2 < 16 ? t + r2 : t + 16;
    const int pb1 = 16 + (r2 == 2 ? 8 : r2 == 4 ? 4 : r2 == 8 ? 2 : r2 == 16 ? 1 : 0);
    int pc1 = r2 * pb1;
    while (pc1 % 32 != 16) ++pc1;
    return 16 * pad0 > 16 * pc1 ? 16 * pad0 : 16 * pc1;
}
constexpr int big_lds_elems(int n) {
    const int m = n / 256, l = m / 16;
    const int p1 = 16 * (m + 2), p3 = 256 * l + 2;
    return (p1 > p3 ? p1 : p3) * 16;
}
constexpr size_t OSM_LDS_MAX = 160 * 1024;        // of a workgroup

// ---- one launch --------------------------------------------------------------------------------
enum OsmFamily {
    OSM_COL16, OSM_COL256, OSM_ROWPASS, OSM_MID16, OSM_SMALL, OSM_SMALL_BIG,    // powers of two (bbt_kernels.hpp, big_kernels.hpp)
    OSM_GEN_SMALL, OSM_GEN_COL, OSM_GEN_ROW,                                    // the general kernels (gen_kernels.hpp)
    OSM_G2_SMALL, OSM_G2_FIRST, OSM_G2_ROW, OSM_G2_LAST                         // compiled for the length (gen2_kernels.hpp)
};
static inline const char* osm_family_name(int f) {
    static const char* const names[] = {"k_osm_col16", "k_osm_col256", "k_osm_rowpass", "k_osm_mid16", "k_osm_small",
                                        "k_osm_small_big", "k_gen_osm_small", "k_gen_col", "k_gen_row", "k_small",
                                        "k_first", "k_row", "k_last"};
    return names[f];
}
struct OsmLaunch {
    int family = 0;
    // what selects the instantiation, where it applies
    bool first = false;         // column passes, mid16: the forward one
    bool spec = false;          // last column pass: spectra out (fused channelizer)
    int F = 0;                  // col256: columns (lanes of a row) per workgroup
    int pp = 1;                 // col16, col256, small: stream pairs per workgroup
    int n = 0;                  // col256: column length; small, small_big: block length; rowpass: row length n2
    bool single = false;        // one stream: pairs of blocks
    bool det = false;           // col256: fused detection
    int nch = 0;                // rowpass: channels of the fused channelizer, 0: the plain row pass
    // the launch
    unsigned gx = 1, gy = 1;
    int threads = 0;
    size_t lds = 0;             // dynamic LDS bytes, the 9 KiB pad included
    bool raise_lds = false;     // the kernel's limit of dynamic LDS is raised to `lds` first
    // kernel arguments that are not the plan's
    int row_len = 0;            // col256: n2, or 16 n2 for the outer pass of three levels
    int y0 = 0, ny = 0;         // rowpass, mid16: the outer rows [y0, y0 + ny) of the work buffer
    int mid_mode = 0;           // mid16
    bool tw = false;            // col256 is handed twa / twg (the four-step twiddles the row pass leaves to it)
    // timing events to record after this launch: 0 none, 1 event 1, 2 event 2, 3 both (one kernel)
    int mark = 0;
};

// ---- what the list is made from ----------------------------------------------------------------
struct OsmLaunchPlan {          // fields of the plan
    int64_t n = 0;
    bool generic = false, rtc = false, single = false;
    int outer = 1, n1 = 1, n2 = 0, n2p = 0, npair = 0, S = 0, gen_ct = 1;
    int q1_threads = 0, q1_ct = 1, q2_threads = 0, q2_ct = 1;      // the compiled column and row transforms
    bool tw_col = false;
};
struct OsmChunkFacts {          // ... and of the chunk
    int nblk = 0, reg_count = 0;
    int n_chan = 0;             // fused channelizer, 0: plain overlap-save output
    bool det = false;           // ... with fused detection
    bool in_plane = false;      // pair-planar input
    bool timing = false;        // the plan's timing is on
};

namespace osm_launch_detail {
struct Maker {
    const OsmLaunchPlan& p;
    const OsmChunkFacts& c;
    std::vector<OsmLaunch>* out;
    int nblkw() const { return p.single ? (c.nblk + 1) / 2 : c.nblk; }    // one stream: pairs of blocks

    OsmLaunch& add(int family, unsigned gx, unsigned gy, int threads, size_t lds, bool raise_lds = false) {
        OsmLaunch l;
        l.family = family;
        l.gx = gx;
        l.gy = gy;
        l.threads = threads;
        l.lds = lds;
        l.raise_lds = raise_lds;
        l.single = p.single;
        out->push_back(l);
        return out->back();
    }

    // A column pass of 256, 512 or 1024 points over rows of `row_len`.
    const char* col256(bool first, bool spec, int row_len) {
        const size_t lds1 = fft_lds_elems(256) * 8;         // per column of a tile
        const int nblk = c.nblk, npair = p.npair;
        OsmLaunch* l;
        if (p.n1 == 512 || p.n1 == 1024) {
            // 512- / 1024-point columns (2^21- / 2^22-sample blocks): 8 columns per workgroup, 128-byte runs
            if (c.det) return "osm: fused detection needs 256-point columns";
            const int F = 8;
            l = &add(OSM_COL256, p.single ? row_len / F : row_len / F * npair, p.single ? (nblk + 1) / 2 : nblk,
                     F * (p.n1 / 16), (size_t)fft_lds_elems(p.n1) * 8 * F, true);
            l->F = F;
        } else if (p.single) {
            if (c.det) return "osm: one-stream plans have no fused detection";
            l = &add(OSM_COL256, row_len / 16, (nblk + 1) / 2, 256, 16 * lds1);
            l->F = 16;
        } else if (spec && !first && c.det) {
            l = &add(OSM_COL256, row_len / 16 * npair, nblk, 256, 16 * lds1);
            l->F = 16;
            l->det = true;
        } else if (first && c.in_plane) {
            // pair-planar input: every pair is a two-stream array, the plain 16-column tiles read
            // 256-byte runs of it (the arrangements below are for interleaved rows)
            l = &add(OSM_COL256, row_len / 16 * npair, nblk, 256, 16 * lds1);
            l->F = 16;
        } else if (npair % 8 == 0) {
            // Many streams: the lanes of a row go over groups of stream pairs so that the stream side
            // moves whole lines.  Measured on MI355X (DESIGN, "column-pass tiles"):
            //   pairs in eights   first pass 8 pairs x 8 columns (64 lanes, 1024 threads: 1 KiB of a row of
            //                     the stream and 128-byte runs of work), last pass 8 pairs x 4 columns (512
            //                     threads, no spills): config 4's share +4.2 %, 16 / 32 streams +5-7 %
            //   pairs in fours    first pass from 8 pairs on 4 pairs x 16 columns (1024 threads; 16 streams
            //                     +3 %, 8 streams -5 %), last pass 4 pairs x 4 columns (8 streams +11 %)
            const int F = first ? 64 : 32;
            l = &add(OSM_COL256, row_len / (F / 8) * (npair / 8), nblk, F * 16, F * lds1, true);
            l->F = F;
            l->pp = 8;
        } else if (first && npair % 4 == 0 && npair >= 8) {
            l = &add(OSM_COL256, row_len / 16 * (npair / 4), nblk, 1024, 64 * lds1, true);
            l->F = 64;
            l->pp = 4;
        } else if (!first && npair % 4 == 0) {
            l = &add(OSM_COL256, row_len / 4 * (npair / 4), nblk, 256, 16 * lds1);
            l->F = 16;
            l->pp = 4;
        } else {
            // Plain 16-column tiles.  The first pass (116 VGPRs, 34 KiB of LDS) fits four workgroups per
            // CU, 464 registers per lane of a SIMD: no row-pass wave (162) of the other lane can join
            // them.  Asking for 9 KiB more of (unused) LDS leaves three (348 + 162 = 510 of 512): config 2
            // +2.4 %, headline +0.3 %, four pairs -0.5 % -- hence for one pair only.
            const size_t col_pad = (first && npair == 1) ? 9216 : 0;
            l = &add(OSM_COL256, row_len / 16 * npair, nblk, 256, 16 * lds1 + col_pad, col_pad != 0);
            l->F = 16;
        }
        l->first = first;
        l->spec = spec;
        l->n = (p.n1 == 512 || p.n1 == 1024) ? p.n1 : 256;
        l->row_len = row_len;
        // (the row pass then leaves the four-step twiddles to this pass: the forward ones always, the
        // inverse ones unless the fused channelizer's transform stands between them and this pass)
        l->tw = p.tw_col && p.outer == 1 && (first || !spec);
        return nullptr;
    }

    void col16(bool first) {
        // (the same count with 8 pairs x 32 columns per workgroup)
        OsmLaunch& l = add(OSM_COL16, p.n2 / 256 * p.npair, nblkw(), 256, 0);
        l.first = first;
        l.spec = !first && c.n_chan != 0;
        l.pp = (!p.single && p.npair % 8 == 0) ? 8 : 1;
    }

    // The row pass over the outer rows [y0, y0 + ny) of the work buffer.
    void rowpass(int y0, int ny) {
        // two-level plans: a flat grid, the workgroups that share a response row on one XCD (k_osm_rowpass)
        const bool flat = p.outer == 1 && nblkw() * p.npair > 1 && (long long)p.n1 * nblkw() * p.npair < (1ll << 31);
        OsmLaunch& l = flat ? add(OSM_ROWPASS, p.n1 * nblkw() * p.npair, 1, p.n2 / 16, 0)
                            : add(OSM_ROWPASS, p.n1, ny, p.n2 / 16, 0);
        l.n = p.n2;
        l.nch = c.n_chan;
        l.y0 = y0;
        l.ny = ny;
    }

    void mid16(bool first, int y0, int ny) {
        OsmLaunch& l = add(OSM_MID16, p.n2 / 256, ny, 256, 0);
        l.first = first;
        l.mid_mode = (!first && c.n_chan) ? 1 : 0;
        l.y0 = y0;
        l.ny = ny;
    }

    // pairs per workgroup of the one-kernel plans at most (round 4's rule; BBT_SMALL_CAP overrides: dev)
    static int small_cap(int n) { return n <= 512 ? 8 : (n <= 2048 ? 4 : 2); }

    const char* small(const OsmKnobs& k) {
        const int n = p.n2;
        const int nblk = c.reg_count ? c.reg_count : c.nblk;
        if (n == 8192 || n == 16384) {
            OsmLaunch& l = add(OSM_SMALL_BIG, p.single ? (nblk + 1) / 2 : nblk * p.npair, 1, n / 16,
                               (size_t)big_lds_elems(n) * 8, true);
            l.n = n;
            l.mark = 3;
            return nullptr;
        }
        if (!fft_len_ok(n)) {
            static thread_local char text[64];
            snprintf(text, sizeof text, "osm: unsupported n_fft %lld", (long long)p.n);
            return text;
        }
        // lanes over groups of pairs when there are many (see k_osm_small): the largest of 8, 4, 2 pairs
        // that divides the pair count and fits a workgroup (1024 threads; the interleaved exchange buffer
        // is dynamic LDS, up to 136 KiB)
        const size_t lds1 = (size_t)fft_lds_elems(n) * 8;
        int pp = 1;
        if (!p.single) {
            const int cap = k.small_cap >= 0 ? k.small_cap : small_cap(n);
            for (int q = 8; q > 1 && pp == 1; q /= 2)
                if (q * n / 16 <= 1024 && lds1 * q <= OSM_LDS_MAX && q <= cap && p.npair % q == 0) pp = q;
        }
        OsmLaunch& l = add(OSM_SMALL, p.single ? (nblk + 1) / 2 : nblk * (p.npair / pp), 1, pp * n / 16, lds1 * pp, pp > 1);
        l.n = n;
        l.pp = pp;
        l.mark = 3;
        return nullptr;
    }

    const char* generic() {
        if (c.n_chan) return "osm: the fused channelizer needs a power-of-two block length";
        const int nblk = c.nblk, npair = p.npair;
        if (p.n1 == 1) {
            if (p.rtc) add(OSM_G2_SMALL, nblk * npair, 1, p.q2_threads, 0).mark = 3;
            else add(OSM_GEN_SMALL, nblk * npair, 1, gen_threads(p.n2), (size_t)p.n2 * 16, true).mark = 3;
            return nullptr;
        }
        const int ct = p.gen_ct, tiles = (p.n2 + ct - 1) / ct;
        if (p.rtc) {
            add(OSM_G2_FIRST, (unsigned)tiles * npair * nblk, 1, p.q1_threads, 0).mark = 1;
            add(OSM_G2_ROW, (p.n1 + p.q2_ct - 1) / p.q2_ct, nblk * npair, p.q2_threads, 0).mark = 2;
            add(OSM_G2_LAST, (unsigned)tiles * npair * nblk, 1, p.q1_threads, 0);
            return nullptr;
        }
        // (what k_gen_col transforms: a tile beyond it would come back untransformed in part)
        if (!(ct >= 1 && (ct & (ct - 1)) == 0 && (long long)p.n1 * ct <= BBT_GEN_MAX_LEN)) {
            static thread_local char text[192];
            snprintf(text, sizeof text,
                     "osm: a column tile of %d x %d elements is more than the general kernels' %d (or not a power of two of columns)",
                     p.n1, ct, BBT_GEN_MAX_LEN);
            return text;
        }
        const size_t lds_c = (size_t)p.n1 * ct * 16, lds_r = (size_t)p.n2 * 16;
        OsmLaunch& a = add(OSM_GEN_COL, tiles * npair, nblk, gen_threads(p.n1 * ct), lds_c, true);
        a.first = true;
        a.mark = 1;
        add(OSM_GEN_ROW, p.n1, nblk * npair, gen_threads(p.n2), lds_r, true).mark = 2;
        add(OSM_GEN_COL, tiles * npair, nblk, gen_threads(p.n1 * ct), lds_c, true);
        return nullptr;
    }

    // Three levels: an outer 256-point column pass over rows of M = 16 * n2, then the two-level
    // machinery in place on every outer row.
    // The three middle passes (outer twiddle + 16-point step, row pass, and back) act on every outer
    // row by itself, in place: they go over the work buffer in pieces of BBT_OSM_MID_MIB (default
    // 128 MiB), so that a piece can still be in the Infinity Cache when the next pass comes for it.
    // Measured on MI355X (config 4's share, two runs each): whole buffer 2.67 / 2.69, pieces of
    // 32 MiB 2.57, 64 MiB 2.70 / 2.71, 128 MiB 2.75 / 2.75, 256 MiB 2.70 / 2.76 G complete samples/s
    // -- +3 %, not the 1.5x fewer HBM bytes would give: the other lane's outer column passes stream
    // 4 GiB through the cache meanwhile (making those accesses non-temporal cost 7 %, one lane 8 %).
    const char* three_levels(const OsmKnobs& k) {
        const int m_len = 16 * p.n2;
        const int rows_all = nblkw() * p.npair * 256;
        const long long mid_bytes = (long long)k.mid_mib << 20;
        const long long row_bytes = 16ll * p.n2 * 16;
        int step = mid_bytes > 0 ? (int)std::max<long long>(1, mid_bytes / row_bytes) : rows_all;
        if (c.timing) step = rows_all;            // (per-pass events: the passes one after the other)
        if (const char* no = col256(true, false, m_len)) return no;
        for (int y0 = 0; y0 < rows_all; y0 += step) {
            const int ny = std::min(step, rows_all - y0);
            mid16(true, y0, ny);
            out->back().mark = 1;
            rowpass(y0, ny);
            out->back().mark = 2;
            mid16(false, y0, ny);
        }
        return col256(false, c.n_chan != 0, m_len);
    }

    const char* two_levels() {
        if (p.n1 == 16) col16(true);
        else if (const char* no = col256(true, false, p.n2)) return no;
        out->back().mark = 1;
        rowpass(0, nblkw() * p.npair);
        out->back().mark = 2;
        if (p.n1 == 16) col16(false);
        else return col256(false, c.n_chan != 0, p.n2);
        return nullptr;
    }
};
}  // namespace osm_launch_detail

// The launches of one chunk, in order, into `out` (cleared first).  Returns null, or the text of
// the refusal: nothing of the chunk is launched then.
static inline const char* osm_chunk_launches(const OsmLaunchPlan& p, const OsmChunkFacts& c, const OsmKnobs& k,
                                             std::vector<OsmLaunch>* out) {
    out->clear();
    osm_launch_detail::Maker m{p, c, out};
    if (p.generic) return m.generic();
    if (p.n1 == 1) return m.small(k);
    if (p.outer > 1) return m.three_levels(k);
    return m.two_levels();
}

}  // namespace bbt
