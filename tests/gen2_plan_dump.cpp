// Prints what the host rules decide without a device, as JSON lines, for tests/test_gen2_planner.py,
// tests/test_osm_geo.py, tests/test_osm_launches.py and tests/test_tune_geo.py:
//   plan <pmax> <n> <ct> ...     a plan of the generic-length engine (csrc/gen2_host.hpp)
//   split <N> ...                the measured split of a block and the plans of both kernels (csrc/osm_geo.hpp: osm_levels)
//   route off|on|failed <N> ...  what a two-level block runs with on the general LDS Stockham kernels (csrc/gen_host.hpp)
//   source <N> | source2 <N>     the translation unit an overlap-save plan compiles for a block (osm_g2_source)
//   osm 0|1|failed <n_fft> <n_stream> ...   levels and buffers of a plan: BBT_RTC=0, compiled, compilation failed
//   parts <run> <chunk> <cap> <lanes> <fork> ...   how a regular run is cut into launches (osm_run_parts)
//   launches 0|1|failed <n_fft> <n_stream> <nblk> <reg_count> <n_chan> <det> <in_plane> <timing> <mid_mib> ...
//                                the kernel launches of one chunk of that plan (csrc/osm_launch.hpp: osm_chunk_launches),
//                                or the refusal; mid_mib: BBT_OSM_MID_MIB, 128 unless set
//   chan [dir=<d>] <n_chan> <n_stream> ...   a channelizer plan (csrc/chan_geo.hpp): its kind or the refusal, the candidates
//                                a timed plan compares, and the untimed choice (-1: none) with the default knobs, with
//                                BBT_G2_TUNE=0, with BBT_G2_CHAN_WIDE too, and with 116 remembered
//   pfb <knobs> <n_tap> <n_chan> <n_stream> ...   a filter-bank plan (csrc/pfb_geo.hpp): the shape or the refusal, and the
//                                route; knobs: - or a list of tune=0, two=0|1, pp=<n>, gl=<n> (the BBT_PFB_* switches)
//   quads <n_tap> <n_chan> <T>   the taps h[i] = i as the window kernels read them (pfb_tap_quads)
// No environment variable decides anything here: the knobs are the defaults, or the arguments.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "chan_geo.hpp"
#include "osm_launch.hpp"
#include "pfb_geo.hpp"
using namespace bbt;

static const char* chan_kind_name(ChanKind k) {
    return k == CHAN_SHORT ? "short" : k == CHAN_ROWS ? "rows" : k == CHAN_BIG ? "big" : "generic";
}
static void print_text(const std::string& text) {        // as a JSON string
    putchar('"');
    for (char c : text) {
        if (c == '\n') printf("\\n");
        else if (c == '"' || c == '\\') printf("\\%c", c);
        else putchar(c);
    }
    putchar('"');
}

static void dump(const G2Plan& g) {
    printf("{\"n\": %d, \"tj\": %d, \"ct\": %d, \"threads\": %d, \"slots\": %d, \"lds_elems\": %d, \"table_len\": %d, \"fac\": [",
           g.n, g.tj, g.ct, g.threads(), g.slots, g.lds_elems, g.table_len);
    for (int s = 0; s < g.nfac; ++s) printf("%s%d", s ? ", " : "", g.fac[s]);
    printf("], \"pitch\": [");
    for (int s = 0; s < g.nfac; ++s) printf("%s%d", s ? ", " : "", g.pitch[s]);
    printf("], \"woff\": [");
    for (int s = 0; s < g.nfac; ++s) printf("%s%d", s ? ", " : "", g.woff[s]);
    printf("]}");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "plan")) {
        const int pmax = atoi(argv[2]);
        for (int i = 3; i + 1 < argc; i += 2) {
            G2Plan g;
            if (!g2_plan(atoi(argv[i]), atoi(argv[i + 1]), &g, pmax)) { printf("null\n"); continue; }
            printf("{\"forward\": ");
            dump(g);
            printf(", \"reversed\": ");
            dump(g2_reversed(g));
            printf(", \"source\": \"%s\"}\n", "ok");
        }
    } else if (!strcmp(argv[1], "split")) {
        for (int i = 2; i < argc; ++i) {
            OsmGeo g;
            std::string text;
            if (!osm_levels(atoll(argv[i]), 2, OsmKnobs(), &g, &text) || !g.measured || !g.compiled) { printf("null\n"); continue; }
            printf("{\"n1\": %d, \"n2\": %d, \"col\": ", g.n1, g.n2);
            dump(g.q1);
            printf(", \"row\": ");
            dump(g.q2);
            printf("}\n");
        }
    } else if (!strcmp(argv[1], "route")) {
        // mode: plan-time compilation off (BBT_RTC=0), on, or on and failed (the general kernels
        // then run with the split and the tile chosen for the compiled ones)
        const int mode = !strcmp(argv[2], "off") ? BBT_GEN_RTC_OFF : !strcmp(argv[2], "on") ? BBT_GEN_RTC_ON : BBT_GEN_RTC_FAILED;
        for (int i = 3; i < argc; ++i) {
            const long long n = atoll(argv[i]);
            int n1 = 0, n2 = 0;
            bool measured = false;          // (the split is the one measured for the compiled kernels)
            GenGeo f1, f2;
            if (!gen_split(n, mode != BBT_GEN_RTC_OFF, &n1, &n2, &measured) || !gen_factor_7smooth(n1, &f1) || !gen_factor_7smooth(n2, &f2)) {
                printf("null\n");
                continue;
            }
            const int ct = gen_col_ct(n, n1, mode);
            // (the columns the compiled kernels take on this split)
            int g2_ct = gen_col_ct_wanted(n, n1, true);
            G2Plan q1;
            const bool fits = g2_fit_col_plan(n1, &g2_ct, &q1);
            printf("{\"n\": %lld, \"n1\": %d, \"n2\": %d, \"ct\": %d, \"col_threads\": %d, \"col_lds\": %lld, "
                   "\"row_threads\": %d, \"row_lds\": %lld, \"g2_split\": %s, \"g2_ct\": %d, \"g2_fits\": %s, \"fac1\": [",
                   n, n1, n2, ct, gen_threads(n1 * ct), (long long)n1 * ct * 16, gen_threads(n2), (long long)n2 * 16,
                   measured ? "true" : "false", g2_ct, fits ? "true" : "false");
            for (int s = 0; s < f1.nfac; ++s) printf("%s%d", s ? ", " : "", f1.fac[s]);
            printf("], \"fac2\": [");
            for (int s = 0; s < f2.nfac; ++s) printf("%s%d", s ? ", " : "", f2.fac[s]);
            printf("]}\n");
        }
    } else if (!strcmp(argv[1], "source") || !strcmp(argv[1], "source2")) {
        // what bbt_osm_plan_create compiles for a block of one kernel (source) or of two levels (source2)
        OsmGeo g;
        std::string text;
        const bool two = !strcmp(argv[1], "source2");
        if (!osm_levels(atoll(argv[2]), 2, OsmKnobs(), &g, &text)) return 1;
        if (!g.generic && !two) {
            // (a power of two: its plan compiles nothing; the same text on the traits of the length, for
            // tests/test_conversion_host.py, which puts another plan's kernel on them)
            g.n1 = 1;
            if (!g2_plan(atoi(argv[2]), 1, &g.q2, g2_pmax(BBT_G2_KIND_ROW))) return 1;
            g.q2r = g2_reversed(g.q2);
        } else if (!g.compiled || (g.n1 > 1) != two) {
            return 1;
        }
        // (source: with the channelizer's kernel on the same traits -- chan_g2_candidate of csrc/chan_geo.hpp -- as a second entry point)
        printf("%s%s", osm_g2_source(g).text.c_str(), two ? "" : "BBT_G2_KERNEL_FFT_ROWS(k_rows, GA, -1, 0)\n");
    } else if (!strcmp(argv[1], "osm")) {
        OsmKnobs knobs;
        knobs.rtc = !strcmp(argv[2], "0") ? 0 : 1;
        const bool rtc_ok = !strcmp(argv[2], "1");
        for (int i = 3; i + 1 < argc; i += 2) {
            OsmGeo g;
            std::string text;
            const long long n = atoll(argv[i]);
            if (!osm_levels(n, atoi(argv[i + 1]), knobs, &g, &text)) {
                printf("{\"n_fft\": %lld, \"n_stream\": %d, \"error\": \"%s\"}\n", n, atoi(argv[i + 1]), text.c_str());
                continue;
            }
            osm_buffers(&g, g.generic && g.compiled && rtc_ok, knobs);
            printf("{\"n_fft\": %lld, \"n_stream\": %d, \"outer\": %d, \"n1\": %d, \"n2\": %d, \"n2p\": %d, \"gen_ct\": %d, "
                   "\"lanes\": %d, \"chunk\": %d, \"cap\": %d, \"work_bytes\": %lld, \"workspace_bytes\": %lld}\n",
                   n, g.S, g.outer, g.n1, g.n2, g.n2p, g.gen_ct, g.lanes, g.chunk, g.cap, (long long)g.work_bytes,
                   (long long)g.work_bytes * g.lanes);
        }
    } else if (!strcmp(argv[1], "parts")) {
        for (int i = 2; i + 4 < argc; i += 5) {
            int64_t parts, per;
            osm_run_parts(atoll(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]) != 0, &parts, &per);
            printf("{\"parts\": %lld, \"per\": %lld}\n", (long long)parts, (long long)per);
        }
    } else if (!strcmp(argv[1], "launches")) {
        OsmKnobs knobs;
        knobs.rtc = !strcmp(argv[2], "0") ? 0 : 1;
        const bool rtc_ok = !strcmp(argv[2], "1");
        std::vector<OsmLaunch> list;
        for (int i = 3; i + 8 < argc; i += 9) {
            OsmGeo g;
            std::string text;
            if (!osm_levels(atoll(argv[i]), atoi(argv[i + 1]), knobs, &g, &text)) {
                printf("{\"error\": \"%s\"}\n", text.c_str());
                continue;
            }
            osm_buffers(&g, g.generic && g.compiled && rtc_ok, knobs);
            OsmLaunchPlan lp;
            lp.n = g.n;
            lp.generic = g.generic;
            lp.rtc = g.generic && g.compiled && rtc_ok;
            lp.single = g.single;
            lp.outer = g.outer;
            lp.n1 = g.n1;
            lp.n2 = g.n2;
            lp.n2p = g.n2p;
            lp.npair = g.npair;
            lp.S = g.S;
            lp.gen_ct = g.gen_ct;
            lp.q1_threads = g.q1.threads();
            lp.q1_ct = g.q1.ct;
            lp.q2_threads = g.q2.threads();
            lp.q2_ct = g.q2.ct;
            lp.tw_col = !g.generic && g.n1 >= 256 && g.outer == 1;       // (bbt_hip.hip: osm_pow2_tables)
            OsmChunkFacts c;
            c.nblk = atoi(argv[i + 2]);
            c.reg_count = atoi(argv[i + 3]);
            c.n_chan = atoi(argv[i + 4]);
            c.det = atoi(argv[i + 5]) != 0;
            c.in_plane = atoi(argv[i + 6]) != 0;
            c.timing = atoi(argv[i + 7]) != 0;
            knobs.mid_mib = atoi(argv[i + 8]);
            if (const char* refusal = osm_chunk_launches(lp, c, knobs, &list)) {
                printf("{\"error\": \"%s\"}\n", refusal);
                continue;
            }
            printf("{\"chunk\": %d, \"npair\": %d, \"outer\": %d, \"n1\": %d, \"n2\": %d, \"fusable\": %s, \"launches\": [", g.chunk,
                   g.npair, g.outer, g.n1, g.n2, osm_fusable(g.generic, g.single, g.outer, g.n1, g.n2, c.n_chan) ? "true" : "false");
            for (size_t j = 0; j < list.size(); ++j) {
                const OsmLaunch& l = list[j];
                const char* const tf[] = {"false", "true"};
                printf("%s{\"kernel\": \"%s\", \"targs\": [", j ? ", " : "", osm_family_name(l.family));
                // (the template arguments as a trace demangles them)
                switch (l.family) {
                    case OSM_COL16: printf("\"%s\", \"%s\", \"%s\", \"%d\"", tf[l.first], tf[l.spec], tf[l.single], l.pp); break;
                    case OSM_COL256:
                        printf("\"%s\", \"%s\", \"%d\", \"%s\", \"%d\", \"%s\", \"%d\"", tf[l.first], tf[l.spec], l.F, tf[l.det], l.pp,
                               tf[l.single], l.n);
                        break;
                    case OSM_ROWPASS: printf("\"%d\", \"%d\"", l.n, l.nch); break;
                    case OSM_MID16: case OSM_GEN_COL: printf("\"%s\"", tf[l.first]); break;
                    case OSM_SMALL: printf("\"%d\", \"%d\", \"%s\"", l.n, l.pp, tf[l.single]); break;
                    case OSM_SMALL_BIG: printf("\"%d\", \"%s\"", l.n, tf[l.single]); break;
                    default: break;
                }
                printf("], \"grid\": [%u, %u], \"threads\": %d, \"lds\": %lld, \"raise_lds\": %s, \"row_len\": %d, \"y0\": %d, "
                       "\"ny\": %d, \"mid_mode\": %d, \"tw\": %s, \"mark\": %d}",
                       l.gx, l.gy, l.threads, (long long)l.lds, tf[l.raise_lds], l.row_len, l.y0, l.ny, l.mid_mode, tf[l.tw], l.mark);
            }
            printf("]}\n");
        }
    } else if (!strcmp(argv[1], "chan")) {
        int direction = -1;
        int i = 2;
        if (!strncmp(argv[i], "dir=", 4)) direction = atoi(argv[i++] + 4);
        for (; i + 1 < argc; i += 2) {
            const int n_chan = atoi(argv[i]), n_stream = atoi(argv[i + 1]);
            ChanShape shape;
            std::string error;
            printf("{\"n_chan\": %d, \"n_stream\": %d, ", n_chan, n_stream);
            if (!chan_check(n_chan, n_stream, direction, &shape, &error)) {
                printf("\"error\": ");
                print_text(error);
                printf("}\n");
                continue;
            }
            ChanKnobs untimed, untimed_wide;
            untimed.tune = untimed_wide.tune = false;
            untimed_wide.wide = true;
            printf("\"kind\": \"%s\", \"single\": %s, \"split_real\": %s, \"direction\": %d, \"untimed\": [%d, %d, %d, %d], "
                   "\"candidates\": [", chan_kind_name(shape.kind), shape.single ? "true" : "false", shape.split_real ? "true" : "false",
                   shape.direction, chan_untimed_code(-1, ChanKnobs()), chan_untimed_code(-1, untimed),
                   chan_untimed_code(-1, untimed_wide), chan_untimed_code(116, untimed));
            // (8192 channels: what the rule would list on its own -- the product runs them on the `big` kernels)
            if (shape.kind == CHAN_GENERIC || n_chan == BBT_GEN_MAX_LEN) {
                bool first = true;
                for (const ChanCandidate& c : chan_candidates(n_chan, n_stream / 2, shape.direction, ChanKnobs(), &error)) {
                    printf("%s{\"code\": %d, \"cp\": %d, \"plan\": ", first ? "" : ", ", c.code, c.cp);
                    dump(c.q);
                    printf(", \"source\": ");
                    print_text(c.source);
                    printf("}");
                    first = false;
                }
            }
            printf("]}\n");
        }
    } else if (!strcmp(argv[1], "pfb")) {
        PfbKnobs knobs;
        for (const char* a = argv[2]; a && *a && *a != '-'; a = strchr(a, ',') ? strchr(a, ',') + 1 : nullptr) {
            if (!strncmp(a, "tune=", 5)) knobs.tune = atoi(a + 5) != 0;
            else if (!strncmp(a, "two=", 4)) knobs.two_pass = atoi(a + 4) != 0;
            else if (!strncmp(a, "pp=", 3)) knobs.pp = atoi(a + 3);
            else if (!strncmp(a, "gl=", 3)) knobs.gl = atoi(a + 3);
            else return 2;
        }
        for (int i = 3; i + 2 < argc; i += 3) {
            const int n_tap = atoi(argv[i]), n_chan = atoi(argv[i + 1]), n_stream = atoi(argv[i + 2]);
            PfbShape s;
            std::string error;
            printf("{\"n_tap\": %d, \"n_chan\": %d, \"n_stream\": %d, ", n_tap, n_chan, n_stream);
            if (!pfb_check(n_tap, n_chan, n_stream, &s, &error)) {
                printf("\"error\": ");
                print_text(error);
                printf("}\n");
                continue;
            }
            const PfbRoute r = pfb_route(knobs, s);
            printf("\"streams\": %d, \"split_real\": %s, \"window\": %s, \"pp_ok\": %s, \"gn\": %d, \"two_ok\": %s, "
                   "\"rule_two\": %s, \"timed\": %s, \"fixed\": [%d, %d], \"candidates\": [", s.S, s.split_real ? "true" : "false",
                   s.window ? "true" : "false", s.pp_ok ? "true" : "false", s.gn, s.two_ok ? "true" : "false",
                   s.rule_two ? "true" : "false", r.timed ? "true" : "false", r.fixed.pp, r.fixed.gl);
            for (size_t c = 0; c < r.candidates.size(); ++c)
                printf("%s[%d, %d]", c ? ", " : "", r.candidates[c].pp, r.candidates[c].gl);
            printf("]}\n");
        }
    } else if (!strcmp(argv[1], "quads")) {
        if (argc < 5) return 2;
        const int n_tap = atoi(argv[2]), n_chan = atoi(argv[3]), T = atoi(argv[4]);
        std::vector<float> h((size_t)n_tap * n_chan);
        for (size_t j = 0; j < h.size(); ++j) h[j] = (float)j;
        const std::vector<float> q = pfb_tap_quads(h.data(), n_tap, n_chan, T);
        printf("[");
        for (size_t j = 0; j < q.size(); ++j) printf("%s%d", j ? ", " : "", (int)q[j]);
        printf("]\n");
    }
    return 0;
}
