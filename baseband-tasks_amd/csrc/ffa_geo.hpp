// How k_ffa_segments / k_ffa_prefix / k_ffa_total / k_ffa_pass / k_ffa_snr / k_ffa_merge (ffa_kernels.hpp) cut one launch of FFASearch
// (ffa.py) into workgroups: plain C++, shared by the host launcher and the kernels (the struct is a
// kernel argument) and compiled on its own by tests/ffa_geo_check.cpp.
//
// A launch is one block x[i][e], i < n, of a stream with `pitch` elements per sample, of which the ne
// columns from e0 on are searched at one base period p.  m = n / p rows of real data, M the power of two
// with M / 2 < m <= M, L = log2(M) stages.  A row is its p bins of ne columns flattened, `lane` = p ne
// floats, so that a roll by c bins is a rotation by c ne lanes: two contiguous runs.
//
// The transform runs in n_pass = ceil(L / fuse) launches; pass q makes `lv` stages at once, from groups of
// G0 = 2^s0 rows to groups of G0 2^lv: output row t of a group is the tree sum of 2^lv leaves, leaf u
// being row u G0 + (t >> lv) of the group as the pass before left it, rotated by ffa_leaf_shift(t, u, lv)
// bins.  Pass 0 reads the block in place (rows >= m are +0, never read); pass q writes scratch buffer q &
// 1.  The S/N pass reads the last of them, nr whole rows of ex columns per workgroup in LDS, and leaves
// one partial winner per (row group, column) in the other buffer; k_ffa_merge folds those into the
// output.
//
// Every index into the block, the scratch and the result is 64-bit; a lane index fits an int.
#pragma once

#define BBT_FFA_THREADS 256
#define BBT_FFA_SEG 32                       // samples of a segment of the two-level sum T
#define BBT_FFA_MIN_P 4
#define BBT_FFA_MAX_P 1025                   // p_hi at most: base periods up to 1024 bins
#define BBT_FFA_MAX_ROWS 65536               // n / p_lo at most
#define BBT_FFA_MAX_WIDTHS 10                // widths 1 ... 512
#define BBT_FFA_FUSE 2                       // stages per pass (default): 1, 2 or 3
#define BBT_FFA_FUSE_MAX 3
#define BBT_FFA_WIDTH 16                     // columns of an S/N workgroup at most (default): 4, 8, 16 or 32
#define BBT_FFA_CAP 8192                     // floats of one of the two LDS buffers of the S/N pass
#define BBT_FFA_MAX_LANE (1 << 30)           // p ne below this
#define BBT_FFA_MAX_BUF (1ll << 34)          // M p ne at most
#define BBT_FFA_MERGE_NX 8                   // columns of a workgroup of k_ffa_merge
#define BBT_FFA_MAX_GRID (1ll << 24)         // workgroups of a launch below this
#define BBT_FFA_NO_ROW 1073741824           // the row of "no winner yet": 2^30, exact as a float

#ifdef __HIPCC__
#define BBT_FFA_HD __host__ __device__
#else
#define BBT_FFA_HD
#endif

// m rows of data, padded to M = 2^L
BBT_FFA_HD inline void ffa_rows(long long n, long long p, long long* m, long long* M, int* L) {
    *m = n / p;
    long long P2 = 1;
    int l = 0;
    while (P2 < *m) P2 *= 2, ++l;
    *M = P2, *L = l;
}

// shift(r, t, M): the bins row r < M is rotated by in final row t < M
BBT_FFA_HD inline long long ffa_shift(long long r, long long t, long long M) {
    long long s = 0;
    while (M > 1) {
        const long long h = M / 2;
        if (r >= h) s += (t + 1) >> 1, r -= h;
        t >>= 1, M = h;
    }
    return s;
}

// the rotation of leaf u < 2^lv in output row t of a group made by lv fused stages: stage l < lv adds
// ((t >> (lv - 1 - l)) + 1) >> 1 to the upper half, the leaves with bit l set
BBT_FFA_HD inline long long ffa_leaf_shift(long long t, int u, int lv) {
    long long s = 0;
    for (int l = 0; l < lv; ++l)
        if ((u >> l) & 1) s += ((t >> (lv - 1 - l)) + 1) >> 1;
    return s;
}

// a_k = float32(sqrt(p / (2^k (p - 2^k) m))), formed in float64: the denominator is an exact integer
inline float ffa_scale(long long p, long long m, int k);

struct FfaGeo {
    long long n, p, m, M;        // samples of the block, bins, rows of data, rows
    int L, K;                    // stages, widths
    long long pitch, ne;         // elements of a sample of the stream, columns of this launch
    int lane;                    // p ne
    int fuse, n_pass;
    int ex, nr;                  // S/N pass: columns and rows of a workgroup; nr p ex <= BBT_FFA_CAP
    long long n_et, n_rg;        // S/N pass: workgroups along the columns, along the rows
    long long n_lt;              // transform: workgroups along a row
    long long buf;               // floats of one scratch buffer: M lane
    float a[BBT_FFA_MAX_WIDTHS]; // a_k
};

// doubles of the running segment sums of a column: one in front of every whole segment of the block, and the last
inline long long ffa_prefix(long long n) { return n / BBT_FFA_SEG + 1; }

// floats of scratch a plan needs for ne columns: the running segment sums (float64), the c_k, then two buffers
// of the largest M p
inline long long ffa_scratch(long long n, long long max_mp, long long ne) {
    return (2 * ffa_prefix(n) + BBT_FFA_MAX_WIDTHS + 2 * max_mp) * ne;
}

// 0, or what is wrong with the sizes of a plan (a static string)
inline const char* ffa_sizes(long long n, long long p_lo, long long p_hi, long long K, long long n_elem) {
    if (p_lo < BBT_FFA_MIN_P || p_lo >= p_hi || p_hi > BBT_FFA_MAX_P) return "the periods must obey 4 <= p_lo < p_hi <= 1025";
    if (n < 1 || n / (p_hi - 1) < 2) return "a block must hold two rows of the longest period at least";
    if (n / p_lo > BBT_FFA_MAX_ROWS) return "a block may hold 65536 rows of the shortest period at most";
    if (K < 1 || K > BBT_FFA_MAX_WIDTHS) return "n_widths must be 1 ... 10";
    if ((1ll << (K - 1)) >= p_lo) return "the widest boxcar, 2^(n_widths - 1), must be shorter than p_lo";
    if (n_elem < 1) return "no elements";
    return 0;
}

// the largest M p over the base periods of a plan
inline long long ffa_max_mp(long long n, long long p_lo, long long p_hi) {
    long long best = 0;
    for (long long p = p_lo; p < p_hi; ++p) {
        long long m, M;
        int L;
        ffa_rows(n, p, &m, &M, &L);
        if (M * p > best) best = M * p;
    }
    return best;
}

#include <math.h>
inline float ffa_scale(long long p, long long m, int k) {
    const long long w = 1ll << k;
    const double den = (double)(w * (p - w) * m);
    const double q = (double)p / den;
    return (float)sqrt(q);
}

// 0, or what is wrong with a launch.  fuse: 1, 2 or 3; width: 4, 8, 16 or 32 (each 0: the default).
inline const char* ffa_geo(long long n, long long p, long long K, long long pitch, long long e0, long long ne, int fuse,
                           int width, FfaGeo* g) {
    if (p < BBT_FFA_MIN_P || p >= BBT_FFA_MAX_P) return "the period must be 4 ... 1024";
    if (n < 1 || n / p < 2 || n / p > BBT_FFA_MAX_ROWS) return "a block must hold 2 ... 65536 rows";
    if (K < 1 || K > BBT_FFA_MAX_WIDTHS || (1ll << (K - 1)) >= p) return "n_widths must be 1 ... 10, the widest boxcar shorter than p";
    if (e0 < 0 || ne < 1 || pitch < 1 || e0 > pitch - ne) return "the columns are not those of the stream";
    if (fuse == 0) fuse = BBT_FFA_FUSE;
    if (width == 0) width = BBT_FFA_WIDTH;
    if (fuse < 1 || fuse > BBT_FFA_FUSE_MAX) return "the stages of a pass must be 1, 2 or 3";
    if (width != 4 && width != 8 && width != 16 && width != 32) return "the width must be 4, 8, 16 or 32 columns";
    if (ne > (BBT_FFA_MAX_LANE - 1) / p) return "too many columns for one launch";
    g->n = n, g->p = p, g->K = (int)K, g->pitch = pitch, g->ne = ne;
    ffa_rows(n, p, &g->m, &g->M, &g->L);
    g->lane = (int)(p * ne);
    if (g->M > BBT_FFA_MAX_BUF / g->lane) return "more than 2^34 values in one launch";
    g->buf = g->M * g->lane;
    g->fuse = fuse, g->n_pass = (g->L + fuse - 1) / fuse;
    int ex = 1;
    while (ex * 2 <= width && ex * 2 * p <= BBT_FFA_CAP) ex *= 2;
    g->ex = ex;
    long long nr = BBT_FFA_CAP / (p * ex);
    if (nr > g->M) nr = g->M;
    g->nr = (int)nr;
    g->n_et = (ne + ex - 1) / ex;
    g->n_rg = (g->M + nr - 1) / nr;
    g->n_lt = (g->lane + BBT_FFA_THREADS - 1) / BBT_FFA_THREADS;
    // every grid stays below 2^24 workgroups of 256 threads, 2^32 threads: the largest fold pass has M / 2 rows of
    // workgroups (one stage), the segment sums one thread per (segment, column)
    const long long most = BBT_FFA_MAX_GRID;
    if (g->n_et >= most / g->n_rg || g->n_lt >= most / (g->M / 2) ||
        (n / BBT_FFA_SEG + 1) * ne / BBT_FFA_THREADS >= most || ne / BBT_FFA_MERGE_NX >= most)
        return "too many tiles for one launch";
    for (int k = 0; k < BBT_FFA_MAX_WIDTHS; ++k) g->a[k] = k < K ? ffa_scale(p, g->m, k) : 0.f;
    return 0;
}

// Pass q < n_pass: the stages done before it, those it makes, and its grid.
struct FfaPass {
    int s0, lv;
    long long n_wg;
};
inline FfaPass ffa_pass(const FfaGeo& g, int q) {
    FfaPass o;
    o.s0 = q * g.fuse;
    o.lv = g.L - o.s0 < g.fuse ? g.L - o.s0 : g.fuse;
    o.n_wg = (g.M >> o.lv) * g.n_lt;
    return o;
}

// What workgroup wg of a pass owns: the group of rows and the row in its 2^s0 (rq = group 2^s0 + tq), the
// first lane.  Leaf u < 2^lv is input row in0 + (u << s0); output t = (tq << lv) + v, v < 2^lv, is row out0 + v.
struct FfaOwn {
    long long in0, out0, tq;
    int x0;
};
BBT_FFA_HD inline void ffa_own(const FfaGeo& g, long long wg, int s0, int lv, FfaOwn* o) {
    const long long rq = wg / g.n_lt;
    const long long grp = rq >> s0;
    o->tq = rq & ((1ll << s0) - 1);
    o->x0 = (int)(wg % g.n_lt) * BBT_FFA_THREADS;
    o->in0 = (grp << (s0 + lv)) + o->tq;
    o->out0 = (grp << (s0 + lv)) + (o->tq << lv);
}

// where lane x < lane of data row r < m lies in the block, relative to column e0 of sample 0
BBT_FFA_HD inline long long ffa_in_at(const FfaGeo& g, long long r, int x) {
    if (g.pitch == g.ne) return r * g.lane + x;
    const long long j = x / g.ne, e = x - j * g.ne;
    return (r * g.p + j) * g.pitch + e;
}
