// How k_sk_estimate / k_sk_excise (sk_kernels.hpp) cut a stream x[block][sample][element] into
// tiles: plain C++, shared by the host launcher and the kernels (the struct is a kernel argument)
// and compiled on its own by tests/sk_geo_check.cpp.
//
// A workgroup of 256 threads owns a tile of `w` adjacent elements (columns) of `nz` consecutive
// blocks of n samples.  A thread reads `v` adjacent elements in one access: 16 bytes (2 complex64,
// 4 float32) where the arrays are 16-byte aligned and n_elem is a multiple of v -- every sample
// then starts on an access --, else one element.  w is a multiple of v and of the join group g,
// so no access and no group straddles two tiles.  The threads of a workgroup are (tx, ty, tz):
//   tx < nx = w / v   along the elements (the lanes: coalesced)
//   ty < ny           the threads that share a column: in the sums they take whole segments of
//                     BBT_SK_SEG samples, segment r * ny + ty in round r; in the rewrite, sample
//                     ty, ty + ny, ...  ny = 1: a thread walks whole columns
//   tz < nz           the block of the workgroup's nz
// with nx * ny * nz <= 256; ny <= segments of a block, so no thread is idle for want of segments
// where blocks are short, and the workgroup takes several blocks instead.
//
// For the excision the tile is sized so that its slab, nz * n * w elements, is about BBT_SK_SLAB
// bytes and still in cache when the second pass comes back for it, but never narrower than
// BBT_SK_ROW bytes of a sample (a whole cache line per sample and tile); the estimate alone reads
// once and takes the widest tile.  Either way a launch of fewer than BBT_SK_FILL workgroups halves
// its tiles, down to that least width, so that few long blocks still occupy every CU.
#pragma once

#define BBT_SK_THREADS 256
#define BBT_SK_SEG 32                    // samples of a segment of the two-level sums
#define BBT_SK_MAX_N 65536
#define BBT_SK_MAX_GROUP 64
#define BBT_SK_SLAB (128 * 1024)         // bytes of a slab the rewrite should find in cache
#define BBT_SK_ROW 128                   // least bytes of a sample in a tile
#define BBT_SK_FILL 1024                 // workgroups a launch should have (256 CUs, a few each)

struct SkGeo {
    int v;               // elements per access
    int w;               // elements of a tile
    int nx, ny, nz;      // threads along the elements, per column, blocks per workgroup
    long long n_tile;    // tiles across the elements
    long long n_zgroup;  // workgroups along the blocks
};

// 0, or what is wrong with the shape (a static string).  `slab`: bytes a tile's slab should stay
// below (0: no second pass, the widest tile).
inline const char* sk_geo(long long n_block, long long n, long long n_elem, int is_complex, long long group,
                          bool aligned16, long long slab, SkGeo* g) {
    if (n < 2 || n > BBT_SK_MAX_N) return "n must be 2 ... 65536";
    if (n_block < 1 || n_elem < 1) return "an empty axis";
    if (group < 1 || group > BBT_SK_MAX_GROUP) return "the group must be 1 ... 64 elements";
    if (n_elem % group) return "the group does not divide n_elem";
    if (n_elem >= (1ll << 31) || n_block >= (1ll << 31)) return "an axis of 2^31 or more elements";
    const int nt = BBT_SK_THREADS;
    const int item = is_complex ? 8 : 4;
    const int wide = 16 / item;
    g->v = aligned16 && n_elem % wide == 0 ? wide : 1;
    // unit = lcm(v, group): v is a power of two
    long long unit = group;
    while (unit % g->v) unit *= 2;
    const long long w_max = (long long)nt * g->v / unit * unit;        // (unit <= 64 v)
    long long w = w_max;
    const long long least = (BBT_SK_ROW / item + unit - 1) / unit * unit;
    if (slab > 0) {
        long long fit = slab / (n * item);
        if (fit < least) fit = least;
        fit = fit / unit * unit;
        if (fit < w) w = fit;
    }
    if (w > n_elem) w = n_elem;                                        // (n_elem is a multiple of unit)
    // few blocks: narrower tiles, down to the least, until there are workgroups for every CU
    while ((n_elem + w - 1) / w * n_block < BBT_SK_FILL && w / 2 >= least) w = w / 2 / unit * unit;
    // tiles of about one width: the last one is not a sliver
    g->n_tile = (n_elem + w - 1) / w;
    w = ((n_elem + g->n_tile - 1) / g->n_tile + unit - 1) / unit * unit;
    g->n_tile = (n_elem + w - 1) / w;
    g->w = (int)w;
    g->nx = (int)(w / g->v);
    const long long n_seg = (n + BBT_SK_SEG - 1) / BBT_SK_SEG;
    long long ny = nt / g->nx;
    if (ny > n_seg) ny = n_seg;
    g->ny = (int)ny;
    long long nz = nt / (g->nx * ny);
    if (nz > n_block) nz = n_block;
    g->nz = (int)nz;
    g->n_zgroup = (n_block + nz - 1) / nz;
    if (g->n_tile * g->n_zgroup >= (1ll << 31)) return "too many tiles for one launch";
    return 0;
}
