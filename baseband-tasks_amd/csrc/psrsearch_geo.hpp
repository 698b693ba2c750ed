// How k_psrsearch_encode / k_psrsearch_decode (psrsearch_kernels.hpp) cut a PSRFITS search-mode
// row into tiles: plain C++, shared by the host launcher and the kernels (the struct is a kernel
// argument) and compiled on its own by tests/psrsearch_geo_check.cpp.
//
// A workgroup of 256 threads owns `ct` channels of one row with all their polarizations: w = ct *
// n_pol <= 256 columns that are adjacent in x[sample][chan][pol].  `unit` codes leave in one store:
// a byte's 8 / nbits, or a dword's 32 / nbits when `vec` (the codes pointer 4-byte aligned and a
// polarization's run of a sample, n_chan * nbits / 8 bytes, a multiple of 4); ct is a multiple of
// it, so every tile starts on a store.  With 64 columns or more in the row a thread owns a column
// and walks its samples in order (ny = 1); with fewer, ny = 256 / w threads share a column,
// thread t taking samples t, t + ny, ..., and their sums meet in a tree.
//
// The coding pass keeps `ts` samples of the tile in LDS, a dword per code: sample t, polarization
// p, channel c of the tile at  t * n_pol * pol_pitch + p * pol_pitch + c + c / 32.  The c / 32 puts
// the runs that the lanes of a store read (unit = 4 ... 32 dwords apart) on different banks; the
// pitch, = 32 / n_pol mod 32 for n_pol a power of two, does the same for the writes of a half-wave,
// which run along (chan, pol).
#pragma once

#define BBT_PSRSEARCH_THREADS 256
#define BBT_PSRSEARCH_LDS 8192           // dwords of the coding tile
#define BBT_PSRSEARCH_MANY 64            // columns of a row from which a thread owns a column
#define BBT_PSRSEARCH_MAX_POL 32

struct PsrSearchGeo {
    int ct;              // channels of a tile
    int unit;            // codes of one store
    int vec;             // stores are dwords
    int ny;              // threads that share a column in the statistics pass
    int pol_pitch;       // dwords between the polarizations of a sample in LDS
    int ts;              // samples of a coding tile
    long long n_tile;    // tiles of a row
};

// 0, or what is wrong with the shape (a static string)
inline const char* psrsearch_geo(long long nsblk, long long n_chan, long long n_pol, int nbits, bool aligned4,
                                 PsrSearchGeo* g) {
    if (nbits != 1 && nbits != 2 && nbits != 4 && nbits != 8) return "nbits must be 1, 2, 4 or 8";
    if (nsblk < 1 || n_chan < 1 || n_pol < 1) return "an empty axis";
    if (n_pol > BBT_PSRSEARCH_MAX_POL) return "more than 32 polarizations";
    if (nsblk >= (1ll << 31) || n_chan >= (1ll << 31) || n_chan * n_pol >= (1ll << 31))
        return "an axis of 2^31 or more elements";
    const int cpb = 8 / nbits;
    if (n_chan % cpb) return "n_chan * nbits is not a multiple of 8: a polarization's channels must fill whole bytes";
    const int nt = BBT_PSRSEARCH_THREADS;
    g->vec = aligned4 && (n_chan / cpb) % 4 == 0 && n_pol * 4 * cpb <= nt;
    g->unit = g->vec ? 4 * cpb : cpb;
    long long ct = (nt / n_pol) / g->unit * g->unit;
    if (ct > n_chan) ct = n_chan;
    g->ct = (int)ct;
    const int w = (int)(ct * n_pol);
    g->ny = n_chan * n_pol >= BBT_PSRSEARCH_MANY ? 1 : nt / w;
    const int run = g->ct + g->ct / 32;
    const int want = (n_pol & (n_pol - 1)) == 0 ? (int)(32 / n_pol) % 32 : 1;
    g->pol_pitch = run + ((want - run) % 32 + 32) % 32;
    g->ts = BBT_PSRSEARCH_LDS / (int)(n_pol * g->pol_pitch);
    g->n_tile = (n_chan + ct - 1) / ct;
    return 0;
}
