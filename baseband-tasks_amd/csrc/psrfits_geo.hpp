// How k_psrfits_encode / k_psrfits_decode (psrfits_kernels.hpp) cut a PSRFITS fold-mode row into
// tiles: plain C++, shared by the host launchers (which instantiation runs, how many workgroups)
// and the kernels (the shape of a tile, from the same two numbers) and compiled on its own by
// tests/psrfits_geo_check.cpp.
//
// A row is an n_bin x n_col matrix of floats, n_col = n_chan * n_pol.  A workgroup of 256 threads
// owns `tc` adjacent columns of one row and all their bins: 32 columns, or 4 when the row has fewer
// than 32 (narrow tiles, long along the bins).  It walks them in tiles of 4096 samples, tb = 4096 /
// tc bins at a time.  A thread owns cpt columns: 4 when `vec` -- floats move as float4 and codes as
// dwords of two: x / out 16-byte aligned, n_col a multiple of 4, codes 4-byte aligned, n_bin even --
// else 1.  nx = tc / cpt threads lie across the columns and ny = 256 / nx along the bins.
//
// LDS: the encoder keeps a tile as dwords of two codes, column pitch tb / 2 + 1 (odd: the writes of
// a half-wave fall on 32 banks, the reads run along a column); the decoder as floats, column pitch
// tb + 1.
#pragma once

#define BBT_PSRFITS_THREADS 256
#define BBT_PSRFITS_TILE 4096            // samples of a tile: tc columns x tb bins
#define BBT_PSRFITS_WIDE 32              // columns of a row from which a tile has 32 of them

struct PsrFitsTile {
    int tc;              // columns of a tile
    int cpt;             // columns of a thread
    int nx, ny;          // threads across the columns, along the bins
    int tb, np;          // bins, pairs of bins of a tile
    int enc_pitch;       // dwords between the columns of the encoder's LDS tile
    int dec_pitch;       // floats between the columns of the decoder's
};

constexpr PsrFitsTile psrfits_tile(int tc, bool vec) {
    const int cpt = vec ? 4 : 1, nx = tc / cpt, tb = BBT_PSRFITS_TILE / tc;
    return PsrFitsTile{tc, cpt, nx, BBT_PSRFITS_THREADS / nx, tb, tb / 2, tb / 2 + 1, tb + 1};
}

struct PsrFitsGeo {
    int tc;              // 32 or 4: with `vec`, the instantiation
    int vec;
    long long n_tile;    // tiles (workgroups) of a row
};

// 0, or what is wrong with the shape (a static string)
inline const char* psrfits_geo(long long n_bin, long long n_chan, long long n_pol, bool x_aligned16,
                               bool codes_aligned4, PsrFitsGeo* g) {
    if (n_bin < 1 || n_chan < 1 || n_pol < 1) return "an empty axis";
    if (n_chan >= (1ll << 31) || n_pol >= (1ll << 31) || n_chan * n_pol >= (1ll << 31) || n_bin >= (1ll << 31))
        return "an axis of 2^31 or more elements";
    const long long n_col = n_chan * n_pol;
    g->tc = n_col >= BBT_PSRFITS_WIDE ? 32 : 4;    // (few columns: narrow tiles, long along the bins)
    g->vec = x_aligned16 && codes_aligned4 && n_col % 4 == 0 && n_bin % 2 == 0;
    g->n_tile = (n_col + g->tc - 1) / g->tc;
    return 0;
}
