// Incoherent dedispersion over many trial DMs (DMTrials in search.py; the host twin is
// search.dm_trials_samples).  The reference has no such task: the rule is this package's.
//
//   out[i][d][r] = sum over c of in[i + offsets[d][c]][c][r]
//
// THE ARITHMETIC IS THE CONTRACT: one float32 accumulator per output element, started at +0, the
// channels added in ascending c, one rounded float32 add per channel.  There is no multiply to
// contract, no lane or workgroup shares a sum, and nothing about the launch enters a value; a NaN
// or Inf goes where its sweep takes it.
//
// The tiling is dmt_geo.hpp's.  k_dmt_transpose turns the channel-fastest chunk into scratch[e][t]
// (e = c * n_rest + r) so that the sweep reads along time; k_dmt_sweep gives a wave 64 consecutive
// times of DB consecutive trials: per channel one wave-uniform load of the DB offsets (the table is
// channel-major and its rows are padded, so the DB entries are adjacent and always there) and DB
// coalesced loads of 64 floats, each added to its own accumulator.  Adjacent trials read nearly the
// same floats of a row; that reuse is left to the vector cache.
//
// WHY NO READ LEAVES THE CHUNK.  The launcher only runs a table that dmt_check_table accepted --
// every offsets[d][c] in [0, span], and the padding entries are 0 -- on a chunk with n_in >= n_out
// + span (dmt_geo).  A wave that does anything has t0 < n_out (dmt_wave).  Its lanes read row e at
// t0 + lane' + offset with lane' = lane where t0 + lane < n_out and 0 otherwise (set once, ahead of
// the loop), so the time is at most n_out - 1 + span <= n_in - 1 and at least 0, and e = c * n_rest
// + r < nchan * n_rest rows of `pitch` >= n_in floats.  The transpose reads in[t][e] only for t <
// n_in and e < nchan * n_rest and writes scratch[e][t] for the same pairs.  Nothing is clamped
// inside a loop.
#pragma once
#include <hip/hip_runtime.h>

#include "dmt_geo.hpp"

namespace bbt {

// in[t][e], t < n_in, e < n_e  ->  scratch[e][t], rows `pitch` floats apart.  Grid (tr_t, tr_e).
__global__ __launch_bounds__(BBT_DMT_THREADS) void k_dmt_transpose(const float* __restrict__ in,
                                                                   float* __restrict__ scratch, long long n_in,
                                                                   int n_e, long long pitch) {
    constexpr int TR = BBT_DMT_TR;
    __shared__ float tile[TR][TR + 1];
    const int x = threadIdx.x % TR, y0 = threadIdx.x / TR;          // 64 x 4
    const long long t_base = (long long)blockIdx.x * TR;
    const int e_base = (int)blockIdx.y * TR;
    // rows of the tile are times, x runs along the elements (the input's fastest axis)
    for (int y = y0; y < TR; y += BBT_DMT_THREADS / TR) {
        const long long t = t_base + y;
        const int e = e_base + x;
        if (t < n_in && e < n_e) tile[y][x] = in[t * n_e + e];
    }
    __syncthreads();
    // and out: x runs along time (the scratch's fastest axis)
    for (int y = y0; y < TR; y += BBT_DMT_THREADS / TR) {
        const long long t = t_base + x;
        const int e = e_base + y;
        if (t < n_in && e < n_e) scratch[(long long)e * pitch + t] = tile[x][y];
    }
}

template <int DB>
__global__ __launch_bounds__(BBT_DMT_THREADS) void k_dmt_sweep(const float* __restrict__ scratch,
                                                               const int* __restrict__ tab,
                                                               float* __restrict__ out, DmtGeo g) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / BBT_DMT_WAVE));
    const unsigned lane = threadIdx.x % BBT_DMT_WAVE;
    DmtWave w;
    if (!dmt_wave(g, (long long)blockIdx.x, wave, &w)) return;       // (the whole wave; no barrier follows)
    const bool live = w.t0 + lane < g.n_out;
    const unsigned lt = live ? lane : 0u;                            // a time of this wave that is there
    const long long row_step = (long long)g.n_rest * g.pitch;        // from channel to channel
    const float* __restrict__ row = scratch + (long long)w.r * g.pitch + w.t0;
    const int* __restrict__ tb = tab + w.d0;
    float acc[DB];
#pragma unroll
    for (int k = 0; k < DB; ++k) acc[k] = 0.f;
    const int nchan = g.nchan;
#pragma unroll 4
    for (int c = 0; c < nchan; ++c) {
        int off[DB];
#pragma unroll
        for (int k = 0; k < DB; ++k) off[k] = tb[k];
        float x[DB];
#pragma unroll
        for (int k = 0; k < DB; ++k) x[k] = (row + off[k])[lt];
#pragma unroll
        for (int k = 0; k < DB; ++k) acc[k] = acc[k] + x[k];
        row += row_step;
        tb += g.ndm_pad;
    }
    if (!live) return;
    float* __restrict__ o = out + ((w.t0 + lane) * g.ndm + w.d0) * g.n_rest + w.r;
#pragma unroll
    for (int k = 0; k < DB; ++k)
        if (w.d0 + k < g.ndm) o[(long long)k * g.n_rest] = acc[k];
}

}  // namespace bbt
