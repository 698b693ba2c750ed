// Limits and stage list of the general LDS Stockham transform (fft_generic.hpp), shared by the
// kernels and by the host rules that plan for them (gen_host.hpp).  Plain C++ (no device code).
#pragma once

namespace bbt {

#define BBT_GEN_MAX_FACTORS 24
#define BBT_GEN_MAX_LEN 8192          // elements of one LDS tile (n * ct)
#ifndef BBT_GEN_EPT
#define BBT_GEN_EPT 8                 // tile elements per thread
#endif
#define BBT_GEN_MAX_THREADS (BBT_GEN_MAX_LEN / BBT_GEN_EPT)
#ifndef BBT_GEN_MAXR
#define BBT_GEN_MAXR 12               // largest radix of a stage (14 .. 16: spilled registers; measured 5 % slower)
#endif
struct GenGeo {
    int n;                            // transform length
    int nfac;                         // number of stages
    int fac[BBT_GEN_MAX_FACTORS];     // radices in {2..10, 12, 14, 15, 16}, product n
    int woff[BBT_GEN_MAX_FACTORS];    // where stage s finds its twiddles in the table (host: get_gen_table)
};

}  // namespace bbt
