// The search-space arithmetic of 36.213 9.1.1 that mi_lte_pdcch_search_space (dci.cc, host) and the search kernels (pdcch.hip, device) share.
// Device code: a .hpp, so the build id covers it.  Under a plain C++ compiler the functions are ordinary inline ones (soft_pack.h's pattern).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PDCCH_SEARCH_FN __host__ __device__ inline
#else
#define PDCCH_SEARCH_FN inline
#endif

// Y_k for k = sf, from Y_(-1) = rnti; and the number of candidates of an aggregation level
PDCCH_SEARCH_FN uint32_t search_space_y(uint32_t rnti, uint32_t sf)
{
    uint32_t y = rnti;
    for (uint32_t k = 0; k <= sf; k++) y = (39827u * y) % 65537u; // (y <= 65536: the product stays below 2^32)
    return y;
}
PDCCH_SEARCH_FN uint32_t search_space_m(uint32_t L) { return L <= 2 ? 6u : 2u; }

// the candidates of n_cce CCEs in reporting order: every L = 8, 4, 2, 1 in turn, first CCEs ascending
PDCCH_SEARCH_FN uint32_t search_n_cand(uint32_t n_cce) { return (n_cce >> 3) + (n_cce >> 2) + (n_cce >> 1) + n_cce; }
PDCCH_SEARCH_FN void search_cand(uint32_t n_cce, uint32_t cand, uint32_t &L, uint32_t &cce)
{
    const uint32_t n8 = n_cce >> 3, n4 = n_cce >> 2, n2 = n_cce >> 1;
    if (cand < n8) { L = 8; cce = 8 * cand; }
    else if (cand < n8 + n4) { L = 4; cce = 4 * (cand - n8); }
    else if (cand < n8 + n4 + n2) { L = 2; cce = 2 * (cand - n8 - n4); }
    else { L = 1; cce = cand - n8 - n4 - n2; }
}
