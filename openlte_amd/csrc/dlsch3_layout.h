// The slot layout of a plan's 3GPP transport-block part (dlsch3gpp.hip): which code-block slot holds which block of which allocation, where
// the slots' soft values and decoded bits lie, and the CRC24A weight of every block.  Pure host arithmetic -- no HIP, no context -- plus the
// GF(2) polynomial helpers the kernels share with it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mi_lte.h"
#include "turbo_plan.hpp" // MI_HD, MiKGroup

constexpr uint32_t G_CRC24A = 0x1864CFBu; // 36.212 5.1.1, x^24 included
constexpr uint32_t G_CRC24B = 0x1800063u;

// x * w mod g for a remainder w < 2^24
MI_HD inline uint32_t mulx(uint32_t w, uint32_t g) { w <<= 1; return (w & 0x1000000u) ? w ^ g : w; }
// a * b mod g (Horner over the bits of b)
MI_HD inline uint32_t mulmod(uint32_t a, uint32_t b, uint32_t g)
{
    uint32_t s = 0;
    for (int i = 23; i >= 0; i--) s = mulx(s, g) ^ (((b >> i) & 1u) ? a : 0u);
    return s;
}
// x^s mod g by squaring
inline uint32_t xpow(uint32_t s, uint32_t g)
{
    uint32_t r = 1, p = 2; // p = x^(2^i)
    for (; s; s >>= 1, p = mulmod(p, p, g))
        if (s & 1u) r = mulmod(r, p, g);
    return r;
}

// The static part of what the per-code-block kernels need (the rest is k_dl3_desc's): block r of C of allocation `alloc`, its size, xs =
// x^s mod gCRC24A with s = the transport-block bits behind the block's payload, and where its soft values (4-byte units) and bits (8-byte units) lie
struct Dl3Slot { uint32_t alloc, r, C, K, xs, soft_off4, bits_off8, pad; };

// Slots grouped by block size (ascending), inside a size allocation after allocation, block after block (mi_plan_group)
struct MiDlsch3Layout {
    std::vector<uint32_t> a_slot, a_nc, a_K, a_tbs; // per allocation: first slot, C, K, tbs
    std::vector<size_t>   a_soft;                   // per allocation: byte offset of its first block's soft values
    std::vector<MiKGroup> groups;                   // a block size's slots, contiguous; ...
    std::vector<size_t>   g_soft, g_bits;           // ... and where they start in the soft / bit arrays (bytes, on 256)
    std::vector<Dl3Slot>  slots;
    size_t                soft_bytes = 0, bits_bytes = 0; // 3 (K + 4) and K bytes per slot
};

// MI_LTE_OK; or mi_lte_dlsch_layout's code for the first allocation whose transport block is outside the mode, or MI_LTE_ERR_UNSUPPORTED for a
// plan whose offsets pass 32 bits, with *err (where given) the message.
int mi_dlsch3_layout(const mi_lte_dlsch_cfg *cfg, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, MiDlsch3Layout *out, const char **err);
