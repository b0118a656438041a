// The PDSCH demodulators' scrambling words (chain.hip: k_pdsch_demod, k_pdsch_demod_llr): runs of consecutive words of the Gold sequence
// of 36.211 7.2 by recurrence.  gold_word (phy_dev.hpp) pays one batch of eight table loads per eight set bits of c_init for EVERY word;
// the sequence is linear, so after one such jump per lane the following words come from a word-wise step of the two shift registers, a
// dozen integer instructions each.  Words are LSB-first: bit n & 31 of word n >> 5.
// Only chain.hip includes this file (and it is no part of the shared-header build id: the other files' kernels are not touched by it).
#pragma once
#include "phy_dev.hpp"

namespace {

// x1(n + 31) = x1(n + 3) ^ x1(n): bits n0 + 32 .. n0 + 63 from bits n0 .. n0 + 31.  Bit k of the next word is W[k + 1] ^ W[k + 4] while both lie in
// W (k <= 27); above, the missing terms are the next word's own bits 0 .. 3 (L), which the first line has already formed.
__device__ __forceinline__ uint32_t gold_step_x1(uint32_t W)
{
    const uint32_t T = (W >> 1) ^ (W >> 4), L = T & 15u;
    return T ^ ((L & 1u) << 31) ^ (L << 28);
}
// x2(n + 31) = x2(n + 3) ^ x2(n + 2) ^ x2(n + 1) ^ x2(n), the same way
__device__ __forceinline__ uint32_t gold_step_x2(uint32_t W)
{
    const uint32_t T = (W >> 1) ^ (W >> 2) ^ (W >> 3) ^ (W >> 4), L = T & 15u;
    return T ^ (L << 28) ^ (L << 29) ^ (L << 30) ^ (L << 31);
}

// word w of x2 for c_init: gold_word's basis-table loop without the x1 term (the loads eight at a time, as there)
__device__ __forceinline__ uint32_t gold_x2_word(const GoldTables &gt, uint32_t c_init, uint32_t w)
{
    uint32_t v = 0, m = c_init;
    while (m) {
        uint32_t t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool     on = m != 0;
            const uint32_t b  = on ? (uint32_t)__builtin_ctz(m) : 0u;
            t[k] = gt.x2b[__umul24(b, gt.words) + w];
            t[k] = on ? t[k] : 0u;
            m &= m - 1;
        }
        v ^= (t[0] ^ t[1]) ^ (t[2] ^ t[3]) ^ (t[4] ^ t[5]) ^ (t[6] ^ t[7]);
    }
    return v;
}

// cw[0 .. n_words_ub] (inclusive) = the scrambling words of c_init, filled by n_lanes threads of which this one is `lane`: a thread takes runs
// of R consecutive words, w0 = R * lane, R * (lane + n_lanes), ...: both registers' words at w0 from the tables, the rest of the run stepped.
// table: the method before this one instead, gold_word per word (the A/B switch: mi_lte_set_gold_recurrence).
template <uint32_t R>
__device__ __forceinline__ void gold_fill_words(uint32_t *cw, const GoldTables &gt, uint32_t c_init, uint32_t n_words_ub, uint32_t lane, uint32_t n_lanes,
                                                bool table)
{
    if (table) {
        for (uint32_t w = lane; w <= n_words_ub; w += n_lanes) cw[w] = gold_word(gt, c_init, w);
        return;
    }
    for (uint32_t w0 = R * lane; w0 <= n_words_ub; w0 += R * n_lanes) {
        uint32_t x1 = gt.x1[w0], x2 = gold_x2_word(gt, c_init, w0);
#pragma unroll
        for (uint32_t k = 0; k < R; k++) {
            if (w0 + k <= n_words_ub) cw[w0 + k] = x1 ^ x2;
            x1 = gold_step_x1(x1);
            x2 = gold_step_x2(x2);
        }
    }
}

} // namespace
