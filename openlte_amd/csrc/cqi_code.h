// The (32, O) block code of CQI on PUSCH (36.212 table 5.2.2.6.4-1), shared by the host encoder and k_ulsch_cqi_decode (ulsch_cqi.hip).
// Column n as a word: bit i is M_{i,n}, so the code word of o_0 .. o_(O-1) is the XOR of the columns whose o_n is 1, and b_i is its bit i.
// Column 0 is all ones, columns 1 .. 5 take every 5-bit pattern once, columns 6 .. 10 are the masks.  tests/test_ulsch_cqi_cpu.py pins the
// weight distributions of the code, which a single wrong bit would break.
#pragma once
#include <cstdint>

#define MI_CQI_COL(n) ((n) == 0 ? 0xffffffffu : (n) == 1 ? 0x4ba5a933u : (n) == 2 ? 0x7d910e5au : (n) == 3 ? 0x6d26339cu : (n) == 4 ? 0x71c7c3e0u : \
                       (n) == 5 ? 0x7e0ffc00u : (n) == 6 ? 0x731d8e64u : (n) == 7 ? 0x6b44f5b0u : (n) == 8 ? 0x7dc218ecu : (n) == 9 ? 0x4da1b746u : 0x42f0ffffu)

constexpr uint32_t MI_CQI_BLOCK_MAX_BITS = 11;            // above: CRC8 and the tail-biting convolutional code
constexpr uint32_t MI_CQI_MAX_Q          = 6 * 12 * 1320; // the soft bits of the largest allocation (110 PRB, 64QAM); see ulsch_cqi.hip for the int32 sums

// the code word of the information bits w (o_n at bit n)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t mi_cqi_block_word(uint32_t w)
{
    uint32_t b = 0;
    for (uint32_t n = 0; n < MI_CQI_BLOCK_MAX_BITS; n++) b ^= ((w >> n) & 1u) ? MI_CQI_COL(n) : 0u;
    return b;
}
