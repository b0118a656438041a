// The (20, A) block code of CQI on PUCCH formats 2 / 2a / 2b (36.212 table 5.2.3.3-1), shared by the host encoder (pucch2_tx.cc) and
// k_pucch2_decode (pucch2.hip).  Stored like cqi_code.h: column n as a word, bit i is M_{i,n}, so the code word of a_0 .. a_(A-1) is the XOR
// of the columns whose a_n is 1, and b_i is its bit i.  Columns 0 .. 10 are the first 20 rows of the (32, O) code's table 5.2.2.6.4-1;
// columns 11 and 12 exist only here.  tests/test_pucch2_cpu.py pins the weight distributions of the code, which a single wrong bit would break.
#pragma once
#include <cstdint>

#include "cqi_code.h"

#define MI_PUCCH2_COL(n) ((n) <= 10 ? (MI_CQI_COL(n) & 0xFFFFFu) : (n) == 11 ? 0x33FFFu : 0x3FFFCu)

constexpr uint32_t MI_PUCCH2_MAX_BITS = 13; // A
constexpr uint32_t MI_PUCCH2_CODED    = 20; // B

// the code word of the information bits w (a_n at bit n)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t mi_pucch2_word(uint32_t w)
{
    uint32_t b = 0;
    for (uint32_t n = 0; n < MI_PUCCH2_MAX_BITS; n++) b ^= ((w >> n) & 1u) ? MI_PUCCH2_COL(n) : 0u;
    return b;
}
