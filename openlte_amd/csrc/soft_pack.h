// The packed hand-over of hard-decision soft bits between the PDSCH demodulator (chain.hip) and the turbo decoder's rate un-matching
// (turbo.hip).  In the reference-faithful de-mapper every 16QAM / 64QAM soft bit is +127 or -127, so an allocation of those travels as one
// BIT per soft bit instead of one byte:
//   soft bit n of the allocation = bit (n & 31) of little-endian dword (n >> 5) of the allocation's slot; set: -127, clear: +127;
//   the slot is the byte form's (e_base + e_off * 64, laid out for e_max BYTES), e_len still counts soft bits, and the bits at and above
//   e_len in the last dword are 0.  Nothing behind the last dword is written.
// What both sides rest on (chain.hip): bit k of the mask qam_neg_bits_nodiv returns -- the mask put_qam XORs with the scrambling bits -- is
// soft bit k of the symbol (qam_lut_entry expands bit k into byte k), and qam_lut_entry yields exactly 0x7F for a clear and 0x81 for a set
// bit, i.e. +-127: the expansion below reproduces the bytes put_qam stores.
// Pure functions on integers: compiles under a plain C++ compiler (tools/asan/soft_pack_driver.cc) and in the kernels alike.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SOFT_PACK_FN __host__ __device__ __forceinline__
#define SOFT_PACK_UNROLL _Pragma("unroll")
#else
#define SOFT_PACK_FN inline
#define SOFT_PACK_UNROLL
#endif

// four bits -> four bytes, bit k in byte k: clear 0x7F (+127), set 0x81 (-127).  The product copies bit k to bit 8k (k + 7k: no two terms meet,
// no carry), the mask keeps those, and 0x7F + 2 * bit stays inside its byte.
SOFT_PACK_FN uint32_t soft_expand4(uint32_t nib) { return (((nib & 15u) * 0x00204081u) & 0x01010101u) * 2u + 0x7F7F7F7Fu; }

// sixteen bits -> sixteen bytes (four little-endian words)
SOFT_PACK_FN void soft_expand16(uint32_t bits, uint32_t (&w)[4])
{
    SOFT_PACK_UNROLL
    for (int k = 0; k < 4; k++) w[k] = soft_expand4(bits >> (4 * k));
}

// the first `keep` (0..16) of sixteen bytes, the rest 0: the staged copy's rule for the quarter line that holds index E (see soft_stage_quad)
SOFT_PACK_FN void soft_keep_bytes(uint32_t (&w)[4], uint32_t keep)
{
    SOFT_PACK_UNROLL
    for (uint32_t k = 0; k < 4; k++) {
        const int kp = (int)keep - 4 * (int)k; // bytes of word k that are kept
        w[k] = kp >= 4 ? w[k] : kp <= 0 ? 0u : (w[k] & ((1u << (8 * kp)) - 1u));
    }
}

// Bytes 16 q .. 16 q + 15 of the allocation as the byte form holds them, read from the packed slot: the sixteen bits of half-dword q,
// expanded, and everything from byte `keep` on zeroed.  This is what the turbo prep kernel's staging writes to LDS per quarter line: the
// full lines with keep = 16, the line that holds index E (or a lap's end) with keep = E & 15 -- a zero at index E and up to the next
// 16-byte boundary, which is what the gathers read as "nothing" -- and, when E is a multiple of 16, a whole line of zeros without a read.
SOFT_PACK_FN void soft_stage_quad(const void *slot, uint32_t q, uint32_t keep, uint32_t (&w)[4])
{
    soft_expand16(((const uint16_t *)slot)[q], w);
    if (keep < 16) soft_keep_bytes(w, keep);
}

// Sixteen symbols' Q_m-bit masks (sixteen bytes as four little-endian words: what the demodulator keeps in LDS, one byte per symbol) ->
// 16 Q_m bits = QM / 2 dwords, symbol s at bits s Q_m .. s Q_m + Q_m - 1.  The masks of the symbols from n_valid on are taken as 0
// (the tail of an allocation: bits at and above e_len stay clear).  Sixteen symbols are a whole number of dwords for Q_m = 4 and 6, so
// every dword of an allocation comes from exactly one group of sixteen.
template <uint32_t QM> SOFT_PACK_FN void soft_pack16(const uint32_t (&m)[4], uint32_t n_valid, uint32_t (&out)[QM / 2])
{
    static_assert(QM == 4 || QM == 6, "16QAM or 64QAM");
    uint64_t lo = 0, hi = 0; // bits 0..63 and 64..127 of the group
    SOFT_PACK_UNROLL
    for (uint32_t s = 0; s < 16; s++) {
        const uint32_t p = s * QM;
        const uint64_t v = s < n_valid ? (uint64_t)((m[s >> 2] >> (8 * (s & 3))) & ((1u << QM) - 1u)) : 0u;
        if (p < 64) lo |= v << p;
        if (p < 64 && p + QM > 64) hi |= v >> (64 - p);
        if (p >= 64) hi |= v << (p - 64);
    }
    out[0] = (uint32_t)lo;
    out[1] = (uint32_t)(lo >> 32);
    if (QM == 6) out[QM / 2 - 1] = (uint32_t)hi;
}
