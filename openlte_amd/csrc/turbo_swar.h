// Byte-parallel ("SWAR") forms of the turbo decoder's soft re-encoder and of Steps 3, 10 and 11 (liblte_phy.cc:10113-10148, :10688-10707,
// :10778-10819): four trellis positions per 32-bit instruction, in SIGN-MAGNITUDE bytes.  Every quantity of those steps fits a byte
// (|x| <= 127, |a| + |b| <= 254), so nothing is widened to int16 before the two sums that really need nine bits (q(d0) + C1, D1 + D2),
// and those take their operands as biased bytes (128 + v, 128 - v), whose widening is a mask or a shift.
//
// A word holds positions 4j .. 4j+3, byte 0 first.  SM4::m are the magnitudes (bit 7 of every byte clear), SM4::s the sign bits (bit 7
// only).  A sign bit says "negative", and the reference counts 0 as positive: where a result's sign is read again, a magnitude of 0
// must come with a clear sign bit ("-0" must not leak), and the helpers below say which of them guarantee that.
//
// Compiles under hipcc (device code of turbo.hip) and under plain g++ (tools/asan/turbo_swar_driver.cc checks every helper against a
// scalar restatement of the reference's case ladders, exhaustively where the domain allows).
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define SWAR_FN __host__ __device__ __forceinline__
#else
#define SWAR_FN inline
#endif

namespace turbo_swar {

constexpr uint32_t HI = 0x80808080u, LO7 = 0x7F7F7F7Fu, ONES = 0x01010101u, EVEN = 0x00FF00FFu;

// low word of (hi:lo) >> sh, sh = 8 or 16: v_alignbit_b32 on the device
SWAR_FN uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
#endif
}
// a - b per 16-bit half
SWAR_FN uint32_t sub_halves(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short v2s_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(v2s_t, a) - __builtin_bit_cast(v2s_t, b));
#else
    return ((a - (b & 0xFFFFu)) & 0xFFFFu) | ((a & 0xFFFF0000u) - (b & 0xFFFF0000u));
#endif
}

struct SM4 { uint32_t m, s; };

// 0x7F in the bytes whose bit 7 is set in `bits` (a word of bit-7 flags): the select mask of a seven-bit value
SWAR_FN uint32_t low7(uint32_t bits) { return bits - (bits >> 7); }

// two's-complement bytes in [-127, 127] -> joined sign-magnitude bytes (sign in bit 7, magnitude below it): -b = (b ^ 0x7F) + 1 in the
// low seven bits, which neither reaches bit 7 (b != -128) nor leaves the byte.  The joined word is what is delayed; unjoin gives the two
// fields the arithmetic works on.
SWAR_FN uint32_t to_joined(uint32_t w)
{
    const uint32_t s = w & HI, t = s >> 7;
    return (w ^ (s - t)) + t;
}
// magnitudes (<= 127) and a mask with 0xFF in the negative bytes -> joined bytes, the sign bit cleared where the magnitude is 0: what
// the trellis kernels' traceback writes
SWAR_FN uint32_t joined_from(uint32_t m, uint32_t neg_mask) { return m | (neg_mask & (m + LO7) & HI); }
// the same from four sign BITS (bit i set: byte i is negative; bits 4 and up clear): what the trellis kernels' traceback writes now, one bit
// per step, and perm and vote expand.  The product puts bit i at bit 8i + 7; its other fifteen partial products land on distinct bits below
// bit 7 of some byte (14 21 28 | 8 22 29 | 9 16 30 | 10 17 24), so nothing carries and the mask removes them
SWAR_FN uint32_t joined_from_bits(uint32_t m, uint32_t nib) { return m | ((nib * 0x10204080u) & (m + LO7) & HI); }
// The sixteen sign bits of unit u (steps 16u .. 16u + 15, bit k = step 16u + k) behind the four of the steps before it (bits 0-3: the halo,
// whose joined form the re-encoder's delays need) out of the trellis kernels' sign words: c = the two words of the unit's 64-step block,
// prev_hi = the second word of the block before (read only where u % 4 == 0; the first unit's halo is the preset, not a sign)
SWAR_FN uint32_t unit_sign_bits(uint32_t c_lo, uint32_t c_hi, uint32_t prev_hi, uint32_t u)
{
    const uint32_t q = u & 3u;
    const uint64_t c = ((uint64_t)c_hi << 32) | c_lo;
    return q ? (uint32_t)(c >> (16u * q - 4u)) & 0xFFFFFu : (c_lo & 0xFFFFu) << 4 | prev_hi >> 28;
}
SWAR_FN SM4 unjoin(uint32_t j) { return SM4{j & LO7, j & HI}; }
SWAR_FN SM4 split(uint32_t w) { return unjoin(to_joined(w)); }
SWAR_FN uint32_t join(const SM4 &a) { return a.m | a.s; }
// ... and back.  Needs a clear sign bit where the magnitude is 0 (soft_xor's results have it; split's have it by construction).
SWAR_FN uint32_t to_tc(const SM4 &a)
{
    const uint32_t t = a.s >> 7;
    return ((a.m ^ (a.s - t)) + t) | a.s;
}

// 128 + (neg ? -x : x) per byte, x = seven-bit magnitudes, neg = bit-7 flags.  A magnitude 0 gives 128 whatever its flag says.
SWAR_FN uint32_t biased(uint32_t x, uint32_t neg)
{
    const uint32_t t = neg >> 7;
    return ((x ^ (neg - t)) + t) + (neg ^ HI);
}
// the even (0, 2) and odd (1, 3) bytes of a word as two unsigned 16-bit halves
SWAR_FN uint32_t even_halves(uint32_t w) { return w & EVEN; }
SWAR_FN uint32_t odd_halves(uint32_t w) { return (w >> 8) & EVEN; }

// sign * ((|a| + |b|) >> 1), the sign negative iff exactly one operand is negative: Step 3's four branches and conv_encode_soft's
// two-tap output in one form.  The sum of two magnitudes does not leave its byte; the shift brings the neighbour's low bit into bit 7,
// which the mask removes.  The result's sign bit is clear where its magnitude is 0.
SWAR_FN uint32_t half_sum(uint32_t ma, uint32_t mb) { return ((ma + mb) >> 1) & LO7; }
SWAR_FN SM4 soft_xor(const SM4 &a, const SM4 &b)
{
    const uint32_t m = half_sum(a.m, b.m);
    return SM4{m, (a.s ^ b.s) & (m + LO7) & HI};
}

// The delayed sequences of the re-encoder across (previous word, current word), as joined sign-magnitude words: x[k-2] and x[k-3] for
// the four positions k of `cur`.  The first unit of a block passes 0x7F7F7F7F as its previous word: conv_encode_soft presets its shift
// register to +127 (liblte_phy.cc:10097-10100).
SWAR_FN uint32_t delay2(uint32_t cur, uint32_t prev) { return alignbit(cur, prev, 16); }
SWAR_FN uint32_t delay3(uint32_t cur, uint32_t prev) { return alignbit(cur, prev, 8); }
// fb[k] = soft_xor(x[k-2], x[k-3]) (g = 03 re-encoder; fb[0] = 127 is the preset's own soft_xor(127, 127))
SWAR_FN SM4 feedback(uint32_t cur_joined, uint32_t prev_joined)
{
    const uint32_t d2 = delay2(cur_joined, prev_joined), d3 = delay3(cur_joined, prev_joined);
    const uint32_t x = d2 ^ d3; // bit 7: the signs' difference; a + b = 2 (a & b) + (a ^ b) on the magnitudes
    const uint32_t m = (d2 & d3 & LO7) + ((x >> 1) & 0x3F3F3F3Fu);
    return SM4{m, x & (m + LO7) & HI};
}

// Step 3: C1 = soft_xor(A, fb(A)), as sign-magnitude (to_tc gives the bytes pass 3 reads) ...
SWAR_FN SM4 step3(const SM4 &A, const SM4 &F) { return soft_xor(A, F); }
// ... and as 128 - C1, the subtrahend of q(d0) + C1 = (128 + q(d0)) - (128 - C1) in 16-bit halves.  (No "-0" care: 128 - 0 either way.)
SWAR_FN uint32_t step3_neg_biased(const SM4 &A, const SM4 &F) { return biased(half_sum(A.m, F.m), A.s ^ F.s ^ HI); }

// 128 + floor((x + y) / 2) per byte from xb = 128 + x, yb = 128 + y: the overflow-free average of unsigned bytes
SWAR_FN uint32_t avg_biased(uint32_t xb, uint32_t yb) { return (xb & yb) + (((xb ^ yb) >> 1) & LO7); }

// Step 10: int_calc_1 from B = int_act_1, G = fb_int_1 and -- in the two mixed-sign branches, which read in_act_1 where Step 11 reads
// its own input (liblte_phy.cc:10791, :10794) -- A = in_act_1:
//   equal signs of B and G   (|B| + |G|) >> 1
//   mixed signs              -((|G| + |A|) >> 1) where A and B have equal sign bits, -((|G| - |A|) >> 1) (floor) where they differ
// G's sign bit must be clear where G is 0 (feedback's is).  Returns 128 + v.
SWAR_FN uint32_t step10_biased(const SM4 &A, const SM4 &B, const SM4 &G)
{
    const uint32_t mx = B.s ^ G.s, tm = mx >> 7, m7 = mx - tm;
    const uint32_t y  = (A.m & m7) | (B.m & ~m7);                          // what is averaged with |G|
    const uint32_t w  = avg_biased(G.m | HI, biased(y, mx & (A.s ^ B.s))); // 128 + floor((|G| +- y) / 2)
    return (w ^ (m7 | mx)) + tm;                                           // mixed signs: 256 - w = 128 - floor(..)
}
// Step 11: int_calc_2 from B = int_act_2, G = fb_int_2:
//   equal signs   (|B| + |G|) >> 1
//   mixed signs   -((|B| + |G|) >> 1) for B >= 0, -((|B| - |G|) >> 1) (floor) for B < 0
// Returns 128 - v, so that D1 + D2 = step10_biased - step11_neg_biased in 16-bit halves.
SWAR_FN uint32_t step11_neg_biased(const SM4 &B, const SM4 &G)
{
    const uint32_t mx = B.s ^ G.s, tm = mx >> 7, m7 = mx - tm;
    const uint32_t w  = avg_biased(B.m | HI, biased(G.m, mx & B.s)); // 128 + floor((|B| +- |G|) / 2)
    return (w ^ ~(m7 | mx)) + (tm ^ ONES);                           // equal signs: 256 - w
}

// One entry of the trellis kernels' traceback table: two steps of the reference's traceback (liblte_phy.cc:10483-10527) from state `cur`,
// `byte` = the stored compare bits of the two steps, the step traced first (the later one) in the low nibble.  Bits 0-2: the state after
// both; bit 31: the first-traced step's output is negative, bit 30: the second's -- alignbit(acc, entry, 30) appends them to a sign word
// in step order.
SWAR_FN uint32_t traceback_entry(uint32_t byte, uint32_t cur)
{
    uint32_t sgn = 0;
    for (int k = 0; k < 2; k++) {
        const uint32_t nib = k ? byte >> 4 : byte & 15u;
        const uint32_t j = cur & 3u, bit = (nib >> (3 - j)) & 1u, st = 2 * j + bit; // pair j is bit (3-j) of the nibble
        const bool     pos = (cur < st) || (cur == st && cur == 0); // "+" when the step moved to a lower state, or stayed in state 0
        if (!pos) sgn |= k ? 1u << 30 : 1u << 31;
        cur = st;
    }
    return cur | sgn;
}

} // namespace turbo_swar
