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

#include <cstddef>
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
// magnitudes (<= 127) and a mask with 0xFF in the negative bytes -> joined bytes, the sign bit cleared where the magnitude is 0: the
// byte form of what the sign words below carry
SWAR_FN uint32_t joined_from(uint32_t m, uint32_t neg_mask) { return m | (neg_mask & (m + LO7) & HI); }

// ---- The trellis kernels' sign words (turbo.hip: SisoPass::sgn): the one definition of their layout.
// One bit per trellis step, set where the path's output is negative (whatever its magnitude), 0 for a step past the block end.
//   * Per code block, contiguous: [tile][lane][word], word = step t >> 5, 2 * nblk words per lane (nblk = kpad64(K) >> 6 blocks of 64 steps).
//     A tile takes nblk * 64 * 2 words: sign_word_index() from the tile's base, which is the magnitude arrays' tile offset >> 5.
//   * By plane inside a word: word S covers steps 32 s .. 32 s + 31, and step 32 s + 4 w + b (w = 0..7: the group of four steps that is one
//     byte word of the magnitude arrays, b = 0..3: the byte in it) is bit 8 b + w (sign_plane_bit).  The bit-7 flags of magnitude word
//     g = t / 4 are then ((S[g >> 3] >> (g & 7)) & ONES) << 7: a shift and a mask (sign_flags).
//   * A unit's halo (steps 16 u - 4 .. 16 u - 1: magnitude word 4 u - 1) is in the unit's own sign word for odd u and in the word before
//     it for even u > 0; the first unit's halo is the re-encoder's preset, not a sign.
SWAR_FN uint32_t sign_plane_bit(uint32_t t) { return 8u * (t & 3u) + ((t >> 2) & 7u); }  // step t % 32 -> its bit
SWAR_FN uint32_t sign_plane_step(uint32_t p) { return 4u * (p & 7u) + ((p >> 3) & 3u); } // bit p -> its step % 32 (the inverse)
SWAR_FN size_t   sign_word_index(uint32_t lane, uint32_t nblk, uint32_t word) { return (size_t)lane * 2u * nblk + word; }
SWAR_FN uint32_t sign_flags(uint32_t S, uint32_t g) { return ((S >> (g & 7u)) & ONES) << 7; }
// The expansion perm and vote run per unit: x = sign_unit(S, u) once, then word j = 0..3 of the unit takes its flags with one shift and
// the mask that also removes "-0": signed_under(m, x, j) = the sign bits of the bytes of m (magnitudes, bit 7 clear) that are negative
// and not 0 -- SM4{m, that} is the word split, m | that the joined word.  signed_under_flags is the same from bit-7 flags (the halo).
SWAR_FN uint32_t sign_unit(uint32_t S, uint32_t u) { return S >> (4u * (u & 1u)); }
SWAR_FN uint32_t signed_under_flags(uint32_t m, uint32_t flags) { return flags & (m + LO7) & HI; }
SWAR_FN uint32_t signed_under(uint32_t m, uint32_t x, int j) { return signed_under_flags(m, x << (7 - j)); }
// the flags of a unit's halo word: bit 3 of every plane of its own word (odd u), bit 7 of the word before (even u > 0)
SWAR_FN uint32_t sign_halo(uint32_t S, uint32_t S_before, uint32_t u) { return (u & 1u) ? S << 4 : S_before; }
// Packing, the lock-step kernel's way: traceback_entry (below) carries the signs of its two steps -- steps 4 w + b of one w, b = (3, 2) or
// (1, 0) -- in bits 24 and 16, eight apart like their planes.  A 32-step word is traced back from w = 7 down to 0, so one accumulator per
// byte pair takes its eight entries by (acc << 1) | entry: the planes end in bits 16-31 (the entries' state bits stay below bit 10), and
// the two accumulators are joined once per word.
SWAR_FN uint32_t sign_acc_push(uint32_t acc, uint32_t entry) { return (acc << 1) | entry; }
SWAR_FN uint32_t sign_word_join(uint32_t acc32, uint32_t acc10)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(acc32, acc10, 0x07060302u);
#else
    return (acc32 & 0xFFFF0000u) | (acc10 >> 16);
#endif
}
// ... and the state-parallel kernel's way: from the 64 signs of a block in step order (a ballot, lanes = steps): bit p of word h is step
// 32 h + sign_plane_step(p).  On the device lane L fetches the flag of lane sign_plane_lane(L) and the ballot is taken again.
SWAR_FN uint32_t sign_plane_lane(uint32_t L) { return (L & 32u) | sign_plane_step(L & 31u); }
SWAR_FN uint32_t sign_word_from_steps(uint64_t steps, uint32_t h)
{
    uint32_t S = 0;
    for (uint32_t p = 0; p < 32; p++) S |= (uint32_t)((steps >> sign_plane_lane(32u * h + p)) & 1u) << p;
    return S;
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
// both; bit 24: the first-traced step's output is negative, bit 16: the second's -- sign_acc_push appends them to the two planes of a
// sign word's byte pair.
SWAR_FN uint32_t traceback_entry(uint32_t byte, uint32_t cur)
{
    uint32_t sgn = 0;
    for (int k = 0; k < 2; k++) {
        const uint32_t nib = k ? byte >> 4 : byte & 15u;
        const uint32_t j = cur & 3u, bit = (nib >> (3 - j)) & 1u, st = 2 * j + bit; // pair j is bit (3-j) of the nibble
        const bool     pos = (cur < st) || (cur == st && cur == 0); // "+" when the step moved to a lower state, or stayed in state 0
        if (!pos) sgn |= k ? 1u << 16 : 1u << 24;
        cur = st;
    }
    return cur | sgn;
}

} // namespace turbo_swar
