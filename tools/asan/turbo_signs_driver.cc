// tools/asan/turbo_signs_driver.cc: the sign-bit interface between the trellis kernels and perm / vote (openlte_amd/csrc/turbo_swar.h:
// joined_from_bits, unit_sign_bits, traceback_entry), built with g++ -fsanitize=address,undefined (run_turbo_signs.sh).  CPU only.
//   1. joined_from_bits(m, nibble) == joined_from(m, byte mask): every nibble x every byte position x all 128 magnitudes with random other
//      bytes, a million random words, magnitude 0 under a set sign bit
//   2. the sign bits of all 2048 traceback table entries == the byte masks of the entry function they replace (restated below)
//   3. a 64-step block packed the way k_turbo_siso's traceback packs it (two steps per table entry, v_alignbit into two words) and expanded the
//      way perm and vote expand it (unit_sign_bits, joined_from_bits, halo from the block before) == the step-by-step traceback's signed bytes;
//      full blocks, last blocks of 8, 40 and 56 valid steps
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../openlte_amd/csrc/turbo_swar.h"

namespace sw = turbo_swar;

static long n_checked = 0, n_bad = 0;
#define CHECK_EQ(a, b, ...)                                                                   \
    do {                                                                                      \
        n_checked++;                                                                          \
        if ((a) != (b)) {                                                                     \
            if (n_bad++ < 20) { printf("MISMATCH %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                     \
    } while (0)

// the entry function this format replaces: state after two steps | byte masks (0xFF = negative) of the two outputs in bits 8-23, the first
// step's in the upper byte
static uint32_t traceback_entry_masks(uint32_t byte, uint32_t cur)
{
    uint32_t mask = 0;
    for (int k = 0; k < 2; k++) {
        const uint32_t nib = k ? byte >> 4 : byte & 15u;
        const uint32_t j = cur & 3u, bit = (nib >> (3 - j)) & 1u, st = 2 * j + bit;
        const bool     pos = (cur < st) || (cur == st && cur == 0);
        if (!pos) mask |= k ? 0x00FFu : 0xFF00u;
        cur = st;
    }
    return cur | mask << 8;
}

static uint32_t mask_of_nibble(uint32_t nib)
{
    uint32_t m = 0;
    for (int i = 0; i < 4; i++)
        if (nib >> i & 1u) m |= 0xFFu << (8 * i);
    return m;
}

// one step of the reference's traceback (liblte_phy.cc:10483-10527): the four compare bits of the step (pair j in bit 3 - j) and the state
// after it -> the state before it, and whether the step's output is negative
static bool step_back(uint32_t nib, uint32_t &cur)
{
    const uint32_t j = cur & 3u, st = 2 * j + ((nib >> (3 - j)) & 1u);
    const bool     pos = (cur < st) || (cur == st && cur == 0);
    cur = st;
    return !pos;
}

int main()
{
    std::mt19937 rng(20240611);
    // ---- 1
    for (uint32_t nib = 0; nib < 16; nib++)
        for (int pos = 0; pos < 4; pos++)
            for (uint32_t mag = 0; mag < 128; mag++) {
                const uint32_t m = ((rng() & sw::LO7) & ~(0xFFu << (8 * pos))) | mag << (8 * pos);
                CHECK_EQ(sw::joined_from_bits(m, nib), sw::joined_from(m, mask_of_nibble(nib)), "nibble %u byte %d magnitude %u (m = %08x)", nib, pos, mag, m);
            }
    for (int i = 0; i < 1000000; i++) {
        const uint32_t m = rng() & sw::LO7, nib = rng() & 15u;
        CHECK_EQ(sw::joined_from_bits(m, nib), sw::joined_from(m, mask_of_nibble(nib)), "random m = %08x nibble %u", m, nib);
    }
    for (uint32_t z = 0; z < 16; z++) { // zero magnitudes in the bytes of z, all four signs set: the sign bit stays clear exactly there
        uint32_t m = 0x7F013440u;
        for (int i = 0; i < 4; i++)
            if (z >> i & 1u) m &= ~(0xFFu << (8 * i));
        const uint32_t j = sw::joined_from_bits(m, 15u);
        for (int i = 0; i < 4; i++) CHECK_EQ((j >> (8 * i + 7)) & 1u, (z >> i & 1u) ? 0u : 1u, "magnitude 0 under a set sign bit: zero set %u byte %d", z, i);
        CHECK_EQ(j & sw::LO7, m, "magnitudes kept, zero set %u", z);
    }
    // ---- 2
    for (uint32_t i = 0; i < 2048; i++) {
        const uint32_t e = sw::traceback_entry(i >> 3, i & 7u), o = traceback_entry_masks(i >> 3, i & 7u);
        CHECK_EQ(e & 7u, o & 7u, "entry %u: state", i);
        CHECK_EQ(e >> 31, (o >> 16) & 1u, "entry %u: first step's sign", i);
        CHECK_EQ((e >> 30) & 1u, (o >> 8) & 1u, "entry %u: second step's sign", i);
        CHECK_EQ(e & 0x3FFFFFF8u, 0u, "entry %u: nothing else set", i);
        CHECK_EQ(((o >> 8) & 0xFFFFu), (uint32_t)((e >> 31 ? 0xFF00u : 0u) | ((e >> 30) & 1u ? 0x00FFu : 0u)), "entry %u: whole bytes", i);
    }
    // ---- 3: two blocks (the second one's first unit takes its halo from the first), the second with n_valid steps
    const int valid[] = {64, 8, 40, 56};
    for (int rep = 0; rep < 4000; rep++) {
        const int K = 64 + valid[rep & 3];
        std::vector<uint8_t> nib(128), mag(128);
        for (int t = 0; t < 128; t++) {
            nib[t] = rng() & 15u;
            const uint32_t r = rng();
            mag[t] = (r & 0x300u) == 0 ? 0 : (r & 0x400u) ? 127 : r & 0x7Fu; // a quarter zeros: "-0" must not appear
        }
        const uint32_t end = rng() & 7u;
        // the reference: step by step from the last step down
        std::vector<uint8_t> want(128, 0);
        uint32_t cur = end;
        for (int t = K - 1; t >= 0; t--) {
            const bool neg = step_back(nib[t], cur);
            want[t] = (neg && mag[t]) ? mag[t] | 0x80u : mag[t];
        }
        // the kernel: the decision word of eight steps has step r in nibble 7 - r, byte b = steps 7 - 2b (low nibble) and 6 - 2b
        uint32_t words[2][2];
        cur = end;
        for (int blk = 1; blk >= 0; blk--) {
            uint32_t sb[2] = {0, 0};
            for (int g = 7; g >= 0; g--) {
                if (blk * 64 + g * 8 >= K) continue;
                uint32_t word = 0;
                for (int r = 0; r < 8; r++) word |= (uint32_t)nib[blk * 64 + g * 8 + r] << (4 * (7 - r));
                for (int b = 0; b < 4; b++) {
                    const uint32_t e = sw::traceback_entry((word >> (8 * b)) & 0xFFu, cur);
                    cur = e & 7u;
                    sb[g >> 2] = sw::alignbit(sb[g >> 2], e, 30);
                }
            }
            words[blk][0] = sb[0]; words[blk][1] = sb[1];
        }
        // perm / vote: unit u of the 8, its magnitude words and the halo word
        for (uint32_t u = 0; u < 8; u++) {
            const uint32_t blk = u >> 2;
            const uint32_t b = sw::unit_sign_bits(words[blk][0], words[blk][1], (u & 3u) == 0 && u > 0 ? words[blk - 1][1] : 0xDEADBEEFu, u);
            CHECK_EQ(b >> 20, 0u, "unit %u: twenty bits", u);
            for (int j = (u > 0 ? -1 : 0); j < 4; j++) {
                uint32_t m = 0, w = 0;
                for (int i = 0; i < 4; i++) { m |= (uint32_t)mag[16 * u + 4 * j + i] << (8 * i); w |= (uint32_t)want[16 * u + 4 * j + i] << (8 * i); }
                int       nv = K - (int)(16 * u + 4 * j); // valid steps of the word: the kernels zero what lies past the block end
                uint32_t  keep = nv >= 4 ? 0xFFFFFFFFu : 0u;
                if (nv > 0 && nv < 4) { printf("MISMATCH: K %% 4 != 0\n"); return 1; }
                const uint32_t got = sw::joined_from_bits(m, (b >> (4 * j + 4)) & 15u);
                if (keep) CHECK_EQ(got, w, "rep %d K %d unit %u word %d: got %08x want %08x", rep, K, u, j, got, w);
                else      CHECK_EQ(got, m, "rep %d K %d unit %u word %d past the end: no sign may be set (%08x, m = %08x)", rep, K, u, j, got, m);
            }
        }
    }
    printf("turbo signs driver: %ld checks, %ld mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
