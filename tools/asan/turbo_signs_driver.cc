// tools/asan/turbo_signs_driver.cc: the sign-bit interface between the trellis kernels and perm / vote (openlte_amd/csrc/turbo_swar.h, "the trellis
// kernels' sign words": sign_plane_bit, sign_flags, signed_under, sign_acc_push / sign_word_join, sign_word_from_steps, traceback_entry), built with
// g++ -fsanitize=address,undefined (run_turbo_signs.sh).  CPU only.
//   1. m | signed_under(m, flags of word g out of a sign word) == joined_from(m, byte mask): every nibble x every byte position x all 128
//      magnitudes with random other bytes and bits, a million random words, magnitude 0 under a set sign bit
//   2. the sign bits of all 2048 traceback table entries == the byte masks of the entry function they replace (restated below)
//   3. code blocks of two 64-step blocks packed the way k_turbo_siso's traceback packs them (two steps per table entry, one accumulator per byte
//      pair, joined per word, stored at [lane][word]) and expanded the way perm and vote expand them (load_unit_signed restated: one sign word,
//      the word before it for an even unit's halo) == the step-by-step traceback's signed bytes; full blocks, last blocks of 8, 40 and 56 steps
//   4. the layout itself ("sign planes"): the bit map is a permutation of the 32 positions and is the definition (step 4 w + b -> bit 8 b + w);
//      packing the lock-step way == packing the state-parallel kernel's way (a step-ordered 64-bit mask) for 100 000 random masks; and part 3's
//      expansion counted per unit position u % 4, with the halo across a word (u = 2, 6) and across a block (u = 4), the first unit's preset
//      and the magnitudes 0 under a set sign bit it met
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

// a block of 64 signs (bit t: step t negative) packed the lock-step kernel's way: traced back from step 63 down, two steps per table entry
// (the entry's signs in bits 24 and 16, a random state below them), one accumulator per byte pair, joined per word
static void pack_lockstep(uint64_t steps, std::mt19937 &rng, uint32_t out[2])
{
    for (int h = 1; h >= 0; h--) {
        uint32_t acc[2] = {0, 0};
        for (int w = 7; w >= 0; w--)
            for (int b = 0; b < 2; b++) { // entry b = 0: steps 4 w + 3 (traced first) and 4 w + 2; b = 1: steps 4 w + 1 and 4 w
                const int      t = 32 * h + 4 * w + (b ? 1 : 3);
                const uint32_t e = (rng() & 7u) | (uint32_t)((steps >> t) & 1u) << 24 | (uint32_t)((steps >> (t - 1)) & 1u) << 16;
                acc[b] = sw::sign_acc_push(acc[b], e);
            }
        out[h] = sw::sign_word_join(acc[0], acc[1]);
    }
}

// perm's / vote's load_unit_signed (turbo.hip) on host arrays: the unit's halo word and four words, joined, and the four words' sign fields
struct UnitSigned { uint32_t w[5], s[4]; };
static UnitSigned load_unit_signed(const std::vector<uint8_t> &mag, const std::vector<uint32_t> &sgn, uint32_t lane, uint32_t nblk, uint32_t u)
{
    UnitSigned r;
    auto word = [&](int g) { uint32_t m = 0; for (int i = 0; i < 4; i++) m |= (uint32_t)mag.at(4 * g + i) << (8 * i); return m; };
    r.w[0] = u > 0 ? word(4 * u - 1) : 0x7F7F7F7Fu;
    for (int j = 0; j < 4; j++) r.w[j + 1] = word(4 * u + j);
    const size_t   at = sw::sign_word_index(lane, nblk, u >> 1);
    const uint32_t S = sgn.at(at);
    uint32_t       Sb = 0;
    if ((u & 1u) == 0 && u > 0) Sb = sgn.at(at - 1);
    if (u > 0) r.w[0] |= sw::signed_under_flags(r.w[0], sw::sign_halo(S, Sb, u));
    const uint32_t x = sw::sign_unit(S, u);
    for (int j = 0; j < 4; j++) {
        r.s[j] = sw::signed_under(r.w[j + 1], x, j);
        r.w[j + 1] |= r.s[j];
    }
    return r;
}

int main()
{
    std::mt19937 rng(20240611);
    // ---- 1: the four flags of magnitude word g out of a sign word whose other bits are random
    auto sign_word_with = [&](uint32_t nib, uint32_t g) {
        uint32_t S = rng();
        for (uint32_t b = 0; b < 4; b++) S = (S & ~(1u << (8 * b + g))) | ((nib >> b) & 1u) << (8 * b + g);
        return S;
    };
    auto expand = [&](uint32_t m, uint32_t S, uint32_t g) { return m | sw::signed_under(m, sw::sign_unit(S, g >> 2), (int)(g & 3u)); }; // unit parity g >> 2, word g & 3
    for (uint32_t nib = 0; nib < 16; nib++)
        for (int pos = 0; pos < 4; pos++)
            for (uint32_t mag = 0; mag < 128; mag++) {
                const uint32_t m = ((rng() & sw::LO7) & ~(0xFFu << (8 * pos))) | mag << (8 * pos), g = rng() & 7u, S = sign_word_with(nib, g);
                CHECK_EQ(expand(m, S, g), sw::joined_from(m, mask_of_nibble(nib)), "nibble %u byte %d magnitude %u (m = %08x, word %u of %08x)", nib, pos, mag, m, g, S);
            }
    for (int i = 0; i < 1000000; i++) {
        const uint32_t m = rng() & sw::LO7, nib = rng() & 15u, g = rng() & 7u, S = sign_word_with(nib, g);
        CHECK_EQ(expand(m, S, g), sw::joined_from(m, mask_of_nibble(nib)), "random m = %08x nibble %u word %u of %08x", m, nib, g, S);
        if ((i & 15) == 0) CHECK_EQ(m | sw::signed_under_flags(m, sw::sign_flags(S, g)), sw::joined_from(m, mask_of_nibble(nib)), "sign_flags: m = %08x nibble %u word %u", m, nib, g);
    }
    for (uint32_t z = 0; z < 16; z++) { // zero magnitudes in the bytes of z, all four signs set: the sign bit stays clear exactly there
        uint32_t m = 0x7F013440u;
        for (int i = 0; i < 4; i++)
            if (z >> i & 1u) m &= ~(0xFFu << (8 * i));
        const uint32_t g = z & 7u, j = expand(m, sign_word_with(15u, g), g);
        for (int i = 0; i < 4; i++) CHECK_EQ((j >> (8 * i + 7)) & 1u, (z >> i & 1u) ? 0u : 1u, "magnitude 0 under a set sign bit: zero set %u byte %d", z, i);
        CHECK_EQ(j & sw::LO7, m, "magnitudes kept, zero set %u", z);
    }
    // ---- 2
    for (uint32_t i = 0; i < 2048; i++) {
        const uint32_t e = sw::traceback_entry(i >> 3, i & 7u), o = traceback_entry_masks(i >> 3, i & 7u);
        CHECK_EQ(e & 7u, o & 7u, "entry %u: state", i);
        CHECK_EQ((e >> 24) & 1u, (o >> 16) & 1u, "entry %u: first step's sign", i);
        CHECK_EQ((e >> 16) & 1u, (o >> 8) & 1u, "entry %u: second step's sign", i);
        CHECK_EQ(e & ~0x01010007u, 0u, "entry %u: nothing else set", i);
        CHECK_EQ(((o >> 8) & 0xFFFFu), (uint32_t)(((e >> 24) & 1u ? 0xFF00u : 0u) | ((e >> 16) & 1u ? 0x00FFu : 0u)), "entry %u: whole bytes", i);
    }
    // ---- 3: code blocks of two 64-step blocks (the second one's first unit takes its halo from the first), the second with n_valid steps,
    // on lanes 0, 1 and 63 of a tile's sign words (the neighbours' words are poisoned: an expansion that strays reads a wrong sign)
    const int valid[] = {64, 8, 40, 56};
    long n_unit[4] = {0, 0, 0, 0}, n_halo_word = 0, n_halo_block = 0, n_preset = 0, n_zero_under_sign = 0;
    for (int rep = 0; rep < 4000; rep++) {
        const int K = 64 + valid[rep & 3];
        const uint32_t nblk = 2, lane = (rep >> 2) % 3 == 0 ? 0u : (rep >> 2) % 3 == 1 ? 1u : 63u;
        std::vector<uint8_t> nib(128), mag(128);
        for (int t = 0; t < 128; t++) {
            nib[t] = rng() & 15u;
            const uint32_t r = rng();
            mag[t] = t >= K ? 0 : (r & 0x300u) == 0 ? 0 : (r & 0x400u) ? 127 : r & 0x7Fu; // a quarter zeros: "-0" must not appear
        }
        const uint32_t end = rng() & 7u;
        // the reference: step by step from the last step down
        std::vector<uint8_t> want(128, 0);
        uint32_t cur = end;
        for (int t = K - 1; t >= 0; t--) {
            const bool neg = step_back(nib[t], cur);
            want[t] = (neg && mag[t]) ? mag[t] | 0x80u : mag[t];
            n_zero_under_sign += neg && !mag[t];
        }
        // the kernel: the decision word of eight steps has step r in nibble 7 - r, byte b = steps 7 - 2b (low nibble) and 6 - 2b
        std::vector<uint32_t> sgn(64 * 2 * nblk);
        for (auto &v : sgn) v = rng();
        cur = end;
        for (int blk = 1; blk >= 0; blk--) {
            uint32_t sb[2] = {0, 0}, acc[2] = {0, 0};
            for (int g = 7; g >= 0; g--) {
                if ((g & 3) == 3) acc[0] = acc[1] = 0;
                if (blk * 64 + g * 8 < K) {
                    uint32_t word = 0;
                    for (int r = 0; r < 8; r++) word |= (uint32_t)nib[blk * 64 + g * 8 + r] << (4 * (7 - r));
                    for (int b = 0; b < 4; b++) {
                        const uint32_t e = sw::traceback_entry((word >> (8 * b)) & 0xFFu, cur);
                        cur = e & 7u;
                        acc[b & 1] = sw::sign_acc_push(acc[b & 1], e);
                    }
                }
                if ((g & 3) == 0) sb[g >> 2] = sw::sign_word_join(acc[0], acc[1]);
            }
            sgn.at(sw::sign_word_index(lane, nblk, 2 * blk)) = sb[0];
            sgn.at(sw::sign_word_index(lane, nblk, 2 * blk + 1)) = sb[1];
        }
        for (int t = 0; t < 128; t++) { // the words against the definition: step t in bit sign_plane_bit(t) of word t >> 5, 0 past the block end
            const uint32_t bit = (sgn[sw::sign_word_index(lane, nblk, t >> 5)] >> sw::sign_plane_bit(t)) & 1u;
            CHECK_EQ((uint32_t)(bit && mag[t]), (uint32_t)(want[t] >> 7), "rep %d K %d step %d: the stored bit", rep, K, t);
            if (t >= K) CHECK_EQ(bit, 0u, "rep %d K %d step %d past the block end", rep, K, t);
        }
        // perm / vote: unit u of the 8, its magnitude words and the halo word
        for (uint32_t u = 0; u < 8; u++) {
            const UnitSigned us = load_unit_signed(mag, sgn, lane, nblk, u);
            n_unit[u & 3]++;
            if (u == 0) { CHECK_EQ(us.w[0], 0x7F7F7F7Fu, "rep %d: the first unit's preset", rep); n_preset++; }
            else if (u == 4) n_halo_block++;
            else if ((u & 1u) == 0) n_halo_word++;
            for (int j = (u > 0 ? -1 : 0); j < 4; j++) {
                uint32_t m = 0, w = 0;
                for (int i = 0; i < 4; i++) { m |= (uint32_t)mag[16 * u + 4 * j + i] << (8 * i); w |= (uint32_t)want[16 * u + 4 * j + i] << (8 * i); }
                int       nv = K - (int)(16 * u + 4 * j); // valid steps of the word: the kernels zero what lies past the block end
                uint32_t  keep = nv >= 4 ? 0xFFFFFFFFu : 0u;
                if (nv > 0 && nv < 4) { printf("MISMATCH: K %% 4 != 0\n"); return 1; }
                const uint32_t got = us.w[j + 1];
                if (keep) CHECK_EQ(got, w, "rep %d K %d unit %u word %d: got %08x want %08x", rep, K, u, j, got, w);
                else      CHECK_EQ(got, m, "rep %d K %d unit %u word %d past the end: no sign may be set (%08x, m = %08x)", rep, K, u, j, got, m);
                if (j >= 0) CHECK_EQ(us.s[j], got & sw::HI, "rep %d K %d unit %u word %d: the split sign field", rep, K, u, j);
            }
        }
    }
    // ---- 4: the layout
    {
        uint32_t seen = 0;
        for (uint32_t t = 0; t < 32; t++) {
            const uint32_t p = sw::sign_plane_bit(t);
            CHECK_EQ(p, 8u * (t % 4u) + t / 4u, "step %u: bit %u is not the definition's", t, p);
            CHECK_EQ(sw::sign_plane_step(p), t, "step %u: the inverse map", t);
            CHECK_EQ(sw::sign_plane_bit(t + 32u), p, "step %u + 32: the same bit of the next word", t);
            if (p < 32) seen |= 1u << p;
        }
        CHECK_EQ(seen, 0xFFFFFFFFu, "the bit map is not a permutation of the 32 positions (%08x)", seen);
        uint64_t lanes = 0;
        for (uint32_t L = 0; L < 64; L++) lanes |= 1ull << sw::sign_plane_lane(L);
        CHECK_EQ(lanes, ~0ull, "the lane map is not a permutation of the 64 lanes");
        for (int i = 0; i < 100000; i++) {
            const uint64_t steps = i < 64 ? 1ull << i : ((uint64_t)rng() << 32 | rng()) & ((i & 7) == 1 ? ((1ull << (8 * (1 + rng() % 7u))) - 1) : ~0ull); // single steps, short blocks, any
            uint32_t a[2];
            pack_lockstep(steps, rng, a);
            const uint32_t b[2] = {sw::sign_word_from_steps(steps, 0), sw::sign_word_from_steps(steps, 1)};
            CHECK_EQ(a[0], b[0], "mask %016llx word 0: lock-step %08x, from the ballot %08x", (unsigned long long)steps, a[0], b[0]);
            CHECK_EQ(a[1], b[1], "mask %016llx word 1: lock-step %08x, from the ballot %08x", (unsigned long long)steps, a[1], b[1]);
            uint64_t back = 0;
            for (uint32_t t = 0; t < 64; t++) back |= (uint64_t)((b[t >> 5] >> sw::sign_plane_bit(t)) & 1u) << t;
            CHECK_EQ(back, steps, "mask %016llx: read back by the definition", (unsigned long long)steps);
        }
        for (int q = 0; q < 4; q++) CHECK_EQ(n_unit[q] > 0, true, "no unit at position u %% 4 = %d was expanded", q);
        CHECK_EQ(n_halo_word > 0 && n_halo_block > 0 && n_preset > 0 && n_zero_under_sign > 0, true, "part 3 missed a case of the halo or of magnitude 0");
        printf("sign planes: units per position u %% 4: %ld %ld %ld %ld; halo across a word %ld, across a block %ld, preset %ld; magnitude 0 under a set sign %ld\n",
               n_unit[0], n_unit[1], n_unit[2], n_unit[3], n_halo_word, n_halo_block, n_preset, n_zero_under_sign);
    }
    printf("turbo signs driver: %ld checks, %ld mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
