// tools/asan/soft_pack_driver.cc: the packed soft-bit hand-over's pure functions (openlte_amd/csrc/soft_pack.h) on the CPU, under
// g++ -fsanitize=address,undefined (tools/asan/run_soft_pack.sh).  The demodulator's packing loop and the turbo prep kernel's two staging loops
// are restated here thread by thread around the header's functions, on heap blocks of exactly the size the kernels may touch, and checked
// against scalar statements of the format and of the staged copy's contract.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../openlte_amd/csrc/soft_pack.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static long n_checked = 0, n_bad = 0;
static void check(bool ok, const char *what, long a, long b)
{
    n_checked++;
    if (!ok && n_bad++ < 20) printf("MISMATCH %s (%ld, %ld)\n", what, a, b);
}

// k_pdsch_demod's copy-out of a packed allocation: `masks` is the LDS block (one byte per symbol, junk behind the last symbol up to the
// next sixteen), `slot` receives exactly ceil(M * QM / 32) dwords; group gi is one thread
template <uint32_t QM> static void demod_pack(const std::vector<uint8_t> &masks, uint32_t M, std::vector<uint32_t> &slot)
{
    const uint32_t N_bits = M * QM, nd = (N_bits + 31) >> 5, ng = (M + 15) >> 4;
    std::vector<int> writes(nd, 0);
    slot.assign(nd, 0xDEADBEEFu);
    for (uint32_t gi = 0; gi < ng; gi++) {
        uint32_t m[4], o[QM / 2];
        memcpy(m, masks.data() + 16 * gi, 16);
        soft_pack16<QM>(m, M - 16 * gi < 16 ? M - 16 * gi : 16, o);
        for (uint32_t k = 0; k < QM / 2; k++)
            if (gi * (QM / 2) + k < nd) { slot[gi * (QM / 2) + k] = o[k]; writes[gi * (QM / 2) + k]++; }
    }
    for (uint32_t d = 0; d < nd; d++) check(writes[d] == 1, "every dword written exactly once", d, writes[d]);
}

// the byte form's value of soft bit n, from the masks
template <uint32_t QM> static int byte_value(const std::vector<uint8_t> &masks, uint32_t n) { return ((masks[n / QM] >> (n % QM)) & 1) ? -127 : 127; }

// SrcRateUnmatch::stage_e on a packed allocation: LDS lines 0 .. E / 16, thread w per line.  Scalar statement of its contract: byte i of the
// copy is soft bit i for i < E and 0 from E to the next 16-byte boundary (a whole line of zeros when E is a multiple of 16), nothing behind it.
static void stage_whole(const std::vector<uint32_t> &slot, uint32_t E, std::vector<int8_t> &lds)
{
    const uint32_t nq = E >> 4, tail = E & 15u;
    lds.assign(16 * (nq + 1), 0x55);
    uint32_t w[4];
    for (uint32_t q = 0; q < nq; q++) { soft_stage_quad(slot.data(), q, 16, w); memcpy(lds.data() + 16 * q, w, 16); }
    if (tail) soft_stage_quad(slot.data(), nq, tail, w); else w[0] = w[1] = w[2] = w[3] = 0;
    memcpy(lds.data() + 16 * nq, w, 16);
}

// gather_windowed_pk's staging of the lap that starts at soft bit `base`, len soft bits long: the copy starts at the 16-byte line `base` lies in
static void stage_lap(const std::vector<uint32_t> &slot, uint32_t base, uint32_t len, std::vector<int8_t> &lds, uint32_t &shift)
{
    shift = base & 15u;
    const uint32_t end = shift + len, nq = end >> 4, tail = end & 15u, q0 = (base - shift) >> 4;
    lds.assign(16 * (nq + 1), 0x55);
    uint32_t w[4];
    for (uint32_t q = 0; q <= nq; q++) {
        const uint32_t keep = q < nq ? 16u : tail;
        if (keep) soft_stage_quad(slot.data(), q0 + q, keep, w); else w[0] = w[1] = w[2] = w[3] = 0;
        memcpy(lds.data() + 16 * q, w, 16);
    }
}

template <uint32_t QM> static void one_length(uint32_t M, int fill)
{
    std::vector<uint8_t> masks(((size_t)M + 15) & ~(size_t)15);
    for (size_t i = 0; i < masks.size(); i++) masks[i] = fill == 0 ? 0 : fill == 1 ? (uint8_t)((1u << QM) - 1u) : (uint8_t)(rnd() & ((1u << QM) - 1u));
    for (size_t i = M; i < masks.size(); i++) masks[i] = (uint8_t)rnd(); // what the kernel's LDS holds behind the last symbol: anything, high bits too
    std::vector<uint32_t> slot;
    demod_pack<QM>(masks, M, slot);
    const uint32_t E = M * QM;
    for (uint32_t n = 0; n < E; n++) check((((slot[n >> 5] >> (n & 31)) & 1u) ? -127 : 127) == byte_value<QM>(masks, n), "bit n of the slot", M, n);
    for (uint32_t n = E; n < 32 * (uint32_t)slot.size(); n++) check(((slot[n >> 5] >> (n & 31)) & 1u) == 0, "tail bit clear", M, n);
    std::vector<int8_t> lds;
    stage_whole(slot, E, lds);
    for (uint32_t i = 0; i < lds.size(); i++) check(lds[i] == (i < E ? byte_value<QM>(masks, i) : 0), "staged byte", M, i);
    // laps: a few lap lengths, every lap of the allocation (the last one short)
    const uint32_t laps[4] = {E / 2 + 1, 37, 132 + (M % 29), E > 48 ? E - 47 : E};
    for (uint32_t Nnn : laps) {
        if (Nnn == 0 || Nnn >= E) continue;
        for (uint32_t base = 0; base < E; base += Nnn) {
            const uint32_t len = Nnn < E - base ? Nnn : E - base;
            uint32_t shift;
            stage_lap(slot, base, len, lds, shift);
            for (uint32_t r = 0; r < len; r++) check(lds[shift + r] == byte_value<QM>(masks, base + r), "lap byte", base, r);
            for (uint32_t i = shift + len; i < lds.size(); i++) check(lds[i] == 0, "lap tail zero", base, i);
        }
    }
}

int main()
{
    // every nibble: byte k is 0x81 where bit k is set and 0x7F where it is clear
    for (uint32_t nib = 0; nib < 16; nib++) {
        uint32_t want = 0;
        for (uint32_t k = 0; k < 4; k++) want |= (((nib >> k) & 1u) ? 0x81u : 0x7Fu) << (8 * k);
        check(soft_expand4(nib) == want, "nibble", nib, soft_expand4(nib));
        check(soft_expand4(nib | 0xFFFFFFF0u) == want, "nibble with junk above", nib, 0);
    }
    for (uint32_t bits = 0; bits < 65536; bits += 1 + (bits & 7)) {
        uint32_t w[4];
        soft_expand16(bits, w);
        for (uint32_t k = 0; k < 16; k++) check((int8_t)(w[k >> 2] >> (8 * (k & 3))) == (((bits >> k) & 1u) ? -127 : 127), "sixteen bits", bits, k);
        for (uint32_t keep = 0; keep <= 16; keep++) {
            uint32_t v[4] = {w[0], w[1], w[2], w[3]};
            soft_keep_bytes(v, keep);
            for (uint32_t k = 0; k < 16; k++)
                check((int8_t)(v[k >> 2] >> (8 * (k & 3))) == (k < keep ? (((bits >> k) & 1u) ? -127 : 127) : 0), "kept bytes", bits, keep * 16 + k);
            if (bits > 64) break; // (every keep for a few patterns)
        }
    }
    // every length of 1 .. 300 symbols, and lengths around multiples of 32 and 128 bits further out
    for (uint32_t M = 1; M <= 300; M++)
        for (int fill = 0; fill < 3; fill++) { one_length<4>(M, fill); one_length<6>(M, fill); }
    for (uint32_t bits = 1024; bits <= 94208; bits = bits < 4096 ? bits + 128 : bits * 2 + 128)
        for (int d = -2; d <= 2; d++) {
            one_length<4>((bits + 32 * d) / 4 + d, 2); one_length<4>(bits / 4 + d, 2);
            one_length<6>((bits + 32 * d) / 6 + d, 2); one_length<6>(bits / 6 + d, 2);
        }
    one_length<6>(1656, 2);  // W4's 12-PRB allocation
    one_length<6>(15600, 2); // the longest packed allocation: 100 PRB, CFI 1
    printf("soft pack driver: %ld checks, %ld mismatches\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}
