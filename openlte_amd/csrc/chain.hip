// PDSCH receive chain on gfx950: RE extraction + pre-decoding + demapping + descrambling in one kernel,
// then DL-SCH decoding (rate un-matching fused into the turbo decoder's prep kernel, CRC fused into
// its vote kernel; see turbo.hip).  Restates liblte_phy_pdsch_channel_decode
// (liblte/src/liblte_phy.cc:3690-3853) -> dlsch_channel_decode (:12762-12872) for a batch of
// allocations, inside the envelope the reference itself can decode (one code block per allocation,
// SURVEY F4).
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>

#include "plan_core.hpp"
#include "phy_dev.hpp"
#include "demap_llr.h"
#include "soft_pack.h"
#include "gold_run.h"
#include "pdsch_launch.h"

using namespace pdsch_geom;

namespace {

constexpr int N_SC_MAX = 1200;

struct DemodGeom { uint32_t N_rb_dl, N_ant, cfi, sf_stride; };
// PBCH / PSS / SSS window (liblte_phy.cc:3722-3742)
__device__ __forceinline__ void sync_window(uint32_t N_rb_dl, uint32_t &first_sc, uint32_t &last_sc)
{
    switch (N_rb_dl) {
    case 6:  first_sc = 0;           last_sc = 71;          break;
    case 15: first_sc = 4 * 12 + 6;  last_sc = 11 * 12 - 7; break;
    case 25: first_sc = 9 * 12 + 6;  last_sc = 16 * 12 - 7; break;
    case 50: first_sc = 22 * 12;     last_sc = 28 * 12 - 1; break;
    case 75: first_sc = 34 * 12 + 6; last_sc = 41 * 12 - 7; break;
    default: first_sc = 47 * 12;     last_sc = 53 * 12 - 1; break;
    }
}
// 12-bit mask of the sub-carriers of (symbol L, PRB prb) that carry PDSCH (liblte_phy.cc:3753-3789): per sub-carrier the
// reference first tests the CRS positions of the port count, and only where none matches the PBCH / PSS / SSS window of
// subframes 0 and 5 -- i.e. the union of two masks, both of which are closed forms of (cell, L, prb).
__device__ __forceinline__ uint32_t pdsch_mask(uint32_t N_ant, uint32_t cell, uint32_t sf, uint32_t L, uint32_t prb,
                                               uint32_t first_sc, uint32_t last_sc)
{
    const uint32_t l7 = L >= 7 ? L - 7 : L, c6 = cell % 6, c3 = cell % 3;
    uint32_t skip = 0;
    if (N_ant == 1) {
        if (l7 == 0) skip = 0x041u << c6;                     // j % 6 == cell % 6
        else if (l7 == 4) skip = 0x041u << ((c6 + 3) % 6);    // j % 6 == (cell + 3) % 6
    } else if (l7 == 0 || l7 == 4 || (N_ant == 4 && l7 == 1))
        skip = (0x249u << c3) & 0xFFFu;                       // j % 3 == cell % 3
    const bool win = (sf == 0 && L >= 7 && L <= 10) || ((sf == 0 || sf == 5) && (L == 5 || L == 6));
    const uint32_t s0 = prb * 12;
    if (win && last_sc >= s0 && first_sc <= s0 + 11) {
        const uint32_t lo = first_sc > s0 ? first_sc - s0 : 0u, hi = last_sc - s0 < 11u ? last_sc - s0 : 11u;
        skip |= ((2u << hi) - 1u) & ~((1u << lo) - 1u);
    }
    return ~skip & 0xFFFu;
}

// Wave 0 of the demodulators: the pair table of one allocation -- per (symbol, PRB) pair, for ALL 14 symbols, tab[q].y = a 12-bit RE mask (0 in the
// control region) under the pair's position L * 1200 + first sub-carrier, tab[q].x = the running count of REs before the pair (a scan inside
// the wave), tab[n_pairs].x = the total.
__device__ __forceinline__ void pair_table_scan(uint2 *tab, const mi_lte_pdsch_alloc &al, uint32_t N_ant, uint32_t cell, uint32_t sf, uint32_t cfi,
                                                uint32_t n_pairs, uint32_t first_sc, uint32_t last_sc)
{
    const uint32_t N_prb = al.N_prb;
    const uint32_t ln = threadIdx.x, per = (n_pairs + 63) / 64, q0 = ln * per, q1 = min(q0 + per, n_pairs);
    // q / N_prb as a truncated float product (q < 1540): the hardware reciprocal is within 1 ulp of 1 / N_prb, three ulp on top make it an
    // upper bound, and the excess -- under 5 * 2^-23 of q / N_prb -- stays far below the 1 / N_prb that separates a quotient from the next
    // integer.  The exact magic number (0xFFFFFFFF / N_prb + 1) was a 32-bit division of a workgroup-uniform value on the vector unit.
    const float r_prb = __builtin_amdgcn_rcpf((float)N_prb) * (1.0f + 0x1.8p-22f);
    uint32_t local = 0;
    for (uint32_t q = q0; q < q1; q++) {
        const uint32_t L = (uint32_t)((float)q * r_prb), prb = al.prb[L >= 7 ? 1 : 0][q - __umul24(L, N_prb)];
        const uint32_t m = L < cfi ? 0u : pdsch_mask(N_ant, cell, sf, L, prb, first_sc, last_sc);
        tab[q].y = m | ((L * N_SC_MAX + prb * 12) << 12); // low 12 bits: RE mask, high 20 bits: L*1200 + first sub-carrier
        local += __popc(m);
    }
    uint32_t incl = local;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t n = __shfl_up(incl, o);
        if ((int)ln >= o) incl += n;
    }
    uint32_t run = incl - local;
    for (uint32_t q = q0; q < q1; q++) {
        tab[q].x = run;
        run += __popc(tab[q].y & 0xFFFu);
    }
    if (ln == 63) tab[n_pairs] = make_uint2(incl, 0u); // total
}

// (k_pdsch_demod's `flags`, DEMOD_PACK and DEMOD_GOLD_TABLE: pdsch_launch.h)
// words per run of the scrambling sequence's recurrence (gold_run.h; 2 / 4 / 8 measured: profiles/r11_variants_demod_prologue.txt)
#ifndef GOLD_RUN_R
#define GOLD_RUN_R 2
#endif

// The kernel is latency-bound (a chain of dependent table reads, then scattered plane reads per resource element), so it lives on
// occupancy: 8 waves per SIMD with a few spilled registers beat 4 without (2.80 -> 2.18 ms per 32k subframes); the single-port
// case is its own instantiation so that the 2/4-port combiners do not set its register count.
template <bool ONE_PORT, bool COMPACT = false>
#ifndef DEMOD_WPE
#define DEMOD_WPE 8
#endif
#ifndef DEMOD_WPE_C
#define DEMOD_WPE_C 8
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(COMPACT ? DEMOD_WPE_C : DEMOD_WPE, 8))) void k_pdsch_demod(const float *__restrict__ subframes, DemodGeom g,
                                                     const mi_lte_pdsch_alloc *__restrict__ allocs,
                                                     const uint32_t *__restrict__ subfr_num, const uint32_t *__restrict__ n_id_cell,
                                                     GoldTables gt, int8_t *__restrict__ e_base, const uint32_t *__restrict__ e_off,
                                                     uint32_t *__restrict__ e_len, uint32_t max_pairs, uint32_t words_al,
                                                     uint32_t e_lds_cap, uint32_t flags)
{
    const uint32_t pack = flags & DEMOD_PACK;
    extern __shared__ __attribute__((aligned(16))) uint32_t smu[]; // tab[max_pairs+1] (offset, mask | position) | cw[...] | soft bits (packed hand-over: one mask byte per symbol)
    __shared__ uint2 qam_lut[64]; // hard-decision mask -> six soft bits (16QAM / 64QAM)
    static_assert(sizeof(qam_lut) == REF_STATIC_LDS, "pdsch_launch.h counts the static LDS");
    const uint32_t a_idx = blockIdx.x;
    const mi_lte_pdsch_alloc &al = allocs[a_idx];
    const uint32_t unit = al.unit, sf = subfr_num[unit], cell = n_id_cell[unit], N_ant = ONE_PORT ? 1u : g.N_ant, N_prb = al.N_prb;
    const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : al.mod_type == 1 ? 2 : 1;
    uint2    *tab = reinterpret_cast<uint2 *>(smu);
    uint32_t *cw  = smu + pairs_words(max_pairs); // cw and e_lds stay 16-byte aligned
    uint32_t first_sc, last_sc;
    sync_window(g.N_rb_dl, first_sc, last_sc);

    // ---- phases 1 and 2 side by side.  Wave 0: which REs, in the reference's loop order L -> PRB -> sub-carrier
    // (liblte_phy.cc:3744-3802) -- per (symbol, PRB) pair, for ALL 14 symbols, a 12-bit mask (0 in the control region) with the pair's
    // position L * 1200 + first sub-carrier above it and, by a scan inside the wave, the running count of REs before the pair.
    // Waves 1-3: the scrambling sequence words (c_init per :3831) for the upper bound of the bit count, which does not wait for the scan.
    // One barrier for both.
    const uint32_t cfi = al.n_pdcch_symbs ? al.n_pdcch_symbs : g.cfi; // the allocation's own control-region size, or the plan's
    const uint32_t n_pairs = 14 * N_prb, pair0 = cfi * N_prb;          // pairs [0, pair0) are the control region: empty masks
    const uint32_t c_init = ((al.rnti << 14) | (0u << 13) | (sf << 9) | cell) & 0x7FFFFFFFu; // 31 bits: the Gold basis has 31 rows
    if (threadIdx.x < 64) pair_table_scan(tab, al, N_ant, cell, sf, cfi, n_pairs, first_sc, last_sc);
    else {
        const uint32_t n_words_ub = ((n_pairs - pair0) * 12 * Qm + 31) / 32; // <= max_words; one word of slack for the 2-word window in put_bits
        if (threadIdx.x < 128) qam_lut[threadIdx.x - 64] = qam_lut_entry(threadIdx.x - 64);
        gold_fill_words<GOLD_RUN_R>(cw, gt, c_init, n_words_ub, threadIdx.x - 64, blockDim.x - 64, (flags & DEMOD_GOLD_TABLE) != 0);
    }
    __syncthreads();
    const uint32_t M_ap = tab[n_pairs].x;
    // pre-decoder / layer de-mapper symbol counts (liblte_phy.cc:7683, 7693, 7720, 7497).  M_ap is a multiple of N_ant for every
    // allocation the extraction above can produce: each (slot, PRB) contributes 12, 8 or -- next to the PBCH / PSS / SSS window of the
    // odd bandwidths -- 6 + 6, 4 + 4 + 6 + 6 resource elements (enumerated over every bandwidth, cell, subframe and control-region size
    // in tests/test_fuzz_cpu.py), so the reference's `M_ap_symb % 4 != 0` branch (:7766-7795, with the mis-strided layer de-mapper
    // it would feed, :7473-7514) is dead code on this path and the division is exact.
    const uint32_t n_grp = M_ap >> (N_ant >> 1), M_symb = n_grp * N_ant, N_bits = M_symb * Qm; // (N_ant is 1, 2 or 4)
    if (threadIdx.x == 0) e_len[a_idx] = N_bits;

    // ---- phase 3: per group of N_ant REs: gather, pre-decode, de-map, descramble.  The modulation is uniform over the workgroup: the whole
    // phase is instantiated per modulation (`run` below), so that the per-element code holds no modulation branch, no re-read of the
    // allocation descriptor and compile-time bit counts -- as one generic routine it was a dozen scalar branches and a scalar load per element
    const float *base = subframes + (size_t)unit * g.sf_stride;
    const float *y_re_p = base, *y_im_p = base + 16 * N_SC_MAX;
    const float *h_re_p = base + 2 * 16 * N_SC_MAX, *h_im_p = h_re_p + (size_t)N_ant * 16 * N_SC_MAX;
    int8_t *e = e_base + (size_t)e_off[a_idx] * 64; // offsets are kept in 64-byte units: a batch may hold more than 4 GiB of soft bits
    auto locate = [&](uint32_t idx) -> uint32_t { // RE index -> L * 1200 + sub-carrier
        uint32_t lo = pair0, hi = n_pairs; // tab[lo].x <= idx < tab[hi].x
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tab[mid].x <= idx) lo = mid; else hi = mid;
        }
        const uint2 t = tab[lo];
        uint32_t r = idx - t.x, m = t.y & 0xFFFu;
        for (; r; r--) m &= m - 1;
        return (t.y >> 12) + (uint32_t)__builtin_ctz(m);
    };
    // soft bits are assembled in LDS when they fit and leave with 16-byte stores
    int8_t    *e_lds  = reinterpret_cast<int8_t *>(cw + words_al);
    const bool via_lds = N_bits <= e_lds_cap;
    // the packed hand-over (soft_pack.h): a 16QAM / 64QAM allocation leaves as one bit per soft bit.  Its symbols' masks are collected in LDS,
    // one byte per symbol (at most 17 160 of them: the host sizes the block for it), and packed after the barrier below
    const bool pk = pack && al.mod_type >= 2;
    auto run = [&](auto modc, auto pkc) {
    constexpr uint32_t MOD = decltype(modc)::value, QM = MOD == 3 ? 6 : MOD == 2 ? 4 : MOD == 1 ? 2 : 1;
    constexpr bool     QAM = MOD >= 2, PK = decltype(pkc)::value;
    static_assert(QAM || !PK, "only hard-decision modulations are packed");
    auto each_dst = [&](auto f) { // where the symbols' soft bits go: the LDS block, or the allocation's slot itself when they do not fit
        if constexpr (PK) f(e_lds);
        else if (via_lds) f(e_lds);
        else f(e);
    };
    // descramble + store the Q_m soft bits of symbol idx: c bit set -> negate (liblte_phy.cc:3833-3836).
    // Q_m*idx is even for Q_m >= 2, so pairs of bytes leave as one 16-bit store.
    auto put_bits = [&](auto *dst, uint32_t idx, const int8_t (&b)[6]) {
        const uint32_t n0 = idx * QM, w = n0 >> 5, sh = n0 & 31;
        const uint32_t c = __builtin_amdgcn_alignbit(cw[w + 1], cw[w], sh); // bits n0.. of the scrambling sequence (cw is padded by one word)
        if (QM == 1) dst[n0] = (c & 1u) ? (int8_t)-b[0] : b[0];
        else {
#pragma unroll
            for (uint32_t k = 0; k < 6; k += 2)
                if (k < QM) {
                    const int lo = ((c >> k) & 1u) ? -b[k] : b[k], hi = ((c >> (k + 1)) & 1u) ? -b[k + 1] : b[k + 1];
                    *reinterpret_cast<uint16_t *>(dst + n0 + k) = (uint16_t)((lo & 0xFF) | ((hi & 0xFF) << 8));
                }
        }
    };
    // 16QAM / 64QAM: every soft bit is +-127, so a symbol is its mask of negative bits; XOR with the scrambling bits and one table
    // read give the Q_m bytes (4: one store; 6: three 16-bit stores, the symbol starts on an even address)
    auto put_qam = [&](auto *dst, uint32_t idx, uint32_t neg) {
        const uint32_t n0 = QM == 4 ? idx << 2 : __umul24(idx, 6u), w = n0 >> 5, sh = n0 & 31;
        const uint32_t c  = __builtin_amdgcn_alignbit(cw[w + 1], cw[w], sh);
        const uint2    v  = qam_lut[(neg ^ c) & (QM == 4 ? 15u : 63u)];
        if (QM == 4) *reinterpret_cast<uint32_t *>(dst + n0) = v.x;
        else {
            *reinterpret_cast<uint16_t *>(dst + n0)     = (uint16_t)v.x;
            *reinterpret_cast<uint16_t *>(dst + n0 + 2) = (uint16_t)(v.x >> 16);
            *reinterpret_cast<uint16_t *>(dst + n0 + 4) = (uint16_t)v.y;
        }
    };
    // equalised symbol (nr, ni) / den -> soft bits of RE idx.  16QAM / 64QAM: the decisions without the divisions (qam_neg_bits_nodiv:
    // the reference's own divisions under a guard next to the thresholds); BPSK / QPSK grade the quotient, so they divide.
    // the packed hand-over's: the XORed mask itself, one byte per symbol
    auto put_mask = [&](auto *dst, uint32_t idx, uint32_t neg) {
        const uint32_t n0 = QM == 4 ? idx << 2 : __umul24(idx, 6u), w = n0 >> 5, sh = n0 & 31;
        const uint32_t c  = __builtin_amdgcn_alignbit(cw[w + 1], cw[w], sh);
        reinterpret_cast<uint8_t *>(dst)[idx] = (uint8_t)((neg ^ c) & (QM == 4 ? 15u : 63u));
    };
    auto put_symbol = [&](auto *dst, uint32_t idx, float nr, float ni, float den) {
        if constexpr (PK) put_mask(dst, idx, qam_neg_bits_nodiv<MOD>(nr, ni, den));
        else if constexpr (QAM) put_qam(dst, idx, qam_neg_bits_nodiv<MOD>(nr, ni, den));
        else {
            int8_t b[6] = {0, 0, 0, 0, 0, 0};
            demap_symbol<true>(nr / den, ni / den, MOD, b);
            put_bits(dst, idx, b);
        }
    };
    if (ONE_PORT && COMPACT) {
        // MI_LTE_CE_COMPACT: the estimate arrives as magnitude / phase rows at the five CRS symbols (mag in the real-part plane, phase in
        // the imaginary-part plane, rows 0-4).  One thread per (slot, PRB, sub-carrier): it loads the six values its slot's two segments
        // hang on (and, in the second slot, the two phases its first row is wrapped through), runs the reference's time interpolation
        // (the later segments depend on the phases wrapped in the earlier ones), and equalises its slot's resource elements with
        // m * (cos a, sin a) -- the values k_dl_ce would have written, bit for bit.  Rows are addressed as a uniform row pointer plus one
        // 32-bit byte offset per thread (global_load ... saddr), the pair table gives the PRB and the first RE in one LDS read.
        constexpr uint32_t ROW = N_SC_MAX * 4, Y_IM = 16 * ROW, H_M = 32 * ROW, H_A = 48 * ROW; // byte offsets of the planes in a unit
        const uint32_t per_slot = N_prb * 12, n_items = 2 * per_slot;
        // one buffer descriptor for the unit: a load is (descriptor, 32-bit byte offset per thread, row offset in a scalar register)
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, (int)(g.sf_stride * 4u), 0x00020000);
        auto ld = [&](uint32_t row, uint32_t off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)off, (int)row, 0)); };
        auto body = [&](auto *dst) {
            for (uint32_t item = threadIdx.x; item < n_items; item += blockDim.x) {
                const uint32_t s = item >= per_slot ? 1u : 0u, r = item - s * per_slot, i = __umul24(r, 43691u) >> 19, j = r - ((i << 3) + (i << 2)); // r / 12 for r < 2^15; 12 i as shifts (the product form became a 64-bit multiply-add at a quarter of the rate)
                const uint32_t bit = 1u << j, below = bit - 1u;
                const uint2   *tp = tab + (s ? 7 * N_prb : 0u) + i; // the pair of the slot's first symbol; the next symbols' are N_prb apart
                const uint2    t0 = *tp;
                const uint32_t vy = ((t0.y >> 12) + j) << 2;                  // byte offset of (symbol 7s, sub-carrier k) in a plane
                const uint32_t vk = vy - s * (7 * ROW), vh = vk + s * (2 * ROW); // (row 0, k) and (row 2s, k)
                const float M0 = ld(H_M, vh), M1 = ld(H_M + ROW, vh), M2 = ld(H_M + 2 * ROW, vh);
                const float P0 = ld(H_A, vh), P1 = ld(H_A + ROW, vh), P2 = ld(H_A + 2 * ROW, vh);
                const float Q0 = ld(H_A, vk), Q1 = ld(H_A + ROW, vk); // the first slot's phases (second slot only; the same rows again in the first)
                // the slot's symbols: requested before the interpolation needs its inputs.  Not the control region's (first slot, symbols below
                // cfi <= 4): their masks are empty and the loop below skips them, so nothing reads what is left in their place.  cfi is uniform
                // over the workgroup, s over all but one of its wavefronts.  (Q0, Q1 stay unconditional: in the first slot they repeat P0, P1's
                // addresses, and a branch around them cost what this one gains -- profiles/r11_variants_demod_prologue.txt)
                float yr[7], yi[7];
#pragma unroll
                for (int t = 0; t < 7; t++) {
                    yr[t] = yi[t] = 0.0f;
                    if (t >= 4 || s || (uint32_t)t >= cfi) { yr[t] = ld(t * ROW, vy); yi[t] = ld(Y_IM + t * ROW, vy); }
                }
                // liblte_phy.cc:6119-6190 for symbols 7s .. 7s+6 (ce_time_interp5 above is the whole subframe): symbols 7s and 7s+4 take
                // the CRS-symbol values as estimated; the slopes see the phases wrapped against their predecessors, from symbol 0 on
                float m[7], a[7];
                m[0] = M0; a[0] = P0; m[4] = M1; a[4] = P1;
                float W0 = P0;
                if (s) W0 = wrap_phase_rare(P0, wrap_phase_rare(Q1, Q0));
                {
                    const float fm = (M1 - M0) / 4, W1 = wrap_phase_rare(P1, W0);
                    const float fa = wrap_phase_rare(W1 - W0, 0.0f) / 4;
                    float cm = M1, ca = W1;
#pragma unroll
                    for (int z = 3; z > 0; z--) { cm -= fm; ca -= fa; m[z] = cm; a[z] = ca; }
                    const float gm = div3(M2 - M1), W2 = wrap_phase_rare(P2, W1);
                    const float ga = div3(wrap_phase_rare(W2 - W1, 0.0f));
                    cm = M2; ca = W2;
#pragma unroll
                    for (int z = 6; z > 4; z--) { cm -= gm; ca -= ga; m[z] = cm; a[z] = ca; }
                }
#pragma unroll
                for (int t = 0; t < 7; t++) {
                    const uint2 pr = t ? tp[t * N_prb] : t0;
                    if (!(pr.y & bit)) continue;
                    const uint32_t idx = pr.x + __popc(pr.y & below);
                    float sn, cs;
                    ce_sincos(a[t], sn, cs);
                    const float mm = m[t], hr = mm * cs, hi = mm * sn;
                    const float hn = hr * hr + hi * hi;
                    put_symbol(dst, idx, yr[t] * hr + yi[t] * hi, yi[t] * hr - yr[t] * hi, hn);
                }
            }
        };
        each_dst(body);
    } else if (ONE_PORT) { // one RE = one symbol (liblte_phy.cc:7684-7690): thread per (PRB-symbol pair, sub-carrier), no search
        constexpr int UNR = 4; // loads of UNR independent REs in flight per thread (the kernel is latency-bound otherwise)
        // 21 pairs x 12 sub-carriers per sweep of the workgroup: a thread keeps its sub-carrier, so nothing is divided in the loop
        const uint32_t q_thr = threadIdx.x / 12, j = threadIdx.x - 12 * q_thr, below = (1u << j) - 1u;
        const bool     lane_on = threadIdx.x < 252;
        auto body = [&](auto *dst) {
            for (uint32_t qb = pair0; qb < n_pairs; qb += 21 * UNR) {
                float    yr[UNR], yi[UNR], hr[UNR], hi[UNR];
                uint32_t idx[UNR];
                bool     on[UNR];
#pragma unroll
                for (int r = 0; r < UNR; r++) {
                    const uint32_t q = qb + 21 * r + q_thr;
                    const bool     in = lane_on && q < n_pairs;
                    const uint2    pr = tab[in ? q : 0u];
                    on[r]  = in && ((pr.y >> j) & 1u);
                    idx[r] = pr.x + __popc(pr.y & below);
                    const uint32_t ob = on[r] ? ((pr.y >> 12) + j) << 2 : 0u; // byte offset in 32 bits: one register serves the four planes
                    yr[r] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(y_re_p) + ob);
                    yi[r] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(y_im_p) + ob);
                    hr[r] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(h_re_p) + ob);
                    hi[r] = *reinterpret_cast<const float *>(reinterpret_cast<const char *>(h_im_p) + ob);
                }
#pragma unroll
                for (int r = 0; r < UNR; r++) {
                    if (!on[r]) continue;
                    const float hn = hr[r] * hr[r] + hi[r] * hi[r];
                    put_symbol(dst, idx[r], yr[r] * hr[r] + yi[r] * hi[r], yi[r] * hr[r] - yr[r] * hi[r], hn);
                }
            }
        };
        each_dst(body);
    } else
    for (uint32_t i = threadIdx.x; i < n_grp; i += blockDim.x) {
        float n_re[4], n_im[4], den[4]; // x_p = (n_re, n_im) / den
        if (N_ant == 2) { // Alamouti combiner with the reference's normaliser (liblte_phy.cc:7694-7717)
            const uint32_t p0 = locate(2 * i), p1 = locate(2 * i + 1);
            const float y0r = y_re_p[p0], y0i = y_im_p[p0], y1r = y_re_p[p1], y1i = y_im_p[p1];
            const float h0r = h_re_p[p0], h0i = h_im_p[p0], h1r = h_re_p[16 * N_SC_MAX + p0], h1i = h_im_p[16 * N_SC_MAX + p0];
            const float a0 = h0r * h0r + h0i * h0i, a1 = h1r * h1r + h1i * h1i;
            const float hn = sqrtf(a0 * a0 + a1 * a1);
            den[0] = den[1] = hn;
            n_re[0] = h0r * y0r + h0i * y0i + h1r * y1r + h1i * y1i;
            n_im[0] = h0r * y0i - h0i * y0r - h1r * y1i + h1i * y1r;
            n_re[1] = -h1r * y0r - h1i * y0i + h0r * y1r + h0i * y1i;
            n_im[1] = h1r * y0i - h1i * y0r + h0r * y1i - h0i * y1r;
        } else { // N_ant == 4 (liblte_phy.cc:7721-7765); M_ap % 4 == 0 always, see the note at n_grp
            const uint32_t p0 = locate(4 * i), p1 = locate(4 * i + 1), p2 = locate(4 * i + 2), p3 = locate(4 * i + 3);
            const size_t   ps = 16 * N_SC_MAX;
            const float y0r = y_re_p[p0], y0i = y_im_p[p0], y1r = y_re_p[p1], y1i = y_im_p[p1];
            const float y2r = y_re_p[p2], y2i = y_im_p[p2], y3r = y_re_p[p3], y3i = y_im_p[p3];
            const float h0r = h_re_p[p0], h0i = h_im_p[p0], h2r = h_re_p[2 * ps + p0], h2i = h_im_p[2 * ps + p0];
            const float h1r = h_re_p[ps + p2], h1i = h_im_p[ps + p2], h3r = h_re_p[3 * ps + p2], h3i = h_im_p[3 * ps + p2];
            const float a0 = h0r * h0r + h0i * h0i, a1 = h1r * h1r + h1i * h1i, a2 = h2r * h2r + h2i * h2i, a3 = h3r * h3r + h3i * h3i;
            const float n02 = sqrtf(a0 * a0 + a2 * a2), n13 = sqrtf(a1 * a1 + a3 * a3);
            den[0] = den[1] = n02; den[2] = den[3] = n13;
            n_re[0] = h0r * y0r + h0i * y0i + h2r * y1r + h2i * y1i;
            n_im[0] = h0r * y0i - h0i * y0r - h2r * y1i + h2i * y1r;
            n_re[1] = -h2r * y0r - h2i * y0i + h0r * y1r + h0i * y1i;
            n_im[1] = -(-h2r * y0i + h2i * y0r - h0r * y1i + h0i * y1r);
            n_re[2] = h1r * y2r + h1i * y2i + h3r * y3r + h3i * y3i;
            n_im[2] = h1r * y2i - h1i * y2r - h3r * y3i + h3i * y3r;
            n_re[3] = -h3r * y2r - h3i * y2i + h1r * y3r + h1i * y3i;
            n_im[3] = -(-h3r * y2i + h3i * y2r - h1r * y3i + h1i * y3r);
        }
        // layer de-mapping d[i*N_ant + p] = x_p[i] (liblte_phy.cc:7506-7513), de-map, descramble (:3833-3836)
#pragma unroll
        for (uint32_t p = 0; p < 4; p++) {
            if (p >= N_ant) break;
            if (PK || via_lds) put_symbol(e_lds, i * N_ant + p, n_re[p], n_im[p], den[p]);
            else               put_symbol(e, i * N_ant + p, n_re[p], n_im[p], den[p]);
        }
    }
    };
    switch (al.mod_type) {
    case 0:  run(std::integral_constant<uint32_t, 0>{}, std::false_type{}); break;
    case 1:  run(std::integral_constant<uint32_t, 1>{}, std::false_type{}); break;
    case 2:  if (pk) run(std::integral_constant<uint32_t, 2>{}, std::true_type{}); else run(std::integral_constant<uint32_t, 2>{}, std::false_type{}); break;
    default: if (pk) run(std::integral_constant<uint32_t, 3>{}, std::true_type{}); else run(std::integral_constant<uint32_t, 3>{}, std::false_type{}); break;
    }
    if (pk) {
        // sixteen symbols' masks -> two (16QAM) or three (64QAM) dwords per thread: every dword of the slot is written by exactly one thread,
        // none behind the last one, and the last one's bits from N_bits on are 0 (soft_pack16 drops the masks past the last symbol)
        __syncthreads();
        const uint32_t nd = (N_bits + 31) >> 5, ng = (M_symb + 15) >> 4;
        uint32_t      *eo = reinterpret_cast<uint32_t *>(e);
        for (uint32_t gi = threadIdx.x; gi < ng; gi += blockDim.x) {
            const uint4    m4 = reinterpret_cast<const uint4 *>(e_lds)[gi];
            const uint32_t m[4] = {m4.x, m4.y, m4.z, m4.w}, nv = min(16u, M_symb - 16 * gi);
            if (Qm == 4) {
                uint32_t o[2];
                soft_pack16<4>(m, nv, o);
                const uint32_t d0 = 2 * gi;
                if (d0 + 2 <= nd) *reinterpret_cast<uint2 *>(eo + d0) = make_uint2(o[0], o[1]); // (8-byte aligned: the slot starts on a 64-byte line)
                else eo[d0] = o[0];
            } else {
                uint32_t o[3];
                soft_pack16<6>(m, nv, o);
                const uint32_t d0 = 3 * gi;
                if (d0 + 3 <= nd) { eo[d0] = o[0]; eo[d0 + 1] = o[1]; eo[d0 + 2] = o[2]; } // (twelve bytes on a 4-byte boundary: one three-dword store)
                else {
                    eo[d0] = o[0];
                    if (d0 + 1 < nd) eo[d0 + 1] = o[1];
                }
            }
        }
    } else if (via_lds) {
        __syncthreads();
        const uint32_t nq = (N_bits + 15) >> 4; // the allocation's slot in e_base is padded to 64 bytes
        for (uint32_t w = threadIdx.x; w < nq; w += blockDim.x) reinterpret_cast<uint4 *>(e)[w] = reinterpret_cast<const uint4 *>(e_lds)[w];
    }
}

// ---- MI_LTE_DEMAP_MAXLOG (include/mi_lte.h, "PDSCH, 3GPP mode: max-log soft-decision demapping"): the 3GPP plans' opt-in demapper.
// The LLR arithmetic (llr_axis, llr_byte) is demap_llr.h's, shared with the uplink's demapper.

// One kernel for the single-port plans (N_ANT = 1) and the transmit-diversity plans (N_ANT = 2, 4: include/mi_lte.h, "PDSCH, 3GPP mode: transmit
// diversity"): k_pdsch_demod's pair table, scrambling words, thread per (pair, sub-carrier), LDS assembly and soft-bit layout over the N_ANT-port
// extraction, with that demapper in place of the reference's.  Every thread does the symbol of its own resource element s and hands
// (t, w) to llr_axis / llr_byte.  One port: t = y(s) conj(h(s)), w = |h(s)|^2.  Two or four ports: the other element o of the thread's pair is the
// neighbouring set bit of the same 12-bit mask -- the next one for an even RE index, the previous one for an odd one.  The mask always has it: on
// two and four ports every (symbol, PRB) entry holds 4, 6, 8 or 12 resource elements, so every entry starts at an even RE index and no pair leaves
// its entry (tests/test_demap_geometry_cpu.py, test_every_txdiv_table_entry_is_even: all six bandwidths, every PRB, the window's half PRBs
// included).  The search of the table where the mask has none (`locate`) is a fallback that no valid geometry reaches.  Both symbols of a pair
// have one form,
//     z = conj(h_pa(s)) y(s) +- h_pb(o) conj(y(o)),  w = (|h_pa(s)|^2 + |h_pb(o)|^2) / 2     (+: even index, -: odd),
// so a thread loads two y and two h values, and t = z / sqrt 2.
// gain > 0: g = gain.  gain == 0: a first sweep over the allocation's estimate planes sums w (per thread, then inside each wave, then over the
// waves' LDS slots, always in that order and in double: a run is reproducible) and g = T / (4 A^2 wbar) (T = auto_t: MI_LTE_DEMAP_AUTO_T),
// rounded to float -- the value llr_gain[allocation] reports is the value the soft bits were scaled with.
// The last argument is the variant's block.  PdschLlrGain (empty): the two gains above.  PdschLlrNoise, the noise-referenced gain
// (mi_lte_pdsch_plan_set_llr_noise; launched and listed under the same names): no wbar sweep, g = scale / sigma2[unit] of the CRS noise
// estimate k_dl_crs_noise left (dl_noise.hip).  With PdschLlrGain every `if constexpr (Args::NOISE)` drops out and the kernel has the
// arguments, the LDS and the code it had before the noise-referenced gain.
struct PdschLlrGain {
    static constexpr bool NOISE = false;
};
struct PdschLlrNoise {
    static constexpr bool NOISE = true;
    const float *sigma2; // [n_units]: k_dl_crs_noise's estimates of this run
    float        scale;  // g = scale / sigma2[unit] in place of either gain
};
template <uint32_t N_ANT, typename Args>
__global__ __launch_bounds__(256) void k_pdsch_demod_llr(const float *__restrict__ subframes, DemodGeom g, const mi_lte_pdsch_alloc *__restrict__ allocs,
                                                         const uint32_t *__restrict__ subfr_num, const uint32_t *__restrict__ n_id_cell, GoldTables gt,
                                                         int8_t *__restrict__ e_base, const uint32_t *__restrict__ e_off, uint32_t *__restrict__ e_len,
                                                         uint32_t max_pairs, uint32_t words_al, uint32_t e_lds_cap, float gain, float auto_t,
                                                         float *__restrict__ llr_gain, uint32_t gold_table, Args args)
{
    static_assert(N_ANT == 1 || N_ANT == 2 || N_ANT == 4, "one port, or transmit diversity on two or four");
    static_assert(std::is_same<Args, PdschLlrGain>::value || std::is_same<Args, PdschLlrNoise>::value, "the variant's argument block");
    constexpr bool NOISE = Args::NOISE;
    extern __shared__ __attribute__((aligned(16))) uint32_t smu[]; // tab[max_pairs+1] (offset, mask | position) | cw[...] | soft bits
    __shared__ double w_wave[4];
    static_assert(sizeof(w_wave) == LLR_STATIC_LDS, "pdsch_launch.h counts the static LDS");
    const uint32_t a_idx = blockIdx.x;
    const mi_lte_pdsch_alloc &al = allocs[a_idx];
    const uint32_t unit = al.unit, sf = subfr_num[unit], cell = n_id_cell[unit], N_prb = al.N_prb;
    const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : 2; // (a 3GPP plan holds no BPSK allocation)
    uint2    *tab = reinterpret_cast<uint2 *>(smu);
    uint32_t *cw  = smu + pairs_words(max_pairs);
    uint32_t first_sc, last_sc;
    sync_window(g.N_rb_dl, first_sc, last_sc);
    const uint32_t cfi = al.n_pdcch_symbs ? al.n_pdcch_symbs : g.cfi;
    const uint32_t n_pairs = 14 * N_prb, pair0 = cfi * N_prb;
    const uint32_t c_init = ((al.rnti << 14) | (0u << 13) | (sf << 9) | cell) & 0x7FFFFFFFu;
    if (threadIdx.x < 64) pair_table_scan(tab, al, N_ANT, cell, sf, cfi, n_pairs, first_sc, last_sc);
    else {
        const uint32_t n_words_ub = ((n_pairs - pair0) * 12 * Qm + 31) / 32;
        gold_fill_words<GOLD_RUN_R>(cw, gt, c_init, n_words_ub, threadIdx.x - 64, blockDim.x - 64, gold_table != 0);
    }
    __syncthreads();
    // (M_ap is a multiple of N_ANT for every allocation: the note at k_pdsch_demod's n_grp)
    const uint32_t M_symb = (tab[n_pairs].x / N_ANT) * N_ANT, N_bits = M_symb * Qm;
    if (threadIdx.x == 0) e_len[a_idx] = N_bits;

    constexpr uint32_t PL = 16 * N_SC_MAX * 4; // bytes of one plane: y_re | y_im | h_re of the N_ANT ports | h_im of the N_ANT ports
    const float *base = subframes + (size_t)unit * g.sf_stride;
    const char  *y_re_p = reinterpret_cast<const char *>(base), *y_im_p = y_re_p + PL;
    const char  *h_re_p = y_im_p + PL, *h_im_p = h_re_p + N_ANT * PL;
    constexpr int  UNR = 4; // symbols in flight per thread: four loads each on one port, eight on two or four
    const uint32_t q_thr = threadIdx.x / 12, j = threadIdx.x - 12 * q_thr, below = (1u << j) - 1u;
    const bool     lane_on = threadIdx.x < 252;
    auto locate = [&](uint32_t idx) -> uint32_t { // RE index -> L * 1200 + sub-carrier (k_pdsch_demod's; two or four ports only)
        uint32_t lo = pair0, hi = n_pairs; // tab[lo].x <= idx < tab[hi].x
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tab[mid].x <= idx) lo = mid; else hi = mid;
        }
        const uint2 t = tab[lo];
        uint32_t r = idx - t.x, m = t.y & 0xFFFu;
        for (; r; r--) m &= m - 1;
        return (t.y >> 12) + (uint32_t)__builtin_ctz(m | 0x1000u);
    };
    // The thread's symbol in table pair q: whether it has one, its RE index, the byte offset inside a plane of its own resource element (os) and,
    // on two or four ports, of the other element of its pair (oo) and of its pair's two port planes (pa, pb).  The offsets are 0 where the thread
    // has no symbol (every load stays inside the unit)
    struct Elem { uint32_t os, oo, pa, pb, idx; bool on; };
    auto element = [&](uint32_t q) __attribute__((always_inline)) -> Elem {
        const bool     in  = lane_on && q < n_pairs;
        const uint2    pr  = tab[in ? q : 0u];
        const uint32_t lowm = pr.y & below, idx = pr.x + __popc(lowm);
        const bool     on  = in && ((pr.y >> j) & 1u) && (N_ANT == 1 || idx < M_symb);
        Elem e = {};
        e.on = on; e.idx = idx;
        e.os = on ? ((pr.y >> 12) + j) << 2 : 0u;
        if constexpr (N_ANT > 1) {
            const uint32_t up = (pr.y & 0xFFFu) >> (j + 1); // the mask's elements above this one
            uint32_t       po;                              // the other element's position
            if (idx & 1u) {
                po = (pr.y >> 12) + 31u - (uint32_t)__builtin_clz(lowm | 1u);
                if (on && !lowm) po = locate(idx - 1);
            } else {
                po = (pr.y >> 12) + j + 1 + (uint32_t)__builtin_ctz(up | 0x800u);
                if (on && !up) po = locate(idx + 1);
            }
            const uint32_t port = N_ANT == 4 ? ((idx >> 1) & 1u) * PL : 0u; // four ports: pair n = idx / 2 on ports (0, 2) for even n, (1, 3) for odd n
            e.oo = on ? po << 2 : 0u;
            e.pa = on ? port : 0u;
            e.pb = on ? port + (N_ANT == 4 ? 2 * PL : PL) : 0u;
        }
        return e;
    };
    auto ldf = [](const char *p, uint32_t off) __attribute__((always_inline)) { return *reinterpret_cast<const float *>(p + off); };
    double gd = (double)gain;
    if constexpr (NOISE) { // every thread forms the same quotient
        const float s2 = args.sigma2[unit], gf = (float)((double)args.scale / (double)s2);
        gd = (s2 > 0.0f && s2 <= 3.4028234e38f && fabsf(gf) <= 3.4028234e38f) ? (double)gf : 0.0; // sigma2 0 or not finite, or a gain past float: every soft bit 0
    } else if (gain == 0.0f) { // wbar: the mean of w over the allocation's symbols
        double part = 0.0;
        for (uint32_t qb = pair0; qb < n_pairs; qb += 21 * UNR) {
            float h[UNR][4];
            bool  on[UNR];
#pragma unroll
            for (int r = 0; r < UNR; r++) {
                const Elem e = element(qb + 21 * r + q_thr);
                on[r]   = e.on;
                h[r][0] = ldf(h_re_p, e.pa + e.os); h[r][1] = ldf(h_im_p, e.pa + e.os); // h_pa(s)  (one port: h(s), pa = 0)
                if constexpr (N_ANT > 1) { h[r][2] = ldf(h_re_p, e.pb + e.oo); h[r][3] = ldf(h_im_p, e.pb + e.oo); } // h_pb(o)
            }
#pragma unroll
            for (int r = 0; r < UNR; r++) {
                if (!on[r]) continue;
                const double wa = (double)h[r][0] * h[r][0] + (double)h[r][1] * h[r][1];
                if constexpr (N_ANT == 1) part += wa;
                else part += (wa + ((double)h[r][2] * h[r][2] + (double)h[r][3] * h[r][3])) * 0.5;
            }
        }
        for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
        if ((threadIdx.x & 63u) == 0) w_wave[threadIdx.x >> 6] = part;
        __syncthreads();
        const double wbar = (((w_wave[0] + w_wave[1]) + w_wave[2]) + w_wave[3]) / (double)M_symb;
        const double a4 = al.mod_type == 3 ? 4.0 / 42 : al.mod_type == 2 ? 4.0 / 10 : 2.0; // 4 A^2
        const float  gf = (float)((double)auto_t / (a4 * wbar));
        gd = (wbar > 0.0 && fabsf(gf) <= 3.4028234e38f) ? (double)gf : 0.0; // wbar 0, NaN or infinite, or a gain past float: every soft bit 0
    }
    if (threadIdx.x == 0) llr_gain[a_idx] = (float)gd;

    int8_t    *e      = e_base + (size_t)e_off[a_idx] * 64;
    int8_t    *e_lds  = reinterpret_cast<int8_t *>(cw + words_al);
    const bool via_lds = N_bits <= e_lds_cap;
    auto run = [&](auto modc, auto *dst) __attribute__((always_inline)) {
        constexpr uint32_t MOD = decltype(modc)::value, QM = MOD == 3 ? 6 : MOD == 2 ? 4 : 2;
        for (uint32_t qb = pair0; qb < n_pairs; qb += 21 * UNR) {
            float    y[UNR][4], h[UNR][4];
            uint32_t idx[UNR];
            bool     on[UNR];
#pragma unroll
            for (int r = 0; r < UNR; r++) {
                const Elem e = element(qb + 21 * r + q_thr);
                on[r] = e.on; idx[r] = e.idx;
                y[r][0] = ldf(y_re_p, e.os);        y[r][1] = ldf(y_im_p, e.os);        // y(s)
                h[r][0] = ldf(h_re_p, e.pa + e.os); h[r][1] = ldf(h_im_p, e.pa + e.os); // h_pa(s)  (one port: h(s), pa = 0)
                if constexpr (N_ANT > 1) {
                    y[r][2] = ldf(y_re_p, e.oo);        y[r][3] = ldf(y_im_p, e.oo);        // y(o)
                    h[r][2] = ldf(h_re_p, e.pb + e.oo); h[r][3] = ldf(h_im_p, e.pb + e.oo); // h_pb(o)
                }
            }
#pragma unroll
            for (int r = 0; r < UNR; r++) {
                if (!on[r]) continue;
                const double sr = y[r][0], si = y[r][1], har = h[r][0], hai = h[r][1];
                double       t_re, t_im, w;
                if constexpr (N_ANT == 1) {
                    w    = har * har + hai * hai;
                    t_re = sr * har + si * hai;
                    t_im = si * har - sr * hai;
                } else {
                    constexpr double RS2 = 0.70710678118654752; // 1 / sqrt 2
                    const double sg = (idx[r] & 1u) ? -1.0 : 1.0; // z0 = conj(h_pa(a)) y(a) + h_pb(b) conj(y(b)),  z1 = conj(h_pa(b)) y(b) - h_pb(a) conj(y(a))
                    const double yor = y[r][2], yoi = y[r][3], hbr = sg * h[r][2], hbi = sg * h[r][3];
                    const double zr = ((har * sr + hai * si) + hbr * yor) + hbi * yoi, zi = ((har * si - hai * sr) + hbi * yor) - hbr * yoi;
                    w    = ((har * har + hai * hai) + (hbr * hbr + hbi * hbi)) * 0.5;
                    t_re = zr * RS2;
                    t_im = zi * RS2;
                }
                double li[3], lq[3];
                llr_axis<MOD>(t_re, w, li);
                llr_axis<MOD>(t_im, w, lq);
                // descramble (c bit set -> negate) and store: Q_m idx is even, so the bytes leave in pairs (bit 2k on the real axis, 2k + 1 on the imaginary)
                const uint32_t n0 = idx[r] * QM, c = __builtin_amdgcn_alignbit(cw[(n0 >> 5) + 1], cw[n0 >> 5], n0 & 31);
#pragma unroll
                for (uint32_t k = 0; k < QM; k += 2) {
                    const int vi = llr_byte(gd, li[k >> 1]), vq = llr_byte(gd, lq[k >> 1]);
                    const int lo = ((c >> k) & 1u) ? -vi : vi, hi8 = ((c >> (k + 1)) & 1u) ? -vq : vq;
                    *reinterpret_cast<uint16_t *>(dst + n0 + k) = (uint16_t)((lo & 0xFF) | ((hi8 & 0xFF) << 8));
                }
            }
        }
    };
    auto per_mod = [&](auto *dst) __attribute__((always_inline)) {
        switch (al.mod_type) {
        case 1:  run(std::integral_constant<uint32_t, 1>{}, dst); break;
        case 2:  run(std::integral_constant<uint32_t, 2>{}, dst); break;
        default: run(std::integral_constant<uint32_t, 3>{}, dst); break;
        }
    };
    if (via_lds) {
        per_mod(e_lds);
        __syncthreads();
        const uint32_t nq = (N_bits + 15) >> 4; // the allocation's slot in e_base is padded to 64 bytes
        for (uint32_t w = threadIdx.x; w < nq; w += blockDim.x) reinterpret_cast<uint4 *>(e)[w] = reinterpret_cast<const uint4 *>(e_lds)[w];
    } else
        per_mod(e);
}

// The stage tap after a run with the packed hand-over (mi_lte_pdsch_plan_soft_bits): one workgroup per allocation turns a packed slot back into
// the byte form IN PLACE -- all of the allocation's dwords into LDS, a barrier, then the bytes (zeros behind e_len up to the next 16 bytes).
__global__ __launch_bounds__(256) void k_soft_expand(const mi_lte_pdsch_alloc *__restrict__ allocs, int8_t *__restrict__ e_base, const uint32_t *__restrict__ e_off,
                                                     const uint32_t *__restrict__ e_len, uint32_t max_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smu[]; // [max_words] the allocation's dwords
    const uint32_t a_idx = blockIdx.x;
    if (allocs[a_idx].mod_type < 2) return; // (uniform) bytes already
    const uint32_t E = e_len[a_idx], nd = min((E + 31) >> 5, max_words), nq = min((E + 15) >> 4, 2 * max_words);
    int8_t *e = e_base + (size_t)e_off[a_idx] * 64;
    for (uint32_t w = threadIdx.x; w < nd; w += blockDim.x) smu[w] = reinterpret_cast<const uint32_t *>(e)[w];
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < nq; q += blockDim.x) {
        uint32_t w[4];
        soft_stage_quad(smu, q, min(16u, E - 16 * q), w);
        reinterpret_cast<uint4 *>(e)[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

} // namespace

// ------------------------------------------------------------------------------------------------
// host side: plans

struct mi_lte_pdsch_plan {
    mi_lte_dl_cfg cfg;
    MiPlanCore    core;
    uint32_t      decoder = MI_LTE_TURBO_REF, n_iter = 8; // MI_LTE_TURBO_BCJR: mi_lte_pdsch_plan_set_decoder
    int           qpp_spec = 0;
    int8_t       *d_bcjr_soft = nullptr;                  // [max n_cb][3(K+4)] int8 channel values of the group being decoded
    uint8_t      *d_bcjr_bits = nullptr;                  // [max n_cb][K] its hard decisions
    size_t        bcjr_soft_cap = 0, bcjr_bits_cap = 0;
    uint32_t      cfi = 0, max_tbs = 0;
    PdschDemodSizes sizes; // what the demodulator's launch is sized by (pdsch_launch.h)
    bool          dynamic = false, wide = false; // wide: the output stride of the largest single-code-block transport block, whatever is held
    bool          mapped = false; // the descriptor arrays ARE the pinned staging block, mapped into the device (mi_pdsch_plan_create_mapped)
    // pinned staging for re-assignments: allocs | e_off | cb_alloc, copied with one command each on the context's stream
    void       *h_stage = nullptr;
    hipEvent_t  staged = nullptr;
    std::vector<uint8_t>  h_row;    // plan_layout's per-allocation scratch: kept, so that a re-assignment (tens of thousands of allocations per
    std::vector<uint32_t> h_e_bits; // chunk of a capture) allocates nothing
    MiDlsch3   *g3 = nullptr; // 3GPP transport-block mode (mi_lte_pdsch_plan_create_3gpp): its code blocks and buffers (dlsch3gpp.hip)
    uint32_t    demap = MI_LTE_DEMAP_REF; // mi_lte_pdsch_plan_set_demapper (3GPP mode)
    float       demap_gain = 0.0f, *d_llr_gain = nullptr; // MAXLOG: the fixed gain (0: automatic); [n_alloc] the gain of the last run (3GPP plans)
    // mi_lte_pdsch_plan_set_llr_noise: the noise-referenced gain's scale (0: off); the last such run's sigma2 [n_units] (behind d_llr_gain's
    // floats); n_units = 1 + the largest unit an allocation names
    float       llr_noise = 0.0f, *d_llr_s2 = nullptr;
    uint32_t    n_units = 0;
    // the packed hand-over (soft_pack.h): the stage tap's debt -- the context of the last run and whether its 16QAM / 64QAM slots still
    // hold bits (mi_lte_pdsch_plan_soft_bits expands them once; a re-assignment voids them)
    mutable mi_lte_ctx *tap_ctx = nullptr;
    mutable bool        tap_packed = false;
};

static void plan_set_stride(mi_lte_pdsch_plan *pl)
{ // a dynamic plan keeps ONE output stride over its assignments: the largest single-code-block size
    pl->core.out_stride = mi_out_stride((pl->dynamic || pl->wide) ? 6120u : pl->max_tbs, pl->core.packed != 0);
}

// Host side of a plan: check the allocations, lay their soft bits out and group them by code-block size.  Fills everything but the device arrays;
// cb_alloc receives the allocation index of every code-block slot, group after group.  cb_alloc == nullptr: the soft-bit layout alone (the 3GPP
// mode: its code blocks are dlsch3gpp.hip's, and no allocation is outside the envelope for its transport block size).
static int plan_layout(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                       std::vector<uint32_t> *cb_alloc, bool prbs_checked = false)
{
    std::vector<uint8_t>  &row    = pl->h_row;
    std::vector<uint32_t> &e_bits = pl->h_e_bits;
    row.resize(n_alloc);
    e_bits.resize(n_alloc);
    const mi_lte_dl_cfg *cfg = &pl->cfg;
    pl->cfi          = N_pdcch_symbs;
    pl->core.n_alloc = n_alloc;
    pl->max_tbs = 0;
    pl->sizes   = PdschDemodSizes{};
    pl->tap_packed = false; // (the slots move: what a last run left in them is no allocation's any more)
    pl->core.groups.clear();
    for (uint32_t a = 0; a < n_alloc; a++) {
        const mi_lte_pdsch_alloc &al = h_allocs[a];
        const int      r   = cb_alloc ? mi_tb_row(al.tbs) : 0;
        const uint32_t cfi = al.n_pdcch_symbs ? al.n_pdcch_symbs : N_pdcch_symbs;
        if (r < 0 || al.N_prb == 0 || al.N_prb > cfg->N_rb_dl || al.mod_type > 3 || cfi < 1 || cfi > 4) {
            // multi-code-block transport blocks: the reference's own C > 1 path is broken
            ctx->err = "allocation outside the single-code-block envelope (tbs + 24 > 6144) or malformed";
            return MI_LTE_ERR_UNSUPPORTED;
        }
        for (uint32_t s = 0; s < 2 && !prbs_checked; s++) // a resource block past the carrier would be read out of the neighbouring symbol row
            for (uint32_t i = 0; i < al.N_prb; i++)
                if (al.prb[s][i] >= cfg->N_rb_dl) {
                    ctx->err = "allocation names a resource block outside the carrier";
                    return MI_LTE_ERR_INVALID_ARG;
                }
        row[a]      = (uint8_t)r;
        pl->max_tbs = std::max(pl->max_tbs, al.tbs);
        e_bits[a]   = pl->sizes.add(al.N_prb, cfi, al.mod_type);
    }
    if (pl->sizes.max_words > MAX_WORDS) { // the demodulator reads one word past the allocation's last scrambling word
        ctx->err = "allocation larger than the scrambling table";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    pl->core.e_bytes = mi_plan_soft_layout(e_bits.data(), n_alloc, pl->core.h_e_off);
    plan_set_stride(pl);
    if (cb_alloc) mi_plan_group(row.data(), nullptr, e_bits.data(), n_alloc, pl->core.groups, *cb_alloc);
    return MI_LTE_OK;
}

extern "C" {

void mi_lte_pdsch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl);

int mi_lte_pdsch_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs,
                             const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, mi_lte_pdsch_plan **out)
{
    if (!ctx || !cfg || !h_allocs || !out || n_alloc == 0 || N_pdcch_symbs < 1 || N_pdcch_symbs > 4) return MI_LTE_ERR_INVALID_ARG;
    if (!(cfg->N_ant == 1 || cfg->N_ant == 2 || cfg->N_ant == 4)) return MI_LTE_ERR_INVALID_ARG;
    if ((cfg->sample_format & MI_LTE_CE_COMPACT) && cfg->N_ant != 1) { ctx->err = "MI_LTE_CE_COMPACT: single-port cells only"; return MI_LTE_ERR_UNSUPPORTED; }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl      = new mi_lte_pdsch_plan();
    auto  guard   = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_lte_pdsch_plan_destroy(nullptr, pl); });
    pl->cfg       = *cfg;
    std::vector<uint32_t> cb_alloc;
    int rc = plan_layout(ctx, pl, N_pdcch_symbs, h_allocs, n_alloc, &cb_alloc);
    if (rc != MI_LTE_OK) return rc;
    MI_HIP_CHECK(ctx, pl->core.allocate(n_alloc, pl->core.e_bytes));
    MI_H2D(ctx, pl->core.d_allocs, h_allocs, sizeof(mi_lte_pdsch_alloc) * n_alloc);
    MI_H2D(ctx, pl->core.d_e_off, pl->core.h_e_off.data(), sizeof(uint32_t) * n_alloc);
    MI_H2D(ctx, pl->core.d_cb_alloc, cb_alloc.data(), sizeof(uint32_t) * n_alloc);
    MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx));
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}

// A plan whose allocation list changes from run to run (a capture: every subframe has its own DCIs, LTE_fdd_dl_fs_samp_buf.cc:445-515):
// device arrays and pinned staging sized once, mi_lte_pdsch_plan_assign re-plans inside them with three asynchronous copies and no
// allocation, no wait.
int mi_lte_pdsch_plan_create_dynamic(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t max_alloc, size_t max_soft_bytes, mi_lte_pdsch_plan **out)
{
    if (!ctx || !cfg || !out || max_alloc == 0) return MI_LTE_ERR_INVALID_ARG;
    if (!(cfg->N_ant == 1 || cfg->N_ant == 2 || cfg->N_ant == 4)) return MI_LTE_ERR_INVALID_ARG;
    if ((cfg->sample_format & MI_LTE_CE_COMPACT) && cfg->N_ant != 1) { ctx->err = "MI_LTE_CE_COMPACT: single-port cells only"; return MI_LTE_ERR_UNSUPPORTED; }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl    = new mi_lte_pdsch_plan();
    auto  guard = on_fail([&] { mi_lte_pdsch_plan_destroy(nullptr, pl); });
    pl->cfg     = *cfg;
    pl->dynamic = true;
    // the capacity a multiple of four entries: the staging block's three arrays (260-byte structs, then two uint32 arrays) then all start on 16
    // bytes whatever the caller asked for, which is what the copy kernel of mi_pdsch_plan_assign_slice needs (otherwise three copy commands)
    max_alloc = (max_alloc + 3u) & ~3u;
    MI_HIP_CHECK(ctx, pl->core.allocate(max_alloc, (max_soft_bytes + 63) & ~(size_t)63));
    MI_HIP_CHECK(ctx, hipHostMalloc(&pl->h_stage, (sizeof(mi_lte_pdsch_alloc) + 2 * sizeof(uint32_t)) * (size_t)max_alloc, hipHostMallocDefault));
    MI_HIP_CHECK(ctx, hipEventCreateWithFlags(&pl->staged, hipEventDisableTiming));
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}
} // extern "C"

// The per-call forms' variant of a dynamic plan (hostapi.cc: a handful of allocations per subframe): the three descriptor arrays are not
// copied at all -- they live in pinned host memory mapped into the device, mi_lte_pdsch_plan_assign stores into it and the kernels read
// the few hundred bytes over the link (a copy command costs more API time than that).  Contract: the caller waits for the stream between a
// run of the plan and its next assignment (every per-call form ends with a wait).
int mi_pdsch_plan_create_mapped(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t max_alloc, size_t max_soft_bytes, mi_lte_pdsch_plan **out)
{
    if (!ctx || !cfg || !out || max_alloc == 0 || max_alloc > 64) return MI_LTE_ERR_INVALID_ARG;
    if (!(cfg->N_ant == 1 || cfg->N_ant == 2 || cfg->N_ant == 4) || (cfg->sample_format & MI_LTE_CE_COMPACT)) return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl    = new mi_lte_pdsch_plan();
    auto  guard = on_fail([&] { mi_lte_pdsch_plan_destroy(nullptr, pl); });
    pl->cfg     = *cfg;
    pl->dynamic = pl->mapped = true;
    MI_HIP_CHECK(ctx, hipHostMalloc(&pl->h_stage, (sizeof(mi_lte_pdsch_alloc) + 2 * sizeof(uint32_t)) * (size_t)max_alloc, hipHostMallocMapped | hipHostMallocCoherent));
    void *d_stage = nullptr;
    MI_HIP_CHECK(ctx, hipHostGetDevicePointer(&d_stage, pl->h_stage, 0));
    MI_HIP_CHECK(ctx, pl->core.allocate(max_alloc, (max_soft_bytes + 63) & ~(size_t)63, d_stage));
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}

// what the demodulator asks of one allocation, whatever its transport block is cut into
static bool alloc_geometry_ok(const mi_lte_dl_cfg *cfg, const mi_lte_pdsch_alloc *al, uint32_t N_pdcch_symbs)
{
    const uint32_t cfi = al->n_pdcch_symbs ? al->n_pdcch_symbs : N_pdcch_symbs;
    if (al->N_prb == 0 || al->N_prb > cfg->N_rb_dl || al->N_prb > 110 || al->mod_type > 3 || cfi < 1 || cfi > 4) return false;
    if ((14 - cfi) * al->N_prb * 12 * (al->mod_type == 3 ? 6u : al->mod_type == 2 ? 4u : al->mod_type == 1 ? 2u : 1u) > 4095u * 32u) return false; // the scrambling table
    for (uint32_t s = 0; s < 2; s++)
        for (uint32_t i = 0; i < al->N_prb; i++)
            if (al->prb[s][i] >= cfg->N_rb_dl) return false;
    return true;
}

extern "C" {

int mi_lte_pdsch_alloc_decodable(const mi_lte_dl_cfg *cfg, const mi_lte_pdsch_alloc *al, uint32_t N_pdcch_symbs)
{ // the per-allocation conditions of plan_layout, for callers that must not lose a whole list to one chance-CRC DCI
    return cfg && al && al->tbs + 24 <= 6144 && al->tbs + 24 >= al->tbs && alloc_geometry_ok(cfg, al, N_pdcch_symbs);
}

int mi_lte_pdsch_alloc_decodable_3gpp(const mi_lte_dl_cfg *cfg, const mi_lte_dlsch_cfg *dlsch, const mi_lte_pdsch_alloc *al, uint32_t N_pdcch_symbs)
{ // mi_lte_pdsch_alloc_decodable's conditions with the 3GPP segmentation in place of the single-block one
    if (!cfg || !dlsch || !al || cfg->N_ant != 1 || al->mod_type == 0 || al->mod_type > 3) return 0;
    mi_lte_dlsch_layout_t lay;
    if (mi_lte_dlsch_layout(al->tbs, 0, 2, al->tx_mode, al->rv_idx & 3u, dlsch, &lay) != MI_LTE_OK) return 0;
    return alloc_geometry_ok(cfg, al, N_pdcch_symbs);
}

int mi_lte_pdsch_alloc_decodable_3gpp_txdiv(const mi_lte_dl_cfg *cfg, const mi_lte_dlsch_cfg *dlsch, const mi_lte_pdsch_alloc *al, uint32_t N_pdcch_symbs)
{ // the same for mi_lte_pdsch_plan_create_3gpp_txdiv: two or four ports, transmit diversity, full estimate planes
    if (!cfg || !dlsch || !al || !(cfg->N_ant == 2 || cfg->N_ant == 4) || (cfg->sample_format & MI_LTE_CE_COMPACT)) return 0;
    if (al->tx_mode != 2 || al->mod_type == 0 || al->mod_type > 3) return 0;
    mi_lte_dlsch_layout_t lay;
    if (mi_lte_dlsch_layout_nl(al->tbs, 0, 2, 2, al->tx_mode, al->rv_idx & 3u, dlsch, &lay) != MI_LTE_OK) return 0;
    return alloc_geometry_ok(cfg, al, N_pdcch_symbs);
}

} // extern "C"

// A static plan in the 3GPP transport-block mode: the demodulator's layout is that of any plan -- it does not depend on the transport block
// size -- and the code blocks are dlsch3gpp.hip's.
// n_l: N_L of the code-block concatenation -- 1: a single-port cell (mi_lte_pdsch_plan_create_3gpp), 2: transmit diversity on the cell's two or
// four ports (mi_lte_pdsch_plan_create_3gpp_txdiv).  The callers have checked the port count.
static int plan_create_3gpp(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs, const mi_lte_dlsch_cfg *dlsch, const mi_lte_pdsch_alloc *h_allocs,
                            uint32_t n_alloc, uint32_t n_l, mi_lte_pdsch_plan **out)
{
    for (uint32_t a = 0; a < n_alloc; a++) {
        mi_lte_dlsch_layout_t lay;
        const int rc = h_allocs[a].mod_type == 0 ? MI_LTE_ERR_UNSUPPORTED : mi_lte_dlsch_layout(h_allocs[a].tbs, 0, 2, h_allocs[a].tx_mode, h_allocs[a].rv_idx & 3u, dlsch, &lay);
        if (rc != MI_LTE_OK) { ctx->err = "allocation outside the 3GPP transport-block mode (BPSK, F != 0, tbs > 75376 or a soft buffer under 2 positions)"; return rc; }
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl    = new mi_lte_pdsch_plan();
    auto  guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_lte_pdsch_plan_destroy(nullptr, pl); });
    pl->cfg     = *cfg;
    pl->decoder = MI_LTE_TURBO_BCJR; pl->n_iter = 8; pl->qpp_spec = 1;
    int rc = plan_layout(ctx, pl, N_pdcch_symbs, h_allocs, n_alloc, nullptr);
    if (rc != MI_LTE_OK) return rc;
    MI_HIP_CHECK(ctx, pl->core.allocate(n_alloc, pl->core.e_bytes));
    rc = mi_dlsch3_create(ctx, dlsch, h_allocs, n_alloc, &pl->g3, n_l);
    if (rc != MI_LTE_OK) return rc;
    for (uint32_t a = 0; a < n_alloc; a++) pl->n_units = std::max(pl->n_units, h_allocs[a].unit + 1u);
    MI_HIP_CHECK(ctx, hipMalloc((void **)&pl->d_llr_gain, sizeof(float) * ((size_t)n_alloc + pl->n_units))); // gain [n_alloc] | sigma2 [n_units]
    MI_HIP_CHECK(ctx, hipMemsetAsync(pl->d_llr_gain, 0, sizeof(float) * ((size_t)n_alloc + pl->n_units), ctx->stream));
    pl->d_llr_s2 = pl->d_llr_gain + n_alloc;
    MI_H2D(ctx, pl->core.d_allocs, h_allocs, sizeof(mi_lte_pdsch_alloc) * n_alloc);
    MI_H2D(ctx, pl->core.d_e_off, pl->core.h_e_off.data(), sizeof(uint32_t) * n_alloc);
    MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx));
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}

extern "C" {

int mi_lte_pdsch_plan_create_3gpp(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs, const mi_lte_dlsch_cfg *dlsch,
                                  const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, mi_lte_pdsch_plan **out)
{
    if (!ctx || !cfg || !dlsch || !h_allocs || !out || n_alloc == 0 || N_pdcch_symbs < 1 || N_pdcch_symbs > 4 || dlsch->M_dl_harq == 0) return MI_LTE_ERR_INVALID_ARG;
    if (cfg->N_ant != 1) { ctx->err = "3GPP transport-block mode: single-port cells only (two or four ports: mi_lte_pdsch_plan_create_3gpp_txdiv)"; return MI_LTE_ERR_UNSUPPORTED; }
    return plan_create_3gpp(ctx, cfg, N_pdcch_symbs, dlsch, h_allocs, n_alloc, 1, out);
}

// The same mode on a cell of two or four CRS ports: every allocation in transmit diversity (36.211 6.3.3.3 / 6.3.4.3, tx_mode 2).  The default
// demapper is the reference-mode plans' k_pdsch_demod<false>, MAXLOG is k_pdsch_demod_llr<2 | 4> (labelled k_pdsch_demod_llr_txd), and the code-block concatenation runs with N_L = 2.
int mi_lte_pdsch_plan_create_3gpp_txdiv(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs, const mi_lte_dlsch_cfg *dlsch,
                                        const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, mi_lte_pdsch_plan **out)
{
    if (!ctx || !cfg || !dlsch || !h_allocs || !out || n_alloc == 0 || N_pdcch_symbs < 1 || N_pdcch_symbs > 4 || dlsch->M_dl_harq == 0) return MI_LTE_ERR_INVALID_ARG;
    if (!(cfg->N_ant == 1 || cfg->N_ant == 2 || cfg->N_ant == 4)) return MI_LTE_ERR_INVALID_ARG;
    if (cfg->N_ant == 1) { ctx->err = "transmit-diversity plan: two or four ports (one port: mi_lte_pdsch_plan_create_3gpp)"; return MI_LTE_ERR_UNSUPPORTED; }
    if (cfg->sample_format & MI_LTE_CE_COMPACT) { ctx->err = "MI_LTE_CE_COMPACT: single-port cells only"; return MI_LTE_ERR_UNSUPPORTED; }
    for (uint32_t a = 0; a < n_alloc; a++)
        if (h_allocs[a].tx_mode != 2) { ctx->err = "transmit-diversity plan: every allocation must have tx_mode 2"; return MI_LTE_ERR_UNSUPPORTED; }
    return plan_create_3gpp(ctx, cfg, N_pdcch_symbs, dlsch, h_allocs, n_alloc, 2, out);
}

int mi_lte_pdsch_plan_cb_soft(const mi_lte_pdsch_plan *pl, uint32_t alloc, const int8_t **d_blocks, uint32_t *C, uint32_t *K)
{
    if (!pl || !pl->g3) return MI_LTE_ERR_INVALID_ARG;
    return mi_dlsch3_cb_soft(pl->g3, alloc, d_blocks, C, K);
}

int mi_lte_pdsch_plan_cb_ok(const mi_lte_pdsch_plan *pl, const uint32_t **d_mask)
{
    if (!pl || !pl->g3 || !d_mask) return MI_LTE_ERR_INVALID_ARG;
    *d_mask = mi_dlsch3_cb_ok(pl->g3);
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_assign(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc)
{
    if (!ctx || !pl || !pl->dynamic || !h_allocs || n_alloc == 0 || N_pdcch_symbs < 1 || N_pdcch_symbs > 4) return MI_LTE_ERR_INVALID_ARG;
    if (n_alloc > pl->core.cap_alloc) { ctx->err = "more allocations than the dynamic plan was created for"; return MI_LTE_ERR_INVALID_ARG; }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<uint32_t> cb_alloc;
    int rc = plan_layout(ctx, pl, N_pdcch_symbs, h_allocs, n_alloc, &cb_alloc);
    if (rc != MI_LTE_OK) { pl->core.n_alloc = 0; return rc; }
    if (pl->core.e_bytes > pl->core.cap_e_bytes) { pl->core.n_alloc = 0; ctx->err = "more soft bits than the dynamic plan was created for"; return MI_LTE_ERR_INVALID_ARG; }
    if (!pl->mapped) MI_HIP_CHECK(ctx, hipEventSynchronize(pl->staged)); // the previous assignment's copies have left the staging block
    auto *sa = (mi_lte_pdsch_alloc *)pl->h_stage;
    auto *so = (uint32_t *)(sa + pl->core.cap_alloc), *sc = so + pl->core.cap_alloc;
    memcpy(sa, h_allocs, sizeof(mi_lte_pdsch_alloc) * n_alloc);
    memcpy(so, pl->core.h_e_off.data(), sizeof(uint32_t) * n_alloc);
    memcpy(sc, cb_alloc.data(), sizeof(uint32_t) * n_alloc);
    if (pl->mapped) return MI_LTE_OK; // the kernels read the block itself (mi_pdsch_plan_create_mapped: the caller has waited for the last run)
    MI_HIP_CHECK(ctx, hipMemcpyAsync(pl->core.d_allocs, sa, sizeof(mi_lte_pdsch_alloc) * n_alloc, hipMemcpyHostToDevice, ctx->stream));
    MI_HIP_CHECK(ctx, hipMemcpyAsync(pl->core.d_e_off, so, sizeof(uint32_t) * n_alloc, hipMemcpyHostToDevice, ctx->stream));
    MI_HIP_CHECK(ctx, hipMemcpyAsync(pl->core.d_cb_alloc, sc, sizeof(uint32_t) * n_alloc, hipMemcpyHostToDevice, ctx->stream));
    MI_HIP_CHECK(ctx, hipEventRecord(pl->staged, ctx->stream));
    return MI_LTE_OK;
}

uint32_t mi_lte_pdsch_plan_n_alloc(const mi_lte_pdsch_plan *pl) { return pl ? pl->core.n_alloc : 0; }
} // extern "C"

// The host pipeline's assignment (pipeline.cc: one per chunk of a capture, tens of thousands of allocations each, on the thread that also
// feeds the copy engines): the chunk's slice of the caller's list goes into the plan's staging block in ONE pass -- unit numbers made
// chunk-local, every allocation tested once (mi_lte_pdsch_alloc_decodable's conditions), one outside the envelope replaced by a one-block
// QPSK stand-in and its index reported -- instead of a copy, a test pass and the layout's own test pass.
// copy_stream: where the three descriptor copies go (nullptr: the context's stream).  The pipeline passes its input-copy stream: a third
// engine moving 4.8 MB per chunk next to the sample and result copies slowed both (profiles/r05_host_pipeline_profile.txt, section 5).
int mi_pdsch_plan_assign_slice(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_src, uint32_t n_alloc, uint32_t unit0,
                               std::vector<uint32_t> *refused, hipStream_t copy_stream)
{
    if (!ctx || !pl || !pl->dynamic || pl->mapped || !h_src || n_alloc == 0 || N_pdcch_symbs < 1 || N_pdcch_symbs > 4) return MI_LTE_ERR_INVALID_ARG;
    const hipStream_t cs = copy_stream ? copy_stream : ctx->stream;
    if (n_alloc > pl->core.cap_alloc) { ctx->err = "more allocations than the dynamic plan was created for"; return MI_LTE_ERR_INVALID_ARG; }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MI_HIP_CHECK(ctx, hipEventSynchronize(pl->staged)); // the previous assignment's copies have left the staging block
    auto *sa = (mi_lte_pdsch_alloc *)pl->h_stage;
    auto *so = (uint32_t *)(sa + pl->core.cap_alloc), *sc = so + pl->core.cap_alloc;
    for (uint32_t i = 0; i < n_alloc; i++) {
        mi_lte_pdsch_alloc &a = sa[i];
        a = h_src[i];
        a.unit -= unit0;
        if (!mi_lte_pdsch_alloc_decodable(&pl->cfg, &a, N_pdcch_symbs)) {
            // a DCI that passed its CRC by chance: the reference fails that one allocation (liblte_phy.cc:3690-3853); the slot keeps its place
            a.N_prb = 1; a.prb[0][0] = a.prb[1][0] = 0; a.mod_type = 1; a.tbs = 16; a.rv_idx = 0; a.tx_mode = pl->cfg.N_ant == 1 ? 1 : 2;
            if (a.n_pdcch_symbs > 4) a.n_pdcch_symbs = 0;
            if (refused) refused->push_back(i);
        }
    }
    std::vector<uint32_t> cb_alloc;
    int rc = plan_layout(ctx, pl, N_pdcch_symbs, sa, n_alloc, &cb_alloc, true);
    if (rc != MI_LTE_OK) { pl->core.n_alloc = 0; return rc; }
    if (pl->core.e_bytes > pl->core.cap_e_bytes) { pl->core.n_alloc = 0; ctx->err = "more soft bits than the dynamic plan was created for"; return MI_LTE_ERR_INVALID_ARG; }
    memcpy(so, pl->core.h_e_off.data(), sizeof(uint32_t) * n_alloc);
    memcpy(sc, cb_alloc.data(), sizeof(uint32_t) * n_alloc);
    // The three arrays leave the (pinned) staging block with a copy KERNEL on the same stream, not with copy commands: the runtime rotates its
    // copy engines from command to command, and three small commands per chunk between the sample copies put every third chunk's samples on
    // the engine the result copy of the chunk before was using -- a 3.1 ms + 1.0 ms pair where 2.4 + 0.3 is the rule
    // (profiles/r05_host_pipeline_profile.txt section 6, and section 7 for this)
    static const bool slice_by_engine = getenv("MI_LTE_SLICE_COPY_COMMANDS") != nullptr; // (A/B switch)
    if (slice_by_engine) {
        MI_HIP_CHECK(ctx, hipMemcpyAsync(pl->core.d_allocs, sa, sizeof(mi_lte_pdsch_alloc) * n_alloc, hipMemcpyHostToDevice, cs));
        MI_HIP_CHECK(ctx, hipMemcpyAsync(pl->core.d_e_off, so, sizeof(uint32_t) * n_alloc, hipMemcpyHostToDevice, cs));
        MI_HIP_CHECK(ctx, hipMemcpyAsync(pl->core.d_cb_alloc, sc, sizeof(uint32_t) * n_alloc, hipMemcpyHostToDevice, cs));
    } else {
        const MiCopySeg segs[3] = {{pl->core.d_allocs, sa, sizeof(mi_lte_pdsch_alloc) * n_alloc}, {pl->core.d_e_off, so, sizeof(uint32_t) * n_alloc}, {pl->core.d_cb_alloc, sc, sizeof(uint32_t) * n_alloc}};
        MI_HIP_CHECK(ctx, mi_pinned_segments_to_device(ctx, segs, 3, cs));
    }
    MI_HIP_CHECK(ctx, hipEventRecord(pl->staged, cs));
    return MI_LTE_OK;
}
void mi_pdsch_plan_wide_stride(mi_lte_pdsch_plan *pl) { pl->wide = true; plan_set_stride(pl); }
extern "C" {

void mi_lte_pdsch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl)
{
    if (!pl) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    pl->core.release(); // (mapped: the three descriptor arrays are views of h_stage)
    if (pl->d_bcjr_soft) (void)hipFree(pl->d_bcjr_soft);
    if (pl->d_bcjr_bits) (void)hipFree(pl->d_bcjr_bits);
    if (pl->d_llr_gain) (void)hipFree(pl->d_llr_gain);
    if (pl->h_stage) (void)hipHostFree(pl->h_stage);
    if (pl->staged) (void)hipEventDestroy(pl->staged);
    mi_dlsch3_free(pl->g3);
    delete pl;
}

uint32_t mi_lte_pdsch_plan_out_stride(const mi_lte_pdsch_plan *pl) { return pl ? pl->core.out_stride : 0; }

// the de-mappers' atan2f (phy_dev.hpp: the host libm's algorithm restated) evaluated on the host, for the test that pins it to libm
int mi_lte_model_atan2f(const float *h_y, const float *h_x, float *h_out, size_t n)
{
    if (!h_y || !h_x || !h_out) return MI_LTE_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; i++) h_out[i] = ref_atan2f(h_y[i], h_x[i]);
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_soft_bits(const mi_lte_pdsch_plan *pl, uint32_t alloc, const int8_t **d_e, const uint32_t **d_len)
{
    if (!pl || alloc >= pl->core.n_alloc || !d_e || !d_len) return MI_LTE_ERR_INVALID_ARG;
    if (pl->tap_packed) { // the last run handed its 16QAM / 64QAM soft bits over as bits: the first tap after it turns them into bytes, once
        mi_lte_ctx *ctx = pl->tap_ctx;
        MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        hipLaunchKernelGGL(k_soft_expand, dim3(pl->core.n_alloc), dim3(256), sizeof(uint32_t) * (pl->sizes.max_words + 4u), ctx->stream, pl->core.d_allocs, pl->core.d_e,
                           pl->core.d_e_off, pl->core.d_e_len, pl->sizes.max_words);
        MI_HIP_CHECK(ctx, hipGetLastError());
        pl->tap_packed = false;
    }
    *d_e   = pl->core.d_e + (size_t)pl->core.h_e_off[alloc] * 64;
    *d_len = pl->core.d_e_len + alloc;
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_set_decoder(mi_lte_pdsch_plan *pl, uint32_t mode, uint32_t n_iter, int qpp_spec)
{
    const bool bcjr = mi_is_bcjr(mode);
    if (!pl || !(mode == MI_LTE_TURBO_REF || bcjr) || (bcjr && (n_iter == 0 || n_iter > 64))) return MI_LTE_ERR_INVALID_ARG;
    if (pl->g3 && mode == MI_LTE_TURBO_REF) return MI_LTE_ERR_UNSUPPORTED; // (the 3GPP mode: BCJR decoders, exact interleaver)
    if (pl->g3 && !qpp_spec) return MI_LTE_ERR_INVALID_ARG;
    pl->decoder = mode; pl->n_iter = n_iter; pl->qpp_spec = qpp_spec;
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_set_demapper(mi_lte_pdsch_plan *pl, uint32_t mode, float gain)
{
    if (!pl || mode > MI_LTE_DEMAP_MAXLOG) return MI_LTE_ERR_INVALID_ARG;
    if (mode == MI_LTE_DEMAP_REF) { pl->demap = MI_LTE_DEMAP_REF; return MI_LTE_OK; }
    if (!(gain >= 0.0f) || gain > 3.4028234e38f) return MI_LTE_ERR_INVALID_ARG; // negative, NaN or infinite
    if (!pl->g3 || (pl->cfg.sample_format & MI_LTE_CE_COMPACT)) return MI_LTE_ERR_UNSUPPORTED;
    pl->demap = mode; pl->demap_gain = gain;
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_llr_gain(const mi_lte_pdsch_plan *pl, const float **d_gain)
{
    if (!pl || !d_gain || !pl->d_llr_gain) return MI_LTE_ERR_INVALID_ARG;
    *d_gain = pl->d_llr_gain;
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_set_llr_noise(mi_lte_pdsch_plan *pl, float scale)
{
    if (!pl || !(scale >= 0.0f) || scale > 3.4028234e38f) return MI_LTE_ERR_INVALID_ARG; // negative, NaN or infinite
    if (!pl->g3) return MI_LTE_ERR_UNSUPPORTED; // a reference-mode plan has no LLR to scale
    pl->llr_noise = scale;
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_llr_noise(const mi_lte_pdsch_plan *pl, const float **d_sigma2, uint32_t *n_units)
{
    if (!pl || !d_sigma2 || !n_units || !pl->d_llr_s2) return MI_LTE_ERR_INVALID_ARG;
    *d_sigma2 = pl->d_llr_s2;
    *n_units  = pl->n_units;
    return MI_LTE_OK;
}

int mi_lte_pdsch_plan_set_output(mi_lte_pdsch_plan *pl, uint32_t packed)
{
    if (!pl) return MI_LTE_ERR_INVALID_ARG;
    pl->core.packed = packed ? 1u : 0u;
    plan_set_stride(pl);
    return MI_LTE_OK;
}

} // extern "C"

// The scrambling words' A/B switch (gold_run.h): the contexts that were told which method to run, every other one follows the environment.
// It lives here and not in mi_lte_ctx for the reason given below for mi_dl_crs_noise; mi_lte_ctx_destroy (ctx.cc) calls mi_chain_ctx_release.
namespace {
std::mutex                         g_gold_mu;
std::map<const mi_lte_ctx *, bool> g_gold_table; // context -> word by word from the tables (the method before gold_run.h)
bool gold_table_of(const mi_lte_ctx *ctx)
{
    static const bool env_table = [] { const char *e = getenv("MI_LTE_NO_GOLD_RUN"); return e && atoi(e) != 0; }();
    std::lock_guard<std::mutex> lk(g_gold_mu);
    const auto it = g_gold_table.find(ctx);
    return it == g_gold_table.end() ? env_table : it->second;
}
} // namespace
extern "C" int mi_lte_set_gold_recurrence(mi_lte_ctx *ctx, uint32_t on)
{
    if (!ctx) return MI_LTE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(g_gold_mu);
    g_gold_table[ctx] = on == 0;
    return MI_LTE_OK;
}
void mi_chain_ctx_release(const mi_lte_ctx *ctx)
{
    std::lock_guard<std::mutex> lk(g_gold_mu);
    g_gold_table.erase(ctx);
}

// dl_noise.hip: k_dl_crs_noise on the context's stream; it checks the bandwidth and the port count.  (Declared here and not in ctx.hpp: the
// shared headers are part of every file's build id, and the committed profiler tables of the other files stay current this way.)
int mi_dl_crs_noise(mi_lte_ctx *ctx, uint32_t N_rb_dl, uint32_t N_ant, const float *d_subframes, const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell,
                    uint32_t n_units, float *d_sigma2);

template <PdschFamily F> using Family = std::integral_constant<PdschFamily, F>; // the planned family as a template argument

// What a demodulator launch reads besides the plan and the planned launch
struct PdschDemodIn {
    const float    *d_subframes;
    const uint32_t *d_subfr_num, *d_n_id_cell;
    float           auto_t; // the automatic gain's target (max-log)
};

// The demodulator's launch as L shapes it: family F on N_ANT ports.  The kernel is instantiated only where pdsch_variant_compiled
// (pdsch_launch.h) says the variant exists; pdsch_launch_plan plans nothing else, so the other branch is never reached.
template <PdschFamily F, uint32_t N_ANT>
static int pdsch_launch(mi_lte_ctx *ctx, const mi_lte_pdsch_plan *pl, const PdschLaunch &L, const PdschDemodIn &in)
{
    if constexpr (pdsch_variant_compiled(F, N_ANT)) {
        const DemodGeom  g{pl->cfg.N_rb_dl, pl->cfg.N_ant, pl->cfi, (uint32_t)mi_lte_subframe_floats(pl->cfg.N_ant)};
        const GoldTables gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
        const auto go = [&](auto kernel, auto... tail) { // the arguments every variant shares, then its own
            MI_LAUNCH(ctx, L.label, kernel, dim3(pl->core.n_alloc), dim3(L.threads), L.lds_bytes, in.d_subframes, g, pl->core.d_allocs, in.d_subfr_num,
                      in.d_n_id_cell, gt, pl->core.d_e, pl->core.d_e_off, pl->core.d_e_len, pl->sizes.max_pairs, L.words_al, L.e_cap, tail...);
        };
        const uint32_t gold_table = (L.flags & DEMOD_GOLD_TABLE) ? 1u : 0u;
        if constexpr (F == PdschFamily::LLR) go(k_pdsch_demod_llr<N_ANT, PdschLlrGain>, pl->demap_gain, in.auto_t, pl->d_llr_gain, gold_table, PdschLlrGain{});
        else if constexpr (F == PdschFamily::LLR_NOISE)
            go(k_pdsch_demod_llr<N_ANT, PdschLlrNoise>, pl->demap_gain, in.auto_t, pl->d_llr_gain, gold_table, PdschLlrNoise{pl->d_llr_s2, pl->llr_noise});
        else go(k_pdsch_demod<F != PdschFamily::REF_PORTS, F == PdschFamily::REF_ONE_PORT_COMPACT>, L.flags);
        return MI_LTE_OK;
    } else { ctx->err = "k_pdsch_demod: no such variant at this port count"; return MI_LTE_ERR_UNSUPPORTED; }
}

// the plan's demodulator: every allocation's descrambled soft bits and their count, launched as pdsch_launch_plan (pdsch_launch.h) shapes it;
// *L: that launch.  pack: 16QAM / 64QAM allocations leave as bits (soft_pack.h; pdsch_run decides per run)
static int pdsch_demod(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, const float *d_subframes, const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell, bool pack,
                       PdschLaunch *L)
{
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = mi_ctx_gold_tables(ctx);
    if (rc != MI_LTE_OK) return rc;
    const char *ev = getenv("MI_LTE_PDSCH_THREADS"); // (tuning aid)
    const bool  maxlog = pl->demap == MI_LTE_DEMAP_MAXLOG; // (a 3GPP plan on full estimate planes: mi_lte_pdsch_plan_set_demapper)
    pdsch_launch_plan(pl->sizes, pl->cfg.N_ant, (pl->cfg.sample_format & MI_LTE_CE_COMPACT) != 0, maxlog, pl->llr_noise > 0.0f, pack, gold_table_of(ctx),
                      ev ? atoi(ev) : 0, L);
    PdschDemodIn in{d_subframes, d_subfr_num, d_n_id_cell, (float)MI_LTE_DEMAP_AUTO_T};
    if (maxlog)
        if (const char *ev_t = getenv("MI_LTE_DEMAP_AUTO_T")) { // (tuning aid: tools/demap_llr_sweep.py chooses the header's constant with it)
            const float t = (float)atof(ev_t);
            if (t >= 1.0f && t <= 127.0f) in.auto_t = t;
        }
    // the noise-referenced gain: the CRS noise estimate of the plan's units, then the instantiation that divides by it
    if (L->noise_first && (rc = mi_dl_crs_noise(ctx, pl->cfg.N_rb_dl, pl->cfg.N_ant, d_subframes, d_subfr_num, d_n_id_cell, pl->n_units, pl->d_llr_s2)) != MI_LTE_OK)
        return rc;
    const auto ports = [&](auto f) { // L's family on L's ports
        constexpr PdschFamily F = decltype(f)::value;
        return L->n_ant == 1 ? pdsch_launch<F, 1>(ctx, pl, *L, in) : L->n_ant == 2 ? pdsch_launch<F, 2>(ctx, pl, *L, in) : pdsch_launch<F, 4>(ctx, pl, *L, in);
    };
    switch (L->family) {
    case PdschFamily::REF_ONE_PORT: rc = ports(Family<PdschFamily::REF_ONE_PORT>{}); break;
    case PdschFamily::REF_ONE_PORT_COMPACT: rc = ports(Family<PdschFamily::REF_ONE_PORT_COMPACT>{}); break;
    case PdschFamily::REF_PORTS: rc = ports(Family<PdschFamily::REF_PORTS>{}); break;
    case PdschFamily::LLR: rc = ports(Family<PdschFamily::LLR>{}); break;
    case PdschFamily::LLR_NOISE: rc = ports(Family<PdschFamily::LLR_NOISE>{}); break;
    }
    if (rc != MI_LTE_OK) return rc;
    MI_HIP_CHECK(ctx, hipGetLastError());
    return MI_LTE_OK;
}

// The reference-mode plans' BCJR decoders (mi_lte_pdsch_plan_set_decoder): the code blocks size by size
static int pdsch_bcjr_decode(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, const MiDecodeIO &io)
{
    int    rc;
    size_t soft = 0, bits = 0;
    for (auto &gr : pl->core.groups) { soft = std::max(soft, (size_t)gr.n_cb * 3 * (gr.K + 4)); bits = std::max(bits, (size_t)gr.n_cb * gr.K); }
    if (soft > pl->bcjr_soft_cap || bits > pl->bcjr_bits_cap) { // first run, or a re-assigned plan that needs more
        MI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (pl->d_bcjr_soft) (void)hipFree(pl->d_bcjr_soft);
        if (pl->d_bcjr_bits) (void)hipFree(pl->d_bcjr_bits);
        pl->d_bcjr_soft = nullptr; pl->d_bcjr_bits = nullptr;
        MI_HIP_CHECK(ctx, hipMalloc((void **)&pl->d_bcjr_soft, soft));
        MI_HIP_CHECK(ctx, hipMalloc((void **)&pl->d_bcjr_bits, bits));
        pl->bcjr_soft_cap = soft; pl->bcjr_bits_cap = bits;
    }
    for (auto &gr : pl->core.groups) {
        rc = mi_turbo_bcjr_group(ctx, gr, io, pl->d_bcjr_soft, pl->d_bcjr_bits, pl->decoder, pl->n_iter, pl->qpp_spec);
        if (rc != MI_LTE_OK) return rc;
    }
    // (what mi_turbo_bcjr_group launched: the one-block-per-wavefront decoder takes the interleaved int8 block, the batch kernels their granule arrays)
    ctx->last_kernels = pl->decoder == MI_LTE_TURBO_BCJR_BLOCK ? "k_rm_to_i8,k_bcjr_block,k_crc_finish per block size"
                                                               : "k_cb_desc,k_rm_bcjr_prep,k_bcjr_half,k_bcjr_final,k_crc_finish per block size";
    return MI_LTE_OK;
}

// A plan run: demodulation, then the 3GPP mode's decode (dlsch3gpp.hip) or the code blocks size by size (BCJR decoders) or through the REF
// dispatch (turbo.hip).  pool / h_bind: a HARQ run (mi_lte_pdsch_decode_run_harq), nullptr otherwise.  Every refusal returns before a launch.
static int pdsch_run(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, mi_lte_harq_pool *pool, const mi_lte_harq_bind *h_bind, const float *d_subframes,
                     const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell, uint8_t *d_out_bits, int32_t *d_status)
{
    if (!ctx || !pl || !d_subframes || !d_subfr_num || !d_n_id_cell || !d_out_bits || !d_status) return MI_LTE_ERR_INVALID_ARG;
    int rc;
    if (pool) {
        if (!pl->g3) { ctx->err = "HARQ soft combining needs a plan in the 3GPP transport-block mode"; return MI_LTE_ERR_UNSUPPORTED; }
        if ((rc = mi_dlsch3_harq_check(ctx, pl->g3, pool, h_bind)) != MI_LTE_OK) return rc;
    }
    if (pl->core.n_alloc == 0) { ctx->err = "the dynamic plan holds no allocations (mi_lte_pdsch_plan_assign)"; return MI_LTE_ERR_INVALID_ARG; }
    // The packed hand-over (soft_pack.h), decided per run -- the decoder may change between two of them: only where the soft bits go to
    // mi_turbo_ref_dispatch and nowhere else.  The BCJR decoders, the 3GPP mode (HARQ and the max-log demapper with it) keep bytes.
    // Nor does a run one of whose block-size groups would be gathered straight from global memory (mi_turbo_ref_reads_packed).
    bool pack = ctx->soft_packed && !pl->g3 && !mi_is_bcjr(pl->decoder) && pl->demap == MI_LTE_DEMAP_REF;
    for (const MiKGroup &gr : pl->core.groups) pack = pack && turbo_geom::mi_turbo_ref_reads_packed(gr.K, gr.e_max);
    PdschLaunch L;
    if ((rc = pdsch_demod(ctx, pl, d_subframes, d_subfr_num, d_n_id_cell, pack, &L)) != MI_LTE_OK) return rc;
    pl->tap_ctx = ctx; pl->tap_packed = pack; // what the slots hold from here on (mi_lte_pdsch_plan_soft_bits)
    const MiDecodeIO io = pl->core.io(d_out_bits, d_status, /*ul=*/false, pack);
    // every decode path lists its own kernels; the demodulator's entry, as it was launched, goes in front of them
    rc = pl->g3                     ? mi_dlsch3_run(ctx, pl->g3, pool, h_bind, io, pl->decoder, pl->n_iter)
         : !mi_is_bcjr(pl->decoder) ? mi_turbo_ref_dispatch(ctx, pl->core.groups.data(), (uint32_t)pl->core.groups.size(), io, &pl->core.multi)
                                    : pdsch_bcjr_decode(ctx, pl, io);
    if (rc != MI_LTE_OK) return rc;
    ctx->last_kernels = std::string(L.noise_first ? "k_dl_crs_noise:1," : "") + L.label + ":1," + ctx->last_kernels;
    return MI_LTE_OK;
}

extern "C" {

int mi_lte_pdsch_decode_run(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, const float *d_subframes, const uint32_t *d_subfr_num,
                            const uint32_t *d_n_id_cell, uint8_t *d_out_bits, int32_t *d_status)
{
    return pdsch_run(ctx, pl, nullptr, nullptr, d_subframes, d_subfr_num, d_n_id_cell, d_out_bits, d_status);
}

int mi_lte_pdsch_decode_run_harq(mi_lte_ctx *ctx, mi_lte_pdsch_plan *pl, mi_lte_harq_pool *pool, const mi_lte_harq_bind *h_bind, const float *d_subframes,
                                 const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell, uint8_t *d_out_bits, int32_t *d_status)
{
    if (!pool || !h_bind) return MI_LTE_ERR_INVALID_ARG;
    return pdsch_run(ctx, pl, pool, h_bind, d_subframes, d_subfr_num, d_n_id_cell, d_out_bits, d_status);
}

} // extern "C"
