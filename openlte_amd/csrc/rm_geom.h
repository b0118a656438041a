// The turbo rate-matching geometry of 36.212 5.1.4.1 as every un-matching kernel (turbo.hip, dlsch3gpp.hip) and the host's layout (synth.cc)
// use it: K_mimo, the soft-buffer rule (N_cb, k0), the circular buffer's positions and NULL counts, and the index of the reference-mode
// rank tables.
//
// Turbo rate un-matching (liblte_phy_rate_unmatch_turbo, liblte_phy.cc:11246-11490) as a gather: the circular buffer w[0..3*K_pi) holds,
// column-major, the sub-block-interleaved streams; the only NULL positions the reference's receiver honours are the N_d = 32R - D
// head-padding slots of each stream.  Walking w from k0 and consuming one e per non-NULL position means position p
// receives e[rank(p) + t*Nnn], t = 0,1,.. (repeats are soft-combined by addition, :11402-11416), with
// rank(p) = number of non-NULL positions between k0 and p in walk order.  Head padding sits in row 0 of a stream's R x 32 matrix,
// so "NULLs below p" is a popcount over the 32 columns.
//
// Pure functions on integers: compiles under a plain C++ compiler (tools/asan/rm_geom_driver.cc, which holds it to the transmitter's own
// walk of the buffer, tx::rate_match_turbo) and in the kernels alike.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h> // __popc, __brev (synth.cc includes no HIP header of its own)
#define RM_GEOM_FN __host__ __device__ __forceinline__
#else
#define RM_GEOM_FN inline
#endif

RM_GEOM_FN uint32_t rm_popc(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(v);
#else
    return (uint32_t)__builtin_popcount(v);
#endif
}

// inter-column permutation = 5-bit reversal (36.212 table 5.1.4-1)
RM_GEOM_FN uint32_t rm_brev5(uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(c) >> 27;
#else
    return ((c & 1u) << 4) | ((c & 2u) << 2) | (c & 4u) | ((c & 8u) >> 2) | ((c & 16u) >> 4);
#endif
}

RM_GEOM_FN uint32_t rm_k_mimo(uint32_t tx_mode) { return (tx_mode == 3 || tx_mode == 4 || tx_mode == 8 || tx_mode == 9) ? 2u : 1u; }

// 36.212 5.1.4.1.2 (liblte_phy.cc:11371-11399): the soft-buffer size of one of C code blocks of D = K + 4 positions per stream, and the
// redundancy version's start.  limited: DLSCH / PCH only (:11387-11398); UL-SCH has N_cb = K_w.
struct RmSoftBuf { uint32_t N_cb, k0; };
RM_GEOM_FN RmSoftBuf rm_soft_buffer(uint32_t D, uint32_t C, uint32_t tx_mode, uint32_t N_soft, uint32_t M_dl_harq, bool limited, uint32_t rv)
{
    const uint32_t R = (D + 31) / 32, K_w = 96 * R;
    const uint32_t N_ir = N_soft / (rm_k_mimo(tx_mode) * (M_dl_harq < 8 ? M_dl_harq : 8));
    RmSoftBuf      b;
    b.N_cb = (limited && N_ir / C < K_w) ? N_ir / C : K_w;
    b.k0   = R * (2 * ((b.N_cb + 8 * R - 1) / (8 * R)) * rv + 2);
    return b;
}

constexpr uint32_t RM_NO_RANK = 0xFFFFFFFFu; // RmGeom::rank of a d element no e bit reaches: not below any E (0xFFFF as a rank-table entry)

struct RmGeom {
    uint32_t R, K_pi, N_d, N_cb, k0m, Nnn, cnt_k0, mask0, mask2;
    RM_GEOM_FN static uint32_t lowmask(uint32_t n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }
    RM_GEOM_FN uint32_t nulls_below(uint32_t p) const
    {
        if (p <= K_pi) return rm_popc(mask0 & lowmask((p + R - 1) / R));
        const uint32_t q = p - K_pi, a = (q + 1) >> 1, b = q >> 1;
        return rm_popc(mask0) + rm_popc(mask0 & lowmask((a + R - 1) / R)) + rm_popc(mask2 & lowmask((b + R - 1) / R)) +
               ((b > K_pi - 1) ? 1u : 0u);
    }
    // R per liblte_phy.cc:11283-11287; N_cb and k0 as rm_soft_buffer gives them.  N_cb = 0 (N_ir / C = 0: a soft buffer without room for one
    // position, where the reference takes a remainder by zero; the host's layout refuses N_cb < 2) holds nothing: no division, and every
    // rank() is RM_NO_RANK.
    RM_GEOM_FN void init(uint32_t D, uint32_t N_cb_, uint32_t k0)
    {
        R    = (D + 31) / 32;
        K_pi = 32 * R;
        N_d  = K_pi - D;
        N_cb = N_cb_;
        k0m  = N_cb ? k0 % N_cb : 0u;
        mask0 = mask2 = 0;
        for (uint32_t c = 0; c < 32; c++) {
            const uint32_t P = rm_brev5(c);
            if (P < N_d) mask0 |= 1u << c;
            if (P + 1 < N_d) mask2 |= 1u << c; // (the third stream is shifted by one: its column P holds element 32 r + P + 1)
        }
        Nnn    = N_cb - nulls_below(N_cb);
        cnt_k0 = k0m - nulls_below(k0m);
    }
    // circular-buffer position of d[i*3+x] together with the non-NULL count below it, without integer division: the
    // element sits in column c, row r of its stream's R x 32 matrix, and only row 0 holds NULLs, so
    // "NULL slots below" is a popcount over the columns up to c (+1 if r > 0)
    RM_GEOM_FN void pos_cnt(uint32_t i, uint32_t x, uint32_t &p, uint32_t &cn) const
    {
        const uint32_t n = i + N_d - (x == 2 ? 1u : 0u), c = rm_brev5(n & 31), r = n >> 5, ii = c * R + r;
        const uint32_t cc = c + (r > 0 ? 1u : 0u);
        uint32_t nulls;
        if (x == 0) {
            p     = ii;
            nulls = rm_popc(mask0 & lowmask(cc));
        } else if (x == 1) {
            p     = K_pi + 2 * ii;
            nulls = rm_popc(mask0) + rm_popc(mask0 & lowmask(cc)) + rm_popc(mask2 & lowmask(cc));
        } else {
            p     = K_pi + 2 * ii + 1;
            nulls = rm_popc(mask0) + rm_popc(mask0 & lowmask(c + 1)) + rm_popc(mask2 & lowmask(cc));
        }
        cn = p - nulls;
    }
    // the first e index that reaches d[i*3+x]; the later ones follow a lap (Nnn) apart: for (k = rank(i, x); k < E; k += Nnn).
    // RM_NO_RANK where the position lies outside the soft buffer.
    RM_GEOM_FN uint32_t rank(uint32_t i, uint32_t x) const
    {
        uint32_t p, c;
        pos_cnt(i, x, p, c);
        const uint32_t k = (p >= k0m) ? c - cnt_k0 : Nnn - cnt_k0 + c;
        return p < N_cb ? k : RM_NO_RANK; // (two selects: as an early return this compiled to two exec-mask branches in the gather loops of k_dl3_rm_i8 and k_harq_rm)
    }
};

RM_GEOM_FN RmGeom rm_geom(uint32_t D, uint32_t C, uint32_t tx_mode, uint32_t N_soft, uint32_t M_dl_harq, bool limited, uint32_t rv)
{
    const RmSoftBuf b = rm_soft_buffer(D, C, tx_mode, N_soft, M_dl_harq, limited, rv);
    RmGeom          g;
    g.init(D, b.N_cb, b.k0);
    return g;
}

// The reference-mode plans' rank tables, one per combination of what the geometry of a block size depends on:
// combo 0..7 = rv*2 + (K_mimo == 2) with M_dl_harq = 8, N_soft = 250368 (liblte_phy.cc:3843-3844), C = 1 as liblte_phy_pdsch_channel_decode
// passes them; combo 8..11 = UL-SCH, rv = combo - 8: ulsch_channel_decode passes chan_type ULSCH, so N_cb = K_w (:12437-12449).
constexpr uint32_t RM_N_COMBOS = 12;
RM_GEOM_FN uint32_t rm_combo(uint32_t ul, uint32_t rv, uint32_t tx_mode)
{
    return ul ? 8u + (rv & 3u) : ((rv & 3u) << 1) | (rm_k_mimo(tx_mode) - 1u);
}
RM_GEOM_FN RmGeom rm_combo_geom(uint32_t combo, uint32_t D)
{
    return combo < 8 ? rm_geom(D, 1, (combo & 1) ? 3 : 1, 250368, 8, true, combo >> 1) : rm_geom(D, 1, 1, 1, 1, false, combo - 8);
}
