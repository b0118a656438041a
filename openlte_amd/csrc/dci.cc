// The DCI unpackers and the search-space list of include/mi_lte.h: host arithmetic on attacker-shaped payloads and bit counts, in plain C++ so
// that tools/asan/run_pdcch_host.sh can build it with g++ and the sanitizers.  The field lists are dci.h's, which the packers read too.
#include <algorithm>
#include <cstring>

#include "../../include/mi_lte.h"
#include "dci.h"
#include "lte_tables.h"
#include "pdcch_search.hpp"

using namespace dci;

extern "C" {

// DCI format 1A for SI-/P-/RA-RNTI -> allocation (dci_1a_unpack, liblte_phy.cc:13273-13378; localized VRBs only, like the
// reference: a distributed assignment leaves prb[][] untouched).  Returns 0, or 4 = LIBLTE_ERROR_INVALID_CONTENTS.
int mi_lte_dci_1a_unpack(uint32_t payload, uint32_t n_bits, uint32_t rnti, uint32_t N_rb_dl, uint32_t N_ant, mi_lte_pdcch_dci *o)
{
    if (!o || n_bits > 32 || N_rb_dl == 0 || N_rb_dl > 110) return MI_LTE_ERR_INVALID_ARG; // (110: LIBLTE_PHY_N_RB_DL_MAX)
    if (format_flag(payload, n_bits) == 0) return 4; // flagged as DCI format 0
    if (!common_rnti(rnti)) return 0;             // the reference leaves the allocation alone and still reports success
    const Fields f = unpack(FORMAT_1A, payload, n_bits, riv_bits(N_rb_dl));
    o->alloc.N_prb = f.riv / N_rb_dl + 1;         // (the first branch of the RIV only, as the reference)
    const uint32_t rb_start = f.riv % N_rb_dl;
    o->mcs = f.mcs;
    o->alloc.rv_idx = f.rv;
    const uint32_t col = (f.tpc % 2) == 0 ? 0 : 1; // N_PRB^1A = 2 or 3
    if (!f.flag)
        for (uint32_t i = 0; i < o->alloc.N_prb && i < 112; i++) o->alloc.prb[0][i] = o->alloc.prb[1][i] = (uint8_t)(rb_start + i);
    o->alloc.mod_type = 1;                        // QPSK
    o->alloc.tx_mode  = N_ant == 1 ? 1 : 2;
    o->alloc.rnti     = rnti;
    if (o->mcs >= 27) return 4;
    o->alloc.tbs = LTE_TBS_NPRB_2_3[o->mcs][col];
    return 0;
}

// DCI format 1C -> allocation (dci_1c_unpack, liblte_phy.cc:13400-13611): distributed VRBs of 36.211 6.2.3.2 and the
// format-1C transport-block sizes.  A RIV that matches no (length, start) pair leaves N_prb as the caller set it.
int mi_lte_dci_1c_unpack(uint32_t payload, uint32_t n_bits, uint32_t rnti, uint32_t N_rb_dl, uint32_t N_ant, mi_lte_pdcch_dci *o)
{
    if (!o || n_bits > 32 || N_rb_dl < 6 || N_rb_dl > 110) return MI_LTE_ERR_INVALID_ARG;
    // the gap bit exists from 10 MHz up, and the reference sizes the RIV field by the gap it signals: read it first, then the whole list
    const uint32_t gap_len = N_rb_dl < 50 ? 0 : 1, gap2 = unpack(FORMAT_1C, payload, n_bits, 0, gap_len).gap;
    uint32_t N_gap;
    if (N_rb_dl <= 10) N_gap = (uint32_t)ceilf(N_rb_dl / 2.0);
    else if (N_rb_dl == 11) N_gap = 4;
    else if (N_rb_dl <= 19) N_gap = 8;
    else if (N_rb_dl <= 26) N_gap = 12;
    else if (N_rb_dl <= 44) N_gap = 18;
    else if (N_rb_dl <= 49) N_gap = 27;
    else if (N_rb_dl <= 63) N_gap = gap2 ? 9 : 27;
    else if (N_rb_dl <= 70) N_gap = gap2 ? 16 : 32;
    else N_gap = gap2 ? 16 : 48;
    const uint32_t n_vrb_gap1 = 2 * std::min(N_gap, N_rb_dl - N_gap), n_vrb_gap2 = (N_rb_dl / (2 * N_gap)) * 2 * N_gap;
    const uint32_t n_vrb = gap2 ? n_vrb_gap2 : n_vrb_gap1, step = N_rb_dl <= 49 ? 2 : 4, n_tilde = gap2 ? 2 * N_gap : n_vrb;
    if (!common_rnti(rnti)) return 4;
    const uint32_t q = n_vrb_gap1 / step;
    const Fields   f = unpack(FORMAT_1C, payload, n_bits, (uint32_t)ceilf(logf(q * (q + 1) / 2.0) / logf(2)), gap_len);
    const uint32_t riv = f.riv, nd = n_vrb / step;
    uint32_t rb_start = 0;
    for (uint32_t len = 1; len <= nd; len++)      // every (length, start) pair is tried and the last match stands
        for (uint32_t st = 0; st + 1 <= nd; st++) {
            const uint32_t code = (len - 1) <= nd / 2 ? nd * (len - 1) + st : nd * (nd - len + 1) + (nd - 1 - st);
            if (riv == code) { o->alloc.N_prb = len * step; rb_start = st * step; }
        }
    o->mcs = f.mcs;
    const uint32_t P = N_rb_dl <= 10 ? 1 : N_rb_dl <= 26 ? 2 : N_rb_dl <= 63 ? 3 : 4;
    const uint32_t n_row = (uint32_t)(ceilf(n_tilde / (4.0 * P)) * P), n_null = 4 * n_row - n_tilde;
    for (uint32_t i = 0, v = rb_start; i < o->alloc.N_prb && i < 112; i++, v++) {
        const uint32_t vt = v % n_tilde, blk = n_tilde * (v / n_tilde);
        const uint32_t two_col = 2 * n_row * (vt % 2) + vt / 2 + blk, four_col = n_row * (vt % 4) + vt / 4 + blk;
        uint32_t even;
        if (n_null != 0 && vt >= n_tilde - n_null && (vt % 2) == 1) even = two_col - n_row;
        else if (n_null != 0 && vt >= n_tilde - n_null && (vt % 2) == 0) even = two_col - n_row + n_null / 2;
        else if (n_null != 0 && vt < n_tilde - n_null && (vt % 4) >= 2) even = four_col - n_null / 2;
        else even = four_col;
        const uint32_t odd = (even + n_tilde / 2) % n_tilde + blk;
        o->alloc.prb[0][i] = (uint8_t)(even < n_tilde / 2 ? even : even + N_gap - n_tilde / 2);
        o->alloc.prb[1][i] = (uint8_t)(odd < n_tilde / 2 ? odd : odd + N_gap - n_tilde / 2);
    }
    o->alloc.mod_type = 1;
    o->alloc.tx_mode  = N_ant == 1 ? 1 : 2;
    o->alloc.rnti     = rnti;
    o->alloc.tbs      = LTE_TBS_DCI_1C[o->mcs & 31]; // a 5-bit field: always in range
    return 0;
}

// A C-RNTI's DCI format 0 / 1A as tx_ctrl.cc packs them from the same field lists; what the fields mean is in include/mi_lte.h
int mi_lte_dci_0_1a_unpack_crnti(uint64_t payload, uint32_t n_bits, uint32_t rnti, uint32_t N_rb, uint32_t N_ant, mi_lte_dci_crnti *o)
{
    if (!o || n_bits > 64 || rnti == 0 || rnti > 0xFFFFu || N_rb == 0 || N_rb > 110 || !(N_ant == 1 || N_ant == 2 || N_ant == 4)) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t riv_len = riv_bits(N_rb);
    if (n_bits < 1) return MI_LTE_ERR_INVALID_ARG;
    memset(o, 0, sizeof(*o));
    o->format = format_flag(payload, n_bits);
    if (n_bits < (o->format ? total_bits(FORMAT_1A, riv_len) : total_bits(FORMAT_0, riv_len))) return MI_LTE_ERR_INVALID_ARG;
    const Fields f = o->format ? unpack(FORMAT_1A, payload, n_bits, riv_len) : unpack(FORMAT_0, payload, n_bits, riv_len);
    o->flag = f.flag; o->riv = f.riv; o->mcs = f.mcs; o->ndi = f.ndi; o->tpc = f.tpc;
    o->harq = f.harq; o->rv = f.rv; o->cyclic_shift = f.cyclic_shift; o->cqi_request = f.cqi_request; // (zero where the format has no such field)
    const bool riv_ok = riv_decode(N_rb, o->riv, &o->N_prb, &o->rb_start);
    o->alloc.rnti = rnti;
    if (!riv_ok || o->N_prb == 0 || o->N_prb > N_rb) { o->N_prb = 0; return 4; }
    if (o->format && o->flag) return 4; // distributed VRBs: no PRB list here
    o->alloc.N_prb = o->N_prb;
    for (uint32_t i = 0; i < o->N_prb; i++) o->alloc.prb[0][i] = o->alloc.prb[1][i] = (uint8_t)(o->rb_start + i);
    if (o->mcs > 28) return 4; // no transport block of its own
    if (o->format) {
        const uint32_t i_tbs = o->mcs <= 9 ? o->mcs : o->mcs <= 16 ? o->mcs - 1 : o->mcs - 2;
        o->alloc.mod_type = o->mcs <= 9 ? 1 : o->mcs <= 16 ? 2 : 3;
        o->alloc.tbs      = 8u * LTE_TBS_DIV8[i_tbs][o->N_prb - 1];
        o->alloc.rv_idx   = o->rv;
        o->alloc.tx_mode  = N_ant == 1 ? 1 : 2;
    }
    return 0;
}

int mi_lte_pdcch_search_space(uint32_t rnti, uint32_t subfr_num, uint32_t N_cce, uint32_t L, uint32_t *first_cce /*[6]*/, uint32_t *n)
{
    if (!first_cce || !n || rnti == 0 || rnti > 0xFFFFu || subfr_num > 9 || !(L == 1 || L == 2 || L == 4 || L == 8)) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t nl = N_cce / L;
    *n = 0;
    if (nl == 0) return MI_LTE_OK; // no candidate fits: no modulus to take
    const uint32_t y = search_space_y(rnti, subfr_num);
    for (uint32_t m = 0; m < search_space_m(L); m++) first_cce[(*n)++] = L * ((y + m) % nl);
    return MI_LTE_OK;
}

} // extern "C"
