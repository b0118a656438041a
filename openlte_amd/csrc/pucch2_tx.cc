// PUCCH formats 2 / 2a / 2b, the transmitting side on the host: the (20, A) block code of 36.212 5.2.3.3 (pucch2_code.h) and the mapping of
// 36.211 5.4.2 onto one UE's resource-block pair -- scrambling, QPSK, d(n) times the cyclically shifted sequence on the five data symbols of
// each slot, the sequence itself on reference symbol 1 and z times it on reference symbol 5 (5.5.2.2.1: d(10) of formats 2a / 2b).  The
// sequences come from mi_lte_ul_pucch2_table (ul_rs.cc).  The reference declares these functions and leaves them empty; mi_lte.h holds
// the definition.
#include <cmath>
#include <cstdint>

#include "../../include/mi_lte.h"
#include "pucch2_code.h"

namespace {

constexpr uint32_t GRID_SC = 1200; // row stride of the UL subframe layout
const uint32_t     DATA_SYMB[5] = {0, 2, 3, 4, 6};

void put(const mi_lte_pucch2_tab *t, uint32_t L, float d_re, float d_im, float *re, float *im)
{
    const uint32_t k0 = 12 * t->prb[L / 7];
    for (uint32_t k = 0; k < 12; k++) {
        const float r_re = t->r_re[L][k], r_im = t->r_im[L][k];
        re[L * GRID_SC + k0 + k] = d_re * r_re - d_im * r_im;
        im[L * GRID_SC + k0 + k] = d_re * r_im + d_im * r_re;
    }
}

} // namespace

extern "C" {

int mi_lte_pucch2_encode(uint32_t A, const uint8_t *a_bits, uint8_t *b)
{
    if (!a_bits || !b || A == 0 || A > MI_PUCCH2_MAX_BITS) return MI_LTE_ERR_INVALID_ARG;
    uint32_t w = 0;
    for (uint32_t n = 0; n < A; n++) w |= (uint32_t)(a_bits[n] & 1u) << n;
    const uint32_t word = mi_pucch2_word(w);
    for (uint32_t i = 0; i < MI_PUCCH2_CODED; i++) b[i] = (uint8_t)((word >> i) & 1u);
    return MI_LTE_OK;
}

int mi_lte_pucch2_modulate(const mi_lte_pucch2_tab *tab, uint32_t format, const uint8_t *b, const uint8_t *ack, float *re, float *im)
{
    if (!tab || !b || !re || !im || format > 2 || (format > 0 && !ack) || tab->prb[0] >= GRID_SC / 12 || tab->prb[1] >= GRID_SC / 12)
        return MI_LTE_ERR_INVALID_ARG;
    const float a = (float)(1 / std::sqrt(2.0));
    for (uint32_t n = 0; n < 10; n++) {
        const uint32_t b0 = (b[2 * n] ^ (tab->c_scr >> (2 * n))) & 1u, b1 = (b[2 * n + 1] ^ (tab->c_scr >> (2 * n + 1))) & 1u;
        put(tab, 7 * (n / 5) + DATA_SYMB[n % 5], b0 ? -a : a, b1 ? -a : a, re, im);
    }
    float z_re = 1, z_im = 0; // 36.211 table 5.4.2-1
    if (format == 1 && (ack[0] & 1u)) z_re = -1;
    if (format == 2) {
        const uint32_t v = 2 * (ack[0] & 1u) + (ack[1] & 1u);
        z_re = v == 0 ? 1.f : v == 3 ? -1.f : 0.f;
        z_im = v == 1 ? -1.f : v == 2 ? 1.f : 0.f;
    }
    for (uint32_t s = 0; s < 2; s++) {
        put(tab, 7 * s + 1, 1, 0, re, im);
        put(tab, 7 * s + 5, z_re, z_im, re, im);
    }
    return MI_LTE_OK;
}

} // extern "C"
