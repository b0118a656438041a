// Control-region geometry (pdcch_geom.h), following the reference step by step: PCFICH resource elements (pcfich_channel_demap,
// liblte_phy.cc:7887-7925), PHICH resource-element groups (phich_channel_demap :8224-8290), the PDCCH REG walk with its PCFICH/PHICH/CRS
// exclusions (:4590-4700), the cyclic-shift and sub-block-interleaver undo (:4702-4824), the CCEs and the six common-search-space candidates
// (4 x aggregation 4, 2 x aggregation 8), and the convolutional rate-unmatching index map (rate_unmatch_conv :11597-11755).
#include <algorithm>
#include <cmath>

#include "../../include/mi_lte.h"
#include "lte_tables.h"
#include "pdcch_geom.h"

namespace pdcch_geom {

void pcfich_regs(uint32_t N_rb_dl, uint32_t cell, uint32_t k[4], float n[4])
{
    const uint32_t k_hat = 6 * (cell % (2 * N_rb_dl));
    for (uint32_t i = 0; i < 4; i++) {
        k[i] = (k_hat + (i * N_rb_dl / 2) * 12 / 2) % (N_rb_dl * 12);
        n[i] = (k[i] / 6) - 0.5;
    }
}

void phich_group_regs(uint32_t N_rb_dl, uint32_t cell, uint32_t m, const float pcfich_n[4], uint32_t n_hat[3])
{
    const uint32_t n_l = N_rb_dl * 2 - 4;
    for (uint32_t i = 0; i < 3; i++) n_hat[i] = (cell + m + i * n_l / 3) % n_l;
    for (uint32_t i = 0; i < 4; i++)
        for (uint32_t j = 0; j < 3; j++)
            if (n_hat[j] > pcfich_n[i]) n_hat[j]++; // sequential, against the float REG number, as the reference does
}

CtrlRegs ctrl_regs(uint32_t N_rb_dl, uint32_t cell, float phich_res, bool regs_36211)
{
    CtrlRegs r;
    pcfich_regs(N_rb_dl, cell, r.pcfich_k, r.pcfich_n);
    const uint32_t N_group = (uint32_t)ceilf((float)phich_res * ((float)N_rb_dl / (float)8));
    std::vector<uint32_t> free_reg; // 36.211 6.9.3: the REGs of symbol 0 the PCFICH left, numbered from the lowest frequency up
    for (uint32_t n = 0; regs_36211 && n < 2 * N_rb_dl; n++)
        if (std::find(r.pcfich_k, r.pcfich_k + 4, 6 * n) == r.pcfich_k + 4) free_reg.push_back(n);
    for (uint32_t m = 0; m < N_group; m++) {
        uint32_t n_hat[3];
        if (regs_36211) {
            const uint32_t n_l = (uint32_t)free_reg.size();
            for (uint32_t i = 0; i < 3; i++) n_hat[i] = free_reg[(cell + m + i * n_l / 3) % n_l];
        } else {
            phich_group_regs(N_rb_dl, cell, m, r.pcfich_n, n_hat);
        }
        for (uint32_t i = 0; i < 3; i++) r.phich_k.push_back(n_hat[i] * 6);
    }
    return r;
}

// (the reference rebuilds this per call, liblte_phy.cc:4717-4812; its transmitter keeps it as a table, pdcch_permute_pre_calc :7970-8067)
void cc_interleaver_order(uint32_t n, std::vector<uint32_t> &order)
{
    const uint32_t R = (n + 31) / 32, N_dummy = 32 * R - n;
    order.clear();
    for (uint32_t j = 0; j < 32; j++)     // read column by column ...
        for (uint32_t i = 0; i < R; i++) { // ... of the column-permuted matrix
            const uint32_t nat = i * 32 + LTE_SUBBLOCK_COL_PERM_CC[j];
            if (nat >= N_dummy) order.push_back(nat - N_dummy);
        }
}

uint32_t cce_res(uint32_t N_rb_dl, uint32_t N_ant, uint32_t cell, float phich_res, uint32_t N_symbs, std::vector<uint32_t> &perm, bool regs_36211)
{
    perm.clear();
    const CtrlRegs cr = ctrl_regs(N_rb_dl, cell, phich_res, regs_36211);
    int64_t n_reg = (int64_t)N_symbs * (N_rb_dl * 3) - N_rb_dl - 4 - (int64_t)cr.phich_k.size();
    if (N_ant == 4 && (N_symbs > 1 || !regs_36211)) n_reg -= N_rb_dl; // (the reference takes symbol 1's CRS off a region that has no symbol 1)
    if (n_reg <= 0) return 0;
    const uint32_t N_reg = (uint32_t)n_reg, N_cce = N_reg / 9;
    std::vector<uint32_t> reg(4 * (size_t)N_reg, NO_RE); // REG m: its 4 RE indices (l*1200 + k)
    uint32_t m = 0;
    for (uint32_t k = 0; k < N_rb_dl * 12; k++)            // Steps 1-10 of 36.211 6.8.5 as the reference walks them
        for (uint32_t l = 0; l < N_symbs; l++) {
            if (m >= N_reg) continue;
            if (l == 0 || (l == 1 && N_ant == 4)) {
                bool valid = (k % 6) == 0;
                if (l == 0) {
                    for (uint32_t i = 0; i < 4; i++) valid &= k != cr.pcfich_k[i];
                    for (uint32_t kk : cr.phich_k) valid &= k != kk;
                }
                if (!valid) continue;
                uint32_t idx = 0;
                for (uint32_t i = 0; i < 6; i++)
                    if ((cell % 3) != (i % 3)) reg[4 * m + idx++] = l * N_SC_MAX + k + i; // skip the CRS positions
                m++;
            } else if ((k % 4) == 0) {
                for (uint32_t i = 0; i < 4; i++) reg[4 * m + i] = l * N_SC_MAX + k + i;
                m++;
            }
        }
    // undo the cell-specific cyclic shift and the sub-block interleaver: the REG sent (i + cell) mod N_reg-th is the order's (i + cell)-th entry
    std::vector<uint32_t> order;
    cc_interleaver_order(N_reg, order);
    perm.resize(4 * (size_t)N_reg);
    for (uint32_t i = 0; i < N_reg; i++) std::copy(&reg[4 * i], &reg[4 * i] + 4, &perm[4 * (size_t)order[(i + cell) % N_reg]]);
    return N_cce;
}

void candidate_res(uint32_t N_rb_dl, uint32_t N_ant, uint32_t cell, float phich_res, uint32_t N_symbs, uint32_t *out /*[N_CAND][RE_MAX]*/)
{
    std::fill(out, out + N_CAND * RE_MAX, NO_RE);
    std::vector<uint32_t> perm;
    const uint32_t N_cce = cce_res(N_rb_dl, N_ant, cell, phich_res, N_symbs, perm);
    for (uint32_t c = 0; c < N_CAND; c++) {
        // the reference always tries all six candidates; CCEs past the last one hold whatever its scratch held before --
        // zeros on a fresh LIBLTE_PHY_STRUCT, which de-map to soft value 0.  Here those elements are marked absent and
        // contribute 0 (the only state-dependent corner of the reference's decoder)
        const uint32_t L = c < 4 ? 4 : 8, first = (c < 4 ? c : c - 4) * L;
        for (uint32_t j = 0; j < L * 36; j++)
            if (first + j / 36 < N_cce) out[c * RE_MAX + j] = perm[(size_t)(first + j / 36) * 36 + j % 36];
    }
}

// (three sub-block-interleaved streams back to back, circular read from position 0, dummies skipped)
void conv_rm_map(uint32_t N_c, uint32_t E, uint16_t *map)
{
    uint32_t R = 0;
    while (N_c > 32 * R) R++;
    const uint32_t K_pi = 32 * R, K_w = 3 * K_pi, N_dummy = K_pi - N_c;
    for (uint32_t k = 0, j = 0; k < E; j++) {
        const uint32_t w = j % K_w, x = w / K_pi, pos = w % K_pi, col = pos / R, row = pos % R;
        const uint32_t nat = row * 32 + LTE_SUBBLOCK_COL_PERM_CC[col];
        if (nat >= N_dummy) map[k++] = (uint16_t)((nat - N_dummy) * 3 + x);
    }
}

} // namespace pdcch_geom

using namespace pdcch_geom;

extern "C" {

// the index tables on their own: where the PCFICH and the six candidates live in the subframe grid
int mi_lte_pdcch_re_tables(uint32_t N_rb_dl, uint32_t N_ant, uint32_t N_id_cell, float phich_res, uint32_t N_symbs, uint32_t *pcfich /*[16]*/,
                           uint32_t *cand /*[6][288]*/)
{
    if (!pcfich || !cand || !standard_ctrl_cfg(N_rb_dl, phich_res) || !(N_ant == 1 || N_ant == 2 || N_ant == 4) || N_id_cell > 503 || N_symbs < 1 || N_symbs > 4)
        return MI_LTE_ERR_INVALID_ARG;
    uint32_t k[4];
    float    n[4];
    pcfich_regs(N_rb_dl, N_id_cell, k, n);
    for (uint32_t i = 0; i < 4; i++) {
        uint32_t idx = 0;
        for (uint32_t j = 0; j < 6; j++)
            if ((N_id_cell % 3) != (j % 3)) pcfich[i * 4 + idx++] = k[i] + j;
    }
    candidate_res(N_rb_dl, N_ant, N_id_cell, phich_res, N_symbs, cand);
    return MI_LTE_OK;
}

// every CCE's resource elements (include/mi_lte.h: "PDCCH, 3GPP mode"): what a search plan holds for one (cell, N_symbs)
int mi_lte_pdcch_cce_tables(uint32_t N_rb_dl, uint32_t N_ant, uint32_t N_id_cell, float phich_res, uint32_t N_symbs, uint32_t flags, uint32_t *n_cce,
                            uint32_t *cce_re /*[36 n_max]*/, uint32_t n_max)
{
    if (!n_cce || (n_max && !cce_re) || !standard_ctrl_cfg(N_rb_dl, phich_res) || !(N_ant == 1 || N_ant == 2 || N_ant == 4) || N_id_cell > 503 || N_symbs < 1 ||
        N_symbs > 4 || (flags & ~MI_LTE_PDCCH_SEARCH_36211_REGS))
        return MI_LTE_ERR_INVALID_ARG;
    std::vector<uint32_t> perm;
    *n_cce = cce_res(N_rb_dl, N_ant, N_id_cell, phich_res, N_symbs, perm, (flags & MI_LTE_PDCCH_SEARCH_36211_REGS) != 0);
    std::copy(perm.begin(), perm.begin() + 36 * (size_t)std::min(*n_cce, n_max), cce_re);
    return MI_LTE_OK;
}

// PCFICH / PHICH resource-element-group positions as the reference reports them in LIBLTE_PHY_PCFICH_STRUCT::k, n and
// LIBLTE_PHY_PHICH_STRUCT::k, N_reg
int mi_lte_ctrl_reg_positions(uint32_t N_rb_dl, uint32_t N_id_cell, float phich_res, uint32_t *pcfich_k /*[4]*/, float *pcfich_n /*[4]*/,
                              uint32_t *phich_N_reg, uint32_t *phich_k /*[75]*/)
{
    if (!pcfich_k || !pcfich_n || !phich_N_reg || !phich_k || !standard_ctrl_cfg(N_rb_dl, phich_res) || N_id_cell > 503) return MI_LTE_ERR_INVALID_ARG;
    const CtrlRegs cr = ctrl_regs(N_rb_dl, N_id_cell, phich_res);
    if (cr.phich_k.size() > 75) return MI_LTE_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < 4; i++) { pcfich_k[i] = cr.pcfich_k[i]; pcfich_n[i] = cr.pcfich_n[i]; }
    *phich_N_reg = (uint32_t)cr.phich_k.size();
    std::copy(cr.phich_k.begin(), cr.phich_k.end(), phich_k);
    return MI_LTE_OK;
}

} // extern "C"
