// Host arithmetic of the uplink shared channel in the 3GPP transport-block mode (include/mi_lte.h): the transport block's layout with the
// uplink's unlimited soft buffer, and the control-information rules of 36.212 5.2.2.6-5.2.2.8 -- the descriptor checks (mi_lte_ulsch_uci_G),
// the Q' arithmetic and the forward map the transmitter is driven by (ulsch_uci.hip's kernels use its inverse).  No device, no context.
#include <cstring>

#include "pusch_plan.h"

// UL-SCH rate matching has no soft-buffer limit (36.212 5.2.2.5: N_cb = K_w).  As a DL-SCH soft-buffer configuration: an N_IR no block reaches
const mi_lte_dlsch_cfg ULSCH_AS_DLSCH = {MI_LTE_ULSCH_N_SOFT, MI_LTE_ULSCH_M_HARQ};

extern "C" {

int mi_lte_ulsch_layout(uint32_t tbs, uint32_t G, uint32_t Q_m, uint32_t rv, mi_lte_dlsch_layout_t *out)
{
    return mi_lte_dlsch_layout(tbs, G, Q_m, 1, rv, &ULSCH_AS_DLSCH, out);
}

int mi_lte_ulsch_uci_qprime(uint32_t kind, uint32_t O, uint32_t beta_x8, uint32_t M_sc_initial, uint32_t N_symb_initial, uint32_t sum_K_r,
                            uint32_t N_prb, uint32_t Qp_ri, uint32_t *Qp)
{
    if (!Qp || kind > MI_LTE_UCI_CQI || sum_K_r == 0 || N_prb == 0 || N_prb > 110) return MI_LTE_ERR_INVALID_ARG;
    // (factors inside what 36.212 / 36.213 allow, generously: the product below then stays under 2^56)
    if (O > 0xFFFFu || beta_x8 > 0xFFFFu || M_sc_initial > 1320 || N_symb_initial > 14) return MI_LTE_ERR_INVALID_ARG;
    const uint64_t M = 12ull * N_prb;
    if (kind == MI_LTE_UCI_CQI && Qp_ri > 4 * M) return MI_LTE_ERR_INVALID_ARG;
    const uint64_t cap = kind == MI_LTE_UCI_CQI ? 12 * M - Qp_ri : 4 * M;
    const uint64_t Oe  = kind == MI_LTE_UCI_CQI && O > 11 ? (uint64_t)O + 8 : O; // the CQI's CRC (36.212 5.2.2.6)
    const uint64_t num = Oe * M_sc_initial * N_symb_initial * beta_x8, den = 8ull * sum_K_r;
    const uint64_t q   = (num + den - 1) / den;
    *Qp = (uint32_t)(q < cap ? q : cap);
    return MI_LTE_OK;
}

int mi_lte_ulsch_uci_G(uint32_t N_prb, uint32_t Q_m, const mi_lte_ulsch_uci *uci, uint32_t *G)
{
    if (!uci || !G || N_prb == 0 || N_prb > 110 || !(Q_m == 2 || Q_m == 4 || Q_m == 6)) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t M = 12 * N_prb;
    if (uci->O_ack > 2 || uci->O_ri > 2 || uci->Qp_ack > 4 * M || uci->Qp_ri > 4 * M) return MI_LTE_ERR_INVALID_ARG;
    if ((uci->O_ack == 0) != (uci->Qp_ack == 0) || (uci->O_ri == 0) != (uci->Qp_ri == 0) || uci->Q_cqi % Q_m) return MI_LTE_ERR_INVALID_ARG;
    const int64_t g = (int64_t)Q_m * (12 * (int64_t)M - uci->Qp_ri) - (int64_t)uci->Q_cqi;
    if (g <= 0) return MI_LTE_ERR_INVALID_ARG;
    *G = (uint32_t)g;
    return MI_LTE_OK;
}

int mi_lte_ulsch_uci_map(uint32_t N_prb, uint32_t Q_m, const mi_lte_ulsch_uci *uci, uint8_t *kind, uint32_t *index)
{
    uint32_t  G;
    const int rc = mi_lte_ulsch_uci_G(N_prb, Q_m, uci, &G);
    if (rc != MI_LTE_OK) return rc;
    if (!kind || !index) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t M = 12 * N_prb, n_cqi = uci->Q_cqi / Q_m;
    static const uint32_t ri_col[4] = {1, 10, 7, 4}, ack_col[4] = {2, 9, 8, 3};
    memset(kind, MI_LTE_UCI_CELL_DATA, 12 * (size_t)M);
    for (uint32_t i = 0; i < uci->Qp_ri; i++) { // 1. rank indication, from the last row upwards
        const uint32_t cell = (M - 1 - i / 4) * 12 + ri_col[i % 4];
        kind[cell] = MI_LTE_UCI_CELL_RI; index[2 * cell] = i; index[2 * cell + 1] = 0xFFFFFFFFu;
    }
    for (uint32_t cell = 0, t = 0; cell < 12 * M; cell++) { // 2. CQI, then data, row by row around the RI cells
        if (kind[cell] == MI_LTE_UCI_CELL_RI) continue;
        kind[cell] = t < n_cqi ? MI_LTE_UCI_CELL_CQI : MI_LTE_UCI_CELL_DATA;
        index[2 * cell] = t < n_cqi ? t : t - n_cqi; index[2 * cell + 1] = 0xFFFFFFFFu;
        t++;
    }
    for (uint32_t i = 0; i < uci->Qp_ack; i++) { // 3. HARQ-ACK over what step 2 wrote
        const uint32_t cell = (M - 1 - i / 4) * 12 + ack_col[i % 4];
        index[2 * cell + 1] = index[2 * cell]; index[2 * cell] = i;
        kind[cell] = kind[cell] == MI_LTE_UCI_CELL_CQI ? MI_LTE_UCI_CELL_ACK_CQI : MI_LTE_UCI_CELL_ACK_DATA;
    }
    return MI_LTE_OK;
}

} // extern "C"
