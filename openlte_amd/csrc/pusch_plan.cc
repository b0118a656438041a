// The host half of a PUSCH plan: see pusch_plan.h.
#include "pusch_plan.h"

#include <algorithm>
#include <map>
#include <tuple>

namespace {
int refuse(const char **err, const char *msg, int rc)
{
    if (err) *err = msg;
    return rc;
}
} // namespace

int pusch_alloc_check(const mi_lte_pdsch_alloc &al, uint32_t N_rb, uint32_t n_units, bool spec, const mi_lte_ulsch_uci *uci, int *row, uint32_t *G,
                      const char **err)
{
    const int r = spec ? 0 : mi_tb_row(al.tbs);
    // (N_prb > 110: no carrier has that many, and prb[] holds 112)
    if (r < 0 || !pusch_nprb_planned(al.N_prb, N_rb, spec) || al.N_prb > 110 || al.mod_type > 3 || al.unit >= n_units)
        return refuse(err, "PUSCH allocation outside the envelope (one code block; N_prb < N_rb_ul and divisible by 2, 3 or 5) or malformed", MI_LTE_ERR_UNSUPPORTED);
    if (spec) {
        mi_lte_dlsch_layout_t lay;
        const int rc = al.mod_type == 0 ? MI_LTE_ERR_UNSUPPORTED : mi_lte_ulsch_layout(al.tbs, 0, 2, al.rv_idx & 3u, &lay);
        if (rc != MI_LTE_OK) return refuse(err, "PUSCH allocation outside the 3GPP transport-block mode (BPSK, F != 0 or tbs > 75376)", rc);
    }
    if (uci) { // the descriptor's own conditions, then the transport block over the G that the control information leaves (36.212 5.2.2.7)
        const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : 2;
        int rc = mi_lte_ulsch_uci_G(al.N_prb, Qm, uci, G);
        if (rc != MI_LTE_OK)
            return refuse(err, "control information refused: O > 2, Q' > 4 M, O without Q' or Q' without O, Q_cqi not a multiple of Q_m, or no room left for data", rc);
        mi_lte_dlsch_layout_t lay;
        if ((rc = mi_lte_ulsch_layout(al.tbs, *G, Qm, al.rv_idx & 3u, &lay)) != MI_LTE_OK)
            return refuse(err, "the transport block does not fit the bits that control information leaves (mi_lte_ulsch_layout)", rc);
        if (*G / Qm < lay.C) return refuse(err, "control information leaves a code block without a symbol", MI_LTE_ERR_INVALID_ARG);
    }
    for (uint32_t sl = 0; sl < 2; sl++) // a resource block past the carrier would be read out of the neighbouring symbol row
        for (uint32_t i = 0; i < al.N_prb; i++)
            if (al.prb[sl][i] >= N_rb) return refuse(err, "PUSCH allocation names a resource block outside the carrier", MI_LTE_ERR_INVALID_ARG);
    if (row) *row = r;
    return MI_LTE_OK;
}

int pusch_plan_layout(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const float *h_dmrs, const uint32_t *h_unit_subfr_num,
                      const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, bool spec,
                      const mi_lte_ulsch_uci *h_uci, PuschPlanLayout *out, const char **err)
{
    if (h_uci && !spec) return refuse(err, "control information on PUSCH needs a plan in the 3GPP transport-block mode", MI_LTE_ERR_UNSUPPORTED);
    if (cfg->N_rb_dl < 6 || cfg->N_rb_dl > 100) return refuse(err, "PUSCH plan on a carrier outside 6..100 resource blocks", MI_LTE_ERR_INVALID_ARG);
    PuschPlanLayout &L = *out;
    L = PuschPlanLayout();
    L.desc.resize(n_alloc); L.row.resize(n_alloc); L.c_init.resize(n_alloc); L.e_len.resize(n_alloc);
    if (h_uci) L.G.resize(n_alloc);
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> dmrs_at; // (cell, subframe, N_prb) -> float offset
    for (uint32_t a = 0; a < n_alloc; a++) {
        const mi_lte_pdsch_alloc &al = h_allocs[a];
        int r = 0;
        int rc = pusch_alloc_check(al, cfg->N_rb_dl, n_units, spec, h_uci ? &h_uci[a] : nullptr, &r, h_uci ? &L.G[a] : nullptr, err);
        if (rc != MI_LTE_OK) return rc;
        const uint32_t sf = h_unit_subfr_num[al.unit] % 10, cell = h_unit_n_id_cell[al.unit], M = 12 * al.N_prb;
        if (h_dmrs) {
            const uint32_t at = (uint32_t)L.dmrs.size();
            L.dmrs.insert(L.dmrs.end(), h_dmrs, h_dmrs + 4 * (size_t)M);
            h_dmrs += 4 * (size_t)M;
            L.desc[a] = {sf, cell, at};
        } else {
            auto key = std::make_tuple(cell, sf, al.N_prb);
            auto it  = dmrs_at.find(key);
            if (it == dmrs_at.end()) {
                const uint32_t at = (uint32_t)L.dmrs.size();
                L.dmrs.resize(L.dmrs.size() + 4 * (size_t)M);
                rc = mi_lte_ul_dmrs_pusch(ul, cell, sf, al.N_prb, &L.dmrs[at], &L.dmrs[at + M], &L.dmrs[at + 2 * M], &L.dmrs[at + 3 * M]);
                if (rc != MI_LTE_OK) return rc;
                it = dmrs_at.emplace(key, at).first;
            }
            L.desc[a] = {sf, cell, it->second};
        }
        L.c_init[a] = (al.rnti << 14) | (sf << 9) | cell; // (k_pusch_demod's)
        L.row[a]    = (uint8_t)r;
        L.max_tbs   = std::max(L.max_tbs, al.tbs);
        const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : al.mod_type == 1 ? 2 : 1, E = 12 * M * Qm;
        L.M_max     = std::max(L.M_max, M);
        L.words_max = std::max(L.words_max, (E + 31) / 32 + 1);
        L.e_len[a]  = E;
    }
    if (L.words_max > 4096) return refuse(err, "allocation larger than the scrambling table", MI_LTE_ERR_UNSUPPORTED);
    L.e_bytes    = mi_plan_soft_layout(L.e_len.data(), n_alloc, L.e_off);
    L.out_stride = mi_out_stride(L.max_tbs, false);
    L.cb_alloc.assign(n_alloc, 0u);
    if (!spec) mi_plan_group(L.row.data(), nullptr, L.e_len.data(), n_alloc, L.groups, L.cb_alloc);
    if (spec) {
        const int rc = mi_dlsch3_layout(&ULSCH_AS_DLSCH, h_allocs, n_alloc, &L.g3, err);
        if (rc != MI_LTE_OK) return rc;
        L.x_off.resize(n_alloc + 1);
        uint64_t at = 0;
        for (uint32_t a = 0; a < n_alloc; a++) { L.x_off[a] = (uint32_t)at; at += 144ull * h_allocs[a].N_prb; }
        if (at > 0xFFFFFFFFull) return refuse(err, "plan larger than the symbol tap's 32-bit offsets", MI_LTE_ERR_UNSUPPORTED);
        L.x_off[n_alloc] = (uint32_t)at;
    }
    for (uint32_t a = 0; h_uci && a < n_alloc; a++) // the gathered run replaces the allocation's 12 * 12 N_prb * Q_m soft bits in a slot of the same size at the same offset
        if ((size_t)L.e_off[a] * 64 + ((size_t)L.G[a] + h_uci[a].Q_cqi + 3) / 4 * 4 > L.e_bytes)
            return refuse(err, "soft-bit layout too small for the allocation", MI_LTE_ERR_INVALID_ARG);
    return MI_LTE_OK;
}
