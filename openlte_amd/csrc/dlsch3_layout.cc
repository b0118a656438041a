// The slot layout of the 3GPP transport-block mode: see dlsch3_layout.h.
#include "dlsch3_layout.h"

#include "plan_arith.h"

int mi_dlsch3_layout(const mi_lte_dlsch_cfg *cfg, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, MiDlsch3Layout *out, const char **err)
{
    MiDlsch3Layout &L = *out;
    L = MiDlsch3Layout();
    L.a_slot.resize(n_alloc); L.a_nc.resize(n_alloc); L.a_K.resize(n_alloc); L.a_tbs.resize(n_alloc); L.a_soft.resize(n_alloc);
    std::vector<uint8_t> row(n_alloc);
    for (uint32_t a = 0; a < n_alloc; a++) {
        mi_lte_dlsch_layout_t lay;
        const int rc = mi_lte_dlsch_layout(h_allocs[a].tbs, 0, 2, h_allocs[a].tx_mode, h_allocs[a].rv_idx & 3u, cfg, &lay);
        if (rc != MI_LTE_OK) { if (err) *err = "transport block size outside the 3GPP mode (F != 0 or tbs > 75376)"; return rc; }
        L.a_nc[a] = lay.C; L.a_K[a] = lay.K; L.a_tbs[a] = h_allocs[a].tbs;
        row[a] = (uint8_t)mi_qpp_row_at_least(lay.K);
    }
    std::vector<uint32_t> slot_alloc;
    mi_plan_group(row.data(), L.a_nc.data(), nullptr, n_alloc, L.groups, slot_alloc);
    L.slots.resize(slot_alloc.size());
    size_t soft = 0, bits = 0;
    for (const MiKGroup &gr : L.groups) { // a size's arrays start on 256 bytes
        soft = (soft + 255) & ~(size_t)255; bits = (bits + 255) & ~(size_t)255;
        L.g_soft.push_back(soft); L.g_bits.push_back(bits);
        for (uint32_t s = gr.cb_base, r = 0; s < gr.cb_base + gr.n_cb; s++, soft += 3 * (size_t)(gr.K + 4), bits += gr.K) {
            const uint32_t a = slot_alloc[s], C = L.a_nc[a], B = h_allocs[a].tbs + 24;
            r = (s > gr.cb_base && slot_alloc[s - 1] == a) ? r + 1 : 0; // an allocation's blocks are adjacent
            if (r == 0) { L.a_slot[a] = s; L.a_soft[a] = soft; }
            // x^s mod gCRC24A, s = B - (r + 1)(K - 24) for C > 1 (0 for C = 1): the transport-block bits behind the block's payload
            const uint32_t xs = xpow(C == 1 ? 0u : B - (r + 1) * (gr.K - 24), G_CRC24A);
            L.slots[s] = {a, r, C, gr.K, xs, (uint32_t)(soft / 4), (uint32_t)(bits / 8), 0};
        }
        if (soft / 4 > 0xFFFFFFFFull || bits / 8 > 0xFFFFFFFFull) { if (err) *err = "3GPP plan too large"; return MI_LTE_ERR_UNSUPPORTED; }
    }
    L.soft_bytes = soft; L.bits_bytes = bits;
    return MI_LTE_OK;
}
