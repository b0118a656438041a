// Control information on PUSCH in the 3GPP transport-block mode (ulsch_uci.hip): what a plan of mi_lte_pusch_plan_create_3gpp_uci holds
// besides the plain 3GPP plan's parts, and the two launches between its demodulator and its code blocks.  Internal to the library.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mi_lte.h"

struct MiUlschUci {
    uint32_t  n_alloc = 0, tiles = 0;      // tiles: gather workgroups per allocation (the longest run's)
    void     *d_desc = nullptr;            // one descriptor per allocation (ulsch_uci.hip: UciDesc)
    int8_t   *d_e = nullptr;               // data | CQI soft bits of every allocation, at the plan's 64-byte offsets
    uint32_t *d_e_len = nullptr;           // G per allocation (static: filled at creation)
    mi_lte_ulsch_uci_result *d_res = nullptr;
    std::vector<uint32_t> h_G, h_Q_cqi;
    // CQI decoding (ulsch_cqi.hip), off until mi_lte_pusch_plan_set_cqi_decode: one descriptor and one record per allocation
    bool               cqi_on = false, cqi_dirty = false; // dirty: h_cqi_desc has yet to reach d_cqi_desc (the next run copies it)
    mi_lte_cqi_desc   *d_cqi_desc = nullptr;
    mi_lte_cqi_result *d_cqi_res = nullptr;               // all zero from creation on
    std::vector<mi_lte_cqi_desc> h_cqi_desc;
};

// h_c_init: the scrambling sequence's c_init per allocation; h_G: what mi_lte_ulsch_uci_G gave for every descriptor; e_bytes: the plan's soft-bit
// buffer, in which every gathered run fits its allocation's slot (pusch_plan_layout has made and checked all three).
int  mi_ulsch_uci_create(mi_lte_ctx *ctx, const mi_lte_pdsch_alloc *h_allocs, const mi_lte_ulsch_uci *h_uci, const uint32_t *h_c_init,
                         const uint32_t *h_G, uint32_t n_alloc, size_t e_bytes, MiUlschUci **out);
void mi_ulsch_uci_free(MiUlschUci *u);
// k_ulsch_uci_gather and k_ulsch_uci_decide over the demodulator's soft bits d_e (allocation a at d_e + 64 d_e_off[a])
int  mi_ulsch_uci_run(mi_lte_ctx *ctx, MiUlschUci *u, const int8_t *d_e, const uint32_t *d_e_off);
// ulsch_cqi.hip.  h_O: information bits per allocation (0: left opaque), NULL: decoding off.  Refusals (O > MI_LTE_CQI_MAX_BITS, O on an
// allocation without CQI) leave u as it was.  mi_ulsch_cqi_run: k_ulsch_cqi_decode over the gathered runs, behind mi_ulsch_uci_run.
int  mi_ulsch_cqi_set(MiUlschUci *u, const uint32_t *h_e_off, size_t e_bytes, const uint32_t *h_O);
int  mi_ulsch_cqi_run(mi_lte_ctx *ctx, MiUlschUci *u);
