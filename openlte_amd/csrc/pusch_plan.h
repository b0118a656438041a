// What a PUSCH plan (uplink.hip: mi_lte_pusch_plan_create and its 3GPP forms) is made of before it owns any device memory: the checks of
// every allocation, the reference signals, the scrambling seeds, the soft-bit layout, the code-block slots of either mode and the symbol
// tap's offsets.  Pure host code -- no HIP, no context, no environment: pusch_plan_create commits what pusch_plan_layout returns, and every
// refusal that is not a HIP error comes from here.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/mi_lte.h"
#include "dlsch3_layout.h"
#include "plan_arith.h"

// The widths the reference has a transform pre-decoding plan for (liblte_phy.cc:2360-2377): below the carrier's and a multiple of 2, 3 or 5.
// spec: the 3GPP mode also takes the single resource block -- M = 12 is a size of 36.211 5.3.3, and a grant that small is where control
// information fills whole rows; the reference's test leaves it out only because 1 is no multiple of 2, 3 or 5.
inline bool pusch_nprb_planned(uint32_t N_prb, uint32_t N_rb, bool spec)
{
    return N_prb > 0 && N_prb < N_rb && (N_prb % 2 == 0 || N_prb % 3 == 0 || N_prb % 5 == 0 || (spec && N_prb == 1));
}

// UL-SCH rate matching has no soft-buffer limit: the DL-SCH soft-buffer configuration mi_lte_ulsch_layout computes with (ulsch_host.cc)
extern const mi_lte_dlsch_cfg ULSCH_AS_DLSCH;

struct PuschDesc {
    uint32_t subfr, cell;   // of the allocation's unit
    uint32_t dmrs_off;      // float offset of dmrs_0_re | dmrs_0_im | dmrs_1_re | dmrs_1_im (M each) in the DMRS pool
};

// One allocation on a carrier of N_rb resource blocks, in this order: the envelope (one code block in the reference mode; a planned N_prb;
// mod_type 0..3; unit < n_units) -> MI_LTE_ERR_UNSUPPORTED; spec: the 3GPP mode's transport block (no BPSK, mi_lte_ulsch_layout) -> its code;
// uci (spec only): mi_lte_ulsch_uci_G, the transport block over the G that is left, a symbol for every code block; a resource block past the
// carrier -> MI_LTE_ERR_INVALID_ARG.  *row (where given): the code block's row in the reference mode (0 in the 3GPP mode); *G: with uci, the
// data bits left.  *err (where given) receives the refusal's message.
int pusch_alloc_check(const mi_lte_pdsch_alloc &al, uint32_t N_rb, uint32_t n_units, bool spec, const mi_lte_ulsch_uci *uci, int *row, uint32_t *G,
                      const char **err);

struct PuschPlanLayout {
    std::vector<PuschDesc> desc;
    std::vector<float>     dmrs;          // the pool: one block of 4 x 12 N_prb floats per (cell, subframe, N_prb) in first-seen order, or the caller's blocks back to back
    std::vector<uint32_t>  c_init, e_len; // the scrambling seed (rnti << 14 | subframe << 9 | cell) and E = 144 N_prb Q_m per allocation
    std::vector<uint32_t>  e_off;         // soft-bit offsets in 64-byte units ...
    size_t                 e_bytes = 0;   // ... and the buffer's bytes (mi_plan_soft_layout)
    uint32_t               M_max = 0, words_max = 0, max_tbs = 0, out_stride = 0; // words_max: scrambling words of the longest allocation, one past its last
    // reference mode: one code block per allocation, grouped by size
    std::vector<uint8_t>   row;
    std::vector<MiKGroup>  groups;
    std::vector<uint32_t>  cb_alloc;
    // 3GPP mode: dlsch3gpp.hip's slots, and the symbol tap's offsets [n_alloc + 1] (144 N_prb symbols per allocation)
    MiDlsch3Layout         g3;
    std::vector<uint32_t>  x_off;
    std::vector<uint32_t>  G;             // with control information: the data bits it leaves per allocation
};

// ul, or h_dmrs: caller-supplied reference signals, 4 x 12*N_prb floats per allocation back to back.  spec: the 3GPP transport-block mode;
// h_uci (optional, spec only): one control-information descriptor per allocation.  Subframe numbers are taken modulo 10.
// Refusals in this order, each with its message in *err (where given): h_uci without spec (MI_LTE_ERR_UNSUPPORTED); cfg->N_rb_dl outside
// 6..100, which is what mi_lte_ul_frontend_batch accepts (MI_LTE_ERR_INVALID_ARG); the allocations one by one (pusch_alloc_check, then
// mi_lte_ul_dmrs_pusch's code); an allocation larger than the scrambling table; the 3GPP slot layout's (mi_dlsch3_layout); tap offsets
// past 32 bits; a control-information run that does not fit its slot.
int pusch_plan_layout(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const float *h_dmrs, const uint32_t *h_unit_subfr_num,
                      const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, bool spec,
                      const mi_lte_ulsch_uci *h_uci, PuschPlanLayout *out, const char **err);
