// What every plan (PDSCH: chain.hip, PUSCH: uplink.hip, 3GPP transport-block mode: dlsch3gpp.hip) holds on the device and hands to the decoder; the
// arithmetic that lays it out -- code-block size lookup, soft-bit layout, slots grouped by size -- is plan_arith.h's.  Nothing here knows which channel calls it.
#pragma once

#include "ctx.hpp"
#include "plan_arith.h"

inline bool mi_is_bcjr(uint32_t mode) { return mode == MI_LTE_TURBO_BCJR || mode == MI_LTE_TURBO_BCJR_BLOCK || mode == MI_LTE_TURBO_BCJR_EARLY; }

// What a plan hands to a decoder entry point (turbo.hip: mi_turbo_ref_dispatch, mi_turbo_bcjr_group; dlsch3gpp.hip: mi_dlsch3_run)
struct MiDecodeIO {
    const mi_lte_pdsch_alloc *d_allocs;
    const uint32_t *d_cb_alloc, *d_e_off, *d_e_len;
    const int8_t   *d_e;
    uint8_t        *d_out_bits;
    int32_t        *d_status;
    uint32_t        out_stride;
    bool            ul, packed;
    bool            soft_packed; // d_e holds the 16QAM / 64QAM allocations one bit per soft bit (soft_pack.h): PDSCH plans into mi_turbo_ref_dispatch only
};

// What every plan holds
struct MiPlanCore {
    uint32_t n_alloc = 0, out_stride = 0, packed = 0;
    size_t   e_bytes = 0;
    // capacity of the device arrays (a dynamic plan is re-assigned within it; a static plan's capacity is its first assignment)
    uint32_t cap_alloc = 0;
    size_t   cap_e_bytes = 0;
    mi_lte_pdsch_alloc *d_allocs = nullptr;
    uint32_t *d_e_off = nullptr, *d_e_len = nullptr, *d_cb_alloc = nullptr;
    int8_t   *d_e = nullptr;
    bool      desc_views = false; // d_allocs, d_e_off, d_cb_alloc are views of a block the plan owns otherwise (allocate)
    std::vector<MiKGroup> groups;
    std::vector<uint32_t> h_e_off;
    MiMultiCache          multi; // the merged decode's device tables for `groups` (turbo.hip: mi_turbo_ref_dispatch)

    // d_desc_block: device memory of the caller's that holds allocs | e_off | cb_alloc, n_alloc_max entries each, instead of three arrays of the plan's own
    hipError_t allocate(uint32_t n_alloc_max, size_t e_bytes_max, void *d_desc_block = nullptr);
    void       release();
    MiDecodeIO io(uint8_t *d_out_bits, int32_t *d_status, bool ul, bool soft_packed = false) const { return {d_allocs, d_cb_alloc, d_e_off, d_e_len, d_e, d_out_bits, d_status, out_stride, ul, packed != 0, soft_packed}; }
};

int   mi_turbo_ref_dispatch(mi_lte_ctx *ctx, const MiKGroup *groups, uint32_t n_groups, const MiDecodeIO &io, MiMultiCache *cache);
// one block size through a BCJR decoder; d_cb_alloc of io: the whole plan's (the group's slots start at gr.cb_base)
int   mi_turbo_bcjr_group(mi_lte_ctx *ctx, const MiKGroup &gr, const MiDecodeIO &io, int8_t *d_soft, uint8_t *d_c_bits, uint32_t mode, uint32_t n_iter, int qpp_spec);

// the 3GPP transport-block mode's part of a plan (dlsch3gpp.hip)
struct MiDlsch3;
struct MiDlsch3Layout; // dlsch3_layout.h: the first form commits a layout the caller has made, the second lays the slots out itself
int             mi_dlsch3_create(mi_lte_ctx *ctx, const mi_lte_dlsch_cfg *cfg, MiDlsch3Layout &&lay, uint32_t n_alloc, MiDlsch3 **out, uint32_t n_l = 1);
int             mi_dlsch3_create(mi_lte_ctx *ctx, const mi_lte_dlsch_cfg *cfg, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, MiDlsch3 **out, uint32_t n_l = 1);
void            mi_dlsch3_free(MiDlsch3 *g);
int             mi_dlsch3_run(mi_lte_ctx *ctx, MiDlsch3 *g, mi_lte_harq_pool *p, const mi_lte_harq_bind *h_bind, const MiDecodeIO &io, uint32_t decoder, uint32_t n_iter);
int             mi_dlsch3_cb_soft(const MiDlsch3 *g, uint32_t alloc, const int8_t **d_blocks, uint32_t *C, uint32_t *K);
const uint32_t *mi_dlsch3_cb_ok(const MiDlsch3 *g);
int             mi_dlsch3_harq_check(mi_lte_ctx *ctx, const MiDlsch3 *g, const mi_lte_harq_pool *p, const mi_lte_harq_bind *h_bind);
