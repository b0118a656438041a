// The arithmetic every plan (PDSCH: chain.hip, PUSCH: pusch_plan.cc, 3GPP transport-block mode: dlsch3_layout.cc) does before it owns any device
// memory: code-block size lookup, soft-bit layout, code-block slots grouped by size, the output stride.  Integer arithmetic on host arrays --
// no HIP, no context: plan_core.hpp adds the device half.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "turbo_plan.hpp" // MiKGroup

// Row of LTE_QPP_ROWS (lte_tables.h) of the first code-block size >= B, -1 when B > 6144.
int mi_qpp_row_at_least(uint32_t B);
// The code-block row of a single-block transport block of tbs bits (B = tbs + 24), -1 when it needs more than one block (tbs > 6120).  The
// bound comes before the addition: a tbs near 2^32 does not wrap into the envelope.
inline int mi_tb_row(uint32_t tbs) { return tbs > 6144 - 24 ? -1 : mi_qpp_row_at_least(tbs + 24); }

// Bytes between two allocations' decoded transport blocks: room for the largest, a multiple of 64 (one bit per byte, or eight when packed)
inline uint32_t mi_out_stride(uint32_t tbs, bool packed) { return packed ? (((tbs + 7) / 8 + 63) & ~63u) : ((tbs + 63) & ~63u); }

// Soft-bit layout: allocation a's e_bits[a] soft bits start h_e_off[a] 64-byte units into the plan's buffer (each padded to 64 bytes).  Returns the buffer's bytes.
size_t mi_plan_soft_layout(const uint32_t *e_bits, uint32_t n_alloc, std::vector<uint32_t> &h_e_off);

// Grouping: allocation a has n_cb[a] code blocks (nullptr: one each) of size row[a] (mi_qpp_row_at_least).  Groups in ascending block
// size; inside a size the allocations in their own order, an allocation's blocks adjacent.  slot_alloc receives the allocation of every
// code-block slot; a group's e_max is its longest allocation's e_bits (nullptr: 0).  A counting sort over the 188 sizes.
void mi_plan_group(const uint8_t *row, const uint32_t *n_cb, const uint32_t *e_bits, uint32_t n_alloc, std::vector<MiKGroup> &groups, std::vector<uint32_t> &slot_alloc);
