// The arithmetic half of a plan: see plan_arith.h.
#include "plan_arith.h"

#include <algorithm>

#include "lte_tables.h"

int mi_qpp_row_at_least(uint32_t B)
{
    if (B > 6144) return -1;
    // the sizes step by 8, 16, 32, 64 (36.212 table 5.1.3-3)
    int r = B <= 40 ? 0 : B <= 512 ? (int)((B - 40 + 7) / 8) : B <= 1024 ? 59 + (int)((B - 512 + 15) / 16) : B <= 2048 ? 91 + (int)((B - 1024 + 31) / 32)
                                                                                                                      : 123 + (int)((B - 2048 + 63) / 64);
    if (r >= LTE_QPP_N_SIZES || LTE_QPP_ROWS[r].K < B || (r > 0 && LTE_QPP_ROWS[r - 1].K >= B)) // (table and closed form disagree: fall back)
        for (r = 0; r < LTE_QPP_N_SIZES && LTE_QPP_ROWS[r].K < B; r++) {}
    return r < LTE_QPP_N_SIZES ? r : -1;
}

size_t mi_plan_soft_layout(const uint32_t *e_bits, uint32_t n_alloc, std::vector<uint32_t> &h_e_off)
{
    size_t off = 0;
    h_e_off.resize(n_alloc);
    for (uint32_t a = 0; a < n_alloc; a++) {
        h_e_off[a] = (uint32_t)(off >> 6); // in 64-byte units
        off += (e_bits[a] + 63) & ~63u;
    }
    return off;
}

// two passes and a counting sort: a capture's chunk re-plans tens of thousands of allocations per call
void mi_plan_group(const uint8_t *row, const uint32_t *n_cb, const uint32_t *e_bits, uint32_t n_alloc, std::vector<MiKGroup> &groups, std::vector<uint32_t> &slot_alloc)
{
    static_assert(LTE_QPP_N_SIZES <= 256, "size index fits a byte");
    uint32_t cnt[LTE_QPP_N_SIZES] = {0}, emax[LTE_QPP_N_SIZES] = {0}, base[LTE_QPP_N_SIZES], run = 0;
    for (uint32_t a = 0; a < n_alloc; a++) {
        cnt[row[a]] += n_cb ? n_cb[a] : 1u;
        if (e_bits) emax[row[a]] = std::max(emax[row[a]], e_bits[a]);
    }
    groups.clear();
    for (int r = 0; r < LTE_QPP_N_SIZES; r++) {
        base[r] = run;
        if (cnt[r]) groups.push_back({LTE_QPP_ROWS[r].K, cnt[r], run, emax[r]});
        run += cnt[r];
    }
    slot_alloc.resize(run);
    for (uint32_t a = 0; a < n_alloc; a++)
        for (uint32_t c = n_cb ? n_cb[a] : 1u; c; c--) slot_alloc[base[row[a]]++] = a;
}
