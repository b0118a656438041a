// PHICH geometry and resource arithmetic (phich_geom.h).  The positions are those the transmitter writes (phich_channel_map,
// liblte_phy.cc:8076-8215) and the reference's demapper reports (phich_channel_demap :8243-8278); the group count and the
// (group, sequence) pair of an uplink grant are 36.211 6.9 and 36.213 9.1.2 with N_SF = 4 (normal cyclic prefix).
#include <cmath>

#include "../../include/mi_lte.h"
#include "pdcch_geom.h"
#include "phich_geom.h"

namespace phich_geom {

uint32_t n_group(uint32_t N_rb_dl, float phich_res)
{
    if (!pdcch_geom::standard_ctrl_cfg(N_rb_dl, phich_res)) return 0;
    return (uint32_t)ceilf((float)phich_res * ((float)N_rb_dl / (float)8)); // (the expression of pdcch_geom::ctrl_regs, so the two agree)
}

void group_res(uint32_t N_rb_dl, uint32_t cell, uint32_t m, const float pcfich_n[4], uint32_t re[N_RE])
{
    uint32_t n_hat[3];
    pdcch_geom::phich_group_regs(N_rb_dl, cell, m, pcfich_n, n_hat);
    for (uint32_t i = 0, idx = 0; i < 3; i++)
        for (uint32_t j = 0; j < 6; j++)
            if ((cell % 3) != (j % 3)) re[idx++] = 6 * n_hat[i] + j; // skip the CRS positions
}

bool cell_res(uint32_t N_rb_dl, uint32_t cell, float phich_res, std::vector<uint32_t> &re)
{
    re.clear();
    const uint32_t N_group = n_group(N_rb_dl, phich_res);
    if (N_group == 0 || N_group > MAX_GROUP || cell > 503) return false;
    uint32_t k[4];
    float    n[4];
    pdcch_geom::pcfich_regs(N_rb_dl, cell, k, n);
    re.resize((size_t)N_group * N_RE);
    for (uint32_t m = 0; m < N_group; m++) group_res(N_rb_dl, cell, m, n, &re[(size_t)m * N_RE]);
    for (uint32_t x : re)
        if (x >= 12 * N_rb_dl) { re.clear(); return false; }
    return true;
}

} // namespace phich_geom

extern "C" {

uint32_t mi_lte_phich_n_group(uint32_t N_rb_dl, float phich_res) { return phich_geom::n_group(N_rb_dl, phich_res); }

int mi_lte_phich_resource(uint32_t I_prb_ra_lowest, uint32_t n_dmrs, uint32_t N_group, uint32_t I_phich, uint32_t *n_group, uint32_t *n_seq)
{
    if (!n_group || !n_seq || N_group == 0 || n_dmrs > 7) return MI_LTE_ERR_INVALID_ARG;
    *n_group = (uint32_t)((((uint64_t)I_prb_ra_lowest + n_dmrs) % N_group + (uint64_t)I_phich * N_group) & 0xFFFFFFFFu);
    *n_seq   = (uint32_t)(((uint64_t)(I_prb_ra_lowest / N_group) + n_dmrs) % phich_geom::N_SEQ); // 2 N_SF = 8
    return MI_LTE_OK;
}

int mi_lte_phich_re_table(uint32_t N_rb_dl, uint32_t N_id_cell, float phich_res, uint32_t *N_group, uint32_t *re /*[25][12]*/)
{
    if (!N_group || !re) return MI_LTE_ERR_INVALID_ARG;
    std::vector<uint32_t> t;
    if (!phich_geom::cell_res(N_rb_dl, N_id_cell, phich_res, t)) return MI_LTE_ERR_INVALID_ARG;
    *N_group = (uint32_t)(t.size() / phich_geom::N_RE);
    for (size_t i = 0; i < t.size(); i++) re[i] = t[i];
    return MI_LTE_OK;
}

} // extern "C"
