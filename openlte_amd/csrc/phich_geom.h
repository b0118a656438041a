// Where the PHICH lives and which PHICH answers which PUSCH: the group count of 36.211 6.9, the twelve resource elements of every group in
// symbol 0 (the REGs of pdcch_geom::phich_group_regs, the same source the PDCCH tables exclude) and the (group, sequence) pair of
// 36.213 9.1.2.  Index arithmetic shared by the receiver's plan (phich.hip) and the entry points of include/mi_lte.h.  Plain C++: no HIP,
// no context.
#pragma once
#include <cstdint>
#include <vector>

namespace phich_geom {

constexpr uint32_t N_SEQ = 8, N_RE = 12, MAX_GROUP = 25; // N_SF = 4: eight sequences, three quadruplets; 25 groups at 100 RB, N_g = 2

// ceil(N_g N_rb_dl / 8), formed as pdcch_geom::ctrl_regs forms it; 0 outside pdcch_geom::standard_ctrl_cfg
uint32_t n_group(uint32_t N_rb_dl, float phich_res);
// grid index (symbol 0: the sub-carrier k) of RE(4 i + j) of group m: REG i's four sub-carriers with k mod 3 != cell mod 3, in increasing k
void group_res(uint32_t N_rb_dl, uint32_t cell, uint32_t m, const float pcfich_n[4], uint32_t re[N_RE]);
// all groups of one cell, re[12 m + 4 i + j]; false (re left empty) when the configuration is not standard, the cell past 503 or an index
// would leave the carrier
bool cell_res(uint32_t N_rb_dl, uint32_t cell, float phich_res, std::vector<uint32_t> &re);

} // namespace phich_geom
