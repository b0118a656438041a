// Where the control region lives in the subframe grid: the PCFICH / PHICH resource-element groups of symbol 0, the PDCCH's REG walk with its
// exclusions, the REG interleaver with the cell's cyclic shift, the CCEs and the six common-search-space candidates, and the convolutional
// rate-matching index map.  Index arithmetic by cell, bandwidth, N_g and region size, shared by the receiver's plans (pdcch.hip), the transmitter
// (tx_ctrl.cc) and the synthesiser (pdcch_synth.cc).  Plain C++: no HIP, no context.
#pragma once
#include <cstdint>
#include <vector>

namespace pdcch_geom {

constexpr int      N_SC_MAX = 1200; // row stride of every subframe array
constexpr uint32_t N_CAND = 6, RE_MAX = 288, NO_RE = 0xFFFFFFFFu;

// the six LTE bandwidths and a PHICH resource N_g in (0, 2] (36.211 6.9: 1/6, 1/2, 1, 2): what bounds the REG tables below (a negative or
// not-a-number N_g would size them by a wrapped group count)
inline bool standard_ctrl_cfg(uint32_t nrb, float phich_res)
{
    return (nrb == 6 || nrb == 15 || nrb == 25 || nrb == 50 || nrb == 75 || nrb == 100) && phich_res > 0.0f && phich_res <= 2.0f;
}

// first sub-carrier k and REG number n of the four PCFICH REGs (pcfich_channel_demap, liblte_phy.cc:7903-7910)
void pcfich_regs(uint32_t N_rb_dl, uint32_t cell, uint32_t k[4], float n[4]);
// REG numbers of PHICH group m's three REGs, counted among the REGs the PCFICH left (phich_channel_demap :8243-8278); first sub-carrier = 6 n_hat
void phich_group_regs(uint32_t N_rb_dl, uint32_t cell, uint32_t m, const float pcfich_n[4], uint32_t n_hat[3]);
// both for a cell whose group count follows from N_g
struct CtrlRegs { uint32_t pcfich_k[4]; float pcfich_n[4]; std::vector<uint32_t> phich_k; };
// (regs_36211: the PHICH groups numbered as 36.211 6.9.3 writes it, over the REGs the PCFICH left in ascending order -- MI_LTE_PDCCH_SEARCH_36211_REGS)
CtrlRegs ctrl_regs(uint32_t N_rb_dl, uint32_t cell, float phich_res, bool regs_36211 = false);

// read-out order of the sub-block interleaver over n positions, dummies skipped (36.212 5.1.4.2.1): order[k] = natural position read k-th
void cc_interleaver_order(uint32_t n, std::vector<uint32_t> &order);
// the resource elements of every CCE of one (cell, N_symbs) in order, 36 per CCE: perm[36 N_cce ..] (plus the REGs behind the last whole CCE);
// returns N_cce.  regs_36211: ctrl_regs' numbering, and N_reg counted as 36.211 6.8.1 does (four ports lose N_rb groups to symbol 1's CRS only
// where the region has a symbol 1)
uint32_t cce_res(uint32_t N_rb_dl, uint32_t N_ant, uint32_t cell, float phich_res, uint32_t N_symbs, std::vector<uint32_t> &perm, bool regs_36211 = false);
// RE lists of the six common-search-space candidates for one (cell, N_symbs)
void candidate_res(uint32_t N_rb_dl, uint32_t N_ant, uint32_t cell, float phich_res, uint32_t N_symbs, uint32_t *out /*[N_CAND][RE_MAX]*/);
// where received bit k of E lands in d[3*N_c] (rate_unmatch_conv :11597-11755)
void conv_rm_map(uint32_t N_c, uint32_t E, uint16_t *map);

} // namespace pdcch_geom
