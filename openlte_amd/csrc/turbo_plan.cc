// The layout plan of a merged turbo decode: see turbo_plan.hpp.  Pure host arithmetic -- no context, no HIP call.
#include "turbo_plan.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/mi_lte.h"

using namespace turbo_geom;

namespace {

// One map of the blob: count(i) / per entries of i for the sizes that `take`, in rising or falling order; where each size starts (in
// counts, not entries) goes into its row, the total is returned.
template <typename Take, typename Count>
uint32_t append_map(MiMultiPlan &p, bool falling, Take take, Count count, uint32_t per, uint32_t KSeg::*start)
{
    const uint32_t n = (uint32_t)p.segs.size();
    uint32_t       total = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t i = falling ? n - 1 - j : j;
        if (!take(i)) continue;
        p.segs[i].*start = total;
        p.map.insert(p.map.end(), count(i) / per, i);
        total += count(i);
    }
    return total;
}

// The order the trellis kernel's workgroups are LAUNCHED in.  A walk is as long as its block size, the device holds 1024 workgroups of four
// walks at a time, and a mixed batch has little more than that (pass 1) or twice that (passes 2 + 3): with the longest walks simply first,
// a compute unit's four resident workgroups are neighbours in the sorted order and the unit that got the four longest decides when the
// launch ends.  Dealt out in rounds of 256 (one workgroup per compute unit and round), every other round backwards, each unit gets the
// r-th longest of one round with the r-th shortest of the next: equal sums (0.07 ms of the mixed batch's 3.6; a scatter that gives up
// "longest first" costs 1.3).  Batches of a few sizes (W4) keep the sorted order: *n_out stays 0.
void deal(std::vector<uint32_t> &map, bool many_sizes, uint32_t n_wv, uint32_t *at, uint32_t *n_out)
{
    const uint32_t n_wg = (n_wv + 3) / 4;
    if (!many_sizes || n_wg < 512) return;
    *at = (uint32_t)map.size();
    for (uint32_t j = 0; j < n_wg; j++) {
        const uint32_t round = j / 256, c = j % 256, in_round = std::min(256u, n_wg - 256 * round);
        const uint32_t src = (round & 1u) ? 256 * round + (in_round - 1 - std::min(c, in_round - 1)) : j;
        for (uint32_t t = 0; t < 4; t++) map.push_back(4 * src + t < n_wv ? 4 * src + t : 0xFFFFFFFFu);
    }
    *n_out = 4 * n_wg;
}

} // namespace

int mi_turbo_multi_plan(const MiKGroup *groups, uint32_t n_groups, MiMultiPlan *out, const char **err)
{
    if (!groups || n_groups == 0 || n_groups > 0xFFFF || !out) return MI_LTE_ERR_INVALID_ARG;
    MiMultiGeom &G = out->geom;
    G = MiMultiGeom{};
    out->segs.resize(n_groups);
    out->map.clear();
    uint32_t tot = 0;
    for (uint32_t i = 0; i < n_groups; i++) {
        const MiKGroup &gr = groups[i];
        if ((i && gr.K <= groups[i - 1].K) || gr.n_cb == 0) {
            if (err) *err = "merged decode: groups must be non-empty and in ascending block size";
            return MI_LTE_ERR_INVALID_ARG;
        }
        KSeg &sg = out->segs[i];
        memset(&sg, 0, sizeof(sg));
        const uint32_t Kp = kpad64(gr.K);
        sg.K = gr.K; sg.n_cb = gr.n_cb; sg.cb_base = gr.cb_base; sg.n_tiles = (gr.n_cb + 63) / 64;
        sg.perm_grid = perm_grid_of(gr.n_cb);
        sg.e_cap     = merged_e_cap(gr.K, gr.e_max);
        sg.arr_off   = G.arr_bytes;
        G.arr_bytes += (uint64_t)sg.n_tiles * Kp * 64;
        G.n_slots = std::max(G.n_slots, gr.cb_base + gr.n_cb);
        const int c = cb_class(gr.K);
        // (a size whose last tile is partly filled stays with the table kernel: it zeroes the idle lanes the trellis kernel will walk)
        G.one_size[c] = (G.lds_prep[c] == 0 && gr.n_cb % 64 == 0) ? (int)i : -1; // the width's only size so far, or not the only one
        G.off_one[c] = sg.arr_off; G.e_cap_one[c] = sg.e_cap;
        G.lds_prep[c] = std::max(G.lds_prep[c], prep_lds_bytes(Kp, sg.e_cap));
        G.kp_max[c]   = std::max(G.kp_max[c], Kp);
        G.kp_all      = std::max(G.kp_all, Kp);
        tot += gr.n_cb;
    }
    const auto all = [](uint32_t) { return true; };
    // workgroup -> size maps of the per-code-block kernels, one entry per 512 (prep, vote) / 128 (perm) workgroups -- a few KB: they stay in the scalar cache --, class after class
    for (int c = 0; c < NCLS; c++) {
        G.map_cb[c]  = (uint32_t)out->map.size();
        G.grid_cb[c] = append_map(*out, false, [&](uint32_t i) { return cb_class(groups[i].K) == c; }, [&](uint32_t i) { return cb_grid(groups[i].n_cb); }, 512, &KSeg::wg_cb);
    }
    for (int c = 0; c < NCLS; c++) {
        G.map_perm[c]  = (uint32_t)out->map.size();
        G.grid_perm[c] = append_map(*out, false, [&](uint32_t i) { return cb_class(groups[i].K) == c; }, [&](uint32_t i) { return out->segs[i].perm_grid; }, 128, &KSeg::wg_perm);
    }
    // wavefront -> size maps of the trellis kernel, the largest sizes first (their walks are the longest: started first, the short ones fill in behind them)
    G.map_wv1  = (uint32_t)out->map.size();
    G.n_wv1    = append_map(*out, true, all, [&](uint32_t i) { return (out->segs[i].n_tiles + 1) / 2; }, 1, &KSeg::wv1);
    G.map_wv23 = (uint32_t)out->map.size();
    G.n_wv23   = append_map(*out, true, all, [&](uint32_t i) { return out->segs[i].n_tiles; }, 1, &KSeg::wv23);
    // Their launch order (deal), and how many of the kernel's workgroups a compute unit holds at a time.  The registers allow four (16 walks
    // per unit, 4096 in all): right for W4, whose walks are equally long and come in more than two rounds of that.  A mixed batch of this
    // size has 1.2 rounds (pass 1) and 2.3 (passes 2 + 3) of walks between 44 and 4612 steps: the units that drew short ones run dry and
    // nothing is left to hand them.  Half as many resident workgroups are twice as many rounds -- the queue stays non-empty until close to
    // the end -- at the price of fewer wavefronts to hide latency behind; measured on the mixed batch (profiles/r06_variants_siso_occupancy.txt): 2 per unit for pass 1 and 3 for passes
    // 2 + 3 take 0.12-0.15 ms off the trellis kernel's 3.6, one per unit costs 0.15.  The limit is set with dynamic LDS that the kernel never touches.
    const bool many_sizes = n_groups >= 8;
    if (many_sizes) { G.siso_pad1 = 60000; G.siso_pad23 = 45000; } // (+ the kernel's own 8 KB: two / three of them in a unit's 160 KB)
    deal(out->map, many_sizes, G.n_wv1, &G.ord_wv1, &G.n_ord1);
    deal(out->map, many_sizes, G.n_wv23, &G.ord_wv23, &G.n_ord23);
    // ... and of the state-parallel trellis kernel (a handful of code blocks in all): workgroup = wavefront = up to gpw trellises of one size
    G.gpw1 = gpw_of(tot); G.gpw23 = gpw_of(2 * tot);
    G.map_ws1  = (uint32_t)out->map.size();
    G.n_ws1    = append_map(*out, false, all, [&](uint32_t i) { return (groups[i].n_cb + G.gpw1 - 1) / G.gpw1; }, 1, &KSeg::ws1);
    G.map_ws23 = (uint32_t)out->map.size();
    G.n_ws23   = append_map(*out, false, all, [&](uint32_t i) { return (2 * groups[i].n_cb + G.gpw23 - 1) / G.gpw23; }, 1, &KSeg::ws23);
    G.map_off  = sizeof(KSeg) * n_groups;
    return MI_LTE_OK;
}
