// CPU driver for the merged turbo decode's layout plan (openlte_amd/csrc/turbo_plan.cc), built with -fsanitize=address,undefined: plans a
// group list and then replays what the kernels do with the tables -- the index expressions of k_turbo_prep / k_turbo_vote, k_turbo_perm,
// k_turbo_siso, k_turbo_siso_small and k_cb_desc_multi (turbo.hip) -- and checks that every code block, tile and trellis of every size is
// reached exactly once, inside its own part of the scratch.  Inputs: the 188 sizes alone, neighbouring pairs, all sizes at once, the group
// lists of the files named on the command line ("K n_cb cb_base e_max" per line), seeded random lists.
//   turbo_plan_driver [random lists] [group file ...]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mi_lte.h"
#include "../../openlte_amd/csrc/lte_tables.h"
#include "../../openlte_amd/csrc/turbo_plan.hpp"

using namespace turbo_geom;
typedef std::vector<MiKGroup> Groups;
static const Groups *g_now = nullptr;
static long g_plans = 0, g_dealt = 0, g_one_size = 0, g_windowed = 0, g_whole = 0;

#define CHECK(cond)                                                                                                              \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            printf("turbo plan driver: %s:%d: %s is false for the %zu groups", __FILE__, __LINE__, #cond, g_now->size());        \
            for (size_t i_ = 0; i_ < g_now->size() && i_ < 8; i_++) printf(" {%u, %u, %u, %u}", (*g_now)[i_].K, (*g_now)[i_].n_cb, (*g_now)[i_].cb_base, (*g_now)[i_].e_max); \
            printf("%s\n", g_now->size() > 8 ? " ..." : "");                                                                     \
            exit(1);                                                                                                             \
        }                                                                                                                        \
    } while (0)

static uint32_t rx = 88172645u;
static uint32_t rnd() { rx ^= rx << 13; rx ^= rx >> 17; rx ^= rx << 5; return rx; }
static uint32_t log_uniform(uint32_t lo, uint32_t hi) { return std::min(hi, (uint32_t)(lo * std::exp(std::log((double)(hi + 1) / lo) * (rnd() / 4294967296.0)))); }

// counts[size][item], every item to be reached exactly once
struct Reach {
    std::vector<std::vector<uint8_t>> n;
    template <typename F> Reach(const Groups &g, F items) { for (const MiKGroup &gr : g) n.emplace_back(items(gr), 0); }
    void hit(uint32_t size, uint64_t item) { CHECK(item < n[size].size() && n[size][item] == 0); n[size][item] = 1; }
    void all_once() const { for (const auto &v : n) CHECK(std::count(v.begin(), v.end(), 1) == (long)v.size()); }
};

// the trellis kernel's launch over a pass's wavefronts (k_turbo_siso<true>)
static void replay_siso(const Groups &g, const MiMultiPlan &p, uint32_t mode)
{
    const MiMultiGeom &G = p.geom;
    const uint32_t n_wv_all = mode ? G.n_wv23 : G.n_wv1, n_ord = mode ? G.n_ord23 : G.n_ord1;
    const uint32_t *map = p.map.data() + (mode ? G.map_wv23 : G.map_wv1), *order = n_ord ? p.map.data() + (mode ? G.ord_wv23 : G.ord_wv1) : nullptr;
    // the launch order: only for many sizes and many workgroups, whole workgroups, a permutation of the wavefronts plus idle entries
    const uint32_t n_wg = (n_wv_all + 3) / 4;
    CHECK((n_ord != 0) == (g.size() >= 8 && n_wg >= 512));
    if (order) {
        CHECK(n_ord % 4 == 0 && n_ord >= n_wv_all && (mode ? G.ord_wv23 : G.ord_wv1) + (size_t)n_ord <= p.map.size());
        std::vector<uint8_t> seen(n_wv_all, 0);
        for (uint32_t j = 0; j < n_ord; j++) {
            if (order[j] < n_wv_all) { CHECK(!seen[order[j]]); seen[order[j]] = 1; }
            else CHECK(order[j] == 0xFFFFFFFFu);
        }
        CHECK(std::count(seen.begin(), seen.end(), 1) == (long)n_wv_all);
    }
    uint32_t sum = 0;
    for (const KSeg &sg : p.segs) sum += mode ? sg.n_tiles : (sg.n_tiles + 1) / 2;
    CHECK(sum == n_wv_all && map[0] == g.size() - 1); // the largest K first
    Reach walks(g, [&](const MiKGroup &gr) { return mode ? (gr.n_cb + 63) / 64 : ((gr.n_cb + 63) / 64 + 1) / 2; });
    Reach tiles(g, [](const MiKGroup &gr) { return (gr.n_cb + 63) / 64; });
    const uint32_t grid = n_ord ? n_ord / 4 : n_wg;
    for (uint32_t b = 0; b < grid; b++)
        for (uint32_t w = 0; w < 4; w++) {
            uint32_t wv = b * 4 + w;
            if (order) wv = order[wv];
            if (wv >= n_wv_all) continue;
            if (wv) CHECK(p.segs[map[wv]].K <= p.segs[map[wv - 1]].K);
            const uint32_t i = map[wv];
            CHECK(i < g.size());
            const KSeg &sg = p.segs[i];
            CHECK(wv >= (mode ? sg.wv23 : sg.wv1));
            wv -= mode ? sg.wv23 : sg.wv1;
            CHECK(wv < (mode ? sg.n_tiles : (sg.n_tiles + 1) / 2));
            walks.hit(i, wv);
            if (mode) tiles.hit(i, wv);
            else {
                tiles.hit(i, 2 * wv); // two tiles per wavefront, an odd count's last one twice
                if (std::min(2 * wv + 1, sg.n_tiles - 1) != 2 * wv) tiles.hit(i, 2 * wv + 1);
            }
        }
    walks.all_once();
    tiles.all_once();
}

static void check_plan(const Groups &g)
{
    g_now = &g;
    MiMultiPlan p;
    const char *err = nullptr;
    CHECK(mi_turbo_multi_plan(g.data(), (uint32_t)g.size(), &p, &err) == MI_LTE_OK && !err);
    const MiMultiGeom &G = p.geom;
    const uint32_t n = (uint32_t)g.size();
    CHECK(p.segs.size() == n && G.map_off == sizeof(KSeg) * n);

    // ---- rows and scratch: every size's tiles in group order, back to back
    uint64_t arr = 0;
    uint32_t slots = 0, kp_all = 0, tot = 0;
    for (uint32_t i = 0; i < n; i++) {
        const KSeg &sg = p.segs[i];
        CHECK(sg.K == g[i].K && sg.n_cb == g[i].n_cb && sg.cb_base == g[i].cb_base && sg.n_tiles == (g[i].n_cb + 63) / 64 && !sg.pi && !sg.inv2 && !sg.tabs && !sg.nnn && !sg.pad);
        CHECK(sg.arr_off == arr);
        arr += (uint64_t)sg.n_tiles * kpad64(sg.K) * 64;
        slots = std::max(slots, g[i].cb_base + g[i].n_cb);
        kp_all = std::max(kp_all, kpad64(sg.K));
        tot += g[i].n_cb;
        // staging: the whole of the longest allocation with its zero slot, or a window of a lap and a quarter; inside the 48 KiB either way
        const uint32_t lap54 = 15 * (sg.K + 4) / 4 + 64;
        CHECK(sg.e_cap % 64 == 0 && (sg.e_cap >= g[i].e_max + 16 || (sg.e_cap >= lap54 && sg.e_cap < lap54 + 64)) && prep_lds_bytes(kpad64(sg.K), sg.e_cap) <= 48 * 1024);
        (sg.e_cap >= g[i].e_max + 16 ? g_whole : g_windowed)++;
    }
    CHECK(G.arr_bytes == arr && G.n_slots == slots && G.kp_all == kp_all);

    // ---- widths
    for (int c = 0; c < NCLS; c++) {
        uint32_t lds = 0, kp = 0, n_in = 0, only = 0;
        for (uint32_t i = 0; i < n; i++)
            if (cb_class(g[i].K) == c) { lds = std::max(lds, prep_lds_bytes(kpad64(g[i].K), p.segs[i].e_cap)); kp = std::max(kp, kpad64(g[i].K)); n_in++; only = i; }
        CHECK(G.lds_prep[c] == lds && lds <= 48 * 1024 && G.kp_max[c] == kp && kp <= 1024u * (c + 1));
        CHECK((G.one_size[c] >= 0) == (n_in == 1 && g[only].n_cb % 64 == 0));
        if (G.one_size[c] >= 0) { CHECK((uint32_t)G.one_size[c] == only && G.off_one[c] == p.segs[only].arr_off && G.e_cap_one[c] == p.segs[only].e_cap); g_one_size++; }
    }

    // ---- prep, vote: blockIdx >> 9 names the size, - wg_cb the workgroup of its own grid, xcd_cb its code block
    // A workgroup whose code block lies past the size's last tile returns at once; every lane of every tile -- a code block, or an idle
    // lane of the last tile, which gets zeros -- is written by exactly one workgroup
    const auto tile_lanes = [](const MiKGroup &gr) { return (gr.n_cb + 63) / 64 * 64; };
    {
        Reach cbs(g, tile_lanes);
        for (int c = 0; c < NCLS; c++) {
            CHECK(G.grid_cb[c] % 512 == 0 && G.map_cb[c] + (size_t)(G.grid_cb[c] >> 9) <= p.map.size());
            for (uint32_t b = 0; b < G.grid_cb[c]; b++) {
                const uint32_t i = p.map[G.map_cb[c] + (b >> 9)];
                CHECK(i < n && cb_class(g[i].K) == c);
                const KSeg &sg = p.segs[i];
                CHECK(b >= sg.wg_cb && b - sg.wg_cb < 8 * xcd_chunk(sg.n_cb) && sg.wg_cb % 512 == 0);
                const uint32_t cb = xcd_cb(b - sg.wg_cb, sg.n_cb);
                if (cb < ((sg.n_cb + 63u) & ~63u)) cbs.hit(i, cb); // its code block, or zeros for an idle lane of the last tile; past that it returns
            }
        }
        cbs.all_once();
    }
    // ---- perm: blockIdx >> 7, - wg_perm, four blocks a grid apart
    {
        Reach cbs(g, tile_lanes);
        for (int c = 0; c < NCLS; c++) {
            CHECK(G.grid_perm[c] % 128 == 0 && G.map_perm[c] + (size_t)(G.grid_perm[c] >> 7) <= p.map.size());
            for (uint32_t b = 0; b < G.grid_perm[c]; b++) {
                const uint32_t i = p.map[G.map_perm[c] + (b >> 7)];
                CHECK(i < n && cb_class(g[i].K) == c);
                const KSeg &sg = p.segs[i];
                CHECK(b >= sg.wg_perm && b - sg.wg_perm < sg.perm_grid && sg.perm_grid % 128 == 0 && sg.perm_grid % 8 == 0);
                for (uint32_t it = 0; it < PERM_BLOCKS; it++) {
                    const uint32_t cb = xcd_cb(b - sg.wg_perm + it * sg.perm_grid, sg.n_cb);
                    if (cb < ((sg.n_cb + 63u) & ~63u)) cbs.hit(i, cb);
                }
            }
        }
        cbs.all_once();
    }
    // ---- the trellis kernel, pass 1 and passes 2 + 3
    replay_siso(g, p, 0);
    replay_siso(g, p, 1);
    if (G.n_ord1 || G.n_ord23) g_dealt++;
    CHECK((G.siso_pad1 != 0) == (n >= 8) && (G.siso_pad23 != 0) == (n >= 8));
    // ---- the state-parallel trellis kernel: workgroup = wavefront = up to gpw trellises of one size
    CHECK(G.gpw1 == gpw_of(tot) && G.gpw23 == gpw_of(2 * tot));
    for (uint32_t mode = 0; mode < 2; mode++) {
        const uint32_t gpw = mode ? G.gpw23 : G.gpw1, grid = mode ? G.n_ws23 : G.n_ws1, at = mode ? G.map_ws23 : G.map_ws1;
        Reach tr(g, [&](const MiKGroup &gr) { return (uint64_t)gr.n_cb * (mode ? 2u : 1u); });
        CHECK(at + (size_t)grid <= p.map.size());
        for (uint32_t b = 0; b < grid; b++) {
            const uint32_t i = p.map[at + b];
            CHECK(i < n);
            const KSeg &sg = p.segs[i];
            CHECK(b >= (mode ? sg.ws23 : sg.ws1));
            const uint32_t T0 = (b - (mode ? sg.ws23 : sg.ws1)) * gpw, n_tr = sg.n_cb * (mode ? 2u : 1u);
            CHECK(T0 < n_tr);
            for (uint32_t t = 0; t < std::min(gpw, n_tr - T0); t++) tr.hit(i, T0 + t);
        }
        tr.all_once();
    }
    // ---- k_cb_desc_multi: the last row with cb_base <= slot
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t cb = g[i].cb_base; cb < g[i].cb_base + g[i].n_cb; cb++) {
            uint32_t lo = 0, hi = n;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (p.segs[mid].cb_base <= cb) lo = mid; else hi = mid;
            }
            CHECK(lo == i);
        }
    g_plans++;
}

static void check_refusals()
{
    const Groups ok = {{40, 1, 0, 120}, {48, 1, 1, 144}};
    g_now = &ok;
    const auto refused = [](const Groups &g, uint32_t n, bool message) {
        MiMultiPlan p;
        const char *err = nullptr;
        return mi_turbo_multi_plan(g.data(), n, &p, &err) == MI_LTE_ERR_INVALID_ARG && (err != nullptr) == message;
    };
    CHECK(refused(ok, 0, false));
    CHECK(refused({{48, 1, 0, 144}, {40, 1, 1, 120}}, 2, true)); // falling K
    CHECK(refused({{40, 1, 0, 120}, {40, 1, 1, 120}}, 2, true)); // one K twice
    CHECK(refused({{40, 1, 0, 120}, {48, 0, 1, 144}}, 2, true)); // an empty group
    CHECK(refused(Groups(0x10000, MiKGroup{40, 1, 0, 120}), 0x10000, false));
}

int main(int argc, char **argv)
{
    const int n_random = argc > 1 ? atoi(argv[1]) : 3000;
    const auto K_of = [](uint32_t r) { return (uint32_t)LTE_QPP_ROWS[r].K; };
    check_refusals();
    static const uint32_t counts[6] = {1, 63, 64, 65, 4096, 4097};
    for (uint32_t r = 0; r < LTE_QPP_N_SIZES; r++)
        for (uint32_t a : counts) {
            check_plan({{K_of(r), a, 0, 3 * K_of(r) + 12}}); // a size alone
            if (r + 1 < LTE_QPP_N_SIZES)
                for (uint32_t b : counts) check_plan({{K_of(r), a, 0, 3 * K_of(r) + 12}, {K_of(r + 1), b, a, 6 * K_of(r + 1)}});
        }
    for (uint32_t each : {1u, 64u}) { // all sizes at once
        Groups g;
        for (uint32_t r = 0; r < LTE_QPP_N_SIZES; r++) g.push_back({K_of(r), each, r * each, 3 * K_of(r) + 12});
        check_plan(g);
    }
    for (int f = 2; f < argc; f++) { // group lists from files
        Groups   g;
        MiKGroup gr;
        FILE    *fp = fopen(argv[f], "r");
        if (!fp) { printf("turbo plan driver: cannot read %s\n", argv[f]); return 1; }
        while (fscanf(fp, "%u %u %u %u", &gr.K, &gr.n_cb, &gr.cb_base, &gr.e_max) == 4) g.push_back(gr);
        fclose(fp);
        check_plan(g);
    }
    // Random lists: 1..20 000 code blocks per size, log-uniform; 2..12 sizes (a per-call caller's subframe), every fourth list 2..188 sizes,
    // log-uniform, and every 64th 8..188 sizes, uniform, of 2000 code blocks or more each, so that the launch order is dealt often enough;
    // e_max up to the 258 laps the merged decode takes; slots with gaps
    for (int it = 0; it < n_random; it++) {
        const bool     big = it % 64 == 0;
        const uint32_t n = big ? 8 + rnd() % 181 : it % 4 == 1 ? log_uniform(2, 188) : 2 + rnd() % 11, lo = big ? 2000 : 1;
        std::vector<uint32_t> rows(LTE_QPP_N_SIZES);
        for (uint32_t r = 0; r < LTE_QPP_N_SIZES; r++) rows[r] = r;
        for (uint32_t r = 0; r < n; r++) std::swap(rows[r], rows[r + rnd() % (LTE_QPP_N_SIZES - r)]);
        std::sort(rows.begin(), rows.begin() + n);
        Groups   g;
        uint32_t base = 0;
        for (uint32_t r = 0; r < n; r++) {
            const uint32_t K = K_of(rows[r]), e_hi = rnd() % 2 ? 3 * (3 * K + 12) : 258 * (3 * K - 81);
            base += rnd() % 4 ? 0 : rnd() % 100;
            g.push_back({K, log_uniform(lo, 20000), base, rnd() % (e_hi + 1)});
            base += g.back().n_cb;
        }
        check_plan(g);
    }
    printf("turbo plan driver: %ld plans checked, %ld with a dealt launch order, %ld one-size widths, %ld sizes staged whole, %ld windowed\n", g_plans, g_dealt, g_one_size, g_whole,
           g_windowed);
    return 0;
}
