// CPU driver for the PHICH host arithmetic (openlte_amd/csrc/phich_geom.cc), built with -fsanitize=address,undefined: walks the entry points
// over their whole argument ranges, the refused ones included, with outputs of exactly the documented size, and checks what must hold:
//   - mi_lte_phich_n_group equals N_reg / 3 of mi_lte_ctrl_reg_positions on the 6 x 4 standard combinations and is 0 anywhere else;
//   - mi_lte_phich_resource equals 36.213 9.1.2 (N_SF = 4) for I_prb 0..109 and at the ends of the 32-bit range, n_dmrs 0..8, N_group 0..26,
//     I_phich 0..1, and leaves its outputs alone when it refuses;
//   - every entry of mi_lte_phich_re_table lies inside the carrier off the CRS positions, each REG's first sub-carrier is
//     mi_lte_ctrl_reg_positions' and its four elements ascend, for every cell 0..503 (the reference's numbering steps over the PCFICH REGs in
//     the order they are listed, not in ascending order, so in some cells a PHICH REG lands on a PCFICH REG: the positions are the
//     reference's, not checked for that here); cells past 503 and non-standard configurations are refused.
// Prints "phich host driver: <calls> calls, <checks> checks, 0 failures" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mi_lte.h"
#include "../../openlte_amd/csrc/phich_geom.h"

static long n_calls = 0, n_checks = 0, n_fail = 0;
#define CHECK(cond, ...) do { n_checks++; if (!(cond)) { if (n_fail++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// an output on the heap at its exact size, so that a write past it is a report
template <typename T> static std::vector<T> fresh(size_t n) { std::vector<T> v(n); memset(v.data(), 0xA5, n * sizeof(T)); return v; }

static const uint32_t BW[6] = {6, 15, 25, 50, 75, 100};
static const float    NGS[4] = {1.0f / 6, 0.5f, 1.0f, 2.0f};

static void group_count()
{
    for (uint32_t nrb = 0; nrb <= 111; nrb++)
        for (float ng : {-1.0f, 0.0f, 1.0f / 6, 0.5f, 1.0f, 2.0f, 2.5f, NAN, INFINITY}) {
            bool standard = ng > 0.0f && ng <= 2.0f;
            bool bw = false;
            for (uint32_t b : BW) bw = bw || b == nrb;
            const uint32_t n = mi_lte_phich_n_group(nrb, ng);
            n_calls++;
            if (!(standard && bw)) { CHECK(n == 0, "N_rb %u N_g %g: %u groups", nrb, ng, n); continue; }
            auto k = fresh<uint32_t>(4), n_reg = fresh<uint32_t>(1), pk = fresh<uint32_t>(75);
            auto nn = fresh<float>(4);
            CHECK(mi_lte_ctrl_reg_positions(nrb, 17, ng, k.data(), nn.data(), n_reg.data(), pk.data()) == MI_LTE_OK && n_reg[0] == 3 * n && n >= 1 && n <= phich_geom::MAX_GROUP,
                  "N_rb %u N_g %g: %u groups, %u REGs", nrb, ng, n, n_reg[0]);
        }
}

static void resource()
{
    const uint32_t prbs[6] = {0x7FFFFFFFu, 0x80000000u, 0xFFFFFFF8u, 0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t N_group = 0; N_group <= 26; N_group++)
        for (uint32_t I_phich = 0; I_phich <= 1; I_phich++)
            for (uint32_t n_dmrs = 0; n_dmrs <= 8; n_dmrs++)
                for (uint32_t i = 0; i < 110 + 6; i++) {
                    const uint32_t I_prb = i < 110 ? i : prbs[i - 110];
                    auto           g = fresh<uint32_t>(1), s = fresh<uint32_t>(1);
                    const int      rc = mi_lte_phich_resource(I_prb, n_dmrs, N_group, I_phich, g.data(), s.data());
                    n_calls++;
                    if (N_group == 0 || n_dmrs > 7) {
                        CHECK(rc == MI_LTE_ERR_INVALID_ARG && g[0] == 0xA5A5A5A5u && s[0] == 0xA5A5A5A5u, "refusal I_prb %u n_dmrs %u N_group %u: %d", I_prb, n_dmrs, N_group, rc);
                        continue;
                    }
                    const uint64_t want_g = ((uint64_t)I_prb + n_dmrs) % N_group + (uint64_t)I_phich * N_group, want_s = ((uint64_t)(I_prb / N_group) + n_dmrs) % 8;
                    CHECK(rc == MI_LTE_OK && g[0] == want_g && s[0] == want_s && g[0] < 2 * N_group && s[0] < 8, "I_prb %u n_dmrs %u N_group %u I_phich %u: %d, (%u, %u)", I_prb, n_dmrs,
                          N_group, I_phich, rc, g[0], s[0]);
                }
    auto g = fresh<uint32_t>(1);
    CHECK(mi_lte_phich_resource(1, 1, 1, 0, nullptr, g.data()) == MI_LTE_ERR_INVALID_ARG && mi_lte_phich_resource(1, 1, 1, 0, g.data(), nullptr) == MI_LTE_ERR_INVALID_ARG, "null outputs");
}

static void table()
{
    for (uint32_t nrb : BW)
        for (float ng : NGS)
            for (uint32_t cell = 0; cell <= 503; cell++) {
                const uint32_t want = mi_lte_phich_n_group(nrb, ng);
                auto           n = fresh<uint32_t>(1), re = fresh<uint32_t>(12 * (size_t)want); // (exactly what the call fills)
                auto           k = fresh<uint32_t>(4), n_reg = fresh<uint32_t>(1), pk = fresh<uint32_t>(75);
                auto           nn = fresh<float>(4);
                CHECK(mi_lte_phich_re_table(nrb, cell, ng, n.data(), re.data()) == MI_LTE_OK && n[0] == want, "N_rb %u N_g %g cell %u: %u groups", nrb, ng, cell, n[0]);
                CHECK(mi_lte_ctrl_reg_positions(nrb, cell, ng, k.data(), nn.data(), n_reg.data(), pk.data()) == MI_LTE_OK && n_reg[0] == 3 * want, "positions N_rb %u cell %u", nrb, cell);
                n_calls += 2;
                bool ok = true;
                for (uint32_t i = 0; ok && i < 12 * want; i++) {
                    const uint32_t x = re[i];
                    ok = x < 12 * nrb && x % 3 != cell % 3 && x / 6 * 6 == pk[i / 4] && (i % 4 == 0 || x > re[i - 1]);
                }
                CHECK(ok, "N_rb %u N_g %g cell %u: an element off the carrier, on a CRS position, off its REG or out of order", nrb, ng, cell);
            }
    auto n = fresh<uint32_t>(1), re = fresh<uint32_t>(300);
    const struct { uint32_t nrb, cell; float ng; } refused[7] = {{7, 0, 1.0f}, {25, 504, 1.0f}, {25, 0xFFFFFFFFu, 1.0f}, {25, 0, 0.0f}, {25, 0, 2.5f}, {25, 0, NAN}, {0, 0, 1.0f}};
    for (const auto &r : refused) {
        CHECK(mi_lte_phich_re_table(r.nrb, r.cell, r.ng, n.data(), re.data()) == MI_LTE_ERR_INVALID_ARG && n[0] == 0xA5A5A5A5u && re[0] == 0xA5A5A5A5u, "refusal N_rb %u cell %u N_g %g", r.nrb,
              r.cell, r.ng);
        n_calls++;
    }
    CHECK(mi_lte_phich_re_table(25, 0, 1.0f, nullptr, re.data()) == MI_LTE_ERR_INVALID_ARG && mi_lte_phich_re_table(25, 0, 1.0f, n.data(), nullptr) == MI_LTE_ERR_INVALID_ARG, "null outputs");
    std::vector<uint32_t> t;
    CHECK(!phich_geom::cell_res(25, 504, 1.0f, t) && t.empty() && phich_geom::cell_res(100, 503, 2.0f, t) && t.size() == 300, "cell_res");
}

int main()
{
    group_count();
    resource();
    table();
    printf("phich host driver: %ld calls, %ld checks, %ld failures\n", n_calls, n_checks, n_fail);
    return n_fail ? 1 : 0;
}
