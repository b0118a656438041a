// CPU driver for the PDCCH host arithmetic (openlte_amd/csrc/dci.cc, pdcch_geom.cc, pdcch_synth.cc), built with -fsanitize=address,undefined:
// walks the entry points over the grids of tools/pdcch_host_compare.py (a coarser cell stride, fewer payloads) with out-structs of exactly
// the documented size, and checks what must hold whatever the reference says:
//   - pack -> unpack round trips of format 1A for a common RNTI and of formats 0 / 1A for a C-RNTI, every (N_prb, start) at N_rb 6..110;
//   - every candidate of mi_lte_pdcch_search_space lies inside N_cce on a multiple of L;
//   - every cce_res entry below 36 N_cce is a grid index of the region and none repeats;
//   - conv_rm_map stays below 3 N_c for N_c 24..80 and E in {72, 144, 288, 576}.
// Prints "pdcch host driver: <calls> calls, <checks> checks, 0 failures" and returns 0, or the first failures and 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mi_lte.h"
#include "../../openlte_amd/csrc/dci.h"
#include "../../openlte_amd/csrc/lte_tables.h"
#include "../../openlte_amd/csrc/pdcch_geom.h"

static long n_calls = 0, n_checks = 0, n_fail = 0;
#define CHECK(cond, ...) do { n_checks++; if (!(cond)) { if (n_fail++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t rnd_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }

// an out-struct on the heap at its exact size, so that a write past it is a report
template <typename T> static std::unique_ptr<T> fresh() { auto p = std::make_unique<T>(); memset(p.get(), 0xA5, sizeof(T)); return p; }
template <typename T> static std::vector<T> fresh(size_t n) { std::vector<T> v(n); memset(v.data(), 0xA5, n * sizeof(T)); return v; }

static const uint32_t BW[6] = {6, 15, 25, 50, 75, 100};

static void unpackers()
{
    const uint32_t rntis[5] = {0xFFFF, 0xFFFE, 1, 0x3C, 0x100}, ports[3] = {1, 2, 4};
    for (uint32_t nrb : BW) {
        uint32_t sz[2];
        dci::sizes(nrb, &sz[0], &sz[1]);
        for (uint32_t nb : sz)
            for (uint32_t rnti : rntis)
                for (uint32_t ant : ports)
                    for (int i = 0; i < 100; i++) {
                        auto o = fresh<mi_lte_pdcch_dci>();
                        mi_lte_dci_1a_unpack((uint32_t)rnd(), nb, rnti, nrb, ant, o.get());
                        mi_lte_dci_1c_unpack((uint32_t)rnd(), nb, rnti, nrb, ant, o.get());
                        n_calls += 2;
                    }
    }
    for (uint32_t nrb = 0; nrb <= 111; nrb++)
        for (uint32_t nb = 0; nb <= 33; nb++) {
            auto o = fresh<mi_lte_pdcch_dci>();
            mi_lte_dci_1a_unpack((uint32_t)rnd(), nb, 0xFFFF, nrb, 2, o.get());
            mi_lte_dci_1c_unpack((uint32_t)rnd(), nb, 0xFFFF, nrb, 2, o.get());
            n_calls += 2;
        }
    for (uint32_t nrb = 0; nrb <= 111; nrb++)
        for (uint32_t nb = 0; nb <= 65; nb++)
            for (int i = 0; i < 4; i++) {
                auto o = fresh<mi_lte_dci_crnti>();
                const int rc = mi_lte_dci_0_1a_unpack_crnti(i == 3 ? ~0ull : rnd(), nb, 0x1234, nrb, 2, o.get());
                CHECK((nrb >= 1 && nrb <= 110 && nb >= 1 && nb <= 64) || rc == MI_LTE_ERR_INVALID_ARG, "N_rb %u n_bits %u: %d", nrb, nb, rc);
                n_calls++;
            }
    auto o = fresh<mi_lte_dci_crnti>();
    CHECK(mi_lte_dci_0_1a_unpack_crnti(1, 43, 0, 100, 1, o.get()) == MI_LTE_ERR_INVALID_ARG && mi_lte_dci_0_1a_unpack_crnti(1, 43, 0x10000, 100, 1, o.get()) == MI_LTE_ERR_INVALID_ARG &&
          mi_lte_dci_0_1a_unpack_crnti(1, 43, 5, 100, 3, o.get()) == MI_LTE_ERR_INVALID_ARG && mi_lte_dci_0_1a_unpack_crnti(1, 43, 5, 100, 1, nullptr) == MI_LTE_ERR_INVALID_ARG, "crnti refusals");
    CHECK(mi_lte_dci_1a_unpack(1, 28, 0xFFFF, 100, 1, nullptr) == MI_LTE_ERR_INVALID_ARG && mi_lte_dci_1c_unpack(1, 15, 0xFFFF, 100, 1, nullptr) == MI_LTE_ERR_INVALID_ARG, "null out");
}

// what the transmitter's packers do with a field list: the fields, n_pad zero bits, one more at an ambiguous size
template <uint32_t N> static uint32_t packed(const dci::Field (&list)[N], const dci::Fields &f, uint32_t nrb, uint32_t n_pad, uint64_t *payload)
{
    uint32_t n = dci::pack(list, f, dci::riv_bits(nrb), payload) + n_pad;
    if (dci::ambiguous_size(n)) n++, n_pad++;
    *payload <<= n_pad;
    return n;
}

static void round_trips()
{
    for (uint32_t nrb = 6; nrb <= 110; nrb++)
        for (uint32_t n_prb = 1; n_prb <= nrb; n_prb++)
            for (uint32_t start = 0; start + n_prb <= nrb; start++) {
                dci::Fields f{};
                uint64_t    payload;
                f.riv = dci::riv_encode(nrb, n_prb, start); f.mcs = (n_prb + start) % 29; f.ndi = start & 1; f.tpc = n_prb & 3;
                { // format 0, C-RNTI
                    const uint32_t n = packed(dci::FORMAT_0, f, nrb, 1, &payload);
                    auto           o = fresh<mi_lte_dci_crnti>();
                    const int      rc = mi_lte_dci_0_1a_unpack_crnti(payload, n, 0x1234, nrb, 2, o.get());
                    CHECK(rc == 0 && o->format == 0 && o->flag == 0 && o->riv == f.riv && o->N_prb == n_prb && o->rb_start == start && o->mcs == f.mcs && o->ndi == f.ndi && o->tpc == f.tpc &&
                              o->cyclic_shift == 0 && o->cqi_request == 0 && o->alloc.N_prb == n_prb && o->alloc.prb[0][0] == start && o->alloc.prb[1][n_prb - 1] == start + n_prb - 1,
                          "format 0: N_rb %u N_prb %u start %u: rc %d, N_prb %u start %u", nrb, n_prb, start, rc, o->N_prb, o->rb_start);
                }
                f.format = 1; f.harq = start % 8; f.rv = n_prb % 4;
                { // format 1A, C-RNTI
                    const uint32_t n = packed(dci::FORMAT_1A, f, nrb, 0, &payload), i_tbs = f.mcs <= 9 ? f.mcs : f.mcs <= 16 ? f.mcs - 1 : f.mcs - 2;
                    auto           o = fresh<mi_lte_dci_crnti>();
                    const int      rc = mi_lte_dci_0_1a_unpack_crnti(payload, n, 0x1234, nrb, 1, o.get());
                    CHECK(rc == 0 && o->format == 1 && o->flag == 0 && o->riv == f.riv && o->N_prb == n_prb && o->rb_start == start && o->mcs == f.mcs && o->harq == f.harq && o->ndi == f.ndi &&
                              o->rv == f.rv && o->tpc == f.tpc && o->alloc.tbs == 8u * LTE_TBS_DIV8[i_tbs][n_prb - 1] && o->alloc.rv_idx == f.rv && o->alloc.prb[0][n_prb - 1] == start + n_prb - 1,
                          "format 1A: N_rb %u N_prb %u start %u: rc %d, N_prb %u start %u", nrb, n_prb, start, rc, o->N_prb, o->rb_start);
                }
                n_calls += 2;
                if (n_prb - 1 > nrb / 2) continue; // the common-RNTI unpacker reads the first branch of the RIV only, as the reference, and the generator sends no other
                { // format 1A for a common RNTI as the synthesiser sends it: N_PRB^1A = 3 in the TPC field, MCS <= 26
                    f.mcs = (n_prb + start) % 27; f.harq = 0; f.ndi = 0; f.tpc = 1;
                    const uint32_t n = packed(dci::FORMAT_1A, f, nrb, 0, &payload);
                    auto           o = fresh<mi_lte_pdcch_dci>();
                    o->alloc.N_prb = 0;
                    const int rc = mi_lte_dci_1a_unpack((uint32_t)payload, n, 0xFFFF, nrb, 2, o.get());
                    CHECK(n <= 32 && rc == 0 && o->alloc.N_prb == n_prb && o->alloc.prb[0][0] == start && o->alloc.prb[1][n_prb - 1] == start + n_prb - 1 && o->mcs == f.mcs &&
                              o->alloc.rv_idx == f.rv && o->alloc.tbs == LTE_TBS_NPRB_2_3[f.mcs][1] && o->alloc.rnti == 0xFFFF,
                          "format 1A, SI-RNTI: N_rb %u N_prb %u start %u: rc %d, N_prb %u", nrb, n_prb, start, rc, o->alloc.N_prb);
                    n_calls++;
                }
            }
}

static void search_space()
{
    const uint32_t rntis[6] = {0, 1, 0x3C, 0x100, 0xFFFF, 0x10000}, levels[5] = {1, 2, 3, 4, 8};
    for (uint32_t rnti : rntis)
        for (uint32_t sf = 0; sf <= 10; sf++)
            for (uint32_t n_cce = 0; n_cce <= 121; n_cce++)
                for (uint32_t L : levels) {
                    auto first = fresh<uint32_t>(6);
                    auto n = fresh<uint32_t>(1);
                    const bool valid = rnti >= 1 && rnti <= 0xFFFF && sf <= 9 && L != 3;
                    const int  rc = mi_lte_pdcch_search_space(rnti, sf, n_cce, L, first.data(), n.data());
                    n_calls++;
                    CHECK(rc == (valid ? MI_LTE_OK : MI_LTE_ERR_INVALID_ARG), "rnti %u sf %u N_cce %u L %u: %d", rnti, sf, n_cce, L, rc);
                    if (!valid) continue;
                    CHECK(n[0] == (n_cce < L ? 0u : L <= 2 ? 6u : 2u), "rnti %u sf %u N_cce %u L %u: %u candidates", rnti, sf, n_cce, L, n[0]);
                    for (uint32_t i = 0; i < n[0] && i < 6; i++)
                        CHECK(first[i] % L == 0 && first[i] + L <= n_cce, "rnti %u sf %u N_cce %u L %u: candidate %u at CCE %u", rnti, sf, n_cce, L, i, first[i]);
                }
}

static void geometry()
{
    const float    ngs[4] = {1.0f / 6, 0.5f, 1.0f, 2.0f};
    const uint32_t ports[3] = {1, 2, 4};
    std::vector<uint32_t> perm;
    std::vector<uint8_t>  seen;
    std::vector<uint32_t> cells; // every residue of 3 and of 2 N_rb at 1.4 MHz, a stride, the last seven
    for (uint32_t c = 0; c <= 503; c += (c < 12 || c >= 496) ? 1 : 22) cells.push_back(c);
    for (uint32_t nrb : BW)
        for (uint32_t cell : cells)
            for (float ng : ngs) {
                auto k = fresh<uint32_t>(4), n_reg = fresh<uint32_t>(1);
                auto nn = fresh<float>(4);
                auto pk = fresh<uint32_t>(75);
                CHECK(mi_lte_ctrl_reg_positions(nrb, cell, ng, k.data(), nn.data(), n_reg.data(), pk.data()) == MI_LTE_OK && n_reg[0] == 3 * (uint32_t)ceilf(ng * (nrb / 8.0f)), "N_rb %u cell %u N_g %g", nrb, cell, ng);
                for (uint32_t i = 0; i < n_reg[0] && i < 75; i++) CHECK(pk[i] % 6 == 0 && pk[i] < 12 * nrb, "N_rb %u cell %u N_g %g: PHICH REG %u at %u", nrb, cell, ng, i, pk[i]);
                n_calls++;
                for (uint32_t ns = 1; ns <= 4; ns++)
                    for (uint32_t ant : ports) {
                        auto pcf = fresh<uint32_t>(16);
                        auto cand = fresh<uint32_t>(6 * 288);
                        CHECK(mi_lte_pdcch_re_tables(nrb, ant, cell, ng, ns, pcf.data(), cand.data()) == MI_LTE_OK, "N_rb %u cell %u N_g %g N_symbs %u ports %u", nrb, cell, ng, ns, ant);
                        const uint32_t n_cce = pdcch_geom::cce_res(nrb, ant, cell, ng, ns, perm);
                        n_calls += 2;
                        seen.assign(4 * pdcch_geom::N_SC_MAX, 0);
                        bool ok = perm.size() >= 36 * (size_t)n_cce;
                        for (size_t i = 0; ok && i < 36 * (size_t)n_cce; i++) {
                            const uint32_t l = perm[i] / pdcch_geom::N_SC_MAX, sc = perm[i] % pdcch_geom::N_SC_MAX;
                            ok = l < ns && sc < 12 * nrb && !seen[perm[i]];
                            if (ok) seen[perm[i]] = 1;
                        }
                        CHECK(ok, "N_rb %u cell %u N_g %g N_symbs %u ports %u: a CCE element off the region or repeated", nrb, cell, ng, ns, ant);
                        for (uint32_t i = 0; i < 6 * 288; i++) CHECK(cand[i] == pdcch_geom::NO_RE || (cand[i] < 4 * (uint32_t)pdcch_geom::N_SC_MAX && seen[cand[i]]), "candidate element %u", i);
                    }
            }
    auto pcf = fresh<uint32_t>(16);
    auto cand = fresh<uint32_t>(6 * 288);
    auto k = fresh<uint32_t>(4), n_reg = fresh<uint32_t>(1);
    auto nn = fresh<float>(4);
    auto pk = fresh<uint32_t>(75);
    const struct { uint32_t nrb, cell; float ng; uint32_t ns, ant; bool positions_too; } refused[8] = {
        {7, 0, 1.0f, 2, 1, true}, {25, 0, 0.0f, 2, 1, true}, {25, 0, 2.5f, 2, 1, true}, {25, 0, NAN, 2, 1, true}, {25, 504, 1.0f, 2, 1, true},
        {25, 0, 1.0f, 0, 1, false}, {25, 0, 1.0f, 5, 1, false}, {25, 0, 1.0f, 2, 3, false}};
    for (const auto &r : refused) {
        CHECK(mi_lte_pdcch_re_tables(r.nrb, r.ant, r.cell, r.ng, r.ns, pcf.data(), cand.data()) == MI_LTE_ERR_INVALID_ARG, "re_tables refusal N_rb %u cell %u N_g %g N_symbs %u ports %u", r.nrb, r.cell, r.ng, r.ns, r.ant);
        if (r.positions_too) CHECK(mi_lte_ctrl_reg_positions(r.nrb, r.cell, r.ng, k.data(), nn.data(), n_reg.data(), pk.data()) == MI_LTE_ERR_INVALID_ARG, "positions refusal N_rb %u cell %u N_g %g", r.nrb, r.cell, r.ng);
        n_calls += 2;
    }
    for (uint32_t N_c = 24; N_c <= 80; N_c++)
        for (uint32_t E : {72u, 144u, 288u, 576u}) {
            auto map = fresh<uint16_t>(576);
            pdcch_geom::conv_rm_map(N_c, E, map.data());
            bool ok = true;
            for (uint32_t i = 0; i < E; i++) ok = ok && map[i] < 3 * N_c;
            CHECK(ok, "conv_rm_map N_c %u E %u", N_c, E);
            n_calls++;
        }
}

static void synthesiser()
{
    const uint32_t ports[3] = {1, 2, 4};
    for (uint32_t nrb : BW)
        for (uint32_t ant : ports)
            for (uint32_t cfi = 0; cfi <= 5; cfi++)
                for (double snr : {200.0, 10.0}) {
                    const mi_lte_dl_cfg        cfg = {2048, nrb, ant, 0};
                    const mi_lte_synth_channel ch = {0.6, 1.4, 0.0, snr, 0.0, 3 + cfi};
                    const uint32_t             sf = (3 + cfi) % 10, cell = (111 + nrb) % 504;
                    const bool                 valid = cfi >= 1 && cfi + (nrb <= 10 ? 1 : 0) <= 4;
                    std::vector<uint32_t>      perm;
                    const bool                 two_cces = valid && pdcch_geom::cce_res(nrb, ant, cell, 1.0f, cfi + (nrb <= 10 ? 1 : 0), perm) >= 2;
                    std::vector<float>         g((size_t)(2 + 2 * ant) * 16 * pdcch_geom::N_SC_MAX);
                    const mi_lte_synth_dci     dcis[4] = {{0xFFFF, 3, 2, 1, 0}, {0xFFFE, 5, 3, 0, 1}, {0, 0, 0, 0, 0}, {0x3C, 26, 1, nrb - 1, 2}};
                    CHECK(mi_lte_synth_ctrl_grids(&cfg, 1.0f, 1, &sf, &cell, &cfi, dcis, 4, &ch, g.data()) == (valid ? MI_LTE_OK : MI_LTE_ERR_INVALID_ARG), "ctrl_grids N_rb %u ports %u CFI %u", nrb, ant, cfi);
                    const mi_lte_synth_dci_rec small[2] = {{0x1234, 1, 0, 28, 0xABCDEF1}, {0xFFFF, 1, 1, 64, ~0ull - 2}};
                    CHECK(mi_lte_synth_ctrl_grids_dci(&cfg, 1.0f, 1, &sf, &cell, &cfi, small, 2, &ch, g.data()) == (two_cces ? MI_LTE_OK : MI_LTE_ERR_INVALID_ARG), "ctrl_grids_dci N_rb %u ports %u CFI %u", nrb, ant, cfi);
                    const mi_lte_synth_dci_rec all[5] = {{0x1234, 1, 0, 43, 0x5A5A5A5A5A5ull}, {0x77, 2, 2, 9, 0x155}, {0xFFF3, 4, 4, 28, 0x2345678}, {0xFFFF, 8, 8, 1, 1}, {9, 8, 120, 64, 5}};
                    for (uint32_t n = 1; n <= 5; n++) mi_lte_synth_ctrl_grids_dci(&cfg, 1.0f, 1, &sf, &cell, &cfi, all, n, &ch, g.data()); // (refused from the first record past N_cce)
                    n_calls += 7;
                }
}

int main()
{
    unpackers();
    round_trips();
    search_space();
    geometry();
    synthesiser();
    printf("pdcch host driver: %ld calls, %ld checks, %ld failures\n", n_calls, n_checks, n_fail);
    return n_fail ? 1 : 0;
}
