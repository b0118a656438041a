// tools/asan/rm_geom_driver.cc: the turbo rate-matching geometry the un-matching kernels gather by (openlte_amd/csrc/rm_geom.h) on the CPU,
// under g++ -fsanitize=address,undefined (tools/asan/run_rm_geom.sh), held to the transmitter's own walk of the circular buffer
// (tx::rate_match_turbo, tx.cc: written independently, and bit for bit the reference's by lifecycle_check tx).
// Where every e bit came from is read off the transmitter: d element 3 i + x carries its own number, one bit plane per run (15 planes: the
// number is below 3 * 6148 < 2^15).  Per case, with E = 2 Nnn + 37 (two whole laps and a partial one):
//   every d element with a rank is what e[rank], e[rank + Nnn], .. (< E) carry; every e index below E is claimed exactly once; an element
//   outside the soft buffer has no rank and claims none.
// (a) all 188 block sizes x the 12 reference-mode rank tables, through rm_combo / rm_combo_geom, termination rows included;
// (b) the 3GPP plans' rule through rm_soft_buffer on a grid of sizes, block counts, soft-buffer sizes, HARQ process counts, modes and rv.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mi_lte.h"
#include "../../openlte_amd/csrc/lte_tables.h"
#include "../../openlte_amd/csrc/rm_geom.h"
#include "../../openlte_amd/csrc/tx_host.h"

static long n_compared = 0, n_bad = 0, n_skipped = 0, n_limited = 0;
static void bad(const char *what, uint32_t D, uint32_t a, uint32_t b)
{
    if (n_bad++ < 20) printf("MISMATCH %s (D %u: %u, %u)\n", what, D, a, b);
}

// the d element (3 i + x) behind each of the first E bits the transmitter sends
static std::vector<uint32_t> transmitted(uint32_t D, uint32_t C, uint32_t tx_mode, uint32_t N_soft, uint32_t M_dl_harq, uint32_t chan, uint32_t rv, uint32_t E)
{
    std::vector<uint32_t> src(E, 0);
    std::vector<uint8_t>  d(3 * (size_t)D), e(E);
    for (uint32_t b = 0; b < 15; b++) {
        for (uint32_t x = 0; x < 3; x++)
            for (uint32_t i = 0; i < D; i++) d[(size_t)D * x + i] = (uint8_t)(((3 * i + x) >> b) & 1u); // (planar, as the transmitter takes it)
        e.assign(E, 0xEE); // (not a bit: an e the transmitter leaves unwritten shows as a wrong element)
        tx::rate_match_turbo(d.data(), 3 * D, C, tx_mode, N_soft, M_dl_harq, chan, rv, E, e.data());
        for (uint32_t k = 0; k < E; k++) src[k] |= (uint32_t)(e[k] == 1) << b | (e[k] > 1 ? 0x8000u : 0u);
    }
    return src;
}

// one geometry against the transmitter's walk with the same parameters
static void one_case(const RmGeom &g, uint32_t D, uint32_t C, uint32_t tx_mode, uint32_t N_soft, uint32_t M_dl_harq, uint32_t chan, uint32_t rv)
{
    if (g.N_cb < 2) { n_skipped++; return; } // (no such case below; the host refuses the buffer: mi_lte_dlsch_layout)
    if (g.N_cb < 3 * g.K_pi) n_limited++;
    const uint32_t              E   = 2 * g.Nnn + 37;
    const std::vector<uint32_t> src = transmitted(D, C, tx_mode, N_soft, M_dl_harq, chan, rv, E);
    std::vector<uint8_t>        claims(E, 0);
    for (uint32_t i = 0; i < D; i++)
        for (uint32_t x = 0; x < 3; x++) {
            const uint32_t r = g.rank(i, x);
            uint32_t       p, cn;
            g.pos_cnt(i, x, p, cn);
            if ((r == RM_NO_RANK) != (p >= g.N_cb)) bad("rank exists exactly inside the soft buffer", D, 3 * i + x, p);
            if (r != RM_NO_RANK && r >= g.Nnn) bad("first visit within the first lap", D, 3 * i + x, r);
            for (uint32_t k = r; k < E; k += g.Nnn) { // (the kernels' loop)
                n_compared++;
                claims[k]++;
                if (src[k] != 3 * i + x) bad("e index carries another element", D, k, src[k]);
            }
        }
    for (uint32_t k = 0; k < E; k++)
        if (claims[k] != 1) bad("e index claimed other than once", D, k, claims[k]);
}

int main()
{
    long n_sizes = 0, n_table = 0, n_grid = 0;
    // (a) the rank tables' meaning: combination -> geometry, and (ul, rv, tx_mode) -> combination
    for (int row = 0; row < LTE_QPP_N_SIZES; row++, n_sizes++) {
        const uint32_t D = LTE_QPP_ROWS[row].K + 4;
        for (uint32_t ul = 0; ul < 2; ul++)
            for (uint32_t rv = 0; rv < 4; rv++)
                for (uint32_t tx_mode = 1; tx_mode <= (ul ? 1u : 3u); tx_mode += 2, n_table++) {
                    const uint32_t combo = rm_combo(ul, rv, tx_mode);
                    if (combo >= RM_N_COMBOS) { bad("combination out of range", D, combo, RM_N_COMBOS); continue; }
                    if (ul) one_case(rm_combo_geom(combo, D), D, 1, tx_mode, 1, 1, MI_LTE_CHAN_ULSCH, rv);
                    else    one_case(rm_combo_geom(combo, D), D, 1, tx_mode, 250368, 8, MI_LTE_CHAN_DLSCH, rv);
                }
    }
    // every tx_mode lands on the K_mimo column of its table, and rv counts modulo 4 as the kernels mask it
    for (uint32_t tx_mode = 0; tx_mode < 16; tx_mode++) {
        const uint32_t two = tx_mode == 3 || tx_mode == 4 || tx_mode == 8 || tx_mode == 9;
        if (rm_k_mimo(tx_mode) != 1 + two) bad("K_mimo", 0, tx_mode, rm_k_mimo(tx_mode));
        for (uint32_t rv = 0; rv < 8; rv++) {
            if (rm_combo(0, rv, tx_mode) != 2 * (rv & 3) + two) bad("downlink combination", 0, tx_mode, rv);
            if (rm_combo(1, rv, tx_mode) != 8 + (rv & 3)) bad("uplink combination", 0, tx_mode, rv);
        }
    }
    // a soft buffer without room for one position holds nothing: no element has a rank (and nothing is divided by zero)
    {
        RmGeom g;
        g.init(44, 0, 2);
        for (uint32_t i = 0; i < 44; i++)
            for (uint32_t x = 0; x < 3; x++)
                if (g.rank(i, x) != RM_NO_RANK) bad("rank in an empty soft buffer", 44, i, x);
    }
    const long n_limited_a = n_limited, n_compared_a = n_compared;
    // (b) the 3GPP plans' soft-buffer rule
    const uint32_t Ks[] = {40, 48, 512, 1008, 2048, 3136, 6144}, Cs[] = {1, 2, 5, 13}, softs[] = {250368, 1237248, 3667200, 40000, 3000}, harqs[] = {1, 4, 8};
    uint32_t min_ncb = 0xFFFFFFFFu;
    for (uint32_t K : Ks)
        for (uint32_t C : Cs)
            for (uint32_t N_soft : softs)
                for (uint32_t M : harqs)
                    for (uint32_t tx_mode = 1; tx_mode <= 3; tx_mode += 2)
                        for (uint32_t rv = 0; rv < 4; rv++, n_grid++) {
                            const RmSoftBuf b = rm_soft_buffer(K + 4, C, tx_mode, N_soft, M, true, rv);
                            if (b.N_cb < min_ncb) min_ncb = b.N_cb;
                            if (b.N_cb < 2) { n_skipped++; continue; }
                            RmGeom g;
                            g.init(K + 4, b.N_cb, b.k0);
                            one_case(g, K + 4, C, tx_mode, N_soft, M, MI_LTE_CHAN_DLSCH, rv);
                        }
    printf("rm geom driver: %ld sizes, %ld table cases (%ld limited, %ld comparisons), %ld grid cases (%ld limited, %ld comparisons, smallest N_cb %u), "
           "%ld skipped, %ld differing\n",
           n_sizes, n_table, n_limited_a, n_compared_a, n_grid, n_limited - n_limited_a, n_compared - n_compared_a, min_ncb, n_skipped, n_bad);
    return n_bad || n_skipped ? 1 : 0;
}
