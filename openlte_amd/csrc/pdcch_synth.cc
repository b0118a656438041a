// Input synthesis (benchmark and tests): control regions as 36.211 / 36.212 transmit them -- PCFICH + DCIs through a smooth random channel
// per port + AWGN, directly as device-subframe grids with noisy channel estimates.  Transmit diversity follows 36.211 6.3.4.3 on all ports.
// The coding chain is the transmitter's (tx.cc: crc_bits, conv_encode_tb, rate_match_conv), the geometry pdcch_geom.h's, the format-1A
// fields dci.h's.  Host arithmetic in plain C++.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mi_lte.h"
#include "dci.h"
#include "pdcch_geom.h"
#include "synth.hpp"
#include "tx_host.h"

using namespace pdcch_geom;

namespace {

// one DCI of a synthetic control region: n_bits payload bits (first bit in bit n_bits - 1) for rnti on CCEs cce .. cce + L - 1
struct CtrlRec { uint32_t rnti, L, cce, n_bits; uint64_t payload; };

// The body both generators share.  records(u, N_cce, out) lists unit u's DCIs (every one inside the N_cce CCEs, none overlapping) or returns
// an error; per DCI: CRC16 masked with the RNTI (36.212 5.3.3.2), the tail-biting convolutional code (5.1.3.1), rate matching to 72 L bits
// (5.1.4.2), scrambling at bit 72 cce of the subframe's sequence, QPSK and transmit diversity onto the CCEs' resource elements.
template <typename Records>
int synth_ctrl_grids(const mi_lte_dl_cfg *cfg, float phich_res, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                     const uint32_t *h_cfi, const mi_lte_synth_channel *chan, float *h_grids, Records records)
{
    const uint32_t nrb = cfg->N_rb_dl, n_ant = cfg->N_ant;
    if (!(n_ant == 1 || n_ant == 2 || n_ant == 4)) return MI_LTE_ERR_INVALID_ARG;
    const size_t plane = 16 * (size_t)N_SC_MAX, nf = (2 + 2 * (size_t)n_ant) * plane;
    const double r2 = 1.0 / std::sqrt(2.0);
    synth::Rng   rng(chan->seed);
    std::vector<double> tr(n_ant * plane), ti(n_ant * plane);
    std::vector<uint32_t> cand(N_CAND * RE_MAX), perm;
    std::vector<CtrlRec>  recs;
    uint32_t pcf[16];
    for (uint32_t u = 0; u < n_units; u++) {
        const uint32_t sf = h_subfr_num[u], cell = h_n_id_cell[u], cfi = h_cfi[u], n_symbs = cfi + (nrb <= 10 ? 1 : 0);
        if (cfi < 1 || cfi > 4 || n_symbs > 4 || cell > 503 || sf > 9) return MI_LTE_ERR_INVALID_ARG;
        int rc = mi_lte_pdcch_re_tables(nrb, n_ant, cell, phich_res, n_symbs, pcf, cand.data());
        if (rc != MI_LTE_OK) return rc;
        const uint32_t N_cce = cce_res(nrb, n_ant, cell, phich_res, n_symbs, perm);
        std::fill(tr.begin(), tr.end(), 0.0);
        std::fill(ti.begin(), ti.end(), 0.0);
        // d[0..n): QPSK symbols of scrambled bits b -> transmit-diversity pre-coding onto the elements pos[]
        auto place = [&](const uint32_t *pos, const uint8_t *b, uint32_t n) {
            std::vector<double> dr(n), di(n);
            for (uint32_t i = 0; i < n; i++) { dr[i] = (1 - 2 * (int)b[2 * i]) * r2; di[i] = (1 - 2 * (int)b[2 * i + 1]) * r2; }
            auto put = [&](uint32_t port, uint32_t p, double re, double im) { tr[port * plane + p] = re; ti[port * plane + p] = im; };
            if (n_ant == 1) {
                for (uint32_t i = 0; i < n; i++) put(0, pos[i], dr[i], di[i]);
            } else {
                for (uint32_t i = 0; i + 1 < n; i += 2) { // pairs (x0, x1): port a sends x0, x1; port b sends -x1*, x0*
                    const uint32_t a = n_ant == 2 ? 0 : ((i & 2) ? 1 : 0), bb = n_ant == 2 ? 1 : ((i & 2) ? 3 : 2);
                    put(a, pos[i], r2 * dr[i], r2 * di[i]);
                    put(a, pos[i + 1], r2 * dr[i + 1], r2 * di[i + 1]);
                    put(bb, pos[i], -r2 * dr[i + 1], r2 * di[i + 1]);
                    put(bb, pos[i + 1], r2 * dr[i], -r2 * di[i]);
                }
            }
        };
        { // PCFICH (36.212 5.3.4, 36.211 6.7)
            uint8_t b[32], c[32];
            synth::gold((((sf + 1) * (2 * cell + 1)) << 9) + cell, 32, c);
            for (uint32_t i = 0; i < 32; i++) b[i] = (uint8_t)((cfi == 4 ? 0u : ((i % 3) == cfi - 1 ? 0u : 1u)) ^ c[i]);
            place(pcf, b, 16);
        }
        recs.clear();
        rc = records(u, N_cce, recs);
        if (rc != MI_LTE_OK) return rc;
        std::vector<uint8_t> c(72 * (size_t)N_cce + 1);
        synth::gold((sf << 9) + cell, 72 * N_cce, c.data());
        for (const CtrlRec &d : recs) {
            const uint32_t K = d.n_bits + 16, E = 72 * d.L;
            uint8_t        bits[64 + 16], dd[3 * (64 + 16)], e[576];
            for (uint32_t i = 0; i < d.n_bits; i++) bits[i] = (uint8_t)((d.payload >> (d.n_bits - 1 - i)) & 1u);
            tx::crc_bits(bits, d.n_bits, 0x11021, 16, bits + d.n_bits);
            for (uint32_t i = 0; i < 16; i++) bits[d.n_bits + i] ^= (d.rnti >> (15 - i)) & 1u;
            tx::conv_encode_tb(bits, K, dd);
            tx::rate_match_conv(dd, 3 * K, E, e);
            for (uint32_t k = 0; k < E; k++) e[k] ^= c[72 * (size_t)d.cce + k]; // scrambling at the first CCE's offset
            place(&perm[36 * (size_t)d.cce], e, E / 2);
        }
        // channel + noise -> rx grid and estimates (symbols 0..3 only: the control region)
        float *g = h_grids + (size_t)u * nf;
        std::fill(g, g + nf, 0.0f);
        const double sig = chan->snr_db >= 200 ? 0.0 : std::pow(10.0, -chan->snr_db / 20.0) * r2;
        std::vector<double> rr(4 * N_SC_MAX, 0.0), ri(4 * N_SC_MAX, 0.0);
        for (uint32_t p = 0; p < n_ant; p++) {
            const double amp = chan->gain_min + (chan->gain_max - chan->gain_min) * rng.uniform();
            const double tau = (2 * rng.uniform() - 1) * 2e-3, ph = (2 * rng.uniform() - 1) * M_PI;
            for (uint32_t l = 0; l < 4; l++)
                for (uint32_t k = 0; k < 12 * nrb; k++) {
                    const double hr = amp * std::cos(ph + 2 * M_PI * tau * k), hi = amp * std::sin(ph + 2 * M_PI * tau * k);
                    const size_t q = l * N_SC_MAX + k;
                    rr[q] += hr * tr[p * plane + q] - hi * ti[p * plane + q];
                    ri[q] += hr * ti[p * plane + q] + hi * tr[p * plane + q];
                    g[(2 + p) * plane + q]         = (float)(hr + 0.2 * sig * rng.normal());
                    g[(2 + n_ant + p) * plane + q] = (float)(hi + 0.2 * sig * rng.normal());
                }
        }
        for (uint32_t l = 0; l < 4; l++)
            for (uint32_t k = 0; k < 12 * nrb; k++) {
                const size_t q = l * N_SC_MAX + k;
                g[q]         = (float)(rr[q] + sig * rng.normal());
                g[plane + q] = (float)(ri[q] + sig * rng.normal());
            }
    }
    return MI_LTE_OK;
}

} // namespace

extern "C" {

int mi_lte_synth_ctrl_grids(const mi_lte_dl_cfg *cfg, float phich_res, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                            const uint32_t *h_cfi, const mi_lte_synth_dci *h_dci /*[n_units][n_dci]*/, uint32_t n_dci,
                            const mi_lte_synth_channel *chan, float *h_grids)
{
    if (!cfg || !h_subfr_num || !h_n_id_cell || !h_cfi || (n_dci && !h_dci) || n_dci > 4 || !chan || !h_grids) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t nrb = cfg->N_rb_dl;
    uint32_t sz[2];
    dci::sizes(nrb, &sz[0], &sz[1]);
    return synth_ctrl_grids(cfg, phich_res, n_units, h_subfr_num, h_n_id_cell, h_cfi, chan, h_grids, [&](uint32_t u, uint32_t N_cce, std::vector<CtrlRec> &out) {
        for (uint32_t a = 0; a < n_dci; a++) {
            const mi_lte_synth_dci &d = h_dci[(size_t)u * n_dci + a];
            if (d.rnti == 0) continue; // unused slot
            if (4 * a + 4 > N_cce) continue; // this candidate's CCEs do not all exist: nothing is sent (as the reference)
            // DCI format 1A for SI-/P-/RA-RNTI (36.212 5.3.3.1.3; the reference's dci_1a_pack :13138-13215): N_PRB^1A = 3 in the TPC field,
            // padded to the bandwidth's size
            if (d.N_prb == 0 || d.N_prb - 1 > nrb / 2 || d.rb_start + d.N_prb > nrb || d.mcs > 26) return (int)MI_LTE_ERR_INVALID_ARG;
            dci::Fields f{};
            f.format = 1; f.riv = dci::riv_encode(nrb, d.N_prb, d.rb_start); f.mcs = d.mcs; f.rv = d.rv_idx; f.tpc = 1;
            uint64_t       payload;
            const uint32_t n = dci::pack(dci::FORMAT_1A, f, dci::riv_bits(nrb), &payload);
            if (n > sz[0]) return (int)MI_LTE_ERR_INVALID_ARG;
            out.push_back(CtrlRec{d.rnti, 4, 4 * a, sz[0], payload << (sz[0] - n)});
        }
        return (int)MI_LTE_OK;
    });
}

// any DCI anywhere (include/mi_lte.h): up to MI_LTE_SYNTH_MAX_REC records per unit, rnti = 0 marks an unused slot
int mi_lte_synth_ctrl_grids_dci(const mi_lte_dl_cfg *cfg, float phich_res, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                const uint32_t *h_cfi, const mi_lte_synth_dci_rec *h_rec /*[n_units][n_rec]*/, uint32_t n_rec,
                                const mi_lte_synth_channel *chan, float *h_grids)
{
    if (!cfg || !h_subfr_num || !h_n_id_cell || !h_cfi || (n_rec && !h_rec) || n_rec > MI_LTE_SYNTH_MAX_REC || !chan || !h_grids) return MI_LTE_ERR_INVALID_ARG;
    return synth_ctrl_grids(cfg, phich_res, n_units, h_subfr_num, h_n_id_cell, h_cfi, chan, h_grids, [&](uint32_t u, uint32_t N_cce, std::vector<CtrlRec> &out) {
        uint8_t used[128] = {0}; // (N_cce <= 121: 100 RB, four symbols)
        for (uint32_t a = 0; a < n_rec; a++) {
            const mi_lte_synth_dci_rec &d = h_rec[(size_t)u * n_rec + a];
            if (d.rnti == 0) continue; // unused slot
            if (d.rnti > 0xFFFFu || !(d.L == 1 || d.L == 2 || d.L == 4 || d.L == 8) || d.cce % d.L || d.n_bits < 1 || d.n_bits > 64) return (int)MI_LTE_ERR_INVALID_ARG;
            if (d.cce >= N_cce || d.cce + d.L > N_cce || N_cce > 128) return (int)MI_LTE_ERR_INVALID_ARG; // reaches past the last CCE
            for (uint32_t i = 0; i < d.L; i++) {
                if (used[d.cce + i]) return (int)MI_LTE_ERR_INVALID_ARG; // overlaps an earlier record
                used[d.cce + i] = 1;
            }
            out.push_back(CtrlRec{d.rnti, d.L, d.cce, d.n_bits, d.n_bits == 64 ? d.payload : d.payload & ((1ull << d.n_bits) - 1ull)});
        }
        return (int)MI_LTE_OK;
    });
}

} // extern "C"
