// Host-side synthesis of uplink test / benchmark captures: a minimal PUSCH transmitter written as the inverse
// of the reference's RECEIVER (liblte_phy_pusch_channel_decode, liblte/src/liblte_phy.cc:2801-2935), following
// 36.212 5.2.2 (UL-SCH coding) and 36.211 5.3-5.6 (scrambling, modulation, transform precoding, DMRS, SC-FDMA).
// The reference's own uplink transmit helpers cannot serve as the model: its channel interleaver walks the
// bit matrix per bit instead of per modulation symbol (liblte_phy.cc:12023-12042) and its SC-FDMA modulator
// multiplies where it should add an offset (:8565-8570) -- the eNodeB never transmits uplink, so neither is
// exercised.  Pure host C++; nothing here is part of the receive path.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mi_lte.h"
#include "lte_tables.h"
#include "prach_sets.hpp"
#include "synth.hpp"

extern "C" {

size_t mi_lte_synth_ul_unit_len(uint32_t fft_size)
{
    const size_t s = 2048 / (fft_size ? fft_size : 2048);
    return (30720 / s + 16 + 15) / 16 * 16; // one subframe plus slack for the channel delay
}

// UL-SCH transmit side of the PUSCH plans' 3GPP transport-block mode (36.212 5.2.2.1-5.2.2.5, N_L = 1): the inverse of what the plan decodes
int mi_lte_ulsch_encode_3gpp(uint32_t tbs, const uint8_t *bits, uint32_t G, uint32_t Q_m, uint32_t rv, uint8_t *e_out)
{
    const mi_lte_dlsch_cfg unlimited = {MI_LTE_ULSCH_N_SOFT, MI_LTE_ULSCH_M_HARQ}; // (mi_lte_ulsch_layout's: N_cb = K_w)
    return mi_lte_dlsch_encode_3gpp(tbs, bits, G, Q_m, 1, rv, &unlimited, e_out);
}

} // extern "C"

// One ACK / RI symbol (36.212 5.2.2.6, tables 5.2.2.6-1 .. -4): O = 1: [o0 y x ..]; O = 2: [w[2n mod 3] w[(2n + 1) mod 3] x ..], w = (o0, o1, o0 ^ o1).
// Placeholders as values: 2 = x, 3 = y
static void uci_symbol(uint32_t O, const uint8_t *bits, uint32_t n, uint32_t Qm, uint8_t *o)
{
    if (O == 1) { o[0] = bits[0] & 1u; o[1] = 3; }
    else {
        const uint8_t w[3] = {(uint8_t)(bits[0] & 1u), (uint8_t)(bits[1] & 1u), (uint8_t)((bits[0] ^ bits[1]) & 1u)};
        o[0] = w[(2 * n) % 3]; o[1] = w[(2 * n + 1) % 3];
    }
    for (uint32_t q = 2; q < Qm; q++) o[q] = 2;
}

// Data and control multiplexing and the channel interleaver (36.212 5.2.2.7-5.2.2.8) cell by cell from mi_lte_ulsch_uci_map: h[(c*M + r)*Q_m + q], the
// order the scrambler and the modulator take, holds cell (r, c)
static int ulsch_mux(uint32_t N_prb, uint32_t Qm, const mi_lte_ulsch_uci *uci, const uint8_t *f, const uint8_t *ack, const uint8_t *ri, const uint8_t *cqi, uint8_t *h)
{
    if (!uci || !f || !h || (uci->O_ack && !ack) || (uci->O_ri && !ri) || (uci->Q_cqi && !cqi)) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t M = 12 * N_prb;
    std::vector<uint8_t>  kind(12 * (size_t)(M ? M : 1));
    std::vector<uint32_t> index(24 * (size_t)(M ? M : 1));
    const int rc = mi_lte_ulsch_uci_map(N_prb, Qm, uci, kind.data(), index.data());
    if (rc != MI_LTE_OK) return rc;
    for (uint32_t r = 0; r < M; r++)
        for (uint32_t c = 0; c < 12; c++) {
            const uint32_t cell = r * 12 + c, n = index[2 * cell];
            uint8_t       *o = h + ((size_t)c * M + r) * Qm;
            switch (kind[cell]) {
            case MI_LTE_UCI_CELL_DATA: memcpy(o, f + (size_t)n * Qm, Qm); break;
            case MI_LTE_UCI_CELL_CQI:  memcpy(o, cqi + (size_t)n * Qm, Qm); break;
            case MI_LTE_UCI_CELL_RI:   uci_symbol(uci->O_ri, ri, n, Qm, o); break;
            default:                   uci_symbol(uci->O_ack, ack, n, Qm, o); break;
            }
        }
    return MI_LTE_OK;
}

// Scrambling with placeholders (36.211 5.3.1): x -> 1, y -> the scrambled bit before it, every other bit b ^ c(i)
static void scramble_ul(uint8_t *h, const uint8_t *c, size_t n)
{
    for (size_t i = 0; i < n; i++) h[i] = h[i] == 2 ? 1 : h[i] == 3 ? (i ? h[i - 1] : 1) : (uint8_t)((h[i] ^ c[i]) & 1u);
}

extern "C" int mi_lte_ulsch_mux_3gpp(uint32_t N_prb, uint32_t Q_m, const mi_lte_ulsch_uci *uci, const uint8_t *f, const uint8_t *h_ack,
                                     const uint8_t *h_ri, const uint8_t *h_cqi, uint32_t c_init, uint8_t *h_mux, uint8_t *h_scr)
{
    const int rc = ulsch_mux(N_prb, Q_m, uci, f, h_ack, h_ri, h_cqi, h_mux);
    if (rc != MI_LTE_OK || !h_scr) return rc;
    const size_t n = 12 * 12 * (size_t)N_prb * Q_m;
    std::vector<uint8_t> c(n);
    synth::gold(c_init, (uint32_t)n, c.data());
    memcpy(h_scr, h_mux, n);
    scramble_ul(h_scr, c.data(), n);
    return MI_LTE_OK;
}

// The uplink generator behind mi_lte_synth_ul_units_i8 (spec = false: one code block, the reference's wrapped interleaver -- what the
// reference-mode plans and the reference itself decode) and mi_lte_synth_ul_units_3gpp_i8 (mi_lte_ulsch_encode_3gpp); with h_uci
// (mi_lte_synth_ul_units_3gpp_uci_i8) the multiplexer above stands in front of the scrambler.  The control values are the caller's: the random
// numbers go to payload bits and channel draws in the same order whatever the descriptors are
struct UlUci { const mi_lte_ulsch_uci *uci; const uint8_t *ack, *ri, *cqi; uint32_t cqi_stride; };
static int synth_ul_units(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units, const uint32_t *h_subfr_num,
                          const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                          const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride, bool spec, const UlUci *uu = nullptr,
                          const uint8_t *h_payload = nullptr, const mi_lte_synth_paths *paths = nullptr)
{
    if (!cfg || !ul || !h_subfr_num || !h_n_id_cell || !h_allocs || !chan || !h_iq) return MI_LTE_ERR_INVALID_ARG;
    // multipath (mi_lte_synth_ul_units_3gpp_paths_i8): the amplitudes normalised to sum a^2 = 1, and sum a, which the int8 scale is divided by
    uint32_t n_paths = 1, p_dly[4] = {0, 0, 0, 0};
    double   p_amp[4] = {1.0, 0.0, 0.0, 0.0}, a_sum = 1.0;
    if (paths) {
        if (paths->n_paths < 1 || paths->n_paths > 4 || paths->delay[0] != 0) return MI_LTE_ERR_INVALID_ARG;
        double e = 0.0;
        for (uint32_t p = 0; p < paths->n_paths; p++) {
            if (!(paths->amp[p] >= 0.0) || !std::isfinite(paths->amp[p])) return MI_LTE_ERR_INVALID_ARG;
            e += paths->amp[p] * paths->amp[p];
        }
        if (!(e > 0.0) || !std::isfinite(e)) return MI_LTE_ERR_INVALID_ARG;
        n_paths = paths->n_paths;
        a_sum   = 0.0;
        for (uint32_t p = 0; p < n_paths; p++) { p_dly[p] = paths->delay[p]; p_amp[p] = n_paths == 1 ? 1.0 : paths->amp[p] / std::sqrt(e); a_sum += p_amp[p]; }
    }
    if (uu && (!spec || !uu->uci || !uu->ack || !uu->ri)) return MI_LTE_ERR_INVALID_ARG;
    if (!synth::valid_grid(cfg->fft_size, cfg->N_rb_dl)) return MI_LTE_ERR_INVALID_ARG;
    auto valid = [&](const mi_lte_pdsch_alloc &al) {
        if (!spec) return synth::valid_alloc(al, cfg->N_rb_dl);
        mi_lte_pdsch_alloc one = al;
        one.tbs = 16; // the grid conditions; the transport block's are the layout's
        mi_lte_dlsch_layout_t lay;
        return synth::valid_alloc(one, cfg->N_rb_dl) && al.mod_type != 0 && mi_lte_ulsch_layout(al.tbs, 0, 2, al.rv_idx, &lay) == MI_LTE_OK;
    };
    for (uint32_t u = 0; u < n_units; u++) {
        if (h_n_id_cell[u] > 503) return MI_LTE_ERR_INVALID_ARG;
        for (uint32_t a = 0; a < n_alloc; a++)
            if (!valid(h_allocs[(size_t)u * n_alloc + a]) || ((h_tx_bits || h_payload) && h_allocs[(size_t)u * n_alloc + a].tbs > tbs_stride))
                return MI_LTE_ERR_INVALID_ARG;
    }
    for (size_t k = 0; uu && k < (size_t)n_units * n_alloc; k++) { // the descriptors, and the transport block over the G they leave
        const mi_lte_pdsch_alloc &al = h_allocs[k];
        const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : 2;
        uint32_t       G  = 0;
        mi_lte_dlsch_layout_t lay;
        int rc = mi_lte_ulsch_uci_G(al.N_prb, Qm, &uu->uci[k], &G);
        if (rc == MI_LTE_OK) rc = mi_lte_ulsch_layout(al.tbs, G, Qm, al.rv_idx, &lay);
        if (rc != MI_LTE_OK) return rc;
        if (G / Qm < lay.C) return MI_LTE_ERR_INVALID_ARG; // a code block without a symbol
        if (uu->uci[k].Q_cqi && (!uu->cqi || uu->uci[k].Q_cqi > uu->cqi_stride)) return MI_LTE_ERR_INVALID_ARG;
    }
    const uint32_t N = cfg->fft_size, sc = 2048 / N, cp0 = 160 / sc, cpe = 144 / sc, N_rb = cfg->N_rb_dl, half = 6 * N_rb, N_sc = 12 * N_rb;
    const size_t unit_len = mi_lte_synth_ul_unit_len(N);
    synth::Rng   rng(chan->seed);
    std::vector<float>  g_re(14 * (size_t)N_sc), g_im(14 * (size_t)N_sc);
    std::vector<double> xr(N), xi(N), t_re(unit_len + 64), t_im(unit_len + 64);

    for (uint32_t u = 0; u < n_units; u++) {
        const uint32_t sf = h_subfr_num[u] % 10, cell = h_n_id_cell[u];
        std::fill(g_re.begin(), g_re.end(), 0.f);
        std::fill(g_im.begin(), g_im.end(), 0.f);
        for (uint32_t a = 0; a < n_alloc; a++) {
            const mi_lte_pdsch_alloc &al = h_allocs[(size_t)u * n_alloc + a];
            const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : al.mod_type == 1 ? 2 : 1;
            const size_t   k_al = (size_t)u * n_alloc + a;
            const uint32_t M = 12 * al.N_prb, N_bits = 12 * M * Qm, B = al.tbs + 24;
            uint32_t       G = N_bits; // the bits left to UL-SCH data (36.212 5.2.2.7)
            if (uu && mi_lte_ulsch_uci_G(al.N_prb, Qm, &uu->uci[k_al], &G) != MI_LTE_OK) return MI_LTE_ERR_INVALID_ARG;
            uint32_t       K = 0, f1, f2;
            for (int r = 0; r < LTE_QPP_N_SIZES; r++)
                if (LTE_QPP_ROWS[r].K >= B) { K = LTE_QPP_ROWS[r].K; break; }
            if (al.N_prb == 0 || al.N_prb > N_rb) return MI_LTE_ERR_UNSUPPORTED;
            if (!spec && (B > 6144 || K != B || !synth::qpp_params(K, &f1, &f2))) return MI_LTE_ERR_UNSUPPORTED;
            // UL-SCH: CRC24A, turbo code, rate matching with N_cb = K_w (36.212 5.2.2.1-5.2.2.5)
            std::vector<uint8_t> b(spec ? al.tbs : K), g(G), h(N_bits), c(N_bits);
            for (uint32_t i = 0; i < al.tbs; i++) b[i] = (uint8_t)(rng.next() & 1u);
            if (h_payload) // the caller's transport block; the draws above keep the rest of the stream where the generator has it
                for (uint32_t i = 0; i < al.tbs; i++) b[i] = h_payload[((size_t)u * n_alloc + a) * tbs_stride + i] & 1u;
            if (h_tx_bits) memcpy(h_tx_bits + ((size_t)u * n_alloc + a) * tbs_stride, b.data(), al.tbs);
            if (spec) { // segmentation and CRC24B as well, the exact interleaver
                const int rc = mi_lte_ulsch_encode_3gpp(al.tbs, b.data(), G, Qm, al.rv_idx, g.data());
                if (rc != MI_LTE_OK) return rc;
            } else {
                std::vector<uint8_t> d(3 * (K + 4));
                synth::crc24a(b.data(), al.tbs, b.data() + al.tbs);
                synth::turbo_encode(b.data(), K, true, d.data());
                synth::rate_match(d.data(), K + 4, 0xFFFFFFFFu, al.rv_idx, G, g.data());
            }
            // channel interleaver without control information (36.212 5.2.2.8): the R' x 12 matrix of Q_m-bit symbols is
            // written row by row and read column by column -> h[(s*M + k)*Q + q] = g[(k*12 + s)*Q + q]
            // with control information: ulsch_mux, which places the same cells around and under the control symbols
            if (uu) {
                const int rc = ulsch_mux(al.N_prb, Qm, &uu->uci[k_al], g.data(), uu->ack + 2 * k_al, uu->ri + 2 * k_al,
                                         uu->cqi ? uu->cqi + k_al * uu->cqi_stride : nullptr, h.data());
                if (rc != MI_LTE_OK) return rc;
            } else
                for (uint32_t s = 0; s < 12; s++)
                    for (uint32_t k = 0; k < M; k++)
                        for (uint32_t q = 0; q < Qm; q++) h[((size_t)s * M + k) * Qm + q] = g[((size_t)k * 12 + s) * Qm + q];
            synth::gold((al.rnti << 14) | (sf << 9) | cell, N_bits, c.data());
            scramble_ul(h.data(), c.data(), N_bits);
            std::vector<float> m_re(12 * (size_t)M), m_im(12 * (size_t)M);
            synth::modulate(h.data(), 12 * M, al.mod_type, m_re.data(), m_im.data());
            // transform precoding (36.211 5.3.3): forward DFT of each symbol's M points scaled by 1/sqrt(M), what a real
            // UE sends (data and DMRS at the same power).  The reference's receiver then recovers M times the
            // constellation point (unnormalised backward DFT times sqrt(M), liblte_phy.cc:6644-6657): QPSK decisions
            // survive (every soft bit saturates at +-1), the inner bits of 16/64QAM do not -- reproduced, not repaired.
            std::vector<float> d0r(M), d0i(M), d1r(M), d1i(M);
            int rc = mi_lte_ul_dmrs_pusch(ul, cell, sf, al.N_prb, d0r.data(), d0i.data(), d1r.data(), d1i.data());
            if (rc != MI_LTE_OK) return rc;
            const double scale = 1.0 / std::sqrt((double)M);
            std::vector<double> cs(M), sn(M);
            for (uint32_t t = 0; t < M; t++) { cs[t] = std::cos(-2.0 * M_PI * t / M); sn[t] = std::sin(-2.0 * M_PI * t / M); }
            for (uint32_t s = 0; s < 12; s++) {
                const uint32_t L = s < 3 ? s : s < 9 ? s + 1 : s + 2;
                for (uint32_t k = 0; k < M; k++) {
                    double ar = 0, ai = 0;
                    for (uint32_t n = 0; n < M; n++) {
                        const uint32_t t = (uint32_t)(((uint64_t)k * n) % M);
                        ar += m_re[s * M + n] * cs[t] - m_im[s * M + n] * sn[t];
                        ai += m_re[s * M + n] * sn[t] + m_im[s * M + n] * cs[t];
                    }
                    const uint32_t scx = al.prb[L / 7][k / 12] * 12 + k % 12;
                    g_re[L * N_sc + scx] = (float)(ar * scale);
                    g_im[L * N_sc + scx] = (float)(ai * scale);
                }
            }
            for (uint32_t k = 0; k < M; k++) { // DMRS on symbols 3 and 10 (36.211 5.5.2.1.2)
                const uint32_t s0 = al.prb[0][k / 12] * 12 + k % 12, s1 = al.prb[1][k / 12] * 12 + k % 12;
                g_re[3 * N_sc + s0]  = d0r[k]; g_im[3 * N_sc + s0]  = d0i[k];
                g_re[10 * N_sc + s1] = d1r[k]; g_im[10 * N_sc + s1] = d1i[k];
            }
        }
        // SC-FDMA modulation (36.211 5.6): grid column i sits on bin (N - half + i) mod N of an N-point inverse DFT whose
        // output is rotated by exp(+i*pi*n/N) (the half-sub-carrier shift the receiver undoes, liblte_phy.cc:8685-8690)
        std::fill(t_re.begin(), t_re.end(), 0.0);
        std::fill(t_im.begin(), t_im.end(), 0.0);
        size_t pos = 0;
        for (uint32_t s = 0; s < 14; s++) {
            const uint32_t cp = (s % 7 == 0) ? cp0 : cpe;
            std::fill(xr.begin(), xr.end(), 0.0);
            std::fill(xi.begin(), xi.end(), 0.0);
            for (uint32_t i = 0; i < N_sc; i++) {
                const uint32_t bin = (N - half + i) % N;
                xr[bin] = g_re[s * N_sc + i];
                xi[bin] = g_im[s * N_sc + i];
            }
            synth::idft(xr, xi);
            for (uint32_t n = 0; n < N; n++) {
                const double cr = std::cos(M_PI * n / N), ci = std::sin(M_PI * n / N), a = xr[n], b2 = xi[n];
                xr[n] = (a * cr - b2 * ci) / N;
                xi[n] = (a * ci + b2 * cr) / N;
            }
            // cyclic prefix: the rotated symbol continued backwards, x(n - N) = -x(n) because of the half-carrier shift
            for (uint32_t i = 0; i < cp && pos + i < unit_len; i++) { t_re[pos + i] = -xr[N - cp + i]; t_im[pos + i] = -xi[N - cp + i]; }
            for (uint32_t i = 0; i < N && pos + cp + i < unit_len; i++) { t_re[pos + cp + i] = xr[i]; t_im[pos + cp + i] = xi[i]; }
            pos += cp + N;
        }
        // flat channel, integer delay, AWGN, int8 quantisation
        const double   gain = chan->gain_min + (chan->gain_max - chan->gain_min) * rng.uniform();
        const double   ph   = 2.0 * M_PI * rng.uniform() - M_PI;
        const uint32_t dly  = (uint32_t)(rng.uniform() * (chan->max_delay + 0.999));
        double p_ph[4] = {ph, 0.0, 0.0, 0.0}; // one further phase per path behind the first, drawn behind the existing three
        for (uint32_t p = 1; p < n_paths; p++) p_ph[p] = 2.0 * M_PI * rng.uniform() - M_PI;
        double p_sig = 0, peak = 0;
        for (size_t i = 0; i < unit_len; i++) {
            p_sig += t_re[i] * t_re[i] + t_im[i] * t_im[i];
            peak = std::max(peak, std::max(std::fabs(t_re[i]), std::fabs(t_im[i])));
        }
        p_sig /= (double)unit_len;
        const double scale = (peak > 0 ? chan->peak / peak : 1.0);
        const double sigma = chan->snr_db >= 200 ? 0.0 : std::sqrt(p_sig / std::pow(10.0, chan->snr_db / 10.0) / 2.0);
        const double hr = gain * p_amp[0] * std::cos(ph), hi = gain * p_amp[0] * std::sin(ph); // (p_amp[0] = 1.0 for one path: the same doubles)
        int8_t *o = h_iq + (size_t)u * unit_len * 2;
        for (size_t i = 0; i < unit_len; i++) {
            double sr = 0, si = 0;
            if (i >= dly) { sr = t_re[i - dly]; si = t_im[i - dly]; }
            double cr = hr * sr - hi * si, ci = hr * si + hi * sr; // the first path: the flat channel's two terms
            for (uint32_t p = 1; p < n_paths; p++) {
                const size_t d = (size_t)dly + p_dly[p];
                if (i < d) continue;
                const double gr = gain * p_amp[p] * std::cos(p_ph[p]), gi = gain * p_amp[p] * std::sin(p_ph[p]);
                cr += gr * t_re[i - d] - gi * t_im[i - d];
                ci += gr * t_im[i - d] + gi * t_re[i - d];
            }
            const double yr = cr + sigma * rng.normal(), yi = ci + sigma * rng.normal();
            const long qr = std::lround(yr * scale / std::max(1.0, chan->gain_max) / a_sum), qi = std::lround(yi * scale / std::max(1.0, chan->gain_max) / a_sum);
            o[2 * i]     = (int8_t)std::max(-127L, std::min(127L, qr));
            o[2 * i + 1] = (int8_t)std::max(-127L, std::min(127L, qi));
        }
    }
    return MI_LTE_OK;
}

extern "C" {

int mi_lte_synth_ul_units_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units, const uint32_t *h_subfr_num,
                             const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                             const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride)
{
    return synth_ul_units(cfg, ul, n_units, h_subfr_num, h_n_id_cell, h_allocs, n_alloc, chan, h_iq, h_tx_bits, tbs_stride, false);
}

int mi_lte_synth_ul_units_3gpp_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units, const uint32_t *h_subfr_num,
                                  const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                  const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride)
{
    return synth_ul_units(cfg, ul, n_units, h_subfr_num, h_n_id_cell, h_allocs, n_alloc, chan, h_iq, h_tx_bits, tbs_stride, true);
}

int mi_lte_synth_ul_units_3gpp_uci_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units, const uint32_t *h_subfr_num,
                                      const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                      const mi_lte_synth_channel *chan, const mi_lte_ulsch_uci *h_uci, const uint8_t *h_ack, const uint8_t *h_ri,
                                      const uint8_t *h_cqi, uint32_t h_cqi_stride, int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride)
{
    const UlUci uu = {h_uci, h_ack, h_ri, h_cqi, h_cqi_stride};
    if (!h_uci) return MI_LTE_ERR_INVALID_ARG;
    return synth_ul_units(cfg, ul, n_units, h_subfr_num, h_n_id_cell, h_allocs, n_alloc, chan, h_iq, h_tx_bits, tbs_stride, true, &uu);
}

int mi_lte_synth_ul_units_3gpp_payload_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units, const uint32_t *h_subfr_num,
                                          const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                          const mi_lte_synth_channel *chan, const mi_lte_ulsch_uci *h_uci, const uint8_t *h_ack, const uint8_t *h_ri,
                                          const uint8_t *h_cqi, uint32_t h_cqi_stride, const uint8_t *h_payload, uint32_t tbs_stride, int8_t *h_iq)
{
    const UlUci uu = {h_uci, h_ack, h_ri, h_cqi, h_cqi_stride};
    if (!h_payload) return MI_LTE_ERR_INVALID_ARG;
    return synth_ul_units(cfg, ul, n_units, h_subfr_num, h_n_id_cell, h_allocs, n_alloc, chan, h_iq, nullptr, tbs_stride, true, h_uci ? &uu : nullptr, h_payload);
}

int mi_lte_synth_ul_units_3gpp_paths_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units, const uint32_t *h_subfr_num,
                                        const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                        const mi_lte_synth_channel *chan, const mi_lte_ulsch_uci *h_uci, const uint8_t *h_ack, const uint8_t *h_ri,
                                        const uint8_t *h_cqi, uint32_t h_cqi_stride, const uint8_t *h_payload, uint32_t tbs_stride,
                                        const mi_lte_synth_paths *paths, int8_t *h_iq)
{
    const UlUci uu = {h_uci, h_ack, h_ri, h_cqi, h_cqi_stride};
    if (!h_payload || !paths) return MI_LTE_ERR_INVALID_ARG;
    return synth_ul_units(cfg, ul, n_units, h_subfr_num, h_n_id_cell, h_allocs, n_alloc, chan, h_iq, nullptr, tbs_stride, true, h_uci ? &uu : nullptr, h_payload, paths);
}

// ---- PRACH (36.211 5.7.2-5.7.3): preamble v of root u is x_u((n + C_v) mod 839); its 839-point DFT sits on the PRACH
// sub-carriers (1.25 kHz spacing) phi + K(k0 + 1/2) + k in natural order; cyclic prefix + sequence (twice for formats 2, 3)
size_t mi_lte_synth_prach_len(uint32_t fft_size, uint32_t preamble_format)
{
    const PrachGeom pg = prach_geom(preamble_format > 4 ? 0 : preamble_format);
    const uint32_t  sc = 2048 / (fft_size ? fft_size : 2048);
    return ((pg.T_cp_30 + pg.T_fft_30 * pg.reps + 1024) / sc + 15) / 16 * 16;
}

// the physical roots u of the cell's 64 preambles in the order they are enumerated (prach_sets.hpp: prach_root_set; host arithmetic only)
int mi_lte_prach_root_set(const mi_lte_prach_cfg *pc, uint32_t *h_u /* [64] */, uint32_t *n_roots)
{
    if (!pc || !h_u || !n_roots) return MI_LTE_ERR_INVALID_ARG;
    const PrachRootSet rs = prach_root_set(pc->preamble_format, pc->root_seq_idx, pc->zczc, pc->hs_flag != 0);
    if (!rs.ok) return pc->preamble_format > 4 || pc->root_seq_idx >= prach_geom(pc->preamble_format > 4 ? 0 : pc->preamble_format).n_root_idx ? MI_LTE_ERR_INVALID_ARG : MI_LTE_ERR_UNSUPPORTED;
    for (uint32_t r = 0; r < rs.n_roots; r++) h_u[r] = rs.u[r];
    *n_roots = rs.n_roots;
    return MI_LTE_OK;
}

int mi_lte_synth_prach_i8(const mi_lte_dl_cfg *cfg, const mi_lte_prach_cfg *pc, uint32_t n_occ, const uint32_t *h_preamble_idx,
                          const uint32_t *h_delay, const mi_lte_synth_channel *chan, int8_t *h_iq)
{
    if (!cfg || !pc || !h_preamble_idx || !h_delay || !chan || !h_iq || pc->preamble_format > 4 || pc->root_seq_idx >= prach_geom(pc->preamble_format).n_root_idx)
        return MI_LTE_ERR_INVALID_ARG;
    // the six PRACH resource blocks lie on the grid (k_0 below is unsigned arithmetic), and a delay keeps the preamble inside the occasion
    if (!synth::valid_grid(cfg->fft_size, cfg->N_rb_dl) || pc->freq_offset + 6 > cfg->N_rb_dl) return MI_LTE_ERR_INVALID_ARG;
    for (uint32_t o = 0; o < n_occ; o++)
        if (h_delay[o] > 1024 / (2048 / cfg->fft_size)) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t  fmt = pc->preamble_format;
    const PrachGeom pg = prach_geom(fmt); // format 4: N_zc = 139 on 7.5 kHz sub-carriers, 4 096 samples, one repetition (36.211 table 5.7.1-1)
    const uint32_t N_ZC = pg.n_zc;
    const uint32_t N = cfg->fft_size, sc = 2048 / N, T = pg.T_fft_30 / sc, T_cp = pg.T_cp_30 / sc;
    const uint32_t reps = pg.reps;
    const size_t   len = mi_lte_synth_prach_len(N, fmt);
    const uint32_t k_0 = pc->freq_offset * 12 - cfg->N_rb_dl * 12 / 2 + N / 2, start = pg.phi + pg.K * k_0 + pg.K / 2;
    synth::Rng rng(chan->seed);
    std::vector<double> xr(N_ZC), xi(N_ZC), Xr(N_ZC), Xi(N_ZC), cz(N_ZC), sz(N_ZC), ct(T), st(T), sr(T), si(T), t_re(len), t_im(len);
    for (uint32_t t = 0; t < N_ZC; t++) { cz[t] = std::cos(-2.0 * M_PI * t / N_ZC); sz[t] = std::sin(-2.0 * M_PI * t / N_ZC); }
    for (uint32_t t = 0; t < T; t++) { ct[t] = std::cos(2.0 * M_PI * t / T); st[t] = std::sin(2.0 * M_PI * t / T); }
    for (uint32_t o = 0; o < n_occ; o++) {
        // which root and cyclic shift carry preamble index p (prach_preamble_seq_gen's enumeration, liblte_phy.cc:7155-7290)
        uint32_t p = h_preamble_idx[o] % 64, r = 0, u = 0, C_v = 0;
        for (;; r++) {
            if (r >= 64) return MI_LTE_ERR_INVALID_ARG;
            u = prach_root(fmt, (pc->root_seq_idx + r) % pg.n_root_idx); // the logical root order is cyclic (36.211 5.7.2; prach.hip)
            const PrachSets ps = prach_sets(u, pc->zczc, pc->hs_flag != 0, fmt);
            if (!ps.ok) return MI_LTE_ERR_UNSUPPORTED; // (the reference's own generator divides by zero / reads past its table there)
            if (p <= ps.v_max) {
                C_v = pc->hs_flag ? ps.d_start * (p / ps.N_RA_shift) + (p % ps.N_RA_shift) * ps.N_cs : p * ps.N_cs;
                break;
            }
            p -= ps.v_max + 1;
        }
        for (uint32_t n = 0; n < N_ZC; n++) {
            const uint32_t m = (n + C_v) % N_ZC;
            const double   ph = -M_PI * u * m * (m + 1) / N_ZC;
            xr[n] = std::cos(ph); xi[n] = std::sin(ph);
        }
        for (uint32_t k = 0; k < N_ZC; k++) {
            double ar = 0, ai = 0;
            uint32_t t = 0;
            for (uint32_t n = 0; n < N_ZC; n++) {
                ar += xr[n] * cz[t] - xi[n] * sz[t];
                ai += xr[n] * sz[t] + xi[n] * cz[t];
                t += k; if (t >= N_ZC) t -= N_ZC;
            }
            Xr[k] = ar; Xi[k] = ai;
        }
        for (uint32_t n = 0; n < T; n++) { // s(n) = sum_k X(k) exp(+2*pi*i*idx_k*n/T)
            double ar = 0, ai = 0;
            for (uint32_t k = 0; k < N_ZC; k++) {
                const uint32_t idx = (k + start + T / 2) % T, t = (uint32_t)(((uint64_t)idx * n) % T);
                ar += Xr[k] * ct[t] - Xi[k] * st[t];
                ai += Xr[k] * st[t] + Xi[k] * ct[t];
            }
            sr[n] = ar; si[n] = ai;
        }
        std::fill(t_re.begin(), t_re.end(), 0.0);
        std::fill(t_im.begin(), t_im.end(), 0.0);
        const uint32_t dly = h_delay[o];
        for (uint32_t i = 0; i < T_cp + reps * T; i++) {
            const uint32_t n = (i + T - (T_cp % T)) % T; // cyclic prefix = tail of the sequence
            if (dly + i < len) { t_re[dly + i] = sr[n]; t_im[dly + i] = si[n]; }
        }
        const double gain = chan->gain_min + (chan->gain_max - chan->gain_min) * rng.uniform(), ph = 2.0 * M_PI * rng.uniform() - M_PI;
        double p_sig = 0, peak = 0;
        for (size_t i = 0; i < len; i++) { p_sig += t_re[i] * t_re[i] + t_im[i] * t_im[i]; peak = std::max(peak, std::max(std::fabs(t_re[i]), std::fabs(t_im[i]))); }
        p_sig /= (double)len;
        const double scale = peak > 0 ? chan->peak / peak : 1.0;
        const double sigma = chan->snr_db >= 200 ? 0.0 : std::sqrt(p_sig / std::pow(10.0, chan->snr_db / 10.0) / 2.0);
        const double hr = gain * std::cos(ph), hi = gain * std::sin(ph);
        int8_t *ob = h_iq + (size_t)o * len * 2;
        for (size_t i = 0; i < len; i++) {
            const double yr = hr * t_re[i] - hi * t_im[i] + sigma * rng.normal(), yi = hr * t_im[i] + hi * t_re[i] + sigma * rng.normal();
            const long qr = std::lround(yr * scale / std::max(1.0, chan->gain_max)), qi = std::lround(yi * scale / std::max(1.0, chan->gain_max));
            ob[2 * i]     = (int8_t)std::max(-127L, std::min(127L, qr));
            ob[2 * i + 1] = (int8_t)std::max(-127L, std::min(127L, qi));
        }
    }
    return MI_LTE_OK;
}

} // extern "C"
