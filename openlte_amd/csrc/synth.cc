// Host-side synthesis of benchmark / test inputs (the role LTE_fdd_dl_file_gen plays for the
// reference, LTE_fdd_dl_file_gen/src/LTE_fdd_dl_fg_samp_buf.cc:269-668): a minimal LTE downlink
// transmitter -- CRC24A, turbo encode, rate match, scramble, QAM map, CRS, OFDM modulate, a one-tap
// channel and int8 quantisation -- written to the 3GPP sections the reference's TX side follows
// (cited per function).  Pure host C++, no GPU work; it only produces the captures the receive
// kernels are fed with, so there is still no CPU path for anything the library *decodes*.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mi_lte.h"
#include "lte_tables.h"
#include "rm_geom.h"
#include "synth.hpp"

namespace synth {

// splitmix64: small, seedable, reproducible across platforms
uint64_t Rng::next()
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
double Rng::uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
double Rng::normal()
{
    double u1 = uniform(), u2 = uniform();
    if (u1 < 1e-300) u1 = 1e-300;
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
}

// 3GPP TS 36.212 5.1.1, gCRC24A (reference: calc_crc, liblte_phy.cc:9713-9743)
void crc24a(const uint8_t *bits, uint32_t n, uint8_t p[24])
{
    uint32_t rem = 0;
    for (uint32_t i = 0; i < n + 24; i++) {
        rem = (rem << 1) | (i < n ? bits[i] : 0u);
        if (rem & 0x1000000u) rem ^= 0x1864CFBu;
    }
    for (int i = 0; i < 24; i++) p[i] = (uint8_t)((rem >> (23 - i)) & 1u);
}

// 36.212 5.1.1, gCRC24B = D^24+D^23+D^6+D^5+D+1: the parity of a code block of a segmented transport block
static void crc24b(const uint8_t *bits, uint32_t n, uint8_t p[24])
{
    uint32_t rem = 0;
    for (uint32_t i = 0; i < n + 24; i++) {
        rem = (rem << 1) | (i < n ? bits[i] : 0u);
        if (rem & 0x1000000u) rem ^= 0x1800063u;
    }
    for (int i = 0; i < 24; i++) p[i] = (uint8_t)((rem >> (23 - i)) & 1u);
}

bool qpp_params(uint32_t K, uint32_t *f1, uint32_t *f2)
{
    for (int r = 0; r < LTE_QPP_N_SIZES; r++)
        if (LTE_QPP_ROWS[r].K == K) { *f1 = LTE_QPP_ROWS[r].f1; *f2 = LTE_QPP_ROWS[r].f2; return true; }
    return false;
}

// QPP interleaver, 36.212 5.1.3.2.3.  ref_wrap reproduces the reference's uint32 evaluation
// (liblte_phy.cc:10954-10958) so that captures made here loop back through the REF decoder the way
// captures made by the reference's own generator do.
void qpp_map(uint32_t K, bool ref_wrap, std::vector<uint16_t> &pi)
{
    uint32_t f1 = 0, f2 = 0;
    qpp_params(K, &f1, &f2);
    pi.resize(K);
    for (uint32_t i = 0; i < K; i++)
        pi[i] = ref_wrap ? (uint16_t)((f1 * i + f2 * i * i) % K) : (uint16_t)(((uint64_t)f1 * i + (uint64_t)f2 * i * i) % K);
}

// 36.212 5.1.3.2.1 constituent encoder g0 = 1+D^2+D^3 (feedback), g1 = 1+D+D^3, with the 3+1 step
// termination of 5.1.3.2.2 (reference: turbo_constituent_encoder, liblte_phy.cc:10855-10924)
static void rsc(const uint8_t *in, uint32_t K, uint8_t *z, uint8_t *x_tail)
{
    int s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t i = 0; i < K + 4; i++) {
        int fb = s2 ^ s3;
        int s0 = (i < K) ? (fb ^ in[i]) : 0;
        z[i]      = (uint8_t)(s0 ^ s1 ^ s3);
        x_tail[i] = (uint8_t)fb;
        s3 = s2; s2 = s1; s1 = s0;
    }
}

// 36.212 5.1.3.2: d planar d0[D] d1[D] d2[D], D = K+4 (reference: turbo_encode, liblte_phy.cc:10541-10589)
void turbo_encode(const uint8_t *c, uint32_t K, bool ref_wrap, uint8_t *d)
{
    const uint32_t        D = K + 4;
    std::vector<uint16_t> pi;
    std::vector<uint8_t>  z(D), x(D), zp(D), xp(D), cp(K);
    qpp_map(K, ref_wrap, pi);
    rsc(c, K, z.data(), x.data());
    for (uint32_t i = 0; i < K; i++) cp[i] = c[pi[i]];
    rsc(cp.data(), K, zp.data(), xp.data());
    uint8_t *d0 = d, *d1 = d + D, *d2 = d + 2 * D;
    for (uint32_t i = 0; i < K; i++) { d0[i] = c[i]; d1[i] = z[i]; d2[i] = zp[i]; }
    d0[K] = x[K];      d1[K] = z[K];       d2[K] = x[K + 1];
    d0[K + 1] = z[K + 1]; d1[K + 1] = x[K + 2]; d2[K + 1] = z[K + 2];
    d0[K + 2] = xp[K];    d1[K + 2] = zp[K];    d2[K + 2] = xp[K + 1];
    d0[K + 3] = zp[K + 1]; d1[K + 3] = xp[K + 2]; d2[K + 3] = zp[K + 2];
}


// Gold sequence, 36.211 7.2 (reference: generate_prs_c, liblte_phy.cc:9669-9704)
void gold(uint32_t c_init, uint32_t len, uint8_t *c)
{
    uint32_t x1 = 1, x2 = c_init;
    for (uint32_t n = 0; n < 1600; n++) { // Nc = 1600: advance both registers past the discarded prefix
        uint32_t n1 = ((x1 >> 3) ^ x1) & 1u, n2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1u;
        x1 = (x1 >> 1) | (n1 << 30);
        x2 = (x2 >> 1) | (n2 << 30);
    }
    for (uint32_t n = 0; n < len; n++) {
        c[n]        = (uint8_t)((x1 ^ x2) & 1u);
        uint32_t n1 = ((x1 >> 3) ^ x1) & 1u, n2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 1u;
        x1 = (x1 >> 1) | (n1 << 30);
        x2 = (x2 >> 1) | (n2 << 30);
    }
}

// sub-block interleaver + circular buffer read-out, 36.212 5.1.4.1 (reference:
// liblte_phy_rate_match_turbo, liblte_phy.cc:11081-11237).  d planar, F = 0 only.
void rate_match(const uint8_t *d, uint32_t D, uint32_t N_cb_limit, uint32_t rv, uint32_t E, uint8_t *e)
{
    uint32_t R = (D + 31) / 32, K_pi = 32 * R, N_d = K_pi - D, K_w = 3 * K_pi;
    std::vector<int16_t> w(K_w);
    auto y = [&](int x, uint32_t n) -> int16_t { return n < N_d ? (int16_t)-1 : (int16_t)d[x * D + (n - N_d)]; };
    for (uint32_t c = 0; c < 32; c++)
        for (uint32_t r = 0; r < R; r++) {
            uint32_t i = c * R + r, n = 32 * r + LTE_SUBBLOCK_COL_PERM[c];
            w[i]                = y(0, n);
            w[K_pi + 2 * i]     = y(1, n);
            w[K_pi + 2 * i + 1] = y(2, (LTE_SUBBLOCK_COL_PERM[c] + 32 * r + 1) % K_pi);
        }
    uint32_t N_cb = N_cb_limit < K_w ? N_cb_limit : K_w;
    uint32_t k0   = R * (2 * ((N_cb + 8 * R - 1) / (8 * R)) * rv + 2);
    for (uint32_t k = 0, j = 0; k < E; j++) {
        int16_t v = w[(k0 + j) % N_cb];
        if (v >= 0) e[k++] = (uint8_t)v;
    }
}

// 36.211 7.1.2-7.1.4 (reference: modulation_mapper, liblte_phy.cc:8704-9490)
void modulate(const uint8_t *b, uint32_t n_sym, uint32_t mod, float *re, float *im)
{
    const float r2 = (float)(1 / std::sqrt(2.0)), r10 = (float)(1 / std::sqrt(10.0)), r42 = (float)(1 / std::sqrt(42.0));
    for (uint32_t i = 0; i < n_sym; i++) {
        if (mod == 1) {
            re[i] = r2 * (1 - 2 * b[2 * i]);
            im[i] = r2 * (1 - 2 * b[2 * i + 1]);
        } else if (mod == 2) {
            const uint8_t *q = b + 4 * i;
            re[i] = r10 * (float)((1 - 2 * q[0]) * (2 - (1 - 2 * q[2])));
            im[i] = r10 * (float)((1 - 2 * q[1]) * (2 - (1 - 2 * q[3])));
        } else if (mod == 3) {
            const uint8_t *q = b + 6 * i;
            re[i] = r42 * (float)((1 - 2 * q[0]) * (4 - (1 - 2 * q[2]) * (2 - (1 - 2 * q[4]))));
            im[i] = r42 * (float)((1 - 2 * q[1]) * (4 - (1 - 2 * q[3]) * (2 - (1 - 2 * q[5]))));
        } else {
            re[i] = im[i] = r2 * (1 - 2 * b[i]);
        }
    }
}

// PBCH / PSS / SSS sub-carrier window and the PDSCH RE exclusion rule (36.211 6.3.5; reference:
// liblte_phy.cc:3722-3789 on RX, :3501-3540 and :3621-3657 on TX)
void sync_window(uint32_t N_rb_dl, uint32_t *first_sc, uint32_t *last_sc)
{
    switch (N_rb_dl) {
    case 6:  *first_sc = 0;           *last_sc = 71;          break;
    case 15: *first_sc = 4 * 12 + 6;  *last_sc = 11 * 12 - 7; break;
    case 25: *first_sc = 9 * 12 + 6;  *last_sc = 16 * 12 - 7; break;
    case 50: *first_sc = 22 * 12;     *last_sc = 28 * 12 - 1; break;
    case 75: *first_sc = 34 * 12 + 6; *last_sc = 41 * 12 - 7; break;
    default: *first_sc = 47 * 12;     *last_sc = 53 * 12 - 1; break;
    }
}
bool pdsch_re_excluded(uint32_t N_ant, uint32_t cell, uint32_t sf, uint32_t L, uint32_t j, uint32_t sc, uint32_t first_sc,
                       uint32_t last_sc)
{
    if (N_ant == 1 && (L % 7) == 0 && (cell % 6) == (j % 6)) return true;
    if (N_ant == 1 && (L % 7) == 4 && ((cell + 3) % 6) == (j % 6)) return true;
    if (N_ant >= 2 && ((L % 7) == 0 || (L % 7) == 4) && (cell % 3) == (j % 3)) return true;
    if (N_ant == 4 && (L % 7) == 1 && (cell % 3) == (j % 3)) return true;
    const bool in_win = sc >= first_sc && sc <= last_sc;
    if (sf == 0 && in_win && L >= 7 && L <= 10) return true;
    if ((sf == 0 || sf == 5) && in_win && (L == 5 || L == 6)) return true;
    return false;
}

// unnormalised inverse DFT (the reference's FFTW_BACKWARD plan, liblte_phy.cc:2311-2315), radix-2
void idft(std::vector<double> &xr, std::vector<double> &xi)
{
    const size_t n = xr.size();
    for (size_t i = 1, j = 0; i < n; i++) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(xr[i], xr[j]); std::swap(xi[i], xi[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = 2.0 * M_PI / (double)len;
        for (size_t j = 0; j < len / 2; j++) {
            const double wr = std::cos(ang * (double)j), wi = std::sin(ang * (double)j);
            for (size_t b = 0; b < n; b += len) {
                const size_t p = b + j, q = p + len / 2;
                const double tr = xr[q] * wr - xi[q] * wi, ti = xr[q] * wi + xi[q] * wr;
                xr[q] = xr[p] - tr; xi[q] = xi[p] - ti;
                xr[p] += tr;        xi[p] += ti;
            }
        }
    }
}

} // namespace synth

extern "C" {

// 36.212 5.1.2 (segmentation with F = 0 and C- = 0: C blocks of one size K, K C = B') and 5.1.4.1.2 (soft buffer, code-block concatenation)
// for the 3GPP transport-block mode: what the transmitter below, the 3GPP plans (chain.hip, dlsch3gpp.hip) and the tests lay a block out by
// (N_L = 1: mi_lte_dlsch_layout; N_L = 2: the transmit-diversity plans, whose symbols leave in pairs)
int mi_lte_dlsch_layout_nl(uint32_t tbs, uint32_t G, uint32_t Q_m, uint32_t N_L, uint32_t tx_mode, uint32_t rv, const mi_lte_dlsch_cfg *dlsch,
                           mi_lte_dlsch_layout_t *out)
{
    if (!dlsch || !out || !(Q_m == 1 || Q_m == 2 || Q_m == 4 || Q_m == 6) || !(N_L == 1 || N_L == 2) || G % (N_L * Q_m) || rv > 3 || dlsch->M_dl_harq == 0)
        return MI_LTE_ERR_INVALID_ARG;
    if (tbs == 0 || tbs > 75376) return MI_LTE_ERR_UNSUPPORTED; // the largest single-layer size of 36.213 Table 7.1.7.2.1-1 (13 blocks)
    const uint32_t B = tbs + 24, C = B <= 6144 ? 1u : (B + 6119) / 6120, Bp = C == 1 ? B : B + 24 * C;
    uint32_t K = 0;
    for (int r = 0; r < LTE_QPP_N_SIZES && !K; r++)
        if (C * LTE_QPP_ROWS[r].K >= Bp) K = LTE_QPP_ROWS[r].K;
    if (C * K != Bp) return MI_LTE_ERR_UNSUPPORTED; // filler bits, or blocks of two sizes
    memset(out, 0, sizeof(*out));
    out->C = C; out->K = K; out->B = B;
    const RmSoftBuf sb = rm_soft_buffer(K + 4, C, tx_mode, dlsch->N_soft, dlsch->M_dl_harq, true, rv);
    out->N_cb = sb.N_cb;
    out->k0   = sb.k0;
    if (out->N_cb < 2) return MI_LTE_ERR_INVALID_ARG; // (position 1 of the buffer is the first that is never NULL)
    const uint32_t Gp = G / (N_L * Q_m), gam = Gp % C, lo = Gp / C;
    for (uint32_t r = 0, off = 0; r < C; r++) {
        out->E[r]   = N_L * Q_m * (r + gam < C ? lo : lo + 1); // r <= C - gamma - 1: floor(G' / C), else ceil
        out->off[r] = off;
        off += out->E[r];
    }
    return MI_LTE_OK;
}

int mi_lte_dlsch_layout(uint32_t tbs, uint32_t G, uint32_t Q_m, uint32_t tx_mode, uint32_t rv, const mi_lte_dlsch_cfg *dlsch, mi_lte_dlsch_layout_t *out)
{
    return mi_lte_dlsch_layout_nl(tbs, G, Q_m, 1, tx_mode, rv, dlsch, out);
}

// The HARQ pool's buffer (include/mi_lte.h): the largest C * 3 (K + 4) int16 positions over the sizes of 36.213 Table 7.1.7.2.1-1 up to max_tbs
size_t mi_lte_harq_buffer_bytes(uint32_t max_tbs)
{
    const mi_lte_dlsch_cfg any{1u << 30, 8};
    size_t best = 0;
    for (uint32_t i = 0; i < 27; i++)
        for (uint32_t n = 0; n < 110; n++) {
            const uint32_t tbs = 8u * LTE_TBS_DIV8[i][n];
            mi_lte_dlsch_layout_t lay;
            if (tbs == 0 || tbs > max_tbs || mi_lte_dlsch_layout(tbs, 0, 2, 1, 0, &any, &lay) != MI_LTE_OK) continue;
            best = std::max(best, (size_t)lay.C * 3 * (lay.K + 4));
        }
    return 2 * best;
}

// 36.212 5.1.1-5.1.4.1 for one transport block in the 3GPP mode (include/mi_lte.h): CRC24A, C blocks of K bits (each with CRC24B when
// C > 1), turbo encoding with the exact interleaver, rate matching with the layout's N_cb and E_r, concatenation
int mi_lte_dlsch_encode_3gpp_nl(uint32_t tbs, const uint8_t *bits, uint32_t G, uint32_t Q_m, uint32_t N_L, uint32_t tx_mode, uint32_t rv,
                                const mi_lte_dlsch_cfg *dlsch, uint8_t *e_out)
{
    if (!bits || !e_out) return MI_LTE_ERR_INVALID_ARG;
    mi_lte_dlsch_layout_t lay;
    const int rc = mi_lte_dlsch_layout_nl(tbs, G, Q_m, N_L, tx_mode, rv, dlsch, &lay);
    if (rc != MI_LTE_OK) return rc;
    const uint32_t K = lay.K, C = lay.C, nb = C == 1 ? K : K - 24;
    std::vector<uint8_t> b(lay.B), c(K), d(3 * (K + 4));
    for (uint32_t i = 0; i < tbs; i++) b[i] = bits[i] & 1u;
    synth::crc24a(b.data(), tbs, b.data() + tbs);
    for (uint32_t r = 0; r < C; r++) {
        memcpy(c.data(), b.data() + (size_t)r * nb, nb);
        if (C > 1) synth::crc24b(c.data(), nb, c.data() + nb);
        synth::turbo_encode(c.data(), K, false, d.data());
        synth::rate_match(d.data(), K + 4, lay.N_cb, rv, lay.E[r], e_out + lay.off[r]);
    }
    return MI_LTE_OK;
}

int mi_lte_dlsch_encode_3gpp(uint32_t tbs, const uint8_t *bits, uint32_t G, uint32_t Q_m, uint32_t tx_mode, uint32_t rv, const mi_lte_dlsch_cfg *dlsch,
                             uint8_t *e_out)
{
    return mi_lte_dlsch_encode_3gpp_nl(tbs, bits, G, Q_m, 1, tx_mode, rv, dlsch, e_out);
}

// 36.211 6.3.3.3 (layer mapping: x_l(i) = d(N_ant i + l)) and 6.3.4.3 (pre-coding for transmit diversity), in one step: output place n of
// port p at y[p * M_symb + n].  Two ports: the pair (d(2i), d(2i+1)) leaves as (x0, x1) on port 0 and (-x1*, x0*) on port 1, all over sqrt 2.
// Four ports: places 4i, 4i+1 carry the pair (d(4i), d(4i+1)) on ports (0, 2), places 4i+2, 4i+3 the pair (d(4i+2), d(4i+3)) on ports (1, 3);
// the other two ports rest.
int mi_lte_txdiv_precode(uint32_t N_ant, const float *d_re, const float *d_im, uint32_t M_symb, float *y_re, float *y_im)
{
    if (!(N_ant == 2 || N_ant == 4) || !d_re || !d_im || !y_re || !y_im || M_symb % N_ant) return MI_LTE_ERR_INVALID_ARG;
    const float a = (float)(1 / std::sqrt(2.0));
    std::fill(y_re, y_re + (size_t)N_ant * M_symb, 0.f);
    std::fill(y_im, y_im + (size_t)N_ant * M_symb, 0.f);
    for (uint32_t n = 0; n < M_symb; n += 2) {
        const uint32_t pa = N_ant == 2 ? 0u : (n >> 1) & 1u, pb = N_ant == 2 ? 1u : pa + 2;
        float *ar = y_re + (size_t)pa * M_symb, *ai = y_im + (size_t)pa * M_symb, *br = y_re + (size_t)pb * M_symb, *bi = y_im + (size_t)pb * M_symb;
        ar[n]     = a * d_re[n];      ai[n]     = a * d_im[n];      // x0
        br[n]     = -a * d_re[n + 1]; bi[n]     = a * d_im[n + 1];  // -x1*
        ar[n + 1] = a * d_re[n + 1];  ai[n + 1] = a * d_im[n + 1];  // x1
        br[n + 1] = a * d_re[n];      bi[n + 1] = -a * d_im[n];     // x0*
    }
    return MI_LTE_OK;
}

size_t mi_lte_synth_unit_len(uint32_t fft_size)
{
    const size_t s = 2048 / (fft_size ? fft_size : 2048);
    return ((30720 + 4400) / s + 15) / 16 * 16;
}

} // extern "C"

// The downlink generator behind mi_lte_synth_dl_units_i8 (dlsch == nullptr: the reference transmitter's single-block DL-SCH, E rounded
// down to a multiple of 2 Q_m) and mi_lte_synth_dl_units_3gpp_i8 (mi_lte_dlsch_encode_3gpp, E = G)
static int synth_dl_units(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell, uint32_t N_pdcch_symbs,
                          const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, const mi_lte_dlsch_cfg *dlsch, const mi_lte_synth_channel *chan,
                          int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride, const uint8_t *h_payload = nullptr)
{
    if (!cfg || !h_subfr_num || !h_n_id_cell || !chan || !h_iq || cfg->N_ant != 1 || (n_alloc && !h_allocs)) return MI_LTE_ERR_INVALID_ARG;
    if (!synth::valid_grid(cfg->fft_size, cfg->N_rb_dl) || N_pdcch_symbs < 1 || N_pdcch_symbs > 4) return MI_LTE_ERR_INVALID_ARG;
    auto valid = [&](const mi_lte_pdsch_alloc &al) {
        if (!dlsch) return synth::valid_alloc(al, cfg->N_rb_dl);
        mi_lte_pdsch_alloc one = al;
        one.tbs = 16; // the grid conditions; the transport block's are the layout's
        mi_lte_dlsch_layout_t lay;
        return synth::valid_alloc(one, cfg->N_rb_dl) && al.mod_type != 0 && mi_lte_dlsch_layout(al.tbs, 0, 2, al.tx_mode, al.rv_idx, dlsch, &lay) == MI_LTE_OK;
    };
    for (uint32_t u = 0; u < n_units; u++) {
        if (h_n_id_cell[u] > 503) return MI_LTE_ERR_INVALID_ARG;
        for (uint32_t a = 0; a < n_alloc; a++)
            if (!valid(h_allocs[(size_t)u * n_alloc + a]) || ((h_tx_bits || h_payload) && h_allocs[(size_t)u * n_alloc + a].tbs > tbs_stride))
                return MI_LTE_ERR_INVALID_ARG;
    }
    const uint32_t N = cfg->fft_size, sc = 2048 / N, cp0 = 160 / sc, cpe = 144 / sc, N_rb = cfg->N_rb_dl, half = 6 * N_rb, N_sc = 12 * N_rb;
    const size_t   unit_len = mi_lte_synth_unit_len(N);
    uint32_t       first_sc, last_sc;
    synth::sync_window(N_rb, &first_sc, &last_sc);
    synth::Rng rng(chan->seed);
    std::vector<float>  g_re(16 * N_sc), g_im(16 * N_sc);
    std::vector<double> xr(N), xi(N), t_re(unit_len + 64), t_im(unit_len + 64);
    const float         r2 = (float)(1 / std::sqrt(2.0));
    double              scale_all = 1.0;

    for (uint32_t u = 0; u < n_units; u++) {
        const uint32_t sf = h_subfr_num[u] % 10, cell = h_n_id_cell[u];
        std::fill(g_re.begin(), g_re.end(), 0.f);
        std::fill(g_im.begin(), g_im.end(), 0.f);
        // CRS for port 0 on symbols 0,4,7,11 of this subframe and symbol 0 of the next (36.211 6.10.1;
        // reference: liblte_phy_map_crs, liblte_phy.cc:5144-5262)
        for (uint32_t s = 0; s < 16; s++) {
            const uint32_t l = s % 7;
            if (!(l == 0 || l == 4)) continue;
            const uint32_t ns = (2 * sf + s / 7) % 20, v = (l == 0) ? 0 : 3;
            uint8_t        c[440];
            synth::gold(1024 * (7 * (ns + 1) + l + 1) * (2 * cell + 1) + 2 * cell + 1, 440, c);
            for (uint32_t j = 0; j < 2 * N_rb; j++) {
                const uint32_t k = 6 * j + (v + cell % 6) % 6, mp = j + 110 - N_rb;
                g_re[s * N_sc + k] = r2 * (1 - 2 * (float)c[2 * mp]);
                g_im[s * N_sc + k] = r2 * (1 - 2 * (float)c[2 * mp + 1]);
            }
        }
        // PDSCH allocations
        for (uint32_t a = 0; a < n_alloc; a++) {
            const mi_lte_pdsch_alloc &al = h_allocs[(size_t)u * n_alloc + a];
            const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : al.mod_type == 1 ? 2 : 1;
            // RE list in mapping order
            std::vector<uint32_t> res;
            for (uint32_t L = N_pdcch_symbs; L < 14; L++)
                for (uint32_t pi = 0; pi < al.N_prb; pi++)
                    for (uint32_t j = 0; j < 12; j++) {
                        const uint32_t scx = al.prb[L / 7][pi] * 12 + j;
                        if (!synth::pdsch_re_excluded(1, cell, sf, L, j, scx, first_sc, last_sc)) res.push_back(L * N_sc + scx);
                    }
            if (dlsch) { // 3GPP mode: every resource element carries a soft bit
                const uint32_t G = (uint32_t)res.size() * Qm;
                std::vector<uint8_t> b(al.tbs), e(G), c(G);
                for (uint32_t i = 0; i < al.tbs; i++) b[i] = (uint8_t)(rng.next() & 1u);
                if (h_payload) // the caller's transport block; the draws above keep the rest of the stream where the generator has it
                    for (uint32_t i = 0; i < al.tbs; i++) b[i] = h_payload[((size_t)u * n_alloc + a) * tbs_stride + i] & 1u;
                if (h_tx_bits) memcpy(h_tx_bits + ((size_t)u * n_alloc + a) * tbs_stride, b.data(), al.tbs);
                const int rc = mi_lte_dlsch_encode_3gpp(al.tbs, b.data(), G, Qm, al.tx_mode, al.rv_idx, dlsch, e.data());
                if (rc != MI_LTE_OK) return rc;
                synth::gold((al.rnti << 14) | (sf << 9) | cell, G, c.data());
                for (uint32_t i = 0; i < G; i++) e[i] ^= c[i];
                std::vector<float> m_re(res.size()), m_im(res.size());
                synth::modulate(e.data(), (uint32_t)res.size(), al.mod_type, m_re.data(), m_im.data());
                for (size_t i = 0; i < res.size(); i++) { g_re[res[i]] = m_re[i]; g_im[res[i]] = m_im[i]; }
                continue;
            }
            const uint32_t G = (uint32_t)res.size() * Qm, E = G / (2 * Qm) * (2 * Qm); // dlsch_channel_encode with N_l = 2 (:3572-3584)
            const uint32_t B = al.tbs + 24;
            uint32_t       K = 0, f1, f2;
            for (int r = 0; r < LTE_QPP_N_SIZES; r++)
                if (LTE_QPP_ROWS[r].K >= B) { K = LTE_QPP_ROWS[r].K; break; }
            if (B > 6144 || K != B || !synth::qpp_params(K, &f1, &f2)) return MI_LTE_ERR_UNSUPPORTED; // single block, F = 0 only
            std::vector<uint8_t> b(K), d(3 * (K + 4)), e(E), c(E);
            for (uint32_t i = 0; i < al.tbs; i++) b[i] = (uint8_t)(rng.next() & 1u);
            synth::crc24a(b.data(), al.tbs, b.data() + al.tbs);
            if (h_tx_bits) memcpy(h_tx_bits + ((size_t)u * n_alloc + a) * tbs_stride, b.data(), al.tbs);
            synth::turbo_encode(b.data(), K, true, d.data());
            synth::rate_match(d.data(), K + 4, 250368 / (rm_k_mimo(al.tx_mode) * 8), al.rv_idx, E, e.data());
            synth::gold((al.rnti << 14) | (sf << 9) | cell, E, c.data());
            for (uint32_t i = 0; i < E; i++) e[i] ^= c[i];
            const uint32_t     M = E / Qm;
            std::vector<float> m_re(M), m_im(M);
            synth::modulate(e.data(), M, al.mod_type, m_re.data(), m_im.data());
            for (uint32_t i = 0; i < M; i++) { g_re[res[i]] = m_re[i]; g_im[res[i]] = m_im[i]; }
        }
        // OFDM modulation of 14 + 2 symbols (36.211 6.12; reference: symbols_to_samples_dl, liblte_phy.cc:8484-8530)
        std::fill(t_re.begin(), t_re.end(), 0.0);
        std::fill(t_im.begin(), t_im.end(), 0.0);
        size_t pos = 0;
        for (uint32_t s = 0; s < 16; s++) {
            const uint32_t cp = (s % 7 == 0) ? cp0 : cpe;
            std::fill(xr.begin(), xr.end(), 0.0);
            std::fill(xi.begin(), xi.end(), 0.0);
            for (uint32_t i = 0; i < half; i++) {
                xr[i + 1]     = g_re[s * N_sc + half + i];     xi[i + 1]     = g_im[s * N_sc + half + i];
                xr[N - 1 - i] = g_re[s * N_sc + half - 1 - i]; xi[N - 1 - i] = g_im[s * N_sc + half - 1 - i];
            }
            synth::idft(xr, xi);
            for (uint32_t i = 0; i < cp && pos + i < unit_len; i++) { t_re[pos + i] = xr[N - cp + i]; t_im[pos + i] = xi[N - cp + i]; }
            for (uint32_t i = 0; i < N && pos + cp + i < unit_len; i++) { t_re[pos + cp + i] = xr[i]; t_im[pos + cp + i] = xi[i]; }
            pos += cp + N;
            if (pos >= unit_len) break;
        }
        // one-tap channel, integer delay, AWGN, int8 quantisation
        // max_delay < 0: a static channel -- no random phase, no delay, one int8 scale for every unit -- so that consecutive units can be
        // laid end to end as ONE capture (a unit's look-ahead symbols are then what the next unit starts with)
        const bool   fixed = chan->max_delay < 0;
        const double gain = chan->gain_min + (chan->gain_max - chan->gain_min) * rng.uniform();
        const double ph   = fixed ? 0.0 * rng.uniform() : 2.0 * M_PI * rng.uniform() - M_PI;
        const uint32_t dly = fixed ? (uint32_t)(0.0 * rng.uniform()) : (uint32_t)(rng.uniform() * (chan->max_delay + 0.999));
        double p_sig = 0, peak = 0;
        for (size_t i = 0; i < unit_len; i++) {
            p_sig += t_re[i] * t_re[i] + t_im[i] * t_im[i];
            peak = std::max(peak, std::max(std::fabs(t_re[i]), std::fabs(t_im[i])));
        }
        p_sig /= (double)unit_len;
        if (!fixed) scale_all = (peak > 0 ? chan->peak / peak : 1.0);
        else if (u == 0) {
            // static: ONE scale whatever the units carry (and whichever call made them): the RMS of a fully loaded symbol of unit-power
            // resource elements lands at peak / 3.6 -- OFDM's crest factor stays inside int8
            std::fill(xr.begin(), xr.end(), 0.0);
            std::fill(xi.begin(), xi.end(), 0.0);
            for (uint32_t i = 0; i < half; i++) { xr[i + 1] = (i & 1) ? 1.0 : -1.0; xr[N - 1 - i] = (i % 3) ? 1.0 : -1.0; }
            synth::idft(xr, xi);
            double pr = 0;
            for (uint32_t i = 0; i < N; i++) pr += xr[i] * xr[i] + xi[i] * xi[i];
            scale_all = chan->peak / (3.6 * std::sqrt(pr / N));
        }
        const double scale = scale_all;
        const double sigma = chan->snr_db >= 200 ? 0.0 : std::sqrt(p_sig / std::pow(10.0, chan->snr_db / 10.0) / 2.0);
        const double hr = gain * std::cos(ph), hi = gain * std::sin(ph);
        int8_t *o = h_iq + (size_t)u * unit_len * 2;
        for (size_t i = 0; i < unit_len; i++) {
            double sr = 0, si = 0;
            if (i >= dly) { sr = t_re[i - dly]; si = t_im[i - dly]; }
            double yr = hr * sr - hi * si + sigma * rng.normal(), yi = hr * si + hi * sr + sigma * rng.normal();
            long qr = std::lround(yr * scale / std::max(1.0, chan->gain_max)), qi = std::lround(yi * scale / std::max(1.0, chan->gain_max));
            o[2 * i]     = (int8_t)std::max(-127L, std::min(127L, qr));
            o[2 * i + 1] = (int8_t)std::max(-127L, std::min(127L, qi));
        }
    }
    return MI_LTE_OK;
}

extern "C" {

int mi_lte_synth_dl_units_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num,
                             const uint32_t *h_n_id_cell, uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs,
                             uint32_t n_alloc, const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits,
                             uint32_t tbs_stride)
{
    return synth_dl_units(cfg, n_units, h_subfr_num, h_n_id_cell, N_pdcch_symbs, h_allocs, n_alloc, nullptr, chan, h_iq, h_tx_bits, tbs_stride);
}

int mi_lte_synth_dl_units_3gpp_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                  uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, const mi_lte_dlsch_cfg *dlsch,
                                  const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride)
{
    if (!dlsch) return MI_LTE_ERR_INVALID_ARG;
    return synth_dl_units(cfg, n_units, h_subfr_num, h_n_id_cell, N_pdcch_symbs, h_allocs, n_alloc, dlsch, chan, h_iq, h_tx_bits, tbs_stride);
}

int mi_lte_synth_dl_units_3gpp_payload_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                          uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                          const mi_lte_dlsch_cfg *dlsch, const mi_lte_synth_channel *chan, const uint8_t *h_payload,
                                          uint32_t tbs_stride, int8_t *h_iq)
{
    if (!dlsch || (n_alloc && n_units && !h_payload)) return MI_LTE_ERR_INVALID_ARG;
    return synth_dl_units(cfg, n_units, h_subfr_num, h_n_id_cell, N_pdcch_symbs, h_allocs, n_alloc, dlsch, chan, h_iq, nullptr, tbs_stride, h_payload);
}

// The transmit-diversity generator (include/mi_lte.h): a cell of 2 or 4 CRS ports, every allocation sent as 36.211 6.3.3.3 / 6.3.4.3 specify
// (tx_mode 2) over the N_L = 2 code-block concatenation.  One grid and one OFDM signal per port; the ports share the unit's delay (co-located
// antennas) and have a gain and a phase each; the receiver sees their sum.  A function of its own: the single-port generators above keep their
// byte streams.
int mi_lte_synth_dl_units_3gpp_txdiv_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                        uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, const mi_lte_dlsch_cfg *dlsch,
                                        const mi_lte_synth_channel *chan, const uint8_t *h_payload, uint32_t tbs_stride, int8_t *h_iq,
                                        uint8_t *h_tx_bits)
{
    if (!cfg || !h_subfr_num || !h_n_id_cell || !chan || !h_iq || !dlsch || (n_alloc && !h_allocs)) return MI_LTE_ERR_INVALID_ARG;
    if (!(cfg->N_ant == 2 || cfg->N_ant == 4)) return MI_LTE_ERR_INVALID_ARG; // (one port: mi_lte_synth_dl_units_3gpp_i8)
    if (!synth::valid_grid(cfg->fft_size, cfg->N_rb_dl) || N_pdcch_symbs < 1 || N_pdcch_symbs > 4) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t P = cfg->N_ant;
    for (uint32_t u = 0; u < n_units; u++) {
        if (h_n_id_cell[u] > 503) return MI_LTE_ERR_INVALID_ARG;
        for (uint32_t a = 0; a < n_alloc; a++) {
            const mi_lte_pdsch_alloc &al = h_allocs[(size_t)u * n_alloc + a];
            mi_lte_pdsch_alloc one = al;
            one.tbs = 16; // the grid conditions; the transport block's are the layout's
            mi_lte_dlsch_layout_t lay;
            if (!synth::valid_alloc(one, cfg->N_rb_dl) || al.mod_type == 0 || al.tx_mode != 2 || al.n_pdcch_symbs > 4 ||
                mi_lte_dlsch_layout_nl(al.tbs, 0, 2, 2, al.tx_mode, al.rv_idx, dlsch, &lay) != MI_LTE_OK || ((h_tx_bits || h_payload) && al.tbs > tbs_stride))
                return MI_LTE_ERR_INVALID_ARG;
        }
    }
    const uint32_t N = cfg->fft_size, sc = 2048 / N, cp0 = 160 / sc, cpe = 144 / sc, N_rb = cfg->N_rb_dl, half = 6 * N_rb, N_sc = 12 * N_rb;
    const size_t   unit_len = mi_lte_synth_unit_len(N);
    uint32_t       first_sc, last_sc;
    synth::sync_window(N_rb, &first_sc, &last_sc);
    synth::Rng rng(chan->seed);
    std::vector<float>  g_re((size_t)P * 16 * N_sc), g_im((size_t)P * 16 * N_sc);
    std::vector<double> xr(N), xi(N), t_re(P * unit_len), t_im(P * unit_len), s_re(unit_len), s_im(unit_len);
    const float         r2 = (float)(1 / std::sqrt(2.0));

    for (uint32_t u = 0; u < n_units; u++) {
        const uint32_t sf = h_subfr_num[u] % 10, cell = h_n_id_cell[u];
        std::fill(g_re.begin(), g_re.end(), 0.f);
        std::fill(g_im.begin(), g_im.end(), 0.f);
        // CRS of every port over this subframe and the first two symbols of the next (36.211 6.10.1): ports 0 / 1 in symbols 0 and 4 of a slot
        // with offsets 0 / 3 and 3 / 0, ports 2 / 3 in symbol 1 with offsets 3 (n_s mod 2) and 3 + 3 (n_s mod 2); where one port has a
        // reference signal the others send nothing
        for (uint32_t p = 0; p < P; p++)
            for (uint32_t s = 0; s < 16; s++) {
                const uint32_t l = s % 7, ns = (2 * sf + s / 7) % 20;
                if (p < 2 ? !(l == 0 || l == 4) : l != 1) continue;
                const uint32_t v = p == 0 ? (l == 0 ? 0 : 3) : p == 1 ? (l == 0 ? 3 : 0) : p == 2 ? 3 * (ns % 2) : 3 + 3 * (ns % 2);
                uint8_t        c[440];
                synth::gold(1024 * (7 * (ns + 1) + l + 1) * (2 * cell + 1) + 2 * cell + 1, 440, c);
                for (uint32_t j = 0; j < 2 * N_rb; j++) {
                    const uint32_t k = 6 * j + (v + cell % 6) % 6, mp = j + 110 - N_rb;
                    g_re[((size_t)p * 16 + s) * N_sc + k] = r2 * (1 - 2 * (float)c[2 * mp]);
                    g_im[((size_t)p * 16 + s) * N_sc + k] = r2 * (1 - 2 * (float)c[2 * mp + 1]);
                }
            }
        for (uint32_t a = 0; a < n_alloc; a++) {
            const mi_lte_pdsch_alloc &al = h_allocs[(size_t)u * n_alloc + a];
            const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : 2, cfi = al.n_pdcch_symbs ? al.n_pdcch_symbs : N_pdcch_symbs;
            std::vector<uint32_t> res; // the allocation's resource elements in mapping order: symbol -> PRB -> sub-carrier
            for (uint32_t L = cfi; L < 14; L++)
                for (uint32_t pi = 0; pi < al.N_prb; pi++)
                    for (uint32_t j = 0; j < 12; j++) {
                        const uint32_t scx = al.prb[L / 7][pi] * 12 + j;
                        if (!synth::pdsch_re_excluded(P, cell, sf, L, j, scx, first_sc, last_sc)) res.push_back(L * N_sc + scx);
                    }
            const uint32_t M = (uint32_t)res.size(), G = M * Qm;
            if (M % P) return MI_LTE_ERR_UNSUPPORTED; // (no allocation on the grid has such a count: tests/test_fuzz_cpu.py)
            std::vector<uint8_t> b(al.tbs), e(G), c(G);
            for (uint32_t i = 0; i < al.tbs; i++) b[i] = (uint8_t)(rng.next() & 1u);
            if (h_payload) // the caller's transport block; the draws above keep the rest of the stream where it is without one
                for (uint32_t i = 0; i < al.tbs; i++) b[i] = h_payload[((size_t)u * n_alloc + a) * tbs_stride + i] & 1u;
            if (h_tx_bits) memcpy(h_tx_bits + ((size_t)u * n_alloc + a) * tbs_stride, b.data(), al.tbs);
            const int rc = mi_lte_dlsch_encode_3gpp_nl(al.tbs, b.data(), G, Qm, 2, al.tx_mode, al.rv_idx, dlsch, e.data());
            if (rc != MI_LTE_OK) return rc;
            synth::gold((al.rnti << 14) | (sf << 9) | cell, G, c.data());
            for (uint32_t i = 0; i < G; i++) e[i] ^= c[i];
            std::vector<float> m_re(M), m_im(M), y_re((size_t)P * M), y_im((size_t)P * M);
            synth::modulate(e.data(), M, al.mod_type, m_re.data(), m_im.data());
            if (M && mi_lte_txdiv_precode(P, m_re.data(), m_im.data(), M, y_re.data(), y_im.data()) != MI_LTE_OK) return MI_LTE_ERR_INVALID_ARG;
            for (uint32_t p = 0; p < P; p++)
                for (uint32_t i = 0; i < M; i++) {
                    g_re[(size_t)p * 16 * N_sc + res[i]] = y_re[(size_t)p * M + i];
                    g_im[(size_t)p * 16 * N_sc + res[i]] = y_im[(size_t)p * M + i];
                }
        }
        // OFDM modulation of every port's 14 + 2 symbols (36.211 6.12)
        std::fill(t_re.begin(), t_re.end(), 0.0);
        std::fill(t_im.begin(), t_im.end(), 0.0);
        for (uint32_t p = 0; p < P; p++) {
            double *tr = t_re.data() + p * unit_len, *ti = t_im.data() + p * unit_len;
            const float *gr = g_re.data() + (size_t)p * 16 * N_sc, *gi = g_im.data() + (size_t)p * 16 * N_sc;
            size_t pos = 0;
            for (uint32_t s = 0; s < 16 && pos < unit_len; s++) {
                const uint32_t cp = (s % 7 == 0) ? cp0 : cpe;
                std::fill(xr.begin(), xr.end(), 0.0);
                std::fill(xi.begin(), xi.end(), 0.0);
                for (uint32_t i = 0; i < half; i++) {
                    xr[i + 1]     = gr[s * N_sc + half + i];     xi[i + 1]     = gi[s * N_sc + half + i];
                    xr[N - 1 - i] = gr[s * N_sc + half - 1 - i]; xi[N - 1 - i] = gi[s * N_sc + half - 1 - i];
                }
                synth::idft(xr, xi);
                for (uint32_t i = 0; i < cp && pos + i < unit_len; i++) { tr[pos + i] = xr[N - cp + i]; ti[pos + i] = xi[N - cp + i]; }
                for (uint32_t i = 0; i < N && pos + cp + i < unit_len; i++) { tr[pos + cp + i] = xr[i]; ti[pos + cp + i] = xi[i]; }
                pos += cp + N;
            }
        }
        // the channel: one integer delay for the unit, then a gain and a phase per port, in port order; the ports summed; AWGN relative to the
        // sum's power; one int8 scale per unit from the sum's peak.  max_delay < 0: no delay and no phase
        const bool     fixed = chan->max_delay < 0;
        const double   ud    = rng.uniform();
        const uint32_t dly   = fixed ? 0u : (uint32_t)(ud * (chan->max_delay + 0.999));
        std::fill(s_re.begin(), s_re.end(), 0.0);
        std::fill(s_im.begin(), s_im.end(), 0.0);
        for (uint32_t p = 0; p < P; p++) {
            const double gain = chan->gain_min + (chan->gain_max - chan->gain_min) * rng.uniform();
            const double up = rng.uniform(), ph = fixed ? 0.0 : 2.0 * M_PI * up - M_PI;
            const double hr = gain * std::cos(ph), hi = gain * std::sin(ph);
            const double *tr = t_re.data() + p * unit_len, *ti = t_im.data() + p * unit_len;
            for (size_t i = dly; i < unit_len; i++) {
                s_re[i] += hr * tr[i - dly] - hi * ti[i - dly];
                s_im[i] += hr * ti[i - dly] + hi * tr[i - dly];
            }
        }
        double p_sig = 0, peak = 0;
        for (size_t i = 0; i < unit_len; i++) {
            p_sig += s_re[i] * s_re[i] + s_im[i] * s_im[i];
            peak = std::max(peak, std::max(std::fabs(s_re[i]), std::fabs(s_im[i])));
        }
        p_sig /= (double)unit_len;
        const double scale = peak > 0 ? chan->peak / peak : 1.0;
        const double sigma = chan->snr_db >= 200 ? 0.0 : std::sqrt(p_sig / std::pow(10.0, chan->snr_db / 10.0) / 2.0);
        int8_t *o = h_iq + (size_t)u * unit_len * 2;
        for (size_t i = 0; i < unit_len; i++) {
            const double yr = s_re[i] + sigma * rng.normal(), yi = s_im[i] + sigma * rng.normal();
            const long   qr = std::lround(yr * scale), qi = std::lround(yi * scale);
            o[2 * i]     = (int8_t)std::max(-127L, std::min(127L, qr));
            o[2 * i + 1] = (int8_t)std::max(-127L, std::min(127L, qi));
        }
    }
    return MI_LTE_OK;
}


// n code blocks of size K: random information bits -> turbo encode -> soft values in the reference's
// interleaved layout d[i*3+x], value +amp for bit 0 / -amp for bit 1, each sign flipped with
// probability flip ("64QAM-like" hard +-127 soft bits, SURVEY 8d W3 distribution (i)).
int mi_lte_synth_turbo_soft_i8(uint32_t K, uint32_t n, double flip, int amp, uint64_t seed, int ref_wrap,
                               int8_t *h_soft /* n*3*(K+4) */, uint8_t *h_tx_bits /* n*K, may be NULL */)
{
    uint32_t f1, f2;
    if (!h_soft || !synth::qpp_params(K, &f1, &f2) || amp < 1 || amp > 127) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t       D = K + 4;
    synth::Rng           rng(seed);
    std::vector<uint8_t> c(K), d(3 * D);
    for (uint32_t b = 0; b < n; b++) {
        for (uint32_t i = 0; i < K; i++) c[i] = (uint8_t)(rng.next() & 1u);
        synth::turbo_encode(c.data(), K, ref_wrap != 0, d.data());
        int8_t *o = h_soft + (size_t)b * 3 * D;
        for (uint32_t i = 0; i < D; i++)
            for (int x = 0; x < 3; x++) {
                int v = d[x * D + i] ? -amp : amp;
                if (rng.uniform() < flip) v = -v;
                o[i * 3 + x] = (int8_t)v;
            }
        if (h_tx_bits) memcpy(h_tx_bits + (size_t)b * K, c.data(), K);
    }
    return MI_LTE_OK;
}

// same blocks through a BPSK/AWGN channel: float soft values 1-2b + sigma*n
int mi_lte_synth_turbo_soft_f32(uint32_t K, uint32_t n, double sigma, uint64_t seed, int ref_wrap, float *h_soft,
                                uint8_t *h_tx_bits)
{
    uint32_t f1, f2;
    if (!h_soft || !synth::qpp_params(K, &f1, &f2)) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t       D = K + 4;
    synth::Rng           rng(seed);
    std::vector<uint8_t> c(K), d(3 * D);
    for (uint32_t b = 0; b < n; b++) {
        for (uint32_t i = 0; i < K; i++) c[i] = (uint8_t)(rng.next() & 1u);
        synth::turbo_encode(c.data(), K, ref_wrap != 0, d.data());
        float *o = h_soft + (size_t)b * 3 * D;
        for (uint32_t i = 0; i < D; i++)
            for (int x = 0; x < 3; x++) o[i * 3 + x] = (float)((d[x * D + i] ? -1.0 : 1.0) + sigma * rng.normal());
        if (h_tx_bits) memcpy(h_tx_bits + (size_t)b * K, c.data(), K);
    }
    return MI_LTE_OK;
}

} // extern "C"
