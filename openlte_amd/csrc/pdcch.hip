// PCFICH + PDCCH common-search-space decoding on gfx950: restates liblte_phy_pdcch_channel_decode
// (liblte/src/liblte_phy.cc:4519-5135) for a batch of device subframes -- the step between the front end and
// liblte_phy_pdsch_channel_decode in every real subframe (LTE_fdd_dl_fs_samp_buf.cc:445-470).
//
// Everything that only depends on the cell and on the control-format indicator is index arithmetic and is done once
// per plan on the host (pdcch_geom.cc: the PCFICH and PHICH positions, the REG walk, the interleaver undo, the CCEs, the six
// common-search-space candidates and the rate-unmatching index map); what the DCIs mean is dci.cc's.  This file holds the
// kernels and the code that launches them.  The device does the arithmetic:
//
//   k_pdcch_decode : one workgroup per subframe, one wavefront per candidate.  PCFICH: gather, transmit-diversity
//       combiner, QPSK soft de-map, descramble, CFI by minimum distance (cfi_channel_decode :13648-13706).  Per candidate:
//       gather / combine / de-map / descramble (:4862-4905), then for DCI formats 1A and 1C: rate un-matching as an
//       LDS scatter-add, the reference's K = 7 Viterbi decoder (viterbi_decode :10161-10332: all states start at 0 -- it
//       is not tail-biting aware --, survivor chosen on the Hamming metric while a weighted metric is accumulated,
//       traceback by re-comparing stored metrics) with ONE TRELLIS STATE PER LANE (64 states = one wavefront; the two
//       predecessor metrics arrive by lane shuffle, the traceback compares are one ballot per step), CRC16 and the RNTI
//       test for SI-, P- and RA-RNTI (dci_channel_decode :12952-13040).
//   k_pdcch_search_demod / _decode / _compact : the PDCCH's own 3GPP mode (include/mi_lte.h), a blind search over the whole control region that
//       shares the PCFICH decoder, the de-mapper and the tables above and none of the reference's candidate handling: every CCE to int8 soft
//       bits with each port's own estimate; one wavefront per (unit, candidate at L = 8, 4, 2, 1, DCI size) with the tail-biting decoder of
//       tbcc_dev.h, CRC16, the RNTI bitmap and the search spaces of 36.213 9.1.1; the hits ordered and capped per unit.
// The soft values are integers from the de-mapper on, so the decoder is exact; the de-mapper itself (atan2f / sqrtf) is
// float.  Candidate CCEs past the last CCE of the subframe read stale scratch in the reference; here they count as erasures
// (what a fresh LIBLTE_PHY_STRUCT gives).
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "dci.h"
#include "pdcch_geom.h"
#include "pdcch_search.hpp"
#include "phy_dev.hpp"
#include "tbcc_dev.h"

using namespace pdcch_geom;

namespace {

struct PdcchDev {
    uint32_t N_rb_dl, N_ant, n_cells, dci_size[2];
    uint32_t per_port; // 1: every port's own estimate (MI_LTE_PDCCH_PER_PORT_ESTIMATES); 0: the rows the reference really reads
    const uint32_t *cells;    // [n_cells] cell ids the tables were built for
    const uint32_t *pcfich;   // [n_cells][16] RE index (l*1200 + k) of the PCFICH
    const uint32_t *cand;     // [n_cells][4 (N_symbs - 1)][N_CAND][RE_MAX] RE index, NO_RE = candidate absent
    const uint16_t *rm_map;   // [2 formats][2 (E = 288, 576)][576] position in d[3*N_c] of every received bit
};

struct PdcchResult { // per unit
    uint32_t cfi;            // 0: PCFICH did not decode
    uint32_t n_symbs;
    uint32_t rnti[12];       // slot = candidate*2 + format (0 = 1A, 1 = 1C); 0 = nothing found
    uint32_t payload[12];    // DCI bits, first bit in the MSB of the n-bit field
};

// transmit-diversity combiner of one group of N_ant resource elements (pre_decoder_and_matched_filter_dl,
// liblte_phy.cc:7645-7796); h[p][e]: estimate of port p at element e of the group
template <uint32_t N_ant>
__device__ __forceinline__ void combine(const float (&yr)[4], const float (&yi)[4], const float (&hr)[4][4], const float (&hi)[4][4], float (&xr)[4],
                                        float (&xi)[4])
{
    if (N_ant == 1) {
        const float hn = hr[0][0] * hr[0][0] + hi[0][0] * hi[0][0];
        xr[0] = (yr[0] * hr[0][0] + yi[0] * hi[0][0]) / hn;
        xi[0] = (yi[0] * hr[0][0] - yr[0] * hi[0][0]) / hn;
    } else if (N_ant == 2) {
        const float h0r = hr[0][0], h0i = hi[0][0], h1r = hr[1][0], h1i = hi[1][0];
        const float a0 = h0r * h0r + h0i * h0i, a1 = h1r * h1r + h1i * h1i, hn = sqrtf(a0 * a0 + a1 * a1);
        xr[0] = (h0r * yr[0] + h0i * yi[0] + h1r * yr[1] + h1i * yi[1]) / hn;
        xi[0] = (h0r * yi[0] - h0i * yr[0] - h1r * yi[1] + h1i * yr[1]) / hn;
        xr[1] = (-h1r * yr[0] - h1i * yi[0] + h0r * yr[1] + h0i * yi[1]) / hn;
        xi[1] = (h1r * yi[0] - h1i * yr[0] + h0r * yi[1] - h0i * yr[1]) / hn;
    } else {
        const float h0r = hr[0][0], h0i = hi[0][0], h2r = hr[2][0], h2i = hi[2][0];
        const float h1r = hr[1][2], h1i = hi[1][2], h3r = hr[3][2], h3i = hi[3][2];
        const float a0 = h0r * h0r + h0i * h0i, a1 = h1r * h1r + h1i * h1i, a2 = h2r * h2r + h2i * h2i, a3 = h3r * h3r + h3i * h3i;
        const float n02 = sqrtf(a0 * a0 + a2 * a2), n13 = sqrtf(a1 * a1 + a3 * a3);
        xr[0] = (h0r * yr[0] + h0i * yi[0] + h2r * yr[1] + h2i * yi[1]) / n02;
        xi[0] = (h0r * yi[0] - h0i * yr[0] - h2r * yi[1] + h2i * yr[1]) / n02;
        xr[1] = (-h2r * yr[0] - h2i * yi[0] + h0r * yr[1] + h0i * yi[1]) / n02;
        xi[1] = -(-h2r * yi[0] + h2i * yr[0] - h0r * yi[1] + h0i * yr[1]) / n02;
        xr[2] = (h1r * yr[2] + h1i * yi[2] + h3r * yr[3] + h3i * yi[3]) / n13;
        xi[2] = (h1r * yi[2] - h1i * yr[2] - h3r * yi[3] + h3i * yr[3]) / n13;
        xr[3] = (-h3r * yr[2] - h3i * yi[2] + h1r * yr[3] + h1i * yi[3]) / n13;
        xi[3] = -(-h3r * yi[2] + h3i * yr[2] - h1r * yi[3] + h1i * yr[3]) / n13;
    }
}

// gather -> combine -> QPSK soft de-map -> descramble for n_re resource elements listed in re[]; soft[2*n_re] integer soft bits
//
// Which estimate the combiner gets for port p.  The reference hands pre_decoder_and_matched_filter_dl the array
// pdcch_c_est_re[4][288] with a port stride of 576 (liblte_phy.cc:4881, :7935), so "port 1" is row 2, and "ports 2, 3"
// run off the end into pdcch_c_est_im rows 0, 2 (real part) and the transmitter's scratch (imaginary part, zeros in a
// receiver).  With two ports row 2 is never written: port 1's estimate is 0 and the second antenna goes unsuppressed; with
// four ports nothing decodes.  per_port = 0 reproduces exactly that (rows never written read as the zeros a fresh
// LIBLTE_PHY_STRUCT holds); per_port = 1 is the decoder the reference meant.
// (n_planes = number of channel-estimate planes the device subframe was laid out with; N_ant = ports the combiner assumes;
// ln, stride: this thread's first group and the number of threads that share the list -- a wavefront's lane and 64 unless given)
template <uint32_t N_ant>
__device__ __forceinline__ void demod_res_n(const float *__restrict__ base, uint32_t n_planes, uint32_t per_port, const uint32_t *__restrict__ re,
                                            uint32_t n_re, const GoldTables &gt, uint32_t c_init, uint32_t c_off, int *soft, uint32_t ln, uint32_t stride)
{
    const float *y_re_p = base, *y_im_p = base + 16 * N_SC_MAX, *h_re_p = base + 2 * 16 * N_SC_MAX;
    const float *h_im_p = h_re_p + (size_t)n_planes * 16 * N_SC_MAX;
    for (uint32_t g = ln; g < n_re / N_ant; g += stride) {
        float yr[4], yi[4], hr[4][4], hi[4][4], xr[4], xi[4];
        const bool absent = re[g * N_ant] == NO_RE;
        for (uint32_t e = 0; e < N_ant; e++) {
            const uint32_t p = absent ? 0u : re[g * N_ant + e];
            yr[e] = y_re_p[p]; yi[e] = y_im_p[p];
            for (uint32_t a = 0; a < N_ant; a++) { hr[a][e] = h_re_p[(size_t)a * 16 * N_SC_MAX + p]; hi[a][e] = h_im_p[(size_t)a * 16 * N_SC_MAX + p]; }
        }
        if (!per_port && N_ant == 2) {
            for (uint32_t e = 0; e < 2; e++) hr[1][e] = hi[1][e] = 0.0f;
        } else if (!per_port && N_ant == 4) {
            for (uint32_t e = 0; e < 4; e++) {
                const float re0 = hr[0][e], im0 = hi[0][e], re2 = hr[2][e], im2 = hi[2][e];
                (void)re0;
                hr[1][e] = re2; hi[1][e] = im2;
                hr[2][e] = im0; hi[2][e] = 0.0f;
                hr[3][e] = im2; hi[3][e] = 0.0f;
            }
        }
        combine<N_ant>(yr, yi, hr, hi, xr, xi);
        for (uint32_t e = 0; e < N_ant; e++) { // layer de-mapping d[g*N_ant + e] = x_e[g] (layer_demapper_dl, :7473-7514)
            int8_t b[6] = {0, 0, 0, 0, 0, 0};
            demap_symbol(xr[e], xi[e], 1 /* QPSK */, b);
            const uint32_t n = 2 * (g * N_ant + e), cn = c_off + n;
            const uint32_t w = gold_word(gt, c_init, cn >> 5), w2 = gold_word(gt, c_init, (cn + 1) >> 5);
            soft[n]     = absent ? 0 : ((w >> (cn & 31)) & 1u) ? -(int)b[0] : (int)b[0];
            soft[n + 1] = absent ? 0 : ((w2 >> ((cn + 1) & 31)) & 1u) ? -(int)b[1] : (int)b[1];
        }
    }
}

__device__ __forceinline__ void demod_res(const float *__restrict__ base, uint32_t n_planes, uint32_t N_ant, uint32_t per_port,
                                          const uint32_t *__restrict__ re, uint32_t n_re, const GoldTables &gt, uint32_t c_init, uint32_t c_off,
                                          int *soft, uint32_t ln, uint32_t stride = 64)
{
    // the port count is a template parameter so that the small per-group arrays stay in registers
    if (N_ant == 1) demod_res_n<1>(base, n_planes, per_port, re, n_re, gt, c_init, c_off, soft, ln, stride);
    else if (N_ant == 2) demod_res_n<2>(base, n_planes, per_port, re, n_re, gt, c_init, c_off, soft, ln, stride);
    else demod_res_n<4>(base, n_planes, per_port, re, n_re, gt, c_init, c_off, soft, ln, stride);
}

// The reference's K = 7, rate-1/3 Viterbi decoder (viterbi_decode, liblte_phy.cc:10161-10332) over N trellis steps, one state per
// lane: all states start at 0 (it is not tail-biting aware), the survivor is chosen on the Hamming branch metric while the
// weighted metric p + w*br is what is stored, the end state is the first strict minimum, and the traceback re-compares the
// stored metrics of each predecessor pair (one ballot per step, kept in dec[]).  d: 3N integer soft bits in LDS.  The decoded
// bits come back on lane 0, bit t at position t of (lo, hi).
__device__ __forceinline__ void viterbi_k7(const int *d, uint32_t N, uint64_t *dec, uint32_t ln, uint32_t &bits_lo, uint32_t &bits_hi)
{
    // trellis labels of this lane's state (:10197-10222): register = input bit | predecessor state
    const uint32_t G[3] = {0133, 0171, 0165};
    uint32_t lab[2] = {0, 0};
    for (uint32_t k = 0; k < 2; k++) {
        const uint32_t prev = (2 * ln + k) & 63u, reg = ((ln >> 5) << 6) | prev;
        for (uint32_t o = 0; o < 3; o++) lab[k] |= ((uint32_t)__popc(reg & G[o]) & 1u) << o;
    }
    int pm = 0;
    for (uint32_t i = 0; i < N; i++) {
        // which of each predecessor pair has the larger stored metric (what the traceback re-compares, :10300-10308)
        const int      up = __shfl_down(pm, 1);
        const uint64_t gt_mask = __ballot(pm > up); // bit 2m: pm[2m] > pm[2m+1]
        if (ln == 0) dec[i] = gt_mask;
        const int d0 = d[3 * i], d1 = d[3 * i + 1], d2 = d[3 * i + 2];
        const uint32_t in = (d0 < 0 ? 1u : 0u) | (d1 < 0 ? 2u : 0u) | (d2 < 0 ? 4u : 0u);
        const int      w  = abs(d0) + abs(d1) + abs(d2);
        const int      p0 = __shfl(pm, (2 * ln) & 63), p1 = __shfl(pm, (2 * ln + 1) & 63);
        const int      b0 = __popc(lab[0] ^ in), b1 = __popc(lab[1] ^ in);
        pm = (b0 + p0 > b1 + p1) ? p1 + w * b1 : p0 + w * b0; // select on the Hamming metric, accumulate the weighted one
    }
    // end state: first strict minimum (:10281-10292)
    int      best = pm;
    uint32_t st   = ln;
    for (int o = 32; o > 0; o >>= 1) {
        const int      ob = __shfl_xor(best, o);
        const uint32_t os = __shfl_xor(st, o);
        if (ob < best || (ob == best && os < st)) { best = ob; st = os; }
    }
    bits_lo = bits_hi = 0;
    if (ln == 0) {
        // traceback (:10294-10309) and bit read-out (:10313-10331): states s_N .. s_0, bit t from (s_{t+1}, s_t)
        uint32_t cur = st;
        for (int i = (int)N - 1; i >= 0; i--) {
            const uint32_t p0 = (2 * cur) & 63u;
            const uint32_t prev = ((dec[i] >> p0) & 1ull) ? p0 + 1 : p0;
            const uint32_t bit  = (cur < prev) ? 0u : (cur > prev) ? 1u : (cur == 0 ? 0u : 1u);
            if (i < 32) bits_lo |= bit << i; else bits_hi |= bit << (i - 32);
            cur = prev;
        }
    }
}

// CRC16 (polynomial 0x11021, calc_crc :9713-9743) of bits 0..n_info-1 XOR the 16 parity bits that follow them; bit t of the block at
// position t of (lo, hi).  Also returns the information bits, first bit in the MSB of an n_info-bit field.
__device__ __forceinline__ uint32_t crc16_syndrome(uint32_t bits_lo, uint32_t bits_hi, uint32_t n_info, uint32_t &payload)
{
    auto bit_at = [&](uint32_t t) { return t < 32 ? (bits_lo >> t) & 1u : (bits_hi >> (t - 32)) & 1u; };
    uint32_t rem = 0, par = 0;
    payload = 0;
    for (uint32_t t = 0; t < n_info + 16; t++) {
        rem = (rem << 1) | (t < n_info ? bit_at(t) : 0u);
        if (rem & 0x10000u) rem ^= 0x11021u;
    }
    for (uint32_t t = 0; t < n_info; t++) payload = (payload << 1) | bit_at(t);
    for (uint32_t t = 0; t < 16; t++) par = (par << 1) | bit_at(n_info + t);
    return (par ^ rem) & 0xFFFFu;
}

// PCFICH (pcfich_channel_demap + cfi_channel_decode) by one wavefront: gather / combine / de-map / descramble the 16 resource elements
// listed in re[] into pc_soft[32] (LDS), then the CFI by minimum distance; 0: no code word within CFI_N_ACCEPTABLE_BERS.  The same value on every lane.
__device__ __forceinline__ uint32_t pcfich_cfi(const float *__restrict__ base, uint32_t N_ant, uint32_t per_port, const uint32_t *__restrict__ re,
                                               const GoldTables &gt, uint32_t sf, uint32_t cell, int *pc_soft, uint32_t ln)
{
    demod_res(base, N_ant, N_ant, per_port, re, 16, gt, (((sf + 1) * (2 * cell + 1)) << 9) + cell, 0, pc_soft, ln);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    uint32_t bit = 0, m[4] = {0, 0, 0, 0};
    if (ln < 32) {
        bit = pc_soft[ln] >= 0 ? 0u : 1u;
        const uint32_t r = ln % 3; // CFI code words (36.212 table 5.3.4-1): 011 011.. | 101 101.. | 110 110.. | all zero
        m[0] = ((r == 0 ? 0u : 1u) != bit); m[1] = ((r == 1 ? 0u : 1u) != bit); m[2] = ((r == 2 ? 0u : 1u) != bit); m[3] = (0u != bit);
    }
    uint32_t ber[4];
    for (int k = 0; k < 4; k++) ber[k] = (uint32_t)__popcll(__ballot(ln < 32 && m[k]));
    uint32_t min_ber = 32, cfi = 0;
    for (uint32_t k = 0; k < 4; k++)
        if (ber[k] < min_ber) { min_ber = ber[k]; cfi = k + 1; }
    return (min_ber < 4) ? cfi : 0u; // CFI_N_ACCEPTABLE_BERS (:2092)
}

__global__ __launch_bounds__(384) void k_pdcch_decode(const float *__restrict__ subframes, uint32_t sf_stride,
                                                      const uint32_t *__restrict__ subfr_num, const uint32_t *__restrict__ n_id_cell,
                                                      PdcchDev P, GoldTables gt, PdcchResult *__restrict__ out)
{
    __shared__ int      soft[N_CAND][2 * RE_MAX];
    __shared__ int      dbits[N_CAND][3 * 48];
    __shared__ uint64_t dec[N_CAND][48];
    __shared__ int      pc_soft[32];
    __shared__ uint32_t s_cfi, s_cell_idx;
    const uint32_t unit = blockIdx.x, wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const uint32_t sf = subfr_num[unit], cell = n_id_cell[unit];
    const float   *base = subframes + (size_t)unit * sf_stride;
    PdcchResult   *res  = out + unit;

    if (threadIdx.x == 0) {
        uint32_t ci = 0xFFFFFFFFu;
        for (uint32_t k = 0; k < P.n_cells; k++)
            if (P.cells[k] == cell) { ci = k; break; }
        s_cell_idx = ci;
        s_cfi      = 0;
    }
    if (threadIdx.x < 12) { res->rnti[threadIdx.x] = 0; res->payload[threadIdx.x] = 0; }
    __syncthreads();
    const uint32_t ci = s_cell_idx;
    if (ci == 0xFFFFFFFFu) { // a cell the plan was not built for
        if (threadIdx.x == 0) { res->cfi = 0; res->n_symbs = 0; }
        return;
    }
    // ---- PCFICH (pcfich_channel_demap + cfi_channel_decode)
    if (wave == 0) {
        const uint32_t cfi = pcfich_cfi(base, P.N_ant, P.per_port, P.pcfich + (size_t)ci * 16, gt, sf, cell, pc_soft, ln);
        if (ln == 0) s_cfi = cfi;
    }
    __syncthreads();
    const uint32_t cfi = s_cfi, n_symbs = cfi + (P.N_rb_dl <= 10 ? 1u : 0u);
    if (threadIdx.x == 0) { res->cfi = cfi; res->n_symbs = cfi ? n_symbs : 0; }
    if (cfi == 0 || n_symbs > 4 || wave >= N_CAND) return;

    // ---- one candidate per wave
    const uint32_t  c = wave, n_re = c < 4 ? 144u : 288u, E = 2 * n_re;
    const uint32_t *re = P.cand + (((size_t)ci * 4 + (n_symbs - 1)) * N_CAND + c) * RE_MAX;
    if (re[0] == NO_RE) return; // the candidate reaches past the last CCE
    const uint32_t c_off = c < 4 ? c * 288u : (c - 4) * 576u; // offset into the subframe's scrambling sequence (:4908, :5035)
    demod_res(base, P.N_ant, P.N_ant, P.per_port, re, n_re, gt, (sf << 9) + cell, c_off, soft[c], ln);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();

    for (uint32_t f = 0; f < 2; f++) {
        const uint32_t n_out = P.dci_size[f], N = n_out + 16; // information + CRC bits = trellis steps
        // rate un-matching with soft combining (rate_unmatch_conv): every received bit adds onto its d position
        for (uint32_t k = ln; k < 3 * N; k += 64) dbits[c][k] = 0;
        __builtin_amdgcn_wave_barrier();
        const uint16_t *map = P.rm_map + ((size_t)f * 2 + (c < 4 ? 0 : 1)) * 576;
        for (uint32_t k = ln; k < E; k += 64) atomicAdd(&dbits[c][map[k]], soft[c][k]);
        __builtin_amdgcn_s_waitcnt(0);
        __builtin_amdgcn_wave_barrier();
        uint32_t bits_lo, bits_hi;
        viterbi_k7(dbits[c], N, dec[c], ln, bits_lo, bits_hi);
        if (ln == 0) {
            uint32_t       payload;
            const uint32_t x = crc16_syndrome(bits_lo, bits_hi, n_out, payload); // = RNTI when the CRC matches (UE antenna mask 0)
            if (x == 0xFFFFu || x == 0xFFFEu || (x >= 1 && x <= 0x3Cu)) { // SI-, P-, RA-RNTI (:4915-4947)
                res->rnti[c * 2 + f]    = x;
                res->payload[c * 2 + f] = payload;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- blind search over the whole control region (include/mi_lte.h: "PDCCH, 3GPP mode") -------------------------------------
constexpr uint32_t SEARCH_N_MAX = 64 + 16, SEARCH_WAVES = 4, SEARCH_CHUNK_CCE = 16, SEARCH_MAP = 576, NO_CELL = 0xFFFFFFFFu;

struct PdcchSearchDev {
    uint32_t N_rb_dl, N_ant, n_cells, n_sizes, n_bits[MI_LTE_PDCCH_SEARCH_MAX_SIZES], flags;
    uint32_t max_cce, max_waves;  // the largest N_cce of the tables and the (candidate, size) pairs it has
    uint32_t unit_stride;         // soft bits per unit: 72 max_cce
    const uint32_t *cells;        // [n_cells]
    const uint32_t *pcfich;       // [n_cells][16]
    const uint32_t *n_cce;        // [n_cells][4 (N_symbs - 1)]
    const uint32_t *cce_re;       // [n_cells][4][36 max_cce] RE index of every CCE's elements in order
    const uint16_t *rm_map;       // [n_sizes][SEARCH_MAP] position in d[3 N] of received bit k (of a candidate of any L)
    const uint32_t *rnti_bits;    // [2048] the RNTI set
};
struct SearchUnit { uint32_t cfi, n_cce; };
struct SearchHit { uint64_t payload; int32_t metric, energy; };
struct SearchOut { uint32_t cfi, n_cce, n_found, pad; mi_lte_pdcch_found found[MI_LTE_PDCCH_SEARCH_MAX_FOUND]; };

// one workgroup per subframe: CFI, then every CCE de-mapped to int8 soft bits, SEARCH_CHUNK_CCE CCEs at a time through LDS
__global__ __launch_bounds__(256) void k_pdcch_search_demod(const float *__restrict__ subframes, uint32_t sf_stride, const uint32_t *__restrict__ subfr_num,
                                                            const uint32_t *__restrict__ n_id_cell, PdcchSearchDev P, GoldTables gt,
                                                            SearchUnit *__restrict__ units, int8_t *__restrict__ soft_out)
{
    __shared__ int      soft[72 * SEARCH_CHUNK_CCE];
    __shared__ int      pc_soft[32];
    __shared__ uint32_t s_cfi, s_cell_idx;
    const uint32_t unit = blockIdx.x, wave = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const uint32_t sf = subfr_num[unit], cell = n_id_cell[unit];
    const float   *base = subframes + (size_t)unit * sf_stride;
    if (threadIdx.x == 0) {
        uint32_t ci = NO_CELL;
        for (uint32_t k = 0; k < P.n_cells; k++)
            if (P.cells[k] == cell) { ci = k; break; }
        s_cell_idx = sf <= 9 ? ci : NO_CELL; // (a subframe number the scrambler and the search spaces have no meaning for)
        s_cfi      = 0;
    }
    __syncthreads();
    const uint32_t ci = s_cell_idx;
    if (ci != NO_CELL && wave == 0) {
        const uint32_t cfi = pcfich_cfi(base, P.N_ant, 1, P.pcfich + (size_t)ci * 16, gt, sf, cell, pc_soft, ln);
        if (ln == 0) s_cfi = cfi;
    }
    __syncthreads();
    const uint32_t n_symbs = s_cfi + (P.N_rb_dl <= 10 ? 1u : 0u);
    const bool     ok = ci != NO_CELL && s_cfi != 0 && n_symbs <= 4;
    const uint32_t cfi = ok ? s_cfi : 0u, n_cce = ok ? min(P.n_cce[(size_t)ci * 4 + n_symbs - 1], P.max_cce) : 0u;
    if (threadIdx.x == 0) units[unit] = SearchUnit{cfi, n_cce};
    if (n_cce == 0) return; // (uniform)
    const uint32_t *re  = P.cce_re + ((size_t)ci * 4 + n_symbs - 1) * 36 * P.max_cce;
    int8_t         *out = soft_out + (size_t)unit * P.unit_stride;
    for (uint32_t c0 = 0; c0 < n_cce; c0 += SEARCH_CHUNK_CCE) { // (uniform)
        const uint32_t nc = min(SEARCH_CHUNK_CCE, n_cce - c0);
        demod_res(base, P.N_ant, P.N_ant, 1, re + 36 * c0, 36 * nc, gt, (sf << 9) + cell, 72 * c0, soft, threadIdx.x, 256);
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 72 * nc; k += 256) out[72 * c0 + k] = (int8_t)soft[k];
        __syncthreads();
    }
}

// one wavefront per (unit, candidate, size); nothing in here waits for another wavefront
__global__ __launch_bounds__(64 * SEARCH_WAVES) void k_pdcch_search_decode(const int8_t *__restrict__ soft, const SearchUnit *__restrict__ units,
                                                                           const uint32_t *__restrict__ subfr_num, PdcchSearchDev P, uint32_t blocks_per_unit,
                                                                           uint16_t *__restrict__ hit_rnti, SearchHit *__restrict__ hit_rec)
{
    __shared__ int32_t  d_all[SEARCH_WAVES][3 * SEARCH_N_MAX];
    __shared__ uint64_t surv_all[SEARCH_WAVES][3 * SEARCH_N_MAX];
    __shared__ uint8_t  cb_all[SEARCH_WAVES][SEARCH_N_MAX];
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), ln = threadIdx.x & 63;
    const uint32_t unit = blockIdx.x / blocks_per_unit, w = (blockIdx.x - unit * blocks_per_unit) * SEARCH_WAVES + wv;
    const uint32_t n_cce = units[unit].n_cce, cand = w / P.n_sizes, si = w - cand * P.n_sizes;
    if (cand >= search_n_cand(n_cce)) return; // (uniform per wavefront, like everything up to the CRC)
    uint32_t L, cce;
    search_cand(n_cce, cand, L, cce);
    const uint32_t n_bits = si == 0 ? P.n_bits[0] : si == 1 ? P.n_bits[1] : si == 2 ? P.n_bits[2] : P.n_bits[3];
    const uint32_t N = n_bits + 16, E = 72 * L, P3 = 3 * N;
    uint16_t      *hit = hit_rnti + (size_t)unit * P.max_waves + w;
    if (N >= E || N > SEARCH_N_MAX) { // no redundancy left
        if (ln == 0) *hit = 0;
        return;
    }
    int32_t  *d    = d_all[wv];
    uint64_t *surv = surv_all[wv];
    uint8_t  *cb   = cb_all[wv];
    auto      wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); };
    // a. rate un-matching: the circular buffer without its dummies has period 3 N, so every d position gathers its own repeats
    const int8_t   *e   = soft + (size_t)unit * P.unit_stride + 72 * cce;
    const uint16_t *map = P.rm_map + (size_t)si * SEARCH_MAP;
    int32_t         energy = 0;
    for (uint32_t r = ln; r < P3; r += 64) {
        int32_t s = 0;
        for (uint32_t k = r; k < E; k += P3) s += e[k];
        d[map[r]] = s;
        energy += abs(s);
    }
    energy = wave_sum(energy);
    wave_sync();
    if (energy == 0) { // b. an empty region
        if (ln == 0) *hit = 0;
        return;
    }
    int32_t metric;
    tbcc_decode(d, N, surv, cb, ln, wave_sync, metric); // c.
    if (ln == 0) { // d. CRC16 and acceptance
        uint32_t rem = 0, par = 0;
        uint64_t payload = 0;
        for (uint32_t i = 0; i < N; i++) {
            rem = (rem << 1) | (i < n_bits ? cb[i] : 0u);
            if (rem & 0x10000u) rem ^= 0x11021u;
            if (i < n_bits) payload = (payload << 1) | cb[i];
            else par = (par << 1) | cb[i];
        }
        const uint32_t x = (rem ^ par) & 0xFFFFu;
        bool ok = x != 0 && ((P.rnti_bits[x >> 5] >> (x & 31u)) & 1u);
        if (ok && !(P.flags & MI_LTE_PDCCH_SEARCH_ANY_CCE) && !(L >= 4 && cce < 16)) { // not in the common search space: x's own candidates
            const uint32_t y = search_space_y(x, subfr_num[unit]), nl = n_cce / L; // (nl >= 1: the candidate exists)
            ok = false;
            for (uint32_t m = 0; m < search_space_m(L); m++) ok = ok || L * ((y + m) % nl) == cce;
        }
        *hit = ok ? (uint16_t)x : (uint16_t)0;
        if (ok) hit_rec[(size_t)unit * P.max_waves + w] = SearchHit{payload, metric, energy};
    }
}

// one wavefront per unit: the hits in wave order (= L descending, first CCE ascending, size position ascending), the first MAX_FOUND kept
__global__ __launch_bounds__(64) void k_pdcch_search_compact(const SearchUnit *__restrict__ units, PdcchSearchDev P, const uint16_t *__restrict__ hit_rnti,
                                                             const SearchHit *__restrict__ hit_rec, SearchOut *__restrict__ out)
{
    const uint32_t   unit = blockIdx.x, ln = threadIdx.x;
    const SearchUnit u = units[unit];
    const uint32_t   n_w = search_n_cand(u.n_cce) * P.n_sizes;
    SearchOut       *o = out + unit;
    uint32_t         total = 0;
    for (uint32_t w0 = 0; w0 < n_w; w0 += 64) { // (uniform)
        const uint32_t w = w0 + ln, x = w < n_w ? hit_rnti[(size_t)unit * P.max_waves + w] : 0u;
        const uint64_t m = __ballot(x != 0);
        const uint32_t rank = total + (uint32_t)__popcll(m & ((1ull << ln) - 1));
        if (x != 0 && rank < MI_LTE_PDCCH_SEARCH_MAX_FOUND) {
            const uint32_t  cand = w / P.n_sizes, si = w - cand * P.n_sizes;
            const SearchHit h = hit_rec[(size_t)unit * P.max_waves + w];
            uint32_t        L, cce;
            search_cand(u.n_cce, cand, L, cce);
            mi_lte_pdcch_found f;
            f.rnti = x; f.L = L; f.cce = cce;
            f.n_bits = si == 0 ? P.n_bits[0] : si == 1 ? P.n_bits[1] : si == 2 ? P.n_bits[2] : P.n_bits[3];
            f.payload = h.payload; f.metric = h.metric; f.energy = h.energy;
            o->found[rank] = f;
        }
        total += (uint32_t)__popcll(m);
    }
    if (ln < MI_LTE_PDCCH_SEARCH_MAX_FOUND && ln >= total) o->found[ln] = mi_lte_pdcch_found{0, 0, 0, 0, 0, 0, 0};
    if (ln == 0) { o->cfi = u.cfi; o->n_cce = u.n_cce; o->n_found = total; o->pad = 0; }
}

// ---- PBCH (liblte_phy_bch_channel_decode, liblte_phy.cc:3968-4105; bch_channel_decode :12581-12650) ----------------------
// One workgroup per subframe 0, twelve wavefronts = {1, 2, 4 antenna ports} x {4 positions in the 40 ms BCH period}: each gathers
// the 240 PBCH resource elements (symbols 7-10, centre 72 sub-carriers, CRS positions of symbols 7, 8 left out) with the
// estimates of the ports its hypothesis needs, combines / de-maps / descrambles with the quarter of the 1920-bit sequence its
// position selects, rate-un-matches (every d position gets 4 of the 480 bits), runs the same Viterbi decoder over 40 steps and
// checks CRC16 against its port-count mask.  The reference tries the hypotheses in this order and stops at the first success:
// the lowest successful wave index wins.
struct PbchLap { uint8_t pos[120]; }; // d position (3i + x) of the k-th bit of one lap of the circular buffer (40 bits per stream)
struct PbchResult { uint32_t N_ant, offset, mib; };

__global__ __launch_bounds__(768) void k_pbch_decode(const float *__restrict__ subframes, uint32_t sf_stride, uint32_t N_rb_dl,
                                                     const uint32_t *__restrict__ n_id_cell, PbchLap lap, GoldTables gt,
                                                     PbchResult *__restrict__ out)
{
    __shared__ uint32_t re[240];
    __shared__ int      soft[12][480];
    __shared__ int      dbits[12][120];
    __shared__ uint64_t dec[12][40];
    __shared__ uint32_t s_mib[12], s_win;
    const uint32_t unit = blockIdx.x, wave = threadIdx.x >> 6, ln = threadIdx.x & 63, cell = n_id_cell[unit];
    const float   *base = subframes + (size_t)unit * sf_stride;
    if (threadIdx.x < 240) {
        const uint32_t t = threadIdx.x, k0 = 6 * N_rb_dl - 36, r = cell % 3;
        uint32_t sym, i;
        if (t < 96) { // symbols 7, 8: the two non-CRS residues of every group of three sub-carriers
            const uint32_t j = t % 48, lo = r == 0 ? 1u : 0u, hi = r == 2 ? 1u : 2u;
            sym = 7 + t / 48;
            i   = 3 * (j / 2) + ((j & 1) ? hi : lo);
        } else {
            sym = 9 + (t - 96) / 72;
            i   = (t - 96) % 72;
        }
        re[t] = sym * N_SC_MAX + k0 + i;
    }
    if (threadIdx.x == 0) s_win = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t p = wave < 4 ? 1u : wave < 8 ? 2u : 4u, off = wave & 3u;
    demod_res(base, 4, p, 1, re, 240, gt, cell, off * 480, soft[wave], ln); // the PBCH estimates are strided correctly (:4030)
    for (uint32_t k = ln; k < 120; k += 64) dbits[wave][k] = 0;
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    for (uint32_t k = ln; k < 480; k += 64) atomicAdd(&dbits[wave][lap.pos[k % 120]], soft[wave][k]);
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    uint32_t bits_lo, bits_hi;
    viterbi_k7(dbits[wave], 40, dec[wave], ln, bits_lo, bits_hi);
    if (ln == 0) {
        uint32_t       mib;
        const uint32_t x = crc16_syndrome(bits_lo, bits_hi, 24, mib), mask = p == 1 ? 0u : p == 2 ? 0xFFFFu : 0x5555u; // 36.212 table 5.3.1.1-1
        s_mib[wave] = mib;
        if (x == mask) atomicMin(&s_win, wave);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t w = s_win;
        out[unit] = w == 0xFFFFFFFFu ? PbchResult{0, 0, 0} : PbchResult{w < 4 ? 1u : w < 8 ? 2u : 4u, w & 3u, s_mib[w]};
    }
}

} // namespace

struct mi_lte_pdcch_plan {
    mi_lte_dl_cfg cfg;
    PdcchDev      dev{};
    std::vector<void *> owned;
};

struct mi_lte_pdcch_search_plan {
    mi_lte_dl_cfg  cfg;
    PdcchSearchDev dev{};
    uint32_t      *d_rnti_bits = nullptr;
    std::vector<void *> owned; // the tables
    // what a run fills, sized for the largest batch seen (cap_units)
    uint32_t    cap_units = 0;
    bool        ran = false;
    int8_t     *d_soft = nullptr;
    SearchUnit *d_units = nullptr;
    uint16_t   *d_hit = nullptr;  // [unit][max_waves] the RNTI found by that (candidate, size) pair, 0 = none
    SearchHit  *d_rec = nullptr;  // [unit][max_waves] written where d_hit is not 0
    SearchOut  *d_out = nullptr;
    std::vector<SearchOut> h_out;
};

extern "C" {

int mi_lte_pdcch_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, float phich_res, uint32_t phich_dur_extended, uint32_t flags,
                             const uint32_t *h_cells, uint32_t n_cells, mi_lte_pdcch_plan **out)
{
    if (!ctx || !cfg || !h_cells || n_cells == 0 || !out) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t nrb = cfg->N_rb_dl;
    if (!standard_ctrl_cfg(nrb, phich_res) || !(cfg->N_ant == 1 || cfg->N_ant == 2 || cfg->N_ant == 4) ||
        phich_dur_extended) { // the reference does not handle the extended PHICH duration either (:8280-8283)
        ctx->err = "PDCCH plan: standard bandwidths, 1/2/4 ports, PHICH resource in (0, 2], normal PHICH duration";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl = new mi_lte_pdcch_plan();
    auto  guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_lte_pdcch_plan_destroy(nullptr, pl); });
    pl->cfg  = *cfg;
    std::vector<uint32_t> cells(h_cells, h_cells + n_cells), pcf((size_t)n_cells * 16), cand((size_t)n_cells * 4 * N_CAND * RE_MAX);
    for (uint32_t c = 0; c < n_cells; c++) {
        if (cells[c] > 503) return MI_LTE_ERR_INVALID_ARG;
        for (uint32_t ns = 1; ns <= 4; ns++)
            mi_lte_pdcch_re_tables(nrb, cfg->N_ant, cells[c], phich_res, ns, &pcf[(size_t)c * 16], &cand[((size_t)c * 4 + ns - 1) * N_CAND * RE_MAX]);
    }
    uint32_t sz[2];
    dci::sizes(nrb, &sz[0], &sz[1]);
    std::vector<uint16_t> rm((size_t)2 * 2 * 576, 0);
    for (uint32_t f = 0; f < 2; f++)
        for (uint32_t e = 0; e < 2; e++) conv_rm_map(sz[f] + 16, e ? 576 : 288, &rm[((size_t)f * 2 + e) * 576]);
    auto up = [&](const void *h, size_t bytes, void **d) -> int {
        if (hipMalloc(d, bytes ? bytes : 4) != hipSuccess) return -1;
        pl->owned.push_back(*d);
        return mi_lte_memcpy_h2d(ctx, *d, h, bytes) == MI_LTE_OK ? 0 : -1;
    };
    void *d_cells, *d_pcf, *d_cand, *d_rm;
    if (up(cells.data(), cells.size() * 4, &d_cells) || up(pcf.data(), pcf.size() * 4, &d_pcf) || up(cand.data(), cand.size() * 4, &d_cand) ||
        up(rm.data(), rm.size() * 2, &d_rm)) {
        ctx->err = "PDCCH plan: device allocation failed";
        return MI_LTE_ERR_NOMEM;
    }
    MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx));
    pl->dev = PdcchDev{nrb, cfg->N_ant, n_cells, {sz[0], sz[1]}, (flags & MI_LTE_PDCCH_PER_PORT_ESTIMATES) ? 1u : 0u, (const uint32_t *)d_cells, (const uint32_t *)d_pcf, (const uint32_t *)d_cand,
                       (const uint16_t *)d_rm};
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}

void mi_lte_pdcch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pdcch_plan *pl)
{
    if (!pl) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    for (void *p : pl->owned) (void)hipFree(p);
    delete pl;
}

int mi_lte_pdcch_decode_run(mi_lte_ctx *ctx, mi_lte_pdcch_plan *pl, const float *d_subframes, const uint32_t *d_subfr_num,
                            const uint32_t *d_n_id_cell, uint32_t n_units, uint32_t *h_rc, uint32_t *h_cfi, uint32_t *h_n_symbs, uint32_t *h_n_dci,
                            mi_lte_pdcch_dci *h_dci /*[n_units][MI_LTE_PDCCH_MAX_DCI]*/)
{
    if (!ctx || !pl || !d_subframes || !d_subfr_num || !d_n_id_cell || n_units == 0 || !h_rc || !h_cfi || !h_n_symbs || !h_n_dci || !h_dci)
        return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = mi_ctx_gold_tables(ctx);
    if (rc != MI_LTE_OK) return rc;
    // a few units' results go straight into pinned host memory; a batch's through scratch and one copy
    const size_t res_bytes = sizeof(PdcchResult) * (size_t)n_units;
    PdcchResult *d_res, *h_res = nullptr;
    if (mi_ctx_small_results(ctx, res_bytes, (void **)&h_res, (void **)&d_res) != MI_LTE_OK) {
        h_res = nullptr;
        rc = mi_ctx_reserve_scratch(ctx, res_bytes);
        if (rc != MI_LTE_OK) return rc;
        d_res = (PdcchResult *)ctx->scratch;
    }
    GoldTables   gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
    MI_LAUNCH(ctx, "k_pdcch_decode", k_pdcch_decode, dim3(n_units), dim3(384), 0, d_subframes, (uint32_t)mi_lte_subframe_floats(pl->cfg.N_ant),
              d_subfr_num, d_n_id_cell, pl->dev, gt, d_res);
    MI_HIP_CHECK(ctx, hipGetLastError());
    std::vector<PdcchResult> res_copy;
    if (!h_res) {
        res_copy.resize(n_units);
        MI_D2H(ctx, res_copy.data(), d_res, res_bytes);
    }
    MI_HIP_CHECK(ctx, h_res ? mi_stream_wait(ctx, n_units) : hipStreamSynchronize(ctx->stream)); // (a copy into pageable memory is done when the runtime says so)
    const PdcchResult *res = h_res ? h_res : res_copy.data();
    for (uint32_t u = 0; u < n_units; u++) {
        h_cfi[u]     = res[u].cfi;
        h_n_symbs[u] = res[u].n_symbs;
        uint32_t n = 0, rc = res[u].cfi ? 1u : 3u; // INVALID_INPUTS until an unpacker ran; INVALID_CRC: no CFI (:4519-4571)
        mi_lte_pdcch_dci *o = h_dci + (size_t)u * MI_LTE_PDCCH_MAX_DCI;
        // the reference's order: aggregation-4 candidates 0..3 (1A then 1C each), then aggregation-8 candidates 0, 1; at most
        // LIBLTE_PHY_PDCCH_MAX_ALLOC = 6 allocations; a 1A that does not unpack is not counted (:4948-4960)
        for (uint32_t slot = 0; slot < 12 && n < MI_LTE_PDCCH_MAX_DCI; slot++) {
            if (res[u].rnti[slot] == 0) continue;
            mi_lte_pdcch_dci d;
            memset(&d, 0, sizeof(d));
            d.rnti = res[u].rnti[slot]; d.format = slot & 1; d.candidate = slot >> 1; d.n_bits = pl->dev.dci_size[slot & 1];
            d.payload = res[u].payload[slot];
            d.alloc.unit = u;
            const int urc = d.format == 0 ? mi_lte_dci_1a_unpack(d.payload, d.n_bits, d.rnti, pl->dev.N_rb_dl, pl->dev.N_ant, &d)
                                          : mi_lte_dci_1c_unpack(d.payload, d.n_bits, d.rnti, pl->dev.N_rb_dl, pl->dev.N_ant, &d);
            rc = urc == 0 ? 0u : 4u;  // the reference returns whatever its last unpacker call returned
            if (urc != 0) continue; // not counted (:4948-4960, :4989-5000)
            d.alloc_valid = 1;
            d.alloc.n_pdcch_symbs = res[u].n_symbs; // the allocation can go into a PDSCH plan as it is
            o[n++] = d;
        }
        h_n_dci[u] = n;
        h_rc[u]    = rc;
    }
    ctx->last_kernels = "k_pdcch_decode:1";
    return MI_LTE_OK;
}


// liblte_phy_bch_channel_decode for a batch of device subframes (subframe 0 of a frame, estimated for 4 ports as the reference's
// callers do, LTE_fdd_dl_fs_samp_buf.cc:395-410): h_N_ant[u] = 0 is LIBLTE_ERROR_DECODE_FAIL
int mi_lte_pbch_decode_run(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const float *d_subframes, const uint32_t *d_n_id_cell, uint32_t n_units,
                           uint32_t *h_N_ant, uint32_t *h_offset, uint32_t *h_mib)
{
    if (!ctx || !cfg || !d_subframes || !d_n_id_cell || n_units == 0 || !h_N_ant || !h_offset || !h_mib) return MI_LTE_ERR_INVALID_ARG;
    if (cfg->N_ant != 4 || cfg->N_rb_dl < 6 || cfg->N_rb_dl > 100) {
        ctx->err = "PBCH decode reads the estimates of all four ports: the device subframes must be laid out with N_ant = 4";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = mi_ctx_gold_tables(ctx);
    if (rc != MI_LTE_OK) return rc;
    const size_t res_bytes = sizeof(PbchResult) * (size_t)n_units;
    PbchResult  *d_res, *h_res = nullptr;
    if (mi_ctx_small_results(ctx, res_bytes, (void **)&h_res, (void **)&d_res) != MI_LTE_OK) {
        h_res = nullptr;
        rc = mi_ctx_reserve_scratch(ctx, res_bytes);
        if (rc != MI_LTE_OK) return rc;
        d_res = (PbchResult *)ctx->scratch;
    }
    PbchLap  lap;
    uint16_t map[120];
    conv_rm_map(40, 120, map);
    for (uint32_t k = 0; k < 120; k++) lap.pos[k] = (uint8_t)map[k];
    GoldTables  gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
    MI_LAUNCH(ctx, "k_pbch_decode", k_pbch_decode, dim3(n_units), dim3(768), 0, d_subframes, (uint32_t)mi_lte_subframe_floats(4), cfg->N_rb_dl, d_n_id_cell,
              lap, gt, d_res);
    MI_HIP_CHECK(ctx, hipGetLastError());
    std::vector<PbchResult> res_copy;
    if (!h_res) {
        res_copy.resize(n_units);
        MI_D2H(ctx, res_copy.data(), d_res, res_bytes);
    }
    MI_HIP_CHECK(ctx, h_res ? mi_stream_wait(ctx, n_units) : hipStreamSynchronize(ctx->stream));
    const PbchResult *res = h_res ? h_res : res_copy.data();
    for (uint32_t u = 0; u < n_units; u++) { h_N_ant[u] = res[u].N_ant; h_offset[u] = res[u].offset; h_mib[u] = res[u].mib; }
    ctx->last_kernels = "k_pbch_decode:1";
    return MI_LTE_OK;
}

// ---- the blind search's plan and run (include/mi_lte.h: "PDCCH, 3GPP mode") ----------------------------------------------------

int mi_lte_pdcch_search_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, float phich_res, uint32_t phich_dur_extended, uint32_t flags,
                                    const uint32_t *h_cells, uint32_t n_cells, const uint32_t *h_n_bits, uint32_t n_sizes, mi_lte_pdcch_search_plan **out)
{
    if (!ctx || !cfg || !h_cells || n_cells == 0 || !h_n_bits || !out) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t nrb = cfg->N_rb_dl;
    if (!standard_ctrl_cfg(nrb, phich_res) || !(cfg->N_ant == 1 || cfg->N_ant == 2 || cfg->N_ant == 4) || phich_dur_extended) {
        ctx->err = "PDCCH search plan: standard bandwidths, 1/2/4 ports, PHICH resource in (0, 2], normal PHICH duration";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    if (n_sizes == 0 || n_sizes > MI_LTE_PDCCH_SEARCH_MAX_SIZES || (flags & ~(MI_LTE_PDCCH_SEARCH_ANY_CCE | MI_LTE_PDCCH_SEARCH_36211_REGS))) return MI_LTE_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n_sizes; i++) {
        if (h_n_bits[i] < 8 || h_n_bits[i] > 64) return MI_LTE_ERR_INVALID_ARG;
        for (uint32_t j = 0; j < i; j++)
            if (h_n_bits[j] == h_n_bits[i]) return MI_LTE_ERR_INVALID_ARG;
    }
    for (uint32_t c = 0; c < n_cells; c++)
        if (h_cells[c] > 503) return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl = new mi_lte_pdcch_search_plan();
    auto  guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_lte_pdcch_search_plan_destroy(nullptr, pl); });
    pl->cfg = *cfg;
    // every CCE's resource elements, per cell and region size; the tables' extent is the largest N_cce among them
    std::vector<std::vector<uint32_t>> perm((size_t)n_cells * 4);
    std::vector<uint32_t> cells(h_cells, h_cells + n_cells), pcf((size_t)n_cells * 16), ncce((size_t)n_cells * 4), cand(N_CAND * RE_MAX);
    uint32_t max_cce = 0;
    for (uint32_t c = 0; c < n_cells; c++) {
        const int rc = mi_lte_pdcch_re_tables(nrb, cfg->N_ant, cells[c], phich_res, 1, &pcf[(size_t)c * 16], cand.data());
        if (rc != MI_LTE_OK) return rc;
        for (uint32_t ns = 1; ns <= 4; ns++) {
            ncce[(size_t)c * 4 + ns - 1] = cce_res(nrb, cfg->N_ant, cells[c], phich_res, ns, perm[(size_t)c * 4 + ns - 1], (flags & MI_LTE_PDCCH_SEARCH_36211_REGS) != 0);
            max_cce = std::max(max_cce, ncce[(size_t)c * 4 + ns - 1]);
        }
    }
    std::vector<uint32_t> res((size_t)n_cells * 4 * 36 * max_cce, NO_RE);
    for (size_t t = 0; t < perm.size(); t++) std::copy(perm[t].begin(), perm[t].begin() + 36 * (size_t)ncce[t], res.begin() + t * 36 * max_cce);
    std::vector<uint16_t> rm((size_t)n_sizes * SEARCH_MAP, 0);
    for (uint32_t i = 0; i < n_sizes; i++) conv_rm_map(h_n_bits[i] + 16, SEARCH_MAP, &rm[(size_t)i * SEARCH_MAP]);
    const std::vector<uint32_t> no_rnti(2048, 0);
    auto up = [&](const void *h, size_t bytes, void **d) -> int {
        if (hipMalloc(d, bytes ? bytes : 4) != hipSuccess) return -1;
        pl->owned.push_back(*d);
        return mi_lte_memcpy_h2d(ctx, *d, h, bytes) == MI_LTE_OK ? 0 : -1;
    };
    void *d_cells, *d_pcf, *d_ncce, *d_res, *d_rm, *d_bits;
    if (up(cells.data(), cells.size() * 4, &d_cells) || up(pcf.data(), pcf.size() * 4, &d_pcf) || up(ncce.data(), ncce.size() * 4, &d_ncce) ||
        up(res.data(), res.size() * 4, &d_res) || up(rm.data(), rm.size() * 2, &d_rm) || up(no_rnti.data(), no_rnti.size() * 4, &d_bits)) {
        ctx->err = "PDCCH search plan: device allocation failed";
        return MI_LTE_ERR_NOMEM;
    }
    MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx));
    PdcchSearchDev &D = pl->dev;
    D = PdcchSearchDev{};
    D.N_rb_dl = nrb; D.N_ant = cfg->N_ant; D.n_cells = n_cells; D.n_sizes = n_sizes; D.flags = flags;
    for (uint32_t i = 0; i < n_sizes; i++) D.n_bits[i] = h_n_bits[i];
    D.max_cce = max_cce; D.max_waves = search_n_cand(max_cce) * n_sizes; D.unit_stride = 72 * max_cce;
    D.cells = (const uint32_t *)d_cells; D.pcfich = (const uint32_t *)d_pcf; D.n_cce = (const uint32_t *)d_ncce; D.cce_re = (const uint32_t *)d_res;
    D.rm_map = (const uint16_t *)d_rm; D.rnti_bits = (const uint32_t *)d_bits;
    pl->d_rnti_bits = (uint32_t *)d_bits;
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}

int mi_lte_pdcch_search_plan_set_rntis(mi_lte_ctx *ctx, mi_lte_pdcch_search_plan *pl, const uint32_t *h_rnti, uint32_t n_rnti)
{
    if (!ctx || !pl || (n_rnti && !h_rnti)) return MI_LTE_ERR_INVALID_ARG;
    std::vector<uint32_t> bits(2048, 0);
    for (uint32_t i = 0; i < n_rnti; i++) {
        if (h_rnti[i] == 0 || h_rnti[i] > 0xFFFFu) return MI_LTE_ERR_INVALID_ARG; // (the set stays as it was)
        bits[h_rnti[i] >> 5] |= 1u << (h_rnti[i] & 31u);
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    MI_H2D(ctx, pl->d_rnti_bits, bits.data(), bits.size() * 4); // (behind whatever run is still queued on the stream)
    return MI_LTE_OK;
}

static void search_free_run_buffers(mi_lte_pdcch_search_plan *pl)
{
    for (void *p : {(void *)pl->d_soft, (void *)pl->d_units, (void *)pl->d_hit, (void *)pl->d_rec, (void *)pl->d_out})
        if (p) (void)hipFree(p);
    pl->d_soft = nullptr; pl->d_units = nullptr; pl->d_hit = nullptr; pl->d_rec = nullptr; pl->d_out = nullptr;
    pl->cap_units = 0;
}

void mi_lte_pdcch_search_plan_destroy(mi_lte_ctx *ctx, mi_lte_pdcch_search_plan *pl)
{
    if (!pl) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    search_free_run_buffers(pl);
    for (void *p : pl->owned) (void)hipFree(p);
    delete pl;
}

int mi_lte_pdcch_search_run(mi_lte_ctx *ctx, mi_lte_pdcch_search_plan *pl, const float *d_subframes, const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell,
                            uint32_t n_units, uint32_t *h_cfi, uint32_t *h_n_cce, uint32_t *h_n_found, mi_lte_pdcch_found *h_found)
{
    if (!ctx || !pl || !d_subframes || !d_subfr_num || !d_n_id_cell || n_units == 0 || !h_cfi || !h_n_cce || !h_n_found || !h_found) return MI_LTE_ERR_INVALID_ARG;
    const PdcchSearchDev &D = pl->dev;
    const uint32_t blocks_per_unit = (D.max_waves + SEARCH_WAVES - 1) / SEARCH_WAVES;
    if ((uint64_t)n_units * std::max(blocks_per_unit, 1u) > 0x7FFFFFFFull) {
        ctx->err = "PDCCH search: too many units for one launch";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = mi_ctx_gold_tables(ctx);
    if (rc != MI_LTE_OK) return rc;
    if (n_units > pl->cap_units) { // the plan's own buffers grow to the largest batch seen; a run at that size or below allocates nothing
        MI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        search_free_run_buffers(pl);
        pl->ran = false;
        const size_t nu = n_units, nw = std::max(D.max_waves, 1u);
        if (hipMalloc((void **)&pl->d_soft, std::max<size_t>(nu * D.unit_stride, 4)) != hipSuccess || hipMalloc((void **)&pl->d_units, nu * sizeof(SearchUnit)) != hipSuccess ||
            hipMalloc((void **)&pl->d_hit, nu * nw * sizeof(uint16_t)) != hipSuccess || hipMalloc((void **)&pl->d_rec, nu * nw * sizeof(SearchHit)) != hipSuccess ||
            hipMalloc((void **)&pl->d_out, nu * sizeof(SearchOut)) != hipSuccess) {
            search_free_run_buffers(pl);
            ctx->err = "PDCCH search: device allocation failed";
            return MI_LTE_ERR_NOMEM;
        }
        pl->cap_units = n_units;
        pl->h_out.resize(n_units);
    }
    GoldTables gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
    MI_LAUNCH(ctx, "k_pdcch_search_demod", k_pdcch_search_demod, dim3(n_units), dim3(256), 0, d_subframes, (uint32_t)mi_lte_subframe_floats(pl->cfg.N_ant), d_subfr_num,
              d_n_id_cell, D, gt, pl->d_units, pl->d_soft);
    MI_HIP_CHECK(ctx, hipGetLastError());
    if (blocks_per_unit) {
        MI_LAUNCH(ctx, "k_pdcch_search_decode", k_pdcch_search_decode, dim3(n_units * blocks_per_unit), dim3(64 * SEARCH_WAVES), 0, pl->d_soft, pl->d_units, d_subfr_num, D,
                  blocks_per_unit, pl->d_hit, pl->d_rec);
        MI_HIP_CHECK(ctx, hipGetLastError());
    }
    MI_LAUNCH(ctx, "k_pdcch_search_compact", k_pdcch_search_compact, dim3(n_units), dim3(64), 0, pl->d_units, D, pl->d_hit, pl->d_rec, pl->d_out);
    MI_HIP_CHECK(ctx, hipGetLastError());
    pl->ran = true;
    MI_D2H(ctx, pl->h_out.data(), pl->d_out, sizeof(SearchOut) * (size_t)n_units); // the run's one wait
    for (uint32_t u = 0; u < n_units; u++) {
        const SearchOut &o = pl->h_out[u];
        h_cfi[u] = o.cfi; h_n_cce[u] = o.n_cce; h_n_found[u] = o.n_found;
        memcpy(h_found + (size_t)u * MI_LTE_PDCCH_SEARCH_MAX_FOUND, o.found, sizeof(o.found));
    }
    ctx->last_kernels = "k_pdcch_search_demod:1,k_pdcch_search_decode:1,k_pdcch_search_compact:1";
    return MI_LTE_OK;
}

int mi_lte_pdcch_search_soft(const mi_lte_pdcch_search_plan *pl, const int8_t **d_soft, uint32_t *unit_stride)
{
    if (!pl || !d_soft || !unit_stride || !pl->ran) return MI_LTE_ERR_INVALID_ARG;
    *d_soft = pl->d_soft;
    *unit_stride = pl->dev.unit_stride;
    return MI_LTE_OK;
}

} // extern "C"

