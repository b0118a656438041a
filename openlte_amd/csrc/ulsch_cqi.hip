// CQI channel coding on PUSCH (36.212 5.2.2.6.4), both directions.  O <= 11 information bits: the (32, O) block code of table 5.2.2.6.4-1
// (cqi_code.h), repeated to Q_cqi bits.  O > 11: CRC8, the tail-biting convolutional code (5.1.3.1) and its rate matching (5.1.4.2).
// A positive soft bit means bit 0, as everywhere in the 3GPP mode.
//
//   mi_lte_cqi_encode   the transmitter, host code over tx.cc's conv_encode_tb / rate_match_conv.
//   k_ulsch_cqi_decode  one wavefront per CQI run, integer work throughout (exact, order-free sums):
//     1. combine: repeats add up in int32.  Block code: r_i = sum of e_k over k = i mod 32.  Convolutional code: transmitted bit k is the
//        (k mod 3L)-th non-dummy entry of the circular buffer, whose place in d[3L] comes from a rank over the L non-dummy entries of one
//        sub-block (ballot prefix); positions never sent stay 0 and an erased (0) soft bit adds nothing.
//        Q_cqi <= 95 040 soft bits of magnitude <= 127: sum |r| and sum |d| <= 1.21e7, a path metric over three laps <= 3.63e7 < 2^31.
//     2a. block code: every one of the 2^O words is correlated with r.  A lane owns o_0 .. o_5, the wavefront walks the up to 32 cosets
//        of o_6 .. o_10 in ascending order; ties go to the smallest w = sum o_n 2^n (strict > inside a lane, (metric, -w) across lanes).
//     2b. convolutional code (tbcc_dev.h, the copy k_pdcch_search_decode runs too): maximum-correlation Viterbi over three laps of the L-step ring, one of the 64 states (c_k-1 .. c_k-6),
//        newest bit on top) per lane, all metrics starting at 0.  Lane n's predecessors are 2 (n & 31) and 2 (n & 31) + 1; the odd one
//        survives only when strictly larger; one ballot of survivors per step goes to LDS.  End state: the first maximum in state order.
//        Lane 0 traces back all 3L steps and keeps the middle lap's bits, then CRC8 is checked over them.
//     3. one 32-byte record per run (mi_lte_cqi_result).  A descriptor that cannot be served yields the all-zero record.
// The run is read byte by byte: it starts at any even offset (inside a plan it lies behind G, a multiple of Q_m only), and lanes read
// consecutive bytes, so the loads coalesce without an alignment path.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "cqi_code.h"
#include "tbcc_dev.h"
#include "tx_host.h"
#include "ulsch_uci.h"

namespace {

constexpr uint32_t L_MAX = MI_LTE_CQI_MAX_BITS + 8; // information bits and CRC8
constexpr uint32_t CRC8_POLY = 0x19Bu;              // gCRC8 = D^8 + D^7 + D^4 + D^3 + D + 1

__device__ __forceinline__ uint32_t bitrev5(uint32_t j) { return ((j & 1) << 4) | ((j & 2) << 2) | (j & 4) | ((j & 8) >> 2) | ((j & 16) >> 4); }

// the sum of e_k over k = n mod period, k < Q
__device__ __forceinline__ int32_t combine(const int8_t *__restrict__ e, uint32_t Q, uint32_t n, uint32_t period)
{
    int32_t s = 0;
    for (uint32_t k = n; k < Q; k += period) s += e[k];
    return s;
}

__device__ __forceinline__ void block_decode(const int8_t *__restrict__ e, uint32_t Q, uint32_t O, int32_t *d, uint32_t ln, mi_lte_cqi_result &res)
{
    d[ln] = combine(e, Q, ln, 64); // (64 = 2 * 32: lanes i and i + 32 hold the two halves of r_i)
    __syncthreads();
    int32_t r[32], total = 0, energy = 0;
#pragma unroll
    for (uint32_t i = 0; i < 32; i++) {
        r[i] = d[i] + d[i + 32]; // (the same address on every lane: a broadcast)
        total += r[i];
        energy += abs(r[i]);
    }
    const uint32_t n_words = 1u << O, lane_word = mi_cqi_block_word(ln);
    int32_t        best = INT32_MIN;
    uint32_t       arg  = 0xFFFFFFFFu;
    for (uint32_t c = 0; c < n_words; c += 64) { // (uniform)
        const uint32_t w = c | ln, b = lane_word ^ mi_cqi_block_word(c);
        int32_t        neg = 0; // the r_i of the word's ones: sum (1 - 2 b_i) r_i = total - 2 neg
#pragma unroll
        for (uint32_t i = 0; i < 32; i++) neg += ((b >> i) & 1u) ? r[i] : 0;
        const int32_t m = total - 2 * neg;
        if (w < n_words && m > best) { best = m; arg = w; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t  ob = __shfl_xor(best, o, 64);
        const uint32_t oa = __shfl_xor(arg, o, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    res.O = O; res.crc = MI_LTE_CQI_NO_CRC; res.metric = best; res.energy = energy;
    res.bits[0] = arg;
}

__device__ __forceinline__ void conv_decode(const int8_t *__restrict__ e, uint32_t Q, uint32_t O, int32_t *d, uint64_t *surv, uint16_t *pos, uint8_t *cb,
                                            uint32_t ln, mi_lte_cqi_result &res)
{
    const uint32_t L = O + 8, R = (L + 31) / 32, K_pi = 32 * R, N_dummy = K_pi - L, P = 3 * L;
    // 1. the sub-block interleaver's non-dummy entries in reading order: entry kk holds element 32 (kk mod R) + perm(kk / R) of the padded stream
    for (uint32_t k0 = 0, base = 0; k0 < K_pi; k0 += 64) { // (uniform; K_pi <= 160)
        const uint32_t kk = k0 + ln, col = kk / R, t = 32 * (kk - col * R) + bitrev5((col + 16) & 31u);
        const bool     sent = kk < K_pi && t >= N_dummy;
        const uint64_t m = __ballot(sent);
        if (sent) pos[base + (uint32_t)__popcll(m & ((1ull << ln) - 1))] = (uint16_t)(t - N_dummy);
        base += (uint32_t)__popcll(m);
    }
    __syncthreads();
    int32_t energy = 0;
    for (uint32_t n = ln; n < P; n += 64) { // circular-buffer entry n: sub-block x = n / L, its r-th non-dummy entry
        const int32_t  s = combine(e, Q, n, P);
        const uint32_t x = n >= 2 * L ? 2u : n >= L ? 1u : 0u, r = n - x * L;
        d[3 * pos[r] + x] = s;
        energy += abs(s);
    }
    energy = wave_sum(energy);
    __syncthreads();
    // 2. the shared decoder (tbcc_dev.h): three laps, traceback, the decided bits re-encoded against d
    int32_t metric;
    tbcc_decode(d, L, surv, cb, ln, [] { __syncthreads(); }, metric);
    // 3. CRC8 over the decided bits, the information bits packed
    uint32_t rem = 0, par = 0;
    if (ln == 0) {
        for (uint32_t i = 0; i < L; i++) {
            rem = (rem << 1) | (i < O ? cb[i] : 0u);
            if (rem & 0x100u) rem ^= CRC8_POLY;
            if (i >= O) par = (par << 1) | cb[i];
        }
    }
    res.O = O; res.crc = rem == par ? MI_LTE_CQI_CRC_OK : MI_LTE_CQI_CRC_FAIL; res.metric = metric; res.energy = energy;
#pragma unroll
    for (uint32_t j = 0; j < 2; j++) {
        const uint32_t n = 64 * j + ln;
        const uint64_t m = __ballot(n < O && cb[n] != 0);
        res.bits[2 * j] = (uint32_t)m; res.bits[2 * j + 1] = (uint32_t)(m >> 32);
    }
}

__global__ __launch_bounds__(64) void k_ulsch_cqi_decode(const int8_t *__restrict__ soft, const mi_lte_cqi_desc *__restrict__ desc, mi_lte_cqi_result *__restrict__ out)
{
    __shared__ int32_t  d[3 * L_MAX];
    __shared__ uint64_t surv[3 * L_MAX];
    __shared__ uint16_t pos[L_MAX];
    __shared__ uint8_t  cb[L_MAX];
    const uint32_t        ln = threadIdx.x;
    const mi_lte_cqi_desc ds = desc[blockIdx.x]; // (uniform: scalar loads)
    mi_lte_cqi_result     res;
    res.O = 0; res.crc = MI_LTE_CQI_NONE; res.metric = 0; res.energy = 0;
    res.bits[0] = res.bits[1] = res.bits[2] = res.bits[3] = 0;
    // the descriptors live on the device: the kernel is their only check, and what it cannot serve it does not read
    if (ds.O >= 1 && ds.O <= MI_LTE_CQI_MAX_BITS && ds.Q_cqi >= 1 && ds.Q_cqi <= MI_CQI_MAX_Q && !(ds.off & 1u)) {
        const int8_t *e = soft + ds.off;
        if (ds.O <= MI_CQI_BLOCK_MAX_BITS) block_decode(e, ds.Q_cqi, ds.O, d, ln, res);
        else conv_decode(e, ds.Q_cqi, ds.O, d, surv, pos, cb, ln, res);
    }
    if (ln == 0) out[blockIdx.x] = res;
}

int cqi_launch(mi_lte_ctx *ctx, const int8_t *d_soft, const mi_lte_cqi_desc *d_desc, uint32_t n, mi_lte_cqi_result *d_out)
{
    MI_LAUNCH(ctx, "k_ulsch_cqi_decode", k_ulsch_cqi_decode, dim3(n), dim3(64), 0, d_soft, d_desc, d_out);
    MI_HIP_CHECK(ctx, hipGetLastError());
    return MI_LTE_OK;
}

} // namespace

// ------------------------------------------------------------------------------------------------
// a plan's part (ulsch_uci.h): the setter's checks, and the launch behind k_ulsch_uci_decide

int mi_ulsch_cqi_set(MiUlschUci *u, const uint32_t *h_e_off, size_t e_bytes, const uint32_t *h_O)
{
    if (!h_O) { u->cqi_on = false; return MI_LTE_OK; }
    if (e_bytes > 0xFFFFFFFFull) return MI_LTE_ERR_UNSUPPORTED; // (a descriptor's offset is 32 bits of bytes)
    for (uint32_t a = 0; a < u->n_alloc; a++)
        if (h_O[a] > MI_LTE_CQI_MAX_BITS || (h_O[a] > 0 && u->h_Q_cqi[a] == 0)) return MI_LTE_ERR_INVALID_ARG;
    u->h_cqi_desc.resize(u->n_alloc);
    for (uint32_t a = 0; a < u->n_alloc; a++) // the CQI soft bits lie behind the allocation's G data soft bits (k_ulsch_uci_gather)
        u->h_cqi_desc[a] = {h_e_off[a] * 64u + u->h_G[a], u->h_Q_cqi[a], h_O[a], 0u};
    u->cqi_on = u->cqi_dirty = true;
    return MI_LTE_OK;
}

int mi_ulsch_cqi_run(mi_lte_ctx *ctx, MiUlschUci *u)
{
    if (u->cqi_dirty) { // (the setter has no context to copy with)
        MI_H2D(ctx, u->d_cqi_desc, u->h_cqi_desc.data(), sizeof(mi_lte_cqi_desc) * u->n_alloc);
        u->cqi_dirty = false;
    }
    return cqi_launch(ctx, u->d_e, u->d_cqi_desc, u->n_alloc, u->d_cqi_res);
}

extern "C" {

int mi_lte_cqi_encode(uint32_t O, const uint8_t *o_bits, uint32_t Q_cqi, uint8_t *q_bits)
{
    if (!o_bits || !q_bits || O == 0 || O > MI_LTE_CQI_MAX_BITS || Q_cqi == 0 || Q_cqi > MI_CQI_MAX_Q) return MI_LTE_ERR_INVALID_ARG;
    if (O <= MI_CQI_BLOCK_MAX_BITS) {
        uint32_t w = 0;
        for (uint32_t n = 0; n < O; n++) w |= (uint32_t)(o_bits[n] & 1u) << n;
        const uint32_t b = mi_cqi_block_word(w);
        for (uint32_t i = 0; i < Q_cqi; i++) q_bits[i] = (uint8_t)((b >> (i & 31u)) & 1u);
        return MI_LTE_OK;
    }
    const uint32_t L = O + 8;
    uint8_t        c[L_MAX], d[3 * L_MAX];
    for (uint32_t n = 0; n < O; n++) c[n] = o_bits[n] & 1u;
    tx::crc_bits(c, O, CRC8_POLY, 8, c + O);
    tx::conv_encode_tb(c, L, d);
    tx::rate_match_conv(d, 3 * L, Q_cqi, q_bits);
    return MI_LTE_OK;
}

int mi_lte_cqi_decode_batch(mi_lte_ctx *ctx, const int8_t *d_soft, const mi_lte_cqi_desc *d_desc, uint32_t n, mi_lte_cqi_result *d_out)
{
    if (!ctx || !d_soft || !d_desc || !d_out || n == 0 || ((uintptr_t)d_soft & 1u)) return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int rc = cqi_launch(ctx, d_soft, d_desc, n, d_out);
    if (rc == MI_LTE_OK) ctx->last_kernels = "k_ulsch_cqi_decode:1";
    return rc;
}

} // extern "C"
