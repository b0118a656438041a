// PUCCH formats 2 / 2a / 2b on the device: periodic CQI reports, with a simultaneous HARQ-ACK on the second reference symbol (36.211 5.4.2,
// 5.4.3, 5.5.2.2; 36.212 5.2.3.3).  The reference declares liblte_phy_pucch_format_2_2a_2b_channel_decode and leaves it empty, so the
// definition in mi_lte.h is the contract; tests/test_pucch2_gpu.py holds a float64 model written from that text.
//
//   k_pucch2_decode  one wavefront per resource:
//     1. correlations: lane 4 L + q sums sub-carriers 3 q .. 3 q + 2 of symbol L against conj(r[L]), two butterflies add the four parts;
//        c[14] goes through LDS to every lane.  Correlating over the whole block is what separates the cyclic shifts.
//     2. D, the ACK decision, z, the two slot estimates, P and g: the same scalars on every lane.
//     3. lane n < 10 forms d(n)'s two soft bits; e[20] goes through LDS to every lane.
//     4. the exhaustive search of k_ulsch_cqi_decode's block code on 20-bit words: a lane owns a_0 .. a_5 and meets the up to 128 cosets
//        of a_6 .. a_12; ties go to the smallest w (the key (metric, -w) is one int32: |metric| <= 20 * 127, w < 8192).
//        A <= 9: the cosets one by one, 20 terms each.  A >= 10 (the WIDE kernel, launched when a call holds such a resource): with the
//        lane's signs folded into e, the metrics of all 128 cosets are the Walsh-Hadamard transform of the 128-entry vector that holds
//        e_i at index (M_i,6 .. M_i,12) -- 7 * 64 butterflies in registers instead of 128 * 20 terms (tools/pucch2_timing.py: the
//        one-by-one search was 94 % of an A = 13 kernel).  Integers throughout: the decision is exact whatever the order of the sums.
//     5. lane 0 writes the 64-byte record.
// The descriptors and tables are the host's and are checked there before any launch; the kernel trusts them.
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "pucch2_code.h"

namespace {

constexpr uint32_t GRID_SC = 1200; // row stride of the UL subframe layout (rx_symb_re[16][1200] rx_symb_im[16][1200])
static_assert(sizeof(mi_lte_pucch2_result) == 64 && sizeof(mi_lte_pucch2_res) == 16 && sizeof(mi_lte_pucch2_tab) == 4 * (2 * 14 * 12 + 3), "mi_lte.h layouts");

__device__ __forceinline__ int32_t soft_q(float x) { return (int32_t)fminf(fmaxf(rintf(x), -127.0f), 127.0f); }

// position i's coset signature: bit j = M_{i, 6 + j}, what a_(6 + j) adds to b_i
__host__ __device__ constexpr uint32_t coset_sig(uint32_t i)
{
    uint32_t g = 0;
    for (uint32_t j = 0; j + 6 < MI_PUCCH2_MAX_BITS; j++) g |= ((MI_PUCCH2_COL(j + 6) >> i) & 1u) << j;
    return g;
}
constexpr uint32_t FHT_MIN_BITS = 10; // from 16 cosets on the transform is the cheaper search

template <bool WIDE>
__global__ __launch_bounds__(64) void k_pucch2_decode(const float *__restrict__ subframes, uint32_t sf_stride, const mi_lte_pucch2_res *__restrict__ res,
                                                      const mi_lte_pucch2_tab *__restrict__ tabs, mi_lte_pucch2_result *__restrict__ out)
{
    __shared__ float   s_c_re[14], s_c_im[14];
    __shared__ int32_t s_e[MI_PUCCH2_CODED];
    const uint32_t           ln = threadIdx.x;
    const mi_lte_pucch2_res  pr = res[blockIdx.x]; // (uniform: scalar loads)
    const mi_lte_pucch2_tab *tb = tabs + pr.tab;
    const float             *y_re = subframes + (size_t)pr.unit * sf_stride, *y_im = y_re + 16 * GRID_SC;
    // 1. c[L] = sum_k y(L, 12 prb + k) conj(r[L][k])
    {
        const uint32_t L = ln >> 2, q = ln & 3u;
        float          a_re = 0, a_im = 0;
        if (L < 14) {
            const uint32_t at = L * GRID_SC + 12 * tb->prb[L >= 7 ? 1 : 0] + 3 * q;
#pragma unroll
            for (uint32_t j = 0; j < 3; j++) {
                const float yr = y_re[at + j], yi = y_im[at + j], rr = tb->r_re[L][3 * q + j], ri = tb->r_im[L][3 * q + j];
                a_re += yr * rr + yi * ri;
                a_im += yi * rr - yr * ri;
            }
        }
        a_re += __shfl_xor(a_re, 1, 64); a_im += __shfl_xor(a_im, 1, 64);
        a_re += __shfl_xor(a_re, 2, 64); a_im += __shfl_xor(a_im, 2, 64);
        if (L < 14 && q == 0) { s_c_re[L] = a_re; s_c_im[L] = a_im; }
    }
    __syncthreads();
    // 2. D = sum_s c[7s+5] conj(c[7s+1]); the ACK symbol z; h_s = (c[7s+1] + conj(z) c[7s+5]) / 24
    float D_re = 0, D_im = 0;
#pragma unroll
    for (uint32_t s = 0; s < 2; s++) {
        const float ar = s_c_re[7 * s + 5], ai = s_c_im[7 * s + 5], br = s_c_re[7 * s + 1], bi = s_c_im[7 * s + 1];
        D_re += ar * br + ai * bi;
        D_im += ai * br - ar * bi;
    }
    uint32_t ack0 = 0, ack1 = 0, n_ack = 0;
    float    z_re = 1, z_im = 0;
    if (pr.format == 1) {
        n_ack = 1;
        if (D_re < 0) { ack0 = 1; z_re = -1; }
    } else if (pr.format == 2) {
        n_ack = 2;
        float best = D_re;                                                            // 00: z = 1
        if (-D_im > best) { best = -D_im; ack0 = 0; ack1 = 1; z_re = 0; z_im = -1; } // 01: z = -j
        if (D_im > best) { best = D_im; ack0 = 1; ack1 = 0; z_re = 0; z_im = 1; }    // 10: z = j
        if (-D_re > best) { ack0 = 1; ack1 = 1; z_re = -1; z_im = 0; }               // 11: z = -1
    }
    float h_re[2], h_im[2];
#pragma unroll
    for (uint32_t s = 0; s < 2; s++) { // conj(z) c = (z_re c_re + z_im c_im) + j (z_re c_im - z_im c_re)
        const float cr = s_c_re[7 * s + 5], ci = s_c_im[7 * s + 5];
        h_re[s] = (s_c_re[7 * s + 1] + (z_re * cr + z_im * ci)) / 24.0f;
        h_im[s] = (s_c_im[7 * s + 1] + (z_re * ci - z_im * cr)) / 24.0f;
    }
    const float P = ((h_re[0] * h_re[0] + h_im[0] * h_im[0]) + (h_re[1] * h_re[1] + h_im[1] * h_im[1])) / 2.0f;
    const float g = 32.0f * 1.41421356237309505f / P;
    const bool  live = P > 0 && isfinite(P) && isfinite(g);
    // 3. v_n = (c[L_n] / 12) conj(h_s): lane n < 10 owns d(n), i.e. e(2n) and e(2n+1)
    if (ln < 10) {
        const uint32_t s = ln >= 5 ? 1u : 0u, i = ln - 5 * s, L = 7 * s + (i == 0 ? 0u : i == 4 ? 6u : i + 1);
        const float    cr = s_c_re[L] / 12.0f, ci = s_c_im[L] / 12.0f, hr = s ? h_re[1] : h_re[0], hi = s ? h_im[1] : h_im[0];
        const float    v_re = cr * hr + ci * hi, v_im = ci * hr - cr * hi;
        int32_t        e0 = live ? soft_q(g * v_re) : 0, e1 = live ? soft_q(g * v_im) : 0;
        if ((tb->c_scr >> (2 * ln)) & 1u) e0 = -e0;
        if ((tb->c_scr >> (2 * ln + 1)) & 1u) e1 = -e1;
        s_e[2 * ln] = e0; s_e[2 * ln + 1] = e1;
    }
    __syncthreads();
    // 4. the maximum of sum_i (1 - 2 b_i(w)) e_i over all 2^A words
    int32_t e[MI_PUCCH2_CODED], total = 0, energy = 0;
#pragma unroll
    for (uint32_t i = 0; i < MI_PUCCH2_CODED; i++) {
        e[i] = s_e[i]; // (the same address on every lane: a broadcast)
        total += e[i];
        energy += abs(e[i]);
    }
    const uint32_t n_words = 1u << pr.A, lane_word = mi_pucch2_word(ln);
    int32_t        key = INT32_MIN; // metric * 8192 + (8191 - w): the larger metric, then the smaller w
    if (WIDE && pr.A >= FHT_MIN_BITS) {
        int32_t F[128];
#pragma unroll
        for (uint32_t c = 0; c < 128; c++) F[c] = 0;
#pragma unroll
        for (uint32_t i = 0; i < MI_PUCCH2_CODED; i++) F[coset_sig(i)] += ((lane_word >> i) & 1u) ? -e[i] : e[i];
#pragma unroll
        for (uint32_t h = 1; h < 128; h <<= 1)
#pragma unroll
            for (uint32_t b = 0; b < 128; b += 2 * h)
#pragma unroll
                for (uint32_t k = b; k < b + h; k++) {
                    const int32_t x = F[k], y = F[k + h];
                    F[k] = x + y; F[k + h] = x - y;
                }
        // F[c] = sum_i (-1)^(c . sig_i) (+-e_i): the metric of w = 64 c + ln; 2^(A-6) cosets count, a multiple of 16 here
        const int32_t low = 8191 - (int32_t)ln;
#pragma unroll
        for (uint32_t blk = 0; blk < 128; blk += 16) {
            if (64 * blk < n_words) { // (uniform)
#pragma unroll
                for (uint32_t c = blk; c < blk + 16; c++) key = max(key, F[c] * 8192 + (low - 64 * (int32_t)c));
            }
        }
    } else {
        int32_t  best = INT32_MIN;
        uint32_t arg  = 0;
        for (uint32_t c = 0; c < n_words; c += 64) { // (uniform; ascending, strict >: the first maximum of the lane)
            const uint32_t w = c | ln, b = lane_word ^ mi_pucch2_word(c);
            int32_t        neg = 0; // the e_i of the word's ones: sum (1 - 2 b_i) e_i = total - 2 neg
#pragma unroll
            for (uint32_t i = 0; i < MI_PUCCH2_CODED; i++) neg += ((b >> i) & 1u) ? e[i] : 0;
            const int32_t m = total - 2 * neg;
            if (w < n_words && m > best) { best = m; arg = w; }
        }
        if (best != INT32_MIN) key = best * 8192 + (8191 - (int32_t)arg);
    }
    for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
    const int32_t  best = key >> 13; // (arithmetic: the floor, whatever the sign)
    const uint32_t arg  = 8191u - ((uint32_t)key & 8191u);
    // 5. the record
    if (ln == 0) {
        mi_lte_pucch2_result r;
        r.A = pr.A; r.bits = arg; r.metric = best; r.energy = energy;
        r.ack[0] = (uint8_t)ack0; r.ack[1] = (uint8_t)ack1; r.n_ack = (uint8_t)n_ack; r.pad0 = 0;
        r.D_re = D_re; r.D_im = D_im; r.P = P;
#pragma unroll
        for (uint32_t i = 0; i < MI_PUCCH2_CODED; i++) r.e[i] = (int8_t)e[i];
#pragma unroll
        for (uint32_t i = 0; i < 12; i++) r.pad[i] = 0;
        out[blockIdx.x] = r;
    }
}

} // namespace

extern "C" int mi_lte_pucch2_decode_run(mi_lte_ctx *ctx, uint32_t N_rb_ul, const float *d_subframes, uint32_t n_units, const mi_lte_pucch2_res *h_res,
                                        uint32_t n_res, const mi_lte_pucch2_tab *h_tabs, uint32_t n_tab, mi_lte_pucch2_result *d_out)
{
    if (!ctx || !d_subframes || !h_res || !h_tabs || !d_out || n_res == 0 || n_tab == 0 || N_rb_ul < 6 || N_rb_ul > GRID_SC / 12) return MI_LTE_ERR_INVALID_ARG;
    for (uint32_t t = 0; t < n_tab; t++)
        if (h_tabs[t].prb[0] >= N_rb_ul || h_tabs[t].prb[1] >= N_rb_ul) return MI_LTE_ERR_INVALID_ARG;
    bool wide = false; // a resource of A >= FHT_MIN_BITS: the kernel with the transform search (and its registers)
    for (uint32_t r = 0; r < n_res; r++) {
        if (h_res[r].format > 2 || h_res[r].A == 0 || h_res[r].A > MI_PUCCH2_MAX_BITS || h_res[r].unit >= n_units || h_res[r].tab >= n_tab) return MI_LTE_ERR_INVALID_ARG;
        wide |= h_res[r].A >= FHT_MIN_BITS;
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    // descriptors | tables, one block of scratch filled by one copy; the kernel is queued behind it and the call returns
    const size_t b_res = sizeof(mi_lte_pucch2_res) * (size_t)n_res, o_tab = (b_res + 255) & ~(size_t)255, total = o_tab + sizeof(mi_lte_pucch2_tab) * (size_t)n_tab;
    const int    rc = mi_ctx_reserve_scratch(ctx, total);
    if (rc != MI_LTE_OK) return rc;
    std::vector<char> stage(total, 0);
    memcpy(stage.data(), h_res, b_res);
    memcpy(stage.data() + o_tab, h_tabs, total - o_tab);
    char *base = (char *)ctx->scratch;
    MI_H2D(ctx, base, stage.data(), total);
    if (wide)
        MI_LAUNCH(ctx, "k_pucch2_decode", k_pucch2_decode<true>, dim3(n_res), dim3(64), 0, d_subframes, (uint32_t)mi_lte_ul_subframe_floats(),
                  (const mi_lte_pucch2_res *)base, (const mi_lte_pucch2_tab *)(base + o_tab), d_out);
    else
        MI_LAUNCH(ctx, "k_pucch2_decode", k_pucch2_decode<false>, dim3(n_res), dim3(64), 0, d_subframes, (uint32_t)mi_lte_ul_subframe_floats(),
                  (const mi_lte_pucch2_res *)base, (const mi_lte_pucch2_tab *)(base + o_tab), d_out);
    MI_HIP_CHECK(ctx, hipGetLastError());
    ctx->last_kernels = "k_pucch2_decode:1";
    return MI_LTE_OK;
}
