// CRS noise estimate of a downlink subframe on gfx950 (include/mi_lte.h, "DL: CRS noise estimate"): one float sigma2 per unit from the second
// differences of the least-squares products at the CRS of ports 0 and 1.  It reads only the received-symbol planes of a unit, so it serves
// full and MI_LTE_CE_COMPACT planes alike; the 3GPP PDSCH plans run it in front of their max-log demapper for the noise-referenced gain
// (mi_lte_pdsch_plan_set_llr_noise, chain.hip).
//
//   k_dl_crs_noise : one workgroup per unit.  The Gold words of the four CRS symbols 0, 4, 7, 11 go to LDS as k_dl_ce forms them (frontend.hip);
//                    every thread forms least-squares products t = y conj(crs) of rows (port, symbol) into LDS; one barrier; every thread
//                    sums |t[j-1] - 2 t[j] + t[j+1]|^2 of its own interior pilots in double; xor butterfly inside the wavefront, the four
//                    wavefronts' slots in ascending order, one store.  No atomics: two runs give identical bytes.
#include "ctx.hpp"
#include "phy_dev.hpp"

namespace {

constexpr int      N_SC_MAX   = 1200; // row stride of every subframe array
constexpr uint32_t NOISE_ROWS = 8;    // ports 0 and 1 x symbols 0, 4, 7, 11
constexpr uint32_t Q_SHIFT    = 22;   // t / n_pil as (t * q_pil) >> 22, q_pil = ceil(2^22 / n_pil): exact for t < 1600, n_pil <= 200 (t (q_pil n_pil - 2^22) < 2^22)

__global__ __launch_bounds__(256) void k_dl_crs_noise(const float *__restrict__ subframes, uint32_t sf_stride, uint32_t N_rb_dl, uint32_t n_rows,
                                                      uint32_t q_pil, const uint32_t *__restrict__ subfr_num, const uint32_t *__restrict__ n_id_cell,
                                                      GoldTables gt, float *__restrict__ sigma2)
{
    extern __shared__ __attribute__((aligned(16))) float2 t_ls[]; // [n_rows][n_pil]: row = 4 p + i
    __shared__ uint32_t crs_bits[4][14];                          // the CRS sequence does not depend on the port
    __shared__ double   s_wave[4];
    const uint32_t unit = blockIdx.x, n_pil = 2 * N_rb_dl, n_items = n_rows * n_pil;
    const uint32_t sf = subfr_num[unit], cell = n_id_cell[unit], v_shift = cell % 6;
    const float   *sym_re = subframes + (size_t)unit * sf_stride, *sym_im = sym_re + 16 * N_SC_MAX;
    auto sym_of = [](uint32_t i) -> uint32_t { return i == 0 ? 0u : i == 1 ? 4u : i == 2 ? 7u : 11u; };

    // CRS bits (k_dl_ce's: generate_crs, liblte_phy.cc:8300-8333; slots per :5960-5967)
    if (threadIdx.x < 4 * 14) {
        const uint32_t i = threadIdx.x / 14, w = threadIdx.x - 14 * i;
        const uint32_t sy = sym_of(i), slot = sy >= 7 ? 1u : 0u, l = sy - 7 * slot;
        const uint32_t ns2 = (sf * 2) % 20 + slot, ns = ns2 >= 20 ? ns2 - 20 : ns2;
        const uint32_t c_init = ((__umul24(7 * (ns + 1) + l + 1, 2 * cell + 1) << 10) + 2 * cell + 1) & 0x7FFFFFFFu; // 31 bits: the Gold basis has 31 rows
        crs_bits[i][w] = gold_word(gt, c_init, w);
    }
    __syncthreads();

    // least-squares product at every pilot of every row: the other ports are silent there, so t = h_p + noise
    const float r2 = (float)(1.0 / sqrt(2.0));
    for (uint32_t t = threadIdx.x; t < n_items; t += blockDim.x) {
        const uint32_t row = (t * q_pil) >> Q_SHIFT, j = t - row * n_pil, p = row >> 2, i = row & 3u;
        const uint32_t voff = ((i ^ p) & 1u) ? 3u : 0u, vs = voff + v_shift;                 // k_dl_ce's voff_of for ports 0 and 1
        const uint32_t k = 6 * j + (vs >= 6 ? vs - 6 : vs), mp = j + 110 - N_rb_dl;          // k < 12 N_rb_dl
        const uint32_t b0 = (crs_bits[i][(2 * mp) >> 5] >> ((2 * mp) & 31)) & 1u, b1 = (crs_bits[i][(2 * mp + 1) >> 5] >> ((2 * mp + 1) & 31)) & 1u;
        const float rs_re = r2 * (1 - 2 * (float)b0), rs_im = r2 * (1 - 2 * (float)b1);
        const uint32_t o = __umul24(sym_of(i), (uint32_t)N_SC_MAX) + k;
        const float s_re = sym_re[o], s_im = sym_im[o];
        t_ls[t] = make_float2(s_re * rs_re + s_im * rs_im, s_im * rs_re - s_re * rs_im);
    }
    __syncthreads();

    // second differences along a row, in double: a channel that is linear over three pilots cancels, white noise leaves 6 sigma^2
    double part = 0.0;
    for (uint32_t t = threadIdx.x; t < n_items; t += blockDim.x) {
        const uint32_t row = (t * q_pil) >> Q_SHIFT, j = t - row * n_pil;
        if (j == 0 || j == n_pil - 1) continue; // (so t - 1 and t + 1 stay inside the row)
        const float2 a = t_ls[t - 1], b = t_ls[t], c = t_ls[t + 1];
        const double dr = (double)a.x - 2.0 * (double)b.x + (double)c.x, di = (double)a.y - 2.0 * (double)b.y + (double)c.y;
        part += dr * dr + di * di;
    }
    for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double S = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
        sigma2[unit] = (float)(S / (6.0 * (double)n_rows * (double)(n_pil - 2)));
    }
}

} // namespace

// The launch alone, for the entry point below and for the plans' noise-on runs (chain.hip): the arguments have been checked
int mi_dl_crs_noise(mi_lte_ctx *ctx, uint32_t N_rb_dl, uint32_t N_ant, const float *d_subframes, const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell,
                    uint32_t n_units, float *d_sigma2)
{
    if (!(N_rb_dl == 6 || N_rb_dl == 15 || N_rb_dl == 25 || N_rb_dl == 50 || N_rb_dl == 75 || N_rb_dl == 100)) return MI_LTE_ERR_INVALID_ARG;
    if (!(N_ant == 1 || N_ant == 2 || N_ant == 4)) return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int rc = mi_ctx_gold_tables(ctx);
    if (rc != MI_LTE_OK) return rc;
    GoldTables     gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
    const uint32_t n_rows = N_ant == 1 ? 4u : NOISE_ROWS, n_pil = 2 * N_rb_dl, q_pil = ((1u << Q_SHIFT) + n_pil - 1) / n_pil;
    MI_LAUNCH(ctx, "k_dl_crs_noise", k_dl_crs_noise, dim3(n_units), dim3(256), sizeof(float2) * n_rows * n_pil, d_subframes,
              (uint32_t)mi_lte_subframe_floats(N_ant), N_rb_dl, n_rows, q_pil, d_subfr_num, d_n_id_cell, gt, d_sigma2);
    MI_HIP_CHECK(ctx, hipGetLastError());
    return MI_LTE_OK;
}

extern "C" int mi_lte_dl_crs_noise_run(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const float *d_subframes, const uint32_t *d_subfr_num,
                                       const uint32_t *d_n_id_cell, uint32_t n_units, float *d_sigma2)
{
    if (!ctx || !cfg || !d_subframes || !d_subfr_num || !d_n_id_cell || !d_sigma2 || n_units == 0) return MI_LTE_ERR_INVALID_ARG;
    const int rc = mi_dl_crs_noise(ctx, cfg->N_rb_dl, cfg->N_ant, d_subframes, d_subfr_num, d_n_id_cell, n_units, d_sigma2);
    if (rc == MI_LTE_OK) ctx->last_kernels = "k_dl_crs_noise:1";
    return rc;
}
