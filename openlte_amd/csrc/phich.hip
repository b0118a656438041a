// PHICH on the device: the HARQ indicators an eNodeB answers a PUSCH with (36.211 6.9, 36.213 9.1.2), for cells of 1, 2 and 4 CRS ports.
// The reference only locates the PHICH (phich_channel_demap, liblte_phy.cc:8243-8278) and sends it (phich_channel_map :8076-8215); it has
// no decoder, so the definition in mi_lte.h ("PHICH, 3GPP mode") is the contract and tests/phich_model.py restates it in float64.
//
//   k_phich_decode<N_ant>  one workgroup per unit (device subframe):
//     1. item (group m, element e = 4 i + j) gathers y and the estimates of the two ports that carry quadruplet i -- port 0 alone; ports
//        (0, 1); ports (0, 2) when (i + m) is even and (1, 3) otherwise -- at its own resource element of symbol 0.  The elements of an
//        Alamouti pair are neighbouring lanes, so the partner's y and second-port estimate arrive by one lane exchange:
//            r = sqrt 2 (conj(hA_own) y_own +- hB_partner conj(y_partner)),  P = |hA_own|^2 + |hB_partner|^2   (+ on e even, - on e odd)
//        r descrambled with bit e of the cell's sequence, and P, go to LDS.
//     2. after one barrier item (m, n) despreads sequence n of group m: per quadruplet the sum over j in order, the projection onto
//        z0 = (1 + j) / sqrt 2 over P_tot (the twelve P in order), the three repetitions added in order, and writes the 32-byte record.
// Every sum has a fixed order and nothing is accumulated across threads: two runs give the same bytes.  The index table is the host's
// (phich_geom.cc) and is checked there; the kernel trusts it.
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "pdcch_geom.h"
#include "phich_geom.h"
#include "phy_dev.hpp"

using namespace phich_geom;

namespace {

constexpr uint32_t PHICH_THREADS = 256, PLANE = 16 * pdcch_geom::N_SC_MAX, NO_CELL = 0xFFFFFFFFu;
static_assert(sizeof(mi_lte_phich_result) == 32, "mi_lte.h layout");
static_assert(MAX_GROUP * N_SEQ <= PHICH_THREADS && PHICH_THREADS % 2 == 0, "one record per thread; Alamouti pairs in neighbouring lanes");

struct PhichDev {
    uint32_t        N_group, n_cells;
    const uint32_t *cells; // [n_cells] cell ids the table was built for
    const uint32_t *re;    // [n_cells][N_group][12] sub-carrier of RE(4 i + j) in symbol 0
};

template <uint32_t N_ant>
__global__ __launch_bounds__(PHICH_THREADS) void k_phich_decode(const float *__restrict__ subframes, uint32_t sf_stride, const uint32_t *__restrict__ subfr_num,
                                                                const uint32_t *__restrict__ n_id_cell, PhichDev P, GoldTables gt,
                                                                mi_lte_phich_result *__restrict__ out)
{
    __shared__ float    s_re[MAX_GROUP * N_RE], s_im[MAX_GROUP * N_RE], s_p[MAX_GROUP * N_RE];
    __shared__ uint32_t s_cell_idx;
    const uint32_t unit = blockIdx.x, tid = threadIdx.x;
    const uint32_t sf = subfr_num[unit], cell = n_id_cell[unit];
    const uint32_t n_items = P.N_group * N_RE, n_rec = P.N_group * N_SEQ;
    mi_lte_phich_result *res = out + (size_t)unit * n_rec;
    if (tid == 0) {
        uint32_t ci = NO_CELL;
        for (uint32_t k = 0; k < P.n_cells; k++)
            if (P.cells[k] == cell) { ci = k; break; }
        s_cell_idx = sf <= 9 ? ci : NO_CELL; // (a subframe number the scrambler has no meaning for)
    }
    __syncthreads();
    const uint32_t ci = s_cell_idx;
    if (ci == NO_CELL) { // a cell the plan was not built for
        if (tid < n_rec) res[tid] = mi_lte_phich_result{0.0f, 0.0f, {0.0f, 0.0f, 0.0f}, 0u, MI_LTE_PHICH_UNKNOWN_CELL, 0u};
        return;
    }
    // ---- 1. gather, combine, descramble
    const float    *y_re = subframes + (size_t)unit * sf_stride, *y_im = y_re + PLANE, *h_re = y_re + 2 * PLANE, *h_im = h_re + (size_t)N_ant * PLANE;
    const uint32_t *re = P.re + (size_t)ci * n_items;
    const uint32_t  c = gold_word(gt, (((sf + 1) * (2 * cell + 1)) << 9) + cell, 0); // (uniform) bits 0 .. 11: c(0) .. c(11)
    for (uint32_t t0 = 0; t0 < n_items; t0 += PHICH_THREADS) { // (uniform trip count: every lane takes part in the exchange)
        const uint32_t t = t0 + tid, m = t / N_RE, e = t - m * N_RE, i = e >> 2;
        const bool     live = t < n_items;
        const uint32_t k = live ? re[t] : 0u;
        const uint32_t pA = N_ant == 4 ? ((i + m) & 1u) : 0u, pB = N_ant == 4 ? pA + 2 : 1u; // 36.211 6.9.2: the pair holds for the whole quadruplet
        const float    yr = y_re[k], yi = y_im[k], ar = h_re[(size_t)pA * PLANE + k], ai = h_im[(size_t)pA * PLANE + k];
        float          r_re = ar * yr + ai * yi, r_im = ar * yi - ai * yr, pw = ar * ar + ai * ai; // conj(hA) y
        if (N_ant > 1) {
            const float br = h_re[(size_t)pB * PLANE + k], bi = h_im[(size_t)pB * PLANE + k];
            const float qyr = __shfl_xor(yr, 1, 64), qyi = __shfl_xor(yi, 1, 64), qbr = __shfl_xor(br, 1, 64), qbi = __shfl_xor(bi, 1, 64);
            const float x_re = qbr * qyr + qbi * qyi, x_im = qbi * qyr - qbr * qyi; // hB_partner conj(y_partner)
            const float root2 = 1.41421356237309505f;
            r_re = (e & 1u) ? (r_re - x_re) * root2 : (r_re + x_re) * root2;
            r_im = (e & 1u) ? (r_im - x_im) * root2 : (r_im + x_im) * root2;
            pw += qbr * qbr + qbi * qbi;
        }
        if (live) {
            const bool neg = (c >> e) & 1u; // s(e) = 1 - 2 c(e)
            s_re[t] = neg ? -r_re : r_re;
            s_im[t] = neg ? -r_im : r_im;
            s_p[t]  = pw;
        }
    }
    __syncthreads();
    // ---- 2. despread: one (group, sequence) per thread
    if (tid >= n_rec) return;
    const uint32_t m = tid >> 3, n = tid & 7u, w = n & 3u;
    const float   *g_re = s_re + m * N_RE, *g_im = s_im + m * N_RE, *g_p = s_p + m * N_RE;
    float          p_tot = 0.0f;
#pragma unroll
    for (uint32_t e = 0; e < N_RE; e++) p_tot += g_p[e];
    const bool          dead = !(p_tot > 0.0f) || !isfinite(p_tot);
    mi_lte_phich_result r;
    r.metric = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < 3; i++) {
        float a_re = 0.0f, a_im = 0.0f; // sum_j walsh[n mod 4][j] r(4 i + j): +, (-1)^j, (-1)^(j >> 1), (-1)^(j + (j >> 1))
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bool minus = (w == 1 && (j & 1u)) || (w == 2 && (j & 2u)) || (w == 3 && (j == 1 || j == 2));
            a_re += minus ? -g_re[4 * i + j] : g_re[4 * i + j];
            a_im += minus ? -g_im[4 * i + j] : g_im[4 * i + j];
        }
        // q = conj(w_n) ...: the sum itself for n < 4, -j times it for n >= 4; Re(q conj(z0)) = (Re q + Im q) / sqrt 2
        const float q_re = n < 4 ? a_re : a_im, q_im = n < 4 ? a_im : -a_re;
        r.rep[i] = dead ? 0.0f : (q_re * 0.70710678118654752f + q_im * 0.70710678118654752f) / p_tot;
        r.metric += r.rep[i];
    }
    r.power    = dead ? 0.0f : p_tot;
    r.hi       = r.metric < 0.0f ? 1u : 0u;
    r.flags    = dead ? MI_LTE_PHICH_NO_POWER : 0u;
    r.reserved = 0;
    res[tid] = r;
}

} // namespace

struct mi_lte_phich_plan {
    mi_lte_dl_cfg       cfg;
    PhichDev            dev{};
    std::vector<void *> owned;
};

extern "C" {

int mi_lte_phich_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, float phich_res, uint32_t phich_dur_extended, uint32_t flags,
                             const uint32_t *h_cells, uint32_t n_cells, mi_lte_phich_plan **out)
{
    if (!ctx || !cfg || !h_cells || n_cells == 0 || !out) return MI_LTE_ERR_INVALID_ARG;
    const uint32_t nrb = cfg->N_rb_dl, N_group = n_group(nrb, phich_res);
    if (N_group == 0 || N_group > MAX_GROUP || !(cfg->N_ant == 1 || cfg->N_ant == 2 || cfg->N_ant == 4) || phich_dur_extended || flags != 0 ||
        (cfg->sample_format & MI_LTE_CE_COMPACT)) {
        ctx->err = "PHICH plan: standard bandwidths, 1/2/4 ports, PHICH resource in (0, 2], normal PHICH duration, full estimate planes, flags = 0";
        return MI_LTE_ERR_INVALID_ARG;
    }
    std::vector<uint32_t> cells(h_cells, h_cells + n_cells), re((size_t)n_cells * N_group * N_RE), one;
    for (uint32_t c = 0; c < n_cells; c++) {
        if (!cell_res(nrb, cells[c], phich_res, one) || one.size() != (size_t)N_group * N_RE) {
            ctx->err = "PHICH plan: a cell identity past 503";
            return MI_LTE_ERR_INVALID_ARG;
        }
        std::copy(one.begin(), one.end(), re.begin() + (size_t)c * N_group * N_RE); // (every entry < 12 N_rb_dl <= 1200: cell_res checked)
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl = new mi_lte_phich_plan();
    auto  guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_lte_phich_plan_destroy(nullptr, pl); });
    pl->cfg = *cfg;
    auto up = [&](const void *h, size_t bytes, void **d) -> int {
        if (hipMalloc(d, bytes ? bytes : 4) != hipSuccess) return -1;
        pl->owned.push_back(*d);
        return mi_lte_memcpy_h2d(ctx, *d, h, bytes) == MI_LTE_OK ? 0 : -1;
    };
    void *d_cells, *d_re;
    if (up(cells.data(), cells.size() * 4, &d_cells) || up(re.data(), re.size() * 4, &d_re)) {
        ctx->err = "PHICH plan: device allocation failed";
        return MI_LTE_ERR_NOMEM;
    }
    MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx));
    pl->dev = PhichDev{N_group, n_cells, (const uint32_t *)d_cells, (const uint32_t *)d_re};
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}

void mi_lte_phich_plan_destroy(mi_lte_ctx *ctx, mi_lte_phich_plan *pl)
{
    if (!pl) return;
    if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
    for (void *p : pl->owned) (void)hipFree(p);
    delete pl;
}

uint32_t mi_lte_phich_plan_n_group(const mi_lte_phich_plan *pl) { return pl ? pl->dev.N_group : 0u; }

int mi_lte_phich_decode_run(mi_lte_ctx *ctx, mi_lte_phich_plan *pl, const float *d_subframes, const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell,
                            uint32_t n_units, mi_lte_phich_result *d_out)
{
    if (!ctx || !pl || !d_subframes || !d_subfr_num || !d_n_id_cell || n_units == 0 || !d_out) return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const int rc = mi_ctx_gold_tables(ctx);
    if (rc != MI_LTE_OK) return rc;
    GoldTables     gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
    const uint32_t stride = (uint32_t)mi_lte_subframe_floats(pl->cfg.N_ant);
    if (pl->cfg.N_ant == 1)
        MI_LAUNCH(ctx, "k_phich_decode", k_phich_decode<1>, dim3(n_units), dim3(PHICH_THREADS), 0, d_subframes, stride, d_subfr_num, d_n_id_cell, pl->dev, gt, d_out);
    else if (pl->cfg.N_ant == 2)
        MI_LAUNCH(ctx, "k_phich_decode", k_phich_decode<2>, dim3(n_units), dim3(PHICH_THREADS), 0, d_subframes, stride, d_subfr_num, d_n_id_cell, pl->dev, gt, d_out);
    else
        MI_LAUNCH(ctx, "k_phich_decode", k_phich_decode<4>, dim3(n_units), dim3(PHICH_THREADS), 0, d_subframes, stride, d_subfr_num, d_n_id_cell, pl->dev, gt, d_out);
    MI_HIP_CHECK(ctx, hipGetLastError());
    ctx->last_kernels = "k_phich_decode:1";
    return MI_LTE_OK;
}

} // extern "C"
