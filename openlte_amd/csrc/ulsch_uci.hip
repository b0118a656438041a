// HARQ-ACK, rank indication and CQI multiplexed on PUSCH (36.212 5.2.2.6-5.2.2.8, scrambling per 36.211 5.3.1) in the 3GPP transport-block
// mode of the PUSCH plans (uplink.hip: mi_lte_pusch_plan_create_3gpp_uci; the rules are written out in include/mi_lte.h).
//
// The interleaver matrix of an allocation has M = 12 N_prb rows and 12 columns of Q_m-bit cells.  k_pusch_demod (unchanged) leaves cell (r, c)
// at byte (r*12 + c)*Q_m of the allocation's soft bits, i.e. row-major -- the order in which 5.2.2.8 writes CQI and then data, skipping the RI
// cells.  After it:
//   k_ulsch_uci_gather  grid (tile, allocation), a lane owns 4 output bytes: the allocation's G data soft bits in sequence order followed by
//                       its Q_cqi CQI soft bits (data | CQI, so that the data start on the plan's 64-byte offset), 0 where an ACK symbol
//                       overwrote the cell.  The cell of stream symbol t is closed-form: rows above the RI region hold 12 stream cells, the
//                       one partial RI row 12 - Qp_ri mod 4, full RI rows 8 -- no scan, no LDS.
//   k_ulsch_uci_decide  one workgroup per allocation: the int32 sums of the ACK and RI symbols' soft bits 0 and 1 (wave reduction, then LDS;
//                       integer sums are order-free, so the result is exact), the decisions, one result record per allocation.
// The host arithmetic -- the descriptor checks (mi_lte_ulsch_uci_G), the Q' arithmetic, and the forward map the transmitter is driven by
// (mi_lte_ulsch_uci_map), written from the placement rules where the kernels use their inverse -- is ulsch_host.cc's.
#include <algorithm>
#include <cstring>
#include <vector>

#include "plan_core.hpp"
#include "phy_dev.hpp"
#include "ulsch_uci.h"

namespace {

struct UciDesc { uint32_t M, Qm, Qp_ack, Qp_ri, O_ack, O_ri, Q_cqi, G, c_init, pad[3]; };
static_assert(sizeof(UciDesc) == 48, "12 words");

// columns by position in the walk (one nibble each): RI 1, 10, 7, 4; ACK 2, 9, 8, 3 (36.212 table 5.2.2.8-1/-2, j <- (j + 3) mod 4)
constexpr uint32_t RI_COLS = 0x47A1u, ACK_COLS = 0x3892u;
// an ACK column's position in its walk by column (nibble c), 15 for the other columns
constexpr uint64_t ACK_POS = 0xFF12FFFF30FFull;
// the columns of a row that hold CQI / data, in ascending order: a row without RI, the partial row after 1, 2, 3 RI symbols, a full RI row
__device__ __forceinline__ uint64_t stream_cols(uint32_t n_ri)
{
    return n_ri == 0 ? 0xBA9876543210ull : n_ri == 1 ? 0xBA987654320ull : n_ri == 2 ? 0xB987654320ull : n_ri == 3 ? 0xB98654320ull : 0xB9865320ull;
}
constexpr uint32_t GATHER_THREADS = 256, GATHER_TILE = 4 * GATHER_THREADS; // bytes of output per workgroup

// Cell (r, c) of symbol t of the CQI | data stream: rows 0 .. R0 - 1 hold 12 of its symbols each, row R0 (when Qp_ri mod 4 != 0) 12 - Qp_ri mod 4,
// the rows below 8.  t < 12 M - Qp_ri.
__device__ __forceinline__ uint32_t stream_cell(uint32_t t, uint32_t M, uint32_t Qp_ri, uint32_t &r)
{
    const uint32_t rem = Qp_ri & 3u;
    uint32_t       R0  = M - (Qp_ri >> 2) - (rem ? 1u : 0u);
    if (t < 12 * R0) {
        r = __umul24(t, 43691u) >> 19; // t / 12 for t < 2^15 (12 M <= 15 840)
        return t - 12 * r;
    }
    t -= 12 * R0;
    if (rem) {
        if (t < 12 - rem) { r = R0; return (uint32_t)(stream_cols(rem) >> (4 * t)) & 15u; }
        t -= 12 - rem;
        R0++;
    }
    r = R0 + (t >> 3);
    return (uint32_t)(stream_cols(4) >> (4 * (t & 7u))) & 15u;
}

__device__ __forceinline__ bool ack_cell(uint32_t r, uint32_t c, uint32_t M, uint32_t Qp_ack)
{
    const uint32_t pos = (uint32_t)(ACK_POS >> (4 * c)) & 15u;
    return pos != 15u && 4 * (M - 1 - r) + pos < Qp_ack;
}

// sizeof(T) soft bits (2 or 4 bytes inside one symbol) at byte s of the CQI | data stream; 0 for a symbol that an ACK symbol overwrote
template <uint32_t QM, typename T> __device__ __forceinline__ uint32_t stream_load(const UciDesc &d, const int8_t *__restrict__ src, uint32_t s)
{
    const uint32_t t = s / QM, q = s - t * QM;
    uint32_t       r;
    const uint32_t c = stream_cell(t, d.M, d.Qp_ri, r);
    if (ack_cell(r, c, d.M, d.Qp_ack)) return 0u;
    return *reinterpret_cast<const T *>(src + (__umul24(r, 12u) + c) * QM + q); // (q even, cells Q_m bytes apart: aligned)
}

template <uint32_t QM> __device__ __forceinline__ void gather_dword(const UciDesc &d, const int8_t *__restrict__ src, int8_t *__restrict__ dst, uint32_t o)
{
    const uint32_t run = d.G + d.Q_cqi; // even; the allocation's slot has room for the dword that holds its last pair (12 * 12 N_prb * Q_m is a multiple of 4)
    if (o >= run) return;
    // output byte o: data bit o for o < G, CQI bit o - G behind them; in the stream CQI comes first
    auto at = [&](uint32_t ob) { return ob < d.G ? ob + d.Q_cqi : ob - d.G; };
    uint32_t v;
    if (QM == 4) v = stream_load<QM, uint32_t>(d, src, at(o)); // one symbol per dword (G and Q_cqi are multiples of 4)
    else {
        v = stream_load<QM, uint16_t>(d, src, at(o));
        if (o + 2 < run) v |= stream_load<QM, uint16_t>(d, src, at(o + 2)) << 16;
    }
    *reinterpret_cast<uint32_t *>(dst + o) = v;
}

__global__ __launch_bounds__(GATHER_THREADS) void k_ulsch_uci_gather(const UciDesc *__restrict__ desc, const int8_t *__restrict__ e_base,
                                                                     const uint32_t *__restrict__ e_off, int8_t *__restrict__ out_base)
{
    const uint32_t a = blockIdx.y, o = 4 * (blockIdx.x * GATHER_THREADS + threadIdx.x);
    const UciDesc  d = desc[a]; // (uniform: scalar loads)
    if (blockIdx.x * GATHER_TILE >= d.G + d.Q_cqi) return;
    const size_t   off = (size_t)e_off[a] * 64;
    if (d.Qm == 2) gather_dword<2>(d, e_base + off, out_base + off, o);
    else if (d.Qm == 4) gather_dword<4>(d, e_base + off, out_base + off, o);
    else gather_dword<6>(d, e_base + off, out_base + off, o);
}

constexpr uint32_t DECIDE_THREADS = 256;

// The sums of one control stream (ACK or RI): symbol n sits in cell (M - 1 - n / 4, cols[n mod 4]); only its bits 0 and 1 are used
__device__ __forceinline__ void uci_sums(const UciDesc &d, const GoldTables &gt, const int8_t *__restrict__ e, uint32_t O, uint32_t Qp, uint32_t cols, int32_t (&S)[3])
{
    S[0] = S[1] = S[2] = 0;
    if (O == 0) return; // (uniform)
    for (uint32_t n = threadIdx.x; n < Qp; n += DECIDE_THREADS) {
        const uint32_t r = d.M - 1 - (n >> 2), c = (cols >> (4 * (n & 3u))) & 15u;
        const int8_t  *p = e + (__umul24(r, 12u) + c) * d.Qm;
        int            u0 = p[0], u1 = p[1];
        if (O == 1) {
            // [o0 y ..]: the transmitter repeated the scrambled bit i0 at i0 + 1 (36.211 5.3.1) and the demodulator descrambled it with
            // c(i0 + 1).  i0 is even, so both bits lie in one word of the sequence
            const uint32_t i0 = (__umul24(c, d.M) + r) * d.Qm, pair = (gold_word(gt, d.c_init, i0 >> 5) >> (i0 & 31u)) & 3u;
            if (pair == 1u || pair == 2u) u1 = -u1;
            S[0] += u0 + u1;
        } else {
            const uint32_t j0 = (2 * n) % 3u, j1 = (2 * n + 1) % 3u;
#pragma unroll
            for (uint32_t j = 0; j < 3; j++) S[j] += (j == j0 ? u0 : 0) + (j == j1 ? u1 : 0);
        }
    }
}

// bits from sums: O = 1: S[0] < 0; O = 2: the first maximum of sum_j (1 - 2 w_j) S[j], w = (o0, o1, o0 ^ o1), over (o0, o1) = 00, 01, 10, 11
__device__ __forceinline__ void uci_decide(uint32_t O, const int32_t *S, uint8_t *bits)
{
    bits[0] = bits[1] = 0;
    if (O == 1) bits[0] = S[0] < 0;
    else if (O == 2) {
        int32_t  best = 0;
        uint32_t arg  = 0;
        for (uint32_t h = 0; h < 4; h++) {
            const uint32_t o0 = h >> 1, o1 = h & 1u, w2 = o0 ^ o1;
            const int32_t  m = (o0 ? -S[0] : S[0]) + (o1 ? -S[1] : S[1]) + (w2 ? -S[2] : S[2]);
            if (h == 0 || m > best) { best = m; arg = h; }
        }
        bits[0] = (uint8_t)(arg >> 1); bits[1] = (uint8_t)(arg & 1u);
    }
}

__global__ __launch_bounds__(DECIDE_THREADS) void k_ulsch_uci_decide(const UciDesc *__restrict__ desc, GoldTables gt, const int8_t *__restrict__ e_base,
                                                                     const uint32_t *__restrict__ e_off, mi_lte_ulsch_uci_result *__restrict__ res)
{
    __shared__ int32_t part[DECIDE_THREADS / 64][6];
    const uint32_t a = blockIdx.x;
    const UciDesc  d = desc[a];
    const int8_t  *e = e_base + (size_t)e_off[a] * 64;
    int32_t        Sa[3], Sr[3];
    uci_sums(d, gt, e, d.O_ack, d.Qp_ack, ACK_COLS, Sa);
    uci_sums(d, gt, e, d.O_ri, d.Qp_ri, RI_COLS, Sr);
    int32_t S[6] = {Sa[0], Sa[1], Sa[2], Sr[0], Sr[1], Sr[2]};
#pragma unroll
    for (uint32_t k = 0; k < 6; k++) {
        for (int off = 32; off > 0; off >>= 1) S[k] += __shfl_down(S[k], off, 64);
        if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6][k] = S[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        mi_lte_ulsch_uci_result out;
        int32_t T[6];
        for (uint32_t k = 0; k < 6; k++) {
            T[k] = 0;
            for (uint32_t w = 0; w < DECIDE_THREADS / 64; w++) T[k] += part[w][k];
        }
        for (uint32_t k = 0; k < 3; k++) { out.S_ack[k] = T[k]; out.S_ri[k] = T[3 + k]; }
        uci_decide(d.O_ack, T, out.ack);
        uci_decide(d.O_ri, T + 3, out.ri);
        res[a] = out; // (an allocation without control information: every sum and bit 0)
    }
}

} // namespace

int mi_ulsch_uci_create(mi_lte_ctx *ctx, const mi_lte_pdsch_alloc *h_allocs, const mi_lte_ulsch_uci *h_uci, const uint32_t *h_c_init,
                        const uint32_t *h_G, uint32_t n_alloc, size_t e_bytes, MiUlschUci **out)
{
    auto *u    = new MiUlschUci();
    auto guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_ulsch_uci_free(u); });
    u->n_alloc = n_alloc;
    u->h_G.assign(h_G, h_G + n_alloc); u->h_Q_cqi.resize(n_alloc);
    std::vector<UciDesc> desc(n_alloc);
    for (uint32_t a = 0; a < n_alloc; a++) {
        const mi_lte_pdsch_alloc &al = h_allocs[a];
        const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : 2;
        desc[a] = {12 * al.N_prb, Qm, h_uci[a].Qp_ack, h_uci[a].Qp_ri, h_uci[a].O_ack, h_uci[a].O_ri, h_uci[a].Q_cqi, h_G[a], h_c_init[a], {0, 0, 0}};
        u->h_Q_cqi[a] = h_uci[a].Q_cqi;
        u->tiles = std::max(u->tiles, (h_G[a] + h_uci[a].Q_cqi + GATHER_TILE - 1) / GATHER_TILE);
    }
    MI_HIP_CHECK(ctx, hipMalloc(&u->d_desc, sizeof(UciDesc) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&u->d_e, std::max<size_t>(e_bytes, 64)));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&u->d_e_len, sizeof(uint32_t) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&u->d_res, sizeof(mi_lte_ulsch_uci_result) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&u->d_cqi_desc, sizeof(mi_lte_cqi_desc) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&u->d_cqi_res, sizeof(mi_lte_cqi_result) * n_alloc));
    MI_HIP_CHECK(ctx, hipMemsetAsync(u->d_e, 0, std::max<size_t>(e_bytes, 64), ctx->stream)); // (the taps read defined bytes before a first run)
    MI_HIP_CHECK(ctx, hipMemsetAsync(u->d_res, 0, sizeof(mi_lte_ulsch_uci_result) * n_alloc, ctx->stream));
    MI_HIP_CHECK(ctx, hipMemsetAsync(u->d_cqi_desc, 0, sizeof(mi_lte_cqi_desc) * n_alloc, ctx->stream));
    MI_HIP_CHECK(ctx, hipMemsetAsync(u->d_cqi_res, 0, sizeof(mi_lte_cqi_result) * n_alloc, ctx->stream));
    MI_H2D(ctx, u->d_desc, desc.data(), sizeof(UciDesc) * n_alloc);
    MI_H2D(ctx, u->d_e_len, u->h_G.data(), sizeof(uint32_t) * n_alloc);
    MI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    guard.armed = false;
    *out = u;
    return MI_LTE_OK;
}

void mi_ulsch_uci_free(MiUlschUci *u)
{
    if (!u) return;
    (void)hipFree(u->d_desc);
    (void)hipFree(u->d_e);
    (void)hipFree(u->d_e_len);
    (void)hipFree(u->d_res);
    (void)hipFree(u->d_cqi_desc);
    (void)hipFree(u->d_cqi_res);
    delete u;
}

int mi_ulsch_uci_run(mi_lte_ctx *ctx, MiUlschUci *u, const int8_t *d_e, const uint32_t *d_e_off)
{
    GoldTables gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
    MI_LAUNCH(ctx, "k_ulsch_uci_gather", k_ulsch_uci_gather, dim3(u->tiles, u->n_alloc), dim3(GATHER_THREADS), 0, (const UciDesc *)u->d_desc, d_e, d_e_off, u->d_e);
    MI_LAUNCH(ctx, "k_ulsch_uci_decide", k_ulsch_uci_decide, dim3(u->n_alloc), dim3(DECIDE_THREADS), 0, (const UciDesc *)u->d_desc, gt, d_e, d_e_off, u->d_res);
    MI_HIP_CHECK(ctx, hipGetLastError());
    return MI_LTE_OK;
}
