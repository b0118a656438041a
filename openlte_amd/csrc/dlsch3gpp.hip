// 3GPP transport-block mode of the PDSCH plans (mi_lte_pdsch_plan_create_3gpp, include/mi_lte.h): DL-SCH decoding of transport blocks of
// one to thirteen code blocks as 36.212 5.1.2 (segmentation, CRC24B), 5.1.3 (turbo code) and 5.1.4.1 (rate matching, concatenation)
// specify.  The reference's own C > 1 path is broken, so this mode is specified by 36.212 alone; the rate-matching geometry
// is the reference's liblte_phy_rate_unmatch_turbo (liblte_phy.cc:11246-11490) with N_codeblocks = C, which the tests pin it to.
//
// After the plan's demodulator (chain.hip, unchanged) has written every allocation's soft bits and their count G:
//   k_dl3_desc       one thread per code-block slot: E_r, its offset, N_cb and k0 from G (G depends on the subframe: device side)
//   k_dl3_rm_i8      one workgroup per code block: rate un-matching into the interleaved int8 block the BCJR decoders take
//   (decode)         mi_lte_turbo_decode_batch's BCJR kernels, one launch set per block size (bcjr.hip, unchanged)
//   k_dl3_cb_finish  one workgroup per code block: CRC24B, the block's payload into the transport block's output row, its share of the CRC24A
//   k_dl3_tb_finish  one thread per transport block: the shares combined, status and the per-block CRC mask
// A HARQ run (mi_lte_pdsch_decode_run_harq) adds the soft combining of the pool's buffers (include/mi_lte.h):
//   k_harq_bind      one thread per allocation, after k_dl3_desc: the flush rule against the buffer's state, the state's new tbs .. n_tx,
//                    and the buffer / flush word of the allocation's code-block slots
//   k_harq_rm        k_dl3_rm_i8's place: the same gather sums, combined into the int16 buffer (saturating), the decoder's int8 input from it
//   k_harq_commit    one thread per allocation, after k_dl3_tb_finish: the transport block's verdict into the state
#include <algorithm>
#include <cstring>
#include <vector>

#include "dlsch3_layout.h"
#include "plan_core.hpp"
#include "rm_geom.h"

namespace {

constexpr uint32_t DL3_E_CAP = 48 * 1024; // LDS a code block stages its soft bits in (larger E_r: read from global memory)

__device__ inline uint32_t q_m(uint32_t mod_type) { return mod_type == 3 ? 6u : mod_type == 2 ? 4u : mod_type == 1 ? 2u : 1u; }
// Everything the per-code-block kernels need: the static part from the plan (Dl3Slot, dlsch3_layout.h), the rest from k_dl3_desc
struct Dl3Desc {
    uint32_t alloc, r, C, K;
    uint32_t E, off, N_cb, k0;
    uint32_t tbs, xs, soft_off4, bits_off8; // xs = x^s mod gCRC24A, s = transport-block bits after the block's last payload bit
};

__global__ __launch_bounds__(256) void k_dl3_desc(const Dl3Slot *__restrict__ slots, uint32_t n_slot, const mi_lte_pdsch_alloc *__restrict__ allocs,
                                                  const uint32_t *__restrict__ e_len, uint32_t N_soft, uint32_t M_dl_harq, uint32_t N_L, Dl3Desc *__restrict__ out)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slot) return;
    const Dl3Slot             sl = slots[s];
    const mi_lte_pdsch_alloc &al = allocs[sl.alloc];
    // (N_L: 2 on a transmit-diversity plan, whose symbols stay in pairs; 1 on every other plan, the uplink's included)
    const uint32_t Qm = N_L * q_m(al.mod_type), Gp = e_len[sl.alloc] / Qm, gam = Gp % sl.C, lo = Gp / sl.C, C = sl.C, r = sl.r;
    Dl3Desc d;
    d.alloc = sl.alloc; d.r = r; d.C = C; d.K = sl.K;
    d.E   = Qm * (r + gam < C ? lo : lo + 1);                    // r <= C - gamma - 1: floor(G' / C), else ceil
    d.off = Qm * (r * lo + (r > C - gam ? r - (C - gam) : 0u)); // blocks C - gamma .. r - 1 have one symbol more
    const RmSoftBuf sb = rm_soft_buffer(sl.K + 4, C, al.tx_mode, N_soft, M_dl_harq, true, al.rv_idx & 3u); // (as the host lays the block out: mi_lte_dlsch_layout, synth.cc)
    d.N_cb = sb.N_cb; d.k0 = sb.k0;
    d.tbs = al.tbs; d.xs = sl.xs; d.soft_off4 = sl.soft_off4; d.bits_off8 = sl.bits_off8;
    out[s] = d;
}

__device__ __forceinline__ int sat16(int v) { return max(-32768, min(32767, v)); }
__device__ __forceinline__ int clamp127(int v) { return max(-127, min(127, v)); }

// Rate un-matching of one code block into the decoder's int8 layout d[i*3+x], tail included, the part k_dl3_rm_i8 and k_harq_rm share:
// stage() puts the block's E_r soft bits in LDS (aligned dwords) when they fit; sum(t) is what position p of d[t] in the circular buffer
// receives, e[rank(p) + t Nnn], t = 0, 1, .. (rank = non-NULL positions between k0 and p in walk order: rm_geom.h), summed; 0 where no soft bit reaches.
struct Dl3Gather {
    RmGeom        rm;
    const int8_t *es;
    uint32_t      E, n; // E_r; the block's 3 (K + 4) positions
    __device__ void stage(const Dl3Desc &d, const int8_t *e_base, const uint32_t *e_off, int8_t *e_lds, uint32_t e_cap)
    {
        const uint32_t D = d.K + 4;
        E = d.E; n = 3 * D;
        rm.init(D, d.N_cb, d.k0);
        const int8_t  *e      = e_base + (size_t)e_off[d.alloc] * 64 + d.off; // (an allocation's slot is 64-byte aligned and padded to 64 bytes)
        const uint32_t shift  = (uint32_t)(reinterpret_cast<uintptr_t>(e) & 3u);
        const bool     staged = shift + E <= e_cap;
        if (staged) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(e - shift);
            for (uint32_t w = threadIdx.x; w < (shift + E + 3) / 4; w += blockDim.x) reinterpret_cast<uint32_t *>(e_lds)[w] = src[w];
        }
        __syncthreads();
        es = staged ? e_lds + shift : e;
    }
    __device__ int sum(uint32_t t) const
    {
        const uint32_t i = t / 3;
        int            v = 0;
        for (uint32_t k = rm.rank(i, t - 3 * i); k < E; k += rm.Nnn) v += es[k];
        return v;
    }
};

// the sums saturated to +-127
__global__ __launch_bounds__(256) void k_dl3_rm_i8(const Dl3Desc *__restrict__ desc, const int8_t *__restrict__ e_base, const uint32_t *__restrict__ e_off,
                                                   int8_t *__restrict__ soft, uint32_t e_cap)
{
    extern __shared__ __attribute__((aligned(16))) int8_t e_lds[];
    const Dl3Desc &d = desc[blockIdx.x];
    Dl3Gather      g;
    g.stage(d, e_base, e_off, e_lds, e_cap);
    int8_t *db = soft + (size_t)d.soft_off4 * 4;
    for (uint32_t t = threadIdx.x; t < g.n; t += blockDim.x) db[t] = (int8_t)clamp127(g.sum(t));
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    return v;
}

// One code block's decisions: CRC24B over its K bits (C > 1), its payload into the output row, and its share of the transport block's
// CRC24A -- the remainder of its payload bits times x^s, s = the bits that follow them in the transport block -- so that the shares of a
// transport block XOR to its CRC24A remainder.  tab_a / tab_b: x^e mod g for e < 6144.
// A block whose 3 (K + 4) channel values (soft: the decoder's input) are ALL zero is an erasure: the decoder's decisions are then all 0, and
// the all-zero block divides by both generators -- CB_ERASED in its ok word makes k_dl3_tb_finish fail the transport block whatever the CRCs say.
constexpr uint32_t CB_ERASED = 0x80000000u;
__global__ __launch_bounds__(256) void k_dl3_cb_finish(const Dl3Desc *__restrict__ desc, const uint8_t *__restrict__ c_bits, const uint32_t *__restrict__ tab_a,
                                                       const uint32_t *__restrict__ tab_b, uint8_t *__restrict__ out_bits, uint32_t out_stride, uint32_t packed,
                                                       uint32_t *__restrict__ part, uint32_t *__restrict__ ok, const int8_t *__restrict__ soft)
{
    __shared__ uint32_t red[3][4];
    const Dl3Desc &d = desc[blockIdx.x];
    const uint32_t K = d.K, C = d.C, tbs = d.tbs, nb = C > 1 ? K - 24 : K, q0 = d.r * (K - 24); // (C = 1: q0 = 0)
    const uint8_t *c = c_bits + (size_t)d.bits_off8 * 8;
    uint8_t       *o = out_bits + (size_t)d.alloc * out_stride;
    uint32_t crc_a = 0, crc_b = 0;
    // eight bits per thread and step (K, nb, q0 and tbs are multiples of 8): one 8-byte read, the weight of the last bit from the table and
    // the other seven by "times x"
    for (uint32_t g8 = threadIdx.x; g8 < K / 8; g8 += blockDim.x) {
        const uint32_t j0 = 8 * g8;
        const uint2    bb = *reinterpret_cast<const uint2 *>(c + j0);
        const uint32_t lo = bb.x & 0x01010101u, hi = bb.y & 0x01010101u;
        const bool     in_a = j0 < nb;
        uint32_t       wa = in_a ? tab_a[nb - 8 - j0] : 0u, wb = tab_b[K - 8 - j0];
#pragma unroll
        for (int k = 7; k >= 0; k--) {
            const uint32_t m = 0u - (((k < 4 ? lo : hi) >> (8 * (k & 3))) & 1u);
            crc_a ^= wa & m;
            crc_b ^= wb & m;
            if (k > 0) { wa = mulx(wa, G_CRC24A); wb = mulx(wb, G_CRC24B); }
        }
        const uint32_t q = q0 + j0; // position in the transport block
        if (in_a && q < tbs) {
            if (packed) o[q >> 3] = (uint8_t)((((lo * 0x08040201u) >> 24) & 0xFu) << 4 | (((hi * 0x08040201u) >> 24) & 0xFu)); // first bit most significant
            else        *reinterpret_cast<uint2 *>(o + q) = make_uint2(lo, hi);
        }
    }
    // (the block's channel values start on a 4-byte boundary and 3 (K + 4) is a multiple of 4: K is a multiple of 8)
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(soft + (size_t)d.soft_off4 * 4);
    uint32_t any = 0;
    for (uint32_t w = threadIdx.x; w < 3 * (K + 4) / 4; w += blockDim.x) any |= sw[w];
    crc_a = wave_xor(crc_a);
    crc_b = wave_xor(crc_b);
    const bool wave_any = __builtin_amdgcn_ballot_w64(any != 0) != 0;
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = crc_a; red[1][threadIdx.x >> 6] = crc_b; red[2][threadIdx.x >> 6] = wave_any ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0, nz = 0;
        for (uint32_t w = 0; w < blockDim.x / 64; w++) { a ^= red[0][w]; b ^= red[1][w]; nz |= red[2][w]; }
        part[blockIdx.x] = mulmod(a, d.xs, G_CRC24A);
        ok[blockIdx.x]   = !nz ? CB_ERASED : (C == 1 || b == 0) ? 1u : 0u;
    }
}

// One thread per transport block: CRC24A = XOR of its blocks' shares, the blocks' CRC24B verdicts as a mask, the status word
__global__ __launch_bounds__(256) void k_dl3_tb_finish(const uint32_t *__restrict__ a_slot, const uint32_t *__restrict__ a_nc, uint32_t n_alloc,
                                                       const uint32_t *__restrict__ part, const uint32_t *__restrict__ ok, int32_t *__restrict__ status,
                                                       uint32_t *__restrict__ cb_ok)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_alloc) return;
    const uint32_t s0 = a_slot[a], C = a_nc[a];
    uint32_t rem = 0, mask = 0, erased = 0;
    for (uint32_t r = 0; r < C; r++) {
        rem ^= part[s0 + r];
        mask |= (ok[s0 + r] & 1u) << r;
        erased |= ok[s0 + r] & CB_ERASED;
    }
    const bool crc_a = rem == 0 && !erased; // (an erased block: no verdict can be read from its CRCs, k_dl3_cb_finish)
    if (C == 1) mask = crc_a ? 1u : 0u;
    status[a] = (crc_a && mask == (1u << C) - 1u) ? 0 : 2;
    cb_ok[a]  = mask;
}

// ------------------------------------------------------------------------------------------------ HARQ soft combining

constexpr uint32_t HARQ_FLUSH = 0x80000000u; // in a slot's word: the buffer starts empty in this run (buffer index below it)

// One thread per allocation of the plan: buffer and flush rule (36.321 5.3.2.2) for a bound one, MI_LTE_HARQ_NONE for the others, written to
// every code-block slot of the allocation.  No buffer is bound twice in a run (the host refuses it), so the state updates do not race.
__global__ __launch_bounds__(256) void k_harq_bind(const Dl3Desc *__restrict__ desc, const uint32_t *__restrict__ a_slot, uint32_t n_alloc,
                                                   const mi_lte_harq_bind *__restrict__ bind, mi_lte_harq_state *__restrict__ state,
                                                   uint32_t *__restrict__ slot_buf)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_alloc) return;
    const uint32_t      s0 = a_slot[a];
    const Dl3Desc      &d  = desc[s0];
    const mi_lte_harq_bind b = bind[a];
    uint32_t w = MI_LTE_HARQ_NONE;
    if (b.buf != MI_LTE_HARQ_NONE) {
        mi_lte_harq_state st = state[b.buf];
        const bool flush = (b.flags & MI_LTE_HARQ_NEW_DATA) || st.n_tx == 0 || st.tbs != d.tbs || st.N_cb != d.N_cb;
        st.tbs = d.tbs; st.C = d.C; st.K = d.K; st.N_cb = d.N_cb;
        st.n_tx = flush ? 1u : (st.n_tx < 0xFFFFFFFFu ? st.n_tx + 1u : st.n_tx);
        state[b.buf] = st;
        w = b.buf | (flush ? HARQ_FLUSH : 0u);
    }
    for (uint32_t r = 0; r < d.C; r++) slot_buf[s0 + r] = w;
}

// k_dl3_rm_i8 with soft combining: a slot bound to a buffer sums position t's soft bits as k_dl3_rm_i8 does (v), then
// buf[t] = sat16(buf[t] + sat16(v)) (buf[t] = 0 when the slot's buffer was flushed) and the decoder's input is clamp(buf[t], +-127).
// Two positions per lane: one dword of the buffer read and written (block r starts at an even position), one int16 of the int8 output.
// An unbound slot takes k_dl3_rm_i8's own path.
__global__ __launch_bounds__(256) void k_harq_rm(const Dl3Desc *__restrict__ desc, const int8_t *__restrict__ e_base, const uint32_t *__restrict__ e_off,
                                                 int8_t *__restrict__ soft, uint32_t e_cap, const uint32_t *__restrict__ slot_buf,
                                                 int16_t *__restrict__ pool, size_t buf_elems)
{
    extern __shared__ __attribute__((aligned(16))) int8_t e_lds[];
    const Dl3Desc &d = desc[blockIdx.x];
    Dl3Gather      g;
    g.stage(d, e_base, e_off, e_lds, e_cap);
    int8_t        *db = soft + (size_t)d.soft_off4 * 4;
    const uint32_t sb = slot_buf[blockIdx.x], n = g.n;
    if (sb == MI_LTE_HARQ_NONE) {
        for (uint32_t t = threadIdx.x; t < n; t += blockDim.x) db[t] = (int8_t)clamp127(g.sum(t));
        return;
    }
    const bool flush = (sb & HARQ_FLUSH) != 0;
    uint32_t  *hb    = reinterpret_cast<uint32_t *>(pool + (size_t)(sb & ~HARQ_FLUSH) * buf_elems + (size_t)d.r * n);
    for (uint32_t t2 = threadIdx.x; t2 < n / 2; t2 += blockDim.x) {
        const int      v0 = sat16(g.sum(2 * t2)), v1 = sat16(g.sum(2 * t2 + 1));
        const uint32_t w  = flush ? 0u : hb[t2];
        const int      b0 = sat16((int)(int16_t)(w & 0xFFFFu) + v0), b1 = sat16((int)(int16_t)(w >> 16) + v1);
        hb[t2] = (uint32_t)(uint16_t)b0 | ((uint32_t)(uint16_t)b1 << 16);
        reinterpret_cast<uint16_t *>(db)[t2] = (uint16_t)((uint8_t)(int8_t)clamp127(b0) | ((uint32_t)(uint8_t)(int8_t)clamp127(b1) << 8));
    }
}

// One thread per allocation, after k_dl3_tb_finish: a bound transport block's verdict into its buffer's state
__global__ __launch_bounds__(256) void k_harq_commit(const mi_lte_harq_bind *__restrict__ bind, uint32_t n_alloc, const int32_t *__restrict__ status,
                                                     mi_lte_harq_state *__restrict__ state)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_alloc) return;
    const uint32_t buf = bind[a].buf;
    if (buf != MI_LTE_HARQ_NONE) state[buf].status = status[a];
}

} // namespace

// ------------------------------------------------------------------------------------------------
// host side

struct MiDlsch3 : MiDlsch3Layout { // (the layout's `slots` are dropped once they are on the device)
    mi_lte_dlsch_cfg cfg{};
    uint32_t n_alloc = 0, n_slot = 0, n_l = 1; // n_l: N_L of the code-block concatenation (36.212 5.1.4.1.2)
    Dl3Slot  *d_slot = nullptr;
    Dl3Desc  *d_desc = nullptr;
    int8_t   *d_soft = nullptr;
    uint8_t  *d_bits = nullptr;
    uint32_t *d_tab = nullptr;                 // x^e mod gCRC24A [6144] | x^e mod gCRC24B [6144]
    uint32_t *d_a_slot = nullptr, *d_a_nc = nullptr, *d_part = nullptr, *d_ok = nullptr, *d_cb_ok = nullptr;
    uint32_t *d_slot_buf = nullptr;            // HARQ runs: per slot, the bound buffer | HARQ_FLUSH, or MI_LTE_HARQ_NONE (k_harq_bind)
};

void mi_dlsch3_free(MiDlsch3 *g)
{
    if (!g) return;
    for (void *p : {(void *)g->d_slot, (void *)g->d_desc, (void *)g->d_soft, (void *)g->d_bits, (void *)g->d_tab, (void *)g->d_a_slot, (void *)g->d_a_nc,
                    (void *)g->d_part, (void *)g->d_ok, (void *)g->d_cb_ok, (void *)g->d_slot_buf})
        if (p) (void)hipFree(p);
    delete g;
}

// The device half of a laid-out plan (mi_dlsch3_layout): the slots' arrays and tables.
int mi_dlsch3_create(mi_lte_ctx *ctx, const mi_lte_dlsch_cfg *cfg, MiDlsch3Layout &&lay, uint32_t n_alloc, MiDlsch3 **out, uint32_t n_l)
{
    auto *g   = new MiDlsch3();
    auto guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_dlsch3_free(g); });
    static_cast<MiDlsch3Layout &>(*g) = std::move(lay);
    g->n_l     = n_l;
    g->cfg     = *cfg;
    g->n_alloc = n_alloc;
    g->n_slot  = (uint32_t)g->slots.size();
    const size_t soft = g->soft_bytes, bits = g->bits_bytes;
    std::vector<uint32_t> tab(2 * 6144);
    for (uint32_t e = 0, wa = 1, wb = 1; e < 6144; e++, wa = mulx(wa, G_CRC24A), wb = mulx(wb, G_CRC24B)) { tab[e] = wa; tab[6144 + e] = wb; }
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_slot, sizeof(Dl3Slot) * g->n_slot));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_desc, sizeof(Dl3Desc) * g->n_slot));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_soft, std::max<size_t>(soft, 256)));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_bits, std::max<size_t>(bits, 256)));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_tab, sizeof(uint32_t) * tab.size()));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_a_slot, sizeof(uint32_t) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_a_nc, sizeof(uint32_t) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_part, sizeof(uint32_t) * g->n_slot));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_ok, sizeof(uint32_t) * g->n_slot));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_cb_ok, sizeof(uint32_t) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&g->d_slot_buf, sizeof(uint32_t) * g->n_slot));
    MI_HIP_CHECK(ctx, hipMemsetAsync(g->d_soft, 0, std::max<size_t>(soft, 256), ctx->stream)); // (the taps read defined bytes before a first run)
    MI_HIP_CHECK(ctx, hipMemsetAsync(g->d_cb_ok, 0, sizeof(uint32_t) * n_alloc, ctx->stream));
    MI_H2D(ctx, g->d_slot, g->slots.data(), sizeof(Dl3Slot) * g->n_slot);
    MI_H2D(ctx, g->d_tab, tab.data(), sizeof(uint32_t) * tab.size());
    MI_H2D(ctx, g->d_a_slot, g->a_slot.data(), sizeof(uint32_t) * n_alloc);
    MI_H2D(ctx, g->d_a_nc, g->a_nc.data(), sizeof(uint32_t) * n_alloc);
    MI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<Dl3Slot>().swap(g->slots);
    guard.armed = false;
    *out = g;
    return MI_LTE_OK;
}

// mi_lte_pdsch_plan_create_3gpp has checked every allocation against mi_lte_dlsch_layout.
int mi_dlsch3_create(mi_lte_ctx *ctx, const mi_lte_dlsch_cfg *cfg, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, MiDlsch3 **out, uint32_t n_l)
{
    MiDlsch3Layout lay;
    const char    *err = nullptr;
    const int      rc  = mi_dlsch3_layout(cfg, h_allocs, n_alloc, &lay, &err);
    if (rc != MI_LTE_OK) { ctx->err = err; return rc; }
    return mi_dlsch3_create(ctx, cfg, std::move(lay), n_alloc, out, n_l);
}

// ------------------------------------------------------------------------------------------------
// HARQ soft-buffer pool (include/mi_lte.h)

struct mi_lte_harq_pool {
    int                device = -1;
    uint32_t           n_buf = 0, max_tbs = 0;
    size_t             buf_bytes = 0, buf_elems = 0; // a buffer's soft bytes (mi_lte_harq_buffer_bytes), its stride in int16 (a multiple of 128)
    int16_t           *d_soft = nullptr;
    mi_lte_harq_state *d_state = nullptr;
    // the bindings of a run: pinned staging block -> device copy, cap of each; `staged` guards the block against the previous run's copy
    mi_lte_harq_bind  *h_bind = nullptr, *d_bind = nullptr;
    uint32_t           cap_bind = 0;
    hipEvent_t         staged = nullptr;
};

static void harq_pool_free(mi_lte_harq_pool *p)
{
    if (!p) return;
    if (p->d_soft) (void)hipFree(p->d_soft);
    if (p->d_state) (void)hipFree(p->d_state);
    if (p->d_bind) (void)hipFree(p->d_bind);
    if (p->h_bind) (void)hipHostFree(p->h_bind);
    if (p->staged) (void)hipEventDestroy(p->staged);
    delete p;
}

extern "C" {

int mi_lte_harq_pool_create(mi_lte_ctx *ctx, uint32_t n_buf, uint32_t max_tbs, mi_lte_harq_pool **out)
{
    if (!ctx || !out || n_buf == 0 || n_buf > (1u << 24)) return MI_LTE_ERR_INVALID_ARG;
    const size_t bytes = mi_lte_harq_buffer_bytes(max_tbs);
    if (bytes == 0) { ctx->err = "HARQ pool: no transport block size of the table is <= max_tbs"; return MI_LTE_ERR_INVALID_ARG; }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *p    = new mi_lte_harq_pool();
    auto guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); harq_pool_free(p); });
    p->device = ctx->device; p->n_buf = n_buf; p->max_tbs = max_tbs; p->buf_bytes = bytes;
    p->buf_elems = (bytes / 2 + 127) & ~(size_t)127;
    MI_HIP_CHECK(ctx, hipMalloc((void **)&p->d_soft, 2 * p->buf_elems * n_buf));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&p->d_state, sizeof(mi_lte_harq_state) * n_buf));
    MI_HIP_CHECK(ctx, hipEventCreateWithFlags(&p->staged, hipEventDisableTiming));
    MI_HIP_CHECK(ctx, hipMemsetAsync(p->d_soft, 0, 2 * p->buf_elems * n_buf, ctx->stream));
    MI_HIP_CHECK(ctx, hipMemsetAsync(p->d_state, 0, sizeof(mi_lte_harq_state) * n_buf, ctx->stream));
    MI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    guard.armed = false;
    *out = p;
    return MI_LTE_OK;
}

void mi_lte_harq_pool_destroy(mi_lte_ctx *ctx, mi_lte_harq_pool *p)
{
    if (!p) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream); // (runs that combine into it may still be queued)
    harq_pool_free(p);
}

int mi_lte_harq_pool_reset(mi_lte_ctx *ctx, mi_lte_harq_pool *p, uint32_t buf)
{
    if (!ctx || !p || (buf != MI_LTE_HARQ_NONE && buf >= p->n_buf)) return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t b0 = buf == MI_LTE_HARQ_NONE ? 0u : buf, nb = buf == MI_LTE_HARQ_NONE ? p->n_buf : 1u;
    MI_HIP_CHECK(ctx, hipMemsetAsync(p->d_soft + (size_t)b0 * p->buf_elems, 0, 2 * p->buf_elems * nb, ctx->stream));
    MI_HIP_CHECK(ctx, hipMemsetAsync(p->d_state + b0, 0, sizeof(mi_lte_harq_state) * nb, ctx->stream));
    return MI_LTE_OK;
}

int mi_lte_harq_pool_soft(const mi_lte_harq_pool *p, uint32_t buf, const int16_t **d_soft, const mi_lte_harq_state **d_state)
{
    if (!p || buf >= p->n_buf) return MI_LTE_ERR_INVALID_ARG;
    if (d_soft) *d_soft = p->d_soft + (size_t)buf * p->buf_elems;
    if (d_state) *d_state = p->d_state + buf;
    return MI_LTE_OK;
}

} // extern "C"

// The bindings of a HARQ run against the plan and the pool, on the host, before anything is launched
int mi_dlsch3_harq_check(mi_lte_ctx *ctx, const MiDlsch3 *g, const mi_lte_harq_pool *p, const mi_lte_harq_bind *h_bind)
{
    if (!g || !p || !h_bind) return MI_LTE_ERR_INVALID_ARG;
    if (p->device != ctx->device) { ctx->err = "HARQ pool of another device"; return MI_LTE_ERR_INVALID_ARG; }
    std::vector<uint32_t> seen;
    for (uint32_t a = 0; a < g->n_alloc; a++) {
        const uint32_t b = h_bind[a].buf;
        if (b == MI_LTE_HARQ_NONE) continue;
        if (b >= p->n_buf) { ctx->err = "HARQ binding: buffer index past the pool"; return MI_LTE_ERR_INVALID_ARG; }
        if (g->a_tbs[a] > p->max_tbs || (size_t)g->a_nc[a] * 3 * (g->a_K[a] + 4) * 2 > p->buf_bytes) {
            ctx->err = "HARQ binding: transport block larger than the pool's max_tbs";
            return MI_LTE_ERR_INVALID_ARG;
        }
        seen.push_back(b);
    }
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { ctx->err = "HARQ binding: one buffer bound twice in a run"; return MI_LTE_ERR_INVALID_ARG; }
    return MI_LTE_OK;
}

// Everything after the demodulator (chain.hip: a plan run on a 3GPP plan).  p: the pool of a HARQ run and h_bind its bindings
// (mi_dlsch3_harq_check has passed); nullptr: a plain run.
int mi_dlsch3_run(mi_lte_ctx *ctx, MiDlsch3 *g, mi_lte_harq_pool *p, const mi_lte_harq_bind *h_bind, const MiDecodeIO &io, uint32_t decoder, uint32_t n_iter)
{
    if (p) {
        if (g->n_alloc > p->cap_bind) { // (a larger plan than any before: the queued runs that read the old blocks finish first)
            MI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
            if (p->d_bind) { (void)hipFree(p->d_bind); p->d_bind = nullptr; }
            if (p->h_bind) { (void)hipHostFree(p->h_bind); p->h_bind = nullptr; }
            p->cap_bind = 0;
            MI_HIP_CHECK(ctx, hipMalloc((void **)&p->d_bind, sizeof(mi_lte_harq_bind) * g->n_alloc));
            MI_HIP_CHECK(ctx, hipHostMalloc((void **)&p->h_bind, sizeof(mi_lte_harq_bind) * g->n_alloc, hipHostMallocDefault));
            p->cap_bind = g->n_alloc;
        }
        MI_HIP_CHECK(ctx, hipEventSynchronize(p->staged)); // the previous run's binding copy has left the staging block
        memcpy(p->h_bind, h_bind, sizeof(mi_lte_harq_bind) * g->n_alloc);
        MI_HIP_CHECK(ctx, hipMemcpyAsync(p->d_bind, p->h_bind, sizeof(mi_lte_harq_bind) * g->n_alloc, hipMemcpyHostToDevice, ctx->stream));
        MI_HIP_CHECK(ctx, hipEventRecord(p->staged, ctx->stream));
    }
    MI_LAUNCH(ctx, "k_dl3_desc", k_dl3_desc, dim3((g->n_slot + 255) / 256), dim3(256), 0, (const Dl3Slot *)g->d_slot, g->n_slot, io.d_allocs, io.d_e_len,
              g->cfg.N_soft, g->cfg.M_dl_harq, g->n_l, g->d_desc);
    if (p) {
        MI_LAUNCH(ctx, "k_harq_bind", k_harq_bind, dim3((g->n_alloc + 255) / 256), dim3(256), 0, (const Dl3Desc *)g->d_desc, (const uint32_t *)g->d_a_slot,
                  g->n_alloc, (const mi_lte_harq_bind *)p->d_bind, p->d_state, g->d_slot_buf);
        MI_LAUNCH(ctx, "k_harq_rm", k_harq_rm, dim3(g->n_slot), dim3(256), DL3_E_CAP, (const Dl3Desc *)g->d_desc, io.d_e, io.d_e_off, g->d_soft, DL3_E_CAP,
                  (const uint32_t *)g->d_slot_buf, p->d_soft, p->buf_elems);
    } else
        MI_LAUNCH(ctx, "k_dl3_rm_i8", k_dl3_rm_i8, dim3(g->n_slot), dim3(256), DL3_E_CAP, (const Dl3Desc *)g->d_desc, io.d_e, io.d_e_off, g->d_soft, DL3_E_CAP);
    MI_HIP_CHECK(ctx, hipGetLastError());
    for (size_t i = 0; i < g->groups.size(); i++) {
        const MiKGroup &gr = g->groups[i];
        const int8_t   *s  = g->d_soft + g->g_soft[i];
        uint8_t        *b  = g->d_bits + g->g_bits[i];
        const int rc = decoder == MI_LTE_TURBO_BCJR_BLOCK ? mi_turbo_bcjr_block_batch(ctx, s, gr.K, gr.n_cb, n_iter, 1, b)
                                                          : mi_turbo_bcjr_batch(ctx, s, gr.K, gr.n_cb, n_iter, 1, b, decoder == MI_LTE_TURBO_BCJR_EARLY);
        if (rc != MI_LTE_OK) return rc;
    }
    MI_LAUNCH(ctx, "k_dl3_cb_finish", k_dl3_cb_finish, dim3(g->n_slot), dim3(256), 0, (const Dl3Desc *)g->d_desc, (const uint8_t *)g->d_bits,
              (const uint32_t *)g->d_tab, (const uint32_t *)(g->d_tab + 6144), io.d_out_bits, io.out_stride, io.packed ? 1u : 0u, g->d_part, g->d_ok, (const int8_t *)g->d_soft);
    MI_LAUNCH(ctx, "k_dl3_tb_finish", k_dl3_tb_finish, dim3((g->n_alloc + 255) / 256), dim3(256), 0, (const uint32_t *)g->d_a_slot,
              (const uint32_t *)g->d_a_nc, g->n_alloc, (const uint32_t *)g->d_part, (const uint32_t *)g->d_ok, io.d_status, g->d_cb_ok);
    if (p)
        MI_LAUNCH(ctx, "k_harq_commit", k_harq_commit, dim3((g->n_alloc + 255) / 256), dim3(256), 0, (const mi_lte_harq_bind *)p->d_bind, g->n_alloc,
                  (const int32_t *)io.d_status, p->d_state);
    MI_HIP_CHECK(ctx, hipGetLastError());
    // (its own kernels: the caller lists its demodulator in front)
    ctx->last_kernels = p ? "k_dl3_desc:1,k_harq_bind:1,k_harq_rm:1,k_bcjr_* per block size,k_dl3_cb_finish:1,k_dl3_tb_finish:1,k_harq_commit:1"
                          : "k_dl3_desc:1,k_dl3_rm_i8:1,k_bcjr_* per block size,k_dl3_cb_finish:1,k_dl3_tb_finish:1";
    return MI_LTE_OK;
}

int mi_dlsch3_cb_soft(const MiDlsch3 *g, uint32_t alloc, const int8_t **d_blocks, uint32_t *C, uint32_t *K)
{
    if (!g || alloc >= g->n_alloc || !d_blocks || !C || !K) return MI_LTE_ERR_INVALID_ARG;
    *d_blocks = g->d_soft + g->a_soft[alloc];
    *C = g->a_nc[alloc];
    *K = g->a_K[alloc];
    return MI_LTE_OK;
}

const uint32_t *mi_dlsch3_cb_ok(const MiDlsch3 *g) { return g ? g->d_cb_ok : nullptr; }
