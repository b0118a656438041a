// The tail-biting convolutional decoder of the 3GPP modes (include/mi_lte.h: CQI section, step 2b), one copy for every kernel that decodes
// the code of 36.212 5.1.3.1: k_ulsch_cqi_decode (ulsch_cqi.hip) and k_pdcch_search_decode (pdcch.hip).  One wavefront per code word, one of
// the 64 states (c_k-1 .. c_k-6, newest bit on top) per lane, integers throughout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

__device__ __forceinline__ int32_t wave_sum(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the three output bits (bit x: generator x) of the register reg = (c_k, c_k-1 .. c_k-6), c_k at bit 6
__device__ __forceinline__ uint32_t conv_label(uint32_t reg)
{
    return ((uint32_t)__popc(reg & 0133u) & 1u) | (((uint32_t)__popc(reg & 0171u) & 1u) << 1) | (((uint32_t)__popc(reg & 0165u) & 1u) << 2);
}

__device__ __forceinline__ int32_t correlate3(uint32_t lab, int32_t d0, int32_t d1, int32_t d2)
{
    return ((lab & 1u) ? -d0 : d0) + ((lab & 2u) ? -d1 : d1) + ((lab & 4u) ? -d2 : d2);
}

// d[3 L] (LDS, complete and visible to the wavefront) -> the decided bits c_0 .. c_(L-1) in cb[] and the correlation of their code word with d
// (on every lane).  Maximum-correlation Viterbi over three laps of the L-step ring, all metrics starting at 0.  Lane n's predecessors are
// 2 (n & 31) and 2 (n & 31) + 1; the odd one survives only when strictly larger; one ballot of survivors per step goes to surv[3 L].  End
// state: the first maximum in state order.  Lane 0 traces back all 3 L steps and keeps the middle lap's bits.  sync() makes the wavefront's
// LDS writes visible to all its lanes: a workgroup of one wavefront passes its barrier, a wavefront among several its own fence.
template <typename Sync>
__device__ __forceinline__ void tbcc_decode(const int32_t *d, uint32_t L, uint64_t *surv, uint8_t *cb, uint32_t ln, Sync sync, int32_t &metric)
{
    // three laps; lane = the state after the step, its input bit is ln >> 5
    const uint32_t lab0 = conv_label(((ln >> 5) << 6) | ((2 * ln) & 63u)), lab1 = conv_label(((ln >> 5) << 6) | ((2 * ln + 1) & 63u));
    int32_t        pm = 0;
    for (uint32_t t = 0, i = 0; t < 3 * L; t++) {
        const int32_t d0 = d[3 * i], d1 = d[3 * i + 1], d2 = d[3 * i + 2];
        const int32_t c0 = __shfl(pm, (2 * ln) & 63, 64) + correlate3(lab0, d0, d1, d2);
        const int32_t c1 = __shfl(pm, (2 * ln + 1) & 63, 64) + correlate3(lab1, d0, d1, d2);
        const bool    odd = c1 > c0; // (a tie keeps the even predecessor)
        const uint64_t m  = __ballot(odd);
        if (ln == 0) surv[t] = m;
        pm = odd ? c1 : c0;
        i  = i + 1 == L ? 0 : i + 1;
    }
    int32_t  best = pm;
    uint32_t st   = ln;
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t  ob = __shfl_xor(best, o, 64);
        const uint32_t os = __shfl_xor(st, o, 64);
        if (ob > best || (ob == best && os < st)) { best = ob; st = os; }
    }
    sync();
    if (ln == 0) { // (the survivor words do not depend on the state walked: their loads run ahead of the chain)
        uint32_t cur = st;
#pragma unroll 8
        for (int t = (int)(3 * L) - 1; t >= 0; t--) {
            if ((uint32_t)t >= L && (uint32_t)t < 2 * L) cb[(uint32_t)t - L] = (uint8_t)(cur >> 5);
            cur = 2 * (cur & 31u) + (uint32_t)((surv[t] >> cur) & 1ull);
        }
    }
    sync();
    // the decided bits re-encoded against d
    metric = 0;
    for (uint32_t i = ln; i < L; i += 64) {
        uint32_t reg = 0;
#pragma unroll
        for (uint32_t j = 0; j < 7; j++) reg |= (uint32_t)cb[i >= j ? i - j : i + L - j] << (6 - j);
        metric += correlate3(conv_label(reg), d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    }
    metric = wave_sum(metric);
}

} // namespace
