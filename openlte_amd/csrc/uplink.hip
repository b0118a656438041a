// PUSCH receive chain on gfx950 (BASELINE config 5): restates liblte_phy_pusch_channel_decode
// (liblte/src/liblte_phy.cc:2801-2935) -> ulsch_channel_decode (:12363-12501) for a batch of allocations
// (one per scheduled UE) inside the envelope the reference itself handles: single antenna, one codeword,
// no RI/ACK/CQI multiplexing, one code block per transport block.
//
//   k_pusch_demod : one workgroup per allocation.
//       DMRS least-squares estimate on symbols 3 and 10 and magnitude/phase interpolation over the 12
//       data symbols (get_ulsch_ce :13718-13790), one-tap equaliser (pre_decoder_and_matched_filter_ul
//       :6708-6736), transform pre-decoding = 12 unnormalised backward DFTs of size M = 12*N_prb times
//       sqrt(M) (:6627-6660; the reference's scaling is reproduced as is), modulation de-mapping, descrambling
//       (:2893-2898) and the channel de-interleaver, which without control bits is the transpose
//       g[(k*12 + s)*Q_m + q] = h[(s*M + k)*Q_m + q] (:12108-12225).  M is any size FFTW would plan
//       (N_prb divisible by 2, 3 or 5 -> radices 4, 2, 3, 5 and whatever prime is left), done as a
//       mixed-radix Stockham transform through LDS.
//   then the downlink's turbo stage (turbo.hip) with the UL-SCH rate-matching rule (N_cb = K_w).
//
// The 3GPP transport-block mode (mi_lte_pusch_plan_create_3gpp, include/mi_lte.h) is the same chain as 36.211 / 36.212 specify it: the
// pre-decoder's output times 1 / sqrt(M) (36.211 5.3.3; k_pusch_demod<.., SPEC = true>), so that 16QAM and 64QAM de-map and QPSK keeps its
// soft information, and transport blocks of 1 .. 13 code blocks through dlsch3gpp.hip's kernels with N_cb = K_w (36.212 5.2.2).  With control
// information (mi_lte_pusch_plan_create_3gpp_uci) ulsch_uci.hip's two kernels run between the demodulator, which is the same, and the code blocks,
// and behind them, opt-in (mi_lte_pusch_plan_set_cqi_decode), ulsch_cqi.hip's CQI decoder.
//
// The DFT sizes are not powers of two and FFTW's operation order is unspecified, so like the downlink FFT
// this stage is tolerance-checked; everything from the int8 soft bits on is integer-exact.
#include <algorithm>

#include <type_traits>

#include <cstring>
#include "plan_core.hpp"
#include "phy_dev.hpp"
#include "ulsch_uci.h"
#include "demap_llr.h"
#include "pusch_launch.h"
#include "pusch_plan.h"

using namespace pusch_geom; // EST_ROWS, the LLR block's sizes, PUSCH_THREADS and the launch rule

namespace {

constexpr int N_SC_MAX = 1200;

// The transform pre-decoding of an allocation of N_prb resource blocks, M = 12 N_prb: the radices of its Stockham passes in the order they
// run (9, 3, 5, 8, 4, 2, then the primes that are left) with each pass's sizes, sqrt(M) as the reference forms it (liblte_phy.cc:6644: integer
// argument -> double sqrt, stored to float) and the reciprocals the index arithmetic divides by.  One row per N_prb, made once per context on
// the host (pusch_shapes below): forming them in the kernel -- a double-precision square root, a dozen 32-bit divisions of workgroup-uniform
// values that have no scalar instruction and so run on the vector unit, the radix search -- was 11 % of its vector instructions at 6 PRB.
constexpr uint32_t MAX_PASSES = 6;
struct DftPass {
    uint32_t R, Ns, nb, tstride; // radix, product of the radices before it, M / R, M / (Ns R)
    float    r_nb, r_ns;         // reciprocals for quot() below
};
struct PuschShape {
    float    sqrt_M, r_M;
    uint32_t n_pass;
    float    r_sqrt_M; // (float)(1 / sqrt((double)M)): the 3GPP mode's scale (36.211 5.3.3)
    DftPass  pass[MAX_PASSES];
};
static_assert(sizeof(PuschShape) == 160, "one row = 40 words");
constexpr uint32_t N_SHAPES = 111; // N_prb 0 .. 110

// floor(n / d) for n < 2^20 as the truncated float product n * r, r = the float next above or equal to 1 / d (recip_up on the host):
// n r >= n / d, so a multiple of d never lands below its quotient (the quotient is representable and rounding is monotonic), and the excess
// n / d * 2^-22 stays under the 1 / d that separates n / d from the next integer while n < 2^22.  Three full-rate instructions where
// v_mul_hi_u32 issues at a quarter of the rate.
__device__ __forceinline__ uint32_t quot(uint32_t n, float r) { return (uint32_t)((float)n * r); }

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmuli(float2 a) { return make_float2(-a.y, a.x); } // a * i

// R-point backward DFTs in registers: v[q] <- sum_r v[r] exp(+2*pi*i * r*q/R).
__device__ __forceinline__ void dft3(float2 &a, float2 &b, float2 &c)
{
    const float  h3 = 0.86602540378443864676f; // sin(2 pi / 3)
    const float2 s = cadd(b, c), d = csub(b, c);
    const float2 m = make_float2(a.x - 0.5f * s.x, a.y - 0.5f * s.y), n = make_float2(-h3 * d.y, h3 * d.x);
    a = cadd(a, s);
    b = cadd(m, n);
    c = csub(m, n);
}
__device__ __forceinline__ void dft4(float2 &a, float2 &b, float2 &c, float2 &d)
{
    const float2 s02 = cadd(a, c), d02 = csub(a, c), s13 = cadd(b, d), d13 = cmuli(csub(b, d));
    a = cadd(s02, s13);
    b = cadd(d02, d13);
    c = csub(s02, s13);
    d = csub(d02, d13);
}
template <uint32_t R> __device__ __forceinline__ void butterfly(float2 (&v)[R]);
template <> __device__ __forceinline__ void butterfly<2>(float2 (&v)[2])
{
    const float2 a = v[0];
    v[0] = cadd(a, v[1]);
    v[1] = csub(a, v[1]);
}
template <> __device__ __forceinline__ void butterfly<3>(float2 (&v)[3]) { dft3(v[0], v[1], v[2]); }
template <> __device__ __forceinline__ void butterfly<4>(float2 (&v)[4]) { dft4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ void butterfly<5>(float2 (&v)[5])
{
    const float  c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f; // cos(2 pi / 5), cos(4 pi / 5)
    const float  s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;  // sin(2 pi / 5), sin(4 pi / 5)
    const float2 a1 = cadd(v[1], v[4]), d1 = csub(v[1], v[4]), a2 = cadd(v[2], v[3]), d2 = csub(v[2], v[3]);
    const float2 m1 = make_float2(v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y);
    const float2 m2 = make_float2(v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y);
    const float2 n1 = cmuli(make_float2(s1 * d1.x + s2 * d2.x, s1 * d1.y + s2 * d2.y));
    const float2 n2 = cmuli(make_float2(s2 * d1.x - s1 * d2.x, s2 * d1.y - s1 * d2.y));
    v[0] = cadd(v[0], cadd(a1, a2));
    v[1] = cadd(m1, n1);
    v[2] = cadd(m2, n2);
    v[3] = csub(m2, n2);
    v[4] = csub(m1, n1);
}
template <> __device__ __forceinline__ void butterfly<8>(float2 (&v)[8])
{
    // even outputs from v[r] + v[r+4], odd ones from (v[r] - v[r+4]) * exp(+2*pi*i * r/8), a 4-point transform of each
    const float r2 = 0.70710678118654752440f;
    float2      a[4], b[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) { a[r] = cadd(v[r], v[r + 4]); b[r] = csub(v[r], v[r + 4]); }
    b[1] = make_float2(r2 * (b[1].x - b[1].y), r2 * (b[1].x + b[1].y));
    b[2] = cmuli(b[2]);
    b[3] = make_float2(-r2 * (b[3].x + b[3].y), r2 * (b[3].x - b[3].y));
    dft4(a[0], a[1], a[2], a[3]);
    dft4(b[0], b[1], b[2], b[3]);
#pragma unroll
    for (uint32_t p = 0; p < 4; p++) { v[2 * p] = a[p]; v[2 * p + 1] = b[p]; }
}
template <> __device__ __forceinline__ void butterfly<9>(float2 (&v)[9])
{
    // r = r1 + 3 r2, q = 3 q1 + q2: 3-point transforms over r2, the twiddles exp(+2*pi*i * r1*q2/9), 3-point transforms over r1
    const float2 w1 = make_float2(0.76604444311897803520f, 0.64278760968653932632f);  // exp(2 pi i / 9)
    const float2 w2 = make_float2(0.17364817766693034885f, 0.98480775301220805937f);  // exp(4 pi i / 9)
    const float2 w4 = make_float2(-0.93969262078590838405f, 0.34202014332566873304f); // exp(8 pi i / 9)
    dft3(v[0], v[3], v[6]); // r1 = 0: results indexed by q2 in v[0], v[3], v[6]
    dft3(v[1], v[4], v[7]); // r1 = 1
    dft3(v[2], v[5], v[8]); // r1 = 2
    v[4] = cmul(v[4], w1); v[7] = cmul(v[7], w2); // r1 = 1: q2 = 1, 2
    v[5] = cmul(v[5], w2); v[8] = cmul(v[8], w4); // r1 = 2: q2 = 1, 2
    dft3(v[0], v[1], v[2]); // q2 = 0: outputs q = 0, 3, 6
    dft3(v[3], v[4], v[5]); // q2 = 1: outputs q = 1, 4, 7
    dft3(v[6], v[7], v[8]); // q2 = 2: outputs q = 2, 5, 8
    const float2 t1 = v[1], t2 = v[2], t3 = v[3], t5 = v[5], t6 = v[6], t7 = v[7];
    v[1] = t3; v[2] = t6; v[3] = t1; v[5] = t7; v[6] = t2; v[7] = t5; // v[3*q2 + q1] -> v[3*q1 + q2]
}

// One Stockham pass of radix R in {2, 3, 4, 5, 8, 9} over S symbols of M points each (symbol s at in + s*M_max), sign +1 (backward
// transform), one thread per butterfly:
//   out[(j-k)*R + k + q*Ns] = sum_r in[j + r*M/R] * w^(r*k) * exp(+2*pi*i * r*q/R),  k = j mod Ns,  w = exp(+2*pi*i / (Ns*R)),
// the twiddle w^(r*k) being entry r*k*M/(Ns*R) (< M) of the allocation's table tw[t] = exp(+2*pi*i*t/M).
template <uint32_t R, uint32_t THREADS>
__device__ __forceinline__ void dft_pass_r(const float2 *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ tw,
                                           uint32_t S, uint32_t M_max, const DftPass ps)
{
    const uint32_t nb = ps.nb, Ns = ps.Ns, tstride = ps.tstride;
    for (uint32_t o = threadIdx.x; o < S * nb; o += THREADS) {
        const uint32_t sy = quot(o, ps.r_nb), j = o - __umul24(sy, nb), k = Ns > 1 ? j - __umul24(quot(j, ps.r_ns), Ns) : 0;
        const float2  *x = in + __umul24(sy, M_max) + j;
        float2         v[R];
#pragma unroll
        for (uint32_t r = 0; r < R; r++) v[r] = x[r * nb];
        if (Ns > 1) { // uniform; the first pass has k = 0 throughout
            const uint32_t t = __umul24(k, tstride);
#pragma unroll
            for (uint32_t r = 1; r < R; r++) v[r] = cmul(v[r], tw[r * t]);
        }
        butterfly<R>(v);
        float2 *y = out + __umul24(sy, M_max) + __umul24(j - k, R) + k;
#pragma unroll
        for (uint32_t q = 0; q < R; q++) y[q * Ns] = v[q];
    }
}

// The same pass for any other radix (the prime FFTW would be left with when N_prb has a factor >= 7), one thread per output:
// step = (k + q*Ns) * M/(Ns*R) < M, twiddle index r*step mod M.
template <uint32_t THREADS>
__device__ __forceinline__ void dft_pass(const float2 *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ tw,
                                         uint32_t S, uint32_t M, float r_M, uint32_t M_max, const DftPass ps)
{
    const uint32_t R = ps.R, nb = ps.nb, Ns = ps.Ns, tstride = ps.tstride;
    for (uint32_t o = threadIdx.x; o < S * M; o += THREADS) {
        const uint32_t sy = quot(o, r_M), oo = o - sy * M;
        const uint32_t q = quot(oo, ps.r_nb), j = oo - q * nb, k = j - quot(j, ps.r_ns) * Ns, step = (k + q * Ns) * tstride;
        const float2  *x = in + sy * M_max + j;
        float    ar = 0.0f, ai = 0.0f;
        uint32_t t  = 0; // r*step mod M
        for (uint32_t r = 0; r < R; r++) {
            const float2 w = tw[t], v = x[r * nb];
            ar += v.x * w.x - v.y * w.y;
            ai += v.x * w.y + v.y * w.x;
            t += step;
            if (t >= M) t -= M;
        }
        out[sy * M_max + (j - k) * R + k + q * Ns] = make_float2(ar, ai);
    }
}

#ifndef WPE
#define WPE 6
#endif
// THREADS = the workgroup's width as a compile-time constant (64 / 128 / 192 / 256): every phase is a loop `o += THREADS` -- with blockDim.x the
// stride was re-read from the dispatch packet in every iteration of the de-mapper's loop (a store in the body could alias it as far as the
// compiler knows) -- and the index products are 24-bit multiplies (v_mul_lo_u32 / v_mad_u64_u32 issue at a quarter of the rate)
// SPEC = the 3GPP mode's demodulator (mi_lte_pusch_plan_create_3gpp): the pre-decoder's output scaled by 1 / sqrt(M) as 36.211 5.3.3 has it,
// where the reference -- and SPEC = false -- multiplies by sqrt(M).  One factor; everything else is the same code.
// LA = the variant: the kernel's last argument is one of the blocks below, whose constants say what the kernel does with it.  A constant
// that is off drops its `if constexpr` sections out, and with N_RX = 1 each antenna loop has one trip.
//   block                 launched as              what it adds; its LDS behind the scrambling words
//   PuschNoLlr            k_pusch_demod            nothing (demap_symbol's soft bits); none
//   PuschLlr              k_pusch_demod_llr        LLR, the max-log de-mapper (MI_LTE_DEMAP_MAXLOG): a pass over the LDS-resident estimates forms the
//                                                  twelve rho_s = M / sum_k hn_k(s) and the gain before the symbol-group loop (the automatic gain needs
//                                                  them all); the de-mapper writes clamp(rint(g L)) (demap_llr.h).  wsum[4][12] (double) | rho[12] (float)
//   PuschLlrNoise         k_pusch_demod_llr        NOISE (mi_lte_pusch_plan_set_llr_noise): a pass in front of the rho pass, the second differences of
//                                                  the two DMRS rows, gives sigma2, and g = noise / sigma2.  PuschLlr's | nsum[4] (double)
//   PuschLlrRx<N, NOISE>  k_pusch_demod_llr_rx     N_RX = 2 or 4 (mi_lte_pusch_plan_set_rx_antennas): antenna r of unit u is subframe r ant_stride + u,
//                                                  every pass loops over the antennas and the equaliser forms z = (sum_r y_r conj(h_r)) / sum_r |h_r|^2.
//                                                  NOISE = false leaves noise and s2_out unused.  PuschLlrNoise's, behind N_RX sets of estimate rows
//   PuschLlrMmse<N>       k_pusch_demod_llr_mmse   MMSE and NOISE, N_RX = 1, 2 or 4 (mi_lte_pusch_plan_set_equaliser): sigma2 is reduced behind a barrier
//                                                  of its own; the rho pass sums q = 1 / (P + sigma2) in place of hn = 1 / P and finishes with nu_s =
//                                                  sigma2 mean(q), w_s = (1 - nu_s) / nu_s; the equaliser multiplies by q, the de-mapper takes t = x / nu_s
//                                                  and w_s, the gain is the noise setter's scale.  PuschLlrNoise's: nu_s in rho's floats, w_s in wsum's
//                                                  first twelve doubles, which their finishing threads have read by then
// Every sum of these passes is in double and in a fixed order (thread, xor butterfly in the wavefront, the wavefronts' LDS slots ascending;
// antennas ascending) and there are no atomics: two runs give the same bytes.  The blocks stay separate types, fields in this order: a
// superset struct would move ant_stride and nu_out in the kernel argument segment.
struct PuschNoLlr {
    static constexpr PuschFamily FAMILY = PuschFamily::PLAIN;
    static constexpr bool LLR = false, NOISE = false, MMSE = false; static constexpr uint32_t N_RX = 1;
};
struct PuschLlr {
    static constexpr PuschFamily FAMILY = PuschFamily::LLR;
    static constexpr bool LLR = true, NOISE = false, MMSE = false; static constexpr uint32_t N_RX = 1;
    float           gain, auto_t; // gain > 0: fixed; 0: automatic, g = auto_t / (4 A^2 mean rho)
    uint32_t        lds_off;      // float offset in the dynamic LDS of wsum[4][12] (double) | rho[12] (float)
    float          *g_out, *rho_out; // [n_alloc], [n_alloc][12]: the taps
    float2         *x_tap;        // the symbol tap (mi_lte_pusch_plan_set_llr_tap) or NULL
    const uint32_t *x_off;        // [n_alloc]: float2 offset of the allocation's 12 M symbols in x_tap
};
struct PuschLlrNoise : PuschLlr {
    static constexpr PuschFamily FAMILY = PuschFamily::LLR_NOISE;
    static constexpr bool NOISE = true;
    float  noise;  // g = noise / sigma2 of the DMRS noise estimate in place of either gain of PuschLlr
    float *s2_out; // [n_alloc]: the sigma2 tap
};
template <uint32_t N, bool NOISE_>
struct PuschLlrRx : PuschLlrNoise {
    static constexpr PuschFamily FAMILY = PuschFamily::LLR_RX;
    static constexpr bool NOISE = NOISE_; static constexpr uint32_t N_RX = N;
    uint32_t ant_stride; // subframes between the grids of antennas r and r + 1 of one unit
};
template <uint32_t N>
struct PuschLlrMmse : PuschLlrNoise {
    static constexpr PuschFamily FAMILY = PuschFamily::LLR_MMSE;
    static constexpr bool MMSE = true; static constexpr uint32_t N_RX = N;
    float   *nu_out;     // [n_alloc][12]: the nu tap
    uint32_t ant_stride; // as PuschLlrRx's; unused for N = 1
};

// h(s) of data symbol sp (0 .. 5) of a slot and hn = 1 / |h|^2 as the one-tap equaliser uses it, from the slot's DMRS estimate: magnitude and
// slope, u = exp(i ang_b), f1 .. f3 = exp(i n f_ang) for n = 1, 2, 3 (liblte_phy.cc:13770-13780: symbols 0-2 / 3-5 of a slot lie -3..-1 /
// +1..+3 steps from its DMRS symbol, symbol 3 of 7)
__device__ __forceinline__ void slot_h(float mag, float f_mag, float2 u, float2 f1, float2 f2, float2 f3, uint32_t sp, float &h_re, float &h_im, float &hn)
{
    const int    n = sp < 3 ? (int)sp - 3 : (int)sp - 2;
    const float2 fa = n == 1 || n == -1 ? f1 : n == 2 || n == -2 ? f2 : f3;
    const float2 f = make_float2(fa.x, n < 0 ? -fa.y : fa.y);
    const float  cm = mag + (float)n * f_mag;
    const float2 ph = cmul(u, f);
    h_re = cm * ph.x; h_im = cm * ph.y;
    hn = 1.0f / (h_re * h_re + h_im * h_im);
}

// sigma2 of the noise pass from its wavefronts' sums: S = nsum[0] + nsum[1] + .. in this order, over the 120 N_prb second differences an
// antenna contributes (2 slots x 10 N_prb terms of 6 sigma^2 each) and, combining, the antennas' mean: MRC assumes equal noise power per
// antenna.  Every thread forms the same sum in the same order.
template <uint32_t THREADS, uint32_t N_RX>
__device__ __forceinline__ float noise_sigma2(const double *nsum, uint32_t N_prb)
{
    double S = nsum[0];
    for (uint32_t w = 1; w < THREADS / 64; w++) S += nsum[w];
    if constexpr (N_RX > 1) return (float)(S / (120.0 * (double)N_prb * (double)N_RX));
    else return (float)(S / (120.0 * (double)N_prb));
}

#ifndef WPE_LLR
#define WPE_LLR 4
#endif

template <uint32_t THREADS, bool SPEC = false, typename LA = PuschNoLlr>
// (four antennas: the equaliser item carries four sets of estimates and grid values for six symbols, and the LDS of such a launch keeps the
// occupancy under 4 from 10 PRB on anyway -- 3 waves per SIMD, 168 registers, in place of a spill)
__attribute__((amdgpu_waves_per_eu(LA::N_RX == 4 ? 3 : LA::LLR ? WPE_LLR : WPE, 8)))
__global__ __launch_bounds__(THREADS) void k_pusch_demod(const float *__restrict__ subframes, uint32_t sf_stride,
                                                     const mi_lte_pdsch_alloc *__restrict__ allocs, const PuschDesc *__restrict__ desc,
                                                     const float *__restrict__ dmrs_pool, GoldTables gt, int8_t *__restrict__ e_base,
                                                     const uint32_t *__restrict__ e_off, uint32_t *__restrict__ e_len, uint32_t M_max,
                                                     uint32_t S_par, float r_S_par, const PuschShape *__restrict__ shapes, [[maybe_unused]] const LA la)
{
    constexpr bool LLR = LA::LLR, NOISE = LA::NOISE, MMSE = LA::MMSE; constexpr uint32_t N_RX = LA::N_RX; // the variant, as its block declares it
    static_assert(!LLR || SPEC, "the max-log de-mapper belongs to the 3GPP mode");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    // LDS: est[N_RX][9][M_max] (mag0 mag1 dmag | unit vectors of ang0, ang1, dang; one set per antenna) | tw[M_max] | buf A[S_par][M_max] |
    // buf B[S_par][M_max] (float2) | scrambling words
    float    *est  = sm;
    float2   *tw   = reinterpret_cast<float2 *>(sm + N_RX * EST_ROWS * (size_t)M_max);
    float2   *bufA = tw + M_max, *bufB = bufA + (size_t)S_par * M_max;
    uint32_t *cw   = reinterpret_cast<uint32_t *>(bufB + (size_t)S_par * M_max);

    const uint32_t a_idx = blockIdx.x;
    const mi_lte_pdsch_alloc &al = allocs[a_idx];
    const PuschDesc           ds = desc[a_idx];
    const uint32_t N_prb = al.N_prb, M = 12 * N_prb;
    const PuschShape &sh = shapes[N_prb]; // (uniform: scalar loads)
    const uint32_t Qm = al.mod_type == 3 ? 6 : al.mod_type == 2 ? 4 : al.mod_type == 1 ? 2 : 1;
    const uint32_t N_bits = 12 * M * Qm;
    const float   *rx_re = subframes + (size_t)al.unit * sf_stride, *rx_im = rx_re + 16 * N_SC_MAX;
    [[maybe_unused]] size_t ant_floats = 0; // from the grid of antenna r of a unit to that of antenna r + 1
    if constexpr (N_RX > 1) ant_floats = (size_t)la.ant_stride * sf_stride;
    if (threadIdx.x == 0) e_len[a_idx] = N_bits;

    // scrambling sequence (c_init per liblte_phy.cc:2893), one word of slack for the 2-word window below
    const uint32_t c_init = (al.rnti << 14) | (0u << 13) | (ds.subfr << 9) | ds.cell, n_words = (N_bits + 31) / 32;
    for (uint32_t w = threadIdx.x; w <= n_words; w += THREADS) cw[w] = gold_word(gt, c_init, w);

    // ---- DMRS estimates and their interpolation slopes (get_ulsch_ce, liblte_phy.cc:13745-13768); DFT twiddles.
    // The reference interpolates in polar form, h(s) = (mag_b + n f_mag) exp(i (ang_b + n f_ang)), n = -3..3 around DMRS symbol b:
    // what is kept per subcarrier is exp(i ang_b) = t_b / |t_b| and exp(i f_ang), so the 12 data symbols cost complex products,
    // not 12 sin/cos pairs.  Work is spread as (subcarrier, task): task 0/1 = DMRS symbol 0/1, task 2 = the twiddle.
    const float *d_pool = dmrs_pool + ds.dmrs_off; // dmrs_0_re | dmrs_0_im | dmrs_1_re | dmrs_1_im (M each)
    // With N_RX antennas the items are (subcarrier, 2 r + b) for antenna r, then the twiddle.
    for (uint32_t o = threadIdx.x; o < (2 * N_RX + 1) * M; o += THREADS) {
        uint32_t task, i, r = 0;
        if constexpr (N_RX == 1) { task = o >= 2 * M ? 2 : o >= M ? 1 : 0; i = o - task * M; }
        else {
            const uint32_t q = quot(o, sh.r_M);
            i = o - __umul24(q, M); r = q >> 1; task = q >= 2 * N_RX ? 2 : q & 1u;
        }
        float       *er = est + r * (EST_ROWS * M_max); // antenna r's nine rows
        const float *ar_re = rx_re + r * ant_floats, *ar_im = rx_im + r * ant_floats; // and its grid
        if (task == 2) {
            float sn, cs;
            sincospif(2.0f * (float)i / (float)M, &sn, &cs);
            tw[i] = make_float2(cs, sn);
        } else {
            const uint32_t rb = __umul24(i, 10923u) >> 17; // i / 12 for i < 1536
            const uint32_t sc = al.prb[task][rb] * 12 + (i - 12 * rb), L = task ? 10 : 3;
            const float    cr = ar_re[L * N_SC_MAX + sc], ci = ar_im[L * N_SC_MAX + sc];
            const float    dr = d_pool[2 * task * M + i], di = d_pool[(2 * task + 1) * M + i];
            const float    t_re = cr * dr + ci * di, t_im = ci * dr - cr * di;
            const float    mag = sqrtf(t_re * t_re + t_im * t_im);
            er[task * M_max + i] = mag;
            er[(3 + 2 * task) * M_max + i] = mag > 0.0f ? t_re / mag : 1.0f; // atan2f(0, 0) = 0
            er[(4 + 2 * task) * M_max + i] = mag > 0.0f ? t_im / mag : 0.0f;
            if (task == 0) er[8 * M_max + i] = atan2f(t_im, t_re);
            else           er[2 * M_max + i] = atan2f(t_im, t_re); // parked in the rows the second step overwrites
        }
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < N_RX * M; o += THREADS) { // (antenna, subcarrier)
        uint32_t i = o, r = 0;
        if constexpr (N_RX > 1) { r = quot(o, sh.r_M); i = o - __umul24(r, M); }
        float      *er = est + r * (EST_ROWS * M_max);
        const float f_mag = (er[M_max + i] - er[i]) / 7;
        float       f_ang = er[2 * M_max + i] - er[8 * M_max + i];
        if ((double)f_ang >= M_PI) f_ang = (float)((double)f_ang - 2 * M_PI); // float compared / corrected in double (:13758-13764)
        else if ((double)f_ang <= -M_PI) f_ang = (float)((double)f_ang + 2 * M_PI);
        f_ang /= 7;
        float sn, cs;
        sincosf(f_ang, &sn, &cs);
        er[2 * M_max + i] = f_mag; er[7 * M_max + i] = cs; er[8 * M_max + i] = sn;
    }
    __syncthreads();

    // liblte_phy.cc:6644 (integer argument -> double sqrt, stored to float: formed on the host), or its reciprocal for the 3GPP mode
    const float scale = SPEC ? sh.r_sqrt_M : sh.sqrt_M;
    int8_t     *e      = e_base + (size_t)e_off[a_idx] * 64; // 64-byte units

    // ---- LLR: rho_s = M / sum_k hn_k(s) for all twelve data symbols, then the gain -- before the first soft bit of the first symbol group
    // is written (the automatic gain needs every rho_s, and S_par < 12 above M = 213).  hn is the equaliser's own float (slot_h); the sum is
    // in double and in a fixed order: each thread over its sub-carriers i = t, t + THREADS, .., then the xor butterfly inside the wavefront,
    // then the wavefronts' LDS slots in ascending order.  No atomics: two runs give the same bytes.
    [[maybe_unused]] const float *rho = nullptr;
    [[maybe_unused]] double       gd  = 0.0;
    [[maybe_unused]] float         s2_m = 0.0f;     // MMSE: sigma2, in every thread, from the reliability pass on
    [[maybe_unused]] const double *w_m  = nullptr; // MMSE: w_s of the twelve symbols
    if constexpr (LLR) {
        double *wsum  = reinterpret_cast<double *>(sm + la.lds_off); // [THREADS / 64][12]
        float  *rho_w = reinterpret_cast<float *>(wsum + 4 * 12);
        [[maybe_unused]] double *nsum = reinterpret_cast<double *>(rho_w + 12); // [THREADS / 64]: PuschLlrNoise's launch alone has them
        // ---- noise estimate (only in the noise-referenced instantiation): t_b[i] = mag_b[i] u_b[i] is the least-squares product of
        // sub-carrier i on DMRS symbol b, from the rows the slope step left alone.  Inside a resource block (i mod 12 = 1 .. 10, so a PRB
        // list with gaps needs no special case) the second difference t[i-1] - 2 t[i] + t[i+1] removes a channel that is linear over three
        // sub-carriers and leaves 6 sigma^2 of white noise: S = sum |d|^2 over 2 slots x 10 N_prb terms, in double and in the rho pass's
        // fixed order (thread, xor butterfly, wavefront slots; the slots are read behind the rho pass's first barrier).
        if constexpr (NOISE) {
            // With N_RX antennas S = sum_r S_r, antenna by antenna in this order (the mean over the antennas is taken where sigma2 is formed).
            double part = 0.0;
#pragma unroll
            for (uint32_t r = 0; r < N_RX; r++)
            for (uint32_t b = 0; b < 2; b++) {
                const float *er = est + r * (EST_ROWS * M_max);
                const float *mg = er + b * M_max, *ur = er + (3 + 2 * b) * M_max, *ui = er + (4 + 2 * b) * M_max;
                for (uint32_t i = threadIdx.x; i < M; i += THREADS) {
                    const uint32_t r = i - 12 * (__umul24(i, 10923u) >> 17); // i mod 12 for i < 1536
                    if (r == 0 || r == 11) continue; // (so i - 1 and i + 1 stay inside the block, and inside 0 .. M - 1)
                    const float m0 = mg[i - 1], m1 = mg[i], m2 = mg[i + 1];
                    const float ar = m0 * ur[i - 1], ai = m0 * ui[i - 1], br = m1 * ur[i], bi = m1 * ui[i], cr = m2 * ur[i + 1], ci = m2 * ui[i + 1];
                    const double dr = (double)ar - 2.0 * (double)br + (double)cr, di = (double)ai - 2.0 * (double)bi + (double)ci;
                    part += dr * dr + di * di;
                }
            }
            for (int o = 32; o; o >>= 1) part += __shfl_xor(part, o);
            if ((threadIdx.x & 63u) == 0) nsum[threadIdx.x >> 6] = part;
        }
        if constexpr (MMSE) { // sigma2 before the reliability pass, which adds it to every P: the noise section's sum and quotient, in every thread
            __syncthreads();
            s2_m = noise_sigma2<THREADS, N_RX>(nsum, N_prb);
        }
        for (uint32_t b = 0; b < 2; b++) { // slot: six data symbols per pass, so a thread carries six partial sums
            double part[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (uint32_t i = threadIdx.x; i < M; i += THREADS) {
                // (Here and in the equaliser item the combining form stays a branch of its own, not the single-antenna loop with more trips: it
                // sums from 0.0f, and 0.0f + x is not x for x = -0, so one merged loop would change the sign of zeros the symbol tap can show)
                if constexpr (N_RX > 1) { // hn = 1 / P, P = sum_r |h_r|^2 in float with r ascending: the float the combining equaliser multiplies with
                    float P[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (uint32_t r = 0; r < N_RX; r++) {
                        const float *er = est + r * (EST_ROWS * M_max);
                        const float  mag = er[b * M_max + i], f_mag = er[2 * M_max + i];
                        const float2 u = make_float2(er[(3 + 2 * b) * M_max + i], er[(4 + 2 * b) * M_max + i]);
                        const float2 f1 = make_float2(er[7 * M_max + i], er[8 * M_max + i]), f2 = cmul(f1, f1), f3 = cmul(f2, f1);
#pragma unroll
                        for (uint32_t sp = 0; sp < 6; sp++) {
                            float h_re, h_im, hn;
                            slot_h(mag, f_mag, u, f1, f2, f3, sp, h_re, h_im, hn);
                            P[sp] += h_re * h_re + h_im * h_im;
                        }
                    }
#pragma unroll
                    for (uint32_t sp = 0; sp < 6; sp++) {
                        if constexpr (MMSE) part[sp] += (double)(1.0f / (P[sp] + s2_m));
                        else part[sp] += (double)(1.0f / P[sp]);
                    }
                    continue;
                }
                const float    mag = est[b * M_max + i], f_mag = est[2 * M_max + i];
                const float2   u = make_float2(est[(3 + 2 * b) * M_max + i], est[(4 + 2 * b) * M_max + i]);
                const float2   f1 = make_float2(est[7 * M_max + i], est[8 * M_max + i]), f2 = cmul(f1, f1), f3 = cmul(f2, f1);
#pragma unroll
                for (uint32_t sp = 0; sp < 6; sp++) {
                    float h_re, h_im, hn;
                    slot_h(mag, f_mag, u, f1, f2, f3, sp, h_re, h_im, hn);
                    if constexpr (MMSE) part[sp] += (double)(1.0f / ((h_re * h_re + h_im * h_im) + s2_m));
                    else part[sp] += (double)hn;
                }
            }
#pragma unroll
            for (uint32_t sp = 0; sp < 6; sp++) {
                for (int o = 32; o; o >>= 1) part[sp] += __shfl_xor(part[sp], o);
                if ((threadIdx.x & 63u) == 0) wsum[(threadIdx.x >> 6) * 12 + 6 * b + sp] = part[sp];
            }
        }
        __syncthreads();
        if (threadIdx.x < 12) {
            double sum = wsum[threadIdx.x];
            for (uint32_t w = 1; w < THREADS / 64; w++) sum += wsum[w * 12 + threadIdx.x];
            if constexpr (MMSE) { // nu_s, w_s and the taps; rho's float holds nu_s (0: no information) and wsum's column head, read above, w_s
                const float  nu = (float)(sum * (double)s2_m / (double)M);
                const bool   ok = nu > 0.0f && nu < 1.0f; // (false for a NaN)
                const double w  = ok ? (1.0 - (double)nu) / (double)nu : 0.0;
                rho_w[threadIdx.x] = ok ? nu : 0.0f;
                wsum[threadIdx.x]  = w;
                la.nu_out[a_idx * 12 + threadIdx.x]  = nu;
                la.rho_out[a_idx * 12 + threadIdx.x] = (float)((double)s2_m * w);
            } else {
            const float r = (float)((double)M / sum);
            // an infinite or NaN hn makes the sum infinite or NaN; a zero sum the quotient: rho_s = 0 in each case
            const float r_ok = (fabs(sum) <= 1.7976931348623157e308 && fabsf(r) <= 3.4028234e38f) ? r : 0.0f;
            rho_w[threadIdx.x] = r_ok;
            la.rho_out[a_idx * 12 + threadIdx.x] = r_ok;
            }
        }
        __syncthreads();
        rho = rho_w;
        gd  = (double)la.gain;
        if constexpr (MMSE) { // g_a = scale: the 1 / sigma2 is inside w_s.  sigma2 0 or not finite: every soft bit 0
            w_m = wsum;
            gd  = (s2_m > 0.0f && s2_m <= 3.4028234e38f) ? (double)la.noise : 0.0;
            if (threadIdx.x == 0) la.s2_out[a_idx] = s2_m;
        } else if constexpr (NOISE) { // every thread forms the same sum in the same order
            const float s2 = noise_sigma2<THREADS, N_RX>(nsum, N_prb);
            const float gf = (float)((double)la.noise / (double)s2);
            // sigma2 0 or not finite, or a gain past float: every soft bit 0
            gd = (s2 > 0.0f && s2 <= 3.4028234e38f && fabsf(gf) <= 3.4028234e38f) ? (double)gf : 0.0;
            if (threadIdx.x == 0) la.s2_out[a_idx] = s2;
        } else if (la.gain == 0.0f) { // automatic: the mean of the twelve floats in double, s = 0 .. 11 in order
            double rbar = 0.0;
            for (uint32_t s = 0; s < 12; s++) rbar += (double)rho_w[s];
            rbar /= 12.0;
            const double a4 = al.mod_type == 3 ? 4.0 / 42 : al.mod_type == 2 ? 4.0 / 10 : 2.0; // 4 A^2
            const float  gf = (float)((double)la.auto_t / (a4 * rbar));
            gd = (rbar > 0.0 && fabsf(gf) <= 3.4028234e38f) ? (double)gf : 0.0; // rbar 0 or not finite, or a gain past float: every soft bit 0
        }
        if (threadIdx.x == 0) la.g_out[a_idx] = (float)gd;
    }

    for (uint32_t s0 = 0; s0 < 12; s0 += S_par) { // S_par data symbols at a time (all 12 when they fit in LDS)
        const uint32_t S = S_par; // (12, 6, 3, 2 or 1: always a divisor of 12)
        // ---- channel estimate of each symbol and the one-tap equaliser.  One item per (subcarrier, slot): the slot's DMRS
        // estimate, its unit vector and the powers of exp(i f_ang) are fetched / formed once and serve the slot's (up to) six data
        // symbols; S is 12 (both slots) or divides 6 (part of one slot).
        const uint32_t slot0 = s0 >= 6, n_slots = S == 12 ? 2 : 1, sp0 = s0 - 6 * slot0, sp1 = sp0 + (S == 12 ? 6 : S);
        for (uint32_t o = threadIdx.x; o < n_slots * M; o += THREADS) {
            const uint32_t b = slot0 + (o >= M), i = o - (o >= M ? M : 0);
            if constexpr (N_RX > 1) { // z = (sum_r y_r conj(h_r)) (1 / P), P = sum_r |h_r|^2: float sums with r ascending, the item's symbols side by side
                const uint32_t rb = __umul24(i, 10923u) >> 17; // i / 12 for i < 1536
                const uint32_t sc = al.prb[b][rb] * 12 + (i - 12 * rb);
                float2        *dst = bufA + ((int)(6 * b) - (int)s0) * (int)M_max + (int)i;
                float          c_re[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, c_im[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, P[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (uint32_t r = 0; r < N_RX; r++) {
                    const float *er = est + r * (EST_ROWS * M_max);
                    const float  mag = er[b * M_max + i], f_mag = er[2 * M_max + i];
                    const float2 u = make_float2(er[(3 + 2 * b) * M_max + i], er[(4 + 2 * b) * M_max + i]);
                    const float2 f1 = make_float2(er[7 * M_max + i], er[8 * M_max + i]), f2 = cmul(f1, f1), f3 = cmul(f2, f1);
                    const float *z_re = rx_re + r * ant_floats + 7 * b * N_SC_MAX + sc, *z_im = rx_im + r * ant_floats + 7 * b * N_SC_MAX + sc;
#pragma unroll
                    for (uint32_t sp = 0; sp < 6; sp++) {
                        if (sp < sp0 || sp >= sp1) continue; // uniform
                        const uint32_t l = sp < 3 ? sp : sp + 1;
                        float          h_re, h_im, hn;
                        slot_h(mag, f_mag, u, f1, f2, f3, sp, h_re, h_im, hn);
                        const float zr = z_re[l * N_SC_MAX], zi = z_im[l * N_SC_MAX];
                        c_re[sp] += zr * h_re + zi * h_im; c_im[sp] += zi * h_re - zr * h_im;
                        P[sp] += h_re * h_re + h_im * h_im;
                    }
                }
#pragma unroll
                for (uint32_t sp = 0; sp < 6; sp++) {
                    if (sp < sp0 || sp >= sp1) continue; // uniform
                    const float hn = MMSE ? 1.0f / (P[sp] + s2_m) : 1.0f / P[sp];
                    dst[sp * M_max] = make_float2(c_re[sp] * hn, c_im[sp] * hn);
                }
                continue;
            }
            const float    mag = est[b * M_max + i], f_mag = est[2 * M_max + i];
            const float2   u = make_float2(est[(3 + 2 * b) * M_max + i], est[(4 + 2 * b) * M_max + i]);
            const float2   f1 = make_float2(est[7 * M_max + i], est[8 * M_max + i]), f2 = cmul(f1, f1), f3 = cmul(f2, f1);
            const uint32_t rb = __umul24(i, 10923u) >> 17; // i / 12 for i < 1536
            const uint32_t sc = al.prb[b][rb] * 12 + (i - 12 * rb);
            const float   *z_re = rx_re + 7 * b * N_SC_MAX + sc, *z_im = rx_im + 7 * b * N_SC_MAX + sc;
            float2        *dst = bufA + ((int)(6 * b) - (int)s0) * (int)M_max + (int)i; // symbol s = 6 b + sp goes to row s - s0
#pragma unroll
            for (uint32_t sp = 0; sp < 6; sp++) {
                if (sp < sp0 || sp >= sp1) continue; // uniform
                const uint32_t l = sp < 3 ? sp : sp + 1; // position in the slot, skipping the DMRS symbol
                float          h_re, h_im, hn;
                slot_h(mag, f_mag, u, f1, f2, f3, sp, h_re, h_im, hn);
                const float  zr = z_re[l * N_SC_MAX], zi = z_im[l * N_SC_MAX];
                if constexpr (MMSE) hn = 1.0f / ((h_re * h_re + h_im * h_im) + s2_m); // q in place of hn
                dst[sp * M_max] = make_float2((zr * h_re + zi * h_im) * hn, (zi * h_re - zr * h_im) * hn);
            }
        }
        __syncthreads();
        // ---- transform pre-decoding: M-point backward DFTs, radices 9, 3, 5, 8, 4, 2, then the remaining prime.  Odd radices go
        // first: the first pass writes its R outputs R float2 apart across lanes, which is conflict-free in LDS only for odd R
        // (M = 12 N_prb always has a factor 3 to start with).
        float2 *src = bufA, *dst = bufB;
        for (uint32_t p = 0; p < sh.n_pass; p++) { // uniform over the workgroup
            const DftPass ps = sh.pass[p];
            switch (ps.R) {
            case 9:  dft_pass_r<9, THREADS>(src, dst, tw, S, M_max, ps); break;
            case 3:  dft_pass_r<3, THREADS>(src, dst, tw, S, M_max, ps); break;
            case 5:  dft_pass_r<5, THREADS>(src, dst, tw, S, M_max, ps); break;
            case 8:  dft_pass_r<8, THREADS>(src, dst, tw, S, M_max, ps); break;
            case 4:  dft_pass_r<4, THREADS>(src, dst, tw, S, M_max, ps); break;
            case 2:  dft_pass_r<2, THREADS>(src, dst, tw, S, M_max, ps); break;
            default: dft_pass<THREADS>(src, dst, tw, S, M, sh.r_M, M_max, ps); break;
            }
            __syncthreads();
            float2 *t = src; src = dst; dst = t;
        }
        // ---- de-map, descramble, de-interleave (transpose): soft bit q of symbol k goes to (k*12 + s)*Q_m + q.  Instantiated per modulation
        // (uniform over the workgroup): no modulation branches and no re-read of the allocation descriptor per element
        auto demap_all = [&](auto modc) {
        constexpr uint32_t MOD = decltype(modc)::value, QM = MOD == 3 ? 6 : MOD == 2 ? 4 : MOD == 1 ? 2 : 1;
        for (uint32_t o = threadIdx.x; o < S * M; o += THREADS) {
            // (all twelve symbols side by side is the common case: o / 12 for o < 2^15 as one 24-bit multiply and a shift)
            const uint32_t k = S == 12 ? __umul24(o, 43691u) >> 19 : quot(o, r_S_par), sy = o - __umul24(k, S), s = s0 + sy; // neighbouring threads write neighbouring bytes of e
            const float2   x = src[__umul24(sy, M_max) + k];
            int8_t         b[6] = {0, 0, 0, 0, 0, 0};
            if constexpr (LLR) { // t = rho_s x, w = rho_s; bit 2k on the real axis, 2k + 1 on the imaginary
                const float xr = scale * x.x, xi = scale * x.y;
                if (la.x_tap) la.x_tap[la.x_off[a_idx] + __umul24(s, M) + k] = make_float2(xr, xi);
                double       li[3] = {0.0, 0.0, 0.0}, lq[3] = {0.0, 0.0, 0.0};
                if constexpr (MMSE) { // t = u / nu_s, w = (1 - nu_s) / nu_s; both 0 where nu_s carries no information
                    const double nu = (double)rho[s], w = w_m[s];
                    llr_axis<(MOD < 1 ? 1u : MOD)>(nu > 0.0 ? (double)xr / nu : 0.0, w, li);
                    llr_axis<(MOD < 1 ? 1u : MOD)>(nu > 0.0 ? (double)xi / nu : 0.0, w, lq);
                } else {
                const double w = (double)rho[s];
                llr_axis<(MOD < 1 ? 1u : MOD)>(w * (double)xr, w, li);
                llr_axis<(MOD < 1 ? 1u : MOD)>(w * (double)xi, w, lq);
                }
#pragma unroll
                for (uint32_t q = 0; q < QM; q += 2) { b[q] = (int8_t)llr_byte(gd, li[q >> 1]); b[q + 1] = (int8_t)llr_byte(gd, lq[q >> 1]); }
            } else
            demap_symbol(scale * x.x, scale * x.y, MOD, b);
            const uint32_t n0 = (__umul24(s, M) + k) * QM, w = n0 >> 5, sh = n0 & 31;
            const uint32_t c  = __builtin_amdgcn_alignbit(cw[w + 1], cw[w], sh);
            int8_t        *ob = e + (__umul24(k, 12u) + s) * QM; // (32-bit offset: an allocation's soft bits are at most 12 * 1320 * 6 bytes)
            // descrambled soft bits q, q + 1 as one 16-bit word (the Q_m bytes of a symbol start on an even address)
            auto pair = [&](uint32_t q) -> uint32_t {
                const int lo = ((c >> q) & 1u) ? -b[q] : b[q], hi = ((c >> (q + 1)) & 1u) ? -b[q + 1] : b[q + 1];
                return (uint32_t)(uint8_t)lo | (uint32_t)(uint8_t)hi << 8;
            };
            if (QM == 2) *reinterpret_cast<uint16_t *>(ob) = (uint16_t)pair(0);
            else if (QM == 4) *reinterpret_cast<uint32_t *>(ob) = pair(0) | pair(2) << 16;
            else if (QM == 6) {
                *reinterpret_cast<uint16_t *>(ob)     = (uint16_t)pair(0);
                *reinterpret_cast<uint16_t *>(ob + 2) = (uint16_t)pair(2);
                *reinterpret_cast<uint16_t *>(ob + 4) = (uint16_t)pair(4);
            } else ob[0] = (c & 1u) ? (int8_t)-b[0] : b[0];
        }
        };
        switch (al.mod_type) {
        case 0:  if constexpr (!LLR) { demap_all(std::integral_constant<uint32_t, 0>{}); break; } // (a 3GPP plan holds no BPSK allocation)
        case 1:  demap_all(std::integral_constant<uint32_t, 1>{}); break;
        case 2:  demap_all(std::integral_constant<uint32_t, 2>{}); break;
        default: demap_all(std::integral_constant<uint32_t, 3>{}); break;
        }
        __syncthreads();
    }
}

// ---- PUCCH formats 1 / 1a / 1b (liblte_phy_pucch_format_1_1a_1b_channel_decode, liblte_phy.cc:2961-3146) -----------------------
// One wavefront per PUCCH resource: the resource's PRB pair (N_1_p in slot 0, N_rb_ul - N_1_p - 1 in slot 1), a channel estimate
// per slot from its three reference symbols (get_ulcch_ce :13799-13868: mean magnitude, the FIRST symbol's phase), one-tap
// equalisation, and the coherent sum over 2 x 4 x 12 elements of z / (s_ns w(i) r_u,v(n)) -- summed in the reference's order by one
// lane, divided by 95 as the reference does (its loop index after the last element, not the count) -- then the reference's decision.
// The sequences are the caller's (what liblte_phy_ul_init left in LIBLTE_PHY_STRUCT): per resource 352 floats, see mi_lte.h.
struct PucchRes { uint32_t unit, format, N_1_p; };
constexpr uint32_t PUCCH_TAB_FLOATS = 4 * 36 + 2 * 96 + 16;

__device__ __forceinline__ float pucch_soft(float rx_re, float rx_im, float exp_re, float exp_im)
{
    const float d_re = rx_re - exp_re, d_im = rx_im - exp_im;
    float dist = sqrtf(d_re * d_re + d_im * d_im); // (C++ overload resolution in the reference: sqrt(float) is the float function)
    const float cap = 1.0f - (1.0f / 120);
    if (dist >= cap) dist = cap;
    return 1.0f - dist;
}

__global__ __launch_bounds__(64) void k_pucch_decode(const float *__restrict__ subframes, uint32_t sf_stride, uint32_t N_rb_ul, uint32_t N_ant,
                                                     const PucchRes *__restrict__ res, const float *__restrict__ tabs, uint8_t *__restrict__ out /*[n][4]*/)
{
    __shared__ float c_re[2][12], c_im[2][12], t_re[96], t_im[96];
    const uint32_t r = blockIdx.x, ln = threadIdx.x;
    const PucchRes pr = res[r];
    const float *base = subframes + (size_t)pr.unit * sf_stride, *y_re = base, *y_im = base + 16 * N_SC_MAX;
    const float *tb = tabs + (size_t)r * PUCCH_TAB_FLOATS;
    const float *dm_re[2] = {tb, tb + 72}, *dm_im[2] = {tb + 36, tb + 108};
    const float *ruv_re = tb + 144, *ruv_im = tb + 240, *sw_re = tb + 336, *sw_im = tb + 344;
    const uint32_t prb[2] = {pr.N_1_p, N_rb_ul - pr.N_1_p - 1};
    if (ln < 24) { // (slot, sub-carrier): channel estimate from the three reference symbols 2, 3, 4 (9, 10, 11)
        const uint32_t s = ln / 12, j = ln % 12;
        float ave_mag = 0, ang0 = 0;
        for (uint32_t i = 0; i < 3; i++) {
            const uint32_t L = 7 * s + 2 + i, k = prb[s] * 12 + j, idx = i * 12 + j;
            const float cr = y_re[L * N_SC_MAX + k], ci = y_im[L * N_SC_MAX + k], dr = dm_re[s][idx], di = dm_im[s][idx];
            const float denom = dr * dr + di * di;
            const float tr = (1 / denom) * (cr * dr + ci * di), ti = (1 / denom) * (ci * dr - cr * di);
            ave_mag += sqrtf(tr * tr + ti * ti) / 3; // (:13842; float sqrt / int)
            if (i == 0) ang0 = atan2f(ti, tr);
        }
        c_re[s][j] = ave_mag * cosf(ang0);
        c_im[s][j] = ave_mag * sinf(ang0);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    for (uint32_t idx = ln; idx < 96; idx += 64) { // element (slot m', data symbol i, sub-carrier j)
        const uint32_t mp = idx / 48, i = (idx % 48) / 12, j = idx % 12, L = 7 * mp + (i < 2 ? i : i + 3), k = prb[mp] * 12 + j;
        const float zr = y_re[L * N_SC_MAX + k], zi = y_im[L * N_SC_MAX + k], hr = c_re[mp][j], hi = c_im[mp][j];
        const float hn = hr * hr + hi * hi;
        const float xr = (zr * hr + zi * hi) / hn, xi = (zi * hr - zr * hi) / hn; // pre_decoder_and_matched_filter_ul (:6727-6732)
        const float swr = sw_re[mp * 4 + i], swi = sw_im[mp * 4 + i], rr = ruv_re[idx], ri = ruv_im[idx];
        const float pr_ = swr * rr - swi * ri, pi_ = swr * ri + swi * rr, denom = pr_ * pr_ + pi_ * pi_;
        t_re[idx] = (1 / denom) * (xr * pr_ + xi * pi_);
        t_im[idx] = (1 / denom) * (-xr * pi_ + xi * pr_);
    }
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    if (ln == 0) {
        float d_re = 0, d_im = 0;
        for (uint32_t idx = 0; idx < 96; idx++) { d_re += t_re[idx]; d_im += t_im[idx]; }
        d_re /= 95u; // the reference divides by its last index (:3097-3098)
        d_im /= 95u;
        d_re *= sqrt((double)N_ant);
        d_im *= sqrt((double)N_ant);
        uint8_t b0 = 0, b1 = 0, nb = 1;
        float   sd;
        if (pr.format <= 1) {
            if (d_re < 0) { sd = pucch_soft(d_re, d_im, -1, 0); b0 = 1; }
            else          { sd = pucch_soft(d_re, d_im, 1, 0); b0 = 0; }
        } else {
            const float ang = ref_atan2f(d_im, d_re); // (decisions on the angle: the host libm's rounding, phy_dev.hpp)
            nb = 2;
            if (ang >= M_PI / 4 && ang < 3 * M_PI / 4)        { sd = pucch_soft(d_re, d_im, 0, 1); b0 = 1; b1 = 0; }
            else if (ang >= -M_PI / 4 && ang < M_PI / 4)      { sd = pucch_soft(d_re, d_im, 1, 0); b0 = 0; b1 = 0; }
            else if (ang >= -3 * M_PI / 4 && ang < -M_PI / 4) { sd = pucch_soft(d_re, d_im, 0, -1); b0 = 0; b1 = 1; }
            else                                              { sd = pucch_soft(d_re, d_im, -1, 0); b0 = 1; b1 = 1; }
        }
        out[4 * r] = b0; out[4 * r + 1] = b1; out[4 * r + 2] = nb; out[4 * r + 3] = sd > 0.5f ? 0 : 1; // LIBLTE_SUCCESS / LIBLTE_ERROR_INVALID_INPUTS
    }
}

} // namespace

// ------------------------------------------------------------------------------------------------
// host side: plans

struct mi_lte_pusch_plan {
    mi_lte_dl_cfg cfg;
    MiPlanCore    core;
    uint32_t      M_max = 0, words_max = 0;
    PuschDesc    *d_desc = nullptr;
    float        *d_dmrs = nullptr;
    std::vector<uint32_t> h_e_len;
    // 3GPP transport-block mode (mi_lte_pusch_plan_create_3gpp): the spec-normalised demodulator, dlsch3gpp.hip's code blocks and a BCJR decoder
    MiDlsch3     *g3 = nullptr;
    uint32_t      decoder = MI_LTE_TURBO_BCJR, n_iter = 8, max_tbs = 0;
    MiUlschUci   *uci = nullptr; // control information on the allocations (mi_lte_pusch_plan_create_3gpp_uci): ulsch_uci.hip's part
    // 3GPP mode, mi_lte_pusch_plan_set_demapper: MAXLOG's fixed gain (0: automatic); the last MAXLOG run's gain [n_alloc] and rho [n_alloc][12]
    int           device = 0;
    uint32_t      demap = MI_LTE_DEMAP_REF;
    float         demap_gain = 0.0f, *d_llr_gain = nullptr, *d_llr_rho = nullptr;
    // mi_lte_pusch_plan_set_llr_noise: the noise-referenced gain's scale (0: off) and the last such run's sigma2 [n_alloc]
    float         llr_noise = 0.0f, *d_llr_s2 = nullptr;
    // mi_lte_pusch_plan_set_llr_tap: the de-mapper's input symbols, 12 M float2 per allocation at h_x_off (nothing of it exists until asked for)
    float2       *d_llr_x = nullptr;
    uint32_t     *d_x_off = nullptr;
    std::vector<uint32_t> h_x_off;
    // mi_lte_pusch_plan_set_rx_antennas: antennas a MAXLOG run combines (1: off) and the subframes between two antennas' grids of one unit;
    // the instantiations of k_pusch_demod_llr_rx whose dynamic-LDS attribute is set on the plan's device (one bit each)
    uint32_t      n_units = 0, n_rx = 1, ant_stride = 0, rx_lds_set = 0;
    // mi_lte_pusch_plan_set_equaliser: the equaliser of a MAXLOG run with the noise gain on, and the last MMSE run's nu [n_alloc][12]
    // (nothing of it exists until MMSE is first set)
    uint32_t      eq = MI_LTE_EQ_ZF;
    float        *d_llr_nu = nullptr;
};

// the float next above or equal to 1 / d (see quot)
static float recip_up(uint32_t d)
{
    const double rd = 1.0 / (double)d;
    float        r  = (float)rd;
    if ((double)r < rd) r = nextafterf(r, 2.0f);
    return r;
}

// One PuschShape per N_prb, in HBM for the life of the context
static int pusch_shapes(mi_lte_ctx *ctx)
{
    if (ctx->d_pusch_shapes) return MI_LTE_OK;
    std::vector<PuschShape> tab(N_SHAPES);
    memset(tab.data(), 0, sizeof(PuschShape) * N_SHAPES);
    for (uint32_t n = 1; n < N_SHAPES; n++) {
        PuschShape    &sh = tab[n];
        const uint32_t M  = 12 * n;
        sh.sqrt_M = (float)sqrt((double)M);
        sh.r_sqrt_M = (float)(1.0 / sqrt((double)M));
        sh.r_M    = recip_up(M);
        uint32_t rem = M, Ns = 1;
        while (rem > 1) {
            uint32_t R;
            if (rem % 9 == 0) R = 9;
            else if (rem % 3 == 0) R = 3;
            else if (rem % 5 == 0) R = 5;
            else if (rem % 8 == 0) R = 8;
            else if (rem % 4 == 0) R = 4;
            else if (rem % 2 == 0) R = 2;
            else { R = 7; while (rem % R) R += 2; }
            if (sh.n_pass == MAX_PASSES) { ctx->err = "transform size with more passes than the table has room for"; return MI_LTE_ERR_UNSUPPORTED; }
            sh.pass[sh.n_pass++] = {R, Ns, M / R, M / (Ns * R), recip_up(M / R), recip_up(Ns)};
            Ns *= R;
            rem /= R;
        }
    }
    void *d = nullptr;
    MI_HIP_CHECK(ctx, hipMalloc(&d, sizeof(PuschShape) * N_SHAPES));
    ctx->owned.push_back(d);
    MI_H2D(ctx, d, tab.data(), sizeof(PuschShape) * N_SHAPES);
    MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx));
    ctx->d_pusch_shapes = d;
    return MI_LTE_OK;
}

// The arguments are pusch_plan_layout's (pusch_plan.h), which makes everything the plan holds but its device memory: every refusal that is
// no HIP error comes from there, before the first allocation on the device.
extern "C" void mi_lte_pusch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pusch_plan *pl);
static int pusch_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const uint32_t *h_unit_subfr_num,
                             const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                             const float *h_dmrs, mi_lte_pusch_plan **out, bool spec, const mi_lte_ulsch_uci *h_uci = nullptr)
{
    if (!ctx || !cfg || (!ul && !h_dmrs) || !h_unit_subfr_num || !h_unit_n_id_cell || !h_allocs || !out || n_alloc == 0 || n_units == 0)
        return MI_LTE_ERR_INVALID_ARG;
    PuschPlanLayout L;
    const char     *err = nullptr;
    const int       rc  = pusch_plan_layout(cfg, ul, h_dmrs, h_unit_subfr_num, h_unit_n_id_cell, n_units, h_allocs, n_alloc, spec, h_uci, &L, &err);
    if (rc != MI_LTE_OK) {
        if (err) ctx->err = err;
        return rc;
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    auto *pl    = new mi_lte_pusch_plan();
    auto  guard = on_fail([&] { (void)hipStreamSynchronize(ctx->stream); mi_lte_pusch_plan_destroy(nullptr, pl); });
    pl->cfg     = *cfg;
    pl->device  = ctx->device;
    pl->n_units = n_units;
    pl->M_max   = L.M_max; pl->words_max = L.words_max; pl->max_tbs = L.max_tbs;
    pl->core.n_alloc    = n_alloc;
    pl->core.e_bytes    = L.e_bytes;
    pl->core.out_stride = L.out_stride;
    pl->core.groups     = std::move(L.groups);
    pl->core.h_e_off    = std::move(L.e_off);
    pl->h_e_len         = std::move(L.e_len);
    pl->h_x_off         = std::move(L.x_off);
    MI_HIP_CHECK(ctx, pl->core.allocate(n_alloc, pl->core.e_bytes));
    if (spec) {
        const int rc3 = mi_dlsch3_create(ctx, &ULSCH_AS_DLSCH, std::move(L.g3), n_alloc, &pl->g3);
        if (rc3 != MI_LTE_OK) return rc3;
        MI_HIP_CHECK(ctx, hipMalloc((void **)&pl->d_llr_gain, sizeof(float) * 14 * (size_t)n_alloc)); // gain [n_alloc] | rho [n_alloc][12] | sigma2 [n_alloc]
        MI_HIP_CHECK(ctx, hipMemsetAsync(pl->d_llr_gain, 0, sizeof(float) * 14 * (size_t)n_alloc, ctx->stream));
        pl->d_llr_rho = pl->d_llr_gain + n_alloc;
        pl->d_llr_s2  = pl->d_llr_gain + 13 * (size_t)n_alloc;
    }
    if (h_uci) {
        const int rcu = mi_ulsch_uci_create(ctx, h_allocs, h_uci, L.c_init.data(), L.G.data(), n_alloc, pl->core.e_bytes, &pl->uci);
        if (rcu != MI_LTE_OK) return rcu;
    }
    MI_HIP_CHECK(ctx, hipMalloc((void **)&pl->d_desc, sizeof(PuschDesc) * n_alloc));
    MI_HIP_CHECK(ctx, hipMalloc((void **)&pl->d_dmrs, sizeof(float) * std::max<size_t>(L.dmrs.size(), 1)));
    MI_H2D(ctx, pl->core.d_allocs, h_allocs, sizeof(mi_lte_pdsch_alloc) * n_alloc);
    MI_H2D(ctx, pl->d_desc, L.desc.data(), sizeof(PuschDesc) * n_alloc);
    MI_H2D(ctx, pl->d_dmrs, L.dmrs.data(), sizeof(float) * L.dmrs.size());
    MI_H2D(ctx, pl->core.d_e_off, pl->core.h_e_off.data(), sizeof(uint32_t) * n_alloc);
    MI_H2D(ctx, pl->core.d_cb_alloc, L.cb_alloc.data(), sizeof(uint32_t) * n_alloc);
    MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx));
    guard.armed = false;
    *out = pl;
    return MI_LTE_OK;
}

int mi_pusch_plan_create_impl(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const uint32_t *h_unit_subfr_num,
                              const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                              const float *h_dmrs, mi_lte_pusch_plan **out)
{
    return pusch_plan_create(ctx, cfg, ul, h_unit_subfr_num, h_unit_n_id_cell, n_units, h_allocs, n_alloc, h_dmrs, out, /*spec=*/false);
}

extern "C" {

int mi_lte_pusch_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const uint32_t *h_unit_subfr_num,
                             const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                             mi_lte_pusch_plan **out)
{
    if (!ul) return MI_LTE_ERR_INVALID_ARG;
    return mi_pusch_plan_create_impl(ctx, cfg, ul, h_unit_subfr_num, h_unit_n_id_cell, n_units, h_allocs, n_alloc, nullptr, out);
}

int mi_lte_pusch_plan_create_3gpp(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const uint32_t *h_unit_subfr_num,
                                  const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                  mi_lte_pusch_plan **out)
{
    if (!ul) return MI_LTE_ERR_INVALID_ARG;
    return pusch_plan_create(ctx, cfg, ul, h_unit_subfr_num, h_unit_n_id_cell, n_units, h_allocs, n_alloc, nullptr, out, /*spec=*/true);
}

int mi_lte_pusch_plan_create_3gpp_uci(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const uint32_t *h_unit_subfr_num,
                                      const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                      const mi_lte_ulsch_uci *h_uci, mi_lte_pusch_plan **out)
{
    if (!ul) return MI_LTE_ERR_INVALID_ARG;
    return pusch_plan_create(ctx, cfg, ul, h_unit_subfr_num, h_unit_n_id_cell, n_units, h_allocs, n_alloc, nullptr, out, /*spec=*/true, h_uci);
}

int mi_lte_pusch_plan_uci_results(const mi_lte_pusch_plan *pl, const mi_lte_ulsch_uci_result **d_records)
{
    if (!pl || !pl->uci || !d_records) return MI_LTE_ERR_INVALID_ARG;
    *d_records = pl->uci->d_res;
    return MI_LTE_OK;
}

// the gathered run of an allocation: G data soft bits at the plan's offset, the Q_cqi CQI soft bits behind them
int mi_lte_pusch_plan_data_soft(const mi_lte_pusch_plan *pl, uint32_t alloc, const int8_t **d_data, uint32_t *G)
{
    if (!pl || !pl->uci || alloc >= pl->core.n_alloc || !d_data || !G) return MI_LTE_ERR_INVALID_ARG;
    *d_data = pl->uci->d_e + (size_t)pl->core.h_e_off[alloc] * 64;
    *G      = pl->uci->h_G[alloc];
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_cqi_soft(const mi_lte_pusch_plan *pl, uint32_t alloc, const int8_t **d_cqi, uint32_t *Q_cqi)
{
    if (!pl || !pl->uci || alloc >= pl->core.n_alloc || !d_cqi || !Q_cqi) return MI_LTE_ERR_INVALID_ARG;
    *d_cqi = pl->uci->d_e + (size_t)pl->core.h_e_off[alloc] * 64 + pl->uci->h_G[alloc];
    *Q_cqi = pl->uci->h_Q_cqi[alloc];
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_cqi_decode(mi_lte_pusch_plan *pl, const uint32_t *h_O_cqi)
{
    if (!pl || !pl->uci) return MI_LTE_ERR_INVALID_ARG;
    return mi_ulsch_cqi_set(pl->uci, pl->core.h_e_off.data(), pl->core.e_bytes, h_O_cqi);
}

int mi_lte_pusch_plan_cqi_results(const mi_lte_pusch_plan *pl, const mi_lte_cqi_result **d_records)
{
    if (!pl || !pl->uci || !d_records) return MI_LTE_ERR_INVALID_ARG;
    *d_records = pl->uci->d_cqi_res;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_decoder(mi_lte_pusch_plan *pl, uint32_t mode, uint32_t n_iter, int qpp_spec)
{
    if (!pl) return MI_LTE_ERR_INVALID_ARG;
    if (!pl->g3) return MI_LTE_ERR_UNSUPPORTED; // a reference-mode plan stays what it is: the REF decoder
    const bool bcjr = mi_is_bcjr(mode);
    if (!(mode == MI_LTE_TURBO_REF || bcjr) || (bcjr && (n_iter == 0 || n_iter > 64))) return MI_LTE_ERR_INVALID_ARG;
    if (mode == MI_LTE_TURBO_REF) return MI_LTE_ERR_UNSUPPORTED;
    if (!qpp_spec) return MI_LTE_ERR_INVALID_ARG;
    pl->decoder = mode; pl->n_iter = n_iter;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_demapper(mi_lte_pusch_plan *pl, uint32_t mode, float gain)
{
    if (!pl || mode > MI_LTE_DEMAP_MAXLOG) return MI_LTE_ERR_INVALID_ARG;
    if (mode == MI_LTE_DEMAP_REF) { pl->demap = MI_LTE_DEMAP_REF; return MI_LTE_OK; }
    if (!(gain >= 0.0f) || gain > 3.4028234e38f) return MI_LTE_ERR_INVALID_ARG; // negative, NaN or infinite
    if (!pl->g3) return MI_LTE_ERR_UNSUPPORTED; // a reference-mode plan keeps the reference's de-mapper
    pl->demap = mode; pl->demap_gain = gain;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_llr_gain(const mi_lte_pusch_plan *pl, const float **d_gain)
{
    if (!pl || !d_gain || !pl->d_llr_gain) return MI_LTE_ERR_INVALID_ARG;
    *d_gain = pl->d_llr_gain;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_llr_rho(const mi_lte_pusch_plan *pl, const float **d_rho)
{
    if (!pl || !d_rho || !pl->d_llr_rho) return MI_LTE_ERR_INVALID_ARG;
    *d_rho = pl->d_llr_rho;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_llr_noise(mi_lte_pusch_plan *pl, float scale)
{
    if (!pl || !(scale >= 0.0f) || scale > 3.4028234e38f) return MI_LTE_ERR_INVALID_ARG; // negative, NaN or infinite
    if (!pl->g3) return MI_LTE_ERR_UNSUPPORTED; // a reference-mode plan has no LLR to scale
    pl->llr_noise = scale;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_llr_noise(const mi_lte_pusch_plan *pl, const float **d_sigma2)
{
    if (!pl || !d_sigma2 || !pl->d_llr_s2) return MI_LTE_ERR_INVALID_ARG;
    *d_sigma2 = pl->d_llr_s2;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_rx_antennas(mi_lte_pusch_plan *pl, uint32_t n_rx, uint32_t ant_stride)
{
    if (!pl || !(n_rx == 1 || n_rx == 2 || n_rx == 4)) return MI_LTE_ERR_INVALID_ARG;
    if (!pl->g3) return MI_LTE_ERR_UNSUPPORTED; // a reference-mode plan has no max-log de-mapper to combine for
    if (n_rx == 1) { pl->n_rx = 1; pl->ant_stride = 0; return MI_LTE_OK; }
    if (ant_stride < pl->n_units) return MI_LTE_ERR_INVALID_ARG;
    int limit = 0; // the device's per-workgroup LDS: the combining launch has to fit it at some S_par
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, pl->device) != hipSuccess) return MI_LTE_ERR_HIP;
    PuschLaunch L; // (the noise-referenced gain does not change what fits)
    if (!pusch_launch_plan(pl->M_max, pl->words_max, {/*maxlog=*/true, /*noise=*/false, /*mmse=*/false, n_rx}, (size_t)std::max(limit, 0), 0, &L)) return MI_LTE_ERR_UNSUPPORTED;
    pl->n_rx = n_rx; pl->ant_stride = ant_stride;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_rx_antennas(const mi_lte_pusch_plan *pl, uint32_t *n_rx, uint32_t *ant_stride)
{
    if (!pl || !n_rx || !ant_stride) return MI_LTE_ERR_INVALID_ARG;
    *n_rx = pl->n_rx; *ant_stride = pl->ant_stride;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_equaliser(mi_lte_pusch_plan *pl, uint32_t mode)
{
    if (!pl || mode > MI_LTE_EQ_MMSE) return MI_LTE_ERR_INVALID_ARG;
    if (!pl->g3) return MI_LTE_ERR_UNSUPPORTED; // a reference-mode plan keeps the reference's equaliser
    if (mode == MI_LTE_EQ_MMSE && !pl->d_llr_nu) { // the nu tap, zeros until an MMSE run
        const size_t bytes = sizeof(float) * 12 * (size_t)pl->core.n_alloc;
        float       *nu = nullptr;
        if (hipSetDevice(pl->device) != hipSuccess || hipMalloc((void **)&nu, bytes) != hipSuccess) return MI_LTE_ERR_HIP;
        if (hipMemset(nu, 0, bytes) != hipSuccess) { (void)hipFree(nu); return MI_LTE_ERR_HIP; }
        pl->d_llr_nu = nu;
    }
    pl->eq = mode;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_equaliser(const mi_lte_pusch_plan *pl, uint32_t *mode)
{
    if (!pl || !mode) return MI_LTE_ERR_INVALID_ARG;
    *mode = pl->eq;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_llr_nu(const mi_lte_pusch_plan *pl, const float **d_nu)
{
    if (!pl || !d_nu || !pl->d_llr_nu) return MI_LTE_ERR_INVALID_ARG;
    *d_nu = pl->d_llr_nu;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_llr_tap(mi_lte_pusch_plan *pl, uint32_t on)
{
    if (!pl || !pl->g3) return MI_LTE_ERR_INVALID_ARG;
    if (hipSetDevice(pl->device) != hipSuccess) return MI_LTE_ERR_HIP;
    if (!on) { // (hipFree waits for a run that may still be writing the buffer)
        (void)hipFree(pl->d_llr_x); (void)hipFree(pl->d_x_off);
        pl->d_llr_x = nullptr; pl->d_x_off = nullptr;
        return MI_LTE_OK;
    }
    if (pl->d_llr_x) return MI_LTE_OK;
    const uint32_t n = pl->core.n_alloc;
    const size_t   bytes = sizeof(float2) * (size_t)pl->h_x_off[n];
    float2   *x = nullptr;
    uint32_t *off = nullptr;
    if (hipMalloc((void **)&x, bytes) != hipSuccess) return MI_LTE_ERR_HIP;
    if (hipMalloc((void **)&off, sizeof(uint32_t) * n) != hipSuccess || hipMemset(x, 0, bytes) != hipSuccess ||
        hipMemcpy(off, pl->h_x_off.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(x); (void)hipFree(off);
        return MI_LTE_ERR_HIP;
    }
    pl->d_llr_x = x; pl->d_x_off = off;
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_llr_symbols(const mi_lte_pusch_plan *pl, uint32_t alloc, const float **d_x, uint32_t *n)
{
    if (!pl || !pl->g3 || !pl->d_llr_x || alloc >= pl->core.n_alloc || !d_x || !n) return MI_LTE_ERR_INVALID_ARG;
    *d_x = reinterpret_cast<const float *>(pl->d_llr_x + pl->h_x_off[alloc]);
    *n   = pl->h_x_off[alloc + 1] - pl->h_x_off[alloc];
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_set_output(mi_lte_pusch_plan *pl, uint32_t packed)
{
    if (!pl) return MI_LTE_ERR_INVALID_ARG;
    if (!pl->g3) return packed ? MI_LTE_ERR_UNSUPPORTED : MI_LTE_OK;
    pl->core.packed     = packed ? 1u : 0u;
    pl->core.out_stride = mi_out_stride(pl->max_tbs, packed != 0);
    return MI_LTE_OK;
}

int mi_lte_pusch_plan_cb_soft(const mi_lte_pusch_plan *pl, uint32_t alloc, const int8_t **d_blocks, uint32_t *C, uint32_t *K)
{
    if (!pl || !pl->g3) return MI_LTE_ERR_INVALID_ARG;
    return mi_dlsch3_cb_soft(pl->g3, alloc, d_blocks, C, K);
}

int mi_lte_pusch_plan_cb_ok(const mi_lte_pusch_plan *pl, const uint32_t **d_mask)
{
    if (!pl || !pl->g3 || !d_mask) return MI_LTE_ERR_INVALID_ARG;
    *d_mask = mi_dlsch3_cb_ok(pl->g3);
    return MI_LTE_OK;
}

void mi_lte_pusch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pusch_plan *pl)
{
    if (!pl) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    pl->core.release();
    (void)hipFree(pl->d_desc);
    (void)hipFree(pl->d_dmrs);
    (void)hipFree(pl->d_llr_gain);
    (void)hipFree(pl->d_llr_x);
    (void)hipFree(pl->d_x_off);
    (void)hipFree(pl->d_llr_nu);
    mi_dlsch3_free(pl->g3);
    mi_ulsch_uci_free(pl->uci);
    delete pl;
}

uint32_t mi_lte_pusch_plan_out_stride(const mi_lte_pusch_plan *pl) { return pl ? pl->core.out_stride : 0; }

int mi_lte_pusch_plan_soft_bits(const mi_lte_pusch_plan *pl, uint32_t alloc, const int8_t **d_e, uint32_t *n_bits)
{
    if (!pl || alloc >= pl->core.n_alloc || !d_e || !n_bits) return MI_LTE_ERR_INVALID_ARG;
    *d_e    = pl->core.d_e + (size_t)pl->core.h_e_off[alloc] * 64;
    *n_bits = pl->h_e_len[alloc];
    return MI_LTE_OK;
}

} // extern "C"

// The workgroup's width as a template argument: f(PuschWidth<64 | 128 | 192 | 256>{}) for what pusch_launch_plan (pusch_launch.h) chose
template <uint32_t T> using PuschWidth = std::integral_constant<uint32_t, T>;
template <typename F> static int pusch_width(uint32_t threads, F f)
{
    return threads == 64 ? f(PuschWidth<64>{}) : threads == 128 ? f(PuschWidth<128>{}) : threads == 192 ? f(PuschWidth<192>{}) : f(PuschWidth<256>{});
}

// The demodulator's launch as L shapes it, k_pusch_demod<T, SPEC, LA> with L's argument block `la`.  The kernel is instantiated only where
// pusch_variant_compiled (pusch_launch.h) says the variant exists, and without SPEC for the plain block alone; pusch_launch_plan plans
// nothing else, so the other branch is never reached.  lds_limit: the device's per-workgroup LDS, read for a combining launch only.
template <uint32_t T, bool SPEC, typename LA>
static int pusch_launch(mi_lte_ctx *ctx, mi_lte_pusch_plan *pl, const PuschLaunch &L, size_t lds_limit, const float *d_subframes, const LA &la)
{
    if constexpr (pusch_variant_compiled(LA::FAMILY, T, LA::N_RX) && (SPEC || !LA::LLR)) {
        if constexpr (LA::N_RX > 1) {
            // More than 64 KB of dynamic LDS has to be asked for, per kernel and device (as for k_bcjr_block, bcjr.hip): once per plan and instantiation
            const uint32_t bit = 1u << ((T == 256 ? 1 : 0) + (LA::N_RX == 4 ? 2 : 0) + (LA::NOISE ? 4 : 0) + (LA::MMSE ? 8 : 0));
            if (!(pl->rx_lds_set & bit)) {
                MI_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k_pusch_demod<T, SPEC, LA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
                pl->rx_lds_set |= bit;
            }
        }
        const GoldTables gt{ctx->d_gold_x1, ctx->d_gold_x2b, ctx->gold_words};
        MI_LAUNCH(ctx, L.label, (k_pusch_demod<T, SPEC, LA>), dim3(pl->core.n_alloc), dim3(T), L.lds_bytes, d_subframes, (uint32_t)mi_lte_ul_subframe_floats(),
                  pl->core.d_allocs, pl->d_desc, pl->d_dmrs, gt, pl->core.d_e, pl->core.d_e_off, pl->core.d_e_len, pl->M_max, L.S_par, recip_up(L.S_par),
                  static_cast<const PuschShape *>(ctx->d_pusch_shapes), la);
        return MI_LTE_OK;
    } else { ctx->err = "k_pusch_demod: no such variant at this workgroup width"; return MI_LTE_ERR_UNSUPPORTED; }
}

// A plan run: the demodulator, then the 3GPP mode's control information and code blocks (ulsch_uci.hip, dlsch3gpp.hip) or the REF dispatch
// (turbo.hip).  pool / h_bind: a HARQ run (mi_lte_pusch_decode_run_harq), nullptr otherwise.  Every refusal returns before a launch.
static int pusch_run(mi_lte_ctx *ctx, mi_lte_pusch_plan *pl, mi_lte_harq_pool *pool, const mi_lte_harq_bind *h_bind, const float *d_subframes,
                     uint8_t *d_out_bits, int32_t *d_status)
{
    if (!ctx || !pl || !d_subframes || !d_out_bits || !d_status) return MI_LTE_ERR_INVALID_ARG;
    int rc;
    if (pool) {
        if (!pl->g3) { ctx->err = "HARQ soft combining needs a plan in the 3GPP transport-block mode"; return MI_LTE_ERR_UNSUPPORTED; }
        if ((rc = mi_dlsch3_harq_check(ctx, pl->g3, pool, h_bind)) != MI_LTE_OK) return rc;
    }
    if (pl->n_rx > 1 && pl->demap != MI_LTE_DEMAP_MAXLOG) { // (mi_lte_pusch_plan_set_rx_antennas: changing either setting makes the plan runnable again)
        ctx->err = "receive-antenna combining needs the max-log demapper (mi_lte_pusch_plan_set_demapper, MI_LTE_DEMAP_MAXLOG)";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    const bool mmse = pl->eq == MI_LTE_EQ_MMSE;
    if (mmse && (pl->demap != MI_LTE_DEMAP_MAXLOG || !(pl->llr_noise > 0.0f))) { // (mi_lte_pusch_plan_set_equaliser: changing either setting makes the plan runnable again)
        ctx->err = "MMSE equalisation needs the max-log demapper and the noise-referenced gain (mi_lte_pusch_plan_set_demapper, mi_lte_pusch_plan_set_llr_noise)";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    rc = mi_ctx_gold_tables(ctx);
    if (rc != MI_LTE_OK) return rc;
    if ((rc = pusch_shapes(ctx)) != MI_LTE_OK) return rc;
    uint32_t threads_override = 0;
    if (const char *ev = getenv("MI_LTE_PUSCH_THREADS")) { // (tuning aid)
        const int t = atoi(ev);
        if (t >= 64 && t <= (int)PUSCH_THREADS && t % 64 == 0) threads_override = (uint32_t)t;
    }
    const bool llr = pl->g3 && pl->demap == MI_LTE_DEMAP_MAXLOG; // (mi_lte_pusch_plan_set_demapper)
    float      auto_t = (float)MI_LTE_DEMAP_AUTO_T;
    if (llr)
        if (const char *ev = getenv("MI_LTE_DEMAP_AUTO_T")) { // (tuning aid: tools/pusch_llr_sweep.py checks the header's constant with it)
            const float t = (float)atof(ev);
            if (t >= 1.0f && t <= 127.0f) auto_t = t;
        }
    size_t lds_limit = 0; // the device's per-workgroup LDS: a combining launch has to fit it at some S_par
    if (llr && pl->n_rx > 1) {
        int limit = 0;
        MI_HIP_CHECK(ctx, hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
        lds_limit = (size_t)std::max(limit, 0);
    }
    PuschLaunch L;
    if (!pusch_launch_plan(pl->M_max, pl->words_max, {llr, pl->llr_noise > 0.0f, mmse, pl->n_rx}, lds_limit, threads_override, &L)) {
        ctx->err = "receive-antenna combining: the plan's widest allocation does not fit the device's LDS";
        return MI_LTE_ERR_UNSUPPORTED;
    }
    const PuschLlr      la{pl->demap_gain, auto_t, (uint32_t)(L.lds_off / sizeof(float)), pl->d_llr_gain, pl->d_llr_rho, pl->d_llr_x, pl->d_x_off};
    const PuschLlrNoise ln{la, pl->llr_noise, pl->d_llr_s2};
    // width and block to the one launch; SPEC is the plan's mode (every max-log launch is the 3GPP mode's)
    const auto go = [&](const auto &block) {
        return pusch_width(L.threads, [&](auto w) {
            return pl->g3 ? pusch_launch<decltype(w)::value, true>(ctx, pl, L, lds_limit, d_subframes, block)
                          : pusch_launch<decltype(w)::value, false>(ctx, pl, L, lds_limit, d_subframes, block);
        });
    };
    switch (L.family) { // L's family, antennas and noise gain as the kernel's argument block
    case PuschFamily::PLAIN: rc = go(PuschNoLlr{}); break;
    case PuschFamily::LLR: rc = go(la); break;
    case PuschFamily::LLR_NOISE: rc = go(ln); break;
    case PuschFamily::LLR_RX:
        rc = L.n_rx == 2 ? (L.noise ? go(PuschLlrRx<2, true>{ln, pl->ant_stride}) : go(PuschLlrRx<2, false>{ln, pl->ant_stride}))
                         : (L.noise ? go(PuschLlrRx<4, true>{ln, pl->ant_stride}) : go(PuschLlrRx<4, false>{ln, pl->ant_stride}));
        break;
    case PuschFamily::LLR_MMSE:
        rc = L.n_rx <= 1 ? go(PuschLlrMmse<1>{ln, pl->d_llr_nu, 0u})
                         : L.n_rx == 2 ? go(PuschLlrMmse<2>{ln, pl->d_llr_nu, pl->ant_stride}) : go(PuschLlrMmse<4>{ln, pl->d_llr_nu, pl->ant_stride});
        break;
    }
    if (rc != MI_LTE_OK) return rc;
    MI_HIP_CHECK(ctx, hipGetLastError());
    if (pl->g3) { // 3GPP mode: the code blocks of dlsch3gpp.hip, combined into the pool's buffers on a HARQ run
        MiDecodeIO io = pl->core.io(d_out_bits, d_status, /*ul=*/true);
        if (pl->uci) { // control information: rate un-matching reads the gathered data run (G soft bits per allocation, the same offsets)
            if ((rc = mi_ulsch_uci_run(ctx, pl->uci, pl->core.d_e, pl->core.d_e_off)) != MI_LTE_OK) return rc;
            if (pl->uci->cqi_on && (rc = mi_ulsch_cqi_run(ctx, pl->uci)) != MI_LTE_OK) return rc; // (opt-in: mi_lte_pusch_plan_set_cqi_decode)
            io.d_e = pl->uci->d_e; io.d_e_len = pl->uci->d_e_len;
        }
        if ((rc = mi_dlsch3_run(ctx, pl->g3, pool, h_bind, io, pl->decoder, pl->n_iter)) != MI_LTE_OK) return rc;
        ctx->last_kernels = std::string(L.label) + ":1," + // (mi_dlsch3_run lists its own kernels)
                            (!pl->uci          ? ""
                             : pl->uci->cqi_on ? "k_ulsch_uci_gather:1,k_ulsch_uci_decide:1,k_ulsch_cqi_decode:1,"
                                               : "k_ulsch_uci_gather:1,k_ulsch_uci_decide:1,") +
                            ctx->last_kernels;
        return MI_LTE_OK;
    }
    // several block sizes (the UEs of a subframe rarely share one): one launch set over all of them, as in the PDSCH chain
    rc = mi_turbo_ref_dispatch(ctx, pl->core.groups.data(), (uint32_t)pl->core.groups.size(), pl->core.io(d_out_bits, d_status, /*ul=*/true), &pl->core.multi);
    if (rc != MI_LTE_OK) return rc;
    ctx->last_kernels.insert(0, std::string(L.label) + ":1,");
    return MI_LTE_OK;
}

extern "C" {

int mi_lte_pusch_decode_run(mi_lte_ctx *ctx, mi_lte_pusch_plan *pl, const float *d_subframes, uint8_t *d_out_bits, int32_t *d_status)
{
    return pusch_run(ctx, pl, nullptr, nullptr, d_subframes, d_out_bits, d_status);
}

int mi_lte_pusch_decode_run_harq(mi_lte_ctx *ctx, mi_lte_pusch_plan *pl, mi_lte_harq_pool *pool, const mi_lte_harq_bind *h_bind,
                                 const float *d_subframes, uint8_t *d_out_bits, int32_t *d_status)
{
    if (!pool || !h_bind) return MI_LTE_ERR_INVALID_ARG;
    return pusch_run(ctx, pl, pool, h_bind, d_subframes, d_out_bits, d_status);
}

} // extern "C"

// The same decode in three steps for a caller that builds ONE launch chain per subframe (hostapi.cc: mi_lte_ul_subframe_decode_host): the
// descriptors and tables go into the context's mapped pinned block while the stream is idle (the caller has waited), the kernel is queued
// behind the caller's front end, the results are read after the caller's single wait.  At most MI_PUCCH_STAGED_MAX resources.
int mi_pucch_stage(mi_lte_ctx *ctx, uint32_t N_rb_ul, const mi_lte_pucch_res *h_res, const float *h_tables, uint32_t n_res, MiPucchStaged *st)
{
    if (!ctx || !h_res || !h_tables || !st || n_res == 0 || n_res > MI_PUCCH_STAGED_MAX) return MI_LTE_ERR_INVALID_ARG;
    for (uint32_t r = 0; r < n_res; r++)
        if (h_res[r].format > 2 || h_res[r].N_1_p_pucch >= N_rb_ul) return MI_LTE_ERR_INVALID_ARG;
    const size_t b_res = sizeof(PucchRes) * (size_t)n_res, b_tab = sizeof(float) * PUCCH_TAB_FLOATS * (size_t)n_res, b_out = 4 * (size_t)n_res;
    st->n_res = n_res;
    st->o_tab = (b_res + 255) & ~(size_t)255;
    st->o_out = (st->o_tab + b_tab + 255) & ~(size_t)255;
    int rc = mi_ctx_small_results(ctx, st->o_out + b_out, (void **)&st->h_base, (void **)&st->d_base);
    if (rc != MI_LTE_OK) return rc;
    PucchRes *res = (PucchRes *)st->h_base;
    for (uint32_t r = 0; r < n_res; r++) res[r] = PucchRes{h_res[r].unit, h_res[r].format, h_res[r].N_1_p_pucch};
    memcpy(st->h_base + st->o_tab, h_tables, b_tab);
    return MI_LTE_OK;
}
int mi_pucch_launch(mi_lte_ctx *ctx, const MiPucchStaged *st, uint32_t N_rb_ul, const float *d_subframes)
{
    MI_LAUNCH(ctx, "k_pucch_decode", k_pucch_decode, dim3(st->n_res), dim3(64), 0, d_subframes, (uint32_t)mi_lte_ul_subframe_floats(), N_rb_ul, 1u,
              (const PucchRes *)st->d_base, (const float *)(st->d_base + st->o_tab), (uint8_t *)(st->d_base + st->o_out));
    MI_HIP_CHECK(ctx, hipGetLastError());
    return MI_LTE_OK;
}
void mi_pucch_collect(const MiPucchStaged *st, uint8_t *h_bits, uint32_t *h_n_bits, uint32_t *h_rc)
{
    const uint8_t *o = (const uint8_t *)st->h_base + st->o_out;
    for (uint32_t r = 0; r < st->n_res; r++) { h_bits[2 * r] = o[4 * r]; h_bits[2 * r + 1] = o[4 * r + 1]; h_n_bits[r] = o[4 * r + 2]; h_rc[r] = o[4 * r + 3]; }
}

extern "C" {
// liblte_phy_pucch_format_1_1a_1b_channel_decode for a batch of PUCCH resources over UL device subframes
int mi_lte_pucch_decode_run(mi_lte_ctx *ctx, uint32_t N_rb_ul, uint32_t N_ant, const float *d_subframes, const mi_lte_pucch_res *h_res,
                            const float *h_tables, uint32_t n_res, uint8_t *h_bits /*[n_res][2]*/, uint32_t *h_n_bits, uint32_t *h_rc)
{
    if (!ctx || !d_subframes || !h_res || !h_tables || n_res == 0 || !h_bits || !h_n_bits || !h_rc || N_rb_ul < 6 || N_rb_ul > 100 || N_ant != 1)
        return MI_LTE_ERR_INVALID_ARG;
    for (uint32_t r = 0; r < n_res; r++)
        if (h_res[r].format > 2 || h_res[r].N_1_p_pucch >= N_rb_ul) return MI_LTE_ERR_INVALID_ARG;
    MI_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t b_res = sizeof(PucchRes) * (size_t)n_res, b_tab = sizeof(float) * PUCCH_TAB_FLOATS * (size_t)n_res, b_out = 4 * (size_t)n_res;
    const size_t o_tab = (b_res + 255) & ~(size_t)255, o_out = (o_tab + b_tab + 255) & ~(size_t)255;
    // a few resources (a per-call caller has one): descriptors, reference tables and results live in pinned host memory that the kernel reads
    // and writes itself -- three copy commands less; a batch goes through scratch
    char *base, *h_base = nullptr;
    int   rc = MI_LTE_OK;
    if (mi_ctx_small_results(ctx, o_out + b_out, (void **)&h_base, (void **)&base) != MI_LTE_OK) {
        h_base = nullptr;
        rc = mi_ctx_reserve_scratch(ctx, o_out + b_out);
        if (rc != MI_LTE_OK) return rc;
        base = (char *)ctx->scratch;
    }
    std::vector<PucchRes> res(n_res);
    for (uint32_t r = 0; r < n_res; r++) res[r] = PucchRes{h_res[r].unit, h_res[r].format, h_res[r].N_1_p_pucch};
    if (h_base) {
        MI_HIP_CHECK(ctx, mi_stream_wait_polling(ctx)); // (a kernel of an earlier call may still be reading the block)
        memcpy(h_base, res.data(), b_res);
        memcpy(h_base + o_tab, h_tables, b_tab);
    } else {
        MI_H2D(ctx, base, res.data(), b_res);
        MI_H2D(ctx, base + o_tab, h_tables, b_tab);
    }
    MI_LAUNCH(ctx, "k_pucch_decode", k_pucch_decode, dim3(n_res), dim3(64), 0, d_subframes, (uint32_t)mi_lte_ul_subframe_floats(), N_rb_ul, N_ant,
              (const PucchRes *)base, (const float *)(base + o_tab), (uint8_t *)(base + o_out));
    MI_HIP_CHECK(ctx, hipGetLastError());
    std::vector<uint8_t> o_copy;
    if (!h_base) {
        o_copy.resize(b_out);
        MI_D2H(ctx, o_copy.data(), base + o_out, b_out);
    }
    MI_HIP_CHECK(ctx, h_base ? mi_stream_wait(ctx, n_res) : hipStreamSynchronize(ctx->stream)); // (a copy into pageable memory is done when the runtime says so)
    const uint8_t *o = h_base ? (const uint8_t *)h_base + o_out : o_copy.data();
    for (uint32_t r = 0; r < n_res; r++) { h_bits[2 * r] = o[4 * r]; h_bits[2 * r + 1] = o[4 * r + 1]; h_n_bits[r] = o[4 * r + 2]; h_rc[r] = o[4 * r + 3]; }
    ctx->last_kernels = "k_pucch_decode:1";
    return MI_LTE_OK;
}

} // extern "C"
