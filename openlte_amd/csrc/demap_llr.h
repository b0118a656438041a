// MI_LTE_DEMAP_MAXLOG (include/mi_lte.h): the max-log LLR arithmetic shared by the 3GPP plans' opt-in demappers, k_pdsch_demod_llr<N_ANT>
// (chain.hip: one kernel for one port and for transmit diversity on two or four) and k_pusch_demod_llr (uplink.hip).
#pragma once
#include <cstdint>

// The max-log LLRs of one axis of the Gray-mapped square constellation (36.211 7.1.2-7.1.4) in their piecewise-linear closed form, from
// t = Re or Im of z = y conj(h) and w = |h|^2, without dividing: with a = |t| and D = A w the axis levels sit at a = D, 3D, 5D, 7D, and
// w (min_{S1} (u - s)^2 - min_{S0} (u - s)^2) = min_{S1} s (w s - 2 t) - min_{S0} s (w s - 2 t).  lam[0]: the sign bit, lam[1] / lam[2]: the
// amplitude bits (b2 / b4 of the real part, b3 / b5 of the imaginary part).  In double: the differences a - k D cancel where a symbol sits next
// to a level, and in float their rounding alone -- some 2^-24 T k (k + 1) w / wbar of a soft-bit step under the automatic gain -- would reach
// the 2^-16 the bytes are pinned to the float64 model with (tests/demap_llr_model.py); in double the products of two floats are exact and
// kernel and model run the same operations.  The kernel waits for its loads, not for its arithmetic (profiles/demap_llr_timing.txt).
template <uint32_t MOD> __device__ __forceinline__ void llr_axis(double t, double w, double (&lam)[3])
{
    constexpr double A = MOD == 3 ? 0.15430334996209191 : MOD == 2 ? 0.31622776601683794 : 0.70710678118654752; // 1/sqrt(42), 1/sqrt(10), 1/sqrt(2)
    const double a = fabs(t), D = A * w;
    if (MOD == 1) lam[0] = 4 * A * t;
    else if (MOD == 2) {
        lam[0] = a <= 2 * D ? 4 * A * t : copysign(8 * A * (a - D), t);
        lam[1] = 4 * A * (2 * D - a);
    } else {
        const double k = a < 2 * D ? 0.0 : a < 4 * D ? 1.0 : a < 6 * D ? 2.0 : 3.0;
        lam[0] = copysign(4 * A * (k + 1) * (a - k * D), t);
        lam[1] = a < 2 * D ? 8 * A * (3 * D - a) : a < 6 * D ? 4 * A * (4 * D - a) : 8 * A * (5 * D - a);
        lam[2] = a < 4 * D ? 4 * A * (a - 2 * D) : 4 * A * (6 * D - a);
    }
}
// v = clamp(rint(g lam), -127, 127), ties to even; 0 when g lam is not finite
__device__ __forceinline__ int llr_byte(double g, double lam)
{
    const double x = g * lam;
    return fabs(x) <= 1.7976931348623157e308 ? (int)fmin(fmax(rint(x), -127.0), 127.0) : 0;
}
