// The launch of k_pusch_demod (uplink.hip) as a pure host rule: the constants the kernel's LDS layout and the launch share, and one function
// from a plan's sizes and settings to everything the run function launches with.  No HIP, no context, no environment: uplink.hip launches by
// it, mi_lte_pusch_plan_set_rx_antennas refuses by it, and tools/asan/pusch_launch_driver.cc prints it for tests/test_pusch_launch_cpu.py,
// which holds it against the Python restatement the GPU tests choose their sizes by (tests/pusch_demod_model.py, launch()).  (A .h, not a
// .hpp: the .hpp files are part of every .hip file's build id.)
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef PUSCH_THREADS
#define PUSCH_THREADS 256
#endif

namespace pusch_geom {

constexpr uint32_t EST_ROWS = 9; // k_pusch_demod: LDS floats kept per subcarrier of the allocation

// The LLR block behind the scrambling words: wsum[4][12] (double) | rho[12] (float), and with the noise-referenced gain or receive-antenna
// combining nsum[4] (double) behind rho
constexpr uint32_t LLR_LDS_BYTES       = 4 * 12 * sizeof(double) + 12 * sizeof(float);
constexpr uint32_t LLR_NOISE_LDS_BYTES = LLR_LDS_BYTES + 4 * sizeof(double);
static_assert(LLR_LDS_BYTES % sizeof(double) == 0, "nsum is read as double");

// Data symbols a workgroup transforms side by side: as many of 12, 6, 3, 2, 1 as keep the two ping-pong buffers (S_par M_max complex floats
// each) within ~40 KiB (all 12 up to 17 PRB)
inline uint32_t pusch_s_par(uint32_t M_max)
{
    uint32_t S_par = 12;
    while (S_par > 1 && (size_t)S_par * M_max * 2 * (2 * sizeof(float)) > 40 * 1024) S_par = S_par == 12 ? 6 : S_par == 6 ? 3 : S_par - 1; // 12, or a divisor of 6
    return S_par;
}

// Dynamic LDS of the demodulator in front of its LLR block: n_rx sets of estimate rows, the twiddles, the ping-pong buffers, the scrambling
// words (words_max and a slack word)
inline size_t pusch_lds(uint32_t n_rx, uint32_t M_max, uint32_t words_max, uint32_t S_par)
{
    return sizeof(float) * EST_ROWS * (size_t)n_rx * M_max + 2 * sizeof(float) * (size_t)M_max * (1 + 2 * S_par) + sizeof(uint32_t) * (words_max + 1);
}

inline size_t pusch_round8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

// S_par of a combining launch (include/mi_lte.h): pusch_s_par's value, stepped further down 3 -> 2 -> 1 until the launch's whole dynamic LDS
// fits `limit` bytes; 0 when it does not fit at S_par = 1.
inline uint32_t pusch_rx_s_par(uint32_t n_rx, uint32_t M_max, uint32_t words_max, size_t limit)
{
    for (uint32_t S_par = pusch_s_par(M_max); S_par >= 1; S_par = S_par == 12 ? 6 : S_par == 6 ? 3 : S_par - 1)
        if (pusch_round8(pusch_lds(n_rx, M_max, words_max, S_par)) + LLR_NOISE_LDS_BYTES <= limit) return S_par;
    return 0;
}

// The families of k_pusch_demod instantiations, one per argument block of uplink.hip (PuschNoLlr, PuschLlr, PuschLlrNoise,
// PuschLlrRx<n_rx, noise>, PuschLlrMmse<n_rx>); pusch_variant_compiled says which of them exist at which width
enum class PuschFamily { PLAIN, LLR, LLR_NOISE, LLR_RX, LLR_MMSE };

// Whether k_pusch_demod is compiled for a family at a workgroup width and antenna count: the single-antenna variants at the four widths, the
// combining ones (two or four antennas) at 192 and 256 only.  uplink.hip instantiates by it, and pusch_launch_plan below plans nothing else
// (tests/test_pusch_launch_cpu.py).
constexpr bool pusch_variant_compiled(PuschFamily family, uint32_t threads, uint32_t n_rx)
{
    const bool single    = n_rx == 1 && (threads == 64 || threads == 128 || threads == 192 || threads == 256);
    const bool combining = (n_rx == 2 || n_rx == 4) && (threads == 192 || threads == 256);
    return family == PuschFamily::LLR_RX ? combining : family == PuschFamily::LLR_MMSE ? single || combining : single;
}

struct PuschLaunch {
    PuschFamily family;
    uint32_t    threads;   // the workgroup's width: 64 / 128 / 192 / 256, a combining launch's 192 or 256
    uint32_t    n_rx;      // antennas combined: 2 or 4 for LLR_RX, 1, 2 or 4 for LLR_MMSE, 1 otherwise
    bool        noise;     // the noise-referenced gain (LLR_NOISE, LLR_RX's NOISE argument; LLR_MMSE always)
    uint32_t    S_par;
    size_t      lds_off;   // bytes in front of the LLR block, rounded up to 8 (PLAIN: unused, 0)
    size_t      lds_bytes; // the launch's dynamic LDS
    const char *label;     // what the launch is profiled and listed as
};

// The plan's settings a launch is chosen by.  maxlog: the max-log demapper on a 3GPP plan; the rest is read for a max-log launch only --
// noise: llr_noise > 0; mmse: MMSE equalisation (mi_lte_pusch_plan_set_equaliser), read with the noise gain on only (the caller refuses an
// MMSE run without either); n_rx: the antennas.
struct PuschSettings {
    bool     maxlog, noise, mmse;
    uint32_t n_rx;
};

// The launch of a plan whose widest allocation has M_max sub-carriers and whose longest has words_max scrambling words.  lds_limit: the
// device's per-workgroup LDS, read for a combining launch only; threads_override: a validated MI_LTE_PUSCH_THREADS (0: none), which does
// not reach a combining launch.  false: a combining launch that does not fit lds_limit at S_par = 1 (*out is not a launch then).
// An MMSE launch is the noise-on launch of the same n_rx under LLR_MMSE's family and label.
inline bool pusch_launch_plan(uint32_t M_max, uint32_t words_max, const PuschSettings &s, size_t lds_limit, uint32_t threads_override, PuschLaunch *out)
{
    // Workgroup size: the kernel's phases hold 3 M, M, 2 M, 12 M / R and 12 M items (M = 12 N_prb sub-carriers) between barriers, and the
    // heavy ones (atan2f, sincosf, the divisions) are the short ones -- a workgroup much wider than 3 M leaves whole wavefronts waiting at
    // every barrier for the one that has the transcendental work (SQ_WAIT_ANY: 67 % of the wave time at 256 threads and M = 72).  Measured on
    // W5 (16 UEs x 6 PRB): 64 / 128 / 192 / 256 threads = see profiles/r04_variants_pusch_threads.txt; larger allocations keep 256.
    const uint32_t threads = threads_override ? threads_override : M_max <= 96 ? 192u : (uint32_t)PUSCH_THREADS;
    const uint32_t S_par   = pusch_s_par(M_max);
    if (!s.maxlog) {
        *out = {PuschFamily::PLAIN, threads, 1, false, S_par, 0, pusch_lds(1, M_max, words_max, S_par), "k_pusch_demod"};
        return true;
    }
    if (s.n_rx <= 1) { // the same launch with the LLR block behind the scrambling words
        const size_t off = pusch_round8(pusch_lds(1, M_max, words_max, S_par));
        *out = {s.noise ? PuschFamily::LLR_NOISE : PuschFamily::LLR, threads, 1, s.noise, S_par, off, off + (s.noise ? LLR_NOISE_LDS_BYTES : LLR_LDS_BYTES), "k_pusch_demod_llr"};
        if (s.mmse && s.noise) { out->family = PuschFamily::LLR_MMSE; out->label = "k_pusch_demod_llr_mmse"; } // LLR_NOISE's launch in every other field
        return true;
    }
    // combining: n_rx sets of estimate rows, S_par stepped down until the whole launch fits, the LLR block always the noise launch's
    const uint32_t S_rx = pusch_rx_s_par(s.n_rx, M_max, words_max, lds_limit);
    const size_t   off  = pusch_round8(pusch_lds(s.n_rx, M_max, words_max, S_rx ? S_rx : 1));
    *out = {PuschFamily::LLR_RX, M_max <= 96 ? 192u : 256u, s.n_rx, s.noise, S_rx, off, off + LLR_NOISE_LDS_BYTES, "k_pusch_demod_llr_rx"};
    if (s.mmse && s.noise) { out->family = PuschFamily::LLR_MMSE; out->label = "k_pusch_demod_llr_mmse"; } // LLR_RX's launch in every other field, and its refusal
    return S_rx != 0;
}

} // namespace pusch_geom
