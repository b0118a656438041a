// The launch of the PDSCH demodulators (chain.hip: k_pdsch_demod, k_pdsch_demod_llr) as a pure host rule: the constants and roundings the
// kernels' LDS layout and the launch share, the sizes plan_layout accumulates per allocation, and one function from those sizes and a plan's
// settings to everything pdsch_demod launches with.  No HIP, no context, no environment: chain.hip launches by it, and
// tools/asan/pdsch_launch_driver.cc prints it for tests/test_pdsch_launch_cpu.py, which holds it against a Python restatement of the layout.
// (A .h, not a .hpp: the .hpp files are part of every .hip file's build id.)
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define PDSCH_HD __host__ __device__
#else
#define PDSCH_HD
#endif

namespace pdsch_geom {

// Dynamic LDS of both kernels, in 32-bit words: tab[max_pairs + 1] (uint2: offset, mask | position) | cw[words_al] | the soft-bit block.
// Both roundings keep what follows 16-byte aligned.
PDSCH_HD constexpr uint32_t pairs_words(uint32_t max_pairs) { return (2 * (max_pairs + 1) + 3u) & ~3u; }
// the scrambling words and the slack word that put_bits' two-word window reads behind the last one
PDSCH_HD constexpr uint32_t words_al(uint32_t max_words) { return (max_words + 1u + 3u) & ~3u; }

constexpr uint32_t E_LDS_MAX   = 32 * 1024; // the soft-bit block: an allocation's soft bits are assembled in LDS up to this many bytes
constexpr uint32_t LLR_THREADS = 256;       // k_pdsch_demod_llr's fixed width (its thread -> (pair, sub-carrier) map is 21 pairs of 12)
constexpr uint32_t MAX_WORDS   = 4095;      // plan_layout refuses a longer allocation: the scrambling tables hold 4096 words and the
                                            // demodulator reads one word past the allocation's last
constexpr uint32_t MAX_PRB     = 110;       // the widest carrier a plan can name (36.211: N_RB^max,DL)
// the kernels' static LDS, which they assert against their own arrays: k_pdsch_demod's qam_lut (uint2[64]), k_pdsch_demod_llr's w_wave (double[4])
constexpr uint32_t REF_STATIC_LDS = 64 * 8, LLR_STATIC_LDS = 4 * 8;

// k_pdsch_demod's `flags`: the packed hand-over (soft_pack.h), and the scrambling words word by word from the tables as before gold_run.h
enum : uint32_t { DEMOD_PACK = 1u, DEMOD_GOLD_TABLE = 2u };

// What the demodulator's launch is sized by, over a plan's allocations: the pair table's entries, the scrambling words of the longest
// allocation, and for the packed hand-over the words of the longest allocation that stays bytes (BPSK / QPSK) and the symbols of the longest
// 16QAM / 64QAM one
struct PdschDemodSizes {
    uint32_t max_pairs = 0, max_words = 0, max_words_lo = 0, max_symb_hi = 0;

    // one allocation of N_prb resource blocks behind a control region of cfi symbols; returns the upper bound of its soft-bit count
    constexpr uint32_t add(uint32_t N_prb, uint32_t cfi, uint32_t mod_type)
    {
        const uint32_t Qm = mod_type == 3 ? 6 : mod_type == 2 ? 4 : mod_type == 1 ? 2 : 1;
        const uint32_t pairs = (14 - cfi) * N_prb, e_max = pairs * 12 * Qm, words = (e_max + 31) / 32;
        if (max_pairs < 14 * N_prb) max_pairs = 14 * N_prb; // the demodulator's pair table spans all 14 symbols
        if (max_words < words) max_words = words;
        if (mod_type >= 2) { if (max_symb_hi < pairs * 12) max_symb_hi = pairs * 12; }
        else if (max_words_lo < words) max_words_lo = words;
        return e_max;
    }
};

// The families of demodulator instantiations: k_pdsch_demod<true>, <true, true>, <false>, and k_pdsch_demod_llr<N_ANT, PdschLlrGain |
// PdschLlrNoise>
enum class PdschFamily { REF_ONE_PORT, REF_ONE_PORT_COMPACT, REF_PORTS, LLR, LLR_NOISE };

// Which instantiation exists: the reference demapper's single-port kernel, its compact-estimate form and the 2 / 4-port one; max-log on one
// port and on two or four (transmit diversity), with and without the noise gain.  chain.hip instantiates by it, and pdsch_launch_plan below
// plans nothing else (tests/test_pdsch_launch_cpu.py).
constexpr bool pdsch_variant_compiled(PdschFamily family, uint32_t n_ant)
{
    return family == PdschFamily::REF_ONE_PORT || family == PdschFamily::REF_ONE_PORT_COMPACT ? n_ant == 1
           : family == PdschFamily::REF_PORTS                                                  ? n_ant == 2 || n_ant == 4
                                                                                               : n_ant == 1 || n_ant == 2 || n_ant == 4;
}

struct PdschLaunch {
    PdschFamily family;
    uint32_t    n_ant;       // the plan's ports: 1, 2 or 4
    uint32_t    threads;     // the workgroup's width
    uint32_t    pairs_al;    // words of the pair table
    uint32_t    words_al;    // words of the scrambling sequence behind it
    uint32_t    e_cap;       // bytes of soft bits an allocation may assemble in the block (0: every allocation stores directly)
    size_t      lds_bytes;   // the launch's dynamic LDS
    uint32_t    flags;       // DEMOD_PACK | DEMOD_GOLD_TABLE
    const char *label;       // what the launch is profiled and listed as
    bool        noise_first; // k_dl_crs_noise runs in front (the noise-referenced gain)
};

// The launch of a plan with these sizes on n_ant ports.  compact: the compact channel estimate (single port, reference demapper); maxlog:
// the max-log demapper, noise: its noise-referenced gain; pack: the packed hand-over of this run (the reference demapper's: the max-log
// kernels have no such form and do not read it); gold_table: scrambling words from the tables; threads_override: MI_LTE_PDSCH_THREADS as
// read (0: none) -- it reaches the reference-demapper kernels only, and only as 64, 128, 192 or 256.
// A packed run: only the allocations that stay bytes count for e_cap, and a packed allocation's symbol masks (one byte each, at most
// 17 160: 110 resource blocks, 13 symbols) ALWAYS go through the block -- a long QPSK allocation next to them still finds its own rule
// (e_cap = 0: direct).
constexpr void pdsch_launch_plan(const PdschDemodSizes &s, uint32_t n_ant, bool compact, bool maxlog, bool noise, bool pack, bool gold_table,
                                 int threads_override, PdschLaunch *out)
{
    pack = pack && !maxlog;
    const bool     wide    = !maxlog && threads_override >= 64 && threads_override <= 256 && threads_override % 64 == 0;
    const uint32_t e_bytes = ((pack ? s.max_words_lo : s.max_words) * 32 + 63u) & ~63u;
    const uint32_t masks   = pack ? (s.max_symb_hi + 15u) & ~15u : 0u;

    out->family = maxlog ? (noise ? PdschFamily::LLR_NOISE : PdschFamily::LLR)
                         : n_ant != 1 ? PdschFamily::REF_PORTS : compact ? PdschFamily::REF_ONE_PORT_COMPACT : PdschFamily::REF_ONE_PORT;
    out->n_ant       = n_ant;
    out->threads     = wide ? (uint32_t)threads_override : LLR_THREADS;
    out->pairs_al    = pairs_words(s.max_pairs);
    out->words_al    = words_al(s.max_words);
    out->e_cap       = e_bytes <= E_LDS_MAX ? e_bytes : 0;
    out->lds_bytes   = sizeof(uint32_t) * ((size_t)out->pairs_al + out->words_al) + (out->e_cap > masks ? out->e_cap : masks);
    out->flags       = (pack ? DEMOD_PACK : 0u) | (gold_table ? DEMOD_GOLD_TABLE : 0u);
    out->label       = !maxlog ? "k_pdsch_demod" : n_ant == 1 ? "k_pdsch_demod_llr" : "k_pdsch_demod_llr_txd"; // (transmit diversity: its own profiling label)
    out->noise_first = maxlog && noise;
}

// The dynamic LDS fits a workgroup's 64 KiB next to the static arrays for every size plan_layout accepts: the widest pair table, the
// longest scrambling run and a full soft-bit block at once (no plan reaches all three)
constexpr size_t pdsch_worst_lds()
{
    PdschDemodSizes s;
    s.max_pairs    = 14 * MAX_PRB;
    s.max_words    = MAX_WORDS;
    s.max_words_lo = E_LDS_MAX / 32;
    s.max_symb_hi  = 13 * MAX_PRB * 12;
    PdschLaunch L{};
    pdsch_launch_plan(s, 1, false, false, false, true, false, 0, &L);
    return L.lds_bytes;
}
static_assert(pdsch_worst_lds() == 4 * (3084 + 4096) + E_LDS_MAX, "pair table | scrambling words | a full block");
static_assert(pdsch_worst_lds() + (REF_STATIC_LDS > LLR_STATIC_LDS ? REF_STATIC_LDS : LLR_STATIC_LDS) <= 64 * 1024, "the demodulator's LDS fits a workgroup");

} // namespace pdsch_geom
