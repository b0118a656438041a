// The launch geometry of the turbo decoders and the layout plan of a merged decode (turbo_plan.cc): integer arithmetic only, each rule
// defined once for the host code that launches (turbo.hip, bcjr.hip), the kernels that index by it and the planner.  The tables planned
// here are the contract between host and kernels: a kernel finds its block size, its tile range and its scratch offset by reading them.
// Needs no HIP runtime: tools/asan/turbo_plan_driver.cc plans on a CPU and replays the kernels' index expressions against the tables.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define MI_HD __host__ __device__
#else
#define MI_HD
#endif
#ifdef __clang__
#define MI_GLOBAL_AS __attribute__((address_space(1)))
#else
#define MI_GLOBAL_AS
#endif

// The geometry rules; the files that launch or plan by them say `using namespace turbo_geom`.
namespace turbo_geom {

MI_HD inline uint32_t kpad64(uint32_t K) { return (K + 63u) & ~63u; }

// XCD-aware block -> code block mapping for the one-workgroup-per-code-block kernels.  Workgroup b runs
// on XCD b % 8 (observed dispatch order; used for speed only), and a tile line is 64 bytes per code
// block inside a 4 KiB burst shared by 64 code blocks: giving each XCD a contiguous range of tiles keeps
// all writers (readers) of a burst behind one L2, so lines leave for HBM whole instead of in halves.
MI_HD inline uint32_t xcd_chunk(uint32_t n_cb) { return ((((n_cb + 63u) >> 6) + 7u) >> 3) << 6; } // code blocks per XCD
MI_HD inline uint32_t xcd_cb(uint32_t b, uint32_t n_cb) { return (b & 7u) * xcd_chunk(n_cb) + (b >> 3); }
inline uint32_t cb_grid(uint32_t n_cb) { return 8 * xcd_chunk(n_cb); } // prep, vote: a workgroup per code block of every XCD's chunk

// the per-code-block kernels' workgroup: one thread per 16-step unit, 64 .. 384 threads; as a class 0 .. 5
constexpr int NCLS = 6;
inline uint32_t cb_width(uint32_t K) { return ((kpad64(K) >> 4) + 63u) & ~63u; }
inline int      cb_class(uint32_t K) { return (int)(cb_width(K) >> 6) - 1; }

// A perm workgroup handles PERM_BLOCKS code blocks one after the other (workgroup b + i * grid, i.e. the same XCD's chunk each time)
constexpr uint32_t PERM_BLOCKS = 4;
inline uint32_t perm_grid_of(uint32_t n_cb) { return ((cb_grid(n_cb) + PERM_BLOCKS - 1) / PERM_BLOCKS + 7u) & ~7u; } // a multiple of 8: b + i * grid stays on b's XCD

// the state-parallel trellis kernel (a handful of code blocks): trellises per wavefront -- one or two wavefronts per SIMD -- and its LDS
constexpr uint32_t SMALL_G = 8; // trellises per wavefront at most (4 lanes each)
inline uint32_t gpw_of(uint32_t n_tr) { return n_tr <= 2048 ? 1u : n_tr <= 4096 ? 2u : n_tr <= 8192 ? 4u : SMALL_G; }
inline size_t   siso_small_lds_bytes(uint32_t gpw, size_t Kp) { return sizeof(uint32_t) * gpw * (64 * 4 * 2 + (Kp >> 5) * 4); }

// LDS tables that replace the per-element IEEE divisions: the quantiser and the SISO output magnitude
// are functions of one small integer and a per-block constant, so each distinct value is divided once
// (with exactly the reference's float expression) and every element looks its result up.
constexpr uint32_t QTAB_N = 4096; // q(x) for |x| <= 2047 (signed index x + max on the integer path); larger maxima divide per element
constexpr uint32_t QTAB_HALF = 2048;
constexpr uint32_t MTAB_N = 256;  // w = |a|+|b| <= 254
// k_turbo_prep's LDS: mtab1 | mtab2 | reduction scratch (64 B) | { staged e [e_cap]  OVER  qtab [QTAB_N] | q(d0) [Kp] }.  The soft bits are dead once
// every wavefront has summed its own (the first block-wide maximum is the fence), the quantiser table and q(d0) are written after it: they
// share the bytes.  Before round 6 the four lay side by side -- 9.7 KB for a 64-thread workgroup, 16.7 for a 128-thread one, which held those
// widths at 4 and 4.5 wavefronts per SIMD where the registers allow 6.
constexpr uint32_t PREP_RED_AT = 2 * MTAB_N, PREP_E_AT = PREP_RED_AT + 64, PREP_QTAB_AT = PREP_E_AT, PREP_Q0_AT = PREP_QTAB_AT + QTAB_N;
MI_HD constexpr uint32_t prep_lds_bytes(uint32_t Kp, uint32_t e_cap) { return PREP_E_AT + (e_cap > QTAB_N + Kp ? e_cap : QTAB_N + Kp); }
// LDS bytes that stage a group's longest allocation: room for the zero slot behind it
inline uint32_t stage_cap(uint32_t e_max_bytes) { return (e_max_bytes + 16u + 63u) & ~63u; }
// ... and whether prep stages it: when the largest allocation of the group fits next to the block's own arrays
inline bool prep_stages(uint32_t K, uint32_t cap) { return prep_lds_bytes(kpad64(K), cap) <= 48 * 1024; }
// The merged decode's staging: room for the size's longest allocation, but no more than a lap and a quarter of the circular buffer
// (3 (K + 4) positions) -- an allocation beyond that is staged lap by lap (gather_windowed_pk), and one repeated allocation of a size
// no longer sets the occupancy of every workgroup of its width (width 64 of the mixed batch: 16 KB -> 9.7 KB per workgroup).
// Only where the LDS is what limits the occupancy -- the 64-thread width, K <= 1024, one wavefront per workgroup: 1.02 -> 0.80 ms of the mixed
// batch's prep; applied to every width it cost the 128- and 192-thread ones 0.05 and 0.11 ms (their blocks beyond a lap and a quarter pay
// two barriers per lap and their occupancy is bound by registers anyway; the log behind these figures is not among the committed profiles)
inline uint32_t merged_e_cap(uint32_t K, uint32_t e_max_bytes)
{
    const uint32_t cap = stage_cap(e_max_bytes), cap_w = (uint32_t)((15 * (size_t)(K + 4) / 4 + 64 + 63) & ~(size_t)63);
    return prep_stages(K, cap) ? (kpad64(K) <= 1024 ? (cap < cap_w ? cap : cap_w) : cap) : cap_w;
}

// Can the block-size group join a merged decode?  Every stream has at most 31 NULL slots, so a lap of the circular buffer consumes at least
// 3K - 81 soft bits: while the longest allocation makes no more than 258 laps no sum of int8 values leaves int16, and the kernels may keep the
// rate un-matching sums in pairs (SrcRateUnmatchPk), as the merged kernels do; a group beyond that takes the per-size path with 32-bit sums.
inline bool mi_turbo_ref_multi_takes(uint32_t K, uint32_t e_max_bytes) { return (e_max_bytes + (3 * K - 81) - 1) / (3 * K - 81) <= 258; }
// May the group's 16QAM / 64QAM allocations arrive as bits (soft_pack.h)?  k_turbo_prep expands them where it stages an allocation in LDS, whole or
// lap by lap; its gather straight from global memory reads bytes.  That gather is what a group with 32-bit sums gets when its longest allocation
// does not fit the LDS block (hundreds of laps at a small size) -- a run that holds such a group keeps the byte hand-over for all its allocations.
inline bool mi_turbo_ref_reads_packed(uint32_t K, uint32_t e_max_bytes) { return mi_turbo_ref_multi_takes(K, e_max_bytes) || prep_stages(K, stage_cap(e_max_bytes)); }

// The scratch of one REF decode: eight byte arrays of arr_bytes each (every size's tiles of 64 code blocks x kpad64(K) steps), three
// arrays of traceback words of half that, three of the trellis passes' sign words of an eighth (a bit per step; arr_bytes is a multiple of
// 4096), and a 32-byte descriptor (CbDesc) per code-block slot, the slots rounded up to whole tiles
constexpr int    N_BYTE_ARRAYS = 8; // X0 X1 X2 I0 M1 M2 I1 M3
constexpr size_t CB_DESC_BYTES = 32;
inline size_t ref_scratch_bytes(size_t arr_bytes, size_t n_slots) { return N_BYTE_ARRAYS * arr_bytes + 3 * (arr_bytes / 2) + 3 * (arr_bytes / 8) + ((n_slots + 63) & ~(size_t)63) * CB_DESC_BYTES; }

} // namespace turbo_geom

// the REF decode of a plan's block-size groups: many sizes in one launch set (KSeg, turbo.hip: mi_turbo_ref_multi) or size by size
struct MiKGroup { uint32_t K, n_cb, cb_base, e_max; }; // a block size's code blocks: slots cb_base .. cb_base + n_cb of the batch's code-block order; e_max: its longest allocation's soft bits

// One block size of a MERGED decode (mi_turbo_ref_multi: a PDSCH batch whose allocations have many code-block sizes -- a cell's TTIs
// have dozens of the 188).  Launched size by size such a batch is ~7 launches per size in series, each far too small for the device (a
// trellis walk is as long for one tile as for a thousand); merged, every kernel is launched ONCE over the tiles / code blocks of
// all sizes (the per-code-block kernels once per workgroup width, 64 .. 384 threads), and what the per-size launches pass as kernel
// arguments -- K, the block count, the interleaver and rank tables, where the size's tiles lie in the scratch arrays -- is read from
// this table by the workgroup (wavefront) at its start: one scalar load of its index in `map`, then scalar loads of the row.
struct KSeg {
    uint32_t        K, n_cb, cb_base, n_tiles; // cb_base: the size's first slot in the batch's code-block order (cb_alloc, desc)
    uint32_t        wg_cb;                     // first workgroup of the size in its prep / vote launch (a multiple of 8: blockIdx % 8 = XCD)
    uint32_t        wg_perm, perm_grid;        // the same for perm, and the size's own grid there (a workgroup takes PERM_NB blocks grid apart)
    uint32_t        e_cap;                     // LDS bytes prep stages an allocation's soft bits in (0: gathers from global memory)
    uint32_t        wv1, wv23;                 // first wavefront of the size in SISO pass 1 / passes 2 + 3
    uint64_t        arr_off;                   // where the size's tiles start in each of the eight byte arrays (traceback words: half of it, sign words: an eighth)
    // mi_ctx_turbo_tables / rm_rank_tables of K.  Typed as GLOBAL pointers: a pointer that comes out of memory is otherwise of unknown address
    // space and every load through it a flat_load, which counts against the LDS counter too -- k_turbo_prep's LDS gathers then waited for its
    // table loads (W4 as a merged decode: 4.88 ms, 4.53 without them)
    MI_GLOBAL_AS const uint16_t *pi, *inv2, *tabs;
    MI_GLOBAL_AS const uint32_t *nnn;
    uint32_t        ws1, ws23;                 // first workgroup of the size in the state-parallel trellis kernel's launches (a handful of blocks: k_turbo_siso_small)
    uint64_t        pad;
};
static_assert(sizeof(KSeg) == 96, "KSeg is read with scalar loads: keep it a multiple of 16 bytes");
struct MultiArgs { const KSeg *segs; const uint32_t *map; }; // map: per 512 workgroups (prep, vote: a size's grid is a multiple of that), per 128 (perm), per wavefront (siso) the index of its size

struct MiMultiGeom { // launch geometry derived from the groups; classes = workgroup widths 64 (c + 1)
    uint64_t arr_bytes = 0;                           // bytes of one scratch array over all sizes
    uint32_t n_slots = 0, n_wv1 = 0, n_wv23 = 0;
    uint32_t grid_cb[6] = {0}, grid_perm[6] = {0}, lds_prep[6] = {0}, kp_max[6] = {0};
    uint32_t map_cb[6] = {0}, map_perm[6] = {0}, map_wv1 = 0, map_wv23 = 0; // where each launch's map starts (entries)
    uint32_t ord_wv1 = 0, ord_wv23 = 0, n_ord1 = 0, n_ord23 = 0;             // the trellis kernel's launch order: launched wavefront -> wavefront of the map (entries; 0 = none)
    uint32_t siso_pad1 = 0, siso_pad23 = 0;                                  // dynamic LDS the trellis kernel is launched with: it holds nothing, it limits the resident workgroups per compute unit
    int      one_size[6] = {-1, -1, -1, -1, -1, -1};   // the index of a width's ONLY size (its prep launch then takes the per-size kernel), -1 otherwise
    uint64_t off_one[6] = {0}; uint32_t e_cap_one[6] = {0};
    uint32_t map_ws1 = 0, map_ws23 = 0, n_ws1 = 0, n_ws23 = 0, gpw1 = 1, gpw23 = 1, kp_all = 0; // the state-parallel trellis kernel's launches (a handful of blocks)
    size_t   map_off = 0;                             // bytes from the table's start to the maps
};

// A merged decode's tables as the device reads them -- segs, then at byte map_off the maps (padded to 16 bytes): prep / vote maps by class,
// perm maps by class, wv1, wv23, ord1, ord23, ws1, ws23 -- and the launches' geometry.  The rows' four table pointers are the caller's.
struct MiMultiPlan { std::vector<KSeg> segs; std::vector<uint32_t> map; MiMultiGeom geom; };
// `groups` in ascending K, cb_base = the group's first slot.  MI_LTE_OK, or MI_LTE_ERR_INVALID_ARG with *err (where err is given) set where there is a message.
int mi_turbo_multi_plan(const MiKGroup *groups, uint32_t n_groups, MiMultiPlan *out, const char **err);
