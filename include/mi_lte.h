/*
 * mi_lte.h -- C-ABI of the MI355X-native LTE receive chains (libmi_lte.so): the downlink hot path (front end, PDSCH,
 * turbo), and -- widened one row at a time -- the eNodeB uplink (SC-FDMA front end, PUSCH, PRACH), the downlink control
 * region (PCFICH, PDCCH, PBCH) and initial synchronisation (coarse timing, PSS, SSS).
 *
 * Drop-in boundary for the hot path of mgp25/OpenLTE's liblte_phy (reference paths are relative to
 * the reference root).  The reference has no plugin/FFI mechanism: its apps link liblte statically
 * and call C++-mangled liblte_phy_* functions over caller-visible structs (liblte/hdr/liblte_phy.h).
 * The binding a maintainer adds is therefore a small C++ translation unit that includes the
 * reference's own liblte_phy.h, defines the liblte_phy_* symbols of this path and forwards to the
 * entry points below (shim/liblte_phy_shim.cc in this repo).
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types.  Pointers named d_* are DEVICE pointers
 *    (HIP memory on the context's GPU, from mi_lte_malloc or any other HIP allocator);
 *    pointers named h_* are HOST pointers.
 *  - every batch function returns MI_LTE_OK (0) or a negative mi_lte_status; decode verdicts
 *    (LIBLTE_ERROR_ENUM values, liblte/hdr/liblte_common.h:59-65) are reported per block in
 *    output arrays, never through the return code.  The per-call *_host forms at the end mirror the
 *    reference's own functions instead: negative on infrastructure errors, else the LIBLTE_ERROR_ENUM value.
 *  - one mi_lte_ctx per GPU and per host thread (the reference's LIBLTE_PHY_STRUCT is likewise not
 *    re-entrant: all its scratch lives in the struct).  All work is issued on the context's stream.
 *  - there is NO CPU fallback: if no gfx950 device is usable every entry point fails loudly.
 */
#ifndef MI_LTE_H
#define MI_LTE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_LTE_VERSION 100

typedef enum {
    MI_LTE_OK               = 0,
    MI_LTE_ERR_INVALID_ARG  = -1, /* NULL / out-of-range argument (reference: LIBLTE_ERROR_INVALID_INPUTS) */
    MI_LTE_ERR_NO_DEVICE    = -2, /* no usable gfx950 GPU: the product path has no CPU fallback          */
    MI_LTE_ERR_HIP          = -3, /* a HIP runtime call failed; see mi_lte_last_error                    */
    MI_LTE_ERR_UNSUPPORTED  = -4, /* outside the envelope (e.g. multi-code-block transport blocks)       */
    MI_LTE_ERR_NOMEM        = -5
} mi_lte_status;

/* per-block verdicts, numerically identical to LIBLTE_ERROR_ENUM (liblte_common.h:59-65) */
enum { MI_LTE_DECODE_SUCCESS = 0, MI_LTE_DECODE_INVALID_INPUTS = 1, MI_LTE_DECODE_FAIL = 2, MI_LTE_DECODE_INVALID_CRC = 3,
       MI_LTE_DECODE_INVALID_CONTENTS = 4 };

typedef struct mi_lte_ctx mi_lte_ctx; /* opaque */

/* ---------------------------------------------------------------- context, memory, timing */
int         mi_lte_version(void);
/* identity of the device code this library was built from: "file.hip:hhhhhhhhHHHHHHHH;" per kernel source (sha1 of the file, sha1 of the
 * shared headers, eight hex digits each).  The committed profiler tables (profiles/pmc_traffic_*.json, sq_counters_*.json) carry the id of
 * the build they were measured on; bench.py reports their numbers only for kernels whose file has not changed since. */
const char *mi_lte_build_id(void);
int         mi_lte_device_count(void);
int         mi_lte_ctx_create(int device, mi_lte_ctx **out);
void        mi_lte_ctx_destroy(mi_lte_ctx *ctx);
const char *mi_lte_last_error(const mi_lte_ctx *ctx);
const char *mi_lte_device_name(const mi_lte_ctx *ctx);
void       *mi_lte_stream(const mi_lte_ctx *ctx); /* the hipStream_t all work is issued on */

int mi_lte_malloc(mi_lte_ctx *ctx, size_t bytes, void **d_ptr);
int mi_lte_free(mi_lte_ctx *ctx, void *d_ptr);
int mi_lte_memset(mi_lte_ctx *ctx, void *d_ptr, int value, size_t bytes);
int mi_lte_memcpy_h2d(mi_lte_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int mi_lte_memcpy_d2h(mi_lte_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int mi_lte_sync(mi_lte_ctx *ctx);

/* HIP-event stopwatch on the context's stream (what bench.py times kernels with) */
int mi_lte_timer_start(mi_lte_ctx *ctx);
int mi_lte_timer_stop(mi_lte_ctx *ctx, float *elapsed_ms); /* records, synchronises, returns ms */

/* What a streaming kernel reaches on this device ("use the measured copy bandwidth as a second denominator"): a 16-bytes-per-lane
 * copy of `bytes` (a multiple of 16) from one scratch buffer to another, `reps` launches between two events on the context's stream, in
 * three kernel shapes; *gb_per_s = the best shape's 2 * bytes * reps / time (bytes read + bytes written). */
int mi_lte_device_copy_rate(mi_lte_ctx *ctx, size_t bytes, uint32_t reps, double *gb_per_s);
/* the last call's three kernel shapes (one 16-byte access per thread; the same with the non-temporal hint; a grid-stride loop): *gb_per_s
 * was their best */
int mi_lte_device_copy_rates(const mi_lte_ctx *ctx, double *out3);

/* Per-kernel timing: when enabled every kernel launch the library issues is bracketed by a pair
 * of HIP events on the context's stream.  The report is "kernel:launches:total_ms;..." since the
 * last reset (this is how bench.py measures the dominant kernel's average duration live). */
int         mi_lte_profile_enable(mi_lte_ctx *ctx, int on);
int         mi_lte_profile_reset(mi_lte_ctx *ctx);
const char *mi_lte_profile_report(mi_lte_ctx *ctx);

/* ---------------------------------------------------------------- DL front end
 * Replaces liblte_phy_get_dl_subframe_and_ce() (liblte/hdr/liblte_phy.h:1170-1177, implementation
 * liblte/src/liblte_phy.cc:5905-6200) for a batch of independent subframe "units": 14 OFDM symbol
 * FFTs + the look-ahead symbols the interpolation needs (symbol 14 = the next subframe's first symbol;
 * with N_ant = 4 also symbol 15, which only ports 2 and 3 read -- row 15 is not produced for N_ant <= 2;
 * the window starts one sample early, liblte_phy.cc:8621) and CRS channel estimation / interpolation for N_ant ports.
 *
 * Samples: either interleaved int8 I,Q (the capture file format the reference's callers convert
 * from, LTE_fdd_dl_file_scan/src/LTE_fdd_dl_fs_samp_buf.cc:657-694) in d_samples_a, or planar fp32
 * i_samps / q_samps (the reference API's own arguments) in d_samples_a / d_samples_b.
 * d_unit_start[u] is the sample index of unit u's subframe start (the reference's
 * frame_start_idx + subfr_num*N_samps_per_subfr); a unit reads up to start + 30720 + 4400 samples at
 * 30.72 MHz (scaled for smaller FFT sizes).
 *
 * Output: one "device subframe" per unit, mi_lte_subframe_floats(N_ant) floats, laid out like the
 * receive half of LIBLTE_PHY_SUBFRAME_STRUCT (liblte_phy.h:226-239) with row stride 1200:
 *     rx_symb_re[16][1200] rx_symb_im[16][1200] rx_ce_re[N_ant][16][1200] rx_ce_im[N_ant][16][1200]
 * (channel-estimate rows 14,15 are never written, as in the reference). */
typedef enum {
    MI_LTE_IQ_I8 = 0, MI_LTE_IQ_F32_PLANAR = 1,
    MI_LTE_IQ_ALL_ROWS = 0x100, /* OR into sample_format for mi_lte_dl_frontend_batch: produce symbol row 15 for N_ant <= 2 as well, as the
                                  reference's struct holds it (the per-call host form and the shim set it) */
    MI_LTE_CE_COMPACT = 0x200  /* OR into sample_format of BOTH mi_lte_dl_frontend_batch and mi_lte_pdsch_plan_create (single-port cells): the
                                  estimator stops after the frequency direction and leaves, instead of the 14 estimate rows, the magnitude and
                                  phase rows at the five CRS symbols (rows 0-4 of rx_ce_re = magnitude, rows 0-4 of rx_ce_im = phase); the PDSCH
                                  demodulator then runs the reference's time interpolation (liblte_phy.cc:6119-6190) itself, for its own
                                  resource elements only.  Same arithmetic in the same order, so soft bits and decoded blocks are identical
                                  to the full form; 172 KB per subframe less HBM traffic.  Device subframes in this form are for the PDSCH
                                  chain only (the control-channel decoders and the host forms want the estimate rows). */
} mi_lte_iq_format;
typedef struct {
    uint32_t fft_size;      /* 128, 256, 512, 1024, 2048 = N_samps_per_symb (liblte_phy.cc:2226-2274) */
    uint32_t N_rb_dl;       /* 6..100 */
    uint32_t N_ant;         /* 1, 2, 4 */
    uint32_t sample_format; /* mi_lte_iq_format */
} mi_lte_dl_cfg;

size_t mi_lte_subframe_floats(uint32_t N_ant);
int    mi_lte_dl_frontend_batch(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const void *d_samples_a,
                                const void *d_samples_b, const uint64_t *d_unit_start, const uint32_t *d_subfr_num,
                                const uint32_t *d_n_id_cell, uint32_t n_units, float *d_subframes);

/* ---------------------------------------------------------------- PDSCH allocations
 * Compact form of LIBLTE_PHY_ALLOCATION_STRUCT (liblte/hdr/liblte_phy.h:684-702): the fields
 * liblte_phy_pdsch_channel_decode reads, plus the index of the subframe unit the allocation lives in. */
typedef struct {
    uint32_t unit;           /* index into the batch of device subframes                         */
    uint32_t mod_type;       /* LIBLTE_PHY_MODULATION_TYPE_ENUM: 0 BPSK 1 QPSK 2 16QAM 3 64QAM     */
    uint32_t tbs;            /* transport block size in bits                                     */
    uint32_t rv_idx;
    uint32_t tx_mode;
    uint32_t rnti;
    uint32_t N_prb;
    uint32_t n_pdcch_symbs;  /* control-region size of the allocation's subframe (the reference's N_pdcch_symbs argument, 1..4); 0 = the
                                plan's.  mi_lte_pdcch_decode_run fills it in the allocations it returns, so that the DCIs of a capture's
                                subframes -- each with its own CFI -- go into ONE plan */
    uint8_t  prb[2][112];    /* PRB indices per slot (alloc->prb[L/7][...]), first N_prb valid    */
} mi_lte_pdsch_alloc;

/* ---------------------------------------------------------------- PDSCH decode
 * Replaces liblte_phy_pdsch_channel_decode() (liblte/hdr/liblte_phy.h:906-913, implementation
 * liblte/src/liblte_phy.cc:3690-3853) and, under it, dlsch_channel_decode() (:12762-12872) for a
 * batch of allocations over a batch of device subframes produced by mi_lte_dl_frontend_batch:
 * RE extraction, pre-decoding (single port, or the reference's transmit-diversity combiner),
 * layer de-mapping, modulation de-mapping, descrambling, turbo rate un-matching
 * (liblte_phy_rate_unmatch_turbo, liblte_phy.h:1311-1323), REF-mode turbo decoding, filler removal
 * and the CRC24A check.  M_dl_harq = 8 and N_soft = 250368 are fixed as in the reference (:3843-3844).
 *
 * Envelope: one code block per transport block (tbs + 24 <= 6144); larger ones make plan_create
 * return MI_LTE_ERR_UNSUPPORTED (the reference's own multi-block path is broken).  The opt-in 3GPP transport-block
 * mode below (mi_lte_pdsch_plan_create_3gpp) decodes them as 36.212 specifies.
 *
 * A plan holds the device copy of the allocation list and its grouping by code-block size, so a
 * repeated schedule (the benchmark, or a semi-static grant pattern) pays for planning once.
 * Outputs of run():  d_out_bits[a*out_stride + i], i < tbs: decoded transport block of allocation a,
 * one bit per byte (the reference's out_bits), meaningful when d_status[a] == 0;
 * d_status[a]: 0 = LIBLTE_SUCCESS, 2 = LIBLTE_ERROR_DECODE_FAIL (CRC mismatch). */
typedef struct mi_lte_pdsch_plan mi_lte_pdsch_plan;
int      mi_lte_pdsch_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs,
                                  const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, mi_lte_pdsch_plan **out);
void     mi_lte_pdsch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pdsch_plan *plan);
/* A plan whose allocation list changes from run to run -- a capture, where every subframe brings its own DCIs
 * (LTE_fdd_dl_file_scan/src/LTE_fdd_dl_fs_samp_buf.cc:445-515 decodes what liblte_phy_pdcch_channel_decode just found): the device arrays
 * and a pinned staging block are sized once (at most max_alloc allocations with at most max_soft_bytes of soft bits between them,
 * every allocation's share rounded up to 64 bytes), and mi_lte_pdsch_plan_assign re-plans inside them -- host grouping by code-block
 * size plus three asynchronous copies on the context's stream; no allocation, no wait.  The allocations' own n_pdcch_symbs (as
 * mi_lte_pdcch_decode_run returns them) let subframes with different control-region sizes share the plan.  The output stride of a
 * dynamic plan is that of the largest single-code-block transport block (6144 bytes, 768 packed) whatever is assigned. */
int      mi_lte_pdsch_plan_create_dynamic(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t max_alloc, size_t max_soft_bytes,
                                          mi_lte_pdsch_plan **out);
int      mi_lte_pdsch_plan_assign(mi_lte_ctx *ctx, mi_lte_pdsch_plan *plan, uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs,
                                  uint32_t n_alloc);
uint32_t mi_lte_pdsch_plan_n_alloc(const mi_lte_pdsch_plan *plan);
/* 1 when the plans decode this allocation, 0 when they refuse it: more than one code block (tbs + 24 > 6144, the reference's own C > 1
 * path is broken), N_prb == 0 or > N_rb_dl, a modulation past 64QAM, a control region outside 1..4 symbols, or a resource block
 * outside the carrier (an invalid RIV: a DCI whose 16-bit CRC matched on noise).  liblte_phy_pdsch_channel_decode (liblte_phy.cc:3690-3853)
 * fails such an allocation on its own -- the callers that plan many allocations at once (mi_lte_dl_pipeline_run_units / _run_capture,
 * mi_lte_dl_subframe_decode_host, shim/scan_batch.cc) use this test to report status 2 (LIBLTE_ERROR_DECODE_FAIL) at the allocation's
 * own index instead of failing the whole list; mi_lte_pdsch_plan_create / _assign themselves keep returning an error for it. */
int      mi_lte_pdsch_alloc_decodable(const mi_lte_dl_cfg *cfg, const mi_lte_pdsch_alloc *alloc, uint32_t N_pdcch_symbs);
/* Decoder of the plan's transport blocks: MI_LTE_TURBO_REF (default; the reference's decoder, bit-exact) or MI_LTE_TURBO_BCJR with
 * n_iter iterations (the max-log-MAP decoder of mi_lte_turbo_decode_batch; the reference has no such mode).  In BCJR mode the soft
 * bits are rate-un-matched to int8 channel values (sums of repeats saturated to +-127) and the decoded block is finished like
 * dlsch_channel_decode does (filler removed, CRC24A, one bit per byte).  qpp_spec != 0: the exact 3GPP interleaver (what a
 * standard eNodeB transmits); 0: the reference transmitter's uint32-wrapped one (they differ for 20 block sizes). */
int      mi_lte_pdsch_plan_set_decoder(mi_lte_pdsch_plan *plan, uint32_t mode /* mi_lte_turbo_mode */, uint32_t n_iter, int qpp_spec);
/* Output form: packed = 0 (default) one bit per byte, the reference's out_bits (liblte_common.h:53); packed != 0 eight bits per byte, the
 * first bit of the transport block in the most significant position of byte 0 (what liblte_bits_2_value would assemble, and SURVEY 8d's
 * K/8-byte accounting): 8x less to bring back over PCIe.  Changes mi_lte_pdsch_plan_out_stride. */
int      mi_lte_pdsch_plan_set_output(mi_lte_pdsch_plan *plan, uint32_t packed);
uint32_t mi_lte_pdsch_plan_out_stride(const mi_lte_pdsch_plan *plan);
int      mi_lte_pdsch_decode_run(mi_lte_ctx *ctx, mi_lte_pdsch_plan *plan, const float *d_subframes,
                                 const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell, uint8_t *d_out_bits,
                                 int32_t *d_status);
/* stage tap: device pointers to the descrambled soft bits (int8) of one allocation and to their count.
 * Always bytes.  Where the last run handed its 16QAM / 64QAM soft bits to the decoder as bits (mi_lte_set_soft_packed), the FIRST tap after
 * that run enqueues one kernel on the stream of the context that ran the plan, which turns every such allocation's slot into bytes in place
 * (zeros from e_len to the next 16-byte boundary); later taps before the next run only return pointers.  So read the pointers on that stream,
 * or after waiting for it, as for the run itself; the context must still exist.  The next run overwrites the slots, and a re-assignment of a
 * dynamic plan voids them. */
int      mi_lte_pdsch_plan_soft_bits(const mi_lte_pdsch_plan *plan, uint32_t alloc, const int8_t **d_e,
                                     const uint32_t **d_len);

/* ---------------------------------------------------------------- PDSCH, 3GPP transport-block mode (opt-in)
 * Transport blocks of any size in 36.213 Table 7.1.7.2.1-1, processed as 36.212 specifies rather than as the reference does (its C > 1
 * path is broken, SURVEY F4, so there is nothing to be bit-exact against).  The plans above keep their single-code-block envelope.
 *
 * Segmentation (36.212 5.1.2): B = tbs + 24 (CRC24A, gCRC24A = D^24+D^23+D^18+D^17+D^14+D^11+D^10+D^7+D^6+D^5+D^4+D^3+D+1);
 *   C = ceil(B / 6120) when B > 6144, else 1; B' = B + 24 C when C > 1; K = the smallest of the 188 turbo sizes with C K >= B'.
 *   Only F = 0 and C- = 0 is supported (every block has the same K, K C = B', no filler bits), which every size of Table 7.1.7.2.1-1
 *   satisfies; any other tbs, and tbs > 75376, is MI_LTE_ERR_UNSUPPORTED.  When C > 1 every block ends in CRC24B
 *   (gCRC24B = D^24+D^23+D^6+D^5+D+1) over its first K - 24 bits; block r carries bits r (K - 24) .. (r + 1)(K - 24) - 1 of the B-bit
 *   transport block with its CRC24A.
 * Code-block concatenation (36.212 5.1.4.1.2), N_L = 1 (single-port cells only): G = the allocation's soft-bit count (e_len of the tap
 *   below; not the reference's E, which is rounded down to a multiple of 2 Q_m), G' = G / Q_m, gamma = G' mod C,
 *   E_r = Q_m floor(G' / C) for r <= C - gamma - 1, Q_m ceil(G' / C) otherwise; block r reads soft bits [sum_{r' < r} E_r', + E_r).
 *   G depends on the subframe number (PBCH / PSS / SSS exclusions), so E_r and the offsets are computed on the device at run time.
 * Soft buffer (36.212 5.1.4.1.2): N_IR = floor(N_soft / (K_MIMO min(M_dl_harq, 8))) (K_C = 1; liblte_phy.cc:11381-11386),
 *   N_cb = min(floor(N_IR / C), K_w), k0 = R (2 ceil(N_cb / (8 R)) rv + 2), R = ceil((K + 4) / 32), K_w = 96 R.
 *   N_soft and M_dl_harq are the caller's (mi_lte_dlsch_cfg): there is no default -- the reference's fixed 250368 is a category-1 soft
 *   buffer, with which a 13-block transport block keeps ~2 400 of its ~17 500 circular-buffer positions and cannot be decoded.
 * Channel values: every block is rate-un-matched into the interleaved int8 layout d[i*3+x] of mi_lte_turbo_decode_batch (MI_LTE_SOFT_I8):
 *   repeats summed, then saturated to +-127; positions no soft bit reaches are 0.
 * Decoder: MI_LTE_TURBO_BCJR (default, 8 iterations), MI_LTE_TURBO_BCJR_EARLY or MI_LTE_TURBO_BCJR_BLOCK, always with the exact 3GPP
 *   interleaver; mi_lte_pdsch_plan_set_decoder returns MI_LTE_ERR_UNSUPPORTED for MI_LTE_TURBO_REF and MI_LTE_ERR_INVALID_ARG for
 *   qpp_spec = 0 on such a plan.  The blocks are decoded by the kernels of mi_lte_turbo_decode_batch, one launch set per block size.
 * Verdict: d_status[a] = 0 when every block's CRC24B and the transport block's CRC24A pass, else 2.  The output row holds the decoded
 *   payload (tbs bits) whatever the verdict, one bit per byte or packed (mi_lte_pdsch_plan_set_output).  A code block whose channel values
 *   are all 0 -- no information reached the decoder, e.g. an all-zero grid under MI_LTE_DEMAP_MAXLOG below -- is an erasure: its decisions
 *   are all 0, which both CRCs accept, so its _cb_ok bit is 0 and the status 2 whatever the CRCs say. */
typedef struct {
    uint32_t N_soft;    /* total soft channel bits of the UE category (36.306 Table 4.1-1), e.g. 250368, 1237248, 1827072 */
    uint32_t M_dl_harq; /* maximum number of DL HARQ processes (8 for FDD) */
} mi_lte_dlsch_cfg;

#define MI_LTE_DLSCH_MAX_CB 13 /* code blocks of the largest single-layer transport block (75376 bits) */
typedef struct {
    uint32_t C, K;                        /* code blocks, their size */
    uint32_t B;                           /* tbs + 24 */
    uint32_t N_cb, k0;                    /* soft-buffer size per block and the rv's starting position (k0 before reduction mod N_cb) */
    uint32_t E[MI_LTE_DLSCH_MAX_CB];      /* E_r */
    uint32_t off[MI_LTE_DLSCH_MAX_CB];    /* first soft bit of block r in the allocation's stream */
} mi_lte_dlsch_layout_t;

/* Host arithmetic only: the segmentation and concatenation above for one transport block of tbs bits sent with G soft bits of Q_m bits per
 * symbol (1, 2, 4, 6; G a multiple of Q_m), transmission mode tx_mode (3, 4, 8, 9: K_MIMO = 2) and redundancy version rv (0..3).
 * MI_LTE_ERR_UNSUPPORTED for tbs = 0, tbs > 75376 or F != 0; MI_LTE_ERR_INVALID_ARG for malformed arguments or a soft buffer of fewer than
 * two positions. */
int mi_lte_dlsch_layout(uint32_t tbs, uint32_t G, uint32_t Q_m, uint32_t tx_mode, uint32_t rv, const mi_lte_dlsch_cfg *dlsch,
                        mi_lte_dlsch_layout_t *out);
/* A static plan in this mode.  mi_lte_pdsch_decode_run, _set_decoder, _set_output, _out_stride, _n_alloc, _soft_bits and _destroy work on
 * it as on any plan; the output stride covers the plan's largest tbs.  MI_LTE_ERR_UNSUPPORTED: cfg->N_ant != 1, an allocation with
 * mod_type 0 (BPSK), or a tbs the segmentation above refuses; the other conditions are those of mi_lte_pdsch_plan_create. */
int mi_lte_pdsch_plan_create_3gpp(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs, const mi_lte_dlsch_cfg *dlsch,
                                  const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, mi_lte_pdsch_plan **out);
/* 1 when mi_lte_pdsch_plan_create_3gpp accepts this allocation, 0 when it refuses it */
int mi_lte_pdsch_alloc_decodable_3gpp(const mi_lte_dl_cfg *cfg, const mi_lte_dlsch_cfg *dlsch, const mi_lte_pdsch_alloc *alloc,
                                      uint32_t N_pdcch_symbs);
/* stage taps of a 3GPP plan, valid after a run; device pointers owned by the plan.
 * _cb_soft: allocation alloc's C rate-un-matched blocks, block r at *d_blocks + r * 3 (K + 4), the decoder's int8 input.
 * _cb_ok:   one uint32 per allocation; bit r set when block r's CRC24B passed (C = 1: bit 0 = the CRC24A verdict). */
int mi_lte_pdsch_plan_cb_soft(const mi_lte_pdsch_plan *plan, uint32_t alloc, const int8_t **d_blocks, uint32_t *C, uint32_t *K);
int mi_lte_pdsch_plan_cb_ok(const mi_lte_pdsch_plan *plan, const uint32_t **d_mask);

/* ---------------------------------------------------------------- PDSCH, 3GPP mode: max-log soft-decision demapping (opt-in per plan)
 * By default a 3GPP plan demaps as every plan does, with the reference's modulation_demapper (MI_LTE_DEMAP_REF): +-127 for every 16QAM /
 * 64QAM bit, a distance grade that ignores the channel gain for QPSK.  MI_LTE_DEMAP_MAXLOG replaces it by log-likelihood ratios; everything
 * after the soft-bit buffer (rate un-matching, HARQ combining, the decoders) is unchanged and sums and saturates the graded bytes.
 *
 * Per resource element (single-port cell: one resource element is one symbol), with y and h from the subframe planes:
 *   w = |h|^2, z = y conj(h), x = z / w.
 * Constellations (36.211 7.1.2-7.1.4), per axis: QPSK A = 1/sqrt(2), levels +-A, b0 / b1 = sign of I / Q (0: positive); 16QAM A = 1/sqrt(10),
 *   levels {+-1, +-3} A, b0 / b1 sign, b2 / b3 0: the inner level; 64QAM A = 1/sqrt(42), levels {+-1, +-3, +-5, +-7} A, b0 / b1 sign,
 *   b2 / b3 0: levels {1, 3}, b4 / b5 0: levels {3, 5}.
 * Log-likelihood ratio of bit k, which sits on the axis u = Re x (even k) or Im x (odd k), S0 / S1 the axis levels whose label has bit k = 0 / 1:
 *   L_k = w (min_{s in S1} (u - s)^2 - min_{s in S0} (u - s)^2), positive: bit 0 (the library's sign convention).  This is the exact max-log
 *   LLR of the Gray-mapped square constellation up to the common factor 1 / sigma^2; the kernel evaluates its piecewise-linear closed form
 *   from z and w, without dividing.
 * Soft bit: v_k = clamp(rint(g_a L_k), -127, 127), rounding to nearest, ties to even; then descrambled with the sequence of the default
 *   demapper and written to the same buffer at the same offsets with the same e_len (mi_lte_pdsch_plan_soft_bits).
 * Gain g_a of allocation a: gain > 0: g_a = gain for every allocation -- for a caller who knows sigma^2 and wants properly weighted combining
 *   across transmissions.  gain == 0, automatic, per allocation and per run: g_a = T / (4 A^2 wbar), wbar the mean of w over the allocation's
 *   M_symb resource elements and T = MI_LTE_DEMAP_AUTO_T: a noiseless symbol at the mean channel power has its least reliable bit at +-T.
 *   g_a is rounded to float before use; mi_lte_pdsch_plan_llr_gain reports it.  Under the automatic gain, retransmissions with different
 *   modulations (or channel powers) combine on this convention and not on 1 / sigma^2; mi_lte_pdsch_plan_set_llr_noise ("PDSCH, 3GPP mode:
 *   noise-referenced gain" below) puts them on 1 / sigma^2 of a CRS noise estimate.
 * Degenerate input, no NaN and no trap: a wbar that is 0 or not finite (or a g_a past the float range) gives g_a = 0 and 0 for every soft bit
 *   of the allocation; w = 0 on a resource element gives 0 for its Q_m soft bits; a non-finite g_a L_k gives 0 for that bit.  An allocation
 *   whose soft bits are all 0 decodes to status 2 (the erasure rule of the mode's verdict, above).
 * Refusals (nothing is launched, the plan stays usable and keeps its demapper): MI_LTE_ERR_INVALID_ARG for a NULL plan, an unknown mode, a
 *   negative or non-finite gain; MI_LTE_ERR_UNSUPPORTED for MAXLOG on a plan that is not in the 3GPP mode or whose sample format has
 *   MI_LTE_CE_COMPACT (left open).  mode = MI_LTE_DEMAP_REF ignores gain and restores the default path. */
#define MI_LTE_DEMAP_REF    0u /* the reference's demapper: the default */
#define MI_LTE_DEMAP_MAXLOG 1u
#define MI_LTE_DEMAP_AUTO_T 16 /* automatic gain: the least reliable bit of a noiseless symbol at the mean channel power (profiles/demap_llr_sweep.txt) */
int mi_lte_pdsch_plan_set_demapper(mi_lte_pdsch_plan *plan, uint32_t mode, float gain);
/* tap, valid after a run: one float per allocation, the gain that run used (0 before a MAXLOG run); device pointer owned by the plan.
 * MI_LTE_ERR_INVALID_ARG on a plan that is not in the 3GPP mode. */
int mi_lte_pdsch_plan_llr_gain(const mi_lte_pdsch_plan *plan, const float **d_gain);

/* ---------------------------------------------------------------- PDSCH, 3GPP mode: transmit diversity on 2 or 4 ports (opt-in)
 * The 3GPP transport-block mode for cells with two or four CRS ports: PDSCH sent with transmit diversity (36.211 6.3.3.3 layer mapping,
 * 6.3.4.3 pre-coding; TM2 and the fallback of every other mode), tx_mode = 2 in every allocation.  mi_lte_pdsch_plan_create_3gpp keeps
 * refusing such cells; these plans are made by mi_lte_pdsch_plan_create_3gpp_txdiv.  The reference's receiver for this case is
 * pre_decoder_and_matched_filter_dl (liblte_phy.cc:7694-7765), which the default demapper below restates.
 *
 * Code-block concatenation (36.212 5.1.4.1.2) with N_L = 2 (transmit diversity): G' = G / (N_L Q_m), gamma = G' mod C,
 *   E_r = N_L Q_m floor(G' / C) for r <= C - gamma - 1, N_L Q_m ceil(G' / C) otherwise -- a code block ends on a symbol pair.
 *   mi_lte_dlsch_layout_nl is mi_lte_dlsch_layout with N_L as an argument (1 or 2; G a multiple of N_L Q_m; N_L = 1 gives
 *   mi_lte_dlsch_layout's results).  Segmentation, soft buffer (N_IR with K_MIMO = 1 for tx_mode 2), channel values, decoders, verdict and
 *   HARQ combining are those of the sections above: after the soft-bit buffer only E_r and the offsets differ.
 * Extraction: the allocation's resource elements in the order of every plan (symbol -> PRB -> sub-carrier, the CRS positions of the cell's
 *   port count and the PBCH / PSS / SSS window left out); RE index idx counts them.  Their number M_ap is a multiple of N_ant for every
 *   allocation; M_symb = M_ap, G = M_symb Q_m (e_len).  Element pair n holds RE indices a = 2n and b = 2n + 1 and was sent from ports
 *   (pa, pb) = (0, 1) on two ports; on four ports from (0, 2) when n is even and (1, 3) when n is odd.  The grouping goes by RE index alone:
 *   a four-port quad may straddle two PRBs and, next to the PBCH / PSS / SSS window of an odd bandwidth, two OFDM symbols, as in the
 *   transmitter's mapping.
 * MI_LTE_DEMAP_REF (the default): the plan demodulates exactly as a plan of mi_lte_pdsch_plan_create on the same cell does -- the
 *   reference's combiner, with the estimates of the pair's first element for both, its normaliser and its modulation_demapper.  That
 *   normaliser, sqrt(a0^2 + a1^2) with a_p = |h_p|^2, equals the correct (a0 + a1) / sqrt 2 only when the two ports are equally strong;
 *   otherwise it is larger, the equalised symbols shrink and 16QAM / 64QAM decisions are biased inwards.  It is the baseline
 *   MI_LTE_DEMAP_MAXLOG is measured against (profiles/txdiv_llr_sweep.txt).
 * MI_LTE_DEMAP_MAXLOG, with y(.) and h_p(.) from the subframe planes at the pair's two resource elements, each element with its own estimates:
 *   z0 = conj(h_pa(a)) y(a) + h_pb(b) conj(y(b)),   w0 = (|h_pa(a)|^2 + |h_pb(b)|^2) / 2
 *   z1 = conj(h_pa(b)) y(b) - h_pb(a) conj(y(a)),   w1 = (|h_pa(b)|^2 + |h_pb(a)|^2) / 2
 *   t_i = z_i / sqrt 2;  symbol idx a has (t, w) = (t0, w0), symbol idx b has (t1, w1).
 *   t / w is the symbol estimate and w its reliability, 1 / sigma^2 up to the common factor; the cross term a channel that differs between
 *   a and b leaves is ignored.  L_k is the single-port section's with u = Re or Im of t / w (evaluated from t and w without dividing), and the
 *   soft byte clamp(rint(g_a L_k)) with ties to even, the descrambling, the buffer layout and e_len are that section's.
 *   Automatic gain: g_a = T / (4 A^2 wbar), wbar the mean of w over the allocation's M_symb symbols, summed in double in a fixed order (so a
 *   run is reproducible), g_a rounded to float and reported by mi_lte_pdsch_plan_llr_gain.  With both ports at unit gain w = 1: the
 *   convention T is the single-port one.  Degenerate input as there: w = 0 gives 0 for the symbol's bits, a wbar that is 0 or not finite gives
 *   g_a = 0, an all-zero code block is an erasure (status 2).
 * mi_lte_pdsch_plan_create_3gpp_txdiv: cfg->N_ant 2 or 4.  MI_LTE_ERR_UNSUPPORTED: N_ant = 1 (use mi_lte_pdsch_plan_create_3gpp), an allocation
 *   whose tx_mode is not 2, BPSK, a tbs the layout refuses, MI_LTE_CE_COMPACT in the sample format; every other condition is
 *   mi_lte_pdsch_plan_create's.  The plan works with mi_lte_pdsch_decode_run, _decode_run_harq (any pool of the context, shared with its
 *   single-port plans), _set_decoder (BCJR decoders, exact interleaver), _set_output, _soft_bits, _cb_soft, _cb_ok, _set_demapper, _llr_gain and
 *   _destroy.  Spatial multiplexing (K_MIMO = 2), dynamic plans and the packed soft-bit hand-over are not part of it. */
int mi_lte_dlsch_layout_nl(uint32_t tbs, uint32_t G, uint32_t Q_m, uint32_t N_L, uint32_t tx_mode, uint32_t rv, const mi_lte_dlsch_cfg *dlsch,
                           mi_lte_dlsch_layout_t *out);
int mi_lte_pdsch_plan_create_3gpp_txdiv(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs, const mi_lte_dlsch_cfg *dlsch,
                                        const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, mi_lte_pdsch_plan **out);
/* 1 when mi_lte_pdsch_plan_create_3gpp_txdiv accepts this allocation, 0 when it refuses it */
int mi_lte_pdsch_alloc_decodable_3gpp_txdiv(const mi_lte_dl_cfg *cfg, const mi_lte_dlsch_cfg *dlsch, const mi_lte_pdsch_alloc *alloc,
                                            uint32_t N_pdcch_symbs);

/* ---------------------------------------------------------------- DL: CRS noise estimate
 * One noise variance per subframe unit from the cell-specific reference signals, for SNR and CQI reporting and for the noise-referenced
 * gain of the next section.  It reads only the received-symbol (y) planes of a unit, so it is valid on full and on MI_LTE_CE_COMPACT planes.
 * Rows.  CRS ports p = 0 .. min(N_ant, 2) - 1 on the subframe's own CRS symbols 0, 4, 7, 11 (i = 0 .. 3; the look-ahead symbol 14 is not
 *   used): n_rows = 4 on one port, 8 on two or four.  Ports 2 and 3 are not used.
 * Pilots.  Row (p, i) has n_pil = 2 N_rb_dl pilots; pilot j sits at sub-carrier k_j = 6 j + (voff(p, i) + N_id_cell mod 6) mod 6 with
 *   voff = 3 where i + p is odd and 0 otherwise.  Its CRS value crs_j = ((1 - 2 c(2 m)) + j (1 - 2 c(2 m + 1))) / sqrt 2, m = j + 110 - N_rb_dl,
 *   c the Gold sequence of c_init = 2^10 (7 (n_s + 1) + l + 1) (2 N_id_cell + 1) + 2 N_id_cell + 1 (36.211 6.10.1.1, normal cyclic prefix),
 *   n_s = 2 subfr_num + (symbol >= 7), l = symbol mod 7 -- exactly what the channel estimator forms.
 * Least-squares product.  t_j = y(symbol, k_j) conj(crs_j) in float.  The other ports are silent on these resource elements, so
 *   t_j = h_p + noise.
 * Second difference.  d_j = t_{j-1} - 2 t_j + t_{j+1} for j = 1 .. n_pil - 2, in double: a channel that is linear over three pilots
 *   (12 sub-carriers) cancels, white noise of variance sigma^2 gives E|d|^2 = 6 sigma^2.  A delay of 4 samples at N_fft = 2048 leaves
 *   4.9e-6 |h|^2.
 * Sum and estimate.  S = sum over rows and j of |d_j|^2 in double and in a fixed order (each thread its own terms; an xor butterfly within
 *   the wavefront; the wavefronts' slots in ascending order; no atomics: two runs give identical bytes).
 *   sigma2 = (float)(S / (6 n_rows (n_pil - 2))).
 * Limits.  The relative standard deviation is about 1.36 / sqrt(n_rows (n_pil - 2)) (the PUSCH section's constant; neighbouring differences
 *   share samples); measured over 300 seeded draws (tests/test_pdsch_noise_cpu.py): 22.5 % (formula 21.5 %) at 6 RB on one port and
 *   15.2 % (15.2 %) on two, 4.6 % (4.8 %) at 100 RB on one port and 3.6 % (3.4 %) on two.
 *   Channel curvature over +-6 sub-carriers biases the estimate upwards: a delay of d samples leaves (2 - 2 cos(2 pi 6 d / N_fft))^2 / 6 of
 *   |h|^2, which is 4.9e-6 at d = 4 and N_fft = 2048 but 0.26 at N_fft = 128 (6 RB) -- there the estimate of a delayed channel is
 *   curvature, not noise.  The error of the channel estimate itself is not in sigma2.
 * mi_lte_dl_crs_noise_run: d_sigma2[unit] for n_units units of d_subframes (the layout of mi_lte_dl_frontend_batch; cfg's N_rb_dl and N_ant
 *   are used), asynchronous on the context's stream; one launch, k_dl_crs_noise.  MI_LTE_ERR_INVALID_ARG for a NULL pointer, n_units = 0, an
 *   N_rb_dl other than 6, 15, 25, 50, 75, 100, or an N_ant other than 1, 2, 4. */
int mi_lte_dl_crs_noise_run(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const float *d_subframes, const uint32_t *d_subfr_num,
                            const uint32_t *d_n_id_cell, uint32_t n_units, float *d_sigma2);

/* ---------------------------------------------------------------- PDSCH, 3GPP mode: noise-referenced gain
 * The automatic gain of MI_LTE_DEMAP_MAXLOG normalises every transmission to T at its own mean channel power: a convention, not
 * 1 / sigma^2.  For HARQ combining (next section) the LLRs of different transmissions have to be on one scale, so a MAXLOG run can take
 * its gain from the CRS noise estimate above instead: with w = |h|^2 (the mean over the pair's ports in transmit diversity) the noise on
 * t / w has variance sigma^2 / w, so g L = (scale / sigma2) L is `scale` times the max-log LLR in natural units.
 * Gain.  A run with the noise gain on first estimates sigma2[u] for u = 0 .. n_units - 1, n_units = 1 + the largest unit an allocation of
 *   the plan names (fixed at creation; the run's d_subfr_num / d_n_id_cell hold at least that many entries), then every allocation a uses
 *   g_a = (float)((double)scale / (double)sigma2[unit_a]) in place of the gain given to mi_lte_pdsch_plan_set_demapper; the sweep over the
 *   estimate planes that forms wbar is not made.  A sigma2 that is 0 or not finite, or a g_a past the float range, gives g_a = 0: every soft
 *   bit of the allocation is 0 and its status is 2 by the erasure rule.  Everything else of the LLR is as in the sections above:
 *   v = clamp(rint(g_a L), -127, 127).  mi_lte_pdsch_plan_llr_gain reports the g_a used.
 * Scale.  scale = 8 is the convention the tests and tools use: an LLR of 16 meets the int8 clamp (profiles/pdsch_harq_sweep.txt).
 * Kernels.  k_dl_crs_noise over the plan's units, then a further instantiation of k_pdsch_demod_llr (listed under that name, _txd on two and
 *   four ports) that holds the one argument more; with the setter off every run launches what it launched before, and so gives the bytes it
 *   gave.  A plan whose N_rb_dl is none of the six bandwidths refuses a noise-on run with MI_LTE_ERR_INVALID_ARG.
 * mi_lte_pdsch_plan_set_llr_noise: scale > 0: MAXLOG runs of the plan use g_a = (float)(scale / sigma2[unit_a]) in place of the gain given to
 *   mi_lte_pdsch_plan_set_demapper; scale == 0: off (the default).  Accepted on any 3GPP plan (mi_lte_pdsch_plan_create_3gpp and _3gpp_txdiv)
 *   whatever its current demapper; takes effect on MAXLOG runs only, and with it off a MAXLOG run gives the bytes it gave before.
 *   Refusals, the plan left as it was: MI_LTE_ERR_INVALID_ARG for a NULL plan and a negative or non-finite scale; MI_LTE_ERR_UNSUPPORTED on a
 *   plan that is not in the 3GPP mode. */
int mi_lte_pdsch_plan_set_llr_noise(mi_lte_pdsch_plan *plan, float scale);
/* tap: float [*n_units], sigma2 of the last MAXLOG run with the noise gain on (zeros before one); device pointer owned by the plan.
 * MI_LTE_ERR_INVALID_ARG for a NULL argument and on a plan that is not in the 3GPP mode. */
int mi_lte_pdsch_plan_llr_noise(const mi_lte_pdsch_plan *plan, const float **d_sigma2, uint32_t *n_units);

/* ---------------------------------------------------------------- PDSCH, 3GPP mode: HARQ soft combining
 * Incremental-redundancy combining of the retransmissions of a transport block in device-resident soft buffers (36.212 5.1.4.1.2: the
 * circular buffer of N_cb positions per code block that every redundancy version reads from; 36.321 5.3.2.2: when a buffer is flushed).
 *
 * Pool: n_buf soft buffers on the context's device, each sized for the largest C * 3 (K + 4) over the sizes of 36.213 Table 7.1.7.2.1-1 up
 *   to max_tbs (mi_lte_harq_buffer_bytes), as int16 in the decoder's interleaved layout d[i*3+x], block r at r * 3 (K + 4), plus a state
 *   record (mi_lte_harq_state).  What a buffer index means -- typically one (UE, HARQ process) pair -- is the caller's.  The pool belongs to
 *   a context, outlives any plan and serves every 3GPP plan of that context.  It is zeroed at creation; an empty buffer has n_tx = 0.
 * Binding: mi_lte_pdsch_decode_run_harq takes one host mi_lte_harq_bind per allocation of the plan.  buf = MI_LTE_HARQ_NONE decodes the
 *   allocation exactly as mi_lte_pdsch_decode_run does and leaves the pool alone; flags & MI_LTE_HARQ_NEW_DATA is the toggled NDI.
 * Flush rule (36.321 5.3.2.2): before combining, a bound buffer is emptied when NEW_DATA is set, when its n_tx is 0, or when its held tbs or
 *   N_cb differs from this transmission's (N_cb follows from the plan's mi_lte_dlsch_cfg and the allocation's tx_mode; C and K from tbs).
 * Combining, at every decoder position t of block r: v = the exact integer sum of this transmission's soft bits that rate un-matching maps
 *   to t (the sum the plain run saturates; 0 where none does, positions >= N_cb included), buf[t] = sat16(buf[t] + sat16(v)), and the
 *   decoder's input (and the _cb_soft tap) is clamp(buf[t], -127, 127).  From an empty buffer this is the plain run's clamp(v) byte for
 *   byte.  Modulation, N_prb, subframe (so G, E_r and the offsets) and rv may all differ between the transmissions of a transport block.
 * After the run the state holds n_tx (transmissions since the last flush, this one included) and the transport block's verdict (status,
 *   the value written to d_status).  A passing CRC does not empty the buffer: only the flush rule and mi_lte_harq_pool_reset do.
 * Refusals, returned before anything is launched, leaving pool and plan usable: MI_LTE_ERR_UNSUPPORTED for a plan not in the 3GPP mode;
 *   MI_LTE_ERR_INVALID_ARG for a NULL binding, buf >= n_buf, one buf bound twice in a run, or an allocation whose tbs exceeds the pool's
 *   max_tbs.
 * Ordering: runs on one context's stream combine in stream order.  The call does not wait for the decode; at most it waits for the previous
 *   HARQ run's binding copy to leave the pool's pinned staging block. */
typedef struct mi_lte_harq_pool mi_lte_harq_pool;
#define MI_LTE_HARQ_NONE     0xFFFFFFFFu
#define MI_LTE_HARQ_NEW_DATA 1u
typedef struct {
    uint32_t buf;   /* buffer index, or MI_LTE_HARQ_NONE */
    uint32_t flags; /* MI_LTE_HARQ_NEW_DATA */
} mi_lte_harq_bind;
typedef struct {
    uint32_t tbs, C, K, N_cb; /* the transport block the buffer holds (0 when empty) */
    uint32_t n_tx;            /* transmissions combined since the last flush; 0: empty */
    int32_t  status;          /* the last run's verdict (d_status) */
} mi_lte_harq_state;
/* host arithmetic: soft-buffer bytes per buffer of a pool for max_tbs (2 * the largest C * 3 (K + 4) over Table 7.1.7.2.1-1 sizes <= max_tbs);
 * 0 when no size of the table is <= max_tbs */
size_t mi_lte_harq_buffer_bytes(uint32_t max_tbs);
/* MI_LTE_ERR_INVALID_ARG: n_buf = 0 or > 2^24, or mi_lte_harq_buffer_bytes(max_tbs) = 0 */
int  mi_lte_harq_pool_create(mi_lte_ctx *ctx, uint32_t n_buf, uint32_t max_tbs, mi_lte_harq_pool **out);
void mi_lte_harq_pool_destroy(mi_lte_ctx *ctx, mi_lte_harq_pool *pool);
/* empties buffer buf (MI_LTE_HARQ_NONE: every buffer): soft bytes and state zeroed, on the context's stream */
int  mi_lte_harq_pool_reset(mi_lte_ctx *ctx, mi_lte_harq_pool *pool, uint32_t buf);
/* mi_lte_pdsch_decode_run on a 3GPP plan with the allocations' soft bits combined into the pool's buffers as above */
int  mi_lte_pdsch_decode_run_harq(mi_lte_ctx *ctx, mi_lte_pdsch_plan *plan, mi_lte_harq_pool *pool, const mi_lte_harq_bind *h_bind,
                                  const float *d_subframes, const uint32_t *d_subfr_num, const uint32_t *d_n_id_cell, uint8_t *d_out_bits,
                                  int32_t *d_status);
/* tap: device pointers to buffer buf's int16 blocks (mi_lte_harq_buffer_bytes(max_tbs) bytes) and to its state; either may be NULL */
int  mi_lte_harq_pool_soft(const mi_lte_harq_pool *pool, uint32_t buf, const int16_t **d_soft, const mi_lte_harq_state **d_state);

/* ---------------------------------------------------------------- turbo decode
 * Replaces turbo_decode() (liblte/src/liblte_phy.cc:10620-10845) for a batch of code blocks of one
 * size K.  Input layout is the reference's: per block 3*(K+4) soft values INTERLEAVED d[i*3+x]
 * (x = 0 systematic, 1 parity-1, 2 parity-2), positive = bit 0, the value 10000 (RX_NULL_BIT,
 * liblte_phy.cc:1620) marks a punctured position.  Blocks are contiguous: block b starts at element
 * b*3*(K+4).
 *
 *   MI_LTE_TURBO_REF   bit-exact restatement of the reference's Steps 0-14 (three hard-metric SISO
 *                      Viterbi passes + soft re-encodes + 4-way vote), including its uint32 QPP
 *                      wrap-around; de-interleaver holes read as 0.  n_iter is ignored.
 *   MI_LTE_TURBO_BCJR  fixed-point max-log-MAP (extrinsic scaled by 3/4), n_iter full iterations, int8 LLRs
 *   MI_LTE_TURBO_BCJR_BLOCK  the same decoder laid out for a HANDFUL of blocks (the per-call forms): one code block per wavefront, the
 *                      64 lanes walk 64 segments of the block, every array of the decode in LDS, one launch for all iterations.  Its
 *                      alpha recursion restarts (from the previous iteration's value) every 32-96 steps instead of every K/8, so its
 *                      output is specified by its own model (lo_turbo_decode_bcjr_block) and can differ from MI_LTE_TURBO_BCJR's on
 *                      blocks near the decoding threshold; ~4x lower latency for a single K = 6144 block.
 *                      (MI_LTE_SOFT_I8) only; qpp_spec != 0 selects the exact 3GPP interleaver instead of the
 *                      reference's wrapped one.  Not a behaviour of the reference (its decoder is REF): specified
 *                      by oracle/lte_oracle.c lo_turbo_decode_bcjr, which the kernels match bit for bit.
 *
 *   MI_LTE_TURBO_BCJR_EARLY  MI_LTE_TURBO_BCJR with hard-decision-aided early termination: from the second iteration on, a tile pair (128
 *                      code blocks that share a wavefront) stops once an iteration changes none of its hard decisions; n_iter is the most
 *                      iterations any pair runs.  A block's output is MI_LTE_TURBO_BCJR's with n_iter = the iterations its pair ran
 *                      (mi_lte_turbo_early_exit_iterations reports them).  A throughput mode of its own: never what the 8-iteration
 *                      numbers are quoted on.
 *
 * Output: d_c_bits, one decoded bit per byte, K bytes per block (the reference's c_bits). */
typedef enum { MI_LTE_TURBO_REF = 0, MI_LTE_TURBO_BCJR = 1, MI_LTE_TURBO_BCJR_BLOCK = 2, MI_LTE_TURBO_BCJR_EARLY = 3 } mi_lte_turbo_mode;
typedef enum { MI_LTE_SOFT_F32 = 0, MI_LTE_SOFT_I8 = 1, MI_LTE_SOFT_I16 = 2 } mi_lte_soft_type;

int mi_lte_turbo_decode_batch(mi_lte_ctx *ctx, const void *d_soft, mi_lte_soft_type soft_type, uint32_t K,
                              uint32_t n_cb, mi_lte_turbo_mode mode, uint32_t n_iter, int qpp_spec,
                              uint8_t *d_c_bits);

/* iterations every tile pair (code blocks 128p .. 128p + 127) of the context's last MI_LTE_TURBO_BCJR_EARLY decode ran: h_pair_iters[p] in
 * 2..n_iter; *n_pairs pairs (MI_LTE_ERR_INVALID_ARG with *n_pairs set when max_pairs is too small) */
int mi_lte_turbo_early_exit_iterations(mi_lte_ctx *ctx, uint32_t *h_pair_iters, uint32_t max_pairs, uint32_t *n_pairs, uint32_t *n_iter);

/* The reference-faithful decoder's trellis kernel comes in two shapes with identical results: code blocks on the lanes (lock-step tiles of
 * 64: the throughput shape, 64k blocks per launch) and, for a decode of at most n_cb_max code blocks, STATES on the lanes (four lanes per
 * trellis, the traceback as a parallel composition of state maps): a third of the latency when one transport block is all there is, which
 * is what a per-call caller (the shim) has.  Default 4096; 0 = always the lock-step kernel.  A tuning / test knob, not a semantic one. */
int mi_lte_set_turbo_small_batch(mi_lte_ctx *ctx, uint32_t n_cb_max);
/* A PDSCH / PUSCH decode whose allocations have several code-block sizes launches each of its kernels ONCE over the blocks of all sizes
 * (the per-code-block kernels once per workgroup width) instead of size by size; on = 0 keeps the per-size launches.  Identical results
 * (tests/test_mixed_gpu.py); a test / tuning knob like the one above.  Default on. */
int mi_lte_set_turbo_merged(mi_lte_ctx *ctx, uint32_t on);
/* A PDSCH plan run with the reference-faithful demapper and MI_LTE_TURBO_REF hands its 16QAM / 64QAM soft bits -- each exactly +127 or -127 --
 * from the demodulator to the decoder as one BIT per soft bit instead of one byte (an eighth of that array's traffic); BPSK / QPSK allocations,
 * the BCJR decoders, the 3GPP mode and PUSCH plans keep bytes.  on = 0 keeps bytes everywhere.  Identical results (tests/test_soft_pack_gpu.py),
 * and mi_lte_pdsch_plan_soft_bits returns bytes either way.  Default on; MI_LTE_NO_SOFT_PACK=1 in the environment makes every context of the
 * process start with it off.  A test / tuning knob like the two above. */
int mi_lte_set_soft_packed(mi_lte_ctx *ctx, uint32_t on);
/* The PDSCH demodulators form their scrambling words (36.211 7.2) in runs: one word per run from the basis tables, the following ones by a
 * word-wise step of the two shift registers.  on = 0 reads every word from the tables, as before.  Identical results
 * (tests/test_gold_run_gpu.py).  Default on; MI_LTE_NO_GOLD_RUN=1 in the environment turns it off for every context of the process that has
 * not been told otherwise here.  A test / tuning knob like the three above. */
int mi_lte_set_gold_recurrence(mi_lte_ctx *ctx, uint32_t on);

/* ---------------------------------------------------------------- turbo rate un-matching
 * Replaces liblte_phy_rate_unmatch_turbo() (liblte/hdr/liblte_phy.h:1311-1323, implementation
 * liblte/src/liblte_phy.cc:11246-11490) with its float interface, for n_cb code blocks that share
 * one parameter set: e bits in (N_e_bits per block), interleaved d[i*3+x] out (3*D per block, D = the
 * reference's N_dummy_bits = K+4), RX_NULL_BIT = 10000.0f where nothing was received.  chan_type uses
 * LIBLTE_PHY_CHAN_TYPE_ENUM values (0 DLSCH, 1 PCH limit the soft buffer; 2 ULSCH, 3 ULCCH do not).
 * (Inside mi_lte_pdsch_decode_run the same gather is fused into the decoder and never touches HBM.) */
int mi_lte_rate_unmatch_turbo_batch(mi_lte_ctx *ctx, const float *d_e_bits, uint32_t N_e_bits, uint32_t D,
                                    uint32_t N_codeblocks, uint32_t tx_mode, uint32_t N_soft, uint32_t M_dl_harq,
                                    uint32_t chan_type, uint32_t rv_idx, uint32_t n_cb, float *d_d_bits);

/* bytes of device scratch the decoder holds for (K, n_cb); grows on demand, reported for sizing */
size_t mi_lte_turbo_scratch_bytes(uint32_t K, uint32_t n_cb);
size_t mi_lte_turbo_bcjr_scratch_bytes(uint32_t K, uint32_t n_cb);

/* name and launch count of the kernels the last batch call issued (for bench.py / profiles) */
const char *mi_lte_last_kernels(const mi_lte_ctx *ctx);

/* ---------------------------------------------------------------- uplink (eNodeB receive side)
 * SURVEY 8f N1 / BASELINE config 5: the PUSCH receive chain of LTE_fdd_enodeb
 * (LTE_fdd_enodeb/src/LTE_fdd_enb_phy.cc:832-917 calls liblte_phy_get_ul_subframe and
 * liblte_phy_pusch_channel_decode once per scheduled UE).
 *
 * mi_lte_ul_frontend_batch replaces liblte_phy_get_ul_subframe() (liblte/hdr/liblte_phy.h:1190-1193,
 * implementation liblte/src/liblte_phy.cc:6209-6236 over samples_to_symbols_ul :8654-8692): 14 SC-FDMA
 * symbols per subframe unit; the reference's 2N-point FFT of the zero-padded N samples, of which it keeps
 * the odd bins (the half-sub-carrier shift), is computed as an N-point FFT of the samples rotated by
 * exp(-i*pi*n/N); the window starts one sample early (:8680) like the downlink one.
 * Output per unit: mi_lte_ul_subframe_floats() floats, rx_symb_re[16][1200] rx_symb_im[16][1200]
 * (rows 14, 15 unused), the receive half of LIBLTE_PHY_SUBFRAME_STRUCT. */
size_t mi_lte_ul_subframe_floats(void);
int    mi_lte_ul_frontend_batch(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg /* N_rb_dl = N_rb_ul, N_ant ignored */,
                                const void *d_samples_a, const void *d_samples_b, const uint64_t *d_unit_start,
                                uint32_t n_units, float *d_subframes);

/* Cell-level uplink configuration: the arguments of liblte_phy_ul_init() (liblte_phy.h:613-625) that the
 * PUSCH demodulation reference signals depend on (generate_dmrs_pusch, liblte_phy.cc:6868-6990); liblte_phy.h:613-625. */
typedef struct {
    uint32_t group_assignment_pusch;   /* delta_ss */
    uint32_t group_hopping_enabled;
    uint32_t sequence_hopping_enabled;
    uint32_t cyclic_shift;             /* n1_DMRS index, 0..7 */
    uint32_t cyclic_shift_dci;         /* n2_DMRS index, 0..7 */
} mi_lte_ul_cfg;

/* PUSCH demodulation reference signal of one (subframe, N_prb): 4 x 12*N_prb floats
 * (dmrs_0_re, dmrs_0_im for symbol 3; dmrs_1_re, dmrs_1_im for symbol 10).  Host function; restates
 * generate_dmrs_pusch / generate_ul_rs (liblte_phy.cc:6745-6990) with the reference's own arithmetic
 * (double-precision libm calls on float-rounded arguments), layer 0. */
int mi_lte_ul_dmrs_pusch(const mi_lte_ul_cfg *ul, uint32_t N_id_cell, uint32_t N_subfr, uint32_t N_prb, float *h_dmrs_0_re,
                         float *h_dmrs_0_im, float *h_dmrs_1_re, float *h_dmrs_1_im);

/* mi_lte_pusch_plan_* / mi_lte_pusch_decode_run replace liblte_phy_pusch_channel_decode()
 * (liblte_phy.h:722-728, implementation liblte_phy.cc:2801-2935) and ulsch_channel_decode (:12363-12501)
 * for a batch of allocations (one per scheduled UE) over a batch of uplink device subframes: RE extraction,
 * DMRS least-squares estimate + magnitude/phase interpolation (get_ulsch_ce :13718-13790), one-tap
 * equaliser (:6708-6736), transform pre-decoding (12 unnormalised backward DFTs of size 12*N_prb scaled by
 * sqrt(12*N_prb), :6627-6660 -- the reference's scaling, reproduced), de-mapping, descrambling, channel
 * de-interleaving (:12108-12225; with no RI/ACK/CQI bits it is a 12-column transpose), turbo rate
 * un-matching with the UL-SCH soft-buffer rule (N_cb = K_w), REF turbo decoding, CRC24A.
 * alloc.unit selects the subframe unit; the unit's subframe number and cell id are host arrays here because
 * the reference signals are generated on the host per (cell, subframe, N_prb).  N_prb must be one the
 * reference has an FFTW plan for: N_prb < N_rb_ul and divisible by 2, 3 or 5 (liblte_phy.cc:2360-2377);
 * single antenna, one code block per transport block.
 * Refusals of mi_lte_pusch_plan_create (and of its 3GPP forms below), all before anything is allocated on the device:
 * MI_LTE_ERR_INVALID_ARG for cfg->N_rb_dl outside 6..100 (what mi_lte_ul_frontend_batch accepts) and for a resource block outside the
 * carrier; MI_LTE_ERR_UNSUPPORTED for an allocation outside the envelope -- tbs above 6120 (more than one code block; sizes near 2^32
 * included: tbs + 24 is not formed before the bound is checked), an N_prb without a transform plan, mod_type above 3, a unit index past
 * n_units. */
typedef struct mi_lte_pusch_plan mi_lte_pusch_plan;
int      mi_lte_pusch_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul,
                                  const uint32_t *h_unit_subfr_num, const uint32_t *h_unit_n_id_cell, uint32_t n_units,
                                  const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, mi_lte_pusch_plan **out);
void     mi_lte_pusch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pusch_plan *plan);
uint32_t mi_lte_pusch_plan_out_stride(const mi_lte_pusch_plan *plan);
int      mi_lte_pusch_decode_run(mi_lte_ctx *ctx, mi_lte_pusch_plan *plan, const float *d_subframes, uint8_t *d_out_bits,
                                 int32_t *d_status);
/* stage tap: device pointer to the de-interleaved, descrambled soft bits (int8, 12*12*N_prb*Q_m of them) */
int      mi_lte_pusch_plan_soft_bits(const mi_lte_pusch_plan *plan, uint32_t alloc, const int8_t **d_e, uint32_t *n_bits);

/* ---------------------------------------------------------------- PUSCH, 3GPP transport-block mode (opt-in)
 * The uplink as 36.211 / 36.212 specify it rather than as the reference receives it.  The reference's receiver cannot decode what a UE
 * sends beyond single-block QPSK: its transform pre-decoder (liblte_phy.cc:6627-6660) multiplies the unnormalised backward DFT by
 * sqrt(M), M = 12 N_prb, where 36.211 5.3.3 needs 1 / sqrt(M), so the de-mapper sees M times the constellation point -- 16QAM and 64QAM
 * fail and every QPSK soft bit saturates at +-1 -- and ulsch_channel_decode (:12363-12501) handles one code block.  The plans above
 * reproduce both; a plan of this mode does neither.
 *
 * Demodulator: that of the plans above -- DMRS estimate, equaliser, transform pre-decoding, de-mapping, descrambling, the 12-column
 *   transpose -- with the pre-decoder's output scaled by r = (float)(1.0 / sqrt((double)M)) (one factor; the same kernel otherwise).
 *   QPSK, 16QAM and 64QAM; mod_type 0 (BPSK) is MI_LTE_ERR_UNSUPPORTED.  N_prb < N_rb_ul and divisible by 2, 3 or 5, as above, or 1
 *   (M = 12, a size 36.211 5.3.3 allows and the reference has no plan for).
 * UL-SCH (36.212 5.2.2.1-5.2.2.5, N_L = 1, no control information): CRC24A, segmentation and CRC24B as in 5.1.2 (the PDSCH 3GPP mode's:
 *   F = 0, C <= 13, every tbs of 36.213 Table 7.1.7.2.1-1), rate matching with N_cb = K_w -- the uplink has no soft-buffer limit --
 *   k0 = R (2 ceil(K_w / (8 R)) rv + 2), G = 12 * 12 N_prb * Q_m, G' = G / Q_m and E_r as in mi_lte_dlsch_layout.  Without control
 *   information the channel interleaver (5.2.2.8) is the transpose the demodulator undoes.
 * Code blocks: the kernels of the PDSCH 3GPP mode (rate un-matching into the int8 layout of mi_lte_turbo_decode_batch, repeats summed
 *   and saturated to +-127; the BCJR kernels, one launch set per block size; CRC24B, desegmentation, CRC24A).
 * Decoder: MI_LTE_TURBO_BCJR (default, 8 iterations), MI_LTE_TURBO_BCJR_EARLY or MI_LTE_TURBO_BCJR_BLOCK with the exact interleaver.
 *   mi_lte_pusch_plan_set_decoder on such a plan: MI_LTE_ERR_UNSUPPORTED for MI_LTE_TURBO_REF, MI_LTE_ERR_INVALID_ARG for qpp_spec = 0 or
 *   n_iter outside 1..64; on a plan of mi_lte_pusch_plan_create: MI_LTE_ERR_UNSUPPORTED whatever is asked (it stays the reference's chain).
 * Verdict: d_status[a] = 0 when every block's CRC24B and the transport block's CRC24A pass, else 2.  The output row holds the decoded
 *   payload (tbs bits) whatever the verdict, one bit per byte or packed (mi_lte_pusch_plan_set_output; a plan of mi_lte_pusch_plan_create
 *   has the one-bit-per-byte form only: packed != 0 is MI_LTE_ERR_UNSUPPORTED there).  The output stride covers the plan's largest tbs.
 * What is exact: everything from the int8 soft bits on (pinned to the reference's liblte_phy_rate_unmatch_turbo with channel type
 *   ULSCH and N_codeblocks = C, to the plain-C BCJR models and to a desegmentation in numpy); the soft bits' half-plane decisions equal
 *   those of the plans above byte for byte (a positive factor does not move a sign). */
/* Host arithmetic only: mi_lte_dlsch_layout with an unlimited soft buffer (N_cb = K_w) and K_MIMO = 1 -- that is, with the soft-buffer
 * configuration {MI_LTE_ULSCH_N_SOFT, MI_LTE_ULSCH_M_HARQ}, whose N_IR / 13 lies far above the largest K_w (18 528) */
#define MI_LTE_ULSCH_N_SOFT 0xFFFFFFFFu
#define MI_LTE_ULSCH_M_HARQ 1u
int mi_lte_ulsch_layout(uint32_t tbs, uint32_t G, uint32_t Q_m, uint32_t rv, mi_lte_dlsch_layout_t *out);
/* A plan in this mode: the arguments of mi_lte_pusch_plan_create.  mi_lte_pusch_decode_run, _out_stride, _soft_bits and _destroy work on it
 * as on any plan.  MI_LTE_ERR_UNSUPPORTED: BPSK, an N_prb without a transform plan, a tbs the segmentation refuses, a unit index past
 * n_units; MI_LTE_ERR_INVALID_ARG: a resource block outside the carrier.  Every refusal comes before any launch and leaves the context usable. */
int mi_lte_pusch_plan_create_3gpp(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const uint32_t *h_unit_subfr_num,
                                  const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                  mi_lte_pusch_plan **out);
int mi_lte_pusch_plan_set_decoder(mi_lte_pusch_plan *plan, uint32_t mode, uint32_t n_iter, int qpp_spec);
int mi_lte_pusch_plan_set_output(mi_lte_pusch_plan *plan, uint32_t packed);
/* stage taps of a 3GPP plan, valid after a run, with the meanings of mi_lte_pdsch_plan_cb_soft / _cb_ok; MI_LTE_ERR_INVALID_ARG on a plan of
 * mi_lte_pusch_plan_create */
int mi_lte_pusch_plan_cb_soft(const mi_lte_pusch_plan *plan, uint32_t alloc, const int8_t **d_blocks, uint32_t *C, uint32_t *K);
int mi_lte_pusch_plan_cb_ok(const mi_lte_pusch_plan *plan, const uint32_t **d_mask);

/* ---------------------------------------------------------------- control information on PUSCH in the 3GPP mode (opt-in)
 * A UE that holds an uplink grant sends its HARQ-ACK, rank indication and CQI inside that PUSCH (36.212 5.2.2.6-5.2.2.8), which changes
 * the channel interleaver from a transpose and G from 12 * 12 N_prb * Q_m.  N_L = 1, normal prefix, no SRS (N_symb = 12), FDD (no ACK
 * bundling).  The interleaver matrix has M = 12 N_prb rows and 12 columns of Q_m-bit cells; cell (r, c) is the demodulator's soft-bit
 * group at byte (r * 12 + c) * Q_m (mi_lte_pusch_plan_soft_bits, unchanged) and bits (c * M + r) * Q_m .. of the scrambled sequence.
 *   RI  (5.2.2.8): symbol i = 0 .. Qp_ri - 1 in cell (M - 1 - i / 4, col), col walking 1, 10, 7, 4 (column set {1, 4, 7, 10}).
 *   CQI then data (5.2.2.7, 5.2.2.8): q_0 .. q_(Q_cqi - 1) | f_0 .. f_(G - 1) written Q_m bits per cell row by row, skipping RI cells:
 *        G = Q_m (12 M - Qp_ri) - Q_cqi.
 *   ACK (5.2.2.8): symbol i = 0 .. Qp_ack - 1 in cell (M - 1 - i / 4, col), col walking 2, 9, 8, 3 (column set {2, 3, 8, 9}); it
 *        overwrites the data or CQI symbol of that cell.
 *   ACK / RI symbols (5.2.2.6, tables 5.2.2.6-1 .. -4): O = 1: [o0 y x .. x]; O = 2: w = (o0, o1, o0 ^ o1), symbol n carries
 *        [w[2n mod 3] w[(2n + 1) mod 3] x .. x].
 *   Scrambling (36.211 5.3.1): x -> 1, y -> the previous scrambled bit, every other bit b ^ c(i).
 * CQI is a run of Q_cqi coded bits.  Its block / convolutional code (5.2.2.6.4) is mi_lte_cqi_encode on the transmitting side and, opt-in
 * per plan, k_ulsch_cqi_decode on the receiving one (the CQI section below); without the opt-in the run stays opaque. */
typedef struct {
    uint8_t  O_ack, O_ri;   /* information bits: 0 (none), 1 or 2 */
    uint16_t Qp_ack, Qp_ri; /* coded symbols Q' (<= 4 M each) */
    uint32_t Q_cqi;         /* coded CQI bits, a multiple of Q_m */
} mi_lte_ulsch_uci;         /* all zero: no control information */
/* Q' of 36.212 5.2.2.6: min(ceil(O' * M_sc_initial * N_symb_initial * beta / sum_K_r), cap) in 64-bit integers, beta = beta_x8 / 8 (every
 * offset of 36.213 tables 8.6.3-1 .. -3 is a multiple of 1 / 8).  kind: MI_LTE_UCI_ACK / _RI (cap 4 M) or _CQI (cap 12 M - Qp_ri, and
 * O' = O + 8, the CRC, above 11 bits); M = 12 N_prb of the present subframe; sum_K_r: C * K of mi_lte_ulsch_layout. */
enum { MI_LTE_UCI_ACK = 0, MI_LTE_UCI_RI = 1, MI_LTE_UCI_CQI = 2 };
int mi_lte_ulsch_uci_qprime(uint32_t kind, uint32_t O, uint32_t beta_x8, uint32_t M_sc_initial, uint32_t N_symb_initial, uint32_t sum_K_r,
                            uint32_t N_prb, uint32_t Qp_ri, uint32_t *Qp);
/* G of an allocation with control information (5.2.2.7).  MI_LTE_ERR_INVALID_ARG: O > 2, Q' > 4 M, O = 0 with Q' != 0 or the reverse,
 * Q_cqi not a multiple of Q_m, Q_m not 2 / 4 / 6, N_prb outside 1 .. 110, G <= 0. */
int mi_lte_ulsch_uci_G(uint32_t N_prb, uint32_t Q_m, const mi_lte_ulsch_uci *uci, uint32_t *G);
/* The channel interleaver with control information (5.2.2.8) cell by cell: kind[r * 12 + c] is the cell's class, index[2 (r * 12 + c)]
 * its symbol's number in its own stream (data: f's symbol, CQI: q's symbol, RI / ACK: i), index[2 (r * 12 + c) + 1] for an ACK cell the
 * data (MI_LTE_UCI_CELL_ACK_DATA) or CQI (_ACK_CQI) symbol it overwrote, 0xFFFFFFFF elsewhere.  The transmitter below is driven by it. */
enum { MI_LTE_UCI_CELL_DATA = 0, MI_LTE_UCI_CELL_CQI = 1, MI_LTE_UCI_CELL_RI = 2, MI_LTE_UCI_CELL_ACK_DATA = 3, MI_LTE_UCI_CELL_ACK_CQI = 4 };
int mi_lte_ulsch_uci_map(uint32_t N_prb, uint32_t Q_m, const mi_lte_ulsch_uci *uci, uint8_t *kind /*[12 M]*/, uint32_t *index /*[12 M][2]*/);
/* A 3GPP plan whose allocation a carries h_uci[a] (h_uci = NULL: mi_lte_pusch_plan_create_3gpp).  After the demodulator
 *   k_ulsch_uci_gather  undoes the interleaver above (36.212 5.2.2.8): the allocation's G data soft bits in sequence order, followed by
 *                       its Q_cqi CQI soft bits, 0 where an ACK symbol overwrote one (an erasure); rate un-matching reads the former;
 *   k_ulsch_uci_decide  sums the ACK and RI symbols' soft bits 0 and 1 (36.212 5.2.2.6; a copied bit y with the descrambling of 36.211
 *                       5.3.1 undone: negated where c(i0) != c(i0 + 1)) and decides: O = 1: S[0] = sum (u0 + u1'), bit = S[0] < 0;
 *                       O = 2: u0 into S[2n mod 3], u1 into S[(2n + 1) mod 3], the first maximum of sum_j (1 - 2 w_j) S[j] over
 *                       (o0, o1) = 00, 01, 10, 11.  Integer sums: exact.  A DTX threshold on |S| is the caller's.
 * then the code blocks of a plain 3GPP plan.  Refusals on top of mi_lte_pusch_plan_create_3gpp's: whatever mi_lte_ulsch_uci_G refuses,
 * mi_lte_ulsch_layout(tbs, G, Q_m, rv) failing, and a G of fewer symbols than the transport block has code blocks (MI_LTE_ERR_INVALID_ARG). */
typedef struct {
    uint8_t ack[2], ri[2];    /* decided bits (unused ones 0) */
    int32_t S_ack[3], S_ri[3]; /* the sums behind them (O = 1: S[0] only) */
} mi_lte_ulsch_uci_result;    /* all zero for an allocation without control information */
int mi_lte_pusch_plan_create_3gpp_uci(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, const uint32_t *h_unit_subfr_num,
                                      const uint32_t *h_unit_n_id_cell, uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                      const mi_lte_ulsch_uci *h_uci /*[n_alloc]*/, mi_lte_pusch_plan **out);
/* after a run of such a plan (MI_LTE_ERR_INVALID_ARG on any other): the n_alloc result records; an allocation's Q_cqi CQI soft bits
 * (36.212 5.2.2.6.4's decoder input) and its G data soft bits (5.2.2.5's), device pointers into the plan */
int mi_lte_pusch_plan_uci_results(const mi_lte_pusch_plan *plan, const mi_lte_ulsch_uci_result **d_records);
int mi_lte_pusch_plan_cqi_soft(const mi_lte_pusch_plan *plan, uint32_t alloc, const int8_t **d_cqi, uint32_t *Q_cqi);
int mi_lte_pusch_plan_data_soft(const mi_lte_pusch_plan *plan, uint32_t alloc, const int8_t **d_data, uint32_t *G);

/* ---------------------------------------------------------------- CQI channel coding on PUSCH (36.212 5.2.2.6.4)
 * O <= 11 information bits: the (32, O) block code of table 5.2.2.6.4-1, b_i = sum_n o_n M_i,n mod 2, repeated: q_i = b_(i mod 32).
 * O > 11 (up to MI_LTE_CQI_MAX_BITS): CRC8 (gCRC8 = D^8 + D^7 + D^4 + D^3 + D + 1, register 0) appended, L = O + 8 bits through the
 * tail-biting convolutional code (5.1.3.1) and its rate matching (5.1.4.2) to Q_cqi bits.  A positive soft bit means bit 0.
 * mi_lte_cqi_encode (host arithmetic, one bit per byte): MI_LTE_ERR_INVALID_ARG for O = 0, O > MI_LTE_CQI_MAX_BITS, Q_cqi = 0,
 * Q_cqi > 6 * 12 * 1320 (the soft bits of the largest allocation) and null pointers.
 * The decoder, k_ulsch_cqi_decode, one wavefront per run, integers throughout (every result is exact):
 *   1. repeats add up in int32: r_i = sum of e_k over k = i mod 32 (block code); rate matching undone into d[3 L], received bit k where
 *      transmitted bit k came from, positions never sent 0 (convolutional code).  A 0 soft bit (an ACK-overwritten cell) adds nothing.
 *   2a. block code: the maximum of sum_i (1 - 2 b_i(o)) r_i over all 2^O words, ties to the smallest w = sum_n o_n 2^n.
 *   2b. convolutional code: maximum-correlation Viterbi, states (c_k-1 .. c_k-6) (newest bit the most significant), all 64 metrics 0 at
 *       the start, 3 L steps, step t on d[3 (t mod L) ..]; state n's survivor is the larger of its predecessors 2 (n & 31) and
 *       2 (n & 31) + 1 by metric + sum_x (1 - 2 label_x) d_x, the even one on a tie; end state: the first maximum in state order;
 *       traceback over all 3 L steps, the bits of steps L .. 2 L - 1 are c_0 .. c_(L-1); CRC8 is checked over them.
 * A DTX decision is the caller's: metric against energy. */
#define MI_LTE_CQI_MAX_BITS 128
enum { MI_LTE_CQI_NONE = 0, MI_LTE_CQI_NO_CRC = 1 /* block code */, MI_LTE_CQI_CRC_OK = 2, MI_LTE_CQI_CRC_FAIL = 3 };
typedef struct {
    uint32_t O;        /* 0: nothing decoded for this run */
    uint32_t crc;      /* MI_LTE_CQI_* */
    int32_t  metric;   /* correlation of the decided code word (convolutional: the decided L bits re-encoded) with r / d */
    int32_t  energy;   /* sum |r_i| or sum |d_k|: what a caller normalises a DTX threshold by */
    uint32_t bits[4];  /* information bit n at bit (n & 31) of word n >> 5; unused bits 0 */
} mi_lte_cqi_result;
typedef struct { uint32_t off /* bytes from d_soft, even */, Q_cqi, O, pad; } mi_lte_cqi_desc;
int mi_lte_cqi_encode(uint32_t O, const uint8_t *o_bits, uint32_t Q_cqi, uint8_t *q_bits /*[Q_cqi]*/);
/* n runs of int8 soft bits, everything device-resident, one launch on the context's stream (no wait).  d_soft is 2-byte aligned and run i
 * spans d_soft + off .. + Q_cqi.  The kernel checks the descriptors itself: O = 0, O > MI_LTE_CQI_MAX_BITS, Q_cqi = 0,
 * Q_cqi > 6 * 12 * 1320 or an odd off yield the all-zero record and read nothing. */
int mi_lte_cqi_decode_batch(mi_lte_ctx *ctx, const int8_t *d_soft, const mi_lte_cqi_desc *d_desc, uint32_t n, mi_lte_cqi_result *d_out);
/* A plan of mi_lte_pusch_plan_create_3gpp_uci decodes the CQI of allocation a as h_O_cqi[a] information bits (0: left opaque) from its next
 * run on: k_ulsch_cqi_decode once, behind k_ulsch_uci_decide, over the runs mi_lte_pusch_plan_cqi_soft hands out.  h_O_cqi = NULL turns
 * decoding off again.  MI_LTE_ERR_INVALID_ARG, the plan left as it was: any other plan, O > MI_LTE_CQI_MAX_BITS, O > 0 where Q_cqi = 0. */
int mi_lte_pusch_plan_set_cqi_decode(mi_lte_pusch_plan *plan, const uint32_t *h_O_cqi /*[n_alloc]*/);
/* the n_alloc records (device pointer into the plan): all zero before a first run with decoding on and for allocations left opaque */
int mi_lte_pusch_plan_cqi_results(const mi_lte_pusch_plan *plan, const mi_lte_cqi_result **d_records);

/* ---------------------------------------------------------------- PUSCH, 3GPP mode: max-log soft-decision demapping (opt-in per plan)
 * By default a 3GPP plan de-maps with the reference's modulation_demapper (MI_LTE_DEMAP_REF): +-127 for every 16QAM / 64QAM bit, for QPSK a
 * distance grade that ignores what the equaliser did to the noise.  MI_LTE_DEMAP_MAXLOG (the constants of the PDSCH section above) replaces it
 * by log-likelihood ratios; everything after the soft-bit buffer -- control-information gather and decisions, the CQI decoder, rate
 * un-matching, the code blocks and their erasure rule -- is unchanged and sums and saturates the graded bytes.
 *
 * Equalised symbol.  For allocation a (M = 12 N_prb sub-carriers) and data symbol s = 0 .. 11 (the twelve non-DMRS symbols in order): h_k(s)
 *   the channel estimate of sub-carrier k as the demodulator interpolates it in polar form between the two DMRS estimates (float, see
 *   uplink.hip), hn_k(s) = 1 / (Re h^2 + Im h^2) the float the one-tap zero-forcing equaliser multiplies with, and x_s[k] the transform
 *   pre-decoder's output times (float)(1 / sqrt(M)) (36.211 5.3.3): the float pair the default de-mapper receives.
 * Per-symbol reliability.  rho_s = (float)(M / sum_k (double)hn_k(s)), the harmonic mean of the channel power over the allocation: zero
 *   forcing colours the noise and the 1 / sqrt(M) inverse DFT spreads it evenly, so every time-domain sample of symbol s carries noise of
 *   variance sigma^2 / rho_s.  rho_s = 0 when the sum, the quotient or its float value is not finite (an infinite or NaN hn makes the sum so;
 *   a zero sum the quotient).  The sum is formed in double in a fixed order, without atomics: two runs give identical bytes.
 * LLR.  Bit 2j of symbol x = x_s[k] sits on the real axis, bit 2j + 1 on the imaginary one: L is the PDSCH section's max-log LLR of that axis
 *   with w = rho_s and z = rho_s x, i.e. rho_s (min_{S1} (u - s)^2 - min_{S0} (u - s)^2) for u = Re x or Im x, evaluated in double in the same
 *   piecewise-linear closed form from t = (double)rho_s * (double)u and w = (double)rho_s.  Positive: bit 0.
 * Soft bit.  v = clamp(rint(g_a L), -127, 127), ties to even, 0 where g_a L is not finite; then descrambled and written to the same byte
 *   (k 12 + s) Q_m + q of the allocation, with the same e_len, as the default de-mapper (mi_lte_pusch_plan_soft_bits).  QPSK, 16QAM, 64QAM.
 * Gain.  gain > 0: g_a = gain for every allocation.  gain == 0, automatic, per allocation and per run: g_a = (float)(T / (4 A^2 rhobar)),
 *   rhobar the mean in double of the twelve rho_s floats (summed s = 0 .. 11) and T = MI_LTE_DEMAP_AUTO_T.  A rhobar that is 0 or not finite,
 *   or a g_a past the float range, gives g_a = 0 and an all-zero allocation, which decodes to status 2 by the erasure rule of the mode's verdict.
 * Refusals (nothing is launched, the plan stays as it was): MI_LTE_ERR_INVALID_ARG for a NULL plan, an unknown mode, a negative or non-finite
 *   gain; MI_LTE_ERR_UNSUPPORTED for MAXLOG on a plan of mi_lte_pusch_plan_create (reference mode).  MI_LTE_DEMAP_REF is accepted on every
 *   plan, ignores gain and restores the default.  Plans with control information (mi_lte_pusch_plan_create_3gpp_uci, with or without
 *   mi_lte_pusch_plan_set_cqi_decode) accept MAXLOG.  A MAXLOG run launches k_pusch_demod_llr in place of k_pusch_demod. */
int mi_lte_pusch_plan_set_demapper(mi_lte_pusch_plan *plan, uint32_t mode, float gain);
/* taps, device pointers owned by the plan, holding the last MAXLOG run's values (zeros before one): the gain g_a, float [n_alloc], and
 * rho_s, float [n_alloc][12].  MI_LTE_ERR_INVALID_ARG on a reference-mode plan. */
int mi_lte_pusch_plan_llr_gain(const mi_lte_pusch_plan *plan, const float **d_gain);
int mi_lte_pusch_plan_llr_rho(const mi_lte_pusch_plan *plan, const float **d_rho);
/* the symbol tap, opt-in (on != 0 allocates it, on = 0 frees it; without it nothing extra is stored or allocated): MAXLOG runs also store
 * the x_s[k] of every allocation.  _llr_symbols: allocation alloc's n = 12 M float pairs (re, im) in [s][k] order; zeros before a MAXLOG
 * run.  MI_LTE_ERR_INVALID_ARG on a reference-mode plan and, for _llr_symbols, while the tap is off. */
int mi_lte_pusch_plan_set_llr_tap(mi_lte_pusch_plan *plan, uint32_t on);
int mi_lte_pusch_plan_llr_symbols(const mi_lte_pusch_plan *plan, uint32_t alloc, const float **d_x, uint32_t *n);

/* ---------------------------------------------------------------- PUSCH, 3GPP mode: DMRS noise estimate and the noise-referenced gain
 * The automatic gain above normalises every transmission to T at its own mean channel power: a convention, not 1 / sigma^2.  For HARQ
 * combining (next section) the LLRs of different transmissions have to be on one scale, so a MAXLOG run can take its gain from a noise
 * estimate instead: g_a = scale / sigma2_a, and v is then `scale` times the max-log LLR in natural units (zero forcing plus the 1 / sqrt(M)
 * inverse DFT leave noise sigma^2 / rho_s per sample, and L = rho_s (min_{S1} - min_{S0})).
 * Inputs.  For allocation a with M = 12 N_prb and slot b = 0, 1: t_b[i], the least-squares product rx conj(dmrs) of sub-carrier i as the
 *   demodulator keeps it after its first phase: the complex float (mag_b[i] u_b[i].re, mag_b[i] u_b[i].im) of the magnitude
 *   mag = sqrtf(re^2 + im^2) and the unit vector u = t / mag it stores ((1, 0) for mag = 0, so mag = 0 gives 0).
 * Second difference.  For every PRB j = 0 .. N_prb - 1 of the allocation's list and i = 12 j + 1 .. 12 j + 10:
 *   d_b[i] = t_b[i - 1] - 2 t_b[i] + t_b[i + 1], in double.  It never crosses a PRB boundary, so a non-contiguous or hopping PRB list needs
 *   no special case, and it removes any channel that is linear in frequency over three sub-carriers: a timing offset of 4 samples (of 2048)
 *   leaves 2e-8 |h|^2.
 * Sum and estimate.  S = sum_b sum_i |d_b[i]|^2 in double, in the fixed order of the rho pass (each thread its own i, i + THREADS, ..; the
 *   xor butterfly within the wavefront; the wavefronts' slots in ascending order; no atomics: two runs give identical bytes).
 *   sigma2_a = (float)(S / (120 N_prb)): white noise of variance sigma^2 per sub-carrier gives E|d|^2 = 6 sigma^2, over 20 N_prb terms.
 * Gain.  g_a = (float)((double)scale / (double)sigma2_a).  A sigma2_a that is 0 or not finite, or a g_a past the float range, gives g_a = 0:
 *   an all-zero allocation and status 2 by the erasure rule.  Everything else of the LLR is as above: v = clamp(rint(g_a L), -127, 127).
 *   mi_lte_pusch_plan_llr_gain reports the g_a used.
 * Limits.  The estimate's relative standard deviation is about 1.36 / sqrt(20 N_prb): 29 % at 1 PRB, 6 % at 25 PRB.  Channel curvature over
 *   three sub-carriers biases it upwards.  The error of the unsmoothed channel estimate itself is not in sigma2.
 * Scale.  scale = 8 is the convention the tests and tools use: an LLR of 16 meets the int8 clamp.  It is not a measured optimum: over
 *   profiles/pusch_harq_sweep.txt's classes of two combined transmissions 4, 8 and 16 decode the same number of blocks to within the
 *   sweep's noise -- the decoder is not sensitive to it.
 * Kernel.  A run with the noise gain on launches a further instantiation of k_pusch_demod_llr (listed under that name) that holds the
 *   noise pass, its two arguments and its LDS slots; with it off the launch, and so every byte, is what it was.
 * mi_lte_pusch_plan_set_llr_noise: scale > 0: MAXLOG runs of the plan use g_a = (float)(scale / sigma2_a) in place of the gain given to
 *   mi_lte_pusch_plan_set_demapper; scale == 0: off (the default).  Accepted whatever the plan's current demapper; takes effect on MAXLOG
 *   runs only, and with it off a MAXLOG run gives the bytes it gave before.  Refusals, the plan left as it was: MI_LTE_ERR_INVALID_ARG for a
 *   NULL plan and a negative or non-finite scale; MI_LTE_ERR_UNSUPPORTED on a reference-mode plan. */
int mi_lte_pusch_plan_set_llr_noise(mi_lte_pusch_plan *plan, float scale);
/* tap: float [n_alloc], sigma2_a of the last MAXLOG run with the noise gain on (zeros before one); device pointer owned by the plan.
 * MI_LTE_ERR_INVALID_ARG on a reference-mode plan. */
int mi_lte_pusch_plan_llr_noise(const mi_lte_pusch_plan *plan, const float **d_sigma2);

/* ---------------------------------------------------------------- PUSCH, 3GPP mode: receive-antenna combining
 * A MAXLOG run of a 3GPP plan can combine n_rx = 2 or 4 receive antennas by maximum-ratio combining in front of the transform pre-decoder:
 * one channel estimate per antenna, one combined symbol per sub-carrier, then the single-antenna chain.  The reference has no counterpart
 * (liblte_phy_pusch_channel_decode estimates and equalises one antenna); this text is the contract and tests/pusch_demod_model.py restates
 * it in float64.
 * Layout of d_subframes on a run of a plan with n_rx > 1 (antenna-major).  The grid of receive antenna r = 0 .. n_rx - 1 of unit u is
 *   subframe index r * ant_stride + u, each grid in the mi_lte_ul_subframe_floats() layout; ant_stride >= the plan's n_units.  One
 *   mi_lte_ul_frontend_batch call over n_rx * ant_stride units, antenna r's captures at units r * ant_stride + u, produces it.  Units
 *   n_units .. ant_stride - 1 of every antenna are not read.
 * Per-antenna estimate.  For each antenna r the DMRS least-squares products t_{r,b}[i] and the polar interpolation h_r(s)[i] are formed as
 *   the sections above describe them for the one antenna: the same float operations, the same zero-magnitude guards (mag = 0 gives the
 *   unit vector (1, 0) and so h = 0) and the same +-pi wrap of the slot-to-slot phase step.
 * Combining, in float with r ascending.  P_s[i] = sum_r (Re h_r(s)[i]^2 + Im h_r(s)[i]^2);
 *   z_s[i] = (sum_r y_r(s)[i] conj(h_r(s)[i])) * (1 / P_s[i]), real and imaginary part each a sum over r of the two-product terms the
 *   single-antenna equaliser forms.  The equaliser's hn becomes 1 / P_s[i]; x_s[k] is the pre-decoder's output for z times (float)(1 / sqrt(M)).
 * Reliability.  rho_s = (float)(M / sum_i (double)(1 / P_s[i])): the double sum, the fixed order and the not-finite -> 0 rule of the max-log
 *   section.  With equal noise sigma^2 per antenna the combined symbol carries noise sigma^2 / rho_s: that section's statement with P in
 *   place of |h|^2.
 * Noise.  S_r, the second-difference sum of the noise section on antenna r's t_{r,b}; sigma2_a = (float)((sum_r S_r) / (120 N_prb n_rx)),
 *   summed in double, antenna by antenna inside the section's fixed order.  The antennas' mean: equal noise power per antenna is the
 *   assumption maximum-ratio combining itself makes.
 * Gains.  Automatic: g_a = (float)(T / (4 A^2 rhobar)) on the combined rho_s.  Noise-referenced: g_a = (float)(scale / sigma2_a).
 * Downstream.  The LLR with t = rho_s x and w = rho_s, the soft byte, descrambling and de-interleaving are byte for byte those of the
 *   max-log section; control information, the CQI decoder, the code blocks and HARQ combining take the bytes as they take any other.
 *   mi_lte_pusch_plan_llr_gain, _llr_rho, _llr_noise and _llr_symbols report the combined quantities.
 * Consequences.  An all-zero grid on one antenna gives h_r = 0 through the guards: the antenna drops out of z and rho_s, and it contributes
 *   S_r = 0, so sigma2_a is the live antennas' sum over n_rx (half the live antenna's estimate at n_rx = 2).  All antennas zero: rho_s = 0
 *   and every soft bit 0, as with one antenna.  The same grid on every antenna gives the single-antenna z, n_rx times its rho_s and its sigma2_a.
 * Kernel.  k_pusch_demod_llr_rx, listed under that name in place of k_pusch_demod_llr: one workgroup per allocation, one launch per run, no
 *   atomics (two runs give identical bytes), 192 threads for M_max <= 96 and 256 above.  Its dynamic LDS in bytes, with M_max = 12 times
 *   the plan's largest N_prb and W = max over the allocations of ceil(12 M Q_m / 32) + 2 scrambling words:
 *     LDS(n_rx, S_par) = roundup8(36 n_rx M_max + 8 M_max (1 + 2 S_par) + 4 W) + 464.
 *   S_par, the data symbols transformed side by side, starts at the single-antenna value (the largest of 12, 6, 3, 2, 1 with
 *   16 S_par M_max <= 40960) and steps further down that list until LDS(n_rx, S_par) is within the device's per-workgroup limit, which is
 *   queried, not assumed.  On a 100-RB cell with 160 KiB per workgroup: n_rx = 2 admits every size a plan accepts, up to 99 PRB (144,224
 *   bytes with 64QAM) at the single-antenna S_par throughout; n_rx = 4 admits up to 76 PRB with a 64QAM allocation of that size (S_par 3 up
 *   to 65 PRB, 2 up to 70, 1 up to 76) and up to 78 PRB when the widest allocation is QPSK (S_par 3 up to 66 PRB, 2 up to 72, 1 up to 78).
 * mi_lte_pusch_plan_set_rx_antennas: n_rx = 1 (the default) restores the single-antenna behaviour and ignores ant_stride: such a plan, like
 *   one that never saw the setter, launches what it launched before with the same arguments and LDS.  Refusals, the plan left as it was:
 *   MI_LTE_ERR_INVALID_ARG for a NULL plan, an n_rx other than 1, 2 or 4, and n_rx > 1 with ant_stride < n_units;
 *   MI_LTE_ERR_UNSUPPORTED on a reference-mode plan (any n_rx) and when LDS(n_rx, 1) exceeds the device's limit.
 *   Accepted whatever the plan's current demapper, but a run with n_rx > 1 while the demapper is MI_LTE_DEMAP_REF launches nothing, returns
 *   MI_LTE_ERR_UNSUPPORTED and sets the context's error text (the hard-decision demapper has no combiner); the plan runs again once either
 *   setting is changed.
 * mi_lte_pusch_plan_rx_antennas: the plan's current n_rx and ant_stride (1 and 0 by default). */
int mi_lte_pusch_plan_set_rx_antennas(mi_lte_pusch_plan *plan, uint32_t n_rx, uint32_t ant_stride);
int mi_lte_pusch_plan_rx_antennas(const mi_lte_pusch_plan *plan, uint32_t *n_rx, uint32_t *ant_stride);

/* ---------------------------------------------------------------- PUSCH, 3GPP mode: MMSE equalisation
 * The sections above equalise with one zero-forcing tap per sub-carrier.  After it and the 1 / sqrt(M) inverse DFT every sample of symbol s
 * carries noise sigma^2 / rho_s, rho_s the harmonic mean of the channel power: on a channel that is flat over the allocation that is the
 * best there is, on one with delay spread a single faded sub-carrier sets the noise of all M samples.  A MAXLOG run with the noise gain on
 * can equalise with the MMSE tap instead, which weighs every sub-carrier by its own signal-to-noise ratio.  The reference has no
 * counterpart; this text is the contract and tests/pusch_demod_model.py restates it in float64.
 * Inputs (n_rx = 1, 2 or 4).  h_r(s)[i], y_r(s)[i] and P_s[i] = sum_r (Re h_r(s)[i]^2 + Im h_r(s)[i]^2) exactly as the combining section forms
 *   them (n_rx = 1: P = Re h^2 + Im h^2, the float whose reciprocal is the zero-forcing hn); s2 = sigma2_a, the float of the noise section
 *   including its mean over the antennas.  The units agree: the DMRS has unit modulus, so the least-squares products, and with them h,
 *   carry the grid's noise variance.
 * Equaliser, in float.  q_s[i] = 1.0f / (P_s[i] + s2); z_s[i] = (sum_r y_r(s)[i] conj(h_r(s)[i])) * q_s[i]: the numerator's sums are those of
 *   the combining section, for n_rx = 1 the two two-product terms of the single-antenna equaliser.  x_s[k] is the pre-decoder's output for z
 *   times (float)(1 / sqrt(M)).  It is biased -- E x = mu_s d for a sent symbol d -- and it is what mi_lte_pusch_plan_llr_symbols reports.
 * Residual.  nu_s = (float)((sum_i (double)q_s[i]) * (double)s2 / M): the sum in double, in the rho pass's fixed order (each thread its own
 *   i, i + THREADS, ..; the xor butterfly within the wavefront; the wavefronts' slots in ascending order; no atomics: two runs give
 *   identical bytes).  nu_s is the mean-square error of x_s[k] for unit-energy symbols; the useful amplitude is mu_s = 1 - nu_s, and the
 *   residual interference plus noise around mu_s d has variance nu_s (1 - nu_s).
 * LLR.  With u = Re x or Im x: the max-log section's llr_axis with w = (1 - (double)nu_s) / (double)nu_s and t = (double)u / (double)nu_s,
 *   i.e. w times the unbiased symbol u / (1 - nu_s): the natural-unit max-log LLR at the post-equaliser SINR w.  A nu_s that is not finite
 *   or lies outside the open interval (0, 1) gives w = 0 and t = 0: the symbol's soft bits are 0.
 * Gain.  An MMSE run needs the noise estimate: it runs only while the demapper is MAXLOG and mi_lte_pusch_plan_set_llr_noise has
 *   scale > 0.  g_a = (float)scale -- the 1 / sigma^2 is already inside w -- and mi_lte_pusch_plan_llr_gain reports it;
 *   v = clamp(rint(g_a L), -127, 127) as in the max-log section.  v is therefore `scale` times the natural LLR, the scale of a zero-forcing
 *   noise-referenced run: HARQ transmissions equalised either way combine.  s2 = 0 or not finite: g_a = 0 and an all-zero allocation, by
 *   the noise section's rule.
 * Taps.  mi_lte_pusch_plan_llr_nu holds nu_s.  mi_lte_pusch_plan_llr_rho holds, on an MMSE run, (float)((double)s2 * w_s): the reliability
 *   on zero forcing's scale (SINR = rho / sigma2), never below zero forcing's rho_s (the harmonic mean of P + s2 less s2 is at least that
 *   of P).  mi_lte_pusch_plan_llr_noise and _llr_symbols as before.
 * Consequences.  P the same on every sub-carrier: nu_s = s2 / (P + s2), w = P / s2 and t = x_zf P / s2 -- the zero-forcing noise-referenced
 *   run's g (rho x, rho) in exact arithmetic.  s2 -> 0: z tends to the zero-forcing z and w s2 to rho_s.  An all-zero grid has s2 = 0 with
 *   it: q is infinite, nu_s is not a number, w = 0 and every byte 0 (with P = 0 and s2 > 0: q = 1 / s2, nu_s = 1, w = 0).  A dead antenna
 *   drops out of numerator and P as in the combining section.
 * Kernel.  k_pusch_demod_llr_mmse, listed under that name: the launch of the noise-on run with the same n_rx -- k_pusch_demod_llr's
 *   threads, S_par and dynamic LDS for n_rx = 1, k_pusch_demod_llr_rx's, with its S_par stepping and its fit, for n_rx = 2 and 4 -- and one
 *   more barrier in front of the reliability pass, which needs s2.  A plan that never saw the setter, or is back at MI_LTE_EQ_ZF, launches
 *   what it launched before with the arguments and LDS it had.
 * Downstream.  Control information, the CQI decoder, the HARQ pool, the code blocks and the outputs take the bytes as they take any others.
 * mi_lte_pusch_plan_set_equaliser: MI_LTE_EQ_ZF (the default) or MI_LTE_EQ_MMSE.  Refusals, the plan left as it was:
 *   MI_LTE_ERR_INVALID_ARG for a NULL plan or an unknown mode; MI_LTE_ERR_UNSUPPORTED on a reference-mode plan, for any mode.  Accepted
 *   whatever the plan's current demapper and noise setting, but a run or HARQ run with MMSE set while the demapper is MI_LTE_DEMAP_REF or the
 *   noise scale is 0 launches nothing, returns MI_LTE_ERR_UNSUPPORTED and sets the context's error text; the plan runs again once either
 *   setting is changed.  (No LDS condition of its own: mi_lte_pusch_plan_set_rx_antennas has refused what does not fit.)
 * mi_lte_pusch_plan_equaliser: the plan's current mode.
 * mi_lte_pusch_plan_llr_nu: tap, float [n_alloc][12], nu_s of the last MMSE run; device pointer owned by the plan, allocated when MMSE is
 *   first set and zero until an MMSE run.  MI_LTE_ERR_INVALID_ARG on a reference-mode plan and while the plan never had MMSE set. */
#define MI_LTE_EQ_ZF 0u
#define MI_LTE_EQ_MMSE 1u
int mi_lte_pusch_plan_set_equaliser(mi_lte_pusch_plan *plan, uint32_t mode);
int mi_lte_pusch_plan_equaliser(const mi_lte_pusch_plan *plan, uint32_t *mode);
int mi_lte_pusch_plan_llr_nu(const mi_lte_pusch_plan *plan, const float **d_nu);

/* ---------------------------------------------------------------- PUSCH, 3GPP mode: HARQ soft combining
 * mi_lte_pusch_decode_run on a 3GPP plan with the allocations' soft bits combined into the pool's buffers.  The pool is the type of
 * "PDSCH, 3GPP mode: HARQ soft combining" above, and one pool of a context serves its PDSCH and PUSCH plans alike; the contract is that
 * section's: the binding with MI_LTE_HARQ_NONE and MI_LTE_HARQ_NEW_DATA, the flush rule, buf[t] = sat16(buf[t] + sat16(v)), the decoder
 * input clamp(buf[t], -127, 127), the state record and the ordering.
 * Uplink specifics.  N_cb = K_w (36.212 5.2.2.5), so the flush rule's N_cb test only fires against a buffer last written by a PDSCH plan
 *   with a limited soft buffer.  Plans with control information combine the gathered data run (mi_lte_pusch_plan_data_soft): G differs
 *   between transmissions with and without control information, which the rule allows.  ACK / RI decisions and the CQI decoder are
 *   untouched by the pool.  Transmissions of different modulation or SNR combine on one scale only under the noise-referenced gain above.
 * Refusals, returned before anything is launched, leaving pool and plan usable: MI_LTE_ERR_UNSUPPORTED for a plan of
 *   mi_lte_pusch_plan_create; MI_LTE_ERR_INVALID_ARG for a NULL binding, buf >= n_buf, one buf bound twice in a run, or an allocation
 *   whose tbs exceeds the pool's max_tbs.
 * last_kernels: the plain run's demodulator prefix, then k_dl3_desc:1,k_harq_bind:1,k_harq_rm:1, .. ,k_harq_commit:1. */
int mi_lte_pusch_decode_run_harq(mi_lte_ctx *ctx, mi_lte_pusch_plan *plan, mi_lte_harq_pool *pool, const mi_lte_harq_bind *h_bind,
                                 const float *d_subframes, uint8_t *d_out_bits, int32_t *d_status);

/* PRACH detection: replaces liblte_phy_detect_prach() (liblte_phy.h:862-868, implementation liblte_phy.cc:3299-3479)
 * for a batch of PRACH occasions (d_occ_start[o] = sample index of the occasion's first cyclic-prefix sample; an
 * occasion spans mi_lte_prach_occasion_samples() samples), preamble formats 0-4 (format 4, the TDD UpPTS preamble of
 * liblte_phy.cc:2462-2468: N_zc = 139 on 7.5 kHz sub-carriers, T_fft = 4 096, root table 5.7.2-5, N_cs table 5.7.2-3 -- the same
 * kernels with the sequence length as an argument).  The 839 (139) PRACH sub-carriers are
 * computed directly from the T_fft samples behind the prefix, correlated with every root sequence the cell's 64
 * preambles use, and the reference's verdict -- one preamble if the peak reaches 50 x the averaged correlation
 * power (:3460-3474) -- is evaluated on the host: h_N_det_pre[o] in {0,1}, h_det_pre[o] = preamble index,
 * h_det_ta[o] = timing advance, exactly the reference's three outputs.  The plan generates the root sequences'
 * spectra itself (prach_preamble_seq_gen :7130-7290 + the 839-point DFTs of liblte_phy_ul_init :2496-2508);
 * mi_lte_prach_plan_create_roots takes them from the caller instead (LIBLTE_PHY_STRUCT::prach_x_u_fft_re/im).
 * A 64-preamble set that starts near the end of the logical root table continues at index 0 (36.211 5.7.2: the order is cyclic);
 * the reference indexes past its table there (liblte_phy.cc:7168-7171), so only the caller's-roots form reproduces it in that case. */
typedef struct {
    uint32_t root_seq_idx;     /* logical root sequence index, 0..837 (format 4: 0..137) */
    uint32_t preamble_format;  /* 0..4 */
    uint32_t zczc;             /* zeroCorrelationZoneConfig */
    uint32_t hs_flag;          /* restricted set */
    uint32_t freq_offset;      /* n_PRBoffset^RA */
} mi_lte_prach_cfg;
typedef struct mi_lte_prach_plan mi_lte_prach_plan;
int      mi_lte_prach_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg /* N_rb_dl = N_rb_ul */, const mi_lte_prach_cfg *prach,
                                  mi_lte_prach_plan **out);
int      mi_lte_prach_plan_create_roots(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const mi_lte_prach_cfg *prach,
                                        const float *h_x_u_fft_re /*[n_roots][839], the first N_zc of a row used*/, const float *h_x_u_fft_im,
                                        uint32_t n_roots, mi_lte_prach_plan **out);
void     mi_lte_prach_plan_destroy(mi_lte_ctx *ctx, mi_lte_prach_plan *plan);
uint32_t mi_lte_prach_plan_n_roots(const mi_lte_prach_plan *plan);
/* Host arithmetic only (no device): the physical root sequence numbers u of the configuration's 64 preambles in the order
 * prach_preamble_seq_gen enumerates them (liblte_phy.cc:7155-7290; cyclic logical order, see above).  MI_LTE_ERR_UNSUPPORTED where the
 * reference itself cannot process the configuration (a restricted-set root without a cyclic shift, zeroCorrelationZoneConfig past the table). */
int      mi_lte_prach_root_set(const mi_lte_prach_cfg *prach, uint32_t *h_u /* [64] */, uint32_t *n_roots);
uint32_t mi_lte_prach_occasion_samples(const mi_lte_prach_plan *plan);
int      mi_lte_prach_detect_run(mi_lte_ctx *ctx, mi_lte_prach_plan *plan, const void *d_samples_a, const void *d_samples_b,
                                 const uint64_t *d_occ_start, uint32_t n_occ, uint32_t *h_N_det_pre, uint32_t *h_det_pre,
                                 uint32_t *h_det_ta);
/* The same detection (liblte_phy_detect_prach, liblte/hdr/liblte_phy.h:727-733, liblte_phy.cc:3293-3480) in two halves for a caller that keeps
 * the stream busy -- a receiver that hands the device the next subframes while the random-access verdicts of these are on their way:
 * _launch queues the kernels and the copy of the per-root maxima (pinned memory of the plan's own) and returns at once; _fetch waits for
 * the stream and forms the verdicts of the launch before it (max_occ = room in the three arrays).  One launch in flight per plan. */
int      mi_lte_prach_detect_launch(mi_lte_ctx *ctx, mi_lte_prach_plan *plan, const void *d_samples_a, const void *d_samples_b,
                                    const uint64_t *d_occ_start, uint32_t n_occ);
int      mi_lte_prach_detect_fetch(mi_lte_ctx *ctx, mi_lte_prach_plan *plan, uint32_t *h_N_det_pre, uint32_t *h_det_pre,
                                   uint32_t *h_det_ta, uint32_t max_occ);
/* the detector's tap, for tests and not for callers: runs the same three kernels over the batch (the correlation kernel in an instantiation
 * that also stores every power; the detection entries above store none) and copies out what they computed, forming no verdict --
 * h_xhat: the kept bins, n_occ x N_zc float pairs (re, im); h_stats: the per-root records the verdict is formed from, [n_occ][n_roots];
 * h_power: the correlation power profiles, float [n_occ][n_roots][N_zc].  N_zc = 839 (format 4: 139).  Waits for the stream; the plan is
 * left as it was.  MI_LTE_ERR_INVALID_ARG as mi_lte_prach_detect_run, and for a NULL output. */
typedef struct { float sum, max_val; uint32_t max_off, pad; } mi_lte_prach_corr_stat;
int      mi_lte_prach_detect_tap(mi_lte_ctx *ctx, mi_lte_prach_plan *plan, const void *d_samples_a, const void *d_samples_b,
                                 const uint64_t *d_occ_start, uint32_t n_occ, float *h_xhat, mi_lte_prach_corr_stat *h_stats,
                                 float *h_power);

/* ---------------------------------------------------------------- PUCCH formats 1 / 1a / 1b
 * mi_lte_pucch_decode_run replaces liblte_phy_pucch_format_1_1a_1b_channel_decode() (liblte/hdr/liblte_phy.h:775-782,
 * implementation liblte/src/liblte_phy.cc:2961-3146 with get_ulcch_ce :13799-13868) for a batch of PUCCH resources over UL device
 * subframes (mi_lte_ul_frontend_batch) -- the fourth receive call of the eNodeB's radio thread (LTE_fdd_enb_phy.cc:867).
 * The sequences are the caller's, i.e. what liblte_phy_ul_init left in LIBLTE_PHY_STRUCT for (subframe N, resource n = N_1_p_pucch);
 * per resource h_tables holds MI_LTE_PUCCH_TAB_FLOATS floats:
 *     pucch_dmrs_0_re[N][n][36] pucch_dmrs_0_im[..][36] pucch_dmrs_1_re[..][36] pucch_dmrs_1_im[..][36]
 *     r_re[2][4][12] r_im[2][4][12]   = pucch_r_u_v_alpha_p_re/_im[N][n][m'][symbol 0, 1, 5, 6][12]
 *     sw_re[2][4]    sw_im[2][4]      = s_ns(m') * W_5_4_1_2[pucch_n_oc_p[N][n][m']][i]   (s_ns = 1 or (cos(pi/2), sin(pi/2)), :3058-3068)
 * Outputs per resource: h_bits[2r], h_bits[2r+1], h_n_bits (1 for formats 1 / 1a, 2 for 1b), h_rc = 0 (LIBLTE_SUCCESS) or 1
 * (LIBLTE_ERROR_INVALID_INPUTS: soft decision <= 0.5, the reference's failure value).  N_ant = 1 like the reference. */
#define MI_LTE_PUCCH_TAB_FLOATS 352
typedef struct {
    uint32_t unit;         /* index into the batch of UL device subframes */
    uint32_t format;       /* 0 = format 1, 1 = 1a, 2 = 1b (LIBLTE_PHY_PUCCH_FORMAT_ENUM) */
    uint32_t N_1_p_pucch;
} mi_lte_pucch_res;
/* The tables of one (subframe, resource) from the cell's configuration, for callers that have no LIBLTE_PHY_STRUCT: restates what
 * liblte_phy_ul_init computes through generate_dmrs_pucch (liblte_phy.cc:2401-2421, :6986-7129) and what the decoder derives from it
 * (:3058-3083).  delta_pucch_shift = deltaPUCCH-Shift (1..3 in 36.211; i.e. the value liblte_phy_ul_init is given + 1, :2414); host function. */
int mi_lte_ul_pucch_tables(const mi_lte_ul_cfg *ul, uint32_t N_id_cell, uint32_t N_subfr, uint32_t N_1_p_pucch, uint32_t N_cs_an,
                           uint32_t delta_pucch_shift, uint32_t N_ant, float *h_tables /* [MI_LTE_PUCCH_TAB_FLOATS] */);
int mi_lte_pucch_decode_run(mi_lte_ctx *ctx, uint32_t N_rb_ul, uint32_t N_ant, const float *d_subframes, const mi_lte_pucch_res *h_res,
                            const float *h_tables, uint32_t n_res, uint8_t *h_bits, uint32_t *h_n_bits, uint32_t *h_rc);

/* ---------------------------------------------------------------- PUCCH formats 2 / 2a / 2b (periodic CQI reports)
 * Stands for liblte_phy_pucch_format_2_2a_2b_channel_encode / _decode, which the reference declares (liblte/hdr/liblte_phy.h:785-816) and
 * leaves empty (liblte/src/liblte_phy.cc:3150-3173, both bodies a FIXME).  So the specification is the authority: 36.211 5.4.2, 5.4.3 and
 * 5.5.2.2, 36.212 5.2.3.3; normal cyclic prefix, one receive antenna, FDD.
 *
 * The (20, A) code, 1 <= A <= 13 (36.212 table 5.2.3.3-1): b_i = sum_n a_n M_i,n mod 2.  Its columns 0 .. 10 are the first 20 rows of
 * the (32, O) code's table 5.2.2.6.4-1.  mi_lte_pucch2_encode: one bit per byte; MI_LTE_ERR_INVALID_ARG for A = 0, A > 13, null pointers.
 *
 * mi_lte_ul_pucch2_table (host arithmetic) fills what one (cell, subframe, resource n2 = n_PUCCH^(2), RNTI) needs on both sides:
 *   r[7 s + l][k] = r_u,v^(alpha(n_s, l))(k) of slot n_s = 2 N_subfr + s, symbol l, sub-carrier k (the base sequences of
 *     mi_lte_ul_pucch_tables), alpha = 2 pi n_cs / 12, n_cs(n_s, l) = (n_cs^cell(n_s, l) + n'(n_s)) mod 12;
 *   n' (5.4.2, every modulo the mathematical one): even slot n' = n2 mod 12 if n2 < 12 N_rb_2, else (n2 + N_cs_1 + 1) mod 12;
 *     odd slot n' = [12 (n'(n_s - 1) + 1)] mod 13 - 1 if n2 < 12 N_rb_2, else (12 - 2 - n2) mod 12;
 *   prb[s] (5.4.3): m = floor(n2 / 12); floor(m / 2) when (m + s) mod 2 = 0, else N_rb_ul - 1 - floor(m / 2);
 *   c_scr: bit i = c(i), i < 20, of the Gold sequence with c_init = (N_subfr + 1) (2 N_id_cell + 1) 2^16 + rnti.
 * MI_LTE_ERR_INVALID_ARG: N_subfr > 9, N_id_cell > 503, N_cs_1 > 7, rnti > 65535, N_rb_ul outside 6 .. 100, N_rb_2 > 110, n2 outside [0, 12 N_rb_2) and
 * (only when N_cs_1 > 0) [12 N_rb_2, 12 N_rb_2 + 10 - N_cs_1), 2 floor(m / 2) >= N_rb_ul, null pointers.
 *
 * mi_lte_pucch2_modulate writes one UE's 2 x 7 x 12 elements into a grid pair re[14][1200], im[14][1200] (the UL subframe layout):
 * b scrambled with c_scr, QPSK d(n) = ((1 - 2 b(2n)) + j (1 - 2 b(2n+1))) / sqrt 2 (36.211 table 7.1.2-1), d(n) r on data symbol
 * l = {0, 2, 3, 4, 6}[n mod 5] of slot floor(n / 5), r on symbol 1 and z r on symbol 5 of each slot; z = 1 for format 0 (format 2),
 * format 1 (2a): ack 0 -> 1, 1 -> -1; format 2 (2b): ack 00 -> 1, 01 -> -j, 10 -> j, 11 -> -1 (table 5.4.2-1).  MI_LTE_ERR_INVALID_ARG:
 * format > 2, a table whose prb >= 100, null pointers (ack may be NULL for format 0).
 *
 * The decoder, k_pucch2_decode, one wavefront per resource.  y(L, k) is the unit's element on symbol L, sub-carrier k, in the UL subframe
 * layout of mi_lte_ul_frontend_batch:
 *   1. Correlations.  c[L] = sum_{k<12} y(L, 12 prb[s] + k) conj(r[L][k]), L = 7 s + l, all 14 symbols, float32.  Correlating over the
 *      12 sub-carriers is what separates UEs on other cyclic shifts of the same resource block; there are no per-sub-carrier estimates.
 *   2. HARQ-ACK.  D = sum_s c[7s+5] conj(c[7s+1]).  Format 2: z = 1, no ACK bits.  2a: ack = (Re D < 0), z = +-1.  2b: the first maximum
 *      of (Re D, -Im D, Im D, -Re D) over (b20, b21) = 00, 01, 10, 11, z as in the modulator.
 *   3. Channel estimates.  h_s = (c[7s+1] + conj(z) c[7s+5]) / 24.  P = (|h_0|^2 + |h_1|^2) / 2.
 *   4. Soft bits.  v_n = (c[L_n] / 12) conj(h_s), L_n the data symbol of d(n).  g = 32 sqrt 2 / P.  e(2n) = clamp(rintf(g Re v_n), +-127)
 *      and e(2n+1) likewise from Im, each negated where c_scr's bit is 1.  Positive = bit 0.  Both slots share one g, so the slots combine
 *      with their own weights.  P = 0 or not finite (or a g that is not finite): all 20 are 0.
 *   5. Decision.  metric(w) = sum_i (1 - 2 b_i(w)) e_i in int32 over all 2^A words, the first maximum (smallest w = sum a_n 2^n).
 *   6. Record.  One 64-byte mi_lte_pucch2_result.  The soft bits inside the record are the stage tap.  A DTX threshold (metric against
 *      energy, P) is the caller's.
 * mi_lte_pucch2_decode_run: resource r reads unit h_res[r].unit of d_subframes with table h_tabs[h_res[r].tab] -- resources with the same
 * (subframe number, n2, rnti) share a table -- and writes d_out[r] (device memory).  Descriptors and tables go up in one staging copy;
 * the call does not wait for the kernel.  Refused before any launch (MI_LTE_ERR_INVALID_ARG): format > 2, A = 0, A > 13, unit >= n_units,
 * tab >= n_tab, a table whose prb >= N_rb_ul, n_res = 0, n_tab = 0, N_rb_ul outside 6 .. 100, null pointers. */
typedef struct {
    float    r_re[14][12], r_im[14][12];
    uint32_t prb[2];
    uint32_t c_scr;
} mi_lte_pucch2_tab;
typedef struct { uint32_t unit, format /* 0 = format 2, 1 = 2a, 2 = 2b */, tab /* index into h_tabs */, A; } mi_lte_pucch2_res;
typedef struct {
    uint32_t A;
    uint32_t bits;        /* a_n at bit n */
    int32_t  metric;      /* of the decided word */
    int32_t  energy;      /* sum |e_i| */
    uint8_t  ack[2], n_ack /* 0, 1, 2 */, pad0;
    float    D_re, D_im, P;
    int8_t   e[20];
    uint8_t  pad[12];
} mi_lte_pucch2_result;   /* 64 bytes */
int mi_lte_ul_pucch2_table(const mi_lte_ul_cfg *ul, uint32_t N_id_cell, uint32_t N_subfr, uint32_t N_rb_ul, uint32_t n_2_pucch, uint32_t N_rb_2,
                           uint32_t N_cs_1, uint32_t rnti, mi_lte_pucch2_tab *out);
int mi_lte_pucch2_encode(uint32_t A, const uint8_t *a_bits, uint8_t *b /*[20]*/);
int mi_lte_pucch2_modulate(const mi_lte_pucch2_tab *tab, uint32_t format, const uint8_t *b /*[20]*/, const uint8_t *ack /*[2]*/, float *re, float *im);
int mi_lte_pucch2_decode_run(mi_lte_ctx *ctx, uint32_t N_rb_ul, const float *d_subframes, uint32_t n_units, const mi_lte_pucch2_res *h_res,
                             uint32_t n_res, const mi_lte_pucch2_tab *h_tabs, uint32_t n_tab, mi_lte_pucch2_result *d_out);

/* ---------------------------------------------------------------- PCFICH + PDCCH (common search space)
 * mi_lte_pdcch_plan_* / mi_lte_pdcch_decode_run replace liblte_phy_pdcch_channel_decode()
 * (liblte/hdr/liblte_phy.h:1012-1020, implementation liblte/src/liblte_phy.cc:4519-5135) for a batch of device
 * subframes -- the call that sits between liblte_phy_get_dl_subframe_and_ce and liblte_phy_pdsch_channel_decode in the
 * reference's receiver (LTE_fdd_dl_fs_samp_buf.cc:445-470).  Per subframe: the control-format indicator from the
 * PCFICH, N_symbs = cfi (+1 for N_rb_dl <= 10), and the DCIs found for SI-, P- and RA-RNTI in the reference's six
 * common-search-space candidates (four at aggregation level 4, two at level 8; formats 1A and 1C each), in the
 * reference's order and capped at LIBLTE_PHY_PDCCH_MAX_ALLOC = 6.  Each DCI comes raw (payload bits) and unpacked into
 * the allocation liblte_phy_pdsch_channel_decode needs (dci_1a_unpack :13273-13378, dci_1c_unpack :13400-13611);
 * a DCI that does not unpack is dropped like the reference does.  h_rc[u] is the reference's return value for the
 * subframe: 3 (LIBLTE_ERROR_INVALID_CRC, h_cfi[u] = 0) when the PCFICH did not decode, else what its last DCI unpacker
 * call returned (0 or 4), or 1 (LIBLTE_ERROR_INVALID_INPUTS, its initial value) when no DCI was found.
 * Candidates reaching past the subframe's last CCE are decoded with the missing CCEs as erasures -- the reference reads
 * stale scratch there, zeros on a fresh LIBLTE_PHY_STRUCT.
 *
 * The plan holds the resource-element index tables of the listed cells (a cell the plan was not built for decodes
 * as cfi = 0).  PHICH: only the positions are needed (its REGs are excluded from the PDCCH), normal duration only --
 * the reference does not handle the extended duration either (:8280-8283).
 *
 * Transmit diversity: the reference passes its per-port estimate array [4][288] to the combiner with a port stride of
 * 576 (:4881, :7935), so with two ports the second port's estimate is read as zero and with four ports the rows are
 * scrambled and nothing decodes.  By default the plan reproduces exactly that arithmetic (parity with the reference,
 * rows it never writes taken as the zeros of a fresh LIBLTE_PHY_STRUCT); MI_LTE_PDCCH_PER_PORT_ESTIMATES gives every
 * port its own estimate instead -- the decoder the reference meant, which does decode 4-port cells. */
#define MI_LTE_PDCCH_MAX_DCI 6
#define MI_LTE_PDCCH_PER_PORT_ESTIMATES 1u
typedef struct {
    uint32_t rnti;         /* 0xFFFF SI, 0xFFFE P, 0x0001..0x003C RA                               */
    uint32_t format;       /* 0 = DCI 1A, 1 = DCI 1C                                              */
    uint32_t candidate;    /* 0..3 aggregation level 4 (CCE 4*c), 4..5 aggregation level 8        */
    uint32_t n_bits;       /* DCI size for this bandwidth (:4835-4857)                            */
    uint32_t payload;      /* the DCI, first bit in bit n_bits-1                                  */
    uint32_t mcs;
    uint32_t alloc_valid;  /* the DCI unpacked into alloc                                         */
    uint32_t reserved;
    mi_lte_pdsch_alloc alloc; /* unit, mod_type, tbs, rv_idx, tx_mode, rnti, N_prb, prb[2][N_prb]   */
} mi_lte_pdcch_dci;
typedef struct mi_lte_pdcch_plan mi_lte_pdcch_plan;
int  mi_lte_pdcch_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, float phich_res /* N_g: 1/6, 1/2, 1, 2 */,
                              uint32_t phich_dur_extended, uint32_t flags, const uint32_t *h_cells, uint32_t n_cells,
                              mi_lte_pdcch_plan **out);
void mi_lte_pdcch_plan_destroy(mi_lte_ctx *ctx, mi_lte_pdcch_plan *plan);
int  mi_lte_pdcch_decode_run(mi_lte_ctx *ctx, mi_lte_pdcch_plan *plan, const float *d_subframes, const uint32_t *d_subfr_num,
                             const uint32_t *d_n_id_cell, uint32_t n_units, uint32_t *h_rc, uint32_t *h_cfi, uint32_t *h_n_symbs,
                             uint32_t *h_n_dci, mi_lte_pdcch_dci *h_dci /* [n_units][MI_LTE_PDCCH_MAX_DCI] */);
/* the plan's index tables on their own (host arithmetic): grid index l*1200 + k of the 16 PCFICH resource elements and of
 * the six candidates' resource elements in decoding order (0xFFFFFFFF: CCE past the subframe's last one) */
int  mi_lte_pdcch_re_tables(uint32_t N_rb_dl, uint32_t N_ant, uint32_t N_id_cell, float phich_res, uint32_t N_symbs,
                            uint32_t *pcfich /* [16] */, uint32_t *cand /* [6][288] */);
/* what the reference leaves in LIBLTE_PHY_PCFICH_STRUCT::k, n and LIBLTE_PHY_PHICH_STRUCT::N_reg, k (:7903-7910, :8243-8278) */
int  mi_lte_ctrl_reg_positions(uint32_t N_rb_dl, uint32_t N_id_cell, float phich_res, uint32_t *pcfich_k /* [4] */,
                               float *pcfich_n /* [4] */, uint32_t *phich_N_reg, uint32_t *phich_k /* [75] */);
/* atan2f as the de-mappers evaluate it where the reference DECIDES on an angle (QPSK / BPSK quadrants, PUCCH 1b regions): the algorithm of
 * the reference host's libm (glibc 2.35) restated in float arithmetic, here on the host (tests pin it to libm bit for bit) */
int  mi_lte_model_atan2f(const float *h_y, const float *h_x, float *h_out, size_t n);
/* the two DCI unpackers on their own (host arithmetic; what the shim and tests compare with the reference's) */
int  mi_lte_dci_1a_unpack(uint32_t payload, uint32_t n_bits, uint32_t rnti, uint32_t N_rb_dl, uint32_t N_ant, mi_lte_pdcch_dci *out);
int  mi_lte_dci_1c_unpack(uint32_t payload, uint32_t n_bits, uint32_t rnti, uint32_t N_rb_dl, uint32_t N_ant, mi_lte_pdcch_dci *out);

/* ---------------------------------------------------------------- PDCCH, 3GPP mode: blind search over the whole control region (opt-in)
 * mi_lte_pdcch_search_* find every DCI of a set of RNTIs anywhere in the control region: the UE-specific search space of 36.213 9.1.1 at
 * aggregation levels 1, 2, 4, 8 next to the common one, any DCI size, with a tail-biting decoder.  The calls above keep the reference's
 * behaviour; this path shares their PCFICH decoder, their de-mapper and their tables and nothing of the reference's candidate handling.
 *
 * Search spaces (mi_lte_pdcch_search_space, host arithmetic).  Y_(-1) = rnti, Y_k = (39827 Y_(k-1)) mod 65537 for k = subfr_num = 0 .. 9;
 * candidate m = 0 .. M(L) - 1 of aggregation level L starts at CCE L ((Y_k + m) mod floor(N_cce / L)), M = 6, 6, 2, 2 for L = 1, 2, 4, 8.
 * floor(N_cce / L) = 0 gives *n = 0 (no modulus is taken).  Duplicates stay as the formula yields them.  MI_LTE_ERR_INVALID_ARG: rnti = 0
 * or > 0xFFFF, L not in {1, 2, 4, 8}, subfr_num > 9, null pointers.  The common search space is L = 4 at CCEs 0, 4, 8, 12 and L = 8 at
 * CCEs 0, 8, wherever those CCEs exist, for any RNTI.
 *
 * The plan holds, per listed cell and N_symbs = 1 .. 4, the resource elements of EVERY CCE in order and N_cce; per listed DCI size the
 * rate-matching map of 36.212 5.1.4.2 (576 entries: received bit k of a candidate of any L came from d[map[k]], k < 72 L -- the map of
 * level L is the first 72 L entries of the map of level 8); and the RNTI set as a 65 536-bit device bitmap.  The set is exactly what the
 * caller lists (SI-, P- and RA-RNTIs included only when listed); mi_lte_pdcch_search_plan_set_rntis replaces it, n_rnti = 0 empties it.
 * Refused like mi_lte_pdcch_plan_create (MI_LTE_ERR_UNSUPPORTED): a non-standard bandwidth, a port count other than 1 / 2 / 4, N_g outside
 * (0, 2], the extended PHICH duration.  MI_LTE_ERR_INVALID_ARG: n_sizes = 0 or > MI_LTE_PDCCH_SEARCH_MAX_SIZES, a size outside 8 .. 64, a
 * size listed twice, a cell past 503, an RNTI of 0 or above 0xFFFF, a flag other than the two below.  Every refusal comes before any launch.
 *
 * mi_lte_pdcch_search_run, everything queued on the context's stream, one wait (before the compacted results are read), no allocation
 * after the first run at a given n_units:
 *   1. k_pdcch_search_demod, one workgroup per subframe.  CFI from the PCFICH as k_pdcch_decode finds it; N_symbs = cfi + (N_rb_dl <= 10).
 *      Every CCE's 36 resource elements through the transmit-diversity combiner with each port's own estimate (the arithmetic of
 *      MI_LTE_PDCCH_PER_PORT_ESTIMATES), the QPSK de-mapper and the descrambler (c_init = (subfr_num << 9) + cell, CCE c at bit 72 c):
 *      int8 soft bits soft[unit][72 cce + k], positive = bit 0.  A cell the plan was not built for, a subframe number past 9, cfi = 0 or
 *      N_symbs > 4: h_cfi = 0, h_n_cce = 0, no hit, and nothing of the unit's soft bits is written; a run writes soft[unit][0 .. 72 h_n_cce)
 *      and nothing past it.
 *      The de-mapper's arithmetic (float32; the same for the PCFICH's 16 elements and for a CCE's 36; tests/pdcch_ctrl_model.py restates
 *      it in float64).  The elements are taken in groups of N_ant in the order of the table; y(e) is the received element, h_p(e) port
 *      p's estimate at it.
 *        1 port:  x(e) = conj(h_0(e)) y(e) / |h_0(e)|^2.
 *        2 ports: the pair (a, b) = (2 g, 2 g + 1) of the pre-coder of 36.211 6.3.4.3 with ports (A, B) = (0, 1).  Both estimates are
 *          read at the pair's FIRST element a, also for x(b):  P_A = |h_A(a)|^2, P_B = |h_B(a)|^2, hn = sqrt(P_A^2 + P_B^2),
 *            x(a) = (conj(h_A(a)) y(a) + h_B(a) conj(y(b))) / hn,   x(b) = (conj(h_A(a)) y(b) - h_B(a) conj(y(a))) / hn.
 *          (hn is the reference's normaliser, not P_A + P_B: without noise |x| = (P_A + P_B) / (sqrt 2 hn), 1 for equal ports and
 *          1 / sqrt 2 for one port in a fade.)
 *        4 ports: per group of four elements 4 g .. 4 g + 3 the same on two pairs: elements (0, 1) of the group with ports (0, 2) and the
 *          estimates at element 0; elements (2, 3) with ports (1, 3) and the estimates at element 2 (36.211 6.3.4.3; a group is one
 *          resource-element group, so the pairs alternate inside every quadruplet).
 *        QPSK soft value: (s_re, s_im) = the signs of x's components, its quadrant (a component that is exactly zero goes where atan2 puts
 *          the angle: [0, pi/2) is +, +; [pi/2, pi) is -, +; [-pi/2, 0) is +, -); dist = |x - (s_re + j s_im) / sqrt 2|,
 *          m = trunc(127 (1 - min(dist, 1 - 1/120))), so 1 <= m <= 127; the symbol's two bits are s_re m and s_im m.
 *        Descrambling: bit n of the region (n = 72 cce + k; the PCFICH: n = 0 .. 31 of its own sequence) is negated where c(n) = 1.
 *        An element marked absent in a table (0xFFFFFFFF; the search's tables have none) gives 0 on both bits.
 *        Zero estimates (hn = 0, or |h_0|^2 = 0) make x 0 / 0: not a number, whatever y is.  Both bits of every element of the pair (of the
 *          element, with 1 port) are then 0 -- the one way the de-mapper yields a 0; for the PCFICH a 0 counts as bit 0.  A finite x
 *          however large (a received sample of 1e30) saturates at m = 1 with its quadrant's signs.
 *      PCFICH decision: the 32 descrambled soft bits, bit = (soft < 0), against the four code words of 36.212 table 5.3.4-1 (CFI 4: all
 *      zero); the smallest Hamming distance wins, the lower CFI on a tie; 4 or more errors: cfi = 0.
 *      Positions: the plan's tables are those of mi_lte_pdcch_re_tables carried on to every CCE (mi_lte_pdcch_cce_tables gives them on the
 *      host): REGs as 36.211 6.2.4 counts them, the walk of 6.8.5 (k' outer, l' inner), the quadruplet interleaver of 36.212 5.1.4.2.1 and
 *      the cyclic shift by N_id_cell.  In two respects they are the reference's and not 36.211's, by default: (i) the PHICH groups the walk
 *      steps over are those of the PHICH section below -- numbered past the PCFICH's four REGs in the order 6.7.4 lists them, which is not
 *      ascending once they wrap round the band's edge, so that a PHICH REG can be a wrong one or a PCFICH REG; (ii) with four ports N_reg
 *      loses N_rb groups to symbol 1's CRS even where N_symbs = 1.  Either moves every CCE of the cells and sizes concerned (about a third
 *      of all (cell, N_g, N_symbs, ports)); this library's transmitter and PHICH decoder share (i).  MI_LTE_PDCCH_SEARCH_36211_REGS builds
 *      the plan's tables as 36.211 6.9.3 and 6.8.1 write both -- what a standard eNodeB sends.
 *   2. k_pdcch_search_decode, one wavefront per (unit, candidate, size).  Candidates: every L in {8, 4, 2, 1} and every first CCE with
 *      cce mod L = 0 and cce + L <= N_cce.  With N = n_bits + 16, a pair with N >= 72 L is skipped (no redundancy left).  Per pair:
 *      a. rate un-matching in int32: d[map[r]] = sum over j of soft[r + 3 N j] (r < 3 N, r + 3 N j < 72 L); positions never sent are 0.
 *      b. energy = sum |d|; energy = 0 is no hit whatever the CRC says.  (With estimates that are not zero step 1's de-mapper never yields a
 *         0: its smallest magnitude is 1, so a noiseless empty region reads +-1 in the scrambler's pattern and is turned away by the CRC and
 *         the RNTI set like any noise.  Zero estimates do yield 0, step 1.)
 *      c. the tail-biting decoder of the CQI section, step 2b (the same device code), over the N steps: maximum-correlation Viterbi, all
 *         64 metrics 0 at the start, three laps, the even predecessor on a tie, end state the first maximum in state order, traceback
 *         over all 3 N steps, the bits of the middle lap; metric = the decided word re-encoded and correlated with d.
 *      d. x = CRC16 remainder (0x11021, register 0) of the n_bits information bits XOR the 16 received parity bits: the RNTI when the
 *         CRC matches (antenna-selection mask 0).  A hit needs x != 0, x in the RNTI set, and either MI_LTE_PDCCH_SEARCH_ANY_CCE, or the
 *         candidate in the common search space, or the candidate among x's own UE-specific candidates of this subframe (the arithmetic
 *         of mi_lte_pdcch_search_space, on the device).
 *   3. k_pdcch_search_compact, one wavefront per unit: the hits ordered by (L descending, first CCE ascending, position of the size in
 *      the plan's list ascending); the first MI_LTE_PDCCH_SEARCH_MAX_FOUND are written, h_n_found[u] is the total and may exceed the cap
 *      (slots past the total are zero).  Only these lists, h_cfi, h_n_cce and h_n_found cross the link.
 * What the search does not resolve: a DCI sent at L = 4 is also found at L = 2 and L = 1 from the same first CCE (a prefix of its
 * rate-matched bits still decodes) and by the L = 8 candidate that holds it plus empty CCEs.  Each is reported with its metric and
 * energy; choosing among them is the caller's, like a DTX threshold elsewhere in this header.
 * mi_lte_pdcch_search_soft: the soft bits of the last run (device pointer into the plan, unit u at u * *unit_stride, 72 h_n_cce[u] valid). */
#define MI_LTE_PDCCH_SEARCH_MAX_SIZES 4
#define MI_LTE_PDCCH_SEARCH_MAX_FOUND 16
#define MI_LTE_PDCCH_SEARCH_ANY_CCE   1u   /* report a hit wherever it lies, not only inside its RNTI's search spaces */
#define MI_LTE_PDCCH_SEARCH_36211_REGS 2u  /* the plan's tables with the PHICH groups and N_reg of 36.211 (step 1, Positions), not the reference's */
typedef struct {
    uint32_t rnti, L, cce, n_bits;   /* cce = first CCE */
    uint64_t payload;                /* first DCI bit in bit n_bits-1 */
    int32_t  metric, energy;         /* as mi_lte_cqi_result: decided word re-encoded against d; sum |d| */
} mi_lte_pdcch_found;
typedef struct mi_lte_pdcch_search_plan mi_lte_pdcch_search_plan;
int  mi_lte_pdcch_search_space(uint32_t rnti, uint32_t subfr_num, uint32_t N_cce, uint32_t L, uint32_t *first_cce /* [6] */, uint32_t *n);
int  mi_lte_pdcch_search_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, float phich_res, uint32_t phich_dur_extended, uint32_t flags,
                                     const uint32_t *h_cells, uint32_t n_cells, const uint32_t *h_n_bits, uint32_t n_sizes,
                                     mi_lte_pdcch_search_plan **out);
int  mi_lte_pdcch_search_plan_set_rntis(mi_lte_ctx *ctx, mi_lte_pdcch_search_plan *plan, const uint32_t *h_rnti, uint32_t n_rnti);
void mi_lte_pdcch_search_plan_destroy(mi_lte_ctx *ctx, mi_lte_pdcch_search_plan *plan);
int  mi_lte_pdcch_search_run(mi_lte_ctx *ctx, mi_lte_pdcch_search_plan *plan, const float *d_subframes, const uint32_t *d_subfr_num,
                             const uint32_t *d_n_id_cell, uint32_t n_units, uint32_t *h_cfi, uint32_t *h_n_cce, uint32_t *h_n_found,
                             mi_lte_pdcch_found *h_found /* [n_units][MI_LTE_PDCCH_SEARCH_MAX_FOUND] */);
int  mi_lte_pdcch_search_soft(const mi_lte_pdcch_search_plan *plan, const int8_t **d_soft, uint32_t *unit_stride); /* valid after a run */
/* a search plan's table for one (cell, N_symbs) on its own (host arithmetic): *n_cce, and the grid indices l*1200 + k of the first min(*n_cce, n_max)
 * CCEs' 36 resource elements in order.  flags: 0 or MI_LTE_PDCCH_SEARCH_36211_REGS.  MI_LTE_ERR_INVALID_ARG as mi_lte_pdcch_re_tables. */
int  mi_lte_pdcch_cce_tables(uint32_t N_rb_dl, uint32_t N_ant, uint32_t N_id_cell, float phich_res, uint32_t N_symbs, uint32_t flags,
                             uint32_t *n_cce, uint32_t *cce_re /* [36 n_max] */, uint32_t n_max);
/* A C-RNTI's DCI format 0 / 1A as this library's transmitter packs them (tx_ctrl.cc, pinned to the reference's dci_0_pack / dci_1a_pack; packer
 * and unpacker read one field list, dci.h), host arithmetic (dci.cc).  Both: the flag bit (1 = format 1A, 0 = format 0), then one more flag, then the resource indication value in
 * ceil(log2(N_rb (N_rb + 1) / 2)) bits, decoded over its WHOLE range (36.213 7.1.6.3 / 8.1): with q = floor(RIV / N_rb), r = RIV mod N_rb,
 * length = q + 1 and start = r when q + r < N_rb, otherwise length = N_rb - q + 1 and start = N_rb - 1 - r.
 * Format 1A: localized (0) / distributed (1), RIV, MCS 5 bits, HARQ process 3, NDI 1, RV 2, TPC 2.  MCS 0-9 QPSK, 10-16 16QAM, 17-28 64QAM
 * with I_TBS = MCS, MCS - 1, MCS - 2; tbs = 8 x (36.213 table 7.1.7.2.1-1)[I_TBS][N_prb - 1].  alloc is filled (mod_type, tbs, rv_idx,
 * tx_mode = 1 or 2 by N_ant, rnti, N_prb, prb[2][N_prb]; unit and n_pdcch_symbs left 0) for the 3GPP PDSCH plans.
 * Format 0: hopping flag, RIV over N_rb (= N_rb_ul), MCS / RV 5 bits, NDI 1, TPC 2, DMRS cyclic shift 3, CQI request 1, padding.  alloc carries
 * rnti, N_prb and prb only (the uplink transport block is the PUSCH plan's business).
 * Returns 0; 4 for what has no transport block of its own here -- MCS 29-31 (either format), a distributed assignment, a RIV past
 * N_rb (N_rb + 1) / 2 - 1 -- with every field read so far filled in; MI_LTE_ERR_INVALID_ARG: a null pointer, n_bits > 64 or too small for the
 * fields, rnti = 0 or > 0xFFFF, N_rb = 0 or > 110, N_ant not 1 / 2 / 4. */
typedef struct {
    uint32_t format;        /* 0 = DCI format 0, 1 = DCI format 1A                                   */
    uint32_t flag;          /* format 1A: 1 = distributed VRBs; format 0: the hopping flag           */
    uint32_t riv, rb_start, N_prb;
    uint32_t mcs, harq, ndi, rv, tpc;   /* harq, rv: format 1A only                                  */
    uint32_t cyclic_shift, cqi_request; /* format 0 only                                             */
    mi_lte_pdsch_alloc alloc;
} mi_lte_dci_crnti;
int  mi_lte_dci_0_1a_unpack_crnti(uint64_t payload, uint32_t n_bits, uint32_t rnti, uint32_t N_rb, uint32_t N_ant, mi_lte_dci_crnti *out);

/* ---------------------------------------------------------------- PHICH, 3GPP mode: the HARQ indicators that answer a PUSCH (opt-in)
 * mi_lte_phich_* decode what phich_channel_map sends (liblte/src/liblte_phy.cc:8076-8215; this library's transmitter: mi_lte_pdcch_channel_encode).
 * The reference has no PHICH decoder -- phich_channel_demap (liblte_phy.cc:8243-8278) only computes the positions, so that the PDCCH can keep
 * off them -- so the specification is the authority: 36.211 6.9 and 36.213 9.1.2.  FDD, normal cyclic prefix, normal PHICH duration (symbol 0
 * only), N_SF = 4; the six standard bandwidths, N_g in (0, 2], cells of 1, 2 and 4 CRS ports, full estimate planes (not MI_LTE_CE_COMPACT).
 *
 * Host arithmetic.  mi_lte_phich_n_group: N_group = ceil(N_g N_rb_dl / 8), what the PDCCH tables and N_reg / 3 of mi_lte_ctrl_reg_positions
 *   count; 0 for a non-standard bandwidth or an N_g outside (0, 2].  mi_lte_phich_resource (36.213 9.1.2, N_SF = 4): the PHICH that answers
 *   the PUSCH whose first slot starts at resource block I_prb_ra_lowest, sent with DMRS cyclic-shift field n_dmrs:
 *     n_group = (I_prb_ra_lowest + n_dmrs) mod N_group + I_phich N_group,  n_seq = (floor(I_prb_ra_lowest / N_group) + n_dmrs) mod 8;
 *   MI_LTE_ERR_INVALID_ARG for N_group = 0, n_dmrs > 7, null pointers.  mi_lte_phich_re_table: the plan's index table for one cell,
 *   re[12 m + 4 i + j] (below); MI_LTE_ERR_INVALID_ARG where mi_lte_phich_n_group gives 0, for a cell past 503 and for null pointers.
 *
 * Positions.  Group m's three REGs are those of phich_channel_demap (:8243-8278): first sub-carrier 6 n_i, n_i counted among the REGs the
 *   PCFICH left, exactly what mi_lte_ctrl_reg_positions reports and the PDCCH tables exclude.  Quadruplet i = 0 .. 2 occupies, in increasing
 *   k, the four of REG i's six sub-carriers with k mod 3 != N_id_cell mod 3: RE(4 i + j), j = 0 .. 3, all in symbol 0.  (The reference steps
 *   over the PCFICH REGs in the order they are listed, not in ascending order, so in some cells a PHICH REG lands on a PCFICH REG; the
 *   positions are kept as the transmitter writes them.)
 * Scrambling.  c(0) .. c(11): the first 12 bits of the Gold sequence with c_init = ((subfr_num + 1) (2 N_id_cell + 1) << 9) + N_id_cell
 *   (phich_channel_map :8076-8215 uses the same); s(e) = 1 - 2 c(e).
 * Sequences.  w_n(j) = walsh[n mod 4][j] (n < 4 ? 1 : j_imag), n = 0 .. 7, walsh = {++++, +-+-, ++--, +--+} (36.211 table 6.9.1-2).  BPSK
 *   reference z0 = (1 + j) / sqrt 2; HI = 0 (NACK) is sent as +z0, HI = 1 (ACK) as -z0 (36.212 5.3.5, 36.211 table 7.1.1-1).
 * Combining.  y(e), h_p(e): the unit's received element and port p's estimate at RE(e), read from the device subframe of
 *   mi_lte_dl_frontend_batch (y planes, then N_ant real and N_ant imaginary estimate planes, index l 1200 + k).
 *   1 port:  r(e) = y(e) conj(h_0(e)), P(e) = |h_0(e)|^2.
 *   2 ports: pairs (a, b) = (4 i, 4 i + 1) and (4 i + 2, 4 i + 3) of the pre-coder of 36.211 6.3.4.3, ports (A, B) = (0, 1):
 *     r(a) = sqrt 2 (conj(h_A(a)) y(a) + h_B(b) conj(y(b))),  P(a) = |h_A(a)|^2 + |h_B(b)|^2,
 *     r(b) = sqrt 2 (conj(h_A(b)) y(b) - h_B(a) conj(y(a))),  P(b) = |h_A(b)|^2 + |h_B(a)|^2.
 *   4 ports: the same with (A, B) = (0, 2) when (i + m) mod 2 = 0 and (1, 3) otherwise, for the whole quadruplet (36.211 6.9.2 -- not the
 *     PDSCH's alternation inside a group of four).
 * Despreading, float32, every sum in the order written:
 *   q_i(n) = sum_{j = 0..3} conj(w_n(j)) s(4 i + j) r(4 i + j);  P_tot = sum_{e = 0..11} P(e);
 *   rep_i(n) = Re(q_i(n) conj(z0)) / P_tot;  metric(n) = rep_0 + rep_1 + rep_2;  hi(n) = (metric(n) < 0).
 *   Without noise a present indicator gives -+1 and an absent one 0; sequences n and n + 4 separate in the projection onto z0.
 *   P_tot = 0 or not finite: metric = rep = power = 0, hi = 0, flags = MI_LTE_PHICH_NO_POWER.  A unit whose cell the plan was not built for
 *   (or whose subframe number is past 9): the same zeros with flags = MI_LTE_PHICH_UNKNOWN_CELL.  A DTX threshold on metric is the caller's.
 * mi_lte_phich_plan_create holds, per listed cell and group, the 12 grid indices, and N_group.  MI_LTE_ERR_INVALID_ARG, nothing allocated:
 *   null pointers, n_cells = 0, a cell past 503, and -- with the context's error text set -- a non-standard bandwidth, a port count other
 *   than 1 / 2 / 4, N_g outside (0, 2], the extended PHICH duration (refused as mi_lte_pdcch_plan_create refuses it), MI_LTE_CE_COMPACT in
 *   cfg->sample_format, flags other than 0.
 * mi_lte_phich_decode_run, the dense form: one launch of k_phich_decode (one workgroup per unit) on the context's stream, which the call does
 *   not wait for; d_out (device memory) receives [n_units][N_group][8] records, every group and sequence of every unit.  No atomics: two
 *   runs give the same bytes.  MI_LTE_ERR_INVALID_ARG before any launch: null pointers, n_units = 0. */
#define MI_LTE_PHICH_NO_POWER     1u
#define MI_LTE_PHICH_UNKNOWN_CELL 2u
typedef struct {
    float    metric;     /* rep[0] + rep[1] + rep[2]: about -1 ACK, +1 NACK, 0 nothing sent */
    float    power;      /* P_tot                                                            */
    float    rep[3];     /* the three repetitions: stage taps                                */
    uint32_t hi;         /* metric < 0: 1 = ACK                                              */
    uint32_t flags;      /* MI_LTE_PHICH_NO_POWER, MI_LTE_PHICH_UNKNOWN_CELL                 */
    uint32_t reserved;
} mi_lte_phich_result;   /* 32 bytes */
typedef struct mi_lte_phich_plan mi_lte_phich_plan;
uint32_t mi_lte_phich_n_group(uint32_t N_rb_dl, float phich_res);
int  mi_lte_phich_resource(uint32_t I_prb_ra_lowest, uint32_t n_dmrs, uint32_t N_group, uint32_t I_phich, uint32_t *n_group, uint32_t *n_seq);
int  mi_lte_phich_re_table(uint32_t N_rb_dl, uint32_t N_id_cell, float phich_res, uint32_t *N_group, uint32_t *re /* [25][12] */);
int  mi_lte_phich_plan_create(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, float phich_res /* N_g: 1/6, 1/2, 1, 2 */, uint32_t phich_dur_extended,
                              uint32_t flags, const uint32_t *h_cells, uint32_t n_cells, mi_lte_phich_plan **out);
void mi_lte_phich_plan_destroy(mi_lte_ctx *ctx, mi_lte_phich_plan *plan);
uint32_t mi_lte_phich_plan_n_group(const mi_lte_phich_plan *plan);
int  mi_lte_phich_decode_run(mi_lte_ctx *ctx, mi_lte_phich_plan *plan, const float *d_subframes, const uint32_t *d_subfr_num,
                             const uint32_t *d_n_id_cell, uint32_t n_units, mi_lte_phich_result *d_out /* [n_units][N_group][8] */);

/* ---------------------------------------------------------------- PBCH
 * mi_lte_pbch_decode_run replaces liblte_phy_bch_channel_decode() (liblte/hdr/liblte_phy.h:947-953, implementation
 * liblte/src/liblte_phy.cc:3968-4105 with bch_channel_decode :12581-12650) for a batch of device subframes holding subframe 0
 * of a frame with channel estimates for all four ports (cfg->N_ant = 4: the reference tries 1, 2 and 4 ports against the
 * same struct, LTE_fdd_dl_fs_samp_buf.cc:395-410).  Twelve hypotheses per subframe -- {1, 2, 4} ports x {0..3} position
 * in the 40 ms BCH period -- in the reference's order, first success wins: h_N_ant[u] (0 = LIBLTE_ERROR_DECODE_FAIL),
 * h_offset[u] (the reference's *offset: SFN mod 4), h_mib[u] = the 24 BCH bits, first bit in bit 23. */
int mi_lte_pbch_decode_run(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const float *d_subframes, const uint32_t *d_n_id_cell,
                           uint32_t n_units, uint32_t *h_N_ant, uint32_t *h_offset, uint32_t *h_mib);

/* ---------------------------------------------------------------- initial synchronisation
 * The three searches that precede the first subframe (LTE_fdd_dl_fs_samp_buf.cc:277-395), over samples resident in HBM
 * (format as for mi_lte_dl_frontend_batch; `start` = index of the capture's first sample in the buffer):
 *   mi_lte_coarse_timing_run  replaces liblte_phy_dl_find_coarse_timing_and_freq_offset (liblte_phy.h:1134-1138, impl.
 *       liblte_phy.cc:5697-5852); reads mi_lte_coarse_timing_samples(fft_size, N_slots) samples.  mi_lte_coarse_timing is
 *       LIBLTE_PHY_COARSE_TIMING_STRUCT (liblte_phy.h:1128-1132).
 *   mi_lte_find_pss_run       replaces liblte_phy_find_pss_and_fine_timing (liblte_phy.h:1068-1075, impl. :5306-5510);
 *       symb_starts[7] is read and rewritten like the reference's; reads up to symb_starts[6] + 12 slots + one symbol + 40.
 *   mi_lte_find_sss_run       replaces liblte_phy_find_sss (liblte_phy.h:1106-1113, impl. :5578-5687); *found = 0 is the
 *       reference's LIBLTE_ERROR_INVALID_INPUTS return (no SSS above 0.9 x pss_thresh).
 * The device computes every correlation sum in the reference's summation order; the decisions on them are evaluated on the
 * host with the reference's expressions.  Coarse timing is bit-identical for integer-valued samples (all sums are exact);
 * the PSS / SSS stages sit behind an FFT and agree to its tolerance (decisions identical unless two candidates tie). */
typedef struct {
    float    freq_offset[5];
    uint32_t symb_starts[5][7];
    uint32_t n_corr_peaks;
} mi_lte_coarse_timing;
size_t mi_lte_coarse_timing_samples(uint32_t fft_size, uint32_t N_slots);
int    mi_lte_coarse_timing_run(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const void *d_samples_a, const void *d_samples_b,
                                uint64_t start, uint32_t N_slots, mi_lte_coarse_timing *out);
int    mi_lte_find_pss_run(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const void *d_samples_a, const void *d_samples_b, uint64_t start,
                           uint32_t *symb_starts /* [7] in/out */, uint32_t *N_id_2, uint32_t *pss_symb, float *pss_thresh,
                           float *freq_offset);
int    mi_lte_find_sss_run(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const void *d_samples_a, const void *d_samples_b, uint64_t start,
                           uint32_t N_id_2, uint32_t *symb_starts /* [7] in/out */, float pss_thresh, uint32_t *N_id_1,
                           uint32_t *frame_start_idx, uint32_t *found);

/* For tests and not for callers: what the kernels of the three searches wrote, copied out.  Each tap runs the same device part as
 * its _run (one function in sync.hip serves both), waits for the stream and forms no verdict; it returns
 * MI_LTE_ERR_INVALID_ARG where its _run does and for a NULL output.  n_slot = 15360 fft_size / 2048, N_sc = 12 N_rb_dl.
 *   mi_lte_coarse_timing_tap  h_corr: float pairs (re, im) [N_slots][n_slot], k_cp_corr's sums; h_acc: float [n_slot], k_cp_accum's.
 *   mi_lte_find_pss_tap       h_rows: float [84][2][1200], the 12 x 7 symbols' spectra as k_sync_fft wrote them (real parts, then
 *       imaginary parts; the first N_sc columns of each are written, the rest is left as it was); h_corr: float pairs [84][9], row
 *       r against PSS k at sub-carrier shift sft - 1 in column 3 k + sft; h_fine_rows: float [80][2][1200] and h_fine_corr: float pairs
 *       [80] of the fine-timing pass.  That pass depends on the first one's verdict, which the tap does NOT form: the caller passes
 *       N_id_2 (0..2), pss_symb (0..83) and shift (-1, 0, +1) -- from h_corr of an earlier call, or as mi_lte_find_pss_run gave them.
 *   mi_lte_find_sss_tap       h_row: float [2][1200] (first N_sc columns written), the symbol at symb_starts[5]; h_corr: float
 *       pairs [336], N_id_1 i against subframe 0's sequence in column 2 i and subframe 5's in column 2 i + 1. */
int    mi_lte_coarse_timing_tap(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const void *d_samples_a, const void *d_samples_b,
                                uint64_t start, uint32_t N_slots, float *h_corr, float *h_acc);
int    mi_lte_find_pss_tap(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const void *d_samples_a, const void *d_samples_b, uint64_t start,
                           const uint32_t *symb_starts /* [7] */, uint32_t N_id_2, uint32_t pss_symb, int32_t shift, float *h_rows,
                           float *h_corr, float *h_fine_rows, float *h_fine_corr);
int    mi_lte_find_sss_tap(mi_lte_ctx *ctx, const mi_lte_dl_cfg *cfg, const void *d_samples_a, const void *d_samples_b, uint64_t start,
                           uint32_t N_id_2, const uint32_t *symb_starts /* [7]; [5] is read */, float *h_row, float *h_corr);

/* The scanner's caller-side steps between the searches, for a capture that stays in HBM:
 *   mi_lte_iq_i8_to_planar  int8 I,Q pairs -> planar fp32 i_samps / q_samps (LTE_fdd_dl_fs_samp_buf.cc:657-694);
 *   mi_lte_freq_shift_run   LTE_fdd_dl_fs_samp_buf::freq_shift (:696-713) in place: sample i (buffer index first_index + k for
 *       k < n_samples, the reference's loop variable) is rotated by exp(-j*(i+1)*freq_offset*2*pi/fs), the argument evaluated in
 *       the mixed float / double precision of the reference's expression; cosf / sinf are the device library's (<= 2 ulp), so the
 *       result agrees with the host's to float rounding, like the FFT behind it. */
int mi_lte_iq_i8_to_planar(mi_lte_ctx *ctx, const int8_t *d_iq, uint64_t n_samples, float *d_i_samps, float *d_q_samps);
/* the scanner's other input format, gr_complex = interleaved float32 pairs (LTE_fdd_dl_fs_samp_buf.cc:686-692) -> planar fp32 */
int mi_lte_iq_f32_pairs_to_planar(mi_lte_ctx *ctx, const float *d_iq, uint64_t n_samples, float *d_i_samps, float *d_q_samps);
int mi_lte_freq_shift_run(mi_lte_ctx *ctx, float *d_i_samps, float *d_q_samps, uint64_t first_index, uint64_t n_samples, float freq_offset,
                          uint32_t fs);

/* ---------------------------------------------------------------- per-call host-pointer forms
 * The bodies of the reference's three entry points on this path, for callers that hold host
 * buffers exactly as the reference's callers do (LTE_fdd_dl_fs_samp_buf.cc:378-515,
 * LTE_fdd_enb_phy.cc).  Each stages its arguments through HBM, runs the batch kernels with a batch
 * of one, and copies the results back; shim/liblte_phy_shim.cc forwards the liblte_phy_* symbols
 * here.  Return value: MI_LTE_* on infrastructure errors (< 0), else the LIBLTE_ERROR_ENUM value the
 * reference would return (0 success, 1 invalid inputs, 2 decode fail). */
/* Nothing in these forms allocates per call: a context keeps pinned staging, device buffers and ONE device subframe tagged with the host
 * arrays it mirrors (rx_symb_re's address + a 64-bit hash of the whole contents, rows 0-13 of every plane), plus plans cached by
 * everything they were built from.  The decoders called on a subframe this context produced with mi_lte_get_dl_subframe_and_ce_host /
 * _get_ul_subframe_host -- or uploaded for an earlier call -- read the copy that is already in HBM; a subframe whose arrays changed in
 * any element hashes differently and is uploaded again (mi_lte_host_cache_invalidate forces that).  One call at a time per context, like the reference's
 * "one call at a time per LIBLTE_PHY_STRUCT" (SURVEY 8b). */
int mi_lte_host_cache_stats(mi_lte_ctx *ctx, uint64_t *n_subframe_reuse, uint64_t *n_subframe_upload, uint32_t *n_plans);
int mi_lte_host_cache_invalidate(mi_lte_ctx *ctx);
/* The explicit contract instead of the hash: in MI_LTE_HOST_CACHE_EXPLICIT mode the copy in HBM counts as current for as long as the
 * decoders are handed the same arrays (rx_symb_re's address, same port count) -- a caller that changes a subframe's contents between
 * decodes says so with mi_lte_host_cache_invalidate.  What LTE_fdd_dl_fs_samp_buf.cc does (it never touches a subframe between
 * get_dl_subframe_and_ce and the decodes) qualifies; the default, MI_LTE_HOST_CACHE_FINGERPRINT, is safe for any caller. */
enum { MI_LTE_HOST_CACHE_FINGERPRINT = 0, MI_LTE_HOST_CACHE_EXPLICIT = 1 };
int mi_lte_host_cache_set_mode(mi_lte_ctx *ctx, uint32_t mode);
/* One subframe in one call: the work of liblte_phy_get_dl_subframe_and_ce + liblte_phy_pdcch_channel_decode +
 * liblte_phy_pdsch_channel_decode for every DCI found (the loop at LTE_fdd_dl_fs_samp_buf.cc:445-515), arguments as those calls take
 * them.  The subframe stays in HBM (no LIBLTE_PHY_SUBFRAME_STRUCT comes back), the host waits twice.  Returns what
 * liblte_phy_pdcch_channel_decode would (0, 1, 2) or MI_LTE_* < 0; on 0, dci[k] (k < *N_dci) is decoded into
 * h_out_bits + k * out_stride (out_stride >= 6120) with status[k] = 0 and N_out_bits[k] = tbs, or status[k] = 2 and nothing
 * written (CRC mismatch, or a transport block outside the single-code-block envelope). */
int mi_lte_dl_subframe_decode_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_dl, const float *h_i_samps, const float *h_q_samps,
                                   uint32_t frame_start_idx, uint32_t subfr_num, uint32_t N_id_cell, uint32_t N_ant, float phich_res,
                                   uint32_t phich_dur_extended, uint32_t flags, uint32_t *cfi, uint32_t *N_symbs, uint32_t *N_dci,
                                   mi_lte_pdcch_dci *dci /* [MI_LTE_PDCCH_MAX_DCI] */, uint8_t *h_out_bits, uint32_t out_stride,
                                   uint32_t *N_out_bits /* [MI_LTE_PDCCH_MAX_DCI] */, int32_t *status /* [MI_LTE_PDCCH_MAX_DCI] */);
/* One UPLINK subframe in one call: the work of liblte_phy_get_ul_subframe (liblte_phy.h:1190-1193, liblte_phy.cc:6209-6236) +
 * liblte_phy_pucch_format_1_1a_1b_channel_decode per resource (liblte_phy.h:775-782, liblte_phy.cc:2961-3146) +
 * liblte_phy_pusch_channel_decode per scheduled UE (liblte_phy.h:722-728, liblte_phy.cc:2801-2935) -- the eNodeB radio thread's receive
 * half of a TTI (LTE_fdd_enb_phy.cc:832-917) -- as one launch chain with one wait; the received grid stays in HBM.  h_i / h_q: the
 * subframe's 30720 / (2048 / fft_size) samples; ul: what liblte_phy_ul_init was given (the reference signals are generated from it);
 * allocs[k] (k < n_alloc <= MI_LTE_UL_SUBFRAME_MAX_ALLOC) is decoded into h_out_bits + k * out_stride (out_stride >= 6120) with
 * status[k] = 0 and N_out_bits[k] = tbs, or status[k] = 1 (the reference's failure value on this path: CRC mismatch, or an allocation it
 * has no transform plan for) and nothing written; pucch[r] (unit 0) with h_pucch_tables as for mi_lte_pucch_decode_run.  Returns 0,
 * 1 (invalid arguments, the reference's value) or MI_LTE_* < 0. */
#define MI_LTE_UL_SUBFRAME_MAX_ALLOC 16
int mi_lte_ul_subframe_decode_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_ul, const float *h_i_samps, const float *h_q_samps,
                                   uint32_t subfr_num, uint32_t N_id_cell, const mi_lte_ul_cfg *ul, const mi_lte_pdsch_alloc *allocs,
                                   uint32_t n_alloc, uint8_t *h_out_bits, uint32_t out_stride, uint32_t *N_out_bits, int32_t *status,
                                   const mi_lte_pucch_res *pucch, const float *h_pucch_tables, uint32_t n_pucch, uint8_t *h_pucch_bits /*[n_pucch][2]*/,
                                   uint32_t *h_pucch_n_bits, uint32_t *h_pucch_rc);
int mi_lte_get_dl_subframe_and_ce_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_dl, const float *h_i_samps,
                                       const float *h_q_samps, uint32_t frame_start_idx, uint32_t subfr_num,
                                       uint32_t N_id_cell, uint32_t N_ant, float *h_rx_symb_re /*[16][1200]*/,
                                       float *h_rx_symb_im, float *h_rx_ce_re /*[4][16][1200]*/, float *h_rx_ce_im);
int mi_lte_pdsch_channel_decode_host(mi_lte_ctx *ctx, uint32_t N_rb_dl, const float *h_rx_symb_re, const float *h_rx_symb_im,
                                     const float *h_rx_ce_re, const float *h_rx_ce_im, uint32_t subfr_num,
                                     const mi_lte_pdsch_alloc *alloc, uint32_t N_pdcch_symbs, uint32_t N_id_cell,
                                     uint32_t N_ant, uint8_t *h_out_bits, uint32_t *N_out_bits);
/* liblte_phy_pdcch_channel_decode: returns the reference's value (0; 1 no DCI found; 3 PCFICH failed; 4 last DCI did
 * not unpack) with *cfi, *N_symbs, *N_dci and dci[] as mi_lte_pdcch_decode_run writes them for one subframe */
int mi_lte_pdcch_channel_decode_host(mi_lte_ctx *ctx, uint32_t N_rb_dl, const float *h_rx_symb_re, const float *h_rx_symb_im,
                                     const float *h_rx_ce_re, const float *h_rx_ce_im, uint32_t subfr_num, uint32_t N_id_cell,
                                     uint32_t N_ant, float phich_res, uint32_t phich_dur_extended, uint32_t flags, uint32_t *cfi,
                                     uint32_t *N_symbs, uint32_t *N_dci, mi_lte_pdcch_dci *dci /* [MI_LTE_PDCCH_MAX_DCI] */);
/* liblte_phy_bch_channel_decode: 0 with *N_ant, h_out_bits[24], *N_out_bits = 24 and *offset written, or 2
 * (LIBLTE_ERROR_DECODE_FAIL) with *N_ant = 0 and the rest untouched; h_rx_ce_* hold all four ports */
int mi_lte_bch_channel_decode_host(mi_lte_ctx *ctx, uint32_t N_rb_dl, const float *h_rx_symb_re, const float *h_rx_symb_im,
                                   const float *h_rx_ce_re /*[4][16][1200]*/, const float *h_rx_ce_im, uint32_t N_id_cell, uint8_t *N_ant,
                                   uint8_t *h_out_bits, uint32_t *N_out_bits, uint8_t *offset);
/* liblte_phy_pucch_format_1_1a_1b_channel_decode: 0 or 1 (the reference's failure value) with the bit(s) and their count written
 * in both cases, as the reference does; h_tables as for mi_lte_pucch_decode_run */
int mi_lte_pucch_decode_host(mi_lte_ctx *ctx, uint32_t N_rb_ul, const float *h_rx_symb_re, const float *h_rx_symb_im, uint32_t format,
                             uint32_t N_ant, uint32_t N_1_p_pucch, const float *h_tables, uint8_t *h_out_bits, uint32_t *N_out_bits);
/* the three synchronisation searches on host sample arrays (they read exactly as far as the reference does); find_sss
 * returns 1 (LIBLTE_ERROR_INVALID_INPUTS, the reference's value) when no SSS clears the threshold */
int mi_lte_dl_find_coarse_timing_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_dl, const float *h_i_samps, const float *h_q_samps,
                                      uint32_t N_slots, mi_lte_coarse_timing *out);
int mi_lte_find_pss_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_dl, const float *h_i_samps, const float *h_q_samps,
                         uint32_t *symb_starts, uint32_t *N_id_2, uint32_t *pss_symb, float *pss_thresh, float *freq_offset);
int mi_lte_find_sss_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_dl, const float *h_i_samps, const float *h_q_samps, uint32_t N_id_2,
                         uint32_t *symb_starts, float pss_thresh, uint32_t *N_id_1, uint32_t *frame_start_idx);
/* uplink: liblte_phy_get_ul_subframe (h_i / h_q point at the subframe's first sample; 14 rows of 1200 floats are
 * written) and liblte_phy_pusch_channel_decode (the DMRS arrays are the caller's, i.e. what liblte_phy_ul_init
 * stored in LIBLTE_PHY_STRUCT::pusch_dmrs_{0,1}_{re,im}[subframe][N_prb]; a CRC failure returns 1 =
 * LIBLTE_ERROR_INVALID_INPUTS like the reference, liblte_phy.cc:2809, :2929) */
int mi_lte_get_ul_subframe_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_ul, const float *h_i_samps, const float *h_q_samps,
                                float *h_rx_symb_re /*[16][1200]*/, float *h_rx_symb_im);
int mi_lte_pusch_channel_decode_host(mi_lte_ctx *ctx, uint32_t N_rb_ul, const float *h_rx_symb_re, const float *h_rx_symb_im,
                                     uint32_t subfr_num, const mi_lte_pdsch_alloc *alloc, uint32_t N_id_cell, uint32_t N_ant,
                                     const float *h_dmrs_0_re, const float *h_dmrs_0_im, const float *h_dmrs_1_re,
                                     const float *h_dmrs_1_im, uint8_t *h_out_bits, uint32_t *N_out_bits);
/* liblte_phy_detect_prach: h_re / h_im point at the occasion's first cyclic-prefix sample; root spectra from the caller's struct
 * (LIBLTE_PHY_STRUCT::prach_x_u_fft_*, what liblte_phy_ul_init left there), or both pointers NULL: the library generates the cell's
 * root set itself (mi_lte_prach_plan_create; n_roots is ignored) */
int mi_lte_detect_prach_host(mi_lte_ctx *ctx, uint32_t fft_size, uint32_t N_rb_ul, const mi_lte_prach_cfg *prach,
                             const float *h_x_u_fft_re /*[n_roots][839]*/, const float *h_x_u_fft_im, uint32_t n_roots, const float *h_re,
                             const float *h_im, uint32_t *N_det_pre, uint32_t *det_pre, uint32_t *det_ta);
int mi_lte_rate_unmatch_turbo_host(mi_lte_ctx *ctx, const float *h_e_bits, uint32_t N_e_bits, uint32_t N_dummy_bits,
                                   uint32_t N_codeblocks, uint32_t tx_mode, uint32_t N_soft, uint32_t M_dl_harq,
                                   uint32_t chan_type, uint32_t rv_idx, float *h_d_bits, uint32_t *N_d_bits);

/* ---------------------------------------------------------------- scheduler-side helpers ("CPU pass-through restatements")
 * Pure host functions of a few small integers that LTE_fdd_enodeb calls every TTI next to the receive chains; no context, no device.
 * Each returns what the reference's function returns (a LIBLTE_ERROR_ENUM value where that one does) and leaves its outputs untouched
 * exactly where the reference does (a search that finds nothing).  sched.cc; compared with the compiled reference over their whole
 * argument ranges by shim/lifecycle_check.
 *   mi_lte_tbs                              36.213 table 7.1.7.2.1-1, I_TBS 0..26, N_PRB 1..110 (TBS_71721, liblte_phy.cc:477-746); 0 outside
 *   mi_lte_get_tbs_mcs_and_n_prb_for_dl     liblte_phy_get_tbs_mcs_and_n_prb_for_dl   liblte_phy.h:1210   liblte_phy.cc:6251-6357
 *   mi_lte_get_tbs_and_n_prb_for_dl         liblte_phy_get_tbs_and_n_prb_for_dl       liblte_phy.h:1234   liblte_phy.cc:6359-6407
 *   mi_lte_get_tbs_mcs_and_n_prb_for_ul     liblte_phy_get_tbs_mcs_and_n_prb_for_ul   liblte_phy.h:1253   liblte_phy.cc:6409-6475
 *   mi_lte_get_n_cce                        liblte_phy_get_n_cce                      liblte_phy.h:1271   liblte_phy.cc:6477-6505 (the struct's
 *                                           N_rb_dl and N_group_phich as arguments; phich_res is not read by the reference either)
 *   mi_lte_pucch_map_sr_config_idx          liblte_phy_pucch_map_sr_config_idx        liblte_phy.h:830    liblte_phy.cc:3183-3217
 *   mi_lte_code_block_segmentation          liblte_phy_code_block_segmentation        liblte_phy.h:1337   liblte_phy.cc:9753-9865
 *   mi_lte_code_block_desegmentation        liblte_phy_code_block_desegmentation      liblte_phy.h:1357   liblte_phy.cc:9875-9987 */
uint32_t mi_lte_tbs(uint32_t I_tbs, uint32_t N_prb);
int      mi_lte_get_tbs_mcs_and_n_prb_for_dl(uint32_t N_bits, uint32_t N_subframe, uint32_t N_rb_dl, uint16_t rnti, uint32_t *tbs, uint8_t *mcs,
                                             uint32_t *N_prb);
int      mi_lte_get_tbs_and_n_prb_for_dl(uint32_t N_bits, uint32_t N_rb_dl, uint8_t mcs, uint32_t *tbs, uint32_t *N_prb);
int      mi_lte_get_tbs_mcs_and_n_prb_for_ul(uint32_t N_bits, uint32_t N_rb_ul, uint32_t *tbs, uint8_t *mcs, uint32_t *N_prb);
uint32_t mi_lte_get_n_cce(uint32_t N_rb_dl, uint32_t N_group_phich, uint32_t N_pdcch_symbs, uint32_t N_ant);
void     mi_lte_pucch_map_sr_config_idx(uint32_t i_sr, uint32_t *sr_periodicity, uint32_t *N_offset_sr);
void     mi_lte_code_block_segmentation(const uint8_t *b_bits, uint32_t N_b_bits, uint32_t *N_codeblocks, uint32_t *N_filler_bits, uint8_t *c_bits,
                                        uint32_t N_c_bits_max, uint32_t *N_c_bits);
void     mi_lte_code_block_desegmentation(const uint8_t *c_bits, const uint32_t *N_c_bits, uint32_t N_c_bits_max, uint32_t tbs, uint8_t *b_bits,
                                          uint32_t N_b_bits);

/* ---------------------------------------------------------------- whole-chain batches from host buffers
 * Captures live in host memory, so the batch form for callers that hold host buffers: int8 I,Q in, transport blocks back packed eight
 * bits per byte ([allocation][mi_lte_dl_pipeline_out_stride()], first bit most significant) with one verdict per allocation.  The batch
 * is cut into chunks of chunk_units subframes that flow H2D -> front end -> PDSCH chain -> D2H on n_lanes independent lanes per device
 * (a context, a stream, plans and device buffers each), so that one lane's copies run under another lane's kernels; nothing is allocated
 * per run.  Host arrays should come from mi_lte_host_alloc (pinned, for every device of the process): with pageable memory the copies are
 * staged by the driver and do not overlap.  cfg->sample_format: MI_LTE_IQ_I8, optionally | MI_LTE_CE_COMPACT.  The link is the limit by
 * design: 70 KB of samples per 20 MHz subframe.
 *
 * Several devices: mi_lte_dl_pipeline_create_multi takes the device ordinals; chunk c of a run goes to device c mod n_devices,
 * every device is driven by its own host thread for the duration of the run, results land at the allocation's own index -- no collective,
 * no peer access.  The same ordinal may be listed more than once (the tests do: G "devices" on one GPU must reproduce the single-device
 * result bit for bit).
 *
 * Three shapes of input:
 *   mi_lte_dl_pipeline_run          units (each mi_lte_dl_pipeline_unit_samples() pairs: one subframe + the two look-ahead symbols, as for
 *                                   mi_lte_dl_frontend_batch with d_unit_start[u] = u * that) that all carry the allocation template the
 *                                   pipeline was created with (a semi-static grant pattern; the template's `unit` field is ignored);
 *                                   results at [unit * n_alloc_per_unit + a].
 *   mi_lte_dl_pipeline_run_units    the same units with PER-UNIT allocation lists -- what a capture yields once its PDCCHs are decoded
 *                                   (LTE_fdd_dl_fs_samp_buf.cc:445-515): h_allocs sorted by unit, h_first[u] .. h_first[u+1] the slice of
 *                                   unit u (n_units + 1 entries, at most n_alloc_per_unit per unit), each allocation's own n_pdcch_symbs or,
 *                                   where that is 0, N_pdcch_symbs; results at the allocation's index in h_allocs.
 *   mi_lte_dl_pipeline_run_capture  one CONTIGUOUS capture: n_subframes subframes from sample first_subframe_start on, subframe numbers
 *                                   first_subfr_num, +1, ... mod 10, one cell.  The capture is split on subframe boundaries and every chunk is
 *                                   copied with the 4 400 look-ahead samples (at 30.72 MHz) behind its last subframe -- the halo -- so that
 *                                   the split is invisible: results equal the unsplit run's. */
typedef struct mi_lte_dl_pipeline mi_lte_dl_pipeline;
void       *mi_lte_host_alloc(size_t bytes);
void        mi_lte_host_free(void *p);
/* Host placement ("each GPU owns a host thread"; eight devices at ~45 GB/s each read ~350 GB/s of host memory, which one
 * NUMA node does not serve).  mi_lte_device_numa_node: the node of the device's PCIe slot (/sys/bus/pci/devices/<bdf>/numa_node), -1
 * where the system does not say.  mi_lte_host_alloc_on: pinned memory for every device of the process like mi_lte_host_alloc, with its
 * pages bound to that node (anonymous mapping + mbind + hipHostRegister); falls back to mi_lte_host_alloc's placement where the node is
 * unknown or binding is not permitted -- mi_lte_host_alloc_node tells which happened (the node the block was bound to, -1 if none).
 * device < 0: a block that every device reads a share of (one contiguous capture for mi_lte_dl_pipeline_run_capture): its pages are
 * interleaved over all memory nodes (mi_lte_host_alloc_node: -2).
 * Release with mi_lte_host_free.  A multi-device pipeline pins every device's host thread to the CPUs of the device's node for the
 * duration of a run (the caller's own thread, which drives a single-device pipeline, is left alone). */
int         mi_lte_device_numa_node(int device);
void       *mi_lte_host_alloc_on(int device, size_t bytes);
int         mi_lte_host_alloc_node(const void *p);
int         mi_lte_dl_pipeline_create(int device, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_unit_allocs,
                                      uint32_t n_alloc_per_unit, uint32_t chunk_units, uint32_t n_lanes, mi_lte_dl_pipeline **out);
/* h_unit_allocs may be NULL (per-unit lists only): then n_alloc_per_unit is the most allocations a unit may carry and
 * max_soft_bytes_per_unit the soft bits of a unit's allocations, averaged over a chunk (0: one full-band 64QAM allocation's worth) */
int         mi_lte_dl_pipeline_create_multi(const int *devices, uint32_t n_devices, const mi_lte_dl_cfg *cfg, uint32_t N_pdcch_symbs,
                                            const mi_lte_pdsch_alloc *h_unit_allocs, uint32_t n_alloc_per_unit, size_t max_soft_bytes_per_unit,
                                            uint32_t chunk_units, uint32_t n_lanes, mi_lte_dl_pipeline **out);
void        mi_lte_dl_pipeline_destroy(mi_lte_dl_pipeline *p);
uint32_t    mi_lte_dl_pipeline_out_stride(const mi_lte_dl_pipeline *p);
size_t      mi_lte_dl_pipeline_unit_samples(const mi_lte_dl_pipeline *p);
uint32_t    mi_lte_dl_pipeline_n_devices(const mi_lte_dl_pipeline *p);
const char *mi_lte_dl_pipeline_last_error(const mi_lte_dl_pipeline *p);
/* What device slot `index` (0 .. n_devices-1) did in the pipeline's last run, so that a scaling run explains its own bottleneck: chunks
 * and units it took, bytes over its link each way, the time its stream spent in each phase summed over its chunks (HIP events on the
 * lanes' streams; phases of different lanes overlap, so the sums may exceed wall_s), the wall time of its host thread, and where that
 * thread ran (numa_node / n_cpus of the affinity mask it was given; -1 / 0: not pinned). */
typedef struct {
    uint32_t device, chunks, units, n_cpus;
    int32_t  numa_node, reserved;
    uint64_t h2d_bytes, d2h_bytes;
    double   wall_s, h2d_s, kernel_s, d2h_s;
} mi_lte_pipeline_dev_stats;
int         mi_lte_dl_pipeline_device_stats(const mi_lte_dl_pipeline *p, uint32_t index, mi_lte_pipeline_dev_stats *out);
int         mi_lte_dl_pipeline_run(mi_lte_dl_pipeline *p, const int8_t *h_iq, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell, uint32_t n_units,
                                   uint8_t *h_out_packed, int32_t *h_status);
int         mi_lte_dl_pipeline_run_units(mi_lte_dl_pipeline *p, const int8_t *h_iq, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                         uint32_t n_units, const mi_lte_pdsch_alloc *h_allocs, const uint32_t *h_first, uint32_t N_pdcch_symbs,
                                         uint8_t *h_out_packed, int32_t *h_status);
int         mi_lte_dl_pipeline_run_capture(mi_lte_dl_pipeline *p, const int8_t *h_capture, uint64_t n_samples, uint64_t first_subframe_start,
                                           uint32_t n_subframes, uint32_t first_subfr_num, uint32_t N_id_cell, const mi_lte_pdsch_alloc *h_allocs,
                                           const uint32_t *h_first, uint32_t N_pdcch_symbs, uint8_t *h_out_packed, int32_t *h_status);

/* ---------------------------------------------------------------- the transmit side (host code, no device work)
 * The ten transmit functions of liblte_phy that LTE_fdd_enodeb's PHY and LTE_fdd_dl_file_gen call (2: "CPU pass-through") restated on
 * the host so that a link against this library and the shim needs no object of the reference's PHY.  Bit outputs are the reference's bit for
 * bit; float outputs come from the same float operations in the same order; the transforms (the reference: FFTW3f) run in float64 rounded to
 * float.  Return values are LIBLTE_ERROR_ENUM's: 0 success, 1 invalid inputs -- also for what the reference has no defined behaviour for
 * (three ports, a pre-coder type it leaves without output, more than 10 000 coded bits per allocation: its own arrays end there).
 * shim/lifecycle_check.cc (`tx`) compares every one with the compiled reference.
 *
 * Grids are LIBLTE_PHY_SUBFRAME_STRUCT::tx_symb_re / tx_symb_im (liblte_phy.h:234-235): float [4 ports][16 symbols][1200 sub-carriers].
 *
 *   mi_lte_rate_match_turbo       liblte_phy_rate_match_turbo       liblte_phy.h:1288  liblte_phy.cc:11081-11237 (d planar, as the reference takes it)
 *   mi_lte_pdsch_channel_encode   liblte_phy_pdsch_channel_encode   liblte_phy.h:888   liblte_phy.cc:3489-3688
 *   mi_lte_bch_channel_encode     liblte_phy_bch_channel_encode     liblte_phy.h:927   liblte_phy.cc:3863-3966
 *   mi_lte_map_crs / _pss / _sss  liblte_phy_map_crs / _pss / _sss  liblte_phy.h:1034 / 1051 / 1089   liblte_phy.cc:5144 / 5265 / 5520
 *   mi_lte_create_dl_subframe     liblte_phy_create_dl_subframe     liblte_phy.h:1152  liblte_phy.cc:5862-5903
 * The handle is the scratch of LIBLTE_PHY_STRUCT that outlives a call (the PBCH's 40 ms block; what a later call can read of an earlier one). */
#define MI_LTE_TX_GRID_SC 1200u
#define MI_LTE_TX_GRID_AT(p, L, k) (((size_t)(p) * 16u + (L)) * MI_LTE_TX_GRID_SC + (k))
#define MI_LTE_TX_GRID_FLOATS (4u * 16u * MI_LTE_TX_GRID_SC)
enum { MI_LTE_MOD_BPSK = 0, MI_LTE_MOD_QPSK = 1, MI_LTE_MOD_16QAM = 2, MI_LTE_MOD_64QAM = 3 };        /* LIBLTE_PHY_MODULATION_TYPE_ENUM */
enum { MI_LTE_CHAN_DLSCH = 0, MI_LTE_CHAN_PCH = 1, MI_LTE_CHAN_ULSCH = 2, MI_LTE_CHAN_ULCCH = 3 };     /* LIBLTE_PHY_CHAN_TYPE_ENUM       */
enum { MI_LTE_PRECODER_TX_DIVERSITY = 0, MI_LTE_PRECODER_SPATIAL_MULTIPLEXING = 1 };                   /* LIBLTE_PHY_PRE_CODER_TYPE_ENUM  */
/* LIBLTE_PHY_ALLOCATION_STRUCT (liblte_phy.h:684-702) as the transmit functions read it */
typedef struct {
    const uint8_t *msg[2];      /* transport-block bits of codeword 0 / 1, one per byte                 */
    uint32_t       msg_bits[2]; /* how many of them are given; the block is zero-padded to tbs          */
    uint32_t       pre_coder_type, mod_type, chan_type, tbs, rv_idx, N_prb;
    uint32_t       prb[2][110]; /* per slot                                                             */
    uint32_t       N_codewords, N_layers, tx_mode, rnti;
    uint32_t       mcs, tpc, ndi, dl_alloc; /* what the DCI of the allocation carries (PDCCH encode)    */
} mi_lte_tx_alloc;
typedef struct mi_lte_tx mi_lte_tx;
int  mi_lte_tx_create(mi_lte_tx **out);
void mi_lte_tx_destroy(mi_lte_tx *tx);
void mi_lte_rate_match_turbo(const uint8_t *d_bits, uint32_t N_d_bits, uint32_t N_codeblocks, uint32_t tx_mode, uint32_t N_soft, uint32_t M_dl_harq,
                             uint32_t chan_type, uint32_t rv_idx, uint32_t N_e_bits, uint8_t *e_bits);
int  mi_lte_pdsch_channel_encode(mi_lte_tx *tx, uint32_t N_rb_dl, uint32_t N_sc_rb_dl, const mi_lte_tx_alloc *allocs, uint32_t N_alloc, uint32_t N_pdcch_symbs,
                                 uint32_t N_id_cell, uint32_t N_ant, uint32_t subfr_num, float *tx_re, float *tx_im);
int  mi_lte_bch_channel_encode(mi_lte_tx *tx, uint32_t N_rb_dl, uint32_t N_sc_rb_dl, const uint8_t *in_bits, uint32_t N_in_bits, uint32_t N_id_cell, uint32_t N_ant,
                               uint32_t sfn, float *tx_re, float *tx_im);
int  mi_lte_map_crs(uint32_t N_rb_dl, uint32_t N_sc_rb_dl, uint32_t subfr_num, uint32_t N_id_cell, uint32_t N_ant, float *tx_re, float *tx_im);
int  mi_lte_map_pss(uint32_t N_rb_dl, uint32_t N_sc_rb_dl, uint32_t N_id_2, uint32_t N_ant, float *tx_re, float *tx_im);
int  mi_lte_map_sss(uint32_t N_rb_dl, uint32_t N_sc_rb_dl, uint32_t subfr_num, uint32_t N_id_1, uint32_t N_id_2, uint32_t N_ant, float *tx_re, float *tx_im);
/* the control region (tx_ctrl.cc): liblte_phy_pdcch_channel_encode (liblte_phy.h:988, liblte_phy.cc:4113-4517) -- PCFICH, PHICH and one DCI per
 * allocation (format 1A for downlink, format 0 for uplink grants) at aggregation level 4 in the common search space.  mi_lte_pcfich / mi_lte_phich
 * have the layout of LIBLTE_PHY_PCFICH_STRUCT / LIBLTE_PHY_PHICH_STRUCT (liblte_phy.h:972-986); like the reference the call writes the REG
 * positions into them, the region's size into *N_pdcch_symbs and each downlink allocation's transport block size into allocs[].tbs. */
typedef struct { float n[4]; uint32_t k[4]; uint32_t cfi; uint32_t N_reg; } mi_lte_pcfich;
typedef struct { float z_re[3], z_im[3]; uint32_t k[75]; uint32_t N_reg; uint8_t b[25][8]; uint8_t present[25][8]; } mi_lte_phich;
int mi_lte_pdcch_channel_encode(mi_lte_tx *tx, uint32_t N_rb_dl, uint32_t N_rb_ul, uint32_t N_sc_rb_dl, uint32_t N_group_phich, uint32_t N_sf_phich,
                                mi_lte_pcfich *pcfich, mi_lte_phich *phich, mi_lte_tx_alloc *allocs, uint32_t N_alloc, uint32_t *N_pdcch_symbs, uint32_t N_id_cell,
                                uint32_t N_ant, uint32_t phich_dur, uint32_t subfr_num, float *tx_re, float *tx_im);
/* the uplink pair (tx_ul.cc): liblte_phy_pusch_channel_encode (liblte_phy.h:704, liblte_phy.cc:2664-2799; one port, one layer, one codeword, an N_prb the
 * reference has a transform-precoder plan for) and liblte_phy_generate_prach (liblte_phy.h:845, liblte_phy.cc:3219-3297; T_cp + T_seq samples).  ul /
 * ul_cell are what liblte_phy_ul_init was given (the reference signal of symbols 3 and 10 comes from mi_lte_ul_dmrs_pusch). */
typedef struct mi_lte_tx_ul mi_lte_tx_ul;
int    mi_lte_tx_ul_create(mi_lte_tx_ul **out);
void   mi_lte_tx_ul_destroy(mi_lte_tx_ul *tx);
int    mi_lte_pusch_channel_encode(mi_lte_tx_ul *tx, const mi_lte_ul_cfg *ul, uint32_t ul_cell, uint32_t N_rb_ul, uint32_t N_sc_rb_ul, const mi_lte_tx_alloc *alloc,
                                   uint32_t N_id_cell, uint32_t N_ant, uint32_t subfr_num, float *tx_re, float *tx_im);
size_t mi_lte_generate_prach_len(uint32_t fft_size, uint32_t preamble_format);
int    mi_lte_generate_prach(const mi_lte_prach_cfg *prach, uint32_t fft_size, uint32_t N_rb_ul, uint32_t N_sc_rb_ul, uint32_t preamble_idx, uint32_t freq_offset,
                             float *samps_re, float *samps_im);
int  mi_lte_create_dl_subframe(uint32_t N_samps_per_symb, uint32_t N_used_sc, uint32_t N_samps_cp_l_0, uint32_t N_samps_cp_l_else, const float *tx_re,
                               const float *tx_im, uint32_t ant, float *i_samps, float *q_samps);

/* ---------------------------------------------------------------- input synthesis (host side)
 * A minimal LTE downlink transmitter for benchmark / test captures, the role LTE_fdd_dl_file_gen
 * plays for the reference (LTE_fdd_dl_file_gen/src/LTE_fdd_dl_fg_samp_buf.cc:269-668).  Host code
 * only; these functions never touch the GPU and nothing the library decodes runs on the CPU. */
int mi_lte_synth_turbo_soft_i8(uint32_t K, uint32_t n, double flip, int amp, uint64_t seed, int ref_wrap,
                               int8_t *h_soft, uint8_t *h_tx_bits);
int mi_lte_synth_turbo_soft_f32(uint32_t K, uint32_t n, double sigma, uint64_t seed, int ref_wrap, float *h_soft,
                                uint8_t *h_tx_bits);

typedef struct {
    double   gain_min, gain_max; /* |h| drawn uniformly per unit                                  */
    double   max_delay;          /* integer timing offset drawn from 0..max_delay samples; < 0: a STATIC channel (no random phase, no
                                    delay, one int8 scale for all units): consecutive units laid end to end are one capture */
    double   snr_db;             /* AWGN relative to the mean signal power; >= 200 disables noise   */
    double   peak;               /* int8 full-scale target for the signal peak (e.g. 100)           */
    uint64_t seed;
} mi_lte_synth_channel;

/* n_units single-port (N_ant = 1) subframes, each with its own cell id / subframe number and
 * n_alloc PDSCH allocations (allocs[u*n_alloc + a], .unit ignored), CFI = N_pdcch_symbs, random
 * transport blocks.  Writes unit_len = 30720*s + 4400*s (s = fft_size/2048, rounded up to a
 * multiple of 16) complex int8 samples per unit to h_iq, and the transport-block bits (one per byte,
 * tbs_stride bytes per allocation) to h_tx_bits. */
size_t mi_lte_synth_unit_len(uint32_t fft_size);
int    mi_lte_synth_dl_units_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num,
                                const uint32_t *h_n_id_cell, uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs,
                                uint32_t n_alloc, const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits,
                                uint32_t tbs_stride);

/* DL-SCH transmit side of the 3GPP transport-block mode (36.212 5.1.1-5.1.4.1, the layout of mi_lte_dlsch_layout): CRC24A, segmentation,
 * CRC24B per block when C > 1, turbo encoding with the exact QPP interleaver, limited-buffer rate matching (N_cb of the layout) and
 * concatenation of the blocks' E_r bits.  bits: tbs payload bits, one per byte; e_out: G bits, one per byte. */
int mi_lte_dlsch_encode_3gpp(uint32_t tbs, const uint8_t *bits, uint32_t G, uint32_t Q_m, uint32_t tx_mode, uint32_t rv,
                             const mi_lte_dlsch_cfg *dlsch, uint8_t *e_out);
/* mi_lte_synth_dl_units_i8 with that encoder and every resource element of an allocation used (E = G): the input of the 3GPP plans.
 * Same arguments plus the soft-buffer configuration; any tbs mi_lte_dlsch_layout accepts. */
int mi_lte_synth_dl_units_3gpp_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                  uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc, const mi_lte_dlsch_cfg *dlsch,
                                  const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride);
/* mi_lte_synth_dl_units_3gpp_i8 with the caller's transport blocks: h_payload[(u * n_alloc + a) * tbs_stride + i], i < tbs, one bit per
 * byte.  The random numbers the payload would have taken are still drawn and discarded, so given the bits mi_lte_synth_dl_units_3gpp_i8
 * drew with the same seed, it writes the same IQ byte for byte; a HARQ retransmission is the same payload with another rv and another seed. */
int mi_lte_synth_dl_units_3gpp_payload_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                          uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                          const mi_lte_dlsch_cfg *dlsch, const mi_lte_synth_channel *chan, const uint8_t *h_payload,
                                          uint32_t tbs_stride, int8_t *h_iq);
/* The transmit side of the transmit-diversity plans ("PDSCH, 3GPP mode: transmit diversity" above).
 * mi_lte_dlsch_encode_3gpp_nl: mi_lte_dlsch_encode_3gpp over mi_lte_dlsch_layout_nl's E_r (N_L = 1: the same bits).
 * mi_lte_txdiv_precode: the layer mapper and pre-coder of 36.211 6.3.3.3 / 6.3.4.3 in one step, host arithmetic.  d: M_symb modulation
 *   symbols (M_symb a multiple of N_ant, N_ant 2 or 4; anything else MI_LTE_ERR_INVALID_ARG); y[p * M_symb + n]: what port p sends in
 *   place n.  Two ports, pair (d(2i), d(2i+1)) = (x0, x1): port 0 sends x0, x1 and port 1 sends -conj(x1), conj(x0), all over sqrt 2.  Four
 *   ports: places 4i, 4i+1 carry (d(4i), d(4i+1)) in that form on ports (0, 2), places 4i+2, 4i+3 carry (d(4i+2), d(4i+3)) on ports (1, 3);
 *   the other two ports send 0 there.
 * mi_lte_synth_dl_units_3gpp_txdiv_i8: mi_lte_synth_dl_units_3gpp_i8 for cfg->N_ant = 2 or 4.  CRS for every port (36.211 6.10.1); each
 *   allocation's resource elements in the same mapping order with the 2 / 4-port CRS exclusions, from the allocation's own n_pdcch_symbs when
 *   it has one; mi_lte_dlsch_encode_3gpp_nl with N_L = 2, scrambling, modulation, mi_lte_txdiv_precode; one OFDM signal per port.  Channel,
 *   per unit: one integer delay common to all ports (co-located antennas; a delay per port would put a phase step between the two elements
 *   of a pair, which at FFT 128 already breaks 64QAM without noise), then per port, in port order, a gain from gain_min..gain_max and a
 *   phase (max_delay < 0: no delay and no phase).  The ports are summed; AWGN at snr_db relative to the power of that sum; int8 with the
 *   sum's peak at `peak`, per unit.  h_payload (may be NULL): the caller's transport blocks as in mi_lte_synth_dl_units_3gpp_payload_i8, the
 *   random ones' draws still made; h_tx_bits (may be NULL): the blocks sent.  MI_LTE_ERR_INVALID_ARG: N_ant = 1 (use the calls above), an
 *   allocation with tx_mode != 2, BPSK, or a tbs mi_lte_dlsch_layout_nl refuses.  The generators above and their byte streams are untouched. */
int mi_lte_dlsch_encode_3gpp_nl(uint32_t tbs, const uint8_t *bits, uint32_t G, uint32_t Q_m, uint32_t N_L, uint32_t tx_mode, uint32_t rv,
                                const mi_lte_dlsch_cfg *dlsch, uint8_t *e_out);
int mi_lte_txdiv_precode(uint32_t N_ant, const float *d_re, const float *d_im, uint32_t M_symb, float *y_re, float *y_im);
int mi_lte_synth_dl_units_3gpp_txdiv_i8(const mi_lte_dl_cfg *cfg, uint32_t n_units, const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell,
                                        uint32_t N_pdcch_symbs, const mi_lte_pdsch_alloc *h_allocs, uint32_t n_alloc,
                                        const mi_lte_dlsch_cfg *dlsch, const mi_lte_synth_channel *chan, const uint8_t *h_payload /* may be NULL */,
                                        uint32_t tbs_stride, int8_t *h_iq, uint8_t *h_tx_bits /* may be NULL */);

/* control regions: PCFICH + n_dci format-1A DCIs (rnti = 0: slot unused) at aggregation level 4 in candidates 0..n_dci-1,
 * standard transmit diversity on cfg->N_ant ports, through a smooth random channel per port (gain_min..gain_max) and
 * AWGN (snr_db), written directly as device-subframe grids (mi_lte_subframe_floats(N_ant) floats per unit, symbols 0-3
 * filled) with noisy channel estimates.  Input of mi_lte_pdcch_decode_run for the benchmark and the tests. */
typedef struct {
    uint32_t rnti, mcs, N_prb, rb_start, rv_idx;
} mi_lte_synth_dci;
int mi_lte_synth_ctrl_grids(const mi_lte_dl_cfg *cfg, float phich_res, uint32_t n_units, const uint32_t *h_subfr_num,
                            const uint32_t *h_n_id_cell, const uint32_t *h_cfi, const mi_lte_synth_dci *h_dci, uint32_t n_dci,
                            const mi_lte_synth_channel *chan, float *h_grids);

/* mi_lte_synth_ctrl_grids with any DCI anywhere: per unit n_rec (at most MI_LTE_SYNTH_MAX_REC) records, rnti = 0 marks an unused slot;
 * n_bits (1 .. 64) payload bits, first bit in bit n_bits - 1, on the L (1, 2, 4, 8) CCEs from cce (a multiple of L).  The processing is the
 * one function the two generators share: CRC16 masked with the RNTI, the tail-biting encoder, rate matching to 72 L bits, scrambling at
 * bit 72 cce, transmit diversity onto that CCE range -- a format-1A DCI given as an L = 4 record at CCE 4 a yields mi_lte_synth_ctrl_grids'
 * grid for the same seed byte for byte.  MI_LTE_ERR_INVALID_ARG: records that overlap, a record reaching past the unit's N_cce. */
#define MI_LTE_SYNTH_MAX_REC 8
typedef struct {
    uint32_t rnti, L, cce, n_bits;
    uint64_t payload;
} mi_lte_synth_dci_rec;
int mi_lte_synth_ctrl_grids_dci(const mi_lte_dl_cfg *cfg, float phich_res, uint32_t n_units, const uint32_t *h_subfr_num,
                                const uint32_t *h_n_id_cell, const uint32_t *h_cfi, const mi_lte_synth_dci_rec *h_rec, uint32_t n_rec,
                                const mi_lte_synth_channel *chan, float *h_grids);

/* n_units uplink subframes for tests / benchmarks: every unit carries n_alloc PUSCH transmissions
 * (allocs[u*n_alloc + a], .unit ignored) with random transport blocks, through one flat channel per unit.
 * The transmit chain is the inverse of the reference's RECEIVER (36.212 5.2.2 / 36.211 5.3-5.6); the
 * reference's own uplink transmit helpers are not usable as a model (its channel interleaver and SC-FDMA
 * modulator index wrongly, liblte_phy.cc:12023-12042, :8565-8570 -- the eNodeB never transmits uplink).
 * The transform precoder scales by 1/sqrt(12*N_prb) as a real UE does; the reference's receiver then sees
 * 12*N_prb times the constellation point (its transform pre-decoding scaling, liblte_phy.cc:6644-6657), so QPSK
 * decodes with every soft bit at +-1 while 16/64QAM fails -- in the reference and, identically, here.
 * Writes mi_lte_synth_ul_unit_len(fft_size) complex int8 samples per unit. */
size_t mi_lte_synth_ul_unit_len(uint32_t fft_size);
int    mi_lte_synth_ul_units_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units,
                                const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs,
                                uint32_t n_alloc, const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits,
                                uint32_t tbs_stride);
/* UL-SCH transmit side of the PUSCH 3GPP mode (36.212 5.2.2.1-5.2.2.5, the layout of mi_lte_ulsch_layout): CRC24A, segmentation, CRC24B per
 * block when C > 1, turbo encoding with the exact QPP interleaver, rate matching with N_cb = K_w, concatenation of the blocks' E_r bits.
 * bits: tbs payload bits, one per byte; e_out: G bits, one per byte (before the channel interleaver). */
int    mi_lte_ulsch_encode_3gpp(uint32_t tbs, const uint8_t *bits, uint32_t G, uint32_t Q_m, uint32_t rv, uint8_t *e_out);
/* mi_lte_synth_ul_units_i8 with that encoder: the input of the PUSCH 3GPP plans.  Same arguments; any tbs mi_lte_ulsch_layout accepts, no
 * BPSK.  A single-block transport block whose interleaver the reference evaluates without overflow gives mi_lte_synth_ul_units_i8's bytes. */
int    mi_lte_synth_ul_units_3gpp_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units,
                                     const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs,
                                     uint32_t n_alloc, const mi_lte_synth_channel *chan, int8_t *h_iq, uint8_t *h_tx_bits,
                                     uint32_t tbs_stride);
/* The UE's multiplexer and scrambler for one allocation (36.212 5.2.2.7-5.2.2.8, 36.211 5.3.1; the rules at mi_lte_ulsch_uci above):
 * f: the G = mi_lte_ulsch_uci_G coded data bits, h_ack / h_ri: O_ack / O_ri information bits, h_cqi: Q_cqi coded bits, one per byte
 * (NULL where there are none).  h_mux: the 12 * 12 N_prb * Q_m interleaved values in transmit order before scrambling, 0 / 1 or the
 * placeholders 2 = x, 3 = y; h_scr (optional): the bits after scrambling with the Gold sequence of c_init. */
int    mi_lte_ulsch_mux_3gpp(uint32_t N_prb, uint32_t Q_m, const mi_lte_ulsch_uci *uci, const uint8_t *f, const uint8_t *h_ack,
                             const uint8_t *h_ri, const uint8_t *h_cqi, uint32_t c_init, uint8_t *h_mux, uint8_t *h_scr);
/* mi_lte_synth_ul_units_3gpp_i8 with control information: per allocation (unit-major, as h_allocs) its descriptor h_uci, 2 bytes of
 * h_ack and of h_ri (the first O_* are sent) and h_cqi_stride bytes of h_cqi (the first Q_cqi are sent; NULL when no allocation has
 * CQI).  The control values are the caller's and none is drawn from the generator's random numbers: with all-zero descriptors the
 * output is mi_lte_synth_ul_units_3gpp_i8's byte for byte. */
int    mi_lte_synth_ul_units_3gpp_uci_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units,
                                         const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs,
                                         uint32_t n_alloc, const mi_lte_synth_channel *chan, const mi_lte_ulsch_uci *h_uci,
                                         const uint8_t *h_ack, const uint8_t *h_ri, const uint8_t *h_cqi, uint32_t h_cqi_stride,
                                         int8_t *h_iq, uint8_t *h_tx_bits, uint32_t tbs_stride);
/* mi_lte_synth_ul_units_3gpp_i8 (h_uci = NULL) or mi_lte_synth_ul_units_3gpp_uci_i8 (h_uci and its companions as there) with the caller's
 * transport blocks: h_payload[(u * n_alloc + a) * tbs_stride + i], i < tbs, one bit per byte.  The random numbers the payload would have
 * taken are still drawn and discarded, so given the bits the plain generator drew with the same seed, it writes the same IQ byte for byte;
 * a HARQ retransmission is the same payload with another rv and another seed.  Refuses what its sibling refuses, and a NULL h_payload. */
int    mi_lte_synth_ul_units_3gpp_payload_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units,
                                             const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs,
                                             uint32_t n_alloc, const mi_lte_synth_channel *chan, const mi_lte_ulsch_uci *h_uci,
                                             const uint8_t *h_ack, const uint8_t *h_ri, const uint8_t *h_cqi, uint32_t h_cqi_stride,
                                             const uint8_t *h_payload, uint32_t tbs_stride, int8_t *h_iq);
/* mi_lte_synth_ul_units_3gpp_payload_i8 (h_uci and its companions optional, as there) through a channel of several paths with integer
 * delays.  Per unit the draws of gain, phase and delay are the existing ones in the existing order; after them one further phase phi_p is
 * drawn per path p >= 1 (phi_0 is the existing phase).  The channel output is gain * sum_p a_p exp(i phi_p) t[i - dly - delay[p]], a_p the
 * amplitudes normalised to sum a_p^2 = 1; AWGN is added as before, and the int8 scale is additionally divided by sum_p a_p so that nothing
 * clips at chan->peak.  One path therefore writes mi_lte_synth_ul_units_3gpp_payload_i8's bytes, byte for byte.  MI_LTE_ERR_INVALID_ARG for a
 * NULL paths, n_paths outside 1 .. 4, delay[0] != 0, an amplitude that is negative or not finite, sum amp^2 = 0. */
typedef struct {
    uint32_t n_paths;  /* 1 .. 4 */
    uint32_t delay[4]; /* delay[0] = 0; delay[p] extra integer samples of path p */
    double   amp[4];   /* relative amplitudes, normalised inside to sum amp^2 = 1 */
} mi_lte_synth_paths;
int    mi_lte_synth_ul_units_3gpp_paths_i8(const mi_lte_dl_cfg *cfg, const mi_lte_ul_cfg *ul, uint32_t n_units,
                                           const uint32_t *h_subfr_num, const uint32_t *h_n_id_cell, const mi_lte_pdsch_alloc *h_allocs,
                                           uint32_t n_alloc, const mi_lte_synth_channel *chan, const mi_lte_ulsch_uci *h_uci,
                                           const uint8_t *h_ack, const uint8_t *h_ri, const uint8_t *h_cqi, uint32_t h_cqi_stride,
                                           const uint8_t *h_payload, uint32_t tbs_stride, const mi_lte_synth_paths *paths, int8_t *h_iq);

/* n_occ PRACH occasions (format 0-3 preambles per 36.211 5.7.2-5.7.3): preamble h_preamble_idx[o] of the cell's 64,
 * delayed by h_delay[o] samples, through a flat channel + AWGN; mi_lte_synth_prach_len() complex int8 samples each. */
size_t mi_lte_synth_prach_len(uint32_t fft_size, uint32_t preamble_format);
int    mi_lte_synth_prach_i8(const mi_lte_dl_cfg *cfg, const mi_lte_prach_cfg *prach, uint32_t n_occ, const uint32_t *h_preamble_idx,
                             const uint32_t *h_delay, const mi_lte_synth_channel *chan, int8_t *h_iq);

#ifdef __cplusplus
}
#endif
#endif
