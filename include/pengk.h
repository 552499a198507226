/* pengk.h -- C ABI of the MI355X (gfx950) hot path of PEnG-motif.
 *
 * The reference (soedinglab/PEnG-motif) has no FFI: its hot path sits behind three C++ classes.
 * This header is the thin extern "C" layer the host-side mirrors of those classes
 * (peng-motif_amd/host/) call; every entry point names the reference function it replaces
 * (file:line relative to the reference tree).  Plain pointers and sizes only; no HIP, torch or
 * C++ types cross the boundary.  All functions return PENGK_OK (0) or a PENGK_ERR_* code and never
 * throw; pengk_last_error() describes the last failure of the calling thread.
 *
 * Pointer naming: `d_` = device memory (hipMalloc'ed by the caller, e.g. through pengk_malloc or a
 * torch tensor's data_ptr()), `h_` = host memory.  Work is enqueued on the context's stream;
 * functions taking only d_ pointers do not synchronise with the host.
 *
 * Encodings (identical to the reference):
 *   pattern id   little-endian base 4, first base = least significant digit (src/base_pattern.h:24-29)
 *   IUPAC id     little-endian base 11, letters A C G T S W R Y M K N = 0..10 (src/iupac_pattern.h:26-29)
 *   BaMM id      big-endian (k+1)-mer id (src/shared/Sequence.cpp:21-33)
 *   V layout     V[0] (4) | V[1] (16) | V[2] (64) floats, 84 in all; bg counts likewise
 *
 * Packed sequence layout in HBM:
 *   words   2 bits per base (A,C,G,T = 0..3), base g in bits [2(g%32), 2(g%32)+2) of 64-bit word g/32;
 *           only the bases of "visited runs" (scan rule of src/base_pattern.cpp:347-381) are stored,
 *           back to back; PENGK_FRONT_PAD_BASES zero bases in front, >= 64 behind.
 *   items   one 64-bit record per scan item: bits 0..39 stream offset of the first window's first
 *           base, bits 40..55 number of windows (1..65535), bit 56 = item continues the previous
 *           item's run (its predecessor windows are stored immediately in front).
 */
#ifndef PENGK_H_
#define PENGK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library itself is built with -fvisibility=hidden */
#endif

#define PENGK_VERSION 100

#define PENGK_OK 0
#define PENGK_ERR_ARG 1         /* bad argument (NULL, odd/unsupported W, order > 2, ...) */
#define PENGK_ERR_DEVICE 2      /* no usable gfx950 device / HIP runtime error */
#define PENGK_ERR_RANGE 3       /* a 32-bit count bin could overflow on this shard */
#define PENGK_ERR_UNSUPPORTED 4 /* operation not defined for this input (see function) */
#define PENGK_ERR_NOMEM 5

#define PENGK_MIN_W 2 /* the reference accepts every even pattern length (src/Global.cpp:103-106) */
#define PENGK_MAX_W 14
#define PENGK_FRONT_PAD_BASES 64
#define PENGK_DEFAULT_ITEM_WINDOWS 256
#define PENGK_MIN_ITEM_WINDOWS 64

typedef struct pengk_ctx pengk_ctx;

/* ---- lifecycle, errors, device memory ------------------------------------------------------- */
int pengk_version(void);
const char* pengk_last_error(void);
const char* pengk_error_name(int code);

/* Binds a context to HIP device `device` and creates its stream.  Fails with PENGK_ERR_DEVICE when
 * no GPU is present -- there is no CPU fallback in this library. */
int pengk_create(int device, pengk_ctx** out);
int pengk_destroy(pengk_ctx* ctx);
int pengk_synchronize(pengk_ctx* ctx);
/* hipStream_t of the context (for callers that record their own events). */
void* pengk_stream(pengk_ctx* ctx);
/* Re-target the context to an externally owned hipStream_t (e.g. torch's current stream). */
int pengk_set_stream(pengk_ctx* ctx, void* hip_stream);

/* Tunables / introspection.  Options: "count_impl" 0 = auto, 1 = direct global atomics, 2 = partitioned LDS
 * histograms (W = 8 .. 14); "count_group" keys per group of the partitioned scan's emitter: 0 = auto (128 -- sixteen
 * buckets of 16-bit keys -- at W = 10 on both strands, 64 everywhere else), 64 = the emitter of 64 everywhere, 128 = as
 * auto where it applies; a count that cannot run it (one strand, another W, the direct emitter) fails with
 * PENGK_ERR_UNSUPPORTED (same bits either way: for A/B timing in one process and for the tests); "n_windows_hint" = total windows of the attached items (sizes the key buffer
 * tightly; set it after pengk_set_sequences); "key_cap_override" (test hook) entries per bucket region of the
 * partitioned count, 0 = automatic; "sweep_pairs" 1 (default) / 0: both strands from W = 12 on, a pattern and its reverse complement evaluated once (0: one thread per pattern; same bits); "iupac_group_bytes" (test hook) scratch budget for one group of large
 * patterns in pengk_iupac_aggregate, 0 = 1 GiB; "em_fast" 2 (default) / 1 / 0, see pengk_em; "sites_record_budget" records per slice of pengk_sites_slices
 * (default 2^24, also readable through pengk_get_info); "enrich_groups_per_launch" (test hook) motif groups per launch of
 * pengk_motif_enrich, 1 .. 65535 (default 1024, also readable through pengk_get_info).  Info: "deferred_items" (of the last pengk_count;
 * synchronises), "count_group" (the option as set), "count_group_used" (keys per group of the emitter the last count ran:
 * 64 or 128; 0 = not the one-level partition of W = 8 / 10), "count_wrapped_workgroups" (pass-B workgroups of the last
 * count whose packed 16-bit bins wrapped and that recounted their slices exactly; 0 under groups of 64; synchronises; like
 * "deferred_items" it reads the count's scratch and is valid until the next pengk_count / pengk_count_bg on the context),
 * test hooks of the same lifetime: "count_slices" (number of (wave, bucket) key slices of the last one-level count) and
 * "count_slice_fill" (entries pass A published for the slice chosen with the option "count_probe_slice" = wave * buckets
 * + bucket; synchronises), "num_cu"; of the last pengk_em / pengk_em_device call in the serial mode with its blocks evaluated ahead
 * (synchronise): "em_fetched_blocks" (blocks a chain added term by term), "em_mispredicted_blocks" (of those: blocks
 * whose estimated binade did not hold), "em_restaged_blocks" / "em_restaged_waits" (csrc/seqsum.h, WalkCounts). */
int pengk_set_option(pengk_ctx* ctx, const char* name, int64_t value);
int pengk_get_info(pengk_ctx* ctx, const char* name, int64_t* value_out);

int pengk_malloc(pengk_ctx* ctx, size_t bytes, void** d_out);
int pengk_free(pengk_ctx* ctx, void* d_ptr);
int pengk_memcpy_h2d(pengk_ctx* ctx, void* d_dst, const void* h_src, size_t bytes); /* synchronous */
int pengk_memcpy_d2h(pengk_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* synchronous */
/* (No counterpart in the reference, whose process has no device runtime to start.)
 * Pays the process's first-use costs ahead of time (first device-to-host copy: 10-17 ms whatever its size; the code
 * objects of the sweep / IUPAC / EM / similarity kernels).  Optional; call once after pengk_create, from any thread,
 * beside other work. */
int pengk_warmup(pengk_ctx* ctx);
int pengk_memset(pengk_ctx* ctx, void* d_dst, int byte, size_t bytes);              /* async */
/* Page-locked host memory for result tables: the reference's BasePattern hands out raw host arrays
 * (src/base_pattern.h:129-140: size_t counts, float probabilities / expected / z / log-p, 4^W each); mirrors of
 * the device tables land in them at link speed when they are allocated here.  Ordinary host pointers otherwise. */
int pengk_host_alloc(pengk_ctx* ctx, size_t bytes, void** h_out);
int pengk_host_free(pengk_ctx* ctx, void* h_ptr);

/* Stream-ordered event timing without exposing HIP types: records an event on the context's stream;
 * pengk_timer_elapsed_ms synchronises on `stop`. */
int pengk_timer_create(pengk_ctx* ctx, void** timer_out);
int pengk_timer_record(pengk_ctx* ctx, void* timer);
int pengk_timer_elapsed_ms(pengk_ctx* ctx, void* start, void* stop, float* ms_out);
int pengk_timer_destroy(pengk_ctx* ctx, void* timer);

/* ---- host packer (pure CPU; replaces the per-sequence byte codes + revcomp copies that
 *      count_patterns walks, src/base_pattern.cpp:339-342, src/shared/Sequence.cpp:4-35) -------- */
typedef struct pengk_packed {
  uint64_t* words;       /* 2-bit stream incl. padding */
  uint64_t n_words;
  uint64_t* items;       /* scan items */
  uint64_t n_items;
  uint64_t n_bases;      /* stored bases (without padding) */
  uint64_t n_windows;    /* = ltot: number of visited windows (src/base_pattern.cpp:367) */
  uint64_t max_bin_bound;/* upper bound on any single count bin: sum over runs of ceil(windows/W) */
  int64_t bg_counts[84]; /* (k+1)-mer counts, k = 0..2, exactly as BackgroundModel counts them incl. the
                            invalid-base rule (src/shared/BackgroundModel.cpp:60-84) */
  uint64_t n_sequences;
  uint64_t max_len;      /* longest input sequence */
  int W;
  int item_windows;
  int all_whole;         /* 1 iff every input sequence is exactly one stored run (no invalid base, L >= W):
                            then pengk_bg_count can recount bg_counts on the device */
} pengk_packed;

/* codes: the reference's byte codes (0 = other, A,C,G,T = 1..4) of all sequences back to back;
 * offs: n_seq+1 offsets into codes.  item_windows: maximum windows per scan item
 * (>= PENGK_MIN_ITEM_WINDOWS, <= 65535; 0 = PENGK_DEFAULT_ITEM_WINDOWS).
 * out->words / out->items are owned by the library (zero-filled blocks on transparent huge pages where the kernel
 * grants them): release them with pengk_packed_free, never with free(). */
int pengk_pack(const uint8_t* h_codes, const int64_t* h_offs, int64_t n_seq, int W, int item_windows,
               pengk_packed* out);
/* The same with a given number of host threads (0 = automatic, as pengk_pack): a caller that packs many chunks of an
 * input from its own worker threads -- the CLI does, while the FASTA file is still being read -- asks for 1. */
int pengk_pack_threads(const uint8_t* h_codes, const int64_t* h_offs, int64_t n_seq, int W, int item_windows, int threads,
                       pengk_packed* out);
void pengk_packed_free(pengk_packed* p);

/* Packing an input chunk by chunk into ONE pair of caller-owned host buffers (zero-filled; e.g. fresh anonymous
 * memory), from any number of threads at once: every call reserves its place with the two cursors (atomically), writes
 * its words -- own zero padding in front and behind, like pengk_pack -- and its items with ABSOLUTE stream offsets, so
 * that words[0 .. word_cursor) / items[0 .. item_cursor) are attached to the device as they stand, with ONE
 * pengk_set_sequences: max_bin_bound = the sum over the chunks, all_whole = the AND.  Counts are additive over
 * sequences, so the order in which chunks land does not matter.  `out` receives the chunk's figures (windows, bounds,
 * background counters ...); out->words / out->items point INTO the buffers and are not to be released.
 * The CLI packs every chunk of the FASTA file this way while the rest is still being read (host/device.cpp).
 * Capacity: words >= sum over chunks of (64 + bases + 31) / 32 + 4, items >= their number; PENGK_ERR_RANGE otherwise. */
typedef struct pengk_pack_target {
  uint64_t* words;
  uint64_t words_cap;
  uint64_t* items;
  uint64_t items_cap;
  uint64_t word_cursor; /* next free word / item: start at 0; advanced atomically by the calls */
  uint64_t item_cursor;
} pengk_pack_target;
int pengk_pack_append(const uint8_t* h_codes, const int64_t* h_offs, int64_t n_seq, int W, int item_windows,
                      pengk_pack_target* target, pengk_packed* out);

/* ---- device-resident sequences ------------------------------------------------------------- */
/* Attach caller-owned device buffers holding a packed stream and its items (layout above).
 * `all_whole` as in pengk_packed.  The buffers must outlive every later call that scans them. */
int pengk_set_sequences(pengk_ctx* ctx, const uint64_t* d_words, uint64_t n_words, const uint64_t* d_items,
                        uint64_t n_items, int W, int item_windows, uint64_t max_bin_bound, int all_whole);

/* Size query + on-device generation of the synthetic input of SURVEY.md 8d (sequences
 * [seq0, seq0+n_seq) of length L, splitmix64 counter-based, motif GCTGAGTCAT planted in 10 %),
 * written straight into caller-owned device buffers in the packed layout, then attached as by
 * pengk_set_sequences.  Bit-identical to the CPU generator the tests use. */
int pengk_synth_sizes(uint64_t n_seq, uint32_t L, int W, int item_windows, uint64_t* n_words, uint64_t* n_items);
int pengk_synth_sequences(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, uint32_t L, int W,
                          int item_windows, uint64_t* d_words, uint64_t* d_items);

/* ---- K1: 4^W k-mer count (BasePattern::count_patterns / count_patterns_single_strand,
 *      src/base_pattern.cpp:331-441) ---------------------------------------------------------------
 * d_counts: uint32[4^W], overwritten.  both_strands: counts land on the canonical id min(id, rc)
 * only (run pengk_mirror_counts for the reference's twin copy, :387-392).  d_ltot: uint64 scalar,
 * overwritten with the number of visited windows.  The non-overlap rule (:361-366) is applied
 * exactly, with 64-bit positions.  Counts of different shards add (the rule is per sequence).
 * Emitters: W = 8 .. 14 use the partitioned LDS-histogram count (one partition level at W = 8, 10; two at W = 12; three
 * at W = 14: 2^28 bins = 2^13 LDS histograms -- the reference itself advises W <= 12, README.md:119); W = 4, 6 (tables
 * that are contended in any form) count with one device-scope atomic per window. */
int pengk_count(pengk_ctx* ctx, int both_strands, uint32_t* d_counts, uint64_t* d_ltot);
int pengk_mirror_counts(pengk_ctx* ctx, int W, uint32_t* d_counts);
/* pengk_count with K1b fused into the same scan (the rolling id's top three digits are the 3-mer ending at
 * the current base): additionally writes uint64[84] background counts as pengk_bg_count would.  Same
 * restriction as pengk_bg_count (whole-sequence runs), else PENGK_ERR_UNSUPPORTED. */
int pengk_count_bg(pengk_ctx* ctx, int both_strands, uint32_t* d_counts, uint64_t* d_ltot, uint64_t* d_bg_counts);

/* K1b: background (k+1)-mer counts k = 0..2 (BackgroundModel ctor loop,
 * src/shared/BackgroundModel.cpp:60-84) -> uint64[84].  Only for inputs whose sequences are all
 * whole runs (pengk_packed.all_whole); otherwise PENGK_ERR_UNSUPPORTED and the packer's
 * bg_counts are the source. */
int pengk_bg_count(pengk_ctx* ctx, uint64_t* d_bg_counts);

/* BackgroundModel::calculateV (src/shared/BackgroundModel.cpp:490-530), interpolated, on device:
 * uint64[84] counts -> float[84] conditional probabilities.  alpha: 3 host floats. */
int pengk_bg_model(pengk_ctx* ctx, const uint64_t* d_bg_counts, int K, const float* h_alpha, float* d_V);

/* ---- K2+K3: pattern-space sweep (calculate_bg_probabilities + aggregate_double_strand_background +
 *      calculate_expected_counts + calculate_log_pvalues + calculate_zscores,
 *      src/base_pattern.cpp:231-325) ---------------------------------------------------------------
 * d_bgprob: float[(max_k+1)][4^W] (order-major), strand-aggregated when both_strands.
 * expected/z/logp use order k <= max_k <= 2.  d_counts must already be mirrored for both strands.
 * d_ltot: the uint64 scalar pengk_count wrote (after any cross-GPU reduction). */
int pengk_pattern_stats(pengk_ctx* ctx, int W, int both_strands, int k, int max_k, const float* d_V,
                        const uint64_t* d_ltot, const uint32_t* d_counts, float* d_bgprob, float* d_expected,
                        float* d_logp, float* d_z);

/* The same sweep held to a SECOND null, a control set's own counts (this project's own; the reference has no such
 * mode: INTEGRATION.md 7l).  d_ctrl_counts: uint32[4^W], the control's k-mer counts -- pengk_count under
 * the same strand setting, mirrored as d_counts is (an un-mirrored table is legal: the value is defined per pattern,
 * each twin gets its own); d_ctrl_ltot: the control's uint64 window total Lc; pseudocount a: finite, >= 0.
 * With p_o[x] the value pengk_pattern_stats writes to bgprob[o][x], for every order o <= max_k
 *     q_o[x] = (float) fmax( (double) p_o[x], ((double) c[x] + a) / (double) Lc )        (Lc == 0: q_o[x] = p_o[x])
 * -- sum and quotient in fp64, one rounding to float32.  d_bgprob receives q_o; expected, log-p and z are made of
 * q_k[x], the INPUT's ltot and the input's counts exactly as pengk_pattern_stats makes them of p_k[x]: the expected
 * count is the larger of what the Markov model predicts and what the control shows.  One pass, every table written
 * once; every even W from 2 to 14; option sweep_pairs as for pengk_pattern_stats. */
int pengk_pattern_stats_control(pengk_ctx* ctx, int W, int both_strands, int k, int max_k, const float* d_V,
                                const uint64_t* d_ltot, const uint32_t* d_counts, const uint32_t* d_ctrl_counts,
                                const uint64_t* d_ctrl_ltot, double pseudocount, float* d_bgprob, float* d_expected,
                                float* d_logp, float* d_z);

/* ---- a GC-stratified null for the sweep (--stratified-background: on an input of mixed composition -- CpG-island
 *      promoters pooled with A+T-rich enhancers -- every G+C-rich and every A+T-rich word is over-represented against ONE
 *      Markov model; HOMER normalises for GC for the same reason) ---------------------
 * This project's own definitions, not promised to give HOMER's numbers.  Integer counters and one fp64 mixture with one
 * rounding: a numpy restatement and any sharding give the same bits.
 *
 * The background counters of every stratum of a scan layout (the layout of pengk_motif_scan; the strata of
 * pengk_seq_strata with use_length = 0, or any other labelling below n_strata).  For every sequence i with
 * d_stratum[i] = s < n_strata (any other value, 0xFFFF included, is skipped), every position p and every order k in
 * 0 .. 2 with p >= k: the (k+1)-mer ending at p is counted, d_bg[s * 84 + at_k + y] += 1, iff ALL of its k + 1 bases are
 * valid -- this project's own rule for invalid bases: an invalid base takes part in no word of any order, and the base
 * behind it starts over at order 0 (the packer's bg_counts keep the reference's treatment of such bases; on an input
 * without invalid bases the strata's counters sum to them exactly).  y: the word in BaMM order, older base more
 * significant; at_k = 0 / 4 / 20.  d_valid = NULL: every base valid.  d_windows[s] (may be NULL) += the positions p with W
 * consecutive valid bases from p on: the windows a count at pattern length W can see, the stratum's weight in
 * pengk_pattern_stats_strata.  d_bg (n_strata x 84 uint64) and d_windows (n_strata uint64) are ADDED to (caller-zeroed):
 * shards and several calls sum exactly.  n_seq = 0 does nothing.  PENGK_ERR_ARG: n_strata outside 1 .. 16, W not an even
 * number in PENGK_MIN_W .. PENGK_MAX_W, n_seq >= 2^32, a null pointer (but d_valid and d_windows) with n_seq > 0.
 * Asynchronous on the context's stream. */
int pengk_strata_bg_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid /* NULL: all valid */,
                          const int64_t* d_offs, const uint32_t* d_lens, uint64_t n_seq, const uint16_t* d_stratum,
                          int n_strata /* 1..16 */, int W, uint64_t* d_bg /* n_strata x 84, ADDED to */,
                          uint64_t* d_windows /* n_strata, ADDED to; may be NULL */);
/* The sweep under the mixture of the strata's models.  d_V: float[n_strata][84], a V table (pengk_bg_model) per stratum;
 * h_windows: n_strata HOST uint64 weights w_s (read before the call returns).  With p_{s,o}[x] the strand-aggregated
 * float32 probability that pengk_pattern_stats would write to bgprob[o][x] for the table V_s, for every order o <= max_k
 *     m_o[x] = (float)( (sum over s of (double) w_s * (double) p_{s,o}[x]) / (double)(sum over s of w_s) )
 * -- the sum in fp64 in ascending s over the strata with w_s > 0, product and addition rounded separately, the weights'
 * sum in uint64, ONE division and ONE rounding to float32.  One non-zero weight gives pengk_pattern_stats' bits for that
 * stratum's table.  With a control (d_ctrl_counts, d_ctrl_ltot, pseudocount as pengk_pattern_stats_control takes them;
 * NULL, NULL, 0: none) q_o[x] = (float) fmax((double) m_o[x], share[x]) with that entry's share.  d_bgprob receives m_o
 * (q_o); expected, log-p and z are made of m_k (q_k), d_ltot and d_counts exactly as pengk_pattern_stats makes them of
 * p_k.  Every even W from 2 to 14; the result does not depend on the option sweep_pairs.  PENGK_ERR_ARG: a NULL argument
 * (but the control's), n_strata outside 1 .. 16, every weight zero or their sum beyond 2^64, one control pointer without
 * the other, a pseudocount that is not finite and >= 0, or not 0 without a control.  Asynchronous on the context's
 * stream: no host wait. */
int pengk_pattern_stats_strata(pengk_ctx* ctx, int W, int both_strands, int k, int max_k, const float* d_V /* n_strata x 84 */,
                               int n_strata, const uint64_t* h_windows /* n_strata */, const uint64_t* d_ltot,
                               const uint32_t* d_counts, const uint32_t* d_ctrl_counts, const uint64_t* d_ctrl_ltot,
                               double pseudocount /* control: NULL, NULL, 0 = none */, float* d_bgprob, float* d_expected,
                               float* d_logp, float* d_z);

/* ---- a Markov null of order 3 .. 5 for the sweep (--high-order-background: genomic sequence has structure beyond
 *      trinucleotides, and an order-2 model under-predicts every word built of common 4-6-mers by an excess that grows with
 *      the square root of the input; MEME-suite users pass an order 3-5 model from fasta-get-markov -m; INTEGRATION.md 7u,
 *      DESIGN.md 29) ---------------------------------------------------------------------------------------------------
 * This project's own definitions (the reference's model stops at order 2).  Integer counters, float32 in a stated order: a
 * numpy restatement and any sharding give the same bits.  The tables of orders 0 .. K lie back to back, order k at
 * at_k = (4^(k+1) - 4) / 3 = 0, 4, 20, 84, 340, 1364; K = 5 has (4^(K+2) - 4) / 3 = 5460 entries.
 *
 * The counters of a scan layout (the layout of pengk_motif_scan).  For every sequence, every position p and every order k in
 * 0 .. K with p >= k: the (k+1)-mer ending at p is counted, d_bg[at_k + y] += 1, iff ALL of its k + 1 bases are valid (the
 * rule of pengk_strata_bg_count: an invalid base takes part in no word of any order, and the base behind it starts over at
 * order 0).  y: the word in BaMM order, older base more significant.  d_valid = NULL: every base valid.  d_bg is ADDED to
 * (caller-zeroed): shards and several calls sum exactly; at K = 2 the counters are those of pengk_strata_bg_count with one
 * stratum.  n_seq = 0 does nothing.  PENGK_ERR_ARG: K outside 0 .. 5, n_seq >= 2^32, a null pointer (but d_valid) with
 * n_seq > 0.  Asynchronous on the context's stream: no host wait. */
int pengk_bg_count_order(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid /* NULL: all valid */,
                         const int64_t* d_offs, const uint32_t* d_lens, uint64_t n_seq, int K /* 0..5 */,
                         uint64_t* d_bg /* (4^(K+2) - 4) / 3, ADDED to */);
/* The model of those counters (host only): BackgroundModel::calculateV continued to order K, float32, the same operations
 * in the same order.  V_0[y] = (n_0[y] + alpha_0 / 4) / (sum of n_0 + alpha_0); for k = 1 .. K
 *     V_k[y] = (n_k[y] + alpha_k * prior) / (n_{k-1}[y / 4] + alpha_k),   prior = V_{k-1}[y mod 4^k] (interpolate) or 1/4,
 * then every row of four is divided by its float32 sum (added in ascending order from 0).  h_alpha: K + 1 floats.  At
 * K <= 2 on the same counters the bits of pengk_bg_model and of the host's BackgroundModel.  PENGK_ERR_ARG: K outside
 * 0 .. 5, a null pointer. */
int pengk_bg_model_order(const uint64_t* h_counts, int K, const float* h_alpha /* K + 1 */, int interpolate, float* h_V);
/* The sweep with that model in its highest slot.  d_V: the run's own model, float[84] as pengk_pattern_stats takes it;
 * d_VK: orders 0 .. K of the high-order model, (4^(K+2) - 4) / 3 floats.  Slots o < max_k of d_bgprob hold exactly what
 * pengk_pattern_stats writes for d_V.  Slot max_k holds the order-K probability from d_VK: the factor of position
 * i = 0 .. W-1 is V_c[x_{i-c} .. x_i] with c = min(i, K), the products float32 in position order starting 1.0f * v0; under
 * both strands p[x] + p[rc x] in float32, a palindrome evaluated once.  At K = 2 with d_VK[0..84) == d_V and max_k = 2 every
 * table has pengk_pattern_stats' bits.  With a control (d_ctrl_counts, d_ctrl_ltot, pseudocount as
 * pengk_pattern_stats_control takes them; NULL, NULL, 0: none) every slot is q_o[x] = (float) fmax((double) p_o[x],
 * share[x]).  Expected, log-p and z are made of slot k, d_ltot and d_counts exactly as pengk_pattern_stats makes them.
 * Every even W from 2 to 14; the result does not depend on the option sweep_pairs.  PENGK_ERR_ARG: a NULL argument (but the
 * control's), K outside 0 .. 5, orders as pengk_pattern_stats refuses them, one control pointer without the other, a
 * pseudocount that is not finite and >= 0, or not 0 without a control.  Asynchronous on the context's stream: no host
 * wait. */
int pengk_pattern_stats_order(pengk_ctx* ctx, int W, int both_strands, int k, int max_k, const float* d_V /* 84 */,
                              int K /* 0..5 */, const float* d_VK /* orders 0..K */, const uint64_t* d_ltot,
                              const uint32_t* d_counts, const uint32_t* d_ctrl_counts, const uint64_t* d_ctrl_ltot,
                              double pseudocount /* control: NULL, NULL, 0 = none */, float* d_bgprob, float* d_expected,
                              float* d_logp, float* d_z);

/* ---- seed candidates (first half of BasePattern::select_base_patterns, src/base_pattern.cpp:443-515) ----------------
 * The reference std::sorts all 4^W ids by z-score and walks the ranking down to the threshold (:458-466); only ids with
 * z >= z_threshold and count >= count_threshold can become seeds.  This call compacts exactly those on the device
 * (unordered) into h_ids / h_z (capacity entries each); *n_out = their number -- when it exceeds capacity only the
 * first `capacity` found were copied and the caller retries with room for n_out.  The caller ranks the survivors.
 * NOTE the ranking of EXACT z ties (every reverse-complement pair under both strands) is std::sort's in the reference,
 * i.e. unspecified: a caller that ranks by (z descending, id ascending) reports the same seed set up to the strand a
 * pair is named on.  The host mirror keeps the reference's ranking by default (host/ranked_prefix.h) and uses this
 * call only on request (PENGK_SEED_SELECT=device). */
int pengk_seed_candidates(pengk_ctx* ctx, int W, const float* d_z, const uint32_t* d_counts, float z_threshold,
                          uint64_t count_threshold, uint32_t* h_ids, float* h_z, int64_t capacity, int64_t* n_out);

/* ---- K4: IUPAC degenerate-pattern aggregation (IUPACPattern::aggregate_attributes_from_basepatterns
 *      and count_combined_occurences, src/iupac_pattern.cpp:331-473,806-833) -------------------- */
typedef struct pengk_iupac_stats {
  uint64_t sites;   /* sum of counts over the distinct underlying k-mers */
  float bg_p;       /* float32 sum of background probabilities, in the reference's summation order */
  float expected;   /* float32 sum of expected counts, same order */
  float zscore;     /* :446 */
  float log_pvalue; /* :453-470, Bonferroni term included */
} pengk_iupac_stats;

/* n patterns (host ids) -> n results (host).  d_bgp: the order-k table used for z-scores. */
int pengk_iupac_aggregate(pengk_ctx* ctx, int W, int both_strands, const uint64_t* h_iupac_ids, int64_t n,
                          const uint32_t* d_counts, const float* d_bgp, const float* d_expected,
                          pengk_iupac_stats* h_out);

/* ---- K5: EM over the whole 4^W table (Peng::em_optimize_pwms + calculate_prob_odds,
 *      src/peng.cpp:48-197; row normalisation src/iupac_pattern.cpp:291-303) ----------------------
 * h_pwms: n_pwm x W x 4 floats, updated in place with the PWM the reference's loop ends on (before the
 * extra normalisation of the IUPACPattern(ori, pwm) constructor).  Three modes (option "em_fast"):
 *   2  (library default) serial: the reference's float32 arithmetic including the ORDER in which it adds the 4^W weights of a PWM
 *      cell (src/peng.cpp:121-127) -- PWMs, iteration counts and `change` are the reference's bit for bit.  From
 *      W = 8 on a cell's chain of roundings is evaluated as a scan (csrc/seqsum.h; a PWM with a negative or non-finite
 *      weight is summed by a plain loop).  What a caller needs when discrete decisions follow (motif merging compares
 *      similarity scores that are exactly tied in real arithmetic for reverse-complement twins); the CLI's default.
 *      Options of this mode (pengk_set_option):
 *      How the sum is carried out: W >= 10 -- the scan with its blocks of 4096 terms evaluated AHEAD of the chain: all
 *      blocks of all cells at once, each under the binade a prefix of plain block sums predicts for it, then one addition
 *      per block along the chain (three launches per iteration; the previous iteration's finalize step sits at the head of
 *      the first); W = 8 -- the scan, block after block; W <= 6 -- one dependent addition after the other (csrc/em_legacy.hip).
 *        "em_serial_scan"      2 (default) as above; 3 (W = 10, 12) the first two launches of an iteration as ONE kernel that
 *                              keeps a span's weights in LDS (half the table traffic at W = 12; measured no faster).
 *        "em_overlap"          W >= 10: streams the batches of PWMs take turns on, 1..4 (default 2; the
 *                              context's own stream waits for the others before the call returns or copies).
 *        "em_head_blocks"      W >= 10, 1..64 (default 1): the first blocks of every cell -- where the sum doubles from
 *                              block to block -- are folded from zero beside the evaluation of the others, the chain
 *                              starts behind them.  Results do not depend on it (and more than block 0 measured no faster).
 *        "em_test_skew"        (test hook) n > 0: about every n-th block gets a WRONG binade estimate -- results must not
 *                              change, only the time (the estimate never carries exactness).  0 = off.
 *        "em_test_lookback"    (test hook, "em_serial_scan" = 3) n > 0: every n-th workgroup acts as if the look-back for
 *                              its estimates had timed out (its blocks are then folded by their chains).  0 = off.
 *        "em_table_budget_mb"  MiB of weight tables in flight (4^W floats per PWM; twice that where the W = 8 scan keeps a
 *                              second copy in position 0's order); the PWMs of a call go
 *                              through in batches of that size.  0 (default) = automatic: 192 MiB for W <= 10 (what a
 *                              batch writes is still in the 256 MiB Infinity Cache when it is read), above that a
 *                              quarter of the free memory, at most 24 GiB.
 *   0  the reference's float32 terms (three divisions per k-mer weight), summed in fp64 through a fixed tree.
 *   1  (opt-in) the weight c*s / (1 + s/(prod/bg)) evaluated as c*s*prod / (prod + s*bg) with one
 *      reciprocal (~1 ulp per term), fp64 tree sums: the throughput mode, 2.3e12 PWM-k-mer evaluations/s.
 *      Its domain: for every k-mer with a count, c*s*prod >= 2^-126 and prod + s*bg < 2^126 (prod = the float32
 *      product over the PWM columns).  Nothing is promised outside it: a c*s*prod below 2^-150 is 0, and so is the term
 *      where s*bg overflows, although the reference's weight may be an ordinary float there.  Modes 0 and 2 take the
 *      reference's three divisions.
 * Modes 0 and 1 (mode 1: on its domain) agree with the reference within BASELINE.json's 1e-5 relative (the reference's own serial float32
 * sums are off by up to 2.6e-4 relative from the exact ones); the float32 product over the PWM columns is built in
 * the reference's order in all modes.
 * max_iterations <= 0: no iteration (the reference's loop condition, src/peng.cpp:104), the PWMs come back unchanged.
 * h_iters / h_change (optional): iterations run and last `change` per PWM. */
int pengk_em(pengk_ctx* ctx, int W, int64_t n_pwm, float* h_pwms, float saturation, float threshold,
             int max_iterations, const uint32_t* d_counts, const float* d_bg, int* h_iters, float* h_change);

/* Test hook: the serial mode (em_fast = 2) by an EARLIER GENERATION of this library, for cross-checks against the
 * current one (csrc/em_legacy.hip): 0 = one dependent addition after the other, 1 = the scan of csrc/seqsum.h block after
 * block (needs W >= 8; below: as 0); 2 / 3 = back to the library's scheme ("em_serial_scan").  Every generation returns
 * the reference's sums bit for bit; only the time differs. */
int pengk_test_em_generation(pengk_ctx* ctx, int generation);

/* Device-resident variant for benchmarking / pipelines: d_pwms n_pwm x W x 4 floats in HBM, updated in
 * place; d_state: n_pwm x 2 int32 scratch {iterations, active}; no host synchronisation. */
int pengk_em_device(pengk_ctx* ctx, int W, int64_t n_pwm, float* d_pwms, float saturation, float threshold,
                    int max_iterations, const uint32_t* d_counts, const float* d_bg, int32_t* d_state,
                    float* d_change);

/* ---- sequential float32 sums (the summation order of src/peng.cpp:121-127 on plain arrays) ---------------------
 * d_out[i] = ((0 + t[0]) + t[1]) + ... over the chain_len floats at d_terms + i * chain_len, every addition rounded
 * to float32 like a left-to-right CPU loop: bit-exact, including denormals and overflow to +inf.  Chains of
 * non-negative finite terms are evaluated by the scan of csrc/seqsum.h (one wave per chain, 4096 terms per step);
 * a chain with a negative, infinite or NaN term is summed by a plain loop on the device.  Device pointers. */
int pengk_sequential_sum_f32(pengk_ctx* ctx, const float* d_terms, uint64_t n_chains, uint64_t chain_len, float* d_out);

/* ---- motif similarity grid (Peng::merge_iupac_patterns' inner loops, src/peng.cpp:251-272, over
 *      IUPACPattern::calculate_S, src/iupac_pattern.cpp:568-615) -------------------------------------------------
 * n motifs: h_pwm / h_comp = n x PENGK_MAX_MOTIF_LEN x 4 floats (PWM and its reverse-complement PWM, rows beyond
 * h_len[i] unused), h_sites[i] = the motif's site count (decides which of a pair is complemented, :592-597), h_bg = the
 * 4 background letter frequencies.  For every pair (i, j), i < j, j >= first_new -- ordered j = first_new .. n-1, then
 * i = 0 .. j-1 -- h_out receives max over strands (both_strands) and shifts with >= 6 overlapping columns of the score
 * s (calculate_s, :551-566), -inf when no shift qualifies.  first_new = 0: the whole triangle; first_new = n - 1: the
 * new motif against all others after a merge.
 * The values are an fp64 evaluation rounded to float; the reference rounds every partial sum to float, so they agree
 * to ~1e-4, NOT bit for bit.  Use: find the pairs that can be the maximum, evaluate those with the reference's
 * arithmetic (the host mirror does exactly that with a margin of 2e-3). */
#define PENGK_MAX_MOTIF_LEN 64
int pengk_motif_similarity(pengk_ctx* ctx, int n, const float* h_pwm, const float* h_comp, const int32_t* h_len,
                           const uint64_t* h_sites, int both_strands, const float* h_bg, int first_new, float* h_out);

/* ---- motif scoring against sampled background sequences (the second user-facing step of the reference's wrapper
 *      scripts/shoot_peng.py, which runs BaMMmotif2's FDR tool and an R script over peng_motif's output; this library's
 *      metric is its own) ---------------------------------------------------------------------------
 * Scan layout of real sequences (NOT the packed layout above, which keeps only the runs the count visits and no
 * sequence identity): sequence i starts at base h_offs[i], a multiple of 32, in a 2-bit stream of uint64 words (base g in
 * bits [2(g%32), 2(g%32)+2) of word g/32; A,C,G,T = 0..3, any other letter stored as 0), has h_lens[i] bases and owns the
 * ceil(len/32) words from h_offs[i]/32 on; valid[g/32] bit g%32 is 1 iff base g is A/C/G/T (0 beyond the sequence's end).
 * The sampled background sequences use the same words layout (same offsets and lengths) with every base valid.
 * Replaces the per-motif sequence scans of scripts/shoot_peng.py's FDR call. */
#define PENGK_SCORE_SENTINEL (-2147483647 - 1) /* best score of a sequence without a window of A/C/G/T only */

/* Words a set of n_seq sequences takes (codes offsets h_code_offs[0..n_seq], as pengk_pack): sum of ceil(len/32). */
int pengk_scan_layout_words(const int64_t* h_code_offs, int64_t n_seq, uint64_t* n_words);
/* Host builder (pure CPU; scripts/shoot_peng.py hands FASTA files to the FDR tool instead): byte codes (0 = other,
 * A,C,G,T = 1..4) of n_seq sequences -> their words / validity words from word `word0` on, h_offs[i] / h_lens[i] for
 * i < n_seq.  Disjoint batches of a set (e.g. the chunks of the FASTA reader) may be built from several threads at once
 * into one set of arrays; each writes only the words it owns. */
int pengk_scan_layout_build(const uint8_t* h_codes, const int64_t* h_code_offs, int64_t n_seq, uint64_t word0,
                            uint64_t* h_words, uint32_t* h_valid, int64_t* h_offs, uint32_t* h_lens);
/* The synthetic input of pengk_synth_sequences (same splitmix64 stream: sequences [seq0, seq0+n_seq) of length L) in the
 * scan layout: d_words / d_valid n_seq * ceil(L/32) entries, d_offs / d_lens n_seq entries. */
int pengk_synth_scan_sequences(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, uint32_t L, uint64_t* d_words,
                               uint32_t* d_valid, int64_t* d_offs, uint32_t* d_lens);
/* Negatives of scripts/shoot_peng.py (its `--negN` random sequences), one per input sequence, sampled on the device from
 * an order-K background model (K <= 2) straight into d_words in the layout given by d_offs / d_lens (every base valid):
 * position p of the sequence with GLOBAL index seq0 + i draws r = mix64(seed + 0x9E3779B97F4A7C15 * (((seq0 + i) << 32)
 * + p + 1)) >> 32 (mod 2^64; mix64 = the splitmix64 finalizer) and takes base (r >= T0) + (r >= T1) + (r >= T2) with
 * the thresholds of its context -- the previous min(p, K) sampled bases.  h_thresholds: uint32 triples for the contexts
 * of orders 0..K back to back (1 + 4 + 16 triples at K = 2), a context of order k indexed like the background model's
 * V[k] (big-endian: the older base more significant); T_b = floor(c_b * 2^32) clamped to 2^32 - 1, c_b the cumulative
 * conditional probability of bases 0..b.  seq0 makes shards of a multi-process run sample what one process samples. */
int pengk_sample_background(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, const int64_t* d_offs,
                            const uint32_t* d_lens, int K, const uint32_t* h_thresholds, uint64_t* d_words);
/* Dinucleotide-preserving shuffle (--score-negatives shuffled): one negative per input sequence with the sequence's own
 * 25 doublet counts, first and last letter, uniform over all such sequences (Altschul and Erickson 1985; uShuffle's
 * construction without edge lists).  Input and output in the scan layout above with the same d_offs / d_lens; every
 * sequence owns its words.  The definition, which a numpy restatement and any sharding reproduce bit for bit:
 *   letters   a = 0..3 (A,C,G,T) where the validity bit is 1, a = 4 where it is 0: runs of other letters keep their
 *             neighbourhoods and the negative gets validity bits of its own.  Sequence g = seq0 + i, letters
 *             s[0..L-1], L < 2^31.
 *   counts    cnt[u][v] = #{p in 0..L-2: s[p] = u, s[p+1] = v}, out[u] = sum_v cnt[u][v], f = s[L-1]
 *   draws     draw(c) = mix64(seed + 0x9E3779B97F4A7C15 * ((g << 32) + c)) >> 32 (mod 2^64; mix64 = the splitmix64
 *             finalizer); pick(c, n) = (draw(c) * n) >> 32 as a 64-bit product, 0 <= pick < n (its bias of at most
 *             n / 2^32 is part of the definition); sel(u, k) = the smallest v with cnt[u][0] + .. + cnt[u][v] > k
 *   tree      the last edge of every letter, a uniform arborescence into f by Wilson's loop-erased walk: in_tree = {f},
 *             t = 0; for u0 = 0..4 in this order, unless out[u0] = 0 or u0 is in the tree: u = u0; while u is not in
 *             the tree { v = sel(u, pick(2^31 + t, out[u])); t += 1; next[u] = v; u = v }; then u = u0; while u is
 *             not in the tree { add u; u = next[u] }
 *   reserve   for every u != f with out[u] > 0: cnt[u][next[u]] -= 1, rem[u] = out[u] - 1; rem[f] = out[f]
 *   walk      o[0] = s[0], u = o[0]; for p = 1..L-1: if rem[u] > 0 { v = sel(u, pick(p, rem[u])); cnt[u][v] -= 1;
 *             rem[u] -= 1 } else v = next[u]; o[p] = v; u = v
 * L = 0 writes nothing; L = 1, 2 come back unchanged.  Output: the 2-bit code is 0 where the letter is 4; word and
 * validity bits beyond a sequence's end are 0.  d_valid = NULL: every base is valid, and d_out_valid may then be NULL
 * (not written).  The output buffers must differ from the inputs; seq0 + n_seq <= 2^32; n_seq = 0 does nothing;
 * PENGK_ERR_ARG otherwise.  Asynchronous on the context's stream. */
int pengk_shuffle_sequences(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, const uint64_t* d_words,
                            const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens, uint64_t* d_out_words,
                            uint32_t* d_out_valid);
/* Best window score of every motif on every sequence (the ZOOPS scan of scripts/shoot_peng.py's FDR call):
 * h_S = n_motifs x PENGK_MAX_MOTIF_LEN x 4 int32 log-odds (rows beyond h_len[m] unused), 1 <= h_len[m] <=
 * PENGK_MAX_MOTIF_LEN, |S| <= 2000.  d_best[m * n_seq + i] = max over the windows of sequence i whose bases are all
 * valid of sum_j S[m][j][base] -- with both_strands also of the reverse-complement matrix S[m][w-1-j][3-a] --,
 * PENGK_SCORE_SENTINEL without such a window.  d_valid = NULL: every base of a sequence is valid (sampled sequences).
 * Motifs are scanned in groups whose tables fit in LDS: each base is read from HBM once per group. */
int pengk_motif_scan(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, int32_t* d_best);
/* Histograms of d_best (n_motifs x n_seq, as pengk_motif_scan wrote it), ADDED to d_hist (uint64, caller-zeroed): motif m
 * owns h_nbins[m] = h_hi[m] - h_lo[m] + 2 bins from d_hist + h_hist_offs[m] on -- bin 0 the sentinel, bin 1 + s - h_lo[m]
 * score s (scores outside [lo, hi] are clamped into it; lo / hi = the sums of the column minima / maxima of S).  Integer
 * sums: histograms of shards and of several calls add exactly (scripts/shoot_peng.py's FDR tool keeps score lists). */
int pengk_score_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, uint64_t n_seq, const int32_t* h_lo,
                           const int32_t* h_hi, const uint64_t* h_hist_offs, uint64_t* d_hist);
/* Pure CPU: the two numbers scripts/shoot_peng.py adds to every motif, from the input (h_pos) and background (h_neg)
 * histograms of one motif (nbins bins, ascending scores, the sentinel bin lowest).  zoops_score = AUC =
 * sum_s P[s] * (2 Nneg_below(s) + N[s]) / (2 Npos Nneg) (numerator in int64; PENGK_ERR_RANGE above 2^62);
 * occur = clamp((TPR - FPR) / (1 - FPR), 0, 1) at the smallest threshold t with 100 Nneg_ge(t) <= Nneg (0 if FPR == 1).
 * This project's metric, not BaMMmotif2's AvRec. */
int pengk_score_summary(const uint64_t* h_pos, const uint64_t* h_neg, uint64_t nbins, double* zoops_out, double* occur_out);

/* ---- motif sites (--sites: every occurrence of the found motifs, with an exact p-value; this project's own) ----------
 * Over the scan layout above and the integer log-odds h_S / h_len of pengk_motif_scan: a site of motif m is a window
 * strand whose bases are all valid and whose score (sum_j S[m][j][base], on the - strand with S_rc[j][a] = S[w-1-j][3-a],
 * scored only with both_strands) is >= h_thr[m].  After the thresholds everything is integer: any slicing, any rank
 * count and a numpy restatement give the same set.
 * Three steps: pengk_sites_count, pengk_sites_slices (cuts the sequences into slices whose records fit a budget), then
 * pengk_sites_emit once per slice. */
#define PENGK_SITES_BLOCK 4096 /* sequences per block total of pengk_sites_slices */
typedef struct {
  uint32_t seq;          /* sequence index within the slice (global index - i0) */
  uint32_t pos;          /* 0-based first base of the window */
  int32_t score;         /* integer log-odds on the matched strand */
  uint32_t motif_strand; /* motif index * 2 + strand (0 = +, 1 = -) */
} pengk_site;

/* Pure CPU.  P(score >= t) for one strand of one window of motif S (w x 4 int32, |S| <= 2000) whose bases are drawn
 * independently from h_bg (4 float32, taken as double), for every t in [lo, hi] (the sums of the column minima /
 * maxima, returned in lo_out / hi_out): h_tail[t - lo], hi - lo + 1 entries (NULL: only lo / hi).  Exact DP over the
 * integer scores in a fixed order: q_0 = delta(0); q_{j+1}[t] = sum over a = 0, 1, 2, 3 in this order of
 * q_j[t - S[j][a]] * bg[a], each from 0.0 (terms outside q_j's range skipped); the tail summed sequentially from hi down. */
int pengk_score_tail_pvalues(const int32_t* h_S, int w, const float* h_bg, int32_t* lo_out, int32_t* hi_out, double* h_tail);
/* Pure CPU.  The smallest integer t in [lo, hi] with h_tail[t - lo] <= p (0 < p <= 1), else hi + 1 (no window reaches it). */
int pengk_score_threshold(const double* h_tail, int32_t lo, int32_t hi, double p, int32_t* t_out);
/* Sites of every motif on every sequence: d_counts[m * n_seq + i] (uint64), the number of window strands of sequence i
 * with score >= h_thr[m].  h_thr: n_motifs int32 (hi + 1 and above: none).  Other arguments as pengk_motif_scan. */
int pengk_sites_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                      const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                      int both_strands, const int32_t* h_thr, uint64_t* d_counts);
/* The count pass with the numbers behind the sites' q-values (--sites-qvalue), in one walk over the
 * sequences.  Motif m owns max(0, h_hi[m] - h_thr[m] + 1) uint64 bins from d_hist + h_hist_offs[m] on: bin s - h_thr[m]
 * counts the window strands with score exactly s, the sites of pengk_sites_count at the same thresholds.  h_hi[m] is the
 * sum of the column maxima of S[m] (pengk_score_tail_pvalues' hi_out; anything below it is PENGK_ERR_ARG, since a score
 * would have no bin).  d_tests[m] (n_motifs uint64) counts the scored window strands of motif m: a window whose bases are
 * all valid counts once, twice with both_strands.  Both are ADDED to (caller-zeroed): shards and several calls sum
 * exactly, as in pengk_score_histograms.  d_counts: NULL, or the n_motifs x n_seq array of pengk_sites_count, written
 * (not added to) with the same values.  d_hist may be NULL when no motif has a bin.  Other arguments as
 * pengk_sites_count; n_seq = 0 or n_motifs = 0 does nothing. */
int pengk_sites_histograms(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                           int both_strands, const int32_t* h_thr, const int32_t* h_hi, const uint64_t* h_hist_offs,
                           uint64_t* d_hist, uint64_t* d_tests, uint64_t* d_counts);
/* ---- database enrichment (--enrich: which motifs of a MEME database are enriched in the input against its negatives;
 *      this project's own definitions, not SEA's or AME's: INTEGRATION.md 7k) ------------------------------------------
 * The scan of pengk_motif_scan with the best score of a sequence kept in a register and binned where it stands: nothing
 * of size n_motifs x n_seq is written, so a whole database fits.  Arguments as pengk_sites_histograms: motif m owns
 * max(0, h_hi[m] - h_thr[m] + 1) uint64 bins from d_hist + h_hist_offs[m] on.  Every sequence with at least one window
 * whose bases are all valid adds 1 to d_scored[m] (n_motifs uint64) and, if its best window-strand score b -- exactly
 * pengk_motif_scan's value -- is >= h_thr[m], 1 to bin b - h_thr[m]; a sequence without such a window adds nothing.
 * Both arrays are ADDED to (caller-zeroed): shards and several calls sum exactly.  d_hist may be NULL when no motif has
 * a bin.  n_seq = 0 or n_motifs = 0 does nothing; n_seq >= 2^32 and an h_hi[m] below the sum of the column maxima of
 * S[m] are PENGK_ERR_ARG.  n_motifs is unbounded: the motif groups are staged and launched in batches of the option
 * "enrich_groups_per_launch" (default 1024, 1 .. 65535; a test hook like "sites_record_budget": a small test can cross
 * the seam between two launches; also readable through pengk_get_info).  Asynchronous on the context's stream but for
 * the staging copies. */
int pengk_motif_enrich(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                       const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                       int both_strands, const int32_t* h_thr, const int32_t* h_hi, const uint64_t* h_hist_offs,
                       uint64_t* d_hist, uint64_t* d_scored);
/* Pure CPU.  log10 P(X >= k) for X ~ Hypergeometric(N, K marked, n drawn), K <= N, n <= N (Fisher's one-sided tail):
 * 0.0 for k <= max(0, n + K - N), -inf for k > min(K, n).  Loader's saddle-point form of the point mass (stirlerr / bd0)
 * at the end of the shorter tail, then the ratio recurrence away from the mode, relative to that point mass; the
 * complement when k lies at or below the mode.  Holds for N of 4e7 with a tail near 1 and for tails far below the
 * smallest double. */
int pengk_hypergeom_log10_sf(uint64_t N, uint64_t K, uint64_t n, uint64_t k, double* out);
typedef struct {
  int32_t threshold;       /* the reported score threshold (thr + nbins when none was tried) */
  uint32_t n_thresholds;   /* T: the thresholds tried */
  uint64_t pos_hits;       /* a: input sequences with a best score >= threshold */
  uint64_t neg_hits;       /* b: negatives likewise */
  double enrichment;       /* ((a + 1) / (n_pos + 1)) / ((b + 1) / (n_neg + 1)) */
  double log10_pvalue;     /* log10 P(X >= a), X ~ Hypergeometric(n_pos + n_neg, a + b, n_pos) */
  double log10_adj_pvalue; /* min(0, log10_pvalue + log10 T) */
} pengk_enrichment;
/* Pure CPU.  One motif's enrichment test from its two histograms of pengk_motif_enrich (h_pos over the input, h_neg over
 * the negatives, nbins bins each, bin k = score thr + k, summed over all ranks) and the scored sequences n_pos / n_neg
 * (d_scored).  From the top bin down a(k) / b(k) are the sums of h_pos / h_neg over the bins >= k; the threshold thr + k
 * is tried only where h_pos[k] + h_neg[k] > 0 (elsewhere it is the test of the threshold above); T counts them.  At a
 * tried k, p(k) = P(X >= a(k)) with N = n_pos + n_neg, K = a(k) + b(k), n = n_pos (pengk_hypergeom_log10_sf).  Reported
 * is the k with the smallest log10 p(k), the higher threshold on equality; log10_adj_pvalue is the Bonferroni correction
 * over the T thresholds.  T = 0: threshold thr + nbins, no hits, enrichment by the same formula, both logs 0.  A sum of
 * h_pos above n_pos or of h_neg above n_neg is PENGK_ERR_ARG. */
int pengk_enrich_summary(const uint64_t* h_pos, const uint64_t* h_neg, uint64_t nbins, int32_t thr, uint64_t n_pos,
                         uint64_t n_neg, pengk_enrichment* out);
typedef struct {
  int32_t threshold;             /* pengk_enrich_summary's threshold on the two training histograms */
  uint32_t n_thresholds;         /* T: the thresholds it tried there */
  uint64_t train_pos_hits;       /* a, b of that call: what the motif was chosen on */
  uint64_t train_neg_hits;
  double train_log10_adj_pvalue; /* its log10_adj_pvalue: Bonferroni over T, and still fitted to these sequences */
  uint64_t hold_pos_hits;        /* a': hold-out input sequences with a best score >= threshold */
  uint64_t hold_neg_hits;        /* b': hold-out negatives likewise */
  double hold_log10_pvalue;      /* log10 P(X >= a'), X ~ Hypergeometric(n_hold_pos + n_hold_neg, a' + b', n_hold_pos) */
  double hold_enrichment;        /* ((a' + 1) / (n_hold_pos + 1)) / ((b' + 1) / (n_hold_neg + 1)) */
} pengk_holdout;
/* Pure CPU.  One motif's test on sequences it was not fitted to (--holdout): four histograms of
 * pengk_motif_enrich with the same thr and nbins (training and hold-out share of the input and of the negatives, summed
 * over all ranks) and the four scored counts.  The threshold is the one pengk_enrich_summary(h_train_pos, h_train_neg,
 * nbins, thr, n_train_pos, n_train_neg) reports, with its T, hits and log10_adj_pvalue.  a' / b' = the sums of h_hold_pos /
 * h_hold_neg over the bins k >= threshold - thr; hold_log10_pvalue = pengk_hypergeom_log10_sf(n_hold_pos + n_hold_neg,
 * a' + b', n_hold_pos, a'): one threshold, fixed before the hold-out was looked at, so no Bonferroni factor.  T = 0 (no
 * training sequence in any bin): threshold thr + nbins, no hits, both logs 0, hold_enrichment by the same formula.  A sum
 * of a histogram above its n is PENGK_ERR_ARG. */
int pengk_holdout_summary(const uint64_t* h_train_pos, const uint64_t* h_train_neg, const uint64_t* h_hold_pos,
                          const uint64_t* h_hold_neg, uint64_t nbins, int32_t thr, uint64_t n_train_pos, uint64_t n_train_neg,
                          uint64_t n_hold_pos, uint64_t n_hold_neg, pengk_holdout* out);
/* Pure CPU.  Benjamini-Hochberg q-values of one motif's sites from its histogram (h_hist[k]: the sites with score t + k,
 * nbins = hi - t + 1 bins, summed over all ranks), the number of tests n_tests (d_tests, summed likewise) and
 * h_tail_from_thr = tail + (t - lo) of pengk_score_tail_pvalues.  n(k) = sum over k' >= k of h_hist[k'] (uint64, from
 * the top down); r(k) = (double)n_tests * h_tail_from_thr[k] / (double)n(k) -- one multiplication, then one division --
 * or +inf when n(k) = 0; h_q[k] = min(1.0, min over k' <= k of r(k')), a running minimum from bin 0 up, so it never
 * rises with the score.  h_q takes nbins doubles; nbins = 0 does nothing. */
int pengk_sites_qvalues(const uint64_t* h_hist, uint64_t nbins, uint64_t n_tests, const double* h_tail_from_thr, double* h_q);
/* Pure CPU.  The smallest score s = t + k, k < nbins, with h_q[k] <= q_max (q_max >= 0), else t + nbins (no site). */
int pengk_qvalue_threshold(const double* h_q, uint64_t nbins, int32_t t, double q_max, int32_t* t_out);
/* From d_counts (pengk_sites_count): h_motif_totals[m] = the sites of motif m over all sequences, and the slices
 * [h_bounds[k], h_bounds[k + 1]) of the sequences, k < *n_slices, in order, covering [0, n_seq), with h_records[k] records
 * each.  A slice is as long as its records stay within the option "sites_record_budget" (default 2^24; >= 1, a test
 * hook can force many slices) and at most 2^31 sequences; a single sequence above the budget is a slice of its own.
 * Only the first max_slices slices are written (h_bounds: max_slices + 1 entries); *n_slices is always the full count,
 * so a caller with too small arrays calls again.  Synchronises with the stream. */
int pengk_sites_slices(pengk_ctx* ctx, const uint64_t* d_counts, uint64_t n_seq, int n_motifs, uint64_t* h_motif_totals,
                       uint64_t max_slices, uint64_t* h_bounds, uint64_t* h_records, uint64_t* n_slices);
/* The sites of sequences [i0, i1) (at most 2^31 of them) as records in d_sites, in this order: motif index, sequence,
 * window position, + before -.  The same arguments as pengk_sites_count, whose d_counts fix every record's place: the
 * slice's records are sum over m, i of d_counts[m * n_seq + i]; none at or beyond cap is written. */
int pengk_sites_emit(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, const int32_t* h_thr, const uint64_t* d_counts, uint64_t i0, uint64_t i1,
                     pengk_site* d_sites, uint64_t cap);

/* ---- erasing sites and packing on the device (--erase: mask the sites of the found motifs and search what is left;
 *      this project's own) -----------------------------------------------------------------------------
 * Integer throughout: a numpy restatement and any sharding give the same bits.
 * A site is what pengk_sites_count counts (same arguments, d_valid = NULL: every base of a sequence valid).  cover = the
 * bases that lie in [p, p + w_m) of some site of some motif; every motif is judged against the INPUT validity, so a site
 * of one motif does not hide a site of another within one call.  d_out_valid (the layout of d_valid, must differ from
 * it) receives d_valid & ~cover for every word of every sequence, the bits at and beyond a sequence's end cleared.
 * d_sites[m] (n_motifs uint64) and d_erased[0] (uint64) are ADDED to (caller-zeroed): the site window strands of motif m
 * -- the row sums of pengk_sites_count -- and the bits that went from 1 to 0, each counted once whatever number of
 * motifs covers it.  n_seq = 0 does nothing; n_motifs = 0 writes d_out_valid (nothing covered) and nothing else. */
int pengk_mask_sites(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, const int32_t* h_thr, uint32_t* d_out_valid, uint64_t* d_sites, uint64_t* d_erased);
/* The host packer on the device: from the scan layout to the count layout, bit for bit what pengk_pack writes for the
 * same sequences given as byte codes (a cleared validity bit = code 0): words[0 .. n_words), items[0 .. n_items), n_bases,
 * n_windows, max_bin_bound, n_sequences, max_len and all_whole.  bg_counts are not produced (zero).
 * pengk_pack_scan_sizes measures: `out` receives the figures (out->words / out->items stay NULL: the buffers are the
 * caller's), d_seq_base[i] / d_seq_item[i] (n_seq uint64 each, caller-owned) the stored bases / items in front of
 * sequence i.  PENGK_ERR_RANGE where pengk_pack gives it.  Synchronises with the host.
 * pengk_pack_scan writes: d_out_words (out->n_words uint64; zeroed here) and d_out_items (out->n_items uint64) from the
 * same input, W, item_windows and the two offset arrays; nothing at or beyond n_words / n_items is written.  Asynchronous
 * on the context's stream.  Attach the result with pengk_set_sequences. */
int pengk_pack_scan_sizes(pengk_ctx* ctx, const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens, uint64_t n_seq,
                          int W, int item_windows, uint64_t* d_seq_base, uint64_t* d_seq_item, pengk_packed* out);
int pengk_pack_scan(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                    const uint32_t* d_lens, uint64_t n_seq, int W, int item_windows, const uint64_t* d_seq_base,
                    const uint64_t* d_seq_item, uint64_t* d_out_words, uint64_t n_words, uint64_t* d_out_items, uint64_t n_items);

/* ---- masking low-complexity stretches (--mask-low-complexity: poly-A tracts, (CA)n and their like are taken out of the
 *      input before anything is counted, as dustmasker, sdust and RepeatMasker's simple-repeat pass do in front of other
 *      discovery tools) ------------------------------------------------------------------------------
 * This project's own statement of the symmetric DUST criterion of Morgulis et al. 2006, integer throughout: a numpy
 * restatement and any sharding give the same bits.  The numbers are NOT promised to be those of NCBI's dustmasker or of
 * sdust.  Per sequence of the scan layout above, letters s[0..L) and validity bits v (d_valid = NULL: every base valid):
 *   triplet   one stands at p (0 <= p <= L-3) iff v[p] & v[p+1] & v[p+2]; its value t[p] = 16 s[p] + 4 s[p+1] + s[p+2]
 *   interval  (i, l) = the triplets i .. i+l-1, all standing, 2 <= l <= PENGK_DUST_WINDOW - 2: at most 64 bases
 *   score     num(i, l) / (l - 1), num(i, l) = sum over the triplet values x of c_x (c_x - 1) / 2, c_x the occurrences of
 *             x in the interval; fractions are compared by cross-multiplication (num <= 1891: 32 bits hold every product)
 *   high      10 * num > threshold * (l - 1)
 *   perfect   high, and no interval (i', l') inside it, l' >= 2, has a strictly larger score (equality keeps it perfect)
 *   cover     the bases [i, i + l + 2) of every perfect interval
 * d_out_valid (the layout of d_valid, must differ from it) receives v & ~cover for every word of every sequence, the bits
 * at and beyond a sequence's end cleared, as pengk_mask_sites leaves them.  d_masked[0] / d_masked[1] (uint64) are ADDED to
 * (caller-zeroed; shards and several calls sum exactly): the bits that went from 1 to 0 and the sequences that lost at
 * least one.  n_seq = 0 does nothing.  PENGK_ERR_ARG: threshold outside 1 .. 1000 (DUST's is 20; above 310 nothing can
 * be high, which is legal), n_seq >= 2^32, d_out_valid == d_valid.  Asynchronous on the context's stream. */
#define PENGK_DUST_WINDOW 64
int pengk_mask_low_complexity(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                              const uint32_t* d_lens, uint64_t n_seq, int threshold, uint32_t* d_out_valid,
                              uint64_t* d_masked /* [2], ADDED to: bits that went 1 -> 0; sequences with at least one */);

/* ---- a control set matched to the input (--score-negatives control: the negatives of the scoring steps are real
 *      sequences, drawn from the control in proportion to the input's GC content and length, as HOMER and BiasAway
 *      match theirs; this project's own definitions) -------------------------------------------------
 * Integer throughout: a numpy restatement and any sharding give the same bits.  A subset of a scan layout is a shorter
 * pair of offs / lens arrays into the same words, which every scan entry above accepts as it stands.
 *
 * The stratum of every sequence of a scan layout: d_stratum[i] (n_seq uint16) and its count, d_hist[stratum] (256
 * uint64, ADDED to: caller-zeroed, shards and several calls sum exactly).  n = the valid bases of the sequence (d_valid =
 * NULL: its length), gc = the C or G among them -- every other letter is stored as A and the words are zero beyond the
 * end, so no validity word is read for it.  n = 0: stratum 0xFFFF, counted nowhere.  Else g = min(G - 1, (gc * G) / n),
 * G = gc_bins in 1 .. 16; with L the length, l = floor(log2 L) and sub = the bit of L below its top bit (0 for L = 1),
 * lb = clamp(2 l + sub - 10, 0, 15) -- half-octave length bins, everything below 48 bases in bin 0, everything from 6144
 * on in bin 15 --, lb = 0 when use_length is 0; stratum = lb * G + g.  n_seq = 0 does nothing; n_seq >= 2^32, gc_bins
 * outside 1 .. 16 and use_length other than 0 / 1 are PENGK_ERR_ARG.  Asynchronous on the context's stream. */
int pengk_seq_strata(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int gc_bins, int use_length, uint16_t* d_stratum, uint64_t* d_hist);
/* Pure CPU.  From the input's and the control's stratum counts (256 uint64 each, summed over all ranks) and ratio R >= 1:
 * h_quota[s] = min(h_ctrl[s], R * h_in[s]), the control sequences of stratum s to keep, and *shortfall_out = sum over s
 * of R * h_in[s] - h_quota[s], what the control could not supply.  A product or a sum beyond 2^63 is PENGK_ERR_RANGE,
 * R = 0 PENGK_ERR_ARG. */
int pengk_match_quotas(const uint64_t* h_in, const uint64_t* h_ctrl, uint64_t ratio, uint64_t* h_quota, uint64_t* shortfall_out);
/* The selection.  d_stratum: the strata of this call's n_seq sequences (pengk_seq_strata; an entry of 256 or above is never
 * kept); h_count[s] the sequences of stratum s over ALL ranks, h_quota[s] <= h_count[s] how many of them to keep, h_rank0[s]
 * how many of them the earlier ranks hold (256 uint64 each).  Sequence i of stratum s has the rank r = h_rank0[s] + the
 * sequences j < i of this call with the same stratum -- a stable rank in file order -- and is kept iff
 * ((r + 1) q) / c > (r q) / c in uint64 (q = h_quota[s], c = h_count[s]): even spacing through the file, exactly q kept
 * over all shards, q = c keeps all, q = 0 none.  The kept sequences' d_offs[i] / d_lens[i] / i are written compacted, in
 * file order, to d_sel_offs / d_sel_lens / d_sel_index (room for n_seq entries each); *n_sel_out = this call's count.
 * n_seq = 0 does nothing.  PENGK_ERR_ARG: n_seq >= 2^32, an h_quota[s] > h_count[s], an h_count[s] >= 2^32, an
 * h_rank0[s] > h_count[s].  Synchronises with the host. */
int pengk_select_strata(pengk_ctx* ctx, const uint16_t* d_stratum, uint64_t n_seq, const uint64_t* h_count, const uint64_t* h_quota,
                        const uint64_t* h_rank0, const int64_t* d_offs, const uint32_t* d_lens, int64_t* d_sel_offs,
                        uint32_t* d_sel_lens, uint32_t* d_sel_index, uint64_t* n_sel_out);

/* ---- a hold-out share (--holdout: motifs are found on one share of the input and tested on the rest, as STREME sets 10 %
 *      of its sequences aside; this project's own definitions) --------------------------------------
 * Integer throughout: a numpy restatement and any sharding give the same bits.  Sequence i of this call's n_seq has the
 * global index g = seq0 + (d_index ? d_index[i] : i) and the class 1 (hold-out) iff
 *   mix64(seed + 0x9E3779B97F4A7C15 * (g + 1)) >> 32 < threshold      (mod 2^64; mix64 = the splitmix64 finalizer),
 * else 0 (training); threshold in 0 .. 2^32 (0: none held out, 2^32: all), a share of threshold / 2^32.  Both classes'
 * d_offs[i] / d_lens[i] / i are written compacted, in file order, to d_offs0 / d_lens0 / d_index0 (training) and d_offs1 /
 * d_lens1 / d_index1 (hold-out), room for n_seq entries each -- with the words of the layout that d_offs / d_lens belong
 * to, two scan layouts; *n0_out / *n1_out (host) = the two counts.  d_class[i] (n_seq uint8) receives the class when
 * given.  d_index (NULL, or n_seq local indices such as pengk_select_strata's d_sel_index): a set that was reduced before
 * is split by its sequences' indices in the file, so a matched and an unmatched control put a sequence on the same side.
 * n_seq = 0 does nothing.  PENGK_ERR_ARG, and nothing written: seq0 + n_seq > 2^32, threshold > 2^32, an output that
 * overlaps d_index, d_offs or d_lens.  Synchronises with the host. */
int pengk_split_sequences(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, uint64_t threshold, const uint32_t* d_index,
                          const int64_t* d_offs, const uint32_t* d_lens, uint8_t* d_class, int64_t* d_offs0, uint32_t* d_lens0,
                          uint32_t* d_index0, uint64_t* n0_out, int64_t* d_offs1, uint32_t* d_lens1, uint32_t* d_index1,
                          uint64_t* n1_out);

/* ---- central enrichment (--centrality: which found motifs sit at the centres of the input sequences; CentriMo's
 *      site distribution and binomial test) ------------------------------------------------------------
 * Over the scan layout and the integer log-odds of pengk_motif_scan.  One best window strand per (motif, sequence); the
 * offsets of those at or above the motif's threshold binned on the device; the test on the host.  Integer up to the
 * summary: any slicing, any rank count and a numpy restatement give the same histograms. */
#define PENGK_CENTRALITY_MAX_LEN 65536 /* longer sequences are not considered */
/* Replaces CentriMo's per-sequence best-site search.  The best window strand of every motif on every sequence:
 * d_best[m * n_seq + i] its score (PENGK_SCORE_SENTINEL without a window of A/C/G/T only), d_site[m * n_seq + i] = 2p + s
 * (p its 0-based start in + coordinates, s 0 for +, 1 for -; 0 without a window).  Best = the largest (score, key), key =
 * mix64(mix64(0x9E3779B97F4A7C15 * (g + 1) ^ m) ^ (2p + s)) mod 2^64 (mix64 = the splitmix64 finalizer, g = seq0 + i the
 * sequence's global index, m the motif index); an equal key: the smaller p, then +.  A deterministic, uniform tie-break
 * that no shard boundary changes.  Other arguments as pengk_motif_scan (both_strands 0: + only). */
int pengk_motif_best_sites(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, uint64_t seq0, int n_motifs, const int32_t* h_S,
                           const int32_t* h_len, int both_strands, int32_t* d_best, uint64_t* d_site);
/* Replaces CentriMo's site-position counts.  For every motif m and every sequence i with h_len[m] <= L <= max_len (L =
 * d_lens[i]; 1 <= max_len <= PENGK_CENTRALITY_MAX_LEN) whose best score (d_best, d_site from pengk_motif_best_sites) is
 * >= h_thr[m]: ADDS 1 to d_hist_offsets[m * (2 max_len + 1) + max_len + d], d = 2p + w - L (twice the distance of the
 * site's centre from the sequence's centre), and to d_hist_lengths[m * (max_len + 1) + L].  uint64, caller-zeroed. */
int pengk_centrality_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                                const uint32_t* d_lens, uint64_t n_seq, const int32_t* h_len, const int32_t* h_thr,
                                uint32_t max_len, uint64_t* d_hist_offsets, uint64_t* d_hist_lengths);
typedef struct {
  uint64_t sites;        /* N: sequences with a site */
  uint32_t max_offset;   /* Dm: the largest L - w among them */
  uint32_t window;       /* r: the window |d| <= r with the smallest p-value (center_distance = r / 2) */
  uint64_t in_window;    /* K(r) */
  double expected;       /* N * mean of f(L, w, r) over the sites' sequences */
  double log10_pvalue;   /* log10 P(X >= K), X ~ Binomial(N, expected / N) */
  double log10_evalue;   /* log10_pvalue + log10(Dm + 1) + log10(n_motifs) */
} pengk_centrality;
/* Pure CPU.  Replaces CentriMo's binomial test.  From one motif's two histograms (max_len as above, w its width,
 * n_motifs the motifs of the run, for the Bonferroni factor): with N = 0 only `sites` is set (0) and the rest is 0.
 * Otherwise, for each r in 0..Dm, K(r) = #{|d| <= r}, p(r) = (1/N) sum_L n_L f(L, w, r), f(L, w, r) = #{p in 0..L-w :
 * |2p + w - L| <= r} / (L - w + 1), and P(r) = P(X >= K(r)) for X ~ Binomial(N, p(r)) -- exact for equal lengths,
 * conservative for mixed ones (Hoeffding 1956).  `window` is the r with the smallest log10 P(r), the smaller r on ties;
 * an r at which no sequence can have an offset is a tie with r - 1 (or has p = 0 at r = 0) and is never reported.  Cost:
 * O(Dm + max_len) to build every p(r); the tail by a continued fraction in log space (no underflow). */
int pengk_centrality_summary(const uint64_t* h_hist_offsets, const uint64_t* h_hist_lengths, uint32_t max_len, int w,
                             int n_motifs, pengk_centrality* out);
/* Pure CPU.  log10 P(X >= k), X ~ Binomial(n, p), k <= n, 0 <= p <= 1: the tail pengk_centrality_summary uses. */
int pengk_binomial_log10_sf(uint64_t n, uint64_t k, double p, double* out);

/* ---- spaced dyads (--dyads: pairs of trinucleotides a fixed number of unconstrained bases apart, the bipartite sites of
 *      dimeric factors -- CGG n11 CCG, TGG n7 CCA -- that no contiguous word of the k-mer table holds; the question RSAT's
 *      dyad-analysis answers) ---------------------------------------------------------------------------
 * This project's own definitions, integer up to the summary: a numpy restatement and any sharding give the same tables.
 * The numbers are NOT promised to be RSAT's.  Per sequence of the scan layout above, letters s[0..L) and validity bits v
 * (d_valid = NULL: every base valid), r[p] = the number of consecutive valid bases from p on:
 *   triplet     one stands at p iff r[p] >= 3; its value t[p] = 16 s[p] + 4 s[p+1] + s[p+2]; it adds 1 to d_mono[t[p]]
 *   occurrence  for every p and every g in 0 .. max_gap with r[p] >= 6 + g: one occurrence of the dyad (a, g, b), a = t[p],
 *               b = t[p + 3 + g], key = 64 a + b.  The whole span is valid, spacer included: a masked stretch cuts dyads
 *               as it cuts words
 *   strands     with both_strands, key = min(key, 64 rc(b) + rc(a)), rc the reverse complement of a triplet: a dyad that
 *               is its own reverse complement counts once per position, and an entry that is not canonical is never
 *               written.  d_mono holds the + strand's triplets either way
 *   count       d_counts[g * 4096 + key] += 1
 * d_counts ((max_gap + 1) x 4096 uint64) and d_mono (64 uint64) are ADDED to (caller-zeroed): shards and several calls sum
 * exactly.  n_seq = 0 does nothing.  PENGK_ERR_ARG: max_gap outside 0 .. PENGK_DYAD_MAX_GAP, both_strands other than 0 / 1,
 * n_seq >= 2^32.  Asynchronous on the context's stream. */
#define PENGK_DYAD_MAX_GAP 26 /* a dyad spans at most 32 bases */
int pengk_dyad_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int max_gap, int both_strands,
                     uint64_t* d_counts /* (max_gap + 1) x 4096, ADDED to */, uint64_t* d_mono /* 64, ADDED to */);
typedef struct {
  uint32_t gap;           /* g */
  uint32_t key;           /* 64 a + b (the canonical one on both strands) */
  uint64_t count;         /* d_counts[g * 4096 + key] */
  uint64_t positions;     /* T[g]: the sum of row g */
  double p;               /* the probability under test */
  double expected;        /* (double)T[g] * p */
  double log10_pvalue;    /* log10 P(X >= count), X ~ Binomial(T[g], p) */
  double log10_evalue;    /* log10_pvalue + log10(tests) */
  double other_gaps_mean; /* the mean count of the same key over the other gaps (0 when max_gap = 0) */
  uint32_t family;        /* the 1-based rank of the family's head */
  uint32_t is_head;       /* 1 for the head itself */
} pengk_dyad;
/* Pure CPU.  The report from the two tables of pengk_dyad_count (summed over all ranks), in this order.  M = the sum of
 * h_mono; f(x) = (double)mono[x] / (double)M on one strand, (double)(mono[x] + mono[rc x]) / (2.0 * (double)M) on both;
 * T[g] = the integer sum of row g; per (g, key): p = f(a) * f(b), on both strands multiplied by 2.0 after that where key
 * is not its own reverse complement; tests = (max_gap + 1) * (both_strands ? 2080 : 4096).  A dyad is a candidate iff
 * count >= min_count and (double)count > (double)T[g] * p; log10_pvalue = pengk_binomial_log10_sf(T[g], count, p),
 * log10_evalue = log10_pvalue + log10((double)tests); candidates with log10_evalue <= log10(max_evalue) are reported,
 * ordered by (log10_evalue, g, key) ascending.
 * Families: a dyad is the string over ACGTn of length 6 + g -- a, g times n, b.  Y is related to X iff for some offset o
 * in -2 .. 2, Y laid at o on X has no column where both hold letters that differ and at least 4 columns where both hold
 * the same letter; on both strands Y's reverse complement is tried as well.  Walking the report in order, a dyad joins
 * the first earlier family head it is related to, else it heads a new family.
 * Only the first `capacity` lines are written to `out`; *n_out is always the full count, so a caller with too small an
 * array calls again.  M = 0 reports nothing.  PENGK_ERR_ARG: max_gap or both_strands as above, max_evalue not > 0. */
int pengk_dyad_summary(const uint64_t* h_counts, const uint64_t* h_mono, int max_gap, int both_strands, uint64_t min_count,
                       double max_evalue, pengk_dyad* out, uint64_t capacity, uint64_t* n_out);

/* ---- positional words (--positional: k-mers that keep one position in the sequences -- a TATA box 30 bases ahead of a
 *      TSS, an Inr, a Kozak or splice-site signal, a weak site at a ChIP summit -- whether or not they are over-represented;
 *      the question RSAT's position-analysis answers) ---------------------------------------------------
 * This project's own definitions, integer up to the summary: a numpy restatement and any sharding give the same table.
 * The numbers are NOT promised to be RSAT's.  Per sequence of the scan layout above, letters s[0..L) and validity bits v
 * (d_valid = NULL: every base valid), r[p] = the number of consecutive valid bases from p on, K in 4 .. 7:
 *   word        one stands at p iff r[p] >= K; its value has the first base highest (as the dyad key); key = the value, with
 *               both_strands min(value, revcomp(value))
 *   clump head  the occurrence at p is counted iff no word with the same key stands at any of p-1 .. p-(K-1).  A
 *               predecessor cut by an invalid base, or before the sequence start, does not stand.  A run of 70 000 equal
 *               letters counts once; ACACAC... counts its first two positions
 *   coordinate  anchor 0 (start): c = p;  1 (end): c = L - K - p;  2 (centre): c = |2p + K - L| >> 1 -- unsigned, so the
 *               answer is the same whichever strand a peak was written on
 *   bin         b = c / bin_size; counted iff b < n_bins (words further out are ignored)
 *   count       d_counts[b * 4^K + key] += 1
 * d_counts (n_bins x 4^K uint64) is ADDED to (caller-zeroed): shards and several calls sum exactly.  No entry that is not
 * canonical is ever written.  n_seq = 0 does nothing.  PENGK_ERR_ARG: K outside 4 .. 7, anchor outside 0 .. 2, bin_size
 * outside 1 .. PENGK_POSITION_MAX_BIN_SIZE, n_bins outside 1 .. PENGK_POSITION_MAX_BINS, both_strands other than 0 / 1,
 * n_seq >= 2^32, a null pointer (but d_valid) with n_seq > 0.  Asynchronous on the context's stream. */
#define PENGK_POSITION_MIN_K 4
#define PENGK_POSITION_MAX_K 7
#define PENGK_POSITION_MAX_BINS 64
#define PENGK_POSITION_MAX_BIN_SIZE 65536
int pengk_position_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                         const uint32_t* d_lens, uint64_t n_seq, int K, int anchor, int bin_size, int n_bins, int both_strands,
                         uint64_t* d_counts /* n_bins x 4^K, ADDED to */);
typedef struct {
  uint32_t key;              /* the word, first base highest (the canonical one on both strands) */
  uint32_t bin;              /* b: the key's best bin */
  uint64_t count;            /* d_counts[b * 4^K + key] */
  uint64_t total;            /* C[key]: the key's count over all bins */
  uint64_t bin_positions;    /* N[b]: the sum of row b */
  double expected;           /* (double)C[key] * q[b] */
  double log10_pvalue;       /* log10 P(X >= count), X ~ Binomial(C[key], q[b]) */
  double log10_evalue;       /* log10_pvalue + log10(tests) */
  uint32_t bins_significant; /* the key's candidate bins at or below max_evalue */
  uint32_t family;           /* the 1-based rank of the family's head */
  uint32_t is_head;          /* 1 for the head itself */
} pengk_position_word;
/* Pure CPU.  The report from the table of pengk_position_count (summed over all ranks), in this order.  N[b] = the integer
 * sum of row b, C[key] = the integer sum of the key's column, Nt = the sum of all N, q[b] = (double)N[b] / (double)Nt;
 * keys = 4^K on one strand, on both 4^K / 2 for odd K and (4^K + 4^(K/2)) / 2 for even K (2080 at K = 6);
 * tests = n_bins * keys.  A (key, b) is a candidate iff count >= min_count and (double)count > (double)C[key] * q[b]
 * (depleted positions are not reported); log10_pvalue = pengk_binomial_log10_sf(C[key], count, q[b]), log10_evalue =
 * log10_pvalue + log10((double)tests).  A key's line carries its best bin -- the smallest log10_evalue, on a tie the
 * lowest bin -- and bins_significant, the number of its candidate bins with log10_evalue <= log10(max_evalue).  Keys whose
 * best bin is at or below that are reported, ordered by (log10_evalue, bin, key) ascending.
 * Families: walking the report in order, a word joins the first earlier family head whose best bin differs by at most 1
 * from its own and to which it is related, else it heads a new family.  Y is related to X iff for some offset o in
 * -2 .. 2, Y laid at o on X has no column where the letters differ and at least 4 columns where they are the same; on both
 * strands Y's reverse complement is tried as well.
 * Only the first `capacity` lines are written to `out`; *n_out is always the full count, so a caller with too small an
 * array calls again.  Nt = 0 reports nothing.  PENGK_ERR_ARG: K, n_bins or both_strands as above, max_evalue not > 0. */
int pengk_position_summary(const uint64_t* h_counts, int K, int n_bins, int both_strands, uint64_t min_count, double max_evalue,
                           pengk_position_word* out, uint64_t capacity, uint64_t* n_out);
/* ---- the composition null of the positional report (--positional-null composition: q[b] above assumes that every bin has
 *      the same composition; where a promoter grows G+C-richer towards its TSS, or a peak towards its summit, a bin lifts
 *      every word made of its own letters.  Here each word's share per bin is tilted by what the bin's letters make of the
 *      word) -- this project's own definitions again, not RSAT's numbers.
 * Pair table.  d_pairs[b * 16 + 4 x + y] (n_bins x 16 uint64, ADDED to, caller-zeroed, as d_counts).  Every position p at
 * which a word stands -- K consecutive valid bases from p on: ALL standing words, not only clump heads -- whose bin
 * b = coordinate(p) / bin_size (the coordinates of pengk_position_count) is < n_bins adds 1 at x = s[p], y = s[p+1] and, with
 * both_strands, 1 more at x = 3 - s[p+K-1], y = 3 - s[p+K-2]: the first pair of the word read on the other strand.  The sum
 * of row b is 1 x / 2 x the standing words of bin b; n1[b][x] = sum_y pairs[b][4 x + y].  The same arguments, argument
 * errors, n_seq = 0 behaviour and stream contract as pengk_position_count. */
int pengk_position_pairs(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                         const uint32_t* d_lens, uint64_t n_seq, int K, int anchor, int bin_size, int n_bins, int both_strands,
                         uint64_t* d_pairs /* n_bins x 16, ADDED to */);
/* Pure CPU.  h_pairs = NULL: pengk_position_summary, byte for byte.  Otherwise the same report with a share q_key[b] of
 * its own for every key in place of q[b]; all of it in fp64, in exactly this order:
 *   T_b[x][y] = (double)(pairs[b][4 x + y] + 1) / (double)(n1[b][x] + 4)        (an n1[b][x] = 0 row: 1/4 each)
 *   f_b[x]    = (double)n1[b][x] / (double)(sum_x n1[b][x])
 *   P_b(w)    = f_b[w_0], then *= T_b[w_i][w_i+1] for i = 0 .. K-2, left to right (w_0 the first base)
 *   with both_strands P_b(key) = P_b(key) + P_b(revcomp(key)); a bin without a pair has P_b = 0
 *   g_b = (double)N[b] * P_b(key);  G = the sum of g_b over b ascending;  q_key[b] = g_b / G
 * A key with G = 0 is skipped (a counted word's first pair lies in its bin, so this happens on constructed tables only).
 * expected = (double)C[key] * q_key[b], log10_pvalue = pengk_binomial_log10_sf(C[key], count, q_key[b]); candidates, the
 * number of tests, the order, the tie-breaks, bins_significant and the families are those of pengk_position_summary.  Where
 * every bin has the same pair frequencies this is the flat null up to rounding.  The same argument errors. */
int pengk_position_summary_null(const uint64_t* h_counts, const uint64_t* h_pairs /* n_bins x 16, or NULL */, int K, int n_bins,
                                int both_strands, uint64_t min_count, double max_evalue, pengk_position_word* out, uint64_t capacity,
                                uint64_t* n_out);

/* ---- motif refinement (--refine: the found motifs re-estimated and extended from their sites, as MEME, HOMER and STREME
 *      end) -------------------------------------------------------------------------------------------
 * Over the scan layout and the best sites of pengk_motif_best_sites.  Integer up to the counts: any slicing, any rank
 * count and a numpy restatement give the same counts; the new matrix is a fixed double-precision formula on them.
 * Both calls clamp the flank per motif: F = min(flank, (PENGK_MAX_MOTIF_LEN - w) / 2), so that w + 2F <=
 * PENGK_MAX_MOTIF_LEN. */
/* Site profiles.  For every motif m (width w = h_len[m], F as above) and every sequence i with a best site (d_best[m *
 * n_seq + i] not PENGK_SCORE_SENTINEL and >= h_thr[m], d_site[m * n_seq + i] = 2p + s with p + w <= d_lens[i]), and every
 * column c in [-F, w + F): the base at that column of the site read on the site's strand -- position p + c on +,
 * position p + w - 1 - c complemented on - -- ADDS 1 to d_counts[(m * PENGK_MAX_MOTIF_LEN + c + F) * 5 + b], b = 0..3 for
 * A, C, G, T and b = 4 where the position lies outside the sequence or holds another letter.  d_counts: n_motifs x
 * PENGK_MAX_MOTIF_LEN x 5 uint64, caller-zeroed, accumulating (slices and shards add up; rows from w + 2F on stay
 * untouched).  d_valid = NULL: every base of a sequence is valid.  flank >= 0. */
int pengk_site_profiles(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                        const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                        const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts);
/* Pure CPU.  One motif's new matrix from its counts (h_counts: the motif's (w + 2F) x 5 rows of d_counts, summed over
 * the ranks), in double, in this order: per column c = 0 .. w + 2F - 1, n = ((k[0] + k[1]) + k[2]) + k[3] (integers); for
 * b = 0, 1, 2, 3 in this order q[c][b] = ((double)k[b] + bg[b]) / ((double)n + 1.0) (bg = h_bg taken as double, all > 0: one
 * pseudocount spread by the background) and IC[c] = sum from 0.0 of q[c][b] * log2(q[c][b] / bg[b]).  The kept range
 * [*first_out, *last_out) runs from the first to the last column with IC >= min_ic (0, 0 when there is none).  h_q ((w +
 * 2F) x 4) and h_ic (w + 2F) receive every column's q and IC, h_pwm (up to PENGK_MAX_MOTIF_LEN x 4) the kept columns'
 * q rounded to float, from row 0 on; sites_out the sequences that had a site (the five bins of column F).  Any of h_q,
 * h_ic, h_pwm, sites_out may be NULL. */
int pengk_profile_refine(const uint64_t* h_counts, int w, int flank, const float* h_bg, double min_ic, double* h_q,
                         double* h_ic, float* h_pwm, int32_t* first_out, int32_t* last_out, uint64_t* sites_out);

/* ---- first-order motif models (--dinuc: whether neighbouring positions of a found motif depend on each other, and what a
 *      model that knows it gains; the first step towards the higher-order models BaMMmotif learns from this tool's PWMs;
 *      INTEGRATION.md 7i) ------------------------------------------------------------------------------------------------
 * Over the scan layout and the best sites of pengk_motif_best_sites.  Integer up to the counts and again from the
 * integer log-odds on: any slicing, any rank count and a numpy restatement give the same counts and the same scores; the
 * model between them is a fixed double-precision formula.  F = min(flank, (PENGK_MAX_MOTIF_LEN - w) / 2) as above. */
/* Pair profiles: pengk_site_profiles for adjacent pairs.  The same arguments and the same sites.  For every column c in
 * (-F, w + F), with a the letter at column c - 1 and b the letter at column c, both read on the site's strand exactly as
 * pengk_site_profiles reads them: ADDS 1 to d_counts[(m * PENGK_MAX_MOTIF_LEN + c + F) * 17 + 4a + b], or to bin 16 of
 * that row when either position lies outside the sequence or holds another letter.  d_counts: n_motifs x
 * PENGK_MAX_MOTIF_LEN x 17 uint64, caller-zeroed, accumulating; row 0 of a motif and the rows from w + 2F on stay
 * untouched.  d_valid = NULL: every base of a sequence is valid. */
int pengk_site_pair_profiles(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                             const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                             const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts);
/* Pure CPU.  One motif's first-order model from its counts: h_counts1 the motif's W x 5 rows of pengk_site_profiles,
 * h_counts2 its W x 17 rows of pengk_site_pair_profiles (same flank, summed over the ranks), W = w + 2F.  h_bg0 (4) and
 * h_bg1 (16, bg1[4a + b] = P(b | a)) are taken as double and must be > 0; alpha > 0.  In double, in this order, per
 * column c = 0 .. W - 1:
 *   n1 = ((k1[0] + k1[1]) + k1[2]) + k1[3] (integers);  q0[c][b] = ((double)k1[b] + bg0[b]) / ((double)n1 + 1.0), b = 0..3
 *   row[a] = ((k2[4a] + k2[4a+1]) + k2[4a+2]) + k2[4a+3],  col[b] = ((k2[b] + k2[4+b]) + k2[8+b]) + k2[12+b] (integers)
 *   q1[c][4a+b] = ((double)k2[4a+b] + alpha * q0[c][b]) / ((double)row[a] + alpha) for c >= 1; q1[0][4a+b] = q0[0][b]
 *   mi[c], c >= 1, N = ((row[0] + row[1]) + row[2]) + row[3]: the sum from 0.0 over a = 0..3, then b = 0..3, of the cells
 *     with k = k2[4a+b] > 0 of ((double)k / (double)N) * log2(((double)k * (double)N) / ((double)row[a] * (double)col[b]));
 *     0 when N = 0; mi[0] = 0
 * and the integer log-odds lo(p, g) = clamp(lround(100 * log2(p / g)), -2000, 2000):
 *   S0[b] = lo(q0[0][b], bg0[b]);  D1[c][4a+b] = lo(q1[c][4a+b], bg1[4a+b]);  D0[c][4a+b] = lo(q0[c][b], bg1[4a+b]), c >= 1
 *   (row 0 of D1 and D0 is written as 0).  D0 is the zeroth-order motif over the same first-order background: scored
 *   with D0 and with D1, the two results differ only by the motif's dependencies.
 * h_q0 (W x 4), h_q1 (W x 16), h_mi (W), h_S0 (4), h_D1 and h_D0 (W x 16 each), sites_out (the five bins of column F of
 * h_counts1) may each be NULL. */
int pengk_dinuc_model(const uint64_t* h_counts1, const uint64_t* h_counts2, int w, int flank, const float* h_bg0,
                      const float* h_bg1, double alpha, double* h_q0, double* h_q1, double* h_mi, int32_t* h_S0, int32_t* h_D1,
                      int32_t* h_D0, uint64_t* sites_out);
/* pengk_motif_scan for first-order models.  h_S0 = n_motifs x 4, h_D = n_motifs x PENGK_MAX_MOTIF_LEN x 16 int32 (row 0
 * and the rows from h_len[m] on unused), every used entry in [-2000, 2000], 1 <= h_len[m] <= PENGK_MAX_MOTIF_LEN.  A
 * window x_0 .. x_{w-1} whose bases are all valid scores S0[x_0] + sum over c = 1 .. w - 1 of D[c][4 x_{c-1} + x_c]; with
 * both_strands also the same formula on y_j = 3 - x_{w-1-j}.  d_best[m * n_seq + i] = the maximum over windows and
 * strands, PENGK_SCORE_SENTINEL without such a window.  With D[c][4a + b] = S[c][b] and S0 = S[0] the result is
 * pengk_motif_scan's, bit for bit.  The other arguments as pengk_motif_scan.  Best scores only: sites, p-values and
 * re-estimation under a first-order model are not provided. */
int pengk_motif_scan_dinuc(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S0, const int32_t* h_D,
                           const int32_t* h_len, int both_strands, int32_t* d_best);

/* ---- motif pair spacing (--spacing: which pairs of found motifs occur in the same sequences more often than chance, and
 *      whether they keep a fixed distance and orientation there; SpaMo's spacing histograms and binomial test, INTEGRATION.md
 *      7g) ------------------------------------------------------------------------------------------------------------------
 * Over the best sites of pengk_motif_best_sites.  Integer up to the summary: any slicing, any rank count and a numpy
 * restatement give the same histograms. */
#define PENGK_SPACING_MAX_MOTIFS 64
#define PENGK_SPACING_MAX_GAP 1024
/* Replaces SpaMo's per-sequence pairing of a primary and a secondary site.  The considered sequences are those with
 * min_len <= L <= max_len (L = d_lens[i]; min_len at least every width, 1 <= max_len <= PENGK_CENTRALITY_MAX_LEN).  Motif m
 * has a site in a considered sequence when its best score (d_best, d_site = 2p + s from pengk_motif_best_sites) is not
 * PENGK_SCORE_SENTINEL, is >= h_thr[m] and p <= L - h_len[m]: ADDS 1 to d_hist_motifs[m].  For every pair a < b (pair
 * index q = b (b - 1) / 2 + a) with sites (p_a, s_a), (p_b, s_b) in one sequence, with G = max_gap and B = 4 (G + 1) + 2
 * bins per pair, ADDS 1 to d_hist_gaps[q * B + bin]:
 *   the intervals [p_a, p_a + w_a) and [p_b, p_b + w_b) intersect                                bin 4 (G + 1)
 *   else side = 0, g = p_b - p_a - w_a when p_b >= p_a + w_a; side = 1, g = p_a - p_b - w_b otherwise;
 *   c = 2 (s_a ^ s_b) + (side ^ s_a)  (b on the other strand than a; b upstream of a read on a's strand)
 *   g <= G: bin c (G + 1) + g;   g > G ("far"): bin 4 (G + 1) + 1
 * and, unless they intersect, 1 to d_hist_lengths[q * (max_len + 1) + L].  Reverse-complementing a sequence changes no
 * bin.  All three arrays uint64, caller-zeroed: slices and shards sum exactly.  n_seq = 0 or n_motifs = 0 does nothing;
 * n_motifs = 1 fills d_hist_motifs only (the other two may be NULL).  At most PENGK_SPACING_MAX_MOTIFS motifs, max_gap
 * <= PENGK_SPACING_MAX_GAP. */
int pengk_spacing_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                             const uint32_t* d_lens, uint64_t n_seq, const int32_t* h_len, const int32_t* h_thr,
                             uint32_t max_gap, uint32_t min_len, uint32_t max_len,
                             uint64_t* d_hist_gaps,    /* pairs x B */
                             uint64_t* d_hist_lengths, /* pairs x (max_len + 1) */
                             uint64_t* d_hist_motifs); /* n_motifs: n_m */
typedef struct {
  uint64_t both;            /* sequences with a site of either motif: overlapping + apart */
  uint64_t overlapping;
  uint64_t apart;           /* Na: not overlapping, far included */
  uint64_t far;             /* of those: gap > max_gap */
  double expected_both;     /* n * (n_a / n) * (n_b / n) */
  double log10_pvalue_both; /* log10 P(X >= both), X ~ Binomial(n, (n_a / n) (n_b / n)) */
  uint32_t orientation;     /* c of the reported bin: 0 same_downstream, 1 same_upstream, 2 opposite_downstream,
                               3 opposite_upstream */
  uint32_t gap;             /* g of the reported bin */
  uint64_t count;           /* its sequences */
  double expected;          /* Na * p(g) */
  double log10_pvalue;      /* log10 P(X >= count), X ~ Binomial(Na, p(g)) */
  double log10_evalue;      /* log10_pvalue + log10(n_classes * tested_gaps) + log10(n_pairs) */
  uint32_t tested_gaps;     /* #{g <= max_gap : p(g) > 0}; 0: no bin was tested (Na = 0) and the six fields above are 0 */
} pengk_spacing;
/* Pure CPU.  Replaces SpaMo's binomial test.  One pair's test from its two histograms (h_gaps: B bins, h_lengths:
 * max_len + 1 bins, as above, summed over the ranks), the widths, n_classes (2 with + scored only: c = 0, 1; else 4), the
 * considered sequences n, those with a site of a and of b, and the pairs of the run (the Bonferroni factor).
 * Co-occurrence: the margins taken as known rates, p_co = ((double)n_a / (double)n) * ((double)n_b / (double)n) -- an
 * approximation (the exact test with fixed margins is hypergeometric).
 * Gap: conditioned on the Na sequences where the two are apart.  Under independent uniform placement every (side, gap) of
 * a sequence of length L has k(L, g) = max(0, L - w_a - w_b - g + 1) placements out of K(L) = T (T + 1) / 2, T = L - w_a -
 * w_b + 1, and the classes are equally likely: p(g) = (1 / Na) * sum over ascending L of n_L * k(L, g) / (n_classes *
 * K(L)), summed in double from 0.0, then one division.  For every c < n_classes and g <= max_gap with p(g) > 0: P(c, g) =
 * P(X >= H[c][g]), X ~ Binomial(Na, p(g)).  Reported: the bin with the smallest log10 P, the smaller c, then the smaller
 * g on ties.  Cost: one pass over the non-zero length bins per tested gap.  PENGK_ERR_ARG when the histograms disagree
 * (different totals of apart sequences, a count in a class >= n_classes, a length below w_a + w_b, more than n_a, n_b). */
int pengk_spacing_summary(const uint64_t* h_gaps /* B */, const uint64_t* h_lengths /* max_len + 1 */,
                          uint32_t max_gap, uint32_t max_len, int w_a, int w_b, int n_classes /* 2 or 4 */,
                          uint64_t n, uint64_t n_a, uint64_t n_b, int n_pairs, pengk_spacing* out);

/* ---- motif comparison (--compare): found motifs against a database of known motifs.  Replaces a Tomtom run on the MEME
 *      output (Gupta et al. 2007), with the Sandelin-Wasserman column score; the definitions below are this project's own
 *      and the numbers are NOT Tomtom's.  tests/motif_compare_model.py restates them in numpy.
 *
 *      Column: a motif row p (4 doubles, any positive scale) becomes X_a = floor(4096 * p_a / s + 0.5), s = ((p_0 + p_1) +
 *      p_2) + p_3, an int16 in [0, 4096].  The reverse complement of a motif reverses its column order and its letter order.
 *      Column score: d = sum_a (X_a - Y_a)^2, s = max(0, 256 - (d >> 17)), an integer in [0, 256] (quantised columns have
 *      d <= 2^25: identical columns score 256, two different pure columns 0; the clamp only meets made-up columns).
 *      Alignments of a query (width wq) and a target (width wt): the target's orientation o is + or, with `both`, - (the
 *      target reverse-complemented); m = min(min_overlap, wq, wt); the offset k = -(wt - m) .. wq - m is the query
 *      coordinate of target column 0; the overlap starts at query column i0 = max(k, 0) and target column j0 = max(-k, 0)
 *      and spans n = min(wq - i0, wt - j0) columns; S is the sum of its n column scores; n_offsets = the number of (o, k).
 *      Null: h_i[v] = the (target, orientation, column) triples of the whole database that score v against query column
 *      i, N their number, pmf_i = h_i / N in double; the null of the overlap [i0, i0 + n) is the convolution of its n
 *      pmfs in double (every term non-negative), p_offset = min(1, P(sum >= S)), and exactly 1 where S does not exceed
 *      the smallest sum the null can give (the sum over the n columns of the lowest v with h_i[v] > 0).  Within one
 *      overlap p_offset never rises with S, whatever the rounding of the sums.
 *      Best alignment of a pair: the smallest p_offset, then the larger overlap, + before -, the smaller k. */
/* Pure CPU.  X[j * 4 + a] of the w rows of h_rows.  PENGK_ERR_ARG: w outside 1..PENGK_MAX_MOTIF_LEN, a negative or NaN
 * entry, a row whose sum is not a positive finite number. */
int pengk_compare_quantize(const double* h_rows /* w x 4 */, int w, int16_t* h_X /* w x 4 */);
/* h_hist[(q * PENGK_MAX_MOTIF_LEN + i) * 257 + v] = h_i[v] of query q (rows at and above its width: zero).  Motifs are
 * n x PENGK_MAX_MOTIF_LEN x 4 int16, only the first h_*len[i] columns are read.  Integer throughout: exact.
 * PENGK_ERR_ARG (naming the function and the argument): n_q or n_t < 1, a width outside 1..PENGK_MAX_MOTIF_LEN, an entry
 * outside [0, 4096].  Synchronises with the host. */
int pengk_compare_nulls(pengk_ctx* ctx, int n_q, const int16_t* h_QX, const int32_t* h_qlen, int n_t, const int16_t* h_TX,
                        const int32_t* h_tlen, int both, uint64_t* h_hist /* n_q x PENGK_MAX_MOTIF_LEN x 257 */);
/* The best alignment of every (query, target): h_align[(q * n_t + t) * 5 ..] = offset, orientation (0 +, 1 -), overlap,
 * score, n_offsets; h_p[q * n_t + t] = its p_offset.  The nulls are rebuilt on the device.  Device memory is bounded:
 * queries go in batches of at most 256 MiB of tabulated tails (a query of width 64 needs 94 MB) and 2^22 records.
 * Errors as pengk_compare_nulls, and PENGK_ERR_ARG for min_overlap < 1.  Synchronises with the host. */
int pengk_compare_motifs(pengk_ctx* ctx, int n_q, const int16_t* h_QX, const int32_t* h_qlen, int n_t, const int16_t* h_TX,
                         const int32_t* h_tlen, int both, int min_overlap, int32_t* h_align /* n_q x n_t x 5 */,
                         double* h_p /* n_q x n_t */);
/* Pure CPU, one query's n_t targets: p_match = -expm1(n_offsets * log1p(-p_offset)), 1 where p_offset is 1; evalue =
 * p_match * n_t; qvalue: Benjamini-Hochberg over the n_t targets -- in ascending p_match (database order on ties) q_(r) =
 * min over r' >= r of p_(r') * n_t / r', at most 1. */
int pengk_compare_summary(const double* h_p /* n_t */, const int32_t* h_noff /* n_t */, int n_t, double* h_p_match,
                          double* h_evalue, double* h_qvalue);
/* Test hook: the whole tail table of ONE query of width w whose null histograms are h_hist (rows i = 0 .. w - 1, N = the
 * sum of row 0), from the kernel, grid, block size and table layout that pengk_compare_motifs uses for a query that is a
 * batch of its own.  h_tails, in the device's order: i0 ascending, then n = 1 .. w - i0, each with 256 n + 1 doubles
 * tail(i0, n)[S] = the p_offset of an overlap [i0, i0 + n) with score S; (i0, n) starts at sum over i0' < i0 of
 * L(w - i0') + L(n - 1), L(m) = 128 m (m + 1) + m, and the table holds sum over i0 of L(w - i0) doubles (w = 64:
 * 11 716 640).  PENGK_ERR_ARG (before the device is touched): a NULL argument, w outside 1..PENGK_MAX_MOTIF_LEN, rows
 * whose sums differ, N = 0 or N > 2^32 (the largest N a database that pengk_compare_nulls accepts can give).
 * Synchronises with the host. */
int pengk_test_compare_tails(pengk_ctx* ctx, int w, const uint64_t* h_hist /* w x 257 */, double* h_tails);

/* Self-test of the division sequence the serial EM's weights kernel uses where a PWM's operand ranges allow (the IEEE
 * division's instructions without its range scaling: csrc/em.hip, lean_div; src/peng.cpp:124-125, 186 are the three
 * divisions of a weight).  4096 x 256 threads draw pairs_per_thread random operand pairs each, keep those inside the
 * guard's domain and compare with the compiler's division bit for bit.  h_out[0] = pairs compared, [1] = pairs that
 * differ (must be 0), [2] = of the compared: pairs with a numerator of zero. */
int pengk_selftest_division(pengk_ctx* ctx, uint64_t seed, uint32_t pairs_per_thread, uint64_t* h_out /* [3] */);

/* ---- C1: the one exchange step of a multi-GPU run (no counterpart in the reference, which is a single
 *      process).  One process per GPU; sequences shard by whole records; every rank counts its shard, then the
 *      count table, ltot and the 84 background counters are summed over the ranks -- exact, because the non-overlap
 *      rule never crosses a sequence boundary (src/base_pattern.cpp:382) -- by ONE grouped RCCL all-reduce over xGMI on
 *      the context's stream.  Afterwards every rank holds the global tables: the sweeps are replicated, the EM splits
 *      the PWM list, pengk_allgather returns the pieces.  librccl is opened on first use.
 *
 *      Rendezvous: either the caller distributes rank 0's id itself (pengk_comm_unique_id + pengk_comm_init, e.g. over
 *      an existing launcher's store), or pengk_comm_init_env reads RANK / WORLD_SIZE / MASTER_ADDR from the launcher
 *      environment (torchrun, mpirun wrappers), opens the process's host channel (below) and hands the id out over it.
 *      With WORLD_SIZE unset or 1 every call below is a no-op that succeeds.
 *
 *      Host channel: what the HOST side of a sharded run has to agree on before any table exists -- every rank reads
 *      only its byte range of the FASTA file (replaces the whole-file pass of src/shared/SequenceSet.cpp:285-447 per
 *      rank), so the number of records, the base counts, the 84 background counters
 *      (src/shared/BackgroundModel.cpp:60-84 -- additive in the counters, not in V) and the reader's warnings are
 *      combined over a star of TCP connections to rank 0 on PENGK_COMM_PORT (default MASTER_PORT + 17), bound to
 *      MASTER_ADDR.  Every socket operation has a deadline of PENGK_COMM_TIMEOUT seconds (default 120) and fails with
 *      PENGK_ERR_DEVICE when a rank is missing; peers are admitted only with their rank and a token derived from the
 *      launcher environment (plus PENGK_COMM_TOKEN, if set).  A rank that fails on its own must exit non-zero: its
 *      peers then fail at their next host-channel call, or are torn down by the launcher.
 *
 *      PENGK_COMM_TRANSPORT=tcp makes pengk_comm_init_env skip RCCL and exchange the tables through host memory over
 *      the host channel: a rehearsal transport for boxes with fewer GPUs than ranks (RCCL cannot put two ranks on one
 *      GPU), never selected automatically. */
int pengk_comm_host_init_env(void);                 /* idempotent; collective over the ranks of the job */
int pengk_comm_host_info(int* rank_out, int* world_out);
int pengk_comm_host_allgather(const void* h_send, void* h_recv, size_t bytes_per_rank);
int pengk_comm_host_allreduce_u64(uint64_t* h_buf, size_t n); /* in-place sum */
int pengk_comm_host_shutdown(void);

#define PENGK_COMM_ID_BYTES 128
int pengk_comm_unique_id(void* id_out /* PENGK_COMM_ID_BYTES */);
int pengk_comm_init(pengk_ctx* ctx, const void* id, int rank, int world);
int pengk_comm_init_env(pengk_ctx* ctx);
int pengk_comm_info(pengk_ctx* ctx, int* rank_out, int* world_out);
/* 1 after a pengk_comm_init / pengk_comm_init_env whose deadline passed: a helper thread of this process is then still inside
 * ncclCommInitRank (which has no deadline of its own, and no communicator yet that ncclCommAbort could be given).  Such a
 * process must leave with _exit(): exit handlers and static destructors of HIP / RCCL under that live thread can crash or
 * hang.  (peng_motif does; csrc/comm.hip.) */
int pengk_comm_init_abandoned(void);
/* ncclGetVersion's code of the librccl this process bound (0 before the first communicator call); libraries that report
 * an API older than NCCL 2.0 are refused when they are loaded. */
int pengk_comm_rccl_version(void);
int pengk_comm_destroy(pengk_ctx* ctx);
/* In-place sum over the ranks of d_counts uint32[4^W] (the global bin bound must stay below 2^32: the caller checks
 * the sum of its shards' pengk_packed.max_bin_bound), d_ltot uint64[1] and, if not NULL, d_bg uint64[84]. */
int pengk_allreduce_tables(pengk_ctx* ctx, int W, uint32_t* d_counts, uint64_t* d_ltot, uint64_t* d_bg_counts);
/* Sums the attached shards' bin bounds (pengk_set_sequences' max_bin_bound) over the ranks and fails with
 * PENGK_ERR_RANGE when a 32-bit bin could overflow globally.  Collective; synchronises with the host. */
int pengk_comm_check_bin_bound(pengk_ctx* ctx);
/* d_recv[r * bytes_per_rank ...) = rank r's d_send[0 .. bytes_per_rank), for every r (ncclAllGather). */
int pengk_allgather(pengk_ctx* ctx, const void* d_send, void* d_recv, size_t bytes_per_rank);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* PENGK_H_ */
