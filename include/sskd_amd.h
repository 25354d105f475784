/*
 * sskd_amd.h — C-ABI of the MI355X (gfx950) embedding-and-search path.
 *
 * This is the drop-in boundary for the hot path of Axionis47/semantic-search-kd:
 * everything its `StudentModel` / `FAISSIndexBuilder` wrappers delegate to
 * sentence-transformers and faiss-cpu is reachable through the entry points
 * below.  The reference has no FFI of its own (it is 100 % Python); each entry
 * point therefore cites the reference call site / third-party call it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add.
 *
 * Conventions (binding):
 *   - plain `extern "C"`, no C++/torch types; pointers + sizes only
 *   - every pointer named `d_*` is a DEVICE pointer (HBM) owned by the caller
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = default stream);
 *     all work is enqueued on it, nothing synchronises, nothing allocates
 *   - every function returns 0 (SSKD_OK) or an SSKD_ERR_* code and never throws;
 *     `sskd_last_error()` gives a thread-local message for the last failure
 *   - scratch memory is caller-provided; `*_workspace_bytes()` sizes it
 *   - the workspace may hold anything on entry (a call initialises every byte it later reads), no byte outside
 *     [d_workspace, d_workspace + the size its `*_workspace_bytes()` reports) is touched, and its contents on return
 *     are unspecified (DESIGN.md "Workspace contract"; tests/test_workspace_contract_gpu.py)
 */
#ifndef SSKD_AMD_H
#define SSKD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSKD_ABI_VERSION 1

#define SSKD_OK 0
#define SSKD_ERR_INVALID 1     /* bad argument (null pointer, bad shape, k < 1 ...) */
#define SSKD_ERR_WORKSPACE 2   /* workspace too small */
#define SSKD_ERR_HIP 3         /* a HIP runtime call / kernel launch failed */
#define SSKD_ERR_UNSUPPORTED 4 /* shape outside what the gfx950 kernels are built for */

/* Embedding width the kernels are specialised for (e5-small-v2: configs/kd.yaml:16,
 * src/config.py:30, scripts/build_faiss_index.py:50). */
#define SSKD_DIM 384
/* Corpus rows per HBM tile (one 32x32x2 f32 MFMA M-block). */
#define SSKD_TILE_ROWS 32
/* Largest k served by ONE scan pass; larger k is served by chained passes. */
#define SSKD_K_PASS 32
/* Largest k accepted by sskd_index_search (schemas.py:12-16 caps k at 100 and
 * rerank_top_k at 200). */
#define SSKD_K_MAX 1024

int sskd_abi_version(void);
const char* sskd_last_error(void);
/* Number of HIP devices visible, or -1; does not initialise a context. */
int sskd_device_count(void);

/* ------------------------------------------------------------------------- *
 * Index storage ("add"):  replaces faiss.normalize_L2 + index.add()
 *   reference: scripts/build_faiss_index.py:55-62 (build_from_parquet),
 *              tests/conftest.py:184-185 (IndexFlatIP(384); index.add(x)),
 *              configs/index.yaml:30 (normalize: true)
 * The index lives in HBM as the plain ROW-MAJOR fp32 matrix (1 536 B per row), zero-padded to a multiple of 32
 * rows ("tile" = 32 consecutive rows: lane l of a scanning wave owns row 32t + (l & 31) and the column half
 * 4 (l >> 5) of every 8-column k-step).  The `d_tiled` / `tiled` names of this API date from rounds 1-3, when the
 * tiles were stored in MFMA-fragment order and the screening sidecar carried a second, row-major fp32 copy; callers
 * treat the buffer as opaque (sskd_index_tiled_bytes, sskd_index_add_rows, sskd_index_get_rows).
 * ------------------------------------------------------------------------- */
int64_t sskd_index_padded_rows(int64_t n_rows);
size_t sskd_index_tiled_bytes(int64_t n_rows);

/* Copy `n_rows` row-major fp32 rows into the index starting at index row
 * `dst_row0` (must be a multiple of 32), optionally L2-normalising each row
 * (x / ||x||_2, rows of zero norm left untouched: faiss.normalize_L2).
 * The last partial tile written is zero-padded. */
int sskd_index_add_rows(const float* d_rows, int64_t n_rows, int normalize,
                        float* d_tiled, int64_t dst_row0, void* stream);

/* Inverse of sskd_index_add_rows (for save(): faiss.write_index equivalent). */
int sskd_index_get_rows(const float* d_tiled, int64_t row0, int64_t n_rows,
                        float* d_rows, void* stream);

/* In-place row L2 normalisation (faiss.normalize_L2 on a query batch). */
int sskd_l2_normalize_rows(float* d_x, int64_t n_rows, int dim, void* stream);

/* ------------------------------------------------------------------------- *
 * Exact inner-product top-k ("search"): replaces faiss index.search()
 *   reference: src/serve/app.py:293-301 (index_builder.search(query_emb, k)),
 *              src/kd/eval.py:86 (np.argsort(scores)[::-1][:k]),
 *              tests/conftest.py:184 (IndexFlatIP)
 * d_queries   : row-major fp32 [nq, 384]
 * d_out_scores: fp32 [nq, k], descending; ties broken by lower id
 * d_out_ids   : int64 [nq, k] = local row + id_offset; when fewer than k rows
 *               exist the tail is (-FLT_MAX, -1) like faiss' heap neutral.
 * Scores are the exact fp32 fma chain of the 32x32x2 f32 MFMA in the column
 * order documented in DESIGN.md (oracle/csrc/oracle.c reproduces it bit for bit).
 * ------------------------------------------------------------------------- */
size_t sskd_index_search_workspace_bytes(int64_t n_rows, int nq, int k);
int sskd_index_search(const float* d_tiled, int64_t n_rows,
                      const float* d_queries, int nq, int k, int64_t id_offset,
                      float* d_out_scores, int64_t* d_out_ids,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* Explicit launch tuning (all zero / NULL = the built-in plan).  The SAME struct must be passed
 * to sskd_index_search_workspace_bytes_ex, sskd_index_search_plan_ex and sskd_index_search_ex:
 * the workspace size depends on it, and there is no process-global (environment) state behind
 * these calls. */
typedef struct sskd_search_tuning {
  int32_t queries_per_block;  /* 0 = auto, else 32 or 64 (B_q of the scan kernel) */
  int32_t target_workgroups;  /* 0 = auto, else the number of workgroups the slicing aims for */
  int32_t pruning_pools;      /* 0 = auto, > 0 force the shared candidate pools on, < 0 off */
} sskd_search_tuning;

size_t sskd_index_search_workspace_bytes_ex(int64_t n_rows, int nq, int k,
                                            const sskd_search_tuning* tuning);
/* sskd_index_search with the tuning struct and two optional hipEvent_t handles (as void*, may be
 * NULL) recorded on `stream` immediately before / after the first scan kernel. */
int sskd_index_search_ex(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                         int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                         void* d_workspace, size_t workspace_bytes, void* stream,
                         const sskd_search_tuning* tuning, void* ev_scan_begin, void* ev_scan_end);

/* sskd_index_search with two optional hipEvent_t handles (as void*, may be NULL)
 * recorded on `stream` immediately before and after the first scan kernel: lets a
 * caller time the dominant kernel in-process (bench.py's roofline). */
int sskd_index_search_profiled(const float* d_tiled, int64_t n_rows,
                               const float* d_queries, int nq, int k, int64_t id_offset,
                               float* d_out_scores, int64_t* d_out_ids,
                               void* d_workspace, size_t workspace_bytes, void* stream,
                               void* ev_scan_begin, void* ev_scan_end);

/* Screened search for batch shapes (k <= 10, nq >= 64, >= 2048 rows): a bf16-MFMA screening pass
 * (16x the fp32 matrix rate) over a bf16 copy of the index, then exact fp32 re-scoring of the
 * candidates inside a PROVED error band, so scores and ids are bit-identical to sskd_index_search's.
 * The band is measured, not assumed: |screen - exact| <= |q~ - q| max|row~| + |q| max|row~ - row| +
 * 1e-4 |q| max(max|row|, max|row~|) (Cauchy-Schwarz on the two bf16 roundings + fp32 accumulation slack), with the
 * query norms taken per query and the row maxima when the sidecar is made; in the worst case (every
 * element on a bf16 tie) that is 2^-7 (1 + 2^-9) |q| max|row|, on random data about 0.42 of it (DESIGN.md 3.1b records
 * the measured figures; tests/test_screen_band_gpu.py holds the band and the sidecar to an fp64 reference).
 * The bf16 copy holds the rows MINUS their mean row (q.mean is the same for every row of a query, so
 * ranking is untouched): on anisotropic embeddings (e5: mean pairwise cosine 0.7-0.8) the centred norms,
 * and with them the band, are 2-2.2x smaller.
 * Every row whose screen score reaches the running bound (a lower bound of the query's k-th best screen
 * score, minus the band) is appended to a per-lane run in the workspace, so the appended set always holds
 * the whole band.  The bound is the minimum of a full pool of K scores of DISTINCT rows: a workgroup whose
 * share of the sample phase lies inside its own slice (slice 0) empties its pool between the two phases, because
 * the same rows are offered again there (round 3 did not, and a row counted twice could lift the bound above
 * the true k-th best score: fixed in round 4, tests/test_screened_gpu.py "count_once" / "topic_sorted").  A query is answered by the exact scan inside the same call only when its band holds
 * more than 256 rows (hundreds of near-duplicates of its neighbours) or one run overflowed (> 32 band rows
 * in one 16-lane group's share of a slice: 4 rows of every 32-row tile a wave takes) - the in-call fallback is sized for every query, so no output row is
 * ever unproven and callers have nothing to check.  d_status (device int[2]): [0] = always 0 (kept for ABI
 * stability), [1] = the number of queries that took the exact fallback (a cost diagnostic).  ev_scan_begin /
 * ev_scan_end bracket the screening launch (a bound-only sample phase over the shard's first rows, then the slices).  d_bf16: the screening sidecar,
 * sskd_index_bf16_bytes(n_rows) bytes filled by sskd_index_make_bf16 from the CURRENT tiled index
 * (re-make it after sskd_index_add_rows): the bf16 tiles of the centred rows (768 B per row) and a 4-KiB
 * block with max |row|^2, max |row~|^2, max |row~ - (row - mean)|^2 and the column sums.  Exact re-scoring
 * reads the fp32 index itself (row-major since round 4: index + sidecar = 1.5x the corpus; rounds 2-3 kept a
 * second fp32 copy in the sidecar, 2.5x).
 * Sidecar layout, a tested contract (tests/test_screen_band_gpu.py, oracle/search.py sidecar_decode):
 *   bytes [0, T x 24576), T = ceil(n_rows / 32): tile t, k-step s (0..23), lane l (0..63), element e (0..7) - the
 *     bf16 at byte ((t x 24 + s) x 64 + l) x 16 + 2 e - holds row 32 t + (l & 31), column 16 s + 8 (l >> 5) + e of
 *     bf16(fl32(row - mean)), mean = fl32(colsum x fl32(1 / n_rows)); rows past n_rows are all-zero bits;
 *   norm block at byte T x 24576, 4096 bytes: int32 words 0..2 = the bit patterns of the three maxima above, in that
 *     order (a row norm that is not finite is stored as +inf), word 3 = the bit pattern of max |element| of the fp32
 *     rows, floats 64..447 = the column sums of the fp32 rows, everything else zero.  The mean row is not stored.
 * Range of the band: a query gets no band, and is answered by the exact scan inside the call, when it or a row norm
 * is not finite, when its largest element is below 2^-96 or the largest corpus element below 2^-40 (an all-zero query
 * or corpus excepted), or when the band itself falls outside [2^-100, 2^100]: there fp32 sums of squares and
 * near-denormal products no longer carry the bound. */
size_t sskd_index_bf16_bytes(int64_t n_rows);
int sskd_index_make_bf16(const float* d_tiled, int64_t n_rows, void* d_bf16, void* stream);
size_t sskd_index_search_screened_workspace_bytes(int64_t n_rows, int nq, int k);
/* launch geometry of the screening pass (roofline accounting): queries per workgroup, corpus passes, slices */
int sskd_index_search_screened_plan(int64_t n_rows, int nq, int k, int* queries_per_block, int* corpus_passes,
                                    int* n_slices);
int sskd_index_search_screened(const float* d_tiled, const void* d_bf16, int64_t n_rows, const float* d_queries,
                               int nq, int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                               int* d_status, void* d_workspace, size_t workspace_bytes, void* stream,
                               void* ev_scan_begin, void* ev_scan_end);

/* Test hook, like sskd_encoder_probe and sskd_generic_op: the error band of every query, d_eps2_out[q] = 2 e(q)
 * (fp32 [nq]), computed by the same set-up launch sskd_index_search_screened opens with and from the same
 * sidecar.  +inf means "no band": the query is answered by the exact scan inside the call.  The launch's other
 * outputs (pruning-bound words, fallback counters, status) go to d_scratch,
 * sskd_index_screen_band_scratch_bytes(nq) bytes.  tests/test_screen_band_gpu.py holds the band, and the sidecar
 * it is made from, to an fp64 reference. */
size_t sskd_index_screen_band_scratch_bytes(int nq);
int sskd_index_screen_band(const void* d_bf16, int64_t n_rows, const float* d_queries, int nq, float* d_eps2_out,
                           void* d_scratch, size_t scratch_bytes, void* stream);

/* Test hooks of the screening kernel's matrix core and pruning bounds (tests/test_screen_mfma16_gpu.py).
 * sskd_index_screen_scores: the raw screen scores - the fp32 accumulators of v_mfma_f32_16x16x32_bf16 over the centred
 * bf16 rows of the sidecar and the bf16-rounded queries - of nq <= 64 queries against every row, through the staging,
 * tile ring and MFMA loop of the screening kernel itself: d_out is fp32 [32 ceil(n_rows / 32)][64], row-major (columns
 * past nq and rows past n_rows are zero).
 * sskd_screen_threshold_roundtrip: the kernel keeps its pruning bounds as fp16, rounded toward -inf when packed (a lower
 * bound only lets more rows through to the exact fp32 test); d_out[i] = that fp16 of d_in[i], widened to fp32: never
 * above d_in[i], -inf below the fp16 range and 65504 above it. */
int sskd_index_screen_scores(const void* d_bf16, int64_t n_rows, const float* d_queries, int nq, float* d_out, void* stream);
int sskd_screen_threshold_roundtrip(const float* d_in, int n, float* d_out, void* stream);

/* Test hooks of the screening kernel's tile claiming (tests/test_screen_tile_claim_gpu.py).
 * sskd_index_search_screened_plan_claims: *claims = 1 when the plan has the waves of the slice phase CLAIM their tiles
 * in chunks from per-slice cursors, 0 when it deals every 12th tile to a wave.
 * sskd_index_search_screened_claim is sskd_index_search_screened_filtered (d_row_mask may be NULL) with that choice
 * as an argument: claim < 0 follows the plan, 0 deals, 1 claims whatever the geometry.  The results do not depend on
 * it; workspace and plan queries are those of sskd_index_search_screened. */
int sskd_index_search_screened_plan_claims(int64_t n_rows, int nq, int k, int* claims);
int sskd_index_search_screened_claim(const float* d_tiled, const void* d_bf16, int64_t n_rows, const float* d_queries,
                                     int nq, int k, int64_t id_offset, const uint32_t* d_row_mask, int claim,
                                     float* d_out_scores, int64_t* d_out_ids, int* d_status, void* d_workspace,
                                     size_t workspace_bytes, void* stream, void* ev_scan_begin, void* ev_scan_end);

/* Test hooks of the screening kernel's bound exchange (tests/test_screen_bound_exchange_gpu.py).
 * A query's pruning bound travels between workgroups as sskd_screen_bucket_count() words per query, bucket (row id mod
 * count) holding the best screen score of its rows as a monotone int32 image (INT32_MIN: empty); the exchanged bound
 * is the k-th largest of a query's words, equal words counted separately - INT32_MIN while fewer than k are filled.
 * sskd_screen_bucket_bound: d_out[q] = that selection over d_in[q][count], by the kernel's own code, for 1 <= k <= 10
 * (the kernel uses k = 10).  A result above the true k-th largest would prune rows of the top k. */
int sskd_screen_bucket_count(void);
int sskd_screen_bucket_bound(const int32_t* d_in, int nq, int k, int32_t* d_out, void* stream);

/* One-pass variant for the online shape (reference: src/serve/app.py:285-301, schemas.py:12-16 -
 * one query, k <= 100, rerank_top_k <= 200).  sskd_index_search serves k > SSKD_K_PASS by chained
 * corpus passes; this entry point scans the corpus ONCE with plain per-lane lists, collects the best
 * k candidates and PROVES them exact where it can: a row is missing from the candidates only if its
 * list was full and it ranks after that list's last entry, so if the k-th best candidate ranks at or
 * before the best such last entry, the result is the exact top k.  *d_inexact (device int) is set
 * to 0 when every query's result is proven, to 1 otherwise - the caller then falls back to
 * sskd_index_search (results are never silently approximate).  Limits: 1 <= nq <= 64,
 * 1 <= k <= 256, n_rows >= 1.  Outputs as sskd_index_search; stream-ordered, no host sync. */
size_t sskd_index_search_onepass_workspace_bytes(int64_t n_rows, int nq, int k);
int sskd_index_search_onepass(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                              int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                              int* d_inexact, void* d_workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------------- *
 * Filtered search: a row allow-mask honoured by every search path
 *   (faiss: SearchParameters(sel=IDSelector...) and, through a mask the caller keeps, remove_ids)
 * Format: a DEVICE uint32 array of sskd_row_mask_words(n_rows) = ceil(n_rows / 32) words; bit (r & 31) of
 * word (r >> 5) set means LOCAL row r may be returned.  Bits at or past n_rows are ignored.  One mask serves
 * every query of a call.
 * The _filtered entry points take the arguments of their unfiltered counterparts plus d_row_mask; a masked row
 * never appears in an output, and the results are bit for bit those of the same search over an index that holds
 * the allowed rows only (ids mapped back).  When fewer than k rows are allowed (none included) the tail is padded
 * exactly as when n_rows < k: (-FLT_MAX, -1).  A NULL d_row_mask means "all rows" and runs the unfiltered kernels.
 * Workspace: the existing *_workspace_bytes queries (and plans) size the filtered calls too - the mask changes
 * neither.  The one-pass proof and the screened path's in-call exact fallback hold as without a mask.
 * ------------------------------------------------------------------------- */
int64_t sskd_row_mask_words(int64_t n_rows);
/* d_flags: one byte per row (uint8 / bool, non-zero = allowed) -> d_mask (every word written) */
int sskd_row_mask_pack(const uint8_t* d_flags, int64_t n_rows, uint32_t* d_mask, void* stream);
/* set (allow != 0) or clear the bits of the n_ids local rows d_rows (int64) with atomic or / and.  Rows outside
 * [0, n_rows) are skipped and counted: *d_bad (device int, zeroed by the call) = how many there were. */
int sskd_row_mask_update(uint32_t* d_mask, int64_t n_rows, const int64_t* d_rows, int64_t n_ids, int allow,
                         int* d_bad, void* stream);
/* d_out = d_a AND d_b (d_out may alias either input) */
int sskd_row_mask_and(const uint32_t* d_a, const uint32_t* d_b, int64_t n_rows, uint32_t* d_out, void* stream);
/* *d_count (device int64) = number of allowed rows among the first n_rows (no pre-zeroing needed) */
int sskd_row_mask_count(const uint32_t* d_mask, int64_t n_rows, int64_t* d_count, void* stream);

int sskd_index_search_filtered(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, int k,
                               int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores,
                               int64_t* d_out_ids, void* d_workspace, size_t workspace_bytes, void* stream,
                               const sskd_search_tuning* tuning, void* ev_scan_begin, void* ev_scan_end);
int sskd_index_search_screened_filtered(const float* d_tiled, const void* d_bf16, int64_t n_rows, const float* d_queries,
                                        int nq, int k, int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores,
                                        int64_t* d_out_ids, int* d_status, void* d_workspace, size_t workspace_bytes,
                                        void* stream, void* ev_scan_begin, void* ev_scan_end);
int sskd_index_search_onepass_filtered(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                                       int k, int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores,
                                       int64_t* d_out_ids, int* d_inexact, void* d_workspace,
                                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Range search (faiss IndexFlatIP::range_search): every allowed row scoring above a per-query threshold
 * Result set of query q: R_q = { allowed local row r : score(q, r) > d_thresholds[q] }, scores in the exact scan's
 * fp32 fma order (bit for bit what sskd_index_search returns).  The comparison is strict (faiss' inner-product
 * rule); -inf (padding, masked rows) and NaN never match, also when the threshold is -inf; a NaN threshold
 * matches nothing.  d_row_mask: NULL = all rows, else the format of "Filtered search" above.
 * Output (CSR, faiss' layout): d_lims [nq + 1] int64, always written and always exact; the results of query q are
 * d_out_scores / d_out_ids [lims[q], lims[q + 1]), ids = row + id_offset, sorted by score descending, then id
 * ascending (faiss leaves this order unspecified; here it is deterministic).
 * Overflow: when lims[nq] > max_results only d_lims is written (the later kernels read the total on the device
 * and exit); nothing is ever written at or past max_results.  The caller compares lims[nq] with max_results.
 * max_results = 0 is a count-only call: d_out_scores / d_out_ids may then be NULL.  n_rows = 0 or nq = 0 writes
 * zero lims.  Stream-ordered, no host sync, allocates nothing.  Arguments are checked before any HIP call:
 * negative nq / max_results / n_rows, NULL lims or inputs, a shard of 2^31 - 64 rows or more
 * (SSKD_ERR_INVALID) and a workspace smaller than sskd_index_range_search_workspace_bytes (SSKD_ERR_WORKSPACE).
 * ------------------------------------------------------------------------- */
size_t sskd_index_range_search_workspace_bytes(int64_t n_rows, int nq, int64_t max_results);
int sskd_index_range_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                            const float* d_thresholds, int64_t id_offset, const uint32_t* d_row_mask, int64_t* d_lims,
                            float* d_out_scores, int64_t* d_out_ids, int64_t max_results, void* d_workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Merge of per-shard range results (the step after the all-gather of a row-sharded range search)
 * Record r (r = 0 .. n_runs-1) starts at d_records + r * sskd_range_record_bytes(nq, cap) and holds
 *   { int64 lims[nq + 1]; int64 ids[cap]; float scores[cap]; padding to 16 B },
 * exactly one shard's sskd_index_range_search output (id_offset = the shard's first global row), padded to the common
 * capacity cap >= every run's lims[nq].  Runs may be empty.  The ids of different runs must be distinct (shards are
 * disjoint): the merge assumes it.
 * Output: bit for bit what one sskd_index_range_search over the union of the shards returns.  d_lims [nq + 1] is the
 * sum of the runs' counts, always written and always exact; query q's segment is the merge of its n_runs sorted
 * segments in the range kernel's order: the monotone integer image of the score descending (so +0.0 ranks before
 * -0.0), then id ascending.  Overflow as sskd_index_range_search: when lims[nq] > max_results only d_lims is written
 * and nothing is written at or past max_results; max_results = 0 is a count-only call and d_out_scores / d_out_ids may
 * then be NULL.  Stream-ordered, no host sync, allocates nothing.  Arguments are checked before any HIP call: n_runs
 * outside [1, 65535], negative nq / cap / max_results, NULL or misaligned (8 B) records, NULL lims, NULL outputs with
 * max_results > 0 (SSKD_ERR_INVALID) and a workspace smaller than sskd_range_merge_workspace_bytes
 * (SSKD_ERR_WORKSPACE).  sskd_range_record_bytes returns 0 for negative sizes.
 * ------------------------------------------------------------------------- */
size_t sskd_range_record_bytes(int nq, int64_t cap);
size_t sskd_range_merge_workspace_bytes(int n_runs, int nq, int64_t max_results);
int sskd_range_merge_packed(const void* d_records, int n_runs, int nq, int64_t cap, int64_t* d_lims,
                            float* d_out_scores, int64_t* d_out_ids, int64_t max_results, void* d_workspace,
                            size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Grouped search: the top-k DISTINCT groups by their best row (MaxSim: a document scores as its best chunk)
 *   reference: src/utils/chunk.py (a text becomes overlapping chunks, chunk_id = "<doc_id>_<n>") and its
 *   maxsim_aggregation (doc score = max over the document's chunks)
 * d_row_group: DEVICE int32 [n_rows], the group number g(r) >= 0 of every local row.  For a query q and the allowed
 * rows (d_row_mask: NULL = all rows, else the format of "Filtered search"):
 *   - the score of group G is max { score(q, r) : r allowed, g(r) = G }, score being the exact scan's fp32 fma chain,
 *     bit for bit the value sskd_index_search returns;
 *   - the representative of G is the row attaining that maximum that ranks first in sskd_index_search's order (score
 *     descending, then lower id);
 *   - a group with no allowed row does not exist for the call.
 * The result is the first k groups in the order of their representatives - equivalently: walk sskd_index_search's full
 * ranking and keep the first row of every group not yet seen.  All-singleton groups reproduce sskd_index_search;
 * masking the best row of a group lowers the group to its next row, it does not drop it.
 * Outputs per query: d_out_scores fp32 [k], d_out_ids int64 [k] (representative row + id_offset), d_out_groups
 * int32 [k] (group numbers are local: id_offset does not shift them); fewer than k groups pad the tail with
 * (-FLT_MAX, -1, -1).  d_out_count int32 [nq] = entries written before the padding.
 * How: the exact row search ranks the best k_rows rows per query into the workspace (k_rows > SSKD_K_PASS through the
 * chained passes), then one wave per query walks that ranking.  The walk is a proof when it found k groups or met
 * the end of the allowed rows.  Otherwise - k_rows ranks held fewer than k groups and rows remain - d_unproved[q] = 1
 * and *d_n_unproved (device int32, zeroed by the call) counts such queries; the d_out_count[q] entries already written
 * are then STILL the exact top-count groups, in order: only what follows them is unknown, and the caller asks again
 * with a larger k_rows (or with those groups' rows masked).  k_rows = (k - 1) * (largest group size) + 1 can never be
 * unproved.  (A query whose allowed rows number exactly k_rows < n_rows is reported unproved although nothing follows:
 * the walk cannot see that; asking again settles it.)
 * Limits: 1 <= k <= k_rows <= SSKD_K_MAX.  Stream-ordered, no host sync, allocates nothing; arguments are checked
 * before any HIP call (SSKD_ERR_INVALID; a workspace smaller than the call needs: SSKD_ERR_WORKSPACE).  The size
 * query is monotone in nq and k_rows and never below sskd_index_search_workspace_bytes(n_rows, nq, k_rows).
 * ------------------------------------------------------------------------- */
size_t sskd_index_search_grouped_workspace_bytes(int64_t n_rows, int nq, int k, int k_rows);
int sskd_index_search_grouped(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, int k, int k_rows,
                              int64_t id_offset, const uint32_t* d_row_mask, const int32_t* d_row_group,
                              float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_groups, int32_t* d_out_count,
                              int32_t* d_unproved, int32_t* d_n_unproved, void* d_workspace, size_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------------- *
 * Compaction: drop the rows a mask clears from HBM and renumber the rest
 *   (faiss: IndexFlat::remove_ids shifts the surviving rows down)
 * d_mask: the format of "Filtered search" (bit set = the row stays); bits at or past n_rows are ignored.
 * sskd_row_mask_rank writes d_word_prefix, DEVICE int64 [sskd_row_mask_words(n_rows) + 1]: entry w = the number of set
 * bits in words 0 .. w-1 (an exclusive prefix sum of popcounts), the last entry = the live count.  The new number of
 * a live row r is
 *     new(r) = d_word_prefix[r >> 5] + popcount(d_mask[r >> 5] & ((1u << (r & 31)) - 1)),
 * which is monotone in r.  One workgroup walks the mask; the call needs no scratch.
 * sskd_index_compact_rows copies every live row of the source matrix to row new(r) of the destination, bit for bit (no
 * arithmetic: NaN, +-0 and denormal patterns survive), zero-fills the destination rows [n_live,
 * sskd_index_padded_rows(n_live)) and writes nothing at or past them; n_live = 0 writes nothing.  d_mask and
 * d_word_prefix are the ones of the rank call for the same n_rows.  The call is OUT OF PLACE: the destination needs
 * sskd_index_tiled_bytes(n_live) bytes that do not overlap the source.  The live count is on the device, so the call
 * refuses (SSKD_ERR_INVALID) what it can see from the host - a destination that starts inside the source's
 * sskd_index_tiled_bytes(n_rows), a source that starts inside the destination's first tile - and a destination placed
 * below the source must end before it: the caller guarantees that.
 * Both: stream-ordered, no host sync, allocate nothing; arguments are checked before any launch (n_rows < 0, a shard
 * of 2^31 - 64 rows or more, NULL pointers: SSKD_ERR_INVALID); n_rows = 0 is a successful no-op that writes nothing.
 * ------------------------------------------------------------------------- */
int sskd_row_mask_rank(const uint32_t* d_mask, int64_t n_rows, int64_t* d_word_prefix, void* stream);
int sskd_index_compact_rows(const float* d_src_tiled, int64_t n_rows, const uint32_t* d_mask,
                            const int64_t* d_word_prefix, float* d_dst_tiled, void* stream);

/* ------------------------------------------------------------------------- *
 * Near-duplicate clusters: the connected components of the self-join's pairs (single linkage), never leaving HBM
 *   (the step between near_duplicates and remove_ids: one row kept per cluster)
 * State, both DEVICE int32 [n_rows]: d_parent (a union-find forest; -1 = the row takes no part) and d_degree (edges per
 * row).  The edges arrive as sskd_index_range_search outputs of a self-join (the queries are stored rows), call by
 * call, in stream order.
 *
 * sskd_dup_init: parent[r] = r for a row that takes part (its bit of d_row_mask is set - the format of "Filtered
 * search" - or d_row_mask is NULL), -1 otherwise; degree[r] = 0.
 *
 * sskd_dup_link: d_lims int64 [nq + 1] / d_ids int64 are one range search's CSR; query q is LOCAL row query_row0 + q.
 * An entry (i, id) is an edge when j = id - id_offset lies in [0, n_rows), j > i (the self-join is symmetric bit for bit:
 * the upper triangle holds every pair once), both rows take part, and the scope rule over d_row_group (DEVICE int32
 * [n_rows], the grouped search's array) holds: scope 0 = every pair, 1 = only pairs of different groups, 2 = only pairs of
 * one group.  Every edge unites the two components and adds 1 to degree[i] and degree[j] (integer atomics: the sums do
 * not depend on the order).  Linking an edge twice leaves the components as they are and counts it twice.
 * Overflow: the kernel reads lims[nq] on the device; when it exceeds max_results (the capacity d_ids was given to the
 * range search with) the arrays are not valid: nothing is linked, nothing is added and *d_overflow (DEVICE int32) is set
 * to 1.  Otherwise *d_overflow is left alone, so one zeroed word per call, read once after the last call, tells which
 * calls must be repeated with more room.  The lims are trusted to be a range search's (ascending from 0); whatever they
 * hold, no entry at or past min(lims[nq], max_results) is read.
 *
 * sskd_dup_labels, after the last link: flattens d_parent so that parent[r] is the SMALLEST row of r's component (-1
 * stays), and writes d_rep int32 [n_rows] = the representative row of r's component (-1 for a row that takes no part):
 * keep 0 ("first") the smallest row, keep 1 ("densest") the row with the largest degree, ties to the smallest row;
 * d_size int32 [n_rows] = the component's size at its smallest row, 0 elsewhere; d_counts int32 [2] = { components, rows
 * taking part }.
 *
 * The larger root is always linked under the smaller one, so every component's final root is its smallest row whatever
 * order the hardware takes the edges in: every output is a pure function of the edge set.  All three: stream-ordered, no
 * host sync, no workspace, allocate nothing; arguments are checked before any launch (negative sizes, a shard of 2^31 - 64
 * rows or more, NULL pointers, query rows outside [0, n_rows), an unknown scope or keep, scope 1 or 2 without groups:
 * SSKD_ERR_INVALID); nq = 0 and n_rows = 0 are successful no-ops (labels then only zeroes d_counts).
 * ------------------------------------------------------------------------- */
int sskd_dup_init(int64_t n_rows, const uint32_t* d_row_mask, int32_t* d_parent, int32_t* d_degree, void* stream);
int sskd_dup_link(const int64_t* d_lims, const int64_t* d_ids, int nq, int64_t max_results, int64_t query_row0,
                  int64_t id_offset, int64_t n_rows, const int32_t* d_row_group, int scope, int32_t* d_parent,
                  int32_t* d_degree, int32_t* d_overflow, void* stream);
int sskd_dup_labels(int64_t n_rows, int32_t* d_parent, const int32_t* d_degree, int keep, int32_t* d_rep, int32_t* d_size,
                    int32_t* d_counts, void* stream);

/* ------------------------------------------------------------------------- *
 * Hard-negative mining over a row ranking (ANCE refresh): the rows that fool the student
 *   reference: ANCEMiner.mine, src/mining/miners.py:232-247 (max positive score, margin rule, stable descending sort,
 *   the first top_k)
 * Inputs per query q: the ranking d_rank_scores / d_rank_ids [nq, search_k] as any of the searches above writes it
 * with id_offset 0 (LOCAL rows, score descending then lower row, padded with id -1), and the query's positives
 * d_pos_rows[d_pos_lims[q] .. d_pos_lims[q + 1]) (DEVICE int64 [nq + 1] / int32, local rows in any order; the caller
 * guarantees d_pos_lims is non-decreasing and ends inside d_pos_rows; d_pos_rows == NULL: no query has positives).
 *   - max_pos = the maximum of score(q, r) over the positives r, score being the fp32 fma chain of the exact scan: bit
 *     for bit the value a search returns for row r.  Positives are labels, not candidates: they are scored whether or
 *     not a row mask or a removal hides them from the search.  No positives: max_pos = 0.0f (the reference's rule).  A
 *     positive outside [0, n_rows) is ignored.
 *   - the walk stops at the first id -1.  A rank is DROPPED when its row is one of the positives, or when d_row_groups
 *     (DEVICE int32 [n_rows], NULL = off) is given and its group equals the group of a positive.
 *   - a rank is KEPT when (double)score >= (double)max_pos - margin, decided in fp64 (the reference's expression under
 *     the NumPy it pins: a float32 score against a Python float).
 *   - the kept ranks are written in rank order, which is the stable descending order the reference sorts into: the
 *     first top_k to d_out_scores fp32 / d_out_ids int64 [nq, top_k] (row + id_offset; id_offset shifts the ids
 *     written, never the positives read), the tail padded with (-FLT_MAX, -1).  d_out_counts int32 [nq] = ALL kept
 *     ranks of the window, before the top_k cut; d_out_max_pos fp32 [nq].
 * One wave per query.  Limits: 1 <= top_k <= search_k <= SSKD_K_MAX; d_queries and d_tiled 16-byte aligned.
 * Stream-ordered, no host sync, no workspace, allocates nothing; arguments are checked before the launch
 * (SSKD_ERR_INVALID); nq = 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
int sskd_index_mine_select(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                           const float* d_rank_scores, const int64_t* d_rank_ids, int search_k,
                           const int64_t* d_pos_lims, const int32_t* d_pos_rows, const int32_t* d_row_groups,
                           double margin, int top_k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                           int32_t* d_out_counts, float* d_out_max_pos, void* stream);

/* ------------------------------------------------------------------------- *
 * Denoising of a ranking: drop the mined candidates that are false negatives (text overlap, teacher score)
 *   reference: configs/kd.yaml `denoising:` (teacher_score_threshold 0.7, text_overlap_threshold 0.8),
 *   docs/guides/hyperparameter-tuning.md:107 (the rule), compute_text_overlap, src/utils/chunk.py:150-182 (the measure)
 * The trigram store is built on the host (semantic-search-kd_amd/denoise.py) and uploaded once: a CSR over set numbers
 * (= corpus rows), d_gram_lims int64 [n_sets + 1] non-decreasing from 0, d_grams uint64 the sets' keys, STRICTLY
 * ascending within a set.  A key is the three code points of one character 3-gram of the lowered, stripped text,
 * (c0 << 42) | (c1 << 21) | c2.  The entry points trust a validated store (as the BM25 postings are trusted); a set
 * holds fewer than 2^31 keys.
 *   jaccard(a, b): inter = |A n B|, uni = |A| + |B| - inter, value = (double)inter / (double)uni - ONE correctly rounded
 *   fp64 division, the bits of Python's `int / int`; exactly 0.0 when either set is empty.  A set number outside
 *   [0, n_sets) is the empty set and never becomes an address.
 *
 * sskd_overlap_pairs: pair i = sets (d_a[i], d_b[i]), DEVICE int32 [n_pairs]; writes d_inter / d_union int32 and
 * d_jaccard fp64 [n_pairs] (union = |A| + |B| for disjoint or empty sets).  One wave per pair, the shorter list
 * searched in the longer.  n_pairs = 0 is a successful no-op.
 *
 * sskd_rank_denoise: the ranking d_rank_scores / d_rank_ids [nq, search_k] has the layout every search writes with
 * id_offset 0 (LOCAL rows = set numbers, padded with id -1); the positives are the CSR sskd_index_mine_select takes
 * (d_pos_rows == NULL: no query has positives); d_aux fp32 [nq, search_k] is aligned with the ranking (the teacher's
 * confidence of each candidate).  Whether a rule is on is decided by its pointer, never by its threshold: d_gram_lims
 * and d_grams both NULL = overlap rule off (giving one of the two is an error), d_aux NULL = teacher rule off; with
 * both off the call copies the window.  Per query, in rank order; the walk stops at the first id -1:
 *   - overlap(rank) = the maximum over the query's positives of jaccard(row, positive); 0.0 without positives or without
 *     a store.  A candidate that is itself a positive has overlap 1.0 (its set is not empty) and goes whenever the
 *     threshold is below 1.
 *   - a rank is DROPPED FOR OVERLAP when overlap > overlap_threshold (strict, in fp64), and DROPPED FOR THE TEACHER
 *     when (double)aux >= aux_threshold (a NaN aux is therefore kept).
 *   - the surviving ranks go to d_out_scores fp32 / d_out_ids int64 [nq, search_k] in their input order, score bits and
 *     ids untouched, the tail padded with (-FLT_MAX, -1): the shape sskd_index_mine_select, sskd_hybrid_fuse and the
 *     re-rankers take.  d_out_aux fp32 [nq, search_k] (NULL ok) carries the survivors' aux values, the tail (and every
 *     entry when d_aux is NULL) NaN.  d_out_counts int32 [nq] = the number of survivors.
 *   - d_out_overlap fp64 / d_out_reason uint8 [nq, search_k] (NULL ok) are aligned with the INPUT ranks: the overlap and
 *     a bit set (1 = overlap, 2 = teacher); past the walk's end they hold 0.0 and 0.
 * One workgroup of 256 threads per query (40 KiB of LDS).  Limits: 1 <= search_k <= SSKD_K_MAX; a threshold whose rule is
 * on must not be NaN; the outputs must not overlap the inputs.  Stream-ordered, no host sync, no workspace, allocates
 * nothing; arguments are checked before the launch (SSKD_ERR_INVALID); nq = 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
int sskd_overlap_pairs(const int64_t* d_gram_lims, const uint64_t* d_grams, int64_t n_sets,
                       const int32_t* d_a, const int32_t* d_b, int64_t n_pairs,
                       int32_t* d_inter, int32_t* d_union, double* d_jaccard, void* stream);

int sskd_rank_denoise(const int64_t* d_gram_lims, const uint64_t* d_grams, int64_t n_sets,
                      const float* d_rank_scores, const int64_t* d_rank_ids, int nq, int search_k,
                      const int64_t* d_pos_lims, const int32_t* d_pos_rows,
                      const float* d_aux, double aux_threshold, double overlap_threshold,
                      float* d_out_scores, int64_t* d_out_ids, float* d_out_aux, int32_t* d_out_counts,
                      double* d_out_overlap, uint8_t* d_out_reason, void* stream);

/* ------------------------------------------------------------------------- *
 * BM25 search over an inverted index in HBM (stage 1 of the mining curriculum)
 *   reference: BM25Index.search, src/data/bm25.py:162-192, over rank_bm25.BM25Okapi.get_scores
 * The index is built on the host (semantic-search-kd_amd/bm25.py) and uploaded once: postings in CSR by term id,
 * d_term_offsets int64 [n_terms + 1], each list ascending by row, posting i = (d_post_rows[i] int32, d_post_w[i] fp64)
 * with w = f (k1 + 1) / (f + k1 (1 - b + b dl / avgdl)) evaluated at build time, and d_idf fp64 [n_terms] (negative
 * idfs already replaced by epsilon * average_idf).  Queries are a CSR of term ids: d_q_lims int64 [nq + 1] (non-
 * decreasing), d_q_terms int32 in query order, repeats kept, out-of-vocabulary tokens dropped by the host (they add
 * nothing, so dropping them is exact); a term id outside [0, n_terms) is skipped.  An empty query is legal.
 *   score(q, row) = the fp64 sum, in query-token order, of idf[t] * w(t, row) over the tokens whose list holds the row:
 *   the product rounded, then the sum rounded (no fma), starting from +0.0 - the bits of `score += idf * w_array`.
 *   Result per query: the best k rows under (score descending, row ascending), rows matching no token included with
 *   +0.0, to d_out_scores fp64 [nq][k] / d_out_ids int64 [nq][k]; slots past n_rows hold (-inf, -1).
 * Two kernels per chunk of queries: one workgroup per (tile of rows, query) scores term at a time into LDS and selects
 * the tile's best min(k, rows) into the workspace; one workgroup per query merges the tiles' records.  Nothing of size
 * n_rows x nq exists: the workspace holds queries_per_chunk x tiles x k records of 16 bytes, and the search runs
 * floor(workspace_bytes / bytes of one query) queries per chunk, so any workspace that holds one query is accepted
 * (less: SSKD_ERR_WORKSPACE).  sskd_bm25_search_workspace_bytes is what keeps the whole batch in one chunk up to a
 * 256 MiB budget (0 for nq = 0 or arguments the search rejects); sskd_bm25_search_plan reports the tile size in rows,
 * the number of tiles and the queries per chunk under that size (any out pointer may be NULL).
 * Limits: 1 <= k <= 256; n_rows < 2^31 - 64 (rows are int32 per index); workspace 16-byte aligned.  Stream-ordered, no
 * host sync, allocates nothing; arguments are checked before the first launch (SSKD_ERR_INVALID); nq = 0 is a
 * successful no-op.
 * ------------------------------------------------------------------------- */
size_t sskd_bm25_search_workspace_bytes(int64_t n_rows, int nq, int k);
int sskd_bm25_search_plan(int64_t n_rows, int nq, int k, int* tile_rows, int* tiles, int* queries_per_chunk);
int sskd_bm25_search(const int64_t* d_term_offsets, const int32_t* d_post_rows, const double* d_post_w,
                     const double* d_idf, int64_t n_rows, int64_t n_terms, const int64_t* d_q_lims,
                     const int32_t* d_q_terms, int nq, int k, double* d_out_scores, int64_t* d_out_ids,
                     void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Hybrid fusion: one dense ranking and one BM25 ranking per query joined into one (rrf / linear)
 *   reference: the hybrid block of configs/service.yaml:43-49 (bm25_weight, semantic_weight, fusion_method "rrf" |
 *   "linear"); the reference has no code behind those keys, so the rule below is this library's definition.
 * Inputs per query q: the dense ranking d_dense_scores fp32 / d_dense_ids int64 [nq, kd] as the searches above write it
 * with id_offset 0 (LOCAL rows, score descending then lower row, padded with id -1), and the BM25 ranking
 * d_bm25_scores fp64 / d_bm25_ids int64 [nq, kb] as sskd_bm25_search writes it (padded with (-inf, -1)).  Both number
 * the same rows 0 .. n_rows - 1, and a list holds a row at most once.
 *   - candidates: a dense entry unless its id is -1 or outside [0, n_rows); a BM25 entry unless its id is -1 or outside
 *     [0, n_rows), its score is exactly +0.0 or -0.0 (the row matched no query word: sskd_bm25_search returns such rows
 *     only to fill k), or d_mask (DEVICE allow-mask words as in "Row filters", NULL = off) clears its row.  Each walk
 *     stops at the first id -1.  Ranks are the 1-based positions among the surviving entries of each list, so a mask
 *     gives the ranks a BM25 search over the allowed rows alone would give.  The dense side is expected to have been
 *     searched under the same mask.
 *   - the union holds one entry per distinct row (at most kd + kb <= 512).
 *   - method 0, rrf: fused = w_semantic * (1.0 / (rrf_k + rank_s)) + w_bm25 * (1.0 / (rrf_k + rank_b)); a side the row
 *     is absent from contributes exactly +0.0.
 *   - method 1, linear: first every union row gets both scores.  A row the dense list lacks is scored against
 *     d_queries[q] (the PREPARED query: normalised when the metric is cosine, the tensor the search used) with the fp32
 *     fma chain of the exact scan - the bits a search returns for that row, as in sskd_index_mine_select.  A row the
 *     BM25 list lacks is scored as sskd_bm25_search scores it: over d_q_terms[d_q_lims[q] .. d_q_lims[q + 1]) in query
 *     order, repeats included, from +0.0, adding idf[t] * w(t, row) for every token whose posting list holds the row
 *     (product rounded, then the sum; a term id outside [0, n_terms) is skipped; the lists ascend by row, so the lookup
 *     is a binary search per (token, row)).  Then ns = (s - s_min) / (s_max - s_min) over the union, s widened to fp64,
 *     ns = 0.0 for every row when s_max == s_min; nb likewise over the BM25 scores; fused = w_semantic * ns +
 *     w_bm25 * nb.  (Where +0.0 and -0.0 both occur, -0.0 is the minimum and +0.0 the maximum.)
 *   - all fusion arithmetic is fp64; every division, product and sum is rounded once (no fma).
 *   - output: the best k of the union under (fused descending, row ascending) to d_out_scores fp64 / d_out_ids int64
 *     [nq, k] (row + id_offset), the tail padded with (-inf, -1); d_out_counts int32 [nq] = the union's size before the
 *     cut.  Optional per-result components d_out_dense fp32 / d_out_bm25 fp64 [nq, k] (either may be NULL): the row's
 *     dense and BM25 score; under rrf a side the row was absent from is a quiet NaN, linear always has both; the
 *     padded tail is NaN.
 * Queries, scores and index tables are finite: the call does not check that (it never synchronises).
 * One workgroup of 256 threads per query, the union in LDS.  Limits: 1 <= kd, kb <= SSKD_K_MAX with kd + kb <= 512;
 * 1 <= k <= kd + kb; rrf_k > 0; both weights finite and >= 0; method 0 or 1; n_rows < 2^31 - 64.  Under rrf nothing is
 * completed and the index-side pointers (d_tiled, d_queries, the postings, d_idf, d_q_lims, d_q_terms) may be NULL;
 * under linear they are required, d_tiled and d_queries 16-byte aligned.  Stream-ordered, no host sync, no workspace,
 * allocates nothing; arguments are checked before the launch (SSKD_ERR_INVALID); nq = 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
int sskd_hybrid_fuse(const float* d_tiled, int64_t n_rows, const float* d_queries, const float* d_dense_scores,
                     const int64_t* d_dense_ids, int kd, const int64_t* d_term_offsets, const int32_t* d_post_rows,
                     const double* d_post_w, const double* d_idf, int64_t n_terms, const int64_t* d_q_lims,
                     const int32_t* d_q_terms, const double* d_bm25_scores, const int64_t* d_bm25_ids, int kb,
                     const uint32_t* d_mask, int method, double w_semantic, double w_bm25, double rrf_k, int nq, int k,
                     int64_t id_offset, double* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts,
                     float* d_out_dense, double* d_out_bm25, void* stream);

/* ------------------------------------------------------------------------- *
 * Query expansion: pseudo-relevance feedback between a first search and a second one (Rocchio, RM3)
 *   reference: features.enable_query_expansion of configs/service.yaml:108-113 (.env.example:
 *   ENABLE_QUERY_EXPANSION), a flag the reference reads and has no code behind.  The two rules below are this
 *   library's definition.
 *
 * sskd_prf_rocchio, the dense side.  Inputs per query q: the PREPARED query d_queries[q] (fp32 [384], the tensor the
 * first search used) and its ranking d_rank_scores fp32 / d_rank_ids int64 [nq, kd] as any search above writes it with
 * id_offset 0 (LOCAL rows, padded with id -1).
 *   - feedback rows: the first fb_docs entries of the ranking up to the first id -1, ids outside [0, n_rows) skipped;
 *     m = how many remain.  m == 0: the output row is the input row bit for bit.
 *   - weights, fp32.  weighting 0 (uniform): b_i = beta / (float)m.  weighting 1 (score): s+_i = s_i when s_i > 0, else
 *     +0.0f; S = the s+_i summed in rank order from +0.0f; S == 0: the uniform weights; else b_i = beta * (s+_i / S)
 *     (the division rounded, then the product).
 *   - per column c: acc = alpha * q[c], then in rank order acc = acc + b_i * row_i[c]; every product and every sum is
 *     rounded once (no fma).  d_out_queries fp32 [nq, 384] = acc, NOT normalised: the second search prepares it as it
 *     prepares any query (sskd_l2_normalize_rows under the cosine metric).  d_out_counts int32 [nq] = m.
 * One wave per query; rows are read whole (1 536 bytes, 16-byte loads).  Limits: 1 <= fb_docs <= kd <= SSKD_K_MAX;
 * alpha and beta finite and >= 0; weighting 0 or 1; n_rows < 2^31 - 64; d_tiled, d_queries and d_out_queries 16-byte
 * aligned; d_out_queries may not overlap d_queries.  Scores, queries and rows are finite: the call does not check that.
 *
 * sskd_prf_rm3, the lexical side, over the BM25 index of "BM25 search" plus a FORWARD INDEX built on the host
 * (semantic-search-kd_amd/bm25.py): CSR by row, d_fwd_lims int64 [n_rows + 1], entry i = (d_fwd_terms[i] int32,
 * d_fwd_p[i] fp64) with p = tf / dl in fp64 (tf = occurrences of the term in the row, dl = the row's full token count);
 * n_fwd = the number of entries.  A row keeps at most SSKD_RM3_ROW_TERMS distinct terms, the largest tf first, ties to
 * the lower term id, stored ascending by term id; a term occurs at most once per row.
 *   - feedback rows: walk the BM25 ranking d_rank_scores fp64 / d_rank_ids int64 [nq, kb] (as sskd_bm25_search writes it)
 *     up to the first id -1, skipping ids outside [0, n_rows), scores equal to 0.0 of either sign and rows that d_mask
 *     (DEVICE allow-mask words as in "Row filters", NULL = off) clears - the candidate rule of sskd_hybrid_fuse.  The
 *     first fb_docs survivors are the feedback rows; d_out_fb int32 [nq] = how many there are.
 *   - term weights, fp64, every operation rounded once: S = the feedback rows' scores summed in rank order from +0.0;
 *     P_d = s_d / S;  w(t) = the sum over the feedback rows that hold t, in rank order, from +0.0, of p(t, d) * P_d.
 *     (S == 0 or a non-finite score: the call is safe and what it selects is unspecified.)
 *   - candidates: a term of a feedback row with an id in [0, n_terms) that is not among the query's own tokens
 *     d_q_terms[d_q_lims[q] .. d_q_lims[q + 1]) and, when max_df > 0, whose document frequency d_term_offsets[t + 1] -
 *     d_term_offsets[t] is <= max_df (max_df = 0: no limit).
 *   - selection: the best fb_terms candidates under (w descending, term id ascending; -0.0 below +0.0).
 *   - output: d_out_terms int32 laid out by d_out_lims int64 [nq + 1]; segment q has exactly orig_repeat * len_q +
 *     fb_terms slots: the query's own token sequence orig_repeat times, the selected terms in selection order, -1 in
 *     every remaining slot.  sskd_bm25_search and sskd_hybrid_fuse skip term ids outside [0, n_terms), so (d_out_lims,
 *     d_out_terms) is a legal query CSR for both as it stands.  Also d_out_sel_terms int32 [nq, fb_terms] (padded with
 *     -1), d_out_sel_w fp64 [nq, fb_terms] (padded with +0.0), d_out_counts int32 [nq] = the number selected.
 *   q_lims and out_lims are given TWICE, as sskd_late_rerank takes its q_lims: on the HOST (validated before the launch:
 *   both start at >= 0, q_lims does not decrease, every segment has the length above) and on the device (read by the
 *   kernel; nothing is copied by the call).
 * One workgroup of 256 threads per query; the term table (8 192 slots: 16 rows x 256 disjoint terms at load factor 1/2,
 * keys and fp64 weights, 96 KiB) lives in LDS; one barrier between feedback rows fixes every sum's order without float
 * atomics.  A malformed forward index cannot make the kernel spin or write outside the table: a row's list is read
 * clamped into [0, n_fwd] and cut to 256 entries, every probe loop is bounded by the table size, and a term that finds
 * no slot is dropped.  Limits: 1 <= fb_docs <= 16; fb_docs <= kb <= 256; 1 <= fb_terms <= 64; 1 <= orig_repeat
 * <= 8; max_df >= 0; n_rows < 2^31 - 64.
 *
 * Both calls: stream-ordered, no host sync (graph-capturable), no workspace, allocate nothing; arguments are checked
 * before the launch (SSKD_ERR_INVALID); nq = 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
#define SSKD_RM3_ROW_TERMS 256
int sskd_prf_rocchio(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, const float* d_rank_scores,
                     const int64_t* d_rank_ids, int kd, int fb_docs, float alpha, float beta, int weighting,
                     float* d_out_queries, int32_t* d_out_counts, void* stream);
int sskd_prf_rm3(const int64_t* d_fwd_lims, const int32_t* d_fwd_terms, const double* d_fwd_p, int64_t n_fwd,
                 const int64_t* d_term_offsets, int64_t n_rows, int64_t n_terms, const int64_t* q_lims,
                 const int64_t* d_q_lims, const int32_t* d_q_terms, const double* d_rank_scores,
                 const int64_t* d_rank_ids, int kb, const uint32_t* d_mask, int nq, int fb_docs, int fb_terms,
                 int orig_repeat, int64_t max_df, const int64_t* out_lims, const int64_t* d_out_lims,
                 int32_t* d_out_terms, int32_t* d_out_sel_terms, double* d_out_sel_w, int32_t* d_out_counts,
                 int32_t* d_out_fb, void* stream);

/* ------------------------------------------------------------------------- *
 * Diversified search: Maximal Marginal Relevance over a first stage's candidates, with a near-duplicate cut-off
 *   Carbonell & Goldstein 1998.  The reference has no such step; the rule below is this library's definition.
 * Inputs per query q: the ranking d_rank_scores fp32 / d_rank_ids int64 [nq, fetch_k] as any dense search above writes it
 * with id_offset 0 (LOCAL rows, padded with id -1).
 *   - candidates: the entries up to the first id -1, ids outside [0, n_rows) skipped, in list order: c_0 .. c_{m-1} with
 *     relevance s_i = the list's score taken as given (not recomputed).  The caller promises that a row occurs at most
 *     once; the call is safe if it does not.
 *   - similarity: sim(i, j) = the fp32 fma chain of the exact scan with row c_i as the row and row c_j as the query
 *     vector - the bits a search for row c_j would return for row c_i, symmetric bit for bit (products commute, the
 *     column order is fixed).  It reads the stored rows (unit rows under the cosine metric), never the query.
 *   - redundancy: every candidate carries red_i, unset at the start.  After a candidate p is selected, every still-alive
 *     i gets red_i = sim(i, p) if red_i is unset or sim(i, p) > red_i (fp32, strict); then, if red_i >= dup_threshold,
 *     the candidate dies: it can never be selected.  dup_threshold = +inf turns the cut-off off.
 *   - value, fp64, every product and the subtraction rounded once (no fma): value_i = a * (double)s_i - b * (double)r_i
 *     with a = lambda, b = 1.0 - lambda, r_i = red_i, or +0.0 while red_i is unset.
 *   - selection: up to k times while a candidate is alive, the alive candidate with the largest value, ties to the
 *     earlier list position, is selected and marked dead; then the redundancy state is updated as above.  (With
 *     lambda > 0 the first selection is therefore candidate c_0.)
 *   - output, in selection order: d_out_scores fp32 [nq, k] = s (padded with -FLT_MAX), d_out_ids int64 [nq, k] = row +
 *     id_offset (padded with -1), d_out_mmr fp64 [nq, k] = the value at selection (padded with -inf; may be NULL),
 *     d_out_red fp32 [nq, k] = r at selection (padded with a quiet NaN; may be NULL), d_out_counts int32 [nq] = how
 *     many were selected.
 * One workgroup of 256 threads per query; candidates, relevance, red and an alive bitmap live in LDS, and a selection
 * costs only the similarities of the selected row to the alive candidates (k * m chains per query, not m * m).  With
 * fetch_k <= 100 every candidate row is held in LDS for the whole call; longer lists go through a 32-row stage.
 * Limits: 1 <= k <= fetch_k <= SSKD_K_MAX; lambda finite and in [0, 1]; dup_threshold not NaN; n_rows < 2^31 - 64;
 * d_tiled 16-byte aligned.  Scores and rows are finite: the call does not check that.  Stream-ordered, no host sync
 * (graph-capturable), no workspace, allocates nothing; arguments are checked before the launch (SSKD_ERR_INVALID);
 * nq = 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
int sskd_mmr_select(const float* d_tiled, int64_t n_rows, const float* d_rank_scores, const int64_t* d_rank_ids, int nq,
                    int fetch_k, double lambda, float dup_threshold, int k, int64_t id_offset, float* d_out_scores,
                    int64_t* d_out_ids, double* d_out_mmr, float* d_out_red, int32_t* d_out_counts, void* stream);

/* ------------------------------------------------------------------------- *
 * Retrieval evaluation: nDCG / MRR / recall / precision per cutoff, and the discordant pairs behind Kendall's tau
 *   reference: ndcg_at_k / mrr_at_k / recall_at_k / precision_at_k / kendall_tau, src/utils/metrics.py:11-157;
 *   KDEvaluator.evaluate_retrieval / _evaluate_model / evaluate_ranking_quality, src/kd/eval.py:42-265
 * Per-cutoff arithmetic (both entry points).  Given a query's grades in rank order g[0 .. n) (int32), its judged grades
 * and up to 8 cutoffs k_c (HOST array `cutoffs` int32 [n_cut], 1 <= n_cut <= 8, strictly increasing, 1 <= k_c <= 256;
 * copied into the launch), with m = min(k_c, n):
 *   - disc[i] = d_discounts[i], a DEVICE fp64 [256] table the caller fills with log2(i + 2).  It is an input so that its
 *     bits are the caller's (NumPy's np.log2 for the reference's results), not the device's log2.
 *   - DCG = sum over i < m of (double)g[i] / disc[i], added in the order np.sum adds a contiguous fp64 vector of length
 *     m <= 256: for m < 8 left to right from 0.0; for 8 <= m <= 128 eight accumulators r[j] = a[j], r[j] += a[i + j] for
 *     i = 8, 16, ... while i + 8 <= m, combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the tail left
 *     to right; for m > 128 the vector is split at h = m/2 - (m/2) % 8, each part summed by this rule, the parts added.
 *   - IDCG, ideal_mode 0 (the reference's): the same sum over the same m retrieved grades sorted descending.
 *     ideal_mode 1 (trec-style): the same sum over the first min(k_c, n_judged) of ALL judged grades sorted descending.
 *   - nDCG = IDCG == 0 ? 0.0 : DCG / IDCG (0.0 for m = 0).  MRR = 1.0 / (i + 1) for the first i < m with g[i] > 0, else
 *     0.0.  recall = hits / n_relevant, hits = the entries with g > 0 among the first m, n_relevant = the judged entries
 *     with grade > 0; 0.0 when n_relevant = 0.  precision = hits / k_c (k_c, not m, as the reference divides).
 *   - all of it fp64, every division and sum rounded once (no fma).
 *   - output: d_out_metrics fp64 [nq, n_cut, 4] = (ndcg, mrr, recall, precision).
 *
 * sskd_eval_judge judges a ranking a search wrote: d_rank_ids int64 [nq, k_rank], 1 <= k_rank <= SSKD_K_MAX; the row of
 * an entry is id - id_offset; the walk stops at the first id -1 (only the first 256 places can reach a cutoff).  The
 * judgements are a CSR: d_rel_lims int64 [nq + 1] non-decreasing with d_rel_lims[nq] <= n_rel, d_rel_rows int32
 * ascending within a query (a row at most once: the lookup is a binary search), d_rel_grades int32 beside them.  A
 * ranked row without a judgement has grade 0.  d_rel_rows == NULL: no query has judgements and every metric is 0.0.
 * A query whose limits are negative, decreasing or beyond n_rel gets NaN metrics and reads nothing.
 *
 * sskd_eval_lists evaluates every query against its OWN candidate list: d_doc_lims int64 [nq + 1] non-decreasing,
 * list q = entries [d_doc_lims[q], d_doc_lims[q + 1]) of the [total]-long arrays, 0 <= length <= 1024.  A query whose
 * limits are negative, decreasing, beyond `total` or longer than 1024 gets NaN metrics; nothing else of it is read or
 * written (lengths the host knows should be checked there).
 *   - scores: d_scores_in fp32 [total] when given (teacher logits, precomputed scores).  When it is NULL they are
 *     computed from d_queries fp32 [nq, dim] and d_docs fp32 [total, dim] (dim a multiple of 8, at most 2048, both
 *     16-byte aligned) with the fp32 fma chain of the exact scan: the bits sskd_similarity returns for the pair.
 *   - the list is ranked by score descending, then lower position within the list (the searches' rule with the position
 *     as the id).  This departs from np.argsort(scores)[::-1] in two places: exactly equal scores (the reversal puts the
 *     HIGHER position first) and NaN, which here ranks below every number, NaNs among themselves by position (the
 *     reversal puts NaN first).  Callers pass finite scores; lists whose order matters should not hold ties.
 *   - d_grades int32 [total] follow their documents; the judged set of a query is its whole list.
 *   - outputs beside the metrics, each optional (NULL): d_out_scores fp32 [total], the scores used; d_out_order int32
 *     [total], at d_doc_lims[q] + r the position within the list of the entry ranked r.
 *   - d_ref_scores fp32 [total] (NULL = off; needs d_out_discordant int64 [nq]): a second score per entry, ranked by the
 *     same rule.  d_out_discordant[q] = the number of unordered pairs of the list that the two rankings order
 *     differently - both are permutations without ties, the count is exact, and Kendall's tau is
 *     (n (n - 1) / 2 - 2 discordant) / (n (n - 1) / 2).  Without d_ref_scores d_out_discordant is not written.
 * One workgroup of 256 threads per query.  Stream-ordered, no host sync, no workspace, allocates nothing; arguments are
 * checked before the launch (SSKD_ERR_INVALID); nq = 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
int sskd_eval_judge(const int64_t* d_rank_ids, int nq, int k_rank, int64_t id_offset, const int64_t* d_rel_lims,
                    const int32_t* d_rel_rows, const int32_t* d_rel_grades, int64_t n_rel, const double* d_discounts,
                    const int32_t* cutoffs, int n_cut, int ideal_mode, double* d_out_metrics, void* stream);
int sskd_eval_lists(const float* d_queries, const float* d_docs, int dim, const float* d_scores_in,
                    const int64_t* d_doc_lims, int64_t total, const int32_t* d_grades, const float* d_ref_scores,
                    const double* d_discounts, const int32_t* cutoffs, int n_cut, int ideal_mode, int nq,
                    double* d_out_metrics, float* d_out_scores, int32_t* d_out_order, int64_t* d_out_discordant,
                    void* stream);

/* ------------------------------------------------------------------------- *
 * IVF index: inverted lists over the flat index, nprobe search with exact scores
 *   reference: the `ivf_pq` index type of configs/index.yaml:4, 13-19 (nlist, nprobe; "for >50M vectors") and its
 *   validation block (recall_threshold 0.97), configs/index.yaml:51-56.  The reference has no code behind the type; the
 *   rules below are this library's definition.  The rows stay fp32 here; the PQ half (m, nbits) is "IVF-PQ" below.
 * Layout.  The rows are the flat index, unchanged and not permuted (d_tiled, row-major fp32 [n_rows, 384]).  The lists
 * are a CSR over row numbers: d_list_offsets DEVICE int64 [nlist + 1] (non-decreasing, from 0 to n_rows), d_list_rows
 * DEVICE int32 [n_rows] (every row once, ascending within a list).  An empty list is two equal offsets.
 *
 * sskd_ivf_search.  d_probe DEVICE int64 [nq, nprobe] holds, per query, the lists to visit, exactly as a top-nprobe
 * search over the centroid rows writes its ids (-1 = none; a number outside [0, nlist) is treated as -1; a list should
 * not repeat).  Bit contract: the result of query q is what sskd_index_search_filtered returns for q under an allow-mask
 * of the rows of its probed lists (AND d_row_mask when given: the format of "Filtered search", NULL = all rows) - every
 * score the fp32 fma chain of the exact scan, order (score descending, then lower id), ids row + id_offset, the tail
 * padded with (-FLT_MAX, -1).  With every list probed it is what sskd_index_search returns.
 *   One workgroup per (part, query): the rows a query probes form one sequence of L_q = the sum of its lists' lengths,
 * part p of P scans positions [p L_q / P, (p + 1) L_q / P) of it, found from a prefix sum over the list lengths, so the
 * split is balanced however skewed the lists are.  Every part writes k (unsorted) records to the workspace and
 * sskd_topk_merge joins them - more than 512 records of a query in two steps (p1 x p2 parts: p1 lists for each of the
 * p2 nq (slot, query) pairs, then p2 lists per query), because that merge is one wave per query.  sskd_ivf_search_plan reports P (and the rows per chunk and the workgroups launched; any
 * out pointer may be NULL) from host-known numbers only - nq, nprobe, k, the longest list, 256 compute units - and
 * sskd_ivf_search_workspace_bytes is the workspace of that plan (0 for arguments the search rejects).  The search is
 * not told the longest list: it runs as many parts as its workspace holds, at most the plan of a list that holds every
 * row, so a workspace of exactly sskd_ivf_search_workspace_bytes(..) runs a plan of that size; any workspace that holds
 * one part is accepted, a smaller one is refused.  The result does not depend on P.
 * Limits: 1 <= k <= 256; 1 <= nprobe <= nlist <= 65 536; nq <= 65 535; id_offset >= 0; n_rows < 2^31 - 64; d_queries,
 * d_tiled and the workspace 16-byte aligned.  Stream-ordered, no host sync (graph-capturable), allocates nothing; every
 * argument is checked before anything is enqueued (SSKD_ERR_INVALID, a short workspace included); nq = 0 is a
 * successful no-op.
 *
 * sskd_ivf_list_sums: the centroid update of the spherical k-means.  d_sums DEVICE fp64 [nlist, 384]: element (l, c) =
 * the sum of column c over the rows of list l, added in CSR order into one fp64 accumulator from +0.0 (each fp32 value
 * widened exactly, each addition rounded once).  One fixed order per element and no atomics: two calls give the same
 * bits.  An empty list gives +0.0 everywhere.  The caller rounds to fp32 and normalises (sskd_l2_normalize_rows).
 * Limits: 0 <= nlist <= 65 536.  Stream-ordered, no host sync, no workspace; nlist = 0 is a successful no-op.
 * ------------------------------------------------------------------------- */
int sskd_ivf_search_plan(int nq, int nprobe, int k, int64_t n_rows, int64_t max_list_rows, int* parts, int* chunk_rows,
                         int* workgroups);
size_t sskd_ivf_search_workspace_bytes(int nq, int nprobe, int k, int64_t n_rows, int64_t max_list_rows);
int sskd_ivf_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, const int64_t* d_probe,
                    int nprobe, const int64_t* d_list_offsets, const int32_t* d_list_rows, int nlist, int k,
                    int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores, int64_t* d_out_ids,
                    void* d_workspace, size_t workspace_bytes, void* stream);
int sskd_ivf_list_sums(const float* d_tiled, int64_t n_rows, const int64_t* d_list_offsets, const int32_t* d_list_rows,
                       int nlist, double* d_sums, void* stream);

/* ------------------------------------------------------------------------- *
 * IVF-PQ: product-quantisation codes over the inverted lists, ADC list scan, exact re-ranking
 *   reference: the `ivf_pq` index type of configs/index.yaml (nlist, nprobe, m: 64, nbits: 8).  PQ decides WHICH rows
 *   of the probed lists are re-scored; every score and order of a refined result is the exact scan's fp32 fma chain.
 * Fixed: dim = 384; nbits = 8 (256 codes per subquantiser); m in {8, 16, 24, 32, 48, 64, 96}; dsub = 384 / m.
 * d_codebooks DEVICE fp32 [m][256][dsub] (cb[j][c][d]); codes are uint8 [rows][m].  The arithmetic is chosen so that
 * every step can be restated bit for bit with sequential IEEE operations:
 *   Residual.  r = row - centroid[list(row)], one fp32 subtraction per element (d_assign DEVICE int64 [n] = the list of
 *     every row, d_centroids fp32 [nlist, 384]; d_assign = NULL: r = row).  For the inner product
 *     <q, row> ~ <q, c_list> + sum_j <q_j, cb[j][code_j]>: the look-up table does not depend on the list and the first
 *     term is the probe's own score.
 *   Encode (sskd_pq_encode).  code[row][j] = argmin over c of sum_d (r_d - cb[j][c][d])^2 over the dsub elements of
 *     subspace j, ties to the lower c; the distance is fp64, summed over d ascending from +0.0, operands widened exactly,
 *     every subtract, multiply and add rounded once and no fma formed.  d_codes DEVICE uint8 [n][m], row order.
 *   Code sums (sskd_pq_code_sums, the k-means update).  d_sums DEVICE fp64 [m][256][dsub]: element (j, c, d) = the sum
 *     of r_d over the rows grouped under code c of subspace j, added in the order d_group_rows lists them into one
 *     accumulator from +0.0 (no atomics: two calls agree bit for bit).  d_group_offsets DEVICE int64 [m][257],
 *     d_group_rows DEVICE int32 [m][n]: per subspace the rows sorted stably by code (ascending row within a code).
 *     d_counts DEVICE int64 [m][256] = the group sizes.  The caller sets the new centroid to fl32(sum / count), the
 *     division in fp64; an empty code (sum +0.0, count 0) keeps its centroid.
 *   LUT (sskd_pq_lut).  lut[q][j][c] = fl32(sum_d (double) q_d (double) cb[j][c][d]), fp64 over d ascending (the
 *     products are exact in fp64).  d_lut DEVICE fp32 [nq][m][256].
 *   ADC score of a row.  s = the probe score of its list (d_probe_scores DEVICE fp32 [nq, nprobe]: the fp32 bits the
 *     coarse search returned beside d_probe), then s = s + lut[j][code_j] for j = 0 .. m - 1, fp32 adds in that order.
 *   Candidates.  The R = refine best probed rows in rank order (ADC score descending, then lower row).  Rows the
 *     allow-mask hides are dropped BEFORE scoring and take no slot.
 *   Result (sskd_pq_search).  refine = R > 0: bit for bit what sskd_index_search_filtered returns for the query under
 *     an allow-mask of its R candidates - scores from the fp32 fma chain of the exact scan, order (score descending,
 *     then lower id), ids row + id_offset, padding (-FLT_MAX, -1).  refine = 0: the top-k by ADC with the ADC scores, in
 *     the same order rule.  d_out_candidates (NULL or DEVICE int64 [nq, R], refine > 0 only) receives the candidate ids
 *     in ADC rank order, -1 padded.  The result does not depend on how the work is split.
 * d_codes_csr DEVICE uint8 [n_rows][m] holds the codes IN CSR ORDER: entry p belongs to row d_list_rows[p], so a list
 * is one contiguous byte range.  One workgroup per (part, query) scans the codes of its positions (partitioned as in
 * sskd_ivf_search) with the query's LUT in LDS and keeps its R (or k) best; one workgroup per query then sorts the
 * partial records, gathers the R candidates' rows, scores them exactly and sorts again.  sskd_pq_search_plan reports
 * the parts, the fewest positions a part is planned for (its code bytes are several times its LUT bytes), the workgroups
 * and the LUT bytes, from host-known numbers only; a query never has more than 4 096 partial records.  The workspace
 * (sskd_pq_search_workspace_bytes; 0 for arguments the search rejects) holds the LUT - 1 KiB m per query, so callers
 * batch a few thousand queries per call - and the records; as with sskd_ivf_search any workspace that holds one part
 * is accepted and a smaller one refused.  The search is not told the longest list: it runs as many parts as its
 * workspace holds, up to the plan of a list that holds every row.  So pass workspace_bytes =
 * sskd_pq_search_workspace_bytes(.., max_list_rows) and no more: a larger figure buys shorter parts than the plan's,
 * each of which still loads the whole LUT first (with nprobe = 1 at 1 M rows, up to 40 parts over a thousand positions).
 * Limits: 1 <= k <= R <= 256 or R = 0; 1 <= nprobe <= nlist <= 65 536; nq <= 65 535; id_offset >= 0; n_rows < 2^31 - 64;
 * d_queries, d_tiled, d_codes_csr and the workspace 16-byte aligned.  Every call is stream-ordered, does no host sync
 * (graph-capturable) and allocates nothing; every argument is checked before anything is enqueued (SSKD_ERR_INVALID, a
 * short workspace included); nq = 0 (n = 0) is a successful no-op.
 * ------------------------------------------------------------------------- */
int sskd_pq_encode(const float* d_rows, int64_t n, const float* d_centroids, const int64_t* d_assign, int nlist,
                   const float* d_codebooks, int m, uint8_t* d_codes, void* stream);
int sskd_pq_code_sums(const float* d_rows, int64_t n, const float* d_centroids, const int64_t* d_assign, int nlist,
                      const int64_t* d_group_offsets, const int32_t* d_group_rows, int m, double* d_sums,
                      int64_t* d_counts, void* stream);
int sskd_pq_lut(const float* d_queries, int nq, const float* d_codebooks, int m, float* d_lut, void* stream);
int sskd_pq_search_plan(int nq, int nprobe, int k, int refine, int m, int64_t n_rows, int64_t max_list_rows, int* parts,
                        int* min_part_rows, int* workgroups, size_t* lut_bytes);
size_t sskd_pq_search_workspace_bytes(int nq, int nprobe, int k, int refine, int m, int64_t n_rows,
                                      int64_t max_list_rows);
int sskd_pq_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, const int64_t* d_probe,
                   const float* d_probe_scores, int nprobe, const int64_t* d_list_offsets, const int32_t* d_list_rows,
                   int nlist, const uint8_t* d_codes_csr, const float* d_codebooks, int m, int k, int refine,
                   int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores, int64_t* d_out_ids,
                   int64_t* d_out_candidates, void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Graph index: a fixed-degree k-NN graph over the flat index, beam search with exact scores
 *   reference: the `hnsw` index type of configs/index.yaml:4-11 (M 32, efConstruction 200, efSearch 64) and its
 *   validation block (recall_threshold 0.97).  This is a single-layer graph, built from exact k-NN lists; the rules
 *   below are this library's definition.  WHICH rows a query scores is approximate; every score is the fp32 fma chain
 *   of the exact scan and every order is (score descending, then lower id).
 * Layout.  The rows are the flat index, unchanged (d_tiled, row-major fp32 [n_rows, 384]).  d_graph DEVICE int32
 * [n_rows, M]: the out-edges of every row, -1 = none.  M even, 4 <= M <= 64.  The search accepts any adjacency: -1,
 * ids outside [0, n_rows), self loops and repeated edges are harmless.
 *
 * Build.  d_knn DEVICE int32 [n_rows, knn_k] holds every row's nearest rows in rank order without the row itself (-1
 * where there are none), M <= knn_k <= 128.  An entry is valid when it is in [0, n_rows) and not the row itself.
 *   sskd_graph_prune.  Let L_u be the list of row u.  The detour count of L_u[j] is the number of i < j, L_u[i] valid,
 *     for which some p < j has L_{L_u[i]}[p] == L_u[j].  d_fwd DEVICE int32 [n_rows, M] = the valid entries of L_u
 *     ordered by (detour count ascending, j ascending), the first M of them, -1 padded.
 *   Reverse edges (the caller's, a stable sort): d_rev DEVICE int32 [n_rows, M / 2], rev[v] = the rows u that have v
 *     among the first M / 2 entries of fwd[u], ordered by (position of v in fwd[u], u), the first M / 2, -1 padded.
 *   sskd_graph_merge.  graph[u] = the first M / 2 entries of fwd[u], then the entries of rev[u], then the remaining
 *     entries of fwd[u]; an entry that is not valid or equals an earlier one is skipped; cut to M, -1 padded.
 *   Both are integer-only and write every element of their output exactly once: two calls give the same bits.
 *
 * Incremental insertion.  n_old rows are linked (d_graph_old [n_old, M]); rows [n_old, n_total) are new, n_new of them.
 * d_knn_new DEVICE int32 [n_new, knn_k]: the lists of the new rows, searched against ALL n_total rows, ids global.
 *   sskd_graph_insert_prune.  sskd_graph_prune's rule for the new rows, where the list N(w) of a neighbour w is
 *     graph_old[w] (width M) for w < n_old and knn_new[w - n_old] (width knn_k) otherwise: the detour count of L[j] is
 *     the number of i < j, L[i] valid, for which some p < min(j, width(N(L[i]))) has N(L[i])[p] == L[j].  d_fwd_new
 *     DEVICE int32 [n_new, M].  With n_old = 0 it is sskd_graph_prune.
 *   Reverse edges (the caller's, one stable sort): incoming[t] = the new rows that name t among the first M / 2 entries
 *     of their fwd_new list, by (position, source), the first M / 2, -1 padded; for new targets and for old ones.
 *   sskd_graph_merge_rows.  sskd_graph_merge for the n_rows rows [row_base, row_base + n_rows) of an index of n_total:
 *     d_fwd / d_incoming / d_graph_rows hold those rows only, ids are global, an entry is valid in [0, n_total) when
 *     it is not row_base + (the row's place).  sskd_graph_merge is this call with row_base = 0, n_total = n_rows.
 *   sskd_graph_link.  d_touched DEVICE int32 [n_touched]: linked rows named by new ones, STRICTLY ascending;
 *     d_incoming DEVICE int32 [n_touched, M / 2]: the row of entry t belongs to d_touched[t].  For u = d_touched[t]:
 *     adj = the valid entries of graph[u] (in [0, n_total), not u, first occurrence only) in order; head = adj[:M / 2]
 *     stays; pool = adj[M / 2:], then the entries of incoming[t] that are valid and neither in adj nor earlier in
 *     incoming[t]; every pool row is scored against row u with the exact scan's fma chain; graph[u] = head, then the
 *     best M - |head| pool rows in rank order, -1 padded.  Rank order here is total: score descending, then lower id, a
 *     NaN score after every number.  d_graph (DEVICE int32 [n_total, M]) is updated IN PLACE, a workgroup reading and
 *     writing its own row only: an entry of d_touched outside [0, n_old), or not greater than the entry before it,
 *     leaves its row as it is, and rows not named are not written.  No float atomics: two calls on equal inputs give
 *     the same bits.  One workgroup of 256 threads per touched row; d_tiled 16-byte aligned.
 *   The three calls take every buffer from the caller: no workspace.  n_new = 0 / n_rows = 0 / n_touched = 0 succeed.
 *
 * sskd_graph_search, per query.  T = the ef best rows scored so far in rank order, whatever the mask says, each with
 * an "expanded" flag; R = the k best scored rows whose bit of d_row_mask is set (NULL: all rows; the format of
 * "Filtered search").  To OFFER a set of rows: drop -1 and ids outside [0, n_rows), score the rest, and for T, and
 * for R among allowed rows, ignore a row the list holds, insert any other, cut the list to its capacity - the top-ef
 * (top-k) of the union under a total order, so the outcome does not depend on the order inside the set.  Procedure:
 * offer the seeds; then, at most max_iterations times: take the first `width` entries of T in rank order that are not
 * expanded (none: stop), mark them, offer the union of their M out-edges.  Result: R in rank order, ids row +
 * id_offset, padded with (-FLT_MAX, -1); d_out_iterations (NULL or DEVICE int32 [nq]) = the iterations that expanded
 * at least one row.  Because the worst entry of T and of R only improves, offering a row again never changes a list:
 * the kernel's visited table is an optimisation and cannot change a bit of the result.
 *   d_seeds DEVICE int64 [nq, n_seeds].  With d_seed_rows = NULL a seed is a row number; otherwise a seed s in
 * [0, n_seed_rows) stands for row d_seed_rows[s] (DEVICE int32), which lets the ids of a search over an entry index
 * be passed as they are.  -1 and anything out of range is no seed; a seed may repeat.
 *   One workgroup of 256 threads per query, its whole state in LDS (sskd_graph_search_plan reports the workgroups,
 * the threads, the LDS bytes of one workgroup - two fit a compute unit - and the rows one iteration offers at most,
 * width * M; any out pointer may be NULL).  There is no workspace: sskd_graph_search_workspace_bytes is 0 for every
 * shape and exists so that callers can size the three index types alike.  One query occupies one compute unit.
 * Limits: 1 <= k <= ef <= 256; 1 <= width <= 8; max_iterations >= 1; 1 <= n_seeds <= 256; id_offset >= 0; n_rows <
 * 2^31 - 64; d_queries and d_tiled 16-byte aligned.  Every call of this section is stream-ordered, does no host sync
 * (graph-capturable) and allocates nothing; every argument is checked before anything is enqueued (SSKD_ERR_INVALID);
 * nq = 0 (n_rows = 0 for the build calls) is a successful no-op.  A query holding NaN returns without fault and its
 * result is unspecified (as built: a NaN score enters neither list, so the query gets padding and 0 iterations).
 * ------------------------------------------------------------------------- */
int sskd_graph_prune(const int32_t* d_knn, int64_t n_rows, int knn_k, int M, int32_t* d_fwd, void* stream);
int sskd_graph_merge(const int32_t* d_fwd, const int32_t* d_rev, int64_t n_rows, int M, int32_t* d_graph, void* stream);
int sskd_graph_insert_prune(const int32_t* d_graph_old, int64_t n_old, const int32_t* d_knn_new, int64_t n_new, int knn_k,
                            int M, int32_t* d_fwd_new, void* stream);
int sskd_graph_merge_rows(const int32_t* d_fwd, const int32_t* d_incoming, int64_t n_rows, int64_t row_base, int64_t n_total,
                          int M, int32_t* d_graph_rows, void* stream);
int sskd_graph_link(const float* d_tiled, int32_t* d_graph, int64_t n_old, int64_t n_total, int M, const int32_t* d_touched,
                    const int32_t* d_incoming, int64_t n_touched, void* stream);
int sskd_graph_search_plan(int nq, int k, int ef, int width, int M, int n_seeds, int* workgroups, int* threads,
                           int* lds_bytes, int* step_rows);
size_t sskd_graph_search_workspace_bytes(int nq, int k, int ef, int width, int M, int n_seeds);
int sskd_graph_search(const float* d_tiled, int64_t n_rows, const int32_t* d_graph, int M, const float* d_queries, int nq,
                      const int64_t* d_seeds, int n_seeds, const int32_t* d_seed_rows, int64_t n_seed_rows, int k, int ef,
                      int width, int max_iterations, int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores,
                      int64_t* d_out_ids, int32_t* d_out_iterations, void* stream);

/* ------------------------------------------------------------------------- *
 * Late interaction: token-level MaxSim re-ranking of a first stage's candidates
 *   reference: features.enable_late_interaction of configs/service.yaml (.env.example: ENABLE_LATE_INTERACTION), a flag
 *   the reference reads and has no code behind.  The rules below are this library's definition.
 * Token store.  d_tokens DEVICE bf16 [n_tokens, 384], one L2-normalised row per real token, in CSR order: the tokens of
 * row r are rows tok_lims[r] .. tok_lims[r + 1] - 1 (d_tok_lims DEVICE int64 [n_rows + 1], ascending from 0).
 *   sskd_late_pack_tokens writes the rows of B texts: d_hidden DEVICE bf16 [B, S, 384] (sskd_encoder_hidden's output),
 * d_lengths DEVICE int32 [B] (real tokens of every text, the attention-masked prefix), d_offsets DEVICE int64 [B] (the
 * store row of every text's first token).  Positions >= the length are neither read nor written, nor is a row outside
 * [0, n_tokens).  Per token, in fp32: columns 8 l .. 8 l + 7 are summed as an fma chain from +0.0 into p_l (l = 0 .. 47,
 * p_48 .. p_63 = +0.0), then for o = 32, 16, 8, 4, 2, 1: p_l = p_l + p_(l xor o); ss = p_0; t = x / max(sqrt(ss), 1e-12)
 * with correctly rounded sqrt and division, rounded to bf16 to nearest even.  One wave per token.
 *
 * sskd_late_rerank.  score(q, c) = sum over the query's tokens i (ascending, sequential fp32 from +0.0) of the max over
 * the document's tokens j of <q_i, d_j>; a dot product is the fp32 accumulation of 384 exact bf16 x bf16 products by 24
 * v_mfma_f32_32x32x16_bf16 from a zero accumulator (columns ascending across instructions; the order inside one
 * instruction is the hardware's).  The bits of score(q, c) depend on the two token lists alone - not on nq, R, k, the
 * candidate's position, its neighbours or the launch geometry.
 *   d_q_tokens DEVICE bf16 [q_lims[nq], 384] with q_lims int64 [nq + 1] given TWICE: q_lims on the HOST (validated: every
 * Tq = q_lims[q + 1] - q_lims[q] in [1, 128], q_lims[0] >= 0) and d_q_lims, the same values on the device (read by the
 * kernel; nothing is copied by the call).  d_candidates DEVICE int64 [nq, R]: global ids as the searches write them
 * (id_offset is subtracted); -1, an id outside the store and a row without tokens are no candidate.  Candidates of one
 * query are expected to be distinct (a repeated id is returned once).
 *   Out: d_out_scores fp32 [nq, k] / d_out_ids int64 [nq, k], score descending, ties by lower id, padded with
 * (-inf, -1); d_out_raw NULL or fp32 [nq, R], every candidate's score in candidate order (-inf = no candidate).  With
 * d_out_raw = NULL the raw scores live in the workspace (sskd_late_rerank_workspace_bytes; otherwise none is needed).
 *   Two launches (sskd_late_rerank_plan reports the first: workgroups, threads, LDS bytes of one, candidates per
 * workgroup): the scores, then one wave per query taking the top-k by the rank-order pick.  Limits: 1 <= Tq <= 128,
 * 1 <= k <= R <= 1024, token matrices 16-byte aligned.  Stream-ordered, no host sync (graph-capturable), allocates
 * nothing; every argument is checked before anything is enqueued (SSKD_ERR_INVALID); nq = 0 is a successful no-op.
 * Non-finite tokens do not fault; what they score is unspecified (a NaN score is never returned in the top-k).
 * ------------------------------------------------------------------------- */
#define SSKD_LATE_TQ_MAX 128
#define SSKD_LATE_R_MAX 1024
int sskd_late_pack_tokens(const void* d_hidden, const int32_t* d_lengths, const int64_t* d_offsets, int B, int S,
                          int64_t n_tokens, void* d_tokens, void* stream);
int sskd_late_rerank_plan(int nq, int max_tq, int R, int k, int* workgroups, int* threads, int* lds_bytes, int* chunk);
size_t sskd_late_rerank_workspace_bytes(int nq, int R);
int sskd_late_rerank(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq, const void* d_tokens,
                     const int64_t* d_tok_lims, int64_t n_rows, int64_t n_tokens, const int64_t* d_candidates, int R, int k,
                     int64_t id_offset, float* d_out_scores, int64_t* d_out_ids, float* d_out_raw, void* d_workspace,
                     size_t workspace_bytes, void* stream);

/* Late interaction: training through MaxSim (the sskd_latet_ entries).  score(q, c) = sum_i max_t <q_i, d_cand[q,c],t> differentiated with respect
 * to both token lists; cand[q, c] names a document of the BATCH (0 .. nd - 1; -1, an id outside the batch and a document
 * without tokens are absent pairs).  Both sides are CSR bf16 [T, 384] with lims as sskd_late_pack_tokens writes them; the
 * query side's lims are given on the host (validated: they run from 0 to n_q_tokens, every Tq in [1, 128]) and on the
 * device.  tq_stride = the batch's largest Tq rounded up to 32 (anything else: SSKD_ERR_INVALID).  Limits per call:
 * R <= 1024, Tq <= 128, dim 384.  Every entry validates the whole call and then enqueues (stream-ordered, no host sync,
 * graph-capturable, allocates nothing); nq = 0 or R = 0 is SSKD_OK with nothing launched.
 *
 * sskd_latet_maxsim_fwd: sskd_late_rerank's score kernel - same geometry, same arithmetic; d_scores fp32 [nq, R] is BIT FOR
 * BIT the d_out_raw of sskd_late_rerank over a store holding the same rows (-inf for an absent pair) - plus
 * d_arg int32 [nq, R, tq_stride]: arg[q, c, i] = the document-relative index t of the token that holds the maximum for
 * query token i, the SMALLEST such t when several dot products are equal; -1 for i >= Tq and for an absent pair.
 *
 * sskd_latet_maxsim_bwd_q: d_dq fp32 [n_q_tokens, 384], dQ[q, i, :] = sum_c g[q, c] * d[cand[q, c], arg[q, c, i], :].
 * sskd_latet_maxsim_bwd_d: d_dd fp32 [n_d_tokens, 384], dD[j, t, :] = sum over the contributions e = (q R + c) tq_stride + i
 *   with cand[q, c] = j and arg[q, c, i] = t of g[q, c] * q[q, i, :].  The caller groups them by destination: d_order
 *   int64 [E = nq R tq_stride] = the contributions stably sorted by key (key = d_lims[j] + t, n_d_tokens for a
 *   contribution with arg < 0), d_seg int64 [n_d_tokens + 1] = the first position of every key in the sorted keys.
 * Arithmetic of both, per column: acc = +0.0f; for the contributions ascending (c for dQ, e for dD) acc = acc + g * x with
 * x the bf16 value widened to fp32, multiply and add rounded SEPARATELY (never an fma).  No atomics: one wave per output
 * row, so the bits do not depend on the launch; a row without contributions is exact zeros.  The g of an absent pair (and
 * of arg < 0) is never read into the arithmetic.  Every output row is written.
 *
 * sskd_latet_pack_tokens_bwd: backward of sskd_late_pack_tokens.  d_hidden / d_lengths / d_offsets / B / S / n_tokens as
 * the pack took them, H must be 384 (else SSKD_ERR_UNSUPPORTED), d_dtok fp32 [n_tokens, 384]; writes d_dhidden bf16
 * [B, S, 384], zeros at positions >= the length.  Per token, fp32: ss and n = max(sqrt(ss), 1e-12) exactly the pack's;
 * y_c = x_c / n (the bf16 rounding of the stored token is straight-through); dot = sum_c g_c y_c in the pack's order
 * (lane chain over columns 8 l .. 8 l + 7 from +0.0 with multiply then add, p_48 .. p_63 = +0.0, xor butterfly 32 .. 1);
 * dh_c = (g_c - y_c * dot) / n with separate multiply, subtract and IEEE division, rounded to bf16 to nearest even. */
int sskd_latet_maxsim_fwd(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq, int64_t n_q_tokens,
                         const void* d_d_tokens, const int64_t* d_d_lims, int64_t nd, int64_t n_d_tokens,
                         const int64_t* d_candidates, int R, float* d_scores, int32_t* d_arg, int tq_stride, void* stream);
int sskd_latet_maxsim_bwd_q(const void* d_d_tokens, const int64_t* d_d_lims, int64_t nd, int64_t n_d_tokens, const int64_t* q_lims,
                           const int64_t* d_q_lims, int nq, int64_t n_q_tokens, const int64_t* d_candidates, int R,
                           const int32_t* d_arg, int tq_stride, const float* d_g, float* d_dq, void* stream);
int sskd_latet_maxsim_bwd_d(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq, int64_t n_q_tokens, int R,
                           int tq_stride, const int64_t* d_order, const int64_t* d_seg, int64_t n_d_tokens, const float* d_g,
                           float* d_dd, void* stream);
int sskd_latet_pack_tokens_bwd(const void* d_hidden, const int32_t* d_lengths, const int64_t* d_offsets, int B, int S, int H,
                              int64_t n_tokens, const float* d_dtok, void* d_dhidden, void* stream);

/* Compressed token store (residual compression as in ColBERTv2 / PLAID).  dim = 384, nbits in {2, 4}, L = 2^nbits.
 * Codec: d_centroids DEVICE bf16 [C, 384] (1 <= C <= 65 536), d_cutoffs DEVICE fp32 [L - 1] ascending, d_weights DEVICE
 * fp32 [L]; all finite.  Store: d_cid int32 [n_tokens], d_scale fp32 [n_tokens], d_codes uint8 [n_tokens, 48 nbits];
 * tok_lims as above.  Per token t with centroid c = centroids[cid], per column d, in fp32:
 *   r = fp32(t_d) - fp32(c_d);  code_d = the number of cutoffs strictly below r (a value on a cutoff falls in the lower
 *   bucket, NaN gives 0);  dec_d = bf16(fp32(c_d) + weights[code_d]) rounded to nearest even - the only value a score sees;
 *   scale = 1 / max(sqrt(ss), 1e-12f), ss the sum of squares of dec in sskd_late_pack_tokens' order, sqrt and division
 *   correctly rounded.
 * Byte order: column d = 16 s + 8 h + e (s < 24, h < 2, e < 8) is position p = 192 h + 8 s + e; position p occupies
 * nbits bits from bit nbits (p mod (8 / nbits)) of byte p / (8 / nbits).
 *   sskd_latec_compress writes store rows [row0, row0 + n) (which must lie inside [0, n_store)) from d_tokens DEVICE bf16
 * [n, 384] and d_assign DEVICE int64 [n] (the centroid of every token; a value outside [0, C) is clamped into it).  One
 * wave per token.
 *   sskd_latec_rerank is sskd_late_rerank over such a store: v_ij = fl32(acc_ij * scale_j) with acc_ij the fp32
 * accumulation of the 384 exact products q_i * dec_j by 24 v_mfma_f32_32x32x16_bf16 from a zero accumulator, score = sum
 * over i ascending (sequential fp32 from +0.0) of max over j of v_ij.  The bits of a score depend on the query's tokens,
 * the document's compressed tokens and the codec alone.  A cid outside [0, C) is read as clamped into it.  Arguments,
 * outputs, limits and the two launches are those of sskd_late_rerank (_plan adds nbits; LDS holds 64 bytes of weights
 * more); query tokens, centroids, cid, scale and codes 16-byte aligned.  Both calls: stream-ordered, no host sync
 * (graph-capturable), nothing allocated, every argument checked before anything is enqueued; n = 0 / nq = 0 succeed. */
#define SSKD_LATE_C_MAX 65536
int sskd_latec_compress(const void* d_tokens, const int64_t* d_assign, int64_t n, const void* d_centroids, int C,
                       const float* d_cutoffs, const float* d_weights, int nbits, int32_t* d_cid, float* d_scale,
                       uint8_t* d_codes, int64_t row0, int64_t n_store, void* stream);
int sskd_latec_rerank_plan(int nq, int max_tq, int R, int k, int nbits, int* workgroups, int* threads, int* lds_bytes,
                                     int* chunk);
size_t sskd_latec_rerank_workspace_bytes(int nq, int R);
int sskd_latec_rerank(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq,
                                const int32_t* d_cid, const float* d_scale, const uint8_t* d_codes, int nbits,
                                const void* d_centroids, int C, const float* d_weights, const int64_t* d_tok_lims, int64_t n_rows,
                                int64_t n_tokens, const int64_t* d_candidates, int R, int k, int64_t id_offset,
                                float* d_out_scores, int64_t* d_out_ids, float* d_out_raw, void* d_workspace,
                                size_t workspace_bytes, void* stream);

/* Candidate generation from the compressed token store (PLAID's first stages).  The store of
 * sskd_latec_rerank plus CENTROID LISTS - d_list_lims DEVICE int64 [C + 1] ascending from 0, d_list_rows DEVICE int32
 * [n_list]: LOCAL row r is in list c exactly when some token of r has centroid c (its cid clamped into [0, C)), every
 * (c, r) pair once, rows ascending inside a list - retrieves by itself:
 *   1. sskd_plaid_centroid_scores: S[c, t] = <centroid_c, q_t> for every query token of the batch, fp32, element (c, t) at
 *      d_S[c * ld + t] (ld >= n_q_tokens): the fp32 accumulation of 384 exact bf16 x bf16 products by 24
 *      v_mfma_f32_32x32x16_bf16 from a zero accumulator.  The bits of S[c, t] depend on the two rows alone.
 *      |S - s64| <= 1.01 * 2 * 384 * 2^-24 |q_t| |centroid_c| against fp64 on the stored bf16 values.
 *   sskd_plaid_candidates, everything below being a function of the bits of S:
 *   2. probes: per query token t, P_t = the first nprobe centroids by (S[c, t] descending, c ascending); NaN and -inf are
 *      never picked (a token may have fewer than nprobe probes);
 *   3. Cand(q) = the rows of the lists of all probes of all tokens of q that d_row_mask allows (the format of "Filtered
 *      search", NULL = all rows) and that lie in [0, n_rows);
 *   4. approx(q, r) = sum over the query's tokens i (ascending, sequential fp32 from +0.0) of the max over ALL tokens j of r
 *      of S[cid_j, t_i] (cid clamped into [0, C); the max is exact, ignores NaN and starts from -inf); a candidate whose
 *      approx is NaN or -inf is dropped;
 *   5. the best R by (approx descending, row ascending): d_cand_ids int64 [nq, R] global ids (row + id_offset) padded with
 *      -1, d_cand_scores fp32 [nq, R] padded with -inf, d_n_cand int32 [nq] = |Cand(q)| before the drop and the cut.
 * d_cand_ids is what sskd_latec_rerank takes as d_candidates.  q_lims / d_q_lims as in sskd_late_rerank; query token i of
 * query q is column q_lims[q] + i of S.  n_list = the length of d_list_rows (at most n_tokens); list bounds are read
 * clamped into [0, n_list] and a listed row outside [0, n_rows) is skipped.
 *   Limits: 1 <= Tq <= 128, 1 <= C <= 65 536, 1 <= nprobe <= min(C, 32), 1 <= R <= 1024; query tokens and centroids
 * 16-byte aligned, the workspace 256-byte aligned.  Workspace: sskd_plaid_candidates_workspace_bytes covers the whole
 * batch up to a budget of 256 MiB (and always one query, sized for every row being a candidate); any workspace that holds
 * one query's worth runs the call in chunks of queries.  sskd_plaid_candidates_plan reports one query's bytes, the
 * queries per chunk under workspace_bytes (0 = what the size query returns), the parts the probe search cuts the centroids
 * into and the interaction's workgroups per query.  Stream-ordered, no host sync (graph-capturable), allocates nothing;
 * every argument is checked before anything is enqueued (SSKD_ERR_INVALID); nq = 0 / n_q_tokens = 0 succeed. */
#define SSKD_PLAID_NPROBE_MAX 32
int sskd_plaid_centroid_scores(const void* d_q_tokens, int64_t n_q_tokens, const void* d_centroids, int C, float* d_S,
                               int64_t ld, void* stream);
size_t sskd_plaid_candidates_workspace_bytes(int nq, int64_t n_rows, int nprobe);
int sskd_plaid_candidates_plan(int nq, int max_tq, int C, int64_t n_rows, int nprobe, int R, size_t workspace_bytes,
                               size_t* per_query_bytes, int* queries_per_chunk, int* probe_parts, int* interact_workgroups);
int sskd_plaid_candidates(const float* d_S, int64_t ld, const int64_t* q_lims, const int64_t* d_q_lims, int nq, int C,
                          const int32_t* d_cid, const int64_t* d_tok_lims, int64_t n_rows, int64_t n_tokens,
                          const int64_t* d_list_lims, const int32_t* d_list_rows, int64_t n_list, const uint32_t* d_row_mask,
                          int nprobe, int R, int64_t id_offset, int64_t* d_cand_ids, float* d_cand_scores, int32_t* d_n_cand,
                          void* d_workspace, size_t workspace_bytes, void* stream);

/* Knowledge-distillation losses of the reference and their gradient (loss
 * half).  Replaces MarginMSELoss / ListwiseKDLoss / ContrastiveLoss / CombinedKDLoss.forward
 * (src/kd/losses.py:35-60, 81-106, 127-149, 219-252) on device-resident [batch, n_docs] fp32 score
 * matrices, n_docs <= 64 (document 0 is the positive).  d_losses[4] = { weighted total, margin-MSE,
 * listwise KD, contrastive }; d_grad (may be NULL) = d total / d student, [batch, n_docs];
 * d_row_workspace = 3 * batch floats.  Single components: set the other weights to 0. */
int sskd_kd_loss(const float* d_student, const float* d_teacher, int batch, int n_docs,
                 float temperature, float contrastive_temperature, float w_margin_mse,
                 float w_listwise, float w_contrastive, float* d_losses, float* d_grad,
                 float* d_row_workspace, void* stream);

/* Launch geometry the search would use (for roofline accounting in bench.py):
 * queries per workgroup tile (B_q), corpus passes, slices, waves per workgroup,
 * and scan passes needed for this k. Any out pointer may be NULL. */
int sskd_index_search_plan(int64_t n_rows, int nq, int k, int* queries_per_block,
                           int* corpus_passes, int* n_slices, int* waves_per_block,
                           int* scan_passes);

int sskd_index_search_plan_ex(int64_t n_rows, int nq, int k, const sskd_search_tuning* tuning,
                              int* queries_per_block, int* corpus_passes, int* n_slices,
                              int* waves_per_block, int* scan_passes);

/* Merge `n_lists` per-shard top-k lists per query into one (the step after the
 * RCCL all-gather; the reference has a single index, so no counterpart).
 * d_scores fp32 [n_lists, nq, k_in], d_ids int64 [n_lists, nq, k_in] (global ids,
 * -1 = empty). Output as sskd_index_search. */
int sskd_topk_merge(const float* d_scores, const int64_t* d_ids, int n_lists, int nq,
                    int k_in, int k_out, float* d_out_scores, int64_t* d_out_ids,
                    void* stream);

/* The same merge over PACKED per-shard records, the form one RCCL all-gather moves: record r
 * (r = 0 .. n_lists-1) starts at d_records + r * sskd_topk_record_bytes(nq, k_in) and holds
 * { int64 ids[nq][k_in]; float scores[nq][k_in]; padding to 16 B }.  A rank lets its local search
 * write ids / scores straight into its own record, all-gathers the records once, and merges. */
size_t sskd_topk_record_bytes(int nq, int k);
int sskd_topk_merge_packed(const void* d_records, int n_lists, int nq, int k_in, int k_out,
                           float* d_out_scores, int64_t* d_out_ids, void* stream);

/* q @ d^T in fp32: replaces StudentModel.compute_similarity
 *   reference: src/kd/eval.py:75, tests/test_student_model.py:104-124 */
int sskd_similarity(const float* d_q, int nq, const float* d_d, int nd, int dim,
                    float* d_out, void* stream);

/* ------------------------------------------------------------------------- *
 * Encoder (e5-small-v2 shaped BERT): replaces SentenceTransformer.encode()'s
 * Transformer -> Pooling(mean) -> Normalize modules
 *   reference: tests/test_model_validation.py:80-89,256-262; configs/kd.yaml:16-19
 * ------------------------------------------------------------------------- */

/* Masked mean-pool + L2 normalise:
 *   e = sum_t m_t h_t / max(sum_t m_t, 1e-9);  if normalize: e /= max(||e||, 1e-12)
 * d_hidden: [B, S, 384] bf16 (hidden_is_bf16 = 1) or fp32 (0); d_mask int32 [B, S];
 * d_out fp32 [B, 384] row-major. */
int sskd_pool_normalize(const void* d_hidden, int hidden_is_bf16, const int32_t* d_mask,
                        int B, int S, int normalize, float* d_out, void* stream);

/* Architecture of the bi-encoder (src/config.py:22-32). */
typedef struct sskd_encoder_config {
  int32_t vocab_size;        /* 30522 */
  int32_t hidden;            /* 384 (only value supported) */
  int32_t layers;            /* 12 */
  int32_t heads;             /* 12 (head dim 32, only value supported) */
  int32_t intermediate;      /* 1536 (only value supported) */
  int32_t max_positions;     /* 512 */
  int32_t type_vocab;        /* 2 */
  float layer_norm_eps;      /* 1e-12 */
} sskd_encoder_config;

/* Device weight table.  All matrices are bf16 row-major in the HF nn.Linear
 * convention [out_features, in_features]; biases and LayerNorm parameters fp32. */
typedef struct sskd_encoder_layer_weights {
  const void* wqkv;   /* bf16 [1152, 384]  (Wq; Wk; Wv stacked) */
  const float* bqkv;  /* [1152] */
  const void* wo;     /* bf16 [384, 384] */
  const float* bo;    /* [384] */
  const float* ln1_g; /* [384] */
  const float* ln1_b;
  const void* w1;     /* bf16 [1536, 384] */
  const float* b1;    /* [1536] */
  const void* w2;     /* bf16 [384, 1536], tiled chunk-major for the fused MLP (see weights.py) */
  const float* b2;    /* [384] */
  const float* ln2_g;
  const float* ln2_b;
} sskd_encoder_layer_weights;

typedef struct sskd_encoder_weights {
  const void* word_emb;  /* bf16 [vocab, 384] */
  const void* pos_emb;   /* bf16 [max_positions, 384] */
  const void* type_emb;  /* bf16 [type_vocab, 384] (row 0 is used) */
  const float* emb_ln_g; /* [384] */
  const float* emb_ln_b;
  const sskd_encoder_layer_weights* layers; /* HOST array of `layers` entries */
} sskd_encoder_weights;

size_t sskd_encoder_workspace_bytes(const sskd_encoder_config* cfg, int B, int S);

/* Full forward: ids/mask int32 [B, S] -> L2-normalised (if normalize) fp32 [B, 384].
 * bf16 activations and MFMA operands, fp32 accumulation / LayerNorm / softmax.
 * Stream semantics: everything is ordered after the work already in `stream` and complete for work enqueued on it
 * afterwards.  Batches whose halves still fill the chip twice (>= 2 x 65 536 padded tokens) run as two halves, one of
 * them on an internal side stream forked from and joined back into `stream` with events (legal under stream capture: the
 * graph gets two branches); the result is bit-identical, rows do not interact.  SSKD_FORWARD_STREAMS=1 in the environment
 * keeps every forward of the library (this one, the packed one, sskd_teacher_score) on the caller's stream alone. */
int sskd_encoder_forward(const sskd_encoder_config* cfg, const sskd_encoder_weights* w,
                         const int32_t* d_ids, const int32_t* d_mask, int B, int S,
                         int normalize, float* d_out, void* d_workspace,
                         size_t workspace_bytes, void* stream);

/* Same forward, stopping after the last encoder layer: bf16 [B, S, 384] hidden
 * states (test hook for per-stage parity against the oracle). */
int sskd_encoder_hidden(const sskd_encoder_config* cfg, const sskd_encoder_weights* w,
                        const int32_t* d_ids, const int32_t* d_mask, int B, int S,
                        void* d_hidden_bf16, void* d_workspace, size_t workspace_bytes,
                        void* stream);

/* Per-kernel test hook: runs cfg->layers layers (0 is legal: the embedding LayerNorm alone) and
 * returns BOTH activation buffers as row-major bf16 [B, S, 384]: the hidden states and the
 * attention context of the last layer run (unspecified for 0 layers).  d_seg != NULL: packed rows
 * (segment words of sskd_pack_tokens, S = capacity, a multiple of 32 up to 256), d_mask is then
 * unused.  Two calls with cfg->layers = l and l + 1 give every kernel of layer l its own inputs and
 * outputs (the kernels are bit-deterministic).  No kernel beyond those of sskd_encoder_hidden. */
int sskd_encoder_probe(const sskd_encoder_config* cfg, const sskd_encoder_weights* w,
                       const int32_t* d_ids, const int32_t* d_mask, const int32_t* d_seg, int B, int S,
                       void* d_hidden_bf16, void* d_context_bf16, void* d_workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Sequence packing (varlen / "cu_seqlens"): SentenceTransformer.encode pads every text of a
 * batch to the longest one (reference: tests/test_model_validation.py:80-110); here whole
 * sequences are concatenated into rows of `capacity` tokens (<= 256, multiple of 32) and
 * attention is block-diagonal per sequence, so only the tail of a row is padding.
 * ------------------------------------------------------------------------- */

/* HOST function.  Best-fit-decreasing placement of n_seq sequences (1 <= lengths[i] <= capacity)
 * into rows.  table[4 i .. 4 i + 3] = { row, lo, hi, i }: sequence i occupies tokens [lo, hi) of
 * `row`.  *n_rows = rows used. */
int sskd_pack_plan(const int32_t* lengths, int n_seq, int capacity, int32_t* table, int* n_rows);

/* Lay the flat token stream out as packed rows: d_flat_ids holds the sequences back to back,
 * d_cu_seqlens[n_seq + 1] their start offsets, d_table the (device copy of the) plan.
 * Outputs int32 [n_rows, capacity]: d_ids (0 = [PAD]) and d_seg (lo | hi << 16 per token,
 * 0 for padding). */
int sskd_pack_tokens(const int32_t* d_flat_ids, const int32_t* d_cu_seqlens, const int32_t* d_table,
                     int n_seq, int n_rows, int capacity, int32_t* d_ids, int32_t* d_seg, void* stream);

/* sskd_encoder_forward over packed rows; position ids restart at every sequence.  d_out fp32
 * [*, 384]: row table[4 i + 3] receives the embedding of sequence i.  Workspace:
 * sskd_encoder_workspace_bytes(cfg, n_rows, capacity). */
int sskd_encoder_forward_packed(const sskd_encoder_config* cfg, const sskd_encoder_weights* w,
                                const int32_t* d_ids, const int32_t* d_seg, int n_rows, int capacity,
                                const int32_t* d_table, int n_seq, int normalize, float* d_out,
                                void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Dimension-generic post-LN BERT-family encoder with SAVED activations and its backward pass:
 * the student forward/backward of the KD training step (reference: src/kd/train.py:176-210,
 * StudentModel.encode_with_gradients -> torch autograd) and the forward of the teacher
 * cross-encoder (reference: src/mining/miners.py:128-151, src/serve/app.py:321-339).
 * Row-major activations; hidden <= 1024; head width, hidden, intermediate multiples of 32;
 * S a multiple of 32 (pad with mask 0).  Weights bf16 row-major [out, in]; the `_t` members are
 * the transposes [in, out] (needed by the backward pass only, may be NULL for inference).
 * Inference (training == 0, and the teacher) runs the fused attention kernel, which serves head widths
 * 32, 64 and 128 with S * width <= 36 864 (width 128: S <= 288); training serves every width that is a
 * multiple of 32.  Arguments are checked before the first launch: a call that is refused (SSKD_ERR_INVALID,
 * SSKD_ERR_WORKSPACE) has enqueued nothing, and the size queries return 0 for a shape the call rejects.
 * ------------------------------------------------------------------------- */
typedef struct sskd_generic_config {
  int32_t vocab_size;
  int32_t hidden;
  int32_t layers;
  int32_t heads;
  int32_t intermediate;
  int32_t max_positions;
  int32_t type_vocab;
  float layer_norm_eps;
  int32_t pos_offset;     /* position id of token 0: 0 (BERT), 2 (XLM-R: padding_idx + 1) */
} sskd_generic_config;

typedef struct sskd_generic_layer_weights {
  const void* wqkv;   /* bf16 [3H, H] (Wq; Wk; Wv) */
  const void* wqkv_t; /* bf16 [H, 3H] */
  const void* wo;     /* bf16 [H, H] */
  const void* wo_t;
  const void* w1;     /* bf16 [F, H] */
  const void* w1_t;   /* bf16 [H, F] */
  const void* w2;     /* bf16 [H, F] */
  const void* w2_t;   /* bf16 [F, H] */
  const float* bqkv;  /* [3H] */
  const float* bo;
  const float* ln1_g;
  const float* ln1_b;
  const float* b1;    /* [F] */
  const float* b2;
  const float* ln2_g;
  const float* ln2_b;
} sskd_generic_layer_weights;

typedef struct sskd_generic_weights {
  const void* word_emb;  /* bf16 [vocab, H] */
  const void* pos_emb;   /* bf16 [max_positions, H] */
  const void* type_emb;  /* bf16 [type_vocab, H] (row 0 is used) */
  const float* emb_ln_g;
  const float* emb_ln_b;
  const sskd_generic_layer_weights* layers; /* HOST array */
} sskd_generic_weights;

/* fp32 gradient buffers with the shapes of the parameters; the backward pass ADDS into them. */
typedef struct sskd_generic_layer_grads {
  float* wqkv;  /* [3H, H] */
  float* bqkv;
  float* wo;
  float* bo;
  float* ln1_g;
  float* ln1_b;
  float* w1;
  float* b1;
  float* w2;
  float* b2;
  float* ln2_g;
  float* ln2_b;
} sskd_generic_layer_grads;

typedef struct sskd_generic_grads {
  float* word_emb;
  float* pos_emb;
  float* type_emb;  /* row 0 receives the gradient */
  float* emb_ln_g;
  float* emb_ln_b;
  const sskd_generic_layer_grads* layers; /* HOST array */
} sskd_generic_grads;

/* training != 0: room for every layer's saved activations + backward scratch. */
size_t sskd_generic_workspace_bytes(const sskd_generic_config* cfg, int B, int S, int training);

/* Forward.  pool != 0: masked mean-pool (+ L2 normalise) -> d_out fp32 [B, H]; pool == 0: d_out
 * receives the final hidden states bf16 [B, S, H].  With training != 0 the workspace afterwards
 * holds what sskd_generic_backward needs (same B, S, same workspace). */
int sskd_generic_forward(const sskd_generic_config* cfg, const sskd_generic_weights* w, const int32_t* d_ids,
                         const int32_t* d_mask, int B, int S, int training, int pool, int normalize, void* d_out,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* Backward of the pooled forward: d_dout fp32 [B, H] = d loss / d embeddings. */
int sskd_generic_backward(const sskd_generic_config* cfg, const sskd_generic_weights* w, const sskd_generic_grads* grads,
                          const int32_t* d_ids, const int32_t* d_mask, int B, int S, int normalize, const float* d_dout,
                          void* d_workspace, size_t workspace_bytes, void* stream);

/* Backward of the forward with pool == 0: d_dhidden DEVICE bf16 [B, S, H] (16-byte aligned) = d loss / d final hidden
 * states, read in place and left unchanged.  Everything else - the saved activations, the parameter gradients that are
 * ACCUMULATED into `grads`, the whole and two-halves runs, every H the generic encoder serves - is sskd_generic_backward's,
 * which is this call behind the backward of the pool. */
int sskd_generic_backward_hidden(const sskd_generic_config* cfg, const sskd_generic_weights* w, const sskd_generic_grads* grads,
                                 const int32_t* d_ids, const int32_t* d_mask, int B, int S, const void* d_dhidden,
                                 void* d_workspace, size_t workspace_bytes, void* stream);

/* Teacher cross-encoder score (replaces CrossEncoder.predict behind TeacherModel.score; reference:
 * src/mining/miners.py:135-137, src/serve/app.py:325-326; model = XLM-R-large shaped
 * XLMRobertaForSequenceClassification with one label, docs/adr-002): generic encoder forward ->
 * hidden state of token 0 -> dense [H, H] + tanh -> out_proj [1, H] -> d_logits fp32 [B] (raw logits).
 * The head runs in fp32: head weights fp32 row-major [out, in], biases fp32 (a reranker's product is the
 * ORDER of its logits; the head is 0.002 % of the FLOPs). */
size_t sskd_teacher_workspace_bytes(const sskd_generic_config* cfg, int B, int S);
int sskd_teacher_score(const sskd_generic_config* cfg, const sskd_generic_weights* w, const float* d_head_dense_w,
                       const float* d_head_dense_b, const float* d_head_out_w, const float* d_head_out_b,
                       const int32_t* d_ids, const int32_t* d_mask, int B, int S, float* d_logits, void* d_workspace,
                       size_t workspace_bytes, void* stream);

/* C[M, N] (bf16 or fp32, optionally +=) = A[M, K] . B[N, K]^T + bias[N]: the NT GEMM every
 * product of the generic path goes through (test hook; K % 32 == 0). */
int sskd_gemm_nt_bf16(const void* d_a, const void* d_b, void* d_c, const float* d_bias, int M, int N, int K,
                      int c_is_f32, int accumulate, void* stream);
/* Which kernels serve the PLAIN large products of the generic path (C = A . W^T + bias, bf16 out, K and N >= 1024: the
 * teacher's QKV, attention-output and FFN2 products): 0 = automatic - hipBLASLt, whose tuned kernels are 15-25 % faster
 * there than this library's 256 x 256 MFMA kernel; 1 = this library's kernels only (tests, A/B probes).  Any other value
 * only queries.  Process-wide; returns the mode in force.  Products with a fused epilogue, K = 384 (student) products,
 * batched / fp32 / accumulating products always run on the hand-written kernels. */
int sskd_gemm_backend(int mode);
/* C[M, N] (fp32) += A[T, M]^T . B[T, N]: the weight-gradient product of the training step with the token
 * dimension as the row of both bf16 operands (test hook; M % 384 == 0, N % 128 == 0, T % 64 == 0, else
 * SSKD_ERR_UNSUPPORTED: the step then transposes and uses the NT kernel). */
int sskd_gemm_tn_bf16(const void* d_a, const void* d_b, float* d_c, int64_t T, int M, int N, void* stream);

/* Every field of the NT GEMM the generic path launches (a plain C mirror of the library's internal argument block):
 * C[z][M, N] (+)= alpha * A[z][M, K] . B[z][N, K]^T + bias[N] over the two-level batch z = b1 * batch2 + b2, with element
 * strides per level.  K % 32 == 0; lda, ldb and the operand strides multiples of 8; 16-byte aligned operands.
 * c_is_f32: fp32 output (else bf16); accumulate: fp32 output only, C += result; split_k > 1: unbatched, fp32 accumulating
 * output without bias, K cut into split_k slices that meet through fp32 atomics; act = 1: erf-GELU of
 * (alpha * acc + bias) in the epilogue (bf16 output only). */
typedef struct sskd_gemm_desc {
  const void* a;
  const void* b;
  void* c;
  const float* bias;   /* [N] or NULL */
  int64_t lda, ldb, ldc;
  int64_t sa1, sa2, sb1, sb2, sc1, sc2;
  int32_t m, n, k;
  int32_t batch1, batch2;
  float alpha;
  int32_t c_is_f32;
  int32_t accumulate;
  int32_t split_k;
  int32_t act;
} sskd_gemm_desc;

/* Test hook: launches the NT GEMM exactly as the training step and the teacher do (same launcher: its argument checks,
 * the kernel choice, and the hipBLASLt route of sskd_gemm_backend(0)). */
int sskd_gemm_nt_ex(const sskd_gemm_desc* d, void* stream);

/* Test hook: one of the generic path's kernels by itself (csrc/generic.h), for per-kernel parity tests.  Arguments are
 * device pointers (`ptrs`, NULL where marked optional), integers and floats, in the order listed per op.  A wrong
 * argument count, an unknown op or a NULL where a pointer is required returns SSKD_ERR_INVALID and launches nothing;
 * a shape outside the kernel's contract returns the launcher's own error.  bf16 unless marked f32 / i32.
 *   ATTENTION_FWD    ptrs {qkv [B*S, 3*heads*DH], key_mask i32 [B, S], ctx [B*S, heads*DH], lse f32 [B, heads, S] opt}
 *                    ints {B, S, heads, DH}  floats {scale}
 *   ATTENTION_BWD    ptrs {qkv, key_mask, ctx, dctx, lse, dqkv [B*S, 3*heads*DH]}  ints {B, S, heads, DH}  floats {scale}
 *   SOFTMAX_FWD      ptrs {scores [B, heads, S, S] (in place), key_mask i32 [B, S]}  ints {B, heads, S}  floats {scale}
 *   SOFTMAX_BWD      ptrs {dP [rows, S] (in place), P [rows, S]}  ints {rows, S}  floats {scale}
 *   ADD_LN_FWD       ptrs {a, b opt, gamma f32, beta f32, y, z_save opt, mean f32 opt, rstd f32 opt (with mean)}
 *                    ints {M, H}  floats {eps}
 *   LN_BWD           ptrs {dy, z, mean f32, rstd f32, gamma f32, dz, dgamma f32, dbeta f32, dz_colsum f32 opt, dy2 opt}
 *                    ints {M, H}
 *   GELU_FWD         ptrs {u, h}  ints {n}
 *   GELU_BWD         ptrs {u, dh, du}  ints {n}
 *   GELU_BWD_COLSUM  ptrs {u [M, F], dh, du, db f32 [F]}  ints {M, F}
 *   COLSUM           ptrs {dY, db f32 [N]}  ints {M, N, ld}
 *   ADD              ptrs {a, b, c}  ints {n}
 *   TRANSPOSE        ptrs {in, out, colsum f32 opt}  ints {R, C, ld_in, ld_out, batch1, batch2, s_in1, s_in2, s_out1, s_out2}
 *   EMBED_FWD        ptrs {ids i32 [B, S], mask i32 [B, S], word [vocab, H], pos, type0 [H], z [B*S, H]}
 *                    ints {B, S, H, vocab, pos_offset}
 *   EMBED_BWD        ptrs {ids, mask, dz, dword f32, dpos f32, dtype0 f32}  ints {B, S, H, vocab, pos_offset}
 *   POOL_FWD         ptrs {hidden [B, S, H], mask i32, out f32 [B, H], pooled_save f32 opt}  ints {B, S, H, normalize}
 *   POOL_BWD         ptrs {dout f32 [B, H], pooled f32, mask i32, dhidden}  ints {B, S, H, normalize}
 *   GEMM_TN          ptrs {A [T, M], B [T, N], C f32 (+=)}  ints {lda, ldb, ldc, T, M, N} */
enum {
  SSKD_OP_ATTENTION_FWD = 1,
  SSKD_OP_ATTENTION_BWD = 2,
  SSKD_OP_SOFTMAX_FWD = 3,
  SSKD_OP_SOFTMAX_BWD = 4,
  SSKD_OP_ADD_LN_FWD = 5,
  SSKD_OP_LN_BWD = 6,
  SSKD_OP_GELU_FWD = 7,
  SSKD_OP_GELU_BWD = 8,
  SSKD_OP_GELU_BWD_COLSUM = 9,
  SSKD_OP_COLSUM = 10,
  SSKD_OP_ADD = 11,
  SSKD_OP_TRANSPOSE = 12,
  SSKD_OP_EMBED_FWD = 13,
  SSKD_OP_EMBED_BWD = 14,
  SSKD_OP_POOL_FWD = 15,
  SSKD_OP_POOL_BWD = 16,
  SSKD_OP_GEMM_TN = 17
};
int sskd_generic_op(int op, const void* const* ptrs, int n_ptrs, const int64_t* ints, int n_ints, const float* floats,
                    int n_floats, void* stream);

/* ------------------------------------------------------------------------- *
 * Host WordPiece tokenizer (uncased BERT): replaces the `tokenizers` call inside
 * SentenceTransformer.encode for ASCII text (reference: AutoTokenizer use src/utils/chunk.py:26;
 * vocabulary / special ids SURVEY.md §8c).  HOST functions, multi-threaded, no device work.
 * ------------------------------------------------------------------------- */

/* vocab_blob: the vocabulary tokens in id order separated by '\n' (vocab.txt layout). */
int sskd_tokenizer_create(const char* vocab_blob, int64_t blob_bytes, void** handle);
void sskd_tokenizer_destroy(void* handle);

/* Tokenise n_texts UTF-8 texts: text i = text_blob[offsets[i], offsets[i+1]) (NUL bytes inside are
 * ignored, so texts may simply be NUL-joined).  Emits "[CLS] pieces [SEP]" ids truncated to
 * max_len (the closing [SEP] is kept) back to back into out_ids; out_lengths[i] = ids of text i.
 * A text containing any non-ASCII byte is not tokenised: out_needs_unicode[i] = 1,
 * out_lengths[i] = 0 - the caller must route it through a Unicode-complete tokenizer.
 * *out_total = ids written; SSKD_ERR_WORKSPACE if out_capacity is too small. */
int sskd_tokenizer_encode(void* handle, const char* text_blob, const int64_t* offsets, int n_texts,
                          int max_len, int n_threads, int32_t* out_ids, int64_t out_capacity,
                          int32_t* out_lengths, uint8_t* out_needs_unicode, int64_t* out_total);

#ifdef __cplusplus
}
#endif
#endif /* SSKD_AMD_H */
