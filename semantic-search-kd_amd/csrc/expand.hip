// Query expansion by pseudo-relevance feedback (sskd_amd.h "Query expansion").
//
// Implements the step the reference's service contract names and its code never had (reference: configs/service.yaml
// 108-113, features.enable_query_expansion): between a first search and a second one, "the best rows of this query"
// become "a better query", on the device, with no host synchronisation.
//   prf_rocchio_kernel  dense side.  One wave per query: it walks the first fb_docs ranks (the common walk of
//                       ranking_walk.h), puts the feedback rows and their weights into LDS, then every lane owns float4
//                       chunks of the 1 536-byte row and adds the rows in rank order: out = alpha q + sum b_i row_i,
//                       every product and every sum rounded once.
//   prf_rm3_kernel      lexical side.  One workgroup per query: wave 0 walks the BM25 ranking under the candidate rule of
//                       the fuse kernel; the feedback rows' forward lists (at most 256 terms each) are added row by row
//                       into an open-addressing table in LDS (term -> fp64 weight; a term occurs once per row, so one
//                       barrier between rows fixes the order of every sum and no float atomics are needed); the best
//                       fb_terms under (weight descending, term ascending) come from the radix select of the BM25
//                       search; the expanded query CSR is written behind the repeated original tokens.
#include "radix_select.h"
#include "ranking_walk.h"
#include "search_device.h"
#include "search_host.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------ Rocchio
constexpr int RC_WAVES = 4;

struct RocchioParams {
  const float* rows;           // the index: row-major fp32 [n_rows][DIM]
  const float* queries;        // [nq][DIM], prepared
  const float* rank_scores;    // [nq][kd]
  const int64_t* rank_ids;     // local rows, -1 padded
  int64_t n_rows;
  int nq;
  int kd;
  int fb_docs;
  int weighting;               // 0 uniform, 1 score
  float alpha, beta;
  float* out_queries;          // [nq][DIM]
  int32_t* out_counts;         // [nq]
};

// One wave per query; the kernel has no workgroup barrier.  Products and sums are plain operators: this translation unit
// is compiled without contraction, so each is rounded once (the __f*_rn intrinsics are inlined from a header compiled
// WITH contraction and fuse into fma).
__global__ __launch_bounds__(RC_WAVES * 64) void prf_rocchio_kernel(RocchioParams p) {
  __shared__ int32_t fb_row_all[RC_WAVES][SSKD_K_MAX];
  __shared__ float fb_b_all[RC_WAVES][SSKD_K_MAX];   // max(score, 0) first, then the weights
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = blockIdx.x * RC_WAVES + wave;
  if (q >= p.nq) return;  // (wave-uniform)
  int32_t* const fb_row = fb_row_all[wave];
  float* const fb_b = fb_b_all[wave];

  // ---- the feedback rows: the first fb_docs ranks, 64 per round
  const float* rs = p.rank_scores + (int64_t)q * p.kd;
  const int64_t* ri = p.rank_ids + (int64_t)q * p.kd;
  int m = 0;            // (wave-uniform) feedback rows so far
  bool ended = false;   // an id -1 was met: nothing behind it counts
  for (int base = 0; base < p.fb_docs && !ended; base += 64) {
    const int at = base + lane;
    const bool inside = at < p.fb_docs;
    const int64_t row = inside ? ri[at] : -1;
    const bool alive = walk_step(inside, row, p.n_rows, lane, ended);
    const int pos = walk_pack(alive, lane, m);   // < fb_docs <= SSKD_K_MAX
    if (alive) {
      const float s = rs[at];
      fb_row[pos] = (int32_t)row;
      fb_b[pos] = s > 0.f ? s : 0.f;
    }
  }
  wave_lds_sync();

  const float4* src = reinterpret_cast<const float4*>(p.queries) + (int64_t)q * CHUNKS;
  float4* dst = reinterpret_cast<float4*>(p.out_queries) + (int64_t)q * CHUNKS;
  if (lane == 0) p.out_counts[q] = m;
  if (m == 0) {   // no feedback: the query as it came, bit for bit
    for (int c = lane; c < CHUNKS; c += 64) dst[c] = src[c];
    return;
  }

  // ---- the weights
  bool uniform = p.weighting == 0;
  float S = 0.f;
  if (!uniform) {
    for (int i = 0; i < m; ++i) S = S + fb_b[i];   // (every lane adds the same values in rank order)
    if (S == 0.f) uniform = true;
    wave_lds_sync();   // every lane has its sum before a lane turns its entries into weights
  }
  const float b_uniform = p.beta / (float)m;
  for (int i = lane; i < m; i += 64) fb_b[i] = uniform ? b_uniform : p.beta * (fb_b[i] / S);
  wave_lds_sync();

  // ---- out = alpha q + sum over the feedback rows, in rank order, of b_i row_i: whole rows in 16-byte loads
  const float4* rows4 = reinterpret_cast<const float4*>(p.rows);
  for (int c = lane; c < CHUNKS; c += 64) {
    const float4 x = src[c];
    float4 acc;
    acc.x = p.alpha * x.x;
    acc.y = p.alpha * x.y;
    acc.z = p.alpha * x.z;
    acc.w = p.alpha * x.w;
#pragma unroll 4
    for (int i = 0; i < m; ++i) {
      const float4 r = rows4[(int64_t)fb_row[i] * CHUNKS + c];
      const float b = fb_b[i];
      acc.x = acc.x + b * r.x;
      acc.y = acc.y + b * r.y;
      acc.z = acc.z + b * r.z;
      acc.w = acc.w + b * r.w;
    }
    dst[c] = acc;
  }
}

// ------------------------------------------------------------------------------------------------ RM3
using sskd::radix::key_score;
using sskd::radix::score_key;
using sskd::radix::select_sorted;
using sskd::radix::SelectShared;

constexpr int RM3_THREADS = sskd::radix::SELECT_THREADS;
constexpr int RM3_KB_MAX = 256;   // what sskd_bm25_search writes at most
constexpr int RM3_FB_DOCS_MAX = 16;
constexpr int RM3_FB_TERMS_MAX = 64;
constexpr int RM3_ORIG_REPEAT_MAX = 8;
constexpr int RM3_ROW_TERMS = SSKD_RM3_ROW_TERMS;   // 256 = one thread per entry of a row's list
// 16 rows x 256 disjoint terms = 4 096 keys at load factor 1/2: 32 KiB of keys + 64 KiB of weights
constexpr int RM3_TABLE_BITS = 13;
constexpr int RM3_TABLE = 1 << RM3_TABLE_BITS;
constexpr int32_t RM3_EMPTY = -1;
constexpr int RM3_CAND_MAX = RM3_FB_DOCS_MAX * RM3_ROW_TERMS;   // every thread claims at most one slot per row
static_assert(RM3_TABLE <= 65536, "the occupied slots are listed as uint16");
static_assert(RM3_ROW_TERMS == RM3_THREADS, "one thread per forward entry");
static_assert(RM3_FB_DOCS_MAX * RM3_ROW_TERMS * 2 <= RM3_TABLE, "the table holds the worst case at load factor 1/2");
static_assert(RM3_FB_TERMS_MAX <= sskd::radix::SELECT_K_MAX, "the select hands out every chosen term");

struct Rm3Params {
  const int64_t* fwd_lims;       // [n_rows + 1]
  const int32_t* fwd_terms;      // per row ascending
  const double* fwd_p;           // tf / dl
  int64_t n_fwd;                 // entries of fwd_terms / fwd_p
  const int64_t* term_offsets;   // [n_terms + 1]: document frequencies
  int64_t n_rows;
  int64_t n_terms;
  const int64_t* q_lims;         // [nq + 1]
  const int32_t* q_terms;
  const double* rank_scores;     // [nq][kb]
  const int64_t* rank_ids;       // local rows, -1 padded
  const uint32_t* mask;          // allow-mask over the rows or null
  int kb, fb_docs, fb_terms, orig_repeat;
  int64_t max_df;                // 0: off
  const int64_t* out_lims;       // [nq + 1]
  int32_t* out_terms;
  int32_t* out_sel_terms;        // [nq][fb_terms]
  double* out_sel_w;             // [nq][fb_terms]
  int32_t* out_counts;           // [nq]
  int32_t* out_fb;               // [nq]
};

__global__ __launch_bounds__(RM3_THREADS) void prf_rm3_kernel(Rm3Params p) {
  __shared__ double t_w[RM3_TABLE];
  __shared__ int32_t t_key[RM3_TABLE];
  __shared__ uint16_t t_used[RM3_CAND_MAX];   // the occupied slots in order of arrival: what the select passes over
  __shared__ SelectShared sh;
  __shared__ double fb_s[RM3_FB_DOCS_MAX];
  __shared__ int32_t fb_row[RM3_FB_DOCS_MAX];
  __shared__ int n_fb_sh, n_cand_sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;

  for (int i = tid; i < RM3_TABLE; i += RM3_THREADS) {
    t_key[i] = RM3_EMPTY;
    t_w[i] = 0.0;
  }
  if (tid == 0) n_cand_sh = 0;

  // ---- walk: the candidate rule of the fuse kernel's BM25 side; the first fb_docs survivors are the feedback rows
  if (wave == 0) {
    const double* rs = p.rank_scores + (int64_t)q * p.kb;
    const int64_t* ri = p.rank_ids + (int64_t)q * p.kb;
    int count = 0;        // (wave-uniform) survivors so far
    bool ended = false;   // an id -1 was met: nothing behind it counts
    for (int base = 0; base < p.kb && !ended && count < p.fb_docs; base += 64) {
      const int at = base + lane;
      const int64_t row = at < p.kb ? ri[at] : -1;
      bool alive = walk_step(at < p.kb, row, p.n_rows, lane, ended);
      double s = 0.0;
      if (alive) {
        s = rs[at];
        if (s == 0.0) alive = false;   // +0.0 or -0.0: the row matched no query word
        if (!row_allowed(p.mask, row)) alive = false;
      }
      const int pos = walk_pack(alive, lane, count);
      if (alive && pos < p.fb_docs) {   // fb_docs <= RM3_FB_DOCS_MAX
        fb_row[pos] = (int32_t)row;
        fb_s[pos] = s;
      }
    }
    if (lane == 0) n_fb_sh = min(count, p.fb_docs);
  }
  __syncthreads();
  const int n_fb = n_fb_sh;

  // ---- the table: w(t) = sum over the feedback rows, in rank order, of p(t, d) * (s_d / S)
  const int64_t q_lo = p.q_lims[q], q_hi = p.q_lims[q + 1];
  double S = 0.0;
  for (int d = 0; d < n_fb; ++d) S = S + fb_s[d];   // (every thread adds the same values in rank order)
  for (int d = 0; d < n_fb; ++d) {
    const int64_t row = fb_row[d];
    int64_t lo = p.fwd_lims[row], hi = p.fwd_lims[row + 1];
    if (lo < 0 || hi > p.n_fwd || hi < lo) hi = lo = 0;      // a malformed list is an empty one
    if (hi - lo > RM3_ROW_TERMS) hi = lo + RM3_ROW_TERMS;    // and a long one is cut
    const double P = fb_s[d] / S;
    if (lo + tid < hi) {
      const int64_t t = p.fwd_terms[lo + tid];
      bool cand = t >= 0 && t < p.n_terms;
      if (cand && p.max_df > 0 && p.term_offsets[t + 1] - p.term_offsets[t] > p.max_df) cand = false;
      for (int64_t i = q_lo; cand && i < q_hi; ++i)
        if ((int64_t)p.q_terms[i] == t) cand = false;   // the query's own words are not expansion words
      if (cand) {
        const double term = p.fwd_p[lo + tid] * P;
        const uint32_t h = ((uint32_t)t * 2654435761u) >> (32 - RM3_TABLE_BITS);
        // at most RM3_TABLE probes; a term that finds no slot is dropped (the table cannot fill: static_assert above)
        for (int probe = 0; probe < RM3_TABLE; ++probe) {
          const int slot = (int)((h + (uint32_t)probe) & (uint32_t)(RM3_TABLE - 1));
          const int32_t prev = atomicCAS(&t_key[slot], RM3_EMPTY, (int32_t)t);
          if (prev == RM3_EMPTY) {
            const int at = atomicAdd(&n_cand_sh, 1);
            if (at < RM3_CAND_MAX) t_used[at] = (uint16_t)slot;   // (always: one claim per thread and row)
          }
          if (prev == RM3_EMPTY || prev == (int32_t)t) {
            t_w[slot] = t_w[slot] + term;   // the row holds t once: no other thread adds to this slot now
            break;
          }
        }
      }
    }
    __syncthreads();   // the next row may hold the same terms
  }

  // ---- output: the query's tokens orig_repeat times, the chosen terms in order, -1 behind them
  const int64_t o_lo = p.out_lims[q], o_hi = p.out_lims[q + 1];
  const int64_t len_q = q_hi > q_lo ? q_hi - q_lo : 0;
  const int64_t own = len_q * p.orig_repeat;
  int32_t* seg = p.out_terms + o_lo;
  const int64_t seg_len = o_hi > o_lo ? o_hi - o_lo : 0;   // (the host checked own + fb_terms == seg_len)
  for (int64_t i = tid; i < own && i < seg_len; i += RM3_THREADS) seg[i] = p.q_terms[q_lo + i % len_q];
  const int n_cand = min(n_cand_sh, RM3_CAND_MAX);
  const int kk = min(p.fb_terms, n_cand);
  int32_t* sel_t = p.out_sel_terms + (int64_t)q * p.fb_terms;
  double* sel_w = p.out_sel_w + (int64_t)q * p.fb_terms;
  for (int i = kk + tid; i < p.fb_terms; i += RM3_THREADS) {
    if (own + i < seg_len) seg[own + i] = -1;
    sel_t[i] = -1;
    sel_w[i] = 0.0;
  }
  if (tid == 0) {
    p.out_counts[q] = kk;
    p.out_fb[q] = n_fb;
  }
  // over the occupied slots only (their order of arrival does not matter: the keys are distinct and the order total);
  // lo = the term id inverted: a lower term id wins a tie of weights
  select_sorted<4>(
      sh, n_cand, kk,
      [&](int i, uint64_t& hi, uint32_t& lo) {
        const int slot = t_used[i];
        hi = score_key(t_w[slot]);
        lo = 0xFFFFFFFFu - (uint32_t)t_key[slot];
        return true;
      },
      [&](int rank, uint64_t hi, uint32_t lo) {
        const int32_t t = (int32_t)(0xFFFFFFFFu - lo);
        if (own + rank < seg_len) seg[own + rank] = t;
        sel_t[rank] = t;
        sel_w[rank] = key_score(hi);
      });
}

inline bool finite_nonneg(float x) { return x >= 0.f && x <= FLT_MAX; }

}  // namespace

extern "C" {

int sskd_prf_rocchio(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, const float* d_rank_scores,
                     const int64_t* d_rank_ids, int kd, int fb_docs, float alpha, float beta, int weighting,
                     float* d_out_queries, int32_t* d_out_counts, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "prf_rocchio: n_rows < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "prf_rocchio: n_rows too large for int32 row ids");
  SSKD_REQUIRE(nq >= 0, "prf_rocchio: nq < 0");
  SSKD_REQUIRE(kd >= 1 && kd <= SSKD_K_MAX, "prf_rocchio: kd=%d outside [1, %d]", kd, SSKD_K_MAX);
  SSKD_REQUIRE(fb_docs >= 1 && fb_docs <= kd, "prf_rocchio: fb_docs=%d outside [1, kd = %d]", fb_docs, kd);
  SSKD_REQUIRE(weighting == 0 || weighting == 1, "prf_rocchio: weighting=%d is neither 0 (uniform) nor 1 (score)",
               weighting);
  SSKD_REQUIRE(finite_nonneg(alpha), "prf_rocchio: alpha must be finite and >= 0");
  SSKD_REQUIRE(finite_nonneg(beta), "prf_rocchio: beta must be finite and >= 0");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_queries && d_rank_scores && d_rank_ids && d_out_queries && d_out_counts, "prf_rocchio: null pointer");
  SSKD_REQUIRE(n_rows == 0 || d_tiled, "prf_rocchio: null index");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0 && reinterpret_cast<uintptr_t>(d_queries) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(d_out_queries) % 16 == 0,
               "prf_rocchio: d_tiled, d_queries and d_out_queries must be 16-byte aligned");
  {
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_queries), b = reinterpret_cast<uintptr_t>(d_out_queries);
    const uintptr_t bytes = (uintptr_t)nq * DIM * sizeof(float);
    SSKD_REQUIRE(a + bytes <= b || b + bytes <= a, "prf_rocchio: d_out_queries may not alias d_queries");
  }
  RocchioParams p{};
  p.rows = d_tiled;
  p.queries = d_queries;
  p.rank_scores = d_rank_scores;
  p.rank_ids = d_rank_ids;
  p.n_rows = n_rows;
  p.nq = nq;
  p.kd = kd;
  p.fb_docs = fb_docs;
  p.weighting = weighting;
  p.alpha = alpha;
  p.beta = beta;
  p.out_queries = d_out_queries;
  p.out_counts = d_out_counts;
  hipLaunchKernelGGL(prf_rocchio_kernel, dim3((unsigned)sskd::ceil_div(nq, RC_WAVES)), dim3(RC_WAVES * 64), 0,
                     sskd::as_stream(stream), p);
  return sskd::check_launch("prf_rocchio_kernel");
}

int sskd_prf_rm3(const int64_t* d_fwd_lims, const int32_t* d_fwd_terms, const double* d_fwd_p, int64_t n_fwd,
                 const int64_t* d_term_offsets, int64_t n_rows, int64_t n_terms, const int64_t* q_lims,
                 const int64_t* d_q_lims, const int32_t* d_q_terms, const double* d_rank_scores,
                 const int64_t* d_rank_ids, int kb, const uint32_t* d_mask, int nq, int fb_docs, int fb_terms,
                 int orig_repeat, int64_t max_df, const int64_t* out_lims, const int64_t* d_out_lims,
                 int32_t* d_out_terms, int32_t* d_out_sel_terms, double* d_out_sel_w, int32_t* d_out_counts,
                 int32_t* d_out_fb, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "prf_rm3: n_rows < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "prf_rm3: n_rows too large for int32 row ids");
  SSKD_REQUIRE(n_terms >= 0 && n_terms <= INT32_MAX, "prf_rm3: n_terms outside [0, 2^31)");
  SSKD_REQUIRE(n_fwd >= 0, "prf_rm3: n_fwd < 0");
  SSKD_REQUIRE(nq >= 0, "prf_rm3: nq < 0");
  SSKD_REQUIRE(kb >= 1 && kb <= RM3_KB_MAX, "prf_rm3: kb=%d outside [1, %d]", kb, RM3_KB_MAX);
  SSKD_REQUIRE(fb_docs >= 1 && fb_docs <= RM3_FB_DOCS_MAX, "prf_rm3: fb_docs=%d outside [1, %d]", fb_docs,
               RM3_FB_DOCS_MAX);
  SSKD_REQUIRE(fb_docs <= kb, "prf_rm3: fb_docs=%d > kb=%d", fb_docs, kb);
  SSKD_REQUIRE(fb_terms >= 1 && fb_terms <= RM3_FB_TERMS_MAX, "prf_rm3: fb_terms=%d outside [1, %d]", fb_terms,
               RM3_FB_TERMS_MAX);
  SSKD_REQUIRE(orig_repeat >= 1 && orig_repeat <= RM3_ORIG_REPEAT_MAX, "prf_rm3: orig_repeat=%d outside [1, %d]",
               orig_repeat, RM3_ORIG_REPEAT_MAX);
  SSKD_REQUIRE(max_df >= 0, "prf_rm3: max_df < 0");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_fwd_lims && d_fwd_terms && d_fwd_p && d_term_offsets, "prf_rm3: null index table");
  SSKD_REQUIRE(q_lims && d_q_lims && d_q_terms, "prf_rm3: null query table");
  SSKD_REQUIRE(d_rank_scores && d_rank_ids, "prf_rm3: null ranking");
  SSKD_REQUIRE(out_lims && d_out_lims && d_out_terms && d_out_sel_terms && d_out_sel_w && d_out_counts && d_out_fb,
               "prf_rm3: null output");
  SSKD_REQUIRE(q_lims[0] >= 0 && out_lims[0] >= 0, "prf_rm3: q_lims and out_lims must start at >= 0");
  for (int q = 0; q < nq; ++q) {
    const int64_t len = q_lims[q + 1] - q_lims[q], seg = out_lims[q + 1] - out_lims[q];
    SSKD_REQUIRE(len >= 0 && len <= (INT64_MAX >> 8), "prf_rm3: q_lims decreases at query %d", q);
    SSKD_REQUIRE(seg == len * orig_repeat + fb_terms,
                 "prf_rm3: out segment of query %d holds %lld slots, orig_repeat * len + fb_terms = %lld", q,
                 (long long)seg, (long long)(len * orig_repeat + fb_terms));
  }
  Rm3Params p{};
  p.fwd_lims = d_fwd_lims;
  p.fwd_terms = d_fwd_terms;
  p.fwd_p = d_fwd_p;
  p.n_fwd = n_fwd;
  p.term_offsets = d_term_offsets;
  p.n_rows = n_rows;
  p.n_terms = n_terms;
  p.q_lims = d_q_lims;
  p.q_terms = d_q_terms;
  p.rank_scores = d_rank_scores;
  p.rank_ids = d_rank_ids;
  p.mask = d_mask;
  p.kb = kb;
  p.fb_docs = fb_docs;
  p.fb_terms = fb_terms;
  p.orig_repeat = orig_repeat;
  p.max_df = max_df;
  p.out_lims = d_out_lims;
  p.out_terms = d_out_terms;
  p.out_sel_terms = d_out_sel_terms;
  p.out_sel_w = d_out_sel_w;
  p.out_counts = d_out_counts;
  p.out_fb = d_out_fb;
  hipLaunchKernelGGL(prf_rm3_kernel, dim3((unsigned)nq), dim3(RM3_THREADS), 0, sskd::as_stream(stream), p);
  return sskd::check_launch("prf_rm3_kernel");
}

}  // extern "C"
