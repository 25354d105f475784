// Hybrid retrieval: one dense ranking and one BM25 ranking per query fused into one (sskd_amd.h "Hybrid fusion";
// DESIGN.md 16).
//
// Implements the join the reference's service contract names and its code never had (reference: configs/service.yaml
// 43-49, hybrid.fusion_method "rrf" / "linear" with semantic_weight / bm25_weight).  One workgroup per query, the union
// of both lists (at most 512 rows) in LDS:
//   walk      wave 0 walks the dense list, wave 1 the BM25 list, 64 entries per round: candidates get their 1-based
//             rank among the survivors (ranking_walk.h); waves 2 and 3 bring the query into LDS meanwhile
//   union     a BM25 candidate whose row the dense list holds hands its score and rank to that slot and leaves
//   complete  (linear only) one lane per row: a row without a dense score is scored with the fma chain of the exact
//             scan, a row without a BM25 score with the search's own sum (binary search per query token)
//   fuse      fp64, every operation rounded once: this translation unit is compiled without contraction
//   order     every row counts the rows that beat it under (fused descending, row ascending) and writes itself there
#include "ranking_walk.h"
#include "search_device.h"
#include "search_host.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int UNION_MAX = 512;   // kd + kb

struct FuseParams {
  const float* rows;             // the dense index: row-major fp32 [n_rows][DIM]
  const float* queries;          // [nq][DIM], prepared (normalised when the metric is cosine)
  const float* dense_scores;     // [nq][kd]
  const int64_t* dense_ids;      // local rows, -1 padded
  const int64_t* term_offsets;   // [n_terms + 1]
  const int32_t* post_rows;      // per term ascending
  const double* post_w;
  const double* idf;             // [n_terms]
  const int64_t* q_lims;         // [nq + 1]
  const int32_t* q_terms;
  const double* bm25_scores;     // [nq][kb]
  const int64_t* bm25_ids;       // local rows, -1 padded
  const uint32_t* mask;          // allow-mask over the rows or null
  int64_t n_rows;
  int64_t n_terms;
  int64_t id_offset;
  double w_semantic, w_bm25, rrf_k;
  int kd, kb, k;
  int method;                    // 0 rrf, 1 linear
  double* out_scores;            // [nq][k]
  int64_t* out_ids;
  int32_t* out_counts;           // [nq]
  float* out_dense;              // [nq][k] or null
  double* out_bm25;              // [nq][k] or null
};

// fp64 -> uint64 whose unsigned order is the order of the doubles, -0.0 below +0.0 (no NaN reaches here)
__device__ inline unsigned long long order_key(double s) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double key_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// score(q, row) of sskd_bm25_search: the query's tokens in order, the product rounded, then the sum
__device__ inline double bm25_row_score(const FuseParams& p, int64_t t_lo, int64_t t_hi, int32_t row) {
  double acc = 0.0;
  for (int64_t i = t_lo; i < t_hi; ++i) {
    const int64_t t = p.q_terms[i];
    if (t < 0 || t >= p.n_terms) continue;
    int64_t lo = p.term_offsets[t];
    const int64_t end = p.term_offsets[t + 1];
    int64_t hi = end;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (p.post_rows[mid] < row) lo = mid + 1;
      else hi = mid;
    }
    if (lo < end && p.post_rows[lo] == row) {
      const double term = p.idf[t] * p.post_w[lo];
      acc = acc + term;
    }
  }
  return acc;
}

__global__ __launch_bounds__(THREADS) void hybrid_fuse_kernel(FuseParams p) {
  __shared__ float4 q4[CHUNKS];
  __shared__ int32_t u_row[UNION_MAX];     // -1: the slot holds no row of the union
  __shared__ float u_s[UNION_MAX];
  __shared__ double u_b[UNION_MAX];
  __shared__ int32_t u_rank_s[UNION_MAX];  // 1-based, 0: the dense list lacks the row
  __shared__ int32_t u_rank_b[UNION_MAX];
  __shared__ double u_fused[UNION_MAX];
  __shared__ unsigned long long lim[4];    // keys of s_min, s_max, b_min, b_max
  __shared__ int union_count;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const int kd = p.kd, n_slots = p.kd + p.kb;

  for (int i = tid; i < n_slots; i += THREADS) {
    u_row[i] = -1;
    u_s[i] = 0.f;
    u_b[i] = 0.0;
    u_rank_s[i] = 0;
    u_rank_b[i] = 0;
  }
  if (tid == 0) {
    lim[0] = ~0ull; lim[1] = 0ull; lim[2] = ~0ull; lim[3] = 0ull;
    union_count = 0;
  }
  __syncthreads();

  // ---- walk: slots [0, kd) are the dense list's, [kd, kd + kb) the BM25 list's
  if (wave < 2) {
    const bool dense = wave == 0;
    const int len = dense ? p.kd : p.kb;
    const int64_t* ids = (dense ? p.dense_ids : p.bm25_ids) + (int64_t)q * len;
    int count = 0;        // (wave-uniform) survivors so far
    bool ended = false;   // an id -1 was met: nothing behind it counts
    for (int base = 0; base < len && !ended; base += 64) {
      const int at = base + lane;
      const int64_t row = at < len ? ids[at] : -1;
      bool alive = walk_step(at < len, row, p.n_rows, lane, ended);
      float s = 0.f;
      double b = 0.0;
      if (alive) {
        if (dense) {
          s = p.dense_scores[(int64_t)q * len + at];
        } else {
          b = p.bm25_scores[(int64_t)q * len + at];
          if (b == 0.0) alive = false;   // +0.0 or -0.0: the row matched no query word
          if (!row_allowed(p.mask, row)) alive = false;
        }
      }
      const int rank = walk_pack(alive, lane, count) + 1;
      if (alive) {
        const int slot = dense ? at : kd + at;
        u_row[slot] = (int32_t)row;
        if (dense) {
          u_s[slot] = s;
          u_rank_s[slot] = rank;
        } else {
          u_b[slot] = b;
          u_rank_b[slot] = rank;
        }
      }
    }
  } else if (p.method == 1) {
    const float4* src = reinterpret_cast<const float4*>(p.queries) + (int64_t)q * CHUNKS;
    for (int i = tid - 128; i < CHUNKS; i += 128) q4[i] = src[i];
  }
  __syncthreads();

  // ---- union: a BM25 candidate the dense list holds too moves into the dense slot
  for (int i = kd + tid; i < n_slots; i += THREADS) {
    const int32_t row = u_row[i];
    if (row < 0) continue;
    int found = -1;
    for (int j = 0; j < kd; ++j)   // (the lanes read the same slot: broadcast)
      if (u_row[j] == row) found = j;
    if (found >= 0) {
      u_b[found] = u_b[i];
      u_rank_b[found] = u_rank_b[i];
      u_row[i] = -1;
    }
  }
  __syncthreads();

  // ---- complete (linear): both scores for every row; the limits of both for the normalisation
  const bool linear = p.method == 1;
  int mine = 0;
  for (int i = tid; i < n_slots; i += THREADS) {
    const int32_t row = u_row[i];
    if (row < 0) continue;
    ++mine;
    if (!linear) continue;
    float s = u_s[i];
    double b = u_b[i];
    if (u_rank_s[i] == 0) {
      s = row_score_fma(reinterpret_cast<const float4*>(p.rows) + (int64_t)row * CHUNKS,
                        reinterpret_cast<const float*>(q4));
      u_s[i] = s;
    }
    if (u_rank_b[i] == 0) {
      b = bm25_row_score(p, p.q_lims[q], p.q_lims[q + 1], row);
      u_b[i] = b;
    }
    const unsigned long long ks = order_key((double)s), kb_ = order_key(b);
    atomicMin(&lim[0], ks);
    atomicMax(&lim[1], ks);
    atomicMin(&lim[2], kb_);
    atomicMax(&lim[3], kb_);
  }
  if (mine) atomicAdd(&union_count, mine);
  __syncthreads();

  // ---- fuse
  const double s_min = key_value(lim[0]), s_max = key_value(lim[1]);
  const double b_min = key_value(lim[2]), b_max = key_value(lim[3]);
  for (int i = tid; i < n_slots; i += THREADS) {
    if (u_row[i] < 0) continue;
    double fs, fb;
    if (linear) {
      double ns = 0.0, nb = 0.0;
      if (s_max != s_min) {
        const double num = (double)u_s[i] - s_min, den = s_max - s_min;
        ns = num / den;
      }
      if (b_max != b_min) {
        const double num = u_b[i] - b_min, den = b_max - b_min;
        nb = num / den;
      }
      fs = p.w_semantic * ns;
      fb = p.w_bm25 * nb;
    } else {
      fs = 0.0;
      fb = 0.0;
      if (u_rank_s[i]) {
        const double den = p.rrf_k + (double)u_rank_s[i];
        const double r = 1.0 / den;
        fs = p.w_semantic * r;
      }
      if (u_rank_b[i]) {
        const double den = p.rrf_k + (double)u_rank_b[i];
        const double r = 1.0 / den;
        fb = p.w_bm25 * r;
      }
    }
    u_fused[i] = fs + fb;
  }
  __syncthreads();

  // ---- order: rows are distinct, so (fused descending, row ascending) is total and the places are distinct
  const int count = union_count;
  const int k = p.k;
  double* os = p.out_scores + (int64_t)q * k;
  int64_t* oi = p.out_ids + (int64_t)q * k;
  float* od = p.out_dense ? p.out_dense + (int64_t)q * k : nullptr;
  double* ob = p.out_bm25 ? p.out_bm25 + (int64_t)q * k : nullptr;
  for (int i = tid; i < n_slots; i += THREADS) {
    const int32_t row = u_row[i];
    if (row < 0) continue;
    const double f = u_fused[i];
    int place = 0;
    for (int j = 0; j < n_slots; ++j) {   // (the lanes read the same slot: broadcast)
      const int32_t orow = u_row[j];
      const double of = u_fused[j];
      place += (orow >= 0 && (of > f || (of == f && orow < row))) ? 1 : 0;
    }
    if (place < k) {
      os[place] = f;
      oi[place] = (int64_t)row + p.id_offset;
      if (od) od[place] = (linear || u_rank_s[i]) ? u_s[i] : __builtin_nanf("");
      if (ob) ob[place] = (linear || u_rank_b[i]) ? u_b[i] : __builtin_nan("");
    }
  }
  for (int i = min(count, k) + tid; i < k; i += THREADS) {
    os[i] = -INFINITY;
    oi[i] = -1;
    if (od) od[i] = __builtin_nanf("");
    if (ob) ob[i] = __builtin_nan("");
  }
  if (tid == 0) p.out_counts[q] = count;
}

}  // namespace

extern "C" {

int sskd_hybrid_fuse(const float* d_tiled, int64_t n_rows, const float* d_queries, const float* d_dense_scores,
                     const int64_t* d_dense_ids, int kd, const int64_t* d_term_offsets, const int32_t* d_post_rows,
                     const double* d_post_w, const double* d_idf, int64_t n_terms, const int64_t* d_q_lims,
                     const int32_t* d_q_terms, const double* d_bm25_scores, const int64_t* d_bm25_ids, int kb,
                     const uint32_t* d_mask, int method, double w_semantic, double w_bm25, double rrf_k, int nq, int k,
                     int64_t id_offset, double* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts,
                     float* d_out_dense, double* d_out_bm25, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "hybrid_fuse: n_rows < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "hybrid_fuse: n_rows too large for int32 row ids");
  SSKD_REQUIRE(nq >= 0, "hybrid_fuse: nq < 0");
  SSKD_REQUIRE(kd >= 1 && kd <= SSKD_K_MAX, "hybrid_fuse: kd=%d outside [1, %d]", kd, SSKD_K_MAX);
  SSKD_REQUIRE(kb >= 1 && kb <= SSKD_K_MAX, "hybrid_fuse: kb=%d outside [1, %d]", kb, SSKD_K_MAX);
  SSKD_REQUIRE(kd + kb <= UNION_MAX, "hybrid_fuse: kd + kb = %d > %d", kd + kb, UNION_MAX);
  SSKD_REQUIRE(k >= 1 && k <= kd + kb, "hybrid_fuse: k=%d outside [1, kd + kb = %d]", k, kd + kb);
  SSKD_REQUIRE(method == 0 || method == 1, "hybrid_fuse: method=%d is neither 0 (rrf) nor 1 (linear)", method);
  SSKD_REQUIRE(rrf_k > 0 && rrf_k <= DBL_MAX, "hybrid_fuse: rrf_k must be finite and > 0");
  SSKD_REQUIRE(w_semantic >= 0 && w_semantic <= DBL_MAX, "hybrid_fuse: w_semantic must be finite and >= 0");
  SSKD_REQUIRE(w_bm25 >= 0 && w_bm25 <= DBL_MAX, "hybrid_fuse: w_bm25 must be finite and >= 0");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_dense_scores && d_dense_ids, "hybrid_fuse: null dense ranking");
  SSKD_REQUIRE(d_bm25_scores && d_bm25_ids, "hybrid_fuse: null bm25 ranking");
  SSKD_REQUIRE(d_out_scores && d_out_ids && d_out_counts, "hybrid_fuse: null output");
  if (method == 1) {
    SSKD_REQUIRE(n_terms >= 0 && n_terms <= INT32_MAX, "hybrid_fuse: n_terms outside [0, 2^31)");
    SSKD_REQUIRE(d_tiled && d_queries, "hybrid_fuse: linear needs d_tiled and d_queries");
    SSKD_REQUIRE(d_term_offsets && d_post_rows && d_post_w && d_idf, "hybrid_fuse: linear needs the bm25 index tables");
    SSKD_REQUIRE(d_q_lims && d_q_terms, "hybrid_fuse: linear needs d_q_lims and d_q_terms");
    SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0 && reinterpret_cast<uintptr_t>(d_queries) % 16 == 0,
                 "hybrid_fuse: d_tiled and d_queries must be 16-byte aligned");
  }
  FuseParams p{};
  p.rows = d_tiled;
  p.queries = d_queries;
  p.dense_scores = d_dense_scores;
  p.dense_ids = d_dense_ids;
  p.term_offsets = d_term_offsets;
  p.post_rows = d_post_rows;
  p.post_w = d_post_w;
  p.idf = d_idf;
  p.q_lims = d_q_lims;
  p.q_terms = d_q_terms;
  p.bm25_scores = d_bm25_scores;
  p.bm25_ids = d_bm25_ids;
  p.mask = d_mask;
  p.n_rows = n_rows;
  p.n_terms = n_terms;
  p.id_offset = id_offset;
  p.w_semantic = w_semantic;
  p.w_bm25 = w_bm25;
  p.rrf_k = rrf_k;
  p.kd = kd;
  p.kb = kb;
  p.k = k;
  p.method = method;
  p.out_scores = d_out_scores;
  p.out_ids = d_out_ids;
  p.out_counts = d_out_counts;
  p.out_dense = d_out_dense;
  p.out_bm25 = d_out_bm25;
  hipLaunchKernelGGL(hybrid_fuse_kernel, dim3((unsigned)nq), dim3(THREADS), 0, sskd::as_stream(stream), p);
  return sskd::check_launch("hybrid_fuse_kernel");
}

}  // extern "C"
