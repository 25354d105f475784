// BM25Okapi top-k over an inverted index in HBM (sskd_amd.h "BM25 search").
//
// Replaces the reference's per-query host loop (reference: src/data/bm25.py:162-192 over rank_bm25.BM25Okapi.get_scores:
// one dense N-vector per query token, then a full sort of N scores).  The index is built once on the host: postings in
// CSR by term, each list sorted by row, each posting (int32 row, fp64 w) with w = f (k1 + 1) / (f + k1 (1 - b + b dl /
// avgdl)) already evaluated.  The device only multiplies idf * w and adds:
//   bm25_score_select_kernel  one workgroup = one tile of TILE_ROWS consecutive rows x one query.  fp64 accumulators in
//                             LDS, term at a time in query order (a barrier between tokens; inside one token a row
//                             occurs at most once, so there are no atomics on the scores and every row's sum has the
//                             query's order), then the tile's best min(k, rows) under (score descending, row ascending)
//                             by a radix select on an order-preserving key, written sorted into the workspace.
//   bm25_merge_kernel         one workgroup per query: the same select over the tiles' records.
// The product and the sum stay two roundings (no fma), as numpy evaluates `score += idf * w_array`.
#include "radix_select.h"
#include "search_host.h"   // sskd::MAX_SHARD_ROWS: rows are int32 per index

#pragma clang fp contract(off)

namespace {

constexpr int TILE_ROWS = 4096;    // 32 KiB of fp64 accumulators: four workgroups per CU by LDS
constexpr int THREADS = 256;
constexpr int BM25_K_MAX = 256;
constexpr int TOKEN_BATCH = THREADS / 2;   // query tokens whose posting segments are located at once (2 bounds each)
constexpr size_t WORKSPACE_BUDGET = (size_t)256 << 20;         // what the size query asks for at most (if one query fits)

struct Rec {
  double score;
  int32_t row;   // -1: empty slot
  int32_t pad;
};
static_assert(sizeof(Rec) == 16, "record layout");

// the select of both kernels (radix_select.h): order-preserving fp64 keys, the kk largest handed out in rank order
using sskd::radix::key_score;
using sskd::radix::score_key;
using sskd::radix::select_sorted;
using sskd::radix::SelectShared;
static_assert(THREADS == sskd::radix::SELECT_THREADS && BM25_K_MAX == sskd::radix::SELECT_K_MAX, "select geometry");

struct ScoreParams {
  const int64_t* term_offsets;   // [n_terms + 1]
  const int32_t* post_rows;      // per term ascending
  const double* post_w;
  const double* idf;             // [n_terms]
  int64_t n_rows;
  int64_t n_terms;
  const int64_t* q_lims;         // [nq + 1]
  const int32_t* q_terms;
  int q0;                        // first query of this chunk
  int k;
  int tiles;
  Rec* records;                  // [chunk][tiles][k]
};

__global__ __launch_bounds__(THREADS) void bm25_score_select_kernel(ScoreParams p) {
  __shared__ double acc[TILE_ROWS];
  __shared__ int64_t seg[2 * TOKEN_BATCH];
  __shared__ double seg_idf[TOKEN_BATCH];
  __shared__ SelectShared sh;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  const int ql = blockIdx.y;
  const int64_t tile_start = (int64_t)tile * TILE_ROWS;
  const int rows = (int)min((int64_t)TILE_ROWS, p.n_rows - tile_start);
  for (int i = tid; i < TILE_ROWS; i += THREADS) acc[i] = 0.0;
  const int64_t q_lo = p.q_lims[p.q0 + ql], q_hi = p.q_lims[p.q0 + ql + 1];
  for (int64_t b = q_lo; b < q_hi; b += TOKEN_BATCH) {
    const int nb = (int)min((int64_t)TOKEN_BATCH, q_hi - b);
    __syncthreads();   // the accumulators are zeroed / the previous batch's segments are consumed
    if (tid < 2 * nb) {
      // thread 2j finds where token j's posting list enters the tile, thread 2j + 1 where it leaves it
      const int64_t t = p.q_terms[b + (tid >> 1)];
      const bool known = t >= 0 && t < p.n_terms;
      int64_t at = 0;
      if (known) {
        int64_t lo = p.term_offsets[t], hi = p.term_offsets[t + 1];
        const int64_t target = tile_start + ((tid & 1) ? rows : 0);
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if ((int64_t)p.post_rows[mid] < target) lo = mid + 1;
          else hi = mid;
        }
        at = lo;
      }
      seg[tid] = at;
      if (!(tid & 1)) seg_idf[tid >> 1] = known ? p.idf[t] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
      const int64_t s0 = seg[2 * j], s1 = seg[2 * j + 1];
      const double idf = seg_idf[j];
      for (int64_t i = s0 + tid; i < s1; i += THREADS) {
        const unsigned at = (unsigned)((int64_t)p.post_rows[i] - tile_start);
        if (at < (unsigned)rows) {
          const double term = idf * p.post_w[i];   // two roundings: the translation unit has contraction off
          acc[at] = acc[at] + term;
        }
      }
      __syncthreads();   // the next token may hit the same rows
    }
  }
  __syncthreads();
  const int kk = min(p.k, rows);
  Rec* out = p.records + ((int64_t)ql * p.tiles + tile) * p.k;
  for (int i = kk + tid; i < p.k; i += THREADS) out[i] = Rec{-INFINITY, -1, 0};
  // lo = the local row, inverted (a lower row wins a tie), in the top 16 bits
  select_sorted<2>(
      sh, rows, kk,
      [&](int i, uint64_t& hi, uint32_t& lo) {
        hi = score_key(acc[i]);
        lo = (uint32_t)(0xFFFF - i) << 16;
        return true;
      },
      [&](int rank, uint64_t hi, uint32_t lo) {
        out[rank] = Rec{key_score(hi), (int32_t)(tile_start + (0xFFFF - (int)(lo >> 16))), 0};
      });
}

struct MergeParams {
  const Rec* records;   // [chunk][slots]
  int slots;            // tiles * k
  int64_t n_rows;
  int q0;
  int k;
  double* out_scores;   // [nq][k]
  int64_t* out_ids;
};

__global__ __launch_bounds__(THREADS) void bm25_merge_kernel(MergeParams p) {
  __shared__ SelectShared sh;
  const int tid = threadIdx.x;
  const int ql = blockIdx.x;
  const Rec* rec = p.records + (int64_t)ql * p.slots;
  double* os = p.out_scores + (int64_t)(p.q0 + ql) * p.k;
  int64_t* oi = p.out_ids + (int64_t)(p.q0 + ql) * p.k;
  const int kk = (int)min((int64_t)p.k, p.n_rows);
  for (int i = kk + tid; i < p.k; i += THREADS) {
    os[i] = -INFINITY;
    oi[i] = -1;
  }
  select_sorted<4>(
      sh, p.slots, kk,
      [&](int i, uint64_t& hi, uint32_t& lo) {
        const Rec r = rec[i];
        hi = score_key(r.score);
        lo = 0xFFFFFFFFu - (uint32_t)r.row;
        return r.row >= 0;
      },
      [&](int rank, uint64_t hi, uint32_t lo) {
        os[rank] = key_score(hi);
        oi[rank] = (int64_t)(0xFFFFFFFFu - lo);
      });
}

struct Plan {
  int tiles;
  size_t per_query;   // record bytes of one query
};

inline Plan make_plan(int64_t n_rows, int k) {
  Plan pl;
  pl.tiles = (int)sskd::ceil_div(n_rows, TILE_ROWS);
  pl.per_query = sskd::align256((size_t)pl.tiles * (size_t)k * sizeof(Rec));
  if (pl.per_query == 0) pl.per_query = 256;
  return pl;
}

// min(nq queries, max(budget, one query)): monotone in nq and in k
inline size_t plan_bytes(const Plan& pl, int nq) {
  const size_t all = pl.per_query * (size_t)nq;
  const size_t cap = pl.per_query > WORKSPACE_BUDGET ? pl.per_query : WORKSPACE_BUDGET;
  return all < cap ? all : cap;
}

inline bool shape_ok(int64_t n_rows, int nq, int k) {
  return n_rows >= 0 && n_rows < sskd::MAX_SHARD_ROWS && nq >= 0 && k >= 1 && k <= BM25_K_MAX;
}

}  // namespace

extern "C" {

size_t sskd_bm25_search_workspace_bytes(int64_t n_rows, int nq, int k) {
  if (!shape_ok(n_rows, nq, k) || nq == 0) return 0;
  return plan_bytes(make_plan(n_rows, k), nq);
}

int sskd_bm25_search_plan(int64_t n_rows, int nq, int k, int* tile_rows, int* tiles, int* queries_per_chunk) {
  SSKD_REQUIRE(n_rows >= 0, "bm25_search_plan: n_rows < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "bm25_search_plan: index too large for int32 row ids");
  SSKD_REQUIRE(nq >= 0, "bm25_search_plan: nq < 0");
  SSKD_REQUIRE(k >= 1 && k <= BM25_K_MAX, "bm25_search_plan: k=%d outside [1, %d]", k, BM25_K_MAX);
  const Plan pl = make_plan(n_rows, k);
  if (tile_rows) *tile_rows = TILE_ROWS;
  if (tiles) *tiles = pl.tiles;
  if (queries_per_chunk) {
    const size_t fit = nq ? plan_bytes(pl, nq) / pl.per_query : 0;
    *queries_per_chunk = (int)(fit < 65535 ? fit : 65535);
  }
  return SSKD_OK;
}

int sskd_bm25_search(const int64_t* d_term_offsets, const int32_t* d_post_rows, const double* d_post_w,
                     const double* d_idf, int64_t n_rows, int64_t n_terms, const int64_t* d_q_lims,
                     const int32_t* d_q_terms, int nq, int k, double* d_out_scores, int64_t* d_out_ids,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "bm25_search: n_rows < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "bm25_search: index too large for int32 row ids");
  SSKD_REQUIRE(n_terms >= 0 && n_terms <= INT32_MAX, "bm25_search: n_terms outside [0, 2^31)");
  SSKD_REQUIRE(nq >= 0, "bm25_search: nq < 0");
  SSKD_REQUIRE(k >= 1 && k <= BM25_K_MAX, "bm25_search: k=%d outside [1, %d]", k, BM25_K_MAX);
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_term_offsets && d_post_rows && d_post_w && d_idf, "bm25_search: null index table");
  SSKD_REQUIRE(d_q_lims && d_q_terms, "bm25_search: null query table");
  SSKD_REQUIRE(d_out_scores && d_out_ids, "bm25_search: null output");
  const Plan pl = make_plan(n_rows, k);
  if (int rc = sskd::require_workspace("bm25_search", d_workspace, workspace_bytes, pl.per_query)) return rc;
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0, "bm25_search: workspace must be 16-byte aligned");
  size_t fit = workspace_bytes / pl.per_query;
  if (fit > 65535) fit = 65535;   // grid.y
  const int chunk = (int)(fit < (size_t)nq ? fit : (size_t)nq);
  hipStream_t st = sskd::as_stream(stream);
  for (int q0 = 0; q0 < nq; q0 += chunk) {
    const int n = nq - q0 < chunk ? nq - q0 : chunk;
    // (the chunks reuse the workspace: stream order keeps a chunk's merge ahead of the next chunk's scoring)
    if (pl.tiles > 0) {
      ScoreParams sp{};
      sp.term_offsets = d_term_offsets;
      sp.post_rows = d_post_rows;
      sp.post_w = d_post_w;
      sp.idf = d_idf;
      sp.n_rows = n_rows;
      sp.n_terms = n_terms;
      sp.q_lims = d_q_lims;
      sp.q_terms = d_q_terms;
      sp.q0 = q0;
      sp.k = k;
      sp.tiles = pl.tiles;
      sp.records = static_cast<Rec*>(d_workspace);
      hipLaunchKernelGGL(bm25_score_select_kernel, dim3((unsigned)pl.tiles, (unsigned)n), dim3(THREADS), 0, st, sp);
      if (int rc = sskd::check_launch("bm25_score_select_kernel")) return rc;
    }
    MergeParams mp{};
    mp.records = static_cast<const Rec*>(d_workspace);
    mp.slots = pl.tiles * k;
    mp.n_rows = n_rows;
    mp.q0 = q0;
    mp.k = k;
    mp.out_scores = d_out_scores;
    mp.out_ids = d_out_ids;
    hipLaunchKernelGGL(bm25_merge_kernel, dim3((unsigned)n), dim3(THREADS), 0, st, mp);
    if (int rc = sskd::check_launch("bm25_merge_kernel")) return rc;
  }
  return SSKD_OK;
}

}  // extern "C"
