// Hard-negative selection over a row ranking (ANCE refresh, sskd_amd.h "Hard-negative mining").
//
// Replaces the per-query host loop behind the reference's ANCEMiner rule (reference: src/mining/miners.py:232-247):
//     max_pos     = max(score(q, positive rows))            (0.0 without positives)
//     adversarial = ranks with  score >= max_pos - margin   (decided in fp64)
//     negatives   = the first top_k adversarial ranks (the ranking is already the stable descending order)
// One wave per query: it scores the query's positive rows with the fma chain of the screened search's exact re-scoring
// (screen.hip, "exact scores, 64 candidates per round"), so a positive scores with the bits a search returns for that
// row, then walks the ranking 64 ranks per round and packs the survivors in rank order (ranking_walk.h: ANY id < 0 ends it).
#include "ranking_walk.h"
#include "search_device.h"
#include "search_host.h"

#include <cfloat>

namespace {

constexpr int MINE_WAVES = 4;

struct MineParams {
  const float* rows;           // the index: row-major fp32 [n_rows][DIM]
  const float* queries;        // [nq][DIM]
  const float* rank_scores;    // [nq][search_k] descending, (-FLT_MAX, -1) padded
  const int64_t* rank_ids;     // local rows
  const int64_t* pos_lims;     // [nq + 1]
  const int32_t* pos_rows;     // local rows
  const int32_t* row_group;    // [n_rows] or null
  int64_t n_rows;
  int nq;
  int search_k;
  int top_k;
  double margin;
  int64_t id_offset;
  float* out_scores;           // [nq][top_k]
  int64_t* out_ids;
  int32_t* out_counts;         // [nq]
  float* out_max_pos;          // [nq]
};

// One wave per query.  The query sits in LDS (one 1 536 B slot per wave); the kernel has no workgroup barrier.
__global__ __launch_bounds__(MINE_WAVES * 64) void mine_select_kernel(MineParams p) {
  __shared__ float4 q_all[MINE_WAVES][CHUNKS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = blockIdx.x * MINE_WAVES + wave;
  if (q >= p.nq) return;  // (wave-uniform)
  float4* const q4 = q_all[wave];
  {
    const float4* src = reinterpret_cast<const float4*>(p.queries) + (int64_t)q * CHUNKS;
    q4[lane] = src[lane];
    if (lane < CHUNKS - 64) q4[64 + lane] = src[64 + lane];
  }
  wave_lds_sync();   // every lane reads what the other lanes of its wave wrote
  const float* qv = reinterpret_cast<const float*>(q4);

  // ---- positives: one lane per row, 64 per round.  A row outside the index is no positive at all.
  const int64_t lo = p.pos_lims[q];
  const int64_t end = p.pos_lims[q + 1];
  const int64_t hi = (p.pos_rows && end > lo) ? end : lo;
  float best = -INFINITY;
  bool any_nan = false;
  int n_pos = 0;  // (wave-uniform) positives scored
  for (int64_t b = lo; b < hi; b += 64) {
    const int64_t j = b + lane;
    const int64_t row = j < hi ? (int64_t)p.pos_rows[j] : -1;
    const bool valid = row >= 0 && row < p.n_rows;
    if (valid) {
      const float4* src = reinterpret_cast<const float4*>(p.rows) + row * CHUNKS;
      const float acc = row_score_fma(src, qv);
      if (acc != acc) any_nan = true;
      best = fmaxf(best, acc);
    }
    n_pos += __popcll(__ballot(valid));
  }
  best = wave_max(best);
  // a NaN positive makes the maximum NaN, and every comparison below false (as ndarray.max() does)
  const float max_pos = n_pos == 0 ? 0.0f : (__any(any_nan) ? __builtin_nanf("") : best);
  const double threshold = (double)max_pos - p.margin;

  // ---- the ranking, 64 ranks per round
  const float* rs = p.rank_scores + (int64_t)q * p.search_k;
  const int64_t* ri = p.rank_ids + (int64_t)q * p.search_k;
  float* os = p.out_scores + (int64_t)q * p.top_k;
  int64_t* oi = p.out_ids + (int64_t)q * p.top_k;
  int count = 0;      // (wave-uniform) ranks kept so far
  bool ended = false; // a negative id was met: nothing behind it counts
  for (int base = 0; base < p.search_k && !ended; base += 64) {
    const int rank = base + lane;
    int64_t row = -1;
    float s = -FLT_MAX;
    if (rank < p.search_k) {
      row = ri[rank];
      s = rs[rank];
    }
    bool alive = walk_step<WalkEnd::AnyNegative>(rank < p.search_k, row, p.n_rows, lane, ended);
    const int32_t g = (alive && p.row_group) ? p.row_group[row] : -1;
    // (every lane reads the same positive: wave-uniform loads)
    for (int64_t j = lo; j < hi; ++j) {
      const int64_t pr = p.pos_rows[j];
      if (pr < 0 || pr >= p.n_rows) continue;
      if (row == pr) alive = false;
      if (p.row_group && g == p.row_group[pr]) alive = false;
    }
    const bool keep = alive && (double)s >= threshold;
    const int pos = walk_pack(keep, lane, count);
    if (keep && pos < p.top_k) {
      os[pos] = s;
      oi[pos] = row + p.id_offset;
    }
  }
  for (int i = min(count, p.top_k) + lane; i < p.top_k; i += 64) {
    os[i] = -FLT_MAX;
    oi[i] = -1;
  }
  if (lane == 0) {
    p.out_counts[q] = count;
    p.out_max_pos[q] = max_pos;
  }
}

}  // namespace

extern "C" {

int sskd_index_mine_select(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                           const float* d_rank_scores, const int64_t* d_rank_ids, int search_k,
                           const int64_t* d_pos_lims, const int32_t* d_pos_rows, const int32_t* d_row_groups,
                           double margin, int top_k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                           int32_t* d_out_counts, float* d_out_max_pos, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "index_mine_select: n_rows < 0");
  SSKD_REQUIRE(nq >= 0, "index_mine_select: nq < 0");
  SSKD_REQUIRE(top_k >= 1, "index_mine_select: top_k=%d < 1", top_k);
  SSKD_REQUIRE(top_k <= search_k, "index_mine_select: top_k=%d > search_k=%d", top_k, search_k);
  SSKD_REQUIRE(search_k <= SSKD_K_MAX, "index_mine_select: search_k=%d > %d", search_k, SSKD_K_MAX);
  SSKD_REQUIRE(margin == margin, "index_mine_select: margin is NaN");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "index_mine_select: shard too large for int32 row ids");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_queries && d_rank_scores && d_rank_ids && d_pos_lims && d_out_scores && d_out_ids && d_out_counts &&
                   d_out_max_pos,
               "index_mine_select: null pointer");
  SSKD_REQUIRE(n_rows == 0 || d_tiled, "index_mine_select: null index");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_queries) % 16 == 0 && reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0,
               "index_mine_select: queries and index must be 16-byte aligned");
  MineParams p{};
  p.rows = d_tiled;
  p.queries = d_queries;
  p.rank_scores = d_rank_scores;
  p.rank_ids = d_rank_ids;
  p.pos_lims = d_pos_lims;
  p.pos_rows = d_pos_rows;
  p.row_group = d_row_groups;
  p.n_rows = n_rows;
  p.nq = nq;
  p.search_k = search_k;
  p.top_k = top_k;
  p.margin = margin;
  p.id_offset = id_offset;
  p.out_scores = d_out_scores;
  p.out_ids = d_out_ids;
  p.out_counts = d_out_counts;
  p.out_max_pos = d_out_max_pos;
  hipLaunchKernelGGL(mine_select_kernel, dim3((unsigned)sskd::ceil_div(nq, MINE_WAVES)), dim3(MINE_WAVES * 64), 0,
                     sskd::as_stream(stream), p);
  return sskd::check_launch("mine_select_kernel");
}

}  // extern "C"
