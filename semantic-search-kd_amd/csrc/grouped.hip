// ------------------------------------------------------------------------- //
// Grouped search (sskd_amd.h): top-k DISTINCT groups by their best row (a document scores as its best chunk).
//
// Step 1 is the unchanged exact row search for k_rows results per query (sskd::exact_search, local ids); step 2 walks
// that ranking and keeps the first row of every group not seen before.  The first k_rows ranks are exact, so the
// groups met among them, in the order they are met, are exactly the first groups of the full walk: the result is
// proven when k groups were found or the ranking ran out of rows, and otherwise the `count` groups written are still
// the exact top-count groups (the caller asks again with a larger k_rows).
// ------------------------------------------------------------------------- //
#include "ranking_walk.h"
#include "search_device.h"
#include "search_host.h"

#include <algorithm>
#include <cfloat>

using sskd::require_shard_rows;

namespace {

struct CollapseParams {
  const float* row_scores;   // [nq][k_rows] the row ranking, (-FLT_MAX, -1) padded
  const int64_t* row_ids;    // local rows
  const int32_t* row_group;  // [n_rows]
  int64_t n_rows;
  int nq;
  int k;
  int k_rows;
  int64_t id_offset;
  float* out_scores;         // [nq][k]
  int64_t* out_ids;
  int32_t* out_groups;
  int32_t* out_count;        // [nq]
  int32_t* unproved;         // [nq]
  int32_t* n_unproved;       // [1], zeroed before the launch
};

constexpr int COLLAPSE_WAVES = 4;

// One wave per query, 64 ranks per step (ranking_walk.h).  kept[] (LDS, k entries per wave) holds the groups written so far.
__global__ __launch_bounds__(COLLAPSE_WAVES * 64) void group_collapse_kernel(CollapseParams p) {
  extern __shared__ int32_t kept_all[];  // [COLLAPSE_WAVES][k]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = blockIdx.x * COLLAPSE_WAVES + wave;
  if (q >= p.nq) return;  // (wave-uniform; the kernel has no workgroup barrier)
  int32_t* const kept = kept_all + wave * p.k;
  const float* rs = p.row_scores + (int64_t)q * p.k_rows;
  const int64_t* ri = p.row_ids + (int64_t)q * p.k_rows;
  float* os = p.out_scores + (int64_t)q * p.k;
  int64_t* oi = p.out_ids + (int64_t)q * p.k;
  int32_t* og = p.out_groups + (int64_t)q * p.k;

  int count = 0;            // (wave-uniform) groups kept
  bool exhausted = false;   // a -1 record was met: the ranking holds every allowed row
  for (int base = 0; base < p.k_rows && count < p.k && !exhausted; base += 64) {
    const int rank = base + lane;
    int64_t row = -1;
    float s = -FLT_MAX;
    if (rank < p.k_rows) {
      row = ri[rank];
      s = rs[rank];
    }
    // a -1 record inside the ranking: the allowed rows ran out (the padding is a suffix)
    bool alive = walk_step<WalkEnd::AnyNegative, false>(rank < p.k_rows, row, p.n_rows, lane, exhausted);
    const int32_t g = alive ? p.row_group[row] : -1;
    // groups kept by earlier steps (every lane reads the same word: an LDS broadcast)
    for (int i = 0; i < count; ++i)
      if (kept[i] == g) alive = false;
    // duplicates inside the step, in rank order: the lowest surviving lane keeps its group, higher lanes holding
    // the same group drop out
    unsigned long long rest = __ballot(alive);
    while (rest) {
      const int l = __ffsll((long long)rest) - 1;
      const int32_t gl = __shfl(g, l);
      const bool dup = alive && lane > l && g == gl;
      if (dup) alive = false;
      rest &= rest - 1;
      rest &= ~__ballot(dup);
    }
    const int pos = walk_pack(alive, lane, count);
    if (alive && pos < p.k) {
      os[pos] = s;
      oi[pos] = row + p.id_offset;
      og[pos] = g;
      kept[pos] = g;
    }
    count = min(p.k, count);
    wave_lds_sync();   // the next step's lanes read what this step's lanes wrote to kept[]
  }
  for (int i = count + lane; i < p.k; i += 64) {
    os[i] = -FLT_MAX;
    oi[i] = -1;
    og[i] = -1;
  }
  if (lane == 0) {
    // stopped at k_rows with rows left to rank: more groups may follow
    const bool open = count < p.k && !exhausted && p.k_rows < p.n_rows;
    p.out_count[q] = count;
    p.unproved[q] = open ? 1 : 0;
    if (open) atomicAdd(p.n_unproved, 1);
  }
}

// workspace of the grouped search: the row ranking, then the exact search's own workspace
struct GroupedWs {
  float* row_scores;
  int64_t* row_ids;
  void* exact;
  size_t exact_bytes;
  size_t bytes;
};

size_t exact_bytes_for(int64_t n_rows, int nq, int k) { return sskd::exact_workspace_bytes(n_rows, nq, k); }

// The exact search's workspace is not monotone in its shape (a query block more means fewer corpus slices, a deeper
// list fewer queries per block).  The size QUERY therefore returns the largest need over every shape at or below the
// asked one: the plan depends on k only through its list depth (k <= 10, <= 16, <= 32, more) and, inside one count
// of query blocks, grows with nq, so the block ends (multiples of 32) and nq itself are the candidates.  The call
// itself needs, and checks, only its own shape's bytes.
size_t exact_bytes_envelope(int64_t n_rows, int nq, int k_rows) {
  const int ks[4] = {std::min(k_rows, 10), std::min(k_rows, 16), std::min(k_rows, SSKD_K_PASS), k_rows};
  size_t best = 0;
  for (int k : ks) {
    best = std::max(best, exact_bytes_for(n_rows, nq, k));
    for (int n = 32; n < nq; n += 32) best = std::max(best, exact_bytes_for(n_rows, n, k));
  }
  return best;
}

GroupedWs grouped_carve(void* base, int64_t n_rows, int nq, int k_rows, bool envelope) {
  sskd::Carver c(base);
  GroupedWs w{};
  w.row_scores = c.take<float>((size_t)nq * k_rows);
  w.row_ids = c.take<int64_t>((size_t)nq * k_rows);
  w.exact_bytes = envelope ? exact_bytes_envelope(n_rows, nq, k_rows) : exact_bytes_for(n_rows, nq, k_rows);
  w.exact = c.take<char>(w.exact_bytes);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" {

size_t sskd_index_search_grouped_workspace_bytes(int64_t n_rows, int nq, int k, int k_rows) {
  if (n_rows < 0 || nq <= 0 || k < 1 || k > k_rows || k_rows > SSKD_K_MAX) return 0;
  return grouped_carve(nullptr, n_rows, nq, k_rows, true).bytes;
}

int sskd_index_search_grouped(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, int k, int k_rows,
                              int64_t id_offset, const uint32_t* d_row_mask, const int32_t* d_row_group,
                              float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_groups, int32_t* d_out_count,
                              int32_t* d_unproved, int32_t* d_n_unproved, void* d_workspace, size_t workspace_bytes,
                              void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "index_search_grouped: n_rows < 0");
  SSKD_REQUIRE(nq >= 0, "index_search_grouped: nq < 0");
  SSKD_REQUIRE(k >= 1, "index_search_grouped: k=%d < 1", k);
  SSKD_REQUIRE(k <= k_rows, "index_search_grouped: k=%d > k_rows=%d", k, k_rows);
  SSKD_REQUIRE(k_rows <= SSKD_K_MAX, "index_search_grouped: k_rows=%d > %d", k_rows, SSKD_K_MAX);
  SSKD_REQUIRE(d_n_unproved, "index_search_grouped: null n_unproved");
  int rc = require_shard_rows("index_search_grouped", n_rows);
  if (rc != SSKD_OK) return rc;
  GroupedWs w{};
  if (nq > 0) {
    w = grouped_carve(d_workspace, n_rows, nq, k_rows, false);
    SSKD_REQUIRE(d_queries && d_out_scores && d_out_ids && d_out_groups && d_out_count && d_unproved,
                 "index_search_grouped: null pointer");
    SSKD_REQUIRE(n_rows == 0 || (d_tiled && d_row_group), "index_search_grouped: null index or row groups");
    if ((rc = sskd::require_workspace("index_search_grouped", d_workspace, workspace_bytes, w.bytes)) != SSKD_OK) return rc;
  }
  hipStream_t st = sskd::as_stream(stream);
  if (hipMemsetAsync(d_n_unproved, 0, sizeof(int32_t), st) != hipSuccess)
    return sskd::fail(SSKD_ERR_HIP, "index_search_grouped: memset failed");
  if (nq == 0) return SSKD_OK;

  // 1. the row ranking: local rows (id_offset 0), k_rows > SSKD_K_PASS through the chained passes
  rc = sskd::exact_search(d_tiled, n_rows, d_queries, nq, k_rows, 0, w.row_scores, w.row_ids, w.exact, w.exact_bytes,
                          stream, nullptr, nullptr, nullptr, nullptr, d_row_mask);
  if (rc != SSKD_OK) return rc;

  // 2. collapse
  CollapseParams cp{};
  cp.row_scores = w.row_scores;
  cp.row_ids = w.row_ids;
  cp.row_group = d_row_group;
  cp.n_rows = n_rows;
  cp.nq = nq;
  cp.k = k;
  cp.k_rows = k_rows;
  cp.id_offset = id_offset;
  cp.out_scores = d_out_scores;
  cp.out_ids = d_out_ids;
  cp.out_groups = d_out_groups;
  cp.out_count = d_out_count;
  cp.unproved = d_unproved;
  cp.n_unproved = d_n_unproved;
  hipLaunchKernelGGL(group_collapse_kernel, dim3((unsigned)sskd::ceil_div(nq, COLLAPSE_WAVES)), dim3(COLLAPSE_WAVES * 64),
                     (size_t)COLLAPSE_WAVES * k * sizeof(int32_t), st, cp);
  return sskd::check_launch("group_collapse_kernel");
}

}  // extern "C"
