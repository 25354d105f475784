// Host-side pieces the search translation units share (internal: not installed).  search.hip defines what is only
// declared here; index_rows.hip, screen.hip, range.hip, grouped.hip, mine.hip, bm25.hip, hybrid.hip, expand.hip and eval.hip
// use it.
#pragma once
#include "common.h"

namespace sskd {

// Rows of one shard: the kernels keep row ids in int32, the last tile's padding rows included.
constexpr int64_t MAX_SHARD_ROWS = ((int64_t)1 << 31) - 64;

inline int require_shard_rows(const char* what, int64_t n_rows) {
  if (n_rows < MAX_SHARD_ROWS) return SSKD_OK;
  return fail(SSKD_ERR_INVALID, "%s: shard too large for int32 row ids", what);
}

// launch plan of the fp32 scan (scan_topk_kernel, range_scan_kernel)
struct Plan {
  int K;          // per-lane list length (template)
  int QB;         // 32-query sub-blocks per workgroup
  int waves;      // waves per workgroup
  int n_qblocks;
  int n_slices;
  int tiles_per_slice;
  int n_tiles;
  int lists_per_query;
  int passes;     // scan passes of K results each (k > K is served by chaining)
  bool pools;     // shared pruning pools on (batch shapes) or off (few tiles per wave)
  size_t part_elems;
  size_t reduce_elems;  // elements of one reduce buffer (0: no reduce step needed); two are kept
};

// Tuning is an explicit argument (sskd_search_tuning) that the caller hands to BOTH the workspace
// query and the search: there is no process-global state behind the hot call.
Plan make_plan(int64_t n_rows, int nq, int k, const sskd_search_tuning* tn = nullptr);

// bytes of the workspace exact_search needs for this shape: the size of the very carve the search uses
size_t exact_workspace_bytes(int64_t n_rows, int nq, int k, const sskd_search_tuning* tn = nullptr);

// the exact search proper; nq_dev (optional) = device-side count of the queries present (<= nq);
// row_mask (optional) = the allow-mask: NULL takes the unmasked kernels
int exact_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                 int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                 void* d_workspace, size_t workspace_bytes, void* stream,
                 const sskd_search_tuning* tuning, void* ev_scan_begin, void* ev_scan_end,
                 const int* nq_dev, const uint32_t* row_mask);

}  // namespace sskd
