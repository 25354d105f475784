// Device helpers the two inverted-list translation units share (internal: not installed): ivf.hip scans fp32 rows,
// pq.hip scans product-quantisation codes over the same lists.  Both need to know how a workgroup finds ITS positions of
// the sequence a query probes (a prefix sum over the list lengths, 256 probes at a time) and how a position becomes a
// row number.  (Each keeps its running top list itself: ivf.hip an unsorted list of k slots, pq.hip, with ten times as
// many records per workgroup, a pool that it sorts and cuts.)
#pragma once
#include "search_device.h"

namespace {

constexpr int IVF_THREADS = 256;
constexpr int IVF_PROBES = 256;                                // probes per prefix block
constexpr int IVF_K_MAX = 256;
constexpr int IVF_NLIST_MAX = 65536;
constexpr int IVF_CUS = 256;                                   // the plans are fixed from host-known numbers only

// the LDS arrays of one prefix block
struct IvfPrefix {
  int64_t* pre;    // [IVF_PROBES + 1] exclusive prefix of the block's list lengths
  int64_t* off;    // [IVF_PROBES]     first list_rows entry of every list of the block
  int64_t* wsum;   // [IVF_THREADS / 64]
};

// Prefix of probe block pb of one query into s.pre / s.off; returns the block's total (workgroup-uniform).  An empty
// list, a -1 probe and a list number outside [0, nlist) are lists of length 0.  Two barriers inside; the caller puts one
// more between this call and the first read of the prefix.
__device__ inline int64_t ivf_prefix_block(const IvfPrefix& s, const int64_t* __restrict__ probe, int nprobe, int nlist,
                                           const int64_t* __restrict__ list_offsets, int pb, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  const int j = pb * IVF_PROBES + tid;
  int64_t len = 0, off = 0;
  if (j < nprobe) {
    const int64_t l = probe[j];
    if (l >= 0 && l < nlist) {
      off = list_offsets[l];
      len = list_offsets[l + 1] - off;
      if (len < 0 || off < 0) len = 0;
    }
  }
  int64_t x = len;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  __syncthreads();   // nobody still reads the previous block's prefix
  if (lane == 63) s.wsum[wave] = x;
  __syncthreads();
  int64_t base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < IVF_THREADS / 64; ++w) {
    if (w < wave) base += s.wsum[w];
    total += s.wsum[w];
  }
  s.pre[tid + 1] = base + x;
  if (tid == 0) s.pre[0] = 0;
  s.off[tid] = off;
  return total;
}

// the list_rows entry of position v of the current block (relative to the block's first position); `probe_in_block`
// receives which of the block's probes the position belongs to
__device__ inline int64_t ivf_entry_at(const IvfPrefix& s, int64_t v, int n_in_block, int& probe_in_block) {
  int a = 0, b = n_in_block;   // first j in (a, b] with pre[j] > v; the list is j - 1
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (s.pre[mid] > v) b = mid; else a = mid;
  }
  probe_in_block = a;
  return s.off[a] + (v - s.pre[a]);
}

// row number of list_rows entry `at`, -1 when the entry or the row is outside the index or the row's mask bit is clear
__device__ inline int ivf_row_of_entry(int64_t at, const int32_t* __restrict__ list_rows,
                                       const uint32_t* __restrict__ row_mask, int64_t n_rows) {
  if (at < 0 || at >= n_rows) return -1;
  const int r = list_rows[at];
  if (r < 0 || r >= n_rows) return -1;
  if (!row_allowed(row_mask, r)) return -1;
  return r;
}

// row number at position v (< end, else -1) of the current block
__device__ inline int ivf_row_at(const IvfPrefix& s, int64_t v, int64_t end, int n_in_block,
                                 const int32_t* __restrict__ list_rows, const uint32_t* __restrict__ row_mask,
                                 int64_t n_rows) {
  if (v >= end) return -1;
  int j;
  return ivf_row_of_entry(ivf_entry_at(s, v, n_in_block, j), list_rows, row_mask, n_rows);
}

}  // namespace
