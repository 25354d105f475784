// Near-duplicate clusters (sskd_amd.h): connected components of the self-join's pairs, by union-find in HBM.
//
// State: parent[r] (int32, -1 = the row takes no part) and degree[r].  Every link puts the LARGER root under the SMALLER
// one, and every other write to parent (path halving) replaces a value by a smaller ancestor.  Hence, at every moment,
//   (a) parent[r] <= r, so a chain r, parent[r], parent[parent[r]], ... strictly decreases until it meets a row that
//       is its own parent: no cycle can form and every walk ends;
//   (b) every value parent[r] ever held is an ancestor of r in every later state (trees only grow at their roots), so
//       a stale read yields an older ancestor - a longer walk, never a foreign tree.
// A row stops being a root only through a successful compare-and-swap on its own entry, so correctness rests on that
// CAS alone: a find that ended on a former root makes the CAS fail (or links under a row of the same tree, which is
// still a correct link), and the failed CAS returns the entry's present value to walk on from.  When all calls are
// done every component is one tree whose root, by (a), is its smallest row - whatever order the edges were taken in.
#include "search_host.h"

namespace {

using namespace sskd;

constexpr int LINK_THREADS = 256;   // 4 waves: one wave per query row at a time
constexpr int LINK_MAX_BLOCKS = 4096;
constexpr int ROW_THREADS = 256;    // the per-row kernels: one thread per row

__device__ inline int load_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's tree as far as this thread can see it (possibly a former root: the caller's CAS decides).  Halves the
// path on the way: parent[x] drops to its grandparent through an atomic min, so a lost or late write changes nothing.
__device__ inline int find_root(int* parent, int x) {
  int p = load_agent(parent + x);
  while (p != x) {
    const int gp = load_agent(parent + p);
    if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = gp;
  }
  return x;
}

// Unites the trees of rows a and b (both take part).
__device__ inline void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;   // one walk's end reached by both: the same tree
    const int big = a > b ? a : b, small = a > b ? b : a;
    int expected = big;
    if (__hip_atomic_compare_exchange_strong(parent + big, &expected, small, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    // big was no root any more: `expected` now holds its parent, a smaller row of its tree; walk on from there
    a = expected;
    b = small;
  }
}

__global__ __launch_bounds__(ROW_THREADS) void dup_init_kernel(int64_t n_rows, const uint32_t* __restrict__ mask,
                                                               int* __restrict__ parent, int* __restrict__ degree) {
  const int64_t r = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
  if (r >= n_rows) return;
  const bool in = !mask || ((mask[r >> 5] >> (r & 31)) & 1u);
  parent[r] = in ? (int)r : -1;
  degree[r] = 0;
}

// One wave per query row i = query_row0 + q (waves stride over the batch); its lanes stride over the row's entries.
__global__ __launch_bounds__(LINK_THREADS) void dup_link_kernel(const int64_t* __restrict__ lims, const int64_t* __restrict__ ids,
                                                                int nq, int64_t max_results, int64_t query_row0,
                                                                int64_t id_offset, int64_t n_rows,
                                                                const int32_t* __restrict__ group, int scope, int* parent,
                                                                int* degree, int* overflow) {
  const int64_t total = lims[nq];
  if (total > max_results) {   // the result arrays are not valid: link nothing, add nothing
    if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 1;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (LINK_THREADS / 64) + (threadIdx.x >> 6);
  const int n_waves = gridDim.x * (LINK_THREADS / 64);
  for (int q = wave; q < nq; q += n_waves) {
    const int i = (int)(query_row0 + q);
    if (load_agent(parent + i) < 0) continue;
    const int gi = scope ? group[i] : 0;
    int64_t begin = lims[q], end = lims[q + 1];
    if (begin < 0) begin = 0;            // lims of a range search ascend from 0 to total; a list that does not can
    if (end > total) end = total;        // lose entries here but never reads past the arrays
    int mine = 0;
    for (int64_t t = begin + lane; t < end; t += 64) {
      const int64_t j64 = ids[t] - id_offset;
      if (j64 <= i || j64 >= n_rows) continue;
      const int j = (int)j64;
      if (load_agent(parent + j) < 0) continue;
      if (scope && ((scope == 1) == (group[j] == gi))) continue;   // 1: different groups only, 2: the same group only
      ++mine;
      __hip_atomic_fetch_add(degree + j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      unite(parent, i, j);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (lane == 0 && mine) __hip_atomic_fetch_add(degree + i, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Labels, step 1: parent[r] becomes the root (concurrent threads may meet either value: both are ancestors), size
// is zeroed, rep starts as the row itself, and the roots and the rows taking part are counted (one add per wave).
__global__ __launch_bounds__(ROW_THREADS) void dup_flatten_kernel(int64_t n_rows, int* parent, int* __restrict__ rep,
                                                                  int* __restrict__ size, int* counts) {
  const int64_t r = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
  bool in = false, root = false;
  if (r < n_rows) {
    int p = load_agent(parent + r);
    in = p >= 0;
    if (in) {
      root = p == (int)r;
      for (int g = load_agent(parent + p); g != p; g = load_agent(parent + p)) p = g;
      if (!root) __hip_atomic_store(parent + r, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    rep[r] = in ? (int)r : -1;
    size[r] = 0;
  }
  const int n_in = __popcll(__ballot(in)), n_root = __popcll(__ballot(root));
  if ((threadIdx.x & 63) == 0) {
    if (n_root) atomicAdd(counts, n_root);
    if (n_in) atomicAdd(counts + 1, n_in);
  }
}

// Labels, step 2 (parent is flat): count every row at its root and, for keep = densest, offer it as the root's
// representative - the row with the largest degree, ties to the smaller row.  The offer is a CAS loop on rep[root]: every
// success moves rep[root] strictly up in that order, so it ends, and the maximum does not depend on the order of offers.
__global__ __launch_bounds__(ROW_THREADS) void dup_elect_kernel(int64_t n_rows, const int* __restrict__ parent,
                                                                const int* __restrict__ degree, int keep, int* rep, int* size) {
  const int64_t r64 = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
  if (r64 >= n_rows) return;
  const int r = (int)r64, root = parent[r];
  if (root < 0) return;
  atomicAdd(size + root, 1);
  if (!keep || root == r) return;   // the root is rep[root]'s first value: it has made its offer
  const int mine = degree[r];
  int cur = load_agent(rep + root);
  for (;;) {
    const int theirs = degree[cur];
    if (!(mine > theirs || (mine == theirs && r < cur))) return;
    int expected = cur;
    if (__hip_atomic_compare_exchange_strong(rep + root, &expected, r, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    cur = expected;
  }
}

// Labels, step 3: every other row of a component takes its root's representative.
__global__ __launch_bounds__(ROW_THREADS) void dup_spread_kernel(int64_t n_rows, const int* __restrict__ parent, int* rep) {
  const int64_t r = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
  if (r >= n_rows) return;
  const int root = parent[r];
  if (root >= 0 && root != (int)r) rep[r] = rep[root];   // rep[root] is written by no thread of this launch
}

int check_rows(const char* what, int64_t n_rows) {
  if (n_rows < 0) return fail(SSKD_ERR_INVALID, "%s: n_rows < 0", what);
  return require_shard_rows(what, n_rows);
}

inline unsigned row_blocks(int64_t n_rows) { return (unsigned)ceil_div(n_rows, ROW_THREADS); }

}  // namespace

extern "C" {

int sskd_dup_init(int64_t n_rows, const uint32_t* d_row_mask, int32_t* d_parent, int32_t* d_degree, void* stream) {
  const int rc = check_rows("dup_init", n_rows);
  if (rc != SSKD_OK) return rc;
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_parent && d_degree, "dup_init: null pointer");
  hipLaunchKernelGGL(dup_init_kernel, dim3(row_blocks(n_rows)), dim3(ROW_THREADS), 0, sskd::as_stream(stream), n_rows,
                     d_row_mask, d_parent, d_degree);
  return sskd::check_launch("dup_init_kernel");
}

int sskd_dup_link(const int64_t* d_lims, const int64_t* d_ids, int nq, int64_t max_results, int64_t query_row0,
                  int64_t id_offset, int64_t n_rows, const int32_t* d_row_group, int scope, int32_t* d_parent,
                  int32_t* d_degree, int32_t* d_overflow, void* stream) {
  SSKD_REQUIRE(nq >= 0, "dup_link: nq < 0");
  SSKD_REQUIRE(max_results >= 0, "dup_link: max_results < 0");
  const int rc = check_rows("dup_link", n_rows);
  if (rc != SSKD_OK) return rc;
  SSKD_REQUIRE(scope >= 0 && scope <= 2, "dup_link: scope=%d is not 0 (all), 1 (across groups) or 2 (within groups)", scope);
  SSKD_REQUIRE(scope == 0 || d_row_group, "dup_link: scope=%d needs the row groups", scope);
  SSKD_REQUIRE(query_row0 >= 0 && query_row0 + nq <= n_rows, "dup_link: query rows [%lld, %lld) outside [0, %lld)",
               (long long)query_row0, (long long)(query_row0 + nq), (long long)n_rows);
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_lims && d_parent && d_degree && d_overflow, "dup_link: null pointer");
  SSKD_REQUIRE(d_ids || max_results == 0, "dup_link: null ids with max_results > 0");
  const int64_t blocks = ceil_div(nq, LINK_THREADS / 64);
  hipLaunchKernelGGL(dup_link_kernel, dim3((unsigned)(blocks < LINK_MAX_BLOCKS ? blocks : LINK_MAX_BLOCKS)),
                     dim3(LINK_THREADS), 0, sskd::as_stream(stream), d_lims, d_ids, nq, max_results, query_row0, id_offset,
                     n_rows, d_row_group, scope, d_parent, d_degree, d_overflow);
  return sskd::check_launch("dup_link_kernel");
}

int sskd_dup_labels(int64_t n_rows, int32_t* d_parent, const int32_t* d_degree, int keep, int32_t* d_rep, int32_t* d_size,
                    int32_t* d_counts, void* stream) {
  const int rc = check_rows("dup_labels", n_rows);
  if (rc != SSKD_OK) return rc;
  SSKD_REQUIRE(keep == 0 || keep == 1, "dup_labels: keep=%d is not 0 (first) or 1 (densest)", keep);
  SSKD_REQUIRE(d_counts, "dup_labels: null pointer");
  SSKD_REQUIRE(n_rows == 0 || (d_parent && d_degree && d_rep && d_size), "dup_labels: null pointer");
  hipStream_t st = sskd::as_stream(stream);
  if (hipMemsetAsync(d_counts, 0, 2 * sizeof(int32_t), st) != hipSuccess)
    return sskd::fail(SSKD_ERR_HIP, "dup_labels: cannot zero the counts");
  if (n_rows == 0) return SSKD_OK;
  const dim3 grid(row_blocks(n_rows)), block(ROW_THREADS);
  hipLaunchKernelGGL(dup_flatten_kernel, grid, block, 0, st, n_rows, d_parent, d_rep, d_size, d_counts);
  hipLaunchKernelGGL(dup_elect_kernel, grid, block, 0, st, n_rows, d_parent, d_degree, keep, d_rep, d_size);
  hipLaunchKernelGGL(dup_spread_kernel, grid, block, 0, st, n_rows, d_parent, d_rep);
  return sskd::check_launch("dup_labels");
}

}  // extern "C"
