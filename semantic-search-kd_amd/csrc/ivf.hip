// Inverted-file search over the flat index (sskd_amd.h "IVF index").
//
// The reference names an `ivf_pq` index type in configs/index.yaml:4, 13-19 (nlist / nprobe, "for >50M vectors") beside the
// HNSW one it builds; this file is the IVF half over uncompressed rows (pq.hip is the PQ half, over the same lists).  WHICH rows a query looks at is approximate (the
// rows of the nprobe lists whose centroids score best); every score and every order is exact: a row is scored by one lane
// running row_score_fma, the fma chain of the exact scan, so an IVF search returns bit for bit what the exact search
// returns under an allow-mask of the probed lists' rows.
//
// ivf_scan_kernel, one workgroup per (part p, query q).  The rows q probes form one virtual sequence of L_q = sum of the
// probed lists' lengths; the workgroup owns positions [p L_q / P, (p + 1) L_q / P) of it and finds them from a prefix sum
// over the list lengths in LDS (256 probes at a time), so the split is balanced however skewed the lists are, and an
// empty list or a -1 probe is a list of length 0 and nothing more.  A part is walked in chunks of 32 rows, staged as in
// row_stage.h:
//   wave 1   turns positions into row numbers two chunks ahead (binary search in the prefix, list_rows, the mask bit)
//   all      load the NEXT chunk's rows into registers
//   wave 0   scores the CURRENT chunk out of LDS meanwhile, one lane per row, and offers the scores to the running top-k
//   all      barrier, registers -> LDS, barrier.
// The running top-k is an unsorted list of k slots in LDS with its worst entry cached in registers; a row enters only if
// it ranks before that entry (ranks_before: score descending, then lower id).  Each workgroup writes its list UNSORTED
// to its [k] slots of the [P, nq, k] partials, padded with (-FLT_MAX, -1); sskd_topk_merge orders and cuts them, in two
// steps when there are many (ivf_split).
//
// ivf_list_sums_kernel: the centroid update of the k-means.  One wave per (list, 64 columns) adds the list's rows in CSR
// order into one fp64 accumulator per column - one fixed order per output element and no atomics, so two runs agree bit
// for bit.
#include "ivf_device.h"
#include "row_stage.h"
#include "search_host.h"

#include <algorithm>
#include <cfloat>

namespace {

constexpr int IVF_MAX_PARTS = 1024;
constexpr int IVF_MERGE_CAND = 2048;                           // parts * k: the candidates of one query
constexpr int IVF_MERGE_DIRECT = 512;                          // up to here one merge step joins them
static_assert(IVF_THREADS == STAGE_THREADS, "ivf_scan_kernel's workgroup is the staging workgroup");

struct IvfParams {
  const float* rows;            // the index: row-major fp32 [n_rows][DIM]
  const float* queries;         // [nq][DIM], prepared
  const int64_t* probe;         // [nq][nprobe] list numbers, -1 = none
  const int64_t* list_offsets;  // [nlist + 1]
  const int32_t* list_rows;     // [n_rows]
  const uint32_t* row_mask;     // allow-mask words or null
  int64_t n_rows;
  int64_t id_offset;
  int nq, nprobe, nlist, k, parts;
  float* part_scores;           // [parts][nq][k]
  int64_t* part_ids;
};

// (the prefix over the probed lists and the position -> row step are in ivf_device.h)
// the running top-k of one workgroup; wave 0 owns it (count, worst are wave-uniform)
struct IvfTop {
  float* s;
  int* i;
  int k, count;
  float ws;
  int wi, wpos;
};

// the list's worst entry: the one every other entry ranks before
__device__ inline void ivf_find_worst(IvfTop& t, int lane) {
  wave_lds_sync();   // what lane 0 wrote to the list is read by every lane of the wave
  float s = 0.f;
  int i = -1, pos = 0;
  for (int e = lane; e < t.k; e += 64)
    if (i < 0 || ranks_before(s, i, t.s[e], t.i[e])) { s = t.s[e]; i = t.i[e]; pos = e; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(s, o);
    const int oi = __shfl_xor(i, o), op = __shfl_xor(pos, o);
    if (oi >= 0 && (i < 0 || ranks_before(s, i, os, oi))) { s = os; i = oi; pos = op; }
  }
  t.ws = s; t.wi = i; t.wpos = pos;
}

// offers the wave's scores (one per lane, row < 0 = none) to the list, one accepted candidate at a time
__device__ inline void ivf_offer(IvfTop& t, float s, int row, int lane) {
  const bool cand = row >= 0 && (t.count < t.k || ranks_before(s, row, t.ws, t.wi));
  unsigned long long m = __ballot(cand);
  while (m) {   // (wave-uniform)
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    const float cs = __shfl(s, src);
    const int ci = __shfl(row, src);
    if (t.count < t.k) {
      if (lane == 0) { t.s[t.count] = cs; t.i[t.count] = ci; }
      if (++t.count == t.k) ivf_find_worst(t, lane);
    } else if (ranks_before(cs, ci, t.ws, t.wi)) {
      if (lane == 0) { t.s[t.wpos] = cs; t.i[t.wpos] = ci; }
      ivf_find_worst(t, lane);
    }
  }
}

__global__ __launch_bounds__(IVF_THREADS) void ivf_scan_kernel(IvfParams p) {
  __shared__ float4 rows_s[STAGE_FLOAT4];   // the current chunk
  __shared__ float4 q_s[CHUNKS];
  __shared__ float top_s[IVF_K_MAX];
  __shared__ int top_i[IVF_K_MAX];
  __shared__ int64_t pre_s[IVF_PROBES + 1];           // exclusive prefix of the block's list lengths
  __shared__ int64_t off_s[IVF_PROBES];               // first list_rows entry of every list of the block
  __shared__ int64_t wsum_s[IVF_THREADS / 64];
  __shared__ int rid_s[2][STAGE_ROWS];                  // row numbers of the current and the next chunk (-1 = skip)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int part = blockIdx.x, q = blockIdx.y;
  if (tid < CHUNKS) q_s[tid] = reinterpret_cast<const float4*>(p.queries)[(int64_t)q * CHUNKS + tid];
  const int64_t* probe = p.probe + (int64_t)q * p.nprobe;
  const float4* rows4 = reinterpret_cast<const float4*>(p.rows);
  const int n_blocks = (p.nprobe + IVF_PROBES - 1) / IVF_PROBES;

  const IvfPrefix pre{pre_s, off_s, wsum_s};
  // prefix of probe block pb into pre_s / off_s; returns the block's total (uniform).  Two barriers inside.
  auto scan_block = [&](int pb) -> int64_t { return ivf_prefix_block(pre, probe, p.nprobe, p.nlist, p.list_offsets, pb, tid); };

  int64_t Lq = 0;
  for (int pb = 0; pb < n_blocks; ++pb) Lq += scan_block(pb);
  const int64_t lo = (int64_t)part * Lq / p.parts, hi = (int64_t)(part + 1) * Lq / p.parts;

  IvfTop top{top_s, top_i, p.k, 0, 0.f, -1, 0};

  // row number at position v of the current block (relative to the block's first position), -1 when there is none,
  // the row is outside the index or its mask bit is clear
  auto row_at = [&](int64_t v, int64_t end, int n_in_block) -> int {
    return ivf_row_at(pre, v, end, n_in_block, p.list_rows, p.row_mask, p.n_rows);
  };
  RowStage stage;
  auto load_chunk = [&](const int* rid) { stage.load(rows4, tid, [&](int row) { return rid[row]; }); };

  int64_t base = 0;
  for (int pb = 0; pb < n_blocks; ++pb) {   // every bound below is workgroup-uniform
    const int64_t total = n_blocks > 1 ? scan_block(pb) : Lq;
    const int n_in_block = min(IVF_PROBES, p.nprobe - pb * IVF_PROBES);
    const int64_t a = max(lo, base) - base, b = min(hi, base + total) - base;
    base += total;
    __syncthreads();   // the prefix is complete
    if (b <= a) continue;
    const int64_t n_chunks = (b - a + STAGE_ROWS - 1) / STAGE_ROWS;
    const bool finder = wave == 1 && lane < STAGE_ROWS;
    if (finder) {
      rid_s[0][lane] = row_at(a + lane, b, n_in_block);
      rid_s[1][lane] = row_at(a + STAGE_ROWS + lane, b, n_in_block);
    }
    __syncthreads();
    load_chunk(rid_s[0]);
    stage.store(rows_s, tid);
    __syncthreads();
    for (int64_t ch = 0; ch < n_chunks; ++ch) {
      const int cur = (int)(ch & 1);
      const bool more = ch + 1 < n_chunks;
      if (more) load_chunk(rid_s[cur ^ 1]);   // in flight while wave 0 scores
      int next_id = -1;
      if (finder && ch + 2 < n_chunks) next_id = row_at(a + (ch + 2) * STAGE_ROWS + lane, b, n_in_block);
      if (wave == 0) {
        const int r = lane < STAGE_ROWS ? rid_s[cur][lane] : -1;
        float s = 0.f;
        if (r >= 0) s = stage_score(rows_s, lane, q_s);
        ivf_offer(top, s, r, lane);
      }
      __syncthreads();   // the chunk and its row numbers have been read
      if (more) stage.store(rows_s, tid);
      if (finder) rid_s[cur][lane] = next_id;
      __syncthreads();
    }
  }

  if (wave == 0) {
    wave_lds_sync();
    const int64_t o = ((int64_t)part * p.nq + q) * p.k;
    for (int e = lane; e < p.k; e += 64) {
      const bool have = e < top.count;
      p.part_scores[o + e] = have ? top_s[e] : -FLT_MAX;
      p.part_ids[o + e] = have ? (int64_t)top_i[e] + p.id_offset : -1;
    }
  }
}

// one wave per (list, 64 columns): fp64 sums of the list's rows in CSR order, four row loads in flight
__global__ __launch_bounds__(64) void ivf_list_sums_kernel(const float* __restrict__ rows, int64_t n_rows,
                                                           const int64_t* __restrict__ list_offsets,
                                                           const int32_t* __restrict__ list_rows, double* __restrict__ sums) {
  const int l = blockIdx.x, c = blockIdx.y * 64 + threadIdx.x;
  int64_t lo = list_offsets[l], hi = list_offsets[l + 1];
  if (lo < 0) lo = 0;
  if (hi > n_rows) hi = n_rows;
  double acc = 0.0;
  int64_t j = lo;
  for (; j + 4 <= hi; j += 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t r = list_rows[j + u];
      v[u] = (r >= 0 && r < n_rows) ? rows[r * DIM + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc += (double)v[u];
  }
  for (; j < hi; ++j) {
    const int64_t r = list_rows[j];
    acc += (double)((r >= 0 && r < n_rows) ? rows[r * DIM + c] : 0.f);
  }
  sums[(int64_t)l * DIM + c] = acc;
}

bool ivf_shape_ok(int nq, int nprobe, int k, int64_t n_rows, int64_t max_list_rows) {
  return nq >= 1 && nprobe >= 1 && nprobe <= IVF_NLIST_MAX && k >= 1 && k <= IVF_K_MAX && n_rows >= 0 &&
         n_rows < sskd::MAX_SHARD_ROWS && max_list_rows >= 0;
}

// Parts per query, from host-known numbers only: two workgroups per CU over the whole call, no part shorter than one
// chunk of the longest sequence a query can probe, and no more candidates than the merge reads comfortably.
int ivf_parts(int nq, int nprobe, int k, int64_t n_rows, int64_t max_list_rows) {
  int64_t longest = (int64_t)nprobe * max_list_rows;
  if (longest > n_rows) longest = n_rows;
  int64_t parts = sskd::ceil_div(2 * IVF_CUS, nq);
  parts = std::min<int64_t>(parts, std::max<int64_t>(1, sskd::ceil_div(longest, STAGE_ROWS)));
  parts = std::min<int64_t>(parts, std::max(1, IVF_MERGE_CAND / k));
  parts = std::min<int64_t>(parts, IVF_MAX_PARTS);
  return (int)std::max<int64_t>(parts, 1);
}

// sskd_topk_merge is one wave per query doing k rounds over all its candidates: 512 parts of k = 10 cost it 0.33 ms, ten
// times the scan they belong to.  So `want` parts are laid out as p1 x p2 (part = i1 * p2 + i2) and merged in two steps
// of the same merge: p1 lists for each of the p2 * nq (i2, query) pairs, then p2 lists per query - about 2 sqrt(parts)
// k candidates per wave instead of parts * k.  Few candidates are merged at once (p2 = 1).
struct IvfSplit {
  int p1, p2;
  int parts() const { return p1 * p2; }
};
IvfSplit ivf_split(int want, int k) {
  if ((int64_t)want * k <= IVF_MERGE_DIRECT) return {want, 1};
  int p2 = 1;
  while (p2 * p2 < want) ++p2;
  return {std::max(want / p2, 1), p2};
}

struct IvfCarve {
  float* scores;       // [p1 * p2][nq][k]
  int64_t* ids;
  float* mid_scores;   // [p2][nq][k] (p2 > 1)
  int64_t* mid_ids;
  size_t bytes;
};
IvfCarve ivf_carve(void* ws, IvfSplit sp, int nq, int k) {
  sskd::Carver c(ws);
  IvfCarve out{};
  out.ids = c.take<int64_t>((size_t)sp.parts() * nq * k);
  out.scores = c.take<float>((size_t)sp.parts() * nq * k);
  if (sp.p2 > 1) {
    out.mid_ids = c.take<int64_t>((size_t)sp.p2 * nq * k);
    out.mid_scores = c.take<float>((size_t)sp.p2 * nq * k);
  }
  out.bytes = c.bytes();
  return out;
}

}  // namespace

extern "C" {

int sskd_ivf_search_plan(int nq, int nprobe, int k, int64_t n_rows, int64_t max_list_rows, int* parts, int* chunk_rows,
                         int* workgroups) {
  SSKD_REQUIRE(ivf_shape_ok(nq, nprobe, k, n_rows, max_list_rows),
               "ivf_search_plan: needs nq >= 1, 1 <= nprobe <= %d, 1 <= k <= %d, 0 <= n_rows < 2^31 - 64, max_list_rows >= 0",
               IVF_NLIST_MAX, IVF_K_MAX);
  const int P = ivf_split(ivf_parts(nq, nprobe, k, n_rows, max_list_rows), k).parts();
  if (parts) *parts = P;
  if (chunk_rows) *chunk_rows = STAGE_ROWS;
  if (workgroups) *workgroups = (int)std::min<int64_t>((int64_t)P * nq, INT32_MAX);
  return SSKD_OK;
}

size_t sskd_ivf_search_workspace_bytes(int nq, int nprobe, int k, int64_t n_rows, int64_t max_list_rows) {
  if (!ivf_shape_ok(nq, nprobe, k, n_rows, max_list_rows)) return 0;
  return ivf_carve(nullptr, ivf_split(ivf_parts(nq, nprobe, k, n_rows, max_list_rows), k), nq, k).bytes;
}

int sskd_ivf_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, const int64_t* d_probe,
                    int nprobe, const int64_t* d_list_offsets, const int32_t* d_list_rows, int nlist, int k,
                    int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores, int64_t* d_out_ids,
                    void* d_workspace, size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "ivf_search: n_rows < 0");
  SSKD_REQUIRE(nq >= 0, "ivf_search: nq < 0");
  SSKD_REQUIRE(k >= 1 && k <= IVF_K_MAX, "ivf_search: k=%d outside [1, %d]", k, IVF_K_MAX);
  SSKD_REQUIRE(nlist >= 1 && nlist <= IVF_NLIST_MAX, "ivf_search: nlist=%d outside [1, %d]", nlist, IVF_NLIST_MAX);
  SSKD_REQUIRE(nprobe >= 1 && nprobe <= nlist, "ivf_search: nprobe=%d outside [1, nlist=%d]", nprobe, nlist);
  SSKD_REQUIRE(id_offset >= 0, "ivf_search: id_offset < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "ivf_search: shard too large for int32 row ids");
  SSKD_REQUIRE(nq <= 65535, "ivf_search: nq=%d > 65535 (split the batch)", nq);
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_queries && d_probe && d_list_offsets && d_out_scores && d_out_ids, "ivf_search: null pointer");
  SSKD_REQUIRE(n_rows == 0 || (d_tiled && d_list_rows), "ivf_search: null index");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_queries) % 16 == 0 && reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0,
               "ivf_search: queries and index must be 16-byte aligned");
  // The call does not know the longest list: it takes as many parts as the workspace holds, up to the plan of a list
  // that holds every row.  A workspace of sskd_ivf_search_workspace_bytes(.., max_list_rows) holds that plan's parts.
  int want = ivf_parts(nq, nprobe, k, n_rows, n_rows);
  IvfSplit sp = ivf_split(want, k);
  if (d_workspace)
    while (want > 1 && ivf_carve(nullptr, sp, nq, k).bytes > workspace_bytes) sp = ivf_split(--want, k);
  const int P = sp.parts();
  const IvfCarve cv = ivf_carve(d_workspace, sp, nq, k);
  SSKD_REQUIRE(d_workspace && workspace_bytes >= cv.bytes, "ivf_search: workspace %zu B < required %zu B (one part)",
               d_workspace ? workspace_bytes : (size_t)0, cv.bytes);
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0, "ivf_search: workspace must be 16-byte aligned");
  IvfParams p{};
  p.rows = d_tiled;
  p.queries = d_queries;
  p.probe = d_probe;
  p.list_offsets = d_list_offsets;
  p.list_rows = d_list_rows;
  p.row_mask = d_row_mask;
  p.n_rows = n_rows;
  p.id_offset = id_offset;
  p.nq = nq;
  p.nprobe = nprobe;
  p.nlist = nlist;
  p.k = k;
  p.parts = P;
  p.part_scores = cv.scores;
  p.part_ids = cv.ids;
  hipLaunchKernelGGL(ivf_scan_kernel, dim3((unsigned)P, (unsigned)nq), dim3(IVF_THREADS), 0, sskd::as_stream(stream), p);
  const int rc = sskd::check_launch("ivf_scan_kernel");
  if (rc != SSKD_OK) return rc;
  if (sp.p2 == 1) return sskd_topk_merge(cv.scores, cv.ids, P, nq, k, k, d_out_scores, d_out_ids, stream);
  const int rc1 = sskd_topk_merge(cv.scores, cv.ids, sp.p1, sp.p2 * nq, k, k, cv.mid_scores, cv.mid_ids, stream);
  if (rc1 != SSKD_OK) return rc1;
  return sskd_topk_merge(cv.mid_scores, cv.mid_ids, sp.p2, nq, k, k, d_out_scores, d_out_ids, stream);
}

int sskd_ivf_list_sums(const float* d_tiled, int64_t n_rows, const int64_t* d_list_offsets, const int32_t* d_list_rows,
                       int nlist, double* d_sums, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "ivf_list_sums: n_rows < 0");
  SSKD_REQUIRE(nlist >= 0 && nlist <= IVF_NLIST_MAX, "ivf_list_sums: nlist=%d outside [0, %d]", nlist, IVF_NLIST_MAX);
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "ivf_list_sums: shard too large for int32 row ids");
  if (nlist == 0) return SSKD_OK;
  SSKD_REQUIRE(d_list_offsets && d_sums, "ivf_list_sums: null pointer");
  SSKD_REQUIRE(n_rows == 0 || (d_tiled && d_list_rows), "ivf_list_sums: null index");
  hipLaunchKernelGGL(ivf_list_sums_kernel, dim3((unsigned)nlist, DIM / 64), dim3(64), 0, sskd::as_stream(stream), d_tiled,
                     n_rows, d_list_offsets, d_list_rows, d_sums);
  return sskd::check_launch("ivf_list_sums_kernel");
}

}  // extern "C"
