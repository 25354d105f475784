// IVF-PQ: product-quantisation codes over the inverted lists (sskd_amd.h "IVF-PQ").
//
// The PQ half of the reference's `ivf_pq` index type (configs/index.yaml: m 64, nbits 8).  The codes decide WHICH rows
// of the probed lists get re-scored; every score and order of the default result is still the exact scan's fp32 fma
// chain (row_score_fma), so a refined search returns bit for bit what the exact search returns under an allow-mask of
// its candidates.  Rows are encoded by residual (row - centroid of its list), so for the inner product
//   <q, row> ~ <q, c_list> + sum_j <q_j, cb[j][code_j]>:
// the look-up table lut[j][c] = <q_j, cb[j][c]> does not depend on the list, and the first term is the probe's own score.
//
// pq_scan_kernel<M>, one workgroup per (part p, query q).  The positions a query probes are partitioned exactly as in
// ivf_scan_kernel (ivf_device.h: prefix over the list lengths, balanced parts).  The codes lie in CSR order
// (codes_csr[position][M]), so a list is one contiguous byte range and lane t of a step reads the M bytes of position
// v0 + t with 16-byte loads (8-byte ones for M = 8 and 24).  The query's LUT (M KiB) is loaded once into LDS as
// lut_s[j * 256 + c]: the code c selects the bank, look-ups are data-dependent and conflicts are expected.  All four
// waves score, 256 positions per step, one lane running one row's chain s = probe score; s = s + lut[j][code_j],
// j = 0 .. M - 1 (fp32 adds in that order); the next step's codes load while the current step is looked up.  The
// running top-C (C = refine, or k when refine = 0) is kept by all four waves: a row that ranks before the bound is
// appended to a pool of 1 024 records in LDS, and when the pool might overflow it is sorted, cut to its C best and the
// C-th becomes the bound.  (ivf.hip's unsorted list with a cached worst entry, one wave replacing one record at a time,
// was measured here first: with C = 100 .. 256 instead of k = 10 its serial replacements cost 5 .. 10 ms per 10 000
// queries whatever nprobe was - DESIGN section 19.)  Every part writes its C records padded with (-FLT_MAX, -1).
//
// pq_refine_kernel, one workgroup per query: a bitonic sort of the query's <= 4 096 partial records in LDS in rank
// order (ADC score descending, then lower row; ids are distinct, so the order is total), the first R are the candidates;
// their rows are gathered through LDS 32 at a time, staged as in row_stage.h, and scored by row_score_fma, one lane per
// row; a second sort orders the exact scores and k are written.  With refine = 0 only the first sort runs and the ADC
// scores are the result.
//
// pq_lut_kernel, pq_encode_kernel, pq_code_sums_kernel: off the hot path, fp64, one fixed order per output element.
#include "ivf_device.h"
#include "row_stage.h"
#include "search_host.h"

#include <algorithm>
#include <cfloat>

namespace {

constexpr int PQ_CODES = 256;            // nbits = 8
constexpr int PQ_R_MAX = 256;
constexpr int PQ_MAX_RECORDS = 4096;     // partial records of one query: what pq_refine_kernel sorts in LDS
// A part's code bytes (M per row) are at least four times the LUT bytes (1 024 M) its workgroup loads first.
constexpr int PQ_MIN_PART_ROWS = 4096;
constexpr int PQ_POOL = 1024;            // the scan's candidate pool in LDS: the kept records, then the pending ones
static_assert(IVF_THREADS == STAGE_THREADS, "pq_refine_kernel's workgroup is the staging workgroup");

bool pq_m_ok(int m) { return m == 8 || m == 16 || m == 24 || m == 32 || m == 48 || m == 64 || m == 96; }

struct PqScanParams {
  const uint8_t* codes;         // [n_rows][M], CSR order
  const float* lut;             // [nq][M][256]
  const int64_t* probe;         // [nq][nprobe]
  const float* probe_scores;    // [nq][nprobe]
  const int64_t* list_offsets;
  const int32_t* list_rows;
  const uint32_t* row_mask;
  int64_t n_rows;
  int nq, nprobe, nlist, cap, parts;
  float* part_scores;           // [parts][nq][cap]
  int32_t* part_rows;
};

// rank order with "no record" (row < 0) after every record
__device__ inline bool pq_before(float sa, int ia, float sb, int ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  return ranks_before(sa, ia, sb, ib);
}

// bitonic sort of n (a power of two) records in LDS into rank order; a barrier before and after
__device__ inline void pq_sort(float* ks, int* ki, int n, int tid) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = tid; t < n / 2; t += IVF_THREADS) {
        const int i = 2 * t - (t & (stride - 1)), j = i + stride;
        const bool up = (i & size) == 0;
        const float sa = ks[i], sb = ks[j];
        const int ia = ki[i], ib = ki[j];
        if (up ? pq_before(sb, ib, sa, ia) : pq_before(sa, ia, sb, ib)) {
          ks[i] = sb; ki[i] = ib;
          ks[j] = sa; ki[j] = ia;
        }
      }
    }
  }
  __syncthreads();
}

// one position's work item: the row (or -1), its list's probe score and its M code bytes
template <int M>
struct PqItem {
  int row;
  float base;
  uint32_t w[M / 4];
};

template <int M>
__global__ __launch_bounds__(IVF_THREADS) void pq_scan_kernel(PqScanParams p) {
  extern __shared__ __attribute__((aligned(16))) float lut_s[];   // [M][256]
  __shared__ float pool_s[PQ_POOL];                  // [0, fill) kept, [fill, fill + pending) waiting for a compaction
  __shared__ int pool_i[PQ_POOL];
  __shared__ int pend_s;                             // slots handed out since the last compaction
  __shared__ int64_t pre_s[IVF_PROBES + 1];
  __shared__ int64_t off_s[IVF_PROBES];
  __shared__ int64_t wsum_s[IVF_THREADS / 64];
  __shared__ float ps_s[IVF_PROBES];                 // probe scores of the current prefix block

  const int tid = threadIdx.x, lane = tid & 63;
  const int part = blockIdx.x, q = blockIdx.y;
  const int64_t* probe = p.probe + (int64_t)q * p.nprobe;
  const float* probe_scores = p.probe_scores + (int64_t)q * p.nprobe;
  const int n_blocks = (p.nprobe + IVF_PROBES - 1) / IVF_PROBES;
  const IvfPrefix pre{pre_s, off_s, wsum_s};
  if (tid == 0) pend_s = 0;

  int64_t Lq = 0;
  for (int pb = 0; pb < n_blocks; ++pb) Lq += ivf_prefix_block(pre, probe, p.nprobe, p.nlist, p.list_offsets, pb, tid);
  const int64_t lo = (int64_t)part * Lq / p.parts, hi = (int64_t)(part + 1) * Lq / p.parts;

  if (hi > lo) {   // (uniform) the query's LUT, once
    const float4* src = reinterpret_cast<const float4*>(p.lut) + (int64_t)q * (M * PQ_CODES / 4);
    float4* dst = reinterpret_cast<float4*>(lut_s);
    for (int i = tid; i < M * PQ_CODES / 4; i += IVF_THREADS) dst[i] = src[i];
  }

  // The running top-cap, kept by all four waves.  A row that ranks before the bound (the cap-th best record of the last
  // compaction; none before the pool first holds cap records) is appended to the pool; when another step's 256 rows
  // might not fit, the pool is sorted in rank order, its first cap records are kept and the cap-th becomes the bound.
  // A row the bound turns away ranks after cap rows already seen, so the kept records are exactly the cap best; the
  // order in which the waves append does not matter, because the sort's order is total.  fill, pending and the bound
  // are workgroup-uniform registers.
  int fill = 0, pending = 0;
  bool bounded = false;
  float bound_s = 0.f;
  int bound_i = -1;
  auto compact = [&]() {   // called by every thread, after a barrier that follows the last append
    const int n = fill + pending;
    int np = 2;
    while (np < n) np <<= 1;
    for (int t = n + tid; t < np; t += IVF_THREADS) { pool_s[t] = -FLT_MAX; pool_i[t] = -1; }
    if (tid == 0) pend_s = 0;
    pq_sort(pool_s, pool_i, np, tid);
    fill = min(n, p.cap);
    pending = 0;
    if (fill == p.cap) {
      bounded = true;
      bound_s = pool_s[p.cap - 1];
      bound_i = pool_i[p.cap - 1];
    }
  };

  int64_t base = 0;
  for (int pb = 0; pb < n_blocks; ++pb) {   // every bound below is workgroup-uniform
    const int64_t total = n_blocks > 1 ? ivf_prefix_block(pre, probe, p.nprobe, p.nlist, p.list_offsets, pb, tid) : Lq;
    const int n_in_block = min(IVF_PROBES, p.nprobe - pb * IVF_PROBES);
    ps_s[tid] = tid < n_in_block ? probe_scores[pb * IVF_PROBES + tid] : 0.f;
    const int64_t a = max(lo, base) - base, b = min(hi, base + total) - base;
    base += total;
    __syncthreads();   // the prefix, the probe scores and the LUT are complete
    if (b <= a) continue;

    auto fetch = [&](int64_t v) {
      PqItem<M> it;
      it.row = -1;
      it.base = 0.f;
#pragma unroll
      for (int i = 0; i < M / 4; ++i) it.w[i] = 0u;
      if (v < b) {
        int j;
        const int64_t at = ivf_entry_at(pre, v, n_in_block, j);
        it.row = ivf_row_of_entry(at, p.list_rows, p.row_mask, p.n_rows);   // -1 unless 0 <= at < n_rows
        if (it.row >= 0) {
          it.base = ps_s[j];
          const uint8_t* c = p.codes + at * M;
          if constexpr (M % 16 == 0) {
#pragma unroll
            for (int i = 0; i < M / 16; ++i) {
              const uint4 x = reinterpret_cast<const uint4*>(c)[i];
              it.w[4 * i] = x.x; it.w[4 * i + 1] = x.y; it.w[4 * i + 2] = x.z; it.w[4 * i + 3] = x.w;
            }
          } else {
#pragma unroll
            for (int i = 0; i < M / 8; ++i) {
              const uint2 x = reinterpret_cast<const uint2*>(c)[i];
              it.w[2 * i] = x.x; it.w[2 * i + 1] = x.y;
            }
          }
        }
      }
      return it;
    };

    PqItem<M> cur = fetch(a + tid);
    for (int64_t v0 = a; v0 < b; v0 += IVF_THREADS) {
      PqItem<M> nxt = fetch(v0 + IVF_THREADS + tid);   // (nothing past b) in flight during the look-ups
      float s = cur.base;
      if (cur.row >= 0) {
#pragma unroll
        for (int j = 0; j < M; ++j) s = s + lut_s[j * PQ_CODES + ((cur.w[j >> 2] >> (8 * (j & 3))) & 255u)];
      }
      const bool take = cur.row >= 0 && (!bounded || ranks_before(s, cur.row, bound_s, bound_i));
      const unsigned long long mask = __ballot(take);
      if (mask) {   // (wave-uniform) one LDS atomic per wave hands out its slots
        int first = 0;
        if (lane == 0) first = atomicAdd(&pend_s, __popcll(mask));
        first = __shfl(first, 0);
        if (take) {
          // fill + pending + 256 <= PQ_POOL held when the step began, so the slot is inside the pool
          const int at = fill + first + __popcll(mask & ((1ull << lane) - 1ull));
          pool_s[at] = s;
          pool_i[at] = cur.row;
        }
      }
      pending += __syncthreads_count(take);
      if (fill + pending + IVF_THREADS > PQ_POOL) compact();   // the next step's rows might not fit
      cur = nxt;
    }
  }

  if (pending > 0) compact();
  __syncthreads();   // (pend_s = 0 of thread 0 when nothing was scanned)
  const int64_t o = ((int64_t)part * p.nq + q) * p.cap;
  for (int e = tid; e < p.cap; e += IVF_THREADS) {
    const bool have = e < fill;
    p.part_scores[o + e] = have ? pool_s[e] : -FLT_MAX;
    p.part_rows[o + e] = have ? pool_i[e] : -1;
  }
}

struct PqRefineParams {
  const float* rows;            // the index: row-major fp32 [n_rows][DIM]
  const float* queries;
  const float* part_scores;     // [parts][nq][cap]
  const int32_t* part_rows;
  int64_t n_rows, id_offset;
  int nq, parts, cap, k, refine;
  float* out_scores;            // [nq][k]
  int64_t* out_ids;
  int64_t* out_cand;            // [nq][refine] or null
};

constexpr int PQ_STAGE_BYTES = STAGE_FLOAT4 * 16;   // 49 664: the gather chunk; the sort arrays (32 KiB) alias it
static_assert(PQ_STAGE_BYTES >= PQ_MAX_RECORDS * 8, "the staging area holds the sort arrays");

__global__ __launch_bounds__(IVF_THREADS) void pq_refine_kernel(PqRefineParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[PQ_STAGE_BYTES];
  __shared__ float4 q_s[CHUNKS];
  __shared__ float keep_s[PQ_R_MAX];
  __shared__ int keep_i[PQ_R_MAX];
  float* ks = reinterpret_cast<float*>(stage);
  int* ki = reinterpret_cast<int*>(stage + PQ_MAX_RECORDS * 4);
  float4* rows_s = reinterpret_cast<float4*>(stage);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  if (tid < CHUNKS) q_s[tid] = reinterpret_cast<const float4*>(p.queries)[(int64_t)q * CHUNKS + tid];

  const int n_rec = p.parts * p.cap;   // <= PQ_MAX_RECORDS by plan
  int np = 2;
  while (np < n_rec) np <<= 1;
  for (int t = tid; t < np; t += IVF_THREADS) {
    float s = -FLT_MAX;
    int r = -1;
    if (t < n_rec) {
      const int part = t / p.cap, e = t - part * p.cap;
      const int64_t o = ((int64_t)part * p.nq + q) * p.cap + e;
      s = p.part_scores[o];
      r = p.part_rows[o];
      if (r >= p.n_rows) r = -1;
    }
    ks[t] = s;
    ki[t] = r < 0 ? -1 : r;
  }
  pq_sort(ks, ki, np, tid);

  // the candidates: the first `want` records in rank order
  const int want = p.refine > 0 ? p.refine : p.k;
  {
    const bool have = tid < want && tid < np && ki[tid] >= 0;
    keep_s[tid] = have ? ks[tid] : -FLT_MAX;
    keep_i[tid] = have ? ki[tid] : -1;
    if (p.out_cand && tid < p.refine) p.out_cand[(int64_t)q * p.refine + tid] = have ? (int64_t)ki[tid] + p.id_offset : -1;
  }
  const int n_cand = __syncthreads_count(tid < want && tid < np && ki[tid] >= 0);   // also: the sort arrays are dead now

  if (p.refine > 0) {
    const float4* rows4 = reinterpret_cast<const float4*>(p.rows);
    RowStage stage;
    for (int c0 = 0; c0 < n_cand; c0 += STAGE_ROWS) {   // (uniform)
      stage.load(rows4, tid, [&](int row) { return c0 + row < n_cand ? keep_i[c0 + row] : -1; });
      stage.store(rows_s, tid);
      __syncthreads();
      // 32 lanes of wave 0 score, the other 224 threads only stage, and nothing is pipelined: deliberate - the layout is
      // row_stage.h's, and the whole kernel is 0.8 ms per 10 000 queries at R = 100, a tenth of
      // the scan before it
      if (wave == 0 && lane < STAGE_ROWS && c0 + lane < n_cand) keep_s[c0 + lane] = stage_score(rows_s, lane, q_s);
      __syncthreads();
    }
    int n2 = 2;
    while (n2 < want) n2 <<= 1;   // <= 256; the entries past the candidates are "no record"
    pq_sort(keep_s, keep_i, n2, tid);
  }
  if (tid < p.k) {
    const bool have = tid < n_cand;
    p.out_scores[(int64_t)q * p.k + tid] = have ? keep_s[tid] : -FLT_MAX;
    p.out_ids[(int64_t)q * p.k + tid] = have ? (int64_t)keep_i[tid] + p.id_offset : -1;
  }
}

// lut[q][j][c] = fl32(sum_d (double) q_d (double) cb[j][c][d]), fp64 over d ascending; the products are exact in fp64
// (24 x 24 significant bits), so a contracted fma gives the same bits as multiply-then-add
__global__ __launch_bounds__(PQ_CODES) void pq_lut_kernel(const float* __restrict__ queries, const float* __restrict__ cb,
                                                          int m, float* __restrict__ lut) {
  __shared__ float q_s[DIM / 8];
  const int j = blockIdx.x, q = blockIdx.y, c = threadIdx.x, dsub = DIM / m;
  if (c < dsub) q_s[c] = queries[(int64_t)q * DIM + j * dsub + c];
  __syncthreads();
  const float* e = cb + ((int64_t)j * PQ_CODES + c) * dsub;
  double acc = 0.0;
  for (int d = 0; d < dsub; ++d) acc += (double)q_s[d] * (double)e[d];
  lut[((int64_t)q * m + j) * PQ_CODES + c] = (float)acc;
}

// code[row][j] = argmin_c sum_d (r_d - cb[j][c][d])^2, fp64 over d ascending from +0.0, ties to the lower c.  One
// thread per row, one workgroup per (256 rows, subspace); the subspace's codebook sits in LDS and every lane reads the
// same entry at the same time (a broadcast).
template <int DSUB>
__global__ __launch_bounds__(IVF_THREADS) void pq_encode_kernel(const float* __restrict__ rows, int64_t n,
                                                                const float* __restrict__ centroids,
                                                                const int64_t* __restrict__ assign, int nlist,
                                                                const float* __restrict__ cb, int m,
                                                                uint8_t* __restrict__ codes) {
// Every fp64 subtract, multiply and add below is rounded once and NO fma is formed: contraction is switched off for this
// function body (the NumPy restatement of the tests does the same three operations).
#pragma clang fp contract(off)
  __shared__ float cb_s[PQ_CODES * DSUB];
  const int tid = threadIdx.x, j = blockIdx.y;
  for (int i = tid; i < PQ_CODES * DSUB; i += IVF_THREADS) cb_s[i] = cb[(int64_t)j * PQ_CODES * DSUB + i];
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * IVF_THREADS + tid;
  if (row >= n) return;
  float r[DSUB];
  const float* x = rows + row * DIM + j * DSUB;
  const float* cen = nullptr;
  if (assign) {
    const int64_t l = assign[row];
    if (l >= 0 && l < nlist) cen = centroids + l * DIM + j * DSUB;
  }
#pragma unroll
  for (int d = 0; d < DSUB; ++d) r[d] = cen ? x[d] - cen[d] : x[d];
  double best = 0.0;
  int best_c = 0;
  for (int c = 0; c < PQ_CODES; ++c) {
    double acc = 0.0;
#pragma unroll
    for (int d = 0; d < DSUB; ++d) {
      const double t = (double)r[d] - (double)cb_s[c * DSUB + d];
      const double t2 = t * t;
      acc = acc + t2;
    }
    if (c == 0 || acc < best) { best = acc; best_c = c; }
  }
  codes[row * m + j] = (uint8_t)best_c;
}

// sums[j][c][d] = fp64 sum of r_d over the rows grouped under code c of subspace j, in the order group_rows lists them
// (ascending row: a stable sort by code), one accumulator per output element from +0.0, no atomics
__global__ __launch_bounds__(64) void pq_code_sums_kernel(const float* __restrict__ rows, int64_t n,
                                                          const float* __restrict__ centroids,
                                                          const int64_t* __restrict__ assign, int nlist,
                                                          const int64_t* __restrict__ group_offsets,
                                                          const int32_t* __restrict__ group_rows, int m,
                                                          double* __restrict__ sums, int64_t* __restrict__ counts) {
  const int c = blockIdx.x, j = blockIdx.y, d = threadIdx.x, dsub = DIM / m;
  int64_t lo = group_offsets[(int64_t)j * (PQ_CODES + 1) + c], hi = group_offsets[(int64_t)j * (PQ_CODES + 1) + c + 1];
  if (lo < 0) lo = 0;
  if (hi > n) hi = n;
  if (hi < lo) hi = lo;
  if (d == 0) counts[j * PQ_CODES + c] = hi - lo;
  if (d >= dsub) return;
  double acc = 0.0;
  for (int64_t e = lo; e < hi; ++e) {
    const int64_t row = group_rows[(int64_t)j * n + e];
    if (row < 0 || row >= n) continue;
    float x = rows[row * DIM + j * dsub + d];
    if (assign) {
      const int64_t l = assign[row];
      if (l >= 0 && l < nlist) x = x - centroids[l * DIM + j * dsub + d];
    }
    acc += (double)x;
  }
  sums[((int64_t)j * PQ_CODES + c) * dsub + d] = acc;
}

int pq_cap(int k, int refine) { return refine > 0 ? refine : k; }

bool pq_shape_ok(int nq, int nprobe, int k, int refine, int m, int64_t n_rows, int64_t max_list_rows) {
  return nq >= 1 && nprobe >= 1 && nprobe <= IVF_NLIST_MAX && k >= 1 && k <= PQ_R_MAX &&
         (refine == 0 || (refine >= k && refine <= PQ_R_MAX)) && pq_m_ok(m) && n_rows >= 0 &&
         n_rows < sskd::MAX_SHARD_ROWS && max_list_rows >= 0;
}

// Parts per query, from host-known numbers only: two workgroups per CU over the whole call, no part shorter than
// PQ_MIN_PART_ROWS positions of the longest sequence a query can probe, at most PQ_MAX_RECORDS records per query.
int pq_parts(int nq, int nprobe, int cap, int64_t n_rows, int64_t max_list_rows) {
  int64_t longest = (int64_t)nprobe * max_list_rows;
  if (longest > n_rows) longest = n_rows;
  int64_t parts = sskd::ceil_div(2 * IVF_CUS, nq);
  parts = std::min<int64_t>(parts, std::max<int64_t>(1, longest / PQ_MIN_PART_ROWS));
  parts = std::min<int64_t>(parts, std::max(1, PQ_MAX_RECORDS / cap));
  return (int)std::max<int64_t>(parts, 1);
}

struct PqCarve {
  float* lut;           // [nq][m][256]
  float* scores;        // [parts][nq][cap]
  int32_t* rows;
  size_t bytes;
};
PqCarve pq_carve(void* ws, int parts, int nq, int cap, int m) {
  sskd::Carver c(ws);
  PqCarve out{};
  out.lut = c.take<float>((size_t)nq * m * PQ_CODES);
  out.scores = c.take<float>((size_t)parts * nq * cap);
  out.rows = c.take<int32_t>((size_t)parts * nq * cap);
  out.bytes = c.bytes();
  return out;
}

template <int M>
int pq_launch_scan(const PqScanParams& p, hipStream_t st) {
  const size_t lds = (size_t)M * PQ_CODES * sizeof(float);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(pq_scan_kernel<M>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
  hipLaunchKernelGGL(pq_scan_kernel<M>, dim3((unsigned)p.parts, (unsigned)p.nq), dim3(IVF_THREADS), lds, st, p);
  return sskd::check_launch("pq_scan_kernel");
}

int pq_launch_lut(const float* d_queries, int nq, const float* d_codebooks, int m, float* d_lut, hipStream_t st) {
  hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)m, (unsigned)nq), dim3(PQ_CODES), 0, st, d_queries, d_codebooks, m, d_lut);
  return sskd::check_launch("pq_lut_kernel");
}

}  // namespace

extern "C" {

int sskd_pq_encode(const float* d_rows, int64_t n, const float* d_centroids, const int64_t* d_assign, int nlist,
                   const float* d_codebooks, int m, uint8_t* d_codes, void* stream) {
  SSKD_REQUIRE(n >= 0, "pq_encode: n < 0");
  SSKD_REQUIRE(pq_m_ok(m), "pq_encode: m=%d is not one of 8, 16, 24, 32, 48, 64, 96", m);
  SSKD_REQUIRE(n < sskd::MAX_SHARD_ROWS, "pq_encode: too many rows for int32 row ids");
  SSKD_REQUIRE(!d_assign || (nlist >= 1 && nlist <= IVF_NLIST_MAX), "pq_encode: nlist=%d outside [1, %d]", nlist,
               IVF_NLIST_MAX);
  SSKD_REQUIRE(!d_assign || d_centroids, "pq_encode: null centroids with an assignment");
  if (n == 0) return SSKD_OK;
  SSKD_REQUIRE(d_rows && d_codebooks && d_codes, "pq_encode: null pointer");
  const dim3 grid((unsigned)sskd::ceil_div(n, IVF_THREADS), (unsigned)m), block(IVF_THREADS);
  hipStream_t st = sskd::as_stream(stream);
#define SSKD_PQ_ENCODE(DSUB)                                                                                        \
  case DSUB:                                                                                                        \
    hipLaunchKernelGGL(pq_encode_kernel<DSUB>, grid, block, 0, st, d_rows, n, d_centroids, d_assign, nlist, d_codebooks, \
                       m, d_codes);                                                                                 \
    break;
  switch (DIM / m) {
    SSKD_PQ_ENCODE(48) SSKD_PQ_ENCODE(24) SSKD_PQ_ENCODE(16) SSKD_PQ_ENCODE(12) SSKD_PQ_ENCODE(8) SSKD_PQ_ENCODE(6)
    SSKD_PQ_ENCODE(4)
  }
#undef SSKD_PQ_ENCODE
  return sskd::check_launch("pq_encode_kernel");
}

int sskd_pq_code_sums(const float* d_rows, int64_t n, const float* d_centroids, const int64_t* d_assign, int nlist,
                      const int64_t* d_group_offsets, const int32_t* d_group_rows, int m, double* d_sums,
                      int64_t* d_counts, void* stream) {
  SSKD_REQUIRE(n >= 0, "pq_code_sums: n < 0");
  SSKD_REQUIRE(pq_m_ok(m), "pq_code_sums: m=%d is not one of 8, 16, 24, 32, 48, 64, 96", m);
  SSKD_REQUIRE(n < sskd::MAX_SHARD_ROWS, "pq_code_sums: too many rows for int32 row ids");
  SSKD_REQUIRE(!d_assign || (nlist >= 1 && nlist <= IVF_NLIST_MAX), "pq_code_sums: nlist=%d outside [1, %d]", nlist,
               IVF_NLIST_MAX);
  SSKD_REQUIRE(!d_assign || d_centroids, "pq_code_sums: null centroids with an assignment");
  SSKD_REQUIRE(d_group_offsets && d_sums && d_counts, "pq_code_sums: null pointer");
  SSKD_REQUIRE(n == 0 || (d_rows && d_group_rows), "pq_code_sums: null rows");
  hipLaunchKernelGGL(pq_code_sums_kernel, dim3(PQ_CODES, (unsigned)m), dim3(64), 0, sskd::as_stream(stream), d_rows, n,
                     d_centroids, d_assign, nlist, d_group_offsets, d_group_rows, m, d_sums, d_counts);
  return sskd::check_launch("pq_code_sums_kernel");
}

int sskd_pq_lut(const float* d_queries, int nq, const float* d_codebooks, int m, float* d_lut, void* stream) {
  SSKD_REQUIRE(nq >= 0, "pq_lut: nq < 0");
  SSKD_REQUIRE(pq_m_ok(m), "pq_lut: m=%d is not one of 8, 16, 24, 32, 48, 64, 96", m);
  SSKD_REQUIRE(nq <= 65535, "pq_lut: nq=%d > 65535 (split the batch)", nq);
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_queries && d_codebooks && d_lut, "pq_lut: null pointer");
  return pq_launch_lut(d_queries, nq, d_codebooks, m, d_lut, sskd::as_stream(stream));
}

int sskd_pq_search_plan(int nq, int nprobe, int k, int refine, int m, int64_t n_rows, int64_t max_list_rows, int* parts,
                        int* min_part_rows, int* workgroups, size_t* lut_bytes) {
  SSKD_REQUIRE(pq_shape_ok(nq, nprobe, k, refine, m, n_rows, max_list_rows),
               "pq_search_plan: needs nq >= 1, 1 <= nprobe <= %d, 1 <= k <= %d, refine = 0 or k <= refine <= %d, m one of "
               "8, 16, 24, 32, 48, 64, 96, 0 <= n_rows < 2^31 - 64, max_list_rows >= 0",
               IVF_NLIST_MAX, PQ_R_MAX, PQ_R_MAX);
  const int P = pq_parts(nq, nprobe, pq_cap(k, refine), n_rows, max_list_rows);
  if (parts) *parts = P;
  if (min_part_rows) *min_part_rows = PQ_MIN_PART_ROWS;
  if (workgroups) *workgroups = (int)std::min<int64_t>((int64_t)P * nq, INT32_MAX);
  if (lut_bytes) *lut_bytes = (size_t)nq * m * PQ_CODES * sizeof(float);
  return SSKD_OK;
}

size_t sskd_pq_search_workspace_bytes(int nq, int nprobe, int k, int refine, int m, int64_t n_rows,
                                      int64_t max_list_rows) {
  if (!pq_shape_ok(nq, nprobe, k, refine, m, n_rows, max_list_rows)) return 0;
  const int cap = pq_cap(k, refine);
  return pq_carve(nullptr, pq_parts(nq, nprobe, cap, n_rows, max_list_rows), nq, cap, m).bytes;
}

int sskd_pq_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, const int64_t* d_probe,
                   const float* d_probe_scores, int nprobe, const int64_t* d_list_offsets, const int32_t* d_list_rows,
                   int nlist, const uint8_t* d_codes_csr, const float* d_codebooks, int m, int k, int refine,
                   int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores, int64_t* d_out_ids,
                   int64_t* d_out_candidates, void* d_workspace, size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "pq_search: n_rows < 0");
  SSKD_REQUIRE(nq >= 0, "pq_search: nq < 0");
  SSKD_REQUIRE(pq_m_ok(m), "pq_search: m=%d is not one of 8, 16, 24, 32, 48, 64, 96", m);
  SSKD_REQUIRE(k >= 1 && k <= PQ_R_MAX, "pq_search: k=%d outside [1, %d]", k, PQ_R_MAX);
  SSKD_REQUIRE(refine == 0 || (refine >= k && refine <= PQ_R_MAX), "pq_search: refine=%d is neither 0 nor in [k=%d, %d]",
               refine, k, PQ_R_MAX);
  SSKD_REQUIRE(nlist >= 1 && nlist <= IVF_NLIST_MAX, "pq_search: nlist=%d outside [1, %d]", nlist, IVF_NLIST_MAX);
  SSKD_REQUIRE(nprobe >= 1 && nprobe <= nlist, "pq_search: nprobe=%d outside [1, nlist=%d]", nprobe, nlist);
  SSKD_REQUIRE(id_offset >= 0, "pq_search: id_offset < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "pq_search: shard too large for int32 row ids");
  SSKD_REQUIRE(nq <= 65535, "pq_search: nq=%d > 65535 (split the batch)", nq);
  SSKD_REQUIRE(d_out_candidates == nullptr || refine > 0, "pq_search: candidates are written only with refine > 0");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_queries && d_probe && d_probe_scores && d_list_offsets && d_codebooks && d_out_scores && d_out_ids,
               "pq_search: null pointer");
  SSKD_REQUIRE(n_rows == 0 || (d_tiled && d_list_rows && d_codes_csr), "pq_search: null index");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_queries) % 16 == 0 && reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(d_codes_csr) % 16 == 0,
               "pq_search: queries, index and codes must be 16-byte aligned");
  // As sskd_ivf_search: the call does not know the longest list and takes as many parts as the workspace holds, up to
  // the plan of a list that holds every row.  workspace_bytes therefore carries the plan: the header tells callers to
  // pass the size of the plan for THEIR longest list, not the size of their buffer (IVFPQIndex.search_device does).
  const int cap = pq_cap(k, refine);
  int P = pq_parts(nq, nprobe, cap, n_rows, n_rows);
  if (d_workspace)
    while (P > 1 && pq_carve(nullptr, P, nq, cap, m).bytes > workspace_bytes) --P;
  const PqCarve cv = pq_carve(d_workspace, P, nq, cap, m);
  SSKD_REQUIRE(d_workspace && workspace_bytes >= cv.bytes, "pq_search: workspace %zu B < required %zu B (one part)",
               d_workspace ? workspace_bytes : (size_t)0, cv.bytes);
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_workspace) % 16 == 0, "pq_search: workspace must be 16-byte aligned");
  hipStream_t st = sskd::as_stream(stream);
  int rc = pq_launch_lut(d_queries, nq, d_codebooks, m, cv.lut, st);
  if (rc != SSKD_OK) return rc;
  PqScanParams sp{};
  sp.codes = d_codes_csr;
  sp.lut = cv.lut;
  sp.probe = d_probe;
  sp.probe_scores = d_probe_scores;
  sp.list_offsets = d_list_offsets;
  sp.list_rows = d_list_rows;
  sp.row_mask = d_row_mask;
  sp.n_rows = n_rows;
  sp.nq = nq;
  sp.nprobe = nprobe;
  sp.nlist = nlist;
  sp.cap = cap;
  sp.parts = P;
  sp.part_scores = cv.scores;
  sp.part_rows = cv.rows;
  switch (m) {
    case 8: rc = pq_launch_scan<8>(sp, st); break;
    case 16: rc = pq_launch_scan<16>(sp, st); break;
    case 24: rc = pq_launch_scan<24>(sp, st); break;
    case 32: rc = pq_launch_scan<32>(sp, st); break;
    case 48: rc = pq_launch_scan<48>(sp, st); break;
    case 64: rc = pq_launch_scan<64>(sp, st); break;
    default: rc = pq_launch_scan<96>(sp, st); break;
  }
  if (rc != SSKD_OK) return rc;
  PqRefineParams rp{};
  rp.rows = d_tiled;
  rp.queries = d_queries;
  rp.part_scores = cv.scores;
  rp.part_rows = cv.rows;
  rp.n_rows = n_rows;
  rp.id_offset = id_offset;
  rp.nq = nq;
  rp.parts = P;
  rp.cap = cap;
  rp.k = k;
  rp.refine = refine;
  rp.out_scores = d_out_scores;
  rp.out_ids = d_out_ids;
  rp.out_cand = d_out_candidates;
  hipLaunchKernelGGL(pq_refine_kernel, dim3((unsigned)nq), dim3(IVF_THREADS), 0, st, rp);
  return sskd::check_launch("pq_refine_kernel");
}

}  // extern "C"
