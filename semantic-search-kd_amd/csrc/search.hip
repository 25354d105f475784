// Exact inner-product top-k over an fp32 corpus in HBM (gfx950 / MI355X).
//
// Replaces faiss `index.add` / `index.search` behind the reference's
// FAISSIndexBuilder (reference: src/serve/app.py:293-301,
// scripts/build_faiss_index.py:49-62, tests/conftest.py:184-185) and the
// exact-search idiom `np.argsort(scores)[::-1][:k]` (src/kd/eval.py:86).
//
// Data layout (see include/sskd_amd.h): the index is the plain row-major fp32
// matrix, zero-padded to a multiple of 32 rows; a "tile" is 32 consecutive rows
// and lane l of a wave reads its A-operand k-steps straight from row
// 32 t + (l & 31) (details and the round-4 measurement beside STEP_FLOATS in search_device.h).
//
// Scan kernel: one workgroup = one block of 32*QB queries (held in LDS in
// B-operand order) x one slice of corpus tiles.  Each wave streams its own
// tiles HBM -> VGPR (software-pipelined 8 KiB ahead), feeds the fp32 MFMA, and
// keeps a per-lane sorted top-K list in registers (lane j / j+32 own query j).
// The lists of all waves / slices are merged by merge_topk_kernel.
//
// This file is the fp32 scan with its merge, reduce and one-pass kernels, the launch plan and sskd::exact_search;
// the other subsystems are index_rows.hip, screen.hip, range.hip and grouped.hip (source map: DESIGN.md section 3).
#include "search_device.h"
#include "search_host.h"

#include <algorithm>
#include <cfloat>
#include <cstdlib>

using sskd::Plan;
using sskd::make_plan;
using sskd::require_shard_rows;

namespace {

// ------------------------------------------------------------------------- //
// scan
// ------------------------------------------------------------------------- //

struct ScanParams {
  const float* tiled;
  const float* queries;
  float* part_scores;    // [nq][lists_per_query][K]
  int* part_ids;
  const float* ub_scores;  // chained pass: exclusive upper bound per query
  const int* ub_ids;
  int* tau;                // shared per-query threshold (monotone int image of a float), see search_device.h
  int* gpool;              // [nq][K] global buckets (best score of rows with id % K == b)
  int64_t n_rows;
  int n_tiles;
  int nq;
  int n_slices;
  int tiles_per_slice;
  int lists_per_query;
  const int* nq_dev;       // optional: the number of queries actually present (<= nq) lives on the device
  const uint32_t* row_mask;  // MASKED kernels only: ceil(n_rows / 32) allow words (row r = bit r & 31 of word r >> 5)
};

#ifndef SSKD_TAU_REFRESH_TILES
#define SSKD_TAU_REFRESH_TILES 8
#endif
constexpr int TAU_REFRESH_TILES = SSKD_TAU_REFRESH_TILES;  // exchange bounds with global memory every this many tiles

#ifdef SSKD_PROBE
// diagnostic build only (tools/scan_probe.hip): [0] tiles, [1] slow-path entries, [2] per-register
// insertion blocks executed, [3] lane insertions, [4] threshold publications
__device__ unsigned long long g_scan_probe[8];
#define SSKD_COUNT(i, n) do { const unsigned long long n_ = (unsigned long long)(n); if ((threadIdx.x & 63) == 0) atomicAdd(&g_scan_probe[i], n_); } while (0)
#else
#define SSKD_COUNT(i, n) do {} while (0)
#endif

template <int K>
struct LaneList {
  float s[K];
  int id[K];
  __device__ inline void clear() {
#pragma unroll
    for (int i = 0; i < K; ++i) { s[i] = -INFINITY; id[i] = -1; }
  }
  // precondition: x > s[K-1]. Rows reach a lane in increasing id order, so a
  // strict compare keeps the lower id ahead among equal scores.
  __device__ inline void insert(float x, int xid) {
    s[K - 1] = x;
    id[K - 1] = xid;
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
      const bool sw = s[i] > s[i - 1];
      const float a = s[i - 1], b = s[i];
      const int ia = id[i - 1], ib = id[i];
      s[i - 1] = sw ? b : a;
      s[i] = sw ? a : b;
      id[i - 1] = sw ? ib : ia;
      id[i] = sw ? ia : ib;
    }
  }
};

// POOLS = false: plain per-lane lists, no shared bound - then the ONLY reason a row is missing from
// a query's candidates is that its own list was full of better rows, which is what the one-pass
// search for k > K relies on (sskd_index_search_onepass).
// MASKED: rows whose bit in p.row_mask is clear score -inf (tile_mask_word, search_device.h).  A list, pool or bucket only ever
// takes scores above -inf, so every full list / pool still holds K distinct ALLOWED rows: the shared bounds, the
// chained passes' upper bound and the one-pass proof hold for the allowed rows as they do for the whole shard.
template <int K, int QB, int WAVES, bool HAS_UB, bool POOLS = true, bool MASKED = false>
__global__ __launch_bounds__(WAVES * 64) void scan_topk_kernel(ScanParams p) {
  extern __shared__ float4 qs[];  // [QB][96 chunks][32 queries]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int slice = blockIdx.x % p.n_slices;  // blocks b, b+8 share an XCD: a slice stays on one L2
  const int qblk = blockIdx.x / p.n_slices;
  const int q0 = qblk * (32 * QB);
  const int nq = eff_nq(p.nq, p.nq_dev);
  if (q0 >= nq) return;  // (workgroup-uniform)

  stage_queries_f32<QB, WAVES>(qs, p.queries, q0, nq);
  const float4* qlane = qs + h * 32 + j;

  // workgroup pool: [QB * 32 queries][K slots] + one cached minimum per query, behind the query block
  int* const pool = reinterpret_cast<int*>(qs + QB * 32 * CHUNKS);
  int* const wthr = pool + QB * 32 * K;
  for (int i = tid; i < QB * 32 * (K + 1); i += WAVES * 64) pool[i] = (int)0x80000000;
  __syncthreads();

  LaneList<K> list[QB];
  float ub_s[QB];
  int ub_i[QB];
  float gthr[QB];  // best known lower bound on the query's final K-th score
  int* tau_q[QB];
  bool real[QB];  // padding queries (>= nq) share the last query's words and must never write them
#pragma unroll
  for (int qq = 0; qq < QB; ++qq) {
    gthr[qq] = -INFINITY;
    const int qg = q0 + qq * 32 + j;
    real[qq] = qg < nq;
    tau_q[qq] = p.tau + (real[qq] ? qg : nq - 1);
    list[qq].clear();
    ub_s[qq] = INFINITY;
    ub_i[qq] = -1;
    if (HAS_UB) {
      const int q = q0 + qq * 32 + j;
      if (q < nq) { ub_s[qq] = p.ub_scores[q]; ub_i[qq] = p.ub_ids[q]; }
    }
  }

  const int t_begin = slice * p.tiles_per_slice;
  const int t_end = min(t_begin + p.tiles_per_slice, p.n_tiles);
  const float* lane_base = p.tiled + (lane & 31) * DIM + 4 * (lane >> 5);   // row (lane & 31) of a tile, column half lane >> 5
  const bool ragged = (p.n_rows & 31) != 0;

  F32TilePipe pipe;
  int t = t_begin + wave;
  if (t < t_end) pipe.start(lane_base + (int64_t)t * TILE_FLOATS);

  int tiles_done = 0;
  for (; t < t_end; t += WAVES, ++tiles_done) {
    const float* tile = lane_base + (int64_t)t * TILE_FLOATS;
    uint32_t mword = 0xFFFFFFFFu;
    if constexpr (MASKED) mword = tile_mask_word(p.row_mask, t);   // issued ahead of the tile's MFMAs
    // the workgroup's bound every tile (one LDS word), the global one every few tiles: an atomic
    // executes at the memory side, so it both publishes ours and returns a fresh value
    const bool exchange = tiles_done < TAU_REFRESH_TILES ? (tiles_done & (tiles_done - 1)) == 0
                                                         : tiles_done % TAU_REFRESH_TILES == 0;
#pragma unroll
    for (int qq = 0; POOLS && qq < QB; ++qq) {
      const int w = wthr[qq * 32 + j];
      gthr[qq] = fmaxf(gthr[qq], ordered_to_float(w));
      if (exchange && real[qq])
        gthr[qq] = fmaxf(gthr[qq], ordered_to_float(exchange_bound<K>(p.gpool, tau_q[qq], q0 + qq * 32 + j, w)));
    }
    f32x16 acc[QB];
    pipe.score<QB, WAVES>(acc, tile, qlane, t + WAVES < t_end);
    // D layout of the 32x32 MFMA: column = lane & 31 (query), row = acc_row(r) + 4h
    const int rowbase = t * TILE_ROWS + 4 * h;
    if (ragged && t == p.n_tiles - 1) {
#pragma unroll
      for (int qq = 0; qq < QB; ++qq)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (rowbase + acc_row(r) >= p.n_rows) acc[qq][r] = -INFINITY;
    }
    if constexpr (MASKED) apply_tile_mask<QB>(acc, mword, h);
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
      float m = acc[qq][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) m = fmaxf(m, acc[qq][r]);
      SSKD_COUNT(0, 1);
      if (__any(m > list[qq].s[K - 1] && m >= gthr[qq])) {
        SSKD_COUNT(1, 1);
        bool grew = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float x = acc[qq][r];
          const int xid = rowbase + acc_row(r);
          bool take = x > list[qq].s[K - 1] && x >= gthr[qq];
          if (HAS_UB) take = take && ranks_before(ub_s[qq], ub_i[qq], x, xid);
          if (__any(take)) {
            SSKD_COUNT(2, 1);
            SSKD_COUNT(3, __popcll(__ballot(take)));
            if (take) {
              list[qq].insert(x, xid);
              // (a wave's first tile fills empty lists: nearly every row is taken, so only the
              // best of them is offered afterwards instead of all sixteen)
              if (POOLS && tiles_done > 0) {
                const int xi = float_to_ordered(x);
                if (pool_offer<K>(pool + (qq * 32 + j) * K, wthr + qq * 32 + j, xi) && real[qq])
                  bucket_forward<K>(p.gpool, q0 + qq * 32 + j, xid, xi);
              }
              grew = true;
            }
          }
        }
        // pick up what the pool learned (our own list's K-th entry is implied by it)
        if (POOLS && grew) {
          SSKD_COUNT(4, __popcll(__ballot(true)));
          if (tiles_done == 0)
            pool_offer<K>(pool + (qq * 32 + j) * K, wthr + qq * 32 + j,
                                 float_to_ordered(list[qq].s[0]));
          gthr[qq] = fmaxf(gthr[qq], fmaxf(ordered_to_float(wthr[qq * 32 + j]), list[qq].s[K - 1]));
        }
      }
    }
  }

  // per-lane lists -> global partials [q][slice, wave, h][K]
#pragma unroll
  for (int qq = 0; qq < QB; ++qq) {
    const int q = q0 + qq * 32 + j;
    if (q < nq) {
      const int64_t base =
          ((int64_t)q * p.lists_per_query + (slice * WAVES + wave) * 2 + h) * K;
#pragma unroll
      for (int i = 0; i < K; ++i) {
        p.part_scores[base + i] = list[qq].s[i];
        p.part_ids[base + i] = list[qq].id[i];
      }
    }
  }
}

// ------------------------------------------------------------------------- //
// merge: one wave per query, `count` rounds of bounded arg-best
// ------------------------------------------------------------------------- //

template <typename IdT>
struct MergeParams {
  const float* scores;
  const IdT* ids;
  int64_t list_stride;     // score elements between consecutive lists of one query
  int64_t id_list_stride;  // id elements between consecutive lists of one query
  int64_t q_stride;        // elements between consecutive queries
  int k_in;             // entries per list
  int n_cand;           // n_lists * k_in
  int nq;
  float* out_scores;    // [nq][out_stride], written at [out_off, out_off + count)
  int64_t* out_ids;
  int out_stride;
  int out_off;
  int count;
  int64_t id_offset;
  float* ub_scores;     // optional: last selected (score, local id) per query
  int* ub_ids;
  const int* nq_dev;    // optional device-side query count (see eff_nq)
};

template <typename IdT>
__global__ __launch_bounds__(256) void merge_topk_kernel(MergeParams<IdT> p) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= eff_nq(p.nq, p.nq_dev)) return;
  const float* sc = p.scores + (int64_t)q * p.q_stride;
  const IdT* id = p.ids + (int64_t)q * p.q_stride;

  float bs = INFINITY;  // bound: last selected entry
  long long bi = -1;
  bool have_bound = false;
  float last_s = -INFINITY;
  long long last_i = -1;
  for (int r = 0; r < p.count; ++r) {
    float best_s = -INFINITY;
    long long best_i = -1;
    for (int c = lane; c < p.n_cand; c += 64) {
      const int l = c / p.k_in, e = c - l * p.k_in;
      const long long ci = (long long)id[(int64_t)l * p.id_list_stride + e];
      if (ci < 0) continue;
      pick_after(best_s, best_i, sc[(int64_t)l * p.list_stride + e], ci, have_bound, bs, bi);
    }
    wave_argbest(best_s, best_i);
    if (lane == 0) {
      const int64_t o = (int64_t)q * p.out_stride + p.out_off + r;
      p.out_scores[o] = best_i >= 0 ? best_s : -FLT_MAX;
      p.out_ids[o] = best_i >= 0 ? (int64_t)best_i + p.id_offset : -1;
    }
    if (best_i < 0) {
      // exhausted: fill the rest and stop
      if (lane == 0) {
        for (int rr = r + 1; rr < p.count; ++rr) {
          const int64_t o = (int64_t)q * p.out_stride + p.out_off + rr;
          p.out_scores[o] = -FLT_MAX;
          p.out_ids[o] = -1;
        }
      }
      last_s = -INFINITY;
      last_i = 0x7fffffff;  // nothing ranks after this bound
      break;
    }
    bs = best_s;
    bi = best_i;
    have_bound = true;
    last_s = best_s;
    last_i = best_i;
  }
  if (p.ub_scores && lane == 0) {
    p.ub_scores[q] = last_s;
    p.ub_ids[q] = (int)last_i;
  }
}

// ------------------------------------------------------------------------- //
// group reduce: one wave per (query, group of `lpg` consecutive lists).  The group's candidates
// (<= 1024) are loaded once and its best k are picked in registers; the output has the layout of
// the input ([query][list][k], sorted lists, (-FLT_MAX, -1) padding), so the step can be repeated.
// It keeps the single-wave final merge short when few queries are spread over many slices
// (one query over 1 M rows leaves > 4000 per-lane lists).
// ------------------------------------------------------------------------- //
constexpr int REDUCE_CPL = 16;               // candidates per lane
constexpr int REDUCE_MAX_CAND = 64 * REDUCE_CPL;
constexpr int MERGE_DIRECT_MAX_LISTS = 64;   // the final merge reads its candidates from memory

struct ReduceParams {
  const float* scores;  // [nq][lists_in][k]   (k entries per input list)
  const int* ids;
  int k;
  int k_out;            // entries per output list (>= k when a wide result is collected)
  int lists_in;
  int lpg;              // lists per group, lpg * k <= REDUCE_MAX_CAND
  int groups;
  int nq;
  const int* nq_dev;    // optional device-side query count (see eff_nq)
  float* out_scores;    // [nq][groups][k_out]
  int* out_ids;
};

__global__ __launch_bounds__(256) void reduce_lists_kernel(ReduceParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (int64_t)eff_nq(p.nq, p.nq_dev) * p.groups) return;
  const int q = (int)(w / p.groups), g = (int)(w - (int64_t)q * p.groups);
  const int first = g * p.lpg;
  const int n_lists = min(p.lpg, p.lists_in - first);
  const int n_cand = n_lists * p.k;
  const int64_t base = ((int64_t)q * p.lists_in + first) * p.k;
  float cs[REDUCE_CPL];
  int ci[REDUCE_CPL];
#pragma unroll
  for (int j = 0; j < REDUCE_CPL; ++j) {
    const int c = lane + 64 * j;
    const bool in = c < n_cand;
    ci[j] = in ? p.ids[base + c] : -1;
    cs[j] = in ? p.scores[base + c] : -FLT_MAX;
  }
  const int64_t ob = ((int64_t)q * p.groups + g) * p.k_out;
  for (int r = 0; r < p.k_out; ++r) {
    float best_s = -INFINITY;
    int best_i = -1;
#pragma unroll
    for (int j = 0; j < REDUCE_CPL; ++j)
      if (ci[j] >= 0 && (best_i < 0 || ranks_before(cs[j], ci[j], best_s, best_i))) {
        best_s = cs[j];
        best_i = ci[j];
      }
    wave_argbest(best_s, best_i);
    if (lane == 0) {
      p.out_scores[ob + r] = best_i >= 0 ? best_s : -FLT_MAX;
      p.out_ids[ob + r] = best_i;
    }
    // row ids are unique among a query's candidates: retire the winner wherever it lives
#pragma unroll
    for (int j = 0; j < REDUCE_CPL; ++j)
      if (ci[j] == best_i) ci[j] = -1;
  }
}

// ------------------------------------------------------------------------- //
// one-pass search for k > K (few queries): proof of exactness
//
// After a scan WITHOUT pools, a row is missing from a query's candidates only if its own list was
// full and it ranks after that list's last entry.  Let E be the best-ranked last entry over the
// query's FULL lists: every missing row ranks after E, so the candidates that rank at or before E
// are exactly the global top of the ranking.  If the k-th best candidate ranks at or before E (or
// no list is full), the candidates' top k is the exact answer.
// ------------------------------------------------------------------------- //
struct BoundParams {
  const float* scores;  // [nq][lists][k] per-lane lists of the scan
  const int* ids;
  int k;
  int lists;
  int nq;
  float* bound_s;       // [nq] E (score, id); id = -1: no list is full
  int* bound_i;
};

__global__ __launch_bounds__(256) void last_entry_bound_kernel(BoundParams p) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= p.nq) return;
  const int64_t base = (int64_t)q * p.lists * p.k + (p.k - 1);
  float bs = -INFINITY;
  int bi = -1;
  for (int l = lane; l < p.lists; l += 64) {
    const int ci = p.ids[base + (int64_t)l * p.k];
    if (ci < 0) continue;  // list not full: it dropped nothing
    const float cs = p.scores[base + (int64_t)l * p.k];
    if (bi < 0 || ranks_before(cs, ci, bs, bi)) { bs = cs; bi = ci; }
  }
  wave_argbest(bs, bi);
  if (lane == 0) {
    p.bound_s[q] = bs;
    p.bound_i[q] = bi;
  }
}

struct FinalizeParams {
  const float* scores;  // [nq][k] best candidates in rank order, (-FLT_MAX, -1) padded
  const int* ids;
  const float* bound_s;
  const int* bound_i;
  int k;
  int nq;
  int64_t id_offset;
  float* out_scores;    // [nq][k]
  int64_t* out_ids;
  int* inexact;         // [1], pre-zeroed: set to 1 if some query's top k is not proven
};

__global__ __launch_bounds__(256) void finalize_onepass_kernel(FinalizeParams p) {
  const int q = blockIdx.x;
  for (int r = threadIdx.x; r < p.k; r += 256) {
    const int64_t o = (int64_t)q * p.k + r;
    const int ci = p.ids[o];
    p.out_scores[o] = ci >= 0 ? p.scores[o] : -FLT_MAX;
    p.out_ids[o] = ci >= 0 ? (int64_t)ci + p.id_offset : -1;
  }
  if (threadIdx.x == 0) {
    const int bi = p.bound_i[q];
    if (bi >= 0) {
      const int64_t o = (int64_t)q * p.k + (p.k - 1);
      const int ci = p.ids[o];
      const float cs = p.scores[o], bs = p.bound_s[q];
      const bool proven = ci >= 0 && !ranks_before(bs, bi, cs, ci);   // at or before E
      if (!proven) atomicExch(p.inexact, 1);
    }
  }
}

__global__ __launch_bounds__(256) void fill_int_kernel(int* p, int n, int v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ __launch_bounds__(256) void fill_empty_kernel(float* s, int64_t* ids, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) { s[i] = -FLT_MAX; ids[i] = -1; }
}

}  // namespace

// ------------------------------------------------------------------------- //
// launch plan
// ------------------------------------------------------------------------- //

namespace sskd {

Plan make_plan(int64_t n_rows, int nq, int k, const sskd_search_tuning* tn) {
  Plan pl{};
  pl.n_tiles = (int)sskd::ceil_div(n_rows, TILE_ROWS);
  const int kk = k < SSKD_K_PASS ? k : SSKD_K_PASS;
  pl.K = kk <= 10 ? 10 : (kk <= 16 ? 16 : 32);
  // k > SSKD_K_PASS is served by chained passes of K results each (a pass returns exactly the next
  // K in rank order because no list can hold more than K of them).  With a handful of queries a
  // wave sees only a few tiles, filling 32-deep lists dominates a pass (5 ms against 1.4 ms for
  // K = 10 at 1 M rows), and more passes of the light kernel win.
  if (k > SSKD_K_PASS && nq <= 64) pl.K = 10;
  pl.passes = (int)sskd::ceil_div(k, pl.K);
  pl.waves = 8;
  int qb = nq > 32 ? 2 : 1;
  if (tn && (tn->queries_per_block == 32 || tn->queries_per_block == 64)) qb = tn->queries_per_block / 32;
  if (pl.K == 32) qb = 1;  // register budget: 2 x 64 list registers do not fit 2 waves/SIMD
  pl.QB = qb;
  pl.n_qblocks = (int)sskd::ceil_div(nq, 32 * qb);
  // enough workgroups to fill 256 CUs several times over; slices in multiples
  // of 8 so that blockIdx % 8 (the XCD label) is a function of the slice
  // (a couple of query blocks - the online /search shape - want one or two workgroups per CU
  // with many tiles each, not a thousand short ones)
  const int target_wgs = (tn && tn->target_workgroups > 0) ? tn->target_workgroups
                                                           : (pl.n_qblocks <= 2 ? 512 : 1024);
  int slices = (int)sskd::ceil_div(target_wgs, pl.n_qblocks);
  slices = (int)sskd::ceil_div(slices, 8) * 8;
  const int max_slices = (int)sskd::ceil_div(pl.n_tiles, pl.waves);  // >= 1 tile per wave
  if (slices > max_slices) slices = max_slices;
  if (slices < 1) slices = 1;
  pl.tiles_per_slice = (int)sskd::ceil_div(pl.n_tiles > 0 ? pl.n_tiles : 1, slices);
  pl.n_slices = (int)sskd::ceil_div(pl.n_tiles > 0 ? pl.n_tiles : 1, pl.tiles_per_slice);
  pl.lists_per_query = pl.n_slices * pl.waves * 2;
  pl.part_elems = (size_t)nq * pl.lists_per_query * pl.K;
  // group-reduce steps before the final merge (see reduce_lists_kernel)
  // shared pruning pools: when a wave sees only a few tiles (few queries spread over many slices:
  // the online shape) they cost more than they prune: one query over 1 M rows 1.7 -> 0.33 ms
  // without them.  Measured crossover (tools/pools_sweep.py, 1 M and 125 k rows, 64..4096
  // queries): 24-32 tiles per wave; the batch configurations of bench.py have 61.
  pl.pools = (tn && tn->pruning_pools != 0) ? tn->pruning_pools > 0 : pl.tiles_per_slice >= 24 * pl.waves;
  pl.reduce_elems = pl.lists_per_query > MERGE_DIRECT_MAX_LISTS
                        ? (size_t)nq * sskd::ceil_div(pl.lists_per_query, REDUCE_MAX_CAND / pl.K) * pl.K
                        : 0;
  return pl;
}

}  // namespace sskd

namespace {

// workspace of the exact search (chained passes): sized by exact_carve(nullptr, ...).bytes
struct ExactWs {
  float* part_scores;
  int* part_ids;
  float* ub_scores;
  int* ub_ids;
  int* tau;             // [nq] + gpool [nq * K]
  float* red_scores[2];  // the reduce steps' ping-pong buffers
  int* red_ids[2];
  size_t bytes;
};

ExactWs exact_carve(void* base, const Plan& pl, int nq) {
  sskd::Carver c(base);
  ExactWs w{};
  w.part_scores = c.take<float>(pl.part_elems);
  w.part_ids = c.take<int>(pl.part_elems);
  w.ub_scores = c.take<float>(nq);
  w.ub_ids = c.take<int>(nq);
  w.tau = c.take<int>((size_t)nq * (1 + pl.K));
  for (int i = 0; i < 2; ++i) {
    w.red_scores[i] = c.take<float>(pl.reduce_elems);
    w.red_ids[i] = c.take<int>(pl.reduce_elems);
  }
  w.bytes = c.bytes();
  return w;
}

// One reduce_lists_kernel step: per query, the candidates' `lists` lists of k_in entries become ceil(lists / lpg)
// lists of k_out in (out_scores, out_ids).  On return (scores, ids, lists) describe the step's output.
int launch_reduce(const float*& scores, const int*& ids, int& lists, int k_in, int k_out, int nq, const int* nq_dev,
                  float* out_scores, int* out_ids, hipStream_t st) {
  ReduceParams rp{};
  rp.scores = scores;
  rp.ids = ids;
  rp.k = k_in;
  rp.k_out = k_out;
  rp.lists_in = lists;
  rp.lpg = REDUCE_MAX_CAND / k_in;
  rp.groups = (int)sskd::ceil_div(lists, rp.lpg);
  rp.nq = nq;
  rp.nq_dev = nq_dev;
  rp.out_scores = out_scores;
  rp.out_ids = out_ids;
  hipLaunchKernelGGL(reduce_lists_kernel, dim3((unsigned)sskd::ceil_div((int64_t)nq * rp.groups, 4)), dim3(256), 0, st, rp);
  scores = out_scores;
  ids = out_ids;
  lists = rp.groups;
  return sskd::check_launch("reduce_lists_kernel");
}

template <int K, int QB, bool HAS_UB, bool POOLS = true, bool MASKED = false>
void launch_scan(const Plan& pl, const ScanParams& sp, hipStream_t st) {
  constexpr int WAVES = 8;
  const size_t lds = (size_t)QB * 32 * CHUNKS * sizeof(float4) + (size_t)QB * 32 * (K + 1) * sizeof(int);
  auto kern = scan_topk_kernel<K, QB, WAVES, HAS_UB, POOLS, MASKED>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(pl.n_qblocks * pl.n_slices), dim3(WAVES * 64), lds, st, sp);
}

template <bool HAS_UB, bool MASKED>
int dispatch_scan_as(const Plan& pl, const ScanParams& sp, hipStream_t st) {
  const bool few = !pl.pools;
  if (pl.K == 10 && pl.QB == 1 && few) launch_scan<10, 1, HAS_UB, false, MASKED>(pl, sp, st);
  else if (pl.K == 10 && pl.QB == 2 && few) launch_scan<10, 2, HAS_UB, false, MASKED>(pl, sp, st);
  else if (pl.K == 10 && pl.QB == 1) launch_scan<10, 1, HAS_UB, true, MASKED>(pl, sp, st);
  else if (pl.K == 10 && pl.QB == 2) launch_scan<10, 2, HAS_UB, true, MASKED>(pl, sp, st);
  else if (pl.K == 16 && pl.QB == 1) launch_scan<16, 1, HAS_UB, true, MASKED>(pl, sp, st);
  else if (pl.K == 16 && pl.QB == 2) launch_scan<16, 2, HAS_UB, true, MASKED>(pl, sp, st);
  else if (pl.K == 32 && pl.QB == 1) launch_scan<32, 1, HAS_UB, true, MASKED>(pl, sp, st);
  else return sskd::fail(SSKD_ERR_UNSUPPORTED, "no scan kernel for K=%d QB=%d", pl.K, pl.QB);
  return sskd::check_launch("scan_topk_kernel");
}

// a NULL row mask takes the unmasked instantiation
template <bool HAS_UB>
int dispatch_scan(const Plan& pl, const ScanParams& sp, hipStream_t st) {
  return sp.row_mask ? dispatch_scan_as<HAS_UB, true>(pl, sp, st) : dispatch_scan_as<HAS_UB, false>(pl, sp, st);
}

}  // namespace

// ------------------------------------------------------------------------- //
// C-ABI
// ------------------------------------------------------------------------- //

size_t sskd::exact_workspace_bytes(int64_t n_rows, int nq, int k, const sskd_search_tuning* tn) {
  return exact_carve(nullptr, make_plan(n_rows, nq, k, tn), nq).bytes;
}

extern "C" {

size_t sskd_index_search_workspace_bytes(int64_t n_rows, int nq, int k) {
  return sskd_index_search_workspace_bytes_ex(n_rows, nq, k, nullptr);
}

size_t sskd_index_search_workspace_bytes_ex(int64_t n_rows, int nq, int k,
                                            const sskd_search_tuning* tuning) {
  if (n_rows < 0 || nq <= 0 || k <= 0) return 0;
  return sskd::exact_workspace_bytes(n_rows, nq, k, tuning);
}

int sskd_index_search_plan(int64_t n_rows, int nq, int k, int* queries_per_block,
                           int* corpus_passes, int* n_slices, int* waves_per_block,
                           int* scan_passes) {
  return sskd_index_search_plan_ex(n_rows, nq, k, nullptr, queries_per_block, corpus_passes,
                                   n_slices, waves_per_block, scan_passes);
}

int sskd_index_search_plan_ex(int64_t n_rows, int nq, int k, const sskd_search_tuning* tuning,
                              int* queries_per_block, int* corpus_passes, int* n_slices,
                              int* waves_per_block, int* scan_passes) {
  SSKD_REQUIRE(n_rows >= 0 && nq > 0 && k > 0, "index_search_plan: bad shape");
  const Plan pl = make_plan(n_rows, nq, k, tuning);
  if (queries_per_block) *queries_per_block = 32 * pl.QB;
  if (corpus_passes) *corpus_passes = pl.n_qblocks * pl.passes;
  if (n_slices) *n_slices = pl.n_slices;
  if (waves_per_block) *waves_per_block = pl.waves;
  if (scan_passes) *scan_passes = pl.passes;
  return SSKD_OK;
}

int sskd_index_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, int k,
                      int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                      void* d_workspace, size_t workspace_bytes, void* stream) {
  return sskd_index_search_ex(d_tiled, n_rows, d_queries, nq, k, id_offset, d_out_scores,
                              d_out_ids, d_workspace, workspace_bytes, stream, nullptr, nullptr,
                              nullptr);
}

int sskd_index_search_profiled(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                               int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                               void* d_workspace, size_t workspace_bytes, void* stream,
                               void* ev_scan_begin, void* ev_scan_end) {
  return sskd_index_search_ex(d_tiled, n_rows, d_queries, nq, k, id_offset, d_out_scores,
                              d_out_ids, d_workspace, workspace_bytes, stream, nullptr,
                              ev_scan_begin, ev_scan_end);
}

int sskd_index_search_ex(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                         int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                         void* d_workspace, size_t workspace_bytes, void* stream,
                         const sskd_search_tuning* tuning, void* ev_scan_begin, void* ev_scan_end) {
  return sskd::exact_search(d_tiled, n_rows, d_queries, nq, k, id_offset, d_out_scores, d_out_ids, d_workspace,
                            workspace_bytes, stream, tuning, ev_scan_begin, ev_scan_end, nullptr, nullptr);
}

int sskd_index_search_filtered(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq, int k,
                               int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores,
                               int64_t* d_out_ids, void* d_workspace, size_t workspace_bytes, void* stream,
                               const sskd_search_tuning* tuning, void* ev_scan_begin, void* ev_scan_end) {
  return sskd::exact_search(d_tiled, n_rows, d_queries, nq, k, id_offset, d_out_scores, d_out_ids, d_workspace,
                            workspace_bytes, stream, tuning, ev_scan_begin, ev_scan_end, nullptr, d_row_mask);
}

}  // extern "C"

int sskd::exact_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                       int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                       void* d_workspace, size_t workspace_bytes, void* stream,
                       const sskd_search_tuning* tuning, void* ev_scan_begin, void* ev_scan_end,
                       const int* nq_dev, const uint32_t* row_mask) {
  SSKD_REQUIRE(n_rows >= 0, "index_search: n_rows < 0");
  SSKD_REQUIRE(nq >= 0, "index_search: nq < 0");
  SSKD_REQUIRE(k >= 1 && k <= SSKD_K_MAX, "index_search: k=%d outside [1, %d]", k, SSKD_K_MAX);
  int rc = require_shard_rows("index_search", n_rows);
  if (rc != SSKD_OK) return rc;
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_queries && d_out_scores && d_out_ids, "index_search: null pointer");
  hipStream_t st = sskd::as_stream(stream);
  if (n_rows == 0) {
    const int64_t n = (int64_t)nq * k;
    hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)sskd::ceil_div(n, 256)), dim3(256), 0, st,
                       d_out_scores, d_out_ids, n);
    return sskd::check_launch("fill_empty_kernel");
  }
  SSKD_REQUIRE(d_tiled, "index_search: null index");
  const Plan pl = make_plan(n_rows, nq, k, tuning);
  const ExactWs w = exact_carve(d_workspace, pl, nq);
  if ((rc = sskd::require_workspace("index_search", d_workspace, workspace_bytes, w.bytes)) != SSKD_OK) return rc;

  ScanParams sp{};
  sp.tiled = d_tiled;
  sp.queries = d_queries;
  sp.part_scores = w.part_scores;
  sp.part_ids = w.part_ids;
  sp.ub_scores = w.ub_scores;
  sp.ub_ids = w.ub_ids;
  sp.tau = w.tau;
  sp.gpool = w.tau + nq;  // filled together with tau
  sp.n_rows = n_rows;
  sp.n_tiles = pl.n_tiles;
  sp.nq = nq;
  sp.n_slices = pl.n_slices;
  sp.tiles_per_slice = pl.tiles_per_slice;
  sp.lists_per_query = pl.lists_per_query;
  sp.nq_dev = nq_dev;
  sp.row_mask = row_mask;

  for (int pass = 0; pass < pl.passes; ++pass) {
    hipLaunchKernelGGL(fill_int_kernel, dim3((unsigned)sskd::ceil_div(nq * (1 + pl.K), 256)), dim3(256),
                       0, st, w.tau, nq * (1 + pl.K), (int)0x80000000);
    if (pass == 0 && ev_scan_begin) (void)hipEventRecord(static_cast<hipEvent_t>(ev_scan_begin), st);
    rc = pass == 0 ? dispatch_scan<false>(pl, sp, st) : dispatch_scan<true>(pl, sp, st);
    if (pass == 0 && ev_scan_end) (void)hipEventRecord(static_cast<hipEvent_t>(ev_scan_end), st);
    if (rc != SSKD_OK) return rc;
    const float* cand_scores = w.part_scores;
    const int* cand_ids = w.part_ids;
    int lists = pl.lists_per_query;
    for (int step = 0; lists > MERGE_DIRECT_MAX_LISTS; ++step)
      if ((rc = launch_reduce(cand_scores, cand_ids, lists, pl.K, pl.K, nq, nq_dev, w.red_scores[step & 1],
                              w.red_ids[step & 1], st)) != SSKD_OK)
        return rc;
    MergeParams<int> mp{};
    mp.nq_dev = nq_dev;
    mp.scores = cand_scores;
    mp.ids = cand_ids;
    mp.list_stride = pl.K;
    mp.id_list_stride = pl.K;
    mp.q_stride = (int64_t)lists * pl.K;
    mp.k_in = pl.K;
    mp.n_cand = lists * pl.K;
    mp.nq = nq;
    mp.out_scores = d_out_scores;
    mp.out_ids = d_out_ids;
    mp.out_stride = k;
    mp.out_off = pass * pl.K;
    mp.count = (k - pass * pl.K) < pl.K ? (k - pass * pl.K) : pl.K;
    mp.id_offset = id_offset;
    mp.ub_scores = (pass + 1 < pl.passes) ? w.ub_scores : nullptr;
    mp.ub_ids = w.ub_ids;
    hipLaunchKernelGGL(merge_topk_kernel<int>, dim3((unsigned)sskd::ceil_div(nq, 4)), dim3(256), 0,
                       st, mp);
    rc = sskd::check_launch("merge_topk_kernel");
    if (rc != SSKD_OK) return rc;
  }
  return SSKD_OK;
}

extern "C" {

namespace {
constexpr int ONEPASS_MAX_NQ = 64, ONEPASS_MAX_K = 256;

// plan of the one-pass search: the K = 10 geometry of a k = 10 search, without pools
Plan onepass_plan(int64_t n_rows, int nq) {
  Plan pl = make_plan(n_rows, nq, 10);
  pl.pools = false;
  return pl;
}

struct OnepassWs {
  float* part_scores;
  int* part_ids;
  float* red_scores[2];  // reduce levels: per-lane lists (10 each) -> [groups][k] -> ... -> [1][k]
  int* red_ids[2];
  float* bound_s;
  int* bound_i;
  size_t bytes;
};

OnepassWs onepass_carve(void* base, const Plan& pl, int nq, int k) {
  const size_t re = (size_t)nq * sskd::ceil_div(pl.lists_per_query, REDUCE_MAX_CAND / pl.K) * k;
  sskd::Carver c(base);
  OnepassWs w{};
  w.part_scores = c.take<float>(pl.part_elems);
  w.part_ids = c.take<int>(pl.part_elems);
  for (int i = 0; i < 2; ++i) {
    w.red_scores[i] = c.take<float>(re);
    w.red_ids[i] = c.take<int>(re);
  }
  w.bound_s = c.take<float>(nq);
  w.bound_i = c.take<int>(nq);
  w.bytes = c.bytes();
  return w;
}

// merge of n_lists int64-id lists of k_in per query into the top k_out (sskd_topk_merge, sskd_topk_merge_packed);
// list l of query q starts at scores[l * list_stride + q * k_in] and ids[l * id_list_stride + q * k_in]
int launch_merge_i64(const float* scores, const int64_t* ids, int64_t list_stride, int64_t id_list_stride, int n_lists,
                     int nq, int k_in, int k_out, float* d_out_scores, int64_t* d_out_ids, void* stream, const char* what) {
  MergeParams<int64_t> mp{};
  mp.scores = scores;
  mp.ids = ids;
  mp.list_stride = list_stride;
  mp.id_list_stride = id_list_stride;
  mp.q_stride = k_in;
  mp.k_in = k_in;
  mp.n_cand = n_lists * k_in;
  mp.nq = nq;
  mp.out_scores = d_out_scores;
  mp.out_ids = d_out_ids;
  mp.out_stride = k_out;
  mp.count = k_out;
  hipLaunchKernelGGL(merge_topk_kernel<int64_t>, dim3((unsigned)sskd::ceil_div(nq, 4)), dim3(256), 0,
                     sskd::as_stream(stream), mp);
  return sskd::check_launch(what);
}
}  // namespace

size_t sskd_index_search_onepass_workspace_bytes(int64_t n_rows, int nq, int k) {
  if (n_rows < 0 || nq <= 0 || nq > ONEPASS_MAX_NQ || k <= 0 || k > ONEPASS_MAX_K) return 0;
  return onepass_carve(nullptr, onepass_plan(n_rows, nq), nq, k).bytes;
}

int sskd_index_search_onepass(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                              int k, int64_t id_offset, float* d_out_scores, int64_t* d_out_ids,
                              int* d_inexact, void* d_workspace, size_t workspace_bytes,
                              void* stream) {
  return sskd_index_search_onepass_filtered(d_tiled, n_rows, d_queries, nq, k, id_offset, nullptr, d_out_scores,
                                            d_out_ids, d_inexact, d_workspace, workspace_bytes, stream);
}

int sskd_index_search_onepass_filtered(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                                       int k, int64_t id_offset, const uint32_t* d_row_mask, float* d_out_scores,
                                       int64_t* d_out_ids, int* d_inexact, void* d_workspace,
                                       size_t workspace_bytes, void* stream) {
  SSKD_REQUIRE(n_rows >= 1, "index_search_onepass: empty index");
  SSKD_REQUIRE(nq >= 1 && nq <= ONEPASS_MAX_NQ, "index_search_onepass: nq=%d outside [1, %d]", nq,
               ONEPASS_MAX_NQ);
  SSKD_REQUIRE(k >= 1 && k <= ONEPASS_MAX_K, "index_search_onepass: k=%d outside [1, %d]", k,
               ONEPASS_MAX_K);
  int rc = require_shard_rows("index_search_onepass", n_rows);
  if (rc != SSKD_OK) return rc;
  SSKD_REQUIRE(d_tiled && d_queries && d_out_scores && d_out_ids && d_inexact,
               "index_search_onepass: null pointer");
  const Plan pl = onepass_plan(n_rows, nq);
  const OnepassWs w = onepass_carve(d_workspace, pl, nq, k);
  if ((rc = sskd::require_workspace("index_search_onepass", d_workspace, workspace_bytes, w.bytes)) != SSKD_OK) return rc;
  hipStream_t st = sskd::as_stream(stream);

  hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(256), 0, st, d_inexact, 1, 0);
  ScanParams sp{};
  sp.tiled = d_tiled;
  sp.queries = d_queries;
  sp.part_scores = w.part_scores;
  sp.part_ids = w.part_ids;
  sp.ub_scores = nullptr;
  sp.ub_ids = nullptr;
  sp.tau = w.bound_i;    // unused without pools (never dereferenced), kept non-null
  sp.gpool = w.bound_i;
  sp.n_rows = n_rows;
  sp.n_tiles = pl.n_tiles;
  sp.nq = nq;
  sp.n_slices = pl.n_slices;
  sp.tiles_per_slice = pl.tiles_per_slice;
  sp.lists_per_query = pl.lists_per_query;
  sp.row_mask = d_row_mask;
  if ((rc = dispatch_scan<false>(pl, sp, st)) != SSKD_OK) return rc;

  BoundParams bp{};
  bp.scores = w.part_scores;
  bp.ids = w.part_ids;
  bp.k = pl.K;
  bp.lists = pl.lists_per_query;
  bp.nq = nq;
  bp.bound_s = w.bound_s;
  bp.bound_i = w.bound_i;
  hipLaunchKernelGGL(last_entry_bound_kernel, dim3((unsigned)sskd::ceil_div(nq, 4)), dim3(256), 0, st, bp);
  rc = sskd::check_launch("last_entry_bound_kernel");
  if (rc != SSKD_OK) return rc;

  const float* cand_scores = w.part_scores;
  const int* cand_ids = w.part_ids;
  int lists = pl.lists_per_query;
  for (int step = 0; step == 0 || lists > 1; ++step)
    if ((rc = launch_reduce(cand_scores, cand_ids, lists, step == 0 ? pl.K : k, k, nq, nullptr, w.red_scores[step & 1],
                            w.red_ids[step & 1], st)) != SSKD_OK)
      return rc;
  FinalizeParams fp{};
  fp.scores = cand_scores;
  fp.ids = cand_ids;
  fp.bound_s = w.bound_s;
  fp.bound_i = w.bound_i;
  fp.k = k;
  fp.nq = nq;
  fp.id_offset = id_offset;
  fp.out_scores = d_out_scores;
  fp.out_ids = d_out_ids;
  fp.inexact = d_inexact;
  hipLaunchKernelGGL(finalize_onepass_kernel, dim3(nq), dim3(256), 0, st, fp);
  return sskd::check_launch("finalize_onepass_kernel");
}

int sskd_topk_merge(const float* d_scores, const int64_t* d_ids, int n_lists, int nq, int k_in,
                    int k_out, float* d_out_scores, int64_t* d_out_ids, void* stream) {
  SSKD_REQUIRE(n_lists >= 1 && nq >= 0 && k_in >= 1 && k_out >= 1, "topk_merge: bad shape");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_scores && d_ids && d_out_scores && d_out_ids, "topk_merge: null pointer");
  return launch_merge_i64(d_scores, d_ids, (int64_t)nq * k_in, (int64_t)nq * k_in, n_lists, nq, k_in, k_out, d_out_scores,
                          d_out_ids, stream, "merge_topk_kernel<int64>");
}

size_t sskd_topk_record_bytes(int nq, int k) {
  if (nq <= 0 || k <= 0) return 0;
  return ((size_t)nq * k * (sizeof(int64_t) + sizeof(float)) + 15) & ~(size_t)15;
}

int sskd_topk_merge_packed(const void* d_records, int n_lists, int nq, int k_in, int k_out,
                           float* d_out_scores, int64_t* d_out_ids, void* stream) {
  SSKD_REQUIRE(n_lists >= 1 && nq >= 0 && k_in >= 1 && k_out >= 1, "topk_merge_packed: bad shape");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_records && d_out_scores && d_out_ids, "topk_merge_packed: null pointer");
  SSKD_REQUIRE((reinterpret_cast<uintptr_t>(d_records) & 7) == 0, "topk_merge_packed: records must be 8-byte aligned");
  const size_t rec = sskd_topk_record_bytes(nq, k_in);
  const char* base = static_cast<const char*>(d_records);
  return launch_merge_i64(reinterpret_cast<const float*>(base + (size_t)nq * k_in * sizeof(int64_t)),
                          reinterpret_cast<const int64_t*>(base), (int64_t)(rec / sizeof(float)),
                          (int64_t)(rec / sizeof(int64_t)), n_lists, nq, k_in, k_out, d_out_scores, d_out_ids, stream,
                          "merge_topk_kernel<int64> (packed)");
}

}  // extern "C"
