// ------------------------------------------------------------------------- //
// range search: every allowed row scoring above a per-query threshold (faiss range_search, inner product)
//
// range_scan_kernel streams tiles and stages queries exactly as scan_topk_kernel does (same load_group /
// compute_group order, same padding-row and MASKED handling), so every score is bit for bit the score the exact
// scan returns.  Its epilogue is a fixed per-query threshold: lane j / j + 32 keeps thr[q] in a register and an
// accumulator element x matches iff x > thr (faiss' strict inner-product rule; -inf and NaN never match).
// Matches are appended to a record pool with wave-aggregated reservations: a wave reserves RANGE_CHUNK slots (or
// the tile's overflow, if larger) with ONE returning atomic, and fills them with 16 ballots per 32-query sub-block;
// the slots a wave reserved and did not fill are marked empty (query -1) when it finishes.  Each lane counts its
// matches in a register and adds them to its query's counter once, at the end.  Records past the pool's capacity
// are dropped but still counted, so the counts (and lims) are always exact.
//
// CSR build: lims = exclusive scan of the counts (reduce-then-scan over blocks of RANGE_SCAN_BLOCK queries, any
// nq), the records are scattered into their query's segment of d_out_ids as 64-bit keys, and each segment is
// sorted by key: high word = bit-inverted monotone image of the score, low word = local row, so an ascending sort
// orders by score descending, then row ascending, and decodes back to the exact score.  Segments of up to
// RANGE_SMALL keys are sorted in LDS by a 256-thread workgroup, up to RANGE_BIG (128 KiB of LDS) by a 1024-thread
// one, longer ones by the same workgroup as LDS-sorted chunks of RANGE_BIG plus merge passes through global memory.
// When lims[nq] > max_results the scatter and sort kernels exit on their first instruction, reading the total on
// the device: nothing is written at or past max_results, and lims stays exact.
// ------------------------------------------------------------------------- //
#include "search_device.h"
#include "search_host.h"

#include <algorithm>
#include <cfloat>

using sskd::Plan;
using sskd::make_plan;
using sskd::require_shard_rows;

namespace {

constexpr int RANGE_CHUNK = 128;           // pool slots a wave reserves at a time
constexpr int RANGE_SCAN_BLOCK = 4096;     // counts per block of the lims scan (256 threads x 16)
constexpr int RANGE_SMALL = 2048;          // keys sorted by the small sort kernel (16 KiB of LDS)
constexpr int RANGE_BIG = 16384;           // keys sorted in LDS by the big sort kernel (128 KiB of LDS)

struct RangeParams {
  const float* tiled;
  const float* queries;
  const float* thresholds;   // [nq]
  const uint32_t* row_mask;  // MASKED kernels only
  int* counts;               // [nq] exact match counts (pre-zeroed)
  unsigned long long* pool_next;  // next free pool slot (pre-zeroed)
  int* rec_q;                // [pool_cap] query of a record, -1 = empty slot
  uint64_t* rec_key;         // [pool_cap] range_key(score, row)
  int64_t pool_cap;
  int64_t n_rows;
  int n_tiles;
  int nq;
  int n_slices;
  int tiles_per_slice;
};

// ascending key order = score descending, then row ascending; decodes back to the exact score
__device__ inline uint64_t range_key(float x, int row) {
  const uint32_t hi = ~((uint32_t)float_to_ordered(x) ^ 0x80000000u);
  return ((uint64_t)hi << 32) | (uint32_t)row;
}
__device__ inline float range_key_score(uint64_t key) {
  return ordered_to_float((int)(~(uint32_t)(key >> 32) ^ 0x80000000u));
}

template <int QB, int WAVES, bool MASKED>
__global__ __launch_bounds__(WAVES * 64) void range_scan_kernel(RangeParams p) {
  extern __shared__ float4 qs[];  // [QB][96 chunks][32 queries]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int j = lane & 31, h = lane >> 5;
  const int slice = blockIdx.x % p.n_slices;
  const int qblk = blockIdx.x / p.n_slices;
  const int q0 = qblk * (32 * QB);
  const int nq = p.nq;
  if (q0 >= nq) return;  // (workgroup-uniform)

  stage_queries_f32<QB, WAVES>(qs, p.queries, q0, nq);
  const float4* qlane = qs + h * 32 + j;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  float thr[QB];
  int cnt[QB];
#pragma unroll
  for (int qq = 0; qq < QB; ++qq) {
    const int q = q0 + qq * 32 + j;
    thr[qq] = q < nq ? p.thresholds[q] : INFINITY;   // padding queries never match
    cnt[qq] = 0;
  }
  // the wave's current pool reservation: slots [cur, cur + rem) are reserved and not yet filled
  int64_t cur = 0;
  int rem = 0;

  const int t_begin = slice * p.tiles_per_slice;
  const int t_end = min(t_begin + p.tiles_per_slice, p.n_tiles);
  const float* lane_base = p.tiled + (lane & 31) * DIM + 4 * (lane >> 5);
  const bool ragged = (p.n_rows & 31) != 0;

  F32TilePipe pipe;
  int t = t_begin + wave;
  if (t < t_end) pipe.start(lane_base + (int64_t)t * TILE_FLOATS);

  for (; t < t_end; t += WAVES) {
    const float* tile = lane_base + (int64_t)t * TILE_FLOATS;
    uint32_t mword = 0xFFFFFFFFu;
    if constexpr (MASKED) mword = tile_mask_word(p.row_mask, t);
    f32x16 acc[QB];
    pipe.score<QB, WAVES>(acc, tile, qlane, t + WAVES < t_end);
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
      uint32_t bits = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (acc[qq][r] > thr[qq]) bits |= 1u << r;   // -inf and NaN never compare greater
      cnt[qq] += __popc(bits);
      if (!__any(bits != 0u) || p.pool_cap == 0) continue;
      // wave total and this wave's reservation (wave-uniform)
      int total = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) total += __popcll(__ballot((bits >> r) & 1u));
      const int old_take = min(total, rem);
      int64_t fresh = 0;
      if (total > rem) {
        const int want = max(RANGE_CHUNK, total - rem);
        unsigned long long b = 0;
        if (lane == 0) b = atomicAdd(p.pool_next, (unsigned long long)want);
        fresh = (int64_t)__shfl((long long)b, 0);
      }
      const int q = q0 + qq * 32 + j;
      int off = 0;   // records of earlier r
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const uint64_t b = __ballot((bits >> r) & 1u);
        if ((bits >> r) & 1u) {
          const int o = off + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
          const int64_t slot = o < old_take ? cur + o : fresh + (o - old_take);
          if (slot < p.pool_cap) {
            p.rec_q[slot] = q;
            p.rec_key[slot] = range_key(acc[qq][r], rowbase + acc_row(r));
          }
        }
        off += __popcll(b);
      }
      if (total > rem) {
        const int want = max(RANGE_CHUNK, total - rem);
        cur = fresh + (total - old_take);
        rem = want - (total - old_take);
      } else {
        cur += total;
        rem -= total;
      }
    }
  }
  // slots reserved and never filled: mark them empty for the scatter
  for (int i = lane; i < rem; i += 64)
    if (cur + i < p.pool_cap) p.rec_q[cur + i] = -1;
  // exact per-query counts: lanes j and j + 32 share query j
#pragma unroll
  for (int qq = 0; qq < QB; ++qq) {
    const int c = cnt[qq] + __shfl_xor(cnt[qq], 32);
    const int q = q0 + qq * 32 + j;
    if (h == 0 && q < nq && c) atomicAdd(&p.counts[q], c);
  }
}

// ---- lims: exclusive scan of the counts over any nq (reduce, scan of the block sums, scan) ----

__device__ inline int64_t block_exclusive_scan_256(int64_t v, int64_t* s_wave, int64_t* block_total) {
  // wave-inclusive scan, then the four wave totals
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_wave[wave] = x;
  __syncthreads();
  int64_t before = 0, all = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += s_wave[w];
    all += s_wave[w];
  }
  __syncthreads();
  *block_total = all;
  return before + x - v;
}

// The counts come from a source `C` (`C::count_t operator()(int64_t q) const`): CountArray for the range search,
// MergeCounts for the sharded merge.  One workgroup takes RANGE_SCAN_BLOCK queries, 16 per thread.
template <typename C>
__global__ __launch_bounds__(256) void range_count_blocks_kernel(C count, int nq, int64_t* __restrict__ block_sums) {
  __shared__ int64_t s_wave[4];
  const int64_t base = (int64_t)blockIdx.x * RANGE_SCAN_BLOCK + threadIdx.x * 16;
  int64_t v = 0;
  for (int i = 0; i < 16; ++i)
    if (base + i < nq) v += count(base + i);
  int64_t total;
  (void)block_exclusive_scan_256(v, s_wave, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive block offsets (in place); lims[nq] = the total
__global__ __launch_bounds__(256) void range_scan_blocks_kernel(int64_t* __restrict__ block_sums, int n_blocks,
                                                                int64_t* __restrict__ lims, int nq) {
  __shared__ int64_t s_wave[4];
  int64_t carry = 0;
  for (int b0 = 0; b0 < n_blocks; b0 += 256) {
    const int b = b0 + threadIdx.x;
    const int64_t v = b < n_blocks ? block_sums[b] : 0;
    int64_t total;
    const int64_t ex = block_exclusive_scan_256(v, s_wave, &total);
    if (b < n_blocks) block_sums[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) lims[nq] = carry;
}

template <typename C>
__global__ __launch_bounds__(256) void range_lims_kernel(C count, int nq, const int64_t* __restrict__ block_offsets,
                                                         int64_t* __restrict__ lims) {
  __shared__ int64_t s_wave[4];
  const int64_t base = (int64_t)blockIdx.x * RANGE_SCAN_BLOCK + threadIdx.x * 16;
  typename C::count_t c[16];
  int64_t v = 0;
  for (int i = 0; i < 16; ++i) {
    c[i] = base + i < nq ? count(base + i) : 0;
    v += c[i];
  }
  int64_t total;
  int64_t run = block_offsets[blockIdx.x] + block_exclusive_scan_256(v, s_wave, &total);
  for (int i = 0; i < 16; ++i) {
    if (base + i < nq) lims[base + i] = run;
    run += c[i];
  }
}

// lims[0 .. nq] = exclusive scan of count(q), lims[nq] = the total: the three launches of both entry points
template <typename C>
int enqueue_lims_scan(C count, int nq, int64_t* block_sums, int64_t* lims, hipStream_t st) {
  const int n_blocks = (int)sskd::ceil_div(nq, RANGE_SCAN_BLOCK);
  hipLaunchKernelGGL(range_count_blocks_kernel<C>, dim3(n_blocks), dim3(256), 0, st, count, nq, block_sums);
  hipLaunchKernelGGL(range_scan_blocks_kernel, dim3(1), dim3(256), 0, st, block_sums, n_blocks, lims, nq);
  hipLaunchKernelGGL(range_lims_kernel<C>, dim3(n_blocks), dim3(256), 0, st, count, nq, block_sums, lims);
  return sskd::check_launch("range_lims_kernel");
}

struct CountArray {
  typedef int count_t;
  const int* __restrict__ counts;
  __device__ int operator()(int64_t q) const { return counts[q]; }
};

// ---- scatter: pool records -> their query's segment of the key buffer (d_out_ids), any order ----
__global__ __launch_bounds__(256) void range_scatter_kernel(const int* __restrict__ rec_q,
                                                            const uint64_t* __restrict__ rec_key,
                                                            const unsigned long long* __restrict__ pool_next,
                                                            int64_t pool_cap, const int64_t* __restrict__ lims, int nq,
                                                            int64_t max_results, int* __restrict__ cursor,
                                                            uint64_t* __restrict__ seg_keys) {
  if (lims[nq] > max_results) return;   // overflow: lims only
  const int64_t used = (int64_t)*pool_next;
  const int64_t n = used < pool_cap ? used : pool_cap;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int q = rec_q[i];
    if (q < 0) continue;
    const int pos = atomicAdd(&cursor[q], 1);
    if (lims[q] + pos < lims[q + 1]) seg_keys[lims[q] + pos] = rec_key[i];   // (always: a record is a counted match)
  }
}

// ---- per-segment sort ----
template <int NT>
__device__ inline void lds_bitonic_sort(uint64_t* s, int n2) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int i = threadIdx.x; i < (n2 >> 1); i += NT) {
        const int lo = ((i & ~(jj - 1)) << 1) | (i & (jj - 1));
        const int hi = lo + jj;
        const bool asc = (lo & k) == 0;
        const uint64_t a = s[lo], b = s[hi];
        if ((a > b) == asc) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
}

__device__ inline int next_pow2(int x) {
  int n = 1;
  while (n < x) n <<= 1;
  return n;
}

// keys [0, len) of src -> LDS -> sorted -> dst (dst may be src)
template <int NT>
__device__ inline void lds_sort_run(uint64_t* s, const uint64_t* src, uint64_t* dst, int len) {
  const int n2 = next_pow2(len);
  for (int i = threadIdx.x; i < n2; i += NT) s[i] = i < len ? src[i] : ~(uint64_t)0;
  __syncthreads();
  lds_bitonic_sort<NT>(s, n2);
  for (int i = threadIdx.x; i < len; i += NT) dst[i] = s[i];
  __syncthreads();
}

struct RangeSortParams {
  const int64_t* lims;
  int nq;
  int64_t max_results;
  int64_t id_offset;
  uint64_t* keys;      // = d_out_ids as keys (in place)
  uint64_t* scratch;   // >= max_results keys: merge passes of long segments
  float* out_scores;
  int64_t* out_ids;
};

__device__ inline void range_write_segment(const RangeSortParams& p, const uint64_t* s, int64_t seg, int len, int nt) {
  for (int i = threadIdx.x; i < len; i += nt) {
    const uint64_t key = s[i];
    p.out_scores[seg + i] = range_key_score(key);
    p.out_ids[seg + i] = (int64_t)(uint32_t)key + p.id_offset;
  }
}

// one 256-thread workgroup per query: segments of 1 .. RANGE_SMALL keys
__global__ __launch_bounds__(256) void range_sort_small_kernel(RangeSortParams p) {
  __shared__ uint64_t s[RANGE_SMALL];
  if (p.lims[p.nq] > p.max_results) return;
  const int q = blockIdx.x;
  const int64_t seg = p.lims[q];
  const int64_t len = p.lims[q + 1] - seg;
  if (len == 0 || len > RANGE_SMALL) return;
  const int n2 = next_pow2((int)len);
  for (int i = threadIdx.x; i < n2; i += 256) s[i] = i < len ? p.keys[seg + i] : ~(uint64_t)0;
  __syncthreads();
  lds_bitonic_sort<256>(s, n2);
  range_write_segment(p, s, seg, (int)len, 256);
}

// one 1024-thread workgroup per query: segments longer than RANGE_SMALL.  Up to RANGE_BIG keys: one LDS sort.
// Longer: LDS-sorted chunks of RANGE_BIG, then merge passes (runs W -> 2W) between the key buffer and the scratch
// buffer; each key finds its output place by a binary search in the other run (keys are unique within a segment).
__global__ __launch_bounds__(1024) void range_sort_big_kernel(RangeSortParams p) {
  extern __shared__ uint64_t s_big[];   // [RANGE_BIG]
  if (p.lims[p.nq] > p.max_results) return;
  const int q = blockIdx.x;
  const int64_t seg = p.lims[q];
  const int64_t len64 = p.lims[q + 1] - seg;
  if (len64 <= RANGE_SMALL) return;
  const int len = (int)len64;   // <= n_rows < 2^31
  if (len <= RANGE_BIG) {
    const int n2 = next_pow2(len);
    for (int i = threadIdx.x; i < n2; i += 1024) s_big[i] = i < len ? p.keys[seg + i] : ~(uint64_t)0;
    __syncthreads();
    lds_bitonic_sort<1024>(s_big, n2);
    range_write_segment(p, s_big, seg, len, 1024);
    return;
  }
  uint64_t* src = p.keys + seg;
  uint64_t* dst = p.scratch + seg;
  for (int c0 = 0; c0 < len; c0 += RANGE_BIG)
    lds_sort_run<1024>(s_big, src + c0, src + c0, min(RANGE_BIG, len - c0));
  __threadfence();
  __syncthreads();
  for (int w = RANGE_BIG; w < len; w <<= 1) {
    for (int i = threadIdx.x; i < len; i += 1024) {
      const int a = (int)((int64_t)i / (2 * (int64_t)w) * (2 * (int64_t)w));
      const int mid = (int)min((int64_t)a + w, (int64_t)len), end = (int)min((int64_t)a + 2 * (int64_t)w, (int64_t)len);
      const uint64_t key = src[i];
      int lo, hi;
      if (i < mid) { lo = mid; hi = end; } else { lo = a; hi = mid; }
      const int first = lo;
      // left keys count the right keys below them; right keys count the left keys below them
      while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (src[m] < key) lo = m + 1; else hi = m;
      }
      const int pos = i < mid ? a + (i - a) + (lo - first) : a + (i - mid) + (lo - first);
      dst[pos] = key;
    }
    __threadfence();
    __syncthreads();
    uint64_t* tmp = src; src = dst; dst = tmp;
  }
  for (int i = threadIdx.x; i < len; i += 1024) {
    const uint64_t key = src[i];   // (src may be the out_ids segment itself: read before the write)
    p.out_scores[seg + i] = range_key_score(key);
    p.out_ids[seg + i] = (int64_t)(uint32_t)key + p.id_offset;
  }
}

// pool capacity: max_results records plus, per wave, less than one unfilled reservation.  The wave count is bounded
// by a formula that only grows with nq and n_rows (make_plan's own count is not monotone in nq).
int64_t range_pool_cap(int64_t n_rows, int nq, int64_t max_results) {
  if (max_results <= 0) return 0;
  const int64_t n_tiles = sskd::ceil_div(n_rows, TILE_ROWS);
  const int64_t qblocks = nq <= 32 ? 1 : sskd::ceil_div(nq, 64);
  const int64_t max_slices = std::max<int64_t>(1, sskd::ceil_div(n_tiles, 8));
  const int64_t wgs = std::min(qblocks * max_slices, 1024 + 8 * qblocks);
  return max_results + wgs * 8 * RANGE_CHUNK;
}

struct RangeWs {
  int* counts;
  int* cursor;
  unsigned long long* pool_next;
  int64_t* block_sums;
  int* rec_q;
  uint64_t* rec_key;
  size_t head_bytes;   // counts + cursor + pool_next, packed: zeroed by each call with one memset
  size_t bytes;
};

RangeWs range_carve(void* base, int64_t n_rows, int nq, int64_t max_results) {
  sskd::Carver c(base);
  RangeWs w{};
  w.counts = c.take<int>(nq, alignof(int));
  w.cursor = c.take<int>(nq, alignof(int));
  w.pool_next = c.take<unsigned long long>(1, alignof(unsigned long long));
  w.head_bytes = c.off;
  w.block_sums = c.take<int64_t>(sskd::ceil_div(nq, RANGE_SCAN_BLOCK));
  const int64_t cap = range_pool_cap(n_rows, nq, max_results);
  w.rec_key = c.take<uint64_t>(cap);
  w.rec_q = c.take<int>(cap);
  w.bytes = c.bytes();
  return w;
}

template <int QB, bool MASKED>
void launch_range_scan(const Plan& pl, const RangeParams& rp, hipStream_t st) {
  constexpr int WAVES = 8;
  const size_t lds = (size_t)QB * 32 * CHUNKS * sizeof(float4);
  auto kern = range_scan_kernel<QB, WAVES, MASKED>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(pl.n_qblocks * pl.n_slices), dim3(WAVES * 64), lds, st, rp);
}

// ------------------------------------------------------------------------- //
// merge of per-shard range results (sskd_range_merge_packed): n_runs packed records, each one rank's
// sskd_index_range_search output with global ids, -> the CSR result of one range search over the union of the shards.
//
// lims: the count of query q is the sum of its segment lengths over the runs; the exclusive scan is the range CSR
// build's (block sums, one-workgroup scan of the block sums, per-block scan).  Placement: one thread per input record.
// Its output slot is lims[q] + its index in its own segment + for every other run, the number of that run's keys in
// q's segment that rank before it (binary search).  The rank order is the range kernel's key order: the monotone
// image float_to_ordered(score) descending, then id ascending (so +0.0 ranks before -0.0).  Ids are distinct across
// runs, so no two keys of a query are equal and its slots are a permutation of [lims[q], lims[q + 1]).  No atomics,
// no sort, one pass.  Every segment bound read from a record is clamped to [0, cap], so a slot never leaves its
// query's output segment, whatever the records hold.
// ------------------------------------------------------------------------- //
struct RangeMergeParams {
  const char* records;
  int64_t rec_bytes;   // stride of the records: sskd_range_record_bytes(nq, cap)
  int64_t cap;
  int nq;
  int64_t* lims;       // [nq + 1] merged
  float* out_scores;
  int64_t* out_ids;
  int64_t max_results;
};

__device__ inline const int64_t* merge_run_lims(const RangeMergeParams& p, int r) {
  return reinterpret_cast<const int64_t*>(p.records + (int64_t)r * p.rec_bytes);
}

// [a, b) of query q's segment in run r, clamped to the record's capacity
__device__ inline void merge_run_segment(const RangeMergeParams& p, const int64_t* lr, int q, int64_t& a, int64_t& b) {
  a = min(max(lr[q], (int64_t)0), p.cap);
  b = min(max(lr[q + 1], a), p.cap);
}

struct MergeCounts {
  typedef int64_t count_t;
  RangeMergeParams p;
  int n_runs;
  __device__ int64_t operator()(int64_t q) const {
    int64_t c = 0;
    for (int r = 0; r < n_runs; ++r) {
      int64_t a, b;
      merge_run_segment(p, merge_run_lims(p, r), (int)q, a, b);
      c += b - a;
    }
    return c;
  }
};

// grid (x: records of a run, grid-stride; y: the run)
__global__ __launch_bounds__(256) void range_merge_place_kernel(RangeMergeParams p) {
  if (p.lims[p.nq] > p.max_results) return;   // overflow: lims only
  const int r = blockIdx.y, n_runs = gridDim.y, nq = p.nq;
  const int64_t* lr = merge_run_lims(p, r);
  const int64_t* ids = lr + nq + 1;
  const float* scores = reinterpret_cast<const float*>(ids + p.cap);
  const int64_t n = min(max(lr[nq], (int64_t)0), p.cap);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    // the query of record i: the first q whose segment ends past i
    int lo = 0, hi = nq;
    while (lo < hi) {
      const int m = (lo + hi) >> 1;
      if (lr[m + 1] <= i) lo = m + 1; else hi = m;
    }
    if (lo >= nq) continue;
    const int q = lo;
    int64_t a, b;
    merge_run_segment(p, lr, q, a, b);
    if (i < a || i >= b) continue;   // (only for records whose lims are not monotone)
    const float x = scores[i];
    const int64_t id = ids[i];
    const int xo = float_to_ordered(x);
    int64_t pos = p.lims[q] + (i - a);
    for (int s = 0; s < n_runs; ++s) {
      if (s == r) continue;
      const int64_t* ls = merge_run_lims(p, s);
      const int64_t* ids_s = ls + nq + 1;
      const float* scores_s = reinterpret_cast<const float*>(ids_s + p.cap);
      int64_t sa, sb;
      merge_run_segment(p, ls, q, sa, sb);
      int64_t l = sa, h = sb;
      while (l < h) {   // keys of run s ranking before (x, id) form a prefix of its segment
        const int64_t m = (l + h) >> 1;
        const int mo = float_to_ordered(scores_s[m]);
        if (mo > xo || (mo == xo && ids_s[m] < id)) l = m + 1; else h = m;
      }
      pos += l - sa;
    }
    if (pos < p.lims[q + 1]) {
      p.out_scores[pos] = x;
      p.out_ids[pos] = id;
    }
  }
}

struct RangeMergeWs {
  int64_t* block_sums;
  size_t bytes;
};

RangeMergeWs range_merge_carve(void* base, int nq) {
  sskd::Carver c(base);
  RangeMergeWs w{};
  w.block_sums = c.take<int64_t>(sskd::ceil_div(nq, RANGE_SCAN_BLOCK));
  w.bytes = c.bytes();
  return w;
}

}  // namespace

extern "C" {

size_t sskd_index_range_search_workspace_bytes(int64_t n_rows, int nq, int64_t max_results) {
  if (n_rows <= 0 || nq <= 0 || max_results < 0) return 0;
  return range_carve(nullptr, n_rows, nq, max_results).bytes;
}

int sskd_index_range_search(const float* d_tiled, int64_t n_rows, const float* d_queries, int nq,
                            const float* d_thresholds, int64_t id_offset, const uint32_t* d_row_mask, int64_t* d_lims,
                            float* d_out_scores, int64_t* d_out_ids, int64_t max_results, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "index_range_search: n_rows < 0");
  SSKD_REQUIRE(nq >= 0, "index_range_search: nq < 0");
  SSKD_REQUIRE(max_results >= 0, "index_range_search: max_results < 0");
  SSKD_REQUIRE(d_lims, "index_range_search: null lims");
  int rc = require_shard_rows("index_range_search", n_rows);
  if (rc != SSKD_OK) return rc;
  const bool empty = nq == 0 || n_rows == 0;
  const RangeWs w = range_carve(d_workspace, n_rows, nq, max_results);
  if (!empty) {
    SSKD_REQUIRE(d_tiled && d_queries && d_thresholds, "index_range_search: null pointer");
    SSKD_REQUIRE(max_results == 0 || (d_out_scores && d_out_ids), "index_range_search: null output with max_results > 0");
    if ((rc = sskd::require_workspace("index_range_search", d_workspace, workspace_bytes, w.bytes)) != SSKD_OK) return rc;
  }
  hipStream_t st = sskd::as_stream(stream);
  if (empty) {
    if (hipMemsetAsync(d_lims, 0, ((size_t)nq + 1) * sizeof(int64_t), st) != hipSuccess)
      return sskd::fail(SSKD_ERR_HIP, "index_range_search: memset failed");
    return SSKD_OK;
  }
  const int64_t cap = range_pool_cap(n_rows, nq, max_results);
  if (hipMemsetAsync(d_workspace, 0, w.head_bytes, st) != hipSuccess)
    return sskd::fail(SSKD_ERR_HIP, "index_range_search: memset failed");

  const Plan pl = make_plan(n_rows, nq, 10);
  RangeParams rp{};
  rp.tiled = d_tiled;
  rp.queries = d_queries;
  rp.thresholds = d_thresholds;
  rp.row_mask = d_row_mask;
  rp.counts = w.counts;
  rp.pool_next = w.pool_next;
  rp.rec_q = w.rec_q;
  rp.rec_key = w.rec_key;
  rp.pool_cap = cap;
  rp.n_rows = n_rows;
  rp.n_tiles = pl.n_tiles;
  rp.nq = nq;
  rp.n_slices = pl.n_slices;
  rp.tiles_per_slice = pl.tiles_per_slice;
  if (pl.QB == 1) {
    if (d_row_mask) launch_range_scan<1, true>(pl, rp, st);
    else launch_range_scan<1, false>(pl, rp, st);
  } else {
    if (d_row_mask) launch_range_scan<2, true>(pl, rp, st);
    else launch_range_scan<2, false>(pl, rp, st);
  }
  rc = sskd::check_launch("range_scan_kernel");
  if (rc != SSKD_OK) return rc;

  if ((rc = enqueue_lims_scan(CountArray{w.counts}, nq, w.block_sums, d_lims, st)) != SSKD_OK) return rc;
  if (max_results == 0) return SSKD_OK;   // count-only

  uint64_t* keys = reinterpret_cast<uint64_t*>(d_out_ids);
  const int64_t scatter_blocks = std::min<int64_t>(sskd::ceil_div(cap, 256), 2048);
  hipLaunchKernelGGL(range_scatter_kernel, dim3((unsigned)scatter_blocks), dim3(256), 0, st, w.rec_q, w.rec_key,
                     w.pool_next, cap, d_lims, nq, max_results, w.cursor, keys);
  if ((rc = sskd::check_launch("range_scatter_kernel")) != SSKD_OK) return rc;
  RangeSortParams sp{};
  sp.lims = d_lims;
  sp.nq = nq;
  sp.max_results = max_results;
  sp.id_offset = id_offset;
  sp.keys = keys;
  sp.scratch = w.rec_key;   // the pool is dead after the scatter; it holds >= max_results keys
  sp.out_scores = d_out_scores;
  sp.out_ids = d_out_ids;
  hipLaunchKernelGGL(range_sort_small_kernel, dim3(nq), dim3(256), 0, st, sp);
  if ((rc = sskd::check_launch("range_sort_small_kernel")) != SSKD_OK) return rc;
  const size_t big_lds = (size_t)RANGE_BIG * sizeof(uint64_t);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(range_sort_big_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds);
  hipLaunchKernelGGL(range_sort_big_kernel, dim3(nq), dim3(1024), big_lds, st, sp);
  return sskd::check_launch("range_sort_big_kernel");
}

size_t sskd_range_record_bytes(int nq, int64_t cap) {
  if (nq < 0 || cap < 0) return 0;
  return (((size_t)nq + 1) * sizeof(int64_t) + (size_t)cap * (sizeof(int64_t) + sizeof(float)) + 15) & ~(size_t)15;
}

size_t sskd_range_merge_workspace_bytes(int n_runs, int nq, int64_t max_results) {
  if (n_runs < 1 || nq <= 0 || max_results < 0) return 0;
  return range_merge_carve(nullptr, nq).bytes;
}

int sskd_range_merge_packed(const void* d_records, int n_runs, int nq, int64_t cap, int64_t* d_lims,
                            float* d_out_scores, int64_t* d_out_ids, int64_t max_results, void* d_workspace,
                            size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_runs >= 1 && n_runs <= 65535, "range_merge_packed: n_runs=%d outside [1, 65535]", n_runs);
  SSKD_REQUIRE(nq >= 0, "range_merge_packed: nq < 0");
  SSKD_REQUIRE(cap >= 0, "range_merge_packed: cap < 0");
  SSKD_REQUIRE(max_results >= 0, "range_merge_packed: max_results < 0");
  SSKD_REQUIRE(d_records && d_lims, "range_merge_packed: null records or lims");
  SSKD_REQUIRE((reinterpret_cast<uintptr_t>(d_records) & 7) == 0, "range_merge_packed: records must be 8-byte aligned");
  SSKD_REQUIRE(max_results == 0 || (d_out_scores && d_out_ids), "range_merge_packed: null output with max_results > 0");
  const RangeMergeWs w = range_merge_carve(d_workspace, nq);
  int rc;
  if (nq > 0 &&
      (rc = sskd::require_workspace("range_merge_packed", d_workspace, workspace_bytes, w.bytes)) != SSKD_OK)
    return rc;
  hipStream_t st = sskd::as_stream(stream);
  if (nq == 0) {
    if (hipMemsetAsync(d_lims, 0, sizeof(int64_t), st) != hipSuccess)
      return sskd::fail(SSKD_ERR_HIP, "range_merge_packed: memset failed");
    return SSKD_OK;
  }
  RangeMergeParams p{};
  p.records = static_cast<const char*>(d_records);
  p.rec_bytes = (int64_t)sskd_range_record_bytes(nq, cap);
  p.cap = cap;
  p.nq = nq;
  p.lims = d_lims;
  p.out_scores = d_out_scores;
  p.out_ids = d_out_ids;
  p.max_results = max_results;
  if ((rc = enqueue_lims_scan(MergeCounts{p, n_runs}, nq, w.block_sums, d_lims, st)) != SSKD_OK) return rc;
  if (max_results == 0 || cap == 0) return SSKD_OK;   // count-only, or nothing to place
  const int64_t blocks = std::min<int64_t>(sskd::ceil_div(cap, 256), 2048);
  hipLaunchKernelGGL(range_merge_place_kernel, dim3((unsigned)blocks, (unsigned)n_runs), dim3(256), 0, st, p);
  return sskd::check_launch("range_merge_place_kernel");
}

}  // extern "C"
