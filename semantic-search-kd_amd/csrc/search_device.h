// Index layout and the device helpers that more than one search translation unit uses (internal: not installed).
// What only one of them uses stays there.
#pragma once
#include "common.h"
#include "wave_ops.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// (unnamed namespace: every translation unit gets its own internal copy, as when these lived in search.hip)
namespace {

constexpr int DIM = SSKD_DIM;                 // 384
constexpr int TILE_ROWS = SSKD_TILE_ROWS;     // 32
constexpr int STEPS = DIM / 8;                // 48 k-steps, 8 columns each
constexpr int CHUNKS = DIM / 4;               // 96 float4 chunks per row
constexpr int TILE_FLOATS = TILE_ROWS * DIM;  // 12288 floats = 48 KiB
constexpr int GROUP = 8;                      // k-steps per prefetch group
constexpr int GROUPS = STEPS / GROUP;         // 6 (even: groups alternate A/B)
// The index is a plain ROW-MAJOR fp32 matrix (1 536 B per row), padded with zero rows to a multiple of 32; a "tile" is 32
// consecutive rows.  Lane l of a wave owns row 32 t + (l & 31) of its tile and the column half 4 (l >> 5): k-step u of the
// A operand of v_mfma_f32_32x32x2_f32 is the 16 bytes at columns 8 u + 4 (l >> 5) of that row - a wave-instruction reads 32
// row segments of 32 B, and four consecutive k-steps use every byte of the 128-byte lines they touch.  (Rounds 1-3 stored
// the tiles in MFMA-fragment order - one contiguous KiB per wave-instruction - and kept a SECOND, row-major fp32 copy in
// the screening sidecar for the re-scoring gathers: 2.5x the corpus in HBM.  Same-box A/B in round 4: the exact scan is
// 1.1 % slower on this layout (54.93 -> 55.52 ms at 1 M x 10 k), the single-query path 3 % (0.328 -> 0.338 ms), and one
// copy serves scan, re-scoring, save() and the bf16 conversion: 1.5x the corpus.)
constexpr int STEP_FLOATS = 8;                // a k-step = the next 8 columns of the lane's row
// float4 index, inside a 32-row tile, of chunk c (columns 4c .. 4c + 3) of row r
__host__ __device__ inline int tile_idx4(int r, int c) { return r * (DIM / 4) + c; }
// D layout of both 32x32 MFMAs: accumulator register r of lane l holds column l & 31 and row acc_row(r) + 4 (l >> 5)
__host__ __device__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// score(q, row) of the exact re-scoring: ONE fp32 accumulator from +0.0f, fma over the columns in the order 0, 4, 1, 5, 2,
// 6, 3, 7 of every 8-column k-step - bit for bit the value a search returns for the row.  `src` = the row (96 float4),
// `qv` = the prepared query (384 floats, 16-byte aligned; LDS in the callers).  mine.hip scores positives with it,
// hybrid.hip the rows a ranking lacks.
__device__ inline float row_score_fma(const float4* src, const float* qv) {
  float acc = 0.f;
#pragma unroll 16
  for (int u = 0; u < STEPS; ++u) {
    const float4 a = src[2 * u], c = src[2 * u + 1];
    const float4 qa = *reinterpret_cast<const float4*>(&qv[8 * u]), qc = *reinterpret_cast<const float4*>(&qv[8 * u + 4]);
    acc = fmaf(a.x, qa.x, acc); acc = fmaf(c.x, qc.x, acc);
    acc = fmaf(a.y, qa.y, acc); acc = fmaf(c.y, qc.y, acc);
    acc = fmaf(a.z, qa.z, acc); acc = fmaf(c.z, qc.z, acc);
    acc = fmaf(a.w, qa.w, acc); acc = fmaf(c.w, qc.w, acc);
  }
  return acc;
}

// the same chain over a row of 8 * steps columns (any width that is a multiple of 8): the bits sskd_similarity returns
// for the pair.  eval.hip scores a query's own candidate list with it.
__device__ inline float row_score_fma(const float4* src, const float* qv, int steps) {
  float acc = 0.f;
#pragma unroll 4
  for (int u = 0; u < steps; ++u) {
    const float4 a = src[2 * u], c = src[2 * u + 1];
    const float4 qa = *reinterpret_cast<const float4*>(&qv[8 * u]), qc = *reinterpret_cast<const float4*>(&qv[8 * u + 4]);
    acc = fmaf(a.x, qa.x, acc); acc = fmaf(c.x, qc.x, acc);
    acc = fmaf(a.y, qa.y, acc); acc = fmaf(c.y, qc.y, acc);
    acc = fmaf(a.z, qa.z, acc); acc = fmaf(c.z, qc.z, acc);
    acc = fmaf(a.w, qa.w, acc); acc = fmaf(c.w, qc.w, acc);
  }
  return acc;
}

// bit r of a row allow-mask given as words (the per-row test; the tile scans test a whole word, below); null = all allowed.
// (Spelled as an early return: as `!mask || bit` the list scans' position -> row step compiles to other control flow.)
template <typename I>
__device__ inline bool row_allowed(const uint32_t* mask, I r) {
  if (mask && ((mask[r >> 5] >> (r & 31)) & 1u) == 0u) return false;
  return true;
}

// number of queries to serve: the host bound, or the device-side count when one is given (the
// screened search sizes its exact fallback launch for a cap and lets the device say how many exist)
__device__ inline int eff_nq(int nq_host, const int* nq_dev) {
  if (!nq_dev) return nq_host;
  const int n = *nq_dev;
  return n < nq_host ? n : nq_host;
}

// strict "a ranks before b": higher score first, then lower id
template <typename I>
__device__ inline bool ranks_before(float sa, I ia, float sb, I ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// wave-wide arg-best in rank order (higher score, then lower id); i < 0 = nothing
template <typename I>
__device__ inline void wave_argbest(float& s, I& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(s, o);
    const I oi = __shfl_xor(i, o);
    if (oi >= 0 && (i < 0 || ranks_before(os, oi, s, i))) { s = os; i = oi; }
  }
}

// one candidate (v, id) of a selection round: it becomes the lane's best (s, i) when it ranks strictly after the last
// selected entry (bs, bi) - if there is one - and before the best so far
template <typename I>
__device__ inline void pick_after(float& s, I& i, float v, I id, bool have, float bs, I bi) {
  if (have && !ranks_before(bs, bi, v, id)) return;
  if (i < 0 || ranks_before(v, id, s, i)) { s = v; i = id; }
}

// Shared threshold.  Every per-lane list that is full holds K distinct rows scoring >= its K-th
// entry, so that entry is a lower bound on the query's final K-th score: any row scoring STRICTLY
// less can never reach the result and need not enter any list.  The bound is shared across all
// lanes / waves / workgroups of a query through one word per query updated with atomicMax on a
// monotone integer image of the float.  Reads may be stale (per-XCD L2s are not coherent): a stale
// value is a smaller bound, i.e. less pruning, never a wrong result.  Rows scoring exactly the
// bound are kept (they may still win on the id tie-break).
__device__ inline int float_to_ordered(float x) {
  const int b = __float_as_int(x);
  return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
__device__ inline float ordered_to_float(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7FFFFFFF); }

// Workgroup pool.  A single list's K-th entry is a weak bound (a list sees 1/128 of a query's
// rows).  Every row a lane accepts is therefore also offered to a per-query pool of K slots in LDS
// shared by the workgroup's 16 lists: lock-free, "replace the current minimum by compare-and-swap".
// Slot values only grow and each is the score of a distinct row seen by this workgroup, so the
// minimum over any (even stale) snapshot of a full pool is a valid lower bound on the query's
// final K-th score; it is cached in `wthr` (one LDS word per query, atomicMax - the screening kernel also raises that
// word to the bounds it exchanges through global memory: any lower bound of the final K-th score may stand there).  What a workgroup
// pool accepts after its first tile is forwarded to K **buckets** per query in global memory:
// bucket (row id mod K) keeps the best score of its rows by a no-return atomicMax - fire and
// forget, because a compare-and-swap pool there cost three dependent round trips to the memory
// side per offer (~0.2 ms per workgroup, 13 % of the scan at the 8-GPU shard size).  The buckets
// hold K distinct rows, so their minimum is a valid bound again; it is read only at the exchange
// points (tiles 1, 2, 4, 8, 16, 24, ...), together with `tau`, which carries the workgroups'
// own bounds.  The first tile is skipped because every workgroup starts empty at the same instant.
// Images are the monotone integers of float_to_ordered(); INT_MIN = empty.
template <int K>
__device__ inline bool pool_offer(int* __restrict__ slots, int* __restrict__ thr, int xi) {
#pragma unroll 1
  for (int attempt = 0; attempt < 4; ++attempt) {
    int v[K];
#pragma unroll
    for (int i = 0; i < K; ++i)
      v[i] = slots[i];
    int mn = v[0], mi = 0;
#pragma unroll
    for (int i = 1; i < K; ++i)
      if (v[i] < mn) { mn = v[i]; mi = i; }
    if (xi <= mn) return false;  // not among the K best seen so far
    if (atomicCAS(&slots[mi], mn, xi) == mn) {
      // minimum of our snapshot with the replaced slot
      int nm = xi;
#pragma unroll
      for (int i = 0; i < K; ++i)
        if (i != mi && v[i] < nm) nm = v[i];
      if (nm != (int)0x80000000) atomicMax(thr, nm);
      return true;
    }
  }
  return false;  // lost the race four times: the pool just stays a little looser
}

// bucket xid % K of query q: fire-and-forget atomicMax of a row the workgroup pool accepted
template <int K>
__device__ __forceinline__ void bucket_forward(int* __restrict__ gpool, int q, int xid, int xi) {
  (void)__hip_atomic_fetch_max(gpool + (int64_t)q * K + xid % K, xi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Bound exchange of query q: the minimum of its K global buckets (agent scope) and the workgroup's own bound w are
// published to tau; returns the fresh ordered bound (the larger of tau's old value and the buckets' minimum).
template <int K>
__device__ __forceinline__ int exchange_bound(const int* __restrict__ gpool, int* tau_q, int q, int w) {
  const int* gb = gpool + (int64_t)q * K;
  int bmin = __hip_atomic_load(&gb[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int i = 1; i < K; ++i)
    bmin = min(bmin, __hip_atomic_load(&gb[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  const int old = atomicMax(tau_q, max(w, bmin));
  return max(old, bmin);
}

// The screening kernel's buckets (screen.hip).  The minimum of K buckets is a bound only once ALL K hold a good row - a
// coupon collector's ~29 good rows for K = 10, so it sits near the 29th best score seen.  With B > K buckets keyed by
// (row id mod B) the K-TH LARGEST of the B maxima is a bound as soon as any K of them are filled: distinct buckets hold
// distinct rows, so K maxima at or above v are K distinct allowed rows scoring at least v.  Fewer than K filled buckets
// give INT_MIN ("no bound": it is the K-th largest of the words, empty ones included).
template <int B>
__device__ __forceinline__ void bucket_forward_wide(int* __restrict__ gpool, int q, int xid, int xi) {
  (void)__hip_atomic_fetch_max(gpool + (int64_t)q * B + (unsigned)xid % B, xi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the B bucket words of query q (agent scope, 8 bytes per load: a query's words are B x 4 contiguous, aligned bytes)
template <int B>
__device__ __forceinline__ void bucket_load_wide(int (&v)[B], const int* __restrict__ gpool, int q) {
  static_assert(B % 2 == 0, "two bucket words per load");
  const unsigned long long* gb = reinterpret_cast<const unsigned long long*>(gpool + (int64_t)q * B);
#pragma unroll
  for (int i = 0; i < B / 2; ++i) {
    const unsigned long long w = __hip_atomic_load(gb + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v[2 * i] = (int)(unsigned)w;
    v[2 * i + 1] = (int)(unsigned)(w >> 32);
  }
}

// the K-th largest of B words, as a multiset (equal words count separately), exactly: a K-deep descending list in
// registers, every word carried down it by max / min - 2 K B VALU less the triangle of the first K words, no branches.
// A result ABOVE the true K-th largest would be a bound above the K-th best score: rows of the top K pruned silently
// (tests/test_screen_bound_exchange_gpu.py holds it to numpy.partition through sskd_screen_bucket_bound).
template <int K, int B>
__device__ __forceinline__ int kth_largest(const int (&v)[B]) {
  static_assert(K >= 1 && K <= B, "K-th largest of B words");
  int top[K];
#pragma unroll
  for (int i = 0; i < K; ++i) top[i] = (int)0x80000000;
#pragma unroll
  for (int j = 0; j < B; ++j) {
    int x = v[j];
#pragma unroll
    for (int i = 0; i < K && i <= j; ++i) {
      const int hi = max(top[i], x);
      x = min(top[i], x);
      top[i] = hi;
    }
  }
  return top[K - 1];
}

// Row allow-mask (sskd_amd.h): one 32-bit word per 32-row tile, so the word of tile t is wave-uniform - one scalar
// load per tile.  In the D layout of both 32x32 MFMAs accumulator register r of lane l holds tile row
// (r & 3) + 8 (r >> 2) + 4 (l >> 5), so lane l tests bit (r & 3) + 8 (r >> 2) of word >> 4 (l >> 5).  A masked row's score
// becomes -inf at the same place as a padding row's past n_rows, before any list insertion, pool offer or append: from
// there on the kernels treat it exactly like padding, which no list, pool, bound or run ever holds.
// (read through the constant address space: nothing writes the mask during a search, and that lets the compiler issue an
// s_load instead of a vector load + v_readfirstlane)
typedef const __attribute__((address_space(4))) uint32_t const_u32;
__device__ inline uint32_t tile_mask_word(const uint32_t* __restrict__ row_mask, int t) {
  return ((const_u32*)row_mask)[t];
}
template <int QB>
__device__ inline void apply_tile_mask(f32x16 (&acc)[QB], uint32_t word, int h) {
  if (word == 0xFFFFFFFFu) return;   // (wave-uniform) every row of the tile is allowed
  const uint32_t lw = word >> (4 * h);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const bool off = ((lw >> acc_row(r)) & 1u) == 0u;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq)
      if (off) acc[qq][r] = -INFINITY;
  }
}

__device__ inline void load_group(float4 (&buf)[GROUP], const float* __restrict__ base) {
#pragma unroll
  for (int s = 0; s < GROUP; ++s)
    buf[s] = *reinterpret_cast<const float4*>(base + s * STEP_FLOATS);
}

template <int QB, int G>
__device__ inline void compute_group(const float4 (&a)[GROUP], const float4* __restrict__ qlane,
                                     f32x16 (&acc)[QB]) {
  // compiler-only barrier: keeps the (tile-invariant) LDS query reads inside the
  // group instead of hoisted out of the tile loop into 192 VGPRs
  asm volatile("" ::: "memory");
#pragma unroll
  for (int s = 0; s < GROUP; ++s) {
    const int u = G * GROUP + s;
#pragma unroll
    for (int qq = 0; qq < QB; ++qq) {
      // chunk 2u + h of query j of sub-block qq (h, j folded into qlane)
      const float4 b = qlane[(qq * CHUNKS + 2 * u) * 32];
      acc[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].x, b.x, acc[qq], 0, 0, 0);
      acc[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].y, b.y, acc[qq], 0, 0, 0);
      acc[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].z, b.z, acc[qq], 0, 0, 0);
      acc[qq] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].w, b.w, acc[qq], 0, 0, 0);
    }
  }
}

// The fp32 tile pipeline of one wave: a tile's six groups of k-steps alternate between two register buffers, and the
// first group of the wave's next tile loads while the last group is multiplied.
struct F32TilePipe {
  float4 a[GROUP], b[GROUP];
  // the first group of the wave's first tile
  __device__ __forceinline__ void start(const float* __restrict__ tile) { load_group(a, tile); }
  // acc = the tile's scores (a holds its first group); more: prefetch the first group of the tile WAVES further
  template <int QB, int WAVES>
  __device__ __forceinline__ void score(f32x16 (&acc)[QB], const float* __restrict__ tile,
                                        const float4* __restrict__ qlane, bool more) {
#pragma unroll
    for (int qq = 0; qq < QB; ++qq)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[qq][r] = 0.f;

    load_group(b, tile + 1 * GROUP * STEP_FLOATS);
    compute_group<QB, 0>(a, qlane, acc);
    load_group(a, tile + 2 * GROUP * STEP_FLOATS);
    compute_group<QB, 1>(b, qlane, acc);
    load_group(b, tile + 3 * GROUP * STEP_FLOATS);
    compute_group<QB, 2>(a, qlane, acc);
    load_group(a, tile + 4 * GROUP * STEP_FLOATS);
    compute_group<QB, 3>(b, qlane, acc);
    load_group(b, tile + 5 * GROUP * STEP_FLOATS);
    compute_group<QB, 4>(a, qlane, acc);
    if (more) load_group(a, tile + (int64_t)WAVES * TILE_FLOATS);
    compute_group<QB, 5>(b, qlane, acc);
  }
};

// stage the block of 32 QB queries from q0 in LDS in B-operand order (zero rows past nq): qs[QB][96 chunks][32 queries]
template <int QB, int WAVES>
__device__ __forceinline__ void stage_queries_f32(float4* __restrict__ qs, const float* __restrict__ queries, int q0, int nq) {
  for (int idx = threadIdx.x; idx < QB * 32 * CHUNKS; idx += WAVES * 64) {
    const int c = idx % CHUNKS, jj = idx / CHUNKS;
    const int q = q0 + jj;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < nq) v = reinterpret_cast<const float4*>(queries)[(int64_t)q * CHUNKS + c];
    qs[((jj >> 5) * CHUNKS + c) * 32 + (jj & 31)] = v;
  }
  __syncthreads();
}

}  // namespace
