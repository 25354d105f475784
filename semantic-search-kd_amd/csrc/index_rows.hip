// The rows of the index and the masks over them (gfx950 / MI355X): add / get / normalise, the row allow-masks,
// the similarity matrix and compaction.  Layout: search_device.h; the search paths themselves: search.hip, screen.hip,
// range.hip, grouped.hip.
#include "search_device.h"
#include "search_host.h"

using sskd::require_shard_rows;

// ------------------------------------------------------------------------- //
// index add / get / normalise
// ------------------------------------------------------------------------- //
namespace {

// One workgroup per tile of 32 rows, one wave per 8 rows: copy (optionally x / ||x||), zero rows past n_rows.
__global__ __launch_bounds__(256) void index_add_rows_kernel(
    const float4* __restrict__ rows, int64_t n_rows, int normalize, float4* __restrict__ tiled,
    int64_t dst_tile0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * TILE_ROWS;
  float4* out = tiled + (dst_tile0 + blockIdx.x) * (int64_t)(TILE_ROWS * CHUNKS);
  for (int rr = 0; rr < 8; ++rr) {
    const int r = wave * 8 + rr;
    const int64_t row = row0 + r;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (row < n_rows) {
      v0 = rows[row * CHUNKS + lane];
      if (lane < CHUNKS - 64) v1 = rows[row * CHUNKS + 64 + lane];
    }
    float ss = v0.x * v0.x + v0.y * v0.y + v0.z * v0.z + v0.w * v0.w;
    ss += v1.x * v1.x + v1.y * v1.y + v1.z * v1.z + v1.w * v1.w;
    ss = wave_sum(ss);
    const float sc = (normalize && ss > 0.f) ? 1.0f / sqrtf(ss) : 1.0f;
    v0.x *= sc; v0.y *= sc; v0.z *= sc; v0.w *= sc;
    v1.x *= sc; v1.y *= sc; v1.z *= sc; v1.w *= sc;
    out[r * CHUNKS + lane] = v0;
    if (lane < CHUNKS - 64) out[r * CHUNKS + 64 + lane] = v1;
  }
}

__global__ __launch_bounds__(256) void index_get_rows_kernel(const float4* __restrict__ tiled,
                                                             int64_t row0, int64_t n_rows,
                                                             float4* __restrict__ rows) {
  const int64_t total = n_rows * CHUNKS;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t r = idx / CHUNKS;
    const int c = (int)(idx - r * CHUNKS);
    const int64_t row = row0 + r;
    rows[idx] = tiled[row * CHUNKS + c];
  }
}

// one wave per row, any dim; x / ||x|| (faiss.normalize_L2: zero rows untouched)
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(float* __restrict__ x,
                                                               int64_t n_rows, int dim) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  float* p = x + row * dim;
  float ss = 0.f;
  for (int i = lane; i < dim; i += 64) ss += p[i] * p[i];
  ss = wave_sum(ss);
  if (ss > 0.f) {
    const float s = 1.0f / sqrtf(ss);
    for (int i = lane; i < dim; i += 64) p[i] *= s;
  }
}

}  // namespace

extern "C" {

int64_t sskd_index_padded_rows(int64_t n_rows) {
  return n_rows <= 0 ? 0 : sskd::ceil_div(n_rows, TILE_ROWS) * TILE_ROWS;
}

size_t sskd_index_tiled_bytes(int64_t n_rows) {
  return (size_t)sskd_index_padded_rows(n_rows) * DIM * sizeof(float);
}

int sskd_index_add_rows(const float* d_rows, int64_t n_rows, int normalize, float* d_tiled,
                        int64_t dst_row0, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "index_add_rows: n_rows < 0");
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_rows && d_tiled, "index_add_rows: null pointer");
  SSKD_REQUIRE(dst_row0 >= 0 && dst_row0 % TILE_ROWS == 0,
               "index_add_rows: dst_row0 must be a non-negative multiple of %d", TILE_ROWS);
  const int64_t tiles = sskd::ceil_div(n_rows, TILE_ROWS);
  hipLaunchKernelGGL(index_add_rows_kernel, dim3((unsigned)tiles), dim3(256), 0,
                     sskd::as_stream(stream), reinterpret_cast<const float4*>(d_rows), n_rows,
                     normalize, reinterpret_cast<float4*>(d_tiled), dst_row0 / TILE_ROWS);
  return sskd::check_launch("index_add_rows_kernel");
}

int sskd_index_get_rows(const float* d_tiled, int64_t row0, int64_t n_rows, float* d_rows,
                        void* stream) {
  SSKD_REQUIRE(n_rows >= 0 && row0 >= 0, "index_get_rows: negative range");
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_rows && d_tiled, "index_get_rows: null pointer");
  const int64_t total = n_rows * CHUNKS;
  int64_t blocks = sskd::ceil_div(total, 256);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(index_get_rows_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     sskd::as_stream(stream), reinterpret_cast<const float4*>(d_tiled), row0,
                     n_rows, reinterpret_cast<float4*>(d_rows));
  return sskd::check_launch("index_get_rows_kernel");
}

int sskd_l2_normalize_rows(float* d_x, int64_t n_rows, int dim, void* stream) {
  SSKD_REQUIRE(n_rows >= 0 && dim > 0, "l2_normalize_rows: bad shape");
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_x, "l2_normalize_rows: null pointer");
  hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((unsigned)sskd::ceil_div(n_rows, 4)),
                     dim3(256), 0, sskd::as_stream(stream), d_x, n_rows, dim);
  return sskd::check_launch("l2_normalize_rows_kernel");
}

}  // extern "C"

// ------------------------------------------------------------------------- //
// row allow-masks (sskd_amd.h): small bandwidth-bound helpers
// ------------------------------------------------------------------------- //
namespace {

// one byte per row -> words: lane l of a wave tests row 64 w + l, one ballot is two words
__global__ __launch_bounds__(256) void row_mask_pack_kernel(const uint8_t* __restrict__ flags, int64_t n_rows,
                                                            uint32_t* __restrict__ mask, int64_t n_words) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t row = w * 64 + lane;
  const unsigned long long b = __ballot(row < n_rows && flags[row] != 0);
  if (lane < 2 && 2 * w + lane < n_words) mask[2 * w + lane] = (uint32_t)(b >> (32 * lane));
}

// set (allow != 0) or clear the bits of a list of rows; rows outside [0, n_rows) are skipped and counted in *bad
__global__ __launch_bounds__(256) void row_mask_update_kernel(uint32_t* __restrict__ mask, int64_t n_rows,
                                                              const int64_t* __restrict__ rows, int64_t n_ids, int allow,
                                                              int* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ids) return;
  const int64_t r = rows[i];
  if (r < 0 || r >= n_rows) {
    atomicAdd(bad, 1);
    return;
  }
  const uint32_t bit = 1u << (r & 31);
  if (allow) atomicOr(mask + (r >> 5), bit);
  else atomicAnd(mask + (r >> 5), ~bit);
}

__global__ __launch_bounds__(256) void row_mask_and_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                           uint32_t* __restrict__ out, int64_t n_words) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_words) out[i] = a[i] & b[i];
}

// one workgroup: popcount of the first n_rows bits (the bits at or past n_rows are ignored); no pre-zeroed output
__global__ __launch_bounds__(1024) void row_mask_count_kernel(const uint32_t* __restrict__ mask, int64_t n_rows,
                                                              int64_t* __restrict__ count) {
  __shared__ unsigned long long part[16];
  const int64_t n_words = (n_rows + 31) >> 5;
  unsigned long long c = 0;
  for (int64_t i = threadIdx.x; i < n_words; i += 1024) {
    uint32_t v = mask[i];
    if (i == n_words - 1 && (n_rows & 31)) v &= (1u << (n_rows & 31)) - 1u;
    c += __popc(v);
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int i = 0; i < 16; ++i) s += part[i];
    *count = (int64_t)s;
  }
}

}  // namespace

extern "C" {

int64_t sskd_row_mask_words(int64_t n_rows) { return n_rows <= 0 ? 0 : sskd::ceil_div(n_rows, 32); }

int sskd_row_mask_pack(const uint8_t* d_flags, int64_t n_rows, uint32_t* d_mask, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "row_mask_pack: n_rows < 0");
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_flags && d_mask, "row_mask_pack: null pointer");
  const int64_t words = sskd_row_mask_words(n_rows);
  hipLaunchKernelGGL(row_mask_pack_kernel, dim3((unsigned)sskd::ceil_div(sskd::ceil_div(words, 2), 4)), dim3(256), 0,
                     sskd::as_stream(stream), d_flags, n_rows, d_mask, words);
  return sskd::check_launch("row_mask_pack_kernel");
}

int sskd_row_mask_update(uint32_t* d_mask, int64_t n_rows, const int64_t* d_rows, int64_t n_ids, int allow,
                         int* d_bad, void* stream) {
  SSKD_REQUIRE(n_rows >= 0 && n_ids >= 0, "row_mask_update: bad shape");
  SSKD_REQUIRE(d_bad, "row_mask_update: null d_bad");
  hipStream_t st = sskd::as_stream(stream);
  if (hipMemsetAsync(d_bad, 0, sizeof(int), st) != hipSuccess) return sskd::fail(SSKD_ERR_HIP, "row_mask_update: memset failed");
  if (n_ids == 0) return SSKD_OK;
  SSKD_REQUIRE(d_mask && d_rows, "row_mask_update: null pointer");
  hipLaunchKernelGGL(row_mask_update_kernel, dim3((unsigned)sskd::ceil_div(n_ids, 256)), dim3(256), 0, st, d_mask, n_rows,
                     d_rows, n_ids, allow, d_bad);
  return sskd::check_launch("row_mask_update_kernel");
}

int sskd_row_mask_and(const uint32_t* d_a, const uint32_t* d_b, int64_t n_rows, uint32_t* d_out, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "row_mask_and: n_rows < 0");
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_a && d_b && d_out, "row_mask_and: null pointer");
  const int64_t words = sskd_row_mask_words(n_rows);
  hipLaunchKernelGGL(row_mask_and_kernel, dim3((unsigned)sskd::ceil_div(words, 256)), dim3(256), 0,
                     sskd::as_stream(stream), d_a, d_b, d_out, words);
  return sskd::check_launch("row_mask_and_kernel");
}

int sskd_row_mask_count(const uint32_t* d_mask, int64_t n_rows, int64_t* d_count, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "row_mask_count: n_rows < 0");
  SSKD_REQUIRE(d_count && (d_mask || n_rows == 0), "row_mask_count: null pointer");
  hipLaunchKernelGGL(row_mask_count_kernel, dim3(1), dim3(1024), 0, sskd::as_stream(stream), d_mask, n_rows, d_count);
  return sskd::check_launch("row_mask_count_kernel");
}

}  // extern "C"

// ------------------------------------------------------------------------- //
// similarity: out[nq, nd] = q d^T, same fma order as the scan
// ------------------------------------------------------------------------- //
namespace {

// one wave per 32 (d rows) x 32 (q rows) output block; generic dim % 8 == 0
__global__ __launch_bounds__(64) void similarity_kernel(const float* __restrict__ q, int nq,
                                                        const float* __restrict__ d, int nd,
                                                        int dim, float* __restrict__ out) {
  const int lane = threadIdx.x;
  const int j = lane & 31, h = lane >> 5;
  const int d0 = blockIdx.x * 32, q0 = blockIdx.y * 32;
  const int drow = min(d0 + j, nd - 1), qrow = min(q0 + j, nq - 1);
  const float4* dp = reinterpret_cast<const float4*>(d + (int64_t)drow * dim) + h;
  const float4* qp = reinterpret_cast<const float4*>(q + (int64_t)qrow * dim) + h;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int u = 0; u < dim / 8; ++u) {
    const float4 a = dp[2 * u], b = qp[2 * u];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
  }
  const int qi = q0 + j;
  if (qi < nq) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int di = d0 + acc_row(r) + 4 * h;
      if (di < nd) out[(int64_t)qi * nd + di] = acc[r];
    }
  }
}

}  // namespace

extern "C" {

int sskd_similarity(const float* d_q, int nq, const float* d_d, int nd, int dim, float* d_out,
                    void* stream) {
  SSKD_REQUIRE(nq >= 0 && nd >= 0 && dim > 0, "similarity: bad shape");
  SSKD_REQUIRE(dim % 8 == 0, "similarity: dim must be a multiple of 8");
  if (nq == 0 || nd == 0) return SSKD_OK;
  SSKD_REQUIRE(d_q && d_d && d_out, "similarity: null pointer");
  hipLaunchKernelGGL(similarity_kernel,
                     dim3((unsigned)sskd::ceil_div(nd, 32), (unsigned)sskd::ceil_div(nq, 32)),
                     dim3(64), 0, sskd::as_stream(stream), d_q, nq, d_d, nd, dim, d_out);
  return sskd::check_launch("similarity_kernel");
}

}  // extern "C"

// ------------------------------------------------------------------------- //
// Compaction (sskd_amd.h): drop the rows a mask clears and renumber the rest.
//
// Step 1 ranks the mask: the exclusive prefix sum of the popcounts of its words, so live row r moves to
// prefix[r >> 5] + popcount(word & ((1u << (r & 31)) - 1)).  Step 2 copies the live rows, out of place, source tile by
// source tile.  A mask word IS a source tile (32 rows each), so a wave needs one word and one prefix entry, and the live
// rows of its tile land on one contiguous run of destination lines.
// ------------------------------------------------------------------------- //
namespace {

constexpr int RANK_THREADS = 1024;
constexpr int RANK_WORDS = 4;  // consecutive words per thread and step: one workgroup ranks 4 096 words per step

// One workgroup walks the whole mask (276 k words at 8.84 M rows: 68 steps), carrying the running count.
__global__ __launch_bounds__(RANK_THREADS) void row_mask_rank_kernel(const uint32_t* __restrict__ mask, int64_t n_rows,
                                                                     int64_t* __restrict__ prefix) {
  __shared__ uint32_t wave_total[RANK_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n_words = (n_rows + 31) >> 5;
  // the bits at or past n_rows are ignored (the index keeps them set)
  const uint32_t last_keep = (n_rows & 31) ? (1u << (n_rows & 31)) - 1u : ~0u;
  int64_t carry = 0;  // set bits in the words before this step
  for (int64_t base = 0; base < n_words; base += (int64_t)RANK_THREADS * RANK_WORDS) {
    const int64_t w0 = base + (int64_t)tid * RANK_WORDS;
    uint32_t c[RANK_WORDS], mine = 0;
#pragma unroll
    for (int j = 0; j < RANK_WORDS; ++j) {
      const int64_t w = w0 + j;
      uint32_t v = w < n_words ? mask[w] : 0u;
      if (w == n_words - 1) v &= last_keep;
      c[j] = __popc(v);
      mine += c[j];
    }
    uint32_t incl = mine;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t below = __shfl_up(incl, o);
      if (lane >= o) incl += below;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < RANK_THREADS / 64; ++i) {
      const uint32_t x = wave_total[i];
      if (i < wave) before += x;
      total += x;
    }
    int64_t p = carry + before + (incl - mine);
#pragma unroll
    for (int j = 0; j < RANK_WORDS; ++j) {
      if (w0 + j < n_words) prefix[w0 + j] = p;
      p += c[j];
    }
    carry += total;
    __syncthreads();  // wave_total is rewritten by the next step
  }
  if (tid == 0) prefix[n_words] = carry;
}

constexpr int COMPACT_WAVES = 4;
constexpr int COMPACT_ROWS = 4;                               // live rows moved per step
constexpr int COMPACT_LOADS = COMPACT_ROWS * CHUNKS / 64;     // 6 wave-wide 16-byte loads in flight, then 6 stores
static_assert(COMPACT_ROWS * CHUNKS % 64 == 0, "a step is a whole number of wave-wide accesses");

// One wave per SOURCE tile t (= mask word t); wave n_tiles zero-fills the tail of the last destination tile.  Everything
// that steers the wave (word, prefix, the rows of a step) is wave-uniform; lanes differ only in the 16-byte chunk they
// move.  The live rows of a tile are consecutive in the destination, so chunk c of a step goes to out + c: a step of four
// rows is 6 KiB of whole 128-byte lines on both sides.
__global__ __launch_bounds__(COMPACT_WAVES * 64) void index_compact_rows_kernel(
    const float4* __restrict__ src, int64_t n_rows, const uint32_t* __restrict__ mask,
    const int64_t* __restrict__ prefix, float4* __restrict__ dst, int64_t n_tiles) {
  const int lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * COMPACT_WAVES + (threadIdx.x >> 6);
  if (t > n_tiles) return;
  if (t == n_tiles) {
    const int64_t n_live = wave_uniform(prefix[n_tiles]);
    const int64_t end = (n_live + TILE_ROWS - 1) / TILE_ROWS * TILE_ROWS * CHUNKS;
    for (int64_t i = n_live * CHUNKS + lane; i < end; i += 64) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  uint32_t word = __builtin_amdgcn_readfirstlane(mask[t]);
  if (t == n_tiles - 1 && (n_rows & 31)) word &= (1u << (n_rows & 31)) - 1u;
  if (word == 0) return;  // a tile without live rows: its rows are never touched
  const float4* in = src + t * (int64_t)(TILE_ROWS * CHUNKS);
  float4* out = dst + wave_uniform(prefix[t]) * CHUNKS;
  while (word) {
    int row[COMPACT_ROWS], n = 0;
#pragma unroll
    for (int j = 0; j < COMPACT_ROWS; ++j) {
      row[j] = 0;
      if (word) {
        row[j] = __ffs((int)word) - 1;
        word &= word - 1;
        ++n;
      }
    }
    const int total = n * CHUNKS;
    float4 v[COMPACT_LOADS];
#pragma unroll
    for (int i = 0; i < COMPACT_LOADS; ++i) {
      const int c = i * 64 + lane;
      const int which = c / CHUNKS;
      int r = row[0];
#pragma unroll
      for (int j = 1; j < COMPACT_ROWS; ++j) r = which == j ? row[j] : r;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < total) x = in[r * CHUNKS + (c - which * CHUNKS)];
      v[i] = x;
    }
#pragma unroll
    for (int i = 0; i < COMPACT_LOADS; ++i) {
      const int c = i * 64 + lane;
      if (c < total) out[c] = v[i];
    }
    out += total;
  }
}

}  // namespace

extern "C" {

int sskd_row_mask_rank(const uint32_t* d_mask, int64_t n_rows, int64_t* d_word_prefix, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "row_mask_rank: n_rows < 0");
  const int rc = require_shard_rows("row_mask_rank", n_rows);
  if (rc != SSKD_OK) return rc;
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_mask && d_word_prefix, "row_mask_rank: null pointer");
  hipLaunchKernelGGL(row_mask_rank_kernel, dim3(1), dim3(RANK_THREADS), 0, sskd::as_stream(stream), d_mask, n_rows,
                     d_word_prefix);
  return sskd::check_launch("row_mask_rank_kernel");
}

int sskd_index_compact_rows(const float* d_src_tiled, int64_t n_rows, const uint32_t* d_mask,
                            const int64_t* d_word_prefix, float* d_dst_tiled, void* stream) {
  SSKD_REQUIRE(n_rows >= 0, "index_compact_rows: n_rows < 0");
  const int rc = require_shard_rows("index_compact_rows", n_rows);
  if (rc != SSKD_OK) return rc;
  if (n_rows == 0) return SSKD_OK;
  SSKD_REQUIRE(d_src_tiled && d_mask && d_word_prefix && d_dst_tiled, "index_compact_rows: null pointer");
  // out of place.  The live count is on the device, so the host knows the source's extent but of the destination's
  // only that it is at least one tile (unless nothing is live): a destination that starts inside the source, or a
  // source that starts inside the destination's first tile, is refused.  A destination placed BELOW the source must
  // end (padded_rows(n_live) rows) before the source begins: that is the caller's to guarantee.
  const uintptr_t s = reinterpret_cast<uintptr_t>(d_src_tiled), d = reinterpret_cast<uintptr_t>(d_dst_tiled);
  const uintptr_t src_bytes = sskd_index_tiled_bytes(n_rows), tile_bytes = (uintptr_t)TILE_FLOATS * sizeof(float);
  SSKD_REQUIRE(!(d >= s && d < s + src_bytes) && !(s >= d && s < d + tile_bytes),
               "index_compact_rows: source and destination overlap");
  const int64_t n_tiles = sskd::ceil_div(n_rows, TILE_ROWS);
  hipLaunchKernelGGL(index_compact_rows_kernel, dim3((unsigned)sskd::ceil_div(n_tiles + 1, COMPACT_WAVES)),
                     dim3(COMPACT_WAVES * 64), 0, sskd::as_stream(stream), reinterpret_cast<const float4*>(d_src_tiled),
                     n_rows, d_mask, d_word_prefix, reinterpret_cast<float4*>(d_dst_tiled), n_tiles);
  return sskd::check_launch("index_compact_rows_kernel");
}

}  // extern "C"
