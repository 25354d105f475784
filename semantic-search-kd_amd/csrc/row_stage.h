// The "exact scores" stage of the approximate indexes (internal: not installed): ivf_scan_kernel, pq_refine_kernel and
// graph_search_kernel gather candidate rows through LDS in chunks of 32 and score them with the exact scan's fma chain.
//   all      load a chunk's rows into registers - thread t takes float4 t, t + 256, ... of the 32 x 96, so every
//            row is read as 1 536 contiguous bytes (whole 128-byte lines), never 16 bytes at a 1 536-byte stride -
//   all      registers -> LDS
//   wave 0   scores the chunk out of LDS, one lane per row (row_score_fma: the bits the exact search returns).
// The LDS row stride is 97 float4 (1 552 B): lane l starts at bank 4 l mod 64, and every 16-lane group of a
// ds_read_b128 ({0-3, 12-15, 20-27}, ...) covers the 16 slots of the 256-byte bank row exactly once - conflict-free.
// Each kernel keeps its own chunk loop and barrier schedule (what happens between the barriers differs); a barrier
// stands between store() and stage_score(), and between stage_score() and the next store().
#pragma once
#include "search_device.h"

namespace {

constexpr int STAGE_THREADS = 256;                                   // the workgroup that stages
constexpr int STAGE_ROWS = 32;                                       // rows per chunk
constexpr int STAGE_STRIDE4 = CHUNKS + 1;                            // LDS row stride in float4 (97: see above)
constexpr int STAGE_LOADS = STAGE_ROWS * CHUNKS / STAGE_THREADS;     // 12 float4 per thread and chunk
constexpr int STAGE_FLOAT4 = STAGE_ROWS * STAGE_STRIDE4;             // the staging area: 49 664 B
static_assert(STAGE_ROWS * CHUNKS % STAGE_THREADS == 0, "a chunk is a whole number of float4 per thread");

// one thread's share of a chunk on its way from the index to LDS
struct RowStage {
  float4 regs[STAGE_LOADS];

  // row_of(i) = the index row that becomes row i of the chunk, negative for none (the row is staged as zeros)
  template <typename RowOf>
  __device__ __forceinline__ void load(const float4* __restrict__ rows4, int tid, RowOf row_of) {
#pragma unroll
    for (int i = 0; i < STAGE_LOADS; ++i) {
      const int f = tid + STAGE_THREADS * i, row = f / CHUNKS, c = f - row * CHUNKS;
      const int r = row_of(row);
      regs[i] = r >= 0 ? rows4[(int64_t)r * CHUNKS + c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  // rows_s = the staging area, STAGE_FLOAT4 float4 of LDS
  __device__ __forceinline__ void store(float4* rows_s, int tid) const {
#pragma unroll
    for (int i = 0; i < STAGE_LOADS; ++i) {
      const int f = tid + STAGE_THREADS * i, row = f / CHUNKS, c = f - row * CHUNKS;
      rows_s[row * STAGE_STRIDE4 + c] = regs[i];
    }
  }
};

// score of row `lane` (< STAGE_ROWS) of the staged chunk against the query in LDS
__device__ __forceinline__ float stage_score(const float4* rows_s, int lane, const float4* q_s) {
  return row_score_fma(&rows_s[lane * STAGE_STRIDE4], reinterpret_cast<const float*>(q_s));
}

}  // namespace
