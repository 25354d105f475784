// Diversified search: Maximal Marginal Relevance over a first stage's candidates (sskd_amd.h "Diversified search";
// DESIGN.md 27).
//
// One workgroup of 256 threads per query, the candidate list (at most 1 024 rows) in LDS.  The work is lazy: a selection
// costs the similarities of the selected row to the candidates that are still alive, never a Gram matrix.
//   compact   wave 0 walks the ranking, 64 entries per round (the common walk of ranking_walk.h):
//             row, relevance and an alive bitmap (one word per 32 candidates) in list order
//   argmax    every thread values its candidates in fp64, every operation rounded once (this translation unit is compiled
//             without contraction); the pair (value, position) is reduced over the wave, then over the four waves
//   pass      the selected row becomes the "query" in LDS; the alive candidates come through the row stage of the
//             approximate indexes, one 32-candidate bitmap word per chunk, the next chunk's loads in flight while wave 0
//             scores the current one (row_score_fma: the exact scan's bits); wave 0 raises red, kills what reaches the
//             threshold and rewrites the word.  A chunk without an alive candidate is skipped, and a chunk that is
//             already staged is not loaded again: with at most 32 candidates the rows are read from HBM once.
// The pass after the last selection is not made, and nothing is done once nobody is alive.
//
// Two kernels share the walk, the argmax and the output code:
//   mmr_resident_kernel<R>  fetch_k <= R (R = 50, 100): ALL candidate rows are copied into LDS once (R x 1 552 B), the
//                           selected row becomes the query by an LDS copy, and a pass is one chain per candidate, one
//                           lane each, on waves 0 and 1 - no row is read from HBM twice.  R = 50 is 80 KiB (two
//                           workgroups per CU), R = 100 is 155 KiB (one).
//   mmr_select_kernel       any fetch_k: the 32-row stage described above, 62 KiB.
#include "ranking_walk.h"
#include "row_stage.h"
#include "search_host.h"

#include <cfloat>

#pragma clang fp contract(off)

namespace {

constexpr int MMR_THREADS = STAGE_THREADS;
constexpr int MMR_WAVES = MMR_THREADS / 64;
constexpr int MMR_CAND_MAX = SSKD_K_MAX;                       // fetch_k at most
constexpr int MMR_WORDS = MMR_CAND_MAX / STAGE_ROWS;           // bitmap words = chunks at most
static_assert(STAGE_ROWS == 32, "one bitmap word per staged chunk");
static_assert(MMR_CAND_MAX % STAGE_ROWS == 0, "whole bitmap words");

struct MmrParams {
  const float* rows;            // the index: row-major fp32 [n_rows][DIM]
  const float* rank_scores;     // [nq][fetch_k]
  const int64_t* rank_ids;      // local rows, -1 padded
  int64_t n_rows;
  int64_t id_offset;
  double a, b;                  // lambda, 1.0 - lambda
  float dup_threshold;
  int fetch_k, k;
  float* out_scores;            // [nq][k]
  int64_t* out_ids;
  double* out_mmr;              // [nq][k] or null
  float* out_red;               // [nq][k] or null
  int32_t* out_counts;          // [nq]
};

// (value, position) of the better candidate: the larger value, then the earlier position; position < 0 = none
__device__ inline void take_better(double& v, int& p, double ov, int op) {
  if (op >= 0 && (p < 0 || ov > v || (ov == v && op < p))) { v = ov; p = op; }
}

// the candidates of query q in list order into c_row / c_s (wave 0 alone, 64 entries per round); returns how many
__device__ inline int compact_candidates(const MmrParams& p, int q, int32_t* c_row, float* c_s, int lane) {
  const float* rs = p.rank_scores + (int64_t)q * p.fetch_k;
  const int64_t* ri = p.rank_ids + (int64_t)q * p.fetch_k;
  int m = 0;            // (wave-uniform) candidates so far
  bool ended = false;   // an id -1 was met: nothing behind it counts
  for (int base = 0; base < p.fetch_k && !ended; base += 64) {
    const int at = base + lane;
    const bool inside = at < p.fetch_k;
    const int64_t row = inside ? ri[at] : -1;
    const bool cand = walk_step(inside, row, p.n_rows, lane, ended);
    const int pos = walk_pack(cand, lane, m);   // < fetch_k
    if (cand) {
      c_row[pos] = (int32_t)row;
      c_s[pos] = rs[at];
    }
  }
  return m;
}

// bitmap word w of m candidates that are all alive
__device__ inline uint32_t full_word(int m, int w) {
  const int left = m - w * STAGE_ROWS;
  return left >= STAGE_ROWS ? 0xFFFFFFFFu : left > 0 ? (1u << left) - 1u : 0u;
}

// The alive candidate with the largest value, ties to the earlier position: (value, position) for every thread of the
// workgroup, position < 0 when nobody is alive.  One barrier inside; best_v / best_p are MMR_WAVES slots of LDS.
// `first`: no pass has been made, red is unset and counts as +0.0.
__device__ inline void argmax_alive(const MmrParams& p, int m, bool first, const uint32_t* alive_w, const float* c_s,
                                    const float* c_red, double* best_v, int* best_p, double& bv, int& bp) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bv = 0.0;
  bp = -1;
  for (int i = tid; i < m; i += MMR_THREADS) {
    if (((alive_w[i >> 5] >> (i & 31)) & 1u) == 0u) continue;
    const double r = first ? 0.0 : (double)c_red[i];
    const double rel = p.a * (double)c_s[i];
    const double pen = p.b * r;
    const double v = rel - pen;
    if (bp < 0 || v > bv) { bv = v; bp = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int op = __shfl_xor(bp, o);
    take_better(bv, bp, ov, op);
  }
  if (lane == 0) {
    best_v[wave] = bv;
    best_p[wave] = bp;
  }
  __syncthreads();
  bv = best_v[0];
  bp = best_p[0];
#pragma unroll
  for (int w = 1; w < MMR_WAVES; ++w) take_better(bv, bp, best_v[w], best_p[w]);
}

// one thread writes selection `count`: candidate bp with value bv
__device__ inline void write_selection(const MmrParams& p, int q, int count, int bp, double bv, bool first,
                                       const int32_t* c_row, const float* c_s, const float* c_red) {
  const int64_t o = (int64_t)q * p.k + count;
  p.out_scores[o] = c_s[bp];
  p.out_ids[o] = (int64_t)c_row[bp] + p.id_offset;
  if (p.out_mmr) p.out_mmr[o] = bv;
  if (p.out_red) p.out_red[o] = first ? 0.f : c_red[bp];
}

// the tail behind `count` selections and the count itself (the whole workgroup)
__device__ inline void write_padding(const MmrParams& p, int q, int count) {
  const int64_t o = (int64_t)q * p.k;
  for (int i = count + threadIdx.x; i < p.k; i += MMR_THREADS) {
    p.out_scores[o + i] = -FLT_MAX;
    p.out_ids[o + i] = -1;
    if (p.out_mmr) p.out_mmr[o + i] = -INFINITY;
    if (p.out_red) p.out_red[o + i] = __builtin_nanf("");
  }
  if (threadIdx.x == 0) p.out_counts[q] = count;
}

// ------------------------------------------------------------------------------------------------ rows resident
constexpr int MMR_RES_WORDS = 4;   // 128 candidates at most
template <int R>
constexpr size_t resident_lds_bytes() {
  return (size_t)R * STAGE_STRIDE4 * sizeof(float4) + CHUNKS * sizeof(float4) + 3 * R * 4 + MMR_RES_WORDS * 4 +
         MMR_WAVES * 12 + 4;
}

template <int R>
__global__ __launch_bounds__(MMR_THREADS) void mmr_resident_kernel(MmrParams p) {
  static_assert(R <= MMR_RES_WORDS * 32 && R <= 2 * 64, "a pass is one lane per candidate on waves 0 and 1");
  static_assert(resident_lds_bytes<R>() <= 160 * 1024, "a CU has 160 KiB of LDS");
  __shared__ float4 rows_s[R * STAGE_STRIDE4];   // every candidate's row, at the stage's conflict-free stride
  __shared__ float4 q_s[CHUNKS];                 // the selected row
  __shared__ int32_t c_row[R];
  __shared__ float c_s[R];
  __shared__ float c_red[R];
  __shared__ uint32_t alive_w[MMR_RES_WORDS];
  __shared__ double best_v[MMR_WAVES];
  __shared__ int best_p[MMR_WAVES];
  __shared__ int m_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;

  if (wave == 0) {
    const int found = compact_candidates(p, q, c_row, c_s, lane);   // <= fetch_k <= R: the host chose R
    if (lane == 0) m_s = found;
  }
  __syncthreads();
  const int m = m_s;
  if (tid < MMR_RES_WORDS) alive_w[tid] = full_word(m, tid);
  // every row once: float4 f of the m x 96, whole rows in consecutive threads
  const float4* rows4 = reinterpret_cast<const float4*>(p.rows);
#pragma unroll 4
  for (int f = tid; f < m * CHUNKS; f += MMR_THREADS) {
    const int row = f / CHUNKS, c = f - row * CHUNKS;
    rows_s[row * STAGE_STRIDE4 + c] = rows4[(int64_t)c_row[row] * CHUNKS + c];
  }
  __syncthreads();

  auto anyone_alive = [&] { return (alive_w[0] | alive_w[1] | alive_w[2] | alive_w[3]) != 0u; };
  int count = 0;
  while (count < p.k && anyone_alive()) {   // every bound is workgroup-uniform
    const bool first = count == 0;
    double bv;
    int bp;
    argmax_alive(p, m, first, alive_w, c_s, c_red, best_v, best_p, bv, bp);
    if (bp < 0) break;   // (cannot happen while somebody is alive)
    if (tid == 0) {
      write_selection(p, q, count, bp, bv, first, c_row, c_s, c_red);
      alive_w[bp >> 5] &= ~(1u << (bp & 31));
    }
    ++count;
    if (count == p.k) break;
    if (tid < CHUNKS) q_s[tid] = rows_s[bp * STAGE_STRIDE4 + tid];
    __syncthreads();
    if (!anyone_alive()) break;
    // ---- pass: one lane per candidate
    if (wave < 2) {
      const unsigned long long word = (unsigned long long)alive_w[2 * wave] | ((unsigned long long)alive_w[2 * wave + 1] << 32);
      const bool live = (word >> lane) & 1ull;   // (a set bit is a position < m)
      bool stay = live;
      if (live) {
        const float sim = stage_score(rows_s, tid, q_s);
        float r = c_red[tid];
        if (first || sim > r) r = sim;
        c_red[tid] = r;
        if (r >= p.dup_threshold) stay = false;
      }
      const unsigned long long keep = __ballot(stay);
      if (lane == 0) {
        alive_w[2 * wave] = (uint32_t)keep;
        alive_w[2 * wave + 1] = (uint32_t)(keep >> 32);
      }
    }
    __syncthreads();
  }
  write_padding(p, q, count);
}

// ------------------------------------------------------------------------------------------------ rows staged
__global__ __launch_bounds__(MMR_THREADS) void mmr_select_kernel(MmrParams p) {
  __shared__ float4 rows_s[STAGE_FLOAT4];   // the staged chunk
  __shared__ float4 q_s[CHUNKS];            // the selected row
  __shared__ int32_t c_row[MMR_CAND_MAX];
  __shared__ float c_s[MMR_CAND_MAX];
  __shared__ float c_red[MMR_CAND_MAX];     // set for every alive candidate from the first pass on
  __shared__ uint32_t alive_w[MMR_WORDS];   // bit j of word c: candidate 32 c + j is alive
  __shared__ double best_v[MMR_WAVES];
  __shared__ int best_p[MMR_WAVES];
  __shared__ int m_s, n_alive_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = blockIdx.x;
  const int k = p.k;

  // ---- compact: the candidates in list order
  if (wave == 0) {
    const int found = compact_candidates(p, q, c_row, c_s, lane);   // <= fetch_k <= MMR_CAND_MAX
    if (lane == 0) {
      m_s = found;
      n_alive_s = found;
    }
  }
  __syncthreads();
  const int m = m_s;
  const int n_chunks = (m + STAGE_ROWS - 1) / STAGE_ROWS;
  if (tid < MMR_WORDS) alive_w[tid] = full_word(m, tid);
  __syncthreads();

  const float4* rows4 = reinterpret_cast<const float4*>(p.rows);

  RowStage stage;
  auto load_chunk = [&](int c) {
    const uint32_t word = alive_w[c];
    stage.load(rows4, tid, [&](int row) { return ((word >> row) & 1u) ? c_row[c * STAGE_ROWS + row] : -1; });
  };
  // the first chunk from `from` on that holds an alive candidate, n_chunks for none (workgroup-uniform)
  auto next_chunk = [&](int from) {
    int c = from;
    while (c < n_chunks && alive_w[c] == 0u) ++c;
    return c;
  };

  int staged = -1;   // (uniform) the chunk whose rows rows_s holds: a superset of its alive rows, the alive only shrink
  int count = 0;
  for (; count < k; ++count) {   // every bound below is workgroup-uniform
    if (n_alive_s <= 0) break;
    const bool first = count == 0;   // no pass has been made: red is unset and counts as +0.0

    double bv;
    int bp;
    argmax_alive(p, m, first, alive_w, c_s, c_red, best_v, best_p, bv, bp);
    if (bp < 0) break;   // (cannot happen while somebody is alive)

    // ---- the selection leaves the alive set and is written
    const int32_t prow = c_row[bp];
    if (tid == 0) {
      write_selection(p, q, count, bp, bv, first, c_row, c_s, c_red);
      alive_w[bp >> 5] &= ~(1u << (bp & 31));
      n_alive_s -= 1;
    }
    const bool last = count + 1 == k;
    if (!last && tid < CHUNKS) q_s[tid] = rows4[(int64_t)prow * CHUNKS + tid];
    __syncthreads();
    if (last || n_alive_s <= 0) {
      ++count;
      break;
    }

    // ---- pass: sim(i, selected) for every alive i, red and the bitmap updated
    int c = next_chunk(0);   // (< n_chunks: somebody is alive)
    if (staged != c) {
      load_chunk(c);
      stage.store(rows_s, tid);   // (its last readers left before the barrier that ended the pass before)
      staged = c;
    }
    __syncthreads();
    while (c < n_chunks) {
      const int nx = next_chunk(c + 1);   // (words behind c: wave 0 rewrites word c alone)
      const bool more = nx < n_chunks;
      if (more) load_chunk(nx);   // in flight while wave 0 scores
      if (wave == 0) {
        const uint32_t word = alive_w[c];
        const int pos = c * STAGE_ROWS + lane;
        const bool live = lane < STAGE_ROWS && ((word >> (lane & 31)) & 1u);
        bool stay = live;
        if (live) {
          const float sim = stage_score(rows_s, lane, q_s);
          float r = c_red[pos];
          if (first || sim > r) r = sim;
          c_red[pos] = r;
          if (r >= p.dup_threshold) stay = false;
        }
        const uint32_t keep = (uint32_t)__ballot(stay);
        if (lane == 0) {
          alive_w[c] = keep;
          n_alive_s -= __popc(word) - __popc(keep);
        }
      }
      __syncthreads();   // the chunk has been read; red, the word and the alive count are written
      if (more) {
        stage.store(rows_s, tid);
        staged = nx;
        __syncthreads();
      }
      c = nx;
    }
  }

  write_padding(p, q, count);
}

constexpr int MMR_RESIDENT_SMALL = 50, MMR_RESIDENT_LARGE = 100;   // the two resident sizes: the host layer's default and twice it

}  // namespace

extern "C" {

int sskd_mmr_select(const float* d_tiled, int64_t n_rows, const float* d_rank_scores, const int64_t* d_rank_ids, int nq,
                    int fetch_k, double lambda, float dup_threshold, int k, int64_t id_offset, float* d_out_scores,
                    int64_t* d_out_ids, double* d_out_mmr, float* d_out_red, int32_t* d_out_counts, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(n_rows >= 0, "mmr_select: n_rows < 0");
  SSKD_REQUIRE(n_rows < sskd::MAX_SHARD_ROWS, "mmr_select: n_rows too large for int32 row ids");
  SSKD_REQUIRE(nq >= 0, "mmr_select: nq < 0");
  SSKD_REQUIRE(fetch_k >= 1 && fetch_k <= SSKD_K_MAX, "mmr_select: fetch_k=%d outside [1, %d]", fetch_k, SSKD_K_MAX);
  SSKD_REQUIRE(k >= 1 && k <= fetch_k, "mmr_select: k=%d outside [1, fetch_k = %d]", k, fetch_k);
  SSKD_REQUIRE(lambda >= 0.0 && lambda <= 1.0, "mmr_select: lambda must be finite and in [0, 1]");
  SSKD_REQUIRE(dup_threshold == dup_threshold, "mmr_select: dup_threshold is NaN");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_rank_scores && d_rank_ids, "mmr_select: null ranking");
  SSKD_REQUIRE(d_out_scores && d_out_ids && d_out_counts, "mmr_select: null output");
  SSKD_REQUIRE(n_rows == 0 || d_tiled, "mmr_select: null index");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_tiled) % 16 == 0, "mmr_select: d_tiled must be 16-byte aligned");
  MmrParams p{};
  p.rows = d_tiled;
  p.rank_scores = d_rank_scores;
  p.rank_ids = d_rank_ids;
  p.n_rows = n_rows;
  p.id_offset = id_offset;
  p.a = lambda;
  p.b = 1.0 - lambda;
  p.dup_threshold = dup_threshold;
  p.fetch_k = fetch_k;
  p.k = k;
  p.out_scores = d_out_scores;
  p.out_ids = d_out_ids;
  p.out_mmr = d_out_mmr;
  p.out_red = d_out_red;
  p.out_counts = d_out_counts;
  // m <= fetch_k: a list that fits is served with every row resident, anything longer through the 32-row stage
  const dim3 grid((unsigned)nq), block(MMR_THREADS);
  hipStream_t st = sskd::as_stream(stream);
  if (fetch_k <= MMR_RESIDENT_SMALL) {
    hipLaunchKernelGGL(mmr_resident_kernel<MMR_RESIDENT_SMALL>, grid, block, 0, st, p);
  } else if (fetch_k <= MMR_RESIDENT_LARGE) {
    hipLaunchKernelGGL(mmr_resident_kernel<MMR_RESIDENT_LARGE>, grid, block, 0, st, p);
  } else {
    hipLaunchKernelGGL(mmr_select_kernel, grid, block, 0, st, p);
  }
  return sskd::check_launch("mmr_select");
}

}  // extern "C"
