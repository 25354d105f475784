// The MaxSim tile engine and the helpers that more than one late-interaction unit uses (internal: not installed):
// late.hip (token store, re-rank, compressed store), late_train.hip (gradients) and plaid.hip (candidate generation).
// What only one of them uses stays there.
//
// score(q, c) = sum over the query's tokens i of max over the document's tokens j of <q_i, d_j>, on L2-normalised bf16
// token rows of 384 columns.  The dot products run on v_mfma_f32_32x32x16_bf16 with the DOCUMENT tokens as the A operand
// and the QUERY tokens as B: both operands of that instruction are K-contiguous (lane l holds row l & 31, columns
// 8 (l >> 5) .. + 7 of a k-step), so row-major token rows feed it with 16-byte reads and no transpose, and the result
// tile has the query token on the lane and 32 document tokens in 16 registers x 2 lane halves - the max over document
// tokens is a max over the lane's registers and one exchange with lane l ^ 32.
//
// Geometry.  A workgroup of 4 waves serves one (query, chunk of candidates): the query's tokens are staged once in LDS in
// B-fragment order (24 KiB per block of 32 tokens, at most 4 blocks), wave w takes candidates w, w + 4, ... of the chunk
// whole.  A document tile (32 consecutive token rows = 24 KiB contiguous in the store) is read by ONE burst of 24 16-byte
// loads per lane - every byte of every 128-byte line of the tile is requested before the first MFMA waits - and then
// multiplied against every block of the query.  One wave alone computes a candidate, in an order fixed by (Tq, Td), so a
// score's bits depend on nothing but the two token lists.  Element (d_j, q_i) is the chain of 24 MFMAs over those two
// rows alone: its bits do not depend on what else the tile or the batch holds.
#pragma once
#include <cfloat>
#include <cmath>

#include "search_device.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int L_WAVES = 4;
constexpr int L_THREADS = L_WAVES * 64;
constexpr int L_KSTEPS = DIM / 16;          // 24 k-steps of v_mfma_f32_32x32x16_bf16
constexpr int L_ROW_VEC = DIM / 8;          // 48 16-byte vectors per bf16 token row
constexpr int L_TQ_MAX = SSKD_LATE_TQ_MAX;  // 128
constexpr int L_R_MAX = SSKD_LATE_R_MAX;    // 1024
constexpr int L_C_MAX = SSKD_LATE_C_MAX;    // 65 536

// ------------------------------------------------------------------------------------------------ bf16
// 8 bf16 of a 16-byte vector, widened to fp32 (exact)
__device__ inline void widen8(const uint4& v, float (&x)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[2 * j] = __uint_as_float(w[j] << 16);
    x[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
  }
}

__device__ inline uint32_t bf16_rn_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;   // round to nearest even (finite input)
}

// 8 fp32 rounded to bf16 (nearest even), as a 16-byte vector
__device__ inline uint4 pack8(const float (&x)[8]) {
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = bf16_rn_bits(x[2 * j]) | (bf16_rn_bits(x[2 * j + 1]) << 16);
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// Sum of squares of a 384-column row held one 16-byte piece per lane (lane l < 48: columns 8 l .. 8 l + 7; `holds` is
// false for lanes 48 .. 63, whose x is not read).  THE order (tests/late_cases.py sum_squares_rows restates it):
//   p_l = fma chain from +0.0f over the lane's 8 columns ascending (a bf16 square is exact in fp32, so the fma equals
//         add(p, x * x));  p_l = +0.0f for lanes 48 .. 63;
//   butterfly: for o = 32, 16, 8, 4, 2, 1: p_l = p_l + p_(l ^ o)   (fp32 addition commutes, so every lane holds the same bits).
__device__ inline float row_sum_squares(const float (&x)[8], bool holds) {
  float p = 0.f;
  if (holds) {
#pragma unroll
    for (int j = 0; j < 8; ++j) p = fmaf(x[j], x[j], p);
  }
  return wave_sum(p);
}

// ------------------------------------------------------------------------------------------------ query range
// the token range of query q as the device reads it: an impossible range is empty (the host validated its copy of the lims)
__device__ inline void query_range(const int64_t* q_lims, int64_t n_q_tokens, int q, int64_t& q0, int64_t& tq) {
  q0 = q_lims[q];
  tq = q_lims[q + 1] - q0;
  if (q0 < 0 || tq < 0 || q0 + tq > n_q_tokens) { q0 = 0; tq = 0; }
}

// ------------------------------------------------------------------------------------------------ tile engine
// B fragments of up to QB blocks of 32 query tokens in LDS: [block][k-step][lane]
template <int QB>
using QueryFragments = bf16x8[QB][L_KSTEPS][64];

// stage (all L_THREADS threads; a barrier follows): token row i of the Tq rows from q0, 16-byte vector ch = 2 s + half
// -> qs[i >> 5][s][32 half + (i & 31)]; the rows from Tq to the end of the last block in use are zeros
template <int QB>
__device__ __forceinline__ void stage_query(QueryFragments<QB>& qs, const bf16x8* q_tokens, int64_t q0, int Tq) {
  const int nb = (Tq + 31) >> 5;
  for (int idx = threadIdx.x; idx < nb * 32 * L_ROW_VEC; idx += L_THREADS) {
    const int i = idx / L_ROW_VEC, ch = idx % L_ROW_VEC;
    bf16x8 v = __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
    if (i < Tq) v = q_tokens[(q0 + i) * L_ROW_VEC + ch];
    qs[i >> 5][ch >> 1][((ch & 1) << 5) | (i & 31)] = v;
  }
}

// the A fragments of the lane's row of a tile: one burst of 24 16-byte loads; src = the row's vectors + (lane >> 5)
__device__ __forceinline__ void load_row_fragments(bf16x8 (&a)[L_KSTEPS], const bf16x8* src) {
#pragma unroll
  for (int s = 0; s < L_KSTEPS; ++s) a[s] = src[2 * s];
}

// 32 rows x 32 query tokens: register r of lane l = row acc_row(r) + 4 (l >> 5) of the tile, query token l & 31 of the block
__device__ __forceinline__ f32x16 tile_product(const bf16x8 (&a)[L_KSTEPS], const bf16x8 (&qb)[L_KSTEPS][64], int lane) {
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int s = 0; s < L_KSTEPS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], qb[s][lane], acc, 0, 0, 0);
  return acc;
}

// ------------------------------------------------------------------------------------------------ MaxSim
// the token range of candidate id (global), or an empty range when there is no such candidate
template <class P>
__device__ inline void cand_range(const P& p, int64_t id, int64_t& beg, int64_t& td) {
  beg = 0; td = 0;
  const int64_t row = id - p.id_offset;
  if (id < 0 || row < 0 || row >= p.n_rows) return;
  const int64_t lo = p.tok_lims[row], hi = p.tok_lims[row + 1];
  if (lo < 0 || hi > p.n_tokens || hi <= lo) return;
  beg = lo; td = hi - lo;
}

// The body of the score kernels: grid (query, chunk of candidates), L_THREADS threads.  P has q_tokens, q_lims,
// n_q_tokens, tok_lims, n_tokens, n_rows, id_offset, cand, raw, R, chunk (and arg, tq_stride when ARG).  A Source is a
// token store format, it says where the 24 A fragments of a tile come from:
//   begin(beg, td, r32)              once per candidate
//   load(a, beg, t0, td, r32, h)     the lane's row of tile t0; rows past the end re-read the last real row (masked here)
// QB = blocks of 32 query tokens the workgroup holds in LDS (the batch's largest query decides; a shorter query uses
// its own ceil(Tq / 32) blocks of them, so its scores do not depend on QB).
// ARG (sskd_latet_maxsim_fwd): also report, per query token, the document-relative index of the token that holds the max -
// the smallest such index.  The values and every operation on them are those of ARG = false (the index is found by
// comparing against the tile's max AFTER it has been formed), so the score's bits are the re-rank's.
template <int QB, bool ARG, class P, class Source>
__device__ __forceinline__ void maxsim_body(const P& p, Source& src, QueryFragments<QB>& qs) {
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  int64_t q0, tq64;
  query_range(p.q_lims, p.n_q_tokens, q, q0, tq64);
  const int Tq = (int)(tq64 < QB * 32 ? tq64 : QB * 32);
  const int nb = (Tq + 31) >> 5;            // blocks in use (workgroup-uniform)
  stage_query<QB>(qs, p.q_tokens, q0, Tq);
  __syncthreads();

  const int c_begin = blockIdx.y * p.chunk;
  const int c_end = min(c_begin + p.chunk, p.R);
  for (int c = c_begin + wave; c < c_end; c += L_WAVES) {
    const int64_t id = p.cand[(int64_t)q * p.R + c];
    int64_t beg, td;
    cand_range(p, id, beg, td);
    float score = -INFINITY;                 // no candidate, or a row without tokens: absent
    if (td > 0 && Tq > 0) {
      float best[QB];
      int barg[QB];                            // ARG: document token of best[b], 0 until a tile beats -inf
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        best[b] = -INFINITY;
        barg[b] = 0;
      }
      src.begin(beg, td, r32);
      for (int64_t t0 = 0; t0 < td; t0 += 32) {
        bf16x8 a[L_KSTEPS];
        src.load(a, beg, t0, td, r32, h);
        const bool partial = td - t0 < 32;
        const int left = (int)(td - t0);    // real rows of the tile when partial
#pragma unroll
        for (int b = 0; b < QB; ++b) {
          if (b < nb) {
            f32x16 acc = tile_product(a, qs[b], lane);
            // register r of lane l: document row acc_row(r) + 4 (l >> 5) of the tile, query token 32 b + (l & 31)
            float m = -INFINITY;
            int rows_left = partial ? left : 32;
            // ARG: the 16 row masks are formed again for every block (one compare each) instead of being kept in 32
            // scalar registers across the block loop, which this variant does not have to spare
            if (ARG) asm volatile("" : "+v"(rows_left));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const bool real = ARG ? acc_row(r) + 4 * h < rows_left : !partial || acc_row(r) + 4 * h < left;
              const float v = real ? acc[r] : -INFINITY;
              if (ARG) acc[r] = v;             // (the masked value is what the index search below compares)
              m = fmaxf(m, v);
            }
            m = fmaxf(m, __shfl_xor(m, 32));
            if (ARG) {
              // first row of the tile that equals the tile's max: the lane's own rows ascend with r, the partner
              // half's interleave with them; an earlier tile keeps a tie (strict >, which a tile of -inf never passes)
              int first = 32;
#pragma unroll
              for (int r = 0; r < 16; ++r) first = min(first, acc[r] == m ? acc_row(r) + 4 * h : 32);
              first = min(first, __shfl_xor(first, 32));
              if (m > best[b] && first < 32) barg[b] = (int)t0 + first;
            }
            best[b] = fmaxf(best[b], m);
          }
        }
      }
      // sequential fp32 sum from +0.0f over the query tokens in ascending order (every lane computes the same chain)
      score = 0.f;
#pragma unroll
      for (int b = 0; b < QB; ++b) {
        if (b < nb) {
          const int n = min(32, Tq - 32 * b);
          for (int i = 0; i < n; ++i) score += __shfl(best[b], i);
        }
      }
      if constexpr (ARG) {   // tq_stride == 32 QB (the host checked): the QB blocks cover a pair's whole row of arg
        int32_t* out = p.arg + ((int64_t)q * p.R + c) * (32 * QB) + r32;
#pragma unroll
        for (int b = 0; b < QB; ++b)
          if (h == 0) out[32 * b] = 32 * b + r32 < Tq ? barg[b] : -1;
      }
    } else if constexpr (ARG) {
      for (int i = lane; i < p.tq_stride; i += 64) p.arg[((int64_t)q * p.R + c) * p.tq_stride + i] = -1;
    }
    if (lane == 0) p.raw[(int64_t)q * p.R + c] = score;
  }
}

// ------------------------------------------------------------------------------------------------ host
bool aligned16(const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; }

// The host copy of the query bounds, checked before anything is enqueued: returns the largest Tq, or -1 after recording
// the error under the entry point's name.  The re-rank and candidate paths take any ascending bounds from q_lims[0] >= 0;
// the training entry points pass n_q_tokens >= 0 and tq_stride: their bounds run from 0 to n_q_tokens, and tq_stride is
// the largest Tq rounded up to 32.
int check_query_lims(const char* what, const int64_t* q_lims, int nq, int64_t n_q_tokens = -1, int tq_stride = 0) {
  const bool training = n_q_tokens >= 0;
  if (!q_lims) return sskd::fail(SSKD_ERR_INVALID, "%s: the host copy of q_lims is required", what), -1;
  if (training && (q_lims[0] != 0 || q_lims[nq] != n_q_tokens))
    return sskd::fail(SSKD_ERR_INVALID, "%s: q_lims runs from %lld to %lld, there are %lld query token rows", what,
                      (long long)q_lims[0], (long long)q_lims[nq], (long long)n_q_tokens), -1;
  if (!training && q_lims[0] < 0) return sskd::fail(SSKD_ERR_INVALID, "%s: q_lims[0] < 0", what), -1;
  int max_tq = 0;
  for (int q = 0; q < nq; ++q) {
    const int64_t tq = q_lims[q + 1] - q_lims[q];
    if (tq < 1 || tq > L_TQ_MAX)
      return sskd::fail(SSKD_ERR_INVALID, "%s: query %d has Tq=%lld outside [1, %d] (q_lims must ascend)", what, q, (long long)tq,
                        L_TQ_MAX), -1;
    if (tq > max_tq) max_tq = (int)tq;
  }
  if (training && tq_stride != (max_tq + 31) / 32 * 32)
    return sskd::fail(SSKD_ERR_INVALID, "%s: tq_stride=%d, the largest Tq=%d rounded up to 32 is %d", what, tq_stride, max_tq,
                      (max_tq + 31) / 32 * 32), -1;
  return max_tq;
}

struct LatePlan {
  int qb, chunk, chunks;
};

bool late_shape_ok(int nq, int max_tq, int R, int k) {
  return nq >= 1 && max_tq >= 1 && max_tq <= L_TQ_MAX && R >= 1 && R <= L_R_MAX && k >= 1 && k <= R;
}

// chunk = candidates of one workgroup: a multiple of the 4 waves, small enough that a single query still spreads over the
// chip (about 8 workgroups per compute unit in all), large enough that the staged query is amortised when there are many
LatePlan late_plan(int nq, int max_tq, int R) {
  LatePlan pl;
  pl.qb = (max_tq + 31) / 32;
  const int64_t target = 8 * (int64_t)sskd::cu_count();
  int64_t per_query = sskd::ceil_div(target, nq);
  const int64_t most = sskd::ceil_div(R, L_WAVES);
  if (per_query > most) per_query = most;
  if (per_query < 1) per_query = 1;
  pl.chunk = (int)(sskd::ceil_div(sskd::ceil_div(R, per_query), L_WAVES) * L_WAVES);
  pl.chunks = (int)sskd::ceil_div(R, pl.chunk);
  return pl;
}

}  // namespace
