// Late interaction (include/sskd_amd.h, "Late interaction"): the token store's pack kernel and the MaxSim re-rank.
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
// score's bits depend on nothing but the two token lists.
#include <cfloat>
#include <cmath>

#include "search_device.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int L_WAVES = 4;
constexpr int L_THREADS = L_WAVES * 64;
constexpr int L_KSTEPS = DIM / 16;          // 24 k-steps of v_mfma_f32_32x32x16_bf16
constexpr int L_ROW_VEC = DIM / 8;          // 48 16-byte vectors per token row
constexpr int L_TQ_MAX = SSKD_LATE_TQ_MAX;  // 128
constexpr int L_R_MAX = SSKD_LATE_R_MAX;    // 1024
constexpr int L_QB_MAX = L_TQ_MAX / 32;

// ------------------------------------------------------------------------------------------------ pack
// One wave per (text, position).  Lane l < 48 holds columns 8 l .. 8 l + 7 of the row (one 16-byte load: the wave reads
// the whole 768-byte row at once).  Sum of squares, THE order (tests/late_cases.py pack_rows restates it):
//   p_l = fma chain from +0.0f over the lane's 8 columns ascending (a bf16 square is exact in fp32, so the fma equals
//         add(p, x * x));  p_l = +0.0f for lanes 48 .. 63;
//   butterfly: for o = 32, 16, 8, 4, 2, 1: p_l = p_l + p_(l ^ o)   (fp32 addition commutes, so every lane holds the same bits).
// t = x / max(sqrt(ss), 1e-12f) with correctly rounded sqrt and division, rounded to bf16 to nearest even.
__global__ __launch_bounds__(L_THREADS) void late_pack_kernel(const uint16_t* __restrict__ hidden, const int32_t* __restrict__ lengths,
                                                              const int64_t* __restrict__ offsets, int B, int S,
                                                              int64_t n_tokens, uint16_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * L_WAVES + (threadIdx.x >> 6);
  if (tok >= (int64_t)B * S) return;
  const int b = (int)(tok / S), s = (int)(tok % S);
  if (s >= lengths[b]) return;                 // padding is never read and never written
  const int64_t row = offsets[b] + s;
  if (row < 0 || row >= n_tokens) return;      // (the host checked what it can see; this keeps a bad offset harmless)
  float x[8];
  float p = 0.f;
  if (lane < L_ROW_VEC) {
    const uint4 v = *reinterpret_cast<const uint4*>(hidden + tok * DIM + 8 * lane);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[2 * j] = __uint_as_float(w[j] << 16);
      x[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) p = fmaf(x[j], x[j], p);
  }
  const float ss = wave_sum(p);
  const float denom = fmaxf(__builtin_sqrtf(ss), 1e-12f);   // IEEE: hipcc rounds fp32 sqrt and division correctly by default
  if (lane < L_ROW_VEC) {
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t h[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint32_t u = __float_as_uint(x[2 * j + e] / denom);
        h[e] = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;   // round to nearest even (finite input)
      }
      o[j] = h[0] | (h[1] << 16);
    }
    *reinterpret_cast<uint4*>(out + row * DIM + 8 * lane) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ------------------------------------------------------------------------------------------------ scores
struct LateParams {
  const bf16x8* q_tokens;    // [sum Tq, 48]
  const int64_t* q_lims;     // [nq + 1]
  const bf16x8* tokens;      // [n_tokens, 48]
  const int64_t* tok_lims;   // [n_rows + 1]
  const int64_t* cand;       // [nq, R]
  float* raw;                // [nq, R]
  int32_t* arg;              // [nq, R, tq_stride], late_score_kernel<QB, true> only (the training forward)
  int64_t n_q_tokens, n_tokens, n_rows, id_offset;
  int R, chunk, tq_stride;
};

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

// QB = blocks of 32 query tokens the workgroup holds in LDS (the batch's largest query decides; a shorter query uses
// its own ceil(Tq / 32) blocks of them, so its scores do not depend on QB).
// ARG (sskd_latet_maxsim_fwd): also report, per query token, the document-relative index of the token that holds the max -
// the smallest such index.  The values and every operation on them are those of ARG = false (the index is found by
// comparing against the tile's max AFTER it has been formed), so the score's bits are the re-rank's.
template <int QB, bool ARG>
__global__ __launch_bounds__(L_THREADS) void late_score_kernel(const LateParams p) {
  __shared__ bf16x8 qs[QB][L_KSTEPS][64];   // B fragments: [block][k-step][lane]
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  int64_t q0 = p.q_lims[q], tq64 = p.q_lims[q + 1] - q0;
  if (q0 < 0 || tq64 < 0 || q0 + tq64 > p.n_q_tokens) tq64 = 0;   // (the host validated its copy of the lims)
  const int Tq = (int)(tq64 < QB * 32 ? tq64 : QB * 32);
  const int nb = (Tq + 31) >> 5;            // blocks in use (workgroup-uniform)
  // stage: token row i, 16-byte vector ch = 2 s + half -> qs[i >> 5][s][32 half + (i & 31)]; rows >= Tq are zeros
  for (int idx = threadIdx.x; idx < nb * 32 * L_ROW_VEC; idx += L_THREADS) {
    const int i = idx / L_ROW_VEC, ch = idx % L_ROW_VEC;
    bf16x8 v = __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
    if (i < Tq) v = p.q_tokens[(q0 + i) * L_ROW_VEC + ch];
    qs[i >> 5][ch >> 1][((ch & 1) << 5) | (i & 31)] = v;
  }
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
      for (int64_t t0 = 0; t0 < td; t0 += 32) {
        // the lane's document row of this tile; rows past the end re-read the last real row and are masked below
        const int64_t j = t0 + r32 < td ? t0 + r32 : td - 1;
        const bf16x8* src = p.tokens + (beg + j) * L_ROW_VEC + h;
        bf16x8 a[L_KSTEPS];
#pragma unroll
        for (int s = 0; s < L_KSTEPS; ++s) a[s] = src[2 * s];
        const bool partial = td - t0 < 32;
        const int left = (int)(td - t0);    // real rows of the tile when partial
#pragma unroll
        for (int b = 0; b < QB; ++b) {
          if (b < nb) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < L_KSTEPS; ++s)
              acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], qs[b][s][lane], acc, 0, 0, 0);
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
      if (ARG) {   // tq_stride == 32 QB (the host checked): the QB blocks cover a pair's whole row of arg
        int32_t* out = p.arg + ((int64_t)q * p.R + c) * (32 * QB) + r32;
#pragma unroll
        for (int b = 0; b < QB; ++b)
          if (h == 0) out[32 * b] = 32 * b + r32 < Tq ? barg[b] : -1;
      }
    } else if (ARG) {
      for (int i = lane; i < p.tq_stride; i += 64) p.arg[((int64_t)q * p.R + c) * p.tq_stride + i] = -1;
    }
    if (lane == 0) p.raw[(int64_t)q * p.R + c] = score;
  }
}

// ------------------------------------------------------------------------------------------------ compressed store
// A token is the id of a centroid (bf16 [C, 384]) plus an NBITS code per column: code = number of cutoffs strictly below
// r = fp32(t) - fp32(c); what the score sees is dec = bf16_rn(fp32(c) + weights[code]) and scale = 1 / max(|dec|, 1e-12)
// (include/sskd_amd.h, "compressed token store"; tests/late_codec_cases.py restates all of it).  Column d = 16 s + 8 h + e
// sits at position 192 h + 8 s + e, NBITS bits each, low bits first: the A operand of lane half h is bytes
// [24 NBITS h, 24 NBITS (h + 1)) of the row, and k-step s of it is the NBITS bytes from 24 NBITS h + NBITS s.
constexpr int L_C_MAX = SSKD_LATE_C_MAX;    // 65 536

__device__ inline uint32_t bf16_rn_bits(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;   // round to nearest even (finite input)
}

// One wave per token; lane l < 48 holds columns 8 l .. 8 l + 7 (k-step l >> 1, lane half l & 1) of the token and of its
// centroid.  The sum of squares of dec runs in the pack kernel's order.
template <int NBITS>
__global__ __launch_bounds__(L_THREADS) void late_compress_kernel(const uint16_t* __restrict__ tokens, const int64_t* __restrict__ assign,
                                                                  int64_t n, const uint16_t* __restrict__ centroids, int C,
                                                                  const float* __restrict__ cutoffs, const float* __restrict__ weights,
                                                                  int32_t* __restrict__ cid_out, float* __restrict__ scale_out,
                                                                  uint8_t* __restrict__ codes_out, int64_t row0) {
  constexpr int L = 1 << NBITS;
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * L_WAVES + (threadIdx.x >> 6);
  if (tok >= n) return;
  const int64_t want = assign[tok];
  const int c = want < 0 ? 0 : (want >= C ? C - 1 : (int)want);   // never an address from unchecked data
  float p = 0.f;
  uint32_t packed = 0u;
  if (lane < L_ROW_VEC) {
    const uint4 tv = *reinterpret_cast<const uint4*>(tokens + tok * DIM + 8 * lane);
    const uint4 cv = *reinterpret_cast<const uint4*>(centroids + (int64_t)c * DIM + 8 * lane);
    const uint32_t tw[4] = {tv.x, tv.y, tv.z, tv.w}, cw[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = __uint_as_float(e & 1 ? tw[e >> 1] & 0xFFFF0000u : tw[e >> 1] << 16);
      const float cc = __uint_as_float(e & 1 ? cw[e >> 1] & 0xFFFF0000u : cw[e >> 1] << 16);
      const float r = t - cc;
      uint32_t code = 0u;
#pragma unroll
      for (int i = 0; i < L - 1; ++i) code += cutoffs[i] < r ? 1u : 0u;   // false for NaN: code 0
      const float dec = __uint_as_float(bf16_rn_bits(cc + weights[code]) << 16);
      p = fmaf(dec, dec, p);
      packed |= code << (NBITS * e);
    }
  }
  const float ss = wave_sum(p);
  const float scale = 1.0f / fmaxf(__builtin_sqrtf(ss), 1e-12f);   // IEEE sqrt and division (see the pack kernel)
  const int64_t row = row0 + tok;
  if (lane < L_ROW_VEC) {
    uint8_t* dst = codes_out + row * (6 * 8 * NBITS) + (24 * NBITS) * (lane & 1) + NBITS * (lane >> 1);
    if (NBITS == 2) *reinterpret_cast<uint16_t*>(dst) = (uint16_t)packed;
    else *reinterpret_cast<uint32_t*>(dst) = packed;
  }
  if (lane == 0) {
    cid_out[row] = c;
    scale_out[row] = scale;
  }
}

struct LateCParams {
  const bf16x8* q_tokens;    // [sum Tq, 48]
  const int64_t* q_lims;     // [nq + 1]
  const int32_t* cid;        // [n_tokens]
  const float* scale;        // [n_tokens]
  const uint8_t* codes;      // [n_tokens, 48 NBITS]
  const bf16x8* centroids;   // [C, 48]
  const float* weights;      // [2^NBITS]
  const int64_t* tok_lims;   // [n_rows + 1]
  const int64_t* cand;       // [nq, R]
  float* raw;                // [nq, R]
  int64_t n_q_tokens, n_tokens, n_rows, id_offset;
  int R, chunk, C;
};

// late_score_kernel with the A operand decoded in registers: per tile a lane reads its row's centroid id, scale and its
// half of the row's codes, gathers the 24 16-byte pieces of the centroid row (the request shape of the bf16 store's token
// loads, the row address taken from the clamped id) and turns each piece into the k-step's fragment in place.  The weights
// sit in a 16-float LDS table: the lanes of a wave read at most 16 consecutive words, which is conflict-free.
template <int QB, int NBITS>
__global__ __launch_bounds__(L_THREADS) void late_score_compressed_kernel(const LateCParams p) {
  constexpr int CODE_VEC = 3 * NBITS / 2;   // 16-byte loads of one lane half's codes: 3 or 6
  constexpr uint32_t MASK = (1u << NBITS) - 1u;
  __shared__ bf16x8 qs[QB][L_KSTEPS][64];   // B fragments: [block][k-step][lane]
  __shared__ float wt[16];
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r32 = lane & 31, h = lane >> 5;
  int64_t q0 = p.q_lims[q], tq64 = p.q_lims[q + 1] - q0;
  if (q0 < 0 || tq64 < 0 || q0 + tq64 > p.n_q_tokens) tq64 = 0;   // (the host validated its copy of the lims)
  const int Tq = (int)(tq64 < QB * 32 ? tq64 : QB * 32);
  const int nb = (Tq + 31) >> 5;            // blocks in use (workgroup-uniform)
  for (int idx = threadIdx.x; idx < nb * 32 * L_ROW_VEC; idx += L_THREADS) {
    const int i = idx / L_ROW_VEC, ch = idx % L_ROW_VEC;
    bf16x8 v = __builtin_bit_cast(bf16x8, make_uint4(0u, 0u, 0u, 0u));
    if (i < Tq) v = p.q_tokens[(q0 + i) * L_ROW_VEC + ch];
    qs[i >> 5][ch >> 1][((ch & 1) << 5) | (i & 31)] = v;
  }
  if (threadIdx.x < 16) wt[threadIdx.x] = threadIdx.x <= MASK ? p.weights[threadIdx.x] : 0.f;
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
#pragma unroll
      for (int b = 0; b < QB; ++b) best[b] = -INFINITY;
      // the centroid id of the lane's row is loaded one tile ahead, so that the centroid gather of a tile does not wait
      // for it behind the previous tile's MFMAs
      int cid_next = p.cid[beg + (r32 < td ? r32 : td - 1)];
      for (int64_t t0 = 0; t0 < td; t0 += 32) {
        // the lane's document row of this tile; rows past the end re-read the last real row and are masked below
        const int64_t row = beg + (t0 + r32 < td ? t0 + r32 : td - 1);
        const int cen = min(max(cid_next, 0), p.C - 1);   // a corrupt store scores garbage and cannot fault
        if (t0 + 32 < td) cid_next = p.cid[beg + (t0 + 32 + r32 < td ? t0 + 32 + r32 : td - 1)];
        const float sc = p.scale[row];
        const uint4* cp = reinterpret_cast<const uint4*>(p.codes + row * (6 * 8 * NBITS) + (24 * NBITS) * h);
        uint32_t cw[4 * CODE_VEC];
#pragma unroll
        for (int v = 0; v < CODE_VEC; ++v) {
          const uint4 u = cp[v];
          cw[4 * v] = u.x; cw[4 * v + 1] = u.y; cw[4 * v + 2] = u.z; cw[4 * v + 3] = u.w;
        }
        const bf16x8* src = p.centroids + (int64_t)cen * L_ROW_VEC + h;
        bf16x8 a[L_KSTEPS];
#pragma unroll
        for (int s = 0; s < L_KSTEPS; ++s) a[s] = src[2 * s];
        // decode in place: widen, add weights[code], round to bf16 (nearest even), pack
#pragma unroll
        for (int s = 0; s < L_KSTEPS; ++s) {
          const uint32_t bits = NBITS == 2 ? cw[s >> 1] >> (16 * (s & 1)) : cw[s];
          const uint4 cv = __builtin_bit_cast(uint4, a[s]);
          const uint32_t w[4] = {cv.x, cv.y, cv.z, cv.w};
          uint32_t o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float lo = __uint_as_float(w[j] << 16) + wt[(bits >> (NBITS * 2 * j)) & MASK];
            const float hi = __uint_as_float(w[j] & 0xFFFF0000u) + wt[(bits >> (NBITS * (2 * j + 1))) & MASK];
            o[j] = bf16_rn_bits(lo) | (bf16_rn_bits(hi) << 16);
          }
          a[s] = __builtin_bit_cast(bf16x8, make_uint4(o[0], o[1], o[2], o[3]));
        }
        // accumulator register r of lane l belongs to document row acc_row(r) + 4 (l >> 5) of the tile: its scale
        float scr[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) scr[r] = __shfl(sc, acc_row(r) + 4 * h);
        const bool partial = td - t0 < 32;
        const int left = (int)(td - t0);    // real rows of the tile when partial
#pragma unroll
        for (int b = 0; b < QB; ++b) {
          if (b < nb) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < L_KSTEPS; ++s)
              acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], qs[b][s][lane], acc, 0, 0, 0);
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const bool real = !partial || acc_row(r) + 4 * h < left;
              m = fmaxf(m, real ? acc[r] * scr[r] : -INFINITY);
            }
            m = fmaxf(m, __shfl_xor(m, 32));
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
    }
    if (lane == 0) p.raw[(int64_t)q * p.R + c] = score;
  }
}

// ------------------------------------------------------------------------------------------------ top-k
// One wave per query: the rank-order pick of search_device.h over the R raw scores (score descending, then lower id).
// -inf and NaN scores are no candidates; the result is padded with (-inf, -1).
__global__ __launch_bounds__(64) void late_pick_kernel(const float* __restrict__ raw, const int64_t* __restrict__ cand, int R,
                                                       int k, float* __restrict__ out_scores, int64_t* __restrict__ out_ids) {
  const int q = blockIdx.x, lane = threadIdx.x;
  float cs[L_R_MAX / 64];
  int64_t cid[L_R_MAX / 64];
#pragma unroll
  for (int c = 0; c < L_R_MAX / 64; ++c) {
    const int idx = c * 64 + lane;
    cs[c] = -INFINITY;
    cid[c] = -1;
    if (idx < R) {
      const float s = raw[(int64_t)q * R + idx];
      cs[c] = s;
      cid[c] = s > -INFINITY ? cand[(int64_t)q * R + idx] : -1;   // false for -inf and for NaN
    }
  }
  float bs = INFINITY;
  int64_t bi = -1;
  bool have = false;
  for (int r = 0; r < k; ++r) {
    float s = -INFINITY;
    int64_t i = -1;
#pragma unroll
    for (int c = 0; c < L_R_MAX / 64; ++c)
      if (cid[c] >= 0) pick_after(s, i, cs[c], cid[c], have, bs, bi);
    wave_argbest(s, i);
    if (i < 0) {
      for (int rr = r + lane; rr < k; rr += 64) {
        out_scores[(int64_t)q * k + rr] = -INFINITY;
        out_ids[(int64_t)q * k + rr] = -1;
      }
      break;
    }
    if (lane == 0) {
      out_scores[(int64_t)q * k + r] = s;
      out_ids[(int64_t)q * k + r] = i;
    }
    bs = s; bi = i; have = true;
  }
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

template <int QB, bool ARG>
void launch_score(const LateParams& p, int nq, int chunks, hipStream_t st) {
  hipLaunchKernelGGL((late_score_kernel<QB, ARG>), dim3((unsigned)nq, (unsigned)chunks), dim3(L_THREADS), 0, st, p);
}

template <bool ARG>
void launch_score_qb(const LateParams& p, int qb, int nq, int chunks, hipStream_t st) {
  switch (qb) {
    case 1: launch_score<1, ARG>(p, nq, chunks, st); break;
    case 2: launch_score<2, ARG>(p, nq, chunks, st); break;
    case 3: launch_score<3, ARG>(p, nq, chunks, st); break;
    default: launch_score<4, ARG>(p, nq, chunks, st); break;
  }
}

template <int QB, int NBITS>
void launch_score_compressed(const LateCParams& p, int nq, int chunks, hipStream_t st) {
  hipLaunchKernelGGL((late_score_compressed_kernel<QB, NBITS>), dim3((unsigned)nq, (unsigned)chunks), dim3(L_THREADS), 0, st, p);
}

template <int NBITS>
void launch_score_compressed_qb(const LateCParams& p, int qb, int nq, int chunks, hipStream_t st) {
  switch (qb) {
    case 1: launch_score_compressed<1, NBITS>(p, nq, chunks, st); break;
    case 2: launch_score_compressed<2, NBITS>(p, nq, chunks, st); break;
    case 3: launch_score_compressed<3, NBITS>(p, nq, chunks, st); break;
    default: launch_score_compressed<4, NBITS>(p, nq, chunks, st); break;
  }
}

bool aligned16(const void* ptr) { return reinterpret_cast<uintptr_t>(ptr) % 16 == 0; }

}  // namespace

extern "C" {

int sskd_late_pack_tokens(const void* d_hidden, const int32_t* d_lengths, const int64_t* d_offsets, int B, int S,
                          int64_t n_tokens, void* d_tokens, void* stream) {
  SSKD_REQUIRE(B >= 0 && S >= 1, "late_pack_tokens: needs B >= 0 and S >= 1 (B=%d, S=%d)", B, S);
  SSKD_REQUIRE(n_tokens >= 0, "late_pack_tokens: n_tokens < 0");
  if (B == 0) return SSKD_OK;
  SSKD_REQUIRE(d_hidden && d_lengths && d_offsets && d_tokens, "late_pack_tokens: null pointer");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_hidden) % 16 == 0 && reinterpret_cast<uintptr_t>(d_tokens) % 16 == 0,
               "late_pack_tokens: hidden states and token store must be 16-byte aligned");
  const int64_t waves = (int64_t)B * S;
  SSKD_REQUIRE(waves / L_WAVES < (int64_t)INT32_MAX, "late_pack_tokens: B * S too large");
  hipLaunchKernelGGL(late_pack_kernel, dim3((unsigned)sskd::ceil_div(waves, L_WAVES)), dim3(L_THREADS), 0, sskd::as_stream(stream),
                     static_cast<const uint16_t*>(d_hidden), d_lengths, d_offsets, B, S, n_tokens,
                     static_cast<uint16_t*>(d_tokens));
  return sskd::check_launch("late_pack_kernel");
}

int sskd_late_rerank_plan(int nq, int max_tq, int R, int k, int* workgroups, int* threads, int* lds_bytes, int* chunk) {
  SSKD_REQUIRE(late_shape_ok(nq, max_tq, R, k), "late_rerank_plan: needs nq >= 1, 1 <= Tq <= %d, 1 <= k <= R <= %d", L_TQ_MAX,
               L_R_MAX);
  const LatePlan pl = late_plan(nq, max_tq, R);
  if (workgroups) *workgroups = nq * pl.chunks;
  if (threads) *threads = L_THREADS;
  if (lds_bytes) *lds_bytes = pl.qb * L_KSTEPS * 64 * (int)sizeof(bf16x8);
  if (chunk) *chunk = pl.chunk;
  return SSKD_OK;
}

size_t sskd_late_rerank_workspace_bytes(int nq, int R) {
  if (nq < 1 || R < 1 || R > L_R_MAX) return 0;
  sskd::Carver ws(nullptr);
  ws.take<float>((size_t)nq * R);   // the raw scores when the caller does not ask for them
  return ws.bytes();
}

int sskd_late_rerank(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq, const void* d_tokens,
                     const int64_t* d_tok_lims, int64_t n_rows, int64_t n_tokens, const int64_t* d_candidates, int R, int k,
                     int64_t id_offset, float* d_out_scores, int64_t* d_out_ids, float* d_out_raw, void* d_workspace,
                     size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(nq >= 0, "late_rerank: nq < 0");
  SSKD_REQUIRE(R >= 1 && R <= L_R_MAX, "late_rerank: R=%d outside [1, %d]", R, L_R_MAX);
  SSKD_REQUIRE(k >= 1 && k <= R, "late_rerank: k=%d outside [1, R=%d]", k, R);
  SSKD_REQUIRE(n_rows >= 0 && n_tokens >= 0 && id_offset >= 0, "late_rerank: n_rows, n_tokens and id_offset must be >= 0");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(q_lims, "late_rerank: the host copy of q_lims is required");
  SSKD_REQUIRE(q_lims[0] >= 0, "late_rerank: q_lims[0] < 0");
  int max_tq = 0;
  for (int q = 0; q < nq; ++q) {
    const int64_t tq = q_lims[q + 1] - q_lims[q];
    SSKD_REQUIRE(tq >= 1 && tq <= L_TQ_MAX, "late_rerank: query %d has Tq=%lld outside [1, %d] (q_lims must ascend)", q,
                 (long long)tq, L_TQ_MAX);
    if (tq > max_tq) max_tq = (int)tq;
  }
  SSKD_REQUIRE(d_q_tokens && d_q_lims && d_candidates && d_out_scores && d_out_ids, "late_rerank: null pointer");
  SSKD_REQUIRE(n_rows == 0 || (d_tokens && d_tok_lims) || n_tokens == 0, "late_rerank: null token store");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_q_tokens) % 16 == 0 && reinterpret_cast<uintptr_t>(d_tokens) % 16 == 0,
               "late_rerank: token matrices must be 16-byte aligned");
  float* raw = d_out_raw;
  if (!raw) {
    const size_t need = sskd_late_rerank_workspace_bytes(nq, R);
    if (int rc = sskd::require_workspace("late_rerank", d_workspace, workspace_bytes, need)) return rc;
    sskd::Carver ws(d_workspace);
    raw = ws.take<float>((size_t)nq * R);
  }
  LateParams p{};
  p.q_tokens = static_cast<const bf16x8*>(d_q_tokens);
  p.q_lims = d_q_lims;
  p.tokens = static_cast<const bf16x8*>(d_tokens);
  p.tok_lims = d_tok_lims;
  p.cand = d_candidates;
  p.raw = raw;
  p.n_q_tokens = q_lims[nq];
  p.n_tokens = (d_tokens && d_tok_lims) ? n_tokens : 0;
  p.n_rows = (d_tokens && d_tok_lims) ? n_rows : 0;
  p.id_offset = id_offset;
  p.R = R;
  const LatePlan pl = late_plan(nq, max_tq, R);
  p.chunk = pl.chunk;
  hipStream_t st = sskd::as_stream(stream);
  launch_score_qb<false>(p, pl.qb, nq, pl.chunks, st);
  if (int rc = sskd::check_launch("late_score_kernel")) return rc;
  hipLaunchKernelGGL(late_pick_kernel, dim3((unsigned)nq), dim3(64), 0, st, raw, d_candidates, R, k, d_out_scores, d_out_ids);
  return sskd::check_launch("late_pick_kernel");
}

int sskd_latet_maxsim_fwd(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq, int64_t n_q_tokens,
                         const void* d_d_tokens, const int64_t* d_d_lims, int64_t nd, int64_t n_d_tokens,
                         const int64_t* d_candidates, int R, float* d_scores, int32_t* d_arg, int tq_stride, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(nq >= 0 && R >= 0, "late_maxsim_fwd: nq=%d, R=%d must be >= 0", nq, R);
  SSKD_REQUIRE(R <= L_R_MAX, "late_maxsim_fwd: R=%d above %d (score the candidates in chunks)", R, L_R_MAX);
  SSKD_REQUIRE(nd >= 0 && n_d_tokens >= 0 && n_q_tokens >= 0, "late_maxsim_fwd: nd, n_d_tokens and n_q_tokens must be >= 0");
  if (nq == 0 || R == 0) return SSKD_OK;
  SSKD_REQUIRE(q_lims, "late_maxsim_fwd: the host copy of q_lims is required");
  SSKD_REQUIRE(q_lims[0] == 0 && q_lims[nq] == n_q_tokens, "late_maxsim_fwd: q_lims runs from %lld to %lld, there are %lld query token rows",
               (long long)q_lims[0], (long long)q_lims[nq], (long long)n_q_tokens);
  int max_tq = 0;
  for (int q = 0; q < nq; ++q) {
    const int64_t tq = q_lims[q + 1] - q_lims[q];
    SSKD_REQUIRE(tq >= 1 && tq <= L_TQ_MAX, "late_maxsim_fwd: query %d has Tq=%lld outside [1, %d] (q_lims must ascend)", q,
                 (long long)tq, L_TQ_MAX);
    if (tq > max_tq) max_tq = (int)tq;
  }
  const LatePlan pl = late_plan(nq, max_tq, R);
  SSKD_REQUIRE(tq_stride == 32 * pl.qb, "late_maxsim_fwd: tq_stride=%d, the largest Tq=%d rounded up to 32 is %d", tq_stride, max_tq,
               32 * pl.qb);
  SSKD_REQUIRE(d_q_tokens && d_q_lims && d_candidates && d_scores && d_arg, "late_maxsim_fwd: null pointer");
  SSKD_REQUIRE(nd == 0 || n_d_tokens == 0 || (d_d_tokens && d_d_lims), "late_maxsim_fwd: null document tokens");
  SSKD_REQUIRE(aligned16(d_q_tokens) && aligned16(d_d_tokens), "late_maxsim_fwd: token matrices must be 16-byte aligned");
  LateParams p{};
  p.q_tokens = static_cast<const bf16x8*>(d_q_tokens);
  p.q_lims = d_q_lims;
  p.tokens = static_cast<const bf16x8*>(d_d_tokens);
  p.tok_lims = d_d_lims;
  p.cand = d_candidates;
  p.raw = d_scores;
  p.arg = d_arg;
  p.n_q_tokens = n_q_tokens;
  p.n_tokens = (d_d_tokens && d_d_lims) ? n_d_tokens : 0;
  p.n_rows = (d_d_tokens && d_d_lims) ? nd : 0;
  p.id_offset = 0;
  p.R = R;
  p.chunk = pl.chunk;
  p.tq_stride = tq_stride;
  launch_score_qb<true>(p, pl.qb, nq, pl.chunks, sskd::as_stream(stream));
  return sskd::check_launch("late_score_kernel<arg>");
}

int sskd_latec_compress(const void* d_tokens, const int64_t* d_assign, int64_t n, const void* d_centroids, int C,
                       const float* d_cutoffs, const float* d_weights, int nbits, int32_t* d_cid, float* d_scale,
                       uint8_t* d_codes, int64_t row0, int64_t n_store, void* stream) {
  SSKD_REQUIRE(nbits == 2 || nbits == 4, "latec_compress: nbits=%d, needs 2 or 4", nbits);
  SSKD_REQUIRE(C >= 1 && C <= L_C_MAX, "latec_compress: C=%d outside [1, %d]", C, L_C_MAX);
  SSKD_REQUIRE(n >= 0 && row0 >= 0 && n_store >= 0 && row0 <= n_store && n <= n_store - row0,
               "latec_compress: rows [%lld, %lld + %lld) outside a store of %lld", (long long)row0, (long long)row0, (long long)n,
               (long long)n_store);
  if (n == 0) return SSKD_OK;
  SSKD_REQUIRE(d_tokens && d_assign && d_centroids && d_cutoffs && d_weights && d_cid && d_scale && d_codes,
               "latec_compress: null pointer");
  SSKD_REQUIRE(aligned16(d_tokens) && aligned16(d_centroids) && aligned16(d_codes) && aligned16(d_cid) && aligned16(d_scale),
               "latec_compress: tokens, centroids and the store's arrays must be 16-byte aligned");
  SSKD_REQUIRE(n / L_WAVES < (int64_t)INT32_MAX, "latec_compress: n too large");
  const dim3 grid((unsigned)sskd::ceil_div(n, L_WAVES));
  hipStream_t st = sskd::as_stream(stream);
  const uint16_t* tokens = static_cast<const uint16_t*>(d_tokens);
  const uint16_t* centroids = static_cast<const uint16_t*>(d_centroids);
  if (nbits == 2)
    hipLaunchKernelGGL(late_compress_kernel<2>, grid, dim3(L_THREADS), 0, st, tokens, d_assign, n, centroids, C, d_cutoffs,
                       d_weights, d_cid, d_scale, d_codes, row0);
  else
    hipLaunchKernelGGL(late_compress_kernel<4>, grid, dim3(L_THREADS), 0, st, tokens, d_assign, n, centroids, C, d_cutoffs,
                       d_weights, d_cid, d_scale, d_codes, row0);
  return sskd::check_launch("late_compress_kernel");
}

int sskd_latec_rerank_plan(int nq, int max_tq, int R, int k, int nbits, int* workgroups, int* threads, int* lds_bytes,
                                     int* chunk) {
  SSKD_REQUIRE(nbits == 2 || nbits == 4, "latec_rerank_plan: nbits=%d, needs 2 or 4", nbits);
  SSKD_REQUIRE(late_shape_ok(nq, max_tq, R, k), "latec_rerank_plan: needs nq >= 1, 1 <= Tq <= %d, 1 <= k <= R <= %d",
               L_TQ_MAX, L_R_MAX);
  const LatePlan pl = late_plan(nq, max_tq, R);
  if (workgroups) *workgroups = nq * pl.chunks;
  if (threads) *threads = L_THREADS;
  if (lds_bytes) *lds_bytes = pl.qb * L_KSTEPS * 64 * (int)sizeof(bf16x8) + 16 * (int)sizeof(float);
  if (chunk) *chunk = pl.chunk;
  return SSKD_OK;
}

size_t sskd_latec_rerank_workspace_bytes(int nq, int R) { return sskd_late_rerank_workspace_bytes(nq, R); }

int sskd_latec_rerank(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq,
                                const int32_t* d_cid, const float* d_scale, const uint8_t* d_codes, int nbits,
                                const void* d_centroids, int C, const float* d_weights, const int64_t* d_tok_lims, int64_t n_rows,
                                int64_t n_tokens, const int64_t* d_candidates, int R, int k, int64_t id_offset,
                                float* d_out_scores, int64_t* d_out_ids, float* d_out_raw, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(nq >= 0, "latec_rerank: nq < 0");
  SSKD_REQUIRE(nbits == 2 || nbits == 4, "latec_rerank: nbits=%d, needs 2 or 4", nbits);
  SSKD_REQUIRE(C >= 1 && C <= L_C_MAX, "latec_rerank: C=%d outside [1, %d]", C, L_C_MAX);
  SSKD_REQUIRE(R >= 1 && R <= L_R_MAX, "latec_rerank: R=%d outside [1, %d]", R, L_R_MAX);
  SSKD_REQUIRE(k >= 1 && k <= R, "latec_rerank: k=%d outside [1, R=%d]", k, R);
  SSKD_REQUIRE(n_rows >= 0 && n_tokens >= 0 && id_offset >= 0,
               "latec_rerank: n_rows, n_tokens and id_offset must be >= 0");
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(q_lims, "latec_rerank: the host copy of q_lims is required");
  SSKD_REQUIRE(q_lims[0] >= 0, "latec_rerank: q_lims[0] < 0");
  int max_tq = 0;
  for (int q = 0; q < nq; ++q) {
    const int64_t tq = q_lims[q + 1] - q_lims[q];
    SSKD_REQUIRE(tq >= 1 && tq <= L_TQ_MAX, "latec_rerank: query %d has Tq=%lld outside [1, %d] (q_lims must ascend)", q,
                 (long long)tq, L_TQ_MAX);
    if (tq > max_tq) max_tq = (int)tq;
  }
  SSKD_REQUIRE(d_q_tokens && d_q_lims && d_candidates && d_out_scores && d_out_ids && d_centroids && d_weights,
               "latec_rerank: null pointer");
  const bool store = d_cid && d_scale && d_codes && d_tok_lims;
  SSKD_REQUIRE(n_rows == 0 || store || n_tokens == 0, "latec_rerank: null token store");
  SSKD_REQUIRE(aligned16(d_q_tokens) && aligned16(d_centroids) && aligned16(d_codes) && aligned16(d_cid) && aligned16(d_scale),
               "latec_rerank: query tokens, centroids and the store's arrays must be 16-byte aligned");
  float* raw = d_out_raw;
  if (!raw) {
    const size_t need = sskd_latec_rerank_workspace_bytes(nq, R);
    if (int rc = sskd::require_workspace("latec_rerank", d_workspace, workspace_bytes, need)) return rc;
    sskd::Carver ws(d_workspace);
    raw = ws.take<float>((size_t)nq * R);
  }
  LateCParams p{};
  p.q_tokens = static_cast<const bf16x8*>(d_q_tokens);
  p.q_lims = d_q_lims;
  p.cid = d_cid;
  p.scale = d_scale;
  p.codes = d_codes;
  p.centroids = static_cast<const bf16x8*>(d_centroids);
  p.weights = d_weights;
  p.tok_lims = d_tok_lims;
  p.cand = d_candidates;
  p.raw = raw;
  p.n_q_tokens = q_lims[nq];
  p.n_tokens = store ? n_tokens : 0;
  p.n_rows = store ? n_rows : 0;
  p.id_offset = id_offset;
  p.R = R;
  p.C = C;
  const LatePlan pl = late_plan(nq, max_tq, R);
  p.chunk = pl.chunk;
  hipStream_t st = sskd::as_stream(stream);
  if (nbits == 2) launch_score_compressed_qb<2>(p, pl.qb, nq, pl.chunks, st);
  else launch_score_compressed_qb<4>(p, pl.qb, nq, pl.chunks, st);
  if (int rc = sskd::check_launch("late_score_compressed_kernel")) return rc;
  hipLaunchKernelGGL(late_pick_kernel, dim3((unsigned)nq), dim3(64), 0, st, raw, d_candidates, R, k, d_out_scores, d_out_ids);
  return sskd::check_launch("late_pick_kernel");
}

}  // extern "C"
