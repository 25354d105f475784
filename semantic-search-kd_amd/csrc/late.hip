// Late interaction (include/sskd_amd.h, "Late interaction"): the token store's pack kernel, the MaxSim re-rank over the
// bf16 store and over the compressed store, and the forward of the training path.  The geometry of the score kernels and
// their one body are in late_device.h; here are the two store formats (the body's tile sources) and the host side.
#include "late_device.h"

namespace {

// ------------------------------------------------------------------------------------------------ pack
// One wave per (text, position).  Lane l < 48 holds columns 8 l .. 8 l + 7 of the row (one 16-byte load: the wave reads
// the whole 768-byte row at once).  Sum of squares: row_sum_squares, THE order.
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
  if (lane < L_ROW_VEC) widen8(*reinterpret_cast<const uint4*>(hidden + tok * DIM + 8 * lane), x);
  const float ss = row_sum_squares(x, lane < L_ROW_VEC);
  const float denom = fmaxf(__builtin_sqrtf(ss), 1e-12f);   // IEEE: hipcc rounds fp32 sqrt and division correctly by default
  if (lane < L_ROW_VEC) {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = x[j] / denom;
    *reinterpret_cast<uint4*>(out + row * DIM + 8 * lane) = pack8(x);
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

// the bf16 store: the lane's row of a tile is 24 16-byte pieces of one token row
struct Bf16Source {
  const bf16x8* tokens;
  __device__ __forceinline__ void begin(int64_t, int64_t, int) const {}
  __device__ __forceinline__ void load(bf16x8 (&a)[L_KSTEPS], int64_t beg, int64_t t0, int64_t td, int r32, int h) const {
    const int64_t j = t0 + r32 < td ? t0 + r32 : td - 1;
    load_row_fragments(a, tokens + (beg + j) * L_ROW_VEC + h);
  }
};

template <int QB, bool ARG>
__global__ __launch_bounds__(L_THREADS) void late_score_kernel(const LateParams p) {
  __shared__ QueryFragments<QB> qs;
  Bf16Source src{p.tokens};
  maxsim_body<QB, ARG>(p, src, qs);
}

// ------------------------------------------------------------------------------------------------ compressed store
// A token is the id of a centroid (bf16 [C, 384]) plus an NBITS code per column: code = number of cutoffs strictly below
// r = fp32(t) - fp32(c); what the score sees is dec = bf16_rn(fp32(c) + weights[code]) and scale = 1 / max(|dec|, 1e-12)
// (include/sskd_amd.h, "compressed token store"; tests/late_codec_cases.py restates all of it).  Column d = 16 s + 8 h + e
// sits at position 192 h + 8 s + e, NBITS bits each, low bits first: the A operand of lane half h is bytes
// [24 NBITS h, 24 NBITS (h + 1)) of the row, and k-step s of it is the NBITS bytes from 24 NBITS h + NBITS s.

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
  float dec[8];
  uint32_t packed = 0u;
  if (lane < L_ROW_VEC) {
    float t[8], cc[8];
    widen8(*reinterpret_cast<const uint4*>(tokens + tok * DIM + 8 * lane), t);
    widen8(*reinterpret_cast<const uint4*>(centroids + (int64_t)c * DIM + 8 * lane), cc);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float r = t[e] - cc[e];
      uint32_t code = 0u;
#pragma unroll
      for (int i = 0; i < L - 1; ++i) code += cutoffs[i] < r ? 1u : 0u;   // false for NaN: code 0
      dec[e] = __uint_as_float(bf16_rn_bits(cc[e] + weights[code]) << 16);
      packed |= code << (NBITS * e);
    }
  }
  const float ss = row_sum_squares(dec, lane < L_ROW_VEC);
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
// The kernel keeps its own body beside late_device.h's maxsim_body: run through that body with a tile source of its own
// it computed the same bits, but its 4-bit instantiations measured 0.3 - 0.6 % slower at Tq = 32
// and the QB >= 2 ones moved by - 19 % .. + 7 % with the spelling of the decode (profiles/late_engine/README.md).  The
// kernels sit at or near 256 VGPRs; what is written here is the schedule that was measured.
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

// What sskd_late_rerank and sskd_latec_rerank share before their own store's checks: the shape checks and the host copy of
// the query bounds.  max_tq = the largest Tq (0 when nq == 0: nothing to do).
int rerank_checks(const char* what, const int64_t* q_lims, int nq, int R, int k, int64_t n_rows, int64_t n_tokens,
                  int64_t id_offset, int& max_tq) {
  max_tq = 0;
  SSKD_REQUIRE(nq >= 0, "%s: nq < 0", what);
  SSKD_REQUIRE(R >= 1 && R <= L_R_MAX, "%s: R=%d outside [1, %d]", what, R, L_R_MAX);
  SSKD_REQUIRE(k >= 1 && k <= R, "%s: k=%d outside [1, R=%d]", what, k, R);
  SSKD_REQUIRE(n_rows >= 0 && n_tokens >= 0 && id_offset >= 0, "%s: n_rows, n_tokens and id_offset must be >= 0", what);
  if (nq == 0) return SSKD_OK;
  max_tq = check_query_lims(what, q_lims, nq);
  return max_tq < 0 ? SSKD_ERR_INVALID : SSKD_OK;
}

// ... and after them (every check has passed, p holds the queries and the store): raw scores from the caller or carved
// from the workspace, the plan, the score launch (launch(qb, chunks, stream): the entry's kernel over p) and the pick.
template <class P, class Launch>
int rerank_tail(const char* what, const char* kernel, P& p, int nq, int max_tq, const int64_t* cand, int R, int k,
                float* out_scores, int64_t* out_ids, float* out_raw, void* workspace, size_t workspace_bytes, void* stream,
                Launch launch) {
  float* raw = out_raw;
  if (!raw) {
    const size_t need = sskd_late_rerank_workspace_bytes(nq, R);
    if (int rc = sskd::require_workspace(what, workspace, workspace_bytes, need)) return rc;
    sskd::Carver ws(workspace);
    raw = ws.take<float>((size_t)nq * R);
  }
  const LatePlan pl = late_plan(nq, max_tq, R);
  p.cand = cand;
  p.raw = raw;
  p.R = R;
  p.chunk = pl.chunk;
  hipStream_t st = sskd::as_stream(stream);
  launch(pl.qb, pl.chunks, st);
  if (int rc = sskd::check_launch(kernel)) return rc;
  hipLaunchKernelGGL(late_pick_kernel, dim3((unsigned)nq), dim3(64), 0, st, raw, cand, R, k, out_scores, out_ids);
  return sskd::check_launch("late_pick_kernel");
}

// the two plan queries: extra_lds = what the kernel keeps in LDS beside the staged query
int rerank_plan(const char* what, int nq, int max_tq, int R, int k, int extra_lds, int* workgroups, int* threads, int* lds_bytes,
                int* chunk) {
  SSKD_REQUIRE(late_shape_ok(nq, max_tq, R, k), "%s: needs nq >= 1, 1 <= Tq <= %d, 1 <= k <= R <= %d", what, L_TQ_MAX, L_R_MAX);
  const LatePlan pl = late_plan(nq, max_tq, R);
  if (workgroups) *workgroups = nq * pl.chunks;
  if (threads) *threads = L_THREADS;
  if (lds_bytes) *lds_bytes = pl.qb * L_KSTEPS * 64 * (int)sizeof(bf16x8) + extra_lds;
  if (chunk) *chunk = pl.chunk;
  return SSKD_OK;
}

}  // namespace

extern "C" {

int sskd_late_pack_tokens(const void* d_hidden, const int32_t* d_lengths, const int64_t* d_offsets, int B, int S,
                          int64_t n_tokens, void* d_tokens, void* stream) {
  SSKD_REQUIRE(B >= 0 && S >= 1, "late_pack_tokens: needs B >= 0 and S >= 1 (B=%d, S=%d)", B, S);
  SSKD_REQUIRE(n_tokens >= 0, "late_pack_tokens: n_tokens < 0");
  if (B == 0) return SSKD_OK;
  SSKD_REQUIRE(d_hidden && d_lengths && d_offsets && d_tokens, "late_pack_tokens: null pointer");
  SSKD_REQUIRE(aligned16(d_hidden) && aligned16(d_tokens), "late_pack_tokens: hidden states and token store must be 16-byte aligned");
  const int64_t waves = (int64_t)B * S;
  SSKD_REQUIRE(waves / L_WAVES < (int64_t)INT32_MAX, "late_pack_tokens: B * S too large");
  hipLaunchKernelGGL(late_pack_kernel, dim3((unsigned)sskd::ceil_div(waves, L_WAVES)), dim3(L_THREADS), 0, sskd::as_stream(stream),
                     static_cast<const uint16_t*>(d_hidden), d_lengths, d_offsets, B, S, n_tokens,
                     static_cast<uint16_t*>(d_tokens));
  return sskd::check_launch("late_pack_kernel");
}

int sskd_late_rerank_plan(int nq, int max_tq, int R, int k, int* workgroups, int* threads, int* lds_bytes, int* chunk) {
  return rerank_plan("late_rerank_plan", nq, max_tq, R, k, 0, workgroups, threads, lds_bytes, chunk);
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
  int max_tq;
  if (int rc = rerank_checks("late_rerank", q_lims, nq, R, k, n_rows, n_tokens, id_offset, max_tq)) return rc;
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_q_tokens && d_q_lims && d_candidates && d_out_scores && d_out_ids, "late_rerank: null pointer");
  const bool store = d_tokens && d_tok_lims;
  SSKD_REQUIRE(n_rows == 0 || store || n_tokens == 0, "late_rerank: null token store");
  SSKD_REQUIRE(aligned16(d_q_tokens) && aligned16(d_tokens), "late_rerank: token matrices must be 16-byte aligned");
  LateParams p{};
  p.q_tokens = static_cast<const bf16x8*>(d_q_tokens);
  p.q_lims = d_q_lims;
  p.tokens = static_cast<const bf16x8*>(d_tokens);
  p.tok_lims = d_tok_lims;
  p.n_q_tokens = q_lims[nq];
  p.n_tokens = store ? n_tokens : 0;
  p.n_rows = store ? n_rows : 0;
  p.id_offset = id_offset;
  return rerank_tail("late_rerank", "late_score_kernel", p, nq, max_tq, d_candidates, R, k, d_out_scores, d_out_ids, d_out_raw,
                     d_workspace, workspace_bytes, stream,
                     [&](int qb, int chunks, hipStream_t st) { launch_score_qb<false>(p, qb, nq, chunks, st); });
}

int sskd_latet_maxsim_fwd(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq, int64_t n_q_tokens,
                         const void* d_d_tokens, const int64_t* d_d_lims, int64_t nd, int64_t n_d_tokens,
                         const int64_t* d_candidates, int R, float* d_scores, int32_t* d_arg, int tq_stride, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(nq >= 0 && R >= 0, "late_maxsim_fwd: nq=%d, R=%d must be >= 0", nq, R);
  SSKD_REQUIRE(R <= L_R_MAX, "late_maxsim_fwd: R=%d above %d (score the candidates in chunks)", R, L_R_MAX);
  SSKD_REQUIRE(nd >= 0 && n_d_tokens >= 0 && n_q_tokens >= 0, "late_maxsim_fwd: nd, n_d_tokens and n_q_tokens must be >= 0");
  if (nq == 0 || R == 0) return SSKD_OK;
  const int max_tq = check_query_lims("late_maxsim_fwd", q_lims, nq, n_q_tokens, tq_stride);
  if (max_tq < 0) return SSKD_ERR_INVALID;
  const LatePlan pl = late_plan(nq, max_tq, R);
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
  return rerank_plan("latec_rerank_plan", nq, max_tq, R, k, 16 * (int)sizeof(float), workgroups, threads, lds_bytes, chunk);
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
  int max_tq;
  if (int rc = rerank_checks("latec_rerank", q_lims, nq, R, k, n_rows, n_tokens, id_offset, max_tq)) return rc;
  if (nq == 0) return SSKD_OK;
  SSKD_REQUIRE(d_q_tokens && d_q_lims && d_candidates && d_out_scores && d_out_ids && d_centroids && d_weights,
               "latec_rerank: null pointer");
  const bool store = d_cid && d_scale && d_codes && d_tok_lims;
  SSKD_REQUIRE(n_rows == 0 || store || n_tokens == 0, "latec_rerank: null token store");
  SSKD_REQUIRE(aligned16(d_q_tokens) && aligned16(d_centroids) && aligned16(d_codes) && aligned16(d_cid) && aligned16(d_scale),
               "latec_rerank: query tokens, centroids and the store's arrays must be 16-byte aligned");
  LateCParams p{};
  p.q_tokens = static_cast<const bf16x8*>(d_q_tokens);
  p.q_lims = d_q_lims;
  p.cid = d_cid;
  p.scale = d_scale;
  p.codes = d_codes;
  p.centroids = static_cast<const bf16x8*>(d_centroids);
  p.weights = d_weights;
  p.tok_lims = d_tok_lims;
  p.n_q_tokens = q_lims[nq];
  p.n_tokens = store ? n_tokens : 0;
  p.n_rows = store ? n_rows : 0;
  p.id_offset = id_offset;
  p.C = C;
  return rerank_tail("latec_rerank", "late_score_compressed_kernel", p, nq, max_tq, d_candidates, R, k, d_out_scores, d_out_ids,
                     d_out_raw, d_workspace, workspace_bytes, stream, [&](int qb, int chunks, hipStream_t st) {
                       if (nbits == 2) launch_score_compressed_qb<2>(p, qb, nq, chunks, st);
                       else launch_score_compressed_qb<4>(p, qb, nq, chunks, st);
                     });
}

}  // extern "C"
