// Late interaction, training side (include/sskd_amd.h, "Late interaction: training through MaxSim"): the gradient of
//   score(q, c) = sum_i max_t <q_i, d_cand[q,c],t>
// given the argmax that sskd_latet_maxsim_fwd (late.hip) reports, and the backward of the token normalisation.
//
//   dQ[q, i, :] = sum_c g[q, c] * d[cand[q, c], arg[q, c, i], :]              late_maxsim_bwd_q_kernel, a gather
//   dD[j, t, :] = sum_{(q, c, i) that selected (j, t)} g[q, c] * q[q, i, :]   late_maxsim_bwd_d_kernel, per destination row
//
// Both are one wave per output row: lane l < 48 owns columns 8 l .. 8 l + 7, reads one 16-byte piece of every source row
// (the wave reads the whole 768-byte row at once) and keeps 8 fp32 accumulators.  Per column the sum is ONE order -
// acc = +0.0f, then acc = acc + g * x over the contributions ascending, multiply and add rounded separately (contraction
// is off in these kernels; tests/late_train_cases.py restates them bit for bit) - so there are no atomics and a gradient's
// bits do not depend on the launch.  A row gather is latency-bound (768 bytes per dependent address), so the loads of
// L_INFLIGHT contributions are issued before the first add waits.
#include "late_device.h"

namespace {

constexpr int L_INFLIGHT = 8;               // source rows whose loads are in flight together

__device__ inline void store8(float* dst, const float (&a)[8]) {
  reinterpret_cast<float4*>(dst)[0] = make_float4(a[0], a[1], a[2], a[3]);
  reinterpret_cast<float4*>(dst)[1] = make_float4(a[4], a[5], a[6], a[7]);
}

struct GradParams {
  const uint4* q_tokens;     // [n_q_tokens, 48]
  const int64_t* q_lims;     // [nq + 1]
  const uint4* d_tokens;     // [n_d_tokens, 48]
  const int64_t* d_lims;     // [nd + 1]
  const int64_t* cand;       // [nq, R]
  const int32_t* arg;        // [nq, R, tq_stride]
  const float* g;            // [nq, R]
  const int64_t* order;      // [E]            (bwd_d)
  const int64_t* seg;        // [n_d_tokens + 1] (bwd_d)
  float* out;                // dQ [n_q_tokens, 384] or dD [n_d_tokens, 384]
  int64_t n_q_tokens, n_d_tokens, nd, E;
  int nq, R, tq_stride;
};

// One wave per (query, query token): grid (nq, ceil(tq_stride / 4)).  arg, cand and g are wave-uniform.  A pair
// contributes when arg >= 0 AND the pair still names a document that has that token (no address from unchecked data);
// the g of any other pair is never read.
__global__ __launch_bounds__(L_THREADS) void late_maxsim_bwd_q_kernel(const GradParams p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x, i = blockIdx.y * L_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int64_t q0, tq;
  query_range(p.q_lims, p.n_q_tokens, q, q0, tq);
  if (i >= tq || i >= p.tq_stride) return;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const int64_t pair0 = (int64_t)q * p.R;
  for (int c0 = 0; c0 < p.R; c0 += L_INFLIGHT) {
    uint4 v[L_INFLIGHT];
    float g[L_INFLIGHT];
    bool ok[L_INFLIGHT];
#pragma unroll
    for (int u = 0; u < L_INFLIGHT; ++u) {
      const int c = c0 + u;
      ok[u] = false;
      g[u] = 0.f;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      int64_t row = 0;
      if (c < p.R) {
        const int a = p.arg[(pair0 + c) * p.tq_stride + i];
        const int64_t id = p.cand[pair0 + c];
        if (a >= 0 && id >= 0 && id < p.nd) {
          const int64_t lo = p.d_lims[id], hi = p.d_lims[id + 1];
          if (lo >= 0 && hi <= p.n_d_tokens && a < hi - lo) {
            ok[u] = true;
            row = lo + a;
          }
        }
      }
      if (ok[u]) {
        g[u] = p.g[pair0 + c];
        if (lane < L_ROW_VEC) v[u] = p.d_tokens[row * L_ROW_VEC + lane];
      }
    }
#pragma unroll
    for (int u = 0; u < L_INFLIGHT; ++u) {
      if (ok[u]) {
        float x[8];
        widen8(v[u], x);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float t = g[u] * x[j];
          acc[j] = acc[j] + t;
        }
      }
    }
  }
  if (lane < L_ROW_VEC) store8(p.out + (q0 + i) * DIM + 8 * lane, acc);
}

// One wave per document token row r: contributions order[seg[r]] .. order[seg[r + 1] - 1] (ascending e, the host's stable
// sort), e = (q R + c) tq_stride + i.  A row nobody selected stores zeros.  seg and order are the host layer's; every
// index taken from them is checked before it becomes an address.
__global__ __launch_bounds__(L_THREADS) void late_maxsim_bwd_d_kernel(const GradParams p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * L_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= p.n_d_tokens) return;
  int64_t lo = p.seg[r], hi = p.seg[r + 1];
  if (lo < 0) lo = 0;
  if (hi > p.E) hi = p.E;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const int64_t per_q = (int64_t)p.R * p.tq_stride;
  for (int64_t s0 = lo; s0 < hi; s0 += L_INFLIGHT) {
    uint4 v[L_INFLIGHT];
    float g[L_INFLIGHT];
    bool ok[L_INFLIGHT];
#pragma unroll
    for (int u = 0; u < L_INFLIGHT; ++u) {
      ok[u] = false;
      g[u] = 0.f;
      v[u] = make_uint4(0u, 0u, 0u, 0u);
      int64_t row = 0, pair = 0;
      if (s0 + u < hi) {
        const int64_t e = p.order[s0 + u];
        if (e >= 0 && e < p.E) {
          const int64_t q = e / per_q, rem = e % per_q;
          const int64_t i = rem % p.tq_stride;
          const int64_t q0 = p.q_lims[q], tq = p.q_lims[q + 1] - q0;
          if (q0 >= 0 && tq >= 0 && q0 + tq <= p.n_q_tokens && i < tq) {
            ok[u] = true;
            row = q0 + i;
            pair = q * p.R + rem / p.tq_stride;
          }
        }
      }
      if (ok[u]) {
        g[u] = p.g[pair];
        if (lane < L_ROW_VEC) v[u] = p.q_tokens[row * L_ROW_VEC + lane];
      }
    }
#pragma unroll
    for (int u = 0; u < L_INFLIGHT; ++u) {
      if (ok[u]) {
        float x[8];
        widen8(v[u], x);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float t = g[u] * x[j];
          acc[j] = acc[j] + t;
        }
      }
    }
  }
  if (lane < L_ROW_VEC) store8(p.out + r * DIM + 8 * lane, acc);
}

// Backward of late_pack_kernel (late.hip), one wave per (text, position), the same lanes and columns.  With x the raw
// hidden row, n = max(sqrt(ss), 1e-12f) the pack's own value (same chain, same butterfly) and y = x / n in fp32 (the
// bf16 rounding of the stored token is straight-through):
//   dot = sum_c g_c y_c   (lane chain over its 8 columns ascending from +0.0f, multiply then add; lanes 48 .. 63 hold
//                          +0.0f; xor butterfly 32 .. 1)
//   dh_c = (g_c - y_c * dot) / n, every operation rounded on its own, then to bf16 to nearest even.
// Positions >= the length (or whose store row does not exist) get zeros: every element of dHidden is written.
__global__ __launch_bounds__(L_THREADS) void late_pack_bwd_kernel(const uint16_t* __restrict__ hidden, const int32_t* __restrict__ lengths,
                                                                  const int64_t* __restrict__ offsets, int B, int S, int64_t n_tokens,
                                                                  const float* __restrict__ dtok, uint16_t* __restrict__ dhidden) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * L_WAVES + (threadIdx.x >> 6);
  if (tok >= (int64_t)B * S) return;
  const int b = (int)(tok / S), s = (int)(tok % S);
  const int64_t row = offsets[b] + s;
  if (s >= lengths[b] || row < 0 || row >= n_tokens) {
    if (lane < L_ROW_VEC) *reinterpret_cast<uint4*>(dhidden + tok * DIM + 8 * lane) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  float x[8], g[8];
  if (lane < L_ROW_VEC) {
    widen8(*reinterpret_cast<const uint4*>(hidden + tok * DIM + 8 * lane), x);
    const float4 g0 = reinterpret_cast<const float4*>(dtok + row * DIM + 8 * lane)[0];
    const float4 g1 = reinterpret_cast<const float4*>(dtok + row * DIM + 8 * lane)[1];
    g[0] = g0.x; g[1] = g0.y; g[2] = g0.z; g[3] = g0.w;
    g[4] = g1.x; g[5] = g1.y; g[6] = g1.z; g[7] = g1.w;
  }
  const float ss = row_sum_squares(x, lane < L_ROW_VEC);   // exact products: the pack's chain
  const float n = fmaxf(__builtin_sqrtf(ss), 1e-12f);
  float y[8];
  float d = 0.f;
  if (lane < L_ROW_VEC) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      y[j] = x[j] / n;
      const float t = g[j] * y[j];
      d = d + t;
    }
  }
  const float dot = wave_sum(d);
  if (lane < L_ROW_VEC) {
    float dh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = y[j] * dot;
      const float num = g[j] - t;
      dh[j] = num / n;
    }
    *reinterpret_cast<uint4*>(dhidden + tok * DIM + 8 * lane) = pack8(dh);
  }
}

}  // namespace

extern "C" {

int sskd_latet_maxsim_bwd_q(const void* d_d_tokens, const int64_t* d_d_lims, int64_t nd, int64_t n_d_tokens, const int64_t* q_lims,
                           const int64_t* d_q_lims, int nq, int64_t n_q_tokens, const int64_t* d_candidates, int R,
                           const int32_t* d_arg, int tq_stride, const float* d_g, float* d_dq, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(nq >= 0 && R >= 0, "late_maxsim_bwd_q: nq=%d, R=%d must be >= 0", nq, R);
  SSKD_REQUIRE(R <= L_R_MAX, "late_maxsim_bwd_q: R=%d above %d", R, L_R_MAX);
  SSKD_REQUIRE(nd >= 0 && n_d_tokens >= 0 && n_q_tokens >= 0, "late_maxsim_bwd_q: nd, n_d_tokens and n_q_tokens must be >= 0");
  if (nq == 0 || R == 0) return SSKD_OK;
  if (check_query_lims("late_maxsim_bwd_q", q_lims, nq, n_q_tokens, tq_stride) < 0) return SSKD_ERR_INVALID;
  SSKD_REQUIRE(d_q_lims && d_candidates && d_arg && d_g && d_dq, "late_maxsim_bwd_q: null pointer");
  SSKD_REQUIRE(nd == 0 || n_d_tokens == 0 || (d_d_tokens && d_d_lims), "late_maxsim_bwd_q: null document tokens");
  SSKD_REQUIRE(aligned16(d_d_tokens) && aligned16(d_dq), "late_maxsim_bwd_q: token matrix and dQ must be 16-byte aligned");
  GradParams p{};
  p.q_lims = d_q_lims;
  p.d_tokens = static_cast<const uint4*>(d_d_tokens);
  p.d_lims = d_d_lims;
  p.cand = d_candidates;
  p.arg = d_arg;
  p.g = d_g;
  p.out = d_dq;
  p.n_q_tokens = n_q_tokens;
  p.n_d_tokens = (d_d_tokens && d_d_lims) ? n_d_tokens : 0;
  p.nd = (d_d_tokens && d_d_lims) ? nd : 0;
  p.nq = nq;
  p.R = R;
  p.tq_stride = tq_stride;
  hipLaunchKernelGGL(late_maxsim_bwd_q_kernel, dim3((unsigned)nq, (unsigned)(tq_stride / L_WAVES)), dim3(L_THREADS), 0,
                     sskd::as_stream(stream), p);
  return sskd::check_launch("late_maxsim_bwd_q_kernel");
}

int sskd_latet_maxsim_bwd_d(const void* d_q_tokens, const int64_t* q_lims, const int64_t* d_q_lims, int nq, int64_t n_q_tokens, int R,
                           int tq_stride, const int64_t* d_order, const int64_t* d_seg, int64_t n_d_tokens, const float* d_g,
                           float* d_dd, void* stream) {
  // every check comes before the first HIP call
  SSKD_REQUIRE(nq >= 0 && R >= 0, "late_maxsim_bwd_d: nq=%d, R=%d must be >= 0", nq, R);
  SSKD_REQUIRE(R <= L_R_MAX, "late_maxsim_bwd_d: R=%d above %d", R, L_R_MAX);
  SSKD_REQUIRE(n_d_tokens >= 0 && n_q_tokens >= 0, "late_maxsim_bwd_d: n_d_tokens and n_q_tokens must be >= 0");
  if (nq == 0 || R == 0 || n_d_tokens == 0) return SSKD_OK;
  if (check_query_lims("late_maxsim_bwd_d", q_lims, nq, n_q_tokens, tq_stride) < 0) return SSKD_ERR_INVALID;
  SSKD_REQUIRE(d_q_tokens && d_q_lims && d_order && d_seg && d_g && d_dd, "late_maxsim_bwd_d: null pointer");
  SSKD_REQUIRE(aligned16(d_q_tokens) && aligned16(d_dd), "late_maxsim_bwd_d: token matrix and dD must be 16-byte aligned");
  SSKD_REQUIRE(n_d_tokens / L_WAVES < (int64_t)INT32_MAX, "late_maxsim_bwd_d: n_d_tokens too large");
  GradParams p{};
  p.q_tokens = static_cast<const uint4*>(d_q_tokens);
  p.q_lims = d_q_lims;
  p.g = d_g;
  p.order = d_order;
  p.seg = d_seg;
  p.out = d_dd;
  p.n_q_tokens = n_q_tokens;
  p.n_d_tokens = n_d_tokens;
  p.E = (int64_t)nq * R * tq_stride;
  p.nq = nq;
  p.R = R;
  p.tq_stride = tq_stride;
  hipLaunchKernelGGL(late_maxsim_bwd_d_kernel, dim3((unsigned)sskd::ceil_div(n_d_tokens, L_WAVES)), dim3(L_THREADS), 0,
                     sskd::as_stream(stream), p);
  return sskd::check_launch("late_maxsim_bwd_d_kernel");
}

int sskd_latet_pack_tokens_bwd(const void* d_hidden, const int32_t* d_lengths, const int64_t* d_offsets, int B, int S, int H,
                              int64_t n_tokens, const float* d_dtok, void* d_dhidden, void* stream) {
  if (H != DIM) return sskd::fail(SSKD_ERR_UNSUPPORTED, "late_pack_tokens_bwd: H=%d, the late-interaction kernels serve %d", H, DIM);
  SSKD_REQUIRE(B >= 0 && S >= 1, "late_pack_tokens_bwd: needs B >= 0 and S >= 1 (B=%d, S=%d)", B, S);
  SSKD_REQUIRE(n_tokens >= 0, "late_pack_tokens_bwd: n_tokens < 0");
  if (B == 0) return SSKD_OK;
  SSKD_REQUIRE(d_hidden && d_lengths && d_offsets && d_dhidden && (d_dtok || n_tokens == 0), "late_pack_tokens_bwd: null pointer");
  SSKD_REQUIRE(aligned16(d_hidden) && aligned16(d_dtok) && aligned16(d_dhidden),
               "late_pack_tokens_bwd: hidden states and gradients must be 16-byte aligned");
  const int64_t waves = (int64_t)B * S;
  SSKD_REQUIRE(waves / L_WAVES < (int64_t)INT32_MAX, "late_pack_tokens_bwd: B * S too large");
  hipLaunchKernelGGL(late_pack_bwd_kernel, dim3((unsigned)sskd::ceil_div(waves, L_WAVES)), dim3(L_THREADS), 0, sskd::as_stream(stream),
                     static_cast<const uint16_t*>(d_hidden), d_lengths, d_offsets, B, S, n_tokens, d_dtok,
                     static_cast<uint16_t*>(d_dhidden));
  return sskd::check_launch("late_pack_bwd_kernel");
}

}  // extern "C"
