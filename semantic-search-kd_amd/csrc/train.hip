// Student forward / backward step (BASELINE cfg 4) and the dimension-generic encoder forward.
//
// Replaces what the reference's KD training step runs inside torch autograd for
// StudentModel.encode_with_gradients (reference: src/kd/train.py:176-210: two encodes with
// gradients -> q @ d.T -> CombinedKDLoss -> backward): a post-LN BERT encoder forward that SAVES
// its activations, and the matching backward producing fp32 parameter gradients.  bf16
// activations and MFMA operands, fp32 accumulation, fp32 LayerNorm / softmax statistics, fp32
// gradients.  Dimension-generic (hidden <= 1024, any head count / width that are multiples of 32):
// the teacher cross-encoder (XLM-R-large shape) runs the same forward.
//
// Attention takes one of three routes, decided once per call by check() (Dims::attn):
//   inference (training == 0): the fused forward.  It serves head widths 32, 64 and 128 with
//     S * DH <= 36 864 (ATT_FWD_MAX_SDH; width 128: S <= 288); any other shape is refused;
//   training, attention_bwd_supported(S, DH): the fused forward / backward pair (keeps lse);
//   training, any other shape: the unfused path (scores materialised), every width that is a multiple of 32.
// A call is validated as a whole - shape, route, workspace, every pointer it will read - and only then enqueued.
//
// Activations are ROW-MAJOR [tokens, features] here (the inference encoder's fragment order is
// tied to hidden 384).  Every GEMM is the one NT kernel of generic.hip; operands whose reduction
// dimension is not contiguous are transposed first by a bandwidth-bound kernel.
#include "generic.h"

#include <cmath>
#include <vector>

using namespace sskd_generic;

namespace {

enum class Attn { FusedInference, FusedTraining, Unfused };

struct Dims {
  int B, S, H, NH, DH, F, L;
  int64_t M;
  bool training;  // false: nothing is kept for a backward pass (fused attention, GELU in the GEMM epilogue)
  Attn attn;      // a function of (training, S, DH) alone: the halves of a batch take the route of the whole
};

struct LayerSaved {
  bf16_t *qkv, *P, *ctx, *z1, *x1, *u, *hmid, *z2, *x2;
  float *mean1, *rstd1, *mean2, *rstd2;
  float* lse;  // Attn::FusedTraining: log-sum-exp per (row, head, query) instead of P
};

struct Saved {
  bf16_t *z0, *x0;
  float *mean0, *rstd0, *pooled;
  LayerSaved* layer;  // host array
  // scratch
  bf16_t *tH0, *tH1, *tH2, *vt, *tF0, *tP0, *tP1, *tA, *tB, *t3H;
  size_t bytes;
};

// carve the workspace; `layers_out` must hold cfg->layers entries (host memory)
Saved carve(void* base, const Dims& d, LayerSaved* layers_out) {
  sskd::Carver c(base);
  auto take_b = [&](size_t elems) { return c.take<bf16_t>(elems); };
  auto take_f = [&](size_t elems) { return c.take<float>(elems); };
  const size_t M = (size_t)d.M, MH = M * d.H, MF = M * d.F, PP = (size_t)d.B * d.NH * d.S * d.S;
  const bool training = d.training, unfused = d.attn == Attn::Unfused;
  Saved s{};
  s.layer = layers_out;
  s.z0 = take_b(MH);
  s.x0 = take_b(MH);
  s.mean0 = take_f(M);
  s.rstd0 = take_f(M);
  s.pooled = take_f((size_t)d.B * d.H);
  const int nl = training ? d.L : (d.L > 0 ? 1 : 0);  // inference re-uses one layer's buffers
  for (int l = 0; l < nl; ++l) {
    LayerSaved& ls = layers_out[l];
    ls.qkv = take_b(3 * MH);
    ls.P = unfused ? take_b(PP) : nullptr;  // fused attention: no score matrix
    ls.lse = d.attn == Attn::FusedTraining ? take_f((size_t)d.B * d.NH * d.S) : nullptr;
    ls.ctx = take_b(MH);
    ls.z1 = training ? take_b(MH) : nullptr;
    ls.x1 = take_b(MH);
    ls.u = training ? take_b(MF) : nullptr;     // inference: GELU in the GEMM epilogue
    ls.hmid = take_b(MF);
    ls.z2 = training ? take_b(MH) : nullptr;
    ls.x2 = take_b(MH);
    ls.mean1 = take_f(M);
    ls.rstd1 = take_f(M);
    ls.mean2 = take_f(M);
    ls.rstd2 = take_f(M);
  }
  if (!training && d.L > 1) {
    // ping-pong the layer output so that layer l reads x2 of layer l-1 while writing its own
    for (int l = 1; l < d.L; ++l) {
      layers_out[l] = layers_out[0];
    }
    bf16_t* alt = take_b(MH);
    for (int l = 1; l < d.L; l += 2) layers_out[l].x2 = alt;
  }
  s.tH0 = take_b(MH);
  s.vt = training ? take_b(MH) : nullptr;
  if (training) {
    s.tH1 = take_b(MH);
    s.tH2 = take_b(MH);
    s.tF0 = take_b(MF);
    s.tP0 = unfused ? take_b(PP) : nullptr;
    s.tP1 = unfused ? take_b(PP) : nullptr;
    const size_t wide = (size_t)(3 * d.H > d.F ? 3 * d.H : d.F);
    s.tA = take_b(wide * M);
    s.tB = take_b((size_t)(d.H > d.F ? d.H : d.F) * M);
    s.t3H = take_b(3 * MH);
  }
  s.bytes = c.bytes();
  return s;
}

// config, shape and attention route of a call: everything that does not depend on the caller's pointers
int check(const sskd_generic_config* cfg, int B, int S, int training, Dims* d) {
  SSKD_REQUIRE(cfg, "generic encoder: null config / weights");
  SSKD_REQUIRE(cfg->hidden > 0 && cfg->hidden % 32 == 0 && cfg->hidden <= 1024,
               "generic encoder: hidden=%d must be a multiple of 32, at most 1024", cfg->hidden);
  SSKD_REQUIRE(cfg->heads > 0 && cfg->hidden % cfg->heads == 0 && (cfg->hidden / cfg->heads) % 32 == 0,
               "generic encoder: head width %d/%d must be a multiple of 32", cfg->hidden, cfg->heads);
  SSKD_REQUIRE(cfg->intermediate > 0 && cfg->intermediate % 32 == 0, "generic encoder: intermediate must be a multiple of 32");
  SSKD_REQUIRE(cfg->layers >= 0 && cfg->vocab_size > 0, "generic encoder: bad layers / vocab");
  SSKD_REQUIRE(B >= 0 && S >= 32 && S % 32 == 0 && S <= 512, "generic encoder: S=%d must be a multiple of 32 in [32, 512]", S);
  SSKD_REQUIRE(S + cfg->pos_offset <= cfg->max_positions, "generic encoder: S=%d + offset %d exceeds max_positions %d", S,
               cfg->pos_offset, cfg->max_positions);
  d->B = B;
  d->S = S;
  d->H = cfg->hidden;
  d->NH = cfg->heads;
  d->DH = cfg->hidden / cfg->heads;
  d->F = cfg->intermediate;
  d->L = cfg->layers;
  d->M = (int64_t)B * S;
  d->training = training != 0;
  d->attn = !d->training ? Attn::FusedInference : attention_bwd_supported(S, d->DH) ? Attn::FusedTraining : Attn::Unfused;
  if (d->attn == Attn::FusedInference && B > 0) {   // what launch_attention_fwd would refuse, before anything is enqueued
    const int DH = d->DH;
    SSKD_REQUIRE(DH == 32 || DH == 64 || DH == 128, "attention_fwd: head width %d not in {32, 64, 128}", DH);
    SSKD_REQUIRE(attention_fwd_supported(S, DH), "attention_fwd: S=%d x head width %d does not fit in LDS (S * DH <= %d)", S,
                 DH, ATT_FWD_MAX_SDH);
  }
  return SSKD_OK;
}

// C[M, N] = A[M, K] B[N, K]^T (+ bias), plain 2-D; act = 1: erf-GELU in the epilogue (bf16 output)
int gemm(const bf16_t* A, int64_t lda, const bf16_t* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int N, int K,
         const float* bias, bool c_f32, bool acc, hipStream_t st, int act = 0) {
  GemmArgs g{};
  g.A = A;
  g.B = B;
  g.C = C;
  g.bias = bias;
  g.M = (int)M;
  g.N = N;
  g.K = K;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.batch1 = g.batch2 = 1;
  g.alpha = 1.0f;
  g.c_is_f32 = c_f32;
  g.accumulate = acc;
  g.act = act;
  // weight-gradient products (few output tiles, K = every token of the step): cut K over enough
  // workgroups to fill the chip; the slices meet through fp32 atomics
  if (acc && c_f32 && !bias) {
    const int64_t tiles = sskd::ceil_div(M, 128) * sskd::ceil_div(N, 128);
#ifndef SSKD_SPLITK_TARGET
#define SSKD_SPLITK_TARGET 256  // one workgroup per CU: every extra slice adds a 128 x 128 tile of device-scope atomics (1024: 104 us, 256: 65 us for 384 x 384 x 65 k)
#endif
    int split = (int)(SSKD_SPLITK_TARGET / (tiles > 0 ? tiles : 1));
    const int max_split = K / 256;  // at least 256 of K per slice
    if (split > max_split) split = max_split;
    g.split_k = split > 1 ? split : 1;
  }
  return launch_gemm_nt(g, st);
}

int transpose2d(const bf16_t* in, int64_t R, int C, int64_t ld_in, bf16_t* out, int64_t ld_out, hipStream_t st,
                float* colsum = nullptr) {
  TransposeArgs t{};
  t.colsum = colsum;
  t.in = in;
  t.out = out;
  t.R = (int)R;
  t.C = C;
  t.ld_in = ld_in;
  t.ld_out = ld_out;
  t.batch1 = t.batch2 = 1;
  return launch_transpose(t, st);
}

// dW[M, N] += dY[T, M]^T X[T, N] and db[M] += column sums of dY.  The student's shapes go to the TN kernel, which
// reads both operands as they lie in memory; others are transposed into tA / tB and take the NT kernel.
int weight_grad(const bf16_t* dY, int M, const bf16_t* X, int N, int64_t T, float* dW, float* db, bf16_t* tA, bf16_t* tB,
                hipStream_t st) {
  if (gemm_tn_supported(T, M, N, M, N)) {
    if (db) {  // nullptr: the kernel that produced dY already summed its columns
      int rc = launch_colsum(dY, T, M, M, db, st);
      if (rc != SSKD_OK) return rc;
    }
    return launch_gemm_tn(dY, M, X, N, dW, N, T, M, N, st);
  }
  int rc = transpose2d(dY, T, M, M, tA, T, st, db);  // [M, T]; db = column sums on the way
  if (rc != SSKD_OK) return rc;
  rc = transpose2d(X, T, N, N, tB, T, st);            // [N, T]
  if (rc != SSKD_OK) return rc;
  return gemm(tA, T, tB, T, dW, N, M, N, (int)T, nullptr, true, true, st);
}

#define TRY(expr)                     \
  do {                                \
    int rc_ = (expr);                 \
    if (rc_ != SSKD_OK) return rc_;   \
  } while (0)

// ---- unfused attention: one product per (batch row, head) over strided views of the step's buffers ----
// Element (r, c) of batch row b, head h lies at p[b * sb + h * sh + r * ld + c].
struct View {
  bf16_t* p;
  int64_t ld, sb, sh;
};
// head h = columns [h * DH, (h + 1) * DH) of a row-major [B * S, width] matrix (a third of qkv, ctx)
View head_cols(const Dims& d, bf16_t* p, int width) { return {p, width, (int64_t)d.S * width, d.DH}; }
// head h = rows [h * DH, (h + 1) * DH) of a transposed [B, rows, S] buffer
View head_rows(const Dims& d, bf16_t* p, int rows) { return {p, d.S, (int64_t)rows * d.S, (int64_t)d.DH * d.S}; }
// a [B, heads, S, S] matrix (scores, probabilities and their gradients)
View head_sq(const Dims& d, bf16_t* p) { return {p, d.S, (int64_t)d.NH * d.S * d.S, (int64_t)d.S * d.S}; }

// C_bh[M, N] = A_bh[M, K] B_bh[N, K]^T for every (batch row, head)
int head_gemm(const Dims& d, View A, View B, View C, int M, int N, int K, hipStream_t st) {
  GemmArgs g{};
  g.A = A.p, g.lda = A.ld, g.sA1 = A.sb, g.sA2 = A.sh;
  g.B = B.p, g.ldb = B.ld, g.sB1 = B.sb, g.sB2 = B.sh;
  g.C = C.p, g.ldc = C.ld, g.sC1 = C.sb, g.sC2 = C.sh;
  g.M = M, g.N = N, g.K = K;
  g.batch1 = d.B, g.batch2 = d.NH;
  g.alpha = 1.0f;
  return launch_gemm_nt(g, st);
}

// out_bh[C, R] = in_bh[R, C]^T for every (batch row, head); heads == 1: whole batch rows, the head strides are not passed
int head_transpose(const Dims& d, int heads, View in, View out, int R, int C, hipStream_t st) {
  TransposeArgs t{};
  t.in = in.p, t.ld_in = in.ld, t.sI1 = in.sb, t.sI2 = heads > 1 ? in.sh : 0;
  t.out = out.p, t.ld_out = out.ld, t.sO1 = out.sb, t.sO2 = heads > 1 ? out.sh : 0;
  t.R = R, t.C = C;
  t.batch1 = d.B, t.batch2 = heads;
  return launch_transpose(t, st);
}

int attention_unfused_fwd(const Dims& d, const int32_t* mask, LayerSaved& ls, Saved& sv, hipStream_t st) {
  const int S = d.S, DH = d.DH, H = d.H;
  const View Q = head_cols(d, ls.qkv, 3 * H), K = head_cols(d, ls.qkv + H, 3 * H), V = head_cols(d, ls.qkv + 2 * H, 3 * H);
  const View P = head_sq(d, ls.P), Vt = head_rows(d, sv.vt, H);
  TRY(head_gemm(d, Q, K, P, S, S, DH, st));                                                  // P = Q K^T
  TRY(launch_softmax_fwd(ls.P, mask, d.B, d.NH, S, 1.0f / sqrtf((float)DH), st));            // P = softmax(scale P + mask)
  TRY(head_transpose(d, d.NH, V, Vt, S, DH, st));                                            // V^T [DH, S]
  return head_gemm(d, P, Vt, head_cols(d, ls.ctx, H), S, DH, S, st);                         // ctx = P V
}

// dqkv [B * S, 3H] = dQ | dK | dV from dctx; uses tP0, tP1 [B, heads, S, S], vt [B, H, S] and tA [B, 3H, S]
int attention_unfused_bwd(const Dims& d, const LayerSaved& ls, Saved& sv, bf16_t* dctx, bf16_t* dqkv, hipStream_t st) {
  const int S = d.S, DH = d.DH, H = d.H, NH = d.NH;
  const View V = head_cols(d, ls.qkv + 2 * H, 3 * H), dO = head_cols(d, dctx, H);
  const View dQ = head_cols(d, dqkv, 3 * H), dK = head_cols(d, dqkv + H, 3 * H), dV = head_cols(d, dqkv + 2 * H, 3 * H);
  const View P = head_sq(d, ls.P), dP = head_sq(d, sv.tP0), T = head_sq(d, sv.tP1);   // dP becomes dS in place
  const View dOt = head_rows(d, sv.vt, H);                                             // dctx^T [B, H, S]
  const View Qt = head_rows(d, sv.tA, 3 * H), Kt = head_rows(d, sv.tA + (int64_t)H * S, 3 * H);   // of qkv^T [B, 3H, S]
  TRY(head_gemm(d, dO, V, dP, S, S, DH, st));                                                // dP = dctx V^T
  TRY(head_transpose(d, NH, P, T, S, S, st));                                                // T = P^T
  TRY(head_transpose(d, 1, dO, dOt, S, H, st));                                              // dctx^T, every head at once
  TRY(head_gemm(d, T, dOt, dV, S, DH, S, st));                                               // dV = P^T dctx
  TRY(launch_softmax_bwd(sv.tP0, ls.P, (int64_t)d.B * NH * S, S, 1.0f / sqrtf((float)DH), st));   // dS = scale P (dP - rowsum(dP P))
  TRY(head_transpose(d, 1, head_cols(d, ls.qkv, 3 * H), Qt, S, 3 * H, st));                  // Q^T, K^T, V^T of every row
  TRY(head_gemm(d, dP, Kt, dQ, S, DH, S, st));                                               // dQ = dS K
  TRY(head_transpose(d, NH, dP, T, S, S, st));                                               // T = dS^T
  return head_gemm(d, T, Qt, dK, S, DH, S, st);                                              // dK = dS^T Q
}

// ---- forward of one layer: x -> ls.x2, saving what the backward needs when training -------------------------
int layer_forward(const Dims& d, const sskd_generic_layer_weights& lw, float eps, const bf16_t* x, const int32_t* mask,
                  LayerSaved& ls, Saved& sv, hipStream_t st) {
  const int H = d.H, F = d.F;
  const int64_t M = d.M;
  const bool keep = d.training;   // inference: no z / mean / rstd saved, GELU inside FFN1's epilogue (no u)
  TRY(gemm(x, H, static_cast<const bf16_t*>(lw.wqkv), H, ls.qkv, 3 * H, M, 3 * H, H, lw.bqkv, false, false, st));
  if (d.attn == Attn::Unfused)
    TRY(attention_unfused_fwd(d, mask, ls, sv, st));
  else   // scores, softmax and P V in one kernel (no [B, heads, S, S] matrix); lse is null on the inference route
    TRY(launch_attention_fwd(ls.qkv, mask, d.B, d.S, d.NH, d.DH, 1.0f / sqrtf((float)d.DH), ls.ctx, ls.lse, st));
  TRY(gemm(ls.ctx, H, static_cast<const bf16_t*>(lw.wo), H, sv.tH0, H, M, H, H, lw.bo, false, false, st));
  TRY(launch_add_ln_fwd(x, sv.tH0, lw.ln1_g, lw.ln1_b, eps, M, H, ls.x1, ls.z1, keep ? ls.mean1 : nullptr,
                        keep ? ls.rstd1 : nullptr, st));
  if (keep) {
    TRY(gemm(ls.x1, H, static_cast<const bf16_t*>(lw.w1), H, ls.u, F, M, F, H, lw.b1, false, false, st));
    TRY(launch_gelu_fwd(ls.u, ls.hmid, M * F, st));
  } else {
    TRY(gemm(ls.x1, H, static_cast<const bf16_t*>(lw.w1), H, ls.hmid, F, M, F, H, lw.b1, false, false, st, 1));
  }
  TRY(gemm(ls.hmid, F, static_cast<const bf16_t*>(lw.w2), F, sv.tH0, H, M, H, F, lw.b2, false, false, st));
  TRY(launch_add_ln_fwd(ls.x1, sv.tH0, lw.ln2_g, lw.ln2_b, eps, M, H, ls.x2, ls.z2, keep ? ls.mean2 : nullptr,
                        keep ? ls.rstd2 : nullptr, st));
  return SSKD_OK;
}

int forward_all(const sskd_generic_config* cfg, const sskd_generic_weights* w, const Dims& d, const int32_t* ids,
                const int32_t* mask, Saved& sv, hipStream_t st, const bf16_t** final_hidden) {
  TRY(launch_embed_fwd(ids, mask, static_cast<const bf16_t*>(w->word_emb), static_cast<const bf16_t*>(w->pos_emb),
                       static_cast<const bf16_t*>(w->type_emb), d.B, d.S, d.H, cfg->vocab_size, cfg->pos_offset, sv.z0, st));
  TRY(launch_add_ln_fwd(sv.z0, nullptr, w->emb_ln_g, w->emb_ln_b, cfg->layer_norm_eps, d.M, d.H, sv.x0, sv.z0, sv.mean0,
                        sv.rstd0, st));
  const bf16_t* x = sv.x0;
  for (int l = 0; l < d.L; ++l) {
    TRY(layer_forward(d, w->layers[l], cfg->layer_norm_eps, x, mask, sv.layer[l], sv, st));
    x = sv.layer[l].x2;
  }
  *final_hidden = x;
  return SSKD_OK;
}

// ---- backward of one layer: dx2 + dx2b (gradient of the layer output; dx2b optional) -> gradient of its input ----
// The result is sv.tH1 + sv.tH0 (the caller hands both to the next consumer).
int layer_backward(const Dims& d, const sskd_generic_layer_weights& lw, const sskd_generic_layer_grads& gw,
                   const bf16_t* x_in, const int32_t* mask, const LayerSaved& ls, Saved& sv, const bf16_t* dx2,
                   const bf16_t* dx2b, hipStream_t st) {
  const int H = d.H, F = d.F;
  const int64_t M = d.M;
  bf16_t* dz2 = sv.tH0;   // may alias dx2b: ln_bwd reads a row before it writes it
  TRY(launch_ln_bwd(dx2, ls.z2, ls.mean2, ls.rstd2, lw.ln2_g, M, H, dz2, gw.ln2_g, gw.ln2_b, st, gw.b2, dx2b));  // + db2
  // y = hmid W2^T + b2
  TRY(weight_grad(dz2, H, ls.hmid, F, M, gw.w2, nullptr, sv.tA, sv.tB, st));
  TRY(gemm(dz2, H, static_cast<const bf16_t*>(lw.w2_t), H, sv.tF0, F, M, F, H, nullptr, false, false, st));  // dhmid
  TRY(launch_gelu_bwd_colsum(ls.u, sv.tF0, sv.tF0, gw.b1, M, F, st));  // du (in place) + db1
  // u = x1 W1^T + b1
  TRY(weight_grad(sv.tF0, F, ls.x1, H, M, gw.w1, nullptr, sv.tA, sv.tB, st));
  bf16_t* dx1 = sv.tH1;
  TRY(gemm(sv.tF0, F, static_cast<const bf16_t*>(lw.w1_t), F, dx1, H, M, H, F, nullptr, false, false, st));
  bf16_t* dz1 = sv.tH0;   // aliases dz2, the residual branch of LN2 that this call adds to dx1 on the fly
  TRY(launch_ln_bwd(dx1, ls.z1, ls.mean1, ls.rstd1, lw.ln1_g, M, H, dz1, gw.ln1_g, gw.ln1_b, st, gw.bo, dz2));  // + dbo
  // attn_out = ctx Wo^T + bo
  TRY(weight_grad(dz1, H, ls.ctx, H, M, gw.wo, nullptr, sv.tA, sv.tB, st));
  bf16_t* dctx = sv.tH2;
  TRY(gemm(dz1, H, static_cast<const bf16_t*>(lw.wo_t), H, dctx, H, M, H, H, nullptr, false, false, st));
  // attention, per (batch row, head)
  bf16_t* dqkv = sv.t3H;
  if (d.attn == Attn::Unfused)
    TRY(attention_unfused_bwd(d, ls, sv, dctx, dqkv, st));
  else
    TRY(launch_attention_bwd(ls.qkv, mask, ls.ctx, dctx, ls.lse, d.B, d.S, d.NH, d.DH, 1.0f / sqrtf((float)d.DH), dqkv, st));
  // qkv = x Wqkv^T + bqkv.  The layer's input gradient is sv.tH1 + dz1 (dz1 = the residual branch of LN1, in sv.tH0):
  // the SUM is formed by the consumer - the LayerNorm backward that opens the layer below (or the embedding
  // LayerNorm's) - not by a pass of its own.
  TRY(weight_grad(dqkv, 3 * H, x_in, H, M, gw.wqkv, gw.bqkv, sv.tA, sv.tB, st));
  return gemm(dqkv, 3 * H, static_cast<const bf16_t*>(lw.wqkv_t), 3 * H, sv.tH1, H, M, H, 3 * H, nullptr, false, false, st);
}


// Cross-encoder head, one workgroup per sequence, ALL in fp32 (RobertaClassificationHead with one label):
//   logit = out_w . tanh(dense_w . h[<s>] + dense_b) + out_b
// A reranker's product is an ordering of near-equal logits, and the head is 2 H^2 FLOPs per pair (0.002 % of the
// encoder's work): there is nothing to gain from bf16 here, and the round-2 bf16 head (bf16 dense output, bf16
// tanh, bf16 weights) added its own rounding on top of the encoder's.  16 waves per workgroup; a wave computes dense
// rows w, w + 16, ... FOUR at a time (16-byte loads of whole fp32 rows, the <s> state in LDS; the first version - 4
// waves, one row and 4-byte loads at a time - was latency-bound at 1.4 ms per launch), then a fixed-order block
// reduction, so a logit is bit-reproducible from run to run.
constexpr int HEAD_WAVES = 16;
__global__ __launch_bounds__(HEAD_WAVES * 64) void teacher_head_kernel(const bf16_t* __restrict__ hidden, int S, int H,
                                                                      const float* __restrict__ dense_w,
                                                                      const float* __restrict__ dense_b,
                                                                      const float* __restrict__ out_w,
                                                                      const float* __restrict__ out_b, float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) float xs[1024];
  __shared__ float part[HEAD_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* h = hidden + (int64_t)b * S * H;   // token 0 of sequence b
  for (int c = tid; c < H; c += HEAD_WAVES * 64) xs[c] = (float)h[c];
  __syncthreads();
  float acc = 0.f;   // this wave's share of sum_r out_w[r] tanh(...), rows in increasing order
  const int H4 = H / 4;   // H % 32 == 0
  for (int r0 = 4 * wave; r0 < H; r0 += 4 * HEAD_WAVES) {
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < H4; c += 64) {
      const float4 x = reinterpret_cast<const float4*>(xs)[c];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 w = reinterpret_cast<const float4*>(dense_w + (int64_t)(r0 + u) * H)[c];
        d[u] = fmaf(w.x, x.x, fmaf(w.y, x.y, fmaf(w.z, x.z, fmaf(w.w, x.w, d[u]))));
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) d[u] += __shfl_xor(d[u], o);
      acc = fmaf(out_w[r0 + u], tanhf(d[u] + dense_b[r0 + u]), acc);   // identical in every lane of the wave
    }
  }
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int w = 0; w < HEAD_WAVES; ++w) s += part[w];
    logits[b] = s + out_b[0];
  }
}


// ---- the call path shared by the three entry points: size, validate, then run whole or as two halves ----

size_t workspace_one_part(const sskd_generic_config* cfg, int B, int S, int training) {
  Dims d{};
  if (B <= 0 || check(cfg, B, S, training, &d) != SSKD_OK) return 0;
  std::vector<LayerSaved> tmp((size_t)(d.L > 0 ? d.L : 1));
  return carve(nullptr, d, tmp.data()).bytes;
}

// Batches of >= 2 x 16 384 tokens run as TWO halves on two streams (sskd::run_parts_on_streams: a side stream forked from /
// joined into the caller's; rows do not interact).  The rule depends on (cfg, B, S, training) alone, so the forward that
// saves activations and the backward that reads them cut the batch - and the workspace - the same way.  Each half keeps
// its token count a multiple of 256 (the 256-row GEMM tiles).  Training splits only where every weight gradient goes
// through the atomically accumulating product (gemm_tn_supported): the halves add into the same gradient buffers.
// (Teacher: + 1.5 ... 2.7 % at 128 pairs x 256 tokens, tools/two_stream_teacher_probe.py; bit-identical.)
int generic_parts(const sskd_generic_config* cfg, int B, int S, int training) {
  if (sskd::forward_stream_parts() < 2 || !cfg || B < 2 || B % 2 != 0) return 1;
  const int64_t T = (int64_t)(B / 2) * S;
  if (T % 256 != 0 || T < 16384) return 1;
  if (training) {
    const int H = cfg->hidden, F = cfg->intermediate;
    if (!(gemm_tn_supported(T, 3 * H, H, 3 * H, H) && gemm_tn_supported(T, H, H, H, H) && gemm_tn_supported(T, F, H, F, H) &&
          gemm_tn_supported(T, H, F, H, F)))
      return 1;
  }
  return 2;
}
size_t part_stride(const sskd_generic_config* cfg, int B, int S, int training) {   // bytes between the halves
  return sskd::align256(workspace_one_part(cfg, B / 2, S, training));
}

size_t workspace_bytes_of(const sskd_generic_config* cfg, int B, int S, int training) {
  const size_t whole = workspace_one_part(cfg, B, S, training);
  if (whole == 0 || generic_parts(cfg, B, S, training) == 1) return whole;
  const size_t split = 2 * part_stride(cfg, B, S, training);
  return split > whole ? split : whole;
}

// What every entry point checks before it enqueues anything: config, shape and route (check), the workspace of the
// whole call, the weight table.  B == 0 passes with nothing else looked at: the caller returns.
int validate(const char* what, const sskd_generic_config* cfg, const sskd_generic_weights* w, int B, int S, int training,
             const void* d_workspace, size_t workspace_bytes, Dims* d) {
  SSKD_REQUIRE(cfg && w, "generic encoder: null config / weights");
  int rc = check(cfg, B, S, training, d);
  if (rc != SSKD_OK || B == 0) return rc;
  rc = sskd::require_workspace(what, d_workspace, workspace_bytes, workspace_bytes_of(cfg, B, S, training));
  if (rc != SSKD_OK) return rc;
  SSKD_REQUIRE(w->word_emb && w->pos_emb && w->type_emb && w->emb_ln_g && w->emb_ln_b && (cfg->layers == 0 || w->layers),
               "generic encoder: null weight pointer");
  return SSKD_OK;
}

// Runs a validated call: part(i, rows, workspace, stream) once over the whole batch, or over its two halves on two
// streams, each with its own slice of the workspace.  Part i starts at batch row i * rows.
template <class F>
int run_whole_or_halves(const sskd_generic_config* cfg, const Dims& d, void* d_workspace, hipStream_t st, F&& part) {
  if (generic_parts(cfg, d.B, d.S, d.training) == 1) return part(0, d.B, d_workspace, st);
  const size_t stride = part_stride(cfg, d.B, d.S, d.training);
  return sskd::run_parts_on_streams(2, st, [&](int i, hipStream_t s) {
    return part(i, d.B / 2, static_cast<char*>(d_workspace) + i * stride, s);
  });
}

// the buffers of `rows` batch rows of a validated call, laid out in `d_workspace`
struct Rows {
  Dims d;
  std::vector<LayerSaved> layers;
  Saved sv;
  Rows(const Dims& whole, int rows, void* d_workspace) : d(whole), layers((size_t)(whole.L > 0 ? whole.L : 1)) {
    d.B = rows;
    d.M = (int64_t)rows * d.S;
    sv = carve(d_workspace, d, layers.data());
  }
};

// d_dhidden: null = backward of the pooled forward (the pool backward turns d_dout into the hidden-state gradient in
// tH2); else the caller's gradient of the final hidden states, bf16 [rows, S, H], read IN PLACE: it is the dx2 of the top
// layer's first kernel (the embedding LayerNorm's when there are no layers), which is its only reader, and nothing of the
// backward writes outside the workspace and the gradient buffers.
int backward_rows(const sskd_generic_config* cfg, const sskd_generic_weights* w, const sskd_generic_grads* grads, Rows& r,
                  const int32_t* d_ids, const int32_t* d_mask, int normalize, const float* d_dout, const bf16_t* d_dhidden,
                  hipStream_t st) {
  const Dims& d = r.d;
  Saved& sv = r.sv;
  // gradient flowing into the current layer's output = dx + dxb (dxb: the residual share, null at the top)
  const bf16_t* dx = d_dhidden ? d_dhidden : sv.tH2;
  const bf16_t* dxb = nullptr;
  if (!d_dhidden) TRY(launch_pool_bwd(d_dout, sv.pooled, d_mask, d.B, d.S, d.H, normalize, sv.tH2, st));
  for (int l = d.L - 1; l >= 0; --l) {
    const bf16_t* x_in = l == 0 ? sv.x0 : sv.layer[l - 1].x2;
    TRY(layer_backward(d, w->layers[l], grads->layers[l], x_in, d_mask, sv.layer[l], sv, dx, dxb, st));
    // the layer's input gradient is tH1 + tH0: the layer below consumes both in its first kernel (which only READS tH1
    // and rewrites tH0 row by row), so nothing is copied and nothing is added in a pass of its own
    dx = sv.tH1;
    dxb = sv.tH0;
  }
  TRY(launch_ln_bwd(dx, sv.z0, sv.mean0, sv.rstd0, w->emb_ln_g, d.M, d.H, sv.tH0, grads->emb_ln_g, grads->emb_ln_b, st, nullptr, dxb));
  return launch_embed_bwd(d_ids, d_mask, sv.tH0, d.B, d.S, d.H, cfg->vocab_size, cfg->pos_offset, grads->word_emb,
                          grads->pos_emb, grads->type_emb, st);
}

}  // namespace

extern "C" {

size_t sskd_generic_workspace_bytes(const sskd_generic_config* cfg, int B, int S, int training) {
  return workspace_bytes_of(cfg, B, S, training);
}

int sskd_generic_forward(const sskd_generic_config* cfg, const sskd_generic_weights* w, const int32_t* d_ids,
                         const int32_t* d_mask, int B, int S, int training, int pool, int normalize, void* d_out,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
  Dims d{};
  int rc = validate("generic encoder", cfg, w, B, S, training, d_workspace, workspace_bytes, &d);
  if (rc != SSKD_OK || B == 0) return rc;
  SSKD_REQUIRE(d_ids && d_mask && d_out, "generic_forward: null pointer");
  const size_t out_row = pool ? (size_t)d.H * sizeof(float) : (size_t)S * d.H * sizeof(bf16_t);
  return run_whole_or_halves(cfg, d, d_workspace, sskd::as_stream(stream), [&](int i, int rows, void* ws, hipStream_t st) {
    Rows r(d, rows, ws);
    const int64_t row0 = (int64_t)i * rows;
    void* out = static_cast<char*>(d_out) + row0 * out_row;
    const int32_t* mask = d_mask + row0 * S;
    const bf16_t* fin = nullptr;
    TRY(forward_all(cfg, w, r.d, d_ids + row0 * S, mask, r.sv, st, &fin));
    if (pool) return launch_pool_fwd(fin, mask, rows, S, d.H, normalize, static_cast<float*>(out), r.sv.pooled, st);
    // raw final hidden states, bf16 [B, S, H]
    if (hipMemcpyAsync(out, fin, (size_t)r.d.M * d.H * sizeof(bf16_t), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return sskd::fail(SSKD_ERR_HIP, "generic_forward: copy of the hidden states failed");
    return SSKD_OK;
  });
}

// the two backward entries: exactly one of d_dout (pooled forward) and d_dhidden (hidden states) is given
static int generic_backward(const sskd_generic_config* cfg, const sskd_generic_weights* w, const sskd_generic_grads* grads,
                            const int32_t* d_ids, const int32_t* d_mask, int B, int S, int normalize, bool hidden,
                            const float* d_dout, const void* d_dhidden, void* d_workspace, size_t workspace_bytes, void* stream) {
  Dims d{};
  int rc = validate("generic encoder", cfg, w, B, S, 1, d_workspace, workspace_bytes, &d);
  if (rc != SSKD_OK || B == 0) return rc;
  SSKD_REQUIRE(grads && d_ids && d_mask && (hidden ? d_dhidden != nullptr : d_dout != nullptr), "generic_backward: null pointer");
  SSKD_REQUIRE(reinterpret_cast<uintptr_t>(d_dhidden) % 16 == 0, "generic_backward_hidden: d_dhidden must be 16-byte aligned");
  SSKD_REQUIRE(grads->word_emb && grads->pos_emb && grads->type_emb && grads->emb_ln_g && grads->emb_ln_b &&
                   (cfg->layers == 0 || grads->layers),
               "generic_backward: null gradient pointer");
  for (int l = d.L - 1; l >= 0; --l) {
    const sskd_generic_layer_weights& lw = w->layers[l];
    SSKD_REQUIRE(lw.wqkv_t && lw.wo_t && lw.w1_t && lw.w2_t, "generic_backward: layer %d lacks transposed weights", l);
  }
  const bf16_t* dhidden = static_cast<const bf16_t*>(d_dhidden);
  // two halves ADD into the same gradient buffers: every accumulation of the backward is atomic (generic_parts)
  return run_whole_or_halves(cfg, d, d_workspace, sskd::as_stream(stream), [&](int i, int rows, void* ws, hipStream_t st) {
    Rows r(d, rows, ws);
    const int64_t row0 = (int64_t)i * rows;
    return backward_rows(cfg, w, grads, r, d_ids + row0 * S, d_mask + row0 * S, normalize, hidden ? nullptr : d_dout + row0 * d.H,
                         hidden ? dhidden + row0 * S * d.H : nullptr, st);
  });
}

int sskd_generic_backward(const sskd_generic_config* cfg, const sskd_generic_weights* w, const sskd_generic_grads* grads,
                          const int32_t* d_ids, const int32_t* d_mask, int B, int S, int normalize, const float* d_dout,
                          void* d_workspace, size_t workspace_bytes, void* stream) {
  return generic_backward(cfg, w, grads, d_ids, d_mask, B, S, normalize, false, d_dout, nullptr, d_workspace, workspace_bytes, stream);
}

int sskd_generic_backward_hidden(const sskd_generic_config* cfg, const sskd_generic_weights* w, const sskd_generic_grads* grads,
                                 const int32_t* d_ids, const int32_t* d_mask, int B, int S, const void* d_dhidden,
                                 void* d_workspace, size_t workspace_bytes, void* stream) {
  return generic_backward(cfg, w, grads, d_ids, d_mask, B, S, 0, true, nullptr, d_dhidden, d_workspace, workspace_bytes, stream);
}

size_t sskd_teacher_workspace_bytes(const sskd_generic_config* cfg, int B, int S) {
  return workspace_bytes_of(cfg, B, S, 0);
}

// Cross-encoder score: generic encoder -> hidden state of token 0 (<s>) -> dense + tanh -> out_proj
// (XLMRobertaForSequenceClassification's RobertaClassificationHead with num_labels = 1); the head runs in fp32.
// A pair's score does not depend on its batch-mates, so the two-halves run is bit-identical to the whole.
int sskd_teacher_score(const sskd_generic_config* cfg, const sskd_generic_weights* w, const float* d_head_dense_w,
                       const float* d_head_dense_b, const float* d_head_out_w, const float* d_head_out_b,
                       const int32_t* d_ids, const int32_t* d_mask, int B, int S, float* d_logits, void* d_workspace,
                       size_t workspace_bytes, void* stream) {
  Dims d{};
  int rc = validate("teacher_score", cfg, w, B, S, 0, d_workspace, workspace_bytes, &d);
  if (rc != SSKD_OK || B == 0) return rc;
  SSKD_REQUIRE(d_head_dense_w && d_head_dense_b && d_head_out_w && d_head_out_b && d_ids && d_mask && d_logits,
               "teacher_score: null pointer");
  return run_whole_or_halves(cfg, d, d_workspace, sskd::as_stream(stream), [&](int i, int rows, void* ws, hipStream_t st) {
    Rows r(d, rows, ws);
    const int64_t row0 = (int64_t)i * rows;
    const bf16_t* fin = nullptr;
    TRY(forward_all(cfg, w, r.d, d_ids + row0 * S, d_mask + row0 * S, r.sv, st, &fin));
    hipLaunchKernelGGL(teacher_head_kernel, dim3(rows), dim3(HEAD_WAVES * 64), 0, st, fin, S, d.H, d_head_dense_w,
                       d_head_dense_b, d_head_out_w, d_head_out_b, d_logits + row0);
    return sskd::check_launch("teacher_head_kernel");
  });
}

// test hook: the NT GEMM by itself
int sskd_gemm_backend(int mode) {
  if (mode == 0 || mode == 1) sskd_generic::set_gemm_backend(mode);
  return sskd_generic::gemm_backend();
}

int sskd_gemm_nt_bf16(const void* d_a, const void* d_b, void* d_c, const float* d_bias, int M, int N, int K, int c_is_f32,
                      int accumulate, void* stream) {
  return gemm(static_cast<const bf16_t*>(d_a), K, static_cast<const bf16_t*>(d_b), K, d_c, N, M, N, K, d_bias,
              c_is_f32 != 0, accumulate != 0, sskd::as_stream(stream));
}

int sskd_gemm_tn_bf16(const void* d_a, const void* d_b, float* d_c, int64_t T, int M, int N, void* stream) {
  if (!gemm_tn_supported(T, M, N, M, N))
    return sskd::fail(SSKD_ERR_UNSUPPORTED, "gemm_tn: T=%lld M=%d N=%d not served (M %% 384, N %% 128, T %% 64)", (long long)T, M, N);
  return launch_gemm_tn(static_cast<const bf16_t*>(d_a), M, static_cast<const bf16_t*>(d_b), N, d_c, N, T, M, N,
                        sskd::as_stream(stream));
}

}  // extern "C"
