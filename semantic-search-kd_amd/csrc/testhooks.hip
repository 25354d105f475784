// Test hooks of the C-ABI (include/sskd_amd.h): the generic path's launchers one at a time, so that every kernel of
// generic.hip can be held against an fp64 reference by itself (tests/test_generic_kernels_gpu.py).  Host code only:
// no kernel is defined here, every launch goes through the same sskd_generic::launch_* function the training step
// and the teacher call.
#include "generic.h"

using namespace sskd_generic;

namespace {

template <class T>
T* ptr(const void* const* p, int i) {
  return static_cast<T*>(const_cast<void*>(p[i]));
}

}  // namespace

extern "C" {

int sskd_gemm_nt_ex(const sskd_gemm_desc* d, void* stream) {
  SSKD_REQUIRE(d, "gemm_nt_ex: null descriptor");
  GemmArgs g{};
  g.A = static_cast<const bf16_t*>(d->a);
  g.B = static_cast<const bf16_t*>(d->b);
  g.C = d->c;
  g.bias = d->bias;
  g.M = d->m;
  g.N = d->n;
  g.K = d->k;
  g.lda = d->lda;
  g.ldb = d->ldb;
  g.ldc = d->ldc;
  g.batch1 = d->batch1;
  g.batch2 = d->batch2;
  g.sA1 = d->sa1;
  g.sA2 = d->sa2;
  g.sB1 = d->sb1;
  g.sB2 = d->sb2;
  g.sC1 = d->sc1;
  g.sC2 = d->sc2;
  g.alpha = d->alpha;
  g.c_is_f32 = d->c_is_f32;
  g.accumulate = d->accumulate;
  g.split_k = d->split_k;
  g.act = d->act;
  return launch_gemm_nt(g, sskd::as_stream(stream));
}

int sskd_generic_op(int op, const void* const* p, int n_ptrs, const int64_t* n, int n_ints, const float* f, int n_floats,
                    void* stream) {
  static const struct {
    int ptrs, ints, floats;
    unsigned required;   // bit i: ptrs[i] must not be NULL
  } sig[] = {
      {0, 0, 0, 0},
      {4, 4, 1, 0x7},     // ATTENTION_FWD
      {6, 4, 1, 0x3f},    // ATTENTION_BWD
      {2, 3, 1, 0x3},     // SOFTMAX_FWD
      {2, 2, 1, 0x3},     // SOFTMAX_BWD
      {8, 2, 1, 0x1d},    // ADD_LN_FWD
      {10, 2, 0, 0xff},   // LN_BWD
      {2, 1, 0, 0x3},     // GELU_FWD
      {3, 1, 0, 0x7},     // GELU_BWD
      {4, 2, 0, 0xf},     // GELU_BWD_COLSUM
      {2, 3, 0, 0x3},     // COLSUM
      {3, 1, 0, 0x7},     // ADD
      {3, 10, 0, 0x3},    // TRANSPOSE
      {6, 5, 0, 0x3f},    // EMBED_FWD
      {6, 5, 0, 0x3f},    // EMBED_BWD
      {4, 4, 0, 0x7},     // POOL_FWD
      {4, 4, 0, 0xf},     // POOL_BWD
      {3, 6, 0, 0x7},     // GEMM_TN
  };
  SSKD_REQUIRE(op >= 1 && op < (int)(sizeof(sig) / sizeof(sig[0])), "generic_op: unknown op %d", op);
  SSKD_REQUIRE(n_ptrs == sig[op].ptrs && n_ints == sig[op].ints && n_floats == sig[op].floats,
               "generic_op %d: takes %d pointers, %d integers, %d floats (got %d, %d, %d)", op, sig[op].ptrs, sig[op].ints,
               sig[op].floats, n_ptrs, n_ints, n_floats);
  SSKD_REQUIRE((n_ptrs == 0 || p) && (n_ints == 0 || n) && (n_floats == 0 || f), "generic_op %d: null argument array", op);
  for (int i = 0; i < n_ptrs; ++i)
    SSKD_REQUIRE(p[i] || !(sig[op].required >> i & 1), "generic_op %d: pointer %d must not be NULL", op, i);
  const hipStream_t st = sskd::as_stream(stream);
  switch (op) {
    case SSKD_OP_ATTENTION_FWD:
      return launch_attention_fwd(ptr<const bf16_t>(p, 0), ptr<const int32_t>(p, 1), (int)n[0], (int)n[1], (int)n[2],
                                  (int)n[3], f[0], ptr<bf16_t>(p, 2), ptr<float>(p, 3), st);
    case SSKD_OP_ATTENTION_BWD:
      return launch_attention_bwd(ptr<const bf16_t>(p, 0), ptr<const int32_t>(p, 1), ptr<const bf16_t>(p, 2),
                                  ptr<const bf16_t>(p, 3), ptr<const float>(p, 4), (int)n[0], (int)n[1], (int)n[2], (int)n[3],
                                  f[0], ptr<bf16_t>(p, 5), st);
    case SSKD_OP_SOFTMAX_FWD:
      return launch_softmax_fwd(ptr<bf16_t>(p, 0), ptr<const int32_t>(p, 1), (int)n[0], (int)n[1], (int)n[2], f[0], st);
    case SSKD_OP_SOFTMAX_BWD:
      return launch_softmax_bwd(ptr<bf16_t>(p, 0), ptr<const bf16_t>(p, 1), n[0], (int)n[1], f[0], st);
    case SSKD_OP_ADD_LN_FWD:
      SSKD_REQUIRE(!p[6] == !p[7], "generic_op %d: mean and rstd are saved together", op);
      return launch_add_ln_fwd(ptr<const bf16_t>(p, 0), ptr<const bf16_t>(p, 1), ptr<const float>(p, 2),
                               ptr<const float>(p, 3), f[0], n[0], (int)n[1], ptr<bf16_t>(p, 4), ptr<bf16_t>(p, 5),
                               ptr<float>(p, 6), ptr<float>(p, 7), st);
    case SSKD_OP_LN_BWD:
      return launch_ln_bwd(ptr<const bf16_t>(p, 0), ptr<const bf16_t>(p, 1), ptr<const float>(p, 2), ptr<const float>(p, 3),
                           ptr<const float>(p, 4), n[0], (int)n[1], ptr<bf16_t>(p, 5), ptr<float>(p, 6), ptr<float>(p, 7),
                           st, ptr<float>(p, 8), ptr<const bf16_t>(p, 9));
    case SSKD_OP_GELU_FWD:
      return launch_gelu_fwd(ptr<const bf16_t>(p, 0), ptr<bf16_t>(p, 1), n[0], st);
    case SSKD_OP_GELU_BWD:
      return launch_gelu_bwd(ptr<const bf16_t>(p, 0), ptr<const bf16_t>(p, 1), ptr<bf16_t>(p, 2), n[0], st);
    case SSKD_OP_GELU_BWD_COLSUM:
      return launch_gelu_bwd_colsum(ptr<const bf16_t>(p, 0), ptr<const bf16_t>(p, 1), ptr<bf16_t>(p, 2), ptr<float>(p, 3),
                                    n[0], (int)n[1], st);
    case SSKD_OP_COLSUM:
      return launch_colsum(ptr<const bf16_t>(p, 0), n[0], (int)n[1], n[2], ptr<float>(p, 1), st);
    case SSKD_OP_ADD:
      return launch_add(ptr<const bf16_t>(p, 0), ptr<const bf16_t>(p, 1), ptr<bf16_t>(p, 2), n[0], st);
    case SSKD_OP_TRANSPOSE: {
      TransposeArgs t{};
      t.in = ptr<const bf16_t>(p, 0);
      t.out = ptr<bf16_t>(p, 1);
      t.colsum = ptr<float>(p, 2);
      t.R = (int)n[0];
      t.C = (int)n[1];
      t.ld_in = n[2];
      t.ld_out = n[3];
      t.batch1 = (int)n[4];
      t.batch2 = (int)n[5];
      t.sI1 = n[6];
      t.sI2 = n[7];
      t.sO1 = n[8];
      t.sO2 = n[9];
      SSKD_REQUIRE(t.batch1 >= 1 && t.batch2 >= 1, "transpose: batch counts must be >= 1");
      return launch_transpose(t, st);
    }
    case SSKD_OP_EMBED_FWD:
      return launch_embed_fwd(ptr<const int32_t>(p, 0), ptr<const int32_t>(p, 1), ptr<const bf16_t>(p, 2),
                              ptr<const bf16_t>(p, 3), ptr<const bf16_t>(p, 4), (int)n[0], (int)n[1], (int)n[2], (int)n[3],
                              (int)n[4], ptr<bf16_t>(p, 5), st);
    case SSKD_OP_EMBED_BWD:
      return launch_embed_bwd(ptr<const int32_t>(p, 0), ptr<const int32_t>(p, 1), ptr<const bf16_t>(p, 2), (int)n[0],
                              (int)n[1], (int)n[2], (int)n[3], (int)n[4], ptr<float>(p, 3), ptr<float>(p, 4),
                              ptr<float>(p, 5), st);
    case SSKD_OP_POOL_FWD:
      return launch_pool_fwd(ptr<const bf16_t>(p, 0), ptr<const int32_t>(p, 1), (int)n[0], (int)n[1], (int)n[2], (int)n[3],
                             ptr<float>(p, 2), ptr<float>(p, 3), st);
    case SSKD_OP_POOL_BWD:
      return launch_pool_bwd(ptr<const float>(p, 0), ptr<const float>(p, 1), ptr<const int32_t>(p, 2), (int)n[0], (int)n[1],
                             (int)n[2], (int)n[3], ptr<bf16_t>(p, 3), st);
    case SSKD_OP_GEMM_TN:
      SSKD_REQUIRE(n[2] >= n[5], "gemm_tn: ldc=%lld < N=%lld", (long long)n[2], (long long)n[5]);
      return launch_gemm_tn(ptr<const bf16_t>(p, 0), n[0], ptr<const bf16_t>(p, 1), n[1], ptr<float>(p, 2), n[2], n[3],
                            (int)n[4], (int)n[5], st);
  }
  return sskd::fail(SSKD_ERR_INVALID, "generic_op: unknown op %d", op);
}

}  // extern "C"
