"""Per-kernel fp64 parity of the generic path (csrc/generic.hip, the hipBLASLt route of csrc/blaslt.hip): every kernel by
itself, through the C-ABI test hooks ``sskd_gemm_nt_ex`` and ``sskd_generic_op``, against oracle/generic_ops.py.

Bounds are PER ELEMENT and scaled by that element's own conditioning; no cosine gate, no normalisation by a global
maximum.  u = 2^-24 (fp32 unit roundoff); ulp(x) = one bf16 ulp of |x| (2^-7 relative: a correctly rounded bf16 output is
within half of it, the other half covers the fp32 arithmetic before the rounding).  An fp32 sum of n terms is off by at
most n u sum|terms| (``mag``), so:

  * products (bf16 out):  |got - ref| <= ulp(ref) + (K + 8) u mag,       mag = |alpha| |A| |B|^T + |bias|
    (fp32 out: 2 u |ref| instead of the ulp; split-K adds split_k more additions);
  * reductions:           |got - ref| <= 2 u |ref| + (n + 8) u sum|terms|  over the n terms of the row / column;
  * where a kernel rounds an intermediate to bf16 by design the reference rounds at the same point (see the oracle);
    where the kernel and the reference may round a value at different points (attention's P under a moving running
    maximum, dS / P in the backward), the bound adds one bf16 rounding of every term: 2^-8 sum|terms|;
  * arithmetic that is fully determined (transpose, add, embed_fwd, masked zeros) is compared bit for bit.

No constant below was calibrated on the GPU: each is derived in the docstring of its group.  A failure reports the worst
element (index, got, ref, bound).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import generic_ops as go

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


def _ptr(x):
    return None if x is None else (x.data_ptr() if isinstance(x, torch.Tensor) else x)


def _op(lib, code, ptrs, ints, floats=()):
    P = (C.c_void_p * len(ptrs))(*[_ptr(p) for p in ptrs])
    I = (C.c_int64 * len(ints))(*[int(v) for v in ints])
    F = (C.c_float * len(floats))(*[float(v) for v in floats])
    return lib.sskd_generic_op(code, P, len(ptrs), I, len(ints), F, len(floats), _st())


def _run(lib, code, ptrs, ints, floats=()):
    from semantic_search_kd_amd import _native

    _native.check(_op(lib, code, ptrs, ints, floats))
    torch.cuda.synchronize()


def _check(got, ref, bound, what):
    """|got - ref| <= bound element-wise (NaN fails); on failure name the worst element."""
    got = got.detach().to("cpu", torch.float64)
    ref, bound = ref.to(torch.float64), torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        excess = torch.where(bad, torch.nan_to_num(err - bound, nan=float("inf")), torch.full_like(err, -1.0))
        idx = np.unravel_index(int(torch.argmax(excess)), tuple(ref.shape))
        pytest.fail(f"{what}: {int(bad.sum())} of {ref.numel()} elements out of bound; worst at {idx}: "
                    f"got {got[idx].item()!r}, ref {ref[idx].item()!r}, bound {bound[idx].item():.3e}")


def _bits_equal(got, want, what):
    g, w = got.detach().cpu(), want.detach().cpu()
    if g.dtype == BF:
        g, w = g.view(torch.int16), w.to(BF).view(torch.int16)
    if not torch.equal(g, w):
        i = int(torch.nonzero((g != w).reshape(-1))[0])
        idx = np.unravel_index(i, tuple(g.shape))
        pytest.fail(f"{what}: not bit-identical, first difference at {idx}: got {got.reshape(-1)[i].item()!r}, "
                    f"want {want.reshape(-1)[i].item()!r}")


def _rand(shape, g, scale=1.0, dtype=BF):
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(dtype)


# ----------------------------------------------------------------------------------------------------------------------
# NT GEMM
# ----------------------------------------------------------------------------------------------------------------------
def _gemm(lib, A, B, Cbuf, M, N, K, lda, ldb, ldc, bias=None, alpha=1.0, f32=0, acc=0, split=1, act=0, batch=(1, 1),
          strides=(0, 0, 0, 0, 0, 0)):
    from semantic_search_kd_amd import _native

    d = _native.GemmDesc(a=_ptr(A), b=_ptr(B), c=_ptr(Cbuf), bias=_ptr(bias), lda=lda, ldb=ldb, ldc=ldc,
                         sa1=strides[0], sa2=strides[1], sb1=strides[2], sb2=strides[3], sc1=strides[4], sc2=strides[5],
                         m=M, n=N, k=K, batch1=batch[0], batch2=batch[1], alpha=alpha, c_is_f32=f32, accumulate=acc,
                         split_k=split, act=act)
    return lib.sskd_gemm_nt_ex(C.byref(d), _st())


def _gemm_case(lib, g, M, N, K, *, pad=0, bias=True, alpha=1.0, f32=0, acc=0, split=1, act=0, what=""):
    """One unbatched product with leading dimensions K + pad (operands) and N + pad (output), checked per element:
    bf16 out  |got - ref| <= ulp(ref) + (K + split + 8) u mag   (act = 1: the pre-activation error times max|gelu'| = 1.13,
              plus the epilogue's erf-GELU approximation error 2.6e-5 (csrc/common.h gelu_erf), plus ulp(ref));
    fp32 out  |got - ref| <= 2 u |ref| + (K + split + 8) u mag, ref and mag including the prefilled C when accumulating.
    The columns of the padding stay untouched (NaN-filled before, NaN after)."""
    from semantic_search_kd_amd import _native

    lda = ldb = K + pad
    ldc = N + pad
    A = _rand((M, lda), g)
    B = _rand((N, ldb), g, K ** -0.5 * 4)
    bvec = torch.randn(N, generator=g, device="cuda") * 2 if bias else None
    if acc:
        Cbuf = torch.randn((M, ldc), generator=g, device="cuda")
        c0 = Cbuf[:, :N].double().cpu()
        Cbuf[:, N:] = float("nan")
    else:
        Cbuf = torch.full((M, ldc), float("nan"), device="cuda", dtype=torch.float32 if f32 else BF)
    _native.check(_gemm(lib, A, B, Cbuf, M, N, K, lda, ldb, ldc, bvec, alpha, f32, acc, split, act))
    torch.cuda.synchronize()
    pre, mag = go.gemm_nt(A[:, :K], B[:, :K], bvec, alpha)
    tail = (K + split + 8) * U * mag
    if acc:
        pre, mag = pre + c0, mag + c0.abs()
        tail = (K + split + 8) * U * mag
    if act == 1:
        ref = go.gelu(pre)
        bound = go.bf16_ulp(ref) + 1.13 * tail + 2.6e-5
    elif f32:
        ref, bound = pre, 2 * U * pre.abs() + tail
    else:
        ref, bound = pre, go.bf16_ulp(pre) + tail
    _check(Cbuf[:, :N], ref, bound, f"gemm_nt {what} M={M} N={N} K={K} pad={pad} f32={f32} acc={acc} split={split} act={act}")
    if pad:
        assert torch.isnan(Cbuf[:, N:].float()).all(), "gemm_nt wrote past N into the padding columns"


@pytest.fixture
def hand_kernels(native_lib):
    """backend 1: every product on the hand-written kernels; the previous mode is restored whatever happens."""
    prev = native_lib.sskd_gemm_backend(-1)
    native_lib.sskd_gemm_backend(1)
    try:
        yield native_lib
    finally:
        native_lib.sskd_gemm_backend(prev)


def test_gemm_nt_small_kernel_shapes_edges_and_epilogues(gpu, hand_kernels):
    """128 x 128 kernel, BK = 32 (K % 64 != 0) and 64: ragged M and N, padded leading dimensions, bias or none, bf16 and
    fp32 outputs, accumulation into a prefilled C, alpha != 1 and the erf-GELU epilogue.  Bounds: see _gemm_case."""
    lib = hand_kernels
    g = torch.Generator(device="cuda").manual_seed(10)
    for K in (96, 128):
        for M in (1, 5, 129, 300):
            for N in (8, 130, 1000):
                _gemm_case(lib, g, M, N, K, pad=8, bias=(M + N) % 2 == 0, what="small")
    _gemm_case(lib, g, 129, 130, 64, pad=16, f32=1, what="fp32")
    _gemm_case(lib, g, 300, 136, 96, pad=8, f32=1, acc=1, what="fp32 +=")
    _gemm_case(lib, g, 129, 1000, 128, pad=8, alpha=0.37, what="alpha")
    _gemm_case(lib, g, 300, 130, 96, pad=8, alpha=1.5, act=1, what="gelu")
    _gemm_case(lib, g, 300, 130, 64, f32=1, alpha=-0.75, what="alpha fp32")


def test_gemm_nt_256_kernel_all_three_tile_widths(gpu, hand_kernels):
    """256-row global-to-LDS kernel (M % 256 == 0, M >= 1024, bf16 out): N = 1024 -> 256-wide tiles, 1152 -> 192,
    640 -> 128; K % 64 == 0; plus alpha != 1 and the GELU epilogue on it.  Bounds: see _gemm_case."""
    lib = hand_kernels
    g = torch.Generator(device="cuda").manual_seed(11)
    _gemm_case(lib, g, 1024, 1024, 128, what="256/BN256")
    _gemm_case(lib, g, 1280, 1152, 384, what="256/BN192")
    _gemm_case(lib, g, 1024, 640, 192, bias=False, what="256/BN128")
    _gemm_case(lib, g, 1024, 1152, 128, alpha=0.5, what="256 alpha")
    _gemm_case(lib, g, 1024, 640, 64, act=1, what="256 gelu")


def test_gemm_nt_batched_strides_of_the_unfused_attention(gpu, hand_kernels):
    """Scores = Q K^T and ctx = P V of the unfused path: batch (B, heads) with the qkv row strides (sA1 = S * 3H,
    sA2 = DH, lda = 3H), alpha = the softmax scale.  Bound: ulp(ref) + (K + 8) u mag per element of every batch."""
    from semantic_search_kd_amd import _native

    lib = hand_kernels
    g = torch.Generator(device="cuda").manual_seed(12)
    Bt, heads, S, DH = 2, 3, 96, 32
    H = heads * DH
    qkv = _rand((Bt * S, 3 * H), g)
    out = torch.full((Bt, heads, S, S), float("nan"), device="cuda", dtype=BF)
    scale = DH ** -0.5
    _native.check(_gemm(lib, qkv, qkv[:, H:], out, S, S, DH, 3 * H, 3 * H, S, alpha=scale, batch=(Bt, heads),
                        strides=(S * 3 * H, DH, S * 3 * H, DH, heads * S * S, S * S)))
    torch.cuda.synchronize()
    q, k, _ = go._split_heads(qkv, Bt, S, heads, DH)
    ref, mag = go.gemm_nt(q, k, None, scale)
    _check(out, ref, go.bf16_ulp(ref) + (DH + 8) * U * mag, "batched Q K^T")


def test_gemm_nt_split_k_atomics(gpu, hand_kernels):
    """split_k in {2, 7} (7 does not divide K / 32 = 20): fp32 accumulating output, partial products meet through
    atomics.  Bound: 2 u |ref| + (K + split + 8) u mag, ref and mag including the prefilled C."""
    lib = hand_kernels
    g = torch.Generator(device="cuda").manual_seed(13)
    for split in (2, 7):
        _gemm_case(lib, g, 200, 264, 640, bias=False, f32=1, acc=1, split=split, what="split-K")


def test_gemm_nt_library_route_backend0(gpu, native_lib):
    """backend 0 on the plain large products (K, N >= 1024, bf16 out, alpha 1): hipBLASLt, same per-element bound as the
    hand-written kernels (a correctly rounded fp32-accumulated product: ulp(ref) + (K + 8) u mag)."""
    lib = native_lib
    prev = lib.sskd_gemm_backend(-1)
    try:
        lib.sskd_gemm_backend(0)
        g = torch.Generator(device="cuda").manual_seed(14)
        _gemm_case(lib, g, 1024, 1024, 1024, what="lib")
        _gemm_case(lib, g, 1024, 1024, 2048, bias=False, what="lib no bias")
        _gemm_case(lib, g, 1024, 1024, 1024, pad=64, what="lib ld")
    finally:
        lib.sskd_gemm_backend(prev)


# ----------------------------------------------------------------------------------------------------------------------
# TN GEMM (weight gradients)
# ----------------------------------------------------------------------------------------------------------------------
def _tn_case(lib, g, T, M, N, ldc_pad, what):
    """C[M, N] (ldc = N + pad) += A[T, M]^T B[T, N].  Bound: 2 u |ref| + (T + 8 + 256) u mag (fp32 MFMA accumulation over
    a slice, then fp32 atomics across at most 256 slices), ref and mag including the prefilled C; padding untouched."""
    ldc = N + ldc_pad
    A, B = _rand((T, M), g), _rand((T, N), g)
    Cbuf = torch.randn((M, ldc), generator=g, device="cuda")
    Cbuf[:, N:] = float("nan")
    c0 = Cbuf[:, :N].double().cpu()
    _run(lib, 17, [A, B, Cbuf], [M, N, ldc, T, M, N])
    ref, mag = go.gemm_tn(A, B)
    ref, mag = ref + c0, mag + c0.abs()
    _check(Cbuf[:, :N], ref, 2 * U * ref.abs() + (T + 264) * U * mag, f"gemm_tn {what} T={T} M={M} N={N} ldc={ldc}")
    assert torch.isnan(Cbuf[:, N:]).all(), "gemm_tn wrote into the padding columns"


def test_gemm_tn_branches_and_ragged_slices(gpu, native_lib):
    """XCD-mapped order (M / 384 > 1 or few tiles) and the dealt order (M = 384 with N >= 1536: 12+ tiles in one row);
    T / 64 not a multiple of the slice length; ldc > N."""
    g = torch.Generator(device="cuda").manual_seed(20)
    _tn_case(native_lib, g, 64 * 37, 768, 256, 8, "xcd-mapped")
    _tn_case(native_lib, g, 64 * 45, 384, 1536, 16, "dealt")
    _tn_case(native_lib, g, 64 * 13, 384, 128, 0, "single tile")


def test_gemm_tn_student_step_shapes(gpu, native_lib):
    """The student's real weight-gradient products at 65 536 tokens: dWqkv (1152 x 384), dWo (384 x 384), dW1 (1536 x 384),
    dW2 (384 x 1536).  Bound as _tn_case."""
    g = torch.Generator(device="cuda").manual_seed(21)
    for M, N in ((1152, 384), (384, 384), (1536, 384), (384, 1536)):
        _tn_case(native_lib, g, 65536, M, N, 0, "step")


# ----------------------------------------------------------------------------------------------------------------------
# fused attention
# ----------------------------------------------------------------------------------------------------------------------
def _attn_inputs(g, B, S, heads, DH, spread=1.5):
    return _rand((B * S, 3 * heads * DH), g, spread)


def _masks(B, S):
    """full; right-padded to 1, 31, 32, 33 and S - 1 valid keys; a hole over key tile 1 (S >= 64) or tile 0; no valid key."""
    rows = [np.ones(S, np.int32)]
    for n in (1, 31, 32, 33, S - 1):
        r = np.zeros(S, np.int32)
        r[:min(n, S)] = 1
        rows.append(r)
    hole = np.ones(S, np.int32)
    hole[32:64] = 0 if S >= 96 else 1
    if S < 96:
        hole[:32] = 0
    rows.append(hole)
    rows.append(np.zeros(S, np.int32))
    m = np.stack([rows[i % len(rows)] for i in range(B)])
    return torch.from_numpy(m).cuda()


def _attn_fwd_check(lib, qkv, mask, B, S, heads, DH, scale):
    """ctx:  |got - ref| <= ulp(ref) + 2^-8 mag + (S + DH + 16) 2^-22 mag, mag = sum_j P_ij |V_jd| (P rounded to bf16 by the
             kernel relative to its running maximum, by the reference relative to the final one: one rounding each);
             2^-22 covers exp2f (1 ulp) and the fp32 sums.
    lse:  |got - ref| <= 2^-20 (1 + |ref|) + (S + 16) 2^-23 + scale2 (DH + 8) u max_j sum_d |q_d| |k_jd|
          (log2 domain: fp32 sums of S exponentials, the final add, the score's fp32 accumulation).
    A row without a valid key: ctx exactly 0, lse = -inf (csrc/generic.h)."""
    H = heads * DH
    ctx = torch.full((B * S, H), float("nan"), device="cuda", dtype=BF)
    lse = torch.full((B, heads, S), float("nan"), device="cuda")
    _run(lib, 1, [qkv, mask, ctx, lse], [B, S, heads, DH], [scale])
    ref, lref, mag = go.attention_fwd(qkv, mask, B, S, heads, DH, scale)
    _check(ctx, ref, go.bf16_ulp(ref) + 2.0 ** -8 * mag + (S + DH + 16) * 2.0 ** -22 * mag, f"attention ctx S={S} DH={DH}")
    q, k, _ = go._split_heads(qkv, B, S, heads, DH)
    qk = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1)
    scale2 = scale * go.LOG2E
    finite = torch.isfinite(lref)
    lb = 2.0 ** -20 * (1 + lref.abs()) + (S + 16) * 2.0 ** -23 + scale2 * (DH + 8) * U * qk
    _check(torch.where(finite.cuda(), lse, torch.zeros_like(lse)), torch.where(finite, lref, torch.zeros_like(lref)),
           torch.where(finite, lb, torch.zeros_like(lb)), f"attention lse S={S} DH={DH}")
    assert torch.isneginf(lse[~finite.cuda()]).all(), "a row without a valid key must save lse = -inf"
    empty = (mask == 0).all(1)
    assert torch.equal(ctx.view(B, S, H)[empty].float(), torch.zeros_like(ctx.view(B, S, H)[empty].float()))
    return ctx, lse


@pytest.mark.parametrize("DH", [32, 64, 128])
def test_attention_fwd_shapes_and_masks(gpu, native_lib, DH):
    """DH in {32, 64, 128}, S in {32, 96, 256, 288, 512} (288 and 512: two workgroups per (row, head), at 288 the second
    has one active wave), every mask of _masks, ctx of every query row and the saved lse.  Bounds: _attn_fwd_check.
    DH = 128 at S = 512 needs 258 KiB of LDS: the launcher refuses it (SSKD_ERR_INVALID) and writes nothing."""
    g = torch.Generator(device="cuda").manual_seed(30 + DH)
    heads = 2
    for S in (32, 96, 256, 288, 512):
        B = 8
        qkv, mask = _attn_inputs(g, B, S, heads, DH), _masks(B, S)
        if S * DH > 36864:   # K and V of a head no longer fit in one workgroup's LDS (csrc/generic.h): refused
            ctx = torch.full((B * S, heads * DH), float("nan"), device="cuda", dtype=BF)
            assert _op(native_lib, 1, [qkv, mask, ctx, None], [B, S, heads, DH], [DH ** -0.5]) == 1
            torch.cuda.synchronize()
            assert torch.isnan(ctx.float()).all()
            continue
        _attn_fwd_check(native_lib, qkv, mask, B, S, heads, DH, DH ** -0.5)


@pytest.mark.parametrize("DH,S", [(32, 64), (32, 256), (64, 96), (64, 128)])
def test_attention_bwd_against_fp64(gpu, native_lib, DH, S):
    """dQ, dK, dV from the forward's own ctx and lse (S * DH up to 8192).
    Bound: ulp(ref) + 2^-8 mag + (S + DH + 16) 2^-22 mag, mag = sum_j |dS_ij| |K_jd| (dQ), sum_i |dS_ij| |Q_id| (dK),
    sum_i P_ij |dO_id| (dV): dS and P are rounded to bf16 before their products (one rounding each, 2^-9, doubled for the
    kernel's fp32 P against the reference's fp64 one); plus 2 (DH + 16) u mag_d: dP (an MFMA sum) and D = rowsum(dO o O)
    (an fp32 sum) are DH terms each and dP - D cancels (exactly, mathematically, for a row with one valid key), so their
    error is relative to P scale sum_d |dO| (|V| + |O|), carried through the product with K or Q.  Masked keys: dK = dV = 0 exactly; the row without a valid key
    gives finite zeros in all of dQ | dK | dV.  dO is nonzero on EVERY query row, padding included: every query attends to
    the valid keys, so dK / dV of a padded row collect all S queries (pass B used to stop at the last valid key tile)."""
    g = torch.Generator(device="cuda").manual_seed(40 + DH + S)
    B, heads = 8, 2
    H = heads * DH
    qkv, mask = _attn_inputs(g, B, S, heads, DH), _masks(B, S)
    scale = DH ** -0.5
    ctx, lse = _attn_fwd_check(native_lib, qkv, mask, B, S, heads, DH, scale)
    dctx = _rand((B * S, H), g)
    dqkv = torch.full((B * S, 3 * H), float("nan"), device="cuda", dtype=BF)
    _run(native_lib, 2, [qkv, mask, ctx, dctx, lse, dqkv], [B, S, heads, DH], [scale])
    ref, mag, mag_d = go.attention_bwd(qkv, mask, ctx, dctx, B, S, heads, DH, scale, lse=lse.cpu())
    bound = go.bf16_ulp(ref) + 2.0 ** -8 * mag + (S + DH + 16) * 2.0 ** -22 * mag + 2 * (DH + 16) * U * mag_d
    _check(dqkv, ref, bound, f"attention dqkv S={S} DH={DH}")
    masked_keys = (mask == 0).reshape(-1)
    assert torch.equal(dqkv[masked_keys, H:].float(), torch.zeros_like(dqkv[masked_keys, H:].float())), \
        "dK / dV of masked keys must be exactly 0"
    empty = (mask == 0).all(1).repeat_interleave(S)
    assert torch.equal(dqkv[empty].float(), torch.zeros_like(dqkv[empty].float()))


# ----------------------------------------------------------------------------------------------------------------------
# unfused attention: softmax
# ----------------------------------------------------------------------------------------------------------------------
def test_softmax_fwd_bwd(gpu, native_lib):
    """P = softmax(scale s + mask) per row: |got - ref| <= ulp(ref) + (S + 16) 2^-22 ref (exp and fp32 sum), masked
    probabilities exactly 0.  dS = scale P (dP - sum dP P): |got - ref| <= ulp(ref) + (S + 8) u mag,
    mag = scale |P| (|dP| + sum_j |dP_j P_j|).  S in {4, 12, 256, 260, 512}."""
    g = torch.Generator(device="cuda").manual_seed(50)
    for S in (4, 12, 256, 260, 512):
        B, heads, scale = 3, 2, 0.3
        s = _rand((B, heads, S, S), g, 3.0)
        mask = torch.ones((B, S), dtype=torch.int32, device="cuda")
        mask[1, max(1, S // 2 + 1):] = 0
        mask[2, 0] = 0
        p = s.clone()
        _run(native_lib, 3, [p, mask], [B, heads, S], [scale])
        ref = go.softmax_fwd(s, mask, B, heads, S, scale)
        _check(p.reshape(-1, S), ref, go.bf16_ulp(ref) + (S + 16) * 2.0 ** -22 * ref, f"softmax S={S}")
        masked = (mask == 0).view(B, 1, 1, S).expand(B, heads, S, S)
        assert torch.equal(p[masked].float(), torch.zeros_like(p[masked].float())), "masked probabilities must be 0"
        dp = _rand((B * heads * S, S), g)
        d = dp.clone()
        _run(native_lib, 4, [d, p], [B * heads * S, S], [scale])
        ref, mag = go.softmax_bwd(dp, p.reshape(-1, S), scale)
        _check(d, ref, go.bf16_ulp(ref) + (S + 8) * U * mag, f"softmax_bwd S={S}")


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def test_add_ln_fwd(gpu, native_lib):
    """mean: 2 u |ref| + delta, delta = (H + 8) u mean|z| (an fp32 sum of H values);
    rstd: relative 2^-21 (rsqrtf) + ((H + 8) u var + delta^2) / (2 (var + eps)) (H squares in fp32; a mean off by delta
    adds exactly delta^2 to the two-pass variance);
    y: ulp(ref) + |gamma| (delta rstd + |xh| rstd's relative error) + 4 u (|xh| |gamma| + |beta|).  Rows with |mean| >> std (300 + N(0, 1)) catch a one-pass variance.
    b and z_save each null and non-null, eps 1e-12 and 1e-5, H in {64, 384, 520, 1024}."""
    g = torch.Generator(device="cuda").manual_seed(60)
    for H in (64, 384, 520, 1024):
        for with_b, with_z, eps in ((False, False, 1e-12), (True, True, 1e-5), (True, False, 1e-12), (False, True, 1e-5)):
            M = 37
            a = torch.randn((M, H), generator=g, device="cuda")
            a[::3] += 300.0                                   # |mean| >> std: one-pass variance loses everything here
            a = a.to(BF)
            b = _rand((M, H), g) if with_b else None
            gamma = torch.randn(H, generator=g, device="cuda")
            beta = torch.randn(H, generator=g, device="cuda")
            y = torch.full((M, H), float("nan"), device="cuda", dtype=BF)
            z = torch.full((M, H), float("nan"), device="cuda", dtype=BF) if with_z else None
            mean = torch.full((M,), float("nan"), device="cuda")
            rstd = torch.full((M,), float("nan"), device="cuda")
            _run(native_lib, 5, [a, b, gamma, beta, y, z, mean, rstd], [M, H], [eps])
            ry, rz, rmean, rrstd, mag = go.add_ln_fwd(a, b, gamma, beta, eps, round_z=with_z)
            what = f"add_ln_fwd H={H} b={with_b} z={with_z} eps={eps}"
            zabs = rz.abs().mean(-1)
            delta = (H + 8) * U * zabs                        # fp32 sum of H values: the mean's error
            _check(mean, rmean, 2 * U * rmean.abs() + delta, what + " mean")
            # sum (z - mean - delta)^2 / H = var + delta^2 (the linear term vanishes): H squares summed in fp32
            var = 1.0 / rrstd ** 2 - eps
            eps_r = 2.0 ** -21 + 0.5 * ((H + 8) * U * var + delta ** 2) / (var + eps)   # + rsqrtf
            _check(rstd, rrstd, eps_r * rrstd, what + " rstd")
            xh = (rz - rmean[:, None]) * rrstd[:, None]
            g64 = gamma.double().cpu()
            yb = go.bf16_ulp(ry) + g64.abs() * ((delta * rrstd)[:, None] + xh.abs() * eps_r[:, None]) + 4 * U * mag
            _check(y, ry, yb, what + " y")
            if with_z:
                _bits_equal(z, rz.float(), what + " z_save")


def _ln_bwd_case(lib, g, M, H, with_dy2, alias):
    """dz: |got - ref| <= ulp(ref) + (2 H + 16) u mag (fp32 row sums of H terms, mag = rstd (|g| + mean|g| + |xh| mean|g xh|));
    dgamma, dbeta, dz_colsum (fp32 atomics into prefilled buffers): 2 u |ref| + (M + 16) u sum_rows|terms|, dz_colsum
    against the column sums of dz AS STORED (bf16)."""
    z = _rand((M, H), g, 2.0)
    zf = z.double().cpu()
    mean = zf.mean(-1).float().cuda()
    rstd = (1.0 / (zf.var(-1, unbiased=False) + 1e-5).sqrt()).float().cuda()
    gamma = torch.randn(H, generator=g, device="cuda")
    dy = _rand((M, H), g)
    dy2 = _rand((M, H), g) if with_dy2 else None
    dy_in, dy2_in = dy.clone(), (dy2.clone() if with_dy2 else None)
    dz = dy_in if alias else torch.full((M, H), float("nan"), device="cuda", dtype=BF)
    pre = [torch.randn(H, generator=g, device="cuda") for _ in range(3)]
    dgamma, dbeta, dzc = (p.clone() for p in pre)
    _run(lib, 6, [dy_in, z, mean, rstd, gamma, dz, dgamma, dbeta, dzc, dy2_in], [M, H])
    rdz, rdg, rdb, rdc, mdz, mdg, mdb, mdc = go.ln_bwd(dy, z, mean, rstd, gamma, dy2)
    what = f"ln_bwd M={M} H={H} dy2={with_dy2} alias={alias}"
    _check(dz, rdz, go.bf16_ulp(rdz) + (2 * H + 16) * U * mdz, what + " dz")
    p0, p1, p2 = (p.double().cpu() for p in pre)
    _check(dgamma, rdg + p0, 2 * U * (rdg + p0).abs() + (M + 16) * U * (mdg + p0.abs()), what + " dgamma")
    _check(dbeta, rdb + p1, 2 * U * (rdb + p1).abs() + (M + 16) * U * (mdb + p1.abs()), what + " dbeta")
    stored = dz.double().cpu().sum(0)
    _check(dzc, stored + p2, 2 * U * (stored + p2).abs() + (M + 16) * U * (mdc + p2.abs()), what + " dz_colsum")


def test_ln_bwd(gpu, native_lib):
    """H in {64, 384, 512} (<1, 2> instantiation) and {520, 1024} (<2, 2>); M in {1, 63, 64, 65, 4097}; dy2 null and
    non-null; dz aliasing dy; dgamma / dbeta / dz_colsum accumulated into prefilled buffers.  Bounds: _ln_bwd_case."""
    g = torch.Generator(device="cuda").manual_seed(70)
    for H in (64, 384, 512, 520, 1024):
        for M in (1, 63, 64, 65, 4097):
            _ln_bwd_case(native_lib, g, M, H, with_dy2=(M + H) % 2 == 1 or M == 4097, alias=M == 65)
        _ln_bwd_case(native_lib, g, 130, H, with_dy2=True, alias=True)


# ----------------------------------------------------------------------------------------------------------------------
# GELU, column sums, transpose, add
# ----------------------------------------------------------------------------------------------------------------------
def test_gelu_fwd_bwd(gpu, native_lib):
    """Every bf16 value over [-12, 12] (both zeros included): h within 1 bf16 ulp of fp64 erf-GELU, du = dh gelu'(u) within
    1 bf16 ulp of its fp64 value, each plus 2^-126 for the subnormal range and plus the absolute error of the kernels' fp32
    form Phi(x) = 0.5 (1 + erff(x / sqrt 2)): erff is within 2 fp32 ulps (2^-23 near -1), and for x below about -4 the sum
    with 1 cancels to a value of the size of that error.  So h gains |u| 2^-24 and du |dh| 2^-22 (with a factor 2 for the
    products around it).  These absolute terms are below 1e-6: the far negative tail, not the 1-ulp accuracy of the rest."""
    g = torch.Generator(device="cuda").manual_seed(80)
    lo, hi = torch.tensor(-12.0, dtype=BF).view(torch.int16).item(), torch.tensor(12.0, dtype=BF).view(torch.int16).item()
    pos = torch.arange(0, hi + 1, dtype=torch.int16).view(BF)
    neg = torch.arange(-32768, lo + 1, dtype=torch.int32).to(torch.int16).view(BF)
    u = torch.cat([pos, neg])
    u = torch.cat([u, torch.zeros((-u.numel()) % 8, dtype=BF)]).cuda()
    n = u.numel()
    assert (u.view(torch.int16) == -32768).any() and (u.view(torch.int16) == 0).any()
    h = torch.full_like(u, float("nan"))
    _run(native_lib, 7, [u, h], [n])
    ref = go.gelu(u)
    _check(h, ref, go.bf16_ulp(ref) + 2.0 ** -126 + go.f64(u).abs() * 2.0 ** -23, "gelu_fwd")
    dh = _rand((n,), g)
    du = torch.full_like(u, float("nan"))
    _run(native_lib, 8, [u, dh, du], [n])
    ref = go.gelu_bwd(u, dh)
    _check(du, ref, go.bf16_ulp(ref) + 2.0 ** -126 + go.f64(dh).abs() * 2.0 ** -22, "gelu_bwd")


def test_gelu_bwd_colsum(gpu, native_lib):
    """F in {8, 384, 1536, 4096 (widest fused case, RY = 2), 4104 (F / 8 = 513: the plain pair)}, M in {1, RY - 1, one M
    above 2 * 512 * RY with an odd remainder}.  du: the bound of gelu_bwd; db (+= into a prefilled buffer) against the column
    sums of du AS STORED: 2 u |ref| + (M + 16) u sum|du|."""
    g = torch.Generator(device="cuda").manual_seed(81)
    for F in (8, 384, 1536, 4096, 4104):
        RY = max(1, 1024 // (F // 8)) if F // 8 <= 512 else 1
        Ms = sorted({1, max(1, RY - 1), 2 * 512 * RY + 2 * RY + 1})
        for M in Ms:
            if M * F > 12_000_000:
                M = 2 * 512 * RY // 4 + 3
            u = _rand((M, F), g, 3.0)
            dh = _rand((M, F), g)
            du = torch.full_like(u, float("nan"))
            pre = torch.randn(F, generator=g, device="cuda")
            db = pre.clone()
            _run(native_lib, 9, [u, dh, du, db], [M, F])
            rdu, _, _ = go.gelu_bwd_colsum(u, dh)
            what = f"gelu_bwd_colsum M={M} F={F}"
            _check(du, rdu, go.bf16_ulp(rdu) + 2.0 ** -126 + go.f64(dh).abs() * 2.0 ** -22, what + " du")
            stored = du.double().cpu()
            p = pre.double().cpu()
            ref = stored.sum(0) + p
            _check(db, ref, 2 * U * ref.abs() + (M + 16) * U * (stored.abs().sum(0) + p.abs()), what + " db")


def test_colsum(gpu, native_lib):
    """N in {8, 1024, 1032, 3080} (one to four 1024-column windows), ld > N, M in {1, 127, 128, 129, 10 000}; db (+= into
    a prefilled buffer): 2 u |ref| + (M + 16) u sum|terms|."""
    g = torch.Generator(device="cuda").manual_seed(82)
    for N in (8, 1024, 1032, 3080):
        for M in (1, 127, 128, 129, 10000):
            ld = N + 24
            y = _rand((M, ld), g)
            pre = torch.randn(N, generator=g, device="cuda")
            db = pre.clone()
            _run(native_lib, 10, [y, db], [M, N, ld])
            s, m = go.colsum(y[:, :N])
            p = pre.double().cpu()
            _check(db, s + p, 2 * U * (s + p).abs() + (M + 16) * U * (m + p.abs()), f"colsum M={M} N={N}")


def test_transpose_and_add_bit_exact(gpu, native_lib):
    """Transpose moves bits (unbatched with ragged tiles and padded leading dimensions, and batched with the attention
    strides); its column-sum side output (+= into a prefilled buffer): 2 u |ref| + (R + 16) u sum|x|.  add: bf16(a + b) of
    an exact fp32 sum, bit for bit."""
    g = torch.Generator(device="cuda").manual_seed(83)
    R, Cc = 200, 132
    x = _rand((R, Cc + 4), g)
    out = torch.full((Cc, R + 8), float("nan"), device="cuda", dtype=BF)
    pre = torch.randn(Cc, generator=g, device="cuda")
    cs = pre.clone()
    _run(native_lib, 12, [x, out, cs], [R, Cc, Cc + 4, R + 8, 1, 1, 0, 0, 0, 0])
    _bits_equal(out[:, :R], x[:, :Cc].T.contiguous(), "transpose")
    assert torch.isnan(out[:, R:].float()).all()
    s, m = go.colsum(x[:, :Cc])
    p = pre.double().cpu()
    _check(cs, s + p, 2 * U * (s + p).abs() + (R + 16) * U * (m + p.abs()), "transpose colsum")
    # batched: [B, heads] blocks of [S, DH] out of rows of width 3H
    Bt, heads, S, DH = 2, 3, 64, 32
    qkv = _rand((Bt * S, 3 * heads * DH), g)
    outb = torch.full((Bt, heads, DH, S), float("nan"), device="cuda", dtype=BF)
    _run(native_lib, 12, [qkv, outb, None], [S, DH, 3 * heads * DH, S, Bt, heads, S * 3 * heads * DH, DH, heads * DH * S, DH * S])
    q, _, _ = go._split_heads(qkv, Bt, S, heads, DH)
    _bits_equal(outb, q.transpose(-1, -2).float(), "batched transpose")
    a, b = _rand((4104,), g, 10.0), _rand((4104,), g)
    c = torch.full_like(a, float("nan"))
    _run(native_lib, 11, [a, b, c], [a.numel()])
    _bits_equal(c, (a.float() + b.float()), "add")


# ----------------------------------------------------------------------------------------------------------------------
# embeddings, pooling
# ----------------------------------------------------------------------------------------------------------------------
def test_embed_fwd_bit_exact(gpu, native_lib):
    """z = bf16((word[clamp(id)] + pos[t + pos_offset]) + type0) in fp32, bit for bit; ids below 0 and >= vocab clamp."""
    g = torch.Generator(device="cuda").manual_seed(90)
    vocab, n_pos, B, S, H = 50, 80, 3, 64, 136
    word, pos, ty = _rand((vocab, H), g), _rand((n_pos, H), g), _rand((H,), g)
    ids = torch.randint(-3, vocab + 3, (B, S), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda()
    ids[0, :3] = torch.tensor([-1, vocab, vocab + 100], dtype=torch.int32)
    mask = torch.ones((B, S), dtype=torch.int32, device="cuda")
    for off in (0, 2):
        z = torch.full((B * S, H), float("nan"), device="cuda", dtype=BF)
        _run(native_lib, 13, [ids, mask, word, pos, ty, z], [B, S, H, vocab, off])
        _bits_equal(z, go.embed_fwd(ids.cpu(), word, pos, ty, S, off).float(), f"embed_fwd pos_offset={off}")


def test_embed_bwd_repeats_masks_and_offsets(gpu, native_lib):
    """dword / dpos / dtype0 (+= into prefilled buffers): all tokens sharing one id, half sharing one id, masked tokens,
    clamped ids; dpos lands at t + pos_offset (2).  Bound 2 u |ref| + (B S + 16) u sum|terms|; rows no token touches stay
    exactly at their prefilled value."""
    g = torch.Generator(device="cuda").manual_seed(91)
    vocab, n_pos, B, S, H, off = 40, 72, 4, 64, 136, 2
    cpu = torch.Generator().manual_seed(2)
    for case in ("one id", "half", "mixed"):
        if case == "one id":
            ids = torch.full((B, S), 7, dtype=torch.int32)
        elif case == "half":
            ids = torch.randint(0, vocab, (B, S), generator=cpu, dtype=torch.int32)
            ids.view(-1)[::2] = 5
        else:
            ids = torch.randint(-5, vocab + 5, (B, S), generator=cpu, dtype=torch.int32)
        mask = torch.ones((B, S), dtype=torch.int32)
        mask[1, 40:] = 0
        mask[3, 1:] = 0
        dz = _rand((B * S, H), g)
        pre = [torch.randn(sh, generator=g, device="cuda") for sh in ((vocab, H), (n_pos, H), (H,))]
        dword, dpos, dtype0 = (p.clone() for p in pre)
        _run(native_lib, 14, [ids.cuda(), mask.cuda(), dz, dword, dpos, dtype0], [B, S, H, vocab, off])
        rw, rp, rt, mw, mp, mt = go.embed_bwd(ids, mask, dz, vocab, n_pos, S, off)
        n = B * S + 16
        for got, r, m, p, what in ((dword, rw, mw, pre[0], "dword"), (dpos, rp, mp, pre[1], "dpos"), (dtype0, rt, mt, pre[2], "dtype0")):
            p = p.double().cpu()
            _check(got, r + p, 2 * U * (r + p).abs() + n * U * (m + p.abs()), f"embed_bwd {case} {what}")
        untouched = (mw == 0).all(1)
        _bits_equal(dword[untouched.cuda()], pre[0][untouched.cuda()], f"embed_bwd {case}: untouched word rows")
        _bits_equal(dpos[:off], pre[1][:off], "dpos below pos_offset")
        _bits_equal(dpos[off + S:], pre[1][off + S:], "dpos above pos_offset + S")


def test_pool_fwd_bwd(gpu, native_lib):
    """H in {128, 320, 384, 1024}, normalize 0 / 1, lengths 1 and S, one all-masked row (finite zeros, neighbours
    unchanged).  out / pooled: 2 u |ref| + (S + 16) u mag with mag = sum|h| / n (/ |e| normalised, plus the norm's H-term
    sum); dhidden: ulp(ref) + (H + 16) u mag with mag = (|g| + |e_hat| sum|e_hat g|) / |e| / n."""
    g = torch.Generator(device="cuda").manual_seed(92)
    B, S = 4, 40
    mask = torch.ones((B, S), dtype=torch.int32, device="cuda")
    mask[0, 1:] = 0        # length 1
    mask[2] = 0            # all masked
    mask[3, 17:] = 0
    for H in (128, 320, 384, 1024):
        for norm in (0, 1):
            hidden = _rand((B, S, H), g)
            out = torch.full((B, H), float("nan"), device="cuda")
            pooled = torch.full((B, H), float("nan"), device="cuda")
            _run(native_lib, 15, [hidden, mask, out, pooled], [B, S, H, norm])
            rout, rpool, mag = go.pool_fwd(hidden, mask, bool(norm))
            what = f"pool H={H} normalize={norm}"
            _check(pooled, rpool, 2 * U * rpool.abs() + (S + 16) * U * go.pool_fwd(hidden, mask, False)[2], what + " pooled")
            _check(out, rout, 2 * U * rout.abs() + (S + H + 16) * U * mag, what + " out")
            assert torch.equal(out[2], torch.zeros_like(out[2])), "an all-masked row pools to finite zeros"
            dout = torch.randn((B, H), generator=g, device="cuda")
            dh = torch.full((B, S, H), float("nan"), device="cuda", dtype=BF)
            _run(native_lib, 16, [dout, pooled, mask, dh], [B, S, H, norm])
            rdh, mdh = go.pool_bwd(dout, pooled, mask, bool(norm))
            _check(dh, rdh, go.bf16_ulp(rdh) + (H + 16) * U * mdh, what + " dhidden")
            assert torch.equal(dh[2].float(), torch.zeros_like(dh[2].float()))


# ----------------------------------------------------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_out_of_contract_shapes_are_refused_and_write_nothing(gpu, native_lib):
    """Shapes outside a launcher's contract return nonzero and leave a NaN-filled output untouched; a wrong argument count
    returns SSKD_ERR_INVALID."""
    lib = native_lib
    nanb = lambda *s: torch.full(s, float("nan"), device="cuda", dtype=BF)
    nanf = lambda *s: torch.full(s, float("nan"), device="cuda")
    mask = torch.ones((1, 64), dtype=torch.int32, device="cuda")
    qkv = torch.zeros((64, 3 * 96), device="cuda", dtype=BF)
    cases = []
    ctx = nanb(64, 96)
    cases.append(("attention S=48", _op(lib, 1, [qkv, mask, ctx, None], [1, 48, 1, 32], [1.0]), ctx))
    ctx2 = nanb(64, 96)
    cases.append(("attention DH=96", _op(lib, 1, [qkv, mask, ctx2, None], [1, 64, 1, 96], [1.0]), ctx2))
    c = nanb(64, 64)
    a = torch.zeros((64, 64), device="cuda", dtype=BF)
    cases.append(("gemm K=48", _gemm(lib, a, a, c, 64, 64, 48, 64, 64, 64), c))
    sc = nanb(1, 1, 6, 6)
    cases.append(("softmax S=6", _op(lib, 3, [sc, mask], [1, 1, 6], [1.0]), sc))
    y = nanb(4, 1032)
    x = torch.zeros((4, 1032), device="cuda", dtype=BF)
    gm = torch.ones(1032, device="cuda")
    cases.append(("layernorm H=1032", _op(lib, 5, [x, None, gm, gm, y, None, None, None], [4, 1032], [1e-5]), y))
    ct = nanf(400, 128)
    t = torch.zeros((64, 400), device="cuda", dtype=BF)
    cases.append(("gemm_tn M=400", _op(lib, 17, [t, t, ct], [400, 128, 128, 64, 400, 128]), ct))
    cw = nanb(64, 96)
    cases.append(("wrong argument count", _op(lib, 1, [qkv, mask, cw], [1, 64, 1, 32], [1.0]), cw))
    torch.cuda.synchronize()
    for what, rc, buf in cases:
        assert rc != 0, f"{what} was not refused"
        assert torch.isnan(buf.float()).all(), f"{what}: refused, but the output was written"
    assert _op(lib, 1, [qkv, mask, ctx], [1, 64, 1, 32], [1.0]) == 1      # SSKD_ERR_INVALID
    assert _op(lib, 99, [], []) == 1


# ----------------------------------------------------------------------------------------------------------------------
# batch invariance of the plain products
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", [0, 1])
def test_plain_products_are_batch_invariant(gpu, native_lib, backend):
    """A row of a plain product must not depend on how many rows are computed with it (a pair's teacher score must not
    depend on its batch-mates, csrc/train.hip): rows 0..1023 of an M = 2048 product equal, bit for bit, the same rows as an
    M = 1024 product, and a repeated call is bit-identical - on the library route (backend 0) and the hand-written one."""
    from semantic_search_kd_amd import _native

    lib = native_lib
    prev = lib.sskd_gemm_backend(-1)
    g = torch.Generator(device="cuda").manual_seed(100)
    try:
        lib.sskd_gemm_backend(backend)
        for N, K in ((3072, 1024), (1024, 4096)):
            A = _rand((2048, K), g)
            B = _rand((N, K), g, K ** -0.5)
            bias = torch.randn(N, generator=g, device="cuda")
            outs = []
            for M in (2048, 1024, 2048):
                c = torch.full((M, N), float("nan"), device="cuda", dtype=BF)
                _native.check(_gemm(lib, A, B, c, M, N, K, K, K, N, bias))
                outs.append(c)
            torch.cuda.synchronize()
            _bits_equal(outs[1], outs[0][:1024], f"backend {backend} N={N} K={K}: M=1024 rows vs the same rows of M=2048")
            _bits_equal(outs[2], outs[0], f"backend {backend} N={N} K={K}: repeat")
    finally:
        lib.sskd_gemm_backend(prev)
