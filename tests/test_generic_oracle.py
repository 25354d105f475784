"""CPU: the hand-written fp64 backward formulas of oracle/generic_ops.py against torch.autograd in fp64.

tests/test_generic_kernels_gpu.py holds every generic.hip kernel against these references, so they are pinned here first:
attention (with padded and holed masks and a row without any valid key), softmax, LayerNorm with and without the residual
gradient dy2, GELU, and masked mean pooling with and without L2 normalisation.  Everything is fp64: the bound is 1e-10
relative to the gradient's largest element.
"""
import numpy as np
import pytest
import torch

from oracle import generic_ops as go

F64 = torch.float64


def _close(got, want, what):
    got, want = got.double(), want.double()
    scale = want.abs().max().item() + 1e-300
    err = (got - want).abs().max().item()
    assert err <= 1e-10 * scale, f"{what}: max |err| {err:.3e} vs max |ref| {scale:.3e}"


def _bf16(x):
    return x.to(torch.bfloat16)


def test_round_bf16_is_round_to_nearest_even():
    vals = torch.tensor([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8 + 2 ** -20, -2.5, 0.0, -0.0, 3.0e38, 1e-40],
                        dtype=torch.float32)
    want = torch.tensor([1.0, 1.0, 1.0 + 2 ** -6, 1.0 + 2 ** -7, -2.5, 0.0, -0.0, 3.0e38, 1e-40], dtype=torch.float32)
    got = go.round_bf16(vals)
    assert torch.equal(got, _bf16(want).double())
    x = torch.randn(10000, dtype=torch.float32) * 100
    assert torch.equal(go.round_bf16(x), _bf16(x).double())   # torch's fp32 -> bf16 cast is RNE
    assert torch.equal(go.bf16_ulp(torch.tensor([1.0, 1.5, 2.0, -3.0])), torch.tensor([2 ** -7, 2 ** -7, 2 ** -6, 2 ** -6], dtype=F64))


@pytest.mark.parametrize("S,DH,heads", [(64, 32, 2), (96, 64, 1)])
def test_attention_forward_and_backward_formulas_match_autograd(S, DH, heads):
    g = torch.Generator().manual_seed(S + DH)
    B, H = 3, heads * DH
    qkv = torch.randn(B * S, 3 * H, generator=g, dtype=F64)
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[0, S - 7:] = 0          # right padding
    mask[1, 32:64] = 0           # a hole covering one whole key tile
    mask[2] = 0                  # no valid key at all
    scale = 1.0 / DH ** 0.5
    ctx, lse, _ = go.attention_fwd(qkv, mask, B, S, heads, DH, scale, round_p=False)

    q, k, v = (t.clone().requires_grad_(True) for t in go._split_heads(qkv, B, S, heads, DH))
    keep = (mask != 0).view(B, 1, 1, S)
    out = go.masked_attention_autograd(q, k, v, keep, scale)
    _close(ctx, go._merge_heads(out.detach()), "ctx")
    assert torch.all(ctx[2 * S:] == 0) and torch.all(torch.isneginf(lse[2]))
    # lse (log2 domain) = log2 sum_j exp(scale q k_j) over valid keys
    s = (q.detach() @ k.detach().transpose(-1, -2)) * scale
    want_lse = torch.logsumexp(s.masked_fill(~keep, float("-inf")), -1) / np.log(2.0)
    _close(lse[:2], want_lse[:2], "lse")

    dctx = torch.randn(B * S, H, generator=g, dtype=F64)
    (out * go._split_heads(torch.cat([dctx] * 3, 1), B, S, heads, DH)[0]).sum().backward()
    dq, dk, dv = (go._merge_heads(t.grad) for t in (q, k, v))
    got, _, _ = go.attention_bwd(qkv, mask, ctx, dctx, B, S, heads, DH, scale)
    _close(got[:, :H], dq, "dQ")
    _close(got[:, H:2 * H], dk, "dK")
    _close(got[:, 2 * H:], dv, "dV")
    # the same with the forward's saved lse fed back in, as the kernel does
    got2, _, _ = go.attention_bwd(qkv, mask, ctx, dctx, B, S, heads, DH, scale, lse=lse)
    _close(got2, got, "dqkv from the saved lse")
    assert torch.all(got[2 * S:] == 0)


def test_softmax_formulas_match_autograd():
    g = torch.Generator().manual_seed(5)
    B, heads, S, scale = 2, 3, 12, 0.37
    x = torch.randn(B, heads, S, S, generator=g, dtype=F64, requires_grad=True)
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[1, 5:] = 0
    keep = (mask != 0).view(B, 1, 1, S)
    p = torch.softmax((x * scale).masked_fill(~keep, float("-inf")), -1)
    P = go.softmax_fwd(x.detach(), mask, B, heads, S, scale)
    _close(P, p.detach().reshape(-1, S), "P")
    dp = torch.randn(B, heads, S, S, generator=g, dtype=F64)
    (p * dp).sum().backward()
    ds, _ = go.softmax_bwd(dp.reshape(-1, S), P, scale)
    _close(ds, x.grad.reshape(-1, S), "dS")


@pytest.mark.parametrize("with_dy2", [False, True])
def test_layernorm_formulas_match_autograd(with_dy2):
    g = torch.Generator().manual_seed(7)
    M, H, eps = 9, 40, 1e-5
    z = (torch.randn(M, H, generator=g, dtype=F64) * 3 + 5).requires_grad_(True)
    gamma = torch.randn(H, generator=g, dtype=F64, requires_grad=True)
    beta = torch.randn(H, generator=g, dtype=F64, requires_grad=True)
    y_ref, _, mean, rstd, _ = go.add_ln_fwd(z.detach(), None, gamma.detach(), beta.detach(), eps, round_z=False)
    y = torch.nn.functional.layer_norm(z, (H,), gamma, beta, eps)
    _close(y_ref, y.detach(), "y")
    dy = torch.randn(M, H, generator=g, dtype=F64)
    dy2 = torch.randn(M, H, generator=g, dtype=F64) if with_dy2 else None
    (y * (dy + (dy2 if with_dy2 else 0))).sum().backward()
    dz, dgamma, dbeta, dz_colsum, *_ = go.ln_bwd(dy, z.detach(), mean, rstd, gamma.detach(), dy2)
    _close(dz, z.grad, "dz")
    _close(dgamma, gamma.grad, "dgamma")
    _close(dbeta, beta.grad, "dbeta")
    assert torch.equal(dz_colsum, go.round_bf16(dz).sum(0))


def test_gelu_formulas_match_autograd():
    u = torch.linspace(-12, 12, 2001, dtype=F64, requires_grad=True)
    h = torch.nn.functional.gelu(u)
    _close(go.gelu(u.detach()), h.detach(), "gelu")
    dh = torch.cos(torch.arange(2001, dtype=F64))
    (h * dh).sum().backward()
    _close(go.gelu_bwd(u.detach(), dh), u.grad, "gelu backward")
    du, db, _ = go.gelu_bwd_colsum(u.detach().view(1, -1), dh.view(1, -1))
    assert torch.equal(db, go.round_bf16(du)[0])


@pytest.mark.parametrize("normalize", [False, True])
def test_pool_formulas_match_autograd(normalize):
    g = torch.Generator().manual_seed(11)
    B, S, H = 3, 7, 20
    hidden = torch.randn(B, S, H, generator=g, dtype=F64, requires_grad=True)
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[0, 3:] = 0
    mask[2] = 0                  # all masked: finite zeros
    m = mask.to(F64)[..., None]
    pooled = (hidden * m).sum(1) / m.sum(1).clamp_min(1e-9)
    out = torch.nn.functional.normalize(pooled, dim=-1, eps=1e-12) if normalize else pooled
    got, got_pooled, _ = go.pool_fwd(hidden.detach(), mask, normalize)
    _close(got, out.detach(), "pool out")
    _close(got_pooled, pooled.detach(), "pooled")
    dout = torch.randn(B, H, generator=g, dtype=F64)
    (out * dout).sum().backward()
    dh, _ = go.pool_bwd(dout, got_pooled, mask, normalize)
    _close(dh, hidden.grad, "dhidden")
    assert torch.all(dh[2] == 0) and torch.isfinite(dh).all()


def test_embedding_references():
    g = torch.Generator().manual_seed(13)
    vocab, n_pos, B, S, H = 10, 12, 2, 4, 16
    ids = torch.tensor([[0, 3, 3, 99], [-5, 3, 9, 1]], dtype=torch.int32)
    mask = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 0]], dtype=torch.int32)
    dz = torch.randn(B * S, H, generator=g, dtype=F64)
    dword, dpos, dtype0, *_ = go.embed_bwd(ids, mask, dz, vocab, n_pos, S, 2)
    want = torch.zeros(vocab, H, dtype=F64)
    for m, i in enumerate(ids.reshape(-1).tolist()):
        if mask.reshape(-1)[m]:
            want[min(max(i, 0), vocab - 1)] += dz[m]
    _close(dword, want, "dword")
    assert torch.all(dpos[:2] == 0) and torch.all(dpos[6:] == 0)
    _close(dpos[2:6], dz[:4] + dz[4:] * mask[1].to(F64)[:, None], "dpos")
    _close(dtype0, (dz * mask.reshape(-1, 1)).sum(0), "dtype0")


def test_attention_register_roundings_mirror_the_online_softmax():
    """``attention_fwd(round_p="running")`` against a plain loop over 32-key tiles that keeps a running maximum, rounds the
    tile's exponentials to bf16 relative to it and rescales the sums when it moves (what the kernel does); with one tile it
    is ``round_p=True``.  ``attention_bwd(round_ps=True)`` against the three products written out with rounded P and dS; both
    stay within one rounding (2^-8 of the terms' magnitude) of the unrounded formulas that autograd pins above."""
    g = torch.Generator().manual_seed(17)
    B, S, heads, DH = 2, 96, 2, 32
    H = heads * DH
    qkv = go.round_bf16(torch.randn(B * S, 3 * H, generator=g, dtype=F64) * 1.5)
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[1, 41:] = 0
    scale = 1.0 / DH ** 0.5
    ctx, lse, mag = go.attention_fwd(qkv, mask, B, S, heads, DH, scale, round_p="running")
    plain, lse0, _ = go.attention_fwd(qkv, mask, B, S, heads, DH, scale, round_p=False)
    assert torch.equal(lse, lse0)
    assert bool(((ctx - plain).abs() <= 2.0 ** -8 * mag).all()) and not torch.equal(ctx, plain)
    s, _ = go.attention_scores(qkv, mask, B, S, heads, DH, scale)
    _, _, v = go._split_heads(qkv, B, S, heads, DH)
    m = torch.full((B, heads, S, 1), float("-inf"), dtype=F64)
    l = torch.zeros(B, heads, S, 1, dtype=F64)
    o = torch.zeros(B, heads, S, DH, dtype=F64)
    for kt in range(S // 32):
        st = s[..., 32 * kt:32 * kt + 32]
        if not torch.isfinite(st).any():
            continue
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - m_new))
        e = torch.exp2(st - m_new)
        l, o, m = l * alpha + e.sum(-1, keepdim=True), o * alpha + go.round_bf16(e) @ v[:, :, 32 * kt:32 * kt + 32], m_new
    _close(ctx, go._merge_heads(o / l), "ctx with P rounded against the running maximum")
    one_tile = [go.attention_fwd(qkv[:64], mask[:, :32], 2, 32, heads, DH, scale, round_p=r)[0] for r in ("running", True)]
    assert torch.equal(one_tile[0], one_tile[1])      # two sequences of 32 keys: the running maximum is the final one

    dctx = go.round_bf16(torch.randn(B * S, H, generator=g, dtype=F64))
    ctx_b = go.round_bf16(plain)
    got, _, _ = go.attention_bwd(qkv, mask, ctx_b, dctx, B, S, heads, DH, scale, lse=lse, round_ps=True)
    ref, mag_b, _ = go.attention_bwd(qkv, mask, ctx_b, dctx, B, S, heads, DH, scale, lse=lse)
    assert bool(((got - ref).abs() <= 2.0 ** -8 * mag_b).all()) and not torch.equal(got, ref)
    q, k, _ = go._split_heads(qkv, B, S, heads, DH)
    p = torch.where(torch.isinf(s), torch.zeros_like(s), torch.exp2(s - lse[..., None]))
    do = dctx.view(B, S, heads, DH).permute(0, 2, 1, 3)
    D = (do * ctx_b.view(B, S, heads, DH).permute(0, 2, 1, 3)).sum(-1, keepdim=True)
    ds = go.round_bf16(p * (do @ v.transpose(-1, -2) - D) * scale)
    want = torch.cat([go._merge_heads(t) for t in (ds @ k, ds.transpose(-1, -2) @ q, go.round_bf16(p).transpose(-1, -2) @ do)], 1)
    _close(got, want, "dqkv with P and dS rounded")
