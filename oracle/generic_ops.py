"""fp64 references of the generic path's kernels (csrc/generic.hip) - TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

Every function takes the kernel's own inputs (bf16 tensors, fp32 where the kernel takes fp32) and computes the operation
in float64 on the CPU.  Where a kernel rounds an intermediate to bf16 BY DESIGN, the reference applies the same
round-to-nearest-even at the same point (``round_bf16``), so that the per-element bounds of
tests/test_generic_kernels_gpu.py stay tight:

  * ``attention_fwd``: the probabilities P before the PV product;
  * ``add_ln_fwd``: z = a + b when it is saved (the kernel then normalises the saved bf16 z);
  * ``gelu_bwd_colsum``: the column sum adds du AS STORED (bf16);
  * ``ln_bwd``: ``dz_colsum`` adds dz AS STORED (bf16).

Two further roundings happen in REGISTERS of the fused attention kernels (the bf16 operand of an MFMA).  The per-kernel
tests cover them with a 2^-8 term in the bound; the chained reference of the whole step (oracle/generic_step.py) asks for
them, because it is compared with a gate that has no such term:

  * ``attention_fwd(round_p="running")``: P of key tile kt (32 keys) is rounded relative to the row's maximum over
    tiles 0 .. kt, as the online softmax does, not relative to the final maximum;
  * ``attention_bwd(round_ps=True)``: P is rounded before P^T dO and dS before dS K and dS^T Q.

Besides the value, most functions return ``mag``: per output element, the sum of the absolute values of the terms that
make it (sum_k |a_ik| |b_jk| for a product, sum |x| for a column sum ...).  An fp32 accumulation of n such terms is off by
at most n * 2^-24 * mag; the tests build their bounds from it.

The backward formulas here are written out by hand (they are what the kernels implement);
tests/test_generic_oracle.py pins each of them against ``torch.autograd`` in fp64.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

F64 = torch.float64
LOG2E = 1.4426950408889634


def f64(x) -> torch.Tensor:
    return x.detach().to("cpu", F64) if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=F64)


def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16 with round-to-nearest-even from the fp32 value (the kernels round fp32 registers), as float64."""
    b = x.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    nan = torch.isnan(x.to(torch.float32))
    r = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    r = torch.where(r >= 0x80000000, r - (1 << 32), r).to(torch.int32)
    out = r.view(torch.float32).to(F64)
    return torch.where(nan, torch.full_like(out, float("nan")), out)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """One bf16 ulp of |x| (the spacing of bf16 numbers at |x|; the smallest normal's spacing at and below 2^-126)."""
    a = f64(x).abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


# ----------------------------------------------------------------------------------------------------------------------
# products
# ----------------------------------------------------------------------------------------------------------------------
def gemm_nt(a, b, bias=None, alpha: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """alpha * A[.., M, K] . B[.., N, K]^T + bias[N] (before any activation) and its magnitude |alpha| |A| |B|^T + |bias|."""
    A, B = f64(a), f64(b)
    ref = alpha * (A @ B.transpose(-1, -2))
    mag = abs(alpha) * (A.abs() @ B.abs().transpose(-1, -2))
    if bias is not None:
        ref = ref + f64(bias)
        mag = mag + f64(bias).abs()
    return ref, mag


def gemm_tn(a, b) -> Tuple[torch.Tensor, torch.Tensor]:
    """A[T, M]^T . B[T, N] and |A|^T |B|."""
    A, B = f64(a), f64(b)
    return A.T @ B, A.abs().T @ B.abs()


def gelu(x) -> torch.Tensor:
    x = f64(x)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x) -> torch.Tensor:
    x = f64(x)
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ----------------------------------------------------------------------------------------------------------------------
# attention (qkv [B*S, 3H] row-major: Q | K | V column blocks, head h = columns h*DH .. of each block)
# ----------------------------------------------------------------------------------------------------------------------
def _split_heads(qkv, B: int, S: int, heads: int, DH: int):
    x = f64(qkv).view(B, S, 3, heads, DH).permute(2, 0, 3, 1, 4)   # [3, B, heads, S, DH]
    return x[0], x[1], x[2]


def _merge_heads(x: torch.Tensor) -> torch.Tensor:
    B, NH, S, DH = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, NH * DH)


def attention_scores(qkv, mask, B, S, heads, DH, scale):
    """log2-domain scaled scores scale * log2(e) * Q K^T with masked keys at -inf, [B, heads, S, S]."""
    q, k, _ = _split_heads(qkv, B, S, heads, DH)
    s = (q @ k.transpose(-1, -2)) * (scale * LOG2E)
    keep = f64(mask).view(B, 1, 1, S) != 0
    return s.masked_fill(~keep, float("-inf")), keep


def attention_fwd(qkv, mask, B, S, heads, DH, scale, round_p=True):
    """ctx [B*S, H] and lse [B, heads, S] (log2 domain) of softmax(scale Q K^T + mask) V.

    The kernel multiplies bf16(P) (relative to its running row maximum) by V and divides by the fp32 sum of the UNROUNDED
    exponentials; with ``round_p`` the reference does the same with P relative to the row's final maximum, and with
    ``round_p="running"`` relative to the maximum over the valid keys of the 32-key tiles up to and including the key's
    own (what the kernel's online softmax holds when it rounds that tile; later tiles rescale the sum exactly).  A row
    without any valid key: ctx = 0 and lse = -inf (the project's contract, csrc/generic.h).
    Also returns mag [B*S, H] = sum_j P_ij |V_jd| (what the bf16 rounding of P is relative to)."""
    s, keep = attention_scores(qkv, mask, B, S, heads, DH, scale)
    _, _, v = _split_heads(qkv, B, S, heads, DH)
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m)
    e = torch.exp2(s - torch.where(empty, torch.zeros_like(m), m))
    e = torch.where(empty, torch.zeros_like(e), e)
    l = e.sum(-1, keepdim=True)
    if isinstance(round_p, str):
        if round_p != "running":
            raise ValueError(round_p)
        mt = s.view(B, heads, S, S // 32, 32).amax(-1).cummax(-1).values.repeat_interleave(32, -1)   # [B, heads, S, S]
        none = torch.isinf(mt)
        er = torch.exp2(s - torch.where(none, torch.zeros_like(mt), mt))
        er = torch.where(none, torch.zeros_like(er), er)
        pe = round_bf16(er) * torch.exp2(torch.where(none, torch.zeros_like(mt), mt - m))
    else:
        pe = round_bf16(e) if round_p else e
    inv = torch.where(l > 0, 1.0 / l.clamp_min(1e-300), torch.zeros_like(l))
    ctx = (pe @ v) * inv
    mag = (e @ v.abs()) * inv
    lse = torch.where(empty, torch.full_like(m, float("-inf")), m + torch.log2(l.clamp_min(1e-300)))[..., 0]
    return _merge_heads(ctx), lse, _merge_heads(mag)


def attention_bwd(qkv, mask, ctx, dctx, B, S, heads, DH, scale, lse=None, round_ps: bool = False):
    """dqkv [B*S, 3H] of the fused backward:
        P  = exp2(s - lse)   (lse: the forward's saved log-sum-exp when given, else the exact one)
        D  = rowsum(dO o O)  with O = the GIVEN ctx (the kernel reads the forward's bf16 output)
        dS = P o (dO V^T - D) * scale,   dQ = dS K,   dK = dS^T Q,   dV = P^T dO.
    ``round_ps``: P and dS are rounded to bf16 before these three products, as the kernel packs them.
    Rows without a valid key contribute nothing.  Also returns mag [B*S, 3H]: sum_j |dS_ij| |K_jd| for dQ,
    sum_i |dS_ij| |Q_id| for dK, sum_i P_ij |dO_id| for dV; and mag_d: the same sums with |dS_ij| replaced by
    P_ij scale (sum_d |dO_id| (|V_jd| + |O_id|)), what the fp32 error of dP - D is relative to."""
    s, keep = attention_scores(qkv, mask, B, S, heads, DH, scale)
    q, k, v = _split_heads(qkv, B, S, heads, DH)
    o = f64(ctx).view(B, S, heads, DH).permute(0, 2, 1, 3)
    do = f64(dctx).view(B, S, heads, DH).permute(0, 2, 1, 3)
    if lse is None:
        _, lse, _ = attention_fwd(qkv, mask, B, S, heads, DH, scale, round_p=False)
    L = f64(lse).view(B, heads, S, 1)
    p = torch.exp2(s - torch.where(torch.isinf(L), torch.zeros_like(L), L))
    p = torch.where(torch.isinf(s) | torch.isinf(L), torch.zeros_like(p), p)
    dp = do @ v.transpose(-1, -2)
    D = (do * o).sum(-1, keepdim=True)
    ds = p * (dp - D) * scale
    pr, dsr = (round_bf16(p), round_bf16(ds)) if round_ps else (p, ds)
    dq, dk, dv = dsr @ k, dsr.transpose(-1, -2) @ q, pr.transpose(-1, -2) @ do
    mq, mk, mv = ds.abs() @ k.abs(), ds.abs().transpose(-1, -2) @ q.abs(), p.transpose(-1, -2) @ do.abs()
    out = torch.cat([_merge_heads(dq), _merge_heads(dk), _merge_heads(dv)], 1)
    mag = torch.cat([_merge_heads(mq), _merge_heads(mk), _merge_heads(mv)], 1)
    # dP - D cancels (exactly, when a query sees one key): its fp32 error is relative to sum_d |dO| (|V_j| + |O|), not |dS|
    pe = p * (do.abs() @ v.abs().transpose(-1, -2) + (do * o).abs().sum(-1, keepdim=True)) * abs(scale)
    cq, ck = pe @ k.abs(), pe.transpose(-1, -2) @ q.abs()
    mag_d = torch.cat([_merge_heads(cq), _merge_heads(ck), torch.zeros_like(_merge_heads(cq))], 1)
    return out, mag, mag_d


def softmax_fwd(scores, mask, B, heads, S, scale):
    """P = softmax(scale * s + (key masked ? -inf : 0)) over rows of [B, heads, S, S]; all-masked rows -> 0."""
    x = f64(scores).view(B, heads, S, S) * scale
    keep = f64(mask).view(B, 1, 1, S) != 0
    x = x.masked_fill(~keep, float("-inf"))
    m = x.amax(-1, keepdim=True)
    e = torch.exp(x - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    e = torch.where(torch.isinf(x), torch.zeros_like(e), e)
    l = e.sum(-1, keepdim=True)
    return torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e)).reshape(-1, S)


def softmax_bwd(dp, p, scale):
    """dS = scale * P o (dP - sum_j dP_j P_j) per row; mag = scale |P| (|dP| + sum_j |dP_j P_j|)."""
    dP, P = f64(dp), f64(p)
    dot = (dP * P).sum(-1, keepdim=True)
    adot = (dP * P).abs().sum(-1, keepdim=True)
    return scale * P * (dP - dot), abs(scale) * P.abs() * (dP.abs() + adot)


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------------------
def add_ln_fwd(a, b, gamma, beta, eps: float, round_z: bool):
    """z = a (+ b) (rounded to bf16 when the kernel saves it), y = (z - mean) rstd gamma + beta.  Returns
    y, z, mean, rstd, and mag = |z - mean| rstd |gamma| + |beta| (what y's fp32 arithmetic is relative to)."""
    z = f64(a) + (f64(b) if b is not None else 0.0)
    if round_z:
        z = round_bf16(z)
    mean = z.mean(-1)
    var = ((z - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (z - mean[:, None]) * rstd[:, None]
    y = xh * f64(gamma) + f64(beta)
    return y, z, mean, rstd, xh.abs() * f64(gamma).abs() + f64(beta).abs()


def ln_bwd(dy, z, mean, rstd, gamma, dy2=None):
    """LayerNorm backward with the kernel's saved statistics:  d = dy (+ dy2), g = d gamma, xh = (z - mean) rstd,
        dz = rstd (g - mean(g) - xh mean(g xh)),  dgamma = sum_rows d xh,  dbeta = sum_rows d,
        dz_colsum = sum_rows bf16(dz)   (the kernel sums dz AS STORED).
    Returns dz, dgamma, dbeta, dz_colsum and the magnitudes: per dz element rstd (|g| + mean|g| + |xh| mean|g xh|),
    per column sum_rows |d xh|, sum_rows |d|, sum_rows |bf16(dz)|."""
    d = f64(dy) + (f64(dy2) if dy2 is not None else 0.0)
    xh = (f64(z) - f64(mean)[:, None]) * f64(rstd)[:, None]
    g = d * f64(gamma)
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    r = f64(rstd)[:, None]
    dz = r * (g - s1 - xh * s2)
    mag = r * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    dzr = round_bf16(dz)
    return (dz, (d * xh).sum(0), d.sum(0), dzr.sum(0),
            mag, (d * xh).abs().sum(0), d.abs().sum(0), dzr.abs().sum(0))


# ----------------------------------------------------------------------------------------------------------------------
# elementwise, reductions, embeddings, pooling
# ----------------------------------------------------------------------------------------------------------------------
def gelu_bwd(u, dh) -> torch.Tensor:
    return f64(dh) * gelu_grad(u)


def gelu_bwd_colsum(u, dh):
    """du = dh gelu'(u) and db = column sums of bf16(du) (the kernel sums du as stored); also sum |bf16(du)|."""
    du = gelu_bwd(u, dh)
    r = round_bf16(du)
    return du, r.sum(0), r.abs().sum(0)


def colsum(y):
    Y = f64(y)
    return Y.sum(0), Y.abs().sum(0)


def embed_fwd(ids, word, pos, type0, S: int, pos_offset: int):
    """z[m] = bf16((word[clamp(id)] + pos[m % S + pos_offset]) + type0) with the two additions in fp32, as the kernel."""
    vocab = word.shape[0]
    i = ids.reshape(-1).long().clamp(0, vocab - 1)
    t = torch.arange(i.numel()) % S + pos_offset
    w, p, ty = word.float().cpu()[i], pos.float().cpu()[t], type0.float().cpu()[None, :]
    return round_bf16((w + p) + ty)


def embed_bwd(ids, mask, dz, vocab: int, n_pos: int, S: int, pos_offset: int):
    """dword[id] += dz (clamped ids, unmasked tokens), dpos[t + pos_offset] += dz, dtype0 += dz; with magnitudes."""
    i = ids.reshape(-1).long().clamp(0, vocab - 1)
    keep = mask.reshape(-1).cpu() != 0
    d = f64(dz).reshape(i.numel(), -1) * keep[:, None]
    H = d.shape[1]
    t = torch.arange(i.numel()) % S + pos_offset
    dword = torch.zeros(vocab, H, dtype=F64).index_add_(0, i, d)
    dpos = torch.zeros(n_pos, H, dtype=F64).index_add_(0, t, d)
    mword = torch.zeros(vocab, H, dtype=F64).index_add_(0, i, d.abs())
    mpos = torch.zeros(n_pos, H, dtype=F64).index_add_(0, t, d.abs())
    return dword, dpos, d.sum(0), mword, mpos, d.abs().sum(0)


def pool_fwd(hidden, mask, normalize: bool):
    """Masked mean over the sequence (+ L2 normalise); returns out, pooled (pre-normalise) and mag = sum |h| / n."""
    h = f64(hidden)
    m = f64(mask)[..., None]
    n = m.sum(1).clamp_min(1e-9)
    pooled = (h * m).sum(1) / n
    mag = (h.abs() * m).sum(1) / n
    if not normalize:
        return pooled, pooled, mag
    nrm = pooled.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return pooled / nrm, pooled, mag / nrm


def pool_bwd(dout, pooled, mask, normalize: bool):
    """dhidden[b, t] = mask[b, t] / n_b * (normalize ? (g - e_hat (e_hat . g)) / |e| : g)."""
    g, e = f64(dout), f64(pooled)
    m = f64(mask)
    n = m.sum(1, keepdim=True).clamp_min(1e-9)
    if normalize:
        nrm = e.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        eh = e / nrm
        mag = (g.abs() + eh.abs() * (eh * g).abs().sum(-1, keepdim=True)) / nrm
        g = (g - eh * (eh * g).sum(-1, keepdim=True)) / nrm
    else:
        mag = g.abs()
    w = (m / n)[..., None]
    return w * g[:, None, :], w * mag[:, None, :]


def masked_attention_autograd(q, k, v, keep, scale):
    """softmax(scale q k^T, masked keys excluded) v with torch ops only (rows without a key give 0): the autograd side of
    tests/test_generic_oracle.py."""
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~keep, float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.nan_to_num(p, nan=0.0)
    return p @ v
