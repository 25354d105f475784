"""fp64 references of the inference encoder's kernels (csrc/encoder.hip) - TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

One function per kernel.  Each takes the kernel's OWN inputs (the bf16 activations it read, bf16 weights, fp32 biases and
LayerNorm parameters), computes the operation in float64 and returns, besides the value, the magnitude terms that the
bounds of tests/test_encoder_kernels_gpu.py are built from.  Where a kernel rounds an intermediate to bf16 BY DESIGN the
reference rounds at the same point (``rounding=True``); the rounding points, with the lines of csrc/encoder.hip:

  * ``embed_ln``       none inside: fp32 sum word + type + pos (l. 163), two-pass LayerNorm, one rounding at the store (l. 184).
  * ``qkv_attention``  Q = bf16((x Wq^T + bq) * log2(e)/sqrt(32)) (l. 935), K = bf16(x Wk^T + bk) (l. 936),
                       V = bf16(x Wv^T + bv) (l. 937); scores in log2 units, masked keys at -1e30 (l. 764, 1025, 1032:
                       excluded here), base-2 softmax; the context is rounded once at the store (l. 1081-1082).
                       P is rounded to bf16 relative to the RUNNING maximum (l. 1060-1062) while its sum is not (l. 1061):
                       that cannot be mirrored and is bounded instead (2^-8 sum_j p_j |v_j|).
  * ``fused_mlp``      X1 = bf16(LN1(x + ctx Wo^T + bo)) (l. 318, 359-360), A = bf16(gelu(X1 W1^T + b1)) (l. 531, 653),
                       out = bf16(LN2(X1 + A W2^T + b2)) (l. 622, 753-754).  gelu is the kernel's DESIGNED function
                       x * sigmoid(x (a + b x^2 + c x^4)) (csrc/common.h gelu_erf), restated here in float64
                       (``gelu_kernel_form``); tests/test_encoder_oracle.py pins it to the exact erf form within the
                       2.6e-5 the kernel documents.  Both LayerNorms take the variance as E[z^2] - mean^2 (l. 341, 735).
  * ``pool``           none: fp32 masked mean and L2 normalisation, fp32 output.

``rounding=False`` switches every rounding off and uses the exact erf GELU: the chain of these functions is then the
plain model, equal to ``oracle.encoder.bert_hidden_states(dtype=float64)`` (pinned in tests/test_encoder_oracle.py).

``acc="f32"`` evaluates the same operation the way an ideal fp32 kernel would: products and sums accumulated in fp32, the
attention as the kernel's tile loop (two key tiles per step, online softmax, P rounded relative to the running maximum).
It exists to MEASURE what fp32 accumulation does to the fp64 reference (the flip shares behind the caps of the GPU
tests) and to carry the planted defects of the sharpness check (``defect=``): it is never a reference.

Bounds (u = 2^-24):  see ``ln_propagate`` for the LayerNorm propagation and the docstrings of ``attention_bounds`` /
``mlp_bounds`` for the two tiers (tight bound T, flip band F).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from .generic_ops import F64, bf16_ulp, f64, round_bf16

U = 2.0 ** -24
H, NH, DH, FF = 384, 12, 32, 1536
LN2 = math.log(2.0)
# the kernel's scale: fp32 log2(e) / sqrtf(32) (csrc/encoder.hip l. 1363)
Q_SCALE = float(np.float32(1.4426950408889634) / np.sqrt(np.float32(DH)))
GELU_A, GELU_B, GELU_C = (float(np.float32(v)) for v in (-2.3011212, -0.10677574, 0.0010142655))
GELU_SLOPE = 1.13   # max |gelu'| (1.129 at x = 1.41)


def _rnd(x: torch.Tensor, on: bool) -> torch.Tensor:
    return round_bf16(x) if on else x


def _mm(a: torch.Tensor, b: torch.Tensor, acc: str) -> torch.Tensor:
    """a @ b^T, accumulated in float64 or in fp32."""
    if acc == "f32":
        return (a.to(torch.float32) @ b.to(torch.float32).transpose(-1, -2)).to(F64)
    return a @ b.transpose(-1, -2)


def gelu_exact(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_kernel_form(x: torch.Tensor) -> torch.Tensor:
    """csrc/common.h gelu_erf in float64: x * sigmoid(-log2e-scaled cubic in x^2), polynomial on clamp(x, -8, 8)."""
    xc = x.clamp(-8.0, 8.0)
    x2 = xc * xc
    q = (GELU_C * x2 + GELU_B) * x2 + GELU_A
    return x / (1.0 + torch.exp2(q * xc))


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm and its error propagation
# ----------------------------------------------------------------------------------------------------------------------
def layer_norm(z: torch.Tensor, gamma, beta, eps: float, acc: str = "f64", one_pass: bool = False):
    """y = (z - mean) rstd gamma + beta over the last axis; returns y, xhat, rstd [.., 1]."""
    g, b = f64(gamma), f64(beta)
    if acc == "f32":
        zf = z.to(torch.float32)
        mean = zf.mean(-1, keepdim=True)
        if one_pass:
            var = ((zf * zf).mean(-1, keepdim=True) - mean * mean).clamp_min(0.0)
        else:
            var = ((zf - mean) ** 2).mean(-1, keepdim=True)
        rstd = torch.rsqrt(var + np.float32(eps))
        xh = (zf - mean) * rstd
        y = xh * g.to(torch.float32) + b.to(torch.float32)
        return y.to(F64), xh.to(F64), rstd.to(F64)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (z - mean) * rstd
    return xh * g + b, xh, rstd


def ln_propagate(e: torch.Tensor, xhat: torch.Tensor, rstd: torch.Tensor, gamma) -> torch.Tensor:
    """First-order bound on the move of a LayerNorm output when its input z moves by at most e (element-wise, e >= 0).

    y_i = gamma_i xhat_i + beta_i with xhat_i = (z_i - mean) rstd, rstd = (var + eps)^-1/2.  Differentiating,
        d mean = mean(dz),   d var = 2 mean((z - mean) dz)   =>   d rstd = -rstd^3 mean((z - mean) dz) = -rstd^2 mean(xhat dz)
        d xhat_i = rstd (dz_i - mean(dz)) + (z_i - mean) d rstd = rstd (dz_i - mean(dz) - xhat_i mean(xhat dz)),
    so with |dz| <= e:   |dy_i| <= |gamma_i| rstd (e_i + mean(e) + |xhat_i| mean(e |xhat|))."""
    g = f64(gamma).abs()
    return g * rstd * (e + e.mean(-1, keepdim=True) + xhat.abs() * (e * xhat.abs()).mean(-1, keepdim=True))


def ln_fp32_slack(z, xhat, rstd, gamma, beta) -> torch.Tensor:
    """What the kernel's OWN fp32 LayerNorm arithmetic adds on exact inputs: the mean is an fp32 sum of H terms
    ((H + 8) u mean|z|), the variance E[z^2] - mean^2 two such sums (relative to mean(z^2) + mean^2, NOT to the variance:
    the one-pass form cancels), rsqrtf and the final multiply-adds a few u."""
    g, b = f64(gamma).abs(), f64(beta).abs()
    n = z.shape[-1]
    mean = z.mean(-1, keepdim=True)
    d_mean = (n + 8) * U * z.abs().mean(-1, keepdim=True)
    d_var = 2 * (n + 8) * U * ((z * z).mean(-1, keepdim=True) + mean * mean)
    rel_rstd = 0.5 * d_var * rstd * rstd + 4 * U
    return g * rstd * d_mean + xhat.abs() * g * rel_rstd + 4 * U * (xhat.abs() * g + b)


# ----------------------------------------------------------------------------------------------------------------------
# embed_ln_kernel
# ----------------------------------------------------------------------------------------------------------------------
def embed_ln(ids, pos_ids, word, pos, type0, gamma, beta, eps: float, acc: str = "f64") -> Dict[str, torch.Tensor]:
    """LN(word[clamp(id)] + type[0] + pos[pos_id]) for a flat list of tokens.  ``pos_ids``: the token's position, which
    restarts at its segment's ``lo`` in packed rows (l. 146-151).  ``T``: ulp(ref) for the one rounding at the store, the
    fp32 error of the three-term sum (2 u sum|terms|) propagated through the LayerNorm, and the LayerNorm's own fp32 slack."""
    i = torch.as_tensor(np.asarray(ids)).long().reshape(-1).clamp(0, word.shape[0] - 1)
    t = torch.as_tensor(np.asarray(pos_ids)).long().reshape(-1)
    w, p, ty = f64(word)[i], f64(pos)[t], f64(type0)[None, :]
    z = w + ty + p
    if acc == "f32":
        z = ((w.float() + ty.float()) + p.float()).to(F64)
    y, xh, rstd = layer_norm(z, gamma, beta, eps, acc)
    e = 2 * U * (w.abs() + ty.abs() + p.abs())
    T = bf16_ulp(y) + ln_propagate(e, xh, rstd, gamma) + ln_fp32_slack(z, xh, rstd, gamma, beta)
    return {"ref": y, "T": T}


# ----------------------------------------------------------------------------------------------------------------------
# qkv_attention_kernel (one batch row at a time: rows do not interact)
# ----------------------------------------------------------------------------------------------------------------------
def keep_from_mask(mask_row) -> torch.Tensor:
    """[S, S] allowed (query, key) pairs of an unpacked row: every query sees the unmasked keys."""
    m = torch.as_tensor(np.asarray(mask_row)) != 0
    return m[None, :].expand(m.numel(), -1).clone()


def keep_from_segments(seg_row) -> torch.Tensor:
    """[S, S] of a packed row (segment words lo | hi << 16, 0 = padding): block-diagonal per segment; padding queries
    see nothing."""
    w = torch.as_tensor(np.asarray(seg_row)).long()
    lo, hi = w & 0xFFFF, (w >> 16) & 0xFFFF
    t = torch.arange(w.numel())
    return (t[None, :] >= lo[:, None]) & (t[None, :] < hi[:, None])


def _heads(y: torch.Tensor) -> torch.Tensor:
    return y.view(y.shape[0], NH, DH).transpose(0, 1)   # [NH, S, DH]


def _project(x, w, b, acc, scale=1.0, drop=None):
    xx = x
    if drop is not None:      # planted defect: one k-step of 32 never reaches the accumulator
        xx = x.clone()
        xx[:, drop:drop + 32] = 0.0
    y = _mm(xx, f64(w), acc) + f64(b)
    if acc == "f32":
        return ((y.float()) * np.float32(scale)).to(F64) if scale != 1.0 else y
    return y * scale


def qkv_attention(x, wq, wk, wv, bq, bk, bv, keep, acc: str = "f64", rounding: bool = True,
                  defect: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """Context [S, 384] of one row: x [S, 384] (the kernel's bf16 input), weights [384, 384] bf16 values, keep [S, S].

    Returns ref and, per output element,
      pv_mag  = sum_j p_j |v_jd|                    what P's bf16 rounding and the fp32 P V sum are relative to,
      s_mag   = max_j sum_d |q_d| |k_jd|  [query]   the fp32 score sum's magnitude (over the keys the query sees),
      s_abs   = max_j |s_j|,
      F       = the flip band (see ``attention_bounds``),
      argmax  = [NH, S] the key position holding the row maximum (-1 for a query without keys).
    A query without any key gives 0 (the kernel: l = 0 -> inv = 0, l. 1076)."""
    X = f64(x)
    if defect == "bias_shift":   # planted defect: the bias columns land 8 further (one lane group)
        bq, bk, bv = (torch.roll(f64(b), 8) for b in (bq, bk, bv))
    drop = 32 if defect == "drop_k" else None
    # unrounded = the plain model: the exact log2(e) / sqrt(32), not the kernel's fp32 constant
    q = _rnd(_project(X, wq, bq, acc, Q_SCALE if rounding else math.log2(math.e) / math.sqrt(DH), drop), rounding)
    k = _rnd(_project(X, wk, bk, acc), rounding)
    v = _rnd(_project(X, wv, bv, acc), rounding)
    qh, kh, vh = _heads(q), _heads(k), _heads(v)
    keep = keep.bool()
    S = X.shape[0]
    if acc == "f32":
        ctx = _attention_tiles_f32(qh, kh, vh, keep, skip_last_rescale=(defect == "late_rescale"))
        return {"ref": ctx.transpose(0, 1).reshape(S, H)}
    s = (qh @ kh.transpose(-1, -2)).masked_fill(~keep[None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m)
    e = torch.exp2(s - torch.where(empty, torch.zeros_like(m), m))
    e = torch.where(empty, torch.zeros_like(e), e)
    l = e.sum(-1, keepdim=True)
    p = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros_like(e))
    ctx = p @ vh
    pv_mag = p @ vh.abs()
    kz = keep[None].to(F64)
    s_mag = ((qh.abs() @ kh.abs().transpose(-1, -2)) * kz).amax(-1, keepdim=True)
    s_abs = (torch.nan_to_num(s, neginf=0.0).abs() * kz).amax(-1, keepdim=True)
    # flip band: one ulp of every Q and K element moves score (i, j) by dq.|k_j| + |q|.dk_j, i.e. p_j by the factor
    # eps_ij = ln2 * that; with p_j' = p_j (1 + eps_ij) / sum_i p_i (1 + eps_i):  |dctx_d| <= sum_j p_j eps_ij |v_jd| +
    # (sum_j p_j eps_ij) sum_j p_j |v_jd|;  one ulp of every V element adds sum_j p_j ulp(v_jd).
    eps = LN2 * (bf16_ulp(qh) @ kh.abs().transpose(-1, -2) + qh.abs() @ bf16_ulp(kh).transpose(-1, -2)) * kz
    Fb = (p * eps) @ vh.abs() + (p * eps).sum(-1, keepdim=True) * pv_mag + p @ bf16_ulp(vh)
    back = lambda t: t.transpose(0, 1).reshape(S, -1)
    arg = torch.where(empty[..., 0], torch.full((NH, S), -1), s.argmax(-1))
    return {"ref": back(ctx), "pv_mag": back(pv_mag), "s_mag": back(s_mag.expand(-1, -1, DH)),
            "s_abs": back(s_abs.expand(-1, -1, DH)), "F": back(Fb), "argmax": arg, "n_keys": keep.sum(-1)}


def attention_bounds(o: Dict[str, torch.Tensor]):
    """The two tiers of the attention context (bf16 output).

    T (no flips):  ulp(ref)                                  the store's rounding
                 + 2^-8 pv_mag                               P rounded to bf16 under a moving maximum (not mirrored)
                 + 2 (n_keys + 8) u pv_mag                   the fp32 sums P V and l over the query's keys
                 + 2 eps_s pv_mag                            a relative error eps_s of every p_j moves ctx by at most
                                                             2 eps_s pv_mag (numerator and normaliser), with
                   eps_s = ln2 ((32 + 8) u s_mag + 2 u s_abs) + 4 u:  the fp32 score sum of 32 terms, the subtraction of
                                                             the running maximum, v_exp_f32 and the final 1 / l.
    F (flip band): worst-case propagation of one bf16 ulp of EVERY Q, K and V element (``qkv_attention``).  The GPU and
    the fp64 reference may round an element of Q, K or V to different neighbours; elements may leave T only up to T + F,
    and only a capped share of them (the cap is measured on the CPU, see tests/encoder_kernel_cases.py)."""
    n = o["n_keys"].to(F64)[:, None]
    eps_s = LN2 * ((DH + 8) * U * o["s_mag"] + 2 * U * o["s_abs"]) + 4 * U
    T = bf16_ulp(o["ref"]) + 2.0 ** -8 * o["pv_mag"] + 2 * (n + 8) * U * o["pv_mag"] + 2 * eps_s * o["pv_mag"]
    return T, o["F"]


def _attention_tiles_f32(qh, kh, vh, keep, skip_last_rescale: bool = False) -> torch.Tensor:
    """The kernel's loop in fp32 (l. 1003-1076): key tiles of 32 taken two at a time (then one), one running maximum per
    query, accumulated O and l rescaled when it moves, P = bf16(exp2(s - m_running)), l summed unrounded.  Key tiles
    beyond the last one any query of the row sees are not visited.  ``skip_last_rescale``: the planted defect - the
    maximum still moves in the last step, but what is accumulated is not rescaled."""
    f = torch.float32
    q, k, v = qh.to(f), kh.to(f), vh.to(f)
    S = q.shape[1]
    cols = torch.nonzero(keep.any(0)).reshape(-1)
    kmax = int(cols.max()) // 32 + 1 if cols.numel() else 0
    steps, kt = [], 0
    while kt + 2 <= kmax:
        steps.append((kt, 2))
        kt += 2
    if kt < kmax:
        steps.append((kt, 1))
    m = torch.full((NH, S, 1), -1.0e30, dtype=f)
    l = torch.zeros((NH, S, 1), dtype=f)
    o = torch.zeros((NH, S, DH), dtype=f)
    for n, (kt, nt) in enumerate(steps):
        a, b = kt * 32, min((kt + nt) * 32, S)
        sc = q @ k[:, a:b].transpose(-1, -2)
        sc = torch.where(keep[None, :, a:b], sc, sc - np.float32(1.0e30))
        m_new = torch.maximum(m, sc.amax(-1, keepdim=True))
        if not (skip_last_rescale and n == len(steps) - 1 and n > 0):
            alpha = torch.exp2(m - m_new)
            l, o = l * alpha, o * alpha
        m = m_new
        e = torch.exp2(sc - m)
        l = l + e.sum(-1, keepdim=True)
        o = o + round_bf16(e).to(f) @ v[:, a:b]
    seen = keep.any(-1)[None, :, None]
    inv = torch.where((l > 0) & seen, 1.0 / l.clamp_min(1e-30), torch.zeros_like(l))
    return (o * inv).to(F64)


# ----------------------------------------------------------------------------------------------------------------------
# fused_mlp_ln_kernel<true> (row-local: any set of tokens)
# ----------------------------------------------------------------------------------------------------------------------
def fused_mlp(x, ctx, wo, bo, g1, be1, w1, b1, w2, b2, g2, be2, eps: float, acc: str = "f64", rounding: bool = True,
              defect: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """out = LN2(X1 + A W2^T + b2), A = gelu(X1 W1^T + b1), X1 = LN1(x + ctx Wo^T + bo) for tokens x, ctx [N, 384].
    Returns ref, T and F (``mlp_bounds`` explains them) and the intermediates X1, A."""
    X, C = f64(x), f64(ctx)
    one_pass = acc == "f32"
    z1 = X + _mm(C, f64(wo), acc) + f64(bo)
    y1, _, _ = layer_norm(z1, g1, be1, eps, acc, one_pass)
    X1 = _rnd(y1, rounding)
    b1v = torch.roll(f64(b1), 8) if defect == "bias_shift" else f64(b1)
    pre = _mm(X1, f64(w1), acc) + b1v
    gelu = gelu_kernel_form if rounding else gelu_exact
    A = _rnd(gelu(pre.float().to(F64) if acc == "f32" else pre), rounding)
    A2 = A
    if defect == "drop_k":
        A2 = A.clone()
        A2[:, 32:64] = 0.0
    z2 = X1 + _mm(A2, f64(w2), acc) + f64(b2)
    y2, xh2, r2 = layer_norm(z2, g2, be2, eps, acc, one_pass)
    out = {"ref": y2, "X1": X1, "A": A}
    if acc == "f32":
        return out
    W1a, W2a = f64(w1).abs(), f64(w2).abs()
    mag2 = X1.abs() + A.abs() @ W2a.T + f64(b2).abs()
    e2 = (FF + 8) * U * mag2
    out["T"] = bf16_ulp(y2) + ln_propagate(e2, xh2, r2, g2) + ln_fp32_slack(z2, xh2, r2, g2, be2)
    uX1 = bf16_ulp(X1)
    dA = GELU_SLOPE * (uX1 @ W1a.T) + bf16_ulp(A)
    out["F"] = ln_propagate(uX1 + dA @ W2a.T, xh2, r2, g2)
    return out


def mlp_bounds(o: Dict[str, torch.Tensor]):
    """T (no flips): with X1 and A as the reference has them, the kernel's z2 = X1 + A W2^T + b2 is an fp32 sum of 1536 + 2
    terms, off by at most e2 = (1536 + 8) u (|X1| + |A| |W2|^T + |b2|); that goes through LN2 (``ln_propagate``), LN2's own
    fp32 arithmetic adds ``ln_fp32_slack``, and the store rounds once: ulp(ref).
    F (flip band): the kernel's fp32 X1 and A may round to the other neighbour.  One ulp of every X1_k moves the
    pre-activation j by sum_k ulp(X1_k) |W1_jk|, A_j by at most 1.13 times that plus its own ulp, and z2_i by
    ulp(X1_i) + sum_j dA_j |W2_ij|; F is that through LN2."""
    return o["T"], o["F"]


# ----------------------------------------------------------------------------------------------------------------------
# pool_normalize_frag_kernel / pool_normalize_packed_kernel
# ----------------------------------------------------------------------------------------------------------------------
def pool(hidden, weight, normalize: bool) -> Dict[str, torch.Tensor]:
    """Mean of hidden [S, 384] over the tokens with weight 1 (clamp 1e-9), then e / max(|e|, 1e-12); fp32 output.
    Bound: the mean is an fp32 sum of n terms and a division, d = (n + 8) u sum|h| / n + 2 u |e|; the normalised vector
    moves by (d_i + |o_i| sum_j |o_j| d_j) / |e| (the Jacobian of e / |e|) plus the norm's own fp32 sum and the division,
    (384 + 8) u |o_i|."""
    h, w = f64(hidden), f64(weight).reshape(-1, 1)
    n = w.sum().clamp_min(1e-9)
    e = (h * w).sum(0) / n
    d = (float(w.sum()) + 8) * U * (h.abs() * w).sum(0) / n + 2 * U * e.abs()
    if not normalize:
        return {"ref": e, "T": d + 1e-45}
    nrm = e.norm().clamp_min(1e-12)
    o = e / nrm
    T = (d + o.abs() * (o.abs() * d).sum()) / nrm + (H + 8) * U * o.abs()
    return {"ref": o, "T": T + 1e-45}


# ----------------------------------------------------------------------------------------------------------------------
# the two-tier rule
# ----------------------------------------------------------------------------------------------------------------------
def tier_report(got, ref, T, F) -> Dict[str, object]:
    """Element-wise |got - ref| against the tight bound T and the flip band T + F.  NaN counts as beyond both."""
    g, r = f64(got), f64(ref)
    err = (g - r).abs()
    over_t = ~(err <= T)
    over_tf = ~(err <= T + F)
    ex = torch.where(over_t, torch.nan_to_num(err - T, nan=float("inf")), torch.full_like(err, -1.0))
    idx = np.unravel_index(int(torch.argmax(ex)), tuple(r.shape))
    return {"n": r.numel(), "over_T": int(over_t.sum()), "share": float(over_t.sum()) / max(r.numel(), 1),
            "over_TF": int(over_tf.sum()), "worst": idx, "got": g[idx].item(), "ref": r[idx].item(),
            "T": float(T[idx]), "F": float(F[idx])}
