"""The student's training step as a CHAIN of the fp64 kernel references - TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

``step`` composes the per-kernel references of oracle/generic_ops.py in the order csrc/train.hip launches the kernels
(``forward_all`` / ``layer_forward``, ``backward_rows`` / ``layer_backward``) and rounds to bf16 (``round_bf16``) wherever
the step keeps a bf16 buffer:

  * forward: z0, x0; per layer qkv, (unfused: the scores and P), ctx, the output projection (tH0), z1, x1, u, hmid, the
    second FFN product (tH0), z2, x2;
  * backward: the pooled entry's tH2; per layer dz2, dhmid, du, dx1, dz1, dctx, (unfused: dP, dS), dqkv, tH1; dz0;
  * the by-design points of generic_ops.py: P before P V (relative to the running maximum of the online softmax), P and dS
    before the fused backward's products, and the three bias gradients that are column sums of a STORED bf16 gradient
    (db2 and dbo out of ``ln_bwd``, db1 out of ``gelu_bwd_colsum``).

mean / rstd of every LayerNorm and the pooled vector are kept in fp32, as the step keeps them.  Everything between two
rounding points is fp64, so the chain differs from the kernels by their fp32 arithmetic (summation order, atomics order,
exp2f / erff / rsqrtf) and by the bf16 roundings that those differences flip - and from exact arithmetic by every rounding.
It holds no formula of its own: a formula belongs in generic_ops.py, pinned to autograd by tests/test_generic_oracle.py.

``defect=`` restates one plausible wiring bug of train.hip each (tests/train_step_cases.py plants them to show that the
gate sees them); ``products=`` replaces the plain products (to stand in for another summation order).
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import generic_ops as go

F64 = go.F64
rb = go.round_bf16

# defect -> (what it restates, the shapes it applies to as a predicate of (layers, pos_offset))
DEFECTS = {
    "residual_dropped": ("dx2b (the residual share of the layer above) not added at layer 0", lambda L, off: L >= 2),
    "db2_from_dx2": ("db2 summed from the incoming gradient dx2 (+ dx2b) instead of dz2", lambda L, off: L >= 1),
    "store_not_add": ("one bias gradient overwrites the buffer's start value", lambda L, off: True),
    "short_sequence_lost": ("the shortest sequence left out of every LayerNorm gamma / beta gradient", lambda L, off: True),
    "one_row_stale": ("the last row of layer 0's dW1 is the one of the layer processed before it", lambda L, off: L >= 2),
    "pos_offset_ignored": ("position gradients land at row t instead of t + pos_offset", lambda L, off: off != 0),
    "tile_20pct": ("rows 0-31 of layer 0's dWo are 1.2 x", lambda L, off: L >= 1),
    "scale_x2": ("every gradient is 2 x", lambda L, off: True),
}


def defect_applies(defect: str, layers: int, pos_offset: int) -> bool:
    return DEFECTS[defect][1](layers, pos_offset)


def store_not_add_target(layers: int) -> str:
    """the bias whose gradient the ``store_not_add`` defect stores"""
    return f"encoder.layer.{layers - 1}.intermediate.dense.bias" if layers else "embeddings.LayerNorm.bias"


def _f32(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float32).to(F64)


def _plain_nt(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return go.gemm_nt(a, b)[0]


def step(sd: Dict[str, np.ndarray], ids, mask, *, heads: int, eps: float = 1e-12, pos_offset: int = 0,
         normalize: bool = True, dout=None, dhidden=None, defect: Optional[str] = None,
         start: Optional[Dict[str, torch.Tensor]] = None,
         products: Optional[Callable[[torch.Tensor, torch.Tensor], torch.Tensor]] = None,
         mirror_attention_registers: bool = True) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """One forward and backward of the student.

    ``sd``: HF-named state dict; the matrices and embedding tables are read as bf16 (rounded here, which changes nothing
    when they already are bf16 values), vectors as fp32.  ``ids`` / ``mask`` int [B, S], S a multiple of 32.
    Exactly one of ``dout`` ([B, H], the pooled entry: masked mean pool, L2-normalised with ``normalize``) and ``dhidden``
    ([B, S, H] bf16 values, the token entry) is given.
    Returns (embeddings [B, H] or hidden states [B, S, H], {HF name: fp64 gradient}) - the gradient the step ADDS to the
    caller's buffer.  ``start`` (the buffers' contents before the step) is read by the ``store_not_add`` defect alone.
    ``products(a [.., M, K], b [.., N, K]) -> a b^T`` replaces the plain products (fp64 by default).
    ``mirror_attention_registers=False`` leaves out the register roundings of the fused attention kernels (P relative to
    the final maximum, no rounding of P / dS in the backward): for measuring what they are worth."""
    if (dout is None) == (dhidden is None):
        raise ValueError("give exactly one of dout and dhidden")
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    nt = products or _plain_nt

    def tn(a, b):   # A[T, M]^T B[T, N]: the same product with the token dimension as K
        return nt(a.T.contiguous(), b.T.contiguous())

    def mat(name):
        return rb(go.f64(torch.as_tensor(np.asarray(sd[name]))))

    def vec(name):
        return go.f64(torch.as_tensor(np.asarray(sd[name], np.float32)))

    ids_t = torch.as_tensor(np.asarray(ids)).to(torch.int32)
    mask_t = torch.as_tensor(np.asarray(mask)).to(torch.int32)
    B, S = ids_t.shape
    word, pos, typ = mat("embeddings.word_embeddings.weight"), mat("embeddings.position_embeddings.weight"), mat(
        "embeddings.token_type_embeddings.weight")
    vocab, H = word.shape
    L = 0
    while f"encoder.layer.{L}.output.dense.weight" in sd:
        L += 1
    if defect is not None and not defect_applies(defect, L, pos_offset):
        raise ValueError(f"defect {defect!r} does not apply to {L} layers, pos_offset {pos_offset}")
    DH = H // heads
    scale = 1.0 / float(np.sqrt(DH))
    fused = DH in (32, 64) and 32 <= S <= 256 and S % 32 == 0 and S * DH <= 8192   # attention_bwd_supported (generic.hip)
    lengths = mask_t.sum(1)
    kept_rows = None
    if defect == "short_sequence_lost":
        b_short = int(torch.argmin(lengths))
        kept_rows = torch.ones(B, S, dtype=torch.bool)
        kept_rows[b_short] = False
        kept_rows = kept_rows.reshape(-1)

    def ln_bwd(dy, z, mean, rstd, gamma, dy2):
        dz, dgamma, dbeta, dzc, *_ = go.ln_bwd(dy, z, mean, rstd, gamma, dy2)
        dsum = dbeta
        if kept_rows is not None:
            k = kept_rows
            _, dgamma, dbeta, *_ = go.ln_bwd(dy[k], z[k], mean[k], rstd[k], gamma, None if dy2 is None else dy2[k])
        return rb(dz), dgamma, dbeta, dzc, dsum

    # ------------------------------------------------------------------ forward (forward_all / layer_forward)
    z0 = go.embed_fwd(ids_t, word, pos, typ[0], S, pos_offset)
    emb_g, emb_b = vec("embeddings.LayerNorm.weight"), vec("embeddings.LayerNorm.bias")
    y, z0, mean0, rstd0, _ = go.add_ln_fwd(z0, None, emb_g, emb_b, eps, round_z=True)
    x0, mean0, rstd0 = rb(y), _f32(mean0), _f32(rstd0)
    saved = []
    x = x0
    for l in range(L):
        p = f"encoder.layer.{l}."
        w = {"wqkv": torch.cat([mat(p + f"attention.self.{n}.weight") for n in ("query", "key", "value")]),
             "bqkv": torch.cat([vec(p + f"attention.self.{n}.bias") for n in ("query", "key", "value")]),
             "wo": mat(p + "attention.output.dense.weight"), "bo": vec(p + "attention.output.dense.bias"),
             "ln1_g": vec(p + "attention.output.LayerNorm.weight"), "ln1_b": vec(p + "attention.output.LayerNorm.bias"),
             "w1": mat(p + "intermediate.dense.weight"), "b1": vec(p + "intermediate.dense.bias"),
             "w2": mat(p + "output.dense.weight"), "b2": vec(p + "output.dense.bias"),
             "ln2_g": vec(p + "output.LayerNorm.weight"), "ln2_b": vec(p + "output.LayerNorm.bias")}
        s = {"x_in": x, "w": w}
        s["qkv"] = qkv = rb(nt(x, w["wqkv"]) + w["bqkv"])
        if fused:
            ctx, lse, _ = go.attention_fwd(qkv, mask_t, B, S, heads, DH, scale,
                                           round_p="running" if mirror_attention_registers else True)
            s["lse"] = _f32(lse)
        else:   # attention_unfused_fwd: scores (bf16, unscaled) -> softmax in place (bf16) -> P V
            q, k, v = go._split_heads(qkv, B, S, heads, DH)
            s["P"] = P = rb(go.softmax_fwd(rb(nt(q, k)), mask_t, B, heads, S, scale)).view(B, heads, S, S)
            ctx = go._merge_heads(nt(P, v.transpose(-1, -2)))
        s["ctx"] = ctx = rb(ctx)
        attn_out = rb(nt(ctx, w["wo"]) + w["bo"])
        y, s["z1"], mean1, rstd1, _ = go.add_ln_fwd(x, attn_out, w["ln1_g"], w["ln1_b"], eps, round_z=True)
        s["x1"], s["mean1"], s["rstd1"] = rb(y), _f32(mean1), _f32(rstd1)
        x1 = s["x1"]
        s["u"] = u = rb(nt(x1, w["w1"]) + w["b1"])
        s["hmid"] = hmid = rb(go.gelu(u))
        ffn_out = rb(nt(hmid, w["w2"]) + w["b2"])
        y, s["z2"], mean2, rstd2, _ = go.add_ln_fwd(x1, ffn_out, w["ln2_g"], w["ln2_b"], eps, round_z=True)
        s["x2"], s["mean2"], s["rstd2"] = rb(y), _f32(mean2), _f32(rstd2)
        saved.append(s)
        x = s["x2"]
    hidden = x.view(B, S, H)

    # ------------------------------------------------------------------ backward (backward_rows / layer_backward)
    g: Dict[str, torch.Tensor] = {}
    if dhidden is None:
        out, pooled, _ = go.pool_fwd(hidden, mask_t, normalize)
        dh, _ = go.pool_bwd(go.f64(torch.as_tensor(np.asarray(dout))), _f32(pooled), mask_t, normalize)
        dx = rb(dh).reshape(B * S, H)                                  # tH2
    else:
        out = hidden
        dx = rb(go.f64(torch.as_tensor(np.asarray(dhidden)))).reshape(B * S, H)
    dxb = None
    for l in range(L - 1, -1, -1):
        p, s = f"encoder.layer.{l}.", saved[l]
        w = s["w"]
        if defect == "residual_dropped" and l == 0:
            dxb = None
        dz2, g[p + "output.LayerNorm.weight"], g[p + "output.LayerNorm.bias"], db2, dsum2 = ln_bwd(
            dx, s["z2"], s["mean2"], s["rstd2"], w["ln2_g"], dxb)
        g[p + "output.dense.bias"] = dsum2 if defect == "db2_from_dx2" else db2
        g[p + "output.dense.weight"] = tn(dz2, s["hmid"])
        dhmid = rb(nt(dz2, w["w2"].T.contiguous()))
        du, g[p + "intermediate.dense.bias"], _ = go.gelu_bwd_colsum(s["u"], dhmid)
        du = rb(du)
        g[p + "intermediate.dense.weight"] = tn(du, s["x1"])
        dx1 = rb(nt(du, w["w1"].T.contiguous()))
        dz1, g[p + "attention.output.LayerNorm.weight"], g[p + "attention.output.LayerNorm.bias"], dbo, _ = ln_bwd(
            dx1, s["z1"], s["mean1"], s["rstd1"], w["ln1_g"], dz2)
        g[p + "attention.output.dense.bias"] = dbo
        g[p + "attention.output.dense.weight"] = tn(dz1, s["ctx"])
        dctx = rb(nt(dz1, w["wo"].T.contiguous()))
        if fused:
            dqkv, _, _ = go.attention_bwd(s["qkv"], mask_t, s["ctx"], dctx, B, S, heads, DH, scale, lse=s["lse"],
                                          round_ps=mirror_attention_registers)
        else:   # attention_unfused_bwd
            q, k, v = go._split_heads(s["qkv"], B, S, heads, DH)
            do = go.f64(dctx).view(B, S, heads, DH).permute(0, 2, 1, 3)
            P = s["P"]
            dP = rb(nt(do, v))
            dv = nt(P.transpose(-1, -2), do.transpose(-1, -2))
            dS = rb(go.softmax_bwd(dP.reshape(-1, S), P.reshape(-1, S), scale)[0]).view(B, heads, S, S)
            dq = nt(dS, k.transpose(-1, -2))
            dk = nt(dS.transpose(-1, -2), q.transpose(-1, -2))
            dqkv = torch.cat([go._merge_heads(t) for t in (dq, dk, dv)], 1)
        dqkv = rb(dqkv)
        dwqkv, dbqkv = tn(dqkv, s["x_in"]), go.colsum(dqkv)[0]
        for i, n in enumerate(("query", "key", "value")):
            g[p + f"attention.self.{n}.weight"] = dwqkv[i * H:(i + 1) * H]
            g[p + f"attention.self.{n}.bias"] = dbqkv[i * H:(i + 1) * H]
        dx = rb(nt(dqkv, w["wqkv"].T.contiguous()))                    # tH1; the layer's input gradient is tH1 + dz1
        dxb = dz1
    dz0, g["embeddings.LayerNorm.weight"], g["embeddings.LayerNorm.bias"], _, _ = ln_bwd(dx, z0, mean0, rstd0, emb_g, dxb)
    dword, dpos, dtype0, *_ = go.embed_bwd(ids_t, mask_t, dz0, vocab, pos.shape[0], S,
                                           0 if defect == "pos_offset_ignored" else pos_offset)
    g["embeddings.word_embeddings.weight"], g["embeddings.position_embeddings.weight"] = dword, dpos
    g["embeddings.token_type_embeddings.weight"] = torch.zeros_like(typ)
    g["embeddings.token_type_embeddings.weight"][0] = dtype0

    # ------------------------------------------------------------------ defects that edit finished gradients
    if defect == "one_row_stale":
        g["encoder.layer.0.intermediate.dense.weight"] = g["encoder.layer.0.intermediate.dense.weight"].clone()
        g["encoder.layer.0.intermediate.dense.weight"][-1] = g["encoder.layer.1.intermediate.dense.weight"][-1]
    elif defect == "tile_20pct":
        g["encoder.layer.0.attention.output.dense.weight"] = g["encoder.layer.0.attention.output.dense.weight"].clone()
        g["encoder.layer.0.attention.output.dense.weight"][:32] *= 1.2
    elif defect == "scale_x2":
        g = {k: 2.0 * v for k, v in g.items()}
    elif defect == "store_not_add":
        if start is None:
            raise ValueError("store_not_add needs start=, the buffers' contents before the step")
        name = store_not_add_target(L)
        g[name] = g[name] - go.f64(start[name])     # buffer = gradient, so what was "added" is gradient - start
    return out, g
