"""Shapes, references and the gate of the composed student step (csrc/train.hip), shared by tests/test_train_step_host.py (CPU:
the gate against simulated gradients and planted defects) and tests/test_train_step_gpu.py (the kernels through
``TrainableEncoder``).

Two references on the SAME bf16-valued matrices (the weight matrices and embedding tables of the state dict are rounded to
bf16 once; biases and LayerNorm parameters stay fp32):

  E  exact: fp64 ``torch.autograd`` over ``oracle.encoder`` (no rounding anywhere);
  R  faithful: ``oracle.generic_step.step``, the fp64 kernel references chained in train.hip's order with a bf16 rounding at
     every point where the step keeps bf16.

R - E is what the step's bf16 storage costs; a computed gradient G differs from R only by fp32 arithmetic (summation and
atomics order, exp2f / erff / rsqrtf) and by the roundings those flip.  The gate, per parameter tensor:

  slices   matrices: every row and every column; embedding tables: every row; vectors: every aligned block of 32
  noise    noise_slice = RMS_slice(R - E), noise_tensor = RMS_tensor(R - E): from the references alone
  gate     RMS_slice(G - R) <= C * max(noise_slice, noise_tensor) for every slice, nothing added or subtracted.  C = 1 would
           say: the computed gradient lies at least as near to the faithful chain as exact arithmetic does.  C = 2 is in
           force and is the ceiling: beyond it the gate would admit more than bf16 rounding itself.  Why not 1: measured on
           an MI355X the worst slices of the two 2-layer shapes are above 1 (1.31 and 1.04; DESIGN.md 3.8 has the figures; the
           one-layer shapes stay below 0.65), and a mere reordering of the fp32 sums on the CPU does the same (tests/test_train_step_host.py: a flipped
           rounding is one whole ulp, and flips cascade through two layers).  No rounding point is missing from R - at one
           layer G equals R to fp32 accuracy in most cases - and no bug was found.
  fp32     Where R = E to within one fp32 rounding of what the buffer holds (max(noise_slice, noise_tensor) <
           2^-24 RMS_slice(|R| + |start|)) the noise rule is void: no fp32 buffer can meet it.  That is the case for exactly
           one tensor, the top LayerNorm's beta gradient of the token entry - a plain sum of dhidden that no rounding touches,
           so R = E bit for bit.  Those slices are held to fp32 arithmetic instead: RMS_slice(G - R) <=
           2^-24 RMS_slice((T + 264) |R| + 4 |start|), an fp32 sum of up to T = B S terms whose partial sums meet through
           atomics (the term of the per-kernel tests) plus a few roundings of the start value.  No other slice sees this term.
  scale    | ||G|| / ||R|| - 1 | < 3 % per tensor
  zeros    where R is zero by structure (vocabulary rows no unmasked token names, position rows outside
           [pos_offset, pos_offset + S), type rows >= 1) the buffer keeps its start value bit for bit
  key bias mathematically zero (a key bias shifts every score of a query alike): max |G| < 2e-2 of the step's largest
           gradient magnitude, the rule of tests/test_training_gpu.py

G is always "buffer after the step minus buffer before it": the buffers start from ``start_values`` (non-zero multiples of
2^-10 in [-1, 1]), so a gradient that is stored instead of added shows up as an error of the start value's size.

The token entry's ``dhidden`` is zero at padded positions: the step gives padding exactly zero embedding gradient
(embed_bwd skips masked tokens), exact arithmetic would not, and MaxSim - the entry's caller - never sends any.
"""
from __future__ import annotations

import functools
import zlib
from typing import Dict, List, NamedTuple, Tuple

import numpy as np
import torch

from oracle import encoder as enc_oracle
from oracle import generic_step
from semantic_search_kd_amd import BertConfig, synthetic_state_dict
from semantic_search_kd_amd.weights import bf16_round

F64 = torch.float64
C = 2.0            # the gate's constant: see the module docstring; never above 2
VOCAB = 600
MODES = ("pooled_norm", "pooled_raw", "tokens")

# name -> (hidden, heads, intermediate, layers, pos_offset, S, lengths, what it reaches)
CASES = {
    "student_tn": (384, 12, 1536, 2, 0, 64, (64, 33, 32, 1),
                   "T = 256: all four dW on the TN kernel; fused attention backward, head width 32"),
    "student_odd_T": (384, 12, 1536, 1, 0, 32, (32, 17, 2),
                      "T = 96, not a multiple of 64: transpose + NT route at H 384, one K slice"),
    "generic_splitk": (128, 2, 256, 2, 0, 128, (128, 97, 64, 31, 3),
                       "T = 640: transpose + NT with two atomic K slices; S x DH = 8192, the fused backward's limit"),
    "unfused_96": (192, 2, 192, 1, 0, 64, (64, 40), "materialised-score attention at head width 96"),
    "no_layers": (64, 2, 128, 0, 0, 32, (32, 19, 5), "backward_rows with the embedding LayerNorm as first consumer"),
    "xlmr_offset": (128, 4, 256, 1, 2, 32, (32, 9), "shifted position rows, last table row in use, rows 0-1 untouched"),
}


def config(case: str) -> BertConfig:
    H, heads, F, L, off, S, _, _ = CASES[case]
    return BertConfig(vocab_size=VOCAB, hidden_size=H, num_hidden_layers=L, num_attention_heads=heads,
                      intermediate_size=F, max_position_embeddings=S + off)


def pos_offset(case: str) -> int:
    return CASES[case][4]


@functools.lru_cache(maxsize=None)
def inputs(case: str):
    """(state dict with bf16-valued matrices, ids, mask, dout fp32 [B, H], dhidden bf16-valued fp32 [B, S, H])."""
    H, _, _, _, _, S, lengths, _ = CASES[case]
    cfg = config(case)
    sd = {k: (bf16_round(v) if v.ndim == 2 else v) for k, v in synthetic_state_dict(cfg, recipe="spread").items()}
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(case.encode())))
    B = len(lengths)
    ids = rng.integers(1, VOCAB, size=(B, S)).astype(np.int32)
    mask = (np.arange(S)[None, :] < np.asarray(lengths)[:, None]).astype(np.int32)
    ids[0, 0], ids[0, 1], ids[-1, 0] = VOCAB - 1, 1, 1      # the table's last row; one id in two sequences
    ids[mask == 0] = 0                                      # [PAD]: named by masked tokens only
    dout = rng.standard_normal((B, H)).astype(np.float32)
    dhidden = bf16_round(rng.standard_normal((B, S, H)).astype(np.float32)) * mask[..., None].astype(np.float32)
    return sd, ids, mask, dout, dhidden


def exact(case: str, mode: str) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """E: (output, gradients) by fp64 autograd over oracle/encoder.py."""
    sd, ids, mask, dout, dhidden = inputs(case)
    _, heads, _, L, off, _, _, _ = CASES[case]
    eps = config(case).layer_norm_eps
    t = {k: torch.from_numpy(v).to(F64).requires_grad_(True) for k, v in sd.items()}
    if mode == "tokens":
        out = enc_oracle.bert_hidden_states_torch(t, ids, mask, L, heads, eps, F64, pos_offset=off)[-1]
        (out * torch.from_numpy(dhidden).to(F64)).sum().backward()
    else:
        out = enc_oracle.embeddings_torch(t, ids, mask, L, heads, eps, normalize=mode == "pooled_norm", pos_offset=off)
        (out * torch.from_numpy(dout).to(F64)).sum().backward()
    return out.detach(), {k: v.grad for k, v in t.items()}


def faithful(case: str, mode: str, **kw) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """R (or, with ``defect=`` / ``products=``, a variation of it): (output, gradients) of oracle/generic_step.py."""
    sd, ids, mask, dout, dhidden = inputs(case)
    _, heads, _, _, off, _, _, _ = CASES[case]
    entry = {"dhidden": dhidden} if mode == "tokens" else {"dout": dout, "normalize": mode == "pooled_norm"}
    return generic_step.step(sd, ids, mask, heads=heads, eps=config(case).layer_norm_eps, pos_offset=off, **entry, **kw)


@functools.lru_cache(maxsize=None)
def references(case: str, mode: str):
    """(E output, E gradients, R output, R gradients), computed once per process and never modified."""
    return exact(case, mode) + faithful(case, mode)


def start_values(name: str, shape) -> torch.Tensor:
    """What a gradient buffer holds before the step: k 2^-10 with k uniform in [-1024, 1024] without 0, fp32."""
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(name.encode())))
    k = rng.integers(1, 1025, size=tuple(shape)) * rng.choice(np.array([-1, 1]), size=tuple(shape))
    return torch.from_numpy((k * 2.0 ** -10).astype(np.float32))


def start_dict(case: str) -> Dict[str, torch.Tensor]:
    return {k: start_values(k, v.shape) for k, v in inputs(case)[0].items()}


def permuted_fp32_products(seed: int):
    """a b^T accumulated in fp32 with the reduction dimension in a random order: stands in for the order in which a GPU
    kernel (MFMA K steps, split-K slices, atomics) adds the same terms."""
    gen = torch.Generator().manual_seed(seed)

    def nt(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        perm = torch.randperm(a.shape[-1], generator=gen)
        return (a[..., perm].float() @ b[..., perm].float().transpose(-1, -2)).to(F64)

    return nt


# ---------------------------------------------------------------------------------------------------------------------
# the gate
# ---------------------------------------------------------------------------------------------------------------------
def _rms(x: torch.Tensor, dim=None) -> torch.Tensor:
    return torch.sqrt((x * x).mean() if dim is None else (x * x).mean(dim))


def slice_rms(name: str, x: torch.Tensor) -> Dict[str, torch.Tensor]:
    """RMS over every slice of a tensor, by kind of slice."""
    if x.ndim == 1:
        return {"block32": _rms(x.view(-1, 32), 1)}
    if name.startswith("embeddings."):
        return {"row": _rms(x, 1)}
    return {"row": _rms(x, 1), "col": _rms(x, 0)}


def structural_zero_rows(case: str) -> Dict[str, torch.Tensor]:
    """embedding-table rows whose gradient is zero by structure, as boolean row masks"""
    _, ids, mask, _, _ = inputs(case)
    cfg, off, S = config(case), pos_offset(case), CASES[case][5]
    word = torch.ones(cfg.vocab_size, dtype=torch.bool)
    word[torch.from_numpy(ids[mask != 0]).long().clamp(0, cfg.vocab_size - 1)] = False
    pos = torch.ones(cfg.max_position_embeddings, dtype=torch.bool)
    pos[off:off + S] = False
    typ = torch.ones(cfg.type_vocab_size, dtype=torch.bool)
    typ[0] = False
    return {"embeddings.word_embeddings.weight": word, "embeddings.position_embeddings.weight": pos,
            "embeddings.token_type_embeddings.weight": typ}


class GateResult(NamedTuple):
    bad: List[str]              # violations; empty passes
    worst: Dict[str, float]     # per tensor, the worst RMS_slice(G - R) / max(noise_slice, noise_tensor), nothing subtracted
    over: int                   # slices above c
    slices: int                 # slices gated by the noise rule
    fp32_slices: int            # slices whose noise an fp32 buffer cannot resolve, gated by the fp32 bound instead


def gate(case: str, mode: str, after: Dict[str, torch.Tensor], start: Dict[str, torch.Tensor], c: float = C) -> GateResult:
    """Hold gradient buffers that held ``start`` before the step and hold ``after`` now against R and E of (case, mode)."""
    _, E, _, R = references(case, mode)
    return gate_against(case, E, R, after, start, c)


def gate_against(case: str, E: Dict[str, torch.Tensor], R: Dict[str, torch.Tensor], after: Dict[str, torch.Tensor],
                 start: Dict[str, torch.Tensor], c: float = C) -> GateResult:
    """``gate`` with the two references handed in"""
    bad: List[str] = []
    worst: Dict[str, float] = {}
    over = slices = fp32_slices = 0
    top = max(float(v.abs().max()) for v in R.values())
    zero_rows = structural_zero_rows(case)
    T, u = inputs(case)[1].size, 2.0 ** -24
    for name, r in R.items():
        a, s = after[name].detach().cpu(), start[name].detach().cpu()
        G = a.to(F64) - s.to(F64)
        if name in zero_rows:
            z = zero_rows[name]
            assert not bool(r[z].any()), name   # the chain agrees that these rows are zero
            if not torch.equal(a[z].float().view(torch.int32), s[z].float().view(torch.int32)):
                bad.append(f"{name}: {int((a[z] != s[z]).any(1).sum())} structurally zero rows changed")
        if "key.bias" in name:
            if not float(G.abs().max()) < 2e-2 * top:
                bad.append(f"{name}: max |G| {float(G.abs().max()):.3e} >= 2e-2 x {top:.3e}")
            continue
        noise_tensor = _rms(r - E[name])
        err, noise = slice_rms(name, G - r), slice_rms(name, r - E[name])
        held = slice_rms(name, u * (r.abs() + s.to(F64).abs()))     # one fp32 rounding of what the buffer holds
        fp32 = slice_rms(name, u * ((T + 264) * r.abs() + 4 * s.to(F64).abs()))
        worst[name] = 0.0
        for kind in err:
            bound = torch.maximum(noise[kind], noise_tensor)
            by_fp32 = bound < held[kind]            # R = E to within the buffer's own resolution: the noise rule is void
            fp32_slices += int(by_fp32.sum())
            if bool((by_fp32 & ~(err[kind] <= fp32[kind])).any()):
                i = int(torch.where(by_fp32, err[kind] / fp32[kind], torch.zeros_like(bound)).argmax())
                bad.append(f"{name} {kind} {i}: RMS(G - R) {float(err[kind][i]):.3e} > fp32 bound {float(fp32[kind][i]):.3e}")
            ratio = torch.where(by_fp32, torch.zeros_like(bound), err[kind] / bound)
            ratio = torch.where(torch.isnan(err[kind]), torch.full_like(ratio, float("inf")), ratio)   # NaN in G fails
            slices += int((~by_fp32).sum())
            over += int((ratio > c).sum())
            worst[name] = max(worst[name], float(ratio.max()))
            if float(ratio.max()) > c:
                i = int(ratio.argmax())
                bad.append(f"{name} {kind} {i}: RMS(G - R) {float(err[kind][i]):.3e} = {float(ratio[i]):.2f} x noise "
                           f"{float(bound[i]):.3e} ({int((ratio > c).sum())} such slices)")
        scale = float(G.norm() / r.norm())
        if not abs(scale - 1.0) < 0.03:
            bad.append(f"{name}: ||G|| / ||R|| = {scale:.4f}")
    return GateResult(bad, worst, over, slices, fp32_slices)


def old_gate(G: Dict[str, torch.Tensor], E: Dict[str, torch.Tensor], norms: bool) -> List[str]:
    """The per-tensor gate of tests/test_training_gpu.py: cosine >= 0.999 (and, in the encoder test only, norms within
    3 %); key biases by magnitude.  ``norms=False`` is the rule of the two KD-step tests before this change."""
    bad = []
    top = max(float(v.abs().max()) for v in E.values())
    for name, e in E.items():
        g = G[name].to(F64)
        if float(e.abs().max()) < 1e-6 * top:
            if not float(g.abs().max()) < 2e-2 * top:
                bad.append(name + ": not zero")
            continue
        cos = float((g * e).sum() / (g.norm() * e.norm() + 1e-300))
        if not cos >= 0.999:
            bad.append(f"{name}: cosine {cos:.5f}")
        elif norms and not abs(float(g.norm() / e.norm()) - 1.0) < 0.03:
            bad.append(f"{name}: norm ratio {float(g.norm() / e.norm()):.4f}")
    return bad


def table(worst: Dict[str, float]) -> str:
    """worst ratio per tensor, one line per layer"""
    lines: Dict[str, List[str]] = {}
    for name, v in worst.items():
        head, short = ("emb", name[len("embeddings."):]) if name.startswith("embeddings.") else (
            "L" + name.split(".")[2], ".".join(name.split(".")[3:]))
        short = short.replace("attention.output.", "attn_out.").replace("attention.", "").replace(".weight", ".w").replace(".bias", ".b").replace("LayerNorm", "LN")
        lines.setdefault(head, []).append(f"{short} {v:.2f}")
    return "\n".join(f"    {k}: " + ", ".join(v) for k, v in lines.items())
