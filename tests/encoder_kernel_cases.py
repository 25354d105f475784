"""The cases of tests/test_encoder_kernels_gpu.py, shared with tests/test_encoder_oracle.py (which measures, without a GPU,
what fp32 accumulation alone does to each case's fp64 reference and checks that the planted defects are caught).

A case = weights (benign / stress / constructed), a batch of token ids with a mask or packed segments, the layer whose
kernel is looked at, and the batch rows whose reference is computed (rows do not interact; sampling keeps the CPU work
bounded).  Shapes are chosen from the launch rules of ``run_layers`` (csrc/encoder.hip), restated in ``launch_regime``.

Caps.  ``CAPS[name] = (measured share, cap)``: ``measured`` is the share of a case's outputs that an ideal fp32 evaluation
(``oracle.encoder_ops`` with ``acc="f32"``) puts outside the tight bound T of the fp64 reference, on this case's inputs,
on the CPU.  cap = 4 x max(measured, 1 / n): the GPU's summation order differs from torch's, and a count of zero among n
elements bounds the share by 1 / n, not by zero.  No cap exceeds 2 %, and no measured share 0.5 %.
tests/test_encoder_oracle.py re-measures every share and asserts it is under a quarter of its cap.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import encoder_ops as eo
from oracle.generic_ops import F64
from semantic_search_kd_amd.weights import BertConfig, bf16_round, synthetic_state_dict

VOCAB = 30522


def launch_regime(B: int, S: int, packed: bool = False) -> Dict[str, object]:
    """The attention launch of run_layers (csrc/encoder.hip: spw l. 1366, hpw l. 1373, kernel l. 1382-1383)."""
    nkt = (S + 31) // 32
    spw = 8 // nkt if nkt <= 4 else 1
    rows = (B + spw - 1) // spw
    hpw = 12 if rows >= 256 else (4 if rows >= 64 else 1)
    return {"nkt": nkt, "spw": spw, "hpw": hpw, "two_tiles": nkt > 8, "packed": packed and nkt <= 8}


def mlp_regime(B: int, S: int, n_cus: int) -> Dict[str, int]:
    """Groups of 128 tokens and the persistent rounds of fused_mlp_ln_kernel (l. 1405-1406)."""
    t_pad = -(-(B * (-(-S // 32) * 32)) // 256) * 256
    groups = t_pad // 128
    return {"groups": groups, "rounds": -(-groups // n_cus), "ragged": int(groups > n_cus and groups % n_cus != 0)}


# ----------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------
CONSTRUCTED_PEAK_ID = 5000


@functools.lru_cache(maxsize=None)
def state_dict(kind: str, layers: int):
    cfg = BertConfig(num_hidden_layers=layers)
    if kind == "constructed":
        return cfg, _constructed_state_dict(cfg)
    return cfg, synthetic_state_dict(cfg, stress=(kind == "stress"))


def _constructed_state_dict(cfg: BertConfig):
    """Weights that put every query's row maximum on ONE known key.  Word embeddings are unit normal noise with a quiet
    channel 0 (x 0.5) that only the peak token raises (to 5); positions and type contribute nothing and the embedding
    LayerNorm is the identity map, so x_j[0] is about 4.8 for the peak token and within +-2 for every other one.  Wk gets
    a column of ones on channel 0 (every key dimension carries x_j[0] besides the benign noise) and the query bias is 0.5
    in every dimension, so score (i, j) = x_j[0] * sum_d q_id + noise with sum_d q_id = log2e/sqrt(32) (16 +- 2.2) > 0: the
    peak key beats every other key of every head and query by about 10 log2 units.  Where the peak token stands in the
    row decides whether the online-softmax rescale fires in the last key tile or never after the first.  The tests
    assert the position of the maximum from the reference's scores."""
    sd = dict(synthetic_state_dict(cfg))
    g = np.random.Generator(np.random.PCG64(4242))
    word = g.standard_normal((cfg.vocab_size, 384)).astype(np.float32)
    word[:, 0] *= 0.5
    word[CONSTRUCTED_PEAK_ID, 0] = 5.0
    sd["embeddings.word_embeddings.weight"] = word
    sd["embeddings.position_embeddings.weight"] = np.zeros_like(sd["embeddings.position_embeddings.weight"])
    sd["embeddings.token_type_embeddings.weight"] = np.zeros_like(sd["embeddings.token_type_embeddings.weight"])
    sd["embeddings.LayerNorm.weight"] = np.ones(384, np.float32)
    sd["embeddings.LayerNorm.bias"] = np.zeros(384, np.float32)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layer.{i}.attention.self."
        wk = sd[p + "key.weight"].copy()
        wk[:, 0] = 1.0
        sd[p + "key.weight"] = wk
        sd[p + "query.bias"] = np.full(384, 0.5, np.float32)
    return sd


def _t(a, matrix: bool) -> torch.Tensor:
    a = np.asarray(a, np.float32)
    return torch.from_numpy(bf16_round(a) if matrix else a).to(F64)


@functools.lru_cache(maxsize=None)
def params(kind: str, layers: int):
    """The kernel's view of the weights as float64 tensors: matrices and embeddings rounded to bf16, the rest fp32."""
    cfg, sd = state_dict(kind, layers)
    out = {"word": _t(sd["embeddings.word_embeddings.weight"], True),
           "pos": _t(sd["embeddings.position_embeddings.weight"], True),
           "type0": _t(sd["embeddings.token_type_embeddings.weight"], True)[0],
           "emb_g": _t(sd["embeddings.LayerNorm.weight"], False), "emb_b": _t(sd["embeddings.LayerNorm.bias"], False),
           "eps": float(cfg.layer_norm_eps), "layers": []}
    for i in range(layers):
        p = f"encoder.layer.{i}."
        L = {}
        for k, nm in (("q", "attention.self.query"), ("k", "attention.self.key"), ("v", "attention.self.value"),
                      ("o", "attention.output.dense"), ("1", "intermediate.dense"), ("2", "output.dense")):
            L["w" + k], L["b" + k] = _t(sd[p + nm + ".weight"], True), _t(sd[p + nm + ".bias"], False)
        for k, nm in (("1", "attention.output.LayerNorm"), ("2", "output.LayerNorm")):
            L["g" + k], L["be" + k] = _t(sd[p + nm + ".weight"], False), _t(sd[p + nm + ".bias"], False)
        out["layers"].append(L)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def _segments_to_words(S: int, segs) -> np.ndarray:
    w = np.zeros(S, np.int32)
    for lo, hi in segs:
        w[lo:hi] = lo | (hi << 16)
    return w


def make_inputs(case) -> Dict[str, np.ndarray]:
    """ids [B, S], mask [B, S] (1 = token; for packed rows: inside a segment), seg [B, S] or None, table [n_seq, 4]."""
    B, S = case["B"], case["S"]
    g = np.random.Generator(np.random.PCG64(case.get("seed", 1)))
    ids = g.integers(999, VOCAB, size=(B, S), dtype=np.int64).astype(np.int32)
    mask = np.ones((B, S), np.int32)
    seg = None
    table: List[List[int]] = []
    if "segments" in case:
        seg = np.zeros((B, S), np.int32)
        for b, segs in enumerate(case["segments"]):
            seg[b] = _segments_to_words(S, segs)
            table += [[b, lo, hi, len(table) + i] for i, (lo, hi) in enumerate(segs)]
        mask = (seg != 0).astype(np.int32)
    else:
        lengths = case.get("lengths")
        if lengths is None:
            lengths = g.integers(2, S + 1, size=B).tolist()
        lengths = list(lengths) + [S] * (B - len(lengths))
        for b, n in enumerate(lengths):
            mask[b, n:] = 0
    ids[mask == 0] = 0                               # [PAD] behind the mask
    for (b, t, v) in case.get("set_ids", ()):        # edge ids / the constructed peak token / non-zero ids behind the mask
        ids[b, t] = v
    return {"ids": ids, "mask": mask, "seg": seg, "table": np.asarray(table, np.int32).reshape(-1, 4)}


def row_positions(inp, b: int) -> np.ndarray:
    S = inp["ids"].shape[1]
    if inp["seg"] is None:
        return np.arange(S)
    lo = inp["seg"][b] & 0xFFFF
    return np.where(inp["seg"][b] != 0, np.arange(S) - lo, 0)


def row_keep(inp, b: int) -> torch.Tensor:
    return eo.keep_from_mask(inp["mask"][b]) if inp["seg"] is None else eo.keep_from_segments(inp["seg"][b])


def attention_row(P, l: int, x, keep, **kw):
    L = P["layers"][l]
    return eo.qkv_attention(x, L["wq"], L["wk"], L["wv"], L["bq"], L["bk"], L["bv"], keep, **kw)


def mlp_rows(P, l: int, x, ctx, **kw):
    L = P["layers"][l]
    return eo.fused_mlp(x, ctx, L["wo"], L["bo"], L["g1"], L["be1"], L["w1"], L["b1"], L["w2"], L["b2"], L["g2"], L["be2"],
                        P["eps"], **kw)


def embed_row(P, inp, b: int, **kw):
    return eo.embed_ln(inp["ids"][b], row_positions(inp, b), P["word"], P["pos"], P["type0"], P["emb_g"], P["emb_b"],
                       P["eps"], **kw)


def cpu_layer_input(P, inp, b: int, layer: int, rounding: bool = True):
    """Row b's input of layer ``layer`` from the mirrored fp64 chain (what the GPU test reads from the probe instead):
    every activation that a kernel stores for the next one is rounded to bf16, as in HBM."""
    x = eo.round_bf16(embed_row(P, inp, b)["ref"]) if rounding else embed_row(P, inp, b)["ref"]
    keep = row_keep(inp, b)
    for l in range(layer):
        c = attention_row(P, l, x, keep, rounding=rounding)["ref"]
        c = eo.round_bf16(c) if rounding else c
        x = mlp_rows(P, l, x, c, rounding=rounding)["ref"]
        x = eo.round_bf16(x) if rounding else x
    return x


def cpu_layer_output(P, inp, b: int, layer: int, rounding: bool = True):
    """The reference of layer ``layer``'s fused-MLP output on the mirrored chain's inputs: what ``fused_mlp`` returns, i.e.
    the value BEFORE the kernel's store rounds it (the store's rounding is the ulp(ref) term of the bounds, not a rounding
    point of the reference)."""
    x, keep = cpu_layer_input(P, inp, b, layer, rounding), row_keep(inp, b)
    c = attention_row(P, layer, x, keep, rounding=rounding)["ref"]
    return mlp_rows(P, layer, x, eo.round_bf16(c) if rounding else c, rounding=rounding)["ref"]


# ----------------------------------------------------------------------------------------------------------------------
# the cases.  ``rows``: batch rows whose reference is computed (first / last of a workgroup and of the batch included)
# ----------------------------------------------------------------------------------------------------------------------
def _lengths(B, S, seed, special):
    g = np.random.Generator(np.random.PCG64(seed))
    out = g.integers(2, S + 1, size=B).tolist()
    for b, n in special.items():
        out[b] = n
    return out


ATTENTION_CASES = [
    # name, weights, shape, mask, rows -> expected regime (asserted by the GPU test)
    dict(name="nkt1_spw8", kind="benign", B=5, S=32, lengths=[32, 31, 2, 1, 0], rows=[0, 1, 2, 3],
         regime=dict(nkt=1, spw=8, hpw=1, two_tiles=False, packed=False), dead_rows=[4]),
    dict(name="nkt2_spw4", kind="stress", B=6, S=64, lengths=[64, 33, 32, 31, 2, 1], rows=[0, 1, 2, 3, 4, 5],
         regime=dict(nkt=2, spw=4, hpw=1, two_tiles=False, packed=False)),
    dict(name="nkt3_spw2", kind="benign", B=5, S=96, lengths=[96, 65, 33, 1, 0], rows=[0, 1, 2, 3],
         regime=dict(nkt=3, spw=2, hpw=1, two_tiles=False, packed=False), dead_rows=[4]),
    dict(name="nkt4_spw2_hpw4", kind="stress", B=131, S=128, lengths=_lengths(131, 128, 7, {0: 128, 1: 33, 129: 31, 130: 128}),
         rows=[0, 1, 64, 65, 129, 130], regime=dict(nkt=4, spw=2, hpw=4, two_tiles=False, packed=False)),
    dict(name="nkt5_spw1_hpw4", kind="benign", B=64, S=160, lengths=_lengths(64, 160, 8, {0: 160, 63: 129}),
         rows=[0, 31, 63], regime=dict(nkt=5, spw=1, hpw=4, two_tiles=False, packed=False)),
    dict(name="nkt7_spw1", kind="stress", B=3, S=200, lengths=[200, 129, 33], rows=[0, 1, 2],
         regime=dict(nkt=7, spw=1, hpw=1, two_tiles=False, packed=False)),
    dict(name="hpw12", kind="stress", B=256, S=256, lengths=_lengths(256, 256, 9, {0: 256, 255: 225, 100: 32}),
         rows=[0, 100, 255], regime=dict(nkt=8, spw=1, hpw=12, two_tiles=False, packed=False)),
    dict(name="two_tiles_nkt10", kind="benign", B=2, S=300, lengths=[300, 257], rows=[0, 1],
         regime=dict(nkt=10, spw=1, hpw=1, two_tiles=True, packed=False)),
    dict(name="two_tiles_nkt16", kind="stress", B=2, S=512, lengths=[512, 2], rows=[0, 1],
         regime=dict(nkt=16, spw=1, hpw=1, two_tiles=True, packed=False)),
    # packed rows: a one-token segment, segments that start and end inside a key tile, a row filled to capacity, a tail
    dict(name="packed", kind="stress", B=2, S=256,
         segments=[[(0, 1), (1, 40), (40, 100), (100, 256)], [(0, 33), (33, 64), (64, 200)]], rows=[0, 1],
         regime=dict(nkt=8, spw=1, hpw=1, two_tiles=False, packed=True)),
    # the row maximum of every query on the LAST key (the rescale fires in the last tile) / on the FIRST (never again)
    dict(name="max_late", kind="constructed", B=2, S=256, lengths=[256, 200], rows=[0, 1],
         set_ids=[(0, 255, CONSTRUCTED_PEAK_ID), (1, 199, CONSTRUCTED_PEAK_ID)], peak=[255, 199],
         regime=dict(nkt=8, spw=1, hpw=1, two_tiles=False, packed=False)),
    dict(name="max_early", kind="constructed", B=2, S=256, lengths=[256, 200], rows=[0, 1],
         set_ids=[(0, 0, CONSTRUCTED_PEAK_ID), (1, 0, CONSTRUCTED_PEAK_ID)], peak=[0, 0],
         regime=dict(nkt=8, spw=1, hpw=1, two_tiles=False, packed=False)),
]

MLP_CASES = [
    # tokens: (row, first position, count) slices whose reference is computed
    dict(name="one_group_per_wg", kind="benign", layers=1, layer=0, B=4, S=96, lengths=[96, 65, 33, 2],
         tokens=[(0, 0, 96), (1, 0, 65), (3, 0, 2)], groups=4),
    dict(name="persistent_ragged_stress", kind="stress", layers=1, layer=0, B=328, S=256,
         lengths=_lengths(328, 256, 31, {0: 256, 327: 256}), tokens=[(0, 0, 32), (127, 100, 32), (128, 0, 32), (327, 224, 32)],
         groups=656),
    dict(name="deep_layer5_stress", kind="stress", layers=12, layer=5, B=4, S=96, lengths=[96, 65, 33, 2],
         tokens=[(0, 0, 96), (1, 0, 65)], groups=4),
]

EMBED_CASES = [
    dict(name="edges", kind="stress", B=3, S=512, lengths=[512, 300, 1],
         set_ids=[(0, 0, 0), (0, 1, VOCAB - 1), (0, 511, VOCAB - 1), (0, 2, VOCAB + 7), (0, 3, -5),
                  (1, 400, 777), (2, 1, 12345)], rows=[0, 1, 2]),
    dict(name="packed", kind="benign", B=2, S=256,
         segments=[[(0, 1), (1, 40), (40, 100), (100, 256)], [(0, 33), (33, 64), (64, 200)]], rows=[0, 1]),
]

# name -> (share measured on the CPU, elements compared, cap); see the module docstring.  The numbers are the report of
# tests/test_encoder_oracle.py::test_flip_shares_stay_under_a_quarter_of_the_caps (python -m pytest -s prints it).
CAPS: Dict[str, tuple] = {
    # case                          (measured share, elements, cap = 4 max(share, 1 / elements))
    "attn/nkt1_spw8": (0.000e+00, 25344, 1.578e-04),
    "attn/nkt2_spw4": (0.000e+00, 62592, 6.391e-05),
    "attn/nkt3_spw2": (0.000e+00, 74880, 5.342e-05),
    "attn/nkt4_spw2_hpw4": (0.000e+00, 173184, 2.310e-05),
    "attn/nkt5_spw1_hpw4": (0.000e+00, 137472, 2.910e-05),
    "attn/nkt7_spw1": (0.000e+00, 139008, 2.878e-05),
    "attn/hpw12": (5.076e-06, 196992, 2.031e-05),
    "attn/two_tiles_nkt10": (0.000e+00, 213888, 1.870e-05),
    "attn/two_tiles_nkt16": (0.000e+00, 197376, 2.027e-05),
    "attn/packed": (0.000e+00, 175104, 2.284e-05),
    "attn/max_late": (0.000e+00, 175104, 2.284e-05),
    "attn/max_early": (0.000e+00, 175104, 2.284e-05),
    "mlp/one_group_per_wg": (0.000e+00, 62592, 6.391e-05),
    "mlp/persistent_ragged_stress": (0.000e+00, 49152, 8.138e-05),
    "mlp/deep_layer5_stress": (0.000e+00, 61824, 6.470e-05),
}


def cap_of(name: str) -> float:
    return CAPS[name][2]


# ----------------------------------------------------------------------------------------------------------------------
# CPU side: the fp32 evaluation (optionally with a planted defect) against the fp64 reference, under the tier rule
# ----------------------------------------------------------------------------------------------------------------------
def tier_verdict(rep, cap: float) -> Optional[str]:
    """None when the tier rule holds, else what broke it."""
    if rep["over_TF"]:
        return (f"{rep['over_TF']} of {rep['n']} elements beyond T + F; worst at {rep['worst']}: got {rep['got']!r}, "
                f"ref {rep['ref']!r}, T {rep['T']:.3e}, F {rep['F']:.3e}")
    if rep["share"] > cap:
        return (f"{rep['over_T']} of {rep['n']} elements ({rep['share']:.4%}) beyond T, cap {cap:.4%}; worst at "
                f"{rep['worst']}: got {rep['got']!r}, ref {rep['ref']!r}, T {rep['T']:.3e}, F {rep['F']:.3e}")
    return None


def attention_cpu(case, defect: Optional[str] = None):
    """Tier report of the fp32 evaluation of an attention case (valid queries of the sampled rows) on the CPU."""
    P, inp = params(case["kind"], 1), make_inputs(case)
    got, ref, T, F = [], [], [], []
    for b in case["rows"]:
        x, keep = cpu_layer_input(P, inp, b, 0), row_keep(inp, b)
        valid = torch.from_numpy(inp["mask"][b] != 0)
        o = attention_row(P, 0, x, keep)
        t, f = eo.attention_bounds(o)
        g = eo.round_bf16(attention_row(P, 0, x, keep, acc="f32", defect=defect)["ref"])
        got.append(g[valid]); ref.append(o["ref"][valid]); T.append(t[valid]); F.append(f[valid])
    return eo.tier_report(torch.cat(got), torch.cat(ref), torch.cat(T), torch.cat(F))


def mlp_cpu(case, defect: Optional[str] = None):
    P, inp = params(case["kind"], case["layers"]), make_inputs(case)
    l = case["layer"]
    got, ref, T, F = [], [], [], []
    for (b, t0, n) in case["tokens"]:
        x, keep = cpu_layer_input(P, inp, b, l), row_keep(inp, b)
        c = eo.round_bf16(attention_row(P, l, x, keep)["ref"])
        x, c = x[t0:t0 + n], c[t0:t0 + n]
        o = mlp_rows(P, l, x, c)
        g = eo.round_bf16(mlp_rows(P, l, x, c, acc="f32", defect=defect)["ref"])
        got.append(g); ref.append(o["ref"]); T.append(o["T"]); F.append(o["F"])
    return eo.tier_report(torch.cat(got), torch.cat(ref), torch.cat(T), torch.cat(F))
