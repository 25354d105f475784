"""Per-kernel fp64 parity of the inference encoder (csrc/encoder.hip): embed_ln_kernel, qkv_attention_kernel<...>,
fused_mlp_ln_kernel<true> and the two pool kernels, each on ITS OWN inputs, against oracle/encoder_ops.py.

How a kernel is isolated.  ``sskd_encoder_probe`` runs l layers and returns the hidden states and the attention context of
the last layer run.  The kernels are bit-deterministic, so the hidden states at l layers are the attention input of
layer l, the context at l + 1 layers is its output, and (hidden at l, context at l + 1) -> hidden at l + 1 is the fused MLP.
The reference is computed from the bf16 values the kernel actually read, never from a reference's own earlier stage.

Bounds (u = 2^-24, ulp = one bf16 ulp of the reference; derived in oracle/encoder_ops.py, none calibrated on the GPU):

  embed      ulp(ref) + LN-propagated 2 u sum|terms| + the LayerNorm's fp32 slack                 (no tier: nothing is
  pool       (n + 8) u sum|h| / n + 2 u |e|, through the Jacobian of e / |e|                       rounded inside)
  attention  T = ulp(ref) + 2^-8 pv_mag + 2 (n_keys + 8) u pv_mag + 2 eps_s pv_mag    (``attention_bounds``)
  fused MLP  T = ulp(ref) + LN2-propagated (1536 + 8) u mag2 + LN2's fp32 slack       (``mlp_bounds``)

Two tiers for the fused kernels.  Q, K, V, X1 and A are rounded to bf16 inside the kernel; its fp32 value and the fp64
reference can round such an element to different neighbours (a flip), which moves downstream terms by one ulp of that
intermediate.  Elements inside T pass.  An element may exceed T only up to T + F, F = the propagation of one ulp of EVERY
upstream intermediate, and only a capped share of a case's elements may do so.  The cap comes from the CPU: 4 x the share
that an ideal fp32 evaluation of the same case puts outside T (tests/encoder_kernel_cases.py CAPS, re-measured by
tests/test_encoder_oracle.py, which also shows that a dropped k-step, a skipped late rescale and a shifted bias break
this rule on these inputs).

  case (CPU: measured share -> cap)                attention: all 0 of 25 344 .. 213 888 elements, hpw12 1 of 196 992
                                                   -> caps 4 / n (1.9e-5 .. 1.6e-4);  fused MLP: all 0 -> 4 / n (6.4e-5 .. 8.1e-5)

Every test asserts the launch regime it exercises (``launch_regime`` / ``mlp_regime`` restate run_layers' rules) and
prints the observed share beside the cap (information only).  A failure names the worst element: index, got, ref, bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import encoder_kernel_cases as kc
from oracle import encoder_ops as eo

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


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


def _check_tiers(parts, name, what):
    """parts: (got, ref, T, F) per sampled row; the tier rule over the whole case."""
    got, ref, T, F = (torch.cat([p[i] for p in parts]) for i in range(4))
    rep = eo.tier_report(got, ref, T, F)
    cap = kc.cap_of(name)
    print(f"{name}: {rep['over_T']} of {rep['n']} beyond T (share {rep['share']:.3e}, cap {cap:.3e}), {rep['over_TF']} beyond T + F")
    verdict = kc.tier_verdict(rep, cap)
    if verdict:
        pytest.fail(f"{what}: {verdict}")


class Probe:
    """Device weights of one synthetic model + the probe entry point at any number of layers."""

    def __init__(self, lib, kind, layers):
        from semantic_search_kd_amd import _native
        from semantic_search_kd_amd.weights import DeviceWeights

        self.lib, self.native = lib, _native
        self.cfg, sd = kc.state_dict(kind, layers)
        self.w = DeviceWeights(self.cfg, sd, torch.device("cuda:0"))
        self.P = kc.params(kind, layers)

    def ccfg(self, layers):
        c = self.cfg
        return self.native.EncoderConfig(c.vocab_size, c.hidden_size, layers, c.num_attention_heads, c.intermediate_size,
                                         c.max_position_embeddings, c.type_vocab_size, float(c.layer_norm_eps))

    def run(self, inp, layers):
        """-> hidden, context: bf16 [B, S, 384] on the host as float64 (context: garbage for 0 layers)."""
        ids = torch.from_numpy(inp["ids"]).cuda()
        mask = torch.from_numpy(inp["mask"]).cuda()
        seg = torch.from_numpy(inp["seg"]).cuda() if inp["seg"] is not None else None
        B, S = ids.shape
        cfg = self.ccfg(layers)
        hid = torch.full((B, S, 384), float("nan"), dtype=BF, device="cuda")
        ctx = torch.full((B, S, 384), float("nan"), dtype=BF, device="cuda")
        ws = torch.empty(int(self.lib.sskd_encoder_workspace_bytes(cfg, B, S)), dtype=torch.uint8, device="cuda")
        self.native.check(self.lib.sskd_encoder_probe(
            cfg, self.w.struct, ids.data_ptr(), mask.data_ptr(), seg.data_ptr() if seg is not None else None, B, S,
            hid.data_ptr(), ctx.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
        torch.cuda.synchronize()
        return hid.cpu().double(), ctx.cpu().double()

    def _workspace(self, cfg, B, S, ws):
        """``(pointer, bytes)`` of the call's workspace: the caller's ``ws`` pair, or a fresh buffer of the reported size"""
        if ws is not None:
            return ws
        buf = torch.empty(int(self.lib.sskd_encoder_workspace_bytes(cfg, B, S)), dtype=torch.uint8, device="cuda")
        self._ws_keep = buf
        return buf.data_ptr(), buf.numel()

    def forward(self, inp, layers, normalize, ws=None):
        ids, mask = torch.from_numpy(inp["ids"]).cuda(), torch.from_numpy(inp["mask"]).cuda()
        B, S = ids.shape
        cfg = self.ccfg(layers)
        out = torch.full((B, 384), float("nan"), device="cuda")
        ws_ptr, ws_bytes = self._workspace(cfg, B, S, ws)
        self.native.check(self.lib.sskd_encoder_forward(cfg, self.w.struct, ids.data_ptr(), mask.data_ptr(), B, S,
                                                        int(normalize), out.data_ptr(), ws_ptr, ws_bytes, _st()))
        torch.cuda.synchronize()
        return out.cpu().double()

    def forward_packed(self, inp, layers, normalize, ws=None):
        ids, seg = torch.from_numpy(inp["ids"]).cuda(), torch.from_numpy(inp["seg"]).cuda()
        table = torch.from_numpy(inp["table"]).cuda()
        B, S = ids.shape
        cfg = self.ccfg(layers)
        n_seq = inp["table"].shape[0]
        out = torch.full((n_seq, 384), float("nan"), device="cuda")
        ws_ptr, ws_bytes = self._workspace(cfg, B, S, ws)
        self.native.check(self.lib.sskd_encoder_forward_packed(
            cfg, self.w.struct, ids.data_ptr(), seg.data_ptr(), B, S, table.data_ptr(), n_seq, int(normalize), out.data_ptr(),
            ws_ptr, ws_bytes, _st()))
        torch.cuda.synchronize()
        return out.cpu().double()


_PROBES = {}


@pytest.fixture
def probe(gpu, native_lib):
    def get(kind, layers):
        if (kind, layers) not in _PROBES:
            _PROBES[(kind, layers)] = Probe(native_lib, kind, layers)
        return _PROBES[(kind, layers)]
    return get


# ----------------------------------------------------------------------------------------------------------------------
# embed_ln_kernel
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.EMBED_CASES, ids=lambda c: c["name"])
def test_embed_ln_kernel(probe, case):
    """0 layers = the embedding LayerNorm alone.  Ids 0, vocab - 1 and out of range (clamped), positions 0 and 511, ids
    behind the mask (unpacked rows normalise every position t < S); packed rows: positions restart at each segment and
    padding stays exactly zero."""
    pr = probe(case["kind"], 1)
    inp = kc.make_inputs(case)
    hid, _ = pr.run(inp, 0)
    for b in case["rows"]:
        o = kc.embed_row(pr.P, inp, b)
        real = torch.from_numpy(inp["mask"][b] != 0) if inp["seg"] is not None else torch.ones(case["S"], dtype=torch.bool)
        _check(hid[b][real], o["ref"][real], o["T"][real], f"embed_ln {case['name']} row {b}")
        assert not hid[b][~real].any(), "padding of a packed row is not exactly zero"


# ----------------------------------------------------------------------------------------------------------------------
# qkv_attention_kernel
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.ATTENTION_CASES, ids=lambda c: c["name"])
def test_qkv_attention_kernel(probe, case):
    """Layer 0's attention on the GPU's own embedding output.  The case list covers hpw 1 / 4 / 12, spw 8 / 4 / 2 / 2 / 1,
    TWO_TILES and PACKED, ragged lengths 1, 2, 31, 32, 33 and S, fully masked rows (finite, nothing more), benign / stress
    weights and the two constructed rows whose maximum sits on the last / first key.  Valid queries of the sampled rows
    are compared under the tier rule; every position of every row must be finite."""
    B, S = case["B"], case["S"]
    assert kc.launch_regime(B, S, "segments" in case) == case["regime"]
    pr = probe(case["kind"], 1)
    inp = kc.make_inputs(case)
    x, _ = pr.run(inp, 0)
    _, ctx = pr.run(inp, 1)
    assert bool(torch.isfinite(ctx).all()), "non-finite context"
    for b in case.get("dead_rows", ()):
        assert not inp["mask"][b].any()
    parts = []
    for i, b in enumerate(case["rows"]):
        keep = kc.row_keep(inp, b)
        valid = torch.from_numpy(inp["mask"][b] != 0)
        o = kc.attention_row(pr.P, 0, x[b], keep)
        if "peak" in case:
            assert bool((o["argmax"][:, valid] == case["peak"][i]).all()), "the constructed maximum is not where the case says"
        T, F = eo.attention_bounds(o)
        parts.append((ctx[b][valid], o["ref"][valid], T[valid], F[valid]))
    _check_tiers(parts, f"attn/{case['name']}", f"qkv_attention {case['name']} {case['regime']}")


# ----------------------------------------------------------------------------------------------------------------------
# fused_mlp_ln_kernel<true>
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.MLP_CASES, ids=lambda c: c["name"])
def test_fused_mlp_ln_kernel(probe, case):
    """(hidden at l, context at l + 1) -> hidden at l + 1: one group per workgroup, several persistent rounds with a ragged
    last one, stress weights (LayerNorm gains in [0.3, 3], +-10 channels), layer 0 and layer 5 of 12."""
    B, S, l = case["B"], case["S"], case["layer"]
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    reg = kc.mlp_regime(B, S, n_cus)
    assert reg["groups"] == case["groups"]
    if case["name"] == "one_group_per_wg" or case["name"].startswith("deep"):
        assert reg["rounds"] == 1
    else:
        assert reg["rounds"] >= 2 and reg["ragged"] == 1, reg
    pr = probe(case["kind"], case["layers"])
    inp = kc.make_inputs(case)
    x, _ = pr.run(inp, l)
    out, ctx = pr.run(inp, l + 1)
    assert bool(torch.isfinite(out).all())
    parts = []
    for (b, t0, n) in case["tokens"]:
        o = kc.mlp_rows(pr.P, l, x[b, t0:t0 + n], ctx[b, t0:t0 + n])
        parts.append((out[b, t0:t0 + n], o["ref"], o["T"], o["F"]))
    _check_tiers(parts, f"mlp/{case['name']}", f"fused_mlp_ln {case['name']} {reg}")


# ----------------------------------------------------------------------------------------------------------------------
# pool kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [True, False])
def test_pool_normalize_frag_kernel(probe, normalize):
    """sskd_encoder_forward's tail against the fp64 pool of the very hidden states the probe returns (same kernels, same
    bits); lengths 1 .. S and an all-masked row (mean of nothing = 0, and it stays 0 when normalised)."""
    case = dict(B=6, S=100, lengths=[100, 77, 33, 32, 1, 0], seed=3)
    pr = probe("stress", 1)
    inp = kc.make_inputs(case)
    hid, _ = pr.run(inp, 1)
    got = pr.forward(inp, 1, normalize)
    for b in range(case["B"]):
        o = eo.pool(hid[b], inp["mask"][b], normalize)
        _check(got[b], o["ref"], o["T"], f"pool row {b} normalize={normalize}")
    assert not got[5].any()


@pytest.mark.parametrize("normalize", [True, False])
def test_pool_normalize_packed_kernel(probe, normalize):
    case = [c for c in kc.ATTENTION_CASES if c["name"] == "packed"][0]
    pr = probe("stress", 1)
    inp = kc.make_inputs(case)
    hid, _ = pr.run(inp, 1)
    got = pr.forward_packed(inp, 1, normalize)
    for row, lo, hi, dst in inp["table"].tolist():
        w = np.zeros(case["S"])
        w[lo:hi] = 1
        o = eo.pool(hid[row], w, normalize)
        _check(got[dst], o["ref"], o["T"], f"packed pool segment [{lo}, {hi}) of row {row} normalize={normalize}")
