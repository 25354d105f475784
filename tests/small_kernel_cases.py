"""The cases of tests/test_small_kernels_gpu.py, shared with tests/test_small_kernel_cases.py (which shows, without a GPU,
that an fp32 evaluation in each kernel's own order stays inside the bound and that every planted defect leaves it).

Kernels: kd_loss_rows_kernel + kd_loss_finish_kernel (csrc/kd_loss.hip), teacher_head_kernel (csrc/train.hip),
pool_normalize_kernel (csrc/pool.hip), similarity_kernel, l2_normalize_rows_kernel, index_add_rows_kernel and the four
row_mask kernels (csrc/index_rows.hip).  Per kernel: ``*_inputs`` (seeded), ``*_reference`` (fp64, with ``defect=`` planting one
realistic error), ``*_bound`` (elementwise) and ``*_emulate`` (fp32 numpy in the kernel's order: same lane assignment,
same butterfly and strided sums).

Bounds.  u = 2^-24 (one fp32 rounding, relative).  A sum of fp32 terms carries depth x u x sum|terms|, depth = the longest
add / fma chain an element goes through in the kernel, read off the code and stated beside each bound; sum|terms| comes
from the fp64 reference, so the bound follows cancellation.  Errors of intermediates are carried forward with the fp64
derivative of each following operation.  Nothing here was tuned on a GPU result.

Transcendentals.  No HIP math accuracy table ships with this project's toolchain documentation, so the allowances are an
ASSUMPTION, not a measurement: 8 ulp of the result for expf, logf and tanhf, 2 ulp for sqrtf and division (1 ulp = 2^-23
relative).  A result below the smallest normal fp32 gets 2^-126 absolute on top (gradual underflow or flush).
"""
from __future__ import annotations

import functools
import itertools
from typing import Dict, Optional, Tuple

import numpy as np

from oracle import kd_losses as kd

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ULP = 2.0 ** -23
EXP = LOG = TANH = 8 * ULP     # assumed, see the module docstring
SQRT = DIV = 2 * ULP           # assumed, see the module docstring
TINY = 2.0 ** -126


def _rng(*key) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(list(key)))


def bf16_round(x: np.ndarray) -> np.ndarray:
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, F32)).to(torch.bfloat16).float().numpy()


def fma32(a, b, c) -> np.ndarray:
    """Correctly rounded fp32 fma of fp32 operands.  a * b is exact in fp64; the fp64 sum is forced to round-to-odd (its
    exact error comes from TwoSum), after which the rounding to fp32 cannot be a double rounding (53 >= 24 + 2 bits)."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.broadcast_to(np.asarray(c, F32).astype(F64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = (err != 0) & np.isfinite(s) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


_LANES = np.arange(64)


def wave_sum32(v: np.ndarray) -> np.ndarray:
    """v += shfl_xor(v, o) for o = 32 .. 1 over the last axis (64 lanes), fp32: every lane ends with the same bits."""
    v = np.asarray(v, F32)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ o]
    return v


def ratio(got, ref, bound) -> float:
    """max |got - ref| / bound; a zero bound demands equality (0 / 0 counts as 0, x / 0 as inf)."""
    got, ref, bound = (np.asarray(a, F64) for a in (got, ref, bound))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# KD loss (sskd_kd_loss).  Reference: oracle/kd_losses.py in fp64.
# ----------------------------------------------------------------------------------------------------------------------
KD_SHAPES = [(1, 1), (1, 64), (3, 2), (5, 9), (1023, 9), (1024, 9), (1025, 9), (2049, 33), (4100, 64)]
KD_TEMPS = [1.0, 2.0, 4.0]
KD_TAUS = [0.05, 1.0]
KD_WEIGHTS = [(0.6, 0.2, 0.2), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
KD_REGIMES = ["cosine", "ties", "zero_mm"]
KD_LOSS_NAMES = ("loss", "margin_mse", "listwise_kd", "contrastive")


def kd_inputs(B: int, D: int, regime: str, T: float) -> Tuple[np.ndarray, np.ndarray]:
    """cosine : student in [-1, 1], teacher logits of spread 5 (the training regime)
    ties   : the row maximum shared by 2, 3 or all D lanes (cycling over the rows; at most D), at random lanes
    zero_mm: teacher = student * T with T a power of two, so t / T == s in fp32 and margin-MSE is exactly 0
    spread : both of spread 1e3 (used with tau = 1e-3)"""
    g = _rng(B, D, KD_REGIMES.index(regime) if regime in KD_REGIMES else 9)
    s = g.uniform(-1, 1, (B, D)).astype(F32)
    t = (5 * g.standard_normal((B, D))).astype(F32)
    if regime == "ties":
        for b in range(B):
            n = min((2, 3, D)[b % 3], D)
            s[b, g.permutation(D)[:n]] = F32(1.5)
    elif regime == "zero_mm":
        t = (s * F32(T)).astype(F32)
    elif regime == "spread":
        s = (1e3 * g.standard_normal((B, D))).astype(F32)
        t = (1e3 * g.standard_normal((B, D))).astype(F32)
    return s, t


def _f(x) -> float:
    return float(F32(x))


_LAST: Dict[str, tuple] = {}


def _once(fn):
    """Keep the last result per function: the weights of a case change nothing in the per-row work, and the tests walk
    the weight triples innermost."""
    @functools.wraps(fn)
    def wrapped(s, t, T, tau):
        key = (s.shape, s.tobytes(), t.tobytes(), float(T), float(tau))
        if _LAST.get(fn.__name__, (None,))[0] != key:
            _LAST[fn.__name__] = (key, fn(s, t, T, tau))
        return _LAST[fn.__name__][1]
    return wrapped


def _kd_softmax64(x, e_x, xmax, e_xmax):
    """d = x - xmax, e = expf(d), z = wave_sum(e), l = d - logf(z) with their absolute error bounds."""
    d = x - xmax
    e_d = e_x + e_xmax + U * np.abs(d)
    e = np.exp(d)
    e_e = e * (np.expm1(e_d) + EXP * np.exp(e_d)) + TINY
    z = e.sum(1, keepdims=True)
    e_z = e_e.sum(1, keepdims=True) + 6 * U * z          # butterfly of 64 lanes: depth 6
    lz = np.log(z)
    e_lz = e_z / z + LOG * np.abs(lz)
    l = d - lz
    e_l = e_d + e_lz + U * np.abs(l)
    return dict(d=d, e_d=e_d, e=e, e_e=e_e, z=z, e_z=e_z, l=l, e_l=e_l)


@_once
def _kd_rows64(s, t, T, tau):
    """The per-row quantities of kd_loss_rows_kernel in fp64, each with the bound of its fp32 error."""
    s, t = s.astype(F64), t.astype(F64)
    ts = t / T
    e_ts = np.abs(ts) * DIV
    smax, tmax = s.max(1, keepdims=True), ts.max(1, keepdims=True)
    e_tmax = np.abs(tmax) * DIV
    a0 = s - smax
    dt = ts - tmax
    e_dt = e_ts + e_tmax + U * np.abs(dt)
    r = a0 - dt
    e_r = U * np.abs(a0) + e_dt + U * np.abs(r)
    o = dict(r=r, e_r=e_r)
    o["sum_r2"] = (r * r).sum(1)                                              # square, butterfly: depth 1 + 6
    o["e_sum_r2"] = (2 * np.abs(r) * e_r + e_r * e_r + U * r * r).sum(1) + 6 * U * o["sum_r2"]
    o["sum_r"] = r.sum(1)
    o["e_sum_r"] = e_r.sum(1) + 6 * U * np.abs(r).sum(1)
    A = _kd_softmax64(s / T, np.abs(s / T) * DIV, smax / T, np.abs(smax / T) * DIV)
    Tt = _kd_softmax64(ts, e_ts, tmax, e_tmax)
    Cc = _kd_softmax64(s / tau, np.abs(s / tau) * DIV, smax / tau, np.abs(smax / tau) * DIV)
    pt = Tt["e"] / Tt["z"]
    e_pt = pt * DIV + Tt["e_e"] / Tt["z"] + pt * Tt["e_z"] / Tt["z"]
    delta = Tt["l"] - A["l"]
    e_delta = Tt["e_l"] + A["e_l"] + U * np.abs(delta)
    w = pt * delta
    e_w = e_pt * np.abs(delta) + pt * e_delta + e_pt * e_delta + U * np.abs(w)
    o["kl"] = w.sum(1)
    o["e_kl"] = e_w.sum(1) + 6 * U * np.abs(w).sum(1)
    o["nll"] = -Cc["l"][:, 0]
    o["e_nll"] = Cc["e_l"][:, 0]
    o.update(A=A, Tt=Tt, Cc=Cc, pt=pt, e_pt=e_pt)
    return o


@_once
def _kd_components(s, t, T, tau):
    return kd.margin_mse(s, t, T), kd.listwise_kd(s, t, T), kd.contrastive(s, tau)


def kd_reference(s, t, T, tau, weights, defect: Optional[str] = None):
    """-> (losses fp64 [4] = total, margin-MSE, listwise, contrastive; gradient fp64 [B, D]).  Without a defect these are
    oracle.kd_losses' three losses combined with oracle.kd_losses.combined's own expression (bit for bit what it
    returns: tests/test_small_kernel_cases.py), on the fp32 values of T, tau and the weights that the entry point receives."""
    T, tau, w = _f(T), _f(tau), tuple(_f(x) for x in weights)
    B, D = s.shape
    (mm, gmm), (lk, glk), (c, gc) = _kd_components(s, t, T, tau)
    if defect is None:
        return np.array([w[0] * mm + w[1] * lk + w[2] * c, mm, lk, c], F64), w[0] * gmm + w[1] * glk + w[2] * gc
    if defect == "last_tie":          # the maximum's gradient to the LAST maximal index
        o = _kd_rows64(s, t, T, tau)
        arg = D - 1 - s[:, ::-1].argmax(1)
        gmm = 2.0 * o["r"] / (B * D)
        gmm[np.arange(B), arg] -= 2.0 * o["sum_r"] / (B * D)
    elif defect == "T_not_T2":        # listwise scaled by T instead of T^2
        lk = lk / T
    elif defect == "mean_over_B":     # margin-MSE averaged over B instead of B * D
        mm = mm * D
    elif defect == "drop_rows_1024":  # the finish kernel's second and later strides lost
        o = _kd_rows64(s, t, T, tau)
        mm = o["sum_r2"][:1024].sum() / (B * D)
        lk = o["kl"][:1024].sum() / B * T * T
        c = o["nll"][:1024].sum() / B
    else:
        raise ValueError(defect)
    return np.array([w[0] * mm + w[1] * lk + w[2] * c, mm, lk, c], F64), w[0] * gmm + w[1] * glk + w[2] * gc


def kd_bound(s, t, T, tau, weights):
    """-> (bound of the 4 losses, bound of the gradient).
    rows kernel : every wave_sum is a 64-lane butterfly, depth 6; the terms' own errors are carried in (_kd_rows64)
    finish      : depth ceil(B / 1024) + 6 + 16 (strided chain per thread, butterfly, 16 partials in order)
    scalars     : mm = s0 / (B D) one division; lk = s1 / B * (T * T) one division + 2 roundings; c = s2 / B one division;
                  total = w . (mm, lk, c): depth 3 on sum |w_i x_i|"""
    T, tau, w = _f(T), _f(tau), tuple(_f(x) for x in weights)
    B, D = s.shape
    o = _kd_rows64(s, t, T, tau)
    depth = -(-B // 1024) + 6 + 16
    tot = {k: (o[k].sum(), o["e_" + k].sum() + depth * U * np.abs(o[k]).sum()) for k in ("sum_r2", "kl", "nll")}
    mm, lk, c = tot["sum_r2"][0] / (B * D), tot["kl"][0] / B * T * T, tot["nll"][0] / B
    e_mm = tot["sum_r2"][1] / (B * D) + DIV * abs(mm)
    e_lk = tot["kl"][1] / B * T * T + (DIV + 2 * U) * abs(lk)
    e_c = tot["nll"][1] / B + DIV * abs(c)
    e_tot = abs(w[0]) * e_mm + abs(w[1]) * e_lk + abs(w[2]) * e_c + 3 * U * (abs(w[0] * mm) + abs(w[1] * lk) + abs(w[2] * c))
    # gradient: g = g1 + g2 + g3 (two adds, possibly contracted: 2 u on sum |g_i|)
    arg = s.argmax(1)
    q = o["r"].copy()
    e_q = o["e_r"].copy()
    q[np.arange(B), arg] -= o["sum_r"]
    e_q[np.arange(B), arg] += o["e_sum_r"]
    e_q += U * np.abs(q)
    k1 = w[0] * 2.0 / (B * D)                                       # w_mm * 2 * (1 / (B D)) * q: division + 2 roundings
    g1, e_g1 = k1 * q, abs(k1) * e_q + np.abs(k1 * q) * (2 * U + DIV)
    A, Cc = o["A"], o["Cc"]
    x = np.exp(A["l"])
    e_x = x * (np.expm1(A["e_l"]) + EXP * np.exp(A["e_l"])) + TINY
    y = x - o["pt"]
    e_y = e_x + o["e_pt"] + U * np.abs(y)
    k2 = w[1] * T / B                                               # w_lk * T * (1 / B) * y: division + 3 roundings
    g2, e_g2 = k2 * y, abs(k2) * e_y + np.abs(k2 * y) * (3 * U + DIV)
    pc = Cc["e"] / Cc["z"]
    e_pc = pc * DIV + Cc["e_e"] / Cc["z"] + pc * Cc["e_z"] / Cc["z"]
    yc = pc.copy()
    yc[:, 0] -= 1.0
    e_yc = e_pc + U * np.abs(yc)
    k3 = w[2] / (B * tau)                                           # w_c * (1 / B) / tau * y: 2 divisions + 2 roundings
    g3, e_g3 = k3 * yc, abs(k3) * e_yc + np.abs(k3 * yc) * (2 * U + 2 * DIV)
    e_g = e_g1 + e_g2 + e_g3 + 2 * U * (np.abs(g1) + np.abs(g2) + np.abs(g3))
    return np.array([e_tot, e_mm, e_lk, e_c], F64), e_g


def _pad64(x, fill):
    out = np.full((x.shape[0], 64), fill, F32)
    out[:, : x.shape[1]] = x
    return out


@_once
def _kd_emulate_rows(s, t, T, tau):
    """kd_loss_rows_kernel in fp32 numpy up to the weights: lane = document, every wave_sum a butterfly."""
    T, tau = F32(T), F32(tau)
    B, D = s.shape
    valid = np.broadcast_to(_LANES < D, (B, 64))
    zero = np.zeros((B, 64), F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        sv = _pad64(s, -np.inf)
        tsv = _pad64((t / T).astype(F32), -np.inf)
        smax, tmax = sv.max(1, keepdims=True), tsv.max(1, keepdims=True)
        arg = np.where(valid & (sv == smax), _LANES, 64).min(1)
        r = np.where(valid, (sv - smax) - (tsv - tmax), zero).astype(F32)
        sum_r2, sum_r = wave_sum32(r * r), wave_sum32(r)

        def lsm(x, xmax):
            d = (x - xmax).astype(F32)
            e = np.where(valid, np.exp(d), zero).astype(F32)
            z = wave_sum32(e)
            return e, z, (d - np.log(z)).astype(F32)

        _, _, ls = lsm((sv / T).astype(F32), (smax / T).astype(F32))
        et, zt, lt = lsm(tsv, tmax)
        pt = (et / zt).astype(F32)
        kl = wave_sum32(np.where(valid, pt * (lt - ls), zero).astype(F32))
        ec, zc, lp = lsm((sv / tau).astype(F32), (smax / tau).astype(F32))
        rows = np.stack([sum_r2[:, 0], kl[:, 0], -lp[:, 0]], 1).astype(F32)
        g1 = (r - np.where(_LANES[None] == arg[:, None], sum_r, zero)).astype(F32)
        g2 = (np.exp(ls) - pt).astype(F32)
        g3 = (ec / zc - (_LANES[None] == 0).astype(F32)).astype(F32)
    # kd_loss_finish_kernel: strides of 1024, a butterfly per wave, 16 partials in order
    n_it = -(-B // 1024)
    padded = np.zeros((n_it * 1024, 3), F32)
    padded[:B] = rows
    acc = np.zeros((1024, 3), F32)
    for i in range(n_it):
        acc = acc + padded[i * 1024:(i + 1) * 1024]
    part = wave_sum32(acc.reshape(16, 64, 3).transpose(0, 2, 1))[:, :, 0]   # [wave, 3]
    tot = np.zeros(3, F32)
    for wv in range(16):
        tot = tot + part[wv]
    return tot, g1, g2, g3


def kd_emulate(s, t, T, tau, weights):
    """Both kernels in fp32 numpy -> (losses fp32 [4], gradient fp32 [B, D])."""
    tot, g1, g2, g3 = _kd_emulate_rows(s, t, T, tau)
    T, tau = F32(T), F32(tau)
    w_mm, w_lk, w_c = (F32(x) for x in weights)
    B, D = s.shape
    inv_bd, inv_b = F32(1) / (F32(B) * F32(D)), F32(1) / F32(B)
    g = w_mm * F32(2) * inv_bd * g1
    g = g + w_lk * T * inv_b * g2
    g = g + w_c * inv_b / tau * g3
    mm = tot[0] / (F32(B) * F32(D))
    lk = tot[1] / F32(B) * (T * T)
    c = tot[2] / F32(B)
    return np.array([w_mm * mm + w_lk * lk + w_c * c, mm, lk, c], F32), g.astype(F32)[:, :D]


# ----------------------------------------------------------------------------------------------------------------------
# teacher head (teacher_head_kernel): logit = out_w . tanh(dense_w . h[b, 0, :] + dense_b) + out_b
# ----------------------------------------------------------------------------------------------------------------------
HEAD_CASES = [  # (H, heads, S, B)
    dict(H=32, heads=1, S=32, B=1), dict(H=32, heads=1, S=32, B=5),
    dict(H=96, heads=3, S=32, B=1), dict(H=96, heads=3, S=32, B=5), dict(H=96, heads=3, S=64, B=5),
    dict(H=352, heads=11, S=32, B=1), dict(H=352, heads=11, S=32, B=5),
    dict(H=1024, heads=16, S=32, B=1), dict(H=1024, heads=16, S=32, B=5),
]
HEAD_VOCAB = 64


def head_name(c) -> str:
    return f"H{c['H']}_S{c['S']}_B{c['B']}"


@functools.lru_cache(maxsize=None)
def head_weights(H: int) -> Dict[str, np.ndarray]:
    """fp32 head: the rows of dense_w carry distinct scales (a row permutation changes the logit), both biases are of
    order 1 (a dropped bias is far outside the bound)."""
    g = _rng(77, H)
    scale = (0.5 + 1.5 * np.arange(H) / H)[:, None]
    return dict(dense_w=(g.standard_normal((H, H)) / np.sqrt(H) * scale).astype(F32),
                dense_b=g.uniform(0.5, 1.5, H).astype(F32) * np.where(np.arange(H) % 2, -1, 1).astype(F32),
                out_w=g.standard_normal(H).astype(F32), out_b=np.array([1.25], F32))


def head_model_inputs(c) -> Dict[str, np.ndarray]:
    """What the zero-layer generic encoder needs (embeddings + their LayerNorm) and the token ids: row b starts with its
    own token, so that the <s> states of the sequences differ."""
    H, S, B = c["H"], c["S"], c["B"]
    g = _rng(78, H, S, B)
    ids = g.integers(0, HEAD_VOCAB, (B, S)).astype(np.int32)
    ids[:, 0] = (np.arange(B) * 7 + 3) % HEAD_VOCAB
    return dict(word=g.standard_normal((HEAD_VOCAB, H)).astype(F32), pos=(0.3 * g.standard_normal((S, H))).astype(F32),
                type=(0.1 * g.standard_normal((1, H))).astype(F32), ln_g=g.uniform(0.8, 1.2, H).astype(F32),
                ln_b=(0.1 * g.standard_normal(H)).astype(F32), ids=ids, mask=np.ones((B, S), np.int32))


def head_cpu_hidden(c) -> np.ndarray:
    """bf16-valued hidden states [B, S, H] for the CPU test (the GPU test reads the encoder's own)."""
    return bf16_round(_rng(79, c["H"], c["S"], c["B"]).standard_normal((c["B"], c["S"], c["H"])).astype(F32))


def head_reference(hidden, W, defect: Optional[str] = None):
    """hidden [B, S, H] (bf16 values) -> dict(ref [B], dot_abs [B, H], pre, y)."""
    hidden = np.asarray(hidden, F64)
    B, S, H = hidden.shape
    x = hidden[:, 0, :]
    if defect == "stride_H":                      # token 0 of sequence b looked up H, not S * H, elements apart
        x = hidden.reshape(B * S, H)[:B]
    dw, db = W["dense_w"].astype(F64), W["dense_b"].astype(F64)
    ow, ob = W["out_w"].astype(F64), float(W["out_b"][0])
    if defect == "no_dense_b":
        db = np.zeros_like(db)
    pre = x @ dw.T + db
    y = np.tanh(pre)
    if defect == "rows_ge_64":                    # dense rows 64 and above never computed
        y = y.copy()
        y[:, 64:] = 0.0
    elif defect not in (None, "stride_H", "no_dense_b"):
        raise ValueError(defect)
    return dict(ref=y @ ow + ob, dot_abs=np.abs(x) @ np.abs(dw).T, pre=pre, y=y, out_abs=np.abs(y) @ np.abs(ow) + abs(ob))


def head_bound(o, W) -> np.ndarray:
    """dense dot : a lane runs ceil(H / 256) float4 steps of 4 fmas, then the butterfly: depth 4 ceil(H / 256) + 6
    + dense_b    : one rounding of the sum;  tanhf: TANH of the result, its input error through 1 - tanh^2
    out_proj     : wave 0 owns the most rows, 4 ceil(H / 64) fmas in order, then 16 partials and out_b:
                   depth 4 ceil(H / 64) + 16 + 1 on sum |out_w tanh| + |out_b|"""
    H = W["dense_w"].shape[0]
    e_pre = (4 * -(-H // 256) + 6) * U * o["dot_abs"] + U * np.abs(o["pre"])
    e_y = (1 - o["y"] ** 2) * e_pre + TANH * np.abs(o["y"])
    return e_y @ np.abs(W["out_w"].astype(F64)) + (4 * -(-H // 64) + 17) * U * o["out_abs"]


def head_emulate(hidden, W) -> np.ndarray:
    hidden = np.asarray(hidden, F32)
    B, S, H = hidden.shape
    H4, n_it = H // 4, -(-(H // 4) // 64)
    dw, db, ow, ob = W["dense_w"], W["dense_b"], W["out_w"], W["out_b"]
    out = np.zeros(B, F32)
    for b in range(B):
        x4 = np.zeros((n_it * 64, 4), F32)
        x4[:H4] = hidden[b, 0].reshape(H4, 4)
        w4 = np.zeros((H, n_it * 64, 4), F32)
        w4[:, :H4] = dw.reshape(H, H4, 4)
        d = np.zeros((H, 64), F32)
        for it in range(n_it):                     # lane c, c + 64, ...; inside a float4 the chain runs w, z, y, x
            xs, ws = x4[it * 64:(it + 1) * 64], w4[:, it * 64:(it + 1) * 64]
            for e in (3, 2, 1, 0):
                d = fma32(ws[:, :, e], xs[None, :, e], d)
        y = np.tanh((wave_sum32(d)[:, 0] + db).astype(F32)).astype(F32)
        part = np.zeros(16, F32)
        for wv in range(16):
            acc = F32(0)
            for r0 in range(4 * wv, H, 64):
                for r in range(r0, r0 + 4):
                    acc = fma32(ow[r], y[r], acc)
            part[wv] = acc
        s = F32(0)
        for wv in range(16):
            s = F32(s + part[wv])
        out[b] = F32(s + ob[0])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# sskd_pool_normalize: e = sum_t m_t h_t / max(sum_t m_t, 1e-9); optionally e / max(|e|, 1e-12)
# ----------------------------------------------------------------------------------------------------------------------
POOL_S = [1, 2, 3, 4, 5, 63, 64, 66, 257]
POOL_B = [1, 3]
POOL_MASKS = ["prefix", "scattered", "last_only", "zero", "weighted"]
POOL_H = 384


def pool_inputs(S: int, B: int, mask_kind: str, bf16: bool) -> Tuple[np.ndarray, np.ndarray]:
    g = _rng(5, S, B, POOL_MASKS.index(mask_kind))
    h = g.standard_normal((B, S, POOL_H)).astype(F32)
    if bf16:
        h = bf16_round(h)
    m = np.zeros((B, S), np.int32)
    for b in range(B):
        if mask_kind == "prefix":
            m[b, : max(1, (S * (b + 1)) // (B + 1))] = 1
        elif mask_kind == "scattered":
            m[b] = g.integers(0, 2, S)
            m[b, S // 2] = 0                       # a hole in the middle, both ends kept
            m[b, 0] = m[b, S - 1] = 1
        elif mask_kind == "last_only":
            m[b, S - 1] = 1
        elif mask_kind == "weighted":
            m[b] = g.integers(0, 4, S)
            m[b, S - 1] = 3 if b % 2 == 0 else 2
    return h, m


def pool_reference(h, m, normalize: bool, defect: Optional[str] = None):
    h, w = np.asarray(h, F64), np.asarray(m, F64)
    B, S, H = h.shape
    if defect == "clamp_mask":
        w = np.minimum(w, 1.0)
    elif defect == "drop_tail_groups":             # the tokens at and after 4 floor(S / 4) never read
        w = w.copy()
        w[:, 4 * (S // 4):] = 0.0
    elif defect not in (None, "divide_by_S"):
        raise ValueError(defect)
    num = np.einsum("bs,bsh->bh", w, h)
    num_abs = np.einsum("bs,bsh->bh", np.abs(w), np.abs(h))
    n = np.full(B, float(S)) if defect == "divide_by_S" else np.maximum(w.sum(1), 1e-9)
    e = num / n[:, None]
    o = dict(e=e, e_abs=num_abs / n[:, None])
    nrm = np.maximum(np.sqrt((e * e).sum(1)), 1e-12)
    o["nrm"] = nrm
    o["ref"] = e / nrm[:, None] if normalize else e
    return o


def pool_bound(o, S: int, normalize: bool) -> np.ndarray:
    """mean : a token group runs ceil(S / 4) multiply-adds in order (+ 1 if the product is rounded by itself), the four
              groups are added in order (3): depth ceil(S / 4) + 4 on sum |m h| / n, then one division
    norm : 4 squares and 3 adds per thread, the butterfly (6), two wave partials (1): depth 11 on ss; sqrtf; a division"""
    e, nrm = o["e"], o["nrm"][:, None]
    e_e = (-(-S // 4) + 4) * U * o["e_abs"] + DIV * np.abs(e)
    if not normalize:
        return e_e
    ss = nrm * nrm
    e_ss = (2 * np.abs(e) * e_e + e_e * e_e).sum(1, keepdims=True) + 11 * U * ss
    e_nrm = e_ss / (2 * nrm) + SQRT * nrm
    return e_e / nrm + np.abs(e) * e_nrm / (nrm * nrm) + DIV * np.abs(o["ref"])


def pool_emulate(h, m, normalize: bool) -> np.ndarray:
    h = np.asarray(h, F32)
    B, S, H = h.shape
    out = np.zeros((B, H), F32)
    for b in range(B):
        part, cnt = np.zeros((4, H), F32), np.zeros(4, F32)
        for g in range(4):
            for t in range(g, S, 4):
                if m[b, t] != 0:
                    part[g] = fma32(F32(m[b, t]), h[b, t], part[g])
                    cnt[g] = F32(cnt[g] + F32(m[b, t]))
        n = max(F32(F32(F32(cnt[0] + cnt[1]) + cnt[2]) + cnt[3]), F32(1e-9))
        e = ((((part[0] + part[1]) + part[2]) + part[3]) / n).astype(F32)
        if normalize:
            q = e.reshape(96, 4)
            ss = fma32(q[:, 3], q[:, 3], fma32(q[:, 2], q[:, 2], fma32(q[:, 1], q[:, 1], q[:, 0] * q[:, 0])))
            lanes = np.zeros(128, F32)
            lanes[:96] = ss
            red = wave_sum32(lanes.reshape(2, 64))[:, 0]
            e = (e / max(np.sqrt(F32(red[0] + red[1])), F32(1e-12))).astype(F32)
        out[b] = e
    return out


# ----------------------------------------------------------------------------------------------------------------------
# sskd_similarity: the fp32 fma chain of the 32x32x2 f32 MFMA, bit for bit oracle.scores_fma
# ----------------------------------------------------------------------------------------------------------------------
SIM_PAIRS = [(1, 1), (1, 33), (31, 32), (32, 1), (32, 32), (33, 31), (33, 65), (65, 33), (31, 65), (65, 65)]
SIM_DIMS = [8, 16, 384, 1024]


def sim_inputs(nq: int, nd: int, dim: int) -> Tuple[np.ndarray, np.ndarray]:
    """Rows nq - 1 and nd - 1, the ones the kernel clamps out-of-range lanes to, are 16 x larger and shifted: a clamped
    read that leaks into a neighbour's output cannot hide."""
    g = _rng(11, nq, nd, dim)
    q, d = g.standard_normal((nq, dim)).astype(F32), g.standard_normal((nd, dim)).astype(F32)
    q[nq - 1] = q[nq - 1] * F32(16) + F32(3)
    d[nd - 1] = d[nd - 1] * F32(16) - F32(5)
    return q, d


def sim_order(dim: int):
    """The chain's column order: per 8 columns (0, 4), (1, 5), (2, 6), (3, 7) - MFMA k = 0 is the lane half that holds
    columns 8 u + e, k = 1 the half that holds 8 u + 4 + e; k ascends inside every MFMA."""
    return [8 * u + 4 * k + e for u in range(dim // 8) for e in range(4) for k in (0, 1)]


def sim_reference(q, d, defect: Optional[str] = None) -> np.ndarray:
    """out[i, j] = the ascending-k fma chain of q[i] . d[j] in fp32; any dim % 8 == 0."""
    order = sim_order(q.shape[1])
    if defect == "swap_last_two":
        order[-1], order[-2] = order[-2], order[-1]
    elif defect is not None:
        raise ValueError(defect)
    acc = np.zeros((q.shape[0], d.shape[0]), F32)
    for c in order:
        acc = fma32(d[None, :, c], q[:, None, c], acc)
    return acc


# ----------------------------------------------------------------------------------------------------------------------
# sskd_l2_normalize_rows (any dim) and sskd_index_add_rows(normalize = 1) (dim 384)
# ----------------------------------------------------------------------------------------------------------------------
L2_DIMS = [1, 7, 63, 64, 65, 384, 1000]
L2_ROWS = [1, 4, 5, 70]
ADD_ROWS_N = [1, 31, 32, 33, 100]
KIND_RANDOM, KIND_ZERO, KIND_TINY, KIND_HUGE = 0, 1, 2, 3


def l2_inputs(n_rows: int, dim: int, specials: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """Rows 1, 2, 3 (mod 8) are zero, all 1e-30 (the sum of squares underflows to 0) and all 1e25 (it overflows); the
    others are normal draws at scales 1e-2 .. 1e2.  -> (x, kind per row)"""
    g = _rng(13, n_rows, dim)
    x = g.standard_normal((n_rows, dim)).astype(F32)
    x *= (10.0 ** ((np.arange(n_rows) % 5) - 2)).astype(F32)[:, None]
    kind = np.zeros(n_rows, np.int32)
    for i in range(n_rows):
        k = i % 8 if specials else (KIND_ZERO if i == 1 else 0)
        if k in (KIND_ZERO, KIND_TINY, KIND_HUGE):
            kind[i] = k
            x[i] = (0.0, 1e-30, 1e25)[k - 1]
    if dim == 1:
        x[kind == KIND_RANDOM] += np.sign(x[kind == KIND_RANDOM]) * F32(1e-3)   # keep a lone element away from 0
    return x, kind


def l2_reference(x, defect: Optional[str] = None) -> Dict[str, np.ndarray]:
    x = np.asarray(x, F64)
    ss = (x * x).sum(1) if defect is None else (x[:, :64] ** 2).sum(1)   # defect "ss_first_64": columns >= 64 left out
    if defect not in (None, "ss_first_64"):
        raise ValueError(defect)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.where(ss[:, None] > 0, x / np.sqrt(ss)[:, None], x)
    return dict(ref=ref)


def l2_depth(dim: int) -> int:
    """l2_normalize_rows_kernel: a lane adds ceil(dim / 64) squares in order (+ 1: the square's own rounding), butterfly 6."""
    return -(-dim // 64) + 7


ADD_ROWS_DEPTH = 8 + 6   # index_add_rows_kernel: 8 squares per lane (two float4), 7 adds among them, butterfly 6


def l2_bound(ref, depth: int) -> np.ndarray:
    """ss has only non-negative terms: relative depth u; s = 1 / sqrtf(ss): half of that + SQRT + DIV; x * s: + u."""
    return np.abs(ref) * (depth * U / 2 + SQRT + DIV + U)


def l2_emulate(x) -> np.ndarray:
    x = np.asarray(x, F32)
    n, dim = x.shape
    n_it = -(-dim // 64)
    p = np.zeros((n, n_it * 64), F32)
    p[:, :dim] = x
    ss = np.zeros((n, 64), F32)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        for it in range(n_it):
            c = p[:, it * 64:(it + 1) * 64]
            ss = fma32(c, c, ss)
        ss = wave_sum32(ss)[:, :1]
        s = (F32(1) / np.sqrt(ss)).astype(F32)
        return np.where(ss > 0, x * s, x).astype(F32)


def add_rows_emulate(x) -> np.ndarray:
    x = np.asarray(x, F32)
    n = x.shape[0]
    v = np.zeros((n, 128, 4), F32)
    v[:, :96] = x.reshape(n, 96, 4)
    sq = v * v
    a = ((sq[:, :64, 0] + sq[:, :64, 1]) + sq[:, :64, 2]) + sq[:, :64, 3]
    b = ((sq[:, 64:, 0] + sq[:, 64:, 1]) + sq[:, 64:, 2]) + sq[:, 64:, 3]
    ss = wave_sum32(a + b)[:, :1]
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(ss > 0, F32(1) / np.sqrt(ss), F32(1)).astype(F32)
    return (x * sc).astype(F32)


# ----------------------------------------------------------------------------------------------------------------------
# row masks: bit (r & 31) of word (r >> 5) = row r
# ----------------------------------------------------------------------------------------------------------------------
MASK_ROWS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 8191, 8193]


def mask_words(n_rows: int) -> int:
    return 0 if n_rows <= 0 else -(-n_rows // 32)


def mask_flags(n_rows: int) -> np.ndarray:
    return _rng(17, n_rows).choice(np.array([0, 1, 2, 255], np.uint8), size=n_rows)


def mask_pack_reference(flags) -> np.ndarray:
    bits = np.zeros(mask_words(len(flags)) * 32, np.uint8)
    bits[: len(flags)] = flags != 0
    return np.packbits(bits, bitorder="little").view(np.uint32)


def mask_ids(n_rows: int) -> np.ndarray:
    """Duplicates, the ids 0 and n - 1, and three out-of-range ids (-1, n, n + 5)."""
    g = _rng(19, n_rows)
    inside = g.integers(0, n_rows, 40)
    ids = np.concatenate([inside, inside[:7], [0, n_rows - 1, -1, n_rows, n_rows + 5, 0]]).astype(np.int64)
    return g.permutation(ids)


def mask_update_reference(words, n_rows: int, ids, allow: bool) -> Tuple[np.ndarray, int]:
    out = np.array(words, np.uint32)
    bad = 0
    for r in ids.tolist():
        if r < 0 or r >= n_rows:
            bad += 1
        elif allow:
            out[r >> 5] |= np.uint32(1 << (r & 31))
        else:
            out[r >> 5] &= np.uint32(~(1 << (r & 31)) & 0xFFFFFFFF)
    return out, bad


def mask_dirty_tail(n_rows: int) -> np.ndarray:
    """Random words whose last one has EVERY bit at or past n_rows set."""
    w = _rng(23, n_rows).integers(0, 2 ** 32, mask_words(n_rows), dtype=np.uint64).astype(np.uint32)
    if n_rows & 31:
        w[-1] |= np.uint32((0xFFFFFFFF << (n_rows & 31)) & 0xFFFFFFFF)
    return w


def mask_count_reference(words, n_rows: int, defect: Optional[str] = None) -> int:
    bits = np.unpackbits(np.asarray(words, np.uint32).view(np.uint8), bitorder="little")
    if defect == "tail_unmasked":
        return int(bits[: mask_words(n_rows) * 32].sum())
    if defect is not None:
        raise ValueError(defect)
    return int(bits[:n_rows].sum())


def kd_combos():
    """(regime, T, tau, weights) of the dense grid + the spread regime at tau = 1e-3."""
    out = list(itertools.product(KD_REGIMES, KD_TEMPS, KD_TAUS, KD_WEIGHTS))
    out += [("spread", T, 1e-3, w) for T in (1.0, 4.0) for w in KD_WEIGHTS]
    return out
