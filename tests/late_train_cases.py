"""Training through MaxSim: the NumPy restatements of the gradient kernels, their fp64 references, the gather formulation
that torch autograd differentiates, and the case generators (no GPU).

* ``dq_rows`` / ``dd_rows`` restate ``sskd_latet_maxsim_bwd_q`` / ``_bwd_d`` bit for bit: per column ``acc = +0.0``, then
  ``acc = acc + g * x`` over the contributions ascending (c for dQ, e = (q R + c) stride + i for dD), the product and the
  sum rounded to fp32 one after the other (NumPy forms no fma).
* ``pack_bwd_rows`` restates ``sskd_latet_pack_tokens_bwd``: ``ss`` and ``n`` by ``late_cases.sum_squares_rows``, the dot in
  the pack's lane-chain-then-butterfly order, ``(g - y * dot) / n`` rounded to bf16.
* ``dq64`` / ``dd64`` / ``pack_bwd64`` are the same sums in fp64.
* ``gather_scores_torch`` is ``sum_i <q_i, d_arg(i)>`` on torch tensors: MaxSim with the argmax held fixed.

Token matrices travel as uint16 bf16 bit patterns, as in ``late_cases``."""
import numpy as np

from late_cases import DIM, bf16_bits, bf16_values, sum_squares_rows, unit_token_bits


def lims_of(lengths) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


def tq_stride(q_lims) -> int:
    return int(-(-int(np.diff(q_lims).max()) // 32) * 32)


# ------------------------------------------------------------------ contributions
def contributions(q_lims, d_lims, cand, arg):
    """Every contribution the kernels honour, ascending in e: ``(e, q, c, i, query token row, document token row)``.  A
    pair contributes for query token i when ``arg >= 0`` and it still names a document holding that token."""
    nq, R = cand.shape
    stride = arg.shape[2]
    nd = d_lims.size - 1
    out = []
    for q in range(nq):
        tq = int(q_lims[q + 1] - q_lims[q])
        for c in range(R):
            j = int(cand[q, c])
            if j < 0 or j >= nd:
                continue
            td = int(d_lims[j + 1] - d_lims[j])
            for i in range(min(tq, stride)):
                t = int(arg[q, c, i])
                if 0 <= t < td:
                    out.append(((q * R + c) * stride + i, q, c, i, int(q_lims[q]) + i, int(d_lims[j]) + t))
    return out


def dq_rows(d_bits, d_lims, q_lims, cand, arg, g) -> np.ndarray:
    """``sskd_latet_maxsim_bwd_q`` restated: fp32 ``[sum Tq, 384]``."""
    d = bf16_values(d_bits).reshape(-1, DIM)
    g = np.asarray(g, np.float32)
    out = np.zeros((int(q_lims[-1]), DIM), np.float32)
    with np.errstate(all="ignore"):
        for _, q, c, _, qrow, drow in contributions(q_lims, d_lims, cand, arg):   # per query token: c ascending
            out[qrow] = out[qrow] + g[q, c] * d[drow]
    return out


def dd_rows(q_bits, q_lims, d_lims, cand, arg, g) -> np.ndarray:
    """``sskd_latet_maxsim_bwd_d`` restated: fp32 ``[sum Td, 384]``; a row nobody selected stays +0.0."""
    x = bf16_values(q_bits).reshape(-1, DIM)
    g = np.asarray(g, np.float32)
    out = np.zeros((int(d_lims[-1]), DIM), np.float32)
    with np.errstate(all="ignore"):
        for _, q, c, _, qrow, drow in contributions(q_lims, d_lims, cand, arg):   # per document token: e ascending
            out[drow] = out[drow] + g[q, c] * x[qrow]
    return out


def dq64(d_bits, d_lims, q_lims, cand, arg, g):
    """fp64 ``dQ`` and, per element, ``sum |g| |x|`` and the number of terms (for the derived bound)."""
    d = bf16_values(d_bits).reshape(-1, DIM).astype(np.float64)
    out = np.zeros((int(q_lims[-1]), DIM))
    mag = np.zeros_like(out)
    n = np.zeros(int(q_lims[-1]), np.int64)
    for _, q, c, _, qrow, drow in contributions(q_lims, d_lims, cand, arg):
        out[qrow] += float(g[q, c]) * d[drow]
        mag[qrow] += abs(float(g[q, c])) * np.abs(d[drow])
        n[qrow] += 1
    return out, mag, n


def dd64(q_bits, q_lims, d_lims, cand, arg, g):
    x = bf16_values(q_bits).reshape(-1, DIM).astype(np.float64)
    out = np.zeros((int(d_lims[-1]), DIM))
    mag = np.zeros_like(out)
    n = np.zeros(int(d_lims[-1]), np.int64)
    for _, q, c, _, qrow, drow in contributions(q_lims, d_lims, cand, arg):
        out[drow] += float(g[q, c]) * x[qrow]
        mag[drow] += abs(float(g[q, c])) * np.abs(x[qrow])
        n[drow] += 1
    return out, mag, n


def sum_bound(mag: np.ndarray, n: np.ndarray) -> np.ndarray:
    """``1.01 (n + 1) 2^-24 sum |g| |x|`` per element.  Derivation: a term ``g x`` is one rounding (relative 2^-24) and
    takes part in at most n of the n additions that follow (the first, to +0.0, is exact; counted anyway), each a
    relative 2^-24 of a partial sum that is at most ``sum |g| |x| (1 + 2^-24)^n``: in all ``((1 + 2^-24)^(n + 1) - 1)
    sum |g| |x| <= 1.01 (n + 1) 2^-24 sum |g| |x|`` for every n the kernels can meet ((n + 1) 2^-24 << 0.01)."""
    return 1.01 * (n[:, None] + 1) * 2.0 ** -24 * mag


# ------------------------------------------------------------------ pack backward
def pack_bwd_rows(hidden_bits: np.ndarray, lengths, dtok: np.ndarray) -> np.ndarray:
    """``sskd_latet_pack_tokens_bwd`` restated: hidden bf16 bits ``[B, S, 384]``, ``lengths [B]``, ``dtok`` fp32
    ``[T, 384]`` in CSR order -> bf16 bits ``[B, S, 384]`` (zeros at positions >= the length)."""
    B, S = hidden_bits.shape[:2]
    lims = lims_of(lengths)
    out = np.zeros((B, S, DIM), np.uint16)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for b in range(B):
            L = int(lengths[b])
            if L == 0:
                continue
            x = bf16_values(hidden_bits[b, :L]).reshape(L, DIM)
            g = np.ascontiguousarray(dtok[lims[b]: lims[b + 1]], np.float32)
            n = np.maximum(np.sqrt(sum_squares_rows(x)), np.float32(1e-12)).astype(np.float32)[:, None]
            y = (x / n).astype(np.float32)
            p = np.zeros((L, 64), np.float32)
            gl, yl = g.reshape(L, DIM // 8, 8), y.reshape(L, DIM // 8, 8)
            for j in range(8):
                t = gl[:, :, j] * yl[:, :, j]
                p[:, : DIM // 8] = p[:, : DIM // 8] + t
            for o in (32, 16, 8, 4, 2, 1):
                p = p + p[:, idx ^ o]
            dot = p[:, :1]
            t = (y * dot).astype(np.float32)
            out[b, :L] = bf16_bits(((g - t).astype(np.float32) / n).astype(np.float32))
    return out


def pack_bwd64(hidden_bits: np.ndarray, lengths, dtok: np.ndarray):
    """fp64 ``(dh [B, S, 384], bound [B, S, 384])`` of the normalisation's backward at the pack's own fp32 ``n`` (the
    test is about the backward's arithmetic; ``n`` is pinned bit for bit by the forward's tests).

    Bound ``2^-8 |ref| + 1.01 (384 + 4) 2^-24 ||g||_2 / n``.  First term: the result is rounded to bf16 (8 significant
    bits, half an ulp = 2^-9 relative; 2^-8 also holds the few fp32 roundings of g - y dot and of the division).  Second:
    the fp32 dot of 384 products with |y_c| <= 1 errs by at most (384 + 2) 2^-24 sum |g_c y_c| (one rounding per product,
    at most 6 + 8 < 384 additions on any column's path through the lane chain and the butterfly; + 2 for the rounding of
    y itself and of y dot) <= (384 + 4) 2^-24 ||g||_2 ||y||_2 with ||y||_2 <= 1; the dot enters dh as y_c dot / n with
    |y_c| <= 1, hence the 1 / n."""
    B, S = hidden_bits.shape[:2]
    lims = lims_of(lengths)
    ref = np.zeros((B, S, DIM))
    bound = np.zeros((B, S, DIM))
    for b in range(B):
        L = int(lengths[b])
        if L == 0:
            continue
        x32 = bf16_values(hidden_bits[b, :L]).reshape(L, DIM)
        n = np.maximum(np.sqrt(sum_squares_rows(x32)), np.float32(1e-12)).astype(np.float64)[:, None]
        x = x32.astype(np.float64)
        g = np.asarray(dtok[lims[b]: lims[b + 1]], np.float64)
        y = x / n
        dot = (g * y).sum(axis=1, keepdims=True)
        ref[b, :L] = (g - y * dot) / n
        bound[b, :L] = 2.0 ** -8 * np.abs(ref[b, :L]) + 1.01 * (DIM + 4) * 2.0 ** -24 * np.sqrt((g * g).sum(axis=1, keepdims=True)) / n
    return ref, bound


# ------------------------------------------------------------------ the gather formulation (torch, differentiable)
def gather_scores_torch(q_tok, q_lims, d_tok, d_lims, cand, arg):
    """``score[q, c] = sum_i <q_i, d_arg[q, c, i]>`` on torch tensors ``[sum Tq, 384]`` / ``[sum Td, 384]`` (any dtype,
    may require grad); absent pairs (no contribution at all) score 0 here - the caller masks them."""
    import torch

    nq, R = cand.shape
    rows = contributions(q_lims, d_lims, cand, arg)
    out = torch.zeros(nq * R, dtype=q_tok.dtype)
    if rows:
        pair = torch.tensor([q * R + c for _, q, c, _, _, _ in rows])
        qi = torch.tensor([r[4] for r in rows])
        di = torch.tensor([r[5] for r in rows])
        out = out.index_add(0, pair, (q_tok[qi] * d_tok[di]).sum(dim=1))
    return out.view(nq, R)


def argmax64(q_bits, q_lims, d_bits, d_lims, cand, stride: int):
    """fp64 on the stored bf16 values: ``(arg [nq, R, stride] - the smallest index of the maximum, -1 where absent or
    padded -, best [nq, R, stride], second [nq, R, stride] (-inf for a one-token document))``."""
    q = bf16_values(q_bits).reshape(-1, DIM).astype(np.float64)
    d = bf16_values(d_bits).reshape(-1, DIM).astype(np.float64)
    nq, R = cand.shape
    nd = d_lims.size - 1
    arg = np.full((nq, R, stride), -1, np.int32)
    best = np.full((nq, R, stride), -np.inf)
    second = np.full((nq, R, stride), -np.inf)
    for qq in range(nq):
        qt = q[q_lims[qq]: q_lims[qq + 1]]
        for c in range(R):
            j = int(cand[qq, c])
            if j < 0 or j >= nd or d_lims[j + 1] == d_lims[j]:
                continue
            dots = qt @ d[d_lims[j]: d_lims[j + 1]].T
            a = dots.argmax(axis=1)
            arg[qq, c, : qt.shape[0]] = a
            best[qq, c, : qt.shape[0]] = dots.max(axis=1)
            if dots.shape[1] > 1:
                rest = dots.copy()
                rest[np.arange(qt.shape[0]), a] = -np.inf
                second[qq, c, : qt.shape[0]] = rest.max(axis=1)
    return arg, best, second


def dot_term(q_bits, d_bits) -> float:
    """The per-dot share of DESIGN section 21's band, ``1.01 * 2 * 384 * 2^-24 * max ||q_i|| * max ||d_t||``."""
    qn = np.sqrt((bf16_values(q_bits).astype(np.float64) ** 2).sum(axis=-1)).max()
    dn = np.sqrt((bf16_values(d_bits).astype(np.float64) ** 2).sum(axis=-1)).max()
    return float(1.01 * 2 * DIM * 2.0 ** -24 * qn * dn)


# ------------------------------------------------------------------ case generators
def random_case(seed: int, tqs, tds, R: int):
    """Random unit tokens.  ``cand [nq, R]``: every query names documents in a rotating order, so a document is shared
    by several queries; where R allows it holds a -1, an id outside the batch and a duplicate; the LAST document is named
    by nobody (when there are at least two)."""
    rng = np.random.default_rng(seed)
    q_lims, d_lims = lims_of(tqs), lims_of(tds)
    q_bits = unit_token_bits(rng, int(q_lims[-1]))
    d_bits = unit_token_bits(rng, int(d_lims[-1]))
    nq, nd = len(tqs), len(tds)
    named = max(nd - 1, 1)
    cand = np.empty((nq, R), np.int64)
    for q in range(nq):
        cand[q] = (np.arange(R) + q) % named
        if R >= 5:
            cand[q, 1] = -1
            cand[q, 2] = nd + 3                   # outside the batch
            cand[q, 4] = cand[q, 0]               # a duplicate: both entries contribute
    return q_bits, q_lims, d_bits, d_lims, cand


SHAPES = [
    # (name, Tq per query, Td per document, R)
    ("nq1-tq1-R1", [1], [1, 31], 1),
    ("nq3-R5", [31, 32, 33], [1, 31, 32, 33, 65, 180], 5),
    ("nq3-R9", [128, 1, 33], [180, 65, 33, 32, 31, 1, 7], 9),
    ("nq1-R9", [32], [33, 180, 2, 65, 5], 9),
]


def separated_case(seed: int = 23, tqs=(33, 5), extra=(32, 147, 0)):
    """Every document of query q holds a copy of EACH of q's tokens, shuffled among ``extra`` random rows: the maximum for
    query token i is its own copy (dot = ||q_i||^2, about 1) and the runner-up a random row or another query token (a few
    tenths at most), so the fp64 argmax is the argmax by a margin no rounding of the kernel can bridge.  One document per
    (query, extra); ``cand [nq, len(extra)]``."""
    rng = np.random.default_rng(seed)
    q_lims = lims_of(tqs)
    q_bits = unit_token_bits(rng, int(q_lims[-1]))
    docs, cand = [], np.empty((len(tqs), len(extra)), np.int64)
    for q, tq in enumerate(tqs):
        for c, n_extra in enumerate(extra):
            rows = np.concatenate([q_bits[q_lims[q]: q_lims[q + 1]], unit_token_bits(rng, n_extra).reshape(-1, DIM)])
            cand[q, c] = len(docs)
            docs.append(rows[rng.permutation(rows.shape[0])])
    d_lims = lims_of([r.shape[0] for r in docs])
    return q_bits, q_lims, np.concatenate(docs), d_lims, cand


def tie_case(seed: int = 29):
    """Documents that hold the SAME row twice, both the maximum for query token 2: at t and t + 40 (different tiles, the
    second in a partial tile for the shorter document) and at t and t + 5 (one tile).  ``(..., cand, expect)`` with
    ``expect[c]`` the index the tie rule reports for query token 2."""
    rng = np.random.default_rng(seed)
    q_lims = lims_of([5])
    q_bits = unit_token_bits(rng, 5)
    spots = [(65, 10, 50), (44, 3, 43), (33, 20, 25), (180, 100, 140)]
    docs = []
    for td, t, t2 in spots:
        rows = unit_token_bits(rng, td)
        rows[t] = rows[t2] = q_bits[2]
        docs.append(rows)
    d_lims = lims_of([s[0] for s in spots])
    return q_bits, q_lims, np.concatenate(docs), d_lims, np.arange(len(spots), dtype=np.int64)[None, :], [s[1] for s in spots]


def pack_bwd_case(seed: int = 31):
    """``(hidden bits [B, S, 384], lengths, dtok fp32 [T, 384])``: S = 40 with lengths 40, 33, 1, 7; a row of zeros (the
    1e-12 floor decides n), rows scaled by 2^20 and 2^-20."""
    rng = np.random.default_rng(seed)
    lengths = np.array([40, 33, 1, 7], np.int32)
    h = rng.standard_normal((4, 40, DIM)).astype(np.float32)
    h[0, 3] = 0.0
    h[0, 5] *= np.float32(2.0 ** 20)
    h[1, 0] *= np.float32(2.0 ** -20)
    h[3] *= np.float32(2.0 ** 20)
    dtok = rng.standard_normal((int(lengths.sum()), DIM)).astype(np.float32)
    dtok[3] *= np.float32(2.0 ** -30)      # the gradient of the zero row: g / 1e-12 stays finite in bf16
    return bf16_bits(h), lengths, dtok
