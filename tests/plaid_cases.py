"""Candidate generation from the compressed token store (``include/sskd_amd.h``, "Candidate generation"; DESIGN section
23): the NumPy restatement, the fp64 reference and band of the centroid scores, and the case generators (no GPU).

* ``centroid_scores64`` / ``band_S``: ``S[c, t] = <centroid_c, q_t>`` in fp64 on the stored bf16 values and the bound
  ``1.01 * 2 * 384 * 2^-24 |q_t| |centroid_c|`` on ``|S - s64|`` (section 21's band for one dot product).
* ``build_lists_ref``: the centroid lists of a store.
* ``probes_ref`` / ``candidates_ref``: steps 2 - 5 as functions of the bits of ``S``: probes by (score descending,
  centroid ascending) without NaN and -inf, the union of the probed lists under the allow-mask, the centroid interaction
  (exact max that ignores NaN and starts from -inf, sequential fp32 sum from +0.0) and the cut by (approx descending, row
  ascending).
* ``clustered_family``: documents that mix a few topics, so that tokens have centroids worth probing.
"""
import numpy as np

import late_cases as lc
import late_codec_cases as cc

DIM = lc.DIM
NPROBE_MAX = 32
R_MAX = 1024


# ------------------------------------------------------------------ centroid scores
def centroid_scores64(centroid_bits, q_bits) -> np.ndarray:
    """fp64 ``[C, T]``: ``<centroid_c, q_t>`` on the stored bf16 values."""
    c = lc.bf16_values(np.asarray(centroid_bits).reshape(-1, DIM)).astype(np.float64)
    q = lc.bf16_values(np.asarray(q_bits).reshape(-1, DIM)).astype(np.float64)
    return c @ q.T


def band_S(centroid_bits, q_bits) -> np.ndarray:
    """``[C, T]``: ``1.01 * 2 * 384 * 2^-24 |q_t| |centroid_c|``."""
    c = lc.bf16_values(np.asarray(centroid_bits).reshape(-1, DIM)).astype(np.float64)
    q = lc.bf16_values(np.asarray(q_bits).reshape(-1, DIM)).astype(np.float64)
    return 1.01 * 2 * DIM * 2.0 ** -24 * np.outer(np.sqrt((c * c).sum(axis=1)), np.sqrt((q * q).sum(axis=1)))


# ------------------------------------------------------------------ lists
def build_lists_ref(cid, tok_lims, n_centroids: int):
    """``(list_lims int64 [C + 1], list_rows int32)``: row ``r`` is in list ``c`` exactly when some token of ``r`` has
    clamped centroid id ``c``; every pair once, rows ascending inside a list."""
    tok_lims = np.asarray(tok_lims, np.int64)
    n = tok_lims.size - 1
    c = np.clip(np.asarray(cid, np.int64), 0, n_centroids - 1)
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(tok_lims))
    pairs = np.unique(c * max(n, 1) + row_of)
    lims = np.concatenate([[0], np.cumsum(np.bincount(pairs // max(n, 1), minlength=n_centroids))]).astype(np.int64)
    return lims, (pairs % max(n, 1)).astype(np.int32)


# ------------------------------------------------------------------ steps 2 - 5
def probes_ref(S_q: np.ndarray, nprobe: int) -> np.ndarray:
    """``S_q`` fp32 ``[C, Tq]`` -> int64 ``[Tq, nprobe]``: per token the first ``nprobe`` centroids by (score descending,
    centroid ascending); NaN and -inf are never picked (-1 pads a token with fewer)."""
    out = np.full((S_q.shape[1], nprobe), -1, dtype=np.int64)
    for t in range(S_q.shape[1]):
        col = S_q[:, t]
        ok = np.flatnonzero(col > -np.inf)                           # false for -inf and for NaN
        best = ok[np.argsort(-col[ok], kind="stable")][:nprobe]      # stable: equal scores keep the lower centroid first
        out[t, : best.size] = best
    return out


def interaction_ref(S_q: np.ndarray, cid, tok_lims, n_centroids: int) -> np.ndarray:
    """fp32 ``[n_rows]``: ``approx(q, r) = sum_i max_j S[cid_j, t_i]`` over ALL tokens of ``r`` - the max exact, ignoring NaN,
    from -inf; the sum a sequential fp32 chain from +0.0 over the query's tokens in ascending order.  -inf for a row
    without tokens."""
    tok_lims = np.asarray(tok_lims, np.int64)
    n = tok_lims.size - 1
    c = np.clip(np.asarray(cid, np.int64), 0, n_centroids - 1)
    G = np.ascontiguousarray(S_q[c, :].T)                            # [Tq, n_tokens]
    best = np.full((S_q.shape[1], n), -np.inf, dtype=np.float32)
    full = np.flatnonzero(tok_lims[1:] > tok_lims[:-1])
    if full.size:
        with np.errstate(all="ignore"):
            seg = np.fmax.reduceat(G, tok_lims[full], axis=1)        # fmax: a NaN loses against any number
        best[:, full] = np.where(np.isnan(seg), -np.inf, seg)        # (all NaN: the max is still at its start, -inf)
    acc = np.zeros(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(S_q.shape[1]):
            acc = (acc + best[i]).astype(np.float32)
    return acc


def candidates_ref(S, q_lims, cid, tok_lims, list_lims, list_rows, n_centroids: int, nprobe: int, R: int, allowed=None,
                   id_offset: int = 0):
    """Steps 2 - 5 on ``S`` fp32 ``[C, >= T]`` (column ``q_lims[q] + i`` = token ``i`` of query ``q``): ``(cand_I int64
    [nq, R], cand_A fp32 [nq, R], n_cand int32 [nq])``.  ``allowed``: bool ``[n_rows]`` or None."""
    S = np.asarray(S, np.float32)
    q_lims, tok_lims = np.asarray(q_lims, np.int64), np.asarray(tok_lims, np.int64)
    list_lims, list_rows = np.asarray(list_lims, np.int64), np.asarray(list_rows, np.int64)
    nq, n = q_lims.size - 1, tok_lims.size - 1
    assert 1 <= nprobe <= min(n_centroids, NPROBE_MAX) and 1 <= R <= R_MAX
    cand_I = np.full((nq, R), -1, dtype=np.int64)
    cand_A = np.full((nq, R), -np.inf, dtype=np.float32)
    n_cand = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        S_q = S[:n_centroids, q_lims[q]: q_lims[q + 1]]
        probed = np.unique(probes_ref(S_q, nprobe))
        member = np.zeros(n, dtype=bool)
        for c in probed[probed >= 0]:
            rows = list_rows[max(list_lims[c], 0): min(list_lims[c + 1], list_rows.size)]
            member[rows[(rows >= 0) & (rows < n)]] = True
        if allowed is not None:
            member &= np.asarray(allowed, bool)
        rows = np.flatnonzero(member)                                # ascending
        n_cand[q] = rows.size
        approx = interaction_ref(S_q, cid, tok_lims, n_centroids)[rows]
        keep = approx > -np.inf                                      # drops -inf and NaN
        rows, approx = rows[keep], approx[keep]
        order = np.argsort(-approx, kind="stable")[:R]              # stable over ascending rows: ties to the lower row
        cand_I[q, : order.size] = rows[order] + id_offset
        cand_A[q, : order.size] = approx[order]
    return cand_I, cand_A, n_cand


def mask_words(allowed) -> np.ndarray:
    """bool ``[n_rows]`` -> the row allow-mask words (uint32, bit ``r & 31`` of word ``r >> 5``)."""
    a = np.asarray(allowed, bool)
    bits = np.zeros(-(-a.size // 32) * 32, dtype=np.uint8)
    bits[: a.size] = a
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)


# ------------------------------------------------------------------ the clustered family
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def clustered_family(seed: int = 29, n_docs: int = 2000, n_topics: int = 48, n_centroids: int = 256, n_queries: int = 100,
                     tq: int = 16, nbits: int = 2):
    """Documents of N(30, 8) tokens clipped to [4, 60], each mixing 3 of ``n_topics`` unit topic vectors: a token is
    ``unit(topic + g / sqrt(384))`` with ``g`` unit-variance Gaussian.  The centroids are ``n_centroids`` tokens spread
    evenly over the store (no training), the tables the quantiles of the residuals (ColBERTv2's rule).  A query is
    ``tq`` tokens drawn from one document, each with 0.3 of that noise added, normalised.  Returns a dict: ``tok`` (bf16
    bits), ``lims``, ``codec`` = (centroid bits, cutoffs, weights), ``q_bits``, ``q_lims``, ``source`` (the document
    every query was drawn from), ``nbits``."""
    rng = np.random.default_rng(seed)
    topics = _unit(rng.standard_normal((n_topics, DIM)))
    td = np.clip(np.rint(rng.normal(30.0, 8.0, n_docs)), 4, 60).astype(np.int64)
    lims = np.concatenate([[0], np.cumsum(td)]).astype(np.int64)
    doc_topics = np.stack([rng.permutation(n_topics)[:3] for _ in range(n_docs)])
    which = doc_topics[np.repeat(np.arange(n_docs), td), rng.integers(0, 3, int(lims[-1]))]
    noise = rng.standard_normal((int(lims[-1]), DIM)) / np.sqrt(DIM)
    tok = lc.normalize_rows_bits(lc.bf16_values(lc.bf16_bits(_unit(topics[which] + noise).astype(np.float32))))
    pick = (np.arange(n_centroids, dtype=np.int64) * int(lims[-1])) // n_centroids
    cen = tok[pick].copy()
    assign = cc.assign_rows(tok, cen)
    cut, w = cc.quantile_tables(lc.bf16_values(tok) - lc.bf16_values(cen[assign]), nbits)
    source = rng.integers(0, n_docs, n_queries)
    q = []
    for d in source:
        rows = rng.integers(lims[d], lims[d + 1], tq)
        q.append(_unit(lc.bf16_values(tok[rows]).astype(np.float64) + 0.3 * rng.standard_normal((tq, DIM)) / np.sqrt(DIM)))
    q_bits = lc.normalize_rows_bits(lc.bf16_values(lc.bf16_bits(np.concatenate(q).astype(np.float32))))
    q_lims = (np.arange(n_queries + 1, dtype=np.int64) * tq)
    return dict(tok=tok, lims=lims, codec=(cen, cut, w), q_bits=q_bits, q_lims=q_lims, source=source, nbits=nbits)


def compress_family(fam):
    """``(cid, scale, codes, dec bits)`` of the family's store under its codec (``late_codec_cases.compress_rows``)."""
    cen, cut, w = fam["codec"]
    return cc.compress_rows(fam["tok"], cc.assign_rows(fam["tok"], cen), cen, cut, w, fam["nbits"])


def exhaustive_ref(q_bits, q_lims, dec_bits, scale, tok_lims, k: int) -> np.ndarray:
    """The top-``k`` rows of every query by the compressed MaxSim in fp64 (``ReferenceC.s64``), lower row first on ties."""
    ref = cc.ReferenceC(q_bits, q_lims, dec_bits, scale, tok_lims)
    return np.argsort(-ref.s64, axis=1, kind="stable")[:, :k]


def recall_ref(fam, k: int = 10, nprobe: int = 2, ndocs: int = 256):
    """Recall@k of the restatement on the family, on the CPU: S in fp32 from the fp64 products (inside the band of the
    device's S), steps 2 - 5 by ``candidates_ref``, then the fp64 compressed MaxSim over the candidates - against the fp64
    compressed MaxSim over all rows.  Returns ``(recall, mean n_cand)``."""
    cid, scale, codes, dec = compress_family(fam)
    cen = fam["codec"][0]
    C = cen.shape[0]
    S = centroid_scores64(cen, fam["q_bits"]).astype(np.float32)
    lists = build_lists_ref(cid, fam["lims"], C)
    cand_I, _, n_cand = candidates_ref(S, fam["q_lims"], cid, fam["lims"], *lists, C, nprobe, ndocs)
    ref = cc.ReferenceC(fam["q_bits"], fam["q_lims"], dec, scale, fam["lims"])
    want = np.argsort(-ref.s64, axis=1, kind="stable")[:, :k]
    hits = 0
    for q in range(cand_I.shape[0]):
        rows = cand_I[q][cand_I[q] >= 0]
        got = rows[np.argsort(-ref.s64[q, rows], kind="stable")[:k]]
        hits += int(np.isin(want[q], got).sum())
    return hits / want.size, float(n_cand.mean())
