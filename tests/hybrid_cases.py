"""The checker of hybrid fusion: the rule of include/sskd_amd.h ("Hybrid fusion") restated in Python floats and loops.

Written from the definition, not from the product code (one HIP kernel behind ``hybrid.py``).  It takes the two
rankings as they are, so it pins the fuse rule and not the searches:

    dense candidates   entries of (S, I) up to the first id -1, ids outside [0, n_rows) skipped
    BM25 candidates    entries of (B, J) up to the first id -1, skipping ids outside [0, n_rows), scores equal to 0.0
                       (either sign) and rows the mask hides
    ranks              1-based positions among each list's candidates
    union              one entry per distinct row
    rrf                fused = ws * (1 / (rrf_k + rank_s)) + wb * (1 / (rrf_k + rank_b)), an absent side adds +0.0
    linear             both scores for every union row (the full score vectors supply what a list lacks), then
                       n = (x - min) / (max - min) per side over the union (0.0 everywhere when max == min) and
                       fused = ws * ns + wb * nb
    result             the best k under (fused descending, row ascending), padded with (-inf, -1)

Python floats are IEEE fp64 and every operation above is rounded once.  A float32 widens exactly through ``float``.
"""
import math

import numpy as np

from bm25_cases import Oracle, float_bits, tokenize   # noqa: F401  (re-exported for the tests)

NAN = float("nan")


def full_dense_scores(queries, corpus):
    """fp32 [nq, n_rows]: every row's score in the fma order of the exact scan (the bits a search returns)."""
    from oracle import search as oracle

    return oracle.scores_fma(queries, corpus)


def full_bm25_scores(oracle_bm25, text):
    """Python floats [n_rows]: every row's BM25Okapi score for the query text."""
    return oracle_bm25.scores(tokenize(text))


def _low(values):
    # the minimum; where +0.0 and -0.0 both occur, -0.0
    return min(values, key=lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1))


def _high(values):
    return max(values, key=lambda x: (x, 0 if math.copysign(1.0, x) < 0 else 1))


def fuse_query(dense_scores, dense_ids, bm25_scores, bm25_ids, *, n_rows, k, method, ws, wb, rrf_k=60.0, id_offset=0,
               allowed=None, full_dense=None, full_bm25=None):
    """One query.  ``allowed``: None or a per-row bool sequence; ``full_dense`` / ``full_bm25``: per-row scores, needed
    by ``linear`` only.  Returns ``(scores, ids, count, dense, bm25)``: four lists of length ``k`` and the union size;
    an absent component is NaN."""
    rows = {}   # row -> [s, rank_s, b, rank_b], in order of first appearance
    rank = 0
    for s, r in zip(dense_scores, dense_ids):
        r = int(r)
        if r == -1:
            break
        if r < 0 or r >= n_rows:
            continue
        rank += 1
        rows[r] = [float(np.float32(s)), rank, None, 0]
    rank = 0
    for b, r in zip(bm25_scores, bm25_ids):
        r, b = int(r), float(b)
        if r == -1:
            break
        if r < 0 or r >= n_rows or b == 0.0 or (allowed is not None and not allowed[r]):
            continue
        rank += 1
        if r in rows:
            rows[r][2], rows[r][3] = b, rank
        else:
            rows[r] = [None, 0, b, rank]
    fused = {}
    if method == "rrf":
        for r, (s, rank_s, b, rank_b) in rows.items():
            ts = ws * (1.0 / (rrf_k + rank_s)) if rank_s else 0.0
            tb = wb * (1.0 / (rrf_k + rank_b)) if rank_b else 0.0
            fused[r] = ts + tb
    elif method == "linear":
        for r, e in rows.items():
            if e[0] is None:
                e[0] = float(np.float32(full_dense[r]))
            if e[2] is None:
                e[2] = float(full_bm25[r])
        if rows:
            s_min, s_max = _low([e[0] for e in rows.values()]), _high([e[0] for e in rows.values()])
            b_min, b_max = _low([e[2] for e in rows.values()]), _high([e[2] for e in rows.values()])
        for r, e in rows.items():
            ns = (e[0] - s_min) / (s_max - s_min) if s_max != s_min else 0.0
            nb = (e[2] - b_min) / (b_max - b_min) if b_max != b_min else 0.0
            fused[r] = ws * ns + wb * nb
    else:
        raise ValueError(method)
    order = sorted(rows, key=lambda r: (-fused[r], r))[:k]
    pad = k - len(order)
    scores = [fused[r] for r in order] + [-math.inf] * pad
    ids = [r + id_offset for r in order] + [-1] * pad
    dense = [NAN if rows[r][0] is None else rows[r][0] for r in order] + [NAN] * pad
    bm25 = [NAN if rows[r][2] is None else rows[r][2] for r in order] + [NAN] * pad
    return scores, ids, len(rows), dense, bm25


def fuse_batch(S, I, B, J, *, n_rows, k, method, ws, wb, rrf_k=60.0, id_offset=0, allowed=None, full_dense=None,
               full_bm25=None):
    """Every query of a batch: NumPy ``(scores fp64 [nq, k], ids int64, counts int32 [nq], dense fp32, bm25 fp64)``."""
    nq = len(I)
    out = [fuse_query(S[q], I[q], B[q], J[q], n_rows=n_rows, k=k, method=method, ws=ws, wb=wb, rrf_k=rrf_k,
                      id_offset=id_offset, allowed=allowed,
                      full_dense=None if full_dense is None else full_dense[q],
                      full_bm25=None if full_bm25 is None else full_bm25[q]) for q in range(nq)]
    return (np.array([o[0] for o in out], np.float64).reshape(nq, k), np.array([o[1] for o in out], np.int64).reshape(nq, k),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.float32).reshape(nq, k),
            np.array([o[4] for o in out], np.float64).reshape(nq, k))


def assert_same(got, want, what=""):
    """Fused scores by bit pattern, ids and counts exactly, components by bit pattern with NaNs at the same places."""
    g_scores, g_ids, g_dense, g_bm25, g_counts = got
    w_scores, w_ids, w_counts, w_dense, w_bm25 = want
    assert np.array_equal(g_ids, w_ids), f"{what}: ids differ at queries {np.flatnonzero((g_ids != w_ids).any(1))[:8]}"
    assert np.array_equal(np.asarray(g_scores, np.float64).view(np.int64), w_scores.view(np.int64)), f"{what}: fused bits"
    assert np.array_equal(np.asarray(g_counts, np.int32), w_counts), f"{what}: counts"
    for name, g, w, bits in (("dense", g_dense, w_dense, np.int32), ("bm25", g_bm25, w_bm25, np.int64)):
        g = np.asarray(g, w.dtype)
        assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: {name} NaN placeholders"
        live = ~np.isnan(w)
        assert np.array_equal(g.view(bits)[live], w.view(bits)[live]), f"{what}: {name} component bits"
