"""Shared cases of the grouped search tests: the oracle walk and the corpora (computed once, never modified).

The expected result of a query: the fma-order scores of every row (``oracle.search.scores_fma``), masked rows set to
-inf, rows ordered by ``lexsort`` on (score descending, row ascending) - ``search``'s full ranking - and the first
occurrence of every group kept, up to k.  Comparisons are bit-equal on D, I and G.
"""
from functools import lru_cache

import numpy as np

from oracle import search as oracle

DIM = 384
NEG_PAD = oracle.NEG_PAD


def ranking(score_row, allowed=None):
    """Local rows in ``search``'s order: score descending, then row ascending; -inf / NaN / masked rows left out."""
    s = np.asarray(score_row, np.float32).copy()
    if allowed is not None:
        s[~np.asarray(allowed, bool)] = -np.inf
    rows = np.flatnonzero(~(np.isnan(s) | np.isneginf(s)))
    return rows[np.lexsort((rows, -s[rows].astype(np.float64)))], s


def walk(score_row, groups, k, allowed=None, id_offset=0, k_rows=None):
    """The oracle for one query: ``(D [k], I [k], G [k], count, unproved)``.  With ``k_rows`` only the first ``k_rows``
    ranks are walked, and ``unproved`` is the oracle's own statement: fewer than k distinct groups among them, and rows
    remain behind them."""
    order, s = ranking(score_row, allowed)
    seen = order if k_rows is None else order[:k_rows]
    g = np.asarray(groups)[seen]
    _, first = np.unique(g, return_index=True)
    keep = seen[np.sort(first)][:k]
    D = np.full(k, NEG_PAD, np.float32)
    I = np.full(k, -1, np.int64)
    G = np.full(k, -1, np.int32)
    D[: keep.size] = s[keep]
    I[: keep.size] = keep + id_offset
    G[: keep.size] = np.asarray(groups)[keep]
    unproved = bool(k_rows is not None and keep.size < k and order.size > k_rows)
    return D, I, G, int(keep.size), unproved


def expected(scores, groups, k, allowed=None, id_offset=0, k_rows=None):
    """``walk`` for every query: D [nq, k], I, G, counts [nq], unproved [nq] bool."""
    rows = [walk(scores[q], groups, k, allowed, id_offset, k_rows) for q in range(scores.shape[0])]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
            np.array([r[3] for r in rows], np.int32), np.array([r[4] for r in rows], bool))


def same(got, ref, what=""):
    """bit-equal D, I, G"""
    D, I, G = (np.asarray(x) for x in got[:3])
    assert np.array_equal(I, ref[1]), (what, np.argwhere(I != ref[1])[:5])
    assert np.array_equal(G, ref[2]), (what, np.argwhere(G != ref[2])[:5])
    assert D.dtype == np.float32 and np.array_equal(D.view(np.uint32), ref[0].view(np.uint32)), what


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def runs_of_three(n=2000, nq=70):
    """Documents of 3 consecutive chunks that resemble each other (a document vector plus noise), so the best rows of
    a query cluster by document: ``(corpus, queries, groups, scores)``."""
    n_docs = -(-n // 3)
    docs = oracle.seeded_unit_rows(n_docs, DIM, 301)
    groups = (np.arange(n) // 3).astype(np.int32)
    corpus = docs[groups] + 0.5 * oracle.seeded_unit_rows(n, DIM, 302)
    corpus = (corpus / np.linalg.norm(corpus, axis=1, keepdims=True)).astype(np.float32)
    queries = oracle.seeded_unit_rows(nq, DIM, 303)
    return _freeze(corpus, queries, groups, oracle.scores_fma(queries, corpus))


@lru_cache(maxsize=None)
def random_groups(n=5000, nq=70, n_groups=40):
    """Rows dealt at random to a few large groups: the best 32 rows of a query hold about 22 distinct groups."""
    rng = np.random.default_rng(311)
    corpus = oracle.seeded_unit_rows(n, DIM, 312)
    queries = oracle.seeded_unit_rows(nq, DIM, 313)
    groups = rng.integers(0, n_groups, n).astype(np.int32)
    return _freeze(corpus, queries, groups, oracle.scores_fma(queries, corpus))


@lru_cache(maxsize=None)
def scaled_copies():
    """Ties at chosen ranks.  Every row is a multiple of one unit vector u, the query is u: a row's score grows with
    its factor and equal factors give equal bits.  By rank: 63 rows of their own groups; then two identical rows of ONE
    group at ranks 63 and 64 (the second lies across the 64-rank step of the collapse); ten more rows; then two
    identical rows of DIFFERENT groups; then the rest.  Row numbers are shuffled.  Returns ``(corpus, queries, groups,
    scores, named)``, ``named`` = the rows (same_lo, same_hi, diff_lo, diff_hi)."""
    n = 200
    u = oracle.seeded_unit_rows(1, DIM, 321)[0]
    factors = np.empty(n, np.float32)
    by_rank_groups = np.empty(n, np.int32)
    factors[:63] = 1.0 - 0.001 * np.arange(63)
    by_rank_groups[:63] = np.arange(63)
    factors[63:65] = 0.9
    by_rank_groups[63:65] = 63
    factors[65:75] = 0.89 - 0.001 * np.arange(10)
    by_rank_groups[65:75] = np.arange(64, 74)
    factors[75:77] = 0.8
    by_rank_groups[75:77] = (74, 75)
    factors[77:] = 0.7 - 0.001 * np.arange(n - 77)
    by_rank_groups[77:] = 76 + np.arange(n - 77) // 2
    perm = np.random.default_rng(322).permutation(n)       # rank position -> row number
    for a, b in ((63, 64), (75, 76)):                       # among equal scores the lower row ranks first
        if perm[a] > perm[b]:
            perm[a], perm[b] = perm[b], perm[a]
    corpus = np.empty((n, DIM), np.float32)
    groups = np.empty(n, np.int32)
    corpus[perm] = factors[:, None] * u[None, :]
    groups[perm] = by_rank_groups
    queries = u[None, :].copy()
    scores = oracle.scores_fma(queries, corpus)
    order, _ = ranking(scores[0])
    assert np.array_equal(order, perm), "the construction must rank the rows as laid out"
    named = (int(perm[63]), int(perm[64]), int(perm[75]), int(perm[76]))
    return _freeze(corpus, queries, groups, scores) + (named,)


@lru_cache(maxsize=None)
def one_big_group(n_copies, n_other, seed):
    """Group 0 = ``n_copies`` near-copies of the query direction (rows 0 .. n_copies - 1), then ``n_other`` singleton
    rows far from it: ``(corpus, queries, groups, scores)`` with one query."""
    q = oracle.seeded_unit_rows(1, DIM, seed)
    copies = q + 0.01 * oracle.seeded_unit_rows(n_copies, DIM, seed + 1)
    copies /= np.linalg.norm(copies, axis=1, keepdims=True)
    corpus = np.concatenate([copies, oracle.seeded_unit_rows(n_other, DIM, seed + 2)]).astype(np.float32)
    groups = np.concatenate([np.zeros(n_copies, np.int32), 1 + np.arange(n_other, dtype=np.int32)])
    return _freeze(corpus, q, groups, oracle.scores_fma(q, corpus))


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own aggregation (tests/golden/maxsim_small.json, made by tests/golden/make_golden_grouped.py)
# ---------------------------------------------------------------------------------------------------------------------
def maxsim_pairs():
    """About 30 ``(chunk_id, score)`` pairs: documents of one to five chunks, ids with several underscores and with
    none, a best chunk in first, middle and last place, equal scores inside a document.  Scores are multiples of 2^-10
    (exact in fp32 and in JSON) and no two documents share their best score."""
    ids = [
        "doc1_0", "doc1_1", "doc1_2",
        "my_long_doc_name_0", "my_long_doc_name_1", "my_long_doc_name_2", "my_long_doc_name_3", "my_long_doc_name_4",
        "plain", "other",
        "a_b_0", "a_b_1", "a_0", "a_1", "a_2",
        "x__0", "x__1", "7_0", "7_1", "7_10", "7_11",
        "trailing_", "single_0", "UPPER_lower_3", "UPPER_lower_12",
        "deep_a_b_c_d_0", "deep_a_b_c_d_1", "deep_a_b_c_0", "0", "1",
    ]
    rng = np.random.default_rng(331)
    raw = rng.permutation(np.arange(40, 40 + len(ids)))       # distinct numerators: no ties between documents
    scores = [float(x - 51) / 1024.0 for x in raw]              # a few are negative
    scores[1] = scores[0]                                      # an equal pair inside doc1
    return [[i, s] for i, s in zip(ids, scores)]
