"""Shared cases of the hard-negative mining tests: the oracle, a NumPy model of the kernel's walk, and the corpora
(computed once, never modified).

The oracle is the project's own ``select_adversarial`` (pinned to the reference by tests/golden/ance_mining.json), applied
to a row ranking ``(D, I)`` with the positives (and, by group, their siblings) taken out of the candidates - what
``ANCEMiner._mine_from_index_host`` computes.  ``walk`` restates what the kernel does (threshold in fp64, survivors in
rank order, no sort) so that the two can be compared without a GPU.  Every comparison is exact: ids, scores as bits,
counts.
"""
from functools import lru_cache

import numpy as np

from oracle import search as oracle
from semantic_search_kd_amd.index import normalize_positives
from semantic_search_kd_amd.mining import select_adversarial

DIM = 384
NEG_PAD = oracle.NEG_PAD


# ---------------------------------------------------------------------------------------------------------------------
# the oracle and the model
# ---------------------------------------------------------------------------------------------------------------------
def _dropped(row, pos, groups, pos_groups):
    return row in pos or (groups is not None and int(groups[row]) in pos_groups)


def oracle_query(rank_scores, rank_rows, pos_rows, pos_scores, margin, top_k, groups=None, id_offset=0):
    """``(D [top_k], I [top_k], count, max_pos)`` of one query by ``select_adversarial``."""
    pos = set(int(r) for r in pos_rows)
    pos_groups = set() if groups is None else set(int(groups[r]) for r in pos)
    cand = []
    for s, r in zip(rank_scores, rank_rows):
        if r < 0:
            break
        if not _dropped(int(r), pos, groups, pos_groups):
            cand.append((int(r), np.float32(s)))
    score_of = dict(cand)
    assert len(score_of) == len(cand), "a ranking holds every row once"
    pos_scores = np.asarray(pos_scores, np.float32)
    kept = select_adversarial([r for r, _ in cand], np.array([s for _, s in cand], np.float32), pos_scores, margin,
                              max(len(cand), 1))
    D = np.full(top_k, NEG_PAD, np.float32)
    I = np.full(top_k, -1, np.int64)
    first = kept[:top_k]
    D[: len(first)] = [score_of[r] for r in first]
    I[: len(first)] = np.asarray(first, np.int64) + id_offset
    max_pos = np.float32(pos_scores.max()) if pos_scores.size else np.float32(0.0)
    return D, I, len(kept), max_pos


def walk(rank_scores, rank_rows, pos_rows, max_pos, margin, top_k, groups=None, id_offset=0, n_rows=None):
    """The kernel's walk for one query, in NumPy: stop at the first NEGATIVE id (-1 or any other: this kernel's own
    rule, ``csrc/ranking_walk.h``), skip an id at or above ``n_rows`` (when given), drop the positives (and their
    groups), keep a rank when ``float64(score) >= float64(max_pos) - margin``, write the first ``top_k`` survivors in
    rank order."""
    pos = set(int(r) for r in pos_rows)
    pos_groups = set() if groups is None else set(int(groups[r]) for r in pos)
    threshold = np.float64(np.float32(max_pos)) - np.float64(margin)
    D = np.full(top_k, NEG_PAD, np.float32)
    I = np.full(top_k, -1, np.int64)
    count = 0
    for s, r in zip(np.asarray(rank_scores, np.float32), rank_rows):
        if r < 0:
            break
        if n_rows is not None and r >= n_rows:
            continue
        if _dropped(int(r), pos, groups, pos_groups):
            continue
        if np.float64(s) >= threshold:
            if count < top_k:
                D[count], I[count] = s, int(r) + id_offset
            count += 1
    return D, I, count, np.float32(max_pos)


def expected(D, I, pos_lims, pos_rows, score_matrix, margin, top_k, groups=None, id_offset=0, fn=oracle_query):
    """``fn`` for every query of a ranking ``(D, I)`` in LOCAL rows; the positive scores come from ``score_matrix``
    ``[nq, n_rows]``.  Returns ``(D [nq, top_k], I, counts int32 [nq], max_pos float32 [nq])``."""
    # the positives go through the product's own normalisation (sorted, de-duplicated, range-checked), as in
    # ``mine_negatives``
    pos_lims, pos_rows = normalize_positives((np.asarray(pos_lims), np.asarray(pos_rows)), D.shape[0], score_matrix.shape[1])
    out = []
    for q in range(D.shape[0]):
        rows = np.asarray(pos_rows[pos_lims[q]:pos_lims[q + 1]], np.int64)
        ps = score_matrix[q, rows] if rows.size else np.zeros(0, np.float32)
        if fn is walk:
            ps = np.float32(ps.max()) if rows.size else np.float32(0.0)
        out.append(fn(D[q], I[q], rows, ps, margin, top_k, groups, id_offset))
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.float32))


def same(got, ref, what=""):
    """ids, scores as bits, counts, max_pos"""
    D, I, counts, max_pos = (np.asarray(x) for x in got)
    assert np.array_equal(I, ref[1]), (what, "ids", np.argwhere(I != ref[1])[:5])
    assert D.dtype == np.float32 and np.array_equal(D.view(np.uint32), ref[0].view(np.uint32)), (what, "scores")
    assert np.array_equal(counts, ref[2]), (what, "counts", np.flatnonzero(counts != ref[2])[:5])
    assert max_pos.dtype == np.float32 and np.array_equal(max_pos, ref[3]), (what, "max_pos")


def csr(lists):
    """row lists as ``(lims, rows)``, in the given order"""
    lims = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=lims[1:])
    rows = np.concatenate([np.asarray(x, np.int32) for x in lists]) if lists else np.zeros(0, np.int32)
    return lims, rows.astype(np.int32)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def full_ranking(scores, k):
    """``search``'s ranking of a score matrix: ``(D [nq, k], I [nq, k])`` local rows, -1 padded."""
    return oracle.topk_of_scores(scores, k)


# ---------------------------------------------------------------------------------------------------------------------
# corpora
# ---------------------------------------------------------------------------------------------------------------------
N_POS_CYCLE = (0, 1, 64, 65, 2)


@lru_cache(maxsize=None)
def mixed(n=2083, nq=70):
    """Random unit rows (a row count that is no multiple of 32, enough rows for the screened path) and 70 queries whose
    number of positives cycles through 0, 1, 64, 65, 2.  A query's positives: the rows at ranks 2 and 40 of its full
    ranking (inside every window of 64 ranks or more; rank 2 alone for one positive), then rows at ranks 300 and below
    (outside every window).  Returns ``(corpus, queries, scores, pos_lims, pos_rows)``; positives sorted per query."""
    corpus = oracle.seeded_unit_rows(n, DIM, 601)
    queries = oracle.seeded_unit_rows(nq, DIM, 602)
    scores = oracle.scores_fma(queries, corpus)
    _, order = full_ranking(scores, n)
    rng = np.random.default_rng(603)
    lists = []
    for q in range(nq):
        m = N_POS_CYCLE[q % len(N_POS_CYCLE)]
        inside = [order[q, 2], order[q, 40]][:m]
        outside = rng.choice(order[q, 300:], size=m - len(inside), replace=False).tolist()
        lists.append(sorted(int(r) for r in inside + outside))
    lims, rows = csr(lists)
    return _freeze(corpus, queries, scores, lims, rows)


@lru_cache(maxsize=None)
def duplicates(n=300):
    """Threshold ties: the corpus holds three exact copies of a query's positive row, so they score ``max_pos`` to the
    bit.  Query 0 is close to its positive (the copies are its best rows); query 1's positive sits at rank 20 of a
    random query, so better rows lie above the copies.  ``margin=0.0`` keeps the copies, ``margin=-1e-9`` drops them
    (in fp64; in fp32 the threshold would round back onto ``max_pos``).  Returns ``(corpus, queries, scores, pos_lims,
    pos_rows, copies)``, ``copies[q]`` = the rows holding copies of query q's positive."""
    corpus = oracle.seeded_unit_rows(n, DIM, 611).copy()
    q1 = oracle.seeded_unit_rows(1, DIM, 612)[0]
    p0 = 77
    q0 = corpus[p0] + 0.3 * oracle.seeded_unit_rows(1, DIM, 613)[0]
    q0 = (q0 / np.linalg.norm(q0)).astype(np.float32)
    taken = {p0, 10, 150, 299, 5, 201, 250}
    s1 = oracle.scores_fma(q1[None], corpus)[0]
    p1 = next(int(r) for r in np.argsort(-s1, kind="stable")[20:] if int(r) not in taken)
    copies = {0: [10, 150, 299], 1: [5, 201, 250]}
    corpus[copies[0]] = corpus[p0]
    corpus[copies[1]] = corpus[p1]
    queries = np.stack([q0, q1]).astype(np.float32)
    scores = oracle.scores_fma(queries, corpus)
    for q, p in ((0, p0), (1, p1)):
        assert (scores[q, copies[q]].view(np.uint32) == scores[q, p:p + 1].view(np.uint32)).all()
    assert (scores[0] > scores[0, p0]).sum() == 0 and 5 <= (scores[1] > scores[1, p1]).sum() <= 60
    lims, rows = csr([[p0], [p1]])
    return _freeze(corpus, queries, scores, lims, rows) + (copies,)


def decisions(s, max_pos, margin):
    """How three arithmetics decide ``s >= max_pos - margin`` for float32 scores ``s``: all in fp64; all in fp32; the
    fp64 difference rounded to fp32 (what NumPy >= 2 makes of a float32 scalar against a Python float)."""
    s = np.asarray(s, np.float32)
    in64 = s.astype(np.float64) >= np.float64(max_pos) - np.float64(margin)
    in32 = s >= np.float32(np.float32(max_pos) - np.float32(margin))
    rounded = s >= np.float32(np.float64(max_pos) - np.float64(margin))
    return in64, in32, rounded


@lru_cache(maxsize=None)
def threshold_neighbours(margin=0.1):
    """Scores within a few ulps of ``max_pos - margin``.  Every row is a multiple of one unit vector u and the query is
    u, so a row's score follows its factor: row 0 is the positive, rows 1 .. 129 have consecutive float32 factors
    around (positive factor - margin), the rest score far lower.  The positive's factor is the first of a few tried
    (on the CPU, here) at which an all-fp32 comparison and the fp64 comparison disagree for at least one row AND the
    rounded-threshold comparison disagrees for at least one row.  Returns ``(corpus, queries, scores, pos_lims,
    pos_rows, (disagree32, disagree_rounded))`` with the row lists."""
    u = oracle.seeded_unit_rows(1, DIM, 621)[0]
    n = 200
    for step in range(64):
        fpos = np.float32(0.9) + np.float32(step) * np.float32(0.0003)
        centre = np.float32(np.float64(fpos) - margin)
        near = np.empty(129, np.float32)
        near[64] = centre
        for i in range(64):
            near[63 - i] = np.nextafter(near[64 - i], np.float32(-1))
            near[65 + i] = np.nextafter(near[64 + i], np.float32(2))
        factors = np.concatenate([[fpos], near, np.float32(0.5) - np.float32(0.001) * np.arange(n - 130, dtype=np.float32)])
        corpus = (factors.astype(np.float32)[:, None] * u[None, :]).astype(np.float32)
        queries = u[None, :].copy()
        scores = oracle.scores_fma(queries, corpus)
        in64, in32, rounded = decisions(scores[0, 1:130], scores[0, 0], margin)
        d32 = (1 + np.flatnonzero(in64 != in32)).tolist()
        drounded = (1 + np.flatnonzero(in64 != rounded)).tolist()
        if d32 and drounded and in64.any() and not in64.all():
            lims, rows = csr([[0]])
            return _freeze(corpus, queries, scores, lims, rows) + ((d32, drounded),)
    raise AssertionError("no positive factor gives a row on which fp32 and fp64 disagree")


@lru_cache(maxsize=None)
def chunked(n_docs=150, nq=70):
    """Documents of 3 to 5 consecutive chunks that resemble each other (a document vector plus noise): the siblings of a
    positive chunk rank close to it.  Every query is close to one document and its positive is ONE chunk of it (the
    second).  Returns ``(corpus, queries, scores, groups, pos_lims, pos_rows)``."""
    rng = np.random.default_rng(631)
    sizes = rng.integers(3, 6, n_docs)
    groups = np.repeat(np.arange(n_docs), sizes).astype(np.int32)
    n = groups.size
    docs = oracle.seeded_unit_rows(n_docs, DIM, 632)
    corpus = docs[groups] + 0.5 * oracle.seeded_unit_rows(n, DIM, 633)
    corpus = (corpus / np.linalg.norm(corpus, axis=1, keepdims=True)).astype(np.float32)
    target = rng.integers(0, n_docs, nq)
    queries = docs[target] + 0.7 * oracle.seeded_unit_rows(nq, DIM, 634)
    queries = (queries / np.linalg.norm(queries, axis=1, keepdims=True)).astype(np.float32)
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    lims, rows = csr([[int(first[d]) + 1] for d in target])
    return _freeze(corpus, queries, oracle.scores_fma(queries, corpus), groups, lims, rows)
