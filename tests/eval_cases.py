"""Cases and the host oracle of the retrieval-evaluation tests (NumPy only, seeded).

The oracle restates the definitions of include/sskd_amd.h "Retrieval evaluation" - the summation order of ``np.sum``
included - and does not call the product's ``evaluation.py``.  ``tests/golden/make_golden_eval.py`` feeds the same cases
to the reference's own metric code; ``tests/golden/eval_small.npz`` / ``.json`` hold what it returned.
"""
from __future__ import annotations

import numpy as np

DISC = np.log2(np.arange(2, 258))        # discount of rank i (0-based): log2(i + 2), NumPy's bits
CUTOFFS = (1, 5, 8, 10, 20, 128, 129, 256)
LIST_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 136, 255, 256, 257, 1023, 1024)
MIN_SCORE_GAP = 5e-4                     # adjacent sorted scores of every generated list differ by at least this
EDGE_MARGIN = 1e-4                       # no ECE confidence lies this close to a bin edge or to 0.5


# ------------------------------------------------------------------------------------------- summation model
def _block_sum(a: np.ndarray) -> np.float64:
    m = len(a)
    if m < 8:
        res = np.float64(0.0)
        for x in a:
            res = res + x
        return res
    r = [np.float64(a[j]) for j in range(8)]
    i = 8
    while i + 8 <= m:
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for x in a[i:]:
        res = res + x
    return res


def np_sum_model(a) -> np.float64:
    """The order in which ``np.sum`` adds a contiguous fp64 vector: blocks of at most 128 by eight accumulators, longer
    vectors split at ``h = m/2 - (m/2) % 8`` and the halves added."""
    a = np.asarray(a, dtype=np.float64)
    m = len(a)
    if m <= 128:
        return _block_sum(a)
    h = m // 2
    h -= h % 8
    return np_sum_model(a[:h]) + np_sum_model(a[h:])


# ------------------------------------------------------------------------------------------- the oracle
def rank_order(scores) -> np.ndarray:
    """Positions of a list in rank order: score descending, then lower position; NaN below every number."""
    s = np.asarray(scores, dtype=np.float32)
    nan = np.isnan(s)
    key = np.where(nan, -np.inf, s.astype(np.float64))
    return np.array(sorted(range(len(s)), key=lambda i: (bool(nan[i]), -key[i], i)), dtype=np.int64)


def discordant_pairs(scores, ref_scores) -> int:
    """Unordered pairs of one list that the two score lists rank in opposite order (O(n^2))."""
    n = len(scores)
    ra, rb = np.empty(n, np.int64), np.empty(n, np.int64)
    ra[rank_order(scores)] = np.arange(n)
    rb[rank_order(ref_scores)] = np.arange(n)
    if n < 2:
        return 0
    a = ra[:, None] < ra[None, :]
    b = rb[:, None] < rb[None, :]
    return int(np.triu(a != b, 1).sum())


def oracle_metrics(ranked_grades, judged_grades, k_values, ideal_mode: int) -> np.ndarray:
    """``[n_cut, 4]`` = (ndcg, mrr, recall, precision) of one query from its grades in rank order and its judged grades."""
    g = np.asarray(ranked_grades, dtype=np.int64)
    judged = np.asarray(judged_grades, dtype=np.int64)
    n_relevant = int((judged > 0).sum())
    out = np.zeros((len(k_values), 4), np.float64)
    for c, k in enumerate(k_values):
        m = min(k, len(g))
        head = g[:m]
        dcg = np_sum_model(head.astype(np.float64) / DISC[:m])
        if ideal_mode == 0:
            best = np.sort(head)[::-1]
        else:
            best = np.sort(judged)[::-1][: min(k, len(judged))]
        idcg = np_sum_model(best.astype(np.float64) / DISC[: len(best)])
        ndcg = np.float64(0.0) if idcg == 0 else dcg / idcg
        hit = np.flatnonzero(head > 0)
        mrr = np.float64(1.0) / np.float64(hit[0] + 1) if len(hit) else np.float64(0.0)
        recall = np.float64(len(hit)) / np.float64(n_relevant) if n_relevant else np.float64(0.0)
        precision = np.float64(len(hit)) / np.float64(k)
        out[c] = (ndcg, mrr, recall, precision)
    return out


# ------------------------------------------------------------------------------------------- candidate lists
def unit_rows(n: int, dim: int, rng) -> np.ndarray:
    v = rng.standard_normal((n, dim))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def separated_documents(query: np.ndarray, cosines: np.ndarray, rng) -> np.ndarray:
    """fp32 documents ``a_j q + sqrt(1 - a_j^2) u_j`` with ``u_j`` a unit vector orthogonal to the unit ``query``: the
    score of document j is ``a_j`` up to fp32 rounding, so the list's order is the order of ``cosines``."""
    q = query.astype(np.float64)
    u = rng.standard_normal((len(cosines), len(q)))
    u -= (u @ q)[:, None] * q[None, :]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = np.asarray(cosines, dtype=np.float64)
    return (a[:, None] * q[None, :] + np.sqrt(1.0 - a * a)[:, None] * u).astype(np.float32)


def cosine_grid(n: int, rng, lo: float = -0.8, hi: float = 0.8) -> np.ndarray:
    """``n`` shuffled values on an even grid over [lo, hi] (spacing (hi - lo) / (n - 1): 1.56e-3 at n = 1024)."""
    if n < 2:
        return np.full(n, 0.5 * (lo + hi) + 0.1)
    grid = np.linspace(lo, hi, n)
    return rng.permutation(grid)


def assert_separated(scores, lims) -> float:
    """Every list's adjacent sorted scores differ by at least MIN_SCORE_GAP; returns the smallest gap."""
    worst = np.inf
    for lo, hi in zip(lims[:-1], lims[1:]):
        if hi - lo > 1:
            worst = min(worst, float(np.diff(np.sort(np.asarray(scores[lo:hi], dtype=np.float64))).min()))
    assert worst >= MIN_SCORE_GAP, worst
    return worst


def list_batch(lengths, dim: int, seed: int, max_grade: int = 3, positive_share: float = 0.3, barren_every: int = 0):
    """One ragged batch: ``(queries fp32 [nq, dim], docs fp32 [total, dim], lims int64 [nq + 1], grades int32 [total],
    ref_scores fp32 [total])``.  Grades are 0 .. max_grade (``positive_share`` of them > 0); every ``barren_every``-th
    query has no positive at all.  ``ref_scores`` is a second, independently shuffled, equally separated score list."""
    rng = np.random.default_rng(seed)
    nq = len(lengths)
    lims = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    queries = unit_rows(nq, dim, rng).astype(np.float32)
    queries64 = queries.astype(np.float64)
    queries64 /= np.linalg.norm(queries64, axis=1, keepdims=True)
    docs = np.zeros((int(lims[-1]), dim), np.float32)
    grades = np.zeros(int(lims[-1]), np.int32)
    ref = np.zeros(int(lims[-1]), np.float32)
    for q, n in enumerate(lengths):
        lo, hi = lims[q], lims[q + 1]
        docs[lo:hi] = separated_documents(queries64[q], cosine_grid(n, rng), rng)
        g = rng.integers(1, max_grade + 1, n) * (rng.random(n) < positive_share)
        if barren_every and q % barren_every == barren_every - 1:
            g[:] = 0
        grades[lo:hi] = g
        ref[lo:hi] = (4.0 * cosine_grid(n, rng)).astype(np.float32)
    scores = np.einsum("ij,ij->i", docs.astype(np.float64), np.repeat(queries.astype(np.float64), lengths, axis=0))
    assert_separated(scores, lims)
    assert_separated(ref, lims)
    return queries, docs, lims, grades, ref


# ------------------------------------------------------------------------------------------- host-function cases
def graded_lists():
    """``[(grades in rank order, k)]`` for the host metric functions: graded and binary, empty, all-zero, k > n."""
    rng = np.random.default_rng(2024)
    cases = [([], 10), ([0, 0, 0, 0], 3), ([0, 0, 0, 0], 10), ([1], 1), ([1], 5), ([0, 1], 1), ([3, 2, 1, 0], 10),
             ([0, 0, 1, 0, 2, 3], 4), ([1, 0, 1, 1, 0, 0, 0, 1], 5), ([2] * 9, 8), ([0, 0, 0, 0, 0, 0, 0, 0, 1], 8)]
    for n in (7, 8, 9, 20, 64, 127, 128, 129, 136, 255, 256, 300):
        for k in (1, 5, 10, 20, 100, 128, 129, 256):
            graded = (rng.integers(1, 4, n) * (rng.random(n) < 0.4)).tolist()
            binary = (rng.random(n) < 0.25).astype(int).tolist()
            cases.append((graded, k))
            cases.append((binary, k))
    return cases


def id_cases():
    """``[(relevant ids, retrieved ids, k)]`` for recall / precision: derived from ``graded_lists`` (a retrieved id is
    relevant where the grade is positive) plus relevant ids that were never retrieved; k = 0 and empty sets included."""
    rng = np.random.default_rng(77)
    cases = [(set(), [1, 2, 3], 2), ({5}, [], 3), ({1, 2}, [2, 1, 7], 0)]
    for grades, k in graded_lists():
        retrieved = rng.permutation(len(grades) + 5)[: len(grades)].tolist()
        relevant = {rid for rid, g in zip(retrieved, grades) if g > 0}
        relevant |= {1000 + i for i in range(int(rng.integers(0, 4)))}
        cases.append((relevant, retrieved, k))
    return cases


def ranking_pairs():
    """``[(ranking1, ranking2)]`` for ``kendall_tau``: permutations, partial overlap, fewer than two common ids."""
    rng = np.random.default_rng(5)
    cases = [([], []), ([1], [1]), ([1, 2], [3, 4]), ([1, 2], [2, 1]), ([1, 2, 3], [1, 2, 3]), ([4, 3, 2, 1], [1, 2, 3, 4])]
    for n in (2, 3, 5, 10, 33, 64, 200):
        for _ in range(4):
            cases.append((rng.permutation(n).tolist(), rng.permutation(n).tolist()))
        a = rng.permutation(n + 6)[:n].tolist()
        b = rng.permutation(n + 6)[:n].tolist()
        cases.append((a, b))
    return cases


def away_from_edges(x: np.ndarray, n_bins: int = 10, but_extremes: bool = False) -> bool:
    """No value within EDGE_MARGIN of a bin edge (0 and 1 included) or of 0.5.  ``but_extremes``: for min-max-normalised
    scores the single smallest and the single largest value are exempt - the smallest maps to exactly 0.0 and the largest
    stays <= 1.0 in any arithmetic, so neither can change bins; every OTHER value must keep clear of 0 and 1 too (a
    second score next to the minimum could become the minimum under another summation order)."""
    x = np.asarray(x, dtype=np.float64)
    if but_extremes:
        x = np.delete(x, [int(np.argmin(x)), int(np.argmax(x))])
    marks = np.concatenate([np.linspace(0, 1, n_bins + 1), [0.5]])
    return bool((np.abs(x[:, None] - marks[None, :]) >= EDGE_MARGIN).all())


def ece_arrays():
    """``[(confidences, accuracies, n_bins)]``: confidences strictly inside (0, 1), none near an edge; fp32 and fp64."""
    rng = np.random.default_rng(9)
    cases = []
    for n, dtype, bins in ((1, np.float64, 10), (50, np.float32, 10), (400, np.float64, 10), (400, np.float32, 5),
                           (1000, np.float32, 10)):
        cells = rng.integers(0, 1000, n)                       # the value sits in the middle part of a 1e-3 cell
        conf = ((cells + rng.uniform(0.2, 0.8, n)) / 1000.0).astype(dtype)
        acc = (rng.random(n) < conf).astype(np.float64)
        assert away_from_edges(conf, bins)
        cases.append((conf, acc, bins))
    return cases


# ------------------------------------------------------------------------------------------- KDEvaluator cases
def retrieval_case():
    """A 384-d corpus all queries share: ``(queries [6, 384], corpus [40, 384], relevance_labels)``.  The queries are
    orthonormal and document j is ``sum_i a_ij q_i + rest``, so score(q_i, d_j) = a_ij: per query a shuffled grid over
    [-0.4, 0.4] (spacing 2e-2).  Some label lists are shorter than the corpus (missing = 0), one query has no positive."""
    rng = np.random.default_rng(31)
    nq, n, dim = 6, 40, 384
    basis, _ = np.linalg.qr(rng.standard_normal((dim, nq + n)))
    queries = basis[:, :nq].T
    a = np.stack([cosine_grid(n, rng, -0.4, 0.4) for _ in range(nq)])            # [nq, n]
    rest = np.sqrt(1.0 - (a * a).sum(axis=0))
    corpus = (a.T @ queries + rest[:, None] * basis[:, nq:].T).astype(np.float32)
    queries = queries.astype(np.float32)
    labels = []
    for q in range(nq):
        row = (rng.integers(1, 4, n) * (rng.random(n) < 0.2)).tolist()
        labels.append(row[: n - 3 * q])
    labels[4] = [0] * n
    scores = queries.astype(np.float64) @ corpus.astype(np.float64).T
    assert_separated(scores.reshape(-1), np.arange(0, nq * n + 1, n))
    return queries, corpus, labels


RANKING_GRID = 64   # every ranking-quality list draws its cosines from one grid of 64 values: j / 63 after normalisation


def ranking_case():
    """Per-query candidate lists for ``_evaluate_model`` / ``evaluate_ranking_quality``: ``(queries [nq, 64], docs
    [total, 64], lims, labels, teacher_scores)``.  Student scores come from the grid ``-0.8 + 1.6 j / 63``, teacher
    scores from ``-3 + 6 j / 63`` (shuffled independently).  The first list holds the whole grid and every other list
    draws from its interior (j = 1 .. 62), so the smallest and the largest score occur once; after the min-max
    normalisation of the flattened scores every value is ``j / 63``: at least 1.5e-3 from every bin edge and from 0.5,
    the one minimum (exactly 0.0) and the one maximum aside."""
    rng = np.random.default_rng(47)
    lengths = [64, 1, 2, 5, 10, 17, 20, 33, 60, 40, 8, 3]
    dim = 64
    nq = len(lengths)
    lims = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    queries = unit_rows(nq, dim, rng).astype(np.float32)
    queries64 = queries.astype(np.float64)
    queries64 /= np.linalg.norm(queries64, axis=1, keepdims=True)
    grid = np.arange(RANKING_GRID) / (RANKING_GRID - 1.0)

    def draw(q, n):
        return rng.permutation(RANKING_GRID)[:n] if q == 0 else 1 + rng.permutation(RANKING_GRID - 2)[:n]

    docs, labels, teacher = [], [], []
    for q, n in enumerate(lengths):
        docs.append(separated_documents(queries64[q], -0.8 + 1.6 * grid[draw(q, n)], rng))
        teacher.append((-3.0 + 6.0 * grid[draw(q, n)]).tolist())
        row = (rng.integers(1, 4, n) * (rng.random(n) < 0.3)).tolist()
        labels.append(row[: max(0, n - (q % 3))])          # some label lists are shorter than their documents
    docs = np.concatenate(docs)
    scores = np.einsum("ij,ij->i", docs.astype(np.float64), np.repeat(queries.astype(np.float64), lengths, axis=0))
    assert_separated(scores, lims)
    assert_separated(np.concatenate(teacher), lims)
    for flat in (scores, np.concatenate(teacher)):
        norm = (flat - flat.min()) / (flat.max() - flat.min() + 1e-8)
        assert away_from_edges(norm, 10, but_extremes=True)
    return queries, docs, lims, labels, teacher
