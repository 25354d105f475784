"""The checker of the diversified search: the rule of include/sskd_amd.h ("Diversified search") restated on the host, and
the input families the tests run on.

Written from the definition, not from the product code (one HIP kernel behind ``diversify.py``):

    candidates   the entries of the ranking up to the first id -1, ids outside [0, n_rows) skipped, in list order:
                 c_0 .. c_{m-1} with relevance s_i, the list's fp32 score as given
    similarity   sim(i, j) = oracle.search.scores_fma(rows[c], rows[c]): the exact scan's fp32 chain, symmetric bit for bit
    redundancy   red_i unset at the start; after p is selected every alive i gets red_i = sim(i, p) if red_i is unset or
                 sim(i, p) > red_i (fp32, strict); then red_i >= dup_threshold kills i
    value        fp64, every operation rounded once: lambda * s_i - (1.0 - lambda) * r_i, r_i = red_i or +0.0 while unset
    selection    up to k times while somebody is alive: the largest value, ties to the earlier position
    output       selection order: s, row + id_offset, the value, r; padded with (-FLT_MAX, -1, -inf, NaN); the count

The candidates of one query are held in NumPy arrays; an elementwise NumPy fp64 (fp32) operation rounds once per
element like the Python float operation it stands for, and ``argmax`` returns the first of equal maxima.
"""
import numpy as np

from oracle import search as oracle

F32 = np.float32
NEG_PAD = np.finfo(np.float32).min   # -FLT_MAX


def mmr_query(scores, ids, rows, *, k, lam, dup_threshold=np.inf, id_offset=0, gram=None):
    """One query: its ranking (fp32 scores, int64 local rows) and the index rows fp32 ``[n, dim]``.  ``gram``: the
    similarities of ALL rows computed once (``scores_fma(rows, rows)``) - entry for entry what the per-query call gives.
    Returns ``(D fp32 [k], I int64 [k], mmr fp64 [k], red fp32 [k], count)``."""
    n_rows = rows.shape[0]
    cand_s, cand = [], []
    for s, r in zip(scores, ids):
        r = int(r)
        if r == -1:
            break
        if r < 0 or r >= n_rows:
            continue
        cand_s.append(F32(s))
        cand.append(r)
    m = len(cand)
    D = np.full(k, NEG_PAD, F32)
    I = np.full(k, -1, np.int64)
    V = np.full(k, -np.inf, np.float64)
    R = np.full(k, np.nan, F32)
    if m == 0:
        return D, I, V, R, 0
    c = np.array(cand, np.int64)
    sim = gram[np.ix_(c, c)] if gram is not None else oracle.scores_fma(rows[c], rows[c])   # [query j][row i]
    s64 = np.array(cand_s, F32).astype(np.float64)
    red = np.zeros(m, F32)
    unset = np.ones(m, bool)
    alive = np.ones(m, bool)
    a, b = float(lam), 1.0 - float(lam)
    thr = F32(dup_threshold)
    count = 0
    while count < k and alive.any():
        r64 = np.where(unset, 0.0, red.astype(np.float64))
        value = a * s64 - b * r64                       # two products and one subtraction, each rounded once
        p = int(np.argmax(np.where(alive, value, -np.inf)))
        if not alive[p]:                                # every alive value is -inf: the first alive one
            p = int(np.flatnonzero(alive)[0])
        D[count], I[count], V[count] = cand_s[p], cand[p] + id_offset, value[p]
        R[count] = F32(0.0) if unset[p] else red[p]
        alive[p] = False
        count += 1
        to_p = sim[p]                                   # sim(i, p): row c_i, query c_p
        raise_ = alive & (unset | (to_p > red))
        red = np.where(raise_, to_p, red).astype(F32)
        unset = unset & ~alive
        alive = alive & ~(red >= thr)
    return D, I, V, R, count


def mmr_batch(S, I, rows, **kw):
    nq = len(I)
    k = kw["k"]
    out = [mmr_query(S[q], I[q], rows, **kw) for q in range(nq)]
    if not out:
        return (np.zeros((0, k), F32), np.zeros((0, k), np.int64), np.zeros((0, k), np.float64), np.zeros((0, k), F32),
                np.zeros(0, np.int32))
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.stack([o[3] for o in out]), np.array([o[4] for o in out], np.int32))


# ---------------------------------------------------------------------------------------------------- families
def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def clustered_family(centres=24, copies=20, noise=0.15, dim=384, n_queries=8, seed=0, twins=0):
    """``(rows fp32 unit [centres * copies + twins, dim], cluster of every row, queries fp32 unit [n_queries, dim])``:
    rows = centre + N(0, I) * noise with N(0, I) centres, L2-normalised (cosine about 0.98 inside a cluster, about 0
    across); query i lies between centres i and i + n_queries (0.6 / 0.4).  ``twins`` appends bit-identical copies of
    the first row of clusters 0 .. twins - 1: the same relevance and the same similarities, so exact value ties."""
    g = np.random.default_rng(seed)
    c = g.standard_normal((centres, dim))
    row_c = np.repeat(np.arange(centres), copies)
    rows = unit(c[row_c] + g.standard_normal((row_c.size, dim)) * noise)
    first = np.arange(n_queries)
    queries = unit(0.6 * c[first] + 0.4 * c[(first + n_queries) % centres])
    if twins:
        src = np.arange(twins) * copies
        rows = np.concatenate([rows, rows[src]])
        row_c = np.concatenate([row_c, row_c[src]])
    return rows, row_c, queries


def ranking(queries, rows, fetch_k):
    """The exact search's ranking at ``fetch_k`` (score descending, then lower row; padded with (-FLT_MAX, -1))."""
    return oracle.topk_fma(queries, rows, fetch_k)


def bits32(x):
    return np.ascontiguousarray(x, F32).view(np.int32)


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same(got, want, what):
    """Scores, ids, mmr, red and counts equal bit for bit (NaN padding included)."""
    assert np.array_equal(got[4], want[4]), f"{what}: counts {got[4]} != {want[4]}"
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ\n{got[1]}\n{want[1]}"
    assert np.array_equal(bits32(got[0]), bits32(want[0])), f"{what}: score bits differ"
    if got[2] is not None:
        assert np.array_equal(bits64(got[2]), bits64(want[2])), f"{what}: mmr bits differ"
    if got[3] is not None:
        assert np.array_equal(bits32(got[3]), bits32(want[3])), f"{what}: red bits differ"
