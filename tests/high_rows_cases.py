"""Shared cases of the high-row tests: a SPARSE index of millions of rows, its planted rows, and the reduced references.

Every entry point that takes the flat index accepts any shard below 2^31 - 64 rows.  A row number becomes an address by
a product (row x 1 536 bytes, row x 384 floats, row x 96 ``float4``), and a product formed in 32 bits goes wrong only
past a boundary no small test reaches.  The boundaries, as the row whose 1 536 bytes straddle each:

    ==========  ===================================  =====
    row         what wraps there                     tier
    ==========  ===================================  =====
     1 398 101  2^31 bytes   (int32 byte offset)     1, 2
     2 796 202  2^32 bytes   (uint32 byte offset)    1, 2
     5 592 405  2^31 floats  (int32 float index)     1, 2
    11 184 810  2^32 floats  (uint32 float index)    2
    22 369 621  2^31 float4  (int32 float4 index)    2
    ==========  ===================================  =====

(A uint32 ``float4`` index wraps at row 44 739 242, 64 GiB: no tier reaches it.)  The bf16 token store of the late
interaction (768 bytes a token) has its 2^31-byte boundary in token 2 796 202 and both its 2^32-byte and its
2^31-element boundary in token 5 592 405.

The index is all zeros but for a few dozen PLANTED rows, distinct seeded unit rows on both sides of every boundary (and
twelve booster rows in the first tiles, which let the screened search screen: ``BOOSTER_ROWS``).  A
zero row scores exactly +0.0 against any query, so the exact top-k of a query over the whole index equals the oracle's
top-k over a COMPRESSED corpus - the planted rows and the first k rows that are not planted (and allowed), in row
order - with the ids mapped back: zeros tie, and ties go to the lower id.  Nothing here is proportional to ``n_rows``.

This module is NumPy only and imports without a GPU.  It holds the data (tiers, plants, queries, masks, thresholds,
lists, graphs, rank lists, token documents), the compressed references - which delegate to ``oracle.search`` and the
``*_cases`` restatements of the entry points' own tests - and the truncation models ``tests/test_high_rows_host.py``
uses to show that the cases can fail.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from oracle import search as oracle

DIM = 384
TILE = 32
ROW_BYTES = DIM * 4
NQ = 70                    # the screened path needs nq >= 64 (and k <= 10) to screen at all
K = 10
ID_OFFSET = (1 << 40) + 7


def straddling(units: int, unit_bytes: int, row_bytes: int = ROW_BYTES) -> int:
    """the row whose bytes hold byte ``units x unit_bytes``"""
    return (units * unit_bytes) // row_bytes


# (row, what wraps there).  Every row here is the LAST one a truncated product still addresses correctly at its first
# byte; the rows after it are wrong from their first byte on.
TIER1_BOUNDARIES = (
    (straddling(1 << 31, 1), "2^31 bytes"),
    (straddling(1 << 32, 1), "2^32 bytes"),
    (straddling(1 << 31, 4), "2^31 floats = 2^33 bytes"),
)
TIER2_BOUNDARIES = TIER1_BOUNDARIES + (
    (straddling(1 << 32, 4), "2^32 floats"),
    (straddling(1 << 31, 16), "2^31 float4 = 2^35 bytes"),
)
assert [b for b, _ in TIER2_BOUNDARIES] == [1_398_101, 2_796_202, 5_592_405, 11_184_810, 22_369_621]
TIER1_N = 5_600_021        # ragged last tile of 21 rows; 8.0 GiB of fp32, 4.0 GiB of sidecar
TIER2_N = 22_400_021       # 32.0 GiB
TOKEN_BYTES = DIM * 2
TOKEN_N = 5_600_021
TOKEN_BOUNDARIES = (
    (straddling(1 << 31, 1, TOKEN_BYTES), "2^31 bytes"),
    (straddling(1 << 32, 1, TOKEN_BYTES), "2^32 bytes = 2^31 elements"),
)
assert [b for b, _ in TOKEN_BOUNDARIES] == [2_796_202, 5_592_405]


def plant_rows(n: int, boundaries) -> np.ndarray:
    """The planting rule: at every boundary the straddling row, the two rows before and the three after it, the first
    and last row of its 32-row tile and of the tile after it; and rows 0, 1, 31, 32, n - 22, n - 21 (the first row of the
    ragged last tile when n = 21 mod 32) and n - 1."""
    rows = {0, 1, 31, 32, n - 22, n - 21, n - 1}
    for b in boundaries:
        rows.update(range(b - 2, b + 4))
        t = b // TILE
        rows.update((TILE * t, TILE * t + 31, TILE * t + 32, TILE * t + 63))
    rows = np.array(sorted(rows), np.int64)
    assert rows[0] >= 0 and rows[-1] == n - 1
    return rows


# The screened search prunes with a lower bound of a query's k-th best score, learnt from a bound-only pass over the
# index's first 64 tiles and exchanged between workgroups through 32 buckets keyed by (row mod 32).  Over an index of
# zeros that bound stays at 0, every zero row lies inside the error band, every run overflows and every query is answered
# by the in-call exact scan: correct, and nothing was screened.  So twelve BOOSTER rows stand in the first tiles, in
# twelve different buckets; each scores between 0.04 and 0.13 against EVERY main query - well above the band, below every
# main query's tenth best planted score, so no booster enters a top 10 - and below 0 against the ties queries.
BOOSTER_ROWS = 64 + 33 * np.arange(12, dtype=np.int64)
BOOSTER_ALPHA = 0.085 + 0.005 * np.arange(12)
QUERY_SEED = 9401


def booster_values(rule_values):
    """booster i = unit(alpha_i u + w_i): u the mean direction of the rule rows, w_i a unit vector orthogonal to every
    rule row and to the random part of every main query - so its score against main query q is alpha_i <u, q> /
    sqrt(1 + alpha_i^2) and nothing else"""
    basis = np.concatenate([rule_values, oracle.seeded_unit_rows(NQ, DIM, QUERY_SEED)]).astype(np.float64)
    assert basis.shape[0] < DIM - BOOSTER_ROWS.size
    qr, _ = np.linalg.qr(basis.T)
    w = oracle.seeded_unit_rows(BOOSTER_ROWS.size, DIM, 9402).astype(np.float64)
    w -= (w @ qr) @ qr.T
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    u = rule_values.astype(np.float64).sum(0)
    u /= np.linalg.norm(u)
    b = BOOSTER_ALPHA[:, None] * u[None] + w
    return (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(np.float32)


class Compressed:
    """A few rows of the big index, in row order: ``rows`` int64 ascending, ``corpus`` fp32 [len(rows), 384].  A
    reference runs on ``corpus`` in compressed numbers (0 .. len - 1, the same ORDER as the rows, so every tie-break by
    lower id falls the same way) and ``ids`` maps its answer back."""

    def __init__(self, rows, corpus):
        self.rows = np.asarray(rows, np.int64)
        assert (np.diff(self.rows) > 0).all()
        self.corpus = np.ascontiguousarray(corpus, np.float32)
        assert self.corpus.shape == (self.rows.size, DIM)

    def ids(self, compressed_ids, id_offset=0):
        """compressed numbers -> rows + id_offset; -1 stays -1"""
        c = np.asarray(compressed_ids, np.int64)
        return np.where(c >= 0, self.rows[np.maximum(c, 0)] + id_offset, -1)

    def numbers(self, rows):
        """rows -> compressed numbers; -1 stays -1; a row that is not held is an error"""
        r = np.asarray(rows, np.int64)
        at = np.searchsorted(self.rows, np.maximum(r, 0))
        assert (self.rows[np.minimum(at, self.rows.size - 1)][r >= 0] == r[r >= 0]).all(), "a row outside the compressed corpus"
        return np.where(r >= 0, at, -1)


class Sparse:
    """``n`` rows, all zero but ``rows`` (ascending), which hold ``values``.  ``boundaries``: the straddling rows."""

    def __init__(self, n, boundaries, seed):
        self.n, self.boundaries = int(n), tuple(int(b) for b in boundaries)
        rule = plant_rows(self.n, self.boundaries)
        rule_values = oracle.seeded_unit_rows(rule.size, DIM, seed)
        assert not np.isin(BOOSTER_ROWS, rule).any()
        rows = np.concatenate([rule, BOOSTER_ROWS])
        values = np.concatenate([rule_values, booster_values(rule_values)])
        order = np.argsort(rows, kind="stable")
        self.rows, self.values, self.booster = rows[order], values[order], (np.arange(rows.size) >= rule.size)[order]
        for a in (self.rows, self.values, self.booster):
            a.setflags(write=False)
        self.padded = -(-self.n // TILE) * TILE

    @property
    def rule_rows(self):
        """the rows of the planting rule: planted row j of them leads main query j"""
        return self.rows[~self.booster]

    @property
    def rule_values(self):
        return self.values[~self.booster]

    @property
    def P(self):
        return self.rows.size

    def high_rows(self):
        """planted rows past the first boundary: the ones a truncated offset can miss"""
        return self.rows[self.rows > self.boundaries[0]]

    def blocks(self):
        """the planted rows as 32-row blocks for ``sskd_index_add_rows``: ``[(dst_row0, fp32 [32, 384])]``"""
        out = []
        for t in np.unique(self.rows // TILE):
            block = np.zeros((TILE, DIM), np.float32)
            sel = self.rows // TILE == t
            block[self.rows[sel] - TILE * t] = self.values[sel]
            out.append((int(TILE * t), block))
        return out

    def zero_rows(self, count, allowed=None, skip=()):
        """the first ``count`` rows that are not planted, not in ``skip`` and (``allowed``: a predicate on an int64
        array) allowed: the zero rows that can reach a result of ``count`` entries"""
        taken, out, lo = set(self.rows.tolist()) | set(int(s) for s in skip), [], 0
        while len(out) < count and lo < self.n:
            cand = np.arange(lo, min(lo + 4 * count + 64, self.n), dtype=np.int64)
            ok = np.ones(cand.size, bool) if allowed is None else np.asarray(allowed(cand), bool)
            out += [int(r) for r in cand[ok] if int(r) not in taken][: count - len(out)]
            lo = int(cand[-1]) + 1
        return np.array(out, np.int64)

    def compressed(self, k, allowed=None, extra=()):
        """planted (and allowed) rows + the first k allowed zero rows + ``extra`` zero rows, in row order"""
        keep = np.ones(self.P, bool) if allowed is None else np.asarray(allowed(self.rows), bool)
        zeros = self.zero_rows(k, allowed)
        extra = np.array([r for r in extra if r not in set(zeros.tolist()) and r not in set(self.rows.tolist())], np.int64)
        rows = np.concatenate([self.rows[keep], zeros, extra])
        corpus = np.concatenate([self.values[keep], np.zeros((zeros.size + extra.size, DIM), np.float32)])
        order = np.argsort(rows, kind="stable")
        return Compressed(rows[order], corpus[order])

    def dense(self):
        """the whole index as an array - for the MINIATURE only"""
        assert self.n <= 1 << 16
        out = np.zeros((self.n, DIM), np.float32)
        out[self.rows] = self.values
        return out


@lru_cache(maxsize=None)
def tier(which: int) -> Sparse:
    if which == 1:
        return Sparse(TIER1_N, [b for b, _ in TIER1_BOUNDARIES], 9100)
    if which == 2:
        return Sparse(TIER2_N, [b for b, _ in TIER2_BOUNDARIES], 9200)
    raise ValueError(which)


@lru_cache(maxsize=None)
def miniature() -> Sparse:
    """the same planting rule around stand-in boundaries at small rows: 3 093 rows, ragged last tile of 21"""
    return Sparse(3093, [290, 1000, 2590], 9300)


# ---------------------------------------------------------------------------------------------------------------------
# queries
# ---------------------------------------------------------------------------------------------------------------------
def _unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def main_queries(sp: Sparse, nq=NQ):
    """Query j leans on rule row j mod (number of rule rows) - its top hit: every rule row leads some query when there
    are at most nq of them - and on the mean direction of all rule rows (so well over k + 2 of them score above 0), plus
    a random part."""
    rnd = oracle.seeded_unit_rows(nq, DIM, QUERY_SEED)
    lead = sp.rule_values.astype(np.float64)
    mean = _unit(lead.sum(0))
    q = _unit(lead[np.arange(nq) % lead.shape[0]] + 1.5 * mean[None] + 0.5 * rnd)
    q.setflags(write=False)
    return q


TIES_POSITIVE = 4


def ties_queries(sp: Sparse, nq=3):
    """Exactly four planted rows score above 0 - one just past each of the first boundaries and the last row - and every
    other planted row below 0: the top 10 is those four and then the six lowest rows that are not planted."""
    mean = _unit(sp.rule_values.astype(np.float64).sum(0)).astype(np.float64)
    out = []
    for j in range(nq):
        chosen = [int(np.flatnonzero(sp.rows == b + 1 + j)[0]) for b in sp.boundaries[:3]] + [sp.P - 1]
        out.append(_unit(sp.values[chosen].astype(np.float64).sum(0) - 4.0 * mean))
    q = np.stack(out)
    q.setflags(write=False)
    return q


# ---------------------------------------------------------------------------------------------------------------------
# the compressed references
# ---------------------------------------------------------------------------------------------------------------------
def planted_scores(sp: Sparse, queries):
    """fma-order scores of every query against every planted row: fp32 [nq, P]"""
    return oracle.scores_fma(queries, sp.values)


def topk_ref(sp: Sparse, queries, k, id_offset=0, allowed=None):
    """(scores fp32 [nq, k], ids int64 [nq, k]) of the exact search over the whole sparse index"""
    c = sp.compressed(k, allowed)
    s, i = oracle.topk_fma(queries, c.corpus, k)
    return s, c.ids(i, id_offset)


def range_ref(sp: Sparse, queries, thresholds, id_offset=0, allowed=None):
    """(lims int64 [nq + 1], scores, ids) of the range search, every threshold at or above 0: only planted rows can
    match, in the order score descending (as the monotone integer image), then id ascending"""
    thresholds = np.asarray(thresholds, np.float32)
    assert (thresholds >= 0).all(), "a threshold below 0 would match every zero row"
    keep = np.ones(sp.P, bool) if allowed is None else np.asarray(allowed(sp.rows), bool)
    s = planted_scores(sp, queries)
    lims, S, I = [0], [], []
    for q in range(s.shape[0]):
        hit = np.flatnonzero(keep & (s[q] > thresholds[q]))
        order = hit[np.lexsort((sp.rows[hit], -s[q, hit].astype(np.float64)))]
        S.append(s[q, order])
        I.append(sp.rows[order] + id_offset)
        lims.append(lims[-1] + order.size)
    return np.array(lims, np.int64), np.concatenate(S).astype(np.float32), np.concatenate(I).astype(np.int64)


def range_thresholds(sp: Sparse, queries):
    """query q: the midpoint of its (m)-th and (m + 1)-th best planted scores, m = 1 + q mod 12 - strictly above 0 and
    strictly between two neighbouring planted scores (the host test asserts both)"""
    s = -np.sort(-planted_scores(sp, queries).astype(np.float64), axis=1)
    m = 1 + np.arange(s.shape[0]) % 12
    return ((s[np.arange(s.shape[0]), m - 1] + s[np.arange(s.shape[0]), m]) / 2).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------
def masked_rows(sp: Sparse) -> np.ndarray:
    """the filtered searches clear two planted rows on each side of every boundary: b - 2, b - 1 and b + 1, b + 2"""
    out = []
    for b in sp.boundaries:
        out += [b - 2, b - 1, b + 1, b + 2]
    return np.array(sorted(out), np.int64)


def allow_all_but(cleared):
    cleared = np.asarray(cleared, np.int64)
    return lambda rows: ~np.isin(np.asarray(rows, np.int64), cleared)


def mask_edits(n, cleared):
    """the words of an all-ones mask that change when ``cleared`` rows are cleared: (word numbers int64, values uint32).
    The bits at or past ``n`` stay set (they are ignored)."""
    cleared = np.asarray(cleared, np.int64)
    assert ((cleared >= 0) & (cleared < n)).all()
    words = np.unique(cleared >> 5)
    vals = np.full(words.size, 0xFFFFFFFF, np.uint32)
    for r in cleared:
        vals[np.searchsorted(words, r >> 5)] &= np.uint32(~(1 << int(r & 31)) & 0xFFFFFFFF)
    return words, vals


def compaction_drops(sp: Sparse, count=1000):
    """about ``count`` rows spread over the index (one every n // count rows, from row 7 on) and every third planted
    row: what compaction removes.  Sorted, unique."""
    spread = np.arange(7, sp.n, sp.n // count, dtype=np.int64)
    return np.unique(np.concatenate([spread, sp.rows[::3]]))


def compacted(sp: Sparse, drops):
    """(new row of every surviving planted row, their values, n_live)"""
    drops = np.asarray(drops, np.int64)
    live = ~np.isin(sp.rows, drops)
    rows = sp.rows[live]
    return rows - np.searchsorted(drops, rows), sp.values[live], sp.n - drops.size


# ---------------------------------------------------------------------------------------------------------------------
# truncation models (the host test): where a row's first byte lands when the product is formed in 32 bits
# ---------------------------------------------------------------------------------------------------------------------
def _wrap(v, signed):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if signed and v >= 1 << 31 else v


def truncation_models(row_bytes=ROW_BYTES):
    """name -> f(row) = the byte offset a kernel with that mistake reads the row at"""
    models = {}
    for name, unit in (("byte", 1), ("float" if row_bytes == ROW_BYTES else "element", 4 if row_bytes == ROW_BYTES else 2),
                       ("float4" if row_bytes == ROW_BYTES else "uint4", 16)):
        per_row = row_bytes // unit
        for signed in (True, False):
            models[f"{name} offset as {'int32' if signed else 'uint32'}"] = \
                (lambda r, per_row=per_row, unit=unit, signed=signed: _wrap(int(r) * per_row, signed) * unit)
    return models


def bytes_at(rows, values, n_padded, offset, nbytes):
    """``nbytes`` bytes of the sparse buffer from byte ``offset`` (uint8 array), or None when any of them lies outside
    the buffer.  ``values``: [P, row width] of any dtype."""
    row_bytes = values.shape[1] * values.dtype.itemsize
    if offset < 0 or offset + nbytes > n_padded * row_bytes:
        return None
    out = np.zeros(nbytes, np.uint8)
    first, last = offset // row_bytes, (offset + nbytes - 1) // row_bytes
    for r in range(first, last + 1):
        at = np.searchsorted(rows, r)
        if at < rows.size and rows[at] == r:
            raw = np.ascontiguousarray(values[at]).view(np.uint8)
            lo, hi = max(offset, r * row_bytes), min(offset + nbytes, (r + 1) * row_bytes)
            out[lo - offset: hi - offset] = raw[lo - r * row_bytes: hi - r * row_bytes]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# grouped search
# ---------------------------------------------------------------------------------------------------------------------
GROUPED_K_ROWS = 64


def planted_groups(sp: Sparse):
    """Background row r is in group r // 32 (its tile).  Planted rows are dealt, in row order, to P // 3 groups numbered
    from ``padded // 32`` on, planted row i to group i mod (P // 3): every such group holds rows on both sides of a
    boundary."""
    base = sp.padded // TILE
    return base, (base + np.arange(sp.P) % (sp.P // 3)).astype(np.int32)


def grouped_ref(sp: Sparse, queries, k, k_rows, id_offset=0):
    """``grouped_cases.expected`` on the compressed corpus: (D, I, G, counts, unproved)"""
    import grouped_cases as gc

    c = sp.compressed(k_rows)
    groups = (c.rows // TILE).astype(np.int32)
    groups[np.searchsorted(c.rows, sp.rows)] = planted_groups(sp)[1]
    D, I, G, cnt, unp = gc.expected(oracle.scores_fma(queries, c.corpus), groups, k, None, 0, k_rows)
    return D, c.ids(I, id_offset), G, cnt, unp


# ---------------------------------------------------------------------------------------------------------------------
# IVF / PQ: lists are contiguous row blocks, so list_rows is arange
# ---------------------------------------------------------------------------------------------------------------------
IVF_LIST_HALF = 96         # a boundary's list: rows [b - 96, b + 96) - both tiles the planting rule names, and more
IVF_K = 32                 # every planted row of a probed list that scores above 0 is returned: at k = 10 two rows of tier 2 never are


def ivf_lists(sp: Sparse):
    """(offsets int64 [nlist + 1], probe lists per boundary).  The cuts are 0, 64, then b - 96 and b + 96 of every
    boundary, n - 64, n: list 0 holds rows 0 .. 63, list 2 i + 2 the rows around boundary i, the last list the ragged
    tail.  ``d_list_rows`` is ``arange(n)``."""
    cuts = [0, 64]
    for b in sp.boundaries:
        cuts += [b - IVF_LIST_HALF, b + IVF_LIST_HALF]
    cuts += [sp.n - 64, sp.n]
    assert cuts == sorted(set(cuts))
    offsets = np.array(cuts, np.int64)
    small = [0] + [2 + 2 * i for i in range(len(sp.boundaries))] + [offsets.size - 2]
    return offsets, small


def ivf_probes(sp: Sparse, nq, nprobe=4):
    """probe lists int64 [nq, nprobe]: query q probes the small lists q, q + 1, ... (cyclically) - every query crosses
    boundaries, every boundary list is probed by many queries"""
    _, small = ivf_lists(sp)
    small = np.array(small, np.int64)
    return small[(np.arange(nq)[:, None] + np.arange(nprobe)[None]) % small.size]


def ivf_ref(sp: Sparse, queries, probe, k, id_offset=0):
    """exact top-k among the rows of the probed lists"""
    offsets, _ = ivf_lists(sp)
    S = np.empty((queries.shape[0], k), np.float32)
    I = np.empty((queries.shape[0], k), np.int64)
    for q in range(queries.shape[0]):
        lo, hi = offsets[probe[q]], offsets[probe[q] + 1]
        inside = lambda rows: ((np.asarray(rows)[:, None] >= lo[None]) & (np.asarray(rows)[:, None] < hi[None])).any(1)  # noqa: E731
        # the first k zero rows of the probed lists: lists are at most 192 rows, so walk their rows directly
        rows = np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in zip(lo, hi)])
        rows = np.unique(rows)
        planted = np.isin(rows, sp.rows)
        keep = np.concatenate([rows[planted], rows[~planted][:k]])
        keep.sort()
        corpus = np.zeros((keep.size, DIM), np.float32)
        at = np.isin(keep, sp.rows)
        corpus[at] = sp.values[np.searchsorted(sp.rows, keep[at])]
        assert inside(keep).all()
        s, i = oracle.topk_fma(queries[q: q + 1], corpus, k)
        S[q], I[q] = s[0], Compressed(keep, corpus).ids(i[0], id_offset)
    return S, I


# ---------------------------------------------------------------------------------------------------------------------
# IVF-PQ over the same lists: m = 8, no residual (d_assign = NULL), so a zero row stays a zero row
# ---------------------------------------------------------------------------------------------------------------------
PQ_M, PQ_REFINE = 8, 64


def pq_codebooks(sp: Sparse):
    """fp32 [8, 256, 48]: entry c < P of subspace j is planted row c's slice (a planted row encodes to itself, so ADC ranks
    it where the exact score would), the rest small random entries - the nearest of which is every zero row's code"""
    import pq_cases as pc

    cb = pc.seeded_codebooks(PQ_M, 9600).copy()
    dsub = DIM // PQ_M
    cb[:, : sp.P] = sp.values.reshape(sp.P, PQ_M, dsub).transpose(1, 0, 2)
    return np.ascontiguousarray(cb, np.float32)


def pq_codes(sp: Sparse, cb):
    """(codes of the planted rows uint8 [P, 8], the code of a zero row uint8 [8]) by ``pq_cases.encode``"""
    import pq_cases as pc

    codes = pc.encode(np.concatenate([sp.values, np.zeros((1, DIM), np.float32)]), cb)
    return codes[:-1], codes[-1]


def pq_code_lists(sp: Sparse, codes, zero_code, zeros_per_subspace=1000):
    """Group lists for ``sskd_pq_code_sums``: per subspace j and code c the planted rows with that code, and under the
    zero rows' code also ``zeros_per_subspace`` zero rows spread over the whole index - ascending rows within a code,
    the lists laid out back to back at the END of subspace j's n entries.
    Returns (offsets int64 [8, 257], [(position in the flat [8 x n] array, rows int32)], the listed rows per subspace)."""
    spread = np.setdiff1d(np.linspace(3, sp.n - 3, zeros_per_subspace).astype(np.int64), sp.rows)
    offsets = np.zeros((PQ_M, 257), np.int64)
    writes, listed = [], []
    for j in range(PQ_M):
        per_code = []
        for c in range(256):
            rows = sp.rows[codes[:, j] == c]
            if c == zero_code[j]:
                rows = np.sort(np.concatenate([rows, spread]))
            per_code.append(rows)
        total = sum(r.size for r in per_code)
        start = sp.n - total
        offsets[j] = start + np.concatenate([[0], np.cumsum([r.size for r in per_code])])
        flat = np.concatenate(per_code).astype(np.int32)
        writes.append((j * sp.n + start, flat))
        listed.append(flat.astype(np.int64))
    return offsets, writes, listed


def pq_code_sums_ref(sp: Sparse, codes, zero_code, listed):
    """``pq_cases.code_sums`` over the listed rows of every subspace: (sums fp64 [8, 256, 48], counts int64 [8, 256])"""
    import pq_cases as pc

    dsub = DIM // PQ_M
    sums = np.zeros((PQ_M, 256, dsub), np.float64)
    counts = np.zeros((PQ_M, 256), np.int64)
    for j in range(PQ_M):
        rows = np.unique(listed[j])
        at = np.isin(rows, sp.rows)
        resid = np.zeros((rows.size, DIM), np.float32)
        resid[at] = sp.values[np.searchsorted(sp.rows, rows[at])]
        code = np.tile(zero_code, (rows.size, 1))
        code[at] = codes[np.searchsorted(sp.rows, rows[at])]
        s, c = pc.code_sums(resid, code, PQ_M)
        sums[j], counts[j] = s[j], c[j]
    return sums, counts


def pq_search_ref(sp: Sparse, queries, probe, probe_scores, cb, codes, zero_code, k, refine, id_offset=0):
    """``pq_cases.adc_ranking`` on the rows of the small lists (every one of them, the zero rows too), then the exact
    top-k among the first ``refine``: (scores [nq, k], ids [nq, k], candidates [nq, refine])"""
    import pq_cases as pc

    offsets, small = ivf_lists(sp)
    nlist = offsets.size - 1
    rows = np.concatenate([np.arange(offsets[l], offsets[l + 1], dtype=np.int64) for l in small])
    at = np.isin(rows, sp.rows)
    corpus = np.zeros((rows.size, DIM), np.float32)
    corpus[at] = sp.values[np.searchsorted(sp.rows, rows[at])]
    code = np.tile(zero_code, (rows.size, 1))
    code[at] = codes[np.searchsorted(sp.rows, rows[at])]
    c = Compressed(rows, corpus)
    offsets_c = np.searchsorted(rows, offsets)            # a big list is empty here: it is never probed
    table = pc.lut(queries, cb)
    exact = oracle.scores_fma(queries, corpus)
    nq = queries.shape[0]
    S = np.empty((nq, k), np.float32)
    I = np.empty((nq, k), np.int64)
    cand = np.full((nq, refine), -1, np.int64)
    for q in range(nq):
        assert np.isin(probe[q], small).all()
        _, order = pc.adc_ranking(probe[q], probe_scores[q], offsets_c, np.arange(rows.size), nlist, table[q], code)
        want = order[:refine]
        cand[q, : want.size] = c.ids(want, id_offset)
        s = np.full((1, rows.size), -np.inf, np.float32)
        s[0, want] = exact[q, want]
        d, i = oracle.topk_of_scores(s, k)
        S[q], I[q] = d[0], c.ids(i[0], id_offset)
    return S, I, cand


# ---------------------------------------------------------------------------------------------------------------------
# graph: a small connected graph over the planted rows
# ---------------------------------------------------------------------------------------------------------------------
GRAPH_M = 8


def graph_edges(sp: Sparse, M=GRAPH_M):
    """adjacency int32 [P, M] in ROW numbers (-1 padded): planted row i links to the planted rows i +- 1, i +- 2 and
    i +- 7 (a ring: connected, and every walk from the low rows crosses every boundary)"""
    adj = np.full((sp.P, M), -1, np.int32)
    for i in range(sp.P):
        nb = [(i + d) % sp.P for d in (1, -1, 2, -2, 7, -7)]
        adj[i, : len(nb)] = sp.rows[nb]
    return adj


def graph_ref(sp: Sparse, queries, seeds_planted, k, ef, width):
    """``graph_cases.beam_search_batch_ref`` on the planted rows alone (no zero row has an edge or is a seed), ids
    mapped back: (scores, ids) and whatever else the restatement returns, untouched"""
    import graph_cases as gc

    c = Compressed(sp.rows, sp.values)
    adj = graph_edges(sp)
    adj_c = c.numbers(adj).astype(np.int32)
    out = gc.beam_search_batch_ref(planted_scores(sp, queries), adj_c, np.asarray(seeds_planted, np.int64), ef, width, ef, k)
    return out, c


# ---------------------------------------------------------------------------------------------------------------------
# rank lists for the gathers (mine, hybrid, Rocchio, MMR): every list names planted rows and a few zero rows
# ---------------------------------------------------------------------------------------------------------------------
RANK_K = 16


def rank_lists(sp: Sparse, queries, fetch_k=RANK_K, zeros=3):
    """A ranking as a search would write it (local rows, score descending then lower row, -1 padded): the exact top
    ``fetch_k`` of a sub-corpus that holds, for query q, the planted rows q, q + 1, ... q + fetch_k - zeros - 1
    (cyclically: every high planted row is in some list) and ``zeros`` zero rows from the high end of the index.
    Returns (scores fp32 [nq, fetch_k], rows int64 [nq, fetch_k], the Compressed corpus that holds every row named)."""
    nq = queries.shape[0]
    zero_rows = np.array([r for r in (sp.n - 2 - np.arange(4 * zeros)) if r not in set(sp.rows.tolist())][:zeros], np.int64)
    c = sp.compressed(0, extra=zero_rows.tolist())
    S = np.full((nq, fetch_k), oracle.NEG_PAD, np.float32)
    I = np.full((nq, fetch_k), -1, np.int64)
    full = oracle.scores_fma(queries, c.corpus)
    for q in range(nq):
        planted = sp.rows[(q + np.arange(fetch_k - zeros)) % sp.P]
        named = c.numbers(np.unique(np.concatenate([planted, zero_rows])))
        s = np.full((1, c.rows.size), -np.inf, np.float32)
        s[0, named] = full[q, named]
        d, i = oracle.topk_of_scores(s, fetch_k)
        S[q], I[q] = d[0], c.ids(i[0])
    return S, I, c, full


# ---------------------------------------------------------------------------------------------------------------------
# the token store of the late interaction
# ---------------------------------------------------------------------------------------------------------------------
def token_documents(n_tokens=TOKEN_N, boundaries=tuple(b for b, _ in TOKEN_BOUNDARIES), seed=9500):
    """Documents whose tokens lie across each boundary of the store, and a few low ones.
    Returns a namespace: ``spans`` [(first token, length)] ascending, ``offsets`` int64 / ``lengths`` int32 [n_docs],
    and the store's CSR ``tok_lims`` int64 [n_rows + 1] over ``n_rows = 2 n_docs + 1`` rows: row 2 d + 1
    (``doc_rows[d]``) is document d, the even rows own the zero tokens between the documents and are never a
    candidate; the last row is empty."""
    rng = np.random.default_rng(seed)
    spans = [(0, 40), (40, 33), (100, 7)]                     # low documents
    for b in boundaries:
        spans += [(b - 70, 60), (b - 10, 37), (b + 27, 5), (b + 32, 64), (b + 96, 1)]
    spans += [(n_tokens - 21, 21)]
    spans.sort()
    # CSR over 2 len(spans) + 1 rows: row 2 d + 1 is document d, the even rows are the gaps (never candidates)
    lims = [0]
    for off, ln in spans:
        assert off >= lims[-1]
        lims += [off, off + ln]
    lims.append(n_tokens)
    assert lims[-2] == n_tokens
    lims = np.array(lims, np.int64)
    docs = 2 * np.arange(len(spans), dtype=np.int64) + 1
    return SimpleNamespace(spans=spans, offsets=np.array([s[0] for s in spans], np.int64),
                           lengths=np.array([s[1] for s in spans], np.int32), tok_lims=lims, doc_rows=docs,
                           n_rows=lims.size - 1, n_tokens=n_tokens, rng=rng)
