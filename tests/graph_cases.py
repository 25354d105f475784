"""Graph index: the rules of ``include/sskd_amd.h`` ("Graph index") restated in plain NumPy / Python.

``beam_search_ref`` has no visited set at all: every offered row is scored and offered to the lists again, which by
the contract cannot change them.  Rank order everywhere: score descending, then lower row id."""
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

NEG_PAD = np.float32(-3.4028234663852886e38)


def _key(score: np.float32, row: int):
    return (-float(score), int(row))   # fp32 -> fp64 is exact, so the order is the fp32 order


def _offer(entries: list, held: set, cap: int, score: np.float32, row: int) -> None:
    """One row into a list of [key, score, row, expanded] kept in rank order (``held`` = the rows it holds): ignored
    when the list holds it, inserted otherwise, and the list cut to ``cap``."""
    if row in held:
        return
    key = _key(score, row)
    if len(entries) == cap and key > entries[-1][0]:
        return
    lo, hi = 0, len(entries)
    while lo < hi:
        mid = (lo + hi) // 2
        if entries[mid][0] < key:
            lo = mid + 1
        else:
            hi = mid
    entries.insert(lo, [key, score, row, False])
    held.add(row)
    if len(entries) > cap:
        held.discard(entries.pop()[2])


def beam_search_ref(score_row: Callable[[int], np.float32], graph: np.ndarray, seeds: Sequence[int], ef: int, width: int,
                    max_iterations: int, k: int, allowed: Optional[np.ndarray] = None
                    ) -> Tuple[np.ndarray, np.ndarray, int]:
    """One query.  ``score_row(r)`` = the exact fp32 score of row r; ``graph`` int ``[n, M]``; ``allowed`` bool ``[n]``
    or None.  Returns ``(scores [k], rows [k], iterations)`` padded with ``(NEG_PAD, -1)``."""
    n = graph.shape[0]
    T, R, in_T, in_R = [], [], set(), set()

    def offer(rows):
        for r in rows:
            r = int(r)
            if r < 0 or r >= n:
                continue
            s = score_row(r)
            _offer(T, in_T, ef, s, r)
            if allowed is None or allowed[r]:
                _offer(R, in_R, k, s, r)

    offer(seeds)
    iterations = 0
    while iterations < max_iterations:
        parents = [e for e in T if not e[3]][:width]
        if not parents:
            break
        for e in parents:
            e[3] = True
        offer([v for e in parents for v in graph[e[2]]])
        iterations += 1
    out_s = np.full(k, NEG_PAD, np.float32)
    out_i = np.full(k, -1, np.int64)
    for j, e in enumerate(R):
        out_s[j], out_i[j] = e[1], e[2]
    return out_s, out_i, iterations


def beam_search_batch_ref(scores: np.ndarray, graph: np.ndarray, seeds: np.ndarray, ef: int, width: int,
                          max_iterations: int, k: int, allowed: Optional[np.ndarray] = None):
    """``scores`` fp32 ``[nq, n]`` (the exact scores of every row), ``seeds`` int ``[nq, n_seeds]``."""
    out = [beam_search_ref(lambda r, row=row: row[r], graph, seeds[i], ef, width, max_iterations, k, allowed)
           for i, row in enumerate(scores)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32))


def _valid(v: int, u: int, n: int) -> bool:
    return 0 <= v < n and v != u


def detours_ref(knn: np.ndarray, M: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(detours int [n, K0] (-1 at entries that are not valid), fwd int32 [n, M])``.  The detour count of ``L_u[j]``:
    the number of i < j, ``L_u[i]`` valid, for which some p < j has ``L_{L_u[i]}[p] == L_u[j]``."""
    knn = np.asarray(knn, dtype=np.int64)
    n, K0 = knn.shape
    det = np.full((n, K0), -1, dtype=np.int64)
    fwd = np.full((n, M), -1, dtype=np.int32)
    pos = np.arange(K0)
    for u in range(n):
        L = knn[u]
        ok = (L >= 0) & (L < n) & (L != u)
        lists = knn[np.where(ok, L, 0)]                                    # [i, p]: the list of L_u[i]
        hit = (lists[:, :, None] == L[None, None, :]) & (pos[None, :, None] < pos[None, None, :])   # [i, p, j], p < j
        route = hit.any(axis=1) & (pos[:, None] < pos[None, :]) & ok[:, None]                       # [i, j], i < j
        det[u] = np.where(ok, route.sum(axis=0), -1)
        order = sorted((int(det[u, j]), j) for j in range(K0) if ok[j])[:M]
        fwd[u, :len(order)] = [L[j] for _, j in order]
    return det, fwd


def reverse_ref(fwd: np.ndarray) -> np.ndarray:
    """int32 ``[n, M / 2]``: the rows u that name v among the first M / 2 entries of ``fwd[u]``, by (position, u)."""
    n, M = fwd.shape
    h = M // 2
    found = [[] for _ in range(n)]
    for u in range(n):
        for pos in range(h):
            v = int(fwd[u, pos])
            if v >= 0:
                found[v].append((pos, u))
    rev = np.full((n, h), -1, dtype=np.int32)
    for v in range(n):
        best = sorted(found[v])[:h]
        rev[v, :len(best)] = [u for _, u in best]
    return rev


def merge_ref(fwd: np.ndarray, rev: np.ndarray) -> np.ndarray:
    n, M = fwd.shape
    h = M // 2
    graph = np.full((n, M), -1, dtype=np.int32)
    for u in range(n):
        row = []
        for v in list(fwd[u, :h]) + list(rev[u]) + list(fwd[u, h:]):
            v = int(v)
            if _valid(v, u, n) and v not in row:
                row.append(v)
        row = row[:M]
        graph[u, :len(row)] = row
    return graph


def remap_graph_ref(graph: np.ndarray, kept: Sequence[int]) -> np.ndarray:
    """The adjacency after compact, in plain Python: walk every surviving row's list, drop edges to rows that are gone,
    renumber the rest by position in ``kept``."""
    new_number = {int(old): j for j, old in enumerate(kept)}
    out = np.full((len(kept), graph.shape[1]), -1, dtype=np.int32)
    for j, old in enumerate(kept):
        row = [new_number[int(v)] for v in graph[int(old)] if int(v) in new_number]
        out[j, :len(row)] = row
    return out


def ring_graph(n: int, M: int) -> np.ndarray:
    """Row u points at u + 1 .. u + M (mod n): every row is reachable from every row."""
    return ((np.arange(n)[:, None] + np.arange(1, M + 1)[None, :]) % n).astype(np.int32)


def random_adjacency(n: int, M: int, seed: int) -> np.ndarray:
    """Arbitrary int32 adjacency: random rows with -1 pads, self loops, repeated edges and out-of-range ids mixed in."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, n, size=(n, M)).astype(np.int32)
    g[rng.random((n, M)) < 0.10] = -1
    loops = rng.random(n) < 0.2
    g[loops, 0] = np.arange(n)[loops]
    twice = rng.random(n) < 0.3
    g[twice, M - 1] = g[twice, 1]
    wild = rng.random((n, M)) < 0.02
    g[wild] = rng.choice(np.array([n, n + 7, 2 ** 31 - 1, -5], dtype=np.int64), size=int(wild.sum())).astype(np.int32)
    return g
