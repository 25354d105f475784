"""Graph index, incremental insertion: the rules of ``include/sskd_amd.h`` ("Incremental insertion") restated in plain
NumPy / Python on top of ``graph_cases``.  ``n0`` rows are linked, ``b`` rows are new, ids are global."""
import math
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np

import graph_cases as gc
from oracle import search as oracle


def knn_new_ref(corpus: np.ndarray, n0: int, K0: int) -> np.ndarray:
    """int32 ``[n1 - n0, K0]``: the exact nearest rows of the rows from ``n0`` on over ALL rows, without the row itself
    (or without the last entry when the row is not among its own results), -1 padded."""
    ids = oracle.topk_of_scores(oracle.scores_fma(corpus[n0:], corpus), K0 + 1)[1]
    out = np.empty((corpus.shape[0] - n0, K0), dtype=np.int32)
    for v, row in enumerate(ids):
        own = np.flatnonzero(row == n0 + v)
        out[v] = np.delete(row, own[0] if own.size else K0)
    return out


def insert_prune_ref(graph_old: np.ndarray, knn_new: np.ndarray, M: int) -> np.ndarray:
    """int32 ``[b, M]``.  The list of a neighbour w is ``graph_old[w]`` below n0 and ``knn_new[w - n0]`` from n0 on; the
    detour count of ``L[j]`` is the number of i < j, ``L[i]`` valid, for which some p < min(j, width of that list) has
    ``N(L[i])[p] == L[j]``; the valid entries by (detours, j), the first M."""
    graph_old = np.asarray(graph_old, dtype=np.int64)
    knn_new = np.asarray(knn_new, dtype=np.int64)
    n0, (b, K0) = graph_old.shape[0], knn_new.shape
    n1 = n0 + b
    width = max(K0, graph_old.shape[1] if n0 else 0)
    table = np.full((n1, width), -1, dtype=np.int64)          # a list narrower than the table ends in -1: never a hit
    if n0:
        table[:n0, :graph_old.shape[1]] = graph_old
    table[n0:, :K0] = knn_new
    fwd = np.full((b, M), -1, dtype=np.int32)
    pos_p, pos_j = np.arange(width), np.arange(K0)
    for v in range(b):
        L = knn_new[v]
        ok = (L >= 0) & (L < n1) & (L != n0 + v)
        lists = table[np.where(ok, L, 0)]                                            # [i, p]
        hit = (lists[:, :, None] == L[None, None, :]) & (pos_p[None, :, None] < pos_j[None, None, :])   # p < j
        route = hit.any(axis=1) & (pos_j[:, None] < pos_j[None, :]) & ok[:, None]                        # i < j
        det = route.sum(axis=0)
        order = sorted((int(det[j]), j) for j in range(K0) if ok[j])[:M]
        fwd[v, :len(order)] = [L[j] for _, j in order]
    return fwd


def incoming_ref(fwd_new: np.ndarray, n0: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(incoming_new [b, H], touched [t], incoming_old [t, H])``: for every target the sources ``n0 + v`` naming it
    among the first H entries of ``fwd_new[v]``, by (position, source), the first H."""
    b, M = fwd_new.shape
    h = M // 2
    found = {}
    for v in range(b):
        for pos in range(h):
            t = int(fwd_new[v, pos])
            if t >= 0:
                found.setdefault(t, []).append((pos, n0 + v))
    incoming_new = np.full((b, h), -1, dtype=np.int32)
    touched = np.array(sorted(t for t in found if t < n0), dtype=np.int32)
    incoming_old = np.full((touched.size, h), -1, dtype=np.int32)
    for t, named in found.items():
        best = [src for _, src in sorted(named)[:h]]
        if t >= n0:
            incoming_new[t - n0, :len(best)] = best
        else:
            incoming_old[int(np.searchsorted(touched, t)), :len(best)] = best
    return incoming_new, touched, incoming_old


def merge_rows_ref(fwd: np.ndarray, incoming: np.ndarray, row_base: int, n_total: int) -> np.ndarray:
    """``merge_ref`` for the rows ``[row_base, row_base + len(fwd))`` of an index of ``n_total`` rows."""
    n, M = fwd.shape
    h = M // 2
    out = np.full((n, M), -1, dtype=np.int32)
    for r in range(n):
        row = []
        for v in list(fwd[r, :h]) + list(incoming[r]) + list(fwd[r, h:]):
            v = int(v)
            if gc._valid(v, row_base + r, n_total) and v not in row:
                row.append(v)
        row = row[:M]
        out[r, :len(row)] = row
    return out


def _rank_key(score: np.float32, row: int):
    """Score descending, then lower id; a NaN score after every number."""
    s = float(score)
    return (1, 0.0, int(row)) if math.isnan(s) else (0, -s, int(row))


def link_row_ref(rows: np.ndarray, adjacency: np.ndarray, u: int, incoming: np.ndarray, n_total: int) -> np.ndarray:
    """The new ``graph[u]``: head = the first H valid entries, then the best of the pool by exact score."""
    M = adjacency.shape[0]
    h = M // 2
    adj = []
    for v in adjacency:
        v = int(v)
        if gc._valid(v, u, n_total) and v not in adj:
            adj.append(v)
    head, pool = adj[:h], adj[h:]
    for v in incoming:
        v = int(v)
        if gc._valid(v, u, n_total) and v not in adj and v not in pool:
            pool.append(v)
    out = np.full(M, -1, dtype=np.int32)
    out[:len(head)] = head
    if pool:
        scores = oracle.scores_fma(rows[u:u + 1], rows[pool])[0]
        best = sorted(range(len(pool)), key=lambda i: _rank_key(scores[i], pool[i]))[:M - len(head)]
        out[len(head):len(head) + len(best)] = [pool[i] for i in best]
    return out


def link_ref(rows: np.ndarray, graph: np.ndarray, n0: int, touched: np.ndarray, incoming_old: np.ndarray) -> np.ndarray:
    """A copy of ``graph`` (``[n1, M]``) with the rows ``touched`` relinked.  An entry of ``touched`` outside
    ``[0, n0)``, or not greater than the entry before it, leaves its row alone."""
    out = np.array(graph, dtype=np.int32, copy=True)
    n1 = graph.shape[0]
    for t, u in enumerate(touched):
        u = int(u)
        if u < 0 or u >= n0 or (t > 0 and int(touched[t - 1]) >= u):
            continue
        out[u] = link_row_ref(rows, graph[u], u, incoming_old[t], n1)
    return out


def entry_rows_after_insert_ref(entry_rows: np.ndarray, n0: int, b: int, M: int, n_entry: Optional[int] = None) -> np.ndarray:
    """The old entry rows, then ``e`` rows spread evenly over the new ones: ``e`` = one in M, or the share ``b / n0`` of
    a fixed ``n_entry``; at least one, at most ``b``."""
    e = math.ceil(b / M) if n_entry is None else math.ceil(b * n_entry / n0)
    e = min(b, max(1, e))
    return np.concatenate([np.asarray(entry_rows, np.int32), np.array([n0 + (i * b) // e for i in range(e)], dtype=np.int32)])


def insert_ref(corpus: np.ndarray, graph_old: np.ndarray, entry_rows: np.ndarray, K0: int, n_entry: Optional[int] = None
               ) -> SimpleNamespace:
    """The whole insertion of ``corpus[n0:]`` behind the ``n0 = len(graph_old)`` linked rows, every step kept."""
    n0, M = graph_old.shape
    b = corpus.shape[0] - n0
    r = SimpleNamespace()
    r.knn_new = knn_new_ref(corpus, n0, K0)
    r.fwd_new = insert_prune_ref(graph_old, r.knn_new, M)
    r.incoming_new, r.touched, r.incoming_old = incoming_ref(r.fwd_new, n0)
    r.new_rows = merge_rows_ref(r.fwd_new, r.incoming_new, n0, n0 + b)
    r.graph = link_ref(corpus, np.concatenate([np.asarray(graph_old, np.int32), r.new_rows]), n0, r.touched, r.incoming_old)
    r.entry_rows = entry_rows_after_insert_ref(entry_rows, n0, b, M, n_entry)
    return r
