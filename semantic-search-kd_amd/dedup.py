"""Near-duplicate clusters: the result type of ``FAISSIndexBuilder.duplicate_clusters`` / ``deduplicate`` and the host
form of the clustering rule.

A cluster is a connected component (single linkage) of the graph whose edges are the pairs ``near_duplicates`` returns.
The device path (``csrc/dedup.hip``: ``sskd_dup_init`` / ``sskd_dup_link`` / ``sskd_dup_labels``) never builds the pair
list; ``cluster_pairs`` is the same rule over a pair list on the host, for small inputs and as the statement the device
path is tested against - the pattern of ``ndcg_at_k`` and ``text_overlap`` beside their device forms.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

KEEP = {"first": 0, "densest": 1}
SCOPE = {"all": 0, "across_groups": 1, "within_groups": 2}


def keep_code(keep: str) -> int:
    """``sskd_dup_labels``' code of a ``keep`` rule; raises ``ValueError`` for an unknown one."""
    if keep not in KEEP:
        raise ValueError(f"keep={keep!r}: one of {sorted(KEEP)}")
    return KEEP[keep]


def scope_code(scope: str) -> int:
    """``sskd_dup_link``'s code of a ``scope`` rule; raises ``ValueError`` for an unknown one."""
    if scope not in SCOPE:
        raise ValueError(f"scope={scope!r}: one of {sorted(SCOPE)}")
    return SCOPE[scope]


@dataclass
class DuplicateClusters:
    """Clusters of near-duplicate rows.  Ids are in the space ``search`` returns (``id_offset + row``).

    ``labels`` int64 ``[n]``: the id of the smallest row of each row's cluster, -1 for removed rows and rows outside
    ``allow``; ``representatives`` int64 ``[n_clusters]``, ascending by label: the row each cluster keeps; ``sizes`` int64
    ``[n_clusters]``; ``n_rows``: the rows taking part; ``id_offset``: the id of row 0.  ``deduplicate`` adds ``removed``
    (the ids it dropped, ascending) and, with ``compact=True``, ``kept`` (what ``compact()`` returned)."""

    labels: np.ndarray
    representatives: np.ndarray
    sizes: np.ndarray
    n_clusters: int
    n_rows: int
    id_offset: int = 0
    removed: Optional[np.ndarray] = None
    kept: Optional[np.ndarray] = None

    def cluster_labels(self) -> np.ndarray:
        """The label of every cluster, ascending (``representatives`` and ``sizes`` are in this order)."""
        return np.unique(self.labels[self.labels >= 0])

    def representative_of_rows(self) -> np.ndarray:
        """int64 ``[n]``: the id of the row kept for each row's cluster, -1 where ``labels`` is -1."""
        out = np.full(self.labels.shape, -1, dtype=np.int64)
        inside = self.labels >= 0
        out[inside] = self.representatives[np.searchsorted(self.cluster_labels(), self.labels[inside])]
        return out

    def duplicates(self) -> np.ndarray:
        """The ids of the rows taking part that are not the row their cluster keeps, ascending (int64)."""
        rep = self.representative_of_rows()
        ids = np.arange(self.labels.size, dtype=np.int64) + self.id_offset
        return ids[(self.labels >= 0) & (rep != ids)]


def clusters_from_arrays(parent: np.ndarray, rep: np.ndarray, size: np.ndarray, id_offset: int) -> DuplicateClusters:
    """The result type from ``sskd_dup_labels``' outputs (host copies): the flat ``parent``, ``rep`` and ``size`` per row."""
    parent = np.asarray(parent, dtype=np.int64)
    roots = np.flatnonzero(np.asarray(size) > 0)
    labels = np.where(parent >= 0, parent + id_offset, -1).astype(np.int64)
    return DuplicateClusters(
        labels=labels,
        representatives=np.asarray(rep, dtype=np.int64)[roots] + id_offset,
        sizes=np.asarray(size, dtype=np.int64)[roots],
        n_clusters=int(roots.size),
        n_rows=int((parent >= 0).sum()),
        id_offset=int(id_offset),
    )


def cluster_pairs(pairs, n: int, *, keep: str = "first", scope: str = "all", groups=None, allow=None,
                  id_offset: int = 0) -> DuplicateClusters:
    """The clusters of ``n`` rows under a pair list (``near_duplicates``' ``pairs``: ids, int ``[m, 2]``), on the host.

    A pair is an edge when both ids lie in ``[id_offset, id_offset + n)``, differ, both rows are allowed (``allow``: a
    bool array over the rows, None = all) and the ``scope`` rule over ``groups`` (one number per row) holds: ``"all"``,
    ``"across_groups"`` (different groups only) or ``"within_groups"`` (the same group only).  A pair listed twice counts
    twice in a row's degree.  ``keep="first"`` keeps each cluster's smallest row, ``"densest"`` its row with the most
    edges, ties to the smallest row."""
    keep_c, scope_c = keep_code(keep), scope_code(scope)
    n = int(n)
    if n < 0:
        raise ValueError(f"n={n} < 0")
    if scope_c and groups is None:
        raise ValueError(f"scope={scope!r} needs groups")
    take = np.ones(n, dtype=np.bool_) if allow is None else np.asarray(allow, dtype=np.bool_)
    if take.shape != (n,):
        raise ValueError(f"allow needs one entry per row: shape {take.shape} for {n} rows")
    g = None if groups is None else np.asarray(groups).reshape(-1)
    if g is not None and g.size != n:
        raise ValueError(f"{g.size} groups for {n} rows")
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2) - int(id_offset)
    parent = np.arange(n, dtype=np.int64)
    degree = np.zeros(n, dtype=np.int64)

    def find(x: int) -> int:
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = int(parent[x])
        return x

    for a, b in p.tolist():
        if a == b or not (0 <= a < n and 0 <= b < n) or not (take[a] and take[b]):
            continue
        if scope_c and ((scope_c == 1) == bool(g[a] == g[b])):
            continue
        degree[a] += 1
        degree[b] += 1
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)   # the larger root under the smaller: a root is its tree's smallest row
    flat = np.array([find(r) if take[r] else -1 for r in range(n)], dtype=np.int64)
    size = np.bincount(flat[flat >= 0], minlength=n)[:n] if n else np.zeros(0, dtype=np.int64)
    rep = flat.copy()
    if keep_c:
        best = {}
        for r in np.flatnonzero(flat >= 0).tolist():
            root = int(flat[r])
            cur = best.get(root)
            if cur is None or degree[r] > degree[cur]:   # rows ascend: a tie keeps the smaller row
                best[root] = r
        rep = np.array([best[int(f)] if f >= 0 else -1 for f in flat], dtype=np.int64)
    return clusters_from_arrays(flat, rep, size, int(id_offset))
