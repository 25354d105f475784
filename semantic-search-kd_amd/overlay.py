"""Shared by the indexes over an unchanged flat index: ``FlatOverlay``, ``recall_at_k``, the ``*.json`` version check."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

from .index import FAISSIndexBuilder


def read_versioned_json(path: Path, version: int) -> dict:
    """The object in ``path``; ``ValueError`` unless its ``format_version`` is ``version``."""
    meta = json.loads(path.read_text())
    if int(meta.get("format_version", -1)) != version:
        raise ValueError(f"{path}: format version {meta.get('format_version')!r}, this build reads {version}")
    return meta


def recall_at_k(found: np.ndarray, truth: np.ndarray) -> float:
    """Mean over the queries of |found ids AND true ids| / |true ids| (-1 padding ignored; a query without true ids
    counts as 1.0)."""
    total = 0.0
    for f, t in zip(np.asarray(found), np.asarray(truth)):
        t = t[t >= 0]
        total += 1.0 if t.size == 0 else np.intersect1d(f[f >= 0], t).size / t.size
    return total / max(len(truth), 1)


class FlatOverlay:
    """A search structure over a ``FAISSIndexBuilder`` whose rows it neither permutes nor copies: ``self.flat`` holds
    the rows, and everything keyed by row id is the flat index's.  A subclass provides ``search``."""

    def __init__(self, flat: FAISSIndexBuilder) -> None:
        self.flat = flat
        self.device = flat.device
        self.embedding_dim = flat.embedding_dim

    ntotal = property(lambda self: self.flat.ntotal)
    doc_ids = property(lambda self: self.flat.doc_ids)
    doc_texts = property(lambda self: self.flat.doc_texts)
    index = property(lambda self: self.flat.index)   # the flat index's IndexHandle (or None)

    def _rows_view(self) -> torch.Tensor:
        """The flat index's rows as a ``[ntotal, dim]`` device view (the layout is plain row-major)."""
        n = self.flat.ntotal
        return self.flat._tiled[: n * self.embedding_dim].view(n, self.embedding_dim)

    def remove_ids(self, ids) -> int:
        """The flat index's tombstones: they reach the search through ``flat.search_mask`` (the graph search still
        traverses a removed row, and never returns it)."""
        return self.flat.remove_ids(ids)

    def validate(self, num_queries: int = 1000, k: int = 10, seed: int = 0, **search_args) -> float:
        """recall@k of ``search`` against ``flat.search`` (the reference's ``validation:`` block: ``num_queries``
        1000, ``brute_force_top_k`` 10), the queries being ``num_queries`` distinct rows of the index."""
        n = self.flat.ntotal
        if n < 1:
            raise RuntimeError("validate(): the index is empty")
        pick = np.sort(np.random.default_rng(seed).permutation(n)[: min(int(num_queries), n)])
        with torch.cuda.device(self.device):
            q = self._rows_view()[torch.from_numpy(pick).to(self.device)].cpu().numpy()
        _, found = self.search(q, k, **search_args)
        _, truth = self.flat.search(q, k)
        return recall_at_k(found, truth)
