"""Diversified search on the MI355X: Maximal Marginal Relevance over a first stage's candidates.

``search_grouped`` collapses chunks of one document where the caller has group keys, and ``near_duplicates`` ->
``remove_ids`` -> ``compact`` removes duplicates offline at one global threshold; ``DiverseIndex`` is the query-time
answer.  Any dense first stage of this package is searched at ``fetch_k``, and ONE ``sskd_mmr_select`` call picks ``k``
of those rows greedily by ``lambda * relevance - (1 - lambda) * (largest similarity to a row already picked)``
(Carbonell & Goldstein 1998), optionally dropping every candidate whose similarity to a picked row reaches
``dup_threshold``.  Similarities are the exact scan's fp32 chain over the stored rows, so the step is exact, reads
nothing but rows that are in HBM already and never synchronises with the host.

The rule (candidates, similarity, values, tie order, padding) is spelled out in ``include/sskd_amd.h`` ("Diversified
search") and DESIGN.md 27; ``tests/mmr_cases.py`` restates it bit for bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _native


@dataclass(frozen=True)
class Diversity:
    """Validated settings of the re-ranking.

    ``lambda_mult`` in ``[0, 1]`` weighs relevance against redundancy (1: the first stage's order, 0: redundancy
    alone); ``fetch_k`` candidates per query come from the first stage (a search for more than ``fetch_k`` results
    fetches that many); a candidate whose similarity to a selected row reaches ``dup_threshold`` is dropped (None: no
    cut-off)."""

    lambda_mult: float = 0.5
    fetch_k: int = 50
    dup_threshold: Optional[float] = None

    def __post_init__(self):
        lam = float(self.lambda_mult)
        if not 0.0 <= lam <= 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"lambda_mult={self.lambda_mult!r} outside [0, 1]")
        object.__setattr__(self, "lambda_mult", lam)
        v = self.fetch_k
        if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= _native.SSKD_K_MAX:
            raise ValueError(f"fetch_k={v!r} outside [1, {_native.SSKD_K_MAX}]")
        object.__setattr__(self, "fetch_k", int(v))
        if self.dup_threshold is not None:
            t = float(self.dup_threshold)
            if math.isnan(t):
                raise ValueError("dup_threshold is NaN")
            object.__setattr__(self, "dup_threshold", t)

    def threshold(self) -> float:
        """What the kernel takes: ``+inf`` switches the cut-off off."""
        return math.inf if self.dup_threshold is None else self.dup_threshold

    def depth(self, k: int) -> int:
        """How many candidates a search for ``k`` results fetches: ``min(max(fetch_k, k), SSKD_K_MAX)``."""
        return min(max(self.fetch_k, int(k)), _native.SSKD_K_MAX)


def mmr_device(flat, rank_scores, rank_ids, k: int, diversity: Diversity, id_offset: int = 0):
    """ONE ``sskd_mmr_select`` over ``flat``'s rows: the ranking fp32 / int64 ``[nq, fetch_k]`` in LOCAL rows, padded
    with id -1.  Returns ``(D fp32 [nq, k], I int64 [nq, k] = row + id_offset, mmr fp64 [nq, k], red fp32 [nq, k],
    counts int32 [nq])`` device tensors in selection order, padded with ``(-FLT_MAX, -1, -inf, NaN)``."""
    import torch

    if rank_ids.dim() != 2 or rank_scores.shape != rank_ids.shape:
        raise ValueError(f"expected a ranking [nq, fetch_k], got scores {tuple(rank_scores.shape)} and ids "
                         f"{tuple(rank_ids.shape)}")
    if rank_scores.dtype != torch.float32 or rank_ids.dtype != torch.int64:
        raise TypeError("mmr_device expects float32 scores and int64 ids")
    rank_scores, rank_ids = rank_scores.contiguous(), rank_ids.contiguous()
    nq, fetch_k = rank_ids.shape
    dev = rank_ids.device
    D = torch.empty((nq, k), dtype=torch.float32, device=dev)
    I = torch.empty((nq, k), dtype=torch.int64, device=dev)
    mmr = torch.empty((nq, k), dtype=torch.float64, device=dev)
    red = torch.empty((nq, k), dtype=torch.float32, device=dev)
    counts = torch.empty(nq, dtype=torch.int32, device=dev)
    _native.check(_native.load().sskd_mmr_select(
        0 if flat._tiled is None else flat._tiled.data_ptr(), int(flat.ntotal), rank_scores.data_ptr(),
        rank_ids.data_ptr(), nq, fetch_k, diversity.lambda_mult, diversity.threshold(), int(k), int(id_offset),
        D.data_ptr(), I.data_ptr(), mmr.data_ptr(), red.data_ptr(), counts.data_ptr(), _native.current_stream_ptr(dev)))
    return D, I, mmr, red, counts


class DiverseIndex:
    """``first`` behind an MMR re-ranking of its own candidates.

    ``first`` is a ``FAISSIndexBuilder``, ``IVFIndex``, ``IVFPQIndex``, ``GraphIndex`` or an ``ExpandedIndex`` over one
    of them; the rows the similarities read are ``first``'s own or ``first.flat``'s.  A ``BM25Index`` or a
    ``HybridIndex`` (bare or expanded) is refused: their fp64 BM25 / fused scores are not cosine relevance, and the rule
    weighs relevance against a cosine."""

    def __init__(self, first, diversity: Optional[Diversity] = None):
        from .bm25 import BM25Index
        from .expand import ExpandedIndex
        from .hybrid import HybridIndex
        from .index import FAISSIndexBuilder

        self.first = first
        self.diversity = Diversity() if diversity is None else diversity
        if not isinstance(self.diversity, Diversity):
            raise TypeError("diversity must be a Diversity")
        inner = first.first if isinstance(first, ExpandedIndex) else first
        if isinstance(inner, (BM25Index, HybridIndex)):
            raise TypeError(f"DiverseIndex does not take a {type(inner).__name__}: its fp64 BM25 / fused scores are not "
                            "cosine relevance, which the MMR value weighs against a cosine similarity")
        flat = first if isinstance(first, FAISSIndexBuilder) else getattr(first, "flat", None)
        if not isinstance(flat, FAISSIndexBuilder):
            raise TypeError(f"{type(first).__name__} is no first stage DiverseIndex knows: expected a dense index, an "
                            "overlay with .flat, or an ExpandedIndex over one of them")
        self.flat = flat
        self._rows = first if hasattr(first, "remove_ids") else flat   # who answers ntotal / doc_ids / remove_ids

    ntotal = property(lambda self: self._rows.ntotal)
    doc_ids = property(lambda self: self._rows.doc_ids)
    doc_texts = property(lambda self: self._rows.doc_texts)

    def remove_ids(self, ids) -> int:
        return self._rows.remove_ids(ids)

    def _select(self, queries, k: int, kw):
        import torch

        if not isinstance(queries, torch.Tensor):
            raise TypeError("DiverseIndex.search_device expects a float32 device tensor (search() takes NumPy)")
        k = int(k)
        if not 1 <= k <= _native.SSKD_K_MAX:
            raise ValueError(f"k={k} outside [1, {_native.SSKD_K_MAX}]")
        with torch.cuda.device(self.flat.device):
            scores, ids = self.first.search_device(queries, self.diversity.depth(k), **kw)[:2]
            off = int(self.flat.id_offset)
            if off:
                ids = torch.where(ids < 0, ids, ids - off)
            return mmr_device(self.flat, scores, ids, k, self.diversity, id_offset=off)

    def search_detailed_device(self, queries, k: int, **kw):
        """``search_device`` plus the selection's own figures: ``(D, I, mmr fp64 [nq, k], red fp32 [nq, k], counts int32
        [nq])`` device tensors."""
        return self._select(queries, k, kw)

    def search_device(self, queries, k: int, **kw):
        """``(D fp32 [nq, k], I int64 [nq, k])`` device tensors in selection order: the first stage's scores and ids
        (``flat.id_offset`` applied) of the rows MMR picked among its ``min(max(fetch_k, k), SSKD_K_MAX)`` best,
        padded with ``(-FLT_MAX, -1)``.  Keyword arguments (``allow``, ``nprobe``, ``ef``, ``refine``, ...) go to
        ``first.search_device``.  Nothing is synchronised on the way."""
        return self._select(queries, k, kw)[:2]

    def _host(self, query_emb, k: int, kw):
        import torch

        from .index import _host_queries_to_device

        emb = np.asarray(query_emb, dtype=np.float32)
        if not np.isfinite(emb).all():
            raise ValueError("query embeddings must be finite (NaN or infinity found)")
        out = self._select(_host_queries_to_device(emb, self.flat.device), k, kw)
        torch.cuda.synchronize(out[0].device)
        return tuple(t.cpu().numpy() for t in out)

    def search(self, query_emb, k: int = 10, **kw):
        """``search_device`` in ``FAISSIndexBuilder.search``'s NumPy form (``[nq, 384]`` or one ``[384]`` vector)."""
        return self._host(query_emb, k, kw)[:2]

    def search_detailed(self, query_emb, k: int = 10, **kw):
        """``search`` plus ``mmr``, ``red`` and ``counts`` as NumPy arrays."""
        return self._host(query_emb, k, kw)
