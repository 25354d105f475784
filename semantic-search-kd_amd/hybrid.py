"""Hybrid retrieval on the MI355X: a dense ranking and a BM25 ranking of the same rows fused on the device.

The reference's service contract names the join (reference: configs/service.yaml:43-49, ``hybrid.bm25_weight``,
``hybrid.semantic_weight``, ``hybrid.fusion_method: rrf | linear``) and has no code behind it.  ``HybridIndex`` puts
one ``FAISSIndexBuilder`` and one ``BM25Index`` over the same corpus behind one search: a dense ``search_device``, a
``BM25Index`` search and ONE ``sskd_hybrid_fuse`` call, all stream-ordered on the device.  The rule (candidates, ranks,
``rrf`` and ``linear`` with completed scores, tie order) is spelled out in ``include/sskd_amd.h`` ("Hybrid fusion") and
DESIGN.md 16.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import _native
from . import bm25 as _bm25

FUSION_METHODS = {"rrf": 0, "linear": 1}


def _method_code(name: str) -> int:
    try:
        return FUSION_METHODS[str(name).lower()]
    except KeyError:
        raise ValueError(f"fusion_method={name!r}: expected one of {sorted(FUSION_METHODS)}") from None


def _weight(name: str, value) -> float:
    w = float(value)
    if not (0.0 <= w < float("inf")):
        raise ValueError(f"{name}={value!r} must be finite and >= 0")
    return w


class HybridIndex:
    """One search over a dense index and a BM25 index that describe the same rows.

    ``semantic_weight`` / ``bm25_weight`` / ``fusion_method`` carry the reference's defaults (0.7 / 0.3 / ``"rrf"``);
    ``rrf_k`` is the constant of reciprocal rank fusion; ``depth`` is how many rows each side contributes per query.
    The two indexes must number the same rows: equal row counts, and equal ``doc_ids`` in order when both carry them.
    A dense index that was ``compact()``ed after the BM25 index was built no longer matches - the BM25 index must be
    rebuilt after ``compact()``.

    One device, one dense index: a row-sharded ``ShardedIndex`` is not supported (hybrid retrieval over shards would
    need the union across ranks)."""

    def __init__(self, dense, bm25, *, semantic_weight: float = 0.7, bm25_weight: float = 0.3,
                 fusion_method: str = "rrf", rrf_k: float = 60.0, depth: int = 100):
        self.dense = dense
        self.bm25 = bm25
        self.semantic_weight = _weight("semantic_weight", semantic_weight)
        self.bm25_weight = _weight("bm25_weight", bm25_weight)
        _method_code(fusion_method)
        self.fusion_method = str(fusion_method).lower()
        self.rrf_k = float(rrf_k)
        if not (0.0 < self.rrf_k < float("inf")):
            raise ValueError(f"rrf_k={rrf_k!r} must be finite and > 0")
        self.depth = int(depth)
        if self.depth < 1:
            raise ValueError(f"depth={depth} < 1")
        self.check_same_rows()

    def check_same_rows(self) -> None:
        """Raises ``ValueError`` unless both indexes describe the same rows (run by the constructor and by every
        search: ``compact()`` or ``add`` on the dense index after construction breaks the match)."""
        hint = "the BM25 index must be rebuilt after compact() (or any other change of the dense index's rows)"
        post = getattr(self.bm25, "bm25", None)
        if post is None:
            raise ValueError("the BM25 index is not loaded: call load() or build_from_texts() first")
        n_dense, n_bm25 = int(self.dense.ntotal), int(post.corpus_size)
        if n_dense != n_bm25:
            raise ValueError(f"the dense index holds {n_dense} rows, the BM25 index {n_bm25}: {hint}")
        a, b = list(self.dense.doc_ids or []), list(self.bm25.doc_ids or [])
        if a and b and a != b:
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            raise ValueError(f"the two indexes' doc_ids differ (first at row {at}): {hint}")

    def clip_depth(self, depth: Optional[int] = None) -> int:
        """``min(depth, rows, K_MAX)``: what each side contributes per query (at least 1)."""
        depth = self.depth if depth is None else int(depth)
        if depth < 1:
            raise ValueError(f"depth={depth} < 1")
        return max(1, min(depth, int(self.dense.ntotal), _bm25.K_MAX))

    def search_device(self, queries: Sequence[str], query_emb, k: int = 10, *, allow=None, depth: Optional[int] = None,
                      fusion_method: Optional[str] = None, semantic_weight: Optional[float] = None,
                      bm25_weight: Optional[float] = None, details: bool = False, query_csr=None):
        """``(D float64 [nq, k], I int64 [nq, k])`` device tensors: the best ``k`` rows of the union of both sides'
        ``depth`` best, by fused score descending then lower row, ids as the dense index's ``search`` numbers them,
        padded with ``(-inf, -1)``.  ``queries`` are the texts (BM25 side), ``query_emb`` their ``[nq, 384]`` float32
        device embeddings (dense side; normalised here when the metric is cosine).  ``details=True`` also returns
        ``dense_scores float32 [nq, k]``, ``bm25_scores float64 [nq, k]`` (each result's two component scores; under
        ``rrf`` a side the row was absent from is NaN, ``linear`` completes both) and ``counts int32 [nq]`` (the
        union's size before the cut).

        Three device calls on the current stream and no host synchronisation (``allow`` should then be a prepared
        ``RowFilter``).  The query embeddings must be finite: this entry point does not check that (``search`` does).

        ``allow`` and the dense index's removed rows are honoured by both sides: the dense search applies them as
        always, the BM25 ranking is filtered inside the fuse kernel by the same mask and ranked among the survivors.
        Because that filter comes after the BM25 retrieval, fewer than ``depth`` lexical candidates may survive it.
        ``depth`` is clipped to ``min(depth, rows, 256)``; ``k`` above twice that raises ``ValueError``.

        ``query_csr``: the BM25 side's queries already as a device CSR ``(lims int64 [nq + 1], terms int32)`` in
        ``BM25Index.query_csr``'s form (an expanded query, ``expand.ExpandedIndex``); the texts are then not
        tokenised.  The dense side takes whatever embeddings it is given, so an expanded embedding needs no keyword."""
        import torch

        self.check_same_rows()
        dense, bm25 = self.dense, self.bm25
        method = _method_code(self.fusion_method if fusion_method is None else fusion_method)
        ws = self.semantic_weight if semantic_weight is None else _weight("semantic_weight", semantic_weight)
        wb = self.bm25_weight if bm25_weight is None else _weight("bm25_weight", bm25_weight)
        d = self.clip_depth(depth)
        k = int(k)
        if not 1 <= k <= 2 * d:
            raise ValueError(f"k={k} outside [1, 2 * depth = {2 * d}]")
        if not isinstance(query_emb, torch.Tensor):
            raise TypeError("HybridIndex.search_device expects a float32 device tensor (search() takes NumPy)")
        q = dense._prepare_queries(query_emb, None, "HybridIndex.search_device")
        nq = q.shape[0]
        if len(queries) != nq:
            raise ValueError(f"{len(queries)} query texts for {nq} query embeddings")
        dev, offsets, post_rows, post_w, idf = bm25._tables()
        if dev != dense.device:
            raise ValueError(f"the dense index lives on {dense.device}, the BM25 index on {dev}")
        lib = _native.load()
        fused = torch.empty((nq, k), dtype=torch.float64, device=dev)
        ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        counts = torch.empty(nq, dtype=torch.int32, device=dev)
        dense_scores = torch.empty((nq, k), dtype=torch.float32, device=dev) if details else None
        bm25_scores = torch.empty((nq, k), dtype=torch.float64, device=dev) if details else None
        if nq:
            with torch.cuda.device(dev):
                mask = dense.search_mask(allow)
                # both rankings in LOCAL rows; the prepared query is what the linear completion scores against
                rank_s, rank_i = dense._search_device_masked(q, d, False, None, None, mask, id_offset=0)
                csr = bm25.query_csr(queries) if query_csr is None else query_csr
                rank_b, rank_j = bm25._search_csr(csr, nq, d)
                n_rows = int(dense.ntotal)
                _native.check(
                    lib.sskd_hybrid_fuse(
                        dense._tiled.data_ptr(), n_rows, q.data_ptr(), rank_s.data_ptr(), rank_i.data_ptr(), d,
                        offsets.data_ptr(), post_rows.data_ptr(), post_w.data_ptr(), idf.data_ptr(), bm25.bm25.n_terms,
                        csr[0].data_ptr(), csr[1].data_ptr(), rank_b.data_ptr(), rank_j.data_ptr(), d,
                        None if mask is None else mask.data_ptr(), method, ws, wb, self.rrf_k, nq, k,
                        int(dense.id_offset), fused.data_ptr(), ids.data_ptr(), counts.data_ptr(),
                        None if dense_scores is None else dense_scores.data_ptr(),
                        None if bm25_scores is None else bm25_scores.data_ptr(), _native.current_stream_ptr(dev),
                    )
                )
        if details:
            return fused, ids, dense_scores, bm25_scores, counts
        return fused, ids

    def search(self, queries: Sequence[str], query_emb, k: int = 10, **kwargs):
        """``search_device`` for host embeddings (NumPy ``[nq, 384]`` or one ``[384]`` vector with one text): NumPy
        results.  A non-finite embedding raises ``ValueError`` (the fusion's arithmetic is defined for finite
        scores)."""
        import torch

        from .index import _host_queries_to_device

        if isinstance(queries, str):
            queries = [queries]
        emb = np.asarray(query_emb, dtype=np.float32)
        if emb.ndim == 1:
            emb = emb[None, :]
        if not np.isfinite(emb).all():
            raise ValueError("query embeddings must be finite (NaN or infinity found)")
        qd = _host_queries_to_device(np.ascontiguousarray(emb), self.dense.device)
        with torch.cuda.device(self.dense.device):
            out = self.search_device(queries, qd, k, **kwargs)
            return tuple(t.cpu().numpy() for t in out)
