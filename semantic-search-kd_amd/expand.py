"""Query expansion on the MI355X: pseudo-relevance feedback between a first search and a second one.

The reference's service contract names the feature (reference: configs/service.yaml:108-113,
``features.enable_query_expansion``; ``.env.example``: ``ENABLE_QUERY_EXPANSION``) and has no code behind it.
``ExpandedIndex`` puts any first stage of this package behind "search once, build a better query, search again", with
the step in between on the device and no host synchronisation:

* a dense stage (``FAISSIndexBuilder``, ``IVFIndex``, ``IVFPQIndex``, ``GraphIndex``) is searched at ``fb_docs``, ONE
  ``sskd_prf_rocchio`` call turns the prepared query and its best rows into ``alpha q + sum b_i row_i``, and the stage's
  own search runs on the new queries;
* a ``BM25Index`` is searched at ``fb_docs``, ONE ``sskd_prf_rm3`` call picks the ``fb_terms`` heaviest words of the
  feedback rows from the forward index and writes the expanded query CSR, which the BM25 search then scores;
* a ``HybridIndex`` gets both: the dense side is expanded from the dense ranking, the BM25 side from the BM25 ranking,
  each under the mask the search honours, then one fuse as always.

Both rules (feedback rows, weights, sums, tie order) are spelled out in ``include/sskd_amd.h`` ("Query expansion") and
DESIGN.md 25; ``tests/expand_cases.py`` restates them bit for bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native
from . import bm25 as _bm25

WEIGHTINGS = {"uniform": 0, "score": 1}
RM3_FB_DOCS_MAX = 16
RM3_FB_TERMS_MAX = 64
RM3_ORIG_REPEAT_MAX = 8


@dataclass(frozen=True)
class QueryExpansion:
    """Validated settings of both expansion rules.

    ``fb_docs`` feedback rows per query (both sides; the lexical side takes at most 16).  Dense side: ``alpha`` /
    ``beta`` weigh the query and the feedback rows, ``weighting`` is ``"uniform"`` (``beta / m`` each) or ``"score"``
    (``beta`` shared in proportion to the positive scores), ``rounds`` repeats search-and-expand on the host.  Lexical
    side: ``fb_terms`` words are appended behind ``orig_repeat`` copies of the query's own tokens; a word that occurs in
    more than ``floor(max_df_fraction * rows)`` rows is no expansion word (0 = no limit)."""

    fb_docs: int = 5
    alpha: float = 1.0
    beta: float = 0.75
    weighting: str = "uniform"
    rounds: int = 1
    fb_terms: int = 10
    orig_repeat: int = 2
    max_df_fraction: float = 0.25

    def __post_init__(self):
        def whole(name, lo, hi):
            v = getattr(self, name)
            if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
                raise ValueError(f"{name}={v!r} outside [{lo}, {hi}]")
            object.__setattr__(self, name, int(v))

        def weight(name):
            v = float(getattr(self, name))
            if not 0.0 <= v <= float(np.finfo(np.float32).max):   # (the kernel takes fp32)
                raise ValueError(f"{name}={getattr(self, name)!r} must be finite and >= 0")
            object.__setattr__(self, name, v)

        whole("fb_docs", 1, _native.SSKD_K_MAX)
        whole("rounds", 1, 16)
        whole("fb_terms", 1, RM3_FB_TERMS_MAX)
        whole("orig_repeat", 1, RM3_ORIG_REPEAT_MAX)
        weight("alpha")
        weight("beta")
        w = str(self.weighting).lower()
        if w not in WEIGHTINGS:
            raise ValueError(f"weighting={self.weighting!r}: expected one of {sorted(WEIGHTINGS)}")
        object.__setattr__(self, "weighting", w)
        f = float(self.max_df_fraction)
        if not 0.0 <= f <= 1.0:
            raise ValueError(f"max_df_fraction={self.max_df_fraction!r} outside [0, 1]")
        object.__setattr__(self, "max_df_fraction", f)

    def max_df(self, rows: int) -> int:
        """``floor(max_df_fraction * rows)``; 0 switches the limit off."""
        return int(math.floor(self.max_df_fraction * int(rows)))

    def lexical_fb_docs(self) -> int:
        if self.fb_docs > RM3_FB_DOCS_MAX:
            raise ValueError(f"fb_docs={self.fb_docs} > {RM3_FB_DOCS_MAX}: the lexical side reads at most "
                             f"{RM3_FB_DOCS_MAX} feedback rows")
        return self.fb_docs


def expanded_lims(q_lims: np.ndarray, orig_repeat: int, fb_terms: int) -> np.ndarray:
    """The layout of the expanded query CSR: int64 ``[nq + 1]`` from 0, segment ``q`` of ``orig_repeat * len_q +
    fb_terms`` slots."""
    q_lims = np.asarray(q_lims, dtype=np.int64)
    out = np.zeros(q_lims.size, dtype=np.int64)
    np.cumsum(np.diff(q_lims) * int(orig_repeat) + int(fb_terms), out=out[1:])
    return out


def rocchio_device(flat, q, rank_scores, rank_ids, expansion: QueryExpansion):
    """ONE ``sskd_prf_rocchio``: ``q`` the PREPARED queries ``[nq, 384]``, the ranking in LOCAL rows ``[nq, kd]``.
    Returns ``(new queries fp32 [nq, 384] - not normalised -, counts int32 [nq])`` device tensors."""
    import torch

    nq, kd = rank_ids.shape
    out = torch.empty_like(q)
    counts = torch.empty(nq, dtype=torch.int32, device=q.device)
    _native.check(_native.load().sskd_prf_rocchio(
        0 if flat._tiled is None else flat._tiled.data_ptr(), int(flat.ntotal), q.data_ptr(), nq, rank_scores.data_ptr(),
        rank_ids.data_ptr(), kd, min(expansion.fb_docs, kd), expansion.alpha, expansion.beta,
        WEIGHTINGS[expansion.weighting], out.data_ptr(), counts.data_ptr(), _native.current_stream_ptr(q.device)))
    return out, counts


def rm3_device(bm25, csr, q_lims_host: np.ndarray, rank_scores, rank_ids, expansion: QueryExpansion, mask=None):
    """ONE ``sskd_prf_rm3`` over ``bm25``'s forward index (uploaded at the first call): ``csr`` the queries' device CSR,
    ``q_lims_host`` its lims on the host, the ranking fp64 / int64 ``[nq, kb]`` as ``BM25Index.search_device`` writes
    it, ``mask`` allow-mask words or None.  Returns ``((out_lims, out_terms), sel_terms int32 [nq, fb_terms], sel_w fp64
    [nq, fb_terms], counts int32 [nq], fb int32 [nq])`` device tensors; the first is a query CSR for
    ``BM25Index._search_csr`` and ``HybridIndex.search_device(query_csr=...)``."""
    import torch

    post = bm25._require_built()
    dev, offsets, _, _, _ = bm25._tables()
    fwd_lims, fwd_terms, fwd_p, n_fwd = bm25.forward_tables()
    nq, kb = rank_ids.shape
    fb_docs = min(expansion.lexical_fb_docs(), kb)
    q_lims_host = np.ascontiguousarray(q_lims_host, dtype=np.int64)
    out_lims = expanded_lims(q_lims_host, expansion.orig_repeat, expansion.fb_terms)
    d_out_lims = torch.from_numpy(out_lims).to(dev)
    out_terms = torch.empty(max(int(out_lims[-1]), 1), dtype=torch.int32, device=dev)
    sel_terms = torch.empty((nq, expansion.fb_terms), dtype=torch.int32, device=dev)
    sel_w = torch.empty((nq, expansion.fb_terms), dtype=torch.float64, device=dev)
    counts = torch.empty(nq, dtype=torch.int32, device=dev)
    fb = torch.empty(nq, dtype=torch.int32, device=dev)
    _native.check(_native.load().sskd_prf_rm3(
        fwd_lims.data_ptr(), fwd_terms.data_ptr(), fwd_p.data_ptr(), n_fwd, offsets.data_ptr(), post.corpus_size,
        post.n_terms, q_lims_host.ctypes.data, csr[0].data_ptr(), csr[1].data_ptr(), rank_scores.data_ptr(),
        rank_ids.data_ptr(), kb, None if mask is None else mask.data_ptr(), nq, fb_docs, expansion.fb_terms,
        expansion.orig_repeat, expansion.max_df(post.corpus_size), out_lims.ctypes.data, d_out_lims.data_ptr(),
        out_terms.data_ptr(), sel_terms.data_ptr(), sel_w.data_ptr(), counts.data_ptr(), fb.data_ptr(),
        _native.current_stream_ptr(dev)))
    return (d_out_lims, out_terms), sel_terms, sel_w, counts, fb


class ExpandedIndex:
    """``first`` behind one round trip of pseudo-relevance feedback.

    ``first`` is a ``FAISSIndexBuilder``, ``IVFIndex``, ``IVFPQIndex``, ``GraphIndex``, ``BM25Index`` or
    ``HybridIndex``; the flat rows the dense rule reads are ``first``'s own or ``first.flat``'s.  ``search_device``
    takes what ``first.search_device`` takes (queries for a dense stage, texts for BM25, texts plus embeddings for
    hybrid; the stage's keyword arguments pass through to both of its searches) and returns what it returns - for the
    expanded query."""

    def __init__(self, first, expansion: Optional[QueryExpansion] = None):
        from .hybrid import HybridIndex
        from .index import FAISSIndexBuilder

        self.first = first
        self.expansion = QueryExpansion() if expansion is None else expansion
        if not isinstance(self.expansion, QueryExpansion):
            raise TypeError("expansion must be a QueryExpansion")
        if isinstance(first, HybridIndex):
            self.kind, self.flat, self.bm25 = "hybrid", first.dense, first.bm25
        elif isinstance(first, _bm25.BM25Index):
            self.kind, self.flat, self.bm25 = "bm25", None, first
        else:
            flat = first if isinstance(first, FAISSIndexBuilder) else getattr(first, "flat", None)
            if not isinstance(flat, FAISSIndexBuilder):
                raise TypeError(f"{type(first).__name__} is no first stage ExpandedIndex knows: expected a dense index "
                                "(or an overlay with .flat), a BM25Index or a HybridIndex")
            self.kind, self.flat, self.bm25 = "dense", flat, None
        if self.kind != "dense":
            self.expansion.lexical_fb_docs()

    # ------------------------------------------------------------------ dense side
    def _first_dense(self, q, k: int, kw):
        """The first stage's own search on PREPARED queries, ids in LOCAL rows."""
        import torch

        if self.kind == "hybrid":
            mask = self.flat.search_mask(kw.get("allow"))
            return self.flat._search_device_masked(q, k, False, None, None, mask, id_offset=0)
        scores, ids = self.first.search_device(q, k, normalize_queries=False, **kw)[:2]
        off = int(self.flat.id_offset)
        if off:
            ids = torch.where(ids < 0, ids, ids - off)
        return scores, ids

    def expand_queries_device(self, queries, **kw):
        """ONE round of the dense rule: ``queries`` float32 device ``[nq, 384]`` as the first stage takes them; returns
        ``(expanded queries, counts int32 [nq])``.  The expanded queries are not normalised: a search prepares them as
        it prepares any query."""
        if self.kind == "bm25":
            raise TypeError("a BM25 index has no dense side")
        flat, x = self.flat, self.expansion
        q = flat._prepare_queries(queries, None, "ExpandedIndex")
        if q.shape[0] == 0:
            import torch

            return q, torch.empty(0, dtype=torch.int32, device=q.device)
        scores, ids = self._first_dense(q, min(x.fb_docs, _native.SSKD_K_MAX), kw)
        return rocchio_device(flat, q, scores, ids, x)

    def _dense_rounds(self, queries, kw):
        counts = None
        for _ in range(self.expansion.rounds):
            queries, counts = self.expand_queries_device(queries, **kw)
        return queries, counts

    # ------------------------------------------------------------------ lexical side
    def _lexical(self, texts: Sequence[str], kb: int, mask=None):
        """The BM25 ranking at ``kb`` and the RM3 step over it: ``rm3_device``'s outputs."""
        bm25 = self.bm25
        lims, terms, lims_host = bm25.query_csr_host(texts)
        rank_s, rank_i = bm25._search_csr((lims, terms), len(texts), kb)
        return rm3_device(bm25, (lims, terms), lims_host, rank_s, rank_i, self.expansion, mask)

    def _kb(self, depth: Optional[int] = None) -> int:
        """How deep the BM25 ranking is that feeds RM3: ``fb_docs``, or under hybrid the depth of the fuse (a mask
        hides rows after the retrieval, so the feedback rows are the first ``fb_docs`` survivors of that list)."""
        if self.kind == "hybrid":
            return self.first.clip_depth(depth)
        return self.expansion.fb_docs

    # ------------------------------------------------------------------ searching
    def search_device(self, *args, **kw):
        """``first.search_device`` for the expanded queries: same arguments, same results (device tensors), nothing
        synchronised on the way.  The dense path is capturable by ``torch.cuda.graph``; the lexical path tokenises on
        the host."""
        import torch

        if self.kind == "dense":
            queries, k = args[0], (args[1] if len(args) > 1 else kw.pop("k"))
            if not isinstance(queries, torch.Tensor):
                raise TypeError("ExpandedIndex.search_device expects a float32 device tensor (search() takes NumPy)")
            with torch.cuda.device(self.flat.device):
                expanded, _ = self._dense_rounds(queries, kw)
                return self.first.search_device(expanded, k, **kw)
        if self.kind == "bm25":
            texts = args[0]
            top_k = int(args[1] if len(args) > 1 else kw.pop("top_k", 100))
            if not 1 <= top_k <= _bm25.K_MAX:
                raise ValueError(f"top_k={top_k} outside [1, {_bm25.K_MAX}]")
            if len(texts) == 0:
                return self.bm25._search_csr(None, 0, top_k)
            csr = self._lexical(texts, self._kb())[0]
            return self.bm25._search_csr(csr, len(texts), top_k, kw.get("max_workspace_bytes"))
        texts, query_emb = args[0], args[1]
        k = args[2] if len(args) > 2 else kw.pop("k", 10)
        if not isinstance(query_emb, torch.Tensor):
            raise TypeError("ExpandedIndex.search_device expects a float32 device tensor (search() takes NumPy)")
        if len(texts) != query_emb.shape[0]:
            raise ValueError(f"{len(texts)} query texts for {query_emb.shape[0]} query embeddings")
        if len(texts) == 0:
            return self.first.search_device(texts, query_emb, k, **kw)
        hybrid = self.first
        hybrid.check_same_rows()
        with torch.cuda.device(self.flat.device):
            allow = kw.get("allow")
            expanded, _ = self._dense_rounds(query_emb, {"allow": allow})
            mask = self.flat.search_mask(allow)
            csr = self._lexical(texts, self._kb(kw.get("depth")), mask)[0]
            return hybrid.search_device(texts, expanded, k, query_csr=csr, **kw)

    def search(self, *args, **kw):
        """``search_device`` in ``first.search``'s NumPy form (embeddings as NumPy ``[nq, 384]`` or one ``[384]`` vector;
        a hybrid search takes one text with one vector as well)."""
        import torch

        from .index import _host_queries_to_device

        args = list(args)
        at = {"dense": 0, "hybrid": 1}.get(self.kind)
        if self.kind == "hybrid" and isinstance(args[0], str):
            args[0] = [args[0]]
        if at is not None:
            emb = np.asarray(args[at], dtype=np.float32)
            if not np.isfinite(emb).all():
                raise ValueError("query embeddings must be finite (NaN or infinity found)")
            args[at] = _host_queries_to_device(emb, self.flat.device)
        out = self.search_device(*args, **kw)
        torch.cuda.synchronize(out[0].device)
        return tuple(t.cpu().numpy() for t in out)

    def explain(self, *args, **kw) -> List[dict]:
        """What the expansion chose, per query, for logs and tests: ``{"feedback_rows": rows the rule used}`` and, where
        there is a lexical side, ``"terms": [(word, weight), ...]`` in selection order and ``"fb_lexical"``.  Takes
        ``search``'s arguments (``k`` is not needed)."""
        import torch

        from .index import _host_queries_to_device

        out: List[dict] = []
        if self.kind != "bm25":
            emb = args[0] if self.kind == "dense" else args[1]
            if not isinstance(emb, torch.Tensor):
                emb = _host_queries_to_device(np.asarray(emb, dtype=np.float32), self.flat.device)
            with torch.cuda.device(self.flat.device):
                dense_kw = {"allow": kw.get("allow")} if self.kind == "hybrid" else kw
                _, counts = self._dense_rounds(emb, dense_kw)
            out = [{"feedback_rows": int(c)} for c in counts.cpu().tolist()]
        if self.kind != "dense":
            texts = [args[0]] if isinstance(args[0], str) else list(args[0])
            if not out:
                out = [{} for _ in texts]
            if texts:
                mask = self.flat.search_mask(kw.get("allow")) if self.kind == "hybrid" else None
                _, sel_t, sel_w, counts, fb = self._lexical(texts, self._kb(kw.get("depth")), mask)
                words = self.bm25.bm25.words
                sel_t, sel_w, counts, fb = (t.cpu().tolist() for t in (sel_t, sel_w, counts, fb))
                for q, entry in enumerate(out):
                    entry["terms"] = [(words[t], w) for t, w in zip(sel_t[q][: counts[q]], sel_w[q][: counts[q]])]
                    entry["fb_lexical"] = fb[q]
        return out
