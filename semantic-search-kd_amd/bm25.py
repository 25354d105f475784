"""BM25 index and search on the MI355X: ``rank_bm25.BM25Okapi`` as the reference's ``BM25Index`` uses it, bit for bit.

Drop-in for the reference's ``BM25Index`` (reference: src/data/bm25.py): same constructor, same methods, same
directory format on disk (``doc_ids.json``, ``tokenized_corpus.json``, ``bm25_params.json``, ``checksum.json``), so an
index saved by either loads in the other.  ``rank_bm25`` itself is not needed.

Where the reference scores one query at a time on the host (one dense ``N``-vector per query token, then a full sort
of ``N`` scores), the index here is inverted once on the host (``BM25Postings``, vectorised NumPy) and uploaded:
postings in CSR by term, each ``(int32 row, fp64 w)`` with the length-normalised term weight ``w`` already evaluated
by the very array expression of the library.  ``batch_search`` is then ONE call of ``sskd_bm25_search`` for all
queries; the kernels multiply ``idf * w`` and add in query-token order in fp64 without fma, which gives the bits of
the library's ``score += idf * array``, and rank by (score descending, row ascending), the order of the
reference's stable ``sorted(..., reverse=True)``.
"""
from __future__ import annotations

import hashlib
import json
import math
from itertools import chain
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native

K_MAX = 256   # sskd_bm25_search: 1 <= k <= 256
RM3_ROW_TERMS = 256   # SSKD_RM3_ROW_TERMS: distinct terms a row keeps in the forward index


class BM25Postings:
    """The host side of the index: vocabulary, idf table and postings of one tokenised corpus.

    ``vocab`` maps a word to its term id, ids in order of first appearance in the corpus (the insertion order of the
    library's dicts); ``idf`` is fp64 ``[n_terms]`` with negative values already replaced by ``epsilon *
    average_idf``; term ``t``'s postings are ``post_rows[term_offsets[t]:term_offsets[t + 1]]`` (int32, ascending) and
    ``post_w`` (fp64) beside them, with ``post_tf`` (int32), the term's count in that row, kept for the forward index
    (``forward_index``)."""

    def __init__(self, tokenized_corpus: Sequence[Sequence[str]], k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25):
        n = len(tokenized_corpus)
        if n == 0:
            raise ValueError("BM25 needs at least one document")   # (the library divides by the corpus size)
        if n >= (1 << 31) - 64:
            raise ValueError("rows are int32 per index: the corpus is too large for one BM25 index")
        self.k1, self.b, self.epsilon = k1, b, epsilon
        self.corpus_size = n
        doc_len = np.fromiter(map(len, tokenized_corpus), dtype=np.int64, count=n)
        total = int(doc_len.sum())
        self.doc_len = doc_len
        self.avgdl = total / n
        flat = list(chain.from_iterable(tokenized_corpus))
        self.vocab: Dict[str, int] = {w: i for i, w in enumerate(dict.fromkeys(flat))}
        n_terms = len(self.vocab)
        terms = np.fromiter(map(self.vocab.__getitem__, flat), dtype=np.int64, count=total)
        del flat
        rows = np.repeat(np.arange(n, dtype=np.int64), doc_len)
        # one posting per distinct (term, row); np.unique sorts by term, then row: CSR by term with ascending rows
        pairs, freq = np.unique(terms * n + rows, return_counts=True)
        del terms, rows
        post_term = pairs // n
        post_rows = pairs - post_term * n
        del pairs
        n_w = np.bincount(post_term, minlength=n_terms)                 # documents containing each word
        self.term_offsets = np.zeros(n_terms + 1, dtype=np.int64)
        np.cumsum(n_w, out=self.term_offsets[1:])
        # idf(w) = log(N - n_w + 0.5) - log(n_w + 0.5) with math.log (np.log may round differently), once per distinct
        # n_w; the average is a plain left-to-right float sum in vocabulary order (np.sum is pairwise, the built-in
        # sum() compensates: both give other bits than the library's loop)
        idf_of = {int(c): math.log(n - int(c) + 0.5) - math.log(int(c) + 0.5) for c in np.unique(n_w)}
        idf = [idf_of[c] for c in n_w.tolist()]
        idf_sum = 0
        for v in idf:
            idf_sum += v
        self.average_idf = idf_sum / n_terms if n_terms else 0.0
        idf = np.asarray(idf, dtype=np.float64).reshape(n_terms)
        idf[idf < 0] = epsilon * self.average_idf
        self.idf = idf
        # the library's expression on the matching entries only (elementwise fp64: same bits as on the dense arrays)
        q_freq = freq.astype(np.int64)
        dl = doc_len[post_rows]
        if total:
            self.post_w = np.asarray(q_freq * (k1 + 1) / (q_freq + k1 * (1 - b + b * dl / self.avgdl)), dtype=np.float64)
        else:
            self.post_w = np.zeros(0, dtype=np.float64)
        self.post_rows = post_rows.astype(np.int32)
        self.post_tf = freq.astype(np.int32)
        self._words: Optional[List[str]] = None

    @property
    def n_terms(self) -> int:
        return len(self.vocab)

    @property
    def words(self) -> List[str]:
        """The vocabulary by term id."""
        if self._words is None:
            self._words = list(self.vocab)
        return self._words

    def forward_index(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The index by row, what query expansion reads (``include/sskd_amd.h``, "Query expansion"): ``(fwd_lims int64
        [rows + 1], fwd_terms int32, fwd_p float64)``, row ``r``'s entries at ``fwd_lims[r]:fwd_lims[r + 1]``, ascending
        by term id, ``p = tf / dl`` in fp64 with ``dl`` the row's full token count.  A row keeps at most
        ``RM3_ROW_TERMS`` = 256 distinct terms: the largest ``tf`` first, ties to the lower term id.  12 bytes per
        distinct (row, term) - the size of the postings - plus 8 per row."""
        n, n_terms = self.corpus_size, self.n_terms
        term = np.repeat(np.arange(n_terms, dtype=np.int64), np.diff(self.term_offsets))
        rows = self.post_rows.astype(np.int64)
        tf = self.post_tf.astype(np.int64)
        per_row = np.bincount(rows, minlength=n)
        if per_row.size and int(per_row.max()) > RM3_ROW_TERMS:
            order = np.lexsort((term, -tf, rows))                        # by row, then tf descending, then term id
            starts = np.cumsum(per_row) - per_row
            place = np.arange(order.size, dtype=np.int64) - starts[rows[order]]
            keep = order[place < RM3_ROW_TERMS]
            term, rows, tf = term[keep], rows[keep], tf[keep]
        order = np.lexsort((term, rows))                                 # CSR by row, ascending term ids
        term, rows, tf = term[order], rows[order], tf[order]
        lims = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=lims[1:])
        p = np.asarray(tf / self.doc_len[rows], dtype=np.float64) if rows.size else np.zeros(0, dtype=np.float64)
        return lims, term.astype(np.int32), p

    def term_ids(self, tokens: Sequence[str]) -> List[int]:
        """Term ids of a token list in order, repeats kept, out-of-vocabulary tokens dropped (they score nothing)."""
        get = self.vocab.get
        return [t for t in map(get, tokens) if t is not None]


class BM25Index:
    """BM25 index with the reference's surface; searches run on the device."""

    def __init__(self, index_path: Optional[str] = None, auto_load: bool = False, device: Optional[str] = None):
        self.index_path = Path(index_path) if index_path else None
        self.bm25: Optional[BM25Postings] = None
        self.doc_ids: list = []
        self.tokenized_corpus: List[List[str]] = []
        self.device = device
        self._device_tables = None
        self._forward_tables = None
        if auto_load and self.index_path and (self.index_path / "tokenized_corpus.json").exists():
            self.load()

    def _tokenize(self, text: str) -> List[str]:
        return text.lower().split()

    # ------------------------------------------------------------------ building
    def _rebuild(self, k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25) -> None:
        self.bm25 = BM25Postings(self.tokenized_corpus, k1=k1, b=b, epsilon=epsilon)
        self._device_tables = None
        self._forward_tables = None

    def build_from_texts(self, doc_ids: Sequence, texts: Sequence[str]) -> None:
        """Index ``texts`` under ``doc_ids`` (nothing is written; ``save()`` does that when ``index_path`` is set)."""
        if len(doc_ids) != len(texts):
            raise ValueError(f"{len(doc_ids)} doc ids for {len(texts)} texts")
        self.doc_ids = list(doc_ids)
        self.tokenized_corpus = [self._tokenize(str(t)) for t in texts]
        self._rebuild()

    def build_from_parquet(self, corpus_file, output_dir, text_field: str = "text", id_field: str = "chunk_id") -> None:
        import pyarrow.parquet as pq

        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        table = pq.read_table(str(corpus_file), columns=[id_field, text_field])
        self.build_from_texts(table.column(id_field).to_pylist(), table.column(text_field).to_pylist())
        self.index_path = output_dir
        self.save()

    # ------------------------------------------------------------------ the reference's directory format
    def save(self) -> None:
        if not self.index_path:
            raise ValueError("index_path not set")
        self.index_path.mkdir(parents=True, exist_ok=True)
        with open(self.index_path / "doc_ids.json", "w") as f:
            json.dump(self.doc_ids, f)
        with open(self.index_path / "tokenized_corpus.json", "w") as f:
            json.dump(self.tokenized_corpus, f)
        params = {
            "k1": getattr(self.bm25, "k1", 1.5),
            "b": getattr(self.bm25, "b", 0.75),
            "epsilon": getattr(self.bm25, "epsilon", 0.25),
            "corpus_size": len(self.tokenized_corpus),
        }
        with open(self.index_path / "bm25_params.json", "w") as f:
            json.dump(params, f)
        with open(self.index_path / "checksum.json", "w") as f:
            json.dump({"sha256": self._compute_checksum()}, f)

    def _compute_checksum(self) -> str:
        h = hashlib.sha256()
        h.update(json.dumps(self.doc_ids, sort_keys=True).encode())
        h.update(json.dumps(self.tokenized_corpus, sort_keys=True).encode())
        return h.hexdigest()

    def load(self) -> None:
        if not self.index_path or not self.index_path.exists():
            raise FileNotFoundError(f"Index not found: {self.index_path}")
        corpus_json = self.index_path / "tokenized_corpus.json"
        if not corpus_json.exists():
            raise FileNotFoundError(f"tokenized_corpus.json not found at {self.index_path}")
        try:
            with open(self.index_path / "doc_ids.json", "r") as f:
                self.doc_ids = json.load(f)
            with open(corpus_json, "r") as f:
                self.tokenized_corpus = json.load(f)
        except json.JSONDecodeError as e:
            raise ValueError(f"Checksum/integrity failure: the index at {self.index_path} is corrupted - {e}") from e
        checksum_file = self.index_path / "checksum.json"
        if checksum_file.exists():
            with open(checksum_file, "r") as f:
                expected = json.load(f)["sha256"]
            actual = self._compute_checksum()
            if actual != expected:
                raise ValueError(
                    f"Index integrity check failed: checksum mismatch. Expected {expected[:12]}..., got {actual[:12]}..."
                )
        if len(self.doc_ids) != len(self.tokenized_corpus):
            raise ValueError(f"{len(self.doc_ids)} doc ids for {len(self.tokenized_corpus)} documents")
        params = {}
        params_file = self.index_path / "bm25_params.json"
        if params_file.exists():
            try:
                with open(params_file, "r") as f:
                    params = json.load(f)
            except json.JSONDecodeError as e:
                raise ValueError(f"bm25_params.json is corrupted - {e}") from e
        self._rebuild(k1=params.get("k1", 1.5), b=params.get("b", 0.75), epsilon=params.get("epsilon", 0.25))

    # ------------------------------------------------------------------ searching
    def _require_built(self) -> BM25Postings:
        if self.bm25 is None:
            raise ValueError("Index not loaded. Call load() or build_from_parquet() first.")
        return self.bm25

    def _tables(self):
        """The index in HBM (uploaded at the first search): term offsets, posting rows, posting weights, idf."""
        if self._device_tables is None:
            import torch

            from .index import _resolve_device

            _native.require_gpu()
            post = self._require_built()
            dev = _resolve_device(self.device)

            def up(a: np.ndarray, dtype) -> "torch.Tensor":
                a = np.ascontiguousarray(a, dtype=dtype)
                if a.size == 0:     # the C-ABI wants real pointers: one unused element
                    a = np.zeros(1, dtype=dtype)
                return torch.from_numpy(a).to(dev)

            self._device_tables = (dev, up(post.term_offsets, np.int64), up(post.post_rows, np.int32),
                                   up(post.post_w, np.float64), up(post.idf, np.float64))
        return self._device_tables

    def forward_tables(self):
        """The forward index in HBM (``BM25Postings.forward_index``; built and uploaded at the first query expansion,
        not before, and never persisted: it follows from the tokenised corpus): ``(fwd_lims, fwd_terms, fwd_p,
        entries)``."""
        if self._forward_tables is None:
            import torch

            dev = self._tables()[0]
            lims, terms, p = self._require_built().forward_index()
            n_fwd = int(terms.size)
            if n_fwd == 0:      # the C-ABI wants real pointers: one unused element
                terms, p = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float64)
            self._forward_tables = (torch.from_numpy(lims).to(dev), torch.from_numpy(terms).to(dev),
                                    torch.from_numpy(p).to(dev), n_fwd)
        return self._forward_tables

    def query_csr(self, queries: Sequence[str]):
        """The queries' term ids as the device CSR the kernels read: ``(lims int64 [nq + 1], terms int32)`` device
        tensors, tokens in query order, repeats kept, out-of-vocabulary tokens dropped.  Made once per batch and shared
        by every call that scores it (``search_device``, ``HybridIndex``)."""
        return self.query_csr_host(queries)[:2]

    def query_csr_host(self, queries: Sequence[str]):
        """``query_csr`` and, third, the host copy of ``lims`` (NumPy int64 ``[nq + 1]``) for a call that validates
        the segment lengths before its launch (``sskd_prf_rm3``)."""
        import torch

        post = self._require_built()
        dev = self._tables()[0]
        nq = len(queries)
        q_ids = [post.term_ids(self._tokenize(q)) for q in queries]
        lims = np.zeros(nq + 1, dtype=np.int64)
        np.cumsum(np.fromiter(map(len, q_ids), dtype=np.int64, count=nq), out=lims[1:])
        flat = np.fromiter(chain.from_iterable(q_ids), dtype=np.int32, count=int(lims[-1]))
        if flat.size == 0:
            flat = np.zeros(1, dtype=np.int32)
        return torch.from_numpy(lims).to(dev), torch.from_numpy(flat).to(dev), lims

    def search_device(self, queries: Sequence[str], top_k: int = 100, max_workspace_bytes: Optional[int] = None):
        """``(D float64 [nq, top_k], I int64 [nq, top_k])`` device tensors: rows of the corpus, best first (score
        descending, then lower row), padded with ``(-inf, -1)`` when ``top_k`` exceeds the corpus.  One device call;
        ``max_workspace_bytes`` caps its scratch buffer (never below what one query needs): the call then works
        through the queries in chunks that fit, with the same result."""
        self._require_built()
        top_k = int(top_k)
        if not 1 <= top_k <= K_MAX:
            raise ValueError(f"top_k={top_k} outside [1, {K_MAX}]")
        nq = len(queries)
        csr = self.query_csr(queries) if nq else None
        return self._search_csr(csr, nq, top_k, max_workspace_bytes)

    def _search_csr(self, csr, nq: int, top_k: int, max_workspace_bytes: Optional[int] = None):
        """``search_device`` for queries already tokenised by ``query_csr`` (``csr`` is not read when ``nq`` is 0)."""
        import torch

        post = self._require_built()
        dev, offsets, rows, w, idf = self._tables()
        lib = _native.load()
        scores = torch.empty((nq, top_k), dtype=torch.float64, device=dev)
        ids = torch.empty((nq, top_k), dtype=torch.int64, device=dev)
        if nq == 0:
            return scores, ids
        d_lims, d_terms = csr
        need = int(lib.sskd_bm25_search_workspace_bytes(post.corpus_size, nq, top_k))
        if max_workspace_bytes is not None:
            one_query = int(lib.sskd_bm25_search_workspace_bytes(post.corpus_size, 1, top_k))
            need = min(need, max(int(max_workspace_bytes), one_query))
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        _native.check(
            lib.sskd_bm25_search(
                offsets.data_ptr(), rows.data_ptr(), w.data_ptr(), idf.data_ptr(), post.corpus_size, post.n_terms,
                d_lims.data_ptr(), d_terms.data_ptr(), nq, top_k, scores.data_ptr(), ids.data_ptr(),
                workspace.data_ptr(), need, _native.current_stream_ptr(dev),
            )
        )
        return scores, ids

    def batch_search(self, queries: List[str], top_k: int = 100) -> List[List[Tuple[str, float]]]:
        """``[(doc_id, score)]`` per query, best first: the reference's ``search`` for every query, one device call."""
        post = self._require_built()
        if not queries:
            return []
        k = min(int(top_k), post.corpus_size)   # the reference's slice stops at the corpus
        if k < 1:
            return [[] for _ in queries]
        if k > K_MAX:
            raise ValueError(f"top_k={top_k} > {K_MAX}: the device search returns at most {K_MAX} rows per query")
        scores, ids = self.search_device(queries, k)
        scores, ids = scores.cpu().tolist(), ids.cpu().tolist()
        doc_ids = self.doc_ids
        return [[(doc_ids[r], s) for r, s in zip(row_ids, row_scores)] for row_ids, row_scores in zip(ids, scores)]

    def search(self, query: str, top_k: int = 100) -> List[Tuple[str, float]]:
        self._require_built()
        return self.batch_search([query], top_k=top_k)[0]

    def get_doc_text(self, doc_id) -> str:
        """The document's text as reconstructed from its tokens ('' for an unknown id)."""
        self._require_built()
        try:
            return " ".join(self.tokenized_corpus[self.doc_ids.index(doc_id)])
        except ValueError:
            return ""


def build_bm25_index(corpus_file, output_dir, text_field: str = "text", id_field: str = "chunk_id") -> BM25Index:
    index = BM25Index(str(output_dir))
    index.build_from_parquet(corpus_file, output_dir, text_field, id_field)
    return index
