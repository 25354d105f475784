"""``GraphIndex``: a fixed-degree k-NN graph over the unchanged flat index, beam search with exact scores.

The reference's ``configs/index.yaml`` names three index types - ``hnsw`` (its default: ``M: 32``, ``efConstruction:
200``, ``efSearch: 64``), ``ivf_pq`` and ``flat`` - and a validation gate (``recall_threshold: 0.97`` against brute
force).  ``flat`` is ``FAISSIndexBuilder``, the inverted lists are ``ivf.IVFIndex`` / ``pq.IVFPQIndex``; this is the graph.

* The rows are a ``FAISSIndexBuilder`` (``graph.flat``), not permuted and not copied; the graph is int32 ``[ntotal, M]``
  in HBM (``-1`` = no edge, no self edge, no edge twice in a row) and the entry points are copies of
  ``entry_rows[i] = floor(i * ntotal / n_entry)`` in a second small ``FAISSIndexBuilder`` (``graph.entry``).  Everything
  keyed by row id - ``allow`` filters, ``remove_ids``, ``doc_ids``, groups and the flat index's own exact searches -
  keeps working on the same ids.
* WHICH rows a query looks at is approximate; every score and every order is exact (``include/sskd_amd.h``, "Graph
  index"): a search returns, of the rows it scored, the top-k in the exact search's order with the exact search's bits.
* The graph is built on the device and deterministically: the k-NN lists are the exact search of the index against
  itself, pruning (``sskd_graph_prune``), reverse edges (a stable sort) and the merge (``sskd_graph_merge``) are
  integer-only.
* ``insert`` appends rows and links them into the graph it has, at a cost proportional to the new rows: their exact
  k-NN lists, the same pruning over two kinds of lists (``sskd_graph_insert_prune``), reverse edges, the adjacency of
  the new rows (``sskd_graph_merge_rows``) and, for every linked row a new row names, a re-selection of its
  replaceable half by exact score (``sskd_graph_link``).  ``add`` rebuilds the graph over all rows.
"""
from __future__ import annotations

import json
import math
from pathlib import Path
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native
from .index import FAISSIndexBuilder, IndexHandle, _host_queries_to_device
from .overlay import FlatOverlay, read_versioned_json

GRAPH_EF_MAX = 256
GRAPH_M_MAX = 64
GRAPH_KNN_MAX = 128
GRAPH_WIDTH_MAX = 8
GRAPH_SEEDS_MAX = 32
DEFAULT_WIDTH = 4              # DESIGN section 20, "Measured"
FORMAT_VERSION = 1


# ------------------------------------------------------------------ host-side graph arithmetic (NumPy, no GPU)
def check_degree(M: int) -> int:
    M = int(M)
    if M < 4 or M > GRAPH_M_MAX or M % 2:
        raise ValueError(f"M={M}: the degree must be even and in [4, {GRAPH_M_MAX}]")
    return M


def default_n_entry(n: int, M: int) -> int:
    """``min(n, max(M, ceil(n / M)))``: one row in M, the population of HNSW's layer 1.  A k-NN graph over clustered
    rows falls into components, and a component is reached only through an entry row inside it.  A component of a
    graph whose rows have ``K0 >= M`` distinct neighbours each holds ``c > K0`` rows, and with one entry row per M rows
    it holds none with probability about ``exp(-c / M)``, whatever ``n`` is."""
    n, M = max(int(n), 0), int(M)
    return min(n, max(M, -(-n // M)))


def entry_rows_of(n: int, n_entry: int) -> np.ndarray:
    """int32 ``[n_entry]``: ``floor(i * n / n_entry)``, rows spread evenly over the index."""
    if n_entry < 0 or n_entry > n:
        raise ValueError(f"n_entry={n_entry} outside [0, {n}]")
    return ((np.arange(n_entry, dtype=np.int64) * int(n)) // max(int(n_entry), 1)).astype(np.int32)


def n_entry_of_insert(b: int, n0: int, M: int, n_entry_requested: Optional[int]) -> int:
    """Entry rows an insertion of ``b`` rows into ``n0`` adds: one in M (``default_n_entry``'s rule), or the share
    ``b / n0`` of the count the caller fixed; at least one, at most ``b``."""
    b, n0 = int(b), int(n0)
    if n_entry_requested is None:
        e = -(-b // int(M))
    else:
        e = -(-b * int(n_entry_requested) // max(n0, 1))
    return min(b, max(1, e))


def check_graph(graph: np.ndarray, n_rows: int) -> None:
    """Raises ``ValueError`` unless ``graph`` is int ``[n_rows, M]`` with an admissible M and every entry in
    ``[-1, n_rows)``."""
    g = np.asarray(graph)
    if g.ndim != 2 or g.shape[0] != n_rows or g.dtype.kind not in "iu":
        raise ValueError(f"expected an integer [{n_rows}, M] adjacency, got {g.dtype} {g.shape}")
    check_degree(g.shape[1])
    if g.size and (g.min() < -1 or g.max() >= n_rows):
        raise ValueError(f"edges outside [-1, {n_rows})")


def remap_graph(graph: np.ndarray, kept: np.ndarray) -> np.ndarray:
    """The adjacency after ``compact``: ``kept`` = the surviving OLD local rows, ascending.  Dropped rows lose their
    lists, edges to them are removed, a survivor gets its new number (its position in ``kept``), and every list is
    packed to the left in its old order and padded with -1."""
    g = np.asarray(graph, dtype=np.int64)
    kept = np.asarray(kept, dtype=np.int64)
    new_of_old = np.full(g.shape[0] + 1, -1, dtype=np.int64)     # the last slot serves the -1 entries
    new_of_old[kept] = np.arange(kept.size, dtype=np.int64)
    mapped = new_of_old[g[kept]]
    order = np.argsort(mapped < 0, axis=1, kind="stable")
    return np.take_along_axis(mapped, order, axis=1).astype(np.int32)


def save_graph(out_dir: Union[str, Path], graph: np.ndarray, entry_rows: np.ndarray, meta: dict) -> None:
    """Writes ``graph.npy``, ``graph_entry_rows.npy`` and ``graph.json``."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "graph.npy", np.ascontiguousarray(graph, dtype=np.int32))
    np.save(out / "graph_entry_rows.npy", np.ascontiguousarray(entry_rows, dtype=np.int32))
    with open(out / "graph.json", "w") as f:
        json.dump({**meta, "M": int(np.asarray(graph).shape[1]), "format_version": FORMAT_VERSION}, f)


def load_graph(index_dir: Union[str, Path]):
    """``(graph, entry_rows, meta)`` as ``save_graph`` wrote them; the adjacency and the entry rows are checked."""
    d = Path(index_dir)
    meta = read_versioned_json(d / "graph.json", FORMAT_VERSION)
    graph = np.load(d / "graph.npy")
    entry_rows = np.load(d / "graph_entry_rows.npy")
    check_graph(graph, graph.shape[0] if graph.ndim == 2 else -1)
    if int(meta["M"]) != graph.shape[1]:
        raise ValueError(f"{d}: graph.json says M={meta['M']}, graph.npy has {graph.shape[1]} columns")
    if entry_rows.ndim != 1 or entry_rows.dtype.kind not in "iu" or (
            entry_rows.size and (entry_rows.min() < 0 or entry_rows.max() >= graph.shape[0])):
        raise ValueError(f"{d}: entry rows outside [0, {graph.shape[0]})")
    if graph.shape[0] and not entry_rows.size:
        raise ValueError(f"{d}: no entry rows")
    return graph.astype(np.int32), entry_rows.astype(np.int32), meta


def is_graph_dir(index_dir: Union[str, Path]) -> bool:
    return (Path(index_dir) / "graph.json").exists()


# ------------------------------------------------------------------------------------------------ the index
class GraphIndex(FlatOverlay):
    """k-NN graph over a ``FAISSIndexBuilder``: ``graph.flat`` holds the rows, ``graph.entry`` copies of the entry rows."""

    def __init__(self, flat: Optional[FAISSIndexBuilder] = None, embedding_dim: int = 384, metric: str = "cosine",
                 device: Optional[str] = None, M: int = 32, ef: int = 64, width: int = DEFAULT_WIDTH,
                 knn_k: Optional[int] = None, n_entry: Optional[int] = None) -> None:
        super().__init__(flat if flat is not None else FAISSIndexBuilder(embedding_dim=embedding_dim, index_type="HNSW",
                                                                         metric=metric, device=device))
        self.entry = FAISSIndexBuilder(embedding_dim=self.embedding_dim, index_type="Flat", metric="ip",
                                       device=str(self.device))
        self.M = check_degree(M)
        self.knn_k = None if knn_k is None else int(knn_k)
        self.n_entry_requested = None if n_entry is None else int(n_entry)   # None: default_n_entry
        self.ef = int(ef)
        self.width = int(width)
        self.graph: Optional[torch.Tensor] = None        # device int32 [ntotal, M]
        self.entry_rows: Optional[torch.Tensor] = None   # device int32 [n_entry]
        self._n_linked = 0
        self.n_inserted = 0                              # rows linked by insert() since the last build_graph()
        self.last_search_path: Optional[str] = None

    # ------------------------------------------------------------------ properties
    @property
    def n_entry(self) -> int:
        return self.entry.ntotal

    def _require_graph(self) -> None:
        if self.graph is None or self._n_linked != self.flat.ntotal:
            raise RuntimeError("the graph is not built for the rows held: call build_graph() (or build_from_embeddings / load)")

    def graph_numpy(self) -> np.ndarray:
        """Host copy of the adjacency, int32 ``[ntotal, M]``."""
        self._require_graph()
        return self.graph.cpu().numpy()

    def entry_rows_numpy(self) -> np.ndarray:
        self._require_graph()
        return self.entry_rows.cpu().numpy()

    # ------------------------------------------------------------------ building
    def knn_device(self, knn_k: int, batch: int = 1 << 14, first: int = 0) -> torch.Tensor:
        """Device int32 ``[ntotal - first, knn_k]``: the nearest rows of every row from ``first`` on (``insert`` asks
        for the new rows only) in the exact search's rank order without the row itself, -1 where the index has fewer
        rows.  Batches of rows are searched for ``knn_k + 1`` results over ALL
        rows; the entry equal to the row is dropped, or the last one when the row is not among its own results (more
        than ``knn_k`` copies of it rank first).  The search is the flat index's ``_search_device_masked`` - what
        ``flat.search_device`` runs - called directly with no mask and ``id_offset = 0``: ``search_device`` would hide
        removed rows, which must take part here, and return global ids where the graph needs local rows.  Dropping the
        entry is a boolean-mask gather in torch, which synchronises the host once per batch: harmless for a build,
        and the reason a build cannot be captured into a graph."""
        n, K0, first = self.flat.ntotal, int(knn_k), int(first)
        rows = self._rows_view()
        out = torch.empty((n - first, K0), dtype=torch.int32, device=self.device)
        cols = torch.arange(K0 + 1, device=self.device)
        for lo in range(first, n, batch):
            part = rows[lo: lo + batch]
            _, ids = self.flat._search_device_masked(part, K0 + 1, False, None, None, None, id_offset=0)
            own = ids == torch.arange(lo, lo + part.shape[0], device=self.device)[:, None]
            drop = torch.where(own.any(dim=1), own.to(torch.int8).argmax(dim=1), torch.full_like(ids[:, 0], K0))
            out[lo - first: lo - first + part.shape[0]] = ids[cols[None, :] != drop[:, None]].view(-1, K0).to(torch.int32)
        return out

    def prune_device(self, knn: torch.Tensor, M: int) -> torch.Tensor:
        """``sskd_graph_prune``: device int32 ``[n, M]``, the M entries of every list with the fewest detours."""
        n, K0 = knn.shape
        fwd = torch.empty((n, M), dtype=torch.int32, device=self.device)
        _native.check(_native.load().sskd_graph_prune(knn.data_ptr(), n, K0, M, fwd.data_ptr(),
                                                      _native.current_stream_ptr(self.device)))
        return fwd

    def reverse_device(self, fwd: torch.Tensor) -> torch.Tensor:
        """Device int32 ``[n, M / 2]``: ``rev[v]`` = the rows u with v among the first M / 2 entries of ``fwd[u]``,
        ordered by (position of v in ``fwd[u]``, u), the first M / 2, -1 padded.  A stable sort by target over the
        edges laid out position-major."""
        n, M = fwd.shape
        h = M // 2
        target = fwd[:, :h].t().reshape(-1).to(torch.int64)                       # (position, u) ascending
        source = torch.arange(n, dtype=torch.int32, device=self.device).repeat(h)
        real = target >= 0
        target, source = target[real], source[real]
        order = torch.sort(target, stable=True).indices
        target, source = target[order], source[order]
        counts = torch.bincount(target, minlength=n)
        first = torch.cumsum(counts, 0) - counts
        place = torch.arange(target.numel(), device=self.device) - first[target]
        rev = torch.full((n, h), -1, dtype=torch.int32, device=self.device)
        fits = place < h
        rev[target[fits], place[fits]] = source[fits]
        return rev

    def merge_device(self, fwd: torch.Tensor, rev: torch.Tensor) -> torch.Tensor:
        """``sskd_graph_merge``: device int32 ``[n, M]``."""
        n, M = fwd.shape
        graph = torch.empty((n, M), dtype=torch.int32, device=self.device)
        _native.check(_native.load().sskd_graph_merge(fwd.data_ptr(), rev.data_ptr(), n, M, graph.data_ptr(),
                                                      _native.current_stream_ptr(self.device)))
        return graph

    # ------------------------------------------------------------------ incremental insertion
    def insert_prune_device(self, graph_old: torch.Tensor, knn_new: torch.Tensor) -> torch.Tensor:
        """``sskd_graph_insert_prune``: device int32 ``[b, M]`` for the ``b`` new rows behind the ``n0`` rows of
        ``graph_old``; the list of a neighbour is its row of ``graph_old`` or of ``knn_new``."""
        n0, M = graph_old.shape
        b, K0 = knn_new.shape
        fwd = torch.empty((b, M), dtype=torch.int32, device=self.device)
        _native.check(_native.load().sskd_graph_insert_prune(graph_old.data_ptr(), n0, knn_new.data_ptr(), b, K0, M,
                                                             fwd.data_ptr(), _native.current_stream_ptr(self.device)))
        return fwd

    def incoming_device(self, fwd_new: torch.Tensor, n0: int):
        """The reverse edges of an insertion, ``(incoming_new [b, M / 2], touched [t], incoming_old [t, M / 2])``, all
        device int32: the sources ``n0 + v`` that name a target among the first M / 2 entries of ``fwd_new[v]``, by
        (position, source), the first M / 2 per target, -1 padded.  ``touched`` = the targets below ``n0``, ascending
        and unique; row i of ``incoming_old`` belongs to ``touched[i]``.  One stable sort by target over the edges laid
        out position-major, as ``reverse_device``."""
        b, M = fwd_new.shape
        h = M // 2
        target = fwd_new[:, :h].t().reshape(-1).to(torch.int64)                   # (position, source) ascending
        source = (n0 + torch.arange(b, dtype=torch.int32, device=self.device)).repeat(h)
        real = target >= 0
        target, source = target[real], source[real]
        order = torch.sort(target, stable=True).indices
        target, source = target[order], source[order]
        named, group, counts = torch.unique_consecutive(target, return_inverse=True, return_counts=True)
        first = torch.cumsum(counts, 0) - counts
        place = torch.arange(target.numel(), device=self.device) - first[group]
        fits = place < h
        incoming = torch.full((named.numel(), h), -1, dtype=torch.int32, device=self.device)
        incoming[group[fits], place[fits]] = source[fits]
        n_touched = int((named < n0).sum().item())
        incoming_new = torch.full((b, h), -1, dtype=torch.int32, device=self.device)
        incoming_new[named[n_touched:] - n0] = incoming[n_touched:]
        return incoming_new, named[:n_touched].to(torch.int32), incoming[:n_touched].contiguous()

    def merge_rows_device(self, fwd_new: torch.Tensor, incoming_new: torch.Tensor, n0: int, out: torch.Tensor) -> None:
        """``sskd_graph_merge_rows`` into ``out`` (device int32 ``[b, M]``, the rows ``[n0, n0 + b)`` of the adjacency)."""
        b, M = fwd_new.shape
        _native.check(_native.load().sskd_graph_merge_rows(fwd_new.data_ptr(), incoming_new.data_ptr(), b, n0, n0 + b, M,
                                                           out.data_ptr(), _native.current_stream_ptr(self.device)))

    def link_device(self, graph: torch.Tensor, n0: int, touched: torch.Tensor, incoming_old: torch.Tensor) -> None:
        """``sskd_graph_link``: rewrites the rows ``touched`` (strictly ascending, below ``n0``) of ``graph`` (device
        int32 ``[ntotal, M]``) in place."""
        n1, M = graph.shape
        _native.check(_native.load().sskd_graph_link(self.flat._tiled.data_ptr(), graph.data_ptr(), n0, n1, M,
                                                     touched.data_ptr(), incoming_old.data_ptr(), touched.numel(),
                                                     _native.current_stream_ptr(self.device)))

    def insert(self, embeddings, groups: Optional[Sequence] = None) -> None:
        """Append rows and link them into the graph the index has ("Incremental insertion"): the
        cost follows the new rows, not the corpus.  The new rows get their exact k-NN lists over ALL rows, pruned like
        a build's; every linked row a new row names re-selects, by exact score, the half of its adjacency that the
        build's forward edges do not protect.  Deterministic.  ``groups`` passes to the flat add.  ``n_inserted`` counts
        the rows linked this way since the last ``build_graph()``: the graph of a corpus that has grown severalfold is
        worth rebuilding."""
        self._require_graph()
        n0 = self.flat.ntotal
        self.flat.add(embeddings, groups=groups)
        n1 = self.flat.ntotal
        b = n1 - n0
        if b == 0:
            return
        M = self.M
        K0 = self.knn_k if self.knn_k is not None else min(2 * M, GRAPH_KNN_MAX)
        e = n_entry_of_insert(b, n0, M, self.n_entry_requested)
        with torch.cuda.device(self.device):
            knn_new = self.knn_device(K0, first=n0)
            fwd_new = self.insert_prune_device(self.graph, knn_new)
            incoming_new, touched, incoming_old = self.incoming_device(fwd_new, n0)
            graph = torch.empty((n1, M), dtype=torch.int32, device=self.device)
            graph[:n0].copy_(self.graph)
            self.merge_rows_device(fwd_new, incoming_new, n0, graph[n0:])
            self.link_device(graph, n0, touched, incoming_old)
            new_entry = torch.from_numpy((n0 + entry_rows_of(b, e).astype(np.int64)).astype(np.int32)).to(self.device)
            self.entry.add(self._rows_view()[new_entry.to(torch.int64)].contiguous())
            self.entry_rows = torch.cat([self.entry_rows, new_entry])
            self.graph = graph
        self._n_linked = n1
        self.n_inserted += b

    def build_graph(self, M: Optional[int] = None, knn_k: Optional[int] = None) -> None:
        """k-NN lists (the exact search of the index against itself), detour pruning, reverse edges, merge; then the
        entry rows.  ``knn_k`` defaults to ``2 M``.  Deterministic."""
        n = self.flat.ntotal
        if n < 1:
            raise RuntimeError("build_graph(): the index is empty")
        M = self.M if M is None else check_degree(M)
        K0 = int(knn_k) if knn_k is not None else (self.knn_k if self.knn_k is not None else 2 * M)
        if K0 < M or K0 > GRAPH_KNN_MAX:
            raise ValueError(f"knn_k={K0} outside [M={M}, {GRAPH_KNN_MAX}]")
        with torch.cuda.device(self.device):
            fwd = self.prune_device(self.knn_device(K0), M)
            graph = self.merge_device(fwd, self.reverse_device(fwd))
        self.M, self.knn_k = M, K0
        self._install(graph, None)
        self.n_inserted = 0

    def _install(self, graph: torch.Tensor, entry_rows: Optional[np.ndarray]) -> None:
        """Adopts a device adjacency over all rows held and (re)builds the entry index (None: the default rows)."""
        n = self.flat.ntotal
        if entry_rows is None:
            want = self.n_entry_requested
            entry_rows = entry_rows_of(n, default_n_entry(n, graph.shape[1]) if want is None else max(1, min(want, n)))
        with torch.cuda.device(self.device):
            self.graph = graph.contiguous()
            self.entry_rows = torch.from_numpy(np.ascontiguousarray(entry_rows, dtype=np.int32)).to(self.device)
            self.entry.build_from_embeddings(self._rows_view()[self.entry_rows.to(torch.int64)].contiguous())
        self.M = int(graph.shape[1])
        self._n_linked = n

    @classmethod
    def from_graph(cls, flat: FAISSIndexBuilder, graph, entry_rows=None, ef: int = 64, width: int = DEFAULT_WIDTH
                   ) -> "GraphIndex":
        """A caller's adjacency over the rows of ``flat``: integer ``[ntotal, M]``, entries in ``[-1, ntotal)``."""
        g = np.asarray(graph)
        check_graph(g, flat.ntotal)
        index = cls(flat=flat, M=g.shape[1], ef=ef, width=width)
        index._from_host(g, entry_rows)
        return index

    def _from_host(self, graph: np.ndarray, entry_rows) -> None:
        with torch.cuda.device(self.device):
            device_graph = torch.from_numpy(np.ascontiguousarray(graph, dtype=np.int32)).to(self.device)
        self._install(device_graph, None if entry_rows is None else np.asarray(entry_rows))

    def build_from_embeddings(self, embeddings, M: Optional[int] = None, knn_k: Optional[int] = None,
                              groups: Optional[Sequence] = None, doc_ids: Optional[Sequence[str]] = None) -> IndexHandle:
        """Add the rows and build the graph."""
        handle = self.flat.build_from_embeddings(embeddings, doc_ids=doc_ids, groups=groups)
        self.build_graph(M=M, knn_k=knn_k)
        return handle

    def build_from_parquet(self, model, parquet_path, M: Optional[int] = None, knn_k: Optional[int] = None,
                           **flat_args) -> IndexHandle:
        """``FAISSIndexBuilder.build_from_parquet`` (its arguments pass through), then the graph."""
        handle = self.flat.build_from_parquet(model=model, parquet_path=parquet_path, **flat_args)
        self.build_graph(M=M, knn_k=knn_k)
        return handle

    def add(self, embeddings, groups: Optional[Sequence] = None) -> None:
        """Flat add, then ``build_graph()`` over ALL rows (DESIGN section 20 has the rebuild time); ``insert`` appends
        without rebuilding."""
        first = self.flat.ntotal
        self.flat.add(embeddings, groups=groups)
        if self.flat.ntotal != first or self.graph is None:
            self.build_graph()

    def compact(self) -> np.ndarray:
        """The flat ``compact()``, then the edges are remapped through the returned ``kept`` (``remap_graph``) and the
        entry rows rebuilt over the new ``ntotal``."""
        self._require_graph()
        graph = self.graph_numpy()
        kept = self.flat.compact()
        self._from_host(remap_graph(graph, kept - self.flat.id_offset), None)
        self.n_inserted = min(self.n_inserted, self.flat.ntotal)
        return kept

    # ------------------------------------------------------------------ search
    def _search_args(self, k: int, ef: Optional[int], width: Optional[int], max_iterations: Optional[int]):
        k = int(k)
        ef = self.ef if ef is None else int(ef)
        width = self.width if width is None else int(width)
        if ef < 1 or ef > GRAPH_EF_MAX:
            raise ValueError(f"ef={ef} outside [1, {GRAPH_EF_MAX}]")
        if k < 1 or k > ef:
            raise ValueError(f"k={k} outside [1, ef={ef}]")
        if width < 1 or width > GRAPH_WIDTH_MAX:
            raise ValueError(f"width={width} outside [1, {GRAPH_WIDTH_MAX}]")
        max_iterations = ef if max_iterations is None else int(max_iterations)
        if max_iterations < 1:
            raise ValueError(f"max_iterations={max_iterations} < 1")
        return k, ef, width, max_iterations

    def seeds_device(self, q: torch.Tensor, ef: int) -> torch.Tensor:
        """Device int64 ``[nq, n_seed]``: the exact top-``min(ef, 32, n_entry)`` of the entry index for prepared
        queries, as entry numbers (``entry_rows`` maps them to rows)."""
        n_seed = min(ef, GRAPH_SEEDS_MAX, self.n_entry)
        return self.entry.search_device(q, n_seed, normalize_queries=False)[1]

    def search_device(self, queries: torch.Tensor, k: int, *, ef: Optional[int] = None, width: Optional[int] = None,
                      max_iterations: Optional[int] = None, allow=None, normalize_queries: Optional[bool] = None,
                      seeds: Optional[torch.Tensor] = None, return_iterations: bool = False):
        """Beam search for device-resident queries; returns device tensors ``(scores [nq, k], ids [nq, k])``, padded
        with ``(-FLT_MAX, -1)`` (and the int32 ``[nq]`` iteration counts with ``return_iterations``).  Everything is
        enqueued on the current stream with no host synchronisation (``allow``, when given, should then be a prepared
        ``RowFilter``), so the call can be captured into a graph.  ``seeds``: device int64 ``[nq, <= 256]`` ROW numbers
        to start from instead of the entry index's (-1 = none)."""
        lib = _native.load()
        self._require_graph()
        k, ef, width, max_iterations = self._search_args(k, ef, width, max_iterations)
        flat = self.flat
        mask = flat.search_mask(allow)
        q = flat._prepare_queries(queries, normalize_queries, "search_device")
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        iterations = torch.zeros(nq, dtype=torch.int32, device=self.device) if return_iterations else None
        if nq:
            if seeds is None:
                seeds, seed_rows = self.seeds_device(q, ef), self.entry_rows
            else:
                if seeds.dtype != torch.int64 or seeds.dim() != 2 or seeds.shape[0] != nq or not seeds.is_cuda:
                    raise ValueError(f"seeds: expected a device int64 [{nq}, n] tensor")
                seeds, seed_rows = seeds.contiguous(), None
            _native.check(lib.sskd_graph_search(
                flat._tiled.data_ptr(), flat.ntotal, self.graph.data_ptr(), self.M, q.data_ptr(), nq, seeds.data_ptr(),
                seeds.shape[1], None if seed_rows is None else seed_rows.data_ptr(),
                0 if seed_rows is None else seed_rows.numel(), k, ef, width, max_iterations, flat.id_offset,
                None if mask is None else mask.data_ptr(), scores.data_ptr(), ids.data_ptr(),
                None if iterations is None else iterations.data_ptr(), _native.current_stream_ptr(self.device)))
        return (scores, ids, iterations) if return_iterations else (scores, ids)

    def search(self, query_emb: np.ndarray, k: int = 10, *, ef: Optional[int] = None, width: Optional[int] = None,
               max_iterations: Optional[int] = None, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(distances, indices)`` in ``FAISSIndexBuilder.search``'s form, over the rows the beam search reaches."""
        qd = _host_queries_to_device(query_emb, self.device)
        with torch.cuda.device(self.device):
            scores, ids = self.search_device(qd, k, ef=ef, width=width, max_iterations=max_iterations, allow=allow)
            self.last_search_path = "graph"
            return scores.cpu().numpy(), ids.cpu().numpy()

    def validate(self, num_queries: int = 1000, k: int = 10, seed: int = 0, ef: Optional[int] = None,
                 width: Optional[int] = None) -> float:
        return super().validate(num_queries, k, seed, ef=ef, width=width)

    # ------------------------------------------------------------------ persistence
    def save(self, output_dir: Union[str, Path]) -> None:
        """The flat index's files as ``FAISSIndexBuilder.save`` writes them, plus ``graph.npy``,
        ``graph_entry_rows.npy`` and ``graph.json``."""
        self._require_graph()
        self.flat.save(output_dir)
        meta = {"knn_k": self.knn_k, "ef": self.ef, "width": self.width}
        if self.n_inserted:
            meta["n_inserted"] = int(self.n_inserted)   # an optional key: absent = 0
        save_graph(output_dir, self.graph_numpy(), self.entry_rows_numpy(), meta)

    def load(self, index_dir: Union[str, Path]) -> None:
        """Restore a saved graph index: its searches return the bits they returned before the save."""
        self.flat.load(index_dir)
        self.load_graph(index_dir)

    def load_graph(self, index_dir: Union[str, Path]) -> None:
        """The graph files of ``index_dir`` over the rows ``self.flat`` already holds."""
        graph, entry_rows, meta = load_graph(index_dir)
        if graph.shape[0] != self.flat.ntotal:
            raise ValueError(f"{index_dir}: a graph over {graph.shape[0]} rows, the index holds {self.flat.ntotal}")
        self._from_host(graph, entry_rows)
        self.knn_k = meta.get("knn_k")
        self.ef = int(meta.get("ef", self.ef))
        self.width = int(meta.get("width", self.width))
        self.n_inserted = int(meta.get("n_inserted", 0))

    def cleanup(self) -> None:
        self.flat.cleanup()
        self.entry.cleanup()
        self.graph = self.entry_rows = None
        self._n_linked = self.n_inserted = 0
