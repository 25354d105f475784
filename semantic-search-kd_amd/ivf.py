"""``IVFIndex``: inverted lists over the unchanged flat index, nprobe search with exact scores.

The reference's ``configs/index.yaml`` names three index types - ``hnsw``, ``ivf_pq`` ("for >50M vectors", with
``nlist`` / ``nprobe``) and ``flat`` - and a validation gate (``recall_threshold: 0.97`` against brute force).  This is
the IVF half over uncompressed rows; the PQ half (``m`` / ``nbits``) is ``pq.IVFPQIndex``, which subclasses this index.

* The rows are a ``FAISSIndexBuilder`` (``ivf.flat``), not permuted and not copied; the lists are a CSR over row numbers
  in HBM (``list_offsets`` int64 ``[nlist + 1]``, ``list_rows`` int32 ``[ntotal]``, ascending within a list) and the
  centroids a second small ``FAISSIndexBuilder`` (``ivf.quantizer``, inner product).  Everything keyed by row id -
  ``allow`` filters, ``remove_ids``, ``doc_ids``, groups, ``reconstruct`` and the flat index's exact ``search``,
  ``range_search``, ``search_grouped`` and ``mine_negatives`` (``ivf.flat.*``) - keeps working on the same ids.
* WHICH rows a query looks at is approximate; every score and every order is exact: ``search(q, k, nprobe=p)`` returns
  bit for bit what ``flat.search(q, k, allow=<rows of the p probed lists>)`` returns, and with ``nprobe >= nlist`` what
  ``flat.search(q, k)`` returns (``include/sskd_amd.h``, "IVF index").
* ``train`` is a spherical k-means on the device, deterministic: assignment is the exact top-1 search over the
  centroids, the update adds each list's rows in CSR order in fp64 (``sskd_ivf_list_sums``).
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native
from .index import FAISSIndexBuilder, IndexHandle, _host_queries_to_device
from .overlay import FlatOverlay, read_versioned_json, recall_at_k  # noqa: F401  (recall_at_k: callers import it from here)

IVF_K_MAX = 256
IVF_NLIST_MAX = 65536
IVF_MAX_BATCH = 65535          # queries per sskd_ivf_search call
FORMAT_VERSION = 1


# ------------------------------------------------------------------ host-side list arithmetic (NumPy, no GPU)
def default_nlist(n: int) -> int:
    """``max(1, round(sqrt(n)))``, at most 65 536."""
    return int(min(IVF_NLIST_MAX, max(1, round(float(np.sqrt(max(int(n), 0)))))))


def csr_from_assignment(assignment, nlist: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(list_offsets int64 [nlist + 1], list_rows int32 [n])`` of an assignment ``row -> list``: every row once,
    ascending within a list (a stable sort of the assignment), an empty list as two equal offsets."""
    a = np.asarray(assignment).reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError("assignment must hold integer list numbers")
    a = a.astype(np.int64)
    if nlist < 1 or nlist > IVF_NLIST_MAX:
        raise ValueError(f"nlist={nlist} outside [1, {IVF_NLIST_MAX}]")
    if a.size and (a.min() < 0 or a.max() >= nlist):
        raise ValueError(f"assignment outside [0, {nlist})")
    offsets = np.zeros(nlist + 1, dtype=np.int64)
    np.cumsum(np.bincount(a, minlength=nlist), out=offsets[1:])
    return offsets, np.argsort(a, kind="stable").astype(np.int32)


def assignment_from_csr(list_offsets: np.ndarray, list_rows: np.ndarray) -> np.ndarray:
    """The inverse of ``csr_from_assignment``: int64 list number of every row."""
    offsets = np.asarray(list_offsets, dtype=np.int64)
    rows = np.asarray(list_rows, dtype=np.int64)
    out = np.empty(rows.size, dtype=np.int64)
    out[rows] = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    return out


def check_csr(list_offsets: np.ndarray, list_rows: np.ndarray, n_rows: int) -> None:
    """Raises ``ValueError`` unless the CSR holds every row of ``range(n_rows)`` exactly once, ascending per list."""
    offsets = np.asarray(list_offsets)
    rows = np.asarray(list_rows)
    if offsets.ndim != 1 or offsets.size < 2 or offsets[0] != 0 or offsets[-1] != n_rows or (np.diff(offsets) < 0).any():
        raise ValueError(f"list_offsets must rise from 0 to {n_rows}")
    if rows.shape != (n_rows,) or not np.array_equal(np.sort(rows), np.arange(n_rows)):
        raise ValueError("list_rows must hold every row exactly once")
    inner = np.ones(n_rows, dtype=np.bool_)
    inner[offsets[1:-1][offsets[1:-1] < n_rows]] = False   # a list's first entry may be lower than the one before it
    if n_rows > 1 and ((np.diff(rows.astype(np.int64)) <= 0) & inner[1:]).any():
        raise ValueError("list_rows must ascend within every list")


def remap_lists(list_offsets: np.ndarray, list_rows: np.ndarray, kept: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The CSR after ``compact``: ``kept`` = the surviving OLD local rows, ascending.  Dropped rows leave their lists,
    a survivor gets its new number (its position in ``kept``), and the order inside a list stays ascending."""
    offsets = np.asarray(list_offsets, dtype=np.int64)
    rows = np.asarray(list_rows, dtype=np.int64)
    kept = np.asarray(kept, dtype=np.int64)
    new_of_old = np.full(rows.size, -1, dtype=np.int64)
    new_of_old[kept] = np.arange(kept.size, dtype=np.int64)
    mapped = new_of_old[rows]
    alive = mapped >= 0
    list_of_entry = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    new_offsets = np.zeros(offsets.size, dtype=np.int64)
    np.cumsum(np.bincount(list_of_entry[alive], minlength=offsets.size - 1), out=new_offsets[1:])
    return new_offsets, mapped[alive].astype(np.int32)


def save_lists(out_dir: Union[str, Path], centroids: np.ndarray, list_offsets: np.ndarray, list_rows: np.ndarray,
               meta: dict) -> None:
    """Writes ``ivf_centroids.npy``, ``ivf_list_offsets.npy``, ``ivf_list_rows.npy`` and ``ivf.json``."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "ivf_centroids.npy", np.ascontiguousarray(centroids, dtype=np.float32))
    np.save(out / "ivf_list_offsets.npy", np.ascontiguousarray(list_offsets, dtype=np.int64))
    np.save(out / "ivf_list_rows.npy", np.ascontiguousarray(list_rows, dtype=np.int32))
    with open(out / "ivf.json", "w") as f:
        json.dump({**meta, "nlist": int(len(list_offsets) - 1), "format_version": FORMAT_VERSION}, f)


def load_lists(index_dir: Union[str, Path]):
    """``(centroids, list_offsets, list_rows, meta)`` as ``save_lists`` wrote them; the CSR is checked."""
    d = Path(index_dir)
    meta = read_versioned_json(d / "ivf.json", FORMAT_VERSION)
    centroids = np.load(d / "ivf_centroids.npy").astype(np.float32)
    offsets = np.load(d / "ivf_list_offsets.npy").astype(np.int64)
    rows = np.load(d / "ivf_list_rows.npy").astype(np.int32)
    if centroids.ndim != 2 or centroids.shape[0] != offsets.size - 1 or int(meta["nlist"]) != offsets.size - 1:
        raise ValueError(f"{d}: {centroids.shape[0]} centroids, {offsets.size - 1} lists, nlist={meta['nlist']}")
    check_csr(offsets, rows, rows.size)
    return centroids, offsets, rows, meta


def is_ivf_dir(index_dir: Union[str, Path]) -> bool:
    return (Path(index_dir) / "ivf.json").exists()


# ------------------------------------------------------------------------------------------------ the index
class IVFIndex(FlatOverlay):
    """Inverted-file index over a ``FAISSIndexBuilder``: ``ivf.flat`` holds the rows, ``ivf.quantizer`` the centroids."""

    def __init__(self, flat: Optional[FAISSIndexBuilder] = None, embedding_dim: int = 384, metric: str = "cosine",
                 device: Optional[str] = None, nlist: Optional[int] = None, nprobe: int = 32) -> None:
        super().__init__(flat if flat is not None else FAISSIndexBuilder(embedding_dim=embedding_dim, index_type="IVF",
                                                                         metric=metric, device=device))
        self.quantizer = FAISSIndexBuilder(embedding_dim=self.embedding_dim, index_type="Flat", metric="ip",
                                           device=str(self.device))
        self.nlist_requested = None if nlist is None else int(nlist)
        self.nprobe = int(nprobe)
        self.seed = 1234
        self.iterations = 0
        self.list_offsets: Optional[torch.Tensor] = None   # device int64 [nlist + 1]
        self.list_rows: Optional[torch.Tensor] = None      # device int32 [ntotal]
        self._assign: Optional[torch.Tensor] = None        # device int64 [ntotal]: the list of every row
        # host copies of what a launch needs, so that a search never reads the device back
        self.max_list_rows = 0
        self._n_listed = 0
        self._workspace: Optional[torch.Tensor] = None
        self._probe_workspace: Optional[torch.Tensor] = None
        self._all_lists = None                             # the centroids as ONE list (see _probe_by_scan)
        self.last_search_path: Optional[str] = None

    # ------------------------------------------------------------------ properties
    @property
    def nlist(self) -> int:
        return self.quantizer.ntotal

    def _require_lists(self) -> None:
        if self.list_offsets is None or self._n_listed != self.flat.ntotal:
            raise RuntimeError("the IVF lists are not built for the rows held: call train() (or build_from_embeddings / load)")

    def lists_numpy(self) -> Tuple[np.ndarray, np.ndarray]:
        """Host copies ``(list_offsets, list_rows)``."""
        self._require_lists()
        return self.list_offsets.cpu().numpy(), self.list_rows.cpu().numpy()

    def centroids_numpy(self) -> np.ndarray:
        return self.quantizer.to_numpy()

    # ------------------------------------------------------------------ lists
    def _set_centroids(self, centroids: torch.Tensor) -> None:
        self.quantizer.build_from_embeddings(centroids.contiguous())   # metric "ip": stored as given

    def _assign_device(self, rows: torch.Tensor, batch: int = 1 << 16) -> torch.Tensor:
        """List of every row of ``rows`` (device fp32 ``[m, dim]``): the exact top-1 search over the centroids, ties
        to the lower list (the search's rank order).  Device int64 ``[m]``."""
        out = torch.empty(rows.shape[0], dtype=torch.int64, device=self.device)
        for lo in range(0, rows.shape[0], batch):
            part = rows[lo: lo + batch]
            _, ids = self.quantizer.search_device(part, 1, normalize_queries=False)
            out[lo: lo + part.shape[0]] = ids[:, 0]
        return out

    def _csr_device(self, assign: torch.Tensor, row_numbers: Optional[torch.Tensor], nlist: int):
        """Device CSR of an assignment (stable sort: rows ascend within a list).  ``row_numbers``: the row of every
        entry of ``assign`` (ascending; None: entry i is row i).  Returns ``(offsets, rows, counts)``."""
        order = torch.sort(assign, stable=True).indices
        rows = (order if row_numbers is None else row_numbers[order]).to(torch.int32).contiguous()
        counts = torch.bincount(assign, minlength=nlist)
        offsets = torch.zeros(nlist + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(counts, 0, out=offsets[1:])
        return offsets, rows, counts

    def _install(self, assign: torch.Tensor) -> None:
        """Build the final CSR from the assignment of ALL rows; one read-back of the longest list."""
        nlist = self.nlist
        self._assign = assign.contiguous()
        self.list_offsets, self.list_rows, counts = self._csr_device(self._assign, None, nlist)
        self.max_list_rows = int(counts.max().item()) if assign.numel() else 0
        self._n_listed = int(assign.numel())

    def list_sums_device(self, list_offsets: torch.Tensor, list_rows: torch.Tensor) -> torch.Tensor:
        """``sskd_ivf_list_sums`` over the flat rows: device fp64 ``[nlist, dim]``."""
        lib = _native.load()
        nlist = list_offsets.numel() - 1
        sums = torch.empty((nlist, self.embedding_dim), dtype=torch.float64, device=self.device)
        _native.check(lib.sskd_ivf_list_sums(
            self.flat._tiled.data_ptr(), self.flat.ntotal, list_offsets.data_ptr(),
            list_rows.data_ptr() if list_rows.numel() else None, nlist, sums.data_ptr(),
            _native.current_stream_ptr(self.device)))
        return sums

    def train(self, nlist: Optional[int] = None, iterations: int = 10, seed: int = 1234,
              max_train_rows: Optional[int] = None) -> None:
        """Spherical k-means on the device, deterministic.  The training sample is ``min(ntotal, max_train_rows)``
        rows spread evenly over the index (default ``256 * nlist``); the first centroids are the sample rows
        ``sorted(default_rng(seed).permutation(n_train)[:nlist])``; every iteration assigns the sample (exact top-1
        over the centroids, ties to the lower list), sums every list's rows in CSR order in fp64, rounds to fp32 and
        normalises; an empty list keeps its centroid.  After the last update ALL rows are assigned and the lists built."""
        lib = _native.load()
        n = self.flat.ntotal
        if n < 1:
            raise RuntimeError("train(): the index is empty")
        if nlist is None:
            nlist = self.nlist_requested if self.nlist_requested is not None else default_nlist(n)
        nlist = int(nlist)
        if nlist < 1 or nlist > IVF_NLIST_MAX:
            raise ValueError(f"nlist={nlist} outside [1, {IVF_NLIST_MAX}]")
        if nlist > n:
            raise ValueError(f"nlist={nlist} > {n} rows")
        if iterations < 0:
            raise ValueError(f"iterations={iterations} < 0")
        n_train = min(n, 256 * nlist if max_train_rows is None else int(max_train_rows))
        if n_train < nlist:
            raise ValueError(f"max_train_rows={max_train_rows} < nlist={nlist}")
        with torch.cuda.device(self.device):
            rows = self._rows_view()
            if n_train == n:
                sample_rows, sample = None, rows
            else:
                host = (np.arange(n_train, dtype=np.int64) * n) // n_train
                sample_rows = torch.from_numpy(host).to(self.device)
                sample = rows[sample_rows]
            first = np.sort(np.random.default_rng(seed).permutation(n_train)[:nlist])
            centroids = sample[torch.from_numpy(first).to(self.device)].clone()
            self._set_centroids(centroids)
            stream = _native.current_stream_ptr(self.device)
            for _ in range(int(iterations)):
                assign = self._assign_device(sample)
                offsets, list_rows, counts = self._csr_device(assign, sample_rows, nlist)
                new = self.list_sums_device(offsets, list_rows).to(torch.float32)
                _native.check(lib.sskd_l2_normalize_rows(new.data_ptr(), nlist, self.embedding_dim, stream))
                centroids = torch.where((counts > 0)[:, None], new, centroids)
                self._set_centroids(centroids)
            self._install(self._assign_device(rows))
        self.seed, self.iterations = int(seed), int(iterations)

    @classmethod
    def from_assignment(cls, flat: FAISSIndexBuilder, centroids, assignment, nprobe: int = 32) -> "IVFIndex":
        """Lists from a caller's arrays (an externally trained quantiser): ``centroids`` fp32 ``[nlist, dim]`` stored
        as given, ``assignment`` the list of every row of ``flat``."""
        ivf = cls(flat=flat, nprobe=nprobe)
        c = np.ascontiguousarray(np.asarray(centroids, dtype=np.float32))
        if c.ndim != 2 or c.shape[1] != flat.embedding_dim or not 1 <= c.shape[0] <= IVF_NLIST_MAX:
            raise ValueError(f"expected [1 .. {IVF_NLIST_MAX}, {flat.embedding_dim}] centroids, got {c.shape}")
        a = np.asarray(assignment).reshape(-1)
        if a.size != flat.ntotal:
            raise ValueError(f"{a.size} assignments for {flat.ntotal} rows")
        offsets, rows = csr_from_assignment(a, c.shape[0])
        ivf._from_host(c, offsets, rows)
        return ivf

    def _from_host(self, centroids: np.ndarray, offsets: np.ndarray, rows: np.ndarray) -> None:
        with torch.cuda.device(self.device):
            self._set_centroids(torch.from_numpy(centroids).to(self.device))
            self.list_offsets = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64)).to(self.device)
            self.list_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(self.device)
            self._assign = torch.from_numpy(assignment_from_csr(offsets, rows)).to(self.device)
        self.max_list_rows = int(np.diff(offsets).max()) if offsets.size > 1 else 0
        self._n_listed = int(rows.size)

    # ------------------------------------------------------------------ building / mutation
    def build_from_embeddings(self, embeddings, nlist: Optional[int] = None, groups: Optional[Sequence] = None,
                              doc_ids: Optional[Sequence[str]] = None, iterations: int = 10, seed: int = 1234) -> IndexHandle:
        """Add, train and assign."""
        handle = self.flat.build_from_embeddings(embeddings, doc_ids=doc_ids, groups=groups)
        self.train(nlist=nlist, iterations=iterations, seed=seed)
        return handle

    def build_from_parquet(self, model, parquet_path, nlist: Optional[int] = None, iterations: int = 10, seed: int = 1234,
                           **flat_args) -> IndexHandle:
        """``FAISSIndexBuilder.build_from_parquet`` (its arguments pass through), then train and assign."""
        handle = self.flat.build_from_parquet(model=model, parquet_path=parquet_path, **flat_args)
        self.train(nlist=nlist, iterations=iterations, seed=seed)
        return handle

    def add(self, embeddings, groups: Optional[Sequence] = None) -> None:
        """Flat add, then the new rows join the lists of the EXISTING centroids (no retraining)."""
        self._require_lists()
        first = self.flat.ntotal
        self.flat.add(embeddings, groups=groups)
        if self.flat.ntotal == first:
            return
        with torch.cuda.device(self.device):
            new = self._assign_device(self._rows_view()[first:])
            self._install(torch.cat([self._assign, new]))

    def compact(self) -> np.ndarray:
        """The flat ``compact()``, then the lists are remapped through the returned ``kept`` (``remap_lists``)."""
        self._require_lists()
        offsets, rows = self.lists_numpy()
        kept = self.flat.compact()
        new_offsets, new_rows = remap_lists(offsets, rows, kept - self.flat.id_offset)
        self._from_host(self.centroids_numpy(), new_offsets, new_rows)
        return kept

    # ------------------------------------------------------------------ search
    def _nprobe(self, nprobe: Optional[int]) -> int:
        p = self.nprobe if nprobe is None else int(nprobe)
        if p < 1:
            raise ValueError(f"nprobe={p} < 1")
        return min(p, self.nlist)

    # The online shape, a handful of queries and 11 .. 32 lists: the coarse search's merge is one wave doing nprobe rounds
    # over the 64 x 32 entries a 1 024-row scan leaves (0.35 ms, more than the exact search over 1 M rows), so the probe
    # runs the list scan itself over the centroids as ONE list of nlist rows - the same fma chain and rank order, hence
    # the same lists in the same order (DESIGN section 18 has the timings on both sides of these bounds).
    PROBE_SCAN_MAX_NQ = 64
    PROBE_SCAN_NPROBE = (11, 32)

    def _probe_by_scan(self, q: torch.Tensor, nprobe: int) -> Tuple[torch.Tensor, torch.Tensor]:
        lib = _native.load()
        nq, nlist, quant = q.shape[0], self.nlist, self.quantizer
        if self._all_lists is None or self._all_lists[1].numel() != nlist:
            self._all_lists = (torch.tensor([0, nlist], dtype=torch.int64, device=self.device),
                               torch.arange(nlist, dtype=torch.int32, device=self.device),
                               torch.zeros((self.PROBE_SCAN_MAX_NQ, 1), dtype=torch.int64, device=self.device))
        offsets, rows, zero = self._all_lists
        scores = torch.empty((nq, nprobe), dtype=torch.float32, device=self.device)
        ids = torch.empty((nq, nprobe), dtype=torch.int64, device=self.device)
        need = int(lib.sskd_ivf_search_workspace_bytes(nq, 1, nprobe, nlist, nlist))
        self._probe_workspace = _native.grown(self._probe_workspace, need, self.device)
        _native.check(lib.sskd_ivf_search(
            quant._tiled.data_ptr(), nlist, q.data_ptr(), nq, zero.data_ptr(), 1, offsets.data_ptr(), rows.data_ptr(), 1,
            nprobe, 0, None, scores.data_ptr(), ids.data_ptr(), self._probe_workspace.data_ptr(), need,
            _native.current_stream_ptr(self.device)))
        return scores, ids

    def _probe_scored(self, q: torch.Tensor, nprobe: int, want_scores: bool = True):
        """``(scores or None, lists)`` of the probe: the scores are the coarse search's own fp32 bits (the fma chain
        over the centroid rows).  Probing every one of more than 1 024 lists has no search behind it; its scores, when
        asked for, come from ``sskd_similarity`` (the same chain)."""
        lo, hi = self.PROBE_SCAN_NPROBE
        if 1 <= q.shape[0] <= self.PROBE_SCAN_MAX_NQ and lo <= nprobe <= hi:
            return self._probe_by_scan(q, nprobe)
        if nprobe <= _native.SSKD_K_MAX:
            return self.quantizer.search_device(q, nprobe, normalize_queries=False)
        if nprobe < self.nlist:
            raise ValueError(f"nprobe={nprobe}: a partial probe takes at most {_native.SSKD_K_MAX} lists")
        ids = torch.arange(self.nlist, dtype=torch.int64, device=self.device).expand(q.shape[0], -1).contiguous()
        if not want_scores:
            return None, ids
        scores = torch.empty((q.shape[0], self.nlist), dtype=torch.float32, device=self.device)
        _native.check(_native.load().sskd_similarity(q.data_ptr(), q.shape[0], self.quantizer._tiled.data_ptr(), self.nlist,
                                                     self.embedding_dim, scores.data_ptr(),
                                                     _native.current_stream_ptr(self.device)))
        return scores, ids

    def _probe_prepared(self, q: torch.Tensor, nprobe: int) -> torch.Tensor:
        return self._probe_scored(q, nprobe, want_scores=False)[1]

    def probe_device(self, queries: torch.Tensor, nprobe: Optional[int] = None,
                     normalize_queries: Optional[bool] = None) -> torch.Tensor:
        """The lists every query probes: device int64 ``[nq, min(nprobe, nlist)]``, best centroid first - the exact
        top-``nprobe`` search over the centroids (every list, in list order, when ``nprobe >= nlist > 1024``).  Up to 64
        queries probing 11 .. 32 lists get the same lists from the list scan run over the centroids themselves."""
        self._require_lists()
        q = self.flat._prepare_queries(queries, normalize_queries, "probe_device")
        return self._probe_prepared(q, self._nprobe(nprobe))

    def search_device(self, queries: torch.Tensor, k: int, *, nprobe: Optional[int] = None, allow=None,
                      normalize_queries: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Top-k over the rows of the probed lists for device-resident queries; returns device tensors ``(scores
        [nq, k], ids [nq, k])``, padded with ``(-FLT_MAX, -1)``.  Everything is enqueued on the current stream with no
        host synchronisation (``allow``, when given, should then be a prepared ``RowFilter``), so the call can be
        captured into a graph.  The IVF kernel runs whatever ``nprobe`` is - also when every list is probed."""
        lib = _native.load()
        self._require_lists()
        k = int(k)
        if k < 1 or k > IVF_K_MAX:
            raise ValueError(f"k={k} outside [1, {IVF_K_MAX}]")
        flat = self.flat
        nprobe = self._nprobe(nprobe)
        mask = flat.search_mask(allow)
        q = flat._prepare_queries(queries, normalize_queries, "search_device")
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        n = flat.ntotal
        stream = _native.current_stream_ptr(self.device)
        for lo in range(0, nq, IVF_MAX_BATCH):
            qb = q[lo: lo + IVF_MAX_BATCH]
            b = qb.shape[0]
            probe = self._probe_prepared(qb, nprobe)
            need = int(lib.sskd_ivf_search_workspace_bytes(b, nprobe, k, n, self.max_list_rows))
            self._workspace = _native.grown(self._workspace, need, self.device)
            _native.check(lib.sskd_ivf_search(
                flat._tiled.data_ptr(), n, qb.data_ptr(), b, probe.data_ptr(), nprobe, self.list_offsets.data_ptr(),
                self.list_rows.data_ptr(), self.nlist, k, flat.id_offset, None if mask is None else mask.data_ptr(),
                scores[lo: lo + b].data_ptr(), ids[lo: lo + b].data_ptr(), self._workspace.data_ptr(), need, stream))
        return scores, ids

    def search(self, query_emb: np.ndarray, k: int = 10, *, nprobe: Optional[int] = None, allow=None
               ) -> Tuple[np.ndarray, np.ndarray]:
        """``(distances, indices)`` in ``FAISSIndexBuilder.search``'s form, over the rows of the probed lists."""
        qd = _host_queries_to_device(query_emb, self.device)
        with torch.cuda.device(self.device):
            scores, ids = self.search_device(qd, k, nprobe=nprobe, allow=allow)
            self.last_search_path = "ivf"
            return scores.cpu().numpy(), ids.cpu().numpy()

    def validate(self, num_queries: int = 1000, k: int = 10, seed: int = 0, nprobe: Optional[int] = None) -> float:
        return super().validate(num_queries, k, seed, nprobe=nprobe)

    # ------------------------------------------------------------------ persistence
    def save(self, output_dir: Union[str, Path]) -> None:
        """The flat index's files as ``FAISSIndexBuilder.save`` writes them, plus ``ivf_centroids.npy``,
        ``ivf_list_offsets.npy``, ``ivf_list_rows.npy`` and ``ivf.json``."""
        self._require_lists()
        self.flat.save(output_dir)
        offsets, rows = self.lists_numpy()
        save_lists(output_dir, self.centroids_numpy(), offsets, rows,
                   {"nprobe": self.nprobe, "seed": self.seed, "iterations": self.iterations})

    def load(self, index_dir: Union[str, Path]) -> None:
        """Restore a saved IVF index: its searches return the bits they returned before the save."""
        self.flat.load(index_dir)
        self.load_lists(index_dir)

    def load_lists(self, index_dir: Union[str, Path]) -> None:
        """The IVF files of ``index_dir`` over the rows ``self.flat`` already holds."""
        centroids, offsets, rows, meta = load_lists(index_dir)
        if rows.size != self.flat.ntotal or centroids.shape[1] != self.embedding_dim:
            raise ValueError(f"{index_dir}: lists over {rows.size} rows, the index holds {self.flat.ntotal}")
        self._from_host(centroids, offsets, rows)
        self.nprobe = int(meta.get("nprobe", self.nprobe))
        self.seed = int(meta.get("seed", self.seed))
        self.iterations = int(meta.get("iterations", self.iterations))

    def cleanup(self) -> None:
        self.flat.cleanup()
        self.quantizer.cleanup()
        self.list_offsets = self.list_rows = self._assign = self._workspace = self._probe_workspace = None
        self._all_lists = None
        self.max_list_rows = self._n_listed = 0
