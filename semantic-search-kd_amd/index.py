"""``FAISSIndexBuilder``-shaped index backed by the gfx950 exact top-k scan.

Mirrors the (absent-from-checkout) reference class ``src.index.build_index.FAISSIndexBuilder``
as reconstructed from its call sites:

* ctor ``(embedding_dim=384, index_type="HNSW", metric="cosine")`` — scripts/build_faiss_index.py:49-53,
  src/serve/app.py:427-429
* ``build_from_parquet(model=, parquet_path=, batch_size=, max_docs=, hnsw_m=, hnsw_ef_construction=)``
  returning an object with ``.ntotal`` — scripts/build_faiss_index.py:55-62,72
* ``search(query_emb, k) -> (distances[nq,k] f32 desc, indices[nq,k] i64, -1 padded)`` — src/serve/app.py:293-301
* ``save(dir)`` / ``load(dir)`` with ``index.faiss`` + ``doc_ids.json`` (+ ``texts.json`` read by the app) —
  scripts/build_faiss_index.py:66, src/serve/app.py:430-442, tests/conftest.py:188-198
* ``.doc_ids`` — src/serve/app.py:433

The reference builds an approximate HNSW graph; this backend answers with the
*exact* inner-product top-k (what the reference checks HNSW against: recall@10 >= 0.97,
configs/index.yaml:51-56), so ``index_type`` and the HNSW knobs are accepted and ignored.
All arithmetic runs in hand-written HIP kernels through the C-ABI; there is no CPU path.
"""
from __future__ import annotations

import json
import struct
from pathlib import Path
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native

_FLAT_IP_FOURCC = b"IxFI"
_FAISS_DUMMY = 1 << 20
_METRIC_INNER_PRODUCT = 0


class RowFilter:
    """A prepared per-call filter: the device allow-mask of ``n_rows`` rows (``include/sskd_amd.h``: int32 words,
    bit ``r & 31`` of word ``r >> 5`` set = local row ``r`` may be returned).  Made by ``FAISSIndexBuilder.row_filter``;
    reusable, and ``search_device`` with it makes no host synchronisation (safe under graph capture)."""

    def __init__(self, words: torch.Tensor, n_rows: int):
        self.words = words
        self.n_rows = int(n_rows)


def mask_words(allow, n_rows: int) -> np.ndarray:
    """Host-side normalisation of a filter: a bool array over ``n_rows`` rows, or an integer array of allowed local
    rows -> the little-endian uint32 mask words (``np.packbits(..., bitorder="little")``, padded to whole words)."""
    a = np.asarray(allow)
    if a.dtype == np.bool_:
        if a.shape != (n_rows,):
            raise ValueError(f"a boolean filter needs one entry per row: shape {a.shape}, index has {n_rows} rows")
        flags = a
    elif a.dtype.kind in "iu" or a.size == 0:
        rows = a.astype(np.int64).ravel()
        if rows.size and (rows.min() < 0 or rows.max() >= n_rows):
            raise ValueError(f"filter rows outside [0, {n_rows})")
        flags = np.zeros(n_rows, dtype=np.bool_)
        flags[rows] = True
    else:
        raise TypeError(f"a filter is a bool array or an integer id array, got dtype {a.dtype}")
    n_words = -(-n_rows // 32)
    packed = np.zeros(4 * n_words, dtype=np.uint8)
    bits = np.packbits(flags, bitorder="little")
    packed[: bits.size] = bits
    return packed.view("<u4")


class IndexHandle:
    """What ``build_from_parquet`` returns: the reference only reads ``.ntotal`` (build_faiss_index.py:72)."""

    def __init__(self, owner: "FAISSIndexBuilder"):
        self._owner = owner

    def remove_ids(self, ids) -> int:
        return self._owner.remove_ids(ids)

    def compact(self) -> np.ndarray:
        return self._owner.compact()

    @property
    def ntotal(self) -> int:
        return self._owner.ntotal

    @property
    def d(self) -> int:
        return self._owner.embedding_dim

    def search(self, x: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """faiss ``index.search`` shape: raw inner product, no query normalisation."""
        return self._owner._search_numpy(x, k, normalize_queries=False)

    def range_search(self, x: np.ndarray, thresh) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """faiss ``index.range_search`` shape ``(lims, D, I)``: raw inner product, no query normalisation."""
        return self._owner._range_numpy(x, thresh, normalize_queries=False)

    def search_grouped(self, x: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``(D, I, G)``: the top-k distinct groups by their best row; raw inner product, no query normalisation."""
        return self._owner._search_grouped_numpy(x, k, normalize_queries=False)


class FAISSIndexBuilder:
    """Exact cosine / inner-product index resident in MI355X HBM."""

    def __init__(
        self,
        embedding_dim: int = 384,
        index_type: str = "HNSW",
        metric: str = "cosine",
        device: Optional[str] = None,
        id_offset: int = 0,
    ) -> None:
        if embedding_dim != _native.SSKD_DIM:
            raise ValueError(
                f"embedding_dim={embedding_dim}: the gfx950 scan kernel is specialised for "
                f"{_native.SSKD_DIM}-d embeddings (e5-small-v2)"
            )
        metric = metric.lower()
        if metric not in ("cosine", "ip", "inner_product", "dot"):
            raise ValueError(f"metric={metric!r}: only cosine / inner product are supported")
        self.embedding_dim = embedding_dim
        self.index_type = index_type
        self.metric = "cosine" if metric == "cosine" else "ip"
        self.device = _resolve_device(device)
        self.doc_ids: List[str] = []
        self.doc_texts: Optional[dict] = None
        self.id_offset = int(id_offset)  # global id of local row 0 (row-sharded corpora)
        self.shard_info: Optional[dict] = None  # {"rank", "world_size", "n_total"} when written by build_sharded
        self._tiled: Optional[torch.Tensor] = None  # fp32 [capacity_rows * 384], tiled layout
        self._n = 0
        self._workspace: Optional[torch.Tensor] = None
        self.last_search_path: Optional[str] = None  # which path the last host search() took (diagnostic)
        # explicit launch tuning (``_native.SearchTuning``) handed to BOTH the workspace query and the
        # search call; ``None`` = the built-in plan.  There is no environment knob behind the search.
        self.search_tuning: Optional[_native.SearchTuning] = None
        # batch searches (k <= 10, >= 64 queries) go through the bf16-screened path: identical bits to
        # the exact scan (measured + proved error band, exact re-scoring, in-call exact fallback sized for
        # every query - no caller ever has to check a status), several times faster.
        # ``screening = False`` forces the plain exact scan.
        self.screening = True
        self._bf16: Optional[torch.Tensor] = None      # screening sidecar (bf16 tiles of the centred rows + norm block: 768 B per row), made lazily
        self._bf16_rows = -1
        # device int32[2] of the last screened search: [0] always 0, [1] = queries that took the in-call
        # exact fallback (a cost diagnostic; nothing to act on)
        self.last_status: Optional[torch.Tensor] = None
        self.index: Optional[IndexHandle] = None
        # tombstones (remove_ids): the device allow-mask of the LIVE rows (made on the first removal; bits past ntotal
        # stay set, so rows added later are live) and how many rows it clears
        self._live: Optional[torch.Tensor] = None
        self._n_removed = 0
        self._mask_scratch: Optional[torch.Tensor] = None   # allow AND live of a filtered call
        # range search: result buffers reused across calls (grown to the exact total when a call overflows them)
        self.range_capacity = 1 << 16
        self._range_scores: Optional[torch.Tensor] = None
        self._range_ids: Optional[torch.Tensor] = None
        # duplicate_clusters: result entries (12 B each) every batch of the self-join gets; a batch that needs more runs again
        self.dedup_capacity = 1 << 20
        # row groups (grouped search: a document = the group of its chunks).  ``group_keys`` is None until groups are
        # set: every row is then its own group, numbered by its row.
        self.group_keys: Optional[List] = None              # group number -> key (None for a row added without one)
        self._row_group_host: Optional[np.ndarray] = None    # int32 per row
        self._group_of_key: dict = {}
        self._row_group_dev: Optional[torch.Tensor] = None   # device int32 per row, made lazily
        self._group_csr: Optional[Tuple[np.ndarray, np.ndarray]] = None   # host CSR group -> rows, made lazily
        self._max_group: Optional[int] = None
        # device int32 tensors of the last search_grouped_device call: entries written per query, and the number of
        # unproved queries
        self.last_group_counts: Optional[torch.Tensor] = None
        self.last_group_n_unproved: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ storage
    @property
    def ntotal(self) -> int:
        """Stored rows, removed ones included (their row numbers stay valid: ``doc_ids[row]``)."""
        return self._n

    @property
    def n_removed(self) -> int:
        """Rows taken out by ``remove_ids`` (tombstones: still stored, never returned)."""
        return self._n_removed

    def _reset_removed(self) -> None:
        self._live = None
        self._n_removed = 0
        self._mask_scratch = None

    def _ensure_capacity(self, rows: int) -> None:
        lib = _native.load()
        need = int(lib.sskd_index_padded_rows(rows)) * self.embedding_dim
        have = 0 if self._tiled is None else self._tiled.numel()
        if need <= have:
            return
        _native.require_gpu()
        new_elems = max(need, int(have * 1.5))
        new = torch.empty(new_elems, dtype=torch.float32, device=self.device)
        if self._tiled is not None and self._n > 0:
            used = int(lib.sskd_index_padded_rows(self._n)) * self.embedding_dim
            new[:used].copy_(self._tiled[:used])
        self._tiled = new

    def reserve(self, rows: int) -> None:
        """Pre-size the HBM buffer (avoids regrowth while streaming a large corpus in)."""
        self._ensure_capacity(rows)

    def add(self, embeddings: Union[np.ndarray, torch.Tensor], groups: Optional[Sequence] = None) -> None:
        """Append rows (``faiss.normalize_L2`` + ``index.add``); host or device fp32 ``[n, 384]``.

        Rows are L2-normalised on the GPU when ``metric == "cosine"`` (configs/index.yaml:30).  ``groups``: one
        hashable key per new row (see ``set_groups``); a key the index already knows joins that group.  Rows added
        without a key (no ``groups``, or a ``None`` entry) become singleton groups.
        """
        if groups is not None:
            groups = list(groups)
            if len(groups) != len(embeddings):
                raise ValueError(f"{len(groups)} group keys for {len(embeddings)} vectors")
        first = self._n
        self._add_rows(embeddings)
        self._extend_groups(first, self._n - first, groups)

    def _add_rows(self, embeddings: Union[np.ndarray, torch.Tensor]) -> None:
        lib = _native.load()
        x = _as_device_f32(embeddings, self.device)
        if x.dim() != 2 or x.shape[1] != self.embedding_dim:
            raise ValueError(f"expected [n, {self.embedding_dim}] embeddings, got {tuple(x.shape)}")
        n_new = x.shape[0]
        if n_new == 0:
            return
        tail = self._n % _native.SSKD_TILE_ROWS
        if tail:
            # rows cannot start mid-tile: re-pack the partial tail tile together with the new
            # rows as one contiguous [tail | new] block written at the tail tile's first row
            stream = _native.current_stream_ptr(self.device)
            staged = torch.empty((tail + n_new, self.embedding_dim), dtype=torch.float32, device=self.device)
            _native.check(
                lib.sskd_index_get_rows(self._tiled.data_ptr(), self._n - tail, tail, staged.data_ptr(), stream)
            )
            staged[tail:].copy_(x)
            if self.metric == "cosine":
                _native.check(
                    lib.sskd_l2_normalize_rows(staged[tail:].data_ptr(), n_new, self.embedding_dim, stream)
                )
            self._ensure_capacity(self._n + n_new)
            _native.check(
                lib.sskd_index_add_rows(
                    staged.data_ptr(), tail + n_new, 0, self._tiled.data_ptr(), self._n - tail, stream
                )
            )
        else:
            self._ensure_capacity(self._n + n_new)
            _native.check(
                lib.sskd_index_add_rows(
                    x.data_ptr(),
                    n_new,
                    1 if self.metric == "cosine" else 0,
                    self._tiled.data_ptr(),
                    self._n,
                    _native.current_stream_ptr(self.device),
                )
            )
        self._n += n_new
        self._bf16_rows = -1  # the bf16 screening copy is stale
        if self._live is not None:
            words = int(lib.sskd_row_mask_words(self._n))
            if words > self._live.numel():   # new words all set: the appended rows are live
                grown = torch.full((max(words, self._live.numel() * 3 // 2),), -1, dtype=torch.int32, device=self.device)
                grown[: self._live.numel()].copy_(self._live)
                self._live = grown
        self.index = IndexHandle(self)

    def build_from_embeddings(
        self, embeddings: Union[np.ndarray, torch.Tensor], doc_ids: Optional[Sequence[str]] = None,
        groups: Optional[Sequence] = None,
    ) -> IndexHandle:
        """``groups``: one key per row (for example the document of every chunk), see ``set_groups``."""
        self._n = 0
        self._tiled = None
        self._reset_removed()
        self._reset_groups()
        self.add(embeddings, groups=groups)
        self.doc_ids = list(doc_ids) if doc_ids is not None else [f"doc_{i}" for i in range(self._n)]
        if len(self.doc_ids) != self._n:
            raise ValueError(f"{len(self.doc_ids)} doc_ids for {self._n} vectors")
        self.index = IndexHandle(self)
        return self.index

    def build_from_parquet(
        self,
        model,
        parquet_path: Union[str, Path],
        batch_size: int = 32,
        max_docs: Optional[int] = None,
        hnsw_m: int = 32,
        hnsw_ef_construction: int = 200,
        text_column: str = "text",
        id_column: str = "chunk_id",
        show_progress: bool = True,
        group_column: Optional[str] = None,
    ) -> IndexHandle:
        """Encode a parquet corpus with ``model.encode_documents`` and index it.

        ``group_column``: a column whose value is the group key of every row, such as ``"doc_id"`` (the reference's
        corpus schema carries it beside ``chunk_id``): ``search_grouped`` then returns distinct documents.

        Columns follow the reference's corpus schema (src/data/prepare.py:72-84,
        tests/conftest.py:210-216): ``text`` and ``chunk_id``.  ``hnsw_*`` are accepted for
        CLI compatibility (scripts/build_faiss_index.py:59-61); an exact scan has no graph.
        """
        del hnsw_m, hnsw_ef_construction
        ids, texts = read_corpus_parquet(parquet_path, max_docs, text_column, id_column)
        keys = None if group_column is None else read_parquet_column(parquet_path, group_column, max_docs)
        self._n = 0
        self._tiled = None
        self._reset_removed()
        self._reset_groups()
        self.reserve(len(texts))
        # stream in slabs so a multi-million-passage corpus never needs one host matrix
        slab = max(batch_size, 65536)
        on_device = getattr(model, "encode_documents_device", None)   # embeddings go encoder -> index tiles inside HBM
        for lo in range(0, len(texts), slab):
            if on_device is not None:
                embs = on_device(texts[lo : lo + slab], batch_size=batch_size)
            else:
                embs = model.encode_documents(texts[lo : lo + slab], batch_size=batch_size, show_progress=show_progress)
            self.add(embs, groups=None if keys is None else keys[lo : lo + slab])
        self.doc_ids = ids
        self.doc_texts = dict(zip(ids, texts))
        self.index = IndexHandle(self)
        return self.index

    # ------------------------------------------------------------------- groups
    def _reset_groups(self) -> None:
        self.group_keys = None
        self._row_group_host = None
        self._group_of_key = {}
        self._groups_changed()

    def _groups_changed(self) -> None:
        self._row_group_dev = None
        self._group_csr = None
        self._max_group = None

    def _extend_groups(self, n_old: int, n_new: int, keys: Optional[Sequence]) -> None:
        """Group numbers of ``n_new`` rows appended behind ``n_old``: a known key joins its group, a new key opens
        one, no key (``keys`` None or a None entry) opens a singleton group."""
        self._groups_changed()
        if keys is None and self.group_keys is None:
            return   # still ungrouped: every row is its own group
        if self.group_keys is None:   # the rows stored so far become singleton groups
            self.group_keys = [None] * n_old
            self._row_group_host = np.arange(n_old, dtype=np.int32)
        new = np.empty(n_new, dtype=np.int32)
        if keys is None:
            new[:] = np.arange(len(self.group_keys), len(self.group_keys) + n_new, dtype=np.int32)
            self.group_keys.extend([None] * n_new)
        else:
            for i, key in enumerate(keys):
                g = None if key is None else self._group_of_key.get(key)
                if g is None:
                    g = len(self.group_keys)
                    self.group_keys.append(key)
                    if key is not None:
                        self._group_of_key[key] = g
                new[i] = g
        self._row_group_host = np.concatenate([self._row_group_host, new])

    def set_groups(self, keys: Sequence) -> None:
        """Group the stored rows: ``keys`` holds one hashable per row (for example the ``doc_id`` of every chunk);
        rows with equal keys form one group, a ``None`` entry makes its row a singleton group.  Group numbers follow
        first appearance; ``group_keys[g]`` is the key of group ``g``.  Replaces any earlier grouping."""
        keys = list(keys)
        if len(keys) != self._n:
            raise ValueError(f"{len(keys)} group keys for {self._n} rows")
        self._reset_groups()
        self.group_keys, self._row_group_host = [], np.zeros(0, dtype=np.int32)
        self._extend_groups(0, self._n, keys)

    @property
    def n_groups(self) -> int:
        return self._n if self.group_keys is None else len(self.group_keys)

    @property
    def max_group_size(self) -> int:
        """Rows of the largest group (1 without groups)."""
        if self._max_group is None:
            g = self._row_group_host
            self._max_group = 1 if g is None or g.size == 0 else int(np.bincount(g).max())
        return self._max_group

    def group_key(self, g):
        """The key of group ``g``, or the list of keys of an array of group numbers (``G`` of ``search_grouped``, any
        shape, flattened row by row into nested lists).  Padding (-1), a singleton group without a key and every
        group of an index without groups give None."""
        if np.ndim(g) == 0:
            g = int(g)
            return None if g < 0 or self.group_keys is None else self.group_keys[g]
        return [self.group_key(x) for x in np.asarray(g)]

    def row_groups(self) -> np.ndarray:
        """int32 group number of every stored row."""
        if self._row_group_host is None:
            return np.arange(self._n, dtype=np.int32)
        return self._row_group_host

    def _row_group_device(self) -> torch.Tensor:
        if self._row_group_dev is None or self._row_group_dev.numel() != max(self._n, 1):
            if self._row_group_host is None:
                self._row_group_dev = torch.arange(max(self._n, 1), dtype=torch.int32, device=self.device)
            else:
                host = self._row_group_host if self._n else np.zeros(1, dtype=np.int32)
                self._row_group_dev = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)
        return self._row_group_dev

    def _rows_of_groups(self, groups) -> np.ndarray:
        """Local rows (int64) of the given group numbers, from the host CSR."""
        groups = np.asarray(groups, dtype=np.int64).reshape(-1)
        if self._row_group_host is None:
            return groups.copy()
        if self._group_csr is None:
            g = self._row_group_host
            indptr = np.zeros(len(self.group_keys) + 1, dtype=np.int64)
            np.cumsum(np.bincount(g, minlength=len(self.group_keys)), out=indptr[1:])
            self._group_csr = (indptr, np.argsort(g, kind="stable").astype(np.int64))
        indptr, rows = self._group_csr
        parts = [rows[indptr[x]:indptr[x + 1]] for x in groups]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)

    # ------------------------------------------------------------ removal / filters
    def remove_ids(self, ids) -> int:
        """Take rows out of every later search (faiss ``remove_ids``).  ``ids`` are in the id space ``search``
        returns (``id_offset + row``): a list, a NumPy array or a device tensor.  Returns the number of rows newly
        removed (removing a row twice is not an error); raises ``ValueError`` for ids outside the index.  Removed
        rows keep their row numbers and stay stored (``ntotal`` counts them, ``n_removed`` counts the tombstones)."""
        lib = _native.load()
        if isinstance(ids, torch.Tensor):
            rows = ids.reshape(-1).to(device=self.device, dtype=torch.int64) - self.id_offset
            bad = bool(((rows < 0) | (rows >= self._n)).any().item()) if rows.numel() else False
        else:
            host = np.asarray(ids, dtype=np.int64).reshape(-1) - self.id_offset
            bad = bool(host.size and (host.min() < 0 or host.max() >= self._n))
            rows = None if bad else torch.from_numpy(host).to(self.device)
        if bad:
            raise ValueError(f"ids outside [{self.id_offset}, {self.id_offset + self._n})")
        if rows.numel() == 0:
            return 0
        stream = _native.current_stream_ptr(self.device)
        if self._live is None:
            self._live = torch.full((int(lib.sskd_row_mask_words(self._n)),), -1, dtype=torch.int32, device=self.device)
        rows = rows.contiguous()
        scratch = torch.zeros(2, dtype=torch.int64, device=self.device)   # [0] live count, [1] (low word) bad ids
        _native.check(lib.sskd_row_mask_update(self._live.data_ptr(), self._n, rows.data_ptr(), rows.numel(), 0,
                                               scratch[1:].data_ptr(), stream))
        _native.check(lib.sskd_row_mask_count(self._live.data_ptr(), self._n, scratch.data_ptr(), stream))
        live, bad_ids = scratch.cpu().tolist()
        if bad_ids:
            raise RuntimeError("sskd_row_mask_update reported ids outside the index after they were checked")
        removed = self._n - int(live)
        newly, self._n_removed = removed - self._n_removed, removed
        return newly

    def removed_rows(self) -> np.ndarray:
        """Local rows taken out by ``remove_ids``, sorted (int64)."""
        if self._live is None or self._n_removed == 0:
            return np.zeros(0, dtype=np.int64)
        words = self._live[: int(_native.load().sskd_row_mask_words(self._n))].cpu().numpy().view(np.uint8)
        live = np.unpackbits(words, bitorder="little")[: self._n].astype(bool)
        return np.flatnonzero(~live).astype(np.int64)

    def compact(self) -> np.ndarray:
        """Drop the rows taken out by ``remove_ids`` from HBM and renumber the rest (what faiss' flat ``remove_ids``
        does at once).  Returns ``kept``: the OLD ids (``id_offset + old row``, int64, ascending) of the surviving rows
        in their new order - new id ``id_offset + j`` was old id ``kept[j]``, so a caller remaps its own references with
        ``np.searchsorted(kept, old_id)``.  The surviving rows keep their order and their bits, so every search
        returns the same scores as before, with the ids renumbered.

        The rows move into a new buffer of exactly the size they need (the old capacity is given back), the tombstones
        are reset, ``doc_ids`` and the row groups are gathered and ``doc_texts`` loses the texts no surviving row refers
        to.  Group numbers do NOT change: a group whose rows are all gone stays as an empty group, so ``G`` values a
        caller holds stay valid.  ``id_offset`` stays.  A ``RowFilter`` prepared before the call no longer fits.
        Nothing removed: returns the identity and touches nothing.  A piece of a row-sharded build (``shard_info``
        set) raises ``ValueError``: compacting one shard alone would break the manifest's contiguous id ranges."""
        if self.shard_info:
            raise ValueError("compact(): this index is one piece of a row-sharded build (shard_info is set); compacting "
                             "one shard alone would break the contiguous id ranges of the shard manifest")
        if self._n_removed == 0:
            return self.id_offset + np.arange(self._n, dtype=np.int64)
        lib = _native.load()
        n_old = self._n
        gone = self.removed_rows()
        n_live = n_old - gone.size
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device)
            prefix = torch.empty(int(lib.sskd_row_mask_words(n_old)) + 1, dtype=torch.int64, device=self.device)
            _native.check(lib.sskd_row_mask_rank(self._live.data_ptr(), n_old, prefix.data_ptr(), stream))
            new = torch.empty(int(lib.sskd_index_padded_rows(n_live)) * self.embedding_dim, dtype=torch.float32,
                              device=self.device)
            if n_live:
                _native.check(lib.sskd_index_compact_rows(self._tiled.data_ptr(), n_old, self._live.data_ptr(),
                                                          prefix.data_ptr(), new.data_ptr(), stream))
            if int(prefix[-1].item()) != n_live:
                raise RuntimeError("sskd_row_mask_rank disagrees with the tombstone count")
        self._tiled = new   # the old buffer (and its spare capacity) goes back to the allocator
        self._n = n_live
        self._reset_removed()
        self._bf16 = None
        self._bf16_rows = -1   # the screening sidecar is stale (its mean row changes anyway)
        self.index = IndexHandle(self)
        kept = _kept_rows(n_old, gone)
        self._compact_host(kept)
        return kept + self.id_offset

    def _compact_host(self, kept: np.ndarray) -> None:
        """The host-side bookkeeping of ``compact``: ``kept`` = the surviving old local rows, ascending."""
        # ``add`` appends rows without doc ids, so the list may be shorter than the rows: the rows that have one keep it
        # (``kept`` ascends, so the gathered list still lines up with the first rows)
        n_ids = len(self.doc_ids)
        self.doc_ids = [self.doc_ids[r] for r in kept.tolist() if r < n_ids]
        if self.doc_texts is not None:
            alive = set(self.doc_ids)
            self.doc_texts = {key: text for key, text in self.doc_texts.items() if key in alive}
        if self._row_group_host is not None:
            self._row_group_host = np.ascontiguousarray(self._row_group_host[kept])
        self._groups_changed()

    def row_filter(self, allow) -> RowFilter:
        """Prepare a per-call filter over the CURRENT ``ntotal`` rows: a bool array (one entry per row), an integer
        array of allowed ids (``id_offset + row``), host or device, or a ``RowFilter`` (returned as is)."""
        if isinstance(allow, RowFilter):
            return allow
        lib = _native.load()
        n = self._n
        n_words = int(lib.sskd_row_mask_words(n))
        words = torch.zeros(max(n_words, 1), dtype=torch.int32, device=self.device)
        if isinstance(allow, torch.Tensor) and allow.is_cuda:
            stream = _native.current_stream_ptr(self.device)
            if allow.dtype == torch.bool or allow.dtype == torch.uint8:
                if allow.numel() != n:
                    raise ValueError(f"a boolean filter needs one entry per row: {allow.numel()} for {n} rows")
                flags = allow.reshape(-1).to(torch.uint8).contiguous()
                _native.check(lib.sskd_row_mask_pack(flags.data_ptr(), n, words.data_ptr(), stream))
            else:
                rows = (allow.reshape(-1).to(torch.int64) - self.id_offset).contiguous()
                bad = torch.empty(1, dtype=torch.int32, device=self.device)
                _native.check(lib.sskd_row_mask_update(words.data_ptr(), n, rows.data_ptr(), rows.numel(), 1,
                                                       bad.data_ptr(), stream))
                if int(bad.item()):
                    raise ValueError(f"filter ids outside [{self.id_offset}, {self.id_offset + n})")
        else:
            a = allow.cpu().numpy() if isinstance(allow, torch.Tensor) else np.asarray(allow)
            if a.dtype != np.bool_:
                a = a.astype(np.int64) - self.id_offset
            host = mask_words(a, n)
            if host.size:
                words[: host.size].copy_(torch.from_numpy(host.view(np.int32)))
        return RowFilter(words, n)

    def _effective_mask(self, allow) -> Optional[torch.Tensor]:
        """The device words a search must honour (``allow AND NOT removed``), or None for the unfiltered path."""
        if allow is None:
            return self._live
        f = self.row_filter(allow)
        if f.n_rows != self._n:
            raise ValueError(f"the filter was prepared for {f.n_rows} rows, the index holds {self._n}")
        if self._live is None:
            return f.words
        lib = _native.load()
        words = int(lib.sskd_row_mask_words(self._n))
        if self._mask_scratch is None or self._mask_scratch.numel() < words:
            self._mask_scratch = torch.empty(max(words, 1), dtype=torch.int32, device=self.device)
        _native.check(lib.sskd_row_mask_and(f.words.data_ptr(), self._live.data_ptr(), self._n,
                                            self._mask_scratch.data_ptr(), _native.current_stream_ptr(self.device)))
        return self._mask_scratch

    def search_mask(self, allow=None) -> Optional[torch.Tensor]:
        """The device mask words a search under ``allow`` honours (``allow AND NOT removed``; None: no row is hidden),
        for a kernel that must filter by the very mask the search used.  The tensor may be a scratch buffer that the
        next filtered call overwrites: use it in stream order, before that call."""
        return self._effective_mask(allow)

    # ------------------------------------------------------------------- search
    def search_device(
        self,
        queries: torch.Tensor,
        k: int,
        normalize_queries: Optional[bool] = None,
        out_scores: Optional[torch.Tensor] = None,
        out_ids: Optional[torch.Tensor] = None,
        allow=None,
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Top-k over the index for device-resident queries; returns device tensors.

        No host synchronisation: everything is enqueued on the current stream (``allow``, when given, should then
        be a prepared ``RowFilter``).  ``allow`` restricts the call to some rows (see ``row_filter``); removed rows
        are never returned.
        """
        mask = self._effective_mask(allow)
        return self._search_device_masked(queries, k, normalize_queries, out_scores, out_ids, mask)

    def _prepare_queries(self, queries: torch.Tensor, normalize_queries: Optional[bool], who: str) -> torch.Tensor:
        """Checks ``[nq, dim]`` float32 device queries and returns them contiguous; normalised (in a copy) when
        ``normalize_queries`` is true, or is None and the metric is cosine."""
        if queries.dim() != 2 or queries.shape[1] != self.embedding_dim:
            raise ValueError(f"expected [nq, {self.embedding_dim}] queries, got {tuple(queries.shape)}")
        if queries.dtype != torch.float32 or not queries.is_cuda:
            raise TypeError(f"{who} expects a float32 device tensor")
        q = queries.contiguous()
        if normalize_queries is None:
            normalize_queries = self.metric == "cosine"
        if normalize_queries and q.shape[0]:
            q = q.clone()
            _native.check(_native.load().sskd_l2_normalize_rows(q.data_ptr(), q.shape[0], self.embedding_dim,
                                                                _native.current_stream_ptr(self.device)))
        return q

    def _workspace_for(self, need: int) -> torch.Tensor:
        """The shared search workspace, grown to at least ``need`` bytes."""
        self._workspace = _native.grown(self._workspace, need, self.device)
        return self._workspace

    def _search_device_masked(self, queries, k, normalize_queries, out_scores, out_ids, mask, id_offset=None):
        """``id_offset``: the id of local row 0 in the ids written (None: the index's own)."""
        lib = _native.load()
        id_offset = self.id_offset if id_offset is None else int(id_offset)
        if k < 1 or k > _native.SSKD_K_MAX:
            raise ValueError(f"k={k} outside [1, {_native.SSKD_K_MAX}]")
        q = self._prepare_queries(queries, normalize_queries, "search_device")
        nq = q.shape[0]
        stream = _native.current_stream_ptr(self.device)
        mask_ptr = None if mask is None else mask.data_ptr()
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        if nq == 0:
            return out_scores, out_ids
        tuning = self.search_tuning
        if self.screening and tuning is None and self._tiled is not None:
            need = int(lib.sskd_index_search_screened_workspace_bytes(self._n, nq, k))
            if need:
                if self._bf16 is None or self._bf16_rows != self._n:
                    self._bf16 = None
                    self._bf16 = torch.empty(int(lib.sskd_index_bf16_bytes(self._n)), dtype=torch.uint8, device=self.device)
                    _native.check(lib.sskd_index_make_bf16(self._tiled.data_ptr(), self._n, self._bf16.data_ptr(), stream))
                    self._bf16_rows = self._n
                ws = self._workspace_for(need)
                self.last_status = torch.empty(2, dtype=torch.int32, device=self.device)
                _native.check(
                    lib.sskd_index_search_screened_filtered(
                        self._tiled.data_ptr(), self._bf16.data_ptr(), self._n, q.data_ptr(), nq, k, id_offset,
                        mask_ptr, out_scores.data_ptr(), out_ids.data_ptr(), self.last_status.data_ptr(),
                        ws.data_ptr(), ws.numel(), stream, None, None,
                    )
                )
                return out_scores, out_ids
        self.last_status = None
        ws = self._workspace_for(int(lib.sskd_index_search_workspace_bytes_ex(self._n, nq, k, tuning)))
        _native.check(
            lib.sskd_index_search_filtered(
                0 if self._tiled is None else self._tiled.data_ptr(), self._n, q.data_ptr(), nq, k, id_offset,
                mask_ptr, out_scores.data_ptr(), out_ids.data_ptr(), ws.data_ptr(), ws.numel(), stream, tuning, None, None,
            )
        )
        return out_scores, out_ids

    # the online shape: a handful of queries (sskd_amd.h, one-pass variant).  With a single query
    # block the shared pruning pools of the batch kernel only cost, so the pool-free one-pass
    # search is also the faster one for small k (where its proof cannot fail for k <= 10).
    ONEPASS_MAX_NQ = 64
    ONEPASS_MAX_K = 256

    def _search_onepass_device(self, q: torch.Tensor, k: int, normalize_queries: bool, mask=None):
        """One corpus pass + proof of exactness; returns ``(scores, ids, inexact_flag)`` device tensors."""
        lib = _native.load()
        q = self._prepare_queries(q, normalize_queries, "search_device")
        nq = q.shape[0]
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        out_ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        flag = torch.empty(1, dtype=torch.int32, device=self.device)
        ws = self._workspace_for(int(lib.sskd_index_search_onepass_workspace_bytes(self._n, nq, k)))
        _native.check(
            lib.sskd_index_search_onepass_filtered(
                self._tiled.data_ptr(), self._n, q.data_ptr(), nq, k, self.id_offset,
                None if mask is None else mask.data_ptr(), out_scores.data_ptr(), out_ids.data_ptr(), flag.data_ptr(),
                ws.data_ptr(), ws.numel(), _native.current_stream_ptr(self.device),
            )
        )
        return out_scores, out_ids, flag

    def _search_numpy(self, query_emb, k: int, normalize_queries: Optional[bool], allow=None) -> Tuple[np.ndarray, np.ndarray]:
        qd = _host_queries_to_device(query_emb, self.device)
        with torch.cuda.device(self.device):
            mask = self._effective_mask(allow)
            nq = qd.shape[0]
            if (
                1 <= k <= self.ONEPASS_MAX_K
                and 1 <= nq <= self.ONEPASS_MAX_NQ
                and self._n >= 1
                and qd.shape[1] == self.embedding_dim
            ):
                norm = self.metric == "cosine" if normalize_queries is None else normalize_queries
                scores, ids, flag = self._search_onepass_device(qd, k, norm, mask)
                # this host path synchronises anyway (NumPy out): read the proof flag with the result
                if int(flag.item()) == 0:
                    self.last_search_path = "onepass"
                    return scores.cpu().numpy(), ids.cpu().numpy()
                self.last_search_path = "onepass-unproven+chained"
            else:
                self.last_search_path = "chained" if k > _native.SSKD_K_PASS else "single"
            scores, ids = self._search_device_masked(qd, k, normalize_queries, None, None, mask)
            if self.last_status is not None:
                self.last_search_path += "+screened"
            return scores.cpu().numpy(), ids.cpu().numpy()

    def search(self, query_emb: np.ndarray, k: int = 10, *, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(distances, indices)`` exactly as the serving route consumes them (app.py:293-301).  ``allow``: an
        optional filter (a bool array over ``ntotal`` rows, an integer id array, or a ``RowFilter``); removed rows
        are never returned.  Fewer than ``k`` matching rows pad the tail with ``(-FLT_MAX, -1)``."""
        if self._n == 0 and self._tiled is None and self.index is None:
            raise RuntimeError("index is empty: call build_from_parquet/add/load first")
        return self._search_numpy(query_emb, k, normalize_queries=None, allow=allow)

    # --------------------------------------------------------------- evaluation
    def qrels_device(self, qrels, nq: int):
        """Either form of qrels (``evaluation.qrels_to_csr``: the reference's dense ``relevance_labels``, ``{row: grade}``
        dicts, or a ready CSR) as the device CSR ``evaluate_device`` takes - built once on the host, so a caller that
        evaluates repeatedly (early stopping) uploads it once.  Rows are the ids ``search`` returns."""
        from . import evaluation

        lims, rows, grades = evaluation.qrels_to_csr(qrels, nq, self.id_offset)
        return tuple(torch.from_numpy(a).to(self.device) for a in (lims, rows, grades))

    def evaluate_device(self, queries: torch.Tensor, qrels_csr, k_values: Sequence[int] = (10, 50, 100), *, allow=None,
                        ideal: str = "retrieved") -> torch.Tensor:
        """Per-query retrieval metrics of device-resident queries: ONE ``search_device(max(k_values))`` and ONE
        ``sskd_eval_judge``, both enqueued on the current stream, no host synchronisation.  Returns a device fp64
        ``[nq, n_cut, 4]`` tensor = (ndcg, mrr, recall, precision) per ascending distinct cutoff (each at most 256).
        ``qrels_csr``: what ``qrels_device`` returned (None: no judgements).  Removed rows and ``allow`` act through the
        search; ``ideal``: ``"retrieved"`` (the reference's nDCG) or ``"judged"`` (ideal ranking over all judged rows)."""
        from . import evaluation

        ks, _ = evaluation._cutoffs(k_values)
        _, ids = self.search_device(queries, ks[-1], allow=allow)
        return evaluation.judge_device(ids, qrels_csr, ks, id_offset=self.id_offset, ideal=ideal)

    def evaluate(self, query_emb: np.ndarray, qrels, k_values: Sequence[int] = (10, 50, 100), *, allow=None,
                 ideal: str = "retrieved") -> dict:
        """``{"ndcg@k", "mrr@k", "recall@k", "precision@k"}`` for every cutoff: the means over the queries of
        ``evaluate_device``, taken with NumPy on the host (the reference's bits).  ``qrels``: per query the
        reference's dense label list indexed by corpus position (shorter lists mean 0) or a ``{row: grade}`` dict."""
        from . import evaluation

        qd = _host_queries_to_device(query_emb, self.device)
        with torch.cuda.device(self.device):
            block = self.evaluate_device(qd, self.qrels_device(qrels, qd.shape[0]), k_values, allow=allow, ideal=ideal)
            return evaluation.means_of(block.cpu().numpy(), sorted({int(k) for k in k_values}))

    # ------------------------------------------------------- hard-negative mining
    def mine_negatives_device(
        self,
        queries: torch.Tensor,
        pos_lims: torch.Tensor,
        pos_rows: torch.Tensor,
        *,
        top_k: int = 5,
        search_k: int = 100,
        margin: float = 0.1,
        allow=None,
        by_group: bool = False,
        normalize_queries: Optional[bool] = None,
        denoising=None,
        trigrams=None,
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """The ANCE rule on the device (``include/sskd_amd.h``, hard-negative mining): the ``search_k`` best rows of
        every query are its candidates, its positives ``pos_rows[pos_lims[q]:pos_lims[q + 1]]`` (device int64 / int32,
        LOCAL rows) are left out, and the candidates scoring ``>= max(positive scores) - margin`` (0.0 without
        positives; decided in fp64) survive.  Returns device tensors ``(D [nq, top_k] float32, I [nq, top_k] int64,
        counts [nq] int32, max_pos [nq] float32)``: the first ``top_k`` survivors in ``search``'s order, padded with
        ``(-FLT_MAX, -1)``; ``counts`` is every survivor among the ``search_k`` candidates, before the cut.

        ``allow`` and removed rows act on the candidates as in ``search``; a positive they hide still sets
        ``max_pos``.  ``by_group=True`` also leaves out every row that shares a group with a positive (the other
        chunks of a positive document).  No host synchronisation (``allow`` should then be a prepared ``RowFilter``):
        the caller guarantees that ``pos_lims`` is non-decreasing and ends inside ``pos_rows``; ``mine_negatives``
        checks all of that on the host.

        ``denoising`` (a ``denoise.Denoising``; None: today's path, untouched) with ``trigrams`` (the ``TrigramStore``
        of the index's rows) puts ``sskd_rank_denoise`` between the search and the selection: a candidate whose text
        overlap with a positive exceeds ``text_overlap_threshold`` leaves the window first, and ``counts`` then counts
        the survivors of both steps.  Still nothing synchronises and the call stays graph-capturable.  Only the overlap
        rule runs here: the teacher rule needs texts to score, so a ``denoising`` with a teacher threshold is refused
        (``ANCEMiner.mine_from_index`` has the texts and a teacher)."""
        self._check_mining_denoising(denoising, trigrams)
        q, lims, rows, rank_scores, rank_rows = self._mine_rank(queries, pos_lims, pos_rows, top_k, search_k, allow,
                                                                normalize_queries)
        if denoising is not None and q.shape[0]:
            rank_scores, rank_rows, _, _ = self.denoise_ranking_device(rank_scores, rank_rows, lims, rows, denoising,
                                                                       trigrams=trigrams)
        return self._mine_select(q, rank_scores, rank_rows, lims, rows, top_k, margin, by_group)

    def _mine_rank(self, queries, pos_lims, pos_rows, top_k, search_k, allow, normalize_queries):
        """The checks and the search of ``mine_negatives_device``: ``(q, pos_lims, pos_rows, rank_scores, rank_rows)``,
        the ranking in LOCAL rows."""
        top_k, search_k = int(top_k), int(search_k)
        if top_k < 1 or top_k > search_k:
            raise ValueError(f"top_k={top_k} outside [1, search_k={search_k}]")
        if search_k > _native.SSKD_K_MAX:
            raise ValueError(f"search_k={search_k} outside [1, {_native.SSKD_K_MAX}]")
        if not isinstance(queries, torch.Tensor):
            raise TypeError("mine_negatives_device expects a float32 device tensor")
        q = self._prepare_queries(queries, normalize_queries, "mine_negatives_device")
        nq = q.shape[0]
        for name, t, dtype in (("pos_lims", pos_lims, torch.int64), ("pos_rows", pos_rows, torch.int32)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != 1:
                raise TypeError(f"mine_negatives_device expects {name} as a 1-d {dtype} device tensor")
        if pos_lims.numel() != nq + 1:
            raise ValueError(f"pos_lims holds {pos_lims.numel()} entries for {nq} queries (needs nq + 1)")
        mask = self._effective_mask(allow)
        # the ranking in LOCAL rows: the kernel compares them with the positives and looks their groups up
        rank_scores, rank_rows = self._search_device_masked(q, search_k, False, None, None, mask, id_offset=0)
        return q, pos_lims.contiguous(), pos_rows.contiguous(), rank_scores, rank_rows

    def _mine_select(self, q, rank_scores, rank_rows, lims, rows, top_k, margin, by_group):
        """``sskd_index_mine_select`` over a ranking in LOCAL rows (the search's, or a denoised one)."""
        lib = _native.load()
        nq, search_k = rank_scores.shape
        top_k = int(top_k)
        scores = torch.empty((nq, top_k), dtype=torch.float32, device=self.device)
        ids = torch.empty((nq, top_k), dtype=torch.int64, device=self.device)
        counts = torch.empty(nq, dtype=torch.int32, device=self.device)
        max_pos = torch.empty(nq, dtype=torch.float32, device=self.device)
        if nq == 0:
            return scores, ids, counts, max_pos
        groups = self._row_group_device() if by_group and self.group_keys is not None else None   # no groups: rows
        _native.check(
            lib.sskd_index_mine_select(
                0 if self._tiled is None else self._tiled.data_ptr(), self._n, q.data_ptr(), nq,
                rank_scores.data_ptr(), rank_rows.data_ptr(), search_k, lims.data_ptr(),
                rows.data_ptr() if rows.numel() else None, None if groups is None else groups.data_ptr(),
                float(margin), top_k, self.id_offset, scores.data_ptr(), ids.data_ptr(), counts.data_ptr(),
                max_pos.data_ptr(), _native.current_stream_ptr(self.device),
            )
        )
        return scores, ids, counts, max_pos

    def mine_negatives(self, query_emb: np.ndarray, positives, *, top_k: int = 5, search_k: int = 100,
                       margin: float = 0.1, allow=None, by_group: bool = False, denoising=None, trigrams=None):
        """``mine_negatives_device`` for host queries: NumPy ``(D, I, counts, max_pos)``.  ``positives``: one list of
        LOCAL rows per query, or a ``(lims, rows)`` tuple (query ``q`` owns ``rows[lims[q]:lims[q + 1]]``); rows are
        sorted and de-duplicated per query, rows outside the index raise ``ValueError``.  ``by_group=True`` on an index
        without groups means every row is its own group, as in ``search_grouped``.  ``denoising`` / ``trigrams``: as
        in ``mine_negatives_device``."""
        self._check_mining_denoising(denoising, trigrams)
        if top_k < 1 or top_k > search_k:
            raise ValueError(f"top_k={top_k} outside [1, search_k={search_k}]")
        if search_k > _native.SSKD_K_MAX:
            raise ValueError(f"search_k={search_k} outside [1, {_native.SSKD_K_MAX}]")
        q = np.ascontiguousarray(np.asarray(query_emb, dtype=np.float32))
        if q.ndim == 1:
            q = q[None, :]
        lims, rows = normalize_positives(positives, q.shape[0], self._n)
        qd = _host_queries_to_device(q, self.device)
        extra = {} if denoising is None else {"denoising": denoising, "trigrams": trigrams}
        with torch.cuda.device(self.device):
            out = self.mine_negatives_device(
                qd, torch.from_numpy(lims).to(self.device), torch.from_numpy(rows).to(self.device), top_k=top_k,
                search_k=search_k, margin=margin, allow=allow, by_group=by_group, **extra)
            return tuple(t.cpu().numpy() for t in out)

    # ------------------------------------------------------------------ denoising
    def _check_mining_denoising(self, denoising, trigrams) -> None:
        """What ``mine_negatives`` can do of a ``Denoising``: the overlap rule, given the store of this index's rows."""
        if denoising is None:
            if trigrams is not None:
                raise ValueError("trigrams given without denoising")
            return
        from .denoise import Denoising

        if not isinstance(denoising, Denoising):
            raise TypeError("denoising must be a Denoising (or None)")
        if denoising.teacher_score_threshold is not None:
            raise ValueError("mine_negatives cannot apply teacher_score_threshold: the teacher rule needs texts to score "
                             "(pass Denoising(teacher_score_threshold=None) here, or mine through ANCEMiner with a teacher)")
        if denoising.text_overlap_threshold is not None and trigrams is None:
            raise ValueError("denoising with a text_overlap_threshold needs trigrams (the TrigramStore of the index's rows)")
        if trigrams is not None and trigrams.n_sets != self._n:
            raise ValueError(f"trigrams holds {trigrams.n_sets} sets for an index of {self._n} rows")

    def denoise_ranking_device(self, rank_scores: torch.Tensor, rank_rows: torch.Tensor, pos_lims: torch.Tensor,
                               pos_rows: torch.Tensor, denoising, trigrams=None, aux: Optional[torch.Tensor] = None,
                               diagnostics: bool = False):
        """Drop the false negatives of a ranking in LOCAL rows (``include/sskd_amd.h``, denoising of a ranking): ONE
        ``sskd_rank_denoise`` on the current stream, no host synchronisation.  A rank goes when its text overlap with
        one of the query's positives is ``> denoising.text_overlap_threshold`` (needs ``trigrams``, the
        ``TrigramStore`` of this index's rows) or when ``aux`` (float32 ``[nq, search_k]``, e.g. the teacher's
        confidence) is ``>= denoising.teacher_score_threshold``; a rule whose threshold is None or whose input is
        missing is off, and with both off the window is copied.  Returns ``(scores, rows, aux, counts)`` - the
        survivors in rank order, ``(-FLT_MAX, -1, NaN)`` padded, the shape ``sskd_index_mine_select`` and the re-rankers
        take - and with ``diagnostics`` also ``(overlap float64, reason uint8)`` aligned with the input ranks."""
        from . import denoise

        if trigrams is not None and trigrams.n_sets != self._n:
            raise ValueError(f"trigrams holds {trigrams.n_sets} sets for an index of {self._n} rows")
        return denoise.rank_denoise_device(rank_scores, rank_rows, pos_lims, pos_rows, denoising, trigrams=trigrams,
                                           aux=aux, diagnostics=diagnostics)

    def denoise_ranking(self, rank_scores, rank_rows, positives, denoising, trigrams=None, aux=None,
                        diagnostics: bool = False):
        """``denoise_ranking_device`` for host arrays: NumPy in (``positives`` as in ``mine_negatives``), NumPy out
        (``None`` stays ``None``)."""
        s = np.ascontiguousarray(np.asarray(rank_scores, dtype=np.float32))
        r = np.ascontiguousarray(np.asarray(rank_rows, dtype=np.int64))
        if s.ndim != 2 or s.shape != r.shape:
            raise ValueError("rank_scores and rank_rows must be 2-d arrays of one shape")
        lims, rows = normalize_positives(positives, s.shape[0], self._n)
        to = lambda a: torch.from_numpy(a).to(self.device)
        with torch.cuda.device(self.device):
            out = self.denoise_ranking_device(
                to(s), to(r), to(lims), to(rows), denoising, trigrams=trigrams,
                aux=None if aux is None else to(np.ascontiguousarray(np.asarray(aux, dtype=np.float32))),
                diagnostics=diagnostics)
            return tuple(None if t is None else t.cpu().numpy() for t in out)

    # ----------------------------------------------------------- grouped search
    def _default_k_rows(self, k: int) -> int:
        """Rows to rank for ``k`` groups: ``(k - 1) m + 1`` (m = largest group) always holds k groups or every row -
        taken when one scan pass serves it; otherwise one pass's worth (the caller doubles on ``unproved``)."""
        need = (k - 1) * self.max_group_size + 1
        return need if need <= _native.SSKD_K_PASS else max(k, _native.SSKD_K_PASS)

    def search_grouped_device(
        self,
        queries: torch.Tensor,
        k: int,
        k_rows: Optional[int] = None,
        allow=None,
        normalize_queries: Optional[bool] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Top-k distinct groups by their best row (``include/sskd_amd.h``, grouped search) for device-resident
        queries: device tensors ``(scores [nq, k], ids [nq, k] int64, groups [nq, k] int32, unproved [nq] int32)``.
        ``ids`` are the groups' best rows; fewer than k groups pad with ``(-FLT_MAX, -1, -1)``.  No host
        synchronisation (``allow`` should then be a prepared ``RowFilter``).  The result is exact for every query
        with ``unproved == 0``; where it is 1 the best ``k_rows`` rows (default: ``(k - 1) * max_group_size + 1`` if
        one scan pass serves that, else 32) held fewer than k groups, the entries written (``last_group_counts``)
        are still the exact first groups, and the caller asks again with a larger ``k_rows`` - ``search_grouped``
        does all of that."""
        mask = self._effective_mask(allow)
        q = self._prepare_queries(queries, normalize_queries, "search_grouped_device")
        return self._search_grouped_masked(q, k, k_rows, mask)

    def _search_grouped_masked(self, q: torch.Tensor, k: int, k_rows: Optional[int], mask):
        lib = _native.load()
        if k < 1 or k > _native.SSKD_K_MAX:
            raise ValueError(f"k={k} outside [1, {_native.SSKD_K_MAX}]")
        if k_rows is None:
            k_rows = self._default_k_rows(k)
        if k_rows < k or k_rows > _native.SSKD_K_MAX:
            raise ValueError(f"k_rows={k_rows} outside [k={k}, {_native.SSKD_K_MAX}]")
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        groups = torch.empty((nq, k), dtype=torch.int32, device=self.device)
        counts = torch.empty(nq, dtype=torch.int32, device=self.device)
        unproved = torch.empty(nq, dtype=torch.int32, device=self.device)
        n_unproved = torch.empty(1, dtype=torch.int32, device=self.device)
        ws = self._workspace_for(int(lib.sskd_index_search_grouped_workspace_bytes(self._n, nq, k, k_rows)))
        _native.check(
            lib.sskd_index_search_grouped(
                0 if self._tiled is None else self._tiled.data_ptr(), self._n, q.data_ptr(), nq, k, k_rows, self.id_offset,
                None if mask is None else mask.data_ptr(), self._row_group_device().data_ptr(), scores.data_ptr(),
                ids.data_ptr(), groups.data_ptr(), counts.data_ptr(), unproved.data_ptr(), n_unproved.data_ptr(),
                ws.data_ptr(), ws.numel(), _native.current_stream_ptr(self.device),
            )
        )
        self.last_group_counts, self.last_group_n_unproved = counts, n_unproved
        return scores, ids, groups, unproved

    def _grouped_rounds(self, q: torch.Tensor, k: int, mask):
        """Host loop of the exact grouped search short of the mask route: the default ``k_rows``, then only the
        unproved queries again with ``k_rows`` doubled, up to SSKD_K_MAX.  Returns NumPy ``(D, I, G, counts,
        unproved)`` and the largest ``k_rows`` used."""
        nq = q.shape[0]
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        G = np.empty((nq, k), dtype=np.int32)
        counts = np.zeros(nq, dtype=np.int32)
        unproved = np.zeros(nq, dtype=np.bool_)
        pending = np.arange(nq)
        k_rows = self._default_k_rows(k)
        while pending.size:
            sub = q if pending.size == nq else q[torch.from_numpy(pending).to(self.device)].contiguous()
            s, i, g, u = self._search_grouped_masked(sub, k, k_rows, mask)
            D[pending], I[pending], G[pending] = s.cpu().numpy(), i.cpu().numpy(), g.cpu().numpy()
            counts[pending] = self.last_group_counts.cpu().numpy()
            open_ = u.cpu().numpy().astype(np.bool_)
            unproved[pending] = open_
            if k_rows >= _native.SSKD_K_MAX:
                break
            pending = pending[open_]
            if pending.size:
                k_rows = min(2 * k_rows, _native.SSKD_K_MAX)
        return D, I, G, counts, unproved, k_rows

    def _search_grouped_numpy(self, query_emb, k: int, normalize_queries: Optional[bool], allow=None):
        lib = _native.load()
        qd = _host_queries_to_device(query_emb, self.device)
        with torch.cuda.device(self.device):
            mask = self._effective_mask(allow)
            q = self._prepare_queries(qd, normalize_queries, "search_grouped")
            first = self._default_k_rows(k)
            D, I, G, counts, unproved, k_rows = self._grouped_rounds(q, k, mask)
            if (k - 1) * self.max_group_size + 1 <= _native.SSKD_K_PASS:
                path = "grouped:counted"
            else:
                path = f"grouped:rows{first}" if k_rows == first else f"grouped:doubled{k_rows}"
            # a query still unproved at SSKD_K_MAX rows (one group fills them): take its groups found so far out
            # through the allow-mask and search for the rest; every round finds a new group, so at most k rounds
            words = int(lib.sskd_row_mask_words(self._n))
            for qi in np.flatnonzero(unproved):
                found = int(counts[qi])
                m_q = (torch.full((max(words, 1),), -1, dtype=torch.int32, device=self.device) if mask is None
                       else mask[: max(words, 1)].clone())
                bad = torch.empty(1, dtype=torch.int32, device=self.device)
                new = G[qi, :found]
                while True:
                    rows = torch.from_numpy(self._rows_of_groups(new)).to(self.device)
                    _native.check(lib.sskd_row_mask_update(m_q.data_ptr(), self._n, rows.data_ptr(), rows.numel(), 0,
                                                           bad.data_ptr(), _native.current_stream_ptr(self.device)))
                    d, i, g, c, u, _ = self._grouped_rounds(q[qi:qi + 1], k - found, m_q)
                    c0 = int(c[0])
                    D[qi, found:found + c0], I[qi, found:found + c0], G[qi, found:found + c0] = d[0, :c0], i[0, :c0], g[0, :c0]
                    new = g[0, :c0]
                    found += c0
                    if not u[0] or found >= k:
                        break
                counts[qi] = found
            if unproved.any():
                path += "+mask"
            self.last_search_path = path
            return D, I, G

    def search_grouped(self, query_emb: np.ndarray, k: int = 10, *, allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The top-k distinct groups (documents) by their best row (chunk), always exact: NumPy ``(D [nq, k], I [nq, k],
        G [nq, k])`` - group score, its best row's id, group number (``group_key`` maps it back).  It is what
        walking ``search``'s full ranking and keeping the first row of every new group gives; without groups it
        equals ``search``.  ``allow`` and removed rows act as in ``search``: a group is scored by its allowed rows
        alone.  Fewer than k groups pad the tail with ``(-FLT_MAX, -1, -1)``.  ``last_search_path`` records the
        route: ``grouped:counted`` (``(k - 1) * max_group_size + 1`` rows fit one scan pass: proven by counting),
        ``grouped:rows32`` / ``grouped:doubledN`` (the best 32 rows, then only the unproved queries again with the
        row count doubled up to N), and a ``+mask`` suffix when a query still unproved at 1024 rows was finished by
        masking the groups found so far and searching again."""
        if self._n == 0 and self._tiled is None and self.index is None:
            raise RuntimeError("index is empty: call build_from_parquet/add/load first")
        return self._search_grouped_numpy(query_emb, k, normalize_queries=None, allow=allow)

    # ------------------------------------------------------------- range search
    def _range_call(self, q: torch.Tensor, thr: torch.Tensor, mask, lims: torch.Tensor, scores, ids, max_results: int):
        lib = _native.load()
        nq = q.shape[0]
        ws = self._workspace_for(int(lib.sskd_index_range_search_workspace_bytes(self._n, nq, max_results)))
        _native.check(
            lib.sskd_index_range_search(
                0 if self._tiled is None else self._tiled.data_ptr(), self._n, q.data_ptr(), nq, thr.data_ptr(),
                self.id_offset, None if mask is None else mask.data_ptr(), lims.data_ptr(),
                None if scores is None else scores.data_ptr(), None if ids is None else ids.data_ptr(), max_results,
                ws.data_ptr(), ws.numel(), _native.current_stream_ptr(self.device),
            )
        )

    def range_search_device(
        self,
        queries: torch.Tensor,
        threshold,
        *,
        allow=None,
        normalize_queries: Optional[bool] = None,
        max_results: Optional[int] = None,
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Every allowed row scoring ``> threshold`` (faiss ``range_search``) for device-resident queries; returns
        device tensors ``(lims [nq + 1] int64, scores float32, ids int64)``: the results of query ``q`` are
        ``[lims[q], lims[q + 1])``, sorted by score descending, then id ascending.  ``threshold``: a float, or one
        per query (array or device tensor).  Removed rows are never returned; ``allow`` works as in ``search``.

        With ``max_results`` the call makes no host synchronisation (``threshold`` should then be a float or a
        device tensor, and ``allow`` a prepared ``RowFilter``): ``scores`` / ``ids`` have ``max_results`` entries and
        hold the results only if ``lims[-1] <= max_results``, which the caller checks (``lims`` is always exact).
        Without it the call synchronises once to read ``lims[-1]``, calls again if the reused result buffer was too
        small (grown to exactly the total), and returns tensors of exactly ``lims[-1]`` entries."""
        q = self._prepare_queries(queries, normalize_queries, "range_search_device")
        nq = q.shape[0]
        if isinstance(threshold, torch.Tensor) and threshold.is_cuda:
            thr = threshold.reshape(-1).to(torch.float32)
            if thr.numel() == 1 and nq != 1:
                thr = thr.expand(nq)
            if thr.numel() != nq:
                raise ValueError(f"{thr.numel()} thresholds for {nq} queries")
            thr = thr.contiguous()
        elif np.ndim(threshold) == 0 and not isinstance(threshold, torch.Tensor):
            thr = torch.full((max(nq, 1),), float(threshold), dtype=torch.float32, device=self.device)
        else:
            host = threshold.cpu().numpy() if isinstance(threshold, torch.Tensor) else threshold
            thr = torch.from_numpy(range_thresholds(host, nq)).to(self.device)
        mask = self._effective_mask(allow)
        lims = torch.empty(nq + 1, dtype=torch.int64, device=self.device)
        if max_results is not None:
            max_results = int(max_results)
            if max_results < 0:
                raise ValueError(f"max_results={max_results} < 0")
            scores = torch.empty(max_results, dtype=torch.float32, device=self.device)
            ids = torch.empty(max_results, dtype=torch.int64, device=self.device)
            self._range_call(q, thr, mask, lims, scores, ids, max_results)
            return lims, scores, ids
        cap = max(int(self.range_capacity), 1)
        if self._range_scores is None or self._range_scores.numel() < cap:
            self._range_scores = torch.empty(cap, dtype=torch.float32, device=self.device)
            self._range_ids = torch.empty(cap, dtype=torch.int64, device=self.device)
        cap = self._range_scores.numel()
        self._range_call(q, thr, mask, lims, self._range_scores, self._range_ids, cap)
        total = int(lims[-1].item())
        if total > cap:   # the count is exact: one retry with exactly the room it needs
            self._range_scores = torch.empty(total, dtype=torch.float32, device=self.device)
            self._range_ids = torch.empty(total, dtype=torch.int64, device=self.device)
            self.range_capacity = total
            self._range_call(q, thr, mask, lims, self._range_scores, self._range_ids, total)
        return lims, self._range_scores[:total].clone(), self._range_ids[:total].clone()

    def _range_numpy(self, query_emb, threshold, normalize_queries: Optional[bool], allow=None):
        qd = _host_queries_to_device(query_emb, self.device)
        thr = range_thresholds(threshold, qd.shape[0])
        with torch.cuda.device(self.device):
            lims, scores, ids = self.range_search_device(
                qd, torch.from_numpy(thr).to(self.device), allow=allow, normalize_queries=normalize_queries
            )
            return lims.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()

    def range_search(self, query_emb: np.ndarray, threshold, *, allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """faiss ``range_search``: every row scoring ``> threshold`` (a float, or one per query), as NumPy
        ``(lims int64 [nq + 1], D float32, I int64)``; query ``q``'s results are ``[lims[q], lims[q + 1])``, sorted by
        score descending, then id ascending.  Queries are normalised for the cosine metric as in ``search``;
        ``allow`` works as in ``search`` and removed rows are never returned."""
        return self._range_numpy(query_emb, threshold, normalize_queries=None, allow=allow)

    def near_duplicates(self, threshold: float, *, batch_size: int = 4096) -> Tuple[np.ndarray, np.ndarray]:
        """Every pair of live rows ``i < j`` (as ids) scoring ``> threshold``: ``(pairs int64 [m, 2], scores float32
        [m])`` sorted by (i, score descending, j).  The queries are the stored rows themselves (not normalised
        again), so score(i, j) == score(j, i) bit for bit; self-matches and removed rows are excluded."""
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} < 1")
        _native.require_gpu()
        lib = _native.load()
        removed = self.removed_rows()
        live = np.ones(self._n, dtype=np.bool_)
        live[removed] = False
        pair_parts, score_parts = [], []
        with torch.cuda.device(self.device):
            for lo in range(0, self._n, batch_size):
                b = min(batch_size, self._n - lo)
                rows = torch.empty((b, self.embedding_dim), dtype=torch.float32, device=self.device)
                _native.check(lib.sskd_index_get_rows(self._tiled.data_ptr(), lo, b, rows.data_ptr(),
                                                      _native.current_stream_ptr(self.device)))
                lims, scores, ids = self.range_search_device(rows, float(threshold), normalize_queries=False)
                p, s = pairs_from_ranges(lims.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy(),
                                         np.arange(lo, lo + b, dtype=np.int64) + self.id_offset, live[lo:lo + b])
                pair_parts.append(p)
                score_parts.append(s)
        if not pair_parts:
            return np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.float32)
        return np.concatenate(pair_parts), np.concatenate(score_parts)

    # ------------------------------------------------------- near-duplicate clusters
    def _range_call_from(self, row0: int, q: torch.Tensor, thr: torch.Tensor, mask, lims, scores, ids, max_results: int):
        """``sskd_index_range_search`` over the stored rows ``[row0, n)`` alone (``row0`` a multiple of 32, so the rows stay
        tile-aligned and ``mask``, the words of ALL rows, is entered at word ``row0 / 32``); the ids written are those
        of a scan over every row."""
        lib = _native.load()
        n_rows, nq = self._n - row0, q.shape[0]
        ws = self._workspace_for(int(lib.sskd_index_range_search_workspace_bytes(n_rows, nq, max_results)))
        tiled = 0 if self._tiled is None else self._tiled.data_ptr() + row0 * self.embedding_dim * 4
        _native.check(
            lib.sskd_index_range_search(
                tiled, n_rows, q.data_ptr(), nq, thr.data_ptr(), self.id_offset + row0,
                None if mask is None else mask.data_ptr() + (row0 // 32) * 4, lims.data_ptr(), scores.data_ptr(),
                ids.data_ptr(), max_results, ws.data_ptr(), ws.numel(), _native.current_stream_ptr(self.device),
            )
        )

    def duplicate_clusters(self, threshold: float, *, keep: str = "first", scope: str = "all", allow=None,
                           batch_size: int = 4096):
        """The clusters of near-duplicate rows: the connected components (single linkage) of the pairs
        ``near_duplicates(threshold)`` returns, as a ``dedup.DuplicateClusters`` - one label per row, and per cluster the row
        it keeps and its size.  ``keep``: ``"first"`` keeps a cluster's smallest row, ``"densest"`` the row with the most
        pairs (ties to the smallest row).  ``scope``: ``"all"`` pairs, or over the row groups (``set_groups``) only the pairs
        ``"across_groups"`` / ``"within_groups"``.  ``allow`` (as in ``search``) restricts the rows taking part; removed rows
        never do.

        The self-join is ``near_duplicates``' (stored rows as queries, not normalised again, strict ``>``), but every
        batch's range result stays in HBM and goes straight into the union-find kernels (``include/sskd_amd.h``, near-
        duplicate clusters): nothing proportional to the number of pairs reaches the host.  The batches are enqueued without
        a synchronisation, each into ``dedup_capacity`` result entries; the per-batch overflow flags are read once at the
        end, and only the batches that overflowed (they linked nothing) run again with exactly the room they need.  A batch
        that starts at a multiple of 32 rows scans only the rows from its start on - the pairs ``i < j`` are all there -
        so the self-join costs about half of ``near_duplicates``'."""
        from . import dedup

        keep_c, scope_c = dedup.keep_code(keep), dedup.scope_code(scope)
        if batch_size < 1:
            raise ValueError(f"batch_size={batch_size} < 1")
        _native.require_gpu()
        lib = _native.load()
        n = self._n
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device)
            mask = self._effective_mask(allow)
            groups = self._row_group_device() if scope_c else None
            state = torch.empty((4, max(n, 1)), dtype=torch.int32, device=self.device)   # parent, degree, rep, size
            parent, degree, rep, size = state[0], state[1], state[2], state[3]
            counts = torch.empty(2, dtype=torch.int32, device=self.device)
            _native.check(lib.sskd_dup_init(n, None if mask is None else mask.data_ptr(), parent.data_ptr(),
                                            degree.data_ptr(), stream))
            starts = list(range(0, n, batch_size))
            overflow = torch.zeros(max(len(starts), 1), dtype=torch.int32, device=self.device)
            totals = torch.zeros(max(len(starts), 1), dtype=torch.int64, device=self.device)

            def run(b: int, cap: int, scores: torch.Tensor, ids: torch.Tensor) -> None:
                lo = starts[b]
                nq = min(batch_size, n - lo)
                rows = torch.empty((nq, self.embedding_dim), dtype=torch.float32, device=self.device)
                _native.check(lib.sskd_index_get_rows(self._tiled.data_ptr(), lo, nq, rows.data_ptr(), stream))
                thr = torch.full((nq,), float(threshold), dtype=torch.float32, device=self.device)
                lims = torch.empty(nq + 1, dtype=torch.int64, device=self.device)
                self._range_call_from(lo if lo % _native.SSKD_TILE_ROWS == 0 else 0, rows, thr, mask, lims, scores, ids, cap)
                totals[b : b + 1].copy_(lims[nq:])
                _native.check(lib.sskd_dup_link(lims.data_ptr(), ids.data_ptr(), nq, cap, lo, self.id_offset, n,
                                                None if groups is None else groups.data_ptr(), scope_c,
                                                parent.data_ptr(), degree.data_ptr(), overflow[b:].data_ptr(), stream))

            cap = max(int(self.dedup_capacity), 1)
            scores = torch.empty(cap, dtype=torch.float32, device=self.device)
            ids = torch.empty(cap, dtype=torch.int64, device=self.device)
            for b in range(len(starts)):
                run(b, cap, scores, ids)
            again = np.flatnonzero(overflow.cpu().numpy()[: len(starts)])   # the one synchronisation of the join
            if again.size:
                need = totals.cpu().numpy()
                overflow.zero_()
                cap = int(need[again].max())   # lims[-1] is exact whatever the capacity was
                scores = torch.empty(cap, dtype=torch.float32, device=self.device)
                ids = torch.empty(cap, dtype=torch.int64, device=self.device)
                for b in again.tolist():
                    run(b, cap, scores, ids)
            _native.check(lib.sskd_dup_labels(n, parent.data_ptr(), degree.data_ptr(), keep_c, rep.data_ptr(),
                                              size.data_ptr(), counts.data_ptr(), stream))
            host = state[:, :n].cpu().numpy()
            if again.size and overflow.cpu().numpy().any():
                raise RuntimeError("a range result overflowed the capacity its own count asked for")
            n_clusters, n_rows = (int(x) for x in counts.cpu().numpy())
        out = dedup.clusters_from_arrays(host[0], host[2], host[3], self.id_offset)
        if (out.n_clusters, out.n_rows) != (n_clusters, n_rows):
            raise RuntimeError("sskd_dup_labels' counts disagree with its labels")
        return out

    def deduplicate(self, threshold: float, *, keep: str = "first", scope: str = "all", allow=None,
                    batch_size: int = 4096, compact: bool = False):
        """``duplicate_clusters`` and then ``remove_ids`` of every row taking part that is not the row its cluster keeps:
        afterwards ``near_duplicates(threshold)`` finds no pair among the rows that took part.  Returns the
        ``DuplicateClusters`` with ``removed`` = the ids dropped (ascending); ``compact=True`` also runs ``compact()`` and
        stores its ``kept`` array on the result (the labels and representatives stay in the OLD ids: ``kept`` maps them)."""
        if compact and self.shard_info:
            raise ValueError("deduplicate(compact=True): this index is one piece of a row-sharded build (see compact())")
        out = self.duplicate_clusters(threshold, keep=keep, scope=scope, allow=allow, batch_size=batch_size)
        out.removed = out.duplicates()
        if out.removed.size:
            self.remove_ids(out.removed)
        if compact:
            out.kept = self.compact()
        return out

    # -------------------------------------------------------------- persistence
    def reconstruct(self, rows: Sequence[int]) -> np.ndarray:
        """Stored vectors of the given local rows (``faiss.Index.reconstruct`` for a list), host fp32."""
        lib = _native.load()
        rows = [int(r) for r in rows]
        out = torch.empty((len(rows), self.embedding_dim), dtype=torch.float32, device=self.device)
        for j, r in enumerate(rows):
            if not 0 <= r < self._n:
                raise IndexError(f"row {r} outside [0, {self._n})")
            _native.check(lib.sskd_index_get_rows(self._tiled.data_ptr(), r, 1, out[j].data_ptr(),
                                                  _native.current_stream_ptr(self.device)))
        return out.cpu().numpy()

    def to_numpy(self) -> np.ndarray:
        """Row-major copy of the stored vectors (host)."""
        lib = _native.load()
        out = torch.empty((self._n, self.embedding_dim), dtype=torch.float32, device=self.device)
        if self._n:
            _native.check(
                lib.sskd_index_get_rows(self._tiled.data_ptr(), 0, self._n, out.data_ptr(),
                                        _native.current_stream_ptr(self.device))
            )
        return out.cpu().numpy()

    def save(self, output_dir: Union[str, Path]) -> None:
        """Write ``index.faiss`` (flat inner-product layout) + ``doc_ids.json`` (+ ``texts.json``).  A row shard
        (``id_offset != 0``, or one written by ``sharded_index.build_sharded``) also gets ``shard.json`` with the
        global id of its first row, which ``load`` restores."""
        out = Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        write_flat_ip(out / "index.faiss", self.to_numpy())
        with open(out / "doc_ids.json", "w") as f:
            json.dump(list(self.doc_ids), f)
        if self.doc_texts is not None:
            with open(out / "texts.json", "w") as f:
                json.dump(self.doc_texts, f)
        if self.id_offset != 0 or self.shard_info:
            with open(out / "shard.json", "w") as f:
                json.dump({**(self.shard_info or {}), "id_offset": self.id_offset, "rows": self._n}, f)
        # tombstones: the flat file keeps every row (it stays faiss-readable); the removed LOCAL rows go beside it
        if self._n_removed:
            np.save(out / "removed.npy", self.removed_rows())
        else:
            (out / "removed.npy").unlink(missing_ok=True)
        # groups: written only when set (an index without groups writes the files it always wrote)
        if self.group_keys is not None:
            np.save(out / "groups.npy", np.ascontiguousarray(self._row_group_host, dtype=np.int32))
            with open(out / "group_keys.json", "w") as f:
                json.dump(list(self.group_keys), f)
        else:
            (out / "groups.npy").unlink(missing_ok=True)
            (out / "group_keys.json").unlink(missing_ok=True)

    def load(self, index_dir: Union[str, Path], append: bool = False) -> None:
        """Restore a saved index (``append=True``: add its rows behind the ones already held - consecutive row
        shards served by one process).  ``shard.json``, when present, restores ``id_offset``; ``groups.npy`` +
        ``group_keys.json``, when present, restore the row groups.  With ``append=True`` the loaded part's group
        numbers are offset behind the ones already held and keys are NEVER merged across the two parts: a document
        whose chunks were saved in both parts stays two groups.  A part without groups joins a grouped index as
        singleton groups."""
        d = Path(index_dir)
        path = d / "index.faiss"
        if not path.exists():
            raise FileNotFoundError(f"{path} not found")
        vecs = read_flat_ip(path)
        if vecs.shape[1] != self.embedding_dim:
            raise ValueError(f"index has dim {vecs.shape[1]}, builder expects {self.embedding_dim}")
        shard_path = d / "shard.json"
        shard = json.loads(shard_path.read_text()) if shard_path.exists() else None
        metric, self.metric = self.metric, "ip"  # stored vectors are already normalised
        try:
            if not append:
                self._n = 0
                self._tiled = None
                self._reset_removed()
                self._reset_groups()
                self.doc_ids = []
                self.doc_texts = None
                if shard is not None:
                    self.id_offset = int(shard["id_offset"])
                    self.shard_info = {k: v for k, v in shard.items() if k not in ("id_offset", "rows")}
            elif shard is not None and int(shard["id_offset"]) != self.id_offset + self._n:
                raise ValueError(f"{d}: shard starts at row {shard['id_offset']}, expected {self.id_offset + self._n}")
            first = self._n
            self.reserve(self._n + vecs.shape[0])
            step = 1 << 18  # stream the (memory-mapped) matrix in 400 MB slabs
            for lo in range(0, vecs.shape[0], step):
                self._add_rows(np.array(vecs[lo : lo + step], dtype=np.float32, copy=True))
        finally:
            self.metric = metric
        self._load_groups(d, first, self._n - first)
        removed_path = d / "removed.npy"
        if removed_path.exists():
            removed = np.load(removed_path).astype(np.int64)
            if removed.size:
                self.remove_ids(removed + first + self.id_offset)
        ids_path = d / "doc_ids.json"
        if ids_path.exists():
            with open(ids_path) as f:
                self.doc_ids = list(self.doc_ids) + list(json.load(f))
        else:
            self.doc_ids = list(self.doc_ids) + [f"doc_{self.id_offset + i}" for i in range(first, self._n)]
        texts_path = d / "texts.json"
        if texts_path.exists():
            with open(texts_path) as f:
                self.doc_texts = {**(self.doc_texts or {}), **json.load(f)}
        self.index = IndexHandle(self)

    def _load_groups(self, d: Path, first: int, n_new: int) -> None:
        """Group numbers of the ``n_new`` rows just loaded behind ``first``: the part's own numbers offset behind the
        groups already held (no key is looked up: parts never merge)."""
        path = d / "groups.npy"
        if not path.exists():
            self._extend_groups(first, n_new, None)
            return
        numbers = np.load(path).astype(np.int32).reshape(-1)
        with open(d / "group_keys.json") as f:
            keys = list(json.load(f))
        if numbers.size != n_new or (numbers.size and (numbers.min() < 0 or numbers.max() >= len(keys))):
            raise ValueError(f"{d}: groups.npy does not match the index ({numbers.size} entries for {n_new} rows, {len(keys)} keys)")
        self._extend_groups(first, 0, [])   # rows already held become singleton groups if they had none
        base = len(self.group_keys)
        self.group_keys.extend(keys)
        self._row_group_host = np.concatenate([self._row_group_host, numbers + np.int32(base)])
        for g, key in enumerate(keys, start=base):
            if key is not None:
                self._group_of_key.setdefault(key, g)
        self._groups_changed()

    def cleanup(self) -> None:
        self._tiled = None
        self._workspace = None
        self._n = 0
        self._reset_removed()
        self._reset_groups()


# ---------------------------------------------------------------------- helpers
def read_corpus_parquet(parquet_path, max_docs: Optional[int] = None, text_column: str = "text",
                        id_column: str = "chunk_id") -> Tuple[List[str], List[str]]:
    """``(ids, texts)`` of a corpus in the reference's schema (src/data/prepare.py:72-84, tests/conftest.py:210-216)."""
    import pandas as pd

    df = pd.read_parquet(parquet_path)
    if max_docs is not None:
        df = df.head(max_docs)
    if text_column not in df.columns:
        raise KeyError(f"parquet file {parquet_path} has no {text_column!r} column")
    texts = df[text_column].astype(str).tolist()
    if id_column in df.columns:
        ids = df[id_column].astype(str).tolist()
    else:
        ids = [f"doc_{i}" for i in range(len(texts))]
    return ids, texts


def read_parquet_column(parquet_path, column: str, max_docs: Optional[int] = None) -> List[str]:
    """One column of a corpus parquet file as strings (the group keys of ``build_from_parquet(group_column=...)``)."""
    import pandas as pd

    df = pd.read_parquet(parquet_path)
    if max_docs is not None:
        df = df.head(max_docs)
    if column not in df.columns:
        raise KeyError(f"parquet file {parquet_path} has no {column!r} column")
    return df[column].astype(str).tolist()


def groups_from_chunk_ids(chunk_ids: Sequence[str]) -> List[str]:
    """The document of every chunk by the reference's rule (its ``maxsim_aggregation``): the chunk id up to its last
    ``_`` - ``"_".join(chunk_id.split("_")[:-1])`` - and the whole id when it holds no ``_``."""
    out = []
    for cid in chunk_ids:
        parts = str(cid).split("_")
        out.append("_".join(parts[:-1]) if len(parts) > 1 else str(cid))
    return out


def normalize_positives(positives, nq: int, n_rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """The positives of ``nq`` queries as ``(lims int64 [nq + 1], rows int32)``, each query's rows sorted and
    de-duplicated.  ``positives``: a sequence of ``nq`` row sequences, or a ``(lims, rows)`` TUPLE in that CSR form.
    Raises ``ValueError`` for a wrong number of queries, limits that do not start at 0, decrease or do not end at
    ``len(rows)``, and rows outside ``[0, n_rows)``."""
    if isinstance(positives, tuple):
        if len(positives) != 2:
            raise ValueError("positives as a tuple is (lims, rows)")
        lims_in = np.asarray(positives[0]).reshape(-1)
        rows_in = np.asarray(positives[1]).reshape(-1)
        if lims_in.size != nq + 1:
            raise ValueError(f"positives: {lims_in.size} limits for {nq} queries (needs nq + 1)")
        if lims_in.dtype.kind not in "iu" or (rows_in.size and rows_in.dtype.kind not in "iu"):
            raise ValueError("positives: limits and rows must be integers")
        lims_in = lims_in.astype(np.int64)
        if lims_in[0] != 0 or (np.diff(lims_in) < 0).any() or lims_in[-1] != rows_in.size:
            raise ValueError(f"positives: limits must start at 0, never decrease and end at len(rows)={rows_in.size}")
        parts = [rows_in[lims_in[i]:lims_in[i + 1]] for i in range(nq)]
    else:
        parts = list(positives)
        if len(parts) != nq:
            raise ValueError(f"positives for {len(parts)} queries, {nq} queries given")
    out = []
    for i, part in enumerate(parts):
        a = np.asarray(part)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError(f"positives[{i}] is not a flat list of integer rows")
        a = np.unique(a.astype(np.int64))
        if a.size and (a[0] < 0 or a[-1] >= n_rows):
            raise ValueError(f"positives[{i}]: rows outside [0, {n_rows})")
        out.append(a.astype(np.int32))
    lims = np.zeros(nq + 1, dtype=np.int64)
    if nq:
        np.cumsum([a.size for a in out], out=lims[1:])
    rows = np.concatenate(out) if out else np.zeros(0, dtype=np.int32)
    return lims, np.ascontiguousarray(rows, dtype=np.int32)


def _kept_rows(n_rows: int, removed: np.ndarray) -> np.ndarray:
    """The rows of ``range(n_rows)`` not in ``removed`` (sorted local rows), ascending int64."""
    live = np.ones(n_rows, dtype=np.bool_)
    live[removed] = False
    return np.flatnonzero(live).astype(np.int64)


def range_thresholds(threshold, nq: int) -> np.ndarray:
    """One float32 threshold per query: a scalar is broadcast, an array must hold ``nq`` values."""
    t = np.asarray(threshold, dtype=np.float32)
    if t.ndim == 0:
        return np.full(nq, t, dtype=np.float32)
    t = t.reshape(-1)
    if t.size == 1 and nq != 1:
        return np.full(nq, t[0], dtype=np.float32)
    if t.size != nq:
        raise ValueError(f"{t.size} thresholds for {nq} queries")
    return np.ascontiguousarray(t)


def pairs_from_ranges(lims: np.ndarray, scores: np.ndarray, ids: np.ndarray, query_ids: np.ndarray,
                      query_live: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The pairs ``(i, j)``, ``i < j``, of a self range search: query ``q`` is id ``query_ids[q]``; queries that are
    not live contribute nothing.  Keeps the per-query order (score descending, then j), so queries given in
    ascending id order yield pairs sorted by (i, score descending, j)."""
    lims = np.asarray(lims, dtype=np.int64)
    counts = np.diff(lims)
    qi = np.repeat(np.asarray(query_ids, dtype=np.int64), counts)
    live = np.repeat(np.asarray(query_live, dtype=np.bool_), counts)
    j = np.asarray(ids, dtype=np.int64)[: lims[-1]]
    keep = live & (j > qi)
    pairs = np.stack([qi[keep], j[keep]], axis=1) if keep.any() else np.zeros((0, 2), dtype=np.int64)
    return pairs.astype(np.int64, copy=False), np.asarray(scores, dtype=np.float32)[: lims[-1]][keep]


def _resolve_device(device: Optional[str]) -> torch.device:
    if device is None or device == "cuda":
        return torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(
            f"device={device!r}: semantic-search-kd_amd runs on MI355X only (PyTorch-ROCm spells it 'cuda[:N]'); "
            "there is no CPU path"
        )
    return dev


def _host_queries_to_device(query_emb, device: torch.device) -> torch.Tensor:
    """Host queries (``[dim]`` or ``[nq, dim]``) as a contiguous float32 ``[nq, dim]`` device tensor."""
    _native.require_gpu()
    q = np.ascontiguousarray(np.asarray(query_emb, dtype=np.float32))
    if q.ndim == 1:
        q = q[None, :]
    return torch.from_numpy(q).to(device)


def _as_device_f32(x: Union[np.ndarray, torch.Tensor], device: torch.device) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))
    _native.require_gpu()
    return t.to(device=device, dtype=torch.float32).contiguous()


def write_flat_ip(path: Union[str, Path], vectors: np.ndarray) -> None:
    """Serialise vectors in faiss' ``IndexFlatIP`` layout (fourcc ``IxFI``, faiss/impl/index_write.cpp)."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    n, d = v.shape
    with open(path, "wb") as f:
        f.write(_FLAT_IP_FOURCC)
        f.write(struct.pack("<iqqqBi", d, n, _FAISS_DUMMY, _FAISS_DUMMY, 1, _METRIC_INNER_PRODUCT))
        f.write(struct.pack("<Q", n * d))
        v.tofile(f)


def read_flat_ip(path: Union[str, Path]) -> np.ndarray:
    """Memory-map the vectors of a flat inner-product index file written by :func:`write_flat_ip`."""
    with open(path, "rb") as f:
        fourcc = f.read(4)
        if fourcc != _FLAT_IP_FOURCC:
            raise ValueError(
                f"{path}: index type {fourcc!r} is not a flat inner-product index; HNSW graph files "
                "cannot be loaded by the exact-scan backend — rebuild the index from the corpus"
            )
        d, n, _, _, _, metric = struct.unpack("<iqqqBi", f.read(4 + 8 * 3 + 1 + 4))
        (count,) = struct.unpack("<Q", f.read(8))
        offset = f.tell()
    if metric != _METRIC_INNER_PRODUCT or count != n * d:
        raise ValueError(f"{path}: malformed flat index header (d={d}, n={n}, count={count}, metric={metric})")
    if n == 0:
        return np.zeros((0, d), dtype=np.float32)
    return np.memmap(path, dtype=np.float32, mode="r", offset=offset, shape=(n, d))
