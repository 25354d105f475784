"""Row-sharded index: build, persist, reload and serve across the GPUs of one node.

The reference builds ONE in-process index (scripts/build_faiss_index.py:45-72) and serves it from ONE process
(src/serve/app.py:407-457).  BASELINE.json's north star shards the corpus row-wise over 8 GPUs (SURVEY.md section
8e): "each GPU writes its embeddings straight into its own index shard" - zero communication while building - and a
search is: queries replicated, every rank scans its shard, ONE all-gather of the packed per-shard top-k, merge.

On disk (``<output_dir>/``)::

    shards.json                 {"format": 1, "n_total": N, "embedding_dim": 384, "metric": "cosine",
                                 "shards": [{"dir": "shard_0", "id_offset": 0, "rows": n0}, ...]}
    shard_<r>/index.faiss       this shard's vectors (flat inner-product layout, as an unsharded index)
    shard_<r>/doc_ids.json      this shard's ids, in row order
    shard_<r>/texts.json        this shard's id -> text table
    shard_<r>/shard.json        {"id_offset", "rows", "rank", "world_size", "n_total"}

Every shard directory is by itself a valid ``FAISSIndexBuilder.load`` target.  An index written by G ranks can be
served by any world size that divides the work into contiguous runs of shards (8 shards on 1, 2, 4 or 8 GPUs): rank r
loads shards ``[r S / G, (r + 1) S / G)`` back to back into one HBM buffer.

Serving (``ShardedIndex``): rank 0 owns the HTTP surface and calls ``search`` like on a ``FAISSIndexBuilder``; the
other ranks sit in ``serve_forever()``.  Every operation (``load``, ``remove_ids``, ``search``, ``range_search``) is
one protocol, ``ShardedIndex._step`` with a row of ``_OPS``:

1. rank 0 checks the call (its rank, a usable deployment, a loaded index, the arguments, the manifest);
2. rank 0 sends a 5-word header (op, nq or length, k, filter kind, filter length) and the call's inputs as host
   tensors on the CONTROL group - the query block, the thresholds, the GLOBAL filter (a bool mask over ``ntotal`` rows
   or an id list), the ids to remove or the directory to load;
3. every rank runs the op's local part inside ``try`` (a search applies its slice ``[lo, hi)`` of the filter) and
   reports one status word on the control group;
4. only when every word is zero does every rank run the op's finish: a load commits, a removal sums its counts on the
   control group, a search takes ``dist.ShardedSearcher``'s all-gather of the packed records and the merge, a range
   search its two all-gathers (per-rank totals, then the records padded to the largest) and rank 0's
   ``sskd_range_merge_packed``.

So the data group is entered only by the record all-gathers, after every rank has agreed.  World size 1 runs the
same local part and finish with no header and no communication; ``load_all_ranks`` (every rank at start-up) runs the
step without a header.  ``torch.distributed`` backend ``nccl`` is RCCL over xGMI; ``gloo`` works for rehearsals
(records are then staged through the host).

Failure path (reference: src/serve/app.py:354-361 turns any exception into a 500; SURVEY.md section 5: a failed
HIP / RCCL call must surface as a Python exception and ``/health.index_loaded`` must reflect shard state):

* the control group is a CPU (``gloo``) group of the same ranks with an effectively unbounded timeout: the waiting
  ranks park in a HOST broadcast, never inside a device collective (an RCCL collective that rank 0 has not joined
  is aborted by the watchdog after the group's timeout - an idle server would die - and spins a GPU meanwhile);
* a call that is wrong in itself raises ``ValueError`` on rank 0 before anything is announced;
* when some rank's local part fails, every rank skips the finish (a load drops what it staged), rank 0 raises
  ``ShardFailure`` (-> the route's 500) naming the ranks and their messages, and the deployment keeps serving: a
  failed ``load`` leaves the previous index in place on EVERY rank (two-phase: prepare, exchange, commit).  At world
  size 1 a search or range search raises the local exception itself;
* status exchanges wait ``op_timeout_s``: a rank that died or hangs turns into ``ShardFailure`` on rank 0 within that
  time, the index is marked broken (``is_loaded`` False -> ``/health.index_loaded`` False) and later calls fail fast.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .dist import ShardedSearcher, _world, shard_bounds
from .index import range_thresholds

MANIFEST = "shards.json"
# the header's first word; the second is the number of queries (search, range) or the length of the ids to remove or
# of the directory to load, the third k
_OP_STOP, _OP_SEARCH, _OP_LOAD, _OP_REMOVE, _OP_RANGE = 0, 1, 2, 3, 4
# how a call's global filter travels on the control group (the header's 4th word; the 5th is its length)
_FILTER_NONE, _FILTER_MASK, _FILTER_IDS = 0, 1, 2


class ShardFailure(RuntimeError):
    """An operation of the sharded deployment failed on one or more ranks (or a rank did not answer in time)."""

    def __init__(self, what: str, failures: Dict[int, str]) -> None:
        self.failures = dict(failures)
        detail = "; ".join(f"rank {r}: {m}" for r, m in sorted(self.failures.items()))
        super().__init__(f"{what} failed on {len(self.failures)} rank(s): {detail}")


def _default_factory(embedding_dim: int, metric: str, device, id_offset: int):
    from .index import FAISSIndexBuilder

    return FAISSIndexBuilder(embedding_dim=embedding_dim, index_type="HNSW", metric=metric, device=device, id_offset=id_offset)


def build_sharded(model, parquet_path: Union[str, Path], output_dir: Union[str, Path], batch_size: int = 32,
                  max_docs: Optional[int] = None, device: Optional[str] = None, group=None, embedding_dim: int = 384,
                  metric: str = "cosine", index_factory: Optional[Callable] = None, show_progress: bool = False,
                  text_column: str = "text", id_column: str = "chunk_id") -> Dict:
    """Every rank encodes ITS contiguous row range ``shard_bounds(N, G, r)`` of the corpus straight into its own HBM
    shard (``id_offset`` = first row) and saves it as ``shard_<r>/``; rank 0 writes the manifest.  No data-path
    communication - two barriers order the directory creation and the manifest.  Works without a process group
    (one shard).  Returns the manifest."""
    import torch.distributed as dist

    from .index import read_corpus_parquet

    world, rank = _world(group)
    out = Path(output_dir)
    ids, texts = read_corpus_parquet(parquet_path, max_docs, text_column, id_column)
    n = len(texts)
    lo, hi = shard_bounds(n, world, rank)
    factory = index_factory or _default_factory
    builder = factory(embedding_dim, metric, device, lo)
    builder.reserve(max(hi - lo, 1))
    slab = max(batch_size, 65536)   # stream: a multi-million-passage shard never needs one host matrix
    on_device = getattr(model, "encode_documents_device", None)   # embeddings go encoder -> index tiles inside HBM
    for a in range(lo, hi, slab):
        b = min(a + slab, hi)
        if on_device is not None:
            builder.add(on_device(texts[a:b], batch_size=batch_size))
        else:
            builder.add(model.encode_documents(texts[a:b], batch_size=batch_size, show_progress=show_progress))
    builder.doc_ids = ids[lo:hi]
    builder.doc_texts = dict(zip(ids[lo:hi], texts[lo:hi]))
    builder.shard_info = {"rank": rank, "world_size": world, "n_total": n}
    if rank == 0:
        out.mkdir(parents=True, exist_ok=True)
    if world > 1:
        dist.barrier(group)
    builder.save(out / f"shard_{rank}")
    if world > 1:
        dist.barrier(group)
    manifest = {
        "format": 1, "n_total": n, "embedding_dim": embedding_dim, "metric": metric,
        "shards": [{"dir": f"shard_{r}", "id_offset": shard_bounds(n, world, r)[0],
                    "rows": shard_bounds(n, world, r)[1] - shard_bounds(n, world, r)[0]} for r in range(world)],
    }
    if rank == 0:
        (out / MANIFEST).write_text(json.dumps(manifest, indent=1) + "\n")
    if world > 1:
        dist.barrier(group)
    return manifest


def is_sharded_dir(index_dir: Union[str, Path]) -> bool:
    return (Path(index_dir) / MANIFEST).exists()


class ShardedIndex:
    """``FAISSIndexBuilder``-shaped front of a row-sharded index (``search`` / ``load`` / ``doc_ids`` / ``ntotal``)."""

    def __init__(self, embedding_dim: int = 384, index_type: str = "HNSW", metric: str = "cosine",
                 device: Optional[str] = None, group=None, index_factory: Optional[Callable] = None,
                 ctrl_group=None, op_timeout_s: float = 60.0, idle_timeout_s: float = 365 * 86400.0) -> None:
        """``group``: the data-path group (packed records); ``ctrl_group``: a gloo group of the same ranks for headers,
        call inputs and status words (made on first use when ``group`` is the default group); ``op_timeout_s``: how
        long a status exchange may take before the missing ranks are declared failed; ``idle_timeout_s``: how long the
        waiting ranks may sit without an announcement from rank 0."""
        self.embedding_dim, self.index_type, self.metric, self.device, self.group = embedding_dim, index_type, metric, device, group
        self._factory = index_factory or _default_factory
        self.local = None                      # this rank's shard(s): a FAISSIndexBuilder
        self.doc_ids: List[str] = []           # rank 0: every shard's ids in global row order
        self.doc_texts: Optional[Dict[str, str]] = None
        self.ntotal = 0
        self.manifest: Optional[Dict] = None
        self._searcher = ShardedSearcher(self._local_search, group=group)   # reads self.local at call time
        self._ctrl_group = ctrl_group
        self.op_timeout_s, self.idle_timeout_s = float(op_timeout_s), float(idle_timeout_s)
        self.broken: Optional[str] = None      # set when a rank stopped answering: the process group is unusable
        self.last_failure: Optional[Dict[int, str]] = None

    # ------------------------------------------------------------------ the collective step
    def _src(self) -> int:
        import torch.distributed as dist

        return dist.get_global_rank(self.group, 0) if self.group is not None else 0

    def _ctrl(self):
        """The control group: CPU tensors over gloo, made collectively on first use (every rank's first use is the
        same step: ``load_all_ranks`` at start-up, or the first header)."""
        import datetime

        import torch.distributed as dist

        if self._ctrl_group is None:
            if self.group is not None:
                if dist.get_backend(self.group) != "gloo":
                    raise RuntimeError("ShardedIndex over a sub-group needs ctrl_group= (a gloo group of the same ranks)")
                self._ctrl_group = self.group
            else:
                self._ctrl_group = dist.new_group(backend="gloo", timeout=datetime.timedelta(seconds=self.idle_timeout_s))
        return self._ctrl_group

    def _wire(self, header: Tuple[int, ...]) -> List[Tuple[Tuple[int, ...], torch.dtype]]:
        """``(shape, dtype)`` of the host tensors that follow a header: a call's inputs are fixed by its header words"""
        op, n, _, fkind, flen = header
        if op == _OP_STOP:
            return []
        if op == _OP_LOAD:
            return [((n,), torch.uint8)]                              # the directory, utf-8
        if op == _OP_REMOVE:
            return [((n,), torch.int64)]                              # global row ids
        wire = [((n, self.embedding_dim), torch.float32)]             # the query block
        if op == _OP_RANGE:
            wire.append(((n,), torch.float32))                        # one threshold per query
        if fkind != _FILTER_NONE:                                     # the GLOBAL filter
            wire.append(((flen,), torch.uint8 if fkind == _FILTER_MASK else torch.int64))
        return wire

    def _announce(self, header: Tuple[int, ...] = (_OP_STOP, 0, 0, _FILTER_NONE, 0),
                  inputs: Sequence[torch.Tensor] = ()) -> Tuple[Tuple[int, ...], List[torch.Tensor]]:
        """rank 0 sends a call's header and inputs, the other ranks receive them: HOST broadcasts on the CONTROL group
        (waiting costs no GPU and no watchdog can abort it), never on the data group, which nothing enters before the
        status exchange"""
        import torch.distributed as dist

        h = torch.tensor(header, dtype=torch.int64)
        dist.broadcast(h, src=self._src(), group=self._ctrl())
        header = tuple(int(x) for x in h)
        if _world(self.group)[1] != 0:
            inputs = [torch.empty(shape, dtype=dtype) for shape, dtype in self._wire(header)]
        for t in inputs:
            dist.broadcast(t, src=self._src(), group=self._ctrl())
        return header, list(inputs)

    def _exchange_status(self, what: str, error: Optional[BaseException]) -> Dict[int, str]:
        """Every rank reports one word (0 = its part succeeded); returns ``{rank: message}`` of the failed ranks, the
        same on every rank.  A rank that does not answer within ``op_timeout_s`` breaks the deployment."""
        import datetime

        import torch.distributed as dist

        world, rank = _world(self.group)
        if world == 1:
            return {0: f"{type(error).__name__}: {error}"} if error is not None else {}
        ctrl = self._ctrl()
        mine = torch.tensor([0 if error is None else 1], dtype=torch.int64)
        words = torch.zeros(world, dtype=torch.int64)
        try:
            work = dist.all_gather_into_tensor(words, mine, group=ctrl, async_op=True)
            work.wait(datetime.timedelta(seconds=self.op_timeout_s))
        except Exception as exc:  # noqa: BLE001 - a peer died or hangs: nothing collective can be trusted any more
            self.broken = f"{what}: a rank did not report within {self.op_timeout_s:.0f} s ({type(exc).__name__}: {exc})"
            raise ShardFailure(what, {-1: self.broken}) from exc
        failed = [r for r in range(world) if int(words[r]) != 0]
        if not failed:
            return {}
        # rare path: collect the messages (every rank saw the same words, so every rank joins)
        texts: List[Optional[str]] = [None] * world
        dist.all_gather_object(texts, None if error is None else f"{type(error).__name__}: {error}", group=ctrl)
        return {r: texts[r] or "failed" for r in failed}

    def _step(self, header: Tuple[int, ...], inputs: Sequence[torch.Tensor]):
        """One operation, run alike by every rank once it has the header and the inputs: the op's local part inside
        ``try``, ONE status exchange, then the op's finish only when every rank succeeded - the data group is entered
        nowhere else.  Otherwise every rank runs the op's abort and raises ``ShardFailure``; at world 1 a search or
        range search raises the local exception itself."""
        op = _OPS[header[0]]
        what = f"load {_text(inputs[0])}" if header[0] == _OP_LOAD else op.name
        part, error = None, None
        try:
            if op.needs_index and self.local is None:
                raise RuntimeError("no index loaded on this rank")
            part = op.part(self, header, inputs)
        except Exception as exc:  # noqa: BLE001 - reported to every rank below
            if op.bare_at_world_1 and _world(self.group)[0] == 1:
                raise
            error = exc
        failures = self._exchange_status(what, error)
        self.last_failure = failures or None
        if failures:
            if part is not None and op.abort is not None:
                op.abort(self, part)
            raise ShardFailure(what, failures) from error
        return op.finish(self, header, part)

    def _call(self, header: Tuple[int, ...], inputs: Sequence[torch.Tensor]):
        """rank 0 (or the one process): announce a checked call to the ranks in ``serve_forever`` and take part in it"""
        if _world(self.group)[0] > 1:
            self._announce(header, inputs)
        return self._step(header, inputs)

    def _prelude(self, op: int) -> None:
        """rank 0, before a call's arguments are checked: it is rank 0's call, the deployment answers, and an index is
        loaded when the op needs one"""
        if _OPS[op].needs_index and self.local is None:
            raise RuntimeError("index is empty: call load first")
        world, rank = _world(self.group)
        if world > 1 and rank != 0:
            raise RuntimeError(f"ShardedIndex.{_OPS[op].name} is rank 0's call; the other ranks run serve_forever()")
        self._check_usable()

    # ------------------------------------------------------------------ load
    @staticmethod
    def read_manifest(index_dir: Path, embedding_dim: int) -> Dict:
        """parse and validate ``shards.json`` (rank 0 does this BEFORE it announces a load)"""
        manifest = json.loads((Path(index_dir) / MANIFEST).read_text())
        if manifest.get("embedding_dim", embedding_dim) != embedding_dim:
            raise ValueError(f"index has dim {manifest['embedding_dim']}, expected {embedding_dim}")
        shards = manifest.get("shards")
        if not isinstance(shards, list) or not shards or "n_total" not in manifest:
            raise ValueError(f"{index_dir}/{MANIFEST}: no shards listed")
        at = 0
        for sh in shards:
            if int(sh["id_offset"]) != at:
                raise ValueError(f"{index_dir}/{MANIFEST}: shard {sh['dir']} starts at row {sh['id_offset']}, expected {at}")
            at += int(sh["rows"])
        if at != int(manifest["n_total"]):
            raise ValueError(f"{index_dir}/{MANIFEST}: shards hold {at} rows, n_total says {manifest['n_total']}")
        return manifest

    def _prepare_local(self, index_dir: Path) -> Dict:
        """phase 1 of a load: this rank's shards into a NEW local index; nothing of the serving state is touched"""
        world, rank = _world(self.group)
        manifest = self.read_manifest(index_dir, self.embedding_dim)
        shards = manifest["shards"]
        s = len(shards)
        mine = shards[rank * s // world : (rank + 1) * s // world]   # a contiguous run (possibly empty)
        offset = mine[0]["id_offset"] if mine else manifest["n_total"]
        local = self._factory(self.embedding_dim, manifest.get("metric", self.metric), self.device, offset)
        for j, sh in enumerate(mine):
            local.load(index_dir / sh["dir"], append=j > 0)
        if not mine:
            local.id_offset = offset
        rows = sum(int(sh["rows"]) for sh in mine)
        have = getattr(local, "ntotal", None)
        if have is not None and int(have) != rows:
            raise ValueError(f"{index_dir}: rank {rank} loaded {have} rows, the manifest lists {rows}")
        staged = {"local": local, "manifest": manifest, "doc_ids": [], "doc_texts": None}
        if rank == 0:   # the serving rank maps global row ids to doc ids / texts
            ids: List[str] = []
            texts: Dict[str, str] = {}
            for sh in shards:
                ids.extend(json.loads((index_dir / sh["dir"] / "doc_ids.json").read_text()))
                tp = index_dir / sh["dir"] / "texts.json"
                if tp.exists():
                    texts.update(json.loads(tp.read_text()))
            if len(ids) != int(manifest["n_total"]):
                raise ValueError(f"{index_dir}: {len(ids)} doc ids for {manifest['n_total']} rows")
            staged["doc_ids"], staged["doc_texts"] = ids, (texts or None)
        return staged

    def _load_part(self, header, inputs) -> Dict:
        return self._prepare_local(Path(_text(inputs[0])))

    def _commit(self, header, staged: Dict) -> None:
        """phase 2 of a load, on EVERY rank or on none"""
        old = self.local
        self.local, self.manifest = staged["local"], staged["manifest"]
        self.ntotal = int(self.manifest["n_total"])
        self.metric = self.manifest.get("metric", self.metric)
        self.doc_ids, self.doc_texts = staged["doc_ids"], staged["doc_texts"]
        if old is not None and old is not self.local and hasattr(old, "cleanup"):
            old.cleanup()

    def _discard(self, staged: Dict) -> None:
        if hasattr(staged["local"], "cleanup"):
            staged["local"].cleanup()

    def load(self, index_dir: Union[str, Path]) -> None:
        """Collective: on rank 0 (the caller in a served deployment) this tells the ranks waiting in
        ``serve_forever`` to load the same directory.  When every rank calls it directly (start-up), pass through
        ``load_all_ranks`` instead.  Raises ``ShardFailure`` when any rank cannot load its shards; the index that
        was being served stays in place on every rank."""
        index_dir = Path(index_dir)
        self._prelude(_OP_LOAD)
        if _world(self.group)[0] > 1:
            self.read_manifest(index_dir, self.embedding_dim)   # nothing is announced for a directory rank 0 cannot read
        self._call(*_load_call(index_dir))

    def load_all_ranks(self, index_dir: Union[str, Path]) -> None:
        """Start-up form: EVERY rank calls this with the same directory (no announcement needed).  Raises
        ``ShardFailure`` on every rank when any rank fails, so that the launcher exits instead of hanging."""
        self._step(*_load_call(Path(index_dir)))

    # ------------------------------------------------------------------ removal
    def _remove_part(self, header, inputs) -> int:
        """this rank's ``[id_offset, id_offset + rows)`` share of the ids -> the rows it newly removed"""
        ids, lo = inputs[0], int(self.local.id_offset)
        mine = ids[(ids >= lo) & (ids < lo + int(self.local.ntotal))]
        return int(self.local.remove_ids(mine.numpy())) if mine.numel() else 0

    def _remove_finish(self, header, newly: int) -> int:
        """the sum over the ranks of the rows newly removed (control group)"""
        import torch.distributed as dist

        if _world(self.group)[0] == 1:
            return newly
        total = torch.tensor([newly], dtype=torch.int64)
        dist.all_reduce(total, group=self._ctrl())
        return int(total[0])

    def remove_ids(self, global_ids) -> int:
        """Take GLOBAL row ids out of every later search on every rank (rank 0's call; the other ranks follow from
        ``serve_forever``).  Returns the number of rows newly removed; ``ValueError`` for ids outside
        ``[0, ntotal)`` (nothing is announced then); ``ShardFailure`` when a rank could not apply its share."""
        self._prelude(_OP_REMOVE)
        ids = torch.from_numpy(np.ascontiguousarray(global_ids.cpu() if isinstance(global_ids, torch.Tensor) else global_ids,
                                                    dtype=np.int64).reshape(-1))
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.ntotal):
            raise ValueError(f"ids outside [0, {self.ntotal})")
        return self._call((_OP_REMOVE, ids.numel(), 0, _FILTER_NONE, 0), [ids])

    # ------------------------------------------------------------------ state
    @property
    def is_loaded(self) -> bool:
        """every rank holds its shards of the index being served and answers (``/health.index_loaded``)"""
        return self.local is not None and self.broken is None

    def health(self) -> Dict:
        world, _ = _world(self.group)
        return {"world_size": world, "loaded": self.is_loaded, "ntotal": self.ntotal,
                "shards": len(self.manifest["shards"]) if self.manifest else 0,
                "broken": self.broken, "last_failure": self.last_failure}

    def _check_usable(self) -> None:
        if self.broken is not None:
            raise ShardFailure("sharded index", {-1: f"deployment is broken ({self.broken}); restart it"})

    # ------------------------------------------------------------------ search
    def _local_search(self, queries: torch.Tensor, k: int, out_scores=None, out_ids=None, allow=None):
        extra = {} if allow is None else {"allow": allow}   # an unfiltered search calls the local index as it always did
        return self.local.search_device(queries, k, normalize_queries=None, out_scores=out_scores, out_ids=out_ids,
                                        **extra)

    def _check_filter(self, allow) -> Tuple[Tuple[int, int], List[torch.Tensor]]:
        """rank 0, before anything is announced: a GLOBAL filter -> its header words ``(kind, length)`` and the host
        tensor that goes on the wire (a bool mask over ``ntotal`` rows as uint8, or int64 global ids; none for no
        filter); ValueError for a wrong length, dtype or id"""
        if allow is None:
            return (_FILTER_NONE, 0), []
        a = allow.cpu().numpy() if isinstance(allow, torch.Tensor) else np.asarray(allow)
        if a.dtype == np.bool_:
            if a.shape != (self.ntotal,):
                raise ValueError(f"a boolean filter needs one entry per row: shape {a.shape}, index has {self.ntotal} rows")
            return (_FILTER_MASK, a.size), [torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))]
        if a.dtype.kind in "iu" or a.size == 0:
            ids = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
            if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.ntotal):
                raise ValueError(f"filter ids outside [0, {self.ntotal})")
            return (_FILTER_IDS, ids.size), [torch.from_numpy(ids)]
        raise ValueError(f"a filter is a bool array over the rows or an integer id array, got dtype {a.dtype}")

    def _local_filter(self, filt: Sequence[torch.Tensor]):
        """this rank's slice ``[lo, lo + rows)`` of the call's global filter (none, a uint8 mask or int64 ids), in the
        form its local index takes"""
        if not filt:
            return None
        lo, rows = int(self.local.id_offset), int(self.local.ntotal)
        if filt[0].dtype == torch.uint8:
            return filt[0][lo : lo + rows].numpy().astype(np.bool_)
        ids = filt[0].numpy()
        return ids[(ids >= lo) & (ids < lo + rows)]

    def _check_queries(self, query_emb) -> np.ndarray:
        q = np.ascontiguousarray(np.asarray(query_emb, dtype=np.float32))
        if q.ndim == 1:
            q = q[None, :]
        if q.ndim != 2 or q.shape[1] != self.embedding_dim:
            raise ValueError(f"queries have shape {q.shape}, expected [nq, {self.embedding_dim}]")
        return q

    def _search_part(self, header, inputs) -> torch.Tensor:
        q, *filt = inputs
        return self._searcher.search_local(q.to(torch.device(self.local.device)), header[2], allow=self._local_filter(filt))

    def _search_finish(self, header, record: torch.Tensor):
        return self._searcher.gather_merge(record, header[1], header[2])

    def search(self, query_emb: np.ndarray, k: int = 10, *, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(distances [nq, k] fp32 desc, GLOBAL row ids [nq, k] int64, -1 padded)`` - rank 0's call.  ``allow``: an
        optional GLOBAL filter, a bool array over ``ntotal`` rows or an integer array of global ids; removed rows are
        never returned."""
        # everything that can be wrong with the CALL is found before the other ranks hear of it
        self._prelude(_OP_SEARCH)
        q = self._check_queries(query_emb)
        if int(k) < 1:
            raise ValueError(f"k must be >= 1, got {k}")
        fwords, filt = self._check_filter(allow)
        if q.shape[0] == 0:
            return np.zeros((0, int(k)), np.float32), np.zeros((0, int(k)), np.int64)
        s, i = self._call((_OP_SEARCH, q.shape[0], int(k), *fwords), [torch.from_numpy(q), *filt])
        return s.cpu().numpy(), i.cpu().numpy()

    def _range_part(self, header, inputs):
        q, thr, *filt = inputs
        dev = torch.device(self.local.device)
        return self.local.range_search_device(q.to(dev), thr.to(dev), allow=self._local_filter(filt), normalize_queries=None)

    def _range_finish(self, header, part):
        return self._searcher.range_gather_merge(*part, header[1])

    def range_search(self, query_emb: np.ndarray, threshold, *, allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """faiss ``range_search`` over every shard - rank 0's call: every allowed, not removed row scoring
        ``> threshold`` (a float, or one per query) as NumPy ``(lims int64 [nq + 1], D float32, I int64)`` with GLOBAL
        ids; query ``q``'s results are ``[lims[q], lims[q + 1])``, sorted by score descending, then id ascending - bit
        for bit what one ``FAISSIndexBuilder.range_search`` over the whole corpus returns.  ``allow`` as in ``search``."""
        self._prelude(_OP_RANGE)
        q = self._check_queries(query_emb)
        thr = range_thresholds(threshold, q.shape[0])
        fwords, filt = self._check_filter(allow)
        if q.shape[0] == 0:
            return np.zeros(1, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64)
        lims, scores, ids = self._call((_OP_RANGE, q.shape[0], 0, *fwords), [torch.from_numpy(q), torch.from_numpy(thr), *filt])
        return lims.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()

    def serve_forever(self) -> None:
        """Ranks other than 0: answer rank 0's announcements until it says stop.  An operation that fails HERE is
        reported to rank 0 through the status word and the loop goes on; only a broken process group ends it."""
        while True:
            header, inputs = self._announce()
            if header[0] == _OP_STOP:
                return
            try:
                self._step(header, inputs)
            except ShardFailure:
                if self.broken is not None:
                    raise
                # some rank's part failed (maybe this one's): rank 0 has raised it to its caller; keep serving

    def close(self) -> None:
        """rank 0: release the ranks waiting in ``serve_forever``"""
        world, rank = _world(self.group)
        if world > 1 and rank == 0 and self.broken is None:
            self._announce()

    def cleanup(self) -> None:
        if self.local is not None:
            self.local.cleanup()


class _Op(NamedTuple):
    """What every rank runs for one operation in ``ShardedIndex._step``."""

    name: str                          # the public call (rank 0's checks, ShardFailure)
    part: Callable                     # (index, header, inputs) -> this rank's part; runs inside try
    finish: Callable                   # (index, header, part) -> the call's result, once every rank has succeeded
    abort: Optional[Callable] = None   # (index, part): drop this rank's part when another rank failed
    needs_index: bool = True           # every rank must hold an index
    bare_at_world_1: bool = False      # world 1 raises the local exception itself rather than ShardFailure


_OPS = {
    _OP_SEARCH: _Op("search", ShardedIndex._search_part, ShardedIndex._search_finish, bare_at_world_1=True),
    _OP_RANGE: _Op("range_search", ShardedIndex._range_part, ShardedIndex._range_finish, bare_at_world_1=True),
    _OP_LOAD: _Op("load", ShardedIndex._load_part, ShardedIndex._commit, ShardedIndex._discard, needs_index=False),
    _OP_REMOVE: _Op("remove_ids", ShardedIndex._remove_part, ShardedIndex._remove_finish),
}


def _load_call(index_dir: Path) -> Tuple[Tuple[int, ...], List[torch.Tensor]]:
    """the header and the input of a load: the directory as utf-8 bytes"""
    path = torch.from_numpy(np.frombuffer(str(index_dir).encode(), dtype=np.uint8).copy())
    return (_OP_LOAD, path.numel(), 0, _FILTER_NONE, 0), [path]


def _text(t: torch.Tensor) -> str:
    return t.numpy().tobytes().decode()


def open_index(index_dir: Union[str, Path], embedding_dim: int = 384, current=None, device: Optional[str] = None):
    """What the serving layer calls for ``/index/load`` (reference: src/serve/app.py:407-441): a directory with a
    ``shards.json`` manifest opens as a ``ShardedIndex`` (re-using ``current`` when it already is one, so that the
    waiting ranks follow), anything else as a plain ``FAISSIndexBuilder``."""
    from .index import FAISSIndexBuilder

    index_dir = Path(index_dir)
    if is_sharded_dir(index_dir):
        idx = current if isinstance(current, ShardedIndex) else ShardedIndex(embedding_dim=embedding_dim, device=device)
        idx.load(index_dir)
        return idx
    if isinstance(current, ShardedIndex) and _world(current.group)[0] > 1:
        raise ValueError(f"{index_dir} has no {MANIFEST}: a {_world(current.group)[0]}-rank deployment serves sharded indexes")
    builder = FAISSIndexBuilder(embedding_dim=embedding_dim, device=device)
    builder.load(index_dir)
    return builder
