"""Row-sharded search across the GPUs of one node (one process per GPU, RCCL over xGMI).

The reference has a single in-process index (src/serve/app.py:49-66); BASELINE.json's
north star shards the corpus row-wise, so this is the one place the path has a real
exchange step:

    every rank: scan its shard  ->  one packed record { ids int64[nq, k]; scores fp32[nq, k] }
                                    (the scan's final merge writes straight into the record)
    all ranks : ONE all-gather  ->  [G] records             (1.2 MB / rank at nq=10k, k=10)
    every rank: merge G*k -> k per query (``sskd_topk_merge_packed``; ties: lower global id)

A range search has results of any length per rank, so it takes two collectives: an all-gather of the per-rank
totals fixes ``cap`` = the largest, every rank pads its record ``{ lims[nq + 1]; ids[cap]; scores[cap] }`` to it, one
all-gather moves the records, and rank 0 merges them (``sskd_range_merge_packed``).

The collective goes through ``torch.distributed`` (backend ``nccl`` = RCCL on ROCm) on
the same stream as the kernels.  ``local_search`` / ``merge`` / ``all_gather`` are injectable
so that the sharding logic can be exercised with ``gloo`` on CPU in the tests.
"""
from __future__ import annotations

import inspect
from typing import Callable, List, Optional, Tuple

import torch

from . import _native


def _world(group=None) -> Tuple[int, int]:
    """``(world size, rank)`` of ``group``; ``(1, 0)`` without an initialised process group"""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def shard_bounds(n_rows: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous row range ``[lo, hi)`` of ``rank``: ceil(N / G) rows per rank."""
    per = -(-n_rows // world_size)
    lo = min(rank * per, n_rows)
    return lo, min(lo + per, n_rows)


def record_bytes(nq: int, k: int) -> int:
    """Bytes of one rank's packed record (``sskd_topk_record_bytes``): ids, scores, pad to 16."""
    return (nq * k * 12 + 15) // 16 * 16 if nq > 0 and k > 0 else 0


def record_views(record: torch.Tensor, nq: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(scores fp32 [nq, k], ids int64 [nq, k])`` views into a packed uint8 record."""
    ids = record[: nq * k * 8].view(torch.int64).view(nq, k)
    scores = record[nq * k * 8 : nq * k * 12].view(torch.float32).view(nq, k)
    return scores, ids


def range_record_bytes(nq: int, cap: int) -> int:
    """Bytes of one rank's packed range record (``sskd_range_record_bytes``): lims, ids, scores, pad to 16."""
    return ((nq + 1) * 8 + cap * 12 + 15) // 16 * 16 if nq >= 0 and cap >= 0 else 0


def range_record_views(record: torch.Tensor, nq: int, cap: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(lims int64 [nq + 1], scores fp32 [cap], ids int64 [cap])`` views into a packed uint8 range record."""
    a = (nq + 1) * 8
    lims = record[:a].view(torch.int64)
    ids = record[a : a + cap * 8].view(torch.int64)
    scores = record[a + cap * 8 : a + cap * 12].view(torch.float32)
    return lims, scores, ids


def hip_range_merge_packed(records: torch.Tensor, g: int, nq: int, cap: int,
                           total: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``[G * range_record_bytes]`` gathered records -> ``(lims [nq + 1], scores [total], ids [total])`` via the HIP
    range merge; ``total`` is the sum of the runs' totals (known to the caller from the first all-gather)."""
    lib = _native.load()
    dev = records.device
    lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    scores = torch.empty(total, dtype=torch.float32, device=dev)
    ids = torch.empty(total, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.sskd_range_merge_workspace_bytes(g, nq, total)), 1), dtype=torch.uint8, device=dev)
    _native.check(
        lib.sskd_range_merge_packed(
            records.data_ptr(), g, nq, cap, lims.data_ptr(), scores.data_ptr() if total else None,
            ids.data_ptr() if total else None, total, ws.data_ptr(), ws.numel(),
            _native.current_stream_ptr(dev),
        )
    )
    return lims, scores, ids


def hip_merge_packed(records: torch.Tensor, g: int, nq: int, k_in: int, k_out: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``[G * record_bytes]`` gathered uint8 records -> ``[nq, k_out]`` (no unpacking copies)."""
    lib = _native.load()
    out_s = torch.empty((nq, k_out), dtype=torch.float32, device=records.device)
    out_i = torch.empty((nq, k_out), dtype=torch.int64, device=records.device)
    _native.check(
        lib.sskd_topk_merge_packed(
            records.data_ptr(), g, nq, k_in, k_out, out_s.data_ptr(), out_i.data_ptr(),
            _native.current_stream_ptr(records.device),
        )
    )
    return out_s, out_i


def sharded_scores(score_fn: Callable[[int, int], torch.Tensor], n_items: int, group=None,
                   device: Optional[torch.device] = None) -> torch.Tensor:
    """Pure data parallelism over ``n_items`` independent work items (teacher scoring, BASELINE cfg 5;
    SURVEY.md section 8e: "pure DP over pairs with a final concat").

    Rank r computes ``score_fn(lo, hi) -> fp32 [hi - lo]`` for its contiguous range ``shard_bounds(n_items, G, r)``;
    ONE ``all_gather_into_tensor`` of ceil(n / G) floats per rank is the final concat - every rank returns all
    ``n_items`` scores in item order.  No collective inside the scoring itself.  Without an initialised process
    group (or world size 1) this is just ``score_fn(0, n_items)``."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return score_fn(0, n_items)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    lo, hi = shard_bounds(n_items, world, rank)
    local = score_fn(lo, hi) if hi > lo else torch.empty(0, dtype=torch.float32, device=device)
    # gloo moves host tensors, nccl (= RCCL) device tensors
    comm_dev = torch.device("cpu") if dist.get_backend(group) == "gloo" else local.device
    per = -(-n_items // world)
    send = torch.zeros(per, dtype=torch.float32, device=comm_dev)
    send[: hi - lo] = local.to(comm_dev, torch.float32)
    recv = torch.empty(world * per, dtype=torch.float32, device=comm_dev)
    dist.all_gather_into_tensor(recv, send, group=group)
    return recv[:n_items].to(local.device)   # ceil-sized shards: only the tail of the LAST ranks is padding


def _stacked(views) -> List[torch.Tensor]:
    """the G ranks' record views -> one ``[G, ...]`` tensor per field (what the injected CPU merges take)"""
    return [torch.stack(field) for field in zip(*views)]


class ShardedSearcher:
    """Search a corpus whose rows are split over the ranks of a process group."""

    def __init__(
        self,
        local_search: Callable[..., Tuple[torch.Tensor, torch.Tensor]],
        group=None,
        merge: Optional[Callable[[torch.Tensor, torch.Tensor, int], Tuple[torch.Tensor, torch.Tensor]]] = None,
        all_gather: Optional[Callable[[torch.Tensor, torch.Tensor], None]] = None,
        range_merge: Optional[Callable[..., Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]] = None,
    ) -> None:
        """``local_search(queries, k[, out_scores=, out_ids=])`` must return this rank's
        ``(scores, GLOBAL ids)`` (e.g. ``FAISSIndexBuilder(id_offset=lo).search_device``); when it
        accepts ``out_scores`` / ``out_ids`` it writes straight into the packed record.
        ``merge(scores [G, nq, k], ids [G, nq, k], k)`` replaces the HIP merge (CPU tests);
        ``all_gather(out, inp)`` replaces ``dist.all_gather_into_tensor`` (e.g. host-staged gloo
        when several test ranks share one GPU; it carries the range path's two all-gathers as well).
        ``range_merge(lims [G, nq + 1], scores [G, cap], ids [G, cap])`` replaces the HIP range merge (CPU tests)."""
        self.local_search = local_search
        self.group = group
        self.merge = merge
        self.all_gather = all_gather
        self.range_merge = range_merge
        self.last_world = 1

    def _local_into(self, queries, k, out_s, out_i, allow=None):
        fn = self.local_search
        try:
            params = inspect.signature(fn).parameters
        except (TypeError, ValueError):
            params = {}
        extra = {} if allow is None else {"allow": allow}   # an unfiltered call passes no allow at all
        if "out_scores" in params and "out_ids" in params:
            s, i = fn(queries, k, out_scores=out_s, out_ids=out_i, **extra)
        else:
            s, i = fn(queries, k, **extra)
        if s.data_ptr() != out_s.data_ptr():
            out_s.copy_(s)
        if i.data_ptr() != out_i.data_ptr():
            out_i.copy_(i)

    def search_local(self, queries: torch.Tensor, k: int, allow=None) -> torch.Tensor:
        """This rank's half of a sharded search, no communication: the local scan writes its ``(scores, GLOBAL
        ids)`` straight into a fresh packed record, which is returned (``gather_merge`` takes it from there).
        Split from ``search`` so that a caller can agree with the other ranks that every local scan succeeded
        BEFORE any rank enters the device collective (sharded_index.ShardedIndex).  ``allow``: this rank's local
        filter, handed to ``local_search`` as ``allow=`` (not passed at all when None)."""
        nq = queries.shape[0]
        send = torch.empty(record_bytes(nq, k), dtype=torch.uint8, device=queries.device)
        out_s, out_i = record_views(send, nq, k)
        self._local_into(queries, k, out_s, out_i, allow)
        return send

    def _all_gather(self, send: torch.Tensor, world: int) -> torch.Tensor:
        """every rank's ``send`` (one size on every rank) -> ``[G, send.numel()]`` on ``send``'s device"""
        import torch.distributed as dist

        recv = torch.empty(world * send.numel(), dtype=send.dtype, device=send.device)
        if self.all_gather is not None:
            self.all_gather(recv, send)
        elif dist.get_backend(self.group) == "gloo" and send.is_cuda:
            # gloo moves host memory (several ranks sharing one GPU in tests, CPU-only rehearsals): stage the
            # records through the host.  On a node with one GPU per rank the backend is nccl (= RCCL over xGMI) and
            # the records never leave HBM.
            host = torch.empty(recv.shape, dtype=recv.dtype)
            dist.all_gather_into_tensor(host, send.cpu(), group=self.group)
            recv.copy_(host)
        else:
            dist.all_gather_into_tensor(recv, send, group=self.group)
        return recv.view(world, -1)

    def gather_merge(self, send: torch.Tensor, nq: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """ONE all-gather of the packed records (RCCL over xGMI on a GPU node) and the merge of the G lists; at world
        size 1 the record's own ``(scores, ids)``."""
        world = self.last_world = _world(self.group)[0]
        if world == 1:
            return record_views(send, nq, k)
        records = self._all_gather(send, world)
        if self.merge is not None:
            return self.merge(*_stacked(record_views(r, nq, k) for r in records), k)
        return hip_merge_packed(records, world, nq, k, k)

    def range_gather_merge(self, lims: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor,
                           nq: int) -> Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
        """The range path's exchange, every rank: this rank's exact-size local range result ``(lims [nq + 1], scores,
        GLOBAL ids)`` -> an all-gather of the per-rank totals (``cap`` = the largest) -> this rank's record padded to
        ``cap`` -> ONE all-gather of the records -> on rank 0 the merge, returned as ``(lims, scores, ids)`` in the
        order of one range search over the whole corpus; the other ranks return None.  World size 1: the local
        result itself."""
        world, rank = _world(self.group)
        self.last_world = world
        if world == 1:
            return lims, scores, ids
        host_totals = self._all_gather(lims[nq:].contiguous(), world).cpu()
        cap, total = int(host_totals.max()), int(host_totals.sum())
        send = torch.zeros(range_record_bytes(nq, cap), dtype=torch.uint8, device=lims.device)
        rec_lims, rec_scores, rec_ids = range_record_views(send, nq, cap)
        n = scores.numel()
        rec_lims.copy_(lims)
        rec_scores[:n].copy_(scores)
        rec_ids[:n].copy_(ids)
        records = self._all_gather(send, world)
        if rank != 0:
            return None
        if self.range_merge is not None:
            return self.range_merge(*_stacked(range_record_views(r, nq, cap) for r in records))
        return hip_range_merge_packed(records, world, nq, cap, total)

    def search(self, queries: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if _world(self.group)[0] == 1:
            self.last_world = 1
            return self.local_search(queries, k)
        nq = queries.shape[0]
        if record_bytes(nq, k) == 0:
            return self.local_search(queries, k)
        return self.gather_merge(self.search_local(queries, k), nq, k)
