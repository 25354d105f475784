"""``ShardedIndex.range_search`` and ``ShardedIndex.search(allow=...)`` over gloo (world 1, 2 and 4), with an
oracle-backed stand-in for each rank's HBM shard: the protocol (header, queries / thresholds / filter on the control
group, each rank's slice of the global filter, status exchange, the two all-gathers of the range path), its argument
checks on rank 0 and its failure path.  The HIP merge is replaced by a numpy merge in the kernel's key order; the
GPU tests of the same path are in test_sharded_range_gpu.py and test_range_merge_gpu.py."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import search as oracle
from semantic_search_kd_amd.dist import shard_bounds
from semantic_search_kd_amd.sharded_index import ShardedIndex, ShardFailure, build_sharded
from test_sharded_index import N_DOCS, _ROWS, OracleIndex, SeededModel, _corpus, _free_port, _oracle_merge, _queries


def ordered(s: np.ndarray) -> np.ndarray:
    """the monotone integer image of a float (the range kernel's float_to_ordered): +0.0 ranks above -0.0"""
    b = np.ascontiguousarray(s, np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, b ^ 0x7FFFFFFF)


def range_of_scores(s: np.ndarray, thr: np.ndarray, id_offset: int = 0):
    """the range rule on a score matrix (-inf = excluded rows): every column scoring > thr[q], ordered by the
    monotone image of the score descending, then id ascending; faiss' (lims, D, I)"""
    lims, D, I = [0], [], []
    for q in range(s.shape[0]):
        sel = np.flatnonzero(s[q] > thr[q])
        sel = sel[np.lexsort((sel, -ordered(s[q, sel])))]
        D.append(s[q, sel])
        I.append(sel.astype(np.int64) + id_offset)
        lims.append(lims[-1] + sel.size)
    return np.array(lims, np.int64), np.concatenate(D).astype(np.float32), np.concatenate(I).astype(np.int64)


def numpy_range_merge(all_lims, all_s, all_i):
    """CPU stand-in of sskd_range_merge_packed: per query, the runs' segments in the range kernel's order"""
    all_lims, all_s, all_i = all_lims.numpy(), all_s.numpy(), all_i.numpy()
    g, nq = all_lims.shape[0], all_lims.shape[1] - 1
    lims, D, I = [0], [], []
    for q in range(nq):
        s = np.concatenate([all_s[r, all_lims[r, q] : all_lims[r, q + 1]] for r in range(g)])
        i = np.concatenate([all_i[r, all_lims[r, q] : all_lims[r, q + 1]] for r in range(g)])
        o = np.lexsort((i, -ordered(s)))
        D.append(s[o])
        I.append(i[o])
        lims.append(lims[-1] + s.size)
    return torch.tensor(lims, dtype=torch.int64), torch.from_numpy(np.concatenate(D)), torch.from_numpy(np.concatenate(I))


class FilterOracleIndex(OracleIndex):
    """The oracle stand-in with tombstones, a local ``allow`` (bool per local row, or global ids) and range search.
    ``search_device`` / ``range_search_device`` raise while <tmp>/fail_<what>_rank<r> exists (removed on use)."""

    tmp = None

    def __init__(self, embedding_dim, metric, device, id_offset):
        super().__init__(embedding_dim, metric, device, id_offset)
        self.removed = set()

    @property
    def ntotal(self):
        return len(self.rows)

    def remove_ids(self, ids):
        new = set((np.asarray(ids, np.int64) - self.id_offset).tolist()) - self.removed
        self.removed |= new
        return len(new)

    def _maybe_fail(self, what):
        flag = Path(FilterOracleIndex.tmp) / f"fail_{what}_rank{dist.get_rank() if dist.is_initialized() else 0}"
        if flag.exists():
            flag.unlink()
            raise RuntimeError(f"HIP error: injected {what} failure")

    def _scores(self, q, allow):
        s = oracle.scores_fma(q.numpy(), self.rows)
        dead = np.zeros(len(self.rows), np.bool_)
        dead[sorted(self.removed)] = True
        if allow is not None:
            a = np.asarray(allow)
            if a.dtype == np.bool_:
                assert a.shape == (len(self.rows),)
                dead |= ~a
            else:
                rows = a.astype(np.int64) - self.id_offset
                assert rows.size == 0 or (rows.min() >= 0 and rows.max() < len(self.rows))
                keep = np.zeros(len(self.rows), np.bool_)
                keep[rows] = True
                dead |= ~keep
        s[:, dead] = -np.inf
        return s

    def search_device(self, q, k, normalize_queries=None, out_scores=None, out_ids=None, allow=None):
        self._maybe_fail("search")
        s, i = oracle.topk_of_scores(self._scores(q, allow), k, self.id_offset)
        return torch.from_numpy(s), torch.from_numpy(i)

    def range_search_device(self, q, threshold, *, allow=None, normalize_queries=None):
        self._maybe_fail("range")
        lims, D, I = range_of_scores(self._scores(q, allow), threshold.numpy(), self.id_offset)
        return torch.from_numpy(lims), torch.from_numpy(D), torch.from_numpy(I)


def _factory(embedding_dim, metric, device, id_offset):
    return FilterOracleIndex(embedding_dim, metric, device, id_offset)


def _cpu_merges(index):
    index._searcher.merge = _oracle_merge
    index._searcher.range_merge = numpy_range_merge


def _thresholds(s):
    """per query: nothing, 1, 5, about half, every row, a NaN (matches nothing), in turn"""
    thr = np.empty(s.shape[0], np.float32)
    for q in range(s.shape[0]):
        desc = np.sort(s[q])[::-1]
        thr[q] = [desc[0], desc[1], desc[5], desc[s.shape[1] // 2], -np.inf, np.nan][q % 6]
    return thr


def _expected_scores(removed, allowed=None):
    s = oracle.scores_fma(_queries(), _ROWS)
    dead = np.zeros(N_DOCS, np.bool_)
    dead[sorted(removed)] = True
    if allowed is not None:
        dead |= ~allowed
    s[:, dead] = -np.inf
    return s


def _same_range(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


def _same_topk(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


def _check_calls(index, tmp, world):
    """rank 0 (or the one process of world 1): every filtered / range call against the oracle over the whole corpus"""
    q = _queries()
    full = oracle.scores_fma(q, _ROWS)
    thr = _thresholds(full)
    rng = np.random.default_rng(world)
    gone = np.array(sorted({0, 7, N_DOCS - 1, shard_bounds(N_DOCS, world, world - 1)[0], 101}), np.int64)
    assert index.remove_ids(gone) == gone.size
    removed = set(gone.tolist())
    mask = rng.random(N_DOCS) < 0.6
    ids = np.sort(rng.choice(N_DOCS, 70, replace=False)).astype(np.int64)
    id_mask = np.zeros(N_DOCS, np.bool_)
    id_mask[ids] = True
    for allow, allowed, what in ((None, None, "none"), (mask, mask, "bool"), (ids, id_mask, "ids"),
                                 (torch.from_numpy(mask), mask, "bool tensor"), (ids.astype(np.int32), id_mask, "int32 ids"),
                                 (np.zeros(0, np.int64), np.zeros(N_DOCS, np.bool_), "empty ids")):
        s = _expected_scores(removed, allowed)
        want = range_of_scores(s, thr)
        _same_range(index.range_search(q, thr, allow=allow), want, ("range", what))
        _same_topk(index.search(q, 10, allow=allow), oracle.topk_of_scores(s, 10), ("search", what))
    # a scalar threshold, one query given 1-D, and no queries at all
    s = _expected_scores(removed)
    _same_range(index.range_search(q, float(np.median(full))), range_of_scores(s, np.full(len(q), np.float32(np.median(full)))), "scalar")
    _same_range(index.range_search(q[3], thr[3:4]), range_of_scores(s[3:4], thr[3:4]), "1-D")
    lims, D, I = index.range_search(np.zeros((0, 384), np.float32), 0.0)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0
    # every call that is wrong in itself is refused on rank 0 before the others hear of it; the next call still works
    for bad in (lambda: index.range_search(q, thr[:3]),
                lambda: index.range_search(q, thr, allow=mask[:-1]),
                lambda: index.search(q, 10, allow=np.ones(N_DOCS + 1, np.bool_)),
                lambda: index.search(q, 10, allow=np.array([N_DOCS])),
                lambda: index.range_search(q, thr, allow=np.array([-1])),
                lambda: index.search(q, 10, allow=np.array([0.5, 2.0])),
                lambda: index.range_search(np.zeros((2, 100), np.float32), 0.0)):
        with pytest.raises(ValueError):
            bad()
    _same_range(index.range_search(q, thr, allow=mask), range_of_scores(_expected_scores(removed, mask), thr), "after errors")
    if world == 1:
        return
    # one rank's local part raises: ShardFailure naming it on rank 0, and the deployment keeps serving
    for r, what, call in ((world - 1, "range", lambda: index.range_search(q, thr)),
                          (0, "range", lambda: index.range_search(q, thr, allow=ids)),
                          (1, "search", lambda: index.search(q, 10, allow=mask))):
        (Path(tmp) / f"fail_{what}_rank{r}").write_text("x")
        with pytest.raises(ShardFailure) as err:
            call()
        assert list(err.value.failures) == [r] and f"injected {what} failure" in str(err.value), err.value
        assert index.is_loaded and index.last_failure == err.value.failures
        _same_range(index.range_search(q, thr), range_of_scores(s, thr), ("after failure", r, what))
        assert index.last_failure is None
    _same_topk(index.search(q, 10), oracle.topk_of_scores(s, 10), "unfiltered after failures")


def _build_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        build_sharded(SeededModel(), _corpus(Path(tmp)), Path(tmp) / "index", batch_size=16, index_factory=_factory)
    finally:
        dist.destroy_process_group()


def _serve_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    FilterOracleIndex.tmp = tmp
    try:
        index = ShardedIndex(index_factory=_factory, op_timeout_s=30.0)
        index.load_all_ranks(Path(tmp) / "index")
        _cpu_merges(index)
        if rank != 0:
            index.serve_forever()
            return
        _check_calls(index, tmp, world)
        index.close()
        (Path(tmp) / f"range_ok_w{world}").write_text("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_range_and_filtered_search_over_gloo(tmp_path, world):
    _corpus(tmp_path)
    mp.spawn(_build_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    mp.spawn(_serve_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert (tmp_path / f"range_ok_w{world}").exists()


def _record_groups(data):
    """wrap the collectives the sharded index calls; returns the names of those called on the ``data`` group"""
    on_data = []
    for name in ("broadcast", "all_gather_into_tensor", "all_reduce", "broadcast_object_list"):
        def wrapped(*args, _orig=getattr(dist, name), _name=name, **kwargs):
            if kwargs.get("group") is data:
                on_data.append(_name)
            return _orig(*args, **kwargs)

        setattr(dist, name, wrapped)
    return on_data


def _groups_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    FilterOracleIndex.tmp = tmp
    try:
        data, ctrl = dist.new_group(backend="gloo"), dist.new_group(backend="gloo")
        index = ShardedIndex(group=data, ctrl_group=ctrl, index_factory=_factory, op_timeout_s=30.0)
        index.load_all_ranks(Path(tmp) / "index")
        _cpu_merges(index)
        on_data = _record_groups(data)
        if rank != 0:
            index.serve_forever()   # the same collectives as rank 0: only the record all-gathers of the good calls
            assert on_data == ["all_gather_into_tensor"] * int((Path(tmp) / "data_calls").read_text()), on_data
            (Path(tmp) / f"groups_ok_rank{rank}").write_text("ok")
            return
        q = _queries()
        s = _expected_scores(set())
        thr = _thresholds(s)
        mask = np.arange(N_DOCS) % 3 != 0
        # a rank's local part raises: nothing reaches the data group, on any rank
        for r, what, call in ((1, "search", lambda: index.search(q, 10)),
                              (0, "search", lambda: index.search(q, 10)),
                              (1, "search", lambda: index.search(q, 10, allow=mask)),
                              (1, "range", lambda: index.range_search(q, thr)),
                              (0, "range", lambda: index.range_search(q, thr, allow=mask))):
            (Path(tmp) / f"fail_{what}_rank{r}").write_text("x")
            with pytest.raises(ShardFailure):
                call()
            assert on_data == [], (r, what, on_data)
        # load and remove stay on the control group; a good search or range call enters the data group only with
        # the record all-gathers (one for a search, the totals and the records for a range search)
        index.load(Path(tmp) / "index")
        assert index.remove_ids([5]) == 1 and on_data == []
        s = _expected_scores({5})
        for n, call, check in ((1, lambda: index.search(q, 10), lambda got: _same_topk(got, oracle.topk_of_scores(s, 10), "")),
                               (1, lambda: index.search(q, 10, allow=mask),
                                lambda got: _same_topk(got, oracle.topk_of_scores(_expected_scores({5}, mask), 10), "")),
                               (2, lambda: index.range_search(q, thr), lambda got: _same_range(got, range_of_scores(s, thr), ""))):
            before = len(on_data)
            check(call())
            assert on_data[before:] == ["all_gather_into_tensor"] * n, on_data
        (Path(tmp) / "data_calls").write_text(str(len(on_data)))
        index.close()
    finally:
        dist.destroy_process_group()


def test_sharded_calls_enter_the_data_group_only_after_agreement(tmp_path):
    """data and control on two separate gloo groups: a call in which some rank's local part fails makes no call on the
    data group at all, and a good search or range call uses it only for the record all-gathers"""
    _corpus(tmp_path)
    mp.spawn(_build_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    mp.spawn(_groups_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "groups_ok_rank1").exists()


def test_sharded_range_and_filtered_search_world_one(tmp_path):
    """no process group: the calls go straight to the one local index holding every shard"""
    _corpus(tmp_path)
    mp.spawn(_build_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    FilterOracleIndex.tmp = str(tmp_path)
    index = ShardedIndex(index_factory=_factory)
    index.load(tmp_path / "index")
    assert index.local.ntotal == N_DOCS
    _check_calls(index, str(tmp_path), 1)


def test_numpy_range_rule_orders_signed_zeros_and_ties():
    """the CPU rule the tests compare against: +0.0 before -0.0, equal scores by id"""
    s = np.array([[0.0, -0.0, 0.5, 0.5, -1.0, np.nan]], np.float32)
    lims, D, I = range_of_scores(s, np.array([-0.5], np.float32))
    assert lims.tolist() == [0, 4] and I.tolist() == [2, 3, 0, 1]
    assert np.signbit(D).tolist() == [False, False, False, True]


def test_range_record_layout_matches_the_c_abi(native_lib):
    """the packed range record: lims [nq + 1] int64, ids [cap] int64, scores [cap] fp32, padded to 16 B"""
    from semantic_search_kd_amd.dist import range_record_bytes, range_record_views

    for nq, cap in ((0, 0), (1, 0), (1, 1), (3, 5), (10_000, 1_250_000), (7, 2**31)):
        assert int(native_lib.sskd_range_record_bytes(nq, cap)) == range_record_bytes(nq, cap)
        assert range_record_bytes(nq, cap) % 16 == 0 and range_record_bytes(nq, cap) >= (nq + 1) * 8 + cap * 12
    assert native_lib.sskd_range_record_bytes(-1, 4) == 0 and native_lib.sskd_range_record_bytes(4, -1) == 0
    rec = torch.zeros(range_record_bytes(2, 3), dtype=torch.uint8)
    lims, scores, ids = range_record_views(rec, 2, 3)
    lims.copy_(torch.tensor([0, 1, 3]))
    ids.copy_(torch.tensor([5, 6, 7]))
    scores.copy_(torch.tensor([0.5, -0.0, 1.0]))
    raw = rec.numpy()
    assert raw[:24].view(np.int64).tolist() == [0, 1, 3] and raw[24:48].view(np.int64).tolist() == [5, 6, 7]
    assert raw[48:60].view(np.float32).tolist() == [0.5, -0.0, 1.0]
    ws = native_lib.sskd_range_merge_workspace_bytes
    assert ws(8, 10_000, 10**7) >= 3 * 8 and ws(8, 0, 5) == 0 and ws(0, 5, 5) == 0 and ws(8, 5, -1) == 0
