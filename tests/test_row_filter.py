"""Filtered search and document removal, the parts that need no GPU: the C-ABI symbols, the host-side normalisation
of a filter into mask words, and ``ShardedIndex.remove_ids`` over gloo with an oracle-backed stand-in index.
The last test also runs on the MI355X with real shards (``-m gpu``)."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import search as oracle
from semantic_search_kd_amd.dist import shard_bounds
from semantic_search_kd_amd.index import RowFilter, mask_words
from semantic_search_kd_amd.sharded_index import ShardedIndex, build_sharded
from test_sharded_index import N_DOCS, _ROWS, OracleIndex, SeededModel, _corpus, _free_port, _oracle_merge, _queries

NEW_SYMBOLS = ["sskd_row_mask_words", "sskd_row_mask_pack", "sskd_row_mask_update", "sskd_row_mask_and",
               "sskd_row_mask_count", "sskd_index_search_filtered", "sskd_index_search_screened_filtered",
               "sskd_index_search_onepass_filtered"]


def test_filter_symbols_are_declared_and_exported(native_lib):
    from semantic_search_kd_amd import _native
    from test_capi_symbols import _declared_symbols

    declared = _declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(native_lib, name), name
    assert native_lib.sskd_row_mask_words(0) == 0
    assert native_lib.sskd_row_mask_words(1) == 1 and native_lib.sskd_row_mask_words(32) == 1
    assert native_lib.sskd_row_mask_words(33) == 2 and native_lib.sskd_row_mask_words(1_000_000) == 31_250
    # the filtered calls validate like the unfiltered ones (no device needed to reach the check)
    assert native_lib.sskd_index_search_filtered(None, 10, None, 1, 0, 0, None, None, None, None, 0, None, None,
                                                 None, None) == 1
    assert b"k=0" in native_lib.sskd_last_error()
    assert native_lib.sskd_row_mask_update(None, 10, None, 0, 0, None, None) == 1


@pytest.mark.parametrize("n", [1, 31, 32, 33, 100, 1000])
def test_host_filter_words_match_packbits(n):
    rng = np.random.default_rng(n)
    flags = rng.random(n) < 0.4
    want = np.packbits(flags, bitorder="little")
    want = np.concatenate([want, np.zeros(-want.size % 4, np.uint8)]).view("<u4")
    got = mask_words(flags, n)
    assert got.dtype == np.dtype("<u4") and np.array_equal(got, want)
    assert np.array_equal(mask_words(np.flatnonzero(flags), n), want)        # the same rows as an id list
    assert np.array_equal(mask_words(np.flatnonzero(flags).astype(np.int32), n), want)
    # bit (r & 31) of word (r >> 5)
    for r in np.flatnonzero(flags)[:5]:
        assert (int(got[r >> 5]) >> (r & 31)) & 1
    assert not mask_words(np.zeros(0, np.int64), n).any()


def test_host_filter_rejects_bad_input():
    with pytest.raises(ValueError):
        mask_words(np.ones(5, bool), 6)            # a bool filter covers every row
    with pytest.raises(ValueError):
        mask_words(np.array([6]), 6)               # ids outside the index
    with pytest.raises(ValueError):
        mask_words(np.array([-1]), 6)
    with pytest.raises(TypeError):
        mask_words(np.array([0.5]), 6)
    f = RowFilter(torch.zeros(1, dtype=torch.int32), 7)
    assert f.n_rows == 7


# ----------------------------------------------------------------------------- ShardedIndex.remove_ids over gloo
class RemovableOracleIndex(OracleIndex):
    """The oracle stand-in of test_sharded_index.py with tombstones: removed rows score -inf (never returned)."""

    def __init__(self, embedding_dim, metric, device, id_offset):
        super().__init__(embedding_dim, metric, device, id_offset)
        self.removed = set()

    @property
    def ntotal(self):
        return len(self.rows)

    def remove_ids(self, ids):
        rows = np.asarray(ids, np.int64) - self.id_offset
        if rows.size and (rows.min() < 0 or rows.max() >= len(self.rows)):
            raise ValueError("ids outside the index")
        new = set(rows.tolist()) - self.removed
        self.removed |= new
        return len(new)

    def search_device(self, q, k, normalize_queries=None, out_scores=None, out_ids=None):
        s = oracle.scores_fma(q.numpy(), self.rows)
        s[:, sorted(self.removed)] = -np.inf
        s, i = oracle.topk_of_scores(s, k, self.id_offset)
        return torch.from_numpy(s), torch.from_numpy(i)


def _factory(embedding_dim, metric, device, id_offset):
    return RemovableOracleIndex(embedding_dim, metric, device, id_offset)


def _expected(removed, k):
    s = oracle.scores_fma(_queries(), _ROWS)
    s[:, sorted(removed)] = -np.inf
    return oracle.topk_of_scores(s, k)


def _build_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        build_sharded(SeededModel(), _corpus(Path(tmp)), Path(tmp) / "index", batch_size=16, index_factory=_factory)
    finally:
        dist.destroy_process_group()


def _remove_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        index = ShardedIndex(index_factory=_factory)
        index.load_all_ranks(Path(tmp) / "index")
        index._searcher.merge = _oracle_merge
        if rank != 0:
            index.serve_forever()
            # every rank dropped exactly its share
            lo, hi = shard_bounds(N_DOCS, world, rank)
            got = {r + lo for r in index.local.removed}
            want = set(np.load(Path(tmp) / "removed.npy").tolist())
            assert got == {g for g in want if lo <= g < hi}, (rank, got)
            return
        _, top = index.search(_queries(), 10)
        gone = np.unique(np.concatenate([top[:, :2].ravel(), [0, N_DOCS - 1], [shard_bounds(N_DOCS, world, 1)[0]]]))
        np.save(Path(tmp) / "removed.npy", gone)
        assert index.remove_ids(gone) == gone.size
        assert index.remove_ids(gone[:3]) == 0                   # again: no error, nothing new
        with pytest.raises(ValueError):
            index.remove_ids([N_DOCS])                           # rank 0 rejects it before announcing anything
        s, i = index.search(_queries(), 10)
        assert not np.isin(i, gone).any()
        ref_s, ref_i = _expected(set(gone.tolist()), 10)
        assert np.array_equal(i, ref_i) and np.array_equal(s, ref_s)
        index.close()
        (Path(tmp) / "remove_ok").write_text("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_remove_ids_over_gloo(tmp_path, world):
    _corpus(tmp_path)
    mp.spawn(_build_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    mp.spawn(_remove_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert (tmp_path / "remove_ok").exists()


# ----------------------------------------------------------------------------- GPU: the real shards
def _gpu_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    multi = torch.cuda.device_count() >= world
    dev = f"cuda:{rank if multi else 0}"
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if multi else "gloo", rank=rank, world_size=world,
                            **({"device_id": torch.device(dev)} if multi else {}))
    try:
        out = Path(tmp) / "gpu_index"
        build_sharded(SeededModel(), _corpus(Path(tmp)), out, batch_size=16, device=dev, metric="ip")
        index = ShardedIndex(device=dev)
        index.load_all_ranks(out)
        if rank != 0:
            index.serve_forever()
            return
        _, top = index.search(_queries(), 10)
        gone = np.unique(np.concatenate([top[:, :3].ravel(), [shard_bounds(N_DOCS, world, 1)[0]]]))
        assert index.remove_ids(gone) == gone.size
        s, i = index.search(_queries(), 10)
        ref_s, ref_i = _expected(set(gone.tolist()), 10)
        assert np.array_equal(i, ref_i) and np.array_equal(s, ref_s)
        index.close()
        (Path(tmp) / "gpu_remove_ok").write_text("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_remove_ids_two_ranks_gpu(gpu, tmp_path):
    """build_sharded -> ShardedIndex.load -> rank 0 removes global ids (top hits on both shards) -> every later search
    on the real HBM shards equals the oracle over the remaining rows."""
    _corpus(tmp_path)
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_gpu_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert (tmp_path / "gpu_remove_ok").exists()
