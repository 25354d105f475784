"""``ShardedIndex.range_search`` and ``ShardedIndex.search(allow=...)`` on the MI355X with real HBM shards.

``build_sharded`` writes a two-shard directory; two processes load it into a ``ShardedIndex`` (rank 0 calls, rank 1
serves) and every answer must be bit for bit that of ONE ``FAISSIndexBuilder`` over the whole corpus, with the same
filter and the same removed rows.  On a box with >= 2 GPUs the data group is RCCL; on the one-GPU test box both ranks
share cuda:0 and the records cross through a host-staged gloo all-gather.  One case returns more results per rank than
the default ``range_capacity`` (65 536), so the local call's retry path runs.  World size 1 (no process group) runs in
the test process itself."""
import os
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import search as oracle
from semantic_search_kd_amd.dist import shard_bounds
from semantic_search_kd_amd.sharded_index import ShardedIndex, build_sharded
from test_sharded_index import _free_port

N = 6000
NQ = 48


def _rows():
    rows = oracle.seeded_unit_rows(N, 384, 2024)
    rows[4500] = rows[10]            # the same row in both shards: equal scores, ordered by id
    rows[N - 7] = rows[10]
    return rows


def _queries():
    q = oracle.seeded_unit_rows(NQ, 384, 77)
    q[1:8] = _rows()[10] + 0.05 * q[1:8]
    q[1:8] /= np.linalg.norm(q[1:8], axis=1, keepdims=True)
    return q


def _thresholds():
    """every other query takes every row (24 x 3000 = 72 000 results per rank > 65 536); the others a spread of
    counts, nothing, and NaN"""
    s = oracle.scores_fma(_queries(), _rows())
    thr = np.empty(NQ, np.float32)
    for q in range(NQ):
        desc = np.sort(s[q])[::-1]
        thr[q] = -np.inf if q % 2 == 0 else [desc[0], desc[3], desc[40], desc[N // 3], np.nan][(q // 2) % 5]
    return thr


class RowsModel:
    """duck-typed StudentModel: text "t<i>" -> row i"""

    embedding_dim = 384

    def encode_documents(self, docs, batch_size=32, show_progress=False):
        return _rows()[[int(d[1:]) for d in docs]]


def _corpus(tmp: Path) -> Path:
    path = tmp / "corpus.parquet"
    if not path.exists():
        pd.DataFrame({"chunk_id": [f"c{i}" for i in range(N)], "text": [f"t{i}" for i in range(N)]}).to_parquet(path)
    return path


def _filters():
    rng = np.random.default_rng(3)
    mask = rng.random(N) < 0.5
    ids = np.sort(rng.choice(N, 900, replace=False)).astype(np.int64)
    return [(None, "none"), (mask, "bool"), (ids, "ids")]


def _same_range(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


def _check_against_single(index, dev, tmp, world):
    """rank 0 (or the one process): sharded answers == one FAISSIndexBuilder over the whole corpus"""
    from semantic_search_kd_amd import FAISSIndexBuilder

    ref = FAISSIndexBuilder(embedding_dim=384, metric="ip", device=dev)
    ref.add(_rows())
    q, thr = _queries(), _thresholds()
    for removed in (False, True):
        if removed:
            _, top = ref.search(q, 3)
            gone = np.unique(np.concatenate([top.ravel(), [0, shard_bounds(N, 2, 1)[0], N - 1]]))
            assert index.remove_ids(gone) == gone.size and ref.remove_ids(gone) == gone.size
        for allow, what in _filters():
            got = index.range_search(q, thr, allow=allow)
            want = ref.range_search(q, thr, allow=allow)
            _same_range(got, want, ("range", what, removed))
            if allow is None and not removed:
                assert want[0][-1] > 2 * 65536
            s, i = index.search(q, 10, allow=allow)
            rs, ri = ref.search(q, 10, allow=allow)
            assert np.array_equal(i, ri) and np.array_equal(s.view(np.uint32), rs.view(np.uint32)), ("search", what, removed)
    got = index.range_search(q[5], 0.1)
    _same_range(got, ref.range_search(q[5], 0.1), "one query, scalar threshold")
    assert index.local.range_capacity > 65536, "the local range call never took its retry path"
    (Path(tmp) / f"gpu_range_ok_w{world}").write_text("ok")


def _worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    multi = torch.cuda.device_count() >= world
    dev = f"cuda:{rank if multi else 0}"
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl" if multi else "gloo", rank=rank, world_size=world,
                            **({"device_id": torch.device(dev)} if multi else {}))
    try:
        out = Path(tmp) / "index"
        build_sharded(RowsModel(), _corpus(Path(tmp)), out, batch_size=256, device=dev, metric="ip")
        index = ShardedIndex(device=dev)
        index.load_all_ranks(out)
        if rank != 0:
            index.serve_forever()
            return
        _check_against_single(index, dev, tmp, world)
        index.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_range_and_filtered_search_two_ranks_gpu(gpu, tmp_path):
    _corpus(tmp_path)
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert (tmp_path / "gpu_range_ok_w2").exists()
    # world size 1: one process holds both shards, the calls go straight to its local index
    single = ShardedIndex(device="cuda:0")
    single.load(tmp_path / "index")
    assert single.local.ntotal == N
    _check_against_single(single, "cuda:0", str(tmp_path), 1)
    assert (tmp_path / "gpu_range_ok_w1").exists()
