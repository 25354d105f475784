"""Grouped search, host side (no GPU): argument checks through ctypes, workspace sizing, the chunk-id rule and the
oracle walk against the reference's own ``maxsim_aggregation`` (tests/golden/maxsim_small.json)."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import GOLDEN
from grouped_cases import walk
from semantic_search_kd_amd import _native
from semantic_search_kd_amd.index import groups_from_chunk_ids

ERR_INVALID, ERR_WORKSPACE = 1, 2
K_MAX = _native.SSKD_K_MAX


def test_grouped_symbols_are_declared_and_bound(native_lib):
    for name in ("sskd_index_search_grouped_workspace_bytes", "sskd_index_search_grouped"):
        assert name in _native.SIGNATURES and hasattr(native_lib, name)


def _call(lib, n_rows=100, nq=4, k=5, k_rows=32, null=(), ws_bytes=None):
    """every pointer is a small host buffer (the checks run before any HIP call) unless named in `null`"""
    buf = (C.c_byte * 64)()
    p = C.addressof(buf)
    ptr = lambda name: None if name in null else p
    if ws_bytes is None:
        ws_bytes = int(lib.sskd_index_search_grouped_workspace_bytes(max(n_rows, 0), max(nq, 0), k, k_rows)) or 1 << 20
    return lib.sskd_index_search_grouped(
        ptr("tiled"), n_rows, ptr("queries"), nq, k, k_rows, 0, None, ptr("row_group"), ptr("scores"), ptr("ids"),
        ptr("groups"), ptr("count"), ptr("unproved"), ptr("n_unproved"), ptr("ws"), ws_bytes, None)


@pytest.mark.parametrize(
    "kwargs,code,message",
    [
        (dict(k=0), ERR_INVALID, b"k=0"),
        (dict(k=-3), ERR_INVALID, b"k=-3"),
        (dict(k=6, k_rows=5), ERR_INVALID, b"k=6 > k_rows=5"),
        (dict(k=5, k_rows=K_MAX + 1), ERR_INVALID, b"k_rows=1025"),
        (dict(k=K_MAX + 1, k_rows=K_MAX + 1), ERR_INVALID, b"k_rows=1025"),
        (dict(nq=-1), ERR_INVALID, b"nq < 0"),
        (dict(n_rows=-5), ERR_INVALID, b"n_rows < 0"),
        (dict(n_rows=(1 << 31) - 64), ERR_INVALID, b"shard too large"),
        (dict(null=("n_unproved",)), ERR_INVALID, b"null"),
        (dict(null=("n_unproved",), nq=0), ERR_INVALID, b"null"),
        (dict(null=("queries",)), ERR_INVALID, b"null"),
        (dict(null=("tiled",)), ERR_INVALID, b"null"),
        (dict(null=("row_group",)), ERR_INVALID, b"null"),
        (dict(null=("scores",)), ERR_INVALID, b"null"),
        (dict(null=("ids",)), ERR_INVALID, b"null"),
        (dict(null=("groups",)), ERR_INVALID, b"null"),
        (dict(null=("count",)), ERR_INVALID, b"null"),
        (dict(null=("unproved",)), ERR_INVALID, b"null"),
        (dict(null=("ws",)), ERR_WORKSPACE, b"workspace"),
        (dict(ws_bytes=1), ERR_WORKSPACE, b"workspace"),
    ],
)
def test_argument_errors_need_no_gpu(native_lib, kwargs, code, message):
    rc = _call(native_lib, **kwargs)
    err = native_lib.sskd_last_error()
    assert rc == code, (kwargs, rc, err)
    assert b"index_search_grouped" in err and message in err, err


def test_workspace_is_monotone_and_covers_the_row_search(native_lib):
    ws = native_lib.sskd_index_search_grouped_workspace_bytes
    rows_ws = native_lib.sskd_index_search_workspace_bytes
    assert ws(1000, 0, 5, 32) == 0 and ws(-1, 4, 5, 32) == 0 and ws(1000, -1, 5, 32) == 0
    assert ws(1000, 4, 0, 32) == 0 and ws(1000, 4, 6, 5) == 0 and ws(1000, 4, 5, K_MAX + 1) == 0
    nqs = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 1000, 4096, 4097, 10_000)
    k_rows_all = (1, 9, 10, 11, 16, 17, 31, 32, 33, 64, 65, 200, 512, K_MAX)
    for n in (0, 1, 31, 33, 3001, 1_000_000):
        table = np.array([[ws(n, nq, 1, kr) for kr in k_rows_all] for nq in nqs], dtype=np.int64)
        assert (table > 0).all(), n
        assert (np.diff(table, axis=0) >= 0).all(), (n, "not monotone in nq")
        assert (np.diff(table, axis=1) >= 0).all(), (n, "not monotone in k_rows")
        for a, nq in enumerate(nqs):
            for b, kr in enumerate(k_rows_all):
                # the ranking itself (4 B score + 8 B row per rank) on top of the row search's own workspace
                assert table[a, b] >= rows_ws(n, nq, kr) + 12 * nq * kr, (n, nq, kr)
    assert ws(1000, 4, 1, 32) == ws(1000, 4, 32, 32)      # k does not size anything


# ---------------------------------------------------------------------------------------------------------------------
# the reference's rule for chunk ids and its aggregation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maxsim():
    return json.loads((GOLDEN / "maxsim_small.json").read_text())


def test_groups_from_chunk_ids_matches_the_reference(maxsim):
    pairs, doc_scores = maxsim["pairs"], maxsim["doc_scores"]
    assert 25 <= len(pairs) <= 40
    ids = [cid for cid, _ in pairs]
    assert any(cid.count("_") >= 3 for cid in ids) and any("_" not in cid for cid in ids)
    docs = groups_from_chunk_ids(ids)
    assert set(docs) == set(doc_scores)
    # per document: the best of its chunks is what the reference kept
    best = {}
    for doc, (_, score) in zip(docs, pairs):
        best[doc] = max(best.get(doc, -np.inf), score)
    assert best == doc_scores
    assert groups_from_chunk_ids(["a_b_c_12", "nounderscore", "x_", "_0", ""]) == ["a_b_c", "nounderscore", "x", "", ""]


@pytest.mark.parametrize("k", [1, 3, 10, 15, 20])
def test_oracle_walk_agrees_with_the_reference_aggregation(maxsim, k):
    pairs, doc_scores = maxsim["pairs"], maxsim["doc_scores"]
    docs = groups_from_chunk_ids([cid for cid, _ in pairs])
    keys = sorted(set(docs), key=docs.index)                  # group numbers follow first appearance
    groups = np.array([keys.index(d) for d in docs], np.int32)
    scores = np.array([s for _, s in pairs], np.float32)
    assert [float(s) for s in scores] == [s for _, s in pairs], "the fixture's scores must be exact in fp32"
    D, I, G, count, _ = walk(scores, groups, k)
    want = sorted(doc_scores.items(), key=lambda kv: -kv[1])[:k]   # no two documents share their best score
    assert count == len(want) == min(k, len(doc_scores))
    assert [keys[g] for g in G[:count]] == [doc for doc, _ in want]
    assert [float(d) for d in D[:count]] == [s for _, s in want]
    for i, g in zip(I[:count], G[:count]):                           # the representative is the group's best chunk
        assert groups[i] == g and scores[i] == scores[groups == g].max()
    assert (I[count:] == -1).all() and (G[count:] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# group bookkeeping of the product class (host state only: no row is stored)
# ---------------------------------------------------------------------------------------------------------------------
def _builder(n_rows=0):
    from semantic_search_kd_amd import FAISSIndexBuilder

    b = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    b._n = n_rows
    return b


def test_group_numbers_follow_first_appearance_and_none_is_a_singleton():
    b = _builder()
    assert b.group_keys is None and b.max_group_size == 1
    b._extend_groups(0, 6, ["d1", "d2", "d1", None, None, "d2"])
    b._n = 6
    assert b.row_groups().tolist() == [0, 1, 0, 2, 3, 1] and b.group_keys == ["d1", "d2", None, None]
    assert b.max_group_size == 2 and b.n_groups == 4
    b._extend_groups(6, 3, ["d2", "d3", "d1"])            # a known key joins its group
    b._n = 9
    assert b.row_groups().tolist() == [0, 1, 0, 2, 3, 1, 1, 4, 0] and b.max_group_size == 3
    b._extend_groups(9, 2, None)                          # rows without keys: singletons
    b._n = 11
    assert b.row_groups().tolist()[-2:] == [5, 6] and b.group_keys[-2:] == [None, None]
    assert b._rows_of_groups([1, 4]).tolist() == [1, 5, 6, 7] and b._rows_of_groups([]).size == 0
    assert b.group_key(1) == "d2" and b.group_key(-1) is None
    assert b.group_key(np.array([[0, 4], [-1, 5]])) == [["d1", "d3"], [None, None]]
    b.set_groups(list("aabbbbbcccd"))
    assert b.row_groups().tolist() == [0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 3] and b.max_group_size == 5
    with pytest.raises(ValueError):
        b.set_groups(["x"])


def test_rows_before_the_first_keys_become_singletons_and_no_groups_means_rows():
    b = _builder(4)
    assert b.row_groups().tolist() == [0, 1, 2, 3] and b.n_groups == 4 and b.group_key(2) is None
    assert b._rows_of_groups([3, 1]).tolist() == [3, 1]
    assert b._default_k_rows(10) == 10 and b._default_k_rows(33) == 33 and b._default_k_rows(1) == 1
    b._extend_groups(4, 3, ["d", "d", "e"])
    b._n = 7
    assert b.row_groups().tolist() == [0, 1, 2, 3, 4, 4, 5] and b.group_keys == [None] * 4 + ["d", "e"]
    assert b._default_k_rows(10) == 19 and b._default_k_rows(17) == 32 and b._default_k_rows(40) == 40
