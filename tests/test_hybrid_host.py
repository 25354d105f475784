"""Hybrid fusion without a GPU: the checker on hand-worked examples, the C-ABI's argument checks, the settings, the
row-match check of ``HybridIndex`` and the serving route with hybrid retrieval off."""
import ctypes as C
import math
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import pytest

from hybrid_cases import fuse_query

F32 = np.float32


# ---------------------------------------------------------------------------------------------- the checker by hand
def test_checker_rrf_symmetric_tie_goes_to_the_lower_row():
    """Row 5: dense rank 1, BM25 rank 3.  Row 2: dense rank 3, BM25 rank 1.  Equal weights: both fuse to
    1/61 + 1/63 (the sum commutes), row 2 comes first.  Rows 9 (dense rank 2 only) and 7 (BM25 rank 2 only) tie at
    1/62: row 7 first."""
    scores, ids, count, dense, bm25 = fuse_query(
        [F32(0.9), F32(0.8), F32(0.7)], [5, 9, 2], [3.0, 2.0, 1.0], [2, 7, 5],
        n_rows=10, k=6, method="rrf", ws=1.0, wb=1.0, rrf_k=60.0)
    top = 1.0 / 61.0 + 1.0 / 63.0
    assert ids == [2, 5, 7, 9, -1, -1] and count == 4
    assert scores == [top, top, 1.0 / 62.0, 1.0 / 62.0, -math.inf, -math.inf]
    assert dense[:2] == [float(F32(0.7)), float(F32(0.9))] and math.isnan(dense[2]) and dense[3] == float(F32(0.8))
    assert bm25[:3] == [3.0, 1.0, 2.0] and math.isnan(bm25[3])
    assert all(math.isnan(x) for x in dense[4:] + bm25[4:])


def test_checker_linear_with_equal_dense_scores():
    """s_max == s_min: the dense side contributes 0.0 for every row.  Union = rows 3 and 1; row 1 comes from the BM25
    list alone and gets its dense score from the full vector, row 3 has both.  nb = (2 - 1) / (2 - 1) = 1 for row 3,
    0 for row 1: fused = 0.7 * 0 + 0.3 * 1 = 0.3 and 0.0."""
    full_dense = np.full(4, 0.5, np.float32)
    scores, ids, count, dense, bm25 = fuse_query(
        [F32(0.5)], [3], [2.0, 1.0], [3, 1], n_rows=4, k=3, method="linear", ws=0.7, wb=0.3,
        full_dense=full_dense, full_bm25=[0.0, 1.0, 0.0, 2.0])
    assert ids == [3, 1, -1] and count == 2
    assert scores == [0.7 * 0.0 + 0.3 * 1.0, 0.0, -math.inf]
    assert dense[:2] == [0.5, 0.5] and bm25[:2] == [2.0, 1.0]


def test_checker_all_zero_bm25_gives_the_dense_order():
    """Every BM25 entry is +0.0 (the query matched no word): none is a candidate, the output is the dense list."""
    scores, ids, count, dense, bm25 = fuse_query(
        [F32(0.9), F32(0.5), F32(0.1)], [4, 0, 2], [0.0, 0.0, 0.0], [0, 1, 2],
        n_rows=5, k=3, method="rrf", ws=0.7, wb=0.3, rrf_k=60.0)
    assert ids == [4, 0, 2] and count == 3
    assert scores == [0.7 * (1.0 / 61.0), 0.7 * (1.0 / 62.0), 0.7 * (1.0 / 63.0)]
    assert all(math.isnan(x) for x in bm25)
    # the same through linear: the BM25 side is completed to 0.0 everywhere (b_max == b_min), the dense side decides
    scores, ids, _, _, bm25 = fuse_query(
        [F32(0.9), F32(0.5), F32(0.1)], [4, 0, 2], [0.0, 0.0, 0.0], [0, 1, 2], n_rows=5, k=3, method="linear",
        ws=0.7, wb=0.3, full_dense=np.zeros(5, np.float32), full_bm25=[0.0] * 5)
    s = [float(F32(x)) for x in (0.9, 0.5, 0.1)]
    assert ids == [4, 0, 2] and bm25 == [0.0, 0.0, 0.0]
    assert scores == [0.7 * ((x - s[2]) / (s[0] - s[2])) + 0.3 * 0.0 for x in s]


# ---------------------------------------------------------------------------------------------- C-ABI argument checks
P = 4096   # a non-null, 16-byte aligned "pointer": every check comes before the first HIP call, nothing is read


def _call(lib, **over):
    a = dict(d_tiled=P, n_rows=100, d_queries=P, d_dense_scores=P, d_dense_ids=P, kd=10, d_term_offsets=P,
             d_post_rows=P, d_post_w=P, d_idf=P, n_terms=50, d_q_lims=P, d_q_terms=P, d_bm25_scores=P, d_bm25_ids=P,
             kb=10, d_mask=None, method=1, w_semantic=0.7, w_bm25=0.3, rrf_k=60.0, nq=1, k=10, id_offset=0,
             d_out_scores=P, d_out_ids=P, d_out_counts=P, d_out_dense=None, d_out_bm25=None, stream=None)
    unknown = set(over) - set(a)
    assert not unknown, unknown
    a.update(over)
    rc = lib.sskd_hybrid_fuse(*a.values())
    return rc, lib.sskd_last_error().decode()


@pytest.mark.parametrize("over, names", [
    (dict(k=0), "k=0"),
    (dict(k=21), "k=21"),
    (dict(kd=0), "kd=0"),
    (dict(kb=0), "kb=0"),
    (dict(kd=1025, k=1), "kd=1025"),
    (dict(kb=1025, k=1), "kb=1025"),
    (dict(kd=300, kb=300), "kd + kb"),
    (dict(rrf_k=0.0), "rrf_k"),
    (dict(rrf_k=float("nan")), "rrf_k"),
    (dict(w_semantic=-0.5), "w_semantic"),
    (dict(w_semantic=float("inf")), "w_semantic"),
    (dict(w_bm25=float("nan")), "w_bm25"),
    (dict(w_bm25=-1.0), "w_bm25"),
    (dict(method=2), "method=2"),
    (dict(method=-1), "method=-1"),
    (dict(n_rows=(1 << 31) - 64), "n_rows"),
    (dict(n_rows=-1), "n_rows"),
    (dict(nq=-1), "nq"),
    (dict(d_dense_scores=None), "dense ranking"),
    (dict(d_dense_ids=None), "dense ranking"),
    (dict(d_bm25_scores=None), "bm25 ranking"),
    (dict(d_bm25_ids=None), "bm25 ranking"),
    (dict(d_out_scores=None), "output"),
    (dict(d_out_ids=None), "output"),
    (dict(d_out_counts=None), "output"),
    (dict(d_tiled=None), "d_tiled"),
    (dict(d_queries=None), "d_queries"),
    (dict(d_term_offsets=None), "bm25 index tables"),
    (dict(d_post_rows=None), "bm25 index tables"),
    (dict(d_post_w=None), "bm25 index tables"),
    (dict(d_idf=None), "bm25 index tables"),
    (dict(d_q_lims=None), "d_q_lims"),
    (dict(d_q_terms=None), "d_q_terms"),
    (dict(d_tiled=P + 8), "16-byte aligned"),
    (dict(d_queries=P + 4), "16-byte aligned"),
])
def test_fuse_refuses_invalid_arguments_before_any_launch(native_lib, over, names):
    rc, message = _call(native_lib, **over)
    assert rc == 1, (rc, message)
    assert message.startswith("hybrid_fuse:") and names in message, message


def test_fuse_with_no_queries_is_a_no_op(native_lib):
    assert _call(native_lib, nq=0)[0] == 0
    # ... with nothing but the shape: no pointer is looked at
    nulls = {n: None for n in ("d_tiled", "d_queries", "d_dense_scores", "d_dense_ids", "d_term_offsets", "d_post_rows",
                               "d_post_w", "d_idf", "d_q_lims", "d_q_terms", "d_bm25_scores", "d_bm25_ids",
                               "d_out_scores", "d_out_ids", "d_out_counts")}
    assert _call(native_lib, nq=0, method=0, **nulls)[0] == 0
    # the shape is still checked
    assert _call(native_lib, nq=0, k=0)[0] == 1


# ---------------------------------------------------------------------------------------------- settings
HYBRID_ENV = ("SEMANTIC_KD_HYBRID__ENABLED", "SEMANTIC_KD_HYBRID__BM25_INDEX_PATH", "SEMANTIC_KD_HYBRID__BM25_WEIGHT",
              "SEMANTIC_KD_HYBRID__SEMANTIC_WEIGHT", "SEMANTIC_KD_HYBRID__FUSION_METHOD")


def test_settings_read_the_hybrid_block_from_the_environment(monkeypatch):
    from semantic_search_kd_amd.serve.app import ServeSettings

    for name in HYBRID_ENV:
        monkeypatch.delenv(name, raising=False)
    s = ServeSettings.from_env()
    assert s.hybrid_enabled is False
    assert (s.bm25_index_path, s.bm25_weight, s.semantic_weight, s.fusion_method) == (
        "./artifacts/indexes/bm25", 0.3, 0.7, "rrf")
    assert ServeSettings().hybrid_enabled is False
    for name, value in zip(HYBRID_ENV, ("true", "/data/bm25", "0.25", "0.75", "linear")):
        monkeypatch.setenv(name, value)
    s = ServeSettings.from_env()
    assert s.hybrid_enabled is True
    assert (s.bm25_index_path, s.bm25_weight, s.semantic_weight, s.fusion_method) == ("/data/bm25", 0.25, 0.75, "linear")
    monkeypatch.setenv("SEMANTIC_KD_HYBRID__ENABLED", "false")
    assert ServeSettings.from_env().hybrid_enabled is False


# ---------------------------------------------------------------------------------------------- HybridIndex
def _stand_ins(n_dense, n_bm25, dense_ids=None, bm25_ids=None):
    dense = SimpleNamespace(ntotal=n_dense, doc_ids=dense_ids or [])
    bm25 = SimpleNamespace(bm25=SimpleNamespace(corpus_size=n_bm25), doc_ids=bm25_ids or [])
    return dense, bm25


def test_hybrid_index_wants_both_indexes_over_the_same_rows():
    from semantic_search_kd_amd import HybridIndex

    h = HybridIndex(*_stand_ins(3, 3, ["a", "b", "c"], ["a", "b", "c"]))
    assert (h.semantic_weight, h.bm25_weight, h.fusion_method, h.rrf_k, h.depth) == (0.7, 0.3, "rrf", 60.0, 100)
    assert h.clip_depth() == 3 and h.clip_depth(2) == 2
    HybridIndex(*_stand_ins(3, 3, [], ["a", "b", "c"]))   # a dense index built without doc ids: the counts decide
    with pytest.raises(ValueError, match=r"rebuilt after compact\(\)"):
        HybridIndex(*_stand_ins(2, 3, ["a", "c"], ["a", "b", "c"]))   # what compact() after remove_ids leaves
    with pytest.raises(ValueError, match=r"doc_ids differ.*rebuilt after compact\(\)"):
        HybridIndex(*_stand_ins(3, 3, ["a", "b", "c"], ["a", "c", "b"]))
    with pytest.raises(ValueError, match="not loaded"):
        HybridIndex(SimpleNamespace(ntotal=3, doc_ids=[]), SimpleNamespace(bm25=None, doc_ids=[]))
    for bad in (dict(fusion_method="max"), dict(semantic_weight=-1.0), dict(bm25_weight=float("nan")), dict(rrf_k=0.0),
                dict(depth=0)):
        with pytest.raises(ValueError):
            HybridIndex(*_stand_ins(3, 3), **bad)
    # the match is checked again at every search: the dense index may have been compacted since
    h.dense.ntotal = 2
    with pytest.raises(ValueError, match=r"rebuilt after compact\(\)"):
        h.search_device(["q"], None, k=1)


# ---------------------------------------------------------------------------------------------- serving, hybrid off
def test_search_route_with_hybrid_off_goes_to_the_dense_index():
    from fastapi.testclient import TestClient

    from semantic_search_kd_amd.serve import app as app_module
    from semantic_search_kd_amd.serve.app import ServeSettings, app_state, create_app

    for key, value in vars(app_module.AppState()).items():
        setattr(app_state, key, value)
    try:
        student = MagicMock()
        student.embedding_dim = 384
        student.encode_queries.return_value = np.zeros((1, 384), np.float32)
        app_state.student = student
        with TestClient(create_app(settings=ServeSettings(environment="test"))) as client:
            assert app_state.settings.hybrid_enabled is False and app_state.hybrid is None
            index = MagicMock()
            index.search.return_value = (np.array([[0.9, 0.8]], np.float32), np.array([[1, 0]], np.int64))
            app_state.index_builder, app_state.doc_ids = index, ["a", "b"]
            body = client.post("/search", json={"query": "what is x", "k": 2}).json()
            assert [(x["doc_id"], x["rank"]) for x in body["results"]] == [("b", 1), ("a", 2)]
            assert index.search.call_args[1] == {"k": 2}
            assert abs(body["results"][0]["score"] - 0.9) < 1e-6
    finally:
        for key, value in vars(app_module.AppState()).items():
            setattr(app_state, key, value)
