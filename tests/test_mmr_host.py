"""The diversified search without a GPU: the checker's own behaviour on the clustered family (so the GPU tests compare
against something that does diversify), the tie rule, the settings object, the serving flags, and the stages
``DiverseIndex`` refuses."""
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import pytest

import mmr_cases as mc


@pytest.fixture(scope="module")
def family():
    rows, row_c, queries = mc.clustered_family()
    assert rows.shape == (480, 384) and queries.shape == (8, 384)
    S, I = mc.ranking(queries, rows, 50)
    return SimpleNamespace(rows=rows, row_c=row_c, queries=queries, S=S, I=I)


def test_lambda_one_is_the_first_stage(family):
    f = family
    D, I, V, R, counts = mc.mmr_batch(f.S, f.I, f.rows, k=10, lam=1.0)
    assert (counts == 10).all()
    assert np.array_equal(I, f.I[:, :10]) and np.array_equal(mc.bits32(D), mc.bits32(f.S[:, :10]))
    assert np.array_equal(V, f.S[:, :10].astype(np.float64))          # 1.0 * s - 0.0 * r
    assert (R[:, 0] == 0).all() and (R[:, 1:] > 0.9).all()             # the top 10 are one cluster


def test_the_clustered_family_differs_from_top_k_on_every_query(family):
    f = family
    D, I, V, R, counts = mc.mmr_batch(f.S, f.I, f.rows, k=10, lam=0.5)
    assert (counts == 10).all()
    for q in range(8):
        plain, diverse = f.row_c[f.I[q, :10]], f.row_c[I[q]]
        print(f"query {q}: clusters plain {sorted(set(plain))} diverse {sorted(set(diverse))}")
        assert len(set(plain)) == 1
        assert len(set(diverse)) >= 3
        assert I[q].tolist() != f.I[q, :10].tolist()
        assert I[q, 0] == f.I[q, 0]                                    # lambda > 0: the best row comes first
        assert sorted(set(I[q].tolist())) == sorted(I[q].tolist())     # a row is selected once
        assert set(I[q].tolist()) <= set(f.I[q].tolist())
        assert (np.diff(V[q]) <= 0).all()                              # red only grows: the values fall
    # the relevance reported is the list's own
    where = {(q, int(r)): s for q in range(8) for r, s in zip(f.I[q], f.S[q])}
    assert all(mc.bits32(D[q, j]) == mc.bits32(where[(q, int(I[q, j]))]) for q in range(8) for j in range(10))


def test_the_threshold_shortens_lists(family):
    f = family
    D, I, V, R, counts = mc.mmr_batch(f.S, f.I, f.rows, k=10, lam=0.5, dup_threshold=0.8)
    assert (counts < 10).all(), counts
    for q in range(8):
        n = counts[q]
        assert n == len(set(f.row_c[f.I[q]])) >= 3                     # cosine >= 0.8 inside a cluster, below it across
        assert len(set(f.row_c[I[q, :n]])) == n                        # one row per cluster
        assert (I[q, n:] == -1).all() and (D[q, n:] == mc.NEG_PAD).all()
        assert np.isneginf(V[q, n:]).all() and np.isnan(R[q, n:]).all()
        assert (R[q, :n] < 0.8).all()
    # -1 kills everything after the first pick; a threshold nobody reaches changes nothing
    _, I1, _, _, c1 = mc.mmr_batch(f.S, f.I, f.rows, k=10, lam=0.5, dup_threshold=-1.0)
    assert (c1 == 1).all() and np.array_equal(I1[:, 0], f.I[:, 0]) and (I1[:, 1:] == -1).all()
    free = mc.mmr_batch(f.S, f.I, f.rows, k=10, lam=0.5)
    mc.same(mc.mmr_batch(f.S, f.I, f.rows, k=10, lam=0.5, dup_threshold=1.5), free, "threshold 1.5")


def test_ties_go_to_the_earlier_list_position():
    rows, _, queries = mc.clustered_family(twins=8)
    assert np.array_equal(mc.bits32(rows[480]), mc.bits32(rows[0]))
    S, I = mc.ranking(queries[:1], rows, 50)
    at = {int(r): j for j, r in enumerate(I[0])}
    assert 0 in at and 480 in at and at[0] < at[480]                   # equal scores: the lower row first
    assert mc.bits32(S[0, at[0]]) == mc.bits32(S[0, at[480]])
    for order in ((0, 480), (480, 0)):                                 # the twins swapped in the list: the earlier wins
        I2 = I.copy()
        I2[0, at[0]], I2[0, at[480]] = order
        _, J, V, _, _ = mc.mmr_batch(S, I2, rows, k=50, lam=0.5)
        pos = {int(r): j for j, r in enumerate(J[0])}
        assert pos[order[0]] < pos[order[1]]
    # lambda = 0 at the start: every value is 0.0 - 0.0, position 0 wins
    _, J, V, R, _ = mc.mmr_batch(S, I, rows, k=3, lam=0.0)
    assert J[0, 0] == I[0, 0] and V[0, 0] == 0.0 and R[0, 0] == 0.0


def test_candidates_follow_the_list_rule(family):
    f = family
    S, I = f.S[:3].copy(), f.I[:3].copy()
    I[0, 5:] = -1
    I[0, 7] = 3                       # behind the padding: never read
    I[1, 2] = 480                     # outside the index: skipped
    I[1, 3] = -9
    I[2, :] = -1
    D, J, V, R, counts = mc.mmr_batch(S, I, f.rows, k=10, lam=0.5, id_offset=1000)
    assert counts.tolist() == [5, 10, 0]
    assert sorted(J[0, :5].tolist()) == sorted((f.I[0, :5] + 1000).tolist()) and (J[0, 5:] == -1).all()
    assert 1480 not in J[1] and 991 not in J[1]
    assert (J[2] == -1).all()


# ---------------------------------------------------------------------------------------------- settings
def test_diversity_validates():
    from semantic_search_kd_amd import Diversity

    d = Diversity()
    assert (d.lambda_mult, d.fetch_k, d.dup_threshold) == (0.5, 50, None)
    assert d.threshold() == float("inf") and Diversity(dup_threshold=0.8).threshold() == 0.8
    assert d.depth(10) == 50 and d.depth(80) == 80 and Diversity(fetch_k=1024).depth(5000) == 1024
    assert Diversity(lambda_mult=0, fetch_k=1, dup_threshold=-1).lambda_mult == 0.0
    assert Diversity(dup_threshold=float("inf")).threshold() == float("inf")
    for bad in (dict(lambda_mult=-0.1), dict(lambda_mult=1.5), dict(lambda_mult=float("nan")), dict(fetch_k=0),
                dict(fetch_k=1025), dict(fetch_k=2.5), dict(fetch_k=True), dict(dup_threshold=float("nan"))):
        with pytest.raises(ValueError):
            Diversity(**bad)


def test_diverse_index_refuses_sparse_and_fused_stages():
    from semantic_search_kd_amd import BM25Index, DiverseIndex, ExpandedIndex, HybridIndex

    bm25 = BM25Index()
    with pytest.raises(TypeError, match="not cosine relevance"):
        DiverseIndex(bm25)
    with pytest.raises(TypeError, match="not cosine relevance"):
        DiverseIndex(ExpandedIndex(bm25))
    hybrid = HybridIndex(SimpleNamespace(ntotal=3, doc_ids=[]),
                         SimpleNamespace(bm25=SimpleNamespace(corpus_size=3), doc_ids=[]))
    with pytest.raises(TypeError, match="HybridIndex.*not cosine relevance"):
        DiverseIndex(hybrid)
    with pytest.raises(TypeError, match="no first stage"):
        DiverseIndex(object())
    with pytest.raises(TypeError, match="Diversity"):
        DiverseIndex(object(), diversity={"fetch_k": 3})


DIVERSITY_ENV = ("SEMANTIC_KD_FEATURES__ENABLE_DIVERSITY", "SEMANTIC_KD_DIVERSITY__LAMBDA",
                 "SEMANTIC_KD_DIVERSITY__FETCH_K", "SEMANTIC_KD_DIVERSITY__DUP_THRESHOLD")


def test_settings_read_the_diversity_block_from_the_environment(monkeypatch):
    from semantic_search_kd_amd import Diversity
    from semantic_search_kd_amd.serve.app import ServeSettings

    for name in DIVERSITY_ENV:
        monkeypatch.delenv(name, raising=False)
    s = ServeSettings.from_env()
    assert s.diversity_enabled is False and s.diversity() is None and ServeSettings().diversity() is None
    assert s.diversity_dup_threshold is None
    monkeypatch.setenv(DIVERSITY_ENV[0], "true")
    assert ServeSettings.from_env().diversity() == Diversity()
    for name, value in zip(DIVERSITY_ENV[1:], ("0.3", "80", "0.9")):
        monkeypatch.setenv(name, value)
    assert ServeSettings.from_env().diversity() == Diversity(lambda_mult=0.3, fetch_k=80, dup_threshold=0.9)
    monkeypatch.setenv(DIVERSITY_ENV[0], "0")
    assert ServeSettings.from_env().diversity() is None


@pytest.mark.parametrize("flag", [False, True])
def test_search_route_with_the_flag_off_is_what_it_was(flag):
    """Off: the first stage is called as before.  On over an index that is not a single-GPU dense index (here a
    stand-in): nothing is wrapped either."""
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
        settings = ServeSettings(environment="test", diversity_enabled=flag)
        with TestClient(create_app(settings=settings)) as client:
            index = MagicMock()
            index.search.return_value = (np.array([[0.9, 0.8]], np.float32), np.array([[1, 0]], np.int64))
            app_state.index_builder, app_state.doc_ids = index, ["a", "b"]
            body = client.post("/search", json={"query": "what is x", "k": 2}).json()
            assert index.search.call_count == 1 and index.search.call_args[1] == {"k": 2}
            assert [(x["doc_id"], x["rank"]) for x in body["results"]] == [("b", 1), ("a", 2)]
    finally:
        for key, value in vars(app_module.AppState()).items():
            setattr(app_state, key, value)
