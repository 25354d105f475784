"""Query expansion without a GPU: the forward-index builder against the checker's own counts, the layout of the
expanded CSR, the settings object, the serving flag, and two quality conditions on the checker alone."""
import random
from unittest.mock import MagicMock

import numpy as np
import pytest

import bm25_cases as bc
import expand_cases as ec


# ---------------------------------------------------------------------------------------------- forward index
def _cut_corpus():
    """Zipf texts plus what the cut is about: a row of 400 distinct words (every word once: the 256 lowest term ids
    stay), a row of 300 distinct words where 100 occur twice (those stay, then the lowest 156 of the rest), an empty
    row, a row of exactly 256 distinct words."""
    rng = random.Random(5)
    texts = bc.zipf_corpus(120, 90, 17)
    long_once = [f"x{i}" for i in range(400)]
    rng.shuffle(long_once)
    twice = [f"y{i}" for i in range(300)]
    doubled = twice + twice[100:200]
    rng.shuffle(doubled)
    exact = [f"z{i}" for i in range(256)]
    texts[10:10] = [" ".join(long_once), "", " ".join(doubled), " ".join(exact)]
    return texts


def test_forward_index_equals_the_checkers_counts():
    from semantic_search_kd_amd.bm25 import RM3_ROW_TERMS, BM25Postings

    corpus = [bc.tokenize(t) for t in _cut_corpus()]
    post = BM25Postings(corpus)
    lex = ec.Lexicon(corpus)
    assert RM3_ROW_TERMS == ec.ROW_TERMS == 256
    assert list(post.vocab) == lex.words and post.words == lex.words
    assert post.doc_len.tolist() == lex.dl                                   # dl: the full token count
    # tf of every posting
    got_tf = [dict() for _ in corpus]
    for t in range(post.n_terms):
        lo, hi = post.term_offsets[t], post.term_offsets[t + 1]
        for row, f in zip(post.post_rows[lo:hi].tolist(), post.post_tf[lo:hi].tolist()):
            got_tf[row][t] = f
    assert got_tf == [dict(c) for c in lex.tf]
    lims, terms, p = post.forward_index()
    assert lims.dtype == np.int64 and terms.dtype == np.int32 and p.dtype == np.float64
    assert lims.shape == (len(corpus) + 1,) and lims[0] == 0 and lims[-1] == terms.size == p.size
    for row in range(len(corpus)):
        lo, hi = int(lims[row]), int(lims[row + 1])
        want = lex.fwd[row]
        assert terms[lo:hi].tolist() == list(want), row                        # the kept terms, ascending
        assert [bc.float_bits(x) for x in p[lo:hi].tolist()] == [bc.float_bits(x) for x in want.values()], row
    # the cut and its tie rule did occur
    n_terms = [int(lims[r + 1] - lims[r]) for r in range(len(corpus))]
    assert n_terms[10] == 256 and len(lex.tf[10]) == 400
    kept = set(terms[lims[10]:lims[11]].tolist())
    assert kept == set(sorted(lex.tf[10])[:256])                                # all tf 1: the lower term ids
    assert n_terms[11] == 0
    assert n_terms[12] == 256 and len(lex.tf[12]) == 300
    kept = set(terms[lims[12]:lims[13]].tolist())
    doubled = {t for t, f in lex.tf[12].items() if f == 2}
    once = sorted(t for t, f in lex.tf[12].items() if f == 1)
    assert len(doubled) == 100 and kept == doubled | set(once[:156])            # the larger tf first
    assert n_terms[13] == 256 == len(lex.tf[13])
    # p = tf / dl over the FULL row, also where the row was cut
    lo = int(lims[12])
    assert sorted(set(p[lo:lo + 256].tolist())) == [1 / 400, 2 / 400]


def test_forward_index_of_a_corpus_without_words():
    from semantic_search_kd_amd.bm25 import BM25Postings

    lims, terms, p = BM25Postings([[], []]).forward_index()
    assert lims.tolist() == [0, 0, 0] and terms.size == 0 and p.size == 0


def test_expanded_lims_layout():
    from semantic_search_kd_amd.expand import expanded_lims

    q_lims = np.array([0, 3, 3, 43, 44], np.int64)
    out = expanded_lims(q_lims, 2, 10)
    assert out.dtype == np.int64 and out.tolist() == [0, 16, 26, 116, 128]
    assert expanded_lims(q_lims, 1, 1).tolist() == [0, 4, 5, 46, 48]
    assert expanded_lims(np.array([0], np.int64), 3, 7).tolist() == [0]
    # the checker's segment has that length
    lex = ec.Lexicon([bc.tokenize(t) for t in bc.FIVE_SENTENCES])
    seg = lex.segment(["learning", "unknown", "deep"], [4, 9], fb_terms=5, orig_repeat=3)
    assert seg == [lex.term_id["learning"], lex.term_id["deep"]] * 3 + [4, 9, -1, -1, -1]


# ---------------------------------------------------------------------------------------------- settings
def test_query_expansion_validates():
    from semantic_search_kd_amd import QueryExpansion

    x = QueryExpansion()
    assert (x.fb_docs, x.alpha, x.beta, x.weighting, x.rounds, x.fb_terms, x.orig_repeat, x.max_df_fraction) == (
        5, 1.0, 0.75, "uniform", 1, 10, 2, 0.25)
    assert x.max_df(512) == 128 and x.max_df(3) == 0 and QueryExpansion(max_df_fraction=0).max_df(1000) == 0
    assert QueryExpansion(weighting="SCORE").weighting == "score"
    assert QueryExpansion(fb_docs=16, fb_terms=64, orig_repeat=8, alpha=0, beta=0).lexical_fb_docs() == 16
    for bad in (dict(fb_docs=0), dict(fb_docs=1025), dict(fb_docs=2.5), dict(alpha=-0.1), dict(alpha=float("nan")),
                dict(beta=float("inf")), dict(beta=1e39), dict(weighting="rank"), dict(rounds=0), dict(fb_terms=0),
                dict(fb_terms=65), dict(orig_repeat=0), dict(orig_repeat=9), dict(max_df_fraction=-0.1),
                dict(max_df_fraction=1.5)):
        with pytest.raises(ValueError):
            QueryExpansion(**bad)
    with pytest.raises(ValueError, match="at most 16"):
        QueryExpansion(fb_docs=17).lexical_fb_docs()        # legal for the dense side alone


def test_expanded_index_refuses_what_is_no_first_stage():
    from semantic_search_kd_amd import ExpandedIndex

    with pytest.raises(TypeError, match="no first stage"):
        ExpandedIndex(object())
    with pytest.raises(TypeError, match="QueryExpansion"):
        ExpandedIndex(object(), expansion={"fb_docs": 3})


EXPANSION_ENV = ("SEMANTIC_KD_FEATURES__ENABLE_QUERY_EXPANSION", "SEMANTIC_KD_EXPANSION__FB_DOCS",
                 "SEMANTIC_KD_EXPANSION__FB_TERMS", "SEMANTIC_KD_EXPANSION__ALPHA", "SEMANTIC_KD_EXPANSION__BETA",
                 "SEMANTIC_KD_EXPANSION__ORIG_REPEAT", "SEMANTIC_KD_EXPANSION__MAX_DF_FRACTION")


def test_settings_read_the_expansion_block_from_the_environment(monkeypatch):
    from semantic_search_kd_amd import QueryExpansion
    from semantic_search_kd_amd.serve.app import ServeSettings

    for name in EXPANSION_ENV:
        monkeypatch.delenv(name, raising=False)
    s = ServeSettings.from_env()
    assert s.query_expansion_enabled is False and s.query_expansion() is None and ServeSettings().query_expansion() is None
    monkeypatch.setenv(EXPANSION_ENV[0], "true")
    assert ServeSettings.from_env().query_expansion() == QueryExpansion()
    for name, value in zip(EXPANSION_ENV[1:], ("3", "7", "0", "0.5", "1", "0")):
        monkeypatch.setenv(name, value)
    assert ServeSettings.from_env().query_expansion() == QueryExpansion(fb_docs=3, fb_terms=7, alpha=0.0, beta=0.5,
                                                                       orig_repeat=1, max_df_fraction=0.0)


# ---------------------------------------------------------------------------------------------- serving, flag off
@pytest.mark.parametrize("flag", [False, True])
def test_search_route_with_the_flag_off_is_what_it_was(flag):
    """Off: the first stage is called as before and the response is the same.  On over an index that is not a
    single-GPU dense index (here a stand-in): nothing is wrapped either."""
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
        settings = ServeSettings(environment="test", query_expansion_enabled=flag)
        with TestClient(create_app(settings=settings)) as client:
            assert app_state.settings.query_expansion_enabled is flag
            index = MagicMock()
            index.search.return_value = (np.array([[0.9, 0.8]], np.float32), np.array([[1, 0]], np.int64))
            app_state.index_builder, app_state.doc_ids = index, ["a", "b"]
            body = client.post("/search", json={"query": "what is x", "k": 2}).json()
            assert index.search.call_count == 1 and index.search.call_args[1] == {"k": 2}
            assert index.search.call_args[0][0] is student.encode_queries.return_value
            assert set(body) >= {"query", "results", "total_results", "reranked"}
            assert body["query"] == "what is x" and body["total_results"] == 2 and body["reranked"] is False
            assert [(x["doc_id"], x["rank"], x["text"]) for x in body["results"]] == [("b", 1, ""), ("a", 2, "")]
            assert [x["score"] for x in body["results"]] == [float(np.float32(0.9)), float(np.float32(0.8))]
    finally:
        for key, value in vars(app_module.AppState()).items():
            setattr(app_state, key, value)


# ---------------------------------------------------------------------------------------------- quality, checker alone
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rm3_lifts_precision_on_the_topical_corpus(seed):
    texts, topic = ec.topical_corpus(seed)
    assert len(texts) == 512
    lex = ec.Lexicon([bc.tokenize(t) for t in texts])
    queries, q_topic = ec.topical_queries(seed)
    plain = expanded = 0.0
    for q, t in zip(queries, q_topic):
        rows, _ = lex.oracle.search(q, 20)
        plain += sum(topic[r] == t for r in rows) / 20
        rows, _, _, _ = lex.expand_and_search(q, 20, fb_docs=5, fb_terms=10, orig_repeat=2, max_df=lex.n // 4)
        expanded += sum(topic[r] == t for r in rows) / 20
    plain, expanded = plain / len(queries), expanded / len(queries)
    print(f"seed {seed}: precision@20 plain {plain:.4f} expanded {expanded:.4f}")
    assert expanded >= plain + 0.25


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rocchio_lifts_precision_on_the_clustered_family(seed):
    rows, row_c, queries, q_c = ec.clustered_family(seed)
    assert rows.shape == (64 * 32, 384)

    def precision(q):
        order = np.argsort(-(q @ rows.T), axis=1, kind="stable")
        return order, float(np.mean(row_c[order[:, :10]] == q_c[:, None]))

    order, plain = precision(queries)
    ids = order[:, :5]
    scores = np.take_along_axis(queries @ rows.T, ids, 1)
    new, m = ec.rocchio_batch(queries, scores, ids, rows, fb_docs=5, alpha=1.0, beta=0.75, weighting="uniform")
    assert (m == 5).all()
    new = new / np.linalg.norm(new, axis=1, keepdims=True)
    _, expanded = precision(new.astype(np.float32))
    print(f"seed {seed}: precision@10 plain {plain:.4f} expanded {expanded:.4f}")
    assert expanded >= plain + 0.05
