"""``ExpandedIndex`` on the MI355X against the checkers chained: each first stage's own checker (or its own search, where
the stage has no host oracle) around the expansion checker of ``expand_cases``.  Ids exact, scores by bit pattern.

One world, built once: 1 500 seeded unit rows under the inner product (so the oracle's fma-order scores apply to the
expanded queries as they are) and 1 500 Zipf texts over 120 words.
"""
import json

import numpy as np
import pandas as pd
import pytest
import torch

import bm25_cases as bc
import expand_cases as ec
import hybrid_cases as hc
from oracle import search as oracle
from semantic_search_kd_amd import (BM25Index, ExpandedIndex, FAISSIndexBuilder, GraphIndex, HybridIndex, IVFIndex,
                                    QueryExpansion)

pytestmark = pytest.mark.gpu

N, VOCAB, NQ = 1500, 120, 9


class World:
    def __init__(self, device):
        self.device = device
        self.rows = oracle.seeded_unit_rows(N, 384, 71)
        self.emb = oracle.seeded_unit_rows(NQ, 384, 72)
        self.d_emb = torch.from_numpy(self.emb).to(device)
        self.texts = bc.zipf_corpus(N, VOCAB, 73)
        self.lex = ec.Lexicon([bc.tokenize(t) for t in self.texts])
        by_df = sorted(self.lex.words, key=lambda w: len(self.lex.oracle.postings[w]))
        self.queries = [bc.zipf_query(VOCAB, 1 + i % 5, 80 + i) for i in range(NQ - 3)] + [
            "", f"{by_df[0]} zzz {by_df[-1]} {by_df[-1]}", by_df[1]]
        self.flat = self.new_flat()
        self.bm25 = BM25Index(device=str(device))
        self.bm25.build_from_texts([f"d{i}" for i in range(N)], self.texts)

    def new_flat(self):
        flat = FAISSIndexBuilder(embedding_dim=384, metric="ip", device=str(self.device))
        flat.build_from_embeddings(self.rows)
        flat.doc_ids = [f"d{i}" for i in range(N)]
        return flat

    def rocchio(self, x: QueryExpansion, emb=None, search=None):
        """The checker's expanded queries: the first ranking from the oracle, or from ``search(queries, k)``."""
        q = self.emb if emb is None else emb
        for _ in range(x.rounds):
            if search is None:
                s, i = oracle.topk_fma(q, self.rows, x.fb_docs)
            else:
                s, i = search(q, x.fb_docs)
            q, _ = ec.rocchio_batch(q, s, i, self.rows, fb_docs=x.fb_docs, alpha=x.alpha, beta=x.beta,
                                    weighting=x.weighting)
        return q


@pytest.fixture(scope="module")
def world(gpu):
    return World(gpu)


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


def _same_dense(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ"
    assert np.array_equal(ec.bits32(got[0]), ec.bits32(want[0])), f"{what}: score bits differ"


# ---------------------------------------------------------------------------------------------------- dense stages
@pytest.mark.parametrize("weighting", ["uniform", "score"])
def test_flat_index_equals_the_checkers_chained(world, weighting):
    w = world
    for x in (QueryExpansion(weighting=weighting), QueryExpansion(fb_docs=1, alpha=0.0, beta=1.0, weighting=weighting),
              QueryExpansion(fb_docs=16, alpha=0.5, beta=2.0, weighting=weighting)):
        e = ExpandedIndex(w.flat, x)
        for k in (1, 10):
            got = _host(e.search_device(w.d_emb, k))
            _same_dense(got, oracle.topk_fma(w.rocchio(x), w.rows, k), f"flat {x} k={k}")
            assert np.array_equal(e.search(w.emb, k)[1], got[1])
    plain = w.flat.search(w.emb, 10)[1]
    assert not np.array_equal(plain, got[1])            # the expansion does move the ranking
    assert [d["feedback_rows"] for d in e.explain(w.emb)] == [16] * NQ


def test_ivf_with_every_list_probed_equals_the_checkers_chained(world):
    w = world
    ivf = IVFIndex(flat=w.flat)
    ivf.train(nlist=8, iterations=3)
    x = QueryExpansion()
    got = _host(ExpandedIndex(ivf, x).search_device(w.d_emb, 10, nprobe=8))
    _same_dense(got, oracle.topk_fma(w.rocchio(x), w.rows, 10), "ivf, nprobe = nlist")
    # fewer lists: the stage's own search on both sides of the checker
    def search(q, k):
        return _host(ivf.search_device(torch.from_numpy(q).to(w.device), k, nprobe=2))
    got = _host(ExpandedIndex(ivf, x).search_device(w.d_emb, 10, nprobe=2))
    _same_dense(got, search(w.rocchio(x, search=search), 10), "ivf, nprobe = 2")


def test_graph_equals_its_own_search_around_the_checker(world):
    w = world
    graph = GraphIndex(flat=w.flat, M=16)
    graph.build_graph()

    def search(q, k):
        return _host(graph.search_device(torch.from_numpy(q).to(w.device), k, ef=64))

    x = QueryExpansion(weighting="score")
    got = _host(ExpandedIndex(graph, x).search_device(w.d_emb, 10, ef=64))
    _same_dense(got, search(w.rocchio(x, search=search), 10), "graph")


def test_two_rounds_equal_two_manual_rounds(world):
    w = world
    one = ExpandedIndex(w.flat, QueryExpansion(fb_docs=3))
    two = ExpandedIndex(w.flat, QueryExpansion(fb_docs=3, rounds=2))
    q1, _ = one.expand_queries_device(w.d_emb)
    q2, _ = one.expand_queries_device(q1)
    manual = _host(w.flat.search_device(q2, 10))
    got = _host(two.search_device(w.d_emb, 10))
    _same_dense(got, manual, "rounds = 2")
    _same_dense(got, oracle.topk_fma(w.rocchio(two.expansion), w.rows, 10), "rounds = 2 vs the checker")


def test_captured_dense_search_replays_to_the_eager_result(world):
    w = world
    e = ExpandedIndex(w.flat, QueryExpansion())
    static_q = w.d_emb.clone()
    eager = e.search_device(static_q, 10)                      # also sizes the workspace before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            D, I = e.search_device(static_q, 10)
    torch.cuda.current_stream().wait_stream(side)
    D.fill_(0)
    I.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(I, eager[1]) and torch.equal(D.view(torch.int32), eager[0].view(torch.int32))
    # other queries through the same graph
    static_q.copy_(torch.from_numpy(oracle.seeded_unit_rows(NQ, 384, 99)).to(w.device))
    g.replay()
    torch.cuda.synchronize()
    want = e.search_device(static_q, 10)
    assert torch.equal(I, want[1]) and torch.equal(D.view(torch.int32), want[0].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- BM25
def test_bm25_equals_the_checker_and_explain_names_its_words(world):
    w = world
    for x in (QueryExpansion(), QueryExpansion(fb_docs=16, fb_terms=64, orig_repeat=1, max_df_fraction=0.0)):
        e = ExpandedIndex(w.bm25, x)
        got_s, got_i = _host(e.search_device(w.queries, 20))
        told = e.explain(w.queries)
        for q, text in enumerate(w.queries):
            rows, scores, chosen, weights = w.lex.expand_and_search(
                text, 20, fb_docs=x.fb_docs, fb_terms=x.fb_terms, orig_repeat=x.orig_repeat, max_df=x.max_df(N))
            assert got_i[q].tolist() == rows, (q, text)
            assert ec.bits64(got_s[q]).tolist() == ec.bits64(np.array(scores)).tolist(), (q, text)
            assert [t for t, _ in told[q]["terms"]] == [w.lex.words[t] for t in chosen], (q, text)
            assert [bc.float_bits(v) for _, v in told[q]["terms"]] == [bc.float_bits(v) for v in weights], (q, text)
        assert told[NQ - 3]["terms"] == [] and told[NQ - 3]["fb_lexical"] == 0          # the empty query
        assert any(t["terms"] for t in told)
    s, i = e.search(w.queries[:2], 5)
    assert np.array_equal(i, got_i[:2, :5])
    assert e.search_device([], 5)[0].shape == (0, 5)


# ---------------------------------------------------------------------------------------------------- hybrid
def _hybrid_want(w, dense, x, method, depth, k, allow=None, allowed=None):
    """Both sides' own searches around the two expansion checkers, then the fuse checker."""
    def dense_search(q, kk):
        s, i = _host(dense.search_device(torch.from_numpy(np.ascontiguousarray(q)).to(w.device), kk, allow=allow))
        return s, i - dense.id_offset
    q2 = w.rocchio(x, search=dense_search)
    B, J = _host(w.bm25.search_device(w.queries, depth))
    expanded = []
    for q, text in enumerate(w.queries):
        tokens = bc.tokenize(text)
        chosen, _, _ = w.lex.select(tokens, B[q], J[q], fb_docs=x.fb_docs, fb_terms=x.fb_terms, max_df=x.max_df(N),
                                    allowed=allowed)
        expanded.append(w.lex.expanded_tokens(tokens, chosen, orig_repeat=x.orig_repeat))
    full_bm25 = [w.lex.oracle.scores(t) for t in expanded]
    ranked = [w.lex.oracle.rank(f, depth) for f in full_bm25]
    B2 = np.array([r[1] for r in ranked], np.float64)
    J2 = np.array([r[0] for r in ranked], np.int64)
    S2, I2 = dense_search(q2, depth)
    return hc.fuse_batch(S2, I2, B2, J2, n_rows=N, k=k, method=method, ws=0.7, wb=0.3, allowed=allowed,
                         full_dense=oracle.scores_fma(q2, w.rows), full_bm25=full_bm25)


@pytest.mark.parametrize("method", ["rrf", "linear"])
def test_hybrid_equals_the_checkers_chained(world, method):
    w = world
    h = HybridIndex(w.flat, w.bm25, depth=40, fusion_method=method)
    x = QueryExpansion()
    e = ExpandedIndex(h, x)
    got = _host(e.search_device(w.queries, w.d_emb, 15, details=True))
    hc.assert_same(got, _hybrid_want(w, w.flat, x, method, 40, 15), f"hybrid {method}")
    plain = _host(h.search_device(w.queries, w.d_emb, 15))
    assert not np.array_equal(plain[1], got[1])
    d, i = e.search(w.queries, w.emb, k=15)
    assert np.array_equal(i, got[1]) and d.tobytes() == got[0].tobytes()
    told = e.explain(w.queries, w.emb)
    assert all(t["feedback_rows"] == 5 for t in told) and any(t["terms"] for t in told)
    # without the keyword the hybrid index does what it did
    again = _host(h.search_device(w.queries, w.d_emb, 15))
    assert again[0].tobytes() == plain[0].tobytes() and np.array_equal(again[1], plain[1])


@pytest.mark.parametrize("method", ["rrf", "linear"])
def test_allow_and_removed_rows_are_honoured_on_both_sides(world, method):
    w = world
    dense = w.new_flat()
    g = np.random.default_rng(5)
    allow = g.random(N) < 0.5
    removed = np.flatnonzero(allow)[::9][:30]
    assert dense.remove_ids(removed.tolist()) == 30
    allowed = allow.copy()
    allowed[removed] = False
    h = HybridIndex(dense, w.bm25, depth=40, fusion_method=method)
    x = QueryExpansion(fb_docs=4, fb_terms=6)
    got = _host(ExpandedIndex(h, x).search_device(w.queries, w.d_emb, 15, allow=allow, details=True))
    hc.assert_same(got, _hybrid_want(w, dense, x, method, 40, 15, allow=allow, allowed=allowed.tolist()),
                   f"masked hybrid {method}")
    assert allowed[got[1][got[1] >= 0]].all()
    # the mask did change what the lexical side chose
    B, J = _host(w.bm25.search_device(w.queries, 40))
    hidden = sum(int((~allowed[j[(j >= 0) & (b != 0.0)][:4]]).sum()) for b, j in zip(B, J))
    assert hidden > 0
    # the dense stage alone
    e = ExpandedIndex(dense, x)
    got = _host(e.search_device(w.d_emb, 10, allow=allow))
    def search(q, k):
        return _host(dense.search_device(torch.from_numpy(q).to(w.device), k, allow=allow))
    _same_dense(got, search(w.rocchio(x, search=search), 10), "masked flat")
    assert allowed[got[1][got[1] >= 0]].all()


# ---------------------------------------------------------------------------------------------------- serving
DOCS = [
    "machine learning is a search of the vector index",
    "deep neural networks work",
    "hello world test document",
    "what is semantic search?",
    "the index of a document text",
    "how does a neural network work?",
]


def test_search_route_with_the_flag_set_returns_the_expanded_ranking(gpu, tmp_path):
    from fastapi.testclient import TestClient

    from semantic_search_kd_amd import BertConfig, synthetic_state_dict
    from semantic_search_kd_amd.build_index_cli import main as build_index_main
    from semantic_search_kd_amd.serve import app as app_module
    from semantic_search_kd_amd.serve.app import ServeSettings, app_state, create_app
    from semantic_search_kd_amd.weights import save_model_dir
    from test_encoder_gpu import _vocab

    vocab = _vocab()
    cfg = BertConfig(vocab_size=len(vocab), num_hidden_layers=2)
    mdir = tmp_path / "e5-small-v2-synthetic"
    save_model_dir(mdir, cfg, synthetic_state_dict(cfg))
    (mdir / "vocab.txt").write_text("\n".join(vocab))
    frame = pd.DataFrame({"chunk_id": [f"chunk_{i}" for i in range(len(DOCS))], "text": DOCS,
                          "doc_id": [f"doc_{i}" for i in range(len(DOCS))]})
    corpus = tmp_path / "corpus.parquet"
    frame.to_parquet(corpus)
    out = tmp_path / "index"
    assert build_index_main(["--model-path", str(mdir), "--data-path", str(corpus), "--output-dir", str(out),
                             "--batch-size", "4", "--device", "cuda:0", "--hnsw-m", "32", "--hnsw-ef-construction", "200"]) == 0
    assert len(json.loads((out / "doc_ids.json").read_text())) == len(DOCS)
    q = "what is semantic search?"

    def serve(flag):
        for key, value in vars(app_module.AppState()).items():
            setattr(app_state, key, value)
        settings = ServeSettings(environment="test", query_expansion_enabled=flag, expansion_fb_docs=2,
                                 expansion_beta=4.0)
        try:
            with TestClient(create_app(student_model_path=str(mdir), device="cuda:0", settings=settings)) as client:
                assert client.post("/index/load", params={"index_path": str(out)}).status_code == 200
                r = client.post("/search", json={"query": q, "k": 3})
                assert r.status_code == 200, r.text
                return r.json(), app_state.index_builder, app_state.student.encode_queries([q])
        finally:
            for key, value in vars(app_module.AppState()).items():
                setattr(app_state, key, value)

    body, builder, emb = serve(True)
    x = QueryExpansion(fb_docs=2, beta=4.0)
    d, i = ExpandedIndex(builder, x).search(emb, k=3)
    assert [r["doc_id"] for r in body["results"]] == [f"chunk_{r}" for r in i[0]]
    np.testing.assert_array_equal(np.array([r["score"] for r in body["results"]], np.float32), d[0])
    off, builder, emb = serve(False)
    d0, i0 = builder.search(emb, k=3)
    assert [r["doc_id"] for r in off["results"]] == [f"chunk_{r}" for r in i0[0]]
    np.testing.assert_array_equal(np.array([r["score"] for r in off["results"]], np.float32), d0[0])
    assert [r["score"] for r in body["results"]] != [r["score"] for r in off["results"]]
    assert set(body) == set(off) and set(body["results"][0]) == set(off["results"][0])     # the wire schema is the same
