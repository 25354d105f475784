"""Hybrid fusion on the MI355X against the checker (``hybrid_cases``): the same ids, the same fused bits, the same
components, for every query.

Corpora (built once per module, with their full oracle scores):
  A      700 dense rows x 700 Zipf texts over 60 words - the sweep, the C-ABI cases, masks, batch independence
  B      5 000 rows, 40 words - posting lists of thousands of rows (many binary-search steps), one BM25 tile boundary
  small  200 rows, cosine metric, queries that are not unit vectors - completed scores against the searches' own
The dense indexes of A and B use the inner product, so the oracle's fma-order scores apply to the queries as given.
"""
import json
import logging

import numpy as np
import pandas as pd
import pytest
import torch

import bm25_cases as bc
import hybrid_cases as hc
import ranking_walk_cases as rw
from oracle import search as oracle
from semantic_search_kd_amd import BM25Index, FAISSIndexBuilder, HybridIndex, _native

pytestmark = pytest.mark.gpu

DEPTHS = [1, 10, 63, 64, 65, 100, 256]
WEIGHTS = [(0.7, 0.3), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0)]
NQS = [1, 5, 67]


class Corpus:
    def __init__(self, n, vocab, seed, device, nq=67, metric="ip"):
        self.n = n
        self.rows = oracle.seeded_unit_rows(n, 384, seed)
        self.texts = bc.zipf_corpus(n, vocab, seed)
        self.oracle = bc.Oracle([bc.tokenize(t) for t in self.texts])
        by_df = sorted(self.oracle.postings, key=lambda w: len(self.oracle.postings[w]))
        rare, common = by_df[0], by_df[-1]
        self.queries = [
            bc.zipf_query(vocab, 6, seed + 1),
            "zzz qqq not-a-word",                    # nothing in the vocabulary
            "",                                      # empty
            f"{common} {rare} {common} {common}",    # a repeated token
            rare,                                    # few matches: the +0.0 fill of the BM25 ranking
        ] + [bc.zipf_query(vocab, 1 + i % 9, seed + 10 + i) for i in range(nq - 5)]
        self.emb = oracle.seeded_unit_rows(nq, 384, seed + 2)
        self.dense = self.new_dense(device, metric)
        self.bm25 = BM25Index(device=str(device))
        self.bm25.build_from_texts([f"d{i}" for i in range(n)], self.texts)
        self.full_dense = hc.full_dense_scores(self.emb, self.rows)
        self.full_bm25 = [hc.full_bm25_scores(self.oracle, q) for q in self.queries]
        self.d_emb = torch.from_numpy(self.emb).to(device)
        assert all(s == 0.0 for s in self.full_bm25[1]) and all(s == 0.0 for s in self.full_bm25[2])

    def new_dense(self, device, metric="ip"):
        dense = FAISSIndexBuilder(embedding_dim=384, metric=metric, device=str(device))
        dense.build_from_embeddings(self.rows)
        dense.doc_ids = [f"d{i}" for i in range(self.n)]
        return dense

    def rankings(self, nq, depth, dense=None, allow=None):
        """Both sides' rankings as the searches write them (local rows), on the host."""
        dense = dense or self.dense
        s, i = dense.search_device(self.d_emb[:nq], depth, allow=allow)
        b, j = self.bm25.search_device(self.queries[:nq], depth)
        return s.cpu().numpy(), i.cpu().numpy() - dense.id_offset, b.cpu().numpy(), j.cpu().numpy()

    def want(self, rankings, nq, k, method, ws, wb, **kw):
        return hc.fuse_batch(*rankings, n_rows=self.n, k=k, method=method, ws=ws, wb=wb,
                             full_dense=self.full_dense[:nq], full_bm25=self.full_bm25[:nq], **kw)


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


@pytest.fixture(scope="module")
def corpus_a(gpu):
    return Corpus(700, 60, 11, gpu)


@pytest.fixture(scope="module")
def corpus_b(gpu):
    return Corpus(5000, 40, 23, gpu, nq=5)


# ------------------------------------------------------------------------------------------------ 1: the whole path
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("method", ["rrf", "linear"])
def test_search_device_equals_the_checker(corpus_a, method, depth):
    c = corpus_a
    h = HybridIndex(c.dense, c.bm25, depth=depth, fusion_method=method)
    for nq in NQS:
        rankings = c.rankings(nq, depth)
        for k in sorted({1, min(10, 2 * depth), 2 * depth}):
            for ws, wb in WEIGHTS:
                got = _host(h.search_device(c.queries[:nq], c.d_emb[:nq], k, semantic_weight=ws, bm25_weight=wb,
                                            details=True))
                assert got[0].shape == got[1].shape == got[2].shape == got[3].shape == (nq, k)
                hc.assert_same(got, c.want(rankings, nq, k, method, ws, wb),
                               f"{method} depth={depth} nq={nq} k={k} weights=({ws}, {wb})")


def test_the_sweep_meets_its_cases(corpus_a):
    """What the sweep above is meant to exercise does occur in it."""
    c = corpus_a
    s, i, b, j = c.rankings(67, 100)
    both = [len(set(i[q]) & set(j[q][b[q] != 0.0])) for q in range(67)]
    only_b = [len(set(j[q][b[q] != 0.0]) - set(i[q])) for q in range(67)]
    assert max(both) > 0 and max(only_b) > 0           # rows on both sides, rows to complete
    assert (b[1] == 0.0).all() and (b[2] == 0.0).all()  # the out-of-vocabulary and the empty query
    assert 0 < (b[4] != 0.0).sum() < 100                # a ranking with a +0.0 tail
    _, _, counts, _, _ = c.want((s, i, b, j), 67, 10, "rrf", 0.7, 0.3)
    assert counts.min() == 100 and counts.max() > 150


@pytest.mark.parametrize("method", ["rrf", "linear"])
def test_long_posting_lists_and_a_tile_boundary(corpus_b, method):
    c = corpus_b
    assert max(len(p) for p in c.oracle.postings.values()) > 2000 and c.n > 4096
    h = HybridIndex(c.dense, c.bm25, depth=100, fusion_method=method)
    got = _host(h.search_device(c.queries, c.d_emb, 10, details=True))
    hc.assert_same(got, c.want(c.rankings(5, 100), 5, 10, method, 0.7, 0.3), f"corpus B {method}")
    if method == "linear":   # rows past the BM25 tile boundary were completed
        got = _host(h.search_device(c.queries, c.d_emb, 200, details=True))
        assert (got[1] > 4096).any()
        hc.assert_same(got, c.want(c.rankings(5, 100), 5, 200, method, 0.7, 0.3), "corpus B linear k=200")


# ------------------------------------------------------------------------------------------------ 2: the C-ABI
def capi_fuse(lib, S, I, B, J, *, n_rows, k, method, ws, wb, rrf_k=60.0, id_offset=0, index=None, mask=None):
    """``sskd_hybrid_fuse`` on host rankings; ``index`` = (tiled, queries, offsets, rows, w, idf, n_terms, lims, terms)
    device tensors, or None: NULL index-side pointers (rrf)."""
    dev = "cuda"
    nq, kd = I.shape
    kb = J.shape[1]
    d_s = torch.from_numpy(np.ascontiguousarray(S, np.float32)).to(dev)
    d_i = torch.from_numpy(np.ascontiguousarray(I, np.int64)).to(dev)
    d_b = torch.from_numpy(np.ascontiguousarray(B, np.float64)).to(dev)
    d_j = torch.from_numpy(np.ascontiguousarray(J, np.int64)).to(dev)
    out_s = torch.full((nq, k), 7.0, dtype=torch.float64, device=dev)
    out_i = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
    out_c = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    out_d = torch.full((nq, k), 7.0, dtype=torch.float32, device=dev)
    out_b = torch.full((nq, k), 7.0, dtype=torch.float64, device=dev)
    if index is None:
        ptrs, n_terms = [None] * 8, 0
    else:
        ptrs, n_terms = [t.data_ptr() for t in index[:6] + index[7:]], index[6]
    tiled, queries, offsets, rows, w, idf, lims, terms = ptrs
    _native.check(lib.sskd_hybrid_fuse(
        tiled, n_rows, queries, d_s.data_ptr(), d_i.data_ptr(), kd, offsets, rows, w, idf, n_terms, lims, terms,
        d_b.data_ptr(), d_j.data_ptr(), kb, None if mask is None else mask.data_ptr(), {"rrf": 0, "linear": 1}[method],
        ws, wb, rrf_k, nq, k, id_offset, out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr(), out_d.data_ptr(),
        out_b.data_ptr(), int(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return _host((out_s, out_i, out_d, out_b, out_c))


def _hand_made(n_rows, kd, kb, seed):
    """Six queries of hand-made rankings: full overlap, no overlap, a dense list padded from position 3 on (with rows
    behind the padding that must not count), a BM25 tail of zeros (either sign), ids out of range on both sides, a
    BM25 list that is all padding."""
    g = np.random.default_rng(seed)
    nq = 6
    I = np.stack([g.permutation(n_rows)[:kd] for _ in range(nq)]).astype(np.int64)
    S = -np.sort(-g.standard_normal((nq, kd)).astype(np.float32), axis=1)
    B = -np.sort(-g.uniform(0.5, 9.0, (nq, kb)), axis=1)
    J = np.empty((nq, kb), np.int64)
    for q in range(nq):
        J[q] = np.setdiff1d(np.arange(n_rows), I[q])[g.permutation(n_rows - kd)[:kb]]   # no BM25 row is in the dense list
    m = min(kd, kb)
    J[0, :m] = I[0][g.permutation(kd)[:m]]                                # query 0: (nearly) every one is
    I[2, 3:] = -1
    behind = I[2, 4:8]                                                    # (kd = 5: one entry)
    behind[:] = np.arange(1, 1 + behind.size)                             # behind the first -1: never read as rows
    B[3, kb // 2:] = 0.0
    B[3, -1] = -0.0
    I[4, [0, 2]] = [n_rows, n_rows + 12345]
    I[4, 4] = -5                                                          # negative but not the padding id: skipped
    J[4, [1, 3]] = [n_rows + 1, -9]
    J[5, :] = -1
    B[5, :] = -np.inf
    return S, I, B, J


def test_c_abi_on_hand_made_rankings(native_lib, corpus_a):
    n_rows, kd, kb = 1000, 256, 7
    S, I, B, J = _hand_made(n_rows, kd, kb, 5)
    for k in (1, 20, kd + kb):      # the padded query's union is smaller than 20: padding in the output
        for ws, wb in ((0.7, 0.3), (1.0, 1.0)):
            got = capi_fuse(native_lib, S, I, B, J, n_rows=n_rows, k=k, method="rrf", ws=ws, wb=wb, id_offset=10_000)
            want = hc.fuse_batch(S, I, B, J, n_rows=n_rows, k=k, method="rrf", ws=ws, wb=wb, id_offset=10_000)
            hc.assert_same(got, want, f"hand-made rrf k={k}")
    assert want[2].tolist() == [256, 263, 10, 256 + 3, 253 + 5, 256]
    assert (want[1][2, 10:] == -1).all() and np.isinf(want[0][2, 10:]).all()
    # the long list on the BM25 side
    got = capi_fuse(native_lib, B[:, :5].astype(np.float32), J[:, :5], S.astype(np.float64) + 4.0, I, n_rows=n_rows, k=30,
                    method="rrf", ws=0.3, wb=0.7, rrf_k=1.5)
    hc.assert_same(got, hc.fuse_batch(B[:, :5].astype(np.float32), J[:, :5], S.astype(np.float64) + 4.0, I, n_rows=n_rows,
                                      k=30, method="rrf", ws=0.3, wb=0.7, rrf_k=1.5), "hand-made rrf, kb = 256")


@pytest.mark.parametrize("width", rw.WIDTHS)
def test_c_abi_walk_at_the_round_boundaries(native_lib, width):
    """Both walks (wave 0 the dense list, wave 1 the BM25 list) on the shared hand-made rankings: the first -1 at rank
    0, 63, 64 and absent, rows behind it, ids outside the index and -9 before it (skipped: the walk goes on)."""
    from semantic_search_kd_amd.index import mask_words

    n = 200
    I, J = rw.ids(n, width), rw.ids(n, width, seed=1)
    S = rw.descending_scores(width)
    B = rw.descending_scores(width, np.float64, seed=1).copy()
    B[3, width // 2] = 0.0                       # a row that matched no query word, between survivors
    B[4, width - 1] = -0.0
    allowed = np.ones(n, bool)
    allowed[::7] = False
    mask = torch.from_numpy(mask_words(allowed, n).view(np.int32)).cuda()
    for k in sorted({1, min(20, 2 * width), 2 * width}):
        for ws, wb in ((0.7, 0.3), (1.0, 1.0)):
            for m, a in ((None, None), (mask, allowed)):
                got = capi_fuse(native_lib, S, I, B, J, n_rows=n, k=k, method="rrf", ws=ws, wb=wb, id_offset=10_000, mask=m)
                want = hc.fuse_batch(S, I, B, J, n_rows=n, k=k, method="rrf", ws=ws, wb=wb, id_offset=10_000, allowed=a)
                hc.assert_same(got, want, f"walk width={width} k={k} mask={m is not None}")
    # each side alone (the other list all padding): the union is what that walk kept, counted here by hand
    pad_i, pad_s, pad_b = np.full((rw.NQ, width), -1, np.int64), np.zeros((rw.NQ, width), np.float32), np.zeros((rw.NQ, width))
    end = rw.first_pad(I)
    kept = [int(((I[q, :end[q]] >= 0) & (I[q, :end[q]] < n)).sum()) for q in range(rw.NQ)]
    got = capi_fuse(native_lib, S, I, pad_b, pad_i, n_rows=n, k=width, method="rrf", ws=1.0, wb=1.0)
    hc.assert_same(got, hc.fuse_batch(S, I, pad_b, pad_i, n_rows=n, k=width, method="rrf", ws=1.0, wb=1.0), "dense alone")
    assert got[4].tolist() == kept
    end = rw.first_pad(J)
    kept = [int(((J[q, :end[q]] >= 0) & (J[q, :end[q]] < n) & (B[q, :end[q]] != 0.0)).sum()) for q in range(rw.NQ)]
    got = capi_fuse(native_lib, pad_s, pad_i, B, J, n_rows=n, k=width, method="rrf", ws=1.0, wb=1.0)
    hc.assert_same(got, hc.fuse_batch(pad_s, pad_i, B, J, n_rows=n, k=width, method="rrf", ws=1.0, wb=1.0), "BM25 alone")
    assert got[4].tolist() == kept
    if width >= 63:
        assert kept[4] == width - 2 and kept[0] == 0, "-9 is skipped and the walk goes on; a -1 at rank 0 ends it"


def test_c_abi_mirrored_ranks_tie_and_the_row_decides(native_lib):
    """Equal weights, the BM25 list the dense list reversed: rank_s + rank_b = 33 for every row, so ranks r and 33 - r
    fuse to the same bits and 16 pairs tie exactly."""
    g = np.random.default_rng(9)
    I = np.stack([g.permutation(500)[:32] for _ in range(3)]).astype(np.int64)
    S = np.tile(np.linspace(1, 0, 32, dtype=np.float32), (3, 1))
    J = I[:, ::-1].copy()
    B = np.tile(np.linspace(9, 1, 32), (3, 1))
    got = capi_fuse(native_lib, S, I, B, J, n_rows=500, k=32, method="rrf", ws=1.0, wb=1.0)
    want = hc.fuse_batch(S, I, B, J, n_rows=500, k=32, method="rrf", ws=1.0, wb=1.0)
    hc.assert_same(got, want, "mirrored ranks")
    assert (want[0][:, 0::2] == want[0][:, 1::2]).all() and (want[1][:, 0::2] < want[1][:, 1::2]).all()


def test_c_abi_linear_on_hand_made_rankings(native_lib, corpus_a):
    """kd != kb under linear: hand-made lists over corpus A's rows, the missing scores completed from the real index."""
    c = corpus_a
    nq = 6
    S, I, B, J = _hand_made(c.n, 5, 7, 6)
    S2, I2, B2, J2 = _hand_made(c.n, 256, 7, 7)
    dev, offsets, rows, w, idf = c.bm25._tables()
    lims, terms = c.bm25.query_csr(c.queries[:nq])
    index = (c.dense._tiled, c.d_emb[:nq].contiguous(), offsets, rows, w, idf, c.bm25.bm25.n_terms, lims, terms)
    for (s, i, b, j) in ((S, I, B, J), (S2, I2, B2, J2)):
        for k in (1, 12, i.shape[1] + 7):
            got = capi_fuse(native_lib, s, i, b, j, n_rows=c.n, k=k, method="linear", ws=0.7, wb=0.3, index=index)
            want = hc.fuse_batch(s, i, b, j, n_rows=c.n, k=k, method="linear", ws=0.7, wb=0.3,
                                 full_dense=c.full_dense[:nq], full_bm25=c.full_bm25[:nq])
            hc.assert_same(got, want, f"hand-made linear kd={i.shape[1]} k={k}")


# ------------------------------------------------------------------------------------------------ 3: completed scores
def test_completed_scores_are_the_searches_own_bits(gpu):
    n, nq = 200, 9
    c = Corpus(n, 30, 31, gpu, nq=nq, metric="cosine")
    emb = (c.emb * np.linspace(0.5, 3.0, nq, dtype=np.float32)[:, None]).astype(np.float32)   # not unit: normalised here
    d_emb = torch.from_numpy(emb).to(gpu)
    all_s, all_i = _host(c.dense.search_device(d_emb, n))
    all_b, all_j = _host(c.bm25.search_device(c.queries, 256))
    dense_of = [dict(zip(all_i[q].tolist(), all_s[q].view(np.int32).tolist())) for q in range(nq)]
    bm25_of = [dict(zip(all_j[q].tolist(), all_b[q].view(np.int64).tolist())) for q in range(nq)]
    h = HybridIndex(c.dense, c.bm25, depth=8, fusion_method="linear")
    _, ids, ds, bs, counts = _host(h.search_device(c.queries, d_emb, 16, details=True))
    completed = 0
    for q in range(nq):
        for pos in range(min(16, int(counts[q]))):
            row = int(ids[q, pos])
            assert ds[q, pos].view(np.int32) == dense_of[q][row], (q, row)
            assert bs[q, pos].view(np.int64) == bm25_of[q][row], (q, row)
        completed += int(counts[q]) - 8
    assert completed > 8   # rows one list lacked were among the results


# ------------------------------------------------------------------------------------------------ 4: masks
@pytest.mark.parametrize("method", ["rrf", "linear"])
def test_allow_and_removed_rows_hide_rows_on_both_sides(gpu, corpus_a, method):
    c = corpus_a
    dense = c.new_dense(gpu)
    g = np.random.default_rng(3)
    allow = g.random(c.n) < 0.6
    removed = np.flatnonzero(allow)[::7][:40]
    assert dense.remove_ids(removed.tolist()) == 40
    allowed = allow.copy()
    allowed[removed] = False
    nq, depth, k = 67, 100, 20
    h = HybridIndex(dense, c.bm25, depth=depth, fusion_method=method)
    got = _host(h.search_device(c.queries, c.d_emb, k, allow=allow, details=True))
    rankings = c.rankings(nq, depth, dense=dense, allow=allow)
    assert allowed[rankings[1][rankings[1] >= 0]].all()
    hidden = sum(int((~allowed[j[(j >= 0) & (b != 0.0)]]).sum()) for b, j in zip(rankings[2], rankings[3]))
    assert hidden > 100                                   # the BM25 rankings did hold rows the mask hides
    hc.assert_same(got, c.want(rankings, nq, k, method, 0.7, 0.3, allowed=allowed), f"masked {method}")
    assert allowed[got[1][got[1] >= 0]].all()
    # BM25 ranks are counted among the survivors: the best allowed BM25 row holds BM25 rank 1
    if method == "rrf":
        for q in (0, 3, 5):
            b, j = rankings[2][q], rankings[3][q]
            first = next(int(r) for r, x in zip(j, b) if x != 0.0 and allowed[r])
            one = _host(h.search_device(c.queries[q:q + 1], c.d_emb[q:q + 1], 1, allow=allow, semantic_weight=0.0,
                                        bm25_weight=1.0))
            assert one[1][0, 0] == first and one[0][0, 0] == 1.0 / 61.0


# ------------------------------------------------------------------------------------------------ 5: batch independence
@pytest.mark.parametrize("method", ["rrf", "linear"])
def test_a_batch_equals_its_queries_one_at_a_time(corpus_a, method):
    c = corpus_a
    h = HybridIndex(c.dense, c.bm25, depth=100, fusion_method=method)
    whole = _host(h.search_device(c.queries, c.d_emb, 10, details=True))
    for q in range(67):
        one = _host(h.search_device(c.queries[q:q + 1], c.d_emb[q:q + 1], 10, details=True))
        for a, b in zip(whole, one):
            assert a[q:q + 1].tobytes() == b.tobytes(), (method, q)


def test_numpy_entry_point_and_its_checks(corpus_a):
    c = corpus_a
    h = HybridIndex(c.dense, c.bm25, depth=10)
    d, i = h.search(c.queries[:5], c.emb[:5], k=4)
    dd, di = _host(h.search_device(c.queries[:5], c.d_emb[:5], 4))
    assert d.tobytes() == dd.tobytes() and np.array_equal(i, di)
    bad = c.emb[:5].copy()
    bad[2, 7] = np.nan
    with pytest.raises(ValueError, match="finite"):
        h.search(c.queries[:5], bad, k=4)
    with pytest.raises(ValueError, match="outside"):
        h.search(c.queries[:5], c.emb[:5], k=21)
    with pytest.raises(ValueError, match="query texts"):
        h.search(c.queries[:4], c.emb[:5], k=4)
    assert h.search([], np.zeros((0, 384), np.float32), k=3)[0].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 6: serving
DOCS = [
    "machine learning is a search of the vector index",
    "deep neural networks work",
    "hello world test document",
    "what is semantic search?",
    "the index of a document text",
    "how does a neural network work?",
]


def test_search_route_retrieves_through_the_hybrid_index(gpu, tmp_path, caplog):
    from fastapi.testclient import TestClient

    from semantic_search_kd_amd import BertConfig, build_bm25_index, synthetic_state_dict
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
    corpus, short = tmp_path / "corpus.parquet", tmp_path / "short.parquet"
    frame.to_parquet(corpus)
    frame.iloc[:5].to_parquet(short)
    out = tmp_path / "index"
    assert build_index_main(["--model-path", str(mdir), "--data-path", str(corpus), "--output-dir", str(out),
                             "--batch-size", "4", "--device", "cuda:0", "--hnsw-m", "32", "--hnsw-ef-construction", "200"]) == 0
    build_bm25_index(corpus, tmp_path / "bm25")
    build_bm25_index(short, tmp_path / "bm25_short")
    assert json.loads((tmp_path / "bm25" / "doc_ids.json").read_text()) == json.loads((out / "doc_ids.json").read_text())
    q = "what is semantic search?"

    def serve(bm25_dir):
        for key, value in vars(app_module.AppState()).items():
            setattr(app_state, key, value)
        settings = ServeSettings(environment="test", hybrid_enabled=True, bm25_index_path=str(bm25_dir),
                                 fusion_method="rrf")
        try:
            with TestClient(create_app(student_model_path=str(mdir), device="cuda:0", settings=settings)) as client:
                assert client.post("/index/load", params={"index_path": str(out)}).status_code == 200
                r = client.post("/search", json={"query": q, "k": 3})
                assert r.status_code == 200, r.text
                emb = app_state.student.encode_queries([q])
                return r.json(), app_state.hybrid, app_state.index_builder, emb
        finally:
            for key, value in vars(app_module.AppState()).items():
                setattr(app_state, key, value)

    body, hybrid, builder, emb = serve(tmp_path / "bm25")
    assert isinstance(hybrid, HybridIndex) and hybrid.dense is builder
    d, i = hybrid.search([q], emb, k=3, depth=hybrid.clip_depth(100))
    assert [x["doc_id"] for x in body["results"]] == [f"chunk_{r}" for r in i[0]]
    assert [x["score"] for x in body["results"]] == d[0].tolist()
    assert 3 in i[0]   # the document that is the query: BM25 rank 1
    # a BM25 index over other rows: a warning, and the dense results
    with caplog.at_level(logging.WARNING, logger="semantic_search_kd_amd.serve"):
        body, hybrid, builder, emb = serve(tmp_path / "bm25_short")
    assert hybrid is None
    assert any("dense-only" in rec.getMessage() and "rebuilt after compact()" in rec.getMessage() for rec in caplog.records)
    ds, di = builder.search(emb, k=3)
    assert [x["doc_id"] for x in body["results"]] == [f"chunk_{r}" for r in di[0]]
    np.testing.assert_array_equal(np.array([x["score"] for x in body["results"]], np.float32), ds[0])
