"""BM25 search on the MI355X against the dict-and-loop oracle (``bm25_cases``): identical rows and identical score bits.

Corpora: Zipf text, 1 - 30 tokens per document, at N = 1, 3, 5 (average_idf < 0: the replaced idfs are negative, so
matching documents rank BELOW untouched ones), at T - 1, T, T + 1 and 3 T + 17 rows (T = the kernel's tile, from
``sskd_bm25_search_plan``: one tile short of full, exactly full, one row into a second tile, four tiles with a ragged
last one).  Each corpus is built and its oracle scores computed once per session; every case is one device call."""
import ctypes as C

import numpy as np
import pytest
import torch

import bm25_cases as bc
from semantic_search_kd_amd import BM25Index

pytestmark = pytest.mark.gpu

SIZES = ["1", "3", "5", "T-1", "T", "T+1", "3T+17"]
KS = [1, 10, 100, 256]
VOCAB_LARGE = 6000


def _tile_rows(native_lib):
    tile = C.c_int()
    assert native_lib.sskd_bm25_search_plan(1000, 1, 10, tile, None, None) == 0
    return tile.value


class Case:
    def __init__(self, label, tile, device):
        self.label = label
        small = label in ("1", "3", "5")
        self.n = n = int(label) if small else {"T-1": tile - 1, "T": tile, "T+1": tile + 1, "3T+17": 3 * tile + 17}[label]
        self.tile = tile
        if small:
            # two words, 10+ tokens per document: every word sits in (nearly) every document
            texts = bc.zipf_corpus(n, 2, seed=100 + n, min_len=10, max_len=30)
        else:
            texts = bc.zipf_corpus(n, VOCAB_LARGE, seed=len(label) * 1000 + n)
        # identical documents: equal scores for every query, inside a tile and across a tile boundary
        self.twins = [r for r in (3, 7) if r < n]
        if n > 7:
            texts[7] = texts[3]
        if n > tile:
            texts[n - 1] = texts[3]
            self.twins.append(n - 1)
        self.texts = texts
        corpus = [bc.tokenize(t) for t in texts]
        self.oracle = oracle = bc.Oracle(corpus)
        self.index = BM25Index(device=str(device))
        self.index.build_from_texts([f"d{i}" for i in range(n)], texts)
        by_df = sorted(oracle.postings, key=lambda w: len(oracle.postings[w]))
        self.rare, self.common = by_df[0], by_df[-1]
        self.queries = [
            "",                                              # empty: all +0.0, rows 0 .. k-1
            "zzz qqq not-a-word",                            # nothing in the vocabulary
            f"{self.common} {self.rare} {self.common} {self.common}",       # a repeated token
            bc.zipf_query(2 if small else VOCAB_LARGE, 40, seed=7 + n),      # 40 tokens
            self.common,                                     # the longest posting list alone
            self.rare,                                       # few matches: the +0.0 fill
            texts[min(3, n - 1)],                            # the twins' own text
            f"W1 {self.rare.upper()} w2",                    # the tokeniser lowers
        ]
        self.scores = [oracle.scores(bc.tokenize(q)) for q in self.queries]
        self._assert_the_cases_are_real()

    def _assert_the_cases_are_real(self):
        o = self.oracle
        if self.n <= 5:
            assert o.average_idf < 0
            _, top = o.rank(self.scores[2], 10)
            assert any(s < 0 for s in top), "no negative score among the best of a small corpus"
        else:
            assert o.average_idf > 0
            assert len(o.postings[self.common]) > self.n / 2 and o.raw_idf[self.common] < 0 < o.idf[self.common]
            assert len(o.postings[self.rare]) < 10, "the rare word matches too many documents for the +0.0 fill"
            assert sum(1 for s in self.scores[5] if s != 0.0) < 10
            assert self.texts[3] == self.texts[7]
            s = self.scores[6]
            assert s[3] == s[7] and s[3] > 0
            if self.n > self.tile:
                assert self.twins[-1] // self.tile != 3 // self.tile and s[self.twins[-1]] == s[3]
            if self.n > 2 * self.tile:
                assert len(o.postings[self.common]) > self.tile      # one token, a posting list longer than a tile
        assert all(s == 0.0 for s in self.scores[0]) and all(s == 0.0 for s in self.scores[1])

    def expect(self, qi, k):
        """(rows, score bits) of query qi as the device lays them out: the oracle's ranking, padded to k"""
        rows, scores = self.oracle.rank(self.scores[qi], k)
        pad = k - len(rows)
        return (np.array(rows + [-1] * pad, dtype=np.int64),
                np.array(scores + [-np.inf] * pad, dtype=np.float64).view(np.int64))


@pytest.fixture(scope="module")
def cases(native_lib, gpu):
    tile = _tile_rows(native_lib)
    built = {}

    def get(label):
        if label not in built:
            built[label] = Case(label, tile, gpu)
        return built[label]

    return get


def _run(index, queries, k, **kw):
    d, i = index.search_device(queries, k, **kw)
    assert d.dtype == torch.float64 and i.dtype == torch.int64 and d.shape == i.shape == (len(queries), k)
    return i.cpu().numpy(), d.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("label", SIZES)
def test_search_device_equals_the_oracle_bit_for_bit(cases, label, k):
    case = cases(label)
    ids, bits = _run(case.index, case.queries, k)
    for qi, query in enumerate(case.queries):
        want_ids, want_bits = case.expect(qi, k)
        assert np.array_equal(ids[qi], want_ids), (label, k, query[:40], ids[qi][:12], want_ids[:12])
        assert np.array_equal(bits[qi], want_bits), (label, k, query[:40])


def test_ties_keep_row_order_across_a_tile_boundary(cases):
    case = cases("3T+17")
    ids, bits = _run(case.index, [case.texts[3]], 10)
    a, b, c = case.twins
    where = [ids[0].tolist().index(r) for r in (a, b, c)]
    assert where == sorted(where) and where[2] - where[0] == 2       # adjacent, lower row first
    assert bits[0][where[0]] == bits[0][where[1]] == bits[0][where[2]]


def test_a_batch_equals_its_queries_one_by_one_and_chunked(cases, native_lib):
    case = cases("3T+17")
    queries = [bc.zipf_query(VOCAB_LARGE, 1 + (j % 9), seed=500 + j) for j in range(62)] + ["", case.common]
    k = 10
    ids, bits = _run(case.index, queries, k)
    again_ids, again_bits = _run(case.index, queries, k)
    assert np.array_equal(ids, again_ids) and np.array_equal(bits, again_bits)       # two runs, identical bits
    for qi in (0, 17, 63):                                                           # against the oracle as well
        want_rows, want_scores = case.oracle.search(queries[qi], k)
        assert ids[qi].tolist() == want_rows
        assert bits[qi].tolist() == [bc.float_bits(s) for s in want_scores]
    # five queries per chunk: 13 chunks through one small workspace
    one = native_lib.sskd_bm25_search_workspace_bytes(case.n, 1, k)
    chunk_ids, chunk_bits = _run(case.index, queries, k, max_workspace_bytes=5 * one)
    assert np.array_equal(ids, chunk_ids) and np.array_equal(bits, chunk_bits)
    single = [_run(case.index, [q], k) for q in queries]
    assert np.array_equal(ids, np.concatenate([s[0] for s in single]))
    assert np.array_equal(bits, np.concatenate([s[1] for s in single]))


def test_search_returns_doc_ids_and_floats_like_the_reference(gpu):
    index = BM25Index(device=str(gpu))
    index.build_from_texts([f"doc_{i}" for i in range(5)], bc.FIVE_SENTENCES)
    results = index.search("neural networks deep learning", top_k=5)
    assert len(results) == 5 and all(isinstance(d, str) and isinstance(s, float) for d, s in results)
    assert "doc_1" in [d for d, _ in results[:2]]
    scores = [s for _, s in results]
    assert scores == sorted(scores, reverse=True)
    oracle = bc.Oracle([bc.tokenize(t) for t in bc.FIVE_SENTENCES])
    rows, want = oracle.search("neural networks deep learning", 5)
    assert [d for d, _ in results] == [f"doc_{r}" for r in rows]
    assert [bc.float_bits(s) for s in scores] == [bc.float_bits(s) for s in want]
    assert len(index.search("machine learning", top_k=100)) == 5          # the reference's slice stops at the corpus
    batch = index.batch_search(["machine learning", "", "computer vision"], top_k=3)
    assert [len(b) for b in batch] == [3, 3, 3] and batch[1] == [("doc_0", 0.0), ("doc_1", 0.0), ("doc_2", 0.0)]
    assert batch[0] == index.search("machine learning", top_k=3)
    assert index.batch_search([], top_k=3) == [] and index.search("x", top_k=0) == []
    with pytest.raises(ValueError):
        index.search_device(["x"], 257)
