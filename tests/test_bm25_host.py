"""BM25 index, host side (no GPU): the built tables against the dict-and-loop oracle (``bm25_cases``), the reference's
directory format, the stage-1 miner and the curriculum dispatch, and the C-ABI's argument checks."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import bm25_cases as bc
from semantic_search_kd_amd import _native
from semantic_search_kd_amd import mining
from semantic_search_kd_amd.bm25 import BM25Index, BM25Postings

ERR_INVALID = 1


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _check_tables(texts, **params):
    corpus = [bc.tokenize(t) for t in texts]
    oracle = bc.Oracle(corpus, **params)
    post = BM25Postings(corpus, **params)
    words = list(oracle.postings)
    assert list(post.vocab) == words and list(post.vocab.values()) == list(range(len(words)))
    assert post.corpus_size == oracle.n
    assert bc.float_bits(post.avgdl) == bc.float_bits(oracle.avgdl)
    assert bc.float_bits(float(post.average_idf)) == bc.float_bits(oracle.average_idf)
    assert post.idf.dtype == np.float64 and post.idf.shape == (len(words),)
    assert np.array_equal(_bits(post.idf), _bits([oracle.idf[w] for w in words]))
    assert post.term_offsets.dtype == np.int64 and post.post_rows.dtype == np.int32 and post.post_w.dtype == np.float64
    assert post.term_offsets[0] == 0 and post.term_offsets[-1] == len(post.post_rows) == len(post.post_w)
    for t, word in enumerate(words):
        lo, hi = int(post.term_offsets[t]), int(post.term_offsets[t + 1])
        want = sorted(oracle.postings[word].items())
        assert post.post_rows[lo:hi].tolist() == [row for row, _ in want], word
        assert np.array_equal(_bits(post.post_w[lo:hi]), _bits([oracle.weight(f, row) for row, f in want])), word
    return oracle, post


@pytest.mark.parametrize("n_docs,vocab,seed", [(1, 3, 1), (3, 2, 2), (5, 4, 3), (300, 50, 4), (1500, 4000, 5)])
def test_built_tables_equal_the_oracle(n_docs, vocab, seed):
    _check_tables(bc.zipf_corpus(n_docs, vocab, seed))


def test_built_tables_on_the_reference_sentences_and_other_parameters():
    _check_tables(bc.FIVE_SENTENCES)
    _check_tables(bc.FIVE_SENTENCES, k1=1.2, b=0.4, epsilon=0.5)
    _check_tables(bc.zipf_corpus(200, 30, 9), k1=2, b=1.0, epsilon=0.1)


def test_average_idf_is_the_ordered_sum_not_a_pairwise_one():
    oracle, post = _check_tables(bc.zipf_corpus(4000, 6000, 11))
    raw = [oracle.raw_idf[w] for w in oracle.postings]
    assert len(raw) >= 2000
    pairwise = float(np.sum(np.asarray(raw, dtype=np.float64))) / len(raw)
    assert bc.float_bits(pairwise) != bc.float_bits(oracle.average_idf), "this corpus does not tell the two sums apart"
    assert bc.float_bits(float(post.average_idf)) == bc.float_bits(oracle.average_idf)
    assert any(v < 0 for v in raw) and oracle.average_idf > 0    # the replaced idfs depend on the average's bits


def test_term_ids_drop_unknown_tokens_and_keep_repeats():
    post = BM25Postings([bc.tokenize(t) for t in bc.FIVE_SENTENCES])
    v = post.vocab
    assert post.term_ids(["deep", "zzz", "learning", "deep"]) == [v["deep"], v["learning"], v["deep"]]
    assert post.term_ids([]) == [] and post.term_ids(["Deep"]) == []
    with pytest.raises(ValueError):
        BM25Postings([])


# ---------------------------------------------------------------------- save / load
def _five(tmp_path, name="idx"):
    index = BM25Index(str(tmp_path / name))
    index.build_from_texts([f"doc_{i}" for i in range(5)], bc.FIVE_SENTENCES)
    return index


def test_save_load_round_trip_and_checksum(tmp_path):
    index = _five(tmp_path)
    index.save()
    root = tmp_path / "idx"
    assert sorted(p.name for p in root.iterdir()) == ["bm25_params.json", "checksum.json", "doc_ids.json",
                                                      "tokenized_corpus.json"]
    assert json.loads((root / "tokenized_corpus.json").read_text()) == [bc.tokenize(t) for t in bc.FIVE_SENTENCES]
    assert json.loads((root / "bm25_params.json").read_text()) == {"k1": 1.5, "b": 0.75, "epsilon": 0.25, "corpus_size": 5}
    h = hashlib.sha256()
    h.update(json.dumps([f"doc_{i}" for i in range(5)], sort_keys=True).encode())
    h.update(json.dumps([bc.tokenize(t) for t in bc.FIVE_SENTENCES], sort_keys=True).encode())
    assert json.loads((root / "checksum.json").read_text()) == {"sha256": h.hexdigest()}
    again = BM25Index(str(root), auto_load=True)
    assert again.doc_ids == index.doc_ids and again.tokenized_corpus == index.tokenized_corpus
    assert again.bm25.vocab == index.bm25.vocab
    assert np.array_equal(_bits(again.bm25.idf), _bits(index.bm25.idf))
    assert np.array_equal(_bits(again.bm25.post_w), _bits(index.bm25.post_w))
    assert np.array_equal(again.bm25.post_rows, index.bm25.post_rows)
    assert again.get_doc_text("doc_1") == "deep learning uses neural networks with many layers."
    assert again.get_doc_text("nope") == ""


def test_load_rejects_tampering_and_missing_files(tmp_path):
    index = _five(tmp_path)
    index.save()
    root = tmp_path / "idx"
    corpus = json.loads((root / "tokenized_corpus.json").read_text())
    corpus[2][0] = "unnatural"
    (root / "tokenized_corpus.json").write_text(json.dumps(corpus))
    with pytest.raises(ValueError, match="checksum"):
        BM25Index(str(root)).load()
    (root / "tokenized_corpus.json").write_text('[["cut", "off"')
    with pytest.raises(ValueError):
        BM25Index(str(root)).load()
    (root / "tokenized_corpus.json").unlink()
    with pytest.raises(FileNotFoundError):
        BM25Index(str(root)).load()
    assert BM25Index(str(root), auto_load=True).bm25 is None     # auto_load only loads what is there
    with pytest.raises(FileNotFoundError):
        BM25Index(str(tmp_path / "absent")).load()
    with pytest.raises(ValueError):
        BM25Index().save()
    with pytest.raises(ValueError, match="not loaded"):
        BM25Index().search("anything")


def test_load_honours_the_saved_parameters(tmp_path):
    index = _five(tmp_path)
    index.save()
    root = tmp_path / "idx"
    (root / "bm25_params.json").write_text(json.dumps({"k1": 1.2, "b": 0.4, "epsilon": 0.5, "corpus_size": 5}))
    again = BM25Index(str(root))
    again.load()
    assert (again.bm25.k1, again.bm25.b, again.bm25.epsilon) == (1.2, 0.4, 0.5)
    oracle = bc.Oracle([bc.tokenize(t) for t in bc.FIVE_SENTENCES], k1=1.2, b=0.4, epsilon=0.5)
    assert np.array_equal(_bits(again.bm25.idf), _bits([oracle.idf[w] for w in oracle.postings]))
    assert not np.array_equal(_bits(again.bm25.post_w), _bits(index.bm25.post_w))
    again.save()   # and writes them back
    assert json.loads((root / "bm25_params.json").read_text())["k1"] == 1.2


def test_build_from_parquet_writes_the_directory(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq

    from semantic_search_kd_amd import build_bm25_index

    table = pa.table({"chunk_id": [f"doc_{i}" for i in range(5)], "text": bc.FIVE_SENTENCES, "other": list(range(5))})
    pq.write_table(table, tmp_path / "corpus.parquet")
    index = build_bm25_index(tmp_path / "corpus.parquet", tmp_path / "out")
    assert index.doc_ids == [f"doc_{i}" for i in range(5)] and len(index.tokenized_corpus) == 5
    assert (tmp_path / "out" / "checksum.json").exists()
    assert BM25Index(str(tmp_path / "out"), auto_load=True).tokenized_corpus == index.tokenized_corpus


# ---------------------------------------------------------------------- miner and curriculum
class _StubIndex:
    def __init__(self):
        self.calls = []

    def batch_search(self, queries, top_k=100):
        self.calls.append((list(queries), top_k))
        return [[(f"d{j}", 10.0 - j) for j in range(min(top_k, 6))] for _ in queries]


def test_bm25_miner_filters_positives_on_the_host():
    stub = _StubIndex()
    miner = mining.BM25Miner(stub)
    got = miner.mine(["q0", "q1", "q2"], [["d1", "d4"], [], ["zz"]], top_k=5)
    assert got == [["d0", "d2", "d3"], ["d0", "d1", "d2", "d3", "d4"], ["d0", "d1", "d2", "d3", "d4"]]
    assert stub.calls == [(["q0", "q1", "q2"], 5)]          # one batched call
    got = miner.mine(["q0"], [["d1"]], top_k=3, exclude_positives=False)
    assert got == [["d0", "d1", "d2"]]
    assert stub.calls[-1] == (["q0"], 3)
    miner.mine(["q0"], [[]])
    assert stub.calls[-1] == (["q0"], 100)
    with pytest.raises(ValueError):
        miner.mine(["q0", "q1"], [[]])


def test_bm25_miner_loads_a_saved_index(tmp_path):
    index = _five(tmp_path)
    index.save()
    miner = mining.BM25Miner(str(tmp_path / "idx"))
    assert miner.index.doc_ids == index.doc_ids and miner.index.bm25 is not None
    with pytest.raises(FileNotFoundError):
        mining.BM25Miner(str(tmp_path / "absent"))


def _stub_miners(monkeypatch):
    log = []

    class Bm25:
        def __init__(self, path):
            log.append(("bm25", path))

        def mine(self, queries, positives, top_k=100, exclude_positives=True):
            log.append(("bm25.mine", top_k, exclude_positives))
            return [["a", "b", "c", "d", "e", "f", "g"] for _ in queries]

    class Teacher:
        def __init__(self, model, confidence_threshold=0.6):
            log.append(("teacher", model, confidence_threshold))

        def mine(self, queries, candidates, candidate_texts, top_k=10):
            log.append(("teacher.mine", top_k, candidates[0]))
            return [c[:6] for c in candidates], [[0.9, 0.8, 0.7, 0.6, 0.5, 0.4] for _ in candidates]

    class Ance:
        def __init__(self, model, margin=0.1):
            log.append(("ance", model, margin))

        def mine(self, queries, positives, candidates, candidate_texts, positive_texts, top_k=5):
            log.append(("ance.mine", top_k, candidates[0], candidate_texts is positive_texts))
            return [["b", "x"] for _ in queries]

    monkeypatch.setattr(mining, "BM25Miner", Bm25)
    monkeypatch.setattr(mining, "TeacherMiner", Teacher)
    monkeypatch.setattr(mining, "ANCEMiner", Ance)
    return log


def test_curriculum_dispatches_the_three_stages(monkeypatch):
    log = _stub_miners(monkeypatch)
    args = (["q0", "q1"], [["p"], []], "some/dir", "TEACHER", "STUDENT", {"a": "text"})
    negatives, scores = mining.build_mining_curriculum(*args, stage=1)
    assert negatives == [["a", "b", "c", "d", "e", "f", "g"]] * 2 and scores == [[0.0] * 7] * 2
    assert log == [("bm25", "some/dir"), ("bm25.mine", 100, True)]
    del log[:]
    negatives, scores = mining.build_mining_curriculum(*args, stage=2)
    assert negatives == [["a", "b", "c", "d", "e", "f"]] * 2 and scores == [[0.9, 0.8, 0.7, 0.6, 0.5, 0.4]] * 2
    assert log == [("bm25", "some/dir"), ("bm25.mine", 100, True), ("teacher", "TEACHER", 0.6),
                   ("teacher.mine", 10, ["a", "b", "c", "d", "e", "f", "g"])]
    del log[:]
    negatives, scores = mining.build_mining_curriculum(*args, stage=3)
    # first five teacher negatives + the ANCE ones as a set: "b" once, the order unspecified
    assert [sorted(n) for n in negatives] == [["a", "b", "c", "d", "e", "x"]] * 2
    assert scores == [[0.9, 0.8, 0.7, 0.6, 0.5, 0.0, 0.0]] * 2
    assert log == [("bm25", "some/dir"), ("bm25.mine", 100, True), ("teacher", "TEACHER", 0.6),
                   ("teacher.mine", 20, ["a", "b", "c", "d", "e", "f", "g"]), ("ance", "STUDENT", 0.1),
                   ("ance.mine", 5, ["a", "b", "c", "d", "e", "f"], True)]
    for stage in (0, 4):
        with pytest.raises(ValueError, match="Invalid stage"):
            mining.build_mining_curriculum(*args, stage=stage)


def test_package_exports_the_bm25_surface():
    import semantic_search_kd_amd as pkg

    for name in ("BM25Index", "BM25Miner", "build_bm25_index", "build_mining_curriculum"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("build_from_parquet", "build_from_texts", "save", "load", "search", "batch_search", "get_doc_text",
                 "search_device"):
        assert callable(getattr(pkg.BM25Index, name))


# ---------------------------------------------------------------------- C-ABI
def test_bm25_symbols_are_exported(native_lib):
    for name in ("sskd_bm25_search_workspace_bytes", "sskd_bm25_search_plan", "sskd_bm25_search"):
        assert name in _native.SIGNATURES and hasattr(native_lib, name)


def test_workspace_is_monotone_and_the_plan_matches_it(native_lib):
    ws = native_lib.sskd_bm25_search_workspace_bytes
    tile, tiles, chunk = C.c_int(), C.c_int(), C.c_int()
    for n_rows in (1, 5000, 1_000_000, 8_841_823):
        for k in (1, 10, 100, 256):
            sizes = [ws(n_rows, nq, k) for nq in (1, 2, 7, 64, 1000, 100_000)]
            assert sizes[0] > 0 and sizes == sorted(sizes), (n_rows, k, sizes)
        for nq in (1, 64, 100_000):
            sizes = [ws(n_rows, nq, k) for k in (1, 2, 10, 100, 255, 256)]
            assert sizes == sorted(sizes), (n_rows, nq, sizes)
            assert native_lib.sskd_bm25_search_plan(n_rows, nq, 100, tile, tiles, chunk) == 0
            assert tile.value > 0 and tiles.value == -(-n_rows // tile.value)
            assert 1 <= chunk.value <= nq
            assert chunk.value * tiles.value * 100 * 16 <= ws(n_rows, nq, 100)      # 16-byte records
    assert ws(1000, 0, 10) == 0 and ws(1000, 4, 0) == 0 and ws(1000, 4, 257) == 0
    assert native_lib.sskd_bm25_search_plan(1000, 4, 10, None, None, None) == 0
    assert native_lib.sskd_bm25_search_plan(1000, 4, 0, tile, tiles, chunk) == ERR_INVALID
    assert ws(8_841_823, 100_000, 100) <= 512 << 20      # nothing of size N x nq


def _search(lib, n_rows=100, n_terms=7, nq=3, k=10, null=(), workspace_bytes=1 << 20):
    """every pointer is a small host buffer (the checks run before any HIP call) unless named in `null`"""
    buf = (C.c_byte * 64)()
    p = (C.addressof(buf) + 15) & ~15
    ptr = lambda name: None if name in null else p
    return lib.sskd_bm25_search(ptr("term_offsets"), ptr("post_rows"), ptr("post_w"), ptr("idf"), n_rows, n_terms,
                                ptr("q_lims"), ptr("q_terms"), nq, k, ptr("out_scores"), ptr("out_ids"),
                                ptr("workspace"), workspace_bytes, None)


@pytest.mark.parametrize(
    "kwargs,code,message",
    [
        (dict(k=0), 1, b"k=0"),
        (dict(k=257), 1, b"k=257"),
        (dict(k=-3), 1, b"k=-3"),
        (dict(nq=-1), 1, b"nq < 0"),
        (dict(n_rows=-1), 1, b"n_rows < 0"),
        (dict(n_rows=(1 << 31) - 64), 1, b"too large"),
        (dict(n_terms=-1), 1, b"n_terms"),
        (dict(null=("term_offsets",)), 1, b"null"),
        (dict(null=("post_rows",)), 1, b"null"),
        (dict(null=("post_w",)), 1, b"null"),
        (dict(null=("idf",)), 1, b"null"),
        (dict(null=("q_lims",)), 1, b"null"),
        (dict(null=("q_terms",)), 1, b"null"),
        (dict(null=("out_scores",)), 1, b"null"),
        (dict(null=("out_ids",)), 1, b"null"),
        (dict(null=("workspace",)), 2, b"workspace"),
        (dict(workspace_bytes=100), 2, b"workspace"),
    ],
)
def test_bm25_argument_errors_need_no_gpu(native_lib, kwargs, code, message):
    rc = _search(native_lib, **kwargs)
    err = native_lib.sskd_last_error()
    assert rc == code, (kwargs, rc, err)
    assert b"bm25_search" in err and message in err, err


def test_bm25_empty_batch_is_a_no_op(native_lib):
    assert _search(native_lib, nq=0, null=("term_offsets", "out_scores", "workspace")) == 0
