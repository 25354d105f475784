"""Retrieval evaluation without a GPU: the host metric functions against what the reference's own code returned
(tests/golden/eval_small.*, made by tests/golden/make_golden_eval.py), the summation model of the oracle against
``np.sum``, qrels parsing, the C-ABI's argument checks and the command-line tool with the model calls stubbed."""
import ctypes as C
import json

import numpy as np
import pytest

import eval_cases
from conftest import GOLDEN

from semantic_search_kd_amd import evaluation


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "eval_small.json").read_text()), np.load(GOLDEN / "eval_small.npz")


# ------------------------------------------------------------------------------------------- metric functions
def test_ndcg_and_mrr_equal_the_reference_bit_for_bit(golden):
    want = golden[0]["graded"]
    cases = eval_cases.graded_lists()
    assert len(cases) == len(want) and any(len(g) == 0 for g, _ in cases) and any(k > len(g) > 0 for g, k in cases)
    for (grades, k), ref in zip(cases, want):
        assert evaluation.ndcg_at_k(grades, k) == ref["ndcg"], (grades, k)
        assert evaluation.mrr_at_k(grades, k) == ref["mrr"], (grades, k)


def test_recall_and_precision_equal_the_reference_bit_for_bit(golden):
    want = golden[0]["ids"]
    cases = eval_cases.id_cases()
    assert len(cases) == len(want) and any(k > len(ret) for _, ret, k in cases)
    for (relevant, retrieved, k), ref in zip(cases, want):
        assert evaluation.recall_at_k(relevant, retrieved, k) == ref["recall"]
        assert evaluation.precision_at_k(relevant, retrieved, k) == ref["precision"]


def test_compute_retrieval_metrics_equals_the_reference(golden):
    want = golden[0]["compute_retrieval_metrics"]
    results = [{"retrieved_ids": ret, "relevant_ids": rel, "scores": g}
               for (g, _), (rel, ret, _) in zip(eval_cases.graded_lists(), eval_cases.id_cases()[3:])]
    plain = [{"retrieved_ids": r["retrieved_ids"], "relevant_ids": r["relevant_ids"]} for r in results]
    for key, got in (("graded_default_k", evaluation.compute_retrieval_metrics(results)),
                     ("graded_k_1_5_20", evaluation.compute_retrieval_metrics(results, k_values=[1, 5, 20])),
                     ("binary_default_k", evaluation.compute_retrieval_metrics(plain))):
        assert {k: float(v) for k, v in got.items()} == want[key], key


def test_ece_equals_the_reference_bit_for_bit(golden):
    want, arrays = golden[0]["ece"], golden[1]
    for i, ref in enumerate(want):
        conf, acc, bins = arrays[f"ece_conf_{i}"], arrays[f"ece_acc_{i}"], int(arrays[f"ece_bins_{i}"])
        assert eval_cases.away_from_edges(conf, bins)          # the stored confidences keep clear of every bin edge
        assert float(evaluation.expected_calibration_error(conf, acc, n_bins=bins)) == ref


def test_kendall_tau_matches_the_reference(golden):
    """Two fp64 roundings of a value of magnitude <= 1 (about 3e-16): 1e-12 is slack, not a measurement."""
    want = golden[0]["kendall"]
    cases = eval_cases.ranking_pairs()
    assert len(cases) == len(want)
    for (a, b), ref in zip(cases, want):
        assert abs(evaluation.kendall_tau(a, b) - ref) <= 1e-12, (a, b)
    assert evaluation.kendall_tau([1, 2], [3, 4]) == 0.0 and evaluation.kendall_tau([1, 2], [2, 1]) == -1.0


def test_tau_from_discordant_counts():
    taus = evaluation.tau_from_discordant([0, 1, 2, 2, 4, 4], [0, 0, 0, 1, 0, 6])
    assert taus.tolist() == [0.0, 0.0, 1.0, -1.0, 1.0, -1.0]


# ------------------------------------------------------------------------------------------- the oracle's own footing
def test_summation_model_equals_np_sum():
    rng = np.random.default_rng(123)
    for trial in range(2000):
        m = int(rng.integers(1, 257)) if trial >= 256 else trial + 1      # every length 1 .. 256, then random ones
        a = rng.standard_normal(m) * 10.0 ** rng.integers(-3, 4, m)
        assert eval_cases.np_sum_model(a) == np.sum(a), m


def test_oracle_by_hand():
    """Ranked grades 0, 2, 1 with one judged grade 3 that was not retrieved."""
    out = eval_cases.oracle_metrics([0, 2, 1], [0, 2, 1, 3], (1, 2, 10), 0)
    d = np.log2(np.arange(2, 6))
    assert out[0].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert out[1].tolist() == [(0.0 + 2.0 / d[1]) / (2.0 / d[0] + 0.0), 0.5, 1.0 / 3.0, 0.5]
    assert out[2].tolist() == [(0.0 + 2.0 / d[1] + 1.0 / d[2]) / (2.0 / d[0] + 1.0 / d[1] + 0.0), 0.5, 2.0 / 3.0, 0.2]
    judged = eval_cases.oracle_metrics([0, 2, 1], [0, 2, 1, 3], (2,), 1)
    assert judged[0, 0] == (0.0 + 2.0 / d[1]) / (3.0 / d[0] + 2.0 / d[1])
    order = eval_cases.rank_order(np.array([0.5, np.nan, 0.7, 0.5, -np.inf], np.float32))
    assert order.tolist() == [2, 0, 3, 4, 1]                  # ties by position, NaN after -inf
    assert eval_cases.discordant_pairs([3, 2, 1], [1, 2, 3]) == 3 and eval_cases.discordant_pairs([3, 2, 1], [9, 8, 7]) == 0


def test_stored_embeddings_keep_their_score_gaps(golden):
    """What the generator asserted holds for the arrays in the file: adjacent sorted scores of every list differ by
    >= 5e-4 (500 x the 1e-6 by which a BLAS product and the fma chain may differ), and the normalised scores of the
    calibration figure keep 1e-4 clear of every bin edge and of 0.5 - all but the one smallest and the one largest, which
    min-max normalisation maps to exactly 0.0 and to at most 1.0 in either arithmetic."""
    meta, arrays = golden
    q, corpus = arrays["retrieval_queries"].astype(np.float64), arrays["retrieval_corpus"].astype(np.float64)
    eval_cases.assert_separated((q @ corpus.T).reshape(-1), np.arange(0, q.shape[0] * corpus.shape[0] + 1, corpus.shape[0]))
    q, docs, lims = arrays["ranking_queries"].astype(np.float64), arrays["ranking_docs"].astype(np.float64), arrays["ranking_lims"]
    scores = np.einsum("ij,ij->i", docs, np.repeat(q, np.diff(lims), axis=0))
    teacher = np.concatenate([np.asarray(t, np.float64) for t in meta["ranking_teacher"]])
    for flat in (scores, teacher):
        eval_cases.assert_separated(flat, lims)
        assert eval_cases.away_from_edges((flat - flat.min()) / (flat.max() - flat.min() + 1e-8), 10, but_extremes=True)


# ------------------------------------------------------------------------------------------- qrels
def test_qrels_dense_and_dict_forms_give_one_csr():
    dense = [[0, 2, 0, 1], [], [0, 0, 0, 0, 0, 3], [1]]           # short lists: the missing positions are 0
    dicts = [{3: 1, 1: 2}, {}, {5: 3}, {0: 1}]                    # unordered keys are sorted
    a = evaluation.qrels_to_csr(dense, 4)
    b = evaluation.qrels_to_csr(dicts, 4)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tolist() == y.tolist()
    lims, rows, grades = a
    assert lims.tolist() == [0, 2, 2, 3, 4] and rows.tolist() == [1, 3, 5, 0] and grades.tolist() == [2, 1, 3, 1]
    assert (lims.dtype, rows.dtype, grades.dtype) == (np.int64, np.int32, np.int32)
    # global ids: the index's id_offset is subtracted
    assert evaluation.qrels_to_csr([{103: 1, 100: 2}], 1, id_offset=100)[1].tolist() == [0, 3]
    assert evaluation.qrels_to_csr([None, {2: 1}], 2)[0].tolist() == [0, 0, 1]
    # a dict entry with grade 0 is a judgement, a dense 0 is not
    assert evaluation.qrels_to_csr([{4: 0}], 1)[1].tolist() == [4] and evaluation.qrels_to_csr([[0, 0]], 1)[1].tolist() == []


def test_qrels_csr_refuses_unsorted_and_duplicate_rows():
    ok = evaluation.qrels_to_csr(([0, 2, 3], [4, 9, 1], [1, 1, 2]), 2)      # row 1 after row 9: a new query starts there
    assert ok[1].tolist() == [4, 9, 1]
    with pytest.raises(ValueError, match="ascend"):
        evaluation.qrels_to_csr(([0, 3], [4, 9, 1], [1, 1, 2]), 1)          # unsorted within the query
    with pytest.raises(ValueError, match="ascend"):
        evaluation.qrels_to_csr(([0, 2, 3], [4, 4, 1], [1, 1, 2]), 2)       # duplicate
    with pytest.raises(ValueError, match="lims"):
        evaluation.qrels_to_csr(([0, 2, 1, 3], [1, 2, 3], [1, 1, 1]), 3)    # decreasing limits
    with pytest.raises(ValueError):
        evaluation.qrels_to_csr([[1], [1]], 3)                              # two entries for three queries


def test_cutoffs_are_checked_on_the_host():
    assert evaluation._cutoffs([10, 1, 10, 5])[0] == [1, 5, 10]
    for bad in ([], [0], [257], list(range(1, 10))):
        with pytest.raises(ValueError):
            evaluation._cutoffs(bad)
    with pytest.raises(ValueError, match="ideal"):
        evaluation._ideal_code("best")


# ------------------------------------------------------------------------------------------- C-ABI argument checks
def _cut(*ks):
    return (C.c_int32 * len(ks))(*ks), len(ks)


@pytest.mark.parametrize("ks, word", [((0, 5), b"cutoff"), ((5, 257), b"cutoff"), ((5, 5), b"strictly"),
                                      ((10, 5), b"strictly"), (tuple(range(1, 10)), b"n_cut")])
def test_invalid_cutoffs_are_refused_without_a_device(native_lib, ks, word):
    """SSKD_ERR_INVALID comes before any HIP call: it is returned on a machine without a GPU, for nq = 0 too."""
    arr, n = _cut(*ks)
    assert native_lib.sskd_eval_judge(None, 0, 10, 0, None, None, None, 0, None, arr, n, 0, None, None) == 1
    assert word in native_lib.sskd_last_error()
    assert native_lib.sskd_eval_lists(None, None, 64, None, None, 0, None, None, None, arr, n, 0, 0, None, None, None,
                                      None, None) == 1
    assert word in native_lib.sskd_last_error()


def test_no_queries_is_a_successful_no_op_and_other_shapes_are_refused(native_lib):
    arr, n = _cut(1, 10)
    assert native_lib.sskd_eval_judge(None, 0, 10, 0, None, None, None, 0, None, arr, n, 0, None, None) == 0
    assert native_lib.sskd_eval_lists(None, None, 64, None, None, 0, None, None, None, arr, n, 1, 0, None, None, None,
                                      None, None) == 0
    assert native_lib.sskd_eval_judge(None, 0, 0, 0, None, None, None, 0, None, arr, n, 0, None, None) == 1      # k_rank 0
    assert native_lib.sskd_eval_judge(None, 0, 1025, 0, None, None, None, 0, None, arr, n, 0, None, None) == 1   # > K_MAX
    assert native_lib.sskd_eval_judge(None, 0, 10, 0, None, None, None, 0, None, arr, n, 2, None, None) == 1     # ideal_mode
    assert native_lib.sskd_eval_judge(None, -1, 10, 0, None, None, None, 0, None, arr, n, 0, None, None) == 1
    assert native_lib.sskd_eval_judge(None, 3, 10, 0, None, None, None, 0, None, arr, n, 0, None, None) == 1     # null ranking
    # dim and alignment are judged from the pointer VALUES, ahead of the null checks: with every other pointer null these
    # calls could not reach a launch even if the check under test were missing
    lists = lambda q, d, dim: native_lib.sskd_eval_lists(q, d, dim, None, None, 0, None, None, None, arr, n, 0, 1, None,
                                                         None, None, None, None)
    assert lists(1024, 2048, 12) == 1 and b"multiple of 8" in native_lib.sskd_last_error()
    assert lists(1024, 2048, 4096) == 1 and b"multiple of 8" in native_lib.sskd_last_error()
    assert lists(1024 + 4, 2048, 64) == 1 and b"16-byte" in native_lib.sskd_last_error()
    assert lists(1024, 2048 + 8, 64) == 1 and b"16-byte" in native_lib.sskd_last_error()
    assert lists(1024, 2048, 64) == 1 and b"null" in native_lib.sskd_last_error()


# ------------------------------------------------------------------------------------------- the report
def test_generate_report_layout(tmp_path):
    out = tmp_path / "sub" / "report.md"
    evaluation.KDEvaluator(None).generate_report({"ndcg@10": 0.51239, "mrr@10": 0.4}, out, training_config={"epochs": 3})
    text = out.read_text()
    assert text.startswith("# Knowledge Distillation Evaluation Report\n**Generated:** ")
    assert "## Training Configuration\n- **epochs:** 3\n\n## Metrics\n\n- **ndcg@10:** 0.5124\n- **mrr@10:** 0.4000\n" in text


# ------------------------------------------------------------------------------------------- the command-line tool
class _StubStudent:
    """Stands in for StudentModel: records every encode call, returns one-hot-ish rows."""

    calls = []

    def __init__(self, path, device=None):
        self.path = str(path)

    def _rows(self, texts):
        return np.array([[float(len(t)), 1.0] + [0.0] * 6 for t in texts], np.float32)

    def encode_queries(self, queries, **kw):
        _StubStudent.calls.append(("queries", self.path, list(queries)))
        return self._rows(queries)

    def encode_documents(self, docs, **kw):
        _StubStudent.calls.append(("documents", self.path, list(docs)))
        return self._rows(docs)

    def cleanup(self):
        pass


def _host_evaluate_lists(query_emb, doc_embs, doc_lims, grades, k_values, *, scores=None, ref_scores=None, ideal="retrieved"):
    """The oracle in place of the kernel (this test has no GPU)."""
    ks = sorted(set(k_values))
    flat = scores if scores is not None else np.einsum(
        "ij,ij->i", doc_embs, np.repeat(query_emb, np.diff(doc_lims), axis=0))
    block = np.zeros((len(doc_lims) - 1, len(ks), 4))
    for q, (lo, hi) in enumerate(zip(doc_lims[:-1], doc_lims[1:])):
        g = np.asarray(grades[lo:hi])
        block[q] = eval_cases.oracle_metrics(g[eval_cases.rank_order(flat[lo:hi])], g, ks, 0)
    return evaluation.means_of(block, ks)


def test_cli_groups_by_query_and_writes_the_reference_keys(tmp_path, monkeypatch):
    import pyarrow as pa
    import pyarrow.parquet as pq

    from semantic_search_kd_amd import evaluate_cli, student

    # six queries, rows interleaved; query ids out of order in the file
    rows = []
    for j in range(4):
        for qid in (5, 2, 9, 1, 7, 3):
            if j < 2 + qid % 3:
                rows.append((qid, f"query {qid}", f"doc {qid}-{j}" + "x" * ((qid * 7 + j * 3) % 5), int(j == qid % 2)))
    table = pa.table({"query_id": [r[0] for r in rows], "query_text": [r[1] for r in rows], "text": [r[2] for r in rows],
                      "is_relevant": [r[3] for r in rows]})
    data = tmp_path / "eval.parquet"
    pq.write_table(table, data)
    for name in ("vanilla", "kd"):
        (tmp_path / name).mkdir()

    queries, documents, labels = evaluate_cli.load_test_data(data, max_samples=4)
    assert queries == ["query 1", "query 2", "query 3", "query 5"]                 # ascending id, capped
    assert documents[1] == [r[2] for r in rows if r[0] == 2] and labels[1] == [r[3] for r in rows if r[0] == 2]
    assert [len(d) for d in documents] == [3, 4, 2, 4]

    monkeypatch.setattr(student, "StudentModel", _StubStudent)
    monkeypatch.setattr(evaluation, "evaluate_lists", _host_evaluate_lists)
    _StubStudent.calls = []
    out = tmp_path / "out"
    rc = evaluate_cli.main(["--vanilla-model", str(tmp_path / "vanilla"), "--kd-model", str(tmp_path / "kd"),
                            "--data-path", str(data), "--output-dir", str(out), "--k-values", "1,5"])
    assert rc == 0
    result = json.loads((out / "evaluation_results.json").read_text())
    assert sorted(result) == ["improvements_pct", "kd_student", "vanilla"]
    metric_keys = ["mrr@1", "mrr@5", "ndcg@1", "ndcg@5"]
    assert sorted(result["vanilla"]) == sorted(result["kd_student"]) == sorted(result["improvements_pct"]) == metric_keys
    assert result["vanilla"] == result["kd_student"] and all(v == 0 for v in result["improvements_pct"].values())
    assert all(0.0 <= v <= 1.0 for v in result["vanilla"].values())
    # one encode call per side and model, all six queries in ascending id order, their documents flat behind them
    assert [(c[0], c[1].rsplit("/", 1)[-1]) for c in _StubStudent.calls] == [
        ("queries", "vanilla"), ("documents", "vanilla"), ("queries", "kd"), ("documents", "kd")]
    assert _StubStudent.calls[0][2] == [f"query {q}" for q in (1, 2, 3, 5, 7, 9)]
    assert len(_StubStudent.calls[1][2]) == len(rows)
    # a model that is not a local directory is refused before anything loads
    with pytest.raises(SystemExit):
        evaluate_cli.main(["--vanilla-model", "intfloat/e5-small-v2", "--kd-model", str(tmp_path / "kd"),
                           "--data-path", str(data), "--output-dir", str(out)])
