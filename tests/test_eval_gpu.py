"""Retrieval evaluation on the MI355X against the host oracle (``eval_cases``) and against what the reference's own
evaluator returned (tests/golden/eval_small.*): the same bits for every query, cutoff and metric.

dim 64 for the candidate lists; the index-backed cases use the index's 384.  Every list of the generated batches has
adjacent scores at least 5e-4 apart (asserted by the generator), so the order does not hang on the last bits of a score.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import eval_cases as ec
from conftest import GOLDEN
from oracle import search as oracle
from semantic_search_kd_amd import FAISSIndexBuilder, KDEvaluator, _native, evaluation

pytestmark = pytest.mark.gpu

KS = ec.CUTOFFS
DIM = 64
PAD = 64            # sentinel entries kept behind every per-candidate output
SENTINEL_F, SENTINEL_I = np.float32(-777.0), np.int32(-777)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _similarity_rows(lib, device, queries, docs, lims):
    """score of every candidate against its own query, by sskd_similarity (the whole [nq, total] matrix, sliced)"""
    nq, total = queries.shape[0], docs.shape[0]
    q, d = _dev(queries, device), _dev(docs, device)
    out = torch.empty((nq, total), dtype=torch.float32, device=device)
    _native.check(lib.sskd_similarity(q.data_ptr(), nq, d.data_ptr(), total, queries.shape[1], out.data_ptr(),
                                      _native.current_stream_ptr(device)))
    sims = out.cpu().numpy()
    return np.concatenate([sims[i, lims[i]:lims[i + 1]] for i in range(nq)]) if total else np.zeros(0, np.float32)


def _call_lists(lib, device, lims, grades, ks, ideal, *, queries=None, docs=None, scores=None, ref=None, nq=None):
    """sskd_eval_lists through the C-ABI with sentinel-filled outputs PAD entries longer than the candidates; returns
    host arrays (metrics, scores, order, discordant)."""
    total = len(grades)
    nq = len(lims) - 1 if nq is None else nq
    cut = (C.c_int32 * len(ks))(*ks)
    t_lims, t_grades = _dev(lims, device), _dev(grades, device)
    t_q = None if queries is None else _dev(queries, device)
    t_d = None if docs is None else _dev(docs, device)
    t_s = None if scores is None else _dev(scores, device)
    t_r = None if ref is None else _dev(ref, device)
    metrics = torch.full((nq, len(ks), 4), -777.0, dtype=torch.float64, device=device)
    out_s = torch.full((total + PAD,), float(SENTINEL_F), dtype=torch.float32, device=device)
    out_o = torch.full((total + PAD,), int(SENTINEL_I), dtype=torch.int32, device=device)
    out_d = torch.full((nq + PAD,), -777, dtype=torch.int64, device=device)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _native.check(lib.sskd_eval_lists(
        ptr(t_q), ptr(t_d), 0 if queries is None else queries.shape[1], ptr(t_s), t_lims.data_ptr(), total,
        t_grades.data_ptr(), ptr(t_r), evaluation.discount_table(device).data_ptr(), cut, len(ks), ideal, nq,
        metrics.data_ptr(), out_s.data_ptr(), out_o.data_ptr(), ptr(out_d) if ref is not None else None,
        _native.current_stream_ptr(device)))
    torch.cuda.synchronize()
    return metrics.cpu().numpy(), out_s.cpu().numpy(), out_o.cpu().numpy(), out_d.cpu().numpy()


def _check_lists(got, lims, grades, scores, ks, ideal, nq, ref=None):
    """Every query of a sskd_eval_lists result against the oracle run on ``scores`` (the bits the kernel ranked by)."""
    metrics, out_s, out_o, out_d = got
    end = int(lims[nq])
    assert out_s[:end].tobytes() == np.asarray(scores[:end], np.float32).tobytes()
    assert (out_s[end:] == SENTINEL_F).all() and (out_o[end:] == SENTINEL_I).all()    # nothing behind the lists
    for q in range(nq):
        lo, hi = int(lims[q]), int(lims[q + 1])
        order = ec.rank_order(scores[lo:hi])
        assert out_o[lo:hi].tolist() == order.tolist(), q
        want = ec.oracle_metrics(grades[lo:hi][order], grades[lo:hi], ks, ideal)
        assert metrics[q].tobytes() == want.tobytes(), (q, hi - lo, metrics[q], want)
        if ref is not None:
            assert out_d[q] == ec.discordant_pairs(scores[lo:hi], ref[lo:hi]), (q, hi - lo)
    assert (out_d[nq:] == -777).all() and (ref is not None or (out_d == -777).all())


BATCHES = {"graded": dict(seed=101, max_grade=3), "binary": dict(seed=102, max_grade=1),
           "barren": dict(seed=103, max_grade=3, positive_share=0.1, barren_every=3)}


@pytest.fixture(scope="module")
def batches(gpu, native_lib):
    """The ragged batches (every boundary length in one doc_lims) with their sskd_similarity scores, made once."""
    out = {}
    for name, kw in BATCHES.items():
        queries, docs, lims, grades, ref = ec.list_batch(ec.LIST_LENGTHS, DIM, **kw)
        out[name] = (queries, docs, lims, grades, ref, _similarity_rows(native_lib, gpu, queries, docs, lims))
    assert (out["barren"][3][out["barren"][2][2]:out["barren"][2][3]] == 0).all()
    return out


# ------------------------------------------------------------------------------------------- sskd_eval_lists
@pytest.mark.parametrize("ideal", [0, 1])
@pytest.mark.parametrize("name", list(BATCHES))
def test_lists_scores_computed(gpu, native_lib, batches, name, ideal):
    queries, docs, lims, grades, _, sims = batches[name]
    nq = len(lims) - 1
    got = _call_lists(native_lib, gpu, lims, grades, KS, ideal, queries=queries, docs=docs)
    _check_lists(got, lims, grades, sims, KS, ideal, nq)


def test_lists_fewer_queries_leave_the_rest_untouched(gpu, native_lib, batches):
    """nq = 9 of the 17 lists: every output entry past the ninth list's end keeps its sentinel."""
    queries, docs, lims, grades, _, sims = batches["graded"]
    got = _call_lists(native_lib, gpu, lims, grades, KS, 0, queries=queries, docs=docs, nq=9)
    _check_lists(got, lims, grades, sims, KS, 0, 9)


def _tie_and_nan_lists():
    """Three lists appended to the ragged batch: exact ties in both score arrays (n = 10 and n = 70), one NaN score."""
    rng = np.random.default_rng(5)
    a = np.array([0.5, 0.25, 0.5, 0.5, -1.0, 0.25, 0.0, -0.0, 0.75, 0.5], np.float32)
    ra = np.array([1.0, 1.0, 2.0, 0.0, 0.0, 2.0, 1.0, 3.0, 3.0, 1.0], np.float32)
    b = rng.integers(0, 6, 70).astype(np.float32) / 8
    rb = rng.integers(0, 4, 70).astype(np.float32)
    c = np.array([0.1, np.nan, 0.9, -np.inf, 0.4, 0.4, np.nan, 0.2, 0.3], np.float32)
    rc = np.array([0.5, 0.7, np.nan, 0.1, 0.2, 0.9, 0.3, 0.3, 0.8], np.float32)
    return [(a, ra), (b, rb), (c, rc)]


@pytest.mark.parametrize("ideal", [0, 1])
def test_lists_given_scores_and_discordant_pairs(gpu, native_lib, batches, ideal):
    """Precomputed scores and a second score list: the discordant counts equal an O(n^2) count on every length; ties go to
    the lower position on both sides, a NaN ranks below every number."""
    _, _, lims, grades, ref, sims = batches["graded"]
    rng = np.random.default_rng(8)
    extra = _tie_and_nan_lists()
    scores = np.concatenate([sims] + [s for s, _ in extra])
    ref = np.concatenate([ref] + [r for _, r in extra])
    lims = np.concatenate([lims, lims[-1] + np.cumsum([len(s) for s, _ in extra])]).astype(np.int64)
    grades = np.concatenate([grades, rng.integers(0, 4, len(scores) - len(grades)).astype(np.int32)])
    nq = len(lims) - 1
    got = _call_lists(native_lib, gpu, lims, grades, KS, ideal, scores=scores, ref=ref)
    _check_lists(got, lims, grades, scores, KS, ideal, nq, ref=ref)
    # the pinned rules, spelled out on the small lists
    lo = int(lims[-4])
    assert got[2][lo:lo + 10].tolist() == [8, 0, 2, 3, 9, 1, 5, 6, 7, 4]          # +0.0 and -0.0 tie: position decides
    lo = int(lims[-2])
    assert got[2][lo:lo + 9].tolist() == [2, 4, 5, 8, 7, 0, 3, 1, 6]              # -inf, then the NaNs by position


def test_evaluate_lists_wrapper_equals_the_oracle_means(gpu, batches):
    queries, docs, lims, grades, ref, sims = batches["graded"]
    got = evaluation.evaluate_lists(queries, docs, lims, grades, (10, 1, 20), ref_scores=ref, ideal="judged")
    nq = len(lims) - 1
    block = np.zeros((nq, 3, 4))
    taus = []
    for q in range(nq):
        lo, hi = int(lims[q]), int(lims[q + 1])
        order = ec.rank_order(sims[lo:hi])
        block[q] = ec.oracle_metrics(grades[lo:hi][order], grades[lo:hi], (1, 10, 20), 1)
        n, dis = hi - lo, ec.discordant_pairs(sims[lo:hi], ref[lo:hi])
        tot = n * (n - 1) // 2
        taus.append(0.0 if n < 2 else min(1.0, max(-1.0, (tot - 2 * dis) / np.sqrt(tot) / np.sqrt(tot))))
    for c, k in enumerate((1, 10, 20)):
        for m, metric in enumerate(("ndcg", "mrr", "recall", "precision")):
            assert got[f"{metric}@{k}"] == float(np.mean(block[:, c, m]))
    assert got["kendall_tau"] == float(np.mean(taus))
    assert got["ece"] == float(evaluation.ranking_ece(sims, ref))
    assert sorted(got) == sorted([f"{m}@{k}" for m in ("ndcg", "mrr", "recall", "precision") for k in (1, 10, 20)]
                                 + ["kendall_tau", "ece"])


# ------------------------------------------------------------------------------------------- sskd_eval_judge
N_ROWS, NQ_JUDGE, ID_OFFSET = 2048, 65, 1000
JUDGED_COUNTS = (0, 1, 64, 65, 300)


@pytest.fixture(scope="module")
def judged_index(gpu):
    """A 2 048-row index with an id offset, 65 queries, and qrels with 0 / 1 / 64 / 65 / 300 judged rows per query: a
    third of them rows the query retrieves near the top, the rest drawn from the whole index (mostly never retrieved);
    grades 0 .. 3, explicit zero judgements included."""
    rows = oracle.seeded_unit_rows(N_ROWS, 384, 2001)
    queries = oracle.seeded_unit_rows(NQ_JUDGE, 384, 2002)
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device=str(gpu), id_offset=ID_OFFSET)
    index.build_from_embeddings(rows)
    _, top = index.search(queries, 256)
    rng = np.random.default_rng(2003)
    qrels = []
    for q in range(NQ_JUDGE):
        count = JUDGED_COUNTS[q % len(JUDGED_COUNTS)]
        near = rng.permutation(top[q])[: count // 3]
        far = rng.permutation(N_ROWS)[:count] + ID_OFFSET
        ids = list(dict.fromkeys(near.tolist() + far.tolist()))[:count]
        qrels.append({int(i): int(g) for i, g in zip(ids, rng.integers(0, 4, len(ids)))})
    assert sorted({len(d) for d in qrels}) == sorted(JUDGED_COUNTS)
    allow = np.zeros(N_ROWS, bool)
    allow[rng.permutation(N_ROWS)[:37]] = True          # 37 allowed rows: rankings of 100 and 256 are padded with -1
    return index, queries, qrels, allow


def _judge_oracle(ids, qrels, ks, ideal):
    block = np.zeros((ids.shape[0], len(ks), 4))
    for q, ranked in enumerate(ids):
        stop = np.flatnonzero(ranked == -1)
        ranked = ranked[: stop[0]] if len(stop) else ranked
        block[q] = ec.oracle_metrics([qrels[q].get(int(i), 0) for i in ranked], list(qrels[q].values()), ks, ideal)
    return block


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k_rank", [1, 10, 100, 256])
def test_judge_equals_the_oracle_on_the_search_ranking(gpu, judged_index, k_rank, masked):
    index, queries, qrels, allow = judged_index
    qd = _dev(queries, gpu)
    csr = index.qrels_device(qrels, NQ_JUDGE)
    _, ids = index.search_device(qd, k_rank, allow=allow if masked else None)
    host_ids = ids.cpu().numpy()
    assert (host_ids[:, : min(k_rank, 37)] >= ID_OFFSET).all()
    assert ((host_ids == -1).any() and (host_ids[:, 37:] == -1).all()) == (masked and k_rank > 37)
    for ideal, name in ((0, "retrieved"), (1, "judged")):
        got = evaluation.judge_device(ids, csr, KS, id_offset=ID_OFFSET, ideal=name).cpu().numpy()
        want = _judge_oracle(host_ids, qrels, KS, ideal)
        assert got.tobytes() == want.tobytes(), (np.argwhere(got != want)[:5], name)
    # no judgements at all: every metric is 0.0
    none = evaluation.judge_device(ids, None, KS, id_offset=ID_OFFSET).cpu().numpy()
    assert none.shape == (NQ_JUDGE, len(KS), 4) and not none.any() and not np.signbit(none).any()


def test_index_evaluate_takes_both_forms_of_qrels(gpu, judged_index):
    index, queries, qrels, allow = judged_index
    positive = [{i: g for i, g in d.items() if g > 0} for d in qrels]          # the dense form cannot say "judged 0"
    dense = []
    for d in positive:
        row = [0] * (max(d) + 1 if d else 0)
        for i, g in d.items():
            row[i] = g
        dense.append(row)
    ks = (10, 50, 100)
    _, ids = index.search(queries, 100)
    for ideal, name in ((0, "retrieved"), (1, "judged")):
        a = index.evaluate(queries, dense, ks, ideal=name)
        b = index.evaluate(queries, positive, ks, ideal=name)
        assert a == b
        want = evaluation.means_of(_judge_oracle(ids, positive, ks, ideal), ks)
        assert a == want
    masked = index.evaluate(queries, positive, ks, allow=allow)
    _, ids = index.search(queries, 100, allow=allow)
    assert masked == evaluation.means_of(_judge_oracle(ids, positive, ks, 0), ks) and masked != a


# ------------------------------------------------------------------------------------------- the reference's goldens
class _FixedEmbeddings:
    """Stands in for StudentModel: the text "q<i>" / "d<i>" is row i of the stored arrays."""

    def __init__(self, queries, docs):
        self.q, self.d = queries, docs
        self.calls = []

    def encode_queries(self, queries, **kw):
        self.calls.append(("queries", len(queries)))
        return self.q[[int(s[1:]) for s in queries]]

    def encode_documents(self, docs, **kw):
        self.calls.append(("documents", len(docs)))
        return self.d[[int(s[1:]) for s in docs]]


class _FixedTeacher:
    def __init__(self, scores):
        self.scores, self.calls = scores, 0

    def score(self, pairs, batch_size=32):
        self.calls += 1
        assert len(pairs) == len(self.scores)
        return list(self.scores)


@pytest.fixture(scope="module")
def golden():
    return json.loads((GOLDEN / "eval_small.json").read_text()), np.load(GOLDEN / "eval_small.npz")


def test_evaluate_retrieval_equals_the_reference(gpu, golden):
    meta, arrays = golden
    model = _FixedEmbeddings(arrays["retrieval_queries"], arrays["retrieval_corpus"])
    nq, n = len(model.q), len(model.d)
    got = KDEvaluator(model).evaluate_retrieval([f"q{i}" for i in range(nq)], [f"d{i}" for i in range(n)],
                                                meta["retrieval_labels"], k_values=meta["k_values"])
    assert got == meta["evaluate_retrieval"]
    assert sorted(model.calls) == [("documents", n), ("queries", nq)]           # one encode call per side


def test_evaluate_model_and_ranking_quality_equal_the_reference(gpu, golden):
    meta, arrays = golden
    model = _FixedEmbeddings(arrays["ranking_queries"], arrays["ranking_docs"])
    lims = arrays["ranking_lims"]
    nq = len(lims) - 1
    queries = [f"q{i}" for i in range(nq)]
    doc_lists = [[f"d{j}" for j in range(lims[i], lims[i + 1])] for i in range(nq)]
    evaluator = KDEvaluator(model)
    got = evaluator._evaluate_model(model, queries, doc_lists, meta["ranking_labels"], meta["k_values"])
    assert got == meta["evaluate_model"]
    table = KDEvaluator(model, vanilla_student=model).compare_models(queries, doc_lists, meta["ranking_labels"], meta["k_values"])
    assert list(table["model"]) == ["Student (KD)", "Student (Vanilla)"]
    assert all(float(table[k][0]) == v and float(table[k][1]) == v for k, v in meta["evaluate_model"].items())
    # Kendall's tau: two fp64 roundings of a value <= 1.  ECE: the scores differ from the reference's BLAS product by
    # <= 1e-6 over a range >= 1 and no bin can flip, so the mean confidences move by <= 3e-6.
    want = meta["ranking_quality"]
    for quality in (evaluator.evaluate_ranking_quality(queries, doc_lists, teacher_scores=meta["ranking_teacher"]),
                    KDEvaluator(model, teacher=_FixedTeacher(np.concatenate(meta["ranking_teacher"])))
                    .evaluate_ranking_quality(queries, doc_lists)):
        assert sorted(quality) == ["ece", "kendall_tau"]
        assert abs(quality["kendall_tau"] - want["kendall_tau"]) <= 1e-12
        assert abs(quality["ece"] - want["ece"]) <= 1e-5
    assert KDEvaluator(model).evaluate_ranking_quality(queries, doc_lists) == {}


# ------------------------------------------------------------------------------------------- contract
def test_invalid_arguments_are_refused_before_any_launch(gpu, native_lib, batches):
    queries, docs, lims, grades, _, _ = batches["graded"]
    nq, total = len(lims) - 1, len(grades)
    t_q, t_d, t_l, t_g = (_dev(a, gpu) for a in (queries, docs, lims, grades))
    disc = evaluation.discount_table(gpu)
    metrics = torch.full((nq, 9, 4), -777.0, dtype=torch.float64, device=gpu)
    ids = torch.zeros((nq, 10), dtype=torch.int64, device=gpu)

    def lists(ks, q=t_q, d=t_d, dim=DIM):
        cut = (C.c_int32 * len(ks))(*ks)
        return native_lib.sskd_eval_lists(q.data_ptr(), d.data_ptr(), dim, None, t_l.data_ptr(), total, t_g.data_ptr(), None,
                                          disc.data_ptr(), cut, len(ks), 0, nq, metrics.data_ptr(), None, None, None,
                                          _native.current_stream_ptr(gpu))

    def judge(ks, k_rank=10):
        cut = (C.c_int32 * len(ks))(*ks)
        return native_lib.sskd_eval_judge(ids.data_ptr(), nq, k_rank, 0, None, None, None, 0, disc.data_ptr(), cut, len(ks),
                                          0, metrics.data_ptr(), _native.current_stream_ptr(gpu))

    for ks in ((0, 5), (5, 257), (5, 5), (10, 5), tuple(range(1, 10))):
        assert lists(ks) == 1 and judge(ks) == 1, ks
    assert lists((1, 5), dim=DIM + 4) == 1                                        # dim % 8 != 0
    off_q = torch.zeros(queries.size + 4, dtype=torch.float32, device=gpu)[1:1 + queries.size]
    off_d = torch.zeros(docs.size + 4, dtype=torch.float32, device=gpu)[1:1 + docs.size]
    assert off_q.data_ptr() % 16 == 4
    assert lists((1, 5), q=off_q) == 1 and lists((1, 5), d=off_d) == 1             # misaligned pointers
    assert judge((1, 5), k_rank=0) == 1 and judge((1, 5), k_rank=1025) == 1
    torch.cuda.synchronize()
    assert (metrics.cpu().numpy() == -777.0).all()                                # nothing ran
    # a list longer than 1024 is found from the host-known sizes
    with pytest.raises(ValueError, match="1024"):
        evaluation.evaluate_lists_device(None, None, [0, 1025], np.zeros(1025, np.int32), (1,), scores=np.zeros(1025, np.float32))
    with pytest.raises(_native.NativeError, match="multiple of 8"):
        evaluation.evaluate_lists_device(np.zeros((1, 12), np.float32), np.zeros((3, 12), np.float32), [0, 3],
                                         np.zeros(3, np.int32), (1,))
    with pytest.raises(ValueError):
        evaluation.evaluate_lists_device(queries, docs, lims, grades, (0, 5))
    # nq = 0 succeeds
    empty = evaluation.evaluate_lists_device(np.zeros((0, DIM), np.float32), np.zeros((0, DIM), np.float32), [0],
                                             np.zeros(0, np.int32), (1, 5))
    assert tuple(empty.metrics.shape) == (0, 2, 4) and empty.discordant is None
    assert judge((1, 5)) == 0


def test_device_side_limits_that_describe_no_list_give_nan_and_write_nothing_else(gpu, native_lib, batches):
    """Limits the host never saw (device tensors): a list longer than 1024 or reaching past the candidates gets NaN
    metrics; its scores and order keep their sentinels, the other queries are evaluated as usual."""
    queries, docs, lims, grades, _, sims = batches["graded"]
    bad = lims.copy()
    bad[-1] = lims[-1] + 5                          # the last list (1024 long) now claims 1029 entries, 5 past the end
    got = _call_lists(native_lib, gpu, bad, grades, KS, 0, queries=queries, docs=docs)
    nq = len(lims) - 1
    assert np.isnan(got[0][nq - 1]).all()
    lo = int(lims[nq - 1])
    assert (got[1][lo:] == SENTINEL_F).all() and (got[2][lo:] == SENTINEL_I).all()
    _check_lists((got[0], np.concatenate([got[1][:lo], np.full(PAD, SENTINEL_F)]),
                  np.concatenate([got[2][:lo], np.full(PAD, SENTINEL_I)]), got[3]), lims, grades, sims, KS, 0, nq - 1)


def test_graph_capture_behind_a_search(gpu, judged_index):
    """search_device then evaluate_lists_device on the search's own scores, captured into one graph: the replay equals the
    eager run.  (The process keeps the default number of hardware queues.)"""
    index, queries, _, _ = judged_index
    k = 10
    q = _dev(queries, gpu)
    rng = np.random.default_rng(12)
    lims = torch.arange(0, (NQ_JUDGE + 1) * k, k, dtype=torch.int64, device=gpu)
    grades = _dev(rng.integers(0, 4, NQ_JUDGE * k).astype(np.int32), gpu)
    ref = _dev(rng.standard_normal(NQ_JUDGE * k).astype(np.float32), gpu)

    def run():
        scores, _ = index.search_device(q, k)
        return evaluation.evaluate_lists_device(None, None, lims, grades, (1, 5, 10), scores=scores.reshape(-1), ref_scores=ref)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = run()                               # sizes the workspace, uploads the discount table
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager[:4], captured[:4]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    host_scores = eager.scores.cpu().numpy()
    block = np.stack([ec.oracle_metrics(grades.cpu().numpy()[i * k:(i + 1) * k][ec.rank_order(host_scores[i * k:(i + 1) * k])],
                                        grades.cpu().numpy()[i * k:(i + 1) * k], (1, 5, 10), 0) for i in range(NQ_JUDGE)])
    assert captured.metrics.cpu().numpy().tobytes() == block.tobytes()
