#!/usr/bin/env python3
"""Regenerates tests/golden/eval_small.json and eval_small.npz: what the REFERENCE'S OWN evaluation code
(src/utils/metrics.py, src/kd/eval.py) returns for the cases of ``tests/eval_cases.py``.

Recorded:
* ``ndcg_at_k`` / ``mrr_at_k`` per graded list, ``recall_at_k`` / ``precision_at_k`` per id case;
* ``kendall_tau`` per ranking pair;
* ``expected_calibration_error`` per (confidences, accuracies) pair, with the arrays;
* ``compute_retrieval_metrics`` over the id cases;
* ``KDEvaluator.evaluate_retrieval``, ``KDEvaluator._evaluate_model`` and ``KDEvaluator.evaluate_ranking_quality`` run with
  a stand-in model that returns fixed embeddings, with those embeddings, labels and teacher scores.

Both files hold data only.  The reference's modules import ``loguru`` (logging) and ``src.models`` (type annotations):
where they are missing, stubs stand in, as in ``make_golden.py``.  ``eval_cases`` asserts while it generates that no
list has adjacent scores closer than 5e-4 and that no ECE confidence lies within 1e-4 of a bin edge or of 0.5.

Usage:  SSKD_REFERENCE=<checkout of the reference project> python tests/golden/make_golden_eval.py
"""
from __future__ import annotations

import json
import os
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))          # tests/

import eval_cases  # noqa: E402


def _reference_modules():
    ref = os.environ.get("SSKD_REFERENCE", "")
    if not (ref and Path(ref, "src", "utils", "metrics.py").is_file()):
        raise SystemExit("set SSKD_REFERENCE to a checkout of the reference project (the directory holding src/)")
    sys.path.insert(0, ref)
    try:
        import loguru  # noqa: F401
    except Exception:
        stub = types.ModuleType("loguru")

        class _Silent:
            def __getattr__(self, name):
                return lambda *a, **k: None

        stub.logger = _Silent()
        sys.modules["loguru"] = stub
    if not Path(ref, "src", "models").is_dir():
        models = types.ModuleType("src.models")
        models.__path__ = []
        student = types.ModuleType("src.models.student")
        student.StudentModel = type("StudentModel", (), {})
        teacher = types.ModuleType("src.models.teacher")
        teacher.TeacherModel = type("TeacherModel", (), {})
        sys.modules.setdefault("src.models", models)
        sys.modules.setdefault("src.models.student", student)
        sys.modules.setdefault("src.models.teacher", teacher)
    from src.kd import eval as ref_eval
    from src.utils import metrics as ref_metrics

    return ref_metrics, ref_eval


class FixedEmbeddingModel:
    """Stand-in for StudentModel: the text "q<i>" / "d<i>" is row i of the given arrays; ``compute_similarity`` is the
    ``q @ d.T`` every call site of the reference assumes."""

    def __init__(self, queries, docs):
        self.q, self.d = queries, docs

    def encode_queries(self, queries, **kw):
        return self.q[[int(s[1:]) for s in queries]]

    def encode_documents(self, docs, **kw):
        return self.d[[int(s[1:]) for s in docs]]

    def compute_similarity(self, q, d):
        return np.matmul(np.asarray(q), np.asarray(d).T)


def _floats(d):
    return {k: float(v) for k, v in d.items()}


def main() -> None:
    metrics, ref_eval = _reference_modules()
    out, arrays = {}, {}

    out["graded"] = [{"ndcg": float(metrics.ndcg_at_k(g, k)), "mrr": float(metrics.mrr_at_k(g, k))}
                     for g, k in eval_cases.graded_lists()]
    out["ids"] = [{"recall": float(metrics.recall_at_k(rel, ret, k)), "precision": float(metrics.precision_at_k(rel, ret, k))}
                  for rel, ret, k in eval_cases.id_cases()]
    out["kendall"] = [float(metrics.kendall_tau(a, b)) for a, b in eval_cases.ranking_pairs()]
    out["ece"] = []
    for i, (conf, acc, bins) in enumerate(eval_cases.ece_arrays()):
        out["ece"].append(float(metrics.expected_calibration_error(conf, acc, n_bins=bins)))
        arrays[f"ece_conf_{i}"], arrays[f"ece_acc_{i}"], arrays[f"ece_bins_{i}"] = conf, acc, np.int64(bins)

    results = [{"retrieved_ids": ret, "relevant_ids": rel, "scores": g}
               for (g, _), (rel, ret, _) in zip(eval_cases.graded_lists(), eval_cases.id_cases()[3:])]
    plain = [{"retrieved_ids": r["retrieved_ids"], "relevant_ids": r["relevant_ids"]} for r in results]
    out["compute_retrieval_metrics"] = {
        "graded_default_k": _floats(metrics.compute_retrieval_metrics(results)),
        "graded_k_1_5_20": _floats(metrics.compute_retrieval_metrics(results, k_values=[1, 5, 20])),
        "binary_default_k": _floats(metrics.compute_retrieval_metrics(plain)),
    }

    q, corpus, labels = eval_cases.retrieval_case()
    model = FixedEmbeddingModel(q, corpus)
    ks = [1, 5, 10, 20]
    out["retrieval_labels"] = labels
    out["evaluate_retrieval"] = _floats(ref_eval.KDEvaluator(model).evaluate_retrieval(
        [f"q{i}" for i in range(len(q))], [f"d{i}" for i in range(len(corpus))], labels, k_values=ks))
    arrays["retrieval_queries"], arrays["retrieval_corpus"] = q, corpus

    q, docs, lims, labels, teacher = eval_cases.ranking_case()
    model = FixedEmbeddingModel(q, docs)
    queries = [f"q{i}" for i in range(len(q))]
    doc_lists = [[f"d{j}" for j in range(lims[i], lims[i + 1])] for i in range(len(q))]
    evaluator = ref_eval.KDEvaluator(model)
    out["ranking_labels"], out["ranking_teacher"], out["k_values"] = labels, teacher, ks
    out["evaluate_model"] = _floats(evaluator._evaluate_model(model, queries, doc_lists, labels, ks))
    out["ranking_quality"] = _floats(evaluator.evaluate_ranking_quality(queries, doc_lists, teacher_scores=teacher))
    arrays["ranking_queries"], arrays["ranking_docs"], arrays["ranking_lims"] = q, docs, lims

    (HERE / "eval_small.json").write_text(json.dumps(out, indent=0) + "\n")
    np.savez_compressed(HERE / "eval_small.npz", **arrays)
    for name in ("eval_small.json", "eval_small.npz"):
        print(f"wrote {name}: {(HERE / name).stat().st_size / 1024:.1f} KiB")
    print({k: out[k] for k in ("evaluate_retrieval", "evaluate_model", "ranking_quality")})


if __name__ == "__main__":
    main()
