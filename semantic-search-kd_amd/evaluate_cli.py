#!/usr/bin/env python3
"""Evaluate a vanilla and a KD-trained student (and optionally the teacher) on per-query candidate lists.

The reference's ``scripts/evaluate_production.py`` / ``scripts/evaluate_and_compare.py`` on the MI355X: the evaluation
parquet (columns ``query_id``, ``query_text``, ``text``, ``is_relevant``) is grouped by ``query_id``, every model ranks
each query's own candidates, and nDCG@k / MRR@k are averaged over the queries.  Where the reference loops over the
queries on the host, each model here costs one encode call per side and one evaluation kernel launch
(``evaluation.KDEvaluator``).  Writes ``<output-dir>/evaluation_results.json`` with the keys ``vanilla``,
``kd_student``, ``teacher`` (when one is given) and ``improvements_pct``.

Models are local directories: nothing is fetched by name.
Run as ``python -m semantic_search_kd_amd.evaluate_cli ...``.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import List, Tuple

from .build_index_cli import _device, _positive
from .evaluation import LIST_MAX, KDEvaluator


def load_test_data(data_path, max_samples: int = 1000) -> Tuple[List[str], List[List[str]], List[List[int]]]:
    """``(queries, documents per query, labels per query)``: rows grouped by ``query_id`` (groups in ascending id
    order, rows in file order, the query text of a group is its first row's), at most ``max_samples`` groups."""
    import pyarrow.parquet as pq

    columns = ["query_id", "query_text", "text", "is_relevant"]
    table = pq.read_table(str(data_path))
    missing = [c for c in columns if c not in table.column_names]
    if missing:
        raise KeyError(f"parquet file {data_path} has no {missing} column(s)")
    cols = {c: table.column(c).to_pylist() for c in columns}
    groups: dict = {}
    for i, qid in enumerate(cols["query_id"]):
        groups.setdefault(qid, []).append(i)
    queries, documents, labels = [], [], []
    for qid in sorted(groups)[:max_samples]:
        rows = groups[qid]
        queries.append(str(cols["query_text"][rows[0]]))
        documents.append([str(cols["text"][i]) for i in rows])
        labels.append([int(cols["is_relevant"][i]) for i in rows])
    return queries, documents, labels


def improvements_pct(vanilla: dict, kd: dict) -> dict:
    """Relative change of every metric in per cent (0 where the vanilla value is not positive)."""
    return {m: ((kd[m] - v) / v) * 100 if v > 0 else 0 for m, v in vanilla.items() if m in kd}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--vanilla-model", type=str, required=True, help="local directory of the untrained student")
    ap.add_argument("--kd-model", type=str, required=True, help="local directory of the KD-trained student")
    ap.add_argument("--teacher-model", type=str, default=None, help="local directory of the teacher (optional)")
    ap.add_argument("--data-path", type=str, required=True,
                    help="parquet file (columns: query_id, query_text, text, is_relevant)")
    ap.add_argument("--output-dir", type=str, required=True)
    ap.add_argument("--max-samples", type=_positive, default=1000, help="queries to evaluate at most")
    ap.add_argument("--k-values", type=str, default="1,5,10", help="comma-separated cutoffs")
    ap.add_argument("--device", type=_device, default="cuda")
    args = ap.parse_args(argv)
    paths = [("--vanilla-model", args.vanilla_model), ("--kd-model", args.kd_model), ("--data-path", args.data_path)]
    if args.teacher_model:
        paths.append(("--teacher-model", args.teacher_model))
    for flag, p in paths:
        if not Path(p).exists():
            ap.error(f"{flag}: {p} does not exist (models are local directories: nothing is fetched by name)")
    try:
        k_values = [int(k) for k in args.k_values.split(",") if k.strip()]
    except ValueError:
        ap.error(f"--k-values: {args.k_values!r} is not a comma-separated list of integers")

    queries, documents, labels = load_test_data(args.data_path, args.max_samples)
    longest = max((len(d) for d in documents), default=0)
    if longest > LIST_MAX:
        ap.error(f"--data-path: a query has {longest} candidates, the evaluation kernel ranks at most {LIST_MAX}")
    print(f"Loaded {len(queries)} queries, {sum(len(d) for d in documents)} candidates")

    from .student import StudentModel

    results = {}
    for key, path in (("vanilla", args.vanilla_model), ("kd_student", args.kd_model)):
        model = StudentModel(path, device=args.device)
        results[key] = KDEvaluator(model)._evaluate_model(model, queries, documents, labels, k_values)
        model.cleanup()
    if args.teacher_model:
        from .teacher import TeacherModel

        teacher = TeacherModel(args.teacher_model, device=args.device)
        results["teacher"] = KDEvaluator(None, teacher=teacher)._evaluate_teacher(queries, documents, labels, k_values)
    results["improvements_pct"] = improvements_pct(results["vanilla"], results["kd_student"])

    out_dir = Path(args.output_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    out_path = out_dir / "evaluation_results.json"
    out_path.write_text(json.dumps(results, indent=2) + "\n")
    for key in ("vanilla", "kd_student", "teacher"):
        if key in results:
            print(key + ": " + ", ".join(f"{m}={v:.4f}" for m, v in results[key].items()))
    print(f"Results saved to {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
