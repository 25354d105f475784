"""``evaluate_lists`` against the reference-style per-query evaluation loop on the same box.

    python tools/ab_eval.py [--queries 1000] [--candidates 10,200] [--k 1,5,10] [--out FILE]

Synthetic e5-shaped student (random weights, synthetic WordPiece vocabulary: nothing is downloaded), ``--queries``
queries with ``--candidates`` passages each, one relevant passage per query.

* host loop: what ``KDEvaluator._evaluate_model`` / ``scripts/evaluate_production.py`` of the reference do, run on this
  package's ``StudentModel``: per query one ``encode_queries``, one ``encode_documents``, one ``compute_similarity``,
  ``np.argsort(...)[::-1][:k]``, the labels as Python lists and the host ``ndcg_at_k`` / ``mrr_at_k``; ``np.mean`` last.
* device: ``KDEvaluator._evaluate_model`` of this package - one ``encode_queries`` and one ``encode_documents`` call
  for everything, then ``evaluate_lists`` (one ``sskd_eval_lists`` launch, the mean on the host).  Timed whole (wall
  clock, synchronised) and split: the two encode calls, and ``evaluate_lists`` alone on the embeddings.

Both legs are run once untimed at a tenth of the shape first (kernels loaded, workspaces sized), then timed once at the
full shape.  Prints one JSON object per shape.  ``same_bits_on_same_embeddings`` compares ``evaluate_lists`` with the
host loop run on the SAME embeddings (the evaluation alone); ``same_bits_whole_legs`` compares the two whole legs, which
also differ in how the encoder batched the texts (one list per call against all lists in one call).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import KDEvaluator, StudentModel, evaluation  # noqa: E402
from semantic_search_kd_amd.bench_support import synthetic_passages, synthetic_vocab  # noqa: E402
from semantic_search_kd_amd.encoder import Mi355xSentenceEncoder, build_wordpiece_tokenizer  # noqa: E402
from semantic_search_kd_amd.weights import BertConfig  # noqa: E402


def host_loop(model, queries, doc_lists, labels_list, k_values):
    per_query = {f"{name}@{k}": [] for k in k_values for name in ("ndcg", "mrr")}
    for query, docs, labels in zip(queries, doc_lists, labels_list):
        q = model.encode_queries([query])
        d = model.encode_documents(docs)
        scores = model.compute_similarity(q, d)[0]
        for k in k_values:
            top = np.argsort(scores)[::-1][:k]
            top_labels = [labels[i] if i < len(labels) else 0 for i in top]
            per_query[f"ndcg@{k}"].append(evaluation.ndcg_at_k(top_labels, k=k))
            per_query[f"mrr@{k}"].append(evaluation.mrr_at_k(top_labels, k=k))
    return {key: float(np.mean(v)) for key, v in per_query.items()}


def host_loop_on_embeddings(model, q_emb, d_emb, lims, labels_list, k_values):
    """The same loop on embeddings already made: what is left of it when both legs rank identical vectors."""
    per_query = {f"{name}@{k}": [] for k in k_values for name in ("ndcg", "mrr")}
    for i, labels in enumerate(labels_list):
        scores = model.compute_similarity(q_emb[i:i + 1], d_emb[lims[i]:lims[i + 1]])[0]
        for k in k_values:
            top = np.argsort(scores)[::-1][:k]
            top_labels = [labels[j] if j < len(labels) else 0 for j in top]
            per_query[f"ndcg@{k}"].append(evaluation.ndcg_at_k(top_labels, k=k))
            per_query[f"mrr@{k}"].append(evaluation.mrr_at_k(top_labels, k=k))
    return {key: float(np.mean(v)) for key, v in per_query.items()}


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--candidates", type=str, default="10,200")
    ap.add_argument("--k", type=str, default="1,5,10")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    k_values = [int(k) for k in args.k.split(",")]
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    cfg = BertConfig()
    enc = Mi355xSentenceEncoder.from_synthetic(cfg, device="cuda:0")
    vocab = synthetic_vocab(cfg.vocab_size)
    enc.tokenizer = build_wordpiece_tokenizer(vocab)
    model = StudentModel.from_encoder(enc, "ab-eval")
    evaluator = KDEvaluator(model)
    rng = np.random.default_rng(17)

    for n in (int(c) for c in args.candidates.split(",")):
        nq = args.queries
        passages = synthetic_passages(vocab, nq * n, seed=100 + n)
        queries = [" ".join(p.split()[:8]) for p in synthetic_passages(vocab, nq, seed=200 + n)]
        doc_lists = [passages[i * n:(i + 1) * n] for i in range(nq)]
        labels = [[int(j == r) for j in range(n)] for r in rng.integers(0, n, nq)]
        warm = max(1, nq // 10)
        host_loop(model, queries[:warm], doc_lists[:warm], labels[:warm], k_values)
        evaluator._evaluate_model(model, queries[:warm], doc_lists[:warm], labels[:warm], k_values)

        host, t_host = clock(lambda: host_loop(model, queries, doc_lists, labels, k_values))
        device, t_device = clock(lambda: evaluator._evaluate_model(model, queries, doc_lists, labels, k_values))
        # the device leg in parts
        flat, lims, grades = evaluation._flatten_lists(doc_lists, labels)
        (q_emb, d_emb), t_encode = clock(lambda: (np.asarray(model.encode_queries(queries), np.float32),
                                                  np.asarray(model.encode_documents(flat), np.float32)))
        on_emb, t_lists = clock(lambda: evaluation.evaluate_lists(q_emb, d_emb, lims, grades, k_values))
        host_on_emb, t_host_emb = clock(lambda: host_loop_on_embeddings(model, q_emb, d_emb, lims, labels, k_values))
        same_on_emb = all(on_emb[key] == v for key, v in host_on_emb.items())
        dq, dd = torch.from_numpy(q_emb).cuda(), torch.from_numpy(d_emb).cuda()
        dl, dg = torch.from_numpy(lims).cuda(), torch.from_numpy(grades).cuda()
        evaluation.evaluate_lists_device(dq, dd, dl, dg, k_values)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        evaluation.evaluate_lists_device(dq, dd, dl, dg, k_values)
        b.record()
        b.synchronize()
        emit({
            "device": torch.cuda.get_device_name(0), "queries": nq, "candidates": n, "k_values": k_values,
            "host_loop_s": round(t_host, 3), "device_s": round(t_device, 3), "ratio": round(t_host / t_device, 1),
            "device_encode_s": round(t_encode, 3), "evaluate_lists_s": round(t_lists, 4),
            "eval_lists_kernel_ms": round(a.elapsed_time(b), 3), "host_loop_on_embeddings_s": round(t_host_emb, 3),
            "same_bits_on_same_embeddings": same_on_emb, "same_bits_whole_legs": host == device,
            "max_abs_diff_whole_legs": max(abs(host[key] - device[key]) for key in host),
            "ndcg@10": device.get("ndcg@10"),
        })


if __name__ == "__main__":
    main()
