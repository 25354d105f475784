"""BM25 ``batch_search`` on the device against the per-query NumPy idiom of the host library.

    python tools/ab_bm25.py [--docs 1000000] [--queries 1024] [--host-queries 8] [--k 100] [--reps 5] [--out FILE]

Corpus: synthetic Zipf text (``--vocab`` words, p(rank r) ~ 1 / (r + 1), 1 - 30 tokens per document), nothing
downloaded; queries: 6 tokens from the same distribution.

* device: ``BM25Index.batch_search`` (tokenise, upload, the two kernels, download, id lookup) and ``search_device``
  alone (device events around the call: the host side of the call and the two kernels), median of ``--reps``.
* host: what ``rank_bm25.BM25Okapi.get_scores`` + the reference's ``sorted(range(N), key=...)[:k]`` do per query -
  one dense N-vector of term counts per query token, the array expression, a full sort - on ``--host-queries`` of the
  queries, with the dense count vectors filled from the postings (cheaper than the library's per-document dict
  lookups).  This is the idiom the reference runs, not a tuned CPU engine.

The first ``--host-queries`` results are compared (rows and score bits).  Prints one JSON object; with
``--profile`` it only runs the device leg three times (the rocprofv3 target).
"""
import argparse
import json
import statistics
import sys
import time
from itertools import chain
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import BM25Index  # noqa: E402


def zipf_texts(n, vocab, rng, lo, hi):
    p = 1.0 / np.arange(1, vocab + 1)
    cum = np.cumsum(p / p.sum())
    lens = rng.integers(lo, hi + 1, size=n)
    ranks = np.minimum(np.searchsorted(cum, rng.random(int(lens.sum()))), vocab - 1)
    words = np.array([f"w{r}" for r in range(vocab)])[ranks].tolist()
    out, at = [], 0
    for m in lens.tolist():
        out.append(" ".join(words[at : at + m]))
        at += m
    return out


def host_search(post, tokens, k):
    n = post.corpus_size
    score = np.zeros(n)
    for t in tokens:
        tid = post.vocab.get(t)
        q_freq = np.zeros(n, dtype=np.int64)
        idf = 0
        if tid is not None:
            lo, hi = post.term_offsets[tid], post.term_offsets[tid + 1]
            rows = post.post_rows[lo:hi]
            q_freq[rows] = post.freq[lo:hi]       # the term's count per document (main() recounts them)
            idf = post.idf[tid]
        score += idf * (q_freq * (post.k1 + 1) / (q_freq + post.k1 * (1 - post.b + post.b * post.doc_len / post.avgdl)))
    top = sorted(range(n), key=lambda i: score[i], reverse=True)[:k]
    return top, score[top]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--host-queries", type=int, default=8)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(2025)
    t0 = time.perf_counter()
    texts = zipf_texts(args.docs, args.vocab, rng, 1, 30)
    queries = zipf_texts(args.queries, args.vocab, rng, 6, 6)
    t_corpus = time.perf_counter() - t0
    index = BM25Index(device="cuda:0")
    t0 = time.perf_counter()
    index.build_from_texts(list(range(args.docs)), texts)
    t_build = time.perf_counter() - t0
    post = index.bm25
    index.search_device(queries[:4], args.k)      # upload + warm-up
    torch.cuda.synchronize()
    if args.profile:
        for _ in range(3):
            index.search_device(queries, args.k)
        torch.cuda.synchronize()
        return
    batch_s, device_ms = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        results = index.batch_search(queries, top_k=args.k)
        batch_s.append(time.perf_counter() - t0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        index.search_device(queries, args.k)
        b.record()
        b.synchronize()
        device_ms.append(a.elapsed_time(b))
    # posting bytes a query's tokens cover (12 B per posting: int32 row + fp64 w)
    lens = np.diff(post.term_offsets)
    per_query = [12 * int(sum(lens[t] for t in post.term_ids(q.split()))) for q in queries]
    # host leg
    post.freq = None
    if args.host_queries:
        # term counts per posting, as the library's per-document dicts hold them
        terms = np.fromiter(map(post.vocab.__getitem__, chain.from_iterable(index.tokenized_corpus)), dtype=np.int64)
        rows = np.repeat(np.arange(args.docs, dtype=np.int64), post.doc_len)
        _, post.freq = np.unique(terms * args.docs + rows, return_counts=True)
        del terms, rows
    host_s, agree = [], True
    for qi in range(min(args.host_queries, len(queries))):
        t0 = time.perf_counter()
        top, scores = host_search(post, queries[qi].split(), args.k)
        host_s.append(time.perf_counter() - t0)
        got = results[qi]
        agree = agree and [r for r, _ in got] == top and np.array_equal(
            np.array([s for _, s in got]).view(np.int64), np.asarray(scores, dtype=np.float64).view(np.int64))
    out = {
        "docs": args.docs, "vocab_seen": post.n_terms, "postings": int(len(post.post_rows)), "queries": len(queries),
        "k": args.k, "corpus_s": round(t_corpus, 2), "build_s": round(t_build, 2),
        "batch_search_s": round(statistics.median(batch_s), 4),
        "batch_search_qps": round(len(queries) / statistics.median(batch_s), 1),
        "search_device_ms": round(statistics.median(device_ms), 3),
        "search_device_range_ms": [round(min(device_ms), 3), round(max(device_ms), 3)],
        "search_device_qps": round(len(queries) / (statistics.median(device_ms) / 1e3), 1),
        "posting_bytes_per_query_mean": round(float(np.mean(per_query)), 1),
        "posting_bytes_per_query_max": int(max(per_query)),
        "host_idiom_s_per_query": round(statistics.median(host_s), 3) if host_s else None,
        "host_idiom_qps": round(1 / statistics.median(host_s), 3) if host_s else None,
        "host_queries": len(host_s), "host_and_device_agree_bitwise": bool(agree) if host_s else None,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
