"""Time of the sharded range-search merge, ``sskd_range_merge_packed``.

    python tools/range_merge_bench.py [--queries 10000] [--per-run 125] [--reps 7] [--out FILE]

Cases: W = 8 runs at about ``--per-run`` matches per run and query (10 M records at the defaults), and W = 2 at the same
total.  The records are synthetic but have the layout and order of real per-shard outputs: every query's matches are
spread over the runs by id range (each run holds one contiguous id range, as a shard does), the match count of a
(run, query) pair varies by +-50 % around its mean, scores are uniform in (0, 1) and every segment is sorted by score
descending, then id.  Each case checks the merge once against a torch sort of all records, then times it with device
events over ``--iters`` back-to-back calls per round; the median of the rounds is reported with min / max.  For
scale, the local call it follows is timed too: ``range_search_device`` over a shard of 1 M / W rows with
``--queries`` queries and a threshold that returns about ``--per-run`` matches per query.  Prints one JSON object.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import FAISSIndexBuilder, _native  # noqa: E402
from semantic_search_kd_amd.dist import range_record_bytes, range_record_views  # noqa: E402


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _records(w, nq, per_run, seed):
    """W packed records of sorted synthetic segments; returns (records, cap, total, (q, score, id) of every record)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    counts = torch.randint(per_run // 2, per_run + per_run // 2 + 1, (w, nq), generator=g, device="cuda")
    span = 1 << 20   # ids of run r: [r * span, (r + 1) * span)
    runs, all_q, all_s, all_i = [], [], [], []
    for r in range(w):
        n = int(counts[r].sum())
        q = torch.repeat_interleave(torch.arange(nq, device="cuda"), counts[r])
        s = torch.rand(n, generator=g, device="cuda")
        i = r * span + torch.randint(0, span, (n,), generator=g, device="cuda")
        order = torch.argsort(i, stable=True)
        order = order[torch.argsort(-s[order], stable=True)]
        order = order[torch.argsort(q[order], stable=True)]
        q, s, i = q[order], s[order], i[order]
        lims = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        lims[1:] = torch.cumsum(counts[r], 0)
        runs.append((lims, s, i))
        all_q.append(q), all_s.append(s), all_i.append(i)
    cap = max(int(l[-1]) for l, _, _ in runs)
    rec = range_record_bytes(nq, cap)
    buf = torch.zeros(w * rec, dtype=torch.uint8, device="cuda")
    for r, (lims, s, i) in enumerate(runs):
        lv, sv, iv = range_record_views(buf[r * rec : (r + 1) * rec], nq, cap)
        lv.copy_(lims)
        sv[: s.numel()].copy_(s)
        iv[: i.numel()].copy_(i)
    total = sum(int(l[-1]) for l, _, _ in runs)
    return buf, cap, total, (torch.cat(all_q), torch.cat(all_s), torch.cat(all_i))


def _merge_case(lib, w, nq, per_run, reps, iters):
    buf, cap, total, (q, s, i) = _records(w, nq, per_run, seed=w)
    lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
    out_s = torch.empty(total, dtype=torch.float32, device="cuda")
    out_i = torch.empty(total, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.sskd_range_merge_workspace_bytes(w, nq, total)), 1), dtype=torch.uint8, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)

    def call():
        _native.check(lib.sskd_range_merge_packed(buf.data_ptr(), w, nq, cap, lims.data_ptr(), out_s.data_ptr(),
                                                  out_i.data_ptr(), total, ws.data_ptr(), ws.numel(), st))

    call()
    order = torch.argsort(i, stable=True)
    order = order[torch.argsort(-s[order], stable=True)]
    order = order[torch.argsort(q[order], stable=True)]
    ok = (int(lims[-1]) == total and torch.equal(out_i, i[order]) and torch.equal(out_s, s[order]))
    if not ok:
        raise SystemExit(f"W={w}: the merge differs from the torch sort of the records")
    for _ in range(3):
        call()
    times = [_time(call, iters) for _ in range(reps)]
    return {"runs": w, "nq": nq, "records": total, "cap": cap, "record_mb": round(buf.numel() / w / 2**20, 2),
            "ms": round(statistics.median(times), 4), "ms_min": round(min(times), 4), "ms_max": round(max(times), 4),
            "checked": ok}


def _unit_rows(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, 384, generator=g, device="cuda")
    return x / x.norm(dim=1, keepdim=True)


def _shard_case(rows, nq, per_query, reps):
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    index.add(_unit_rows(rows, 7))
    q = _unit_rows(nq, 8)
    # scores of random unit rows in 384-d are ~N(0, 1/384): the threshold of about per_query matches per query
    z = torch.distributions.Normal(0.0, 1.0).icdf(torch.tensor(1.0 - per_query / rows)).item()
    thr = torch.full((nq,), z / 384 ** 0.5, dtype=torch.float32, device="cuda")
    lims, _, _ = index.range_search_device(q, thr, normalize_queries=False)
    total = int(lims[-1])
    cap = total + 1024

    def call():
        index.range_search_device(q, thr, normalize_queries=False, max_results=cap)

    for _ in range(3):
        call()
    times = [_time(call, 3) for _ in range(reps)]
    return {"rows": rows, "nq": nq, "results": total, "ms": round(statistics.median(times), 3),
            "ms_min": round(min(times), 3), "ms_max": round(max(times), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--per-run", type=int, default=125)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _native.require_gpu()
    lib = _native.load()
    res = {"merge": [], "local_range": []}
    for w, per_run in ((8, args.per_run), (2, args.per_run * 4)):
        res["merge"].append(_merge_case(lib, w, args.queries, per_run, args.reps, args.iters))
        res["local_range"].append(_shard_case(1_000_000 // w, args.queries, per_run, args.reps))
    for m, l in zip(res["merge"], res["local_range"]):
        m["share_of_local_range"] = round(m["ms"] / l["ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
