"""The MMR select against the first stage beside it and against a torch restatement.

    python tools/ab_mmr.py [--docs 100000] [--queries 1,1024,10000] [--fetch-k 50,100,200] [--k 10] [--rounds 7] [--out FILE]

One process; per shape (nq, fetch_k) four legs alternate for ``--rounds`` rounds after one warm-up round, device events
around each leg, medians reported:

* ``first``        ``FAISSIndexBuilder.search_device`` at ``fetch_k`` over ``--docs`` random unit rows (the exact scan);
* ``first_mmr``    ``DiverseIndex.search_device``: the same search plus ONE ``sskd_mmr_select``;
* ``mmr``          the select alone on the ranking the first leg wrote (``mmr_device``);
* ``torch``        a torch restatement of the select on the same ranking: gather the candidates' rows, one ``bmm`` Gram
                   matrix per query, then ``k`` rounds of masked argmax / running maximum (no cut-off, like the legs
                   above).  It is eager PyTorch at its best shape - batched over all queries - not a strawman; its ids
                   are compared with the kernel's (they may differ where fp32 summation order decides a near-tie; the
                   fraction that agrees is reported).

``--profile`` runs only ``first_mmr`` three times per shape: the target of

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ab_mmr.py --profile

whose ``*_kernel_stats.csv`` holds the kernels' own time (``mmr_resident_kernel<50>`` / ``<100>`` for ``fetch_k`` up to
50 / 100, ``mmr_select_kernel`` above: the default shapes stand on both sides).

Prints one JSON object per shape (so a run that is cut short leaves what it measured) and the summary last.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import DiverseIndex, Diversity, FAISSIndexBuilder  # noqa: E402
from semantic_search_kd_amd.diversify import mmr_device  # noqa: E402


def unit_rows(n, gen, dev):
    x = torch.randn((n, 384), generator=gen, device=dev)
    x /= x.norm(dim=1, keepdim=True)
    return x


def torch_mmr(rows, S, I, k, lam):
    """The rule in eager PyTorch (fp32 Gram matrix from ``bmm``, fp64 values): ``(D, I)`` in selection order."""
    nq, f = I.shape
    valid = I >= 0
    cand = rows[I.clamp(min=0)]                                   # [nq, f, 384]
    gram = torch.bmm(cand, cand.transpose(1, 2))                  # [nq, f, f]
    s64 = S.double()
    red = torch.zeros((nq, f), dtype=torch.float32, device=S.device)
    alive = valid.clone()
    at = torch.arange(nq, device=S.device)
    out_s = torch.full((nq, k), torch.finfo(torch.float32).min, device=S.device)
    out_i = torch.full((nq, k), -1, dtype=torch.int64, device=S.device)
    for j in range(k):
        value = lam * s64 - (1.0 - lam) * red.double()
        p = torch.where(alive, value, torch.full_like(value, -float("inf"))).argmax(dim=1)
        ok = alive[at, p]
        out_s[:, j] = torch.where(ok, S[at, p], out_s[:, j])
        out_i[:, j] = torch.where(ok, I[at, p], out_i[:, j])
        alive[at, p] = False
        to_p = gram[at, p]
        red = to_p if j == 0 else torch.maximum(red, to_p)
    return out_s, out_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000)
    ap.add_argument("--queries", default="1,1024,10000")
    ap.add_argument("--fetch-k", default="50,100,200")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lambda-mult", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7)
    flat = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    flat.build_from_embeddings(unit_rows(args.docs, gen, dev))
    rows = flat._tiled[: args.docs * 384].view(args.docs, 384)
    nqs = [int(x) for x in args.queries.split(",")]
    emb = unit_rows(max(nqs), gen, dev)
    k, lam = args.k, args.lambda_mult
    emit({"stage": "setup", "device": torch.cuda.get_device_name(0), "docs": args.docs, "k": k, "lambda": lam,
          "rounds": args.rounds})
    summary = {"stage": "summary", "device": torch.cuda.get_device_name(0)}

    for nq in nqs:
        for fetch_k in (int(x) for x in args.fetch_k.split(",")):
            q = emb[:nq].contiguous()
            d = Diversity(lambda_mult=lam, fetch_k=fetch_k)
            div = DiverseIndex(flat, d)
            if args.profile:
                for _ in range(3):
                    div.search_device(q, k)
                torch.cuda.synchronize()
                continue
            S, I = flat.search_device(q, fetch_k)
            legs = {
                "first": lambda: flat.search_device(q, fetch_k),
                "first_mmr": lambda: div.search_device(q, k),
                "mmr": lambda: mmr_device(flat, S, I, k, d),
                "torch": lambda: torch_mmr(rows, S, I, k, lam),
            }
            times = {name: [] for name in legs}
            for rnd in range(args.rounds + 1):           # round 0 warms every leg up at the timed shape
                for name, fn in legs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    if rnd:
                        times[name].append(a.elapsed_time(b))
            ours = mmr_device(flat, S, I, k, d)[1]
            theirs = torch_mmr(rows, S, I, k, lam)[1]
            row = {"stage": f"nq{nq}_fetch{fetch_k}", "nq": nq, "fetch_k": fetch_k,
                   "ids_equal_torch": round(float((ours == theirs).all(dim=1).float().mean()), 4)}
            for name, t in times.items():
                row[name] = {"median_ms": round(statistics.median(t), 4), "range_ms": [round(min(t), 4), round(max(t), 4)]}
            row["mmr_over_first"] = round(row["mmr"]["median_ms"] / row["first"]["median_ms"], 3)
            row["torch_over_mmr"] = round(row["torch"]["median_ms"] / row["mmr"]["median_ms"], 2)
            row["mmr_us_per_query_selection"] = round(1e3 * row["mmr"]["median_ms"] / (nq * k), 3)
            emit(row)
            summary[row["stage"]] = {key: (row[key]["median_ms"] if isinstance(row[key], dict) else row[key])
                                     for key in ("first", "first_mmr", "mmr", "torch", "mmr_over_first", "torch_over_mmr",
                                                 "ids_equal_torch")}
    if not args.profile:
        emit(summary)


if __name__ == "__main__":
    main()
