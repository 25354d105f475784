"""Timing of the differentiable MaxSim (late_training.maxsim_scores) against the restatement a user would write in
torch - padded einsum + amax + autograd - on the same hidden states, in the same process.

    python tools/ab_late_train.py [--tq 32] [--mean-td 80] [--layers 12] [--reps 5] [--iters 10] [--out FILE]

Two shapes: 32 queries x 8 documents each (``docs_per_query``) and 64 x 64 in-batch.  Per shape:
  * ``maxsim``: forward + backward of the score alone, from bf16 hidden states that are leaves (``[n, S, 384]``, random,
    document lengths drawn around ``--mean-td``, sigma an eighth of it, clipped to [8, S]) to their bf16 gradients;
  * ``kd_step``: the whole step - two ``forward_tokens`` of a synthetic ``--layers``-layer encoder, the scores,
    ``CombinedKDLoss``, backward, AdamW - with the scores computed either way.
Every time is the median of ``--reps`` rounds of ``--iters`` eager calls between two events, after a warm-up call (the
step is host-bound or not as it is: no graph replay is timed here).  Prints one JSON object."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import BertConfig, CombinedKDLoss, TokenLayout, TokenStates, maxsim_scores, synthetic_state_dict  # noqa: E402
from semantic_search_kd_amd.bench_support import synthetic_ids  # noqa: E402
from semantic_search_kd_amd.training import TrainableEncoder  # noqa: E402

DIM = 384


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _median(fn, iters, reps):
    fn()
    torch.cuda.synchronize()
    return round(statistics.median(_events(fn, iters) for _ in range(reps)), 4)


def torch_maxsim(qh, q_len, dh, d_len, docs_per_query):
    """What a user writes without the kernels: normalise, all pairwise token dots, mask the padding, max over document
    tokens, sum over query tokens, mean.  ``q_len`` / ``d_len`` device int tensors."""
    q = torch.nn.functional.normalize(qh, dim=-1)
    d = torch.nn.functional.normalize(dh, dim=-1)
    d_pad = torch.arange(dh.shape[1], device=dh.device)[None, :] >= d_len[:, None]          # [nd, S]
    q_real = (torch.arange(qh.shape[1], device=qh.device)[None, :] < q_len[:, None]).float()  # [nq, Sq]
    if docs_per_query:
        nq = qh.shape[0]
        sim = torch.einsum("qid,qntd->qnit", q, d.view(nq, docs_per_query, dh.shape[1], DIM)).float()
        sim = sim.masked_fill(d_pad.view(nq, docs_per_query, 1, -1), float("-inf"))
    else:
        sim = torch.einsum("qid,ntd->qnit", q, d).float().masked_fill(d_pad[None, :, None, :], float("-inf"))
    best = sim.amax(dim=3) * q_real[:, None, :]
    return best.sum(dim=2) / q_len[:, None].float()


def cell(nq, docs_per_query, nd, args, gen):
    rng = np.random.default_rng(nq)
    Sq, Sd = -(-args.tq // 32) * 32, 96
    q_len = np.full(nq, args.tq, np.int64)
    d_len = np.clip(rng.normal(args.mean_td, args.mean_td / 8, size=nd).round(), 8, Sd).astype(np.int64)
    ql, dl = TokenLayout(q_len, "cuda:0"), TokenLayout(d_len, "cuda:0")
    qh = torch.randn((nq, Sq, DIM), device="cuda", generator=gen).to(torch.bfloat16).requires_grad_(True)
    dh = torch.randn((nd, Sd, DIM), device="cuda", generator=gen).to(torch.bfloat16).requires_grad_(True)
    R = docs_per_query or nd
    probe = torch.randn((nq, R), device="cuda", generator=gen)

    def ours():
        qh.grad = dh.grad = None
        (maxsim_scores(TokenStates(qh, ql), TokenStates(dh, dl), docs_per_query=docs_per_query) * probe).sum().backward()

    def theirs():
        qh.grad = dh.grad = None
        (torch_maxsim(qh, ql.lengths_dev, dh, dl.lengths_dev, docs_per_query) * probe).sum().backward()

    with torch.no_grad():
        a = maxsim_scores(TokenStates(qh, ql), TokenStates(dh, dl), docs_per_query=docs_per_query)
        b = torch_maxsim(qh, ql.lengths_dev, dh, dl.lengths_dev, docs_per_query)
    out = {"nq": nq, "docs_per_query": docs_per_query, "nd": nd, "R": R, "tq": args.tq, "mean_td": float(d_len.mean()),
           "max_abs_score_difference": float((a - b).abs().max()),
           "maxsim_fwd_bwd_ms": {"hip": _median(ours, args.iters, args.reps), "torch": _median(theirs, args.iters, args.reps)}}

    # the whole KD step on a synthetic encoder, the scores computed either way
    cfg = BertConfig(num_hidden_layers=args.layers)
    q_ids, q_mask = synthetic_ids(nq, Sq, cfg.vocab_size, torch.device("cuda:0"), seed=1)
    d_ids, d_mask = synthetic_ids(nd, Sd, cfg.vocab_size, torch.device("cuda:0"), seed=2)
    d_mask = (torch.arange(Sd, device="cuda")[None, :] < dl.lengths_dev[:, None]).int()
    teacher = torch.randn((nq, R), device="cuda", generator=gen) * 3.0
    steps = {}
    for name in ("hip", "torch"):
        model = TrainableEncoder(cfg, synthetic_state_dict(cfg), "cuda:0")
        opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
        loss_fn = CombinedKDLoss()
        loss_fn.component_tensors = True

        def step():
            opt.zero_grad(set_to_none=True)
            hq, hd = model.forward_tokens(q_ids, q_mask), model.forward_tokens(d_ids, d_mask)
            if name == "hip":
                scores = maxsim_scores(TokenStates(hq, ql), TokenStates(hd, dl), docs_per_query=docs_per_query)
            else:
                scores = torch_maxsim(hq, ql.lengths_dev, hd, dl.lengths_dev, docs_per_query)
            loss_fn(scores, teacher)["loss"].backward()
            opt.step()

        steps[name] = _median(step, max(args.iters // 2, 2), args.reps)
        del model, opt
    out["kd_step_ms"] = steps
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tq", type=int, default=32)
    ap.add_argument("--mean-td", type=float, default=80.0)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "layers": args.layers, "reps": args.reps, "iters": args.iters,
              "cells": [cell(32, 8, 256, args, gen), cell(64, None, 64, args, gen)]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
