#!/usr/bin/env python3
"""Build a search index from a parquet corpus with the MI355X encoder.

Same flags as the reference's ``scripts/build_faiss_index.py:15-24`` (``--hnsw-*`` are accepted and
ignored by every index type but ``graph``: the default index is an exact scan, there is no graph to build).
Run as ``python -m semantic_search_kd_amd.build_index_cli ...``.

``--index-type ivf`` trains inverted lists over the rows (``ivf.IVFIndex``: ``--nlist``, ``--nprobe``), checks recall@10
of the IVF search against the exact search as the reference's ``validation:`` block prescribes (configs/index.yaml:51-56)
and exits non-zero below ``--recall-threshold``; single-index builds only.  ``--index-type ivf_pq`` adds product-quantisation
codes over the same lists (``pq.IVFPQIndex``: ``--pq-m``, ``--pq-refine``) behind the same recall gate.
``--index-type graph`` builds a k-NN graph over the rows (``graph.GraphIndex``: ``--hnsw-m`` is its degree, ``--ef-search``
its beam), again behind the recall gate and for single-index builds only.

``--late-interaction`` adds the token store of ``late.LateInteractionIndex`` (``--late-max-doc-tokens``) beside any
single index: the service re-ranks by token-level MaxSim when ``SEMANTIC_KD_FEATURES__ENABLE_LATE_INTERACTION`` is set.
``--late-compress {2,4} --late-centroid-lists`` also writes the compressed store's centroid lists, from which the service
takes its candidates when ``SEMANTIC_KD_LATE__FIRST_STAGE=centroids``.

Row-sharded build (BASELINE cfg 3): launch the same command under
``python -m torch.distributed.run --nproc-per-node G --master-addr 127.0.0.1 -m semantic_search_kd_amd.build_index_cli ...``
and rank r encodes rows ``shard_bounds(N, G, r)`` straight into its own HBM shard and writes
``<output-dir>/shard_<r>/`` (+ ``shards.json`` from rank 0): see ``sharded_index.py``.  ``--shards 1`` forces the
manifest layout from a single process.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
from pathlib import Path

from .index import FAISSIndexBuilder
from .student import StudentModel


def _positive(value: str) -> int:
    v = int(value)
    if v <= 0:
        raise argparse.ArgumentTypeError(f"must be a positive integer, got {value}")
    return v


def _device(value: str) -> str:
    # the reference accepts cpu | cuda | cuda:N (scripts/_validate_args.py:35-39); this backend is GPU-only
    if not re.fullmatch(r"cuda(:\d+)?", value):
        raise argparse.ArgumentTypeError(f"--device must be cuda or cuda:N (MI355X backend, no CPU path), got {value!r}")
    return value


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model-path", type=str, required=True, help="local model directory")
    ap.add_argument("--data-path", type=str, required=True, help="parquet corpus (columns: text, chunk_id)")
    ap.add_argument("--output-dir", type=str, required=True)
    ap.add_argument("--max-docs", type=_positive, default=None)
    ap.add_argument("--batch-size", type=_positive, default=32)
    ap.add_argument("--device", type=_device, default="cuda")
    ap.add_argument("--hnsw-m", type=_positive, default=32, help="graph: the degree (even, 4 .. 64); otherwise accepted for compatibility and unused")
    ap.add_argument("--hnsw-ef-construction", type=_positive, default=200, help="accepted for compatibility; unused")
    ap.add_argument("--shards", type=int, default=0,
                    help="0 = one shard per rank when launched under torch.distributed.run, plain single index otherwise; "
                         "1 = write the sharded layout (shards.json + shard_0/) from this single process")
    ap.add_argument("--group-column", type=str, default=None,
                    help="parquet column holding the group key of every row (for example doc_id): the saved index "
                         "then answers search_grouped with distinct documents; single-index builds only")
    ap.add_argument("--index-type", type=str, choices=("flat", "ivf", "ivf_pq", "graph"), default="flat",
                    help="flat = the exact scan; ivf = inverted lists over the same rows (nprobe search, exact scores); "
                         "ivf_pq = the lists scanned through product-quantisation codes, the best candidates re-scored exactly; "
                         "graph = a k-NN graph over the same rows (beam search, exact scores)")
    ap.add_argument("--nlist", type=_positive, default=None, help="ivf: number of lists (default round(sqrt(rows)))")
    ap.add_argument("--nprobe", type=_positive, default=32, help="ivf: lists a query visits")
    ap.add_argument("--pq-m", type=_positive, default=64, help="ivf_pq: subquantisers per row (8, 16, 24, 32, 48, 64 or 96)")
    ap.add_argument("--pq-refine", type=int, default=None,
                    help="ivf_pq: candidates re-scored exactly per query, at least; a search for more than N results re-scores "
                         "that many (default: min(256, max(100, 4 k)) per search)")
    ap.add_argument("--ef-search", type=_positive, default=64, help="graph: rows a search keeps in its beam (at most 256)")
    ap.add_argument("--recall-threshold", type=float, default=0.97,
                    help="ivf, ivf_pq, graph: fail if recall@10 against the exact search is below this")
    ap.add_argument("--late-interaction", action="store_true",
                    help="also build the late-interaction token store (late.LateInteractionIndex) and save it beside the "
                         "index: 768 B per document token; single-index builds only")
    ap.add_argument("--late-max-doc-tokens", type=_positive, default=180,
                    help="late interaction: tokens kept per document ([CLS] and the closing [SEP] included)")
    ap.add_argument("--late-compress", type=int, choices=(2, 4), default=None,
                    help="late interaction: hold the token store residual-compressed at this many bits per column (104 B "
                         "or 200 B per token instead of 768 B); the codec is trained on a subset of the documents")
    ap.add_argument("--late-centroid-lists", action="store_true",
                    help="late interaction: also write the centroid lists of the compressed store (late_list_lims.npy, "
                         "late_list_rows.npy), so that the store retrieves by itself (LateInteractionIndex.search_tokens)")
    ap.add_argument("--dedup-threshold", type=float, default=None,
                    help="after the build, drop near-duplicate rows: rows scoring above this cosine form clusters "
                         "(single linkage), one row per cluster stays and the index is compacted; single-index builds only")
    ap.add_argument("--dedup-keep", type=str, choices=("first", "densest"), default="first",
                    help="the row a cluster keeps: its first row, or the one with the most near-duplicates")
    ap.add_argument("--dedup-scope", type=str, choices=("all", "across_groups", "within_groups"), default="all",
                    help="the pairs that count: all, or over --group-column only those across / within groups")
    args = ap.parse_args(argv)
    if args.dedup_threshold is None and (args.dedup_keep != "first" or args.dedup_scope != "all"):
        ap.error("--dedup-keep / --dedup-scope need --dedup-threshold")
    if args.late_compress and not args.late_interaction:
        ap.error("--late-compress needs --late-interaction")
    if args.late_centroid_lists and not args.late_compress:
        ap.error("--late-centroid-lists needs --late-interaction --late-compress {2,4}: the lists index a compressed store")
    for flag, p in (("--model-path", args.model_path), ("--data-path", args.data_path)):
        if not Path(p).exists():
            ap.error(f"{flag}: {p} does not exist")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 or args.shards == 1:
        if args.group_column:
            ap.error("--group-column: the row-sharded index has no grouped search yet")
        if args.index_type != "flat":
            what = "graph" if args.index_type == "graph" else "inverted lists"
            ap.error(f"--index-type {args.index_type}: the row-sharded index has no {what} yet")
        if args.late_interaction:
            ap.error("--late-interaction: the row-sharded index has no token store yet")
        if args.dedup_threshold is not None:
            ap.error("--dedup-threshold: clusters span shards; the row-sharded index has no de-duplication yet")
        return _build_sharded(args, world)

    if args.late_interaction and args.late_max_doc_tokens < 2:
        ap.error("--late-max-doc-tokens: at least 2 ([CLS] and [SEP])")
    if args.index_type == "graph":
        from .graph import GRAPH_EF_MAX, check_degree

        try:
            check_degree(args.hnsw_m)
        except ValueError as exc:
            ap.error(f"--hnsw-m: {exc}")
        if args.ef_search > GRAPH_EF_MAX or args.ef_search < 10:
            ap.error(f"--ef-search: a number in [10, {GRAPH_EF_MAX}] (the recall gate searches for 10 results)")

    model = StudentModel(args.model_path, device=args.device)
    builder = FAISSIndexBuilder(embedding_dim=384, index_type="HNSW", metric="cosine", device=args.device)
    index = builder.build_from_parquet(
        model=model,
        parquet_path=Path(args.data_path),
        batch_size=args.batch_size,
        max_docs=args.max_docs,
        hnsw_m=args.hnsw_m,
        hnsw_ef_construction=args.hnsw_ef_construction,
        group_column=args.group_column,
    )
    if args.dedup_threshold is not None:
        # before anything is trained over the rows or saved: every later step sees the surviving rows only
        before = index.ntotal
        clusters = builder.deduplicate(args.dedup_threshold, keep=args.dedup_keep, scope=args.dedup_scope, compact=True)
        print(f"De-duplication at {args.dedup_threshold}: {before} rows, {clusters.n_clusters} clusters, "
              f"{clusters.removed.size} rows dropped")
    if args.index_type == "ivf":
        from .ivf import IVFIndex

        ivf = IVFIndex(flat=builder, nlist=args.nlist, nprobe=args.nprobe)
        ivf.train()
        ivf.save(Path(args.output_dir))
        recall = ivf.validate(num_queries=1000, k=10)
        print(f"IVF lists: {ivf.nlist}, nprobe: {min(ivf.nprobe, ivf.nlist)}, recall@10 vs exact: {recall:.4f}")
        if recall < args.recall_threshold:
            print(f"recall@10 {recall:.4f} is below the threshold {args.recall_threshold}", file=sys.stderr)
            return 1
    elif args.index_type == "ivf_pq":
        from .pq import PQ_CODES, PQ_M_ALLOWED, IVFPQIndex

        if args.pq_m not in PQ_M_ALLOWED:
            ap.error(f"--pq-m: must be one of {PQ_M_ALLOWED}")
        if args.pq_refine is not None and not 1 <= args.pq_refine <= 256:
            # 0 (raw ADC scores as the result) is left to callers of IVFPQIndex.search: a built index is served, and
            # the service's scores are exact inner products
            ap.error("--pq-refine: a number in [1, 256]")
        if index.ntotal < PQ_CODES:
            ap.error(f"--index-type ivf_pq: product quantisation trains on at least {PQ_CODES} rows, the corpus has {index.ntotal}")
        ivf = IVFPQIndex(flat=builder, nlist=args.nlist, nprobe=args.nprobe, m=args.pq_m, refine=args.pq_refine)
        ivf.train()
        ivf.save(Path(args.output_dir))
        recall = ivf.validate(num_queries=1000, k=10)
        refine = "default" if ivf.refine is None else ivf.refine
        print(f"IVF-PQ lists: {ivf.nlist}, nprobe: {min(ivf.nprobe, ivf.nlist)}, m: {ivf.m}, refine: {refine}, "
              f"recall@10 vs exact: {recall:.4f}")
        if recall < args.recall_threshold:
            print(f"recall@10 {recall:.4f} is below the threshold {args.recall_threshold}", file=sys.stderr)
            return 1
    elif args.index_type == "graph":
        from .graph import GraphIndex

        graph = GraphIndex(flat=builder, M=args.hnsw_m, ef=args.ef_search)
        graph.build_graph()
        graph.save(Path(args.output_dir))
        recall = graph.validate(num_queries=1000, k=10)
        print(f"Graph degree: {graph.M}, k-NN lists: {graph.knn_k}, entry rows: {graph.n_entry}, ef: {graph.ef}, "
              f"width: {graph.width}, recall@10 vs exact: {recall:.4f}")
        if recall < args.recall_threshold:
            print(f"recall@10 {recall:.4f} is below the threshold {args.recall_threshold}", file=sys.stderr)
            return 1
    else:
        builder.save(Path(args.output_dir))
    if args.late_interaction:
        from .late import LateInteractionIndex, store_bytes

        late = LateInteractionIndex(builder, max_doc_tokens=args.late_max_doc_tokens)
        late.build_from_texts(model, [builder.doc_texts[i] for i in builder.doc_ids], batch_size=args.batch_size,
                              compress=args.late_compress)
        if args.late_centroid_lists:
            late.build_centroid_lists()
        late.save(Path(args.output_dir))
        if args.late_centroid_lists:
            print(f"Late-interaction centroid lists: {int(late.list_rows.numel())} (centroid, row) pairs over "
                  f"{late.n_centroids} lists, {late.centroid_list_bytes} bytes")
        if args.late_compress:
            print(f"Late-interaction token store: {late.n_tokens} tokens, {late.nbytes} bytes compressed to "
                  f"{late.nbits} bits over {late.n_centroids} centroids ({store_bytes(late.n_tokens)} bytes as bf16; "
                  f"{late.n_tokens / max(late.ntotal, 1):.1f} tokens per row, at most {late.max_doc_tokens})")
        else:
            print(f"Late-interaction token store: {late.n_tokens} tokens, {late.nbytes} bytes "
                  f"({late.n_tokens / max(late.ntotal, 1):.1f} tokens per row, at most {late.max_doc_tokens})")
    print(f"Index saved to: {args.output_dir}")
    print(f"Total vectors: {index.ntotal}")
    return 0


def _build_sharded(args, world: int) -> int:
    """One process per GPU (``torch.distributed.run`` sets RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*)."""
    import torch
    import torch.distributed as dist

    from .sharded_index import build_sharded

    device = args.device
    started = False
    if world > 1:
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        one_gpu_each = torch.cuda.device_count() >= world
        device = f"cuda:{local_rank}" if one_gpu_each else args.device   # rehearsal: ranks share a device over gloo
        torch.cuda.set_device(torch.device(device if ":" in device else "cuda:0"))
        if not dist.is_initialized():
            if one_gpu_each:
                dist.init_process_group("nccl", device_id=torch.device(device))   # RCCL over xGMI
            else:
                dist.init_process_group("gloo")
            started = True
    try:
        model = StudentModel(args.model_path, device=device)
        manifest = build_sharded(model, Path(args.data_path), Path(args.output_dir), batch_size=args.batch_size,
                                 max_docs=args.max_docs, device=device)
        if not dist.is_initialized() or dist.get_rank() == 0:
            print(f"Index saved to: {args.output_dir}")
            print(f"Total vectors: {manifest['n_total']} in {len(manifest['shards'])} shard(s)")
    finally:
        if started:
            dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
