"""Retrieval evaluation on the MI355X: nDCG / MRR / recall / precision per cutoff, Kendall's tau and ECE.

The reference evaluates one query at a time on the host (reference: src/utils/metrics.py, src/kd/eval.py
``KDEvaluator``, scripts/evaluate_production.py): one ``encode`` call, one similarity row, one ``np.argsort`` and Python
lists of labels per query.  Here ALL queries of a call are judged by one kernel launch:

* ``sskd_eval_lists``: every query against its own candidate list (``evaluate_lists`` / ``evaluate_lists_device``);
* ``sskd_eval_judge``: a ranking an index search wrote against qrels (``FAISSIndexBuilder.evaluate``).

Both return the reference's fp64 bits per query (definitions, summation order and tie rules: ``include/sskd_amd.h``
"Retrieval evaluation").  What stays on the host is what is not hot: the mean over the per-query block
(``np.mean`` keeps the reference's bits), Kendall's tau from the device's integer pair counts, and ECE over the score
arrays the kernel wrote.  The metric functions with the reference's names below are the small-input host forms.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native

K_CUT_MAX = 256     # largest cutoff (the discount table's length)
CUT_MAX = 8         # cutoffs per kernel call
LIST_MAX = 1024     # longest candidate list of evaluate_lists
IDEAL_MODES = {"retrieved": 0, "judged": 1}
METRIC_NAMES = ("ndcg", "mrr", "recall", "precision")

# log2(i + 2) for the ranks 0 .. 255, NumPy's bits: the device table is this array
DISCOUNTS = np.log2(np.arange(2, K_CUT_MAX + 2))


# ------------------------------------------------------------------ host metric functions (the reference's names)
def ndcg_at_k(relevance_scores: Sequence[float], k: int = 10) -> float:
    """nDCG@k of grades given in rank order; the ideal ranking is the same first ``k`` grades sorted descending."""
    gains = np.array(relevance_scores[:k])
    if len(gains) == 0:
        return 0.0
    disc = np.log2(np.arange(2, len(gains) + 2))
    dcg = np.sum(gains / disc)
    idcg = np.sum(np.sort(gains)[::-1] / disc)
    if idcg == 0:
        return 0.0
    return dcg / idcg


def mrr_at_k(relevance_scores: Sequence[float], k: int = 10) -> float:
    """1 / (rank of the first grade > 0 among the first ``k``), else 0.0."""
    for i, grade in enumerate(relevance_scores[:k]):
        if grade > 0:
            return 1.0 / (i + 1)
    return 0.0


def _hits(relevant_ids: set, retrieved_ids: Sequence, k: int) -> int:
    return len(set(relevant_ids) & set(retrieved_ids[:k]))


def recall_at_k(relevant_ids: set, retrieved_ids: Sequence, k: int = 100) -> float:
    """Relevant ids among the first ``k`` retrieved / all relevant ids (0.0 when nothing is relevant)."""
    if len(relevant_ids) == 0:
        return 0.0
    return _hits(relevant_ids, retrieved_ids, k) / len(relevant_ids)


def precision_at_k(relevant_ids: set, retrieved_ids: Sequence, k: int = 10) -> float:
    """Relevant ids among the first ``k`` retrieved / ``k`` (``k``, not the number retrieved)."""
    if k == 0:
        return 0.0
    return _hits(relevant_ids, retrieved_ids, k) / k


def tau_from_discordant(n_items, discordant):
    """Kendall's tau of two tie-free rankings of ``n_items`` from the number of discordant pairs: scipy's tau-b
    expression without ties, ``(tot - 2 dis) / sqrt(tot) / sqrt(tot)`` clamped to [-1, 1] in NumPy fp64 (the plain
    quotient differs from it in the last bit about half the time).  Scalars or arrays; 0.0 below two items."""
    n = np.asarray(n_items, dtype=np.int64)
    dis = np.asarray(discordant, dtype=np.int64)
    tot = n * (n - 1) // 2
    safe = np.maximum(tot, 1)
    tau = (tot - 2 * dis) / np.sqrt(safe) / np.sqrt(safe)
    tau = np.minimum(1.0, np.maximum(-1.0, tau))
    return np.where(n < 2, 0.0, tau)


def kendall_tau(ranking1: Sequence, ranking2: Sequence) -> float:
    """Kendall's tau between two rankings (lists of ids), over the ids both hold, each ranked by its position;
    0.0 for fewer than two common ids."""
    place1 = {item: i for i, item in enumerate(ranking1)}
    place2 = {item: i for i, item in enumerate(ranking2)}
    common = [item for item in place1 if item in place2]
    if len(common) < 2:
        return 0.0
    a = np.array([place1[item] for item in common])
    b = np.array([place2[item] for item in common])
    # positions are distinct on both sides: a pair is discordant when the two sides order it differently
    order = np.argsort(a, kind="stable")
    b = b[order]
    discordant = int(np.sum(np.triu(b[:, None] > b[None, :], 1)))
    return float(tau_from_discordant(len(common), discordant))


def expected_calibration_error(confidences: np.ndarray, accuracies: np.ndarray, n_bins: int = 10) -> float:
    """ECE over ``n_bins`` equal bins (lower, upper] of [0, 1]: the sum of |mean confidence - mean accuracy| of a bin
    weighted by the share of samples in it."""
    edges = np.linspace(0, 1, n_bins + 1)
    ece = 0.0
    for lower, upper in zip(edges[:-1], edges[1:]):
        inside = (confidences > lower) & (confidences <= upper)
        share = np.mean(inside)
        if share > 0:
            gap = np.mean(confidences[inside]) - np.mean(accuracies[inside])
            ece += np.abs(gap) * share
    return ece


def compute_retrieval_metrics(query_results: List[Dict], k_values: Sequence[int] = (10, 50, 100)) -> Dict[str, float]:
    """Means of the four metrics over queries given as dicts with ``retrieved_ids``, ``relevant_ids`` and optionally
    ``scores`` (the grades in rank order; default: 1 where the retrieved id is relevant)."""
    per_query = {(name, k): [] for k in k_values for name in METRIC_NAMES}
    for result in query_results:
        retrieved, relevant = result["retrieved_ids"], result["relevant_ids"]
        grades = result.get("scores", [1 if rid in relevant else 0 for rid in retrieved])
        for k in k_values:
            per_query["ndcg", k].append(ndcg_at_k(grades, k))
            per_query["mrr", k].append(mrr_at_k(grades, k))
            per_query["recall", k].append(recall_at_k(relevant, retrieved, k))
            per_query["precision", k].append(precision_at_k(relevant, retrieved, k))
    metrics = {}
    for k in k_values:
        for name in METRIC_NAMES:
            metrics[f"{name}@{k}"] = np.mean(per_query[name, k])
    return metrics


def ranking_ece(scores: np.ndarray, ref_scores: np.ndarray) -> float:
    """The calibration figure of the reference's ``evaluate_ranking_quality``: both flat score arrays min-max
    normalised (+ 1e-8 in the denominator), accuracy = the two agree on which side of 0.5 an entry falls, ECE of the
    normalised scores against it in 10 bins."""
    s, t = np.asarray(scores), np.asarray(ref_scores)
    s_norm = (s - s.min()) / (s.max() - s.min() + 1e-8)
    t_norm = (t - t.min()) / (t.max() - t.min() + 1e-8)
    agree = (s_norm > 0.5).astype(float) == (t_norm > 0.5).astype(float)
    return expected_calibration_error(s_norm, agree.astype(float), n_bins=10)


# ------------------------------------------------------------------------------------------- arguments
def _cutoffs(k_values: Sequence[int]) -> Tuple[List[int], "C.Array"]:
    """The distinct cutoffs ascending, and the host int32 array the C-ABI takes."""
    ks = sorted({int(k) for k in k_values})
    if not ks:
        raise ValueError("k_values is empty")
    if len(ks) > CUT_MAX:
        raise ValueError(f"{len(ks)} distinct cutoffs: at most {CUT_MAX} per call")
    if ks[0] < 1 or ks[-1] > K_CUT_MAX:
        raise ValueError(f"cutoffs {ks} outside [1, {K_CUT_MAX}]")
    return ks, (C.c_int32 * len(ks))(*ks)


def _ideal_code(ideal: str) -> int:
    try:
        return IDEAL_MODES[str(ideal).lower()]
    except KeyError:
        raise ValueError(f"ideal={ideal!r}: expected one of {sorted(IDEAL_MODES)}") from None


_discount_tables: dict = {}


def discount_table(device):
    """The device fp64 [256] table of ``DISCOUNTS`` (made once per device: call an evaluation once before capturing one
    into a graph)."""
    import torch

    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    table = _discount_tables.get(device)
    if table is None:
        table = torch.from_numpy(DISCOUNTS).to(device)
        _discount_tables[device] = table
    return table


def means_of(block: np.ndarray, ks: Sequence[int]) -> Dict[str, float]:
    """``{f"{metric}@{k}": float(np.mean(per-query values))}`` of a ``[nq, n_cut, 4]`` block (0.0 for no queries)."""
    out = {}
    for c, k in enumerate(ks):
        for m, name in enumerate(METRIC_NAMES):
            out[f"{name}@{k}"] = float(np.mean(block[:, c, m])) if block.shape[0] else 0.0
    return out


# ------------------------------------------------------------------------------------------- qrels
def check_qrels_csr(lims, rows, grades) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A qrels CSR as the kernel wants it, or ``ValueError``: ``lims`` int64 non-decreasing from 0 to ``len(rows)``,
    ``rows`` int32 strictly ascending within a query (so a row at most once), ``grades`` int32 beside them."""
    lims = np.ascontiguousarray(np.asarray(lims, dtype=np.int64))
    rows64 = np.asarray(rows, dtype=np.int64)
    grades = np.ascontiguousarray(np.asarray(grades, dtype=np.int32))
    if lims.ndim != 1 or lims.size < 1 or lims[0] != 0 or lims[-1] != rows64.size or (np.diff(lims) < 0).any():
        raise ValueError("qrels: lims must run non-decreasing from 0 to the number of judged rows")
    if rows64.shape != grades.shape or rows64.ndim != 1:
        raise ValueError("qrels: rows and grades must be flat arrays of one length")
    if rows64.size and (rows64.min() < -(2**31) or rows64.max() >= 2**31):
        raise ValueError("qrels: a row lies outside int32")
    if rows64.size > 1:
        rising = np.diff(rows64) > 0
        rising[lims[1:-1][(lims[1:-1] > 0) & (lims[1:-1] < rows64.size)] - 1] = True   # a new query may start anywhere
        if not rising.all():
            raise ValueError("qrels: the rows of a query must ascend strictly (unsorted or duplicate row)")
    return lims, np.ascontiguousarray(rows64.astype(np.int32)), grades


def qrels_to_csr(qrels, nq: int, id_offset: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(lims int64 [nq + 1], rows int32, grades int32)`` from either form of qrels:

    * the reference's dense ``relevance_labels``: per query a list indexed by corpus position, shorter lists meaning 0
      - the non-zero entries become judgements;
    * per query a ``{row: grade}`` dict (or None / empty for a query without judgements), every entry a judgement;
    * a ready ``(lims, rows, grades)`` tuple of arrays, checked (unsorted or duplicate rows are refused).

    Rows are the ids the index returns; ``id_offset`` is subtracted to obtain its rows."""
    if isinstance(qrels, tuple) and len(qrels) == 3:
        lims, rows, grades = check_qrels_csr(*qrels)
        if lims.size != nq + 1:
            raise ValueError(f"qrels: {lims.size - 1} queries in the CSR for {nq} queries")
        return lims, rows, grades
    if len(qrels) != nq:
        raise ValueError(f"qrels: {len(qrels)} entries for {nq} queries")
    lims = np.zeros(nq + 1, np.int64)
    rows, grades = [], []
    for q, entry in enumerate(qrels):
        if entry is None:
            r = g = np.zeros(0, np.int64)
        elif isinstance(entry, dict):
            r = np.fromiter((int(key) for key in entry), np.int64, len(entry))
            g = np.fromiter((int(v) for v in entry.values()), np.int64, len(entry))
            order = np.argsort(r, kind="stable")
            r, g = r[order], g[order]
        else:
            dense = np.asarray(entry, dtype=np.int64).reshape(-1)
            r = np.flatnonzero(dense)
            g = dense[r]
        rows.append(r - int(id_offset))
        grades.append(g)
        lims[q + 1] = lims[q] + r.size
    return check_qrels_csr(lims, np.concatenate(rows) if rows else np.zeros(0, np.int64),
                           np.concatenate(grades) if grades else np.zeros(0, np.int64))


def judge_device(rank_ids, qrels_csr, k_values: Sequence[int], *, id_offset: int = 0, ideal: str = "retrieved"):
    """``sskd_eval_judge`` on a device ranking ``rank_ids`` int64 ``[nq, k_rank]`` (ids as a search wrote them, -1
    padded): the per-query metrics as a device fp64 ``[nq, n_cut, 4]`` tensor = (ndcg, mrr, recall, precision) per
    ascending distinct cutoff.  ``qrels_csr`` = ``(lims, rows, grades)`` device tensors (int64, int32, int32) or None
    when no query has judgements.  Enqueued on the current stream; no synchronisation."""
    import torch

    ks, cut = _cutoffs(k_values)
    mode = _ideal_code(ideal)
    if rank_ids.dim() != 2 or rank_ids.dtype != torch.int64 or not rank_ids.is_cuda:
        raise TypeError("judge_device expects an int64 [nq, k_rank] device tensor")
    rank_ids = rank_ids.contiguous()
    nq, k_rank = rank_ids.shape
    dev = rank_ids.device
    out = torch.empty((nq, len(ks), 4), dtype=torch.float64, device=dev)
    if nq == 0:
        return out
    lims = rows = grades = None
    n_rel = 0
    if qrels_csr is not None:
        lims, rows, grades = qrels_csr
        if lims.dtype != torch.int64 or rows.dtype != torch.int32 or grades.dtype != torch.int32:
            raise TypeError("qrels CSR tensors must be int64 lims, int32 rows, int32 grades")
        if lims.numel() != nq + 1 or rows.numel() != grades.numel():
            raise ValueError("qrels CSR does not match the ranking")
        n_rel = rows.numel()
    with torch.cuda.device(dev):
        _native.check(
            _native.load().sskd_eval_judge(
                rank_ids.data_ptr(), nq, k_rank, int(id_offset), None if lims is None else lims.data_ptr(),
                None if rows is None or n_rel == 0 else rows.data_ptr(),
                None if grades is None or n_rel == 0 else grades.data_ptr(), n_rel, discount_table(dev).data_ptr(),
                cut, len(ks), mode, out.data_ptr(), _native.current_stream_ptr(dev),
            )
        )
    return out


# ------------------------------------------------------------------------------------------- candidate lists
class ListsResult(NamedTuple):
    """What ``evaluate_lists_device`` returns (device tensors)."""

    metrics: "object"       # fp64 [nq, n_cut, 4] = (ndcg, mrr, recall, precision) per ascending distinct cutoff
    scores: "object"        # fp32 [total]: the scores the lists were ranked by
    order: "object"         # int32 [total]: at doc_lims[q] + r the position within list q of the entry ranked r
    discordant: "object"    # int64 [nq] when ref_scores was given, else None
    k_values: tuple         # the cutoffs of the metrics block, ascending


def _device_tensor(x, dtype, device, what: str):
    import torch

    if isinstance(x, torch.Tensor):
        if x.dtype != dtype or x.device != device:
            x = x.to(device=device, dtype=dtype)
        return x.contiguous()
    np_dtype = {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64}[dtype]
    try:
        arr = np.ascontiguousarray(np.asarray(x, dtype=np_dtype))
    except (TypeError, ValueError) as exc:
        raise TypeError(f"{what}: cannot be read as {np_dtype.__name__}") from exc
    return torch.from_numpy(arr).to(device)


def evaluate_lists_device(query_emb, doc_embs, doc_lims, grades, k_values: Sequence[int], *, scores=None,
                          ref_scores=None, ideal: str = "retrieved") -> ListsResult:
    """Every query against its OWN candidate list in one ``sskd_eval_lists`` call on the current stream.

    ``doc_lims`` int64 ``[nq + 1]`` cuts the ``total`` candidates into one list per query (each at most 1024 long);
    ``grades`` int ``[total]`` follow the candidates.  The lists are ranked by ``scores`` fp32 ``[total]`` when given
    (teacher logits, precomputed scores), else by the inner product of ``query_emb`` fp32 ``[nq, dim]`` with
    ``doc_embs`` fp32 ``[total, dim]`` (``dim`` a multiple of 8), bit for bit what ``compute_similarity`` returns
    for the pair.  ``ref_scores`` fp32 ``[total]`` adds, per query, the number of pairs the two score lists order
    differently.  ``ideal``: ``"retrieved"`` (the reference's nDCG) or ``"judged"`` (trec-style: the ideal ranking
    is over all of the list's grades).

    Arguments may be device tensors or host arrays; with device tensors nothing here synchronises (list lengths can then
    not be checked on the host: a list longer than 1024 gets NaN metrics).  Host ``doc_lims`` are checked."""
    import torch

    ks, cut = _cutoffs(k_values)
    mode = _ideal_code(ideal)
    dev = None
    for t in (query_emb, doc_embs, scores, grades, doc_lims, ref_scores):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            dev = t.device
            break
    if dev is None:
        _native.require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(doc_lims, torch.Tensor):
        lims_host = np.asarray(doc_lims, dtype=np.int64).reshape(-1)
        if lims_host.size < 1 or lims_host[0] != 0 or (np.diff(lims_host) < 0).any():
            raise ValueError("doc_lims must run non-decreasing from 0")
        if lims_host.size > 1 and int(np.diff(lims_host).max()) > LIST_MAX:
            raise ValueError(f"a candidate list holds {int(np.diff(lims_host).max())} entries: at most {LIST_MAX}")
    lims = _device_tensor(doc_lims, torch.int64, dev, "doc_lims")
    nq = lims.numel() - 1
    grades = _device_tensor(grades, torch.int32, dev, "grades")
    total = grades.numel()
    if not isinstance(doc_lims, torch.Tensor) and int(lims_host[-1]) != total:
        raise ValueError(f"doc_lims ends at {int(lims_host[-1])}, grades hold {total} entries")
    q = d = s_in = ref = None
    dim = 0
    if scores is not None:
        s_in = _device_tensor(scores, torch.float32, dev, "scores").reshape(-1)
        if s_in.numel() != total:
            raise ValueError(f"{s_in.numel()} scores for {total} candidates")
    else:
        q = _device_tensor(query_emb, torch.float32, dev, "query_emb")
        d = _device_tensor(doc_embs, torch.float32, dev, "doc_embs")
        if q.dim() != 2 or d.dim() != 2 or q.shape[1] != d.shape[1]:
            raise ValueError(f"expected [nq, dim] queries and [total, dim] documents, got {tuple(q.shape)} and {tuple(d.shape)}")
        if q.shape[0] != nq or d.shape[0] != total:
            raise ValueError(f"{q.shape[0]} queries / {d.shape[0]} documents for {nq} lists / {total} grades")
        dim = int(q.shape[1])
    if ref_scores is not None:
        ref = _device_tensor(ref_scores, torch.float32, dev, "ref_scores").reshape(-1)
        if ref.numel() != total:
            raise ValueError(f"{ref.numel()} ref_scores for {total} candidates")
    metrics = torch.empty((nq, len(ks), 4), dtype=torch.float64, device=dev)
    out_scores = torch.empty(total, dtype=torch.float32, device=dev)
    out_order = torch.empty(total, dtype=torch.int32, device=dev)
    discordant = torch.empty(nq, dtype=torch.int64, device=dev) if ref is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        _native.check(
            _native.load().sskd_eval_lists(
                ptr(q), ptr(d), dim, ptr(s_in), lims.data_ptr(), total, grades.data_ptr(), ptr(ref),
                discount_table(dev).data_ptr(), cut, len(ks), mode, nq, metrics.data_ptr(), out_scores.data_ptr(),
                out_order.data_ptr(), ptr(discordant), _native.current_stream_ptr(dev),
            )
        )
    return ListsResult(metrics, out_scores, out_order, discordant, tuple(ks))


def evaluate_lists(query_emb, doc_embs, doc_lims, grades, k_values: Sequence[int], *, scores=None, ref_scores=None,
                   ideal: str = "retrieved") -> Dict[str, float]:
    """``evaluate_lists_device`` averaged on the host: ``{"ndcg@k", "mrr@k", "recall@k", "precision@k"}`` as
    ``float(np.mean(per-query values))``.  With ``ref_scores`` also ``kendall_tau`` (the mean of the per-query taus,
    from the device's integer pair counts) and ``ece`` (``ranking_ece`` of the scores the kernel wrote against
    ``ref_scores`` as given)."""
    import torch

    res = evaluate_lists_device(query_emb, doc_embs, doc_lims, grades, k_values, scores=scores, ref_scores=ref_scores,
                                ideal=ideal)
    out = means_of(res.metrics.cpu().numpy(), res.k_values)
    if ref_scores is not None:
        lims = doc_lims.cpu().numpy() if isinstance(doc_lims, torch.Tensor) else np.asarray(doc_lims, dtype=np.int64)
        taus = tau_from_discordant(np.diff(lims), res.discordant.cpu().numpy())
        out["kendall_tau"] = float(np.mean(taus)) if taus.size else 0.0
        ref_host = ref_scores.cpu().numpy() if isinstance(ref_scores, torch.Tensor) else np.asarray(ref_scores)
        flat = res.scores.cpu().numpy()
        out["ece"] = float(ranking_ece(flat, ref_host.reshape(-1))) if flat.size else 0.0
    return out


# ------------------------------------------------------------------------------------------- KDEvaluator
def _flatten_lists(doc_lists: Sequence[Sequence], relevance_labels: Optional[Sequence[Sequence[int]]]):
    """``(flat documents, doc_lims, flat grades)``: label i of a query belongs to its document i, missing labels are 0."""
    lims = np.zeros(len(doc_lists) + 1, np.int64)
    flat, grades = [], []
    for i, docs in enumerate(doc_lists):
        lims[i + 1] = lims[i] + len(docs)
        flat.extend(docs)
        labels = relevance_labels[i] if relevance_labels is not None else ()
        grades.extend(int(labels[j]) if j < len(labels) else 0 for j in range(len(docs)))
    return flat, lims, np.asarray(grades, dtype=np.int32)


def _ndcg_mrr(metrics: Dict[str, float], k_values: Sequence[int]) -> Dict[str, float]:
    """The keys the reference's evaluator reports, in its order."""
    out = {}
    for k in k_values:
        out[f"ndcg@{k}"] = metrics[f"ndcg@{k}"]
        out[f"mrr@{k}"] = metrics[f"mrr@{k}"]
    return out


class KDEvaluator:
    """The reference's ``KDEvaluator`` (src/kd/eval.py:21-335) with every loop over queries replaced by one encode call
    per side and one evaluation kernel launch.  ``student`` / ``vanilla_student`` are ``StudentModel``-shaped
    (``encode_queries``, ``encode_documents``), ``teacher`` is ``TeacherModel``-shaped (``score(pairs)``)."""

    def __init__(self, student, teacher=None, vanilla_student=None):
        self.student = student
        self.teacher = teacher
        self.vanilla_student = vanilla_student

    def evaluate_retrieval(self, queries: List[str], corpus: List[str], relevance_labels: List[List[int]],
                           k_values: Sequence[int] = (1, 5, 10, 20), batch_size: int = 32) -> Dict[str, float]:
        """``{ndcg@k, mrr@k}`` of the student retrieving over ``corpus``: the corpus is encoded once into a throw-away
        inner-product index, all queries are encoded in one call, and one search plus one ``sskd_eval_judge`` do the
        rest.  ``relevance_labels[q][i]`` is the grade of corpus document i (missing entries are 0)."""
        from .index import FAISSIndexBuilder

        corpus_embs = np.asarray(self.student.encode_documents(list(corpus), batch_size=batch_size), dtype=np.float32)
        query_embs = np.asarray(self.student.encode_queries(list(queries)), dtype=np.float32)
        index = FAISSIndexBuilder(embedding_dim=corpus_embs.shape[1], metric="ip")
        try:
            index.add(corpus_embs)
            metrics = index.evaluate(query_embs, relevance_labels, k_values)
        finally:
            index.cleanup()
        return _ndcg_mrr(metrics, k_values)

    def evaluate_ranking_quality(self, queries: List[str], doc_lists: List[List[str]],
                                 teacher_scores: Optional[List[List[float]]] = None) -> Dict[str, float]:
        """``{kendall_tau, ece}`` of the student's ranking of every query's documents against the teacher's scores
        (given, or computed by ONE ``teacher.score`` call); empty without either."""
        flat, lims, grades = _flatten_lists(doc_lists, None)
        if teacher_scores is not None:
            ref = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1) for s in teacher_scores]) \
                if len(teacher_scores) else np.zeros(0)
        elif self.teacher is not None:
            pairs = [[q, doc] for q, docs in zip(queries, doc_lists) for doc in docs]
            ref = np.asarray(self.teacher.score(pairs), dtype=np.float64).reshape(-1) if pairs else np.zeros(0)
        else:
            return {}
        if ref.size != len(flat):
            raise ValueError(f"{ref.size} teacher scores for {len(flat)} documents")
        q_embs = np.asarray(self.student.encode_queries(list(queries)), dtype=np.float32)
        d_embs = np.asarray(self.student.encode_documents(flat), dtype=np.float32).reshape(len(flat), q_embs.shape[1])
        out = evaluate_lists(q_embs, d_embs, lims, grades, (1,), ref_scores=ref)
        return {"kendall_tau": out["kendall_tau"], "ece": out["ece"]}

    def compare_models(self, queries: List[str], doc_lists: List[List[str]], relevance_labels: List[List[int]],
                       k_values: Sequence[int] = (1, 5, 10, 20)):
        """One row per model (student after KD, vanilla student, teacher - those that were given): a
        ``pandas.DataFrame`` when pandas imports, else the list of row dicts."""
        rows = []
        row = self._evaluate_model(self.student, queries, doc_lists, relevance_labels, k_values)
        row["model"] = "Student (KD)"
        rows.append(row)
        if self.vanilla_student is not None:
            row = self._evaluate_model(self.vanilla_student, queries, doc_lists, relevance_labels, k_values)
            row["model"] = "Student (Vanilla)"
            rows.append(row)
        if self.teacher is not None:
            row = self._evaluate_teacher(queries, doc_lists, relevance_labels, k_values)
            row["model"] = "Teacher"
            rows.append(row)
        try:
            import pandas as pd
        except ImportError:
            return rows
        return pd.DataFrame(rows)

    def _evaluate_model(self, model, queries, doc_lists, relevance_labels, k_values) -> Dict[str, float]:
        flat, lims, grades = _flatten_lists(doc_lists, relevance_labels)
        q_embs = np.asarray(model.encode_queries(list(queries)), dtype=np.float32)
        d_embs = np.asarray(model.encode_documents(flat), dtype=np.float32).reshape(len(flat), q_embs.shape[1])
        return _ndcg_mrr(evaluate_lists(q_embs, d_embs, lims, grades, k_values), k_values)

    def _evaluate_teacher(self, queries, doc_lists, relevance_labels, k_values) -> Dict[str, float]:
        flat, lims, grades = _flatten_lists(doc_lists, relevance_labels)
        pairs = [[q, doc] for q, docs in zip(queries, doc_lists) for doc in docs]
        scores = np.asarray(self.teacher.score(pairs), dtype=np.float32).reshape(-1) if pairs else np.zeros(0, np.float32)
        return _ndcg_mrr(evaluate_lists(None, None, lims, grades, k_values, scores=scores), k_values)

    def generate_report(self, metrics: Dict[str, float], output_path, training_config: Optional[Dict] = None) -> None:
        """The reference's markdown report: title, time stamp, optional training configuration, the metrics to four
        decimals."""
        try:
            import pandas as pd

            now = pd.Timestamp.now()
        except ImportError:
            import datetime

            now = datetime.datetime.now()
        lines = ["# Knowledge Distillation Evaluation Report\n", f"**Generated:** {now}\n\n"]
        if training_config:
            lines.append("## Training Configuration\n")
            lines.extend(f"- **{key}:** {value}\n" for key, value in training_config.items())
            lines.append("\n")
        lines.append("## Metrics\n\n")
        lines.extend(f"- **{key}:** {value:.4f}\n" for key, value in metrics.items())
        output_path = Path(output_path)
        output_path.parent.mkdir(parents=True, exist_ok=True)
        output_path.write_text("".join(lines))
