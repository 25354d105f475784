"""BM25 (stage 1), teacher (stage 2) and ANCE (stage 3) hard-negative mining on the MI355X, and the reference's
three-stage curriculum over them (``build_mining_curriculum``).

``BM25Miner`` is the drop-in for the reference's class of that name (src/mining/miners.py:22-78): same ``mine``
signature and the same host filter, but ONE ``BM25Index.batch_search`` device call for all queries instead of one
host search per query.


``TeacherMiner`` is the drop-in for the reference's class of that name (src/mining/miners.py:80-158): same
constructor, same ``mine`` signature, same selection rule (stable descending sort by teacher score, the first
``top_k``, then the confidence filter) - but ONE ``teacher.score`` call over the pairs of every query instead of
one call of <= 100 pairs per query, so the GPU sees launches cut by a token budget, not by the query loop (and,
after ``TeacherModel.data_parallel()``, pair ranges sharded over the process group).


Drop-in for the reference's ``ANCEMiner`` (reference: src/mining/miners.py:160-253): same constructor,
same ``mine`` signature and the same selection rule -

    adversarial = candidates with  score >= max(positive scores) - margin   (0.0 when no positives)
    hard negatives = the ``top_k`` highest-scoring adversarial candidates, ties in candidate order

- but where the reference encodes one query, its positives and its candidates per loop iteration
(three ``encode`` calls per query), every text is encoded ONCE here, in a few large launches of the
packed varlen encoder, and the scores are ``q @ d.T`` on the GPU.  ``refresh`` + ``mine_from_index``
is the "ANCE refresh" use of the fast path (docs/adr-003: re-encode the corpus with the current
student every N steps, re-search it, mine): corpus -> ``FAISSIndexBuilder`` in HBM -> exact top-k
-> the selection kernel (``sskd_index_mine_select``), one call for all queries.
The student is duck-typed exactly as in the reference (``encode_queries`` / ``encode_documents`` /
``compute_similarity``).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def select_adversarial(cand_ids: Sequence[str], cand_scores: np.ndarray, pos_scores: np.ndarray,
                       margin: float, top_k: int) -> List[str]:
    """The reference's rule (src/mining/miners.py:232-247), including its stable descending sort.  The threshold
    test is decided in fp64, as the reference's expression is under the NumPy it pins (1.x: a float32 scalar against
    a Python float is compared as float64); ``float(s)`` says so whatever NumPy is installed (2.x would round the
    threshold to float32 first and keep a score that equals the rounded value but lies below the threshold)."""
    max_pos = float(pos_scores.max()) if len(pos_scores) > 0 else 0.0
    adversarial = [(d, float(s)) for d, s in zip(cand_ids, cand_scores) if float(s) >= max_pos - margin]
    adversarial.sort(key=lambda x: x[1], reverse=True)
    return [d for d, _ in adversarial[:top_k]]


def select_confident(cand_ids: Sequence[str], scores: Sequence[float], get_confidence, threshold: float, top_k: int):
    """The reference's rule (src/mining/miners.py:140-151): ``sorted(zip(ids, scores), key=score, reverse=True)`` is a
    STABLE descending sort (equal scores keep candidate order), the first ``top_k`` survive, then those whose
    confidence is below the threshold are dropped (so fewer than ``top_k`` may remain)."""
    ranked = sorted(zip(cand_ids, scores), key=lambda x: x[1], reverse=True)
    ids, kept = [], []
    for doc_id, score in ranked[:top_k]:
        if get_confidence(score) >= threshold:
            ids.append(doc_id)
            kept.append(score)
    return ids, kept


class BM25Miner:
    def __init__(self, index_or_path):
        """``index_or_path``: a built / loaded ``BM25Index``, or the directory of a saved one (loaded here, as the
        reference's constructor does)."""
        from .bm25 import BM25Index

        if hasattr(index_or_path, "batch_search"):
            self.index = index_or_path
        else:
            self.index = BM25Index(str(index_or_path))
            self.index.load()

    def mine(self, queries: List[str], positives: List[List[str]], top_k: int = 100,
             exclude_positives: bool = True) -> List[List[str]]:
        """The ``top_k`` BM25 candidates of every query, best first, its positives filtered out afterwards on the host
        as in the reference (src/mining/miners.py:66-73), so a list may be shorter than ``top_k``.  ``positives`` needs
        one list per query (the reference zipped the two lists and silently stopped at the shorter)."""
        if len(positives) != len(queries):
            raise ValueError(f"{len(positives)} positive lists for {len(queries)} queries")
        results = self.index.batch_search(list(queries), top_k=top_k)
        all_negatives: List[List[str]] = []
        for hits, pos_ids in zip(results, positives):
            if exclude_positives:
                pos_set = set(pos_ids)
                all_negatives.append([doc_id for doc_id, _ in hits if doc_id not in pos_set])
            else:
                all_negatives.append([doc_id for doc_id, _ in hits])
        return all_negatives


def _check_denoising(denoising):
    from .denoise import Denoising

    if denoising is not None and not isinstance(denoising, Denoising):
        raise TypeError("denoising must be a Denoising (or None)")
    return denoising


def denoise_candidates(cand_ids: Sequence[str], cand_texts: Sequence[str], scores: Sequence[float], get_confidence,
                       positive_texts: Sequence[str], denoising) -> Tuple[List[str], List[float]]:
    """The denoising rule on one query's scored candidates, on the host: a candidate goes when the teacher's confidence
    in it is ``>= teacher_score_threshold`` or when its text overlap with one of ``positive_texts`` is ``>
    text_overlap_threshold`` (both in fp64, a NaN is kept; a rule whose threshold is None is off).  The survivors keep
    their order."""
    from .denoise import trigram_keys

    t_thr, o_thr = denoising.teacher_score_threshold, denoising.text_overlap_threshold
    pos_sets = [k for k in (trigram_keys(t) for t in positive_texts) if k.size] if o_thr is not None else []
    ids, kept = [], []
    for doc_id, text, score in zip(cand_ids, cand_texts, scores):
        if t_thr is not None and get_confidence(score) >= t_thr:
            continue
        if pos_sets:
            a = trigram_keys(text)
            overlap = 0.0
            for b in pos_sets:
                inter = int(np.intersect1d(a, b, assume_unique=True).size) if a.size else 0
                overlap = max(overlap, inter / (int(a.size) + int(b.size) - inter))
            if overlap > o_thr:
                continue
        ids.append(doc_id)
        kept.append(score)
    return ids, kept


class TeacherMiner:
    def __init__(self, teacher_model, confidence_threshold: float = 0.6, denoising=None):
        """``denoising`` (a ``denoise.Denoising``; None: the reference's miner as it is): drop the false negatives
        among the candidates before the selection (``mine``)."""
        self.teacher = teacher_model
        self.confidence_threshold = confidence_threshold
        self.denoising = _check_denoising(denoising)

    def mine(self, queries: List[str], candidates: List[List[str]], candidate_texts: Dict[str, str], top_k: int = 10,
             positive_texts: Optional[List[List[str]]] = None):
        """``(hard_negative_ids, teacher_scores)``, one list per query (src/mining/miners.py:104-158).  A candidate id
        missing from ``candidate_texts`` is scored against the empty text, as in the reference (:130).

        With ``denoising`` both of its rules act on the candidates BEFORE the stable sort and the ``top_k`` cut, with
        the scores just computed (no second teacher pass): confidence ``>= teacher_score_threshold`` goes, and so does
        a text overlap ``> text_overlap_threshold`` with one of ``positive_texts[q]`` (one list of texts per query;
        None: the overlap rule has nothing to compare with and is off).  The candidate lists are short, so this is
        the host form of the rule (``denoise_candidates``); a ranking over an index is filtered on the device."""
        if positive_texts is not None and len(positive_texts) != len(queries):
            raise ValueError(f"{len(positive_texts)} positive text lists for {len(queries)} queries")
        pairs = [(q, candidate_texts.get(doc_id, "")) for q, cand_ids in zip(queries, candidates) for doc_id in cand_ids]
        scores = list(self.teacher.score(pairs, batch_size=32)) if pairs else []
        all_ids: List[List[str]] = []
        all_scores: List[List[float]] = []
        at = 0
        for qi, (_, cand_ids) in enumerate(zip(queries, candidates)):
            part = scores[at : at + len(cand_ids)]
            at += len(cand_ids)
            if self.denoising is not None:
                cand_ids, part = denoise_candidates(
                    cand_ids, [candidate_texts.get(d, "") for d in cand_ids], part, self.teacher.get_confidence,
                    positive_texts[qi] if positive_texts is not None else (), self.denoising)
            ids, kept = select_confident(cand_ids, part, self.teacher.get_confidence, self.confidence_threshold, top_k)
            all_ids.append(ids)
            all_scores.append(kept)
        return all_ids, all_scores


class ANCEMiner:
    def __init__(self, student_model, margin: float = 0.1, denoising=None):
        """``denoising`` (a ``denoise.Denoising``; None: every method takes today's path): drop the candidates whose
        text overlaps a positive's (on the device) and, where ``mine_from_index`` is given a teacher, those the teacher
        is confident about, before the margin rule."""
        self.student = student_model
        self.margin = margin
        self.denoising = _check_denoising(denoising)
        self._index = None
        self._trigrams = None            # TrigramStore of the refreshed corpus: depends on the texts, not on the student
        self._corpus_texts: List[str] = []
        self._corpus_ids: List[str] = []
        self._rows_of_id: Dict[str, List[int]] = {}

    # ------------------------------------------------------------------ reference API
    def mine(
        self,
        queries: List[str],
        positives: List[List[str]],
        candidates: List[List[str]],
        candidate_texts: Dict[str, str],
        positive_texts: Dict[str, str],
        top_k: int = 5,
    ) -> List[List[str]]:
        if not queries:
            return []
        q_embs = np.asarray(self.student.encode_queries(list(queries)))
        # every distinct (role, doc id) text once; role matters because the two dicts may disagree
        slots: Dict[tuple, int] = {}
        texts: List[str] = []

        def slot(role: str, doc_id: str, table: Dict[str, str]) -> int:
            key = (role, doc_id)
            if key not in slots:
                slots[key] = len(texts)
                texts.append(table.get(doc_id, ""))
            return slots[key]

        pos_idx = [[slot("p", d, positive_texts) for d in ids] for ids in positives]
        cand_idx = [[slot("c", d, candidate_texts) for d in ids] for ids in candidates]
        d_embs = np.asarray(self.student.encode_documents(texts)) if texts else np.zeros((0, q_embs.shape[1]), np.float32)
        dropped = self._overlap_dropped(texts, pos_idx, cand_idx)
        # ONE similarity launch per block of queries (every query x every distinct text; a (query, text) score does
        # not depend on its batch-mates), not two launches + two host round trips per query as in the reference loop
        out: List[List[str]] = []
        block = max(1, (1 << 24) // max(len(texts), 1))
        for q_lo in range(0, len(queries), block):
            sims = (np.asarray(self.student.compute_similarity(q_embs[q_lo : q_lo + block], d_embs))
                    if texts else np.zeros((len(q_embs[q_lo : q_lo + block]), 0), np.float32))
            for qi in range(q_lo, min(q_lo + block, len(queries))):
                row = sims[qi - q_lo]
                pos_scores = row[pos_idx[qi]] if pos_idx[qi] else np.zeros(0, np.float32)
                cand_scores = row[cand_idx[qi]] if cand_idx[qi] else np.zeros(0, np.float32)
                cand_ids = candidates[qi]
                if dropped is not None and cand_idx[qi]:
                    keep = ~dropped[qi, : len(cand_idx[qi])]
                    cand_ids = [d for d, k in zip(cand_ids, keep) if k]
                    cand_scores = cand_scores[keep]
                out.append(select_adversarial(cand_ids, cand_scores, pos_scores, self.margin, top_k))
        return out

    def _overlap_dropped(self, texts: List[str], pos_idx: List[List[int]], cand_idx: List[List[int]]):
        """``mine``'s overlap rule: a throw-away ``TrigramStore`` over the distinct texts and ONE ``sskd_rank_denoise``
        over their slot numbers.  Returns bool ``[nq, widest candidate list]`` (True: the candidate at that position
        overlaps one of the query's positives beyond the threshold), or None when the rule is off."""
        if self.denoising is None or self.denoising.text_overlap_threshold is None or not texts:
            return None
        import torch

        from . import _native
        from .denoise import Denoising, TrigramStore, rank_denoise_device

        width = max((len(c) for c in cand_idx), default=0)
        if width == 0:
            return None
        if width > _native.SSKD_K_MAX:
            raise ValueError(f"{width} candidates for one query: denoising takes at most {_native.SSKD_K_MAX}")
        _native.require_gpu()
        device = torch.device(getattr(self.student, "device", None) or "cuda:0")
        store = TrigramStore.build_from_texts(texts)
        slots = np.full((len(cand_idx), width), -1, np.int64)
        for qi, c in enumerate(cand_idx):
            slots[qi, : len(c)] = c
        lims = np.zeros(len(pos_idx) + 1, np.int64)
        np.cumsum([len(p) for p in pos_idx], out=lims[1:])
        rows = np.fromiter((s for p in pos_idx for s in p), dtype=np.int32, count=int(lims[-1]))
        to = lambda a: torch.from_numpy(a).to(device)
        with torch.cuda.device(device):
            out = rank_denoise_device(to(np.zeros(slots.shape, np.float32)), to(slots), to(lims), to(rows),
                                      Denoising(self.denoising.text_overlap_threshold, None), trigrams=store,
                                      diagnostics=True)
            return (out[5].cpu().numpy() & 1).astype(bool)

    # ------------------------------------------------------------------ ANCE refresh
    def refresh(self, corpus_ids: Sequence[str], corpus_texts: Sequence[str], device: Optional[str] = None):
        """Re-encode the corpus with the CURRENT student and rebuild the exact index in HBM."""
        from .index import FAISSIndexBuilder

        dev = device or getattr(self.student, "device", None)
        encode_device = getattr(self.student, "encode_documents_device", None)
        if encode_device is not None:
            embs = encode_device(list(corpus_texts))      # embeddings stay in HBM: encoder output -> index tiles
        else:
            embs = np.asarray(self.student.encode_documents(list(corpus_texts)))
        index = FAISSIndexBuilder(embedding_dim=int(embs.shape[1]), index_type="Flat", metric="ip", device=dev)
        index.add(embs)
        self._index, self._corpus_ids = index, list(corpus_ids)
        if self.denoising is not None:
            texts = list(corpus_texts)
            # the store follows the texts, not the student: a refresh of the same corpus keeps it (and its copy in HBM)
            if self._trigrams is None or texts != self._corpus_texts:
                from .denoise import TrigramStore

                self._trigrams = TrigramStore.build_from_texts(texts)
            self._corpus_texts = texts
        # doc id -> every row that carries it (an id may repeat: all of its rows are positives of a query naming it)
        self._rows_of_id = {}
        for row, doc_id in enumerate(self._corpus_ids):
            self._rows_of_id.setdefault(doc_id, []).append(row)
        return index

    def _window(self, top_k: int, search_k: int):
        """``(top_k, search_k)`` clipped to the rows the index holds."""
        search_k = min(search_k, max(self._index.ntotal, 1))
        return min(top_k, search_k), search_k

    def mine_from_index(self, queries: List[str], positives: List[List[str]], top_k: int = 5,
                        search_k: int = 100, teacher=None) -> List[List[str]]:
        """Adversarial negatives straight from the refreshed index: the ``search_k`` nearest corpus
        rows of each query are its candidates (its positives excluded), then the same margin rule.

        One search and one selection kernel for all queries (``FAISSIndexBuilder.mine_negatives``): the positives of a
        query are every row carrying one of its ids, so where an id repeats with different texts all of its rows set
        the positive score (``_mine_from_index_host`` scores the last such row only; the exclusion is the same).
        ``positives`` needs one list per query: another length raises ``ValueError`` (the host loop zipped the two
        lists and silently stopped at the shorter).

        With ``denoising`` the overlap rule runs on the device between the search and the selection
        (``sskd_rank_denoise`` against the corpus' ``TrigramStore``).  Given a ``teacher`` (and a
        ``teacher_score_threshold``) the ``(query, candidate text)`` pairs of the whole window are scored in ONE
        ``teacher.score`` call and ``teacher.get_confidence`` of the scores goes in as the kernel's ``aux``.  That is the
        one place that synchronises: the candidate rows come to the host to look their texts up."""
        if self._index is None:
            raise RuntimeError("call refresh(corpus_ids, corpus_texts) first")
        if not queries:
            return []
        q_embs = np.ascontiguousarray(self.student.encode_queries(list(queries)), np.float32)
        pos_rows = [[r for d in pos_ids for r in self._rows_of_id.get(d, ())] for pos_ids in positives]
        top_k, search_k = self._window(top_k, search_k)
        if self.denoising is None:
            _, ids, _, _ = self._index.mine_negatives(q_embs, pos_rows, top_k=top_k, search_k=search_k, margin=self.margin)
        elif teacher is None or self.denoising.teacher_score_threshold is None:
            from .denoise import Denoising

            _, ids, _, _ = self._index.mine_negatives(
                q_embs, pos_rows, top_k=top_k, search_k=search_k, margin=self.margin,
                denoising=Denoising(self.denoising.text_overlap_threshold, None),
                trigrams=self._trigrams if self.denoising.text_overlap_threshold is not None else None)
        else:
            ids = self._mine_from_index_with_teacher(list(queries), q_embs, pos_rows, top_k, search_k, teacher)
        return [[self._corpus_ids[r] for r in row if r >= 0] for row in ids.tolist()]

    def _mine_from_index_with_teacher(self, queries, q_embs, pos_rows, top_k, search_k, teacher) -> np.ndarray:
        """search -> (host: texts of the window, one ``teacher.score``) -> ``sskd_rank_denoise`` with both rules ->
        ``sskd_index_mine_select``; returns the selected rows ``[nq, top_k]``."""
        import torch

        from .index import _host_queries_to_device, normalize_positives

        index = self._index
        lims, rows = normalize_positives(pos_rows, q_embs.shape[0], index.ntotal)
        with torch.cuda.device(index.device):
            q, lims, rows, rank_scores, rank_rows = index._mine_rank(
                _host_queries_to_device(q_embs, index.device), torch.from_numpy(lims).to(index.device),
                torch.from_numpy(rows).to(index.device), top_k, search_k, None, None)
            window = rank_rows.cpu().numpy()                         # the synchronisation
            valid = (window >= 0) & (window < len(self._corpus_texts))
            at_q, at_rank = np.nonzero(valid)                        # row-major: the order aux[valid] is filled in
            pairs = [(queries[qi], self._corpus_texts[window[qi, rank]]) for qi, rank in zip(at_q.tolist(), at_rank.tolist())]
            aux = np.full(window.shape, np.nan, np.float32)
            if pairs:
                aux[valid] = [teacher.get_confidence(s) for s in teacher.score(pairs, batch_size=32)]
            out = index.denoise_ranking_device(
                rank_scores, rank_rows, lims, rows, self.denoising, aux=torch.from_numpy(aux).to(index.device),
                trigrams=self._trigrams if self.denoising.text_overlap_threshold is not None else None)
            _, ids, _, _ = index._mine_select(q, out[0], out[1], lims, rows, top_k, self.margin, False)
            return ids.cpu().numpy() - index.id_offset

    def mine_from_index_device(self, q_embs, pos_lims, pos_rows, top_k: int = 5, search_k: int = 100):
        """The same selection for callers that hold everything in HBM: ``q_embs`` float32 ``[nq, dim]``, positives as
        device ``(pos_lims int64 [nq + 1], pos_rows int32)`` rows of the refreshed index.  Returns device ``(D, I,
        counts, max_pos)`` of ``FAISSIndexBuilder.mine_negatives_device`` (``I`` = rows of ``refresh``'s corpus, -1
        padded); nothing leaves the device and nothing synchronises."""
        if self._index is None:
            raise RuntimeError("call refresh(corpus_ids, corpus_texts) first")
        top_k, search_k = self._window(top_k, search_k)
        return self._index.mine_negatives_device(q_embs, pos_lims, pos_rows, top_k=top_k, search_k=search_k,
                                                 margin=self.margin)

    def _mine_from_index_host(self, queries: List[str], positives: List[List[str]], top_k: int = 5,
                              search_k: int = 100) -> List[List[str]]:
        """``mine_from_index`` as a host loop over the queries (one ``reconstruct`` and one ``compute_similarity``
        round trip each): what the device selection is checked and timed against."""
        if self._index is None:
            raise RuntimeError("call refresh(corpus_ids, corpus_texts) first")
        if not queries:
            return []
        q_embs = np.ascontiguousarray(self.student.encode_queries(list(queries)), np.float32)
        scores, rows = self._index.search(q_embs, min(search_k, max(self._index.ntotal, 1)))
        row_of = {d: i for i, d in enumerate(self._corpus_ids)}
        out: List[List[str]] = []
        for qi, pos_ids in enumerate(positives):
            pos_rows = [row_of[d] for d in pos_ids if d in row_of]
            if pos_rows:
                pos_vecs = self._index.reconstruct(pos_rows)
                pos_scores = self.student.compute_similarity(q_embs[qi : qi + 1], pos_vecs)[0]
            else:
                pos_scores = np.zeros(0, np.float32)
            keep = [(self._corpus_ids[r], s) for r, s in zip(rows[qi], scores[qi]) if r >= 0 and self._corpus_ids[r] not in set(pos_ids)]
            out.append(select_adversarial([d for d, _ in keep], np.array([s for _, s in keep], np.float32),
                                          pos_scores, self.margin, top_k))
        return out


def build_mining_curriculum(queries: List[str], positives: List[List[str]], bm25_index_path, teacher_model,
                            student_model, corpus_texts: Dict[str, str],
                            stage: int = 1, denoising=None) -> Tuple[List[List[str]], List[List[float]]]:
    """``(hard_negatives, teacher_scores)`` of one curriculum stage, the reference's three branches
    (src/mining/miners.py:256-335):

    1. BM25, ``top_k=100``; placeholder scores 0.0.
    2. BM25 ``top_k=100`` -> teacher ``top_k=10`` at confidence 0.6; the teacher's scores.
    3. BM25 ``top_k=100`` -> teacher ``top_k=20`` -> ANCE ``top_k=5`` at margin 0.1; the negatives of a query are
       ``list(set(first five teacher negatives + ANCE negatives))`` and the scores are the first five teacher scores
       followed by one 0.0 per ANCE negative.  As in the reference, the set has no defined order (it varies with the
       interpreter's string hashing) and drops duplicates, so the order of a stage-3 list is unspecified and it does
       not line up with its scores one to one.

    ``bm25_index_path`` is the directory of a saved index (a ``BM25Index`` is accepted too).  ``denoising`` (a
    ``denoise.Denoising``; None: the reference's curriculum as it is) goes to the miners of stages 2 and 3, the
    positives' texts looked up in ``corpus_texts``; stage 1 has no denoising block in the reference."""
    positive_texts = None if denoising is None else [[corpus_texts.get(d, "") for d in pos] for pos in positives]
    if stage == 1:
        negatives = BM25Miner(bm25_index_path).mine(queries, positives, top_k=100)
        return negatives, [[0.0] * len(n) for n in negatives]
    if stage == 2:
        candidates = BM25Miner(bm25_index_path).mine(queries, positives, top_k=100)
        if denoising is not None:
            return TeacherMiner(teacher_model, confidence_threshold=0.6, denoising=denoising).mine(
                queries, candidates, corpus_texts, top_k=10, positive_texts=positive_texts)
        return TeacherMiner(teacher_model, confidence_threshold=0.6).mine(queries, candidates, corpus_texts, top_k=10)
    if stage == 3:
        candidates = BM25Miner(bm25_index_path).mine(queries, positives, top_k=100)
        if denoising is not None:
            teacher_negatives, teacher_scores = TeacherMiner(teacher_model, confidence_threshold=0.6, denoising=denoising).mine(
                queries, candidates, corpus_texts, top_k=20, positive_texts=positive_texts)
        else:
            teacher_negatives, teacher_scores = TeacherMiner(teacher_model, confidence_threshold=0.6).mine(
                queries, candidates, corpus_texts, top_k=20)
        ance = ANCEMiner(student_model, margin=0.1) if denoising is None else ANCEMiner(student_model, margin=0.1,
                                                                                         denoising=denoising)
        ance_negatives = ance.mine(queries, positives, teacher_negatives, corpus_texts, corpus_texts, top_k=5)
        combined_negatives, combined_scores = [], []
        for t_negs, t_scores, a_negs in zip(teacher_negatives, teacher_scores, ance_negatives):
            combined_negatives.append(list(set(t_negs[:5] + a_negs)))
            combined_scores.append(t_scores[:5] + [0.0] * len(a_negs))
        return combined_negatives, combined_scores
    raise ValueError(f"Invalid stage: {stage}. Must be 1, 2, or 3.")
