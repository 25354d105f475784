"""Denoising of mined negatives on the MI355X: ``sskd_overlap_pairs`` and ``sskd_rank_denoise`` through the C-ABI, then
``FAISSIndexBuilder.mine_negatives(..., denoising, trigrams)`` and ``ANCEMiner`` on top (``include/sskd_amd.h``).

The oracle is ``denoise_cases.py``: Python sets and loops, ``int / int``.  Every comparison is exact: ids, counts and
reasons as integers, scores, overlaps and Jaccard values by their bits.  Shapes are the smallest at which the kernels can
go wrong: a wave strides 64 keys, a positive is staged in LDS up to 4 096 keys and searched in HBM beyond, a workgroup
decides 256 ranks per round, and ``search_k`` reaches ``SSKD_K_MAX``.
"""
import numpy as np
import pytest
import torch

import denoise_cases as dc
import mine_cases as mc
import ranking_walk_cases as rw
from capi_helpers import stream
from semantic_search_kd_amd import _native

SENT_F, SENT_I, SENT_C, SENT_B = 12345.0, -77, -55, 0xEE

_device_stores = {}


def _device_store(name, sets):
    if name not in _device_stores:
        lims, keys = dc.csr_of(list(sets))
        keys = keys if keys.size else np.zeros(1, np.uint64)
        _device_stores[name] = (torch.from_numpy(lims).cuda(), torch.from_numpy(keys.view(np.int64)).cuda(), len(sets))
    return _device_stores[name]


def _guarded(nq, k, dtype, fill):
    """[nq + 2, k] filled with a sentinel; the call writes rows 1 .. nq, rows 0 and nq + 1 must come back untouched"""
    return torch.full((nq + 2, k), fill, dtype=dtype, device="cuda")


def _rank_denoise(lib, store, scores, ids, lims, rows, aux=None, aux_thr=0.0, ov_thr=0.0, optional=True):
    """the entry point on guarded buffers; ``store`` None = overlap rule off, ``aux`` None = teacher rule off,
    ``optional`` False = the three optional outputs as NULL"""
    nq, k = ids.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ds, di, dl = d(scores), d(ids), d(lims)
    dr = d(rows) if len(rows) else None
    da = d(aux) if aux is not None else None
    out_s, out_i = _guarded(nq, k, torch.float32, SENT_F), _guarded(nq, k, torch.int64, SENT_I)
    out_a = _guarded(nq, k, torch.float32, SENT_F) if optional else None
    out_o = _guarded(nq, k, torch.float64, SENT_F) if optional else None
    out_r = _guarded(nq, k, torch.uint8, SENT_B) if optional else None
    cnt = torch.full((nq + 2,), SENT_C, dtype=torch.int32, device="cuda")
    at = lambda t, width=k: None if t is None else t.data_ptr() + width * t.element_size()
    g_lims, g_keys, n_sets = store if store is not None else (None, None, 0)
    _native.check(lib.sskd_rank_denoise(
        None if g_lims is None else g_lims.data_ptr(), None if g_keys is None else g_keys.data_ptr(), n_sets,
        ds.data_ptr(), di.data_ptr(), nq, k, dl.data_ptr(), None if dr is None else dr.data_ptr(),
        None if da is None else da.data_ptr(), aux_thr, ov_thr, at(out_s), at(out_i), at(out_a), at(cnt, 1), at(out_o),
        at(out_r), stream()))
    torch.cuda.synchronize()
    result = []
    for t, fill in ((out_s, SENT_F), (out_i, SENT_I), (out_a, SENT_F), (cnt, SENT_C), (out_o, SENT_F), (out_r, SENT_B)):
        if t is None:
            result.append(None)
            continue
        h = t.cpu().numpy()
        assert (h[0] == fill).all() and (h[-1] == fill).all(), "wrote outside its rows"
        result.append(h[1:-1])
    return tuple(result)


# ---------------------------------------------------------------------------------------------------------------------
# sskd_overlap_pairs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_pairs", [1, 257])
def test_overlap_pairs_at_every_size(gpu, native_lib, n_pairs):
    sets = dc.sized_sets()
    n = len(sets)
    g_lims, g_keys, _ = _device_store("sized", sets)
    ns = len(dc.SIZES)
    # identical (a copy, and a == b), half-shared, disjoint, every size against every size, set numbers out of range
    pairs = [(3 * i, 3 * i + 1) for i in range(ns)] + [(3 * i, 3 * i) for i in range(ns)]
    pairs += [(3 * i, 3 * i + 2) for i in range(ns)] + [(3 * i + 2, 3 * i) for i in range(ns)]
    pairs += [(3 * i, 3 * ns + i) for i in range(ns)]
    pairs += [(3 * i, 3 * j + 2) for i in range(ns) for j in range(ns)]
    # subsets of the largest set against it and against each other: the shorter list is searched in the longer
    pairs += [(4 * ns + i, 3 * (ns - 1)) for i in range(ns)] + [(3 * (ns - 1) + 1, 4 * ns + i) for i in range(ns)]
    pairs += [(4 * ns + i, 4 * ns + j) for i in range(ns) for j in range(i)]
    pairs += [(n, 3), (3, n), (-1, 6), (6, -5), (n + 1000, -1), (2**31 - 1, -(2**31))]
    pairs = pairs[:n_pairs] if n_pairs == 1 else (pairs * 2)[:n_pairs]
    if n_pairs == 1:
        pairs = [(3 * 7, 3 * 7 + 2)]            # 4 097 keys against their half-shared partner
    a = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device="cuda")
    b = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device="cuda")
    inter = torch.full((n_pairs + 2,), SENT_C, dtype=torch.int32, device="cuda")
    union = torch.full((n_pairs + 2,), SENT_C, dtype=torch.int32, device="cuda")
    jac = torch.full((n_pairs + 2,), SENT_F, dtype=torch.float64, device="cuda")
    _native.check(native_lib.sskd_overlap_pairs(
        g_lims.data_ptr(), g_keys.data_ptr(), n, a.data_ptr(), b.data_ptr(), n_pairs, inter.data_ptr() + 4,
        union.data_ptr() + 4, jac.data_ptr() + 8, stream()))
    torch.cuda.synchronize()
    inter, union, jac = inter.cpu().numpy(), union.cpu().numpy(), jac.cpu().numpy()
    for t, fill in ((inter, SENT_C), (union, SENT_C), (jac, SENT_F)):
        assert t[0] == fill and t[-1] == fill, "wrote outside its rows"
    empty = np.zeros(0, np.uint64)
    seen = set()
    for i, (x, y) in enumerate(pairs):
        A = sets[x] if 0 <= x < n else empty
        B = sets[y] if 0 <= y < n else empty
        want = dc.jaccard_ref(A, B)
        assert (int(inter[i + 1]), int(union[i + 1])) == want[:2], (x, y)
        assert float(jac[i + 1]).hex() == want[2].hex(), (x, y)
        seen.add(want[2])
    if n_pairs > 1:
        assert {0.0, 1.0} <= seen and len(seen) > 25


@pytest.mark.gpu
def test_the_device_wrapper_of_overlap_pairs(gpu, native_lib):
    from semantic_search_kd_amd import TrigramStore, text_overlap
    from semantic_search_kd_amd.denoise import overlap_pairs_device

    texts = dc.texts()
    store = TrigramStore.build_from_texts(texts)
    rng = np.random.default_rng(5)
    a = rng.integers(0, len(texts), 300).astype(np.int32)
    b = rng.integers(0, len(texts), 300).astype(np.int32)
    a[:3], b[:3] = len(texts) - 1, (len(texts) - 1, 20, 6)          # the 6 000-character text
    _, _, jac = overlap_pairs_device(store, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    jac = jac.cpu().numpy()
    for i in range(300):
        assert float(jac[i]).hex() == text_overlap(texts[a[i]], texts[b[i]]).hex(), i


# ---------------------------------------------------------------------------------------------------------------------
# sskd_rank_denoise against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_pos", [0, 1, 3, 40])
@pytest.mark.parametrize("search_k", [1, 10, 100, 1024])
@pytest.mark.parametrize("nq", [1, 3, 65])
def test_rank_denoise_equals_the_restatement(gpu, native_lib, nq, search_k, n_pos):
    sets, jac = dc.family()
    store = _device_store("family", sets)
    scores, ids, lims, rows, aux = dc.ranking_case(nq, search_k, n_pos)
    ref = dc.denoise_ref(jac, scores, ids, lims, rows, aux, 0.7, 0.5)
    got = _rank_denoise(native_lib, store, scores, ids, lims, rows, aux, 0.7, 0.5)
    dc.same(got, ref, (nq, search_k, n_pos))
    if nq == 65 and search_k == 1024 and n_pos == 40:
        reason = ref[5]
        assert {0, 1, 2, 3} <= set(np.unique(reason).tolist()), "both rules, alone and together"
        assert (ids == len(sets) + 11).any() and (ids == -7).any() and len(set(ref[3].tolist())) > 10
        assert ref[3][2 + 4] == 0 and 0 < ref[3][1] <= (search_k * 2) // 3, "an all -1 window, an early -1"
        assert (ref[4] == 1.0).any(), "a candidate equal to a positive"


@pytest.mark.gpu
@pytest.mark.parametrize("width", rw.WIDTHS)
def test_rank_denoise_walk_at_the_round_boundaries(gpu, native_lib, width):
    """The shared hand-made rankings over the first 200 sets of the family.  This kernel's own row of the table in
    ``csrc/ranking_walk.h``: the first -1 ends the window and nothing behind it is kept, but every other id - outside
    the store, or negative like -9 - is the empty set and STAYS in the output (the select that follows drops it)."""
    sets, _ = dc.family()
    n = 200
    g_lims, g_keys, _ = _device_store("family", sets)
    jac = dc.Pairs(sets[:n])
    ids = rw.ids(n, width)
    scores = rw.descending_scores(width, low=0.0, high=1.0)
    lims = np.arange(0, 2 * rw.NQ + 1, 2, dtype=np.int64)
    rows = np.array([r for q in range(rw.NQ) for r in (q + 3, q + 43)], np.int32)
    aux = np.random.default_rng(width).random((rw.NQ, width)).astype(np.float32)
    end = rw.first_pad(ids)
    for use_store, use_aux in ((True, True), (False, False)):
        ref = dc.denoise_ref(jac if use_store else None, scores, ids, lims, rows, aux if use_aux else None, 0.7, 0.5)
        got = _rank_denoise(native_lib, (g_lims, g_keys, n) if use_store else None, scores, ids, lims, rows,
                            aux if use_aux else None, 0.7, 0.5)
        dc.same(got, ref, (width, use_store, use_aux))
    assert ref[3].tolist() == end.tolist(), "no rule: a copy of the window up to the first -1, -9 and all"
    if width >= 63:
        assert (ref[1][4, :end[4]] == ids[4]).all() and ref[1][4, 2] == -9


@pytest.mark.gpu
@pytest.mark.parametrize("rules", ["overlap", "teacher", "both", "neither"])
@pytest.mark.parametrize("optional", [True, False])
def test_each_rule_alone_both_and_neither(gpu, native_lib, rules, optional):
    sets, jac = dc.family()
    store = _device_store("family", sets)
    scores, ids, lims, rows, aux = dc.ranking_case(65, 100, 3)
    use_store, use_aux = rules in ("overlap", "both"), rules in ("teacher", "both")
    ref = dc.denoise_ref(jac if use_store else None, scores, ids, lims, rows, aux if use_aux else None, 0.6, 0.4)
    got = _rank_denoise(native_lib, store if use_store else None, scores, ids, lims, rows, aux if use_aux else None,
                        0.6, 0.4, optional=optional)
    dc.same(got, ref, (rules, optional))
    if rules == "neither":
        # a copy of the window up to the first -1
        for q in range(65):
            n = ref[3][q]
            assert np.array_equal(ref[1][q, :n], ids[q, :n]) and (n == 100 or ids[q, n] == -1)
        assert (ref[5] == 0).all() and (ref[4] == 0.0).all()
    else:
        want_bits = {"overlap": {0, 1}, "teacher": {0, 2}, "both": {0, 1, 2, 3}}[rules]
        assert set(np.unique(ref[5]).tolist()) == want_bits
    if not use_aux and optional:
        assert np.isnan(got[2]).all(), "no aux in: NaN out"


@pytest.mark.gpu
def test_a_positive_longer_than_the_lds_cap(gpu, native_lib):
    """every positive is searched where it lies (4 097 and 6 011 keys) or staged whole (4 095, 4 096), against candidates
    of every size"""
    sets, jac = dc.family()
    store = _device_store("family", sets)
    big = [i for i, s in enumerate(sets) if len(s) >= 4095]
    assert sorted({len(sets[i]) for i in big}) == [4095, 4096, 4097, 6011] and len(dc.big_rows()) >= 4
    nq = len(big)
    ids = np.tile(np.array(big + list(range(0, 40)), np.int64), (nq, 1))
    k = ids.shape[1]
    scores = np.tile(np.linspace(1, 0, k, dtype=np.float32), (nq, 1))
    lims, rows = mc.csr([[p] for p in big])
    ref = dc.denoise_ref(jac, scores, ids, lims, rows, None, None, 0.45)
    got = _rank_denoise(native_lib, store, scores, ids, lims, rows, None, 0.0, 0.45)
    dc.same(got, ref, "big positives")
    assert ((ref[4] > 0.0) & (ref[4] < 1.0)).sum() >= nq and (ref[5] == 1).sum() >= nq


@pytest.mark.gpu
def test_the_edges_of_both_comparisons(gpu, native_lib):
    """(key) strict ``>`` for the overlap, ``>=`` for the teacher, both in fp64"""
    sets, jac = dc.family()
    store = _device_store("family", sets)
    assert jac(0, 1) == 4 / 5 == 0.8 and jac(0, 0) == 1.0
    # rank 0: inter / uni == 4 / 5 at threshold 0.8; rank 1: the positive itself; ranks 2 ..: the aux edges
    ids = np.array([[1, 0, 5, 6, 7, 8, 9, 2]], np.int64)
    scores = np.linspace(1, 0, 8, dtype=np.float32)[None]
    lims, rows = mc.csr([[0]])
    below = np.nextafter(np.float32(0.5), np.float32(0))
    aux = np.array([[0.1, 0.1, 0.5, below, np.float32(0.7), np.nextafter(np.float32(0.7), np.float32(1)), np.nan, 0.0]], np.float32)
    for thr in (0.5, 0.7):
        ref = dc.denoise_ref(jac, scores, ids, lims, rows, aux, thr, 0.8)
        got = _rank_denoise(native_lib, store, scores, ids, lims, rows, aux, thr, 0.8)
        dc.same(got, ref, thr)
        overlap, reason = got[4][0], got[5][0]
        assert overlap[0] == 0.8 and reason[0] == 0, "4 / 5 at threshold 0.8 is KEPT"
        assert overlap[1] == 1.0 and reason[1] == 1, "the positive itself goes"
        assert reason[6] == 0 and np.isnan(got[2][0]).any(), "a NaN aux is kept"
        if thr == 0.5:
            assert reason[2] == 2 and reason[3] == 0, "exactly 0.5 at threshold 0.5 is DROPPED, the float below it is kept"
        else:
            assert float(np.float32(0.7)) < 0.7
            assert reason[4] == 0 and reason[5] == 2, "float32(0.7) lies below 0.7 in fp64: KEPT; the next float32 goes"
    # the same pair a hair under the threshold
    got = _rank_denoise(native_lib, store, scores, ids, lims, rows, None, 0.0, np.nextafter(0.8, 0.0))
    assert got[5][0][0] == 1
    got = _rank_denoise(native_lib, store, scores, ids, lims, rows, None, 0.0, 1.0)
    assert (got[5] == 0).all() and got[3][0] == 8, "nothing exceeds 1.0"


# ---------------------------------------------------------------------------------------------------------------------
# composition: search -> denoise -> select
# ---------------------------------------------------------------------------------------------------------------------
_mixed = {}


def _mixed_index(gpu):
    """``mine_cases.mixed`` (2 083 rows, 70 queries) with texts: every row a random text, and for every query the rows
    at ranks 1, 3 and 5 of its ranking near-copies (one word replaced) of its first positive's text"""
    if not _mixed:
        from semantic_search_kd_amd import FAISSIndexBuilder, TrigramStore

        corpus, queries, _, lims, rows = mc.mixed()
        index = FAISSIndexBuilder(embedding_dim=mc.DIM, metric="ip", device=str(gpu))
        index.build_from_embeddings(np.array(corpus))
        D, I = index.search(np.array(queries), 100)
        rng = np.random.default_rng(751)
        vocab = [f"t{i:03d}" for i in range(400)]
        texts = [" ".join(vocab[int(i)] for i in rng.integers(0, 400, 30)) for _ in range(corpus.shape[0])]
        taken = set(int(r) for r in rows)
        for q in range(queries.shape[0]):
            if lims[q + 1] == lims[q]:
                continue
            words = texts[int(rows[lims[q]])].split(" ")
            for rank in (1, 3, 5):
                r = int(I[q, rank])
                if r in taken:
                    continue
                taken.add(r)
                copy = list(words)
                copy[int(rng.integers(0, 30))] = "edited"
                texts[r] = " ".join(copy)
        sets = [dc.trigram_keys_ref(t) for t in texts]
        rows_tensor = torch.from_numpy(index.to_numpy()).cuda()
        qd = torch.from_numpy(np.array(queries, np.float32)).cuda()
        S = torch.empty((qd.shape[0], rows_tensor.shape[0]), dtype=torch.float32, device="cuda")
        _native.check(_native.load().sskd_similarity(qd.data_ptr(), qd.shape[0], rows_tensor.data_ptr(), rows_tensor.shape[0],
                                                     mc.DIM, S.data_ptr(), stream()))
        _mixed.update(index=index, texts=texts, jac=dc.Pairs(sets), store=TrigramStore.build_from_texts(texts),
                      S=S.cpu().numpy())
    return _mixed


@pytest.mark.gpu
@pytest.mark.parametrize("search_k,top_k,margin", [(100, 5, 0.1), (100, 100, 0.3), (64, 1, 0.0), (10, 10, 2.0)])
def test_mine_negatives_is_denoise_then_select(gpu, native_lib, search_k, top_k, margin):
    from semantic_search_kd_amd import Denoising

    corpus, queries, _, lims, rows = mc.mixed()
    m = _mixed_index(gpu)
    index = m["index"]
    D, I = index.search(np.array(queries), search_k)
    den = dc.denoise_ref(m["jac"], D, I, lims, rows, None, None, 0.8)
    ref = mc.expected(den[0], den[1], lims, rows, m["S"], margin, top_k, fn=mc.walk)
    got = index.mine_negatives(np.array(queries), (lims, rows), top_k=top_k, search_k=search_k, margin=margin,
                               denoising=Denoising(0.8, None), trigrams=m["store"])
    mc.same(got, ref, (search_k, top_k, margin))
    plain = index.mine_negatives(np.array(queries), (lims, rows), top_k=top_k, search_k=search_k, margin=margin)
    if search_k == 100:
        assert (den[5] == 1).sum() > 60 and not np.array_equal(plain[2], got[2]), "the copies are inside the window"
    # denoising=None is the call without the keyword, bit for bit
    none = index.mine_negatives(np.array(queries), (lims, rows), top_k=top_k, search_k=search_k, margin=margin,
                                denoising=None, trigrams=None)
    mc.same(none, plain, "denoising=None")
    # the host-array form of the one call
    host = index.denoise_ranking(D, I, (lims, rows), Denoising(0.8, None), trigrams=m["store"], diagnostics=True)
    dc.same((host[0], host[1], None, host[3], host[4], host[5]), den, "denoise_ranking")
    assert host[2] is None


@pytest.mark.gpu
def test_the_overlap_only_call_replays_from_a_graph(gpu, native_lib):
    from semantic_search_kd_amd import Denoising

    corpus, queries, _, lims, rows = mc.mixed()
    m = _mixed_index(gpu)
    index = m["index"]
    qd = torch.from_numpy(np.array(queries, np.float32)).cuda()
    dl, dr = torch.from_numpy(np.array(lims)).cuda(), torch.from_numpy(np.array(rows)).cuda()
    call = lambda: index.mine_negatives_device(qd, dl, dr, top_k=5, search_k=100, margin=0.1,
                                               denoising=Denoising(0.8, None), trigrams=m["store"])
    eager = tuple(t.clone() for t in call())          # also warms the workspace and the store's copy in HBM
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, eager):
        assert torch.equal(got, want)
    assert (eager[2] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# the case the feature exists for
# ---------------------------------------------------------------------------------------------------------------------
class _Student:
    """stand-in student: the embedding of text "q<i>" / corpus text i is given directly"""

    device = "cuda:0"

    def __init__(self, texts, corpus, queries):
        self.rows = {t: corpus[i] for i, t in enumerate(texts)}
        self.queries = queries

    def encode_queries(self, queries, **kw):
        return np.stack([self.queries[int(q[1:])] for q in queries])

    def encode_documents(self, docs, **kw):
        return np.stack([self.rows[d] for d in docs])

    def compute_similarity(self, q, d):
        return (np.asarray(q, np.float64) @ np.asarray(d, np.float64).T).astype(np.float32)


class _Teacher:
    """stand-in teacher: confident (logit 3) about texts holding the word w007, unsure (logit 0) about the rest"""

    def __init__(self):
        self.calls = 0

    def score(self, pairs, batch_size=32):
        self.calls += 1
        return [3.0 if "w007" in t.split(" ") else 0.0 for _, t in pairs]

    @staticmethod
    def get_confidence(score):
        import math

        return 1.0 / (1.0 + math.exp(-float(score)))


@pytest.mark.gpu
def test_near_copies_of_the_positive_are_not_mined(gpu, native_lib):
    """(key) 30 of 300 texts are one-word edits of a query's positive and sit next to it in embedding space"""
    from semantic_search_kd_amd import ANCEMiner, Denoising, FAISSIndexBuilder, TrigramStore, text_overlap

    texts, corpus, queries, positives, copy_of = dc.copies_case()
    nq = len(positives)
    index = FAISSIndexBuilder(embedding_dim=corpus.shape[1], metric="ip", device=str(gpu))
    index.build_from_embeddings(np.array(corpus))
    store = TrigramStore.build_from_texts(texts)
    kw = dict(search_k=100, margin=2.0)      # every candidate is adversarial: the window itself is compared
    _, plain6, _, _ = index.mine_negatives(np.array(queries), positives, top_k=6, **kw)
    _, plain, _, _ = index.mine_negatives(np.array(queries), positives, top_k=5, **kw)
    _, clean, counts, _ = index.mine_negatives(np.array(queries), positives, top_k=5, denoising=Denoising(0.8, None),
                                               trigrams=store, **kw)
    for q in range(nq):
        assert copy_of[q] in plain[q], "without denoising the copy IS mined: the test discriminates"
        assert text_overlap(texts[copy_of[q]], texts[q]) > 0.8
        for r in clean[q]:
            assert r >= 0 and max(text_overlap(texts[r], texts[p]) for p in positives[q]) <= 0.8
        assert clean[q].tolist() == [r for r in plain6[q].tolist() if r != copy_of[q]][:5], "every other row is unchanged"
    assert (counts == 98).all(), "100 candidates less the positive and its copy"

    # the same through the miner: refresh builds the store once and keeps it across refreshes of the same corpus
    ids = [f"d{i}" for i in range(len(texts))]
    student = _Student(texts, np.array(corpus), np.array(queries))
    names = [f"q{q}" for q in range(nq)]
    pos_ids = [[f"d{q}"] for q in range(nq)]
    miner = ANCEMiner(student, margin=2.0, denoising=Denoising())
    miner.refresh(ids, list(texts))
    first_store = miner._trigrams
    miner.refresh(ids, list(texts))
    assert miner._trigrams is first_store and first_store.n_sets == len(texts)
    mined = miner.mine_from_index(names, pos_ids, top_k=5, search_k=100)
    assert mined == [[f"d{r}" for r in clean[q]] for q in range(nq)]
    bare = ANCEMiner(student, margin=2.0)
    bare.refresh(ids, list(texts))
    assert bare._trigrams is None
    assert bare.mine_from_index(names, pos_ids, top_k=5, search_k=100) == [[f"d{r}" for r in plain[q]] for q in range(nq)]

    # with a teacher: one scoring call for the whole window, and what it is confident about goes too
    teacher = _Teacher()
    with_teacher = miner.mine_from_index(names, pos_ids, top_k=5, search_k=100, teacher=teacher)
    assert teacher.calls == 1
    D, I = index.search(np.array(queries), 100)
    changed = 0
    for q in range(nq):
        want = [int(r) for r in I[q] if r != q and r != copy_of[q] and "w007" not in texts[r].split(" ")][:5]
        assert with_teacher[q] == [f"d{r}" for r in want]
        changed += want != clean[q].tolist()
    assert changed > 0, "the teacher rule dropped something the overlap rule kept"

    # the reference API over text dictionaries: a throw-away store over the distinct texts, one kernel call
    table = dict(zip(ids, texts))
    cands = [[f"d{r}" for r in I[q] if r != q][:20] for q in range(nq)]
    ref_api = bare.mine(names, pos_ids, cands, table, table, top_k=5)
    den_api = miner.mine(names, pos_ids, cands, table, table, top_k=5)
    for q in range(nq):
        assert f"d{copy_of[q]}" in ref_api[q] and f"d{copy_of[q]}" not in den_api[q]
        assert den_api[q] == [d for d in bare.mine(names[q:q + 1], pos_ids[q:q + 1], [cands[q]], table, table, top_k=6)[0]
                              if d != f"d{copy_of[q]}"][:5]
