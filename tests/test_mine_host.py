"""Hard-negative mining, host side (no GPU): exported symbols, argument checks, the normalisation of the positives, and
the NumPy model of the kernel's walk (``mine_cases.walk``) against ``select_adversarial`` - on the reference's own
selections (tests/golden/ance_mining.json) and on the tie cases the GPU tests run."""
import ctypes as C
import json
import sys

import numpy as np
import pytest

import mine_cases as mc
from conftest import GOLDEN
from semantic_search_kd_amd import _native
from semantic_search_kd_amd.mining import select_adversarial

ERR_INVALID = 1
K_MAX = _native.SSKD_K_MAX


def test_mining_symbols_and_methods_are_exported(native_lib):
    from semantic_search_kd_amd import ANCEMiner, FAISSIndexBuilder
    from semantic_search_kd_amd import index as index_module

    assert "sskd_index_mine_select" in _native.SIGNATURES and hasattr(native_lib, "sskd_index_mine_select")
    for name in ("mine_negatives", "mine_negatives_device"):
        assert callable(getattr(FAISSIndexBuilder, name))
    for name in ("mine_from_index", "mine_from_index_device", "_mine_from_index_host"):
        assert callable(getattr(ANCEMiner, name))
    assert callable(index_module.normalize_positives)


def _call(lib, n_rows=100, nq=4, search_k=100, top_k=5, margin=0.1, null=()):
    """every pointer is a small host buffer (the checks run before any HIP call) unless named in `null`"""
    buf = (C.c_byte * 80)()
    p = (C.addressof(buf) + 15) & ~15      # the call wants 16-byte aligned queries
    ptr = lambda name: None if name in null else p
    return lib.sskd_index_mine_select(
        ptr("tiled"), n_rows, ptr("queries"), nq, ptr("rank_scores"), ptr("rank_ids"), search_k, ptr("pos_lims"),
        ptr("pos_rows"), None, margin, top_k, 0, ptr("scores"), ptr("ids"), ptr("counts"), ptr("max_pos"), None)


@pytest.mark.parametrize(
    "kwargs,message",
    [
        (dict(top_k=0), b"top_k=0"),
        (dict(top_k=-2), b"top_k=-2"),
        (dict(top_k=6, search_k=5), b"top_k=6 > search_k=5"),
        (dict(search_k=K_MAX + 1), b"search_k=1025"),
        (dict(nq=-1), b"nq < 0"),
        (dict(n_rows=-5), b"n_rows < 0"),
        (dict(n_rows=(1 << 31) - 64), b"shard too large"),
        (dict(margin=float("nan")), b"NaN"),
        (dict(null=("queries",)), b"null"),
        (dict(null=("tiled",)), b"null"),
        (dict(null=("rank_scores",)), b"null"),
        (dict(null=("rank_ids",)), b"null"),
        (dict(null=("pos_lims",)), b"null"),
        (dict(null=("scores",)), b"null"),
        (dict(null=("ids",)), b"null"),
        (dict(null=("counts",)), b"null"),
        (dict(null=("max_pos",)), b"null"),
    ],
)
def test_argument_errors_need_no_gpu(native_lib, kwargs, message):
    rc = _call(native_lib, **kwargs)
    err = native_lib.sskd_last_error()
    assert rc == ERR_INVALID, (kwargs, rc, err)
    assert b"index_mine_select" in err and message in err, err


def test_no_queries_is_a_no_op(native_lib):
    assert _call(native_lib, nq=0, null=("queries", "tiled", "rank_scores", "rank_ids", "pos_lims", "scores", "ids",
                                         "counts", "max_pos")) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the product class: checks that run before anything touches the GPU
# ---------------------------------------------------------------------------------------------------------------------
def _builder(n_rows):
    from semantic_search_kd_amd import FAISSIndexBuilder

    b = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    b._n = n_rows
    return b


def test_mine_negatives_rejects_bad_arguments():
    b = _builder(50)
    q = np.zeros((2, 384), np.float32)
    with pytest.raises(ValueError, match="top_k=7"):
        b.mine_negatives(q, [[1], [2]], top_k=7, search_k=5)
    with pytest.raises(ValueError, match="top_k=0"):
        b.mine_negatives(q, [[1], [2]], top_k=0)
    with pytest.raises(ValueError, match="search_k=2000"):
        b.mine_negatives(q, [[1], [2]], search_k=2000)
    with pytest.raises(ValueError, match=r"outside \[0, 50\)"):
        b.mine_negatives(q, [[1], [50]])
    with pytest.raises(ValueError, match=r"outside \[0, 50\)"):
        b.mine_negatives(q, [[-1], [2]])
    with pytest.raises(ValueError, match="3 queries"):
        b.mine_negatives(q, [[1], [2], [3]])
    with pytest.raises(ValueError):                                  # ragged inside one query
        b.mine_negatives(q, [[1, [2, 3]], [2]])
    with pytest.raises(ValueError, match="integer"):
        b.mine_negatives(q, [[1.5], [2]])
    with pytest.raises(ValueError, match="limits"):                  # the CSR form: limits for another nq
        b.mine_negatives(q, (np.array([0, 1]), np.array([3])))
    with pytest.raises(ValueError, match="start at 0"):
        b.mine_negatives(q, (np.array([1, 1, 2]), np.array([3, 4])))
    with pytest.raises(ValueError, match="never decrease"):
        b.mine_negatives(q, (np.array([0, 2, 1]), np.array([3, 4])))
    with pytest.raises(ValueError, match="end at"):
        b.mine_negatives(q, (np.array([0, 1, 3]), np.array([3, 4])))
    with pytest.raises(ValueError, match=r"outside \[0, 50\)"):
        b.mine_negatives(q, (np.array([0, 1, 2]), np.array([3, 77])))


def test_positives_are_sorted_and_deduplicated_per_query():
    from semantic_search_kd_amd.index import normalize_positives

    lims, rows = normalize_positives([[9, 3, 3, 7], [], [5, 5], [0, 49]], 4, 50)
    assert lims.dtype == np.int64 and rows.dtype == np.int32
    assert lims.tolist() == [0, 3, 3, 4, 6] and rows.tolist() == [3, 7, 9, 5, 0, 49]
    lims2, rows2 = normalize_positives((np.array([0, 4, 4, 6, 8]), np.array([9, 3, 3, 7, 5, 5, 49, 0])), 4, 50)
    assert lims2.tolist() == lims.tolist() and rows2.tolist() == rows.tolist()
    lims3, rows3 = normalize_positives([], 0, 50)
    assert lims3.tolist() == [0] and rows3.size == 0
    lims4, rows4 = normalize_positives([[], []], 2, 0)
    assert lims4.tolist() == [0, 0, 0] and rows4.size == 0 and rows4.dtype == np.int32


# ---------------------------------------------------------------------------------------------------------------------
# the threshold is decided in fp64, whatever NumPy makes of a float32 scalar against a Python float
# ---------------------------------------------------------------------------------------------------------------------
def test_select_adversarial_decides_in_fp64():
    max_pos = np.float32(0.8125)
    ties = np.array([0.9, 0.8125, 0.8125, 0.7], np.float32)
    pos = np.array([0.1, max_pos], np.float32)
    assert select_adversarial("abcd", ties, pos, 0.0, 5) == ["a", "b", "c"]
    # max_pos + 1e-9 rounds back onto max_pos in fp32: an fp32 comparison would keep the ties
    assert select_adversarial("abcd", ties, pos, -1e-9, 5) == ["a"]
    _, _, scores, _, _, (d32, drounded) = mc.threshold_neighbours()
    in64, in32, rounded = mc.decisions(scores[0], scores[0, 0], 0.1)
    kept = select_adversarial(list(range(1, scores.shape[1])), scores[0, 1:], scores[0, :1], 0.1, scores.shape[1])
    assert sorted(kept) == (1 + np.flatnonzero(in64[1:])).tolist()
    assert d32 and drounded and set(kept) != set(1 + np.flatnonzero(in32[1:])) and set(kept) != set(1 + np.flatnonzero(rounded[1:]))


# ---------------------------------------------------------------------------------------------------------------------
# the model of the kernel's walk against the reference's selections
# ---------------------------------------------------------------------------------------------------------------------
def test_walk_reproduces_the_reference_fixture():
    """tests/golden/ance_mining.json: what the REFERENCE'S OWN ANCEMiner.mine selected.  Its candidates are ranked the
    way a search would (stable descending) and walked; positives are not candidates there, so nothing is dropped."""
    sys.path.insert(0, str(GOLDEN))
    from make_golden import HashedEmbeddingStudent, ance_case

    gold = json.loads((GOLDEN / "ance_mining.json").read_text())
    queries, positives, candidates, docs = ance_case()
    student = HashedEmbeddingStudent()
    q_embs = student.encode_queries(queries)
    checked = 0
    for margin in (0.1, 0.3, 0.0):
        for top_k in (5, 2):
            want = gold[f"margin{margin}_k{top_k}"]
            for qi, (pos_ids, cand_ids) in enumerate(zip(positives, candidates)):
                pos = student.compute_similarity(q_embs[qi:qi + 1], student.encode_documents([docs.get(d, "") for d in pos_ids]))[0] \
                    if pos_ids else np.zeros(0, np.float32)
                cand = student.compute_similarity(q_embs[qi:qi + 1], student.encode_documents([docs.get(d, "") for d in cand_ids]))[0] \
                    if cand_ids else np.zeros(0, np.float32)
                order = np.argsort(-cand.astype(np.float64), kind="stable")
                max_pos = np.float32(pos.max()) if pos.size else np.float32(0.0)
                k = max(top_k, 1)
                _, I, count, _ = mc.walk(cand[order], order, [], max_pos, margin, k)
                got = [cand_ids[i] for i in I[: min(count, k)]]
                assert got == want[qi] == select_adversarial(cand_ids, cand, pos, margin, top_k), (margin, top_k, qi)
                checked += len(got)
    assert checked > 100


@pytest.mark.parametrize("margin", [0.1, 0.0, -1e-9, -0.05])
@pytest.mark.parametrize("name", ["duplicates", "threshold_neighbours", "mixed", "chunked", "chunked_by_group"])
def test_walk_equals_the_oracle_on_the_gpu_cases(name, margin):
    case = getattr(mc, name.replace("_by_group", ""))()
    groups = case[3] if name == "chunked_by_group" else None
    scores = case[2]
    lims, rows = (case[4], case[5]) if name.startswith("chunked") else (case[3], case[4])
    for search_k in (1, 64, 65, 100, min(scores.shape[1], 200)):
        D, I = mc.full_ranking(scores, search_k)
        top_k = min(5, search_k)
        ref = mc.expected(D, I, lims, rows, scores, margin, top_k, groups, id_offset=7)
        got = mc.expected(D, I, lims, rows, scores, margin, top_k, groups, id_offset=7, fn=mc.walk)
        mc.same(got, ref, (name, margin, search_k))


def test_the_tie_cases_say_what_they_are_meant_to():
    corpus, queries, scores, lims, rows, copies = mc.duplicates()
    D, I = mc.full_ranking(scores, 100)
    at0 = mc.expected(D, I, lims, rows, scores, 0.0, 100)
    below = mc.expected(D, I, lims, rows, scores, -1e-9, 100)
    for q in (0, 1):
        assert set(copies[q]) <= set(at0[1][q].tolist()), "margin=0.0 keeps the copies of the positive"
        assert not set(copies[q]) & set(below[1][q].tolist()), "margin=-1e-9 drops them"
        assert at0[2][q] == below[2][q] + 3
        assert int(rows[lims[q]]) not in at0[1][q]
    assert below[2][0] == 0 and below[2][1] >= 5
    _, _, scores, lims, rows, (d32, drounded) = mc.threshold_neighbours()
    D, I = mc.full_ranking(scores, 150)
    ref = mc.expected(D, I, lims, rows, scores, 0.1, 150)
    in64, _, _ = mc.decisions(scores[0], scores[0, 0], 0.1)
    assert set(ref[1][0, : ref[2][0]].tolist()) == set((1 + np.flatnonzero(in64[1:])).tolist())
    assert 0 < ref[2][0] < 129


def test_the_mixed_case_covers_the_shapes():
    corpus, queries, scores, lims, rows = mc.mixed()
    n_pos = np.diff(lims)
    assert corpus.shape[0] % 32 and set(n_pos.tolist()) == {0, 1, 2, 64, 65} and queries.shape[0] == 70
    D, I = mc.full_ranking(scores, 100)
    inside = [np.isin(rows[lims[q]:lims[q + 1]], I[q]).sum() for q in range(70)]
    assert max(inside) == 2 and any(i < n for i, n in zip(inside, n_pos) if n), "positives inside and outside the window"
    ref = mc.expected(D, I, lims, rows, scores, 0.1, 5)
    assert (ref[2] > 5).any(), "counts above top_k"
    ref0 = mc.expected(D, I, lims, rows, scores, 0.0, 5)
    assert ((ref0[2] > 0) & (ref0[2] < 5)).any() and (ref0[1] == -1).any(), "fewer survivors than top_k: padding"
