"""Denoising of mined negatives, host side (no GPU): the overlap against the reference's own values
(tests/golden/text_overlap.json), the trigram store against the plain-Python definition (``denoise_cases``), files,
settings, the argument checks of both entry points, and the miners with stand-in models."""
import ctypes as C
import dataclasses
import json
import sys

import numpy as np
import pytest

import denoise_cases as dc
from conftest import GOLDEN
from semantic_search_kd_amd import _native

ERR_INVALID = 1
K_MAX = _native.SSKD_K_MAX


# ---------------------------------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------------------------------
def test_text_overlap_equals_the_reference_bit_for_bit():
    """(key) tests/golden/text_overlap.json: what the REFERENCE'S ``compute_text_overlap`` returned"""
    from semantic_search_kd_amd import compute_text_overlap, text_overlap

    gold = json.loads((GOLDEN / "text_overlap.json").read_text())
    assert compute_text_overlap is text_overlap and len(gold) > 300
    values = []
    for rec in gold:
        got = text_overlap(rec["a"], rec["b"])
        assert isinstance(got, float) and got.hex() == rec["overlap"], (rec, got)
        _, _, mine = dc.jaccard_ref(dc.trigram_keys_ref(rec["a"]), dc.trigram_keys_ref(rec["b"]))
        assert mine.hex() == rec["overlap"], "the tests' own restatement agrees with the reference too"
        values.append(got)
    values = np.array(values)
    assert (values == 0.0).sum() > 10 and (values == 1.0).sum() > 10 and ((values > 0.8) & (values < 1.0)).sum() > 5
    assert ((values > 0.0) & (values <= 0.8)).sum() > 50


def test_the_golden_pairs_are_the_cases():
    gold = json.loads((GOLDEN / "text_overlap.json").read_text())
    want = [(a, b) for a, b in dc.text_pairs() if len(a) < 1000 and len(b) < 1000]
    assert [(r["a"], r["b"]) for r in gold] == want
    chars = set("".join(a for a, _ in want))
    assert {"İ", "ß", "\t", "日", "ï"} <= chars


# ---------------------------------------------------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------------------------------------------------
def _store(texts):
    from semantic_search_kd_amd import TrigramStore

    return TrigramStore.build_from_texts(texts)


def test_store_equals_the_definition_per_row():
    texts = dc.texts()
    store = _store(texts)
    assert store.n_sets == len(texts) and store.lims.dtype == np.int64 and store.keys.dtype == np.uint64
    assert store.nbytes == store.lims.nbytes + store.keys.nbytes
    sizes = []
    for i, t in enumerate(texts):
        want = dc.trigram_keys_ref(t)
        assert np.array_equal(store.keys_of(i), want), (i, t[:40])
        sizes.append(want.size)
    assert sizes[:6] == [0] * 6 and sizes[6] == 1 and max(sizes) > dc.LDS_CAP
    assert store.keys_of(6)[0] == (ord("a") << 42) | (ord("b") << 21) | ord("c")
    with pytest.raises(IndexError):
        store.keys_of(len(texts))
    empty = _store([])
    assert empty.n_sets == 0 and empty.lims.tolist() == [0] and empty.keys.size == 0


def test_blocks_of_the_vectorised_build_join_up(monkeypatch):
    from semantic_search_kd_amd import denoise

    texts = dc.texts()
    whole = _store(texts)
    monkeypatch.setattr(denoise, "_BUILD_CHUNK", 7)
    pieces = _store(texts)
    assert np.array_equal(pieces.lims, whole.lims) and np.array_equal(pieces.keys, whole.keys)


def test_append_and_take():
    texts = dc.texts()
    store = _store(texts[:50])
    assert store.append(texts[50:]) is store
    whole = _store(texts)
    assert np.array_equal(store.lims, whole.lims) and np.array_equal(store.keys, whole.keys)
    kept = np.array([3, 6, 7, 40, 41, len(texts) - 1, 12])
    part = whole.take(kept)
    assert part.n_sets == kept.size
    for j, i in enumerate(kept):
        assert np.array_equal(part.keys_of(j), whole.keys_of(int(i)))
    assert whole.take([]).n_sets == 0
    with pytest.raises(ValueError, match="outside"):
        whole.take([len(texts)])
    with pytest.raises(ValueError, match="outside"):
        whole.take([-1])


def test_file_round_trip_and_every_kind_of_damage(tmp_path):
    from semantic_search_kd_amd import TrigramStore
    from semantic_search_kd_amd.denoise import KEYS_FILE, LIMS_FILE

    store = _store(dc.texts()[:40])
    store.save(tmp_path / "ok")
    assert sorted(p.name for p in (tmp_path / "ok").iterdir()) == ["trigram_keys.npy", "trigram_lims.npy"]
    back = TrigramStore.load(tmp_path / "ok")
    assert np.array_equal(back.lims, store.lims) and np.array_equal(back.keys, store.keys)

    def damaged(name, lims, keys):
        d = tmp_path / name
        d.mkdir()
        np.save(d / LIMS_FILE, lims)
        np.save(d / KEYS_FILE, keys)
        return d

    lims, keys = store.lims.copy(), store.keys.copy()
    first = int(np.flatnonzero(np.diff(lims) >= 3)[0])           # a set of three keys or more
    lo = int(lims[first])
    bad = lims.copy()
    bad[first + 1], bad[first + 2] = lims[first + 2], lims[first + 1]
    if bad[first + 1] == bad[first + 2]:
        bad[first + 1] += 1
    with pytest.raises(ValueError, match="never decrease"):
        TrigramStore.load(damaged("decreasing", bad, keys))
    with pytest.raises(ValueError, match="end at"):
        TrigramStore.load(damaged("short_keys", lims, keys[:-1]))
    with pytest.raises(ValueError, match="end at"):
        TrigramStore.load(damaged("long_keys", lims, np.append(keys, keys[-1] + np.uint64(1))))
    swapped = keys.copy()
    swapped[lo], swapped[lo + 1] = keys[lo + 1], keys[lo]
    with pytest.raises(ValueError, match="strictly ascend"):
        TrigramStore.load(damaged("descending", lims, swapped))
    repeat = keys.copy()
    repeat[lo + 1] = repeat[lo]
    with pytest.raises(ValueError, match="strictly ascend"):
        TrigramStore.load(damaged("repeat", lims, repeat))
    shifted = lims.copy()
    shifted[0] = 1
    with pytest.raises(ValueError, match="start at 0"):
        TrigramStore.load(damaged("start", shifted, keys))
    with pytest.raises(ValueError, match="int64"):
        TrigramStore.load(damaged("dtype", lims.astype(np.int32), keys))
    with pytest.raises(ValueError, match="uint64"):
        TrigramStore.load(damaged("key_dtype", lims, keys.astype(np.int64)))
    # a set's first key may be smaller than the last key of the set before: that is no damage
    assert (np.diff(keys.astype(np.int64)) < 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# the settings
# ---------------------------------------------------------------------------------------------------------------------
def test_denoising_defaults_and_validation():
    from semantic_search_kd_amd import Denoising

    d = Denoising()
    assert (d.text_overlap_threshold, d.teacher_score_threshold) == (0.8, 0.7), "the reference's configs/kd.yaml"
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.text_overlap_threshold = 0.5
    assert Denoising(None, None).text_overlap_threshold is None
    assert Denoising(1, np.float32(0.5)) == Denoising(1.0, 0.5) and isinstance(Denoising(1, 0).text_overlap_threshold, float)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            Denoising(text_overlap_threshold=bad)
        with pytest.raises(ValueError, match="finite"):
            Denoising(teacher_score_threshold=bad)
    for bad in ("0.8", True, [0.8]):
        with pytest.raises(TypeError):
            Denoising(text_overlap_threshold=bad)


# ---------------------------------------------------------------------------------------------------------------------
# the entry points: every refusal comes before any HIP call (this test runs without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_denoise_symbols_and_methods_are_exported(native_lib):
    from semantic_search_kd_amd import ANCEMiner, FAISSIndexBuilder, TeacherMiner

    for name in ("sskd_overlap_pairs", "sskd_rank_denoise"):
        assert name in _native.SIGNATURES and hasattr(native_lib, name)
    for name in ("denoise_ranking", "denoise_ranking_device", "mine_negatives", "mine_negatives_device"):
        assert callable(getattr(FAISSIndexBuilder, name))
    assert ANCEMiner(None, denoising=None).denoising is None and TeacherMiner(None, denoising=None).denoising is None


_buf = (C.c_byte * 64)()
_P = C.addressof(_buf)


def _denoise(lib, nq=4, search_k=100, n_sets=50, aux_thr=0.7, ov_thr=0.8, null=()):
    ptr = lambda name: None if name in null else _P
    return lib.sskd_rank_denoise(
        ptr("lims"), ptr("grams"), n_sets, ptr("rank_scores"), ptr("rank_ids"), nq, search_k, ptr("pos_lims"),
        ptr("pos_rows"), ptr("aux"), aux_thr, ov_thr, ptr("scores"), ptr("ids"), ptr("out_aux"), ptr("counts"),
        ptr("overlap"), ptr("reason"), None)


@pytest.mark.parametrize(
    "kwargs,message",
    [
        (dict(search_k=0), b"search_k=0"),
        (dict(search_k=-3), b"search_k=-3"),
        (dict(search_k=K_MAX + 1), b"search_k=1025"),
        (dict(nq=-1), b"nq < 0"),
        (dict(n_sets=-1), b"n_sets < 0"),
        (dict(null=("lims",)), b"both of its pointers"),
        (dict(null=("grams",)), b"both of its pointers"),
        (dict(ov_thr=float("nan")), b"overlap_threshold is NaN"),
        (dict(aux_thr=float("nan")), b"aux_threshold is NaN"),
        (dict(null=("rank_scores",)), b"null"),
        (dict(null=("rank_ids",)), b"null"),
        (dict(null=("pos_lims",)), b"null"),
        (dict(null=("scores",)), b"null"),
        (dict(null=("ids",)), b"null"),
        (dict(null=("counts",)), b"null"),
    ],
)
def test_rank_denoise_argument_errors_need_no_gpu(native_lib, kwargs, message):
    rc = _denoise(native_lib, **kwargs)
    err = native_lib.sskd_last_error()
    assert rc == ERR_INVALID, (kwargs, rc, err)
    assert b"rank_denoise" in err and message in err, err


def _pairs(lib, n_sets=50, n_pairs=4, null=()):
    ptr = lambda name: None if name in null else _P
    return lib.sskd_overlap_pairs(ptr("lims"), ptr("grams"), n_sets, ptr("a"), ptr("b"), n_pairs, ptr("inter"),
                                  ptr("union"), ptr("jaccard"), None)


@pytest.mark.parametrize(
    "kwargs,message",
    [
        (dict(n_pairs=-1), b"n_pairs < 0"),
        (dict(n_sets=-2), b"n_sets < 0"),
        (dict(n_pairs=1 << 40), b"too large"),
        (dict(null=("lims",)), b"null store"),
        (dict(null=("grams",)), b"null store"),
        (dict(null=("a",)), b"null"),
        (dict(null=("b",)), b"null"),
        (dict(null=("inter",)), b"null"),
        (dict(null=("union",)), b"null"),
        (dict(null=("jaccard",)), b"null"),
    ],
)
def test_overlap_pairs_argument_errors_need_no_gpu(native_lib, kwargs, message):
    rc = _pairs(native_lib, **kwargs)
    err = native_lib.sskd_last_error()
    assert rc == ERR_INVALID, (kwargs, rc, err)
    assert b"overlap_pairs" in err and message in err, err


def test_empty_calls_are_no_ops(native_lib):
    everything = ("lims", "grams", "rank_scores", "rank_ids", "pos_lims", "pos_rows", "aux", "scores", "ids", "out_aux",
                  "counts", "overlap", "reason", "a", "b", "inter", "union", "jaccard")
    assert _denoise(native_lib, nq=0, null=everything) == 0
    assert _pairs(native_lib, n_pairs=0, null=everything) == 0


def _builder(n_rows):
    from semantic_search_kd_amd import FAISSIndexBuilder

    b = FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")
    b._n = n_rows
    return b


def test_mine_negatives_refuses_what_it_cannot_denoise():
    from semantic_search_kd_amd import Denoising

    b = _builder(len(dc.texts()))
    q = np.zeros((2, 384), np.float32)
    store = _store(dc.texts())
    with pytest.raises(ValueError, match="teacher rule needs texts"):
        b.mine_negatives(q, [[1], [2]], denoising=Denoising(), trigrams=store)
    with pytest.raises(ValueError, match="needs trigrams"):
        b.mine_negatives(q, [[1], [2]], denoising=Denoising(0.8, None))
    with pytest.raises(ValueError, match="without denoising"):
        b.mine_negatives(q, [[1], [2]], trigrams=store)
    with pytest.raises(TypeError, match="Denoising"):
        b.mine_negatives(q, [[1], [2]], denoising=0.8, trigrams=store)
    with pytest.raises(ValueError, match="sets for an index of 7 rows"):
        _builder(7).mine_negatives(q, [[1], [2]], denoising=Denoising(0.8, None), trigrams=store)
    with pytest.raises(ValueError, match="sets for an index of 7 rows"):
        _builder(7).denoise_ranking_device(None, None, None, None, Denoising(0.8, None), trigrams=store)
    # the checks of the call without denoising are still the first to answer
    with pytest.raises(ValueError, match="top_k=7"):
        b.mine_negatives(q, [[1], [2]], top_k=7, search_k=5)


# ---------------------------------------------------------------------------------------------------------------------
# the miners with stand-in models
# ---------------------------------------------------------------------------------------------------------------------
def _stand_ins():
    sys.path.insert(0, str(GOLDEN))
    from make_golden import HashedEmbeddingStudent, HashedTeacher, ance_case, teacher_mining_case

    return HashedEmbeddingStudent, HashedTeacher, ance_case, teacher_mining_case


def test_denoising_none_is_the_call_without_the_argument():
    from semantic_search_kd_amd import ANCEMiner, TeacherMiner

    Student, Teacher, ance_case, teacher_case = _stand_ins()
    queries, positives, candidates, docs = ance_case()
    for top_k in (5, 2):
        plain = ANCEMiner(Student(), margin=0.1).mine(queries, positives, candidates, docs, docs, top_k=top_k)
        assert ANCEMiner(Student(), margin=0.1, denoising=None).mine(queries, positives, candidates, docs, docs, top_k=top_k) == plain
        assert sum(len(x) for x in plain) > 5
    queries, candidates, docs = teacher_case()
    plain = TeacherMiner(Teacher(), 0.6).mine(queries, candidates, docs, top_k=10)
    teacher = Teacher()
    same = TeacherMiner(teacher, 0.6, denoising=None).mine(queries, candidates, docs, top_k=10,
                                                          positive_texts=[["anything"]] * len(queries))
    assert same == plain and teacher.calls == [(sum(len(c) for c in candidates), 32)]


def _teacher_restatement(teacher, queries, candidates, docs, positive_texts, denoising, confidence, top_k):
    """the rule as the issue states it, in loops: both rules on the candidates BEFORE the stable sort and the cut"""
    all_ids, all_scores = [], []
    for q, cand, pos in zip(queries, candidates, positive_texts):
        scored = [(d, teacher.score([(q, docs.get(d, ""))])[0]) for d in cand]
        kept = []
        for d, s in scored:
            if denoising.teacher_score_threshold is not None and teacher.get_confidence(s) >= denoising.teacher_score_threshold:
                continue
            if denoising.text_overlap_threshold is not None:
                o = max((dc.jaccard_ref(dc.trigram_keys_ref(docs.get(d, "")), dc.trigram_keys_ref(p))[2] for p in pos), default=0.0)
                if o > denoising.text_overlap_threshold:
                    continue
            kept.append((d, s))
        ranked = sorted(kept, key=lambda x: x[1], reverse=True)[:top_k]
        ranked = [(d, s) for d, s in ranked if teacher.get_confidence(s) >= confidence]
        all_ids.append([d for d, _ in ranked])
        all_scores.append([s for _, s in ranked])
    return all_ids, all_scores


@pytest.mark.parametrize("overlap_thr,teacher_thr", [(0.8, 0.7), (0.3, None), (None, 0.7), (None, None), (0.0, 0.9)])
def test_teacher_miner_with_denoising_equals_the_restatement(overlap_thr, teacher_thr):
    from semantic_search_kd_amd import Denoising, TeacherMiner

    _, Teacher, ance_case, teacher_case = _stand_ins()
    queries, candidates, docs = teacher_case()
    _, positives, _, _ = ance_case()
    # positives that resemble candidates: the first candidate's text with one word replaced, and a second plain text
    positive_texts = []
    for cand, pos in zip(candidates, positives):
        texts = [docs.get(d, "") for d in pos]
        if cand:
            words = docs.get(cand[0], "").split(" ")
            texts.append(" ".join(words[:-1] + ["w0"]) if len(words) > 2 else docs.get(cand[0], ""))
        positive_texts.append(texts)
    d = Denoising(overlap_thr, teacher_thr)
    plain = TeacherMiner(Teacher(), 0.6).mine(queries, candidates, docs, top_k=10)
    for top_k in (10, 3):
        teacher = Teacher()
        got = TeacherMiner(teacher, 0.6, denoising=d).mine(queries, candidates, docs, top_k=top_k, positive_texts=positive_texts)
        assert len(teacher.calls) == 1, "one scoring pass: the rule reuses the scores"
        want = _teacher_restatement(Teacher(), queries, candidates, docs, positive_texts, d, 0.6, top_k)
        assert got == want
    if overlap_thr is None and teacher_thr is None:
        assert TeacherMiner(Teacher(), 0.6, denoising=d).mine(queries, candidates, docs, top_k=10) == plain
    else:
        got10 = TeacherMiner(Teacher(), 0.6, denoising=d).mine(queries, candidates, docs, top_k=10, positive_texts=positive_texts)
        assert got10 != plain, "the case discriminates: the rule drops something the plain miner returns"
    with pytest.raises(ValueError, match="positive text lists"):
        TeacherMiner(Teacher(), 0.6, denoising=d).mine(queries, candidates, docs, positive_texts=[[]])
    with pytest.raises(TypeError, match="Denoising"):
        TeacherMiner(Teacher(), 0.6, denoising=0.8)


def test_curriculum_hands_denoising_to_stages_two_and_three(monkeypatch):
    from semantic_search_kd_amd import Denoising, mining

    seen = []

    class Bm25:
        def __init__(self, path):
            pass

        def mine(self, queries, positives, top_k=100):
            return [["d1", "d2"] for _ in queries]

    class Teach:
        def __init__(self, teacher, confidence_threshold=0.6, denoising=None):
            seen.append(("teacher", denoising))

        def mine(self, queries, candidates, texts, top_k=10, **kw):
            seen.append(("teacher.mine", kw))
            return [["d1"] for _ in queries], [[0.5] for _ in queries]

    class Ance:
        def __init__(self, student, margin=0.1, denoising=None):
            seen.append(("ance", denoising))

        def mine(self, *a, **kw):
            return [["d2"] for _ in a[0]]

    monkeypatch.setattr(mining, "BM25Miner", Bm25)
    monkeypatch.setattr(mining, "TeacherMiner", Teach)
    monkeypatch.setattr(mining, "ANCEMiner", Ance)
    texts = {"d1": "one", "d2": "two", "p": "positive text"}
    d = Denoising()
    mining.build_mining_curriculum(["q"], [["p", "gone"]], None, None, None, texts, stage=2, denoising=d)
    assert seen == [("teacher", d), ("teacher.mine", {"positive_texts": [["positive text", ""]]})]
    seen.clear()
    mining.build_mining_curriculum(["q"], [["p"]], None, None, None, texts, stage=3, denoising=d)
    assert seen == [("teacher", d), ("teacher.mine", {"positive_texts": [["positive text"]]}), ("ance", d)]
    seen.clear()
    mining.build_mining_curriculum(["q"], [["p"]], None, None, None, texts, stage=3)
    assert seen == [("teacher", None), ("teacher.mine", {}), ("ance", None)]
    seen.clear()
    assert mining.build_mining_curriculum(["q"], [["p"]], None, None, None, texts, stage=1, denoising=d)[0] == [["d1", "d2"]]
    assert seen == []
