"""Candidate generation from the compressed store, host side (no GPU): the restatement stands on its own, the list
files round-trip and damaged ones are refused, the C-ABI declares the new symbols and refuses bad arguments before any
device call."""
import ctypes as C
import json
import re

import numpy as np
import pytest

import late_cases as lc
import late_codec_cases as cc
import plaid_cases as pc
from conftest import REPO


def _small_world(seed=3, n_rows=60, n_centroids=7):
    rng = np.random.default_rng(seed)
    td = rng.integers(0, 6, n_rows)
    td[5] = 0
    lims = np.concatenate([[0], np.cumsum(td)]).astype(np.int64)
    cid = rng.integers(0, n_centroids, int(lims[-1])).astype(np.int32)
    return rng, lims, cid


def test_build_lists_ref_against_a_triple_loop():
    rng, lims, cid = _small_world()
    cid[::7] = -3                                  # corrupt ids are clamped into [0, C)
    cid[1::11] = 99
    C_ = 7
    list_lims, list_rows = pc.build_lists_ref(cid, lims, C_)
    assert list_lims.dtype == np.int64 and list_rows.dtype == np.int32 and list_lims[0] == 0 and list_lims[-1] == list_rows.size
    for c in range(C_):
        want = []
        for r in range(lims.size - 1):
            for j in range(lims[r], lims[r + 1]):
                if min(max(int(cid[j]), 0), C_ - 1) == c and r not in want:
                    want.append(r)
        assert list_rows[list_lims[c]: list_lims[c + 1]].tolist() == sorted(want), f"list {c}"
    assert 5 not in list_rows.tolist(), "a row without tokens is in no list"


def test_every_centroid_probed_and_full_R_ranks_all_rows_by_approx():
    rng, lims, cid = _small_world(seed=4, n_centroids=5)
    C_, n = 5, lims.size - 1
    q_lims = np.array([0, 3, 8], np.int64)
    S = rng.standard_normal((C_, 8)).astype(np.float32)
    S[:, 2] = S[:, 1]                               # ties across tokens
    lists = pc.build_lists_ref(cid, lims, C_)
    cand_I, cand_A, n_cand = pc.candidates_ref(S, q_lims, cid, lims, *lists, C_, nprobe=C_, R=64)
    has_tokens = np.flatnonzero(lims[1:] > lims[:-1])
    for q in range(2):
        approx = pc.interaction_ref(S[:, q_lims[q]: q_lims[q + 1]], cid, lims, C_)
        # by the plain definition, row by row
        for r in has_tokens:
            best = S[cid[lims[r]: lims[r + 1]]][:, q_lims[q]: q_lims[q + 1]].max(axis=0)
            acc = np.float32(0)
            for v in best:
                acc = np.float32(acc + v)
            assert acc.view(np.uint32) == approx[r].view(np.uint32)
        assert n_cand[q] == has_tokens.size
        order = sorted(has_tokens.tolist(), key=lambda r: (-float(approx[r]), r))
        assert cand_I[q, : len(order)].tolist() == order and (cand_I[q, len(order):] == -1).all()
        assert np.array_equal(cand_A[q, : len(order)].view(np.uint32), approx[order].view(np.uint32))
        assert np.isneginf(cand_A[q, len(order):]).all()


def test_probes_skip_nan_and_minus_infinity_and_break_ties_by_lower_centroid():
    S = np.array([[1.0, np.nan], [2.0, -np.inf], [2.0, np.nan], [np.nan, -np.inf], [-np.inf, 0.5]], np.float32)
    got = pc.probes_ref(S, 3)
    assert got[0].tolist() == [1, 2, 0]
    assert got[1].tolist() == [4, -1, -1]


def test_mask_words_follow_the_row_mask_format():
    allowed = np.zeros(70, bool)
    allowed[[0, 31, 32, 69]] = True
    w = pc.mask_words(allowed)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 1, 1 << 5]


def test_list_files_round_trip_and_damaged_files_are_refused(tmp_path):
    from semantic_search_kd_amd import late

    rng = np.random.default_rng(5)
    tok, lims = lc.sweep_store(seed=9, n_rows=40)
    codec = cc.random_codec(rng, 6, 2)
    cid, scale, codes, _ = cc.compress_rows(tok, cc.assign_rows(tok, codec[0]), *codec, 2)
    late.save_compressed_store(tmp_path, cid, scale, codes, *codec, lims, {"max_doc_tokens": 180, "max_query_tokens": 32})
    assert not late.has_centroid_lists(tmp_path)
    assert "centroid_lists" not in json.loads((tmp_path / "late.json").read_text())
    list_lims, list_rows = pc.build_lists_ref(cid, lims, 6)
    late.save_centroid_lists(tmp_path, list_lims, list_rows)
    assert late.has_centroid_lists(tmp_path) and all((tmp_path / f).exists() for f in late.LIST_FILES)
    meta = json.loads((tmp_path / "late.json").read_text())
    assert meta["centroid_lists"] is True and meta["n_centroids"] == 6 and meta["nbits"] == 2
    got = late.load_centroid_lists(tmp_path)
    assert np.array_equal(got[0], list_lims) and np.array_equal(got[1], list_rows)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    late.load_compressed_store(tmp_path)            # the store itself still loads

    def damaged(lims_=list_lims, rows_=list_rows):
        np.save(tmp_path / "late_list_lims.npy", lims_)
        np.save(tmp_path / "late_list_rows.npy", rows_)
        with pytest.raises(ValueError):
            late.load_centroid_lists(tmp_path)

    damaged(lims_=list_lims[:-1])                                             # a list short
    damaged(lims_=np.concatenate([list_lims[:-1], [list_lims[-1] + 1]]))      # ends past the rows
    damaged(lims_=np.concatenate([[1], list_lims[1:]]))                       # does not start at 0
    down = list_lims.copy()
    down[1] = down[2] + 1
    damaged(lims_=down)                                                       # descends
    damaged(rows_=list_rows[:-1])                                             # a row short
    bad = list_rows.copy()
    bad[0] = 40
    damaged(rows_=bad)                                                        # a row outside the store
    bad = list_rows.copy()
    bad[0] = -1
    damaged(rows_=bad)
    first_long = int(np.flatnonzero(np.diff(list_lims) >= 2)[0])
    swapped = list_rows.copy()
    a = list_lims[first_long]
    swapped[a], swapped[a + 1] = swapped[a + 1], swapped[a]
    damaged(rows_=swapped)                                                    # a list that does not ascend
    damaged(rows_=list_rows.astype(np.int64))                                 # the wrong type
    damaged(lims_=list_lims.astype(np.int32))
    np.save(tmp_path / "late_list_lims.npy", list_lims)
    np.save(tmp_path / "late_list_rows.npy", list_rows)
    late.load_centroid_lists(tmp_path)


def test_header_declares_the_plaid_symbols_and_the_tables_agree():
    from semantic_search_kd_amd import _build, _native

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sskd_amd.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(sskd_plaid_[a-z0-9_]+)\s*\(", text))
    want = {"sskd_plaid_centroid_scores", "sskd_plaid_candidates", "sskd_plaid_candidates_plan",
            "sskd_plaid_candidates_workspace_bytes"}
    assert declared == want
    assert want <= set(_native.SIGNATURES)
    assert "plaid.hip" in _build.SOURCES
    assert "#define SSKD_PLAID_NPROBE_MAX 32" in text


def _candidates(lib, q_lims=(0, 5, 10), nq=2, C_=8, n_rows=100, n_tokens=400, n_list=300, nprobe=2, R=16, ld=10, id_offset=0,
                ws_bytes=1 << 20):
    host = np.asarray(q_lims, np.int64)
    return lib.sskd_plaid_candidates(None, ld, host.ctypes.data if host.size else None, None, nq, C_, None, None, n_rows, n_tokens,
                                     None, None, n_list, None, nprobe, R, id_offset, None, None, None, None, ws_bytes, None)


def test_refusals_come_before_any_device_call(native_lib):
    lib = native_lib
    for what, args in (("nq < 0", dict(nq=-1)), ("Tq = 129", dict(q_lims=(0, 129, 134), ld=134)), ("Tq = 0", dict(q_lims=(0, 5, 5))),
                       ("q_lims[0] < 0", dict(q_lims=(-1, 4, 9))), ("C = 0", dict(C_=0)), ("C > 65 536", dict(C_=65537)),
                       ("nprobe = 0", dict(nprobe=0)), ("nprobe = 33", dict(nprobe=33, C_=64)), ("nprobe > C", dict(nprobe=9)),
                       ("R = 0", dict(R=0)), ("R = 1025", dict(R=1025)), ("n_rows < 0", dict(n_rows=-1)),
                       ("n_rows too large", dict(n_rows=2 ** 31)), ("n_tokens < 0", dict(n_tokens=-1)), ("id_offset < 0", dict(id_offset=-1)),
                       ("n_list < 0", dict(n_list=-1)), ("n_list > n_tokens", dict(n_list=401)), ("ld < tokens", dict(ld=9)),
                       ("null pointers", dict())):
        assert _candidates(lib, **args) == 1, what                      # SSKD_ERR_INVALID, and no fault on the null pointers
        assert lib.sskd_last_error().startswith(b"plaid_candidates"), what
    assert _candidates(lib, nq=0, q_lims=()) == 0, "nq = 0 is a successful no-op"
    scores = lambda T=10, C_=8, ld=10: lib.sskd_plaid_centroid_scores(None, T, None, C_, None, ld, None)   # noqa: E731
    for what, args in (("T < 0", dict(T=-1)), ("T too large", dict(T=65535 * 32 + 1, ld=1 << 22)), ("C = 0", dict(C_=0)),
                       ("C > 65 536", dict(C_=65537)), ("ld < T", dict(ld=9)), ("null pointers", dict())):
        assert scores(**args) == 1, what
    assert scores(T=0, ld=0) == 0, "no query tokens is a successful no-op"


def test_workspace_query_and_plan(native_lib):
    lib = native_lib
    ws = lambda nq, n_rows, nprobe: int(lib.sskd_plaid_candidates_workspace_bytes(nq, n_rows, nprobe))   # noqa: E731
    for bad in ((0, 100, 2), (-1, 100, 2), (1, -1, 2), (1, 2 ** 31, 2), (1, 100, 0), (1, 100, 33)):
        assert ws(*bad) == 0, bad
    one = ws(1, 100_000, 2)
    # sized for every row being a candidate: a row id and a score per row, and a bit
    assert one >= 100_000 * 8 + 100_000 // 8
    assert ws(3, 100_000, 2) == 3 * one and ws(2, 100_000, 4) > 2 * one
    assert ws(10_000, 100_000, 2) == 256 << 20, "the size query stops at its budget"
    assert ws(1, 200_000_000, 2) > 256 << 20, "one query's worth is always asked for"
    per, chunk, parts, wgs = C.c_size_t(), C.c_int(), C.c_int(), C.c_int()
    assert lib.sskd_plaid_candidates_plan(10_000, 32, 4096, 100_000, 2, 256, 0, per, chunk, parts, wgs) == 0
    assert per.value == one and chunk.value == (256 << 20) // one and 1 <= parts.value <= 64 and wgs.value >= 1
    assert lib.sskd_plaid_candidates_plan(3, 32, 4096, 100_000, 2, 256, one, per, chunk, parts, wgs) == 0
    assert chunk.value == 1, "a workspace of one query's worth runs the batch query by query"
    assert lib.sskd_plaid_candidates_plan(1, 128, 65536, 100_000, 32, 1024, 0, per, chunk, parts, wgs) == 0
    assert chunk.value == 1 and parts.value == 64
    assert lib.sskd_plaid_candidates_plan(3, 32, 4096, 100_000, 2, 256, one - 1, per, chunk, parts, wgs) == 1
    for bad in ((0, 32, 8, 10, 2, 4), (1, 0, 8, 10, 2, 4), (1, 129, 8, 10, 2, 4), (1, 32, 0, 10, 2, 4), (1, 32, 65537, 10, 2, 4),
                (1, 32, 8, -1, 2, 4), (1, 32, 8, 10, 0, 4), (1, 32, 8, 10, 9, 4), (1, 32, 64, 10, 33, 4), (1, 32, 8, 10, 2, 0),
                (1, 32, 8, 10, 2, 1025)):
        assert lib.sskd_plaid_candidates_plan(*bad, 0, None, None, None, None) == 1, bad


def test_clustered_family_is_what_the_gate_describes():
    fam = pc.clustered_family(n_docs=200, n_queries=5)
    td = np.diff(fam["lims"])
    assert td.min() >= 4 and td.max() <= 60 and 25 < td.mean() < 35
    assert fam["codec"][0].shape == (256, lc.DIM) and fam["codec"][1].size == 3 and fam["codec"][2].size == 4
    assert fam["q_lims"].tolist() == [0, 16, 32, 48, 64, 80]
    norms = np.linalg.norm(lc.bf16_values(fam["tok"]).astype(np.float64), axis=1)
    assert np.abs(norms - 1).max() < 2.0 ** -7
