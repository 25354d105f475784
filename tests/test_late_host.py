"""Late interaction, host side (no GPU): the restatements and the band stand on their own, the store's file format
round-trips, and the C-ABI declares the new symbols."""
import json
import re

import numpy as np
import pytest

import late_cases as lc
from conftest import REPO


def test_pack_restatement_agrees_with_fp64_normalisation_to_one_bf16_ulp():
    rng = np.random.default_rng(1)
    for scale in (1.0, 1e15, 2.0 ** -20):
        x = lc.bf16_values(lc.bf16_bits(rng.standard_normal((64, lc.DIM)).astype(np.float32) * np.float32(scale)))
        got = lc.bf16_values(lc.normalize_rows_bits(x)).astype(np.float64)
        x64 = x.astype(np.float64)
        want = x64 / np.sqrt((x64 * x64).sum(axis=1, keepdims=True))
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-300))) - 7)      # bf16: 8 significant bits
        assert (np.abs(got - want) <= ulp).all()
        assert np.abs(np.sqrt((got * got).sum(axis=1)) - 1).max() < 2.0 ** -8
    # the floor: an all-zero row stays zero, a row shorter than 1e-12 is divided by 1e-12
    z = lc.normalize_rows_bits(np.zeros((1, lc.DIM), np.float32))
    assert not z.any()
    tiny = lc.bf16_values(lc.bf16_bits(np.full((1, lc.DIM), 1e-15, np.float32)))
    got = lc.bf16_values(lc.normalize_rows_bits(tiny))
    assert np.array_equal(got, lc.bf16_values(lc.bf16_bits(tiny / np.float32(1e-12))))


def test_pack_rows_keeps_csr_order_and_drops_padding():
    name, hidden, lengths = lc.pack_cases()[-1]
    tokens, lims = lc.pack_rows(hidden, lengths)
    assert lims[-1] == lengths.sum() == tokens.shape[0]
    b = 1
    assert np.array_equal(tokens[lims[b]: lims[b + 1]], lc.normalize_rows_bits(lc.bf16_values(hidden[b, : lengths[b]])))


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -2.5], np.float32)
    assert lc.bf16_values(lc.bf16_bits(x)).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -2.5]


def _families():
    rng = np.random.default_rng(23)
    tok, lims = lc.sweep_store()
    big = lc.big_rows(lims)
    # the sweep's store is the GPU test's; here a slice of it (the long rows and a few short ones) keeps the fp32
    # emulation to a second
    rows = np.concatenate([big[:12], [7, 1, 3]])
    sub_lims = np.concatenate([[0], np.cumsum(lims[rows + 1] - lims[rows])]).astype(np.int64)
    sub = np.concatenate([tok[lims[r]: lims[r + 1]] for r in rows])
    q_bits, q_lims = lc.queries(rng, [1, 5, 32, 33, 64, 128])
    yield "sweep", q_bits, q_lims, sub, sub_lims
    q_bits, q_lims, t, l, _ = lc.last_tile_family()
    yield "last-tile", q_bits, q_lims, t, l
    q_bits, q_lims, t, l, _ = lc.negative_family()
    yield "negative", q_bits, q_lims, t, l
    q_bits, q_lims, t, l, _, _ = lc.separated_family()
    yield "separated", q_bits, q_lims, t, l


@pytest.mark.parametrize("family", list(_families()), ids=lambda f: f[0])
def test_fp32_emulation_lies_within_the_band(family):
    _, q_bits, q_lims, tok, lims = family
    ref = lc.Reference(q_bits, q_lims, tok, lims, emulate=True)
    live = ~np.broadcast_to(ref.empty, ref.s64.shape)
    err = np.abs(ref.f32[live].astype(np.float64) - ref.s64[live])
    assert (err <= ref.E[live]).all(), f"max |f32 - s64| / E = {(err / ref.E[live]).max():.3f}"
    assert np.isneginf(ref.s64[~live]).all()


def test_reference_matches_the_plain_definition():
    q_bits, q_lims, tok, lims, cand = lc.last_tile_family()
    ref = lc.Reference(q_bits, q_lims, tok, lims)
    for r in range(lims.size - 1):
        assert ref.s64[0, r] == pytest.approx(lc.s64(q_bits, tok[lims[r]: lims[r + 1]]), rel=1e-14)
    # the copy of a query token sits in the last row: every document scores at least that exact self-product
    qv = lc.bf16_values(q_bits).astype(np.float64)
    assert (ref.s64[0] > (qv * qv).sum(axis=1).min() - 1.0).all()


def test_negative_family_would_notice_a_zero_row():
    q_bits, q_lims, tok, lims, cand = lc.negative_family()
    ref = lc.Reference(q_bits, q_lims, tok, lims)
    got = ref.of_candidates(ref.s64, cand)
    E = ref.of_candidates(ref.E, cand, fill=0.0)
    # a zero-scored row would lift every per-token max to 0, so the score to 0: far outside the band
    assert (got < -100 * E).all() and (got < -0.5).all()


def test_separated_family_gaps_exceed_twice_the_band():
    q_bits, q_lims, tok, lims, cand, m = lc.separated_family()
    ref = lc.Reference(q_bits, q_lims, tok, lims)
    s = np.sort(ref.s64[0])
    assert len(set(m.tolist())) == m.size
    assert np.diff(s).min() > 2 * ref.E[0].max()
    assert np.diff(s).min() > 0.5
    assert np.array_equal(np.argsort(-ref.s64[0]), np.argsort(-m))          # more copies, higher score


def test_check_ranking_accepts_the_true_order_and_rejects_a_wrong_one():
    raw = np.array([[0.5, -np.inf, 2.0, 2.0, 1.0]], np.float32)
    cand = np.array([[10, -1, 30, 20, 40]], np.int64)
    D = np.array([[2.0, 2.0, 1.0]], np.float32)
    lc.check_ranking(D, np.array([[20, 30, 40]]), raw, cand, 3)
    with pytest.raises(AssertionError):
        lc.check_ranking(D, np.array([[30, 20, 40]]), raw, cand, 3)           # tie not by lower id
    with pytest.raises(AssertionError):
        lc.check_ranking(np.array([[2.0, 2.0, 0.5]], np.float32), np.array([[20, 30, 10]]), raw, cand, 3)
    full_D = np.array([[2.0, 2.0, 1.0, 0.5, -np.inf]], np.float32)
    lc.check_ranking(full_D, np.array([[20, 30, 40, 10, -1]]), raw, cand, 5)


def test_store_files_round_trip(tmp_path):
    from semantic_search_kd_amd import late

    rng = np.random.default_rng(3)
    lims = np.array([0, 3, 3, 10], np.int64)
    bits = lc.unit_token_bits(rng, 10)
    assert not late.is_late_dir(tmp_path)
    late.save_store(tmp_path, bits, lims, {"max_doc_tokens": 180, "max_query_tokens": 32})
    assert late.is_late_dir(tmp_path)
    assert (tmp_path / "late_tokens.bf16").stat().st_size == late.store_bytes(10) == 10 * 768
    got_bits, got_lims, meta = late.load_store(tmp_path)
    assert np.array_equal(got_bits, bits) and np.array_equal(got_lims, lims)
    assert meta["ntotal"] == 3 and meta["n_tokens"] == 10 and meta["max_doc_tokens"] == 180
    # a truncated token file, a foreign version and broken bounds are refused
    (tmp_path / "late_tokens.bf16").write_bytes(bits.tobytes()[:-2])
    with pytest.raises(ValueError):
        late.load_store(tmp_path)
    bits.tofile(tmp_path / "late_tokens.bf16")
    meta["format_version"] = 99
    (tmp_path / "late.json").write_text(json.dumps(meta))
    with pytest.raises(ValueError):
        late.load_store(tmp_path)
    for bad in ([1, 3], [0, 5, 3], []):
        with pytest.raises(ValueError):
            late.check_lims(bad)
    with pytest.raises(ValueError):
        late.check_lims([0, 3], n_rows=2)


def test_header_declares_the_late_symbols_and_the_tables_agree():
    from semantic_search_kd_amd import _build, _native

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sskd_amd.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(sskd_late_[a-z0-9_]+)\s*\(", text))
    want = {"sskd_late_pack_tokens", "sskd_late_rerank_plan", "sskd_late_rerank_workspace_bytes", "sskd_late_rerank"}
    assert declared == want
    assert want <= set(_native.SIGNATURES)
    assert "late.hip" in _build.SOURCES
    assert "#define SSKD_LATE_TQ_MAX 128" in text and "#define SSKD_LATE_R_MAX 1024" in text


def test_plan_and_refusals_need_no_device(native_lib):
    import ctypes as C

    wgs, threads, lds, chunk = (C.c_int() for _ in range(4))
    assert native_lib.sskd_late_rerank_plan(1024, 32, 100, 10, wgs, threads, lds, chunk) == 0
    assert threads.value == 256 and lds.value == 24 * 1024 and chunk.value % 4 == 0 and chunk.value >= 4
    assert wgs.value == 1024 * -(-100 // chunk.value)
    assert native_lib.sskd_late_rerank_plan(1, 128, 100, 10, wgs, threads, lds, chunk) == 0
    assert lds.value == 96 * 1024 and chunk.value == 4 and wgs.value == 25
    for bad in ((1, 0, 10, 1), (1, 129, 10, 1), (1, 32, 1025, 1), (1, 32, 10, 11), (1, 32, 10, 0), (0, 32, 10, 1)):
        assert native_lib.sskd_late_rerank_plan(*bad, None, None, None, None) == 1
    assert native_lib.sskd_late_rerank_workspace_bytes(3, 100) >= 3 * 100 * 4
    assert native_lib.sskd_late_rerank_workspace_bytes(3, 1025) == 0
