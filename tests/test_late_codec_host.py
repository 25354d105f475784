"""The compressed token store, host side (no GPU): the byte order, the bucket rule, the file format, the refusals of
``check_codec`` and a sanity condition on the restatement itself."""
import json

import numpy as np
import pytest

import late_cases as lc
import late_codec_cases as cc


@pytest.mark.parametrize("nbits", [2, 4])
def test_byte_order_over_all_positions(nbits):
    per = 8 // nbits
    pos = cc.positions()
    assert sorted(pos.tolist()) == list(range(384))
    for d in (0, 7, 8, 15, 16, 383):
        s, h, e = d // 16, (d // 8) % 2, d % 8
        assert pos[d] == 192 * h + 8 * s + e
    # one column at a time: exactly its bits are set, in the byte and at the shift the rule names
    full = (1 << nbits) - 1
    for d in range(384):
        codes = np.zeros((1, 384), np.uint8)
        codes[0, d] = full
        packed = cc.pack_codes(codes, nbits)
        assert packed.shape == (1, 48 * nbits)
        want = np.zeros(48 * nbits, np.uint8)
        want[pos[d] // per] = full << (nbits * (pos[d] % per))
        assert np.array_equal(packed[0], want), d
    # lane half h of a row reads bytes [24 nbits h, 24 nbits (h + 1)): k-step s of it is nbits bytes
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 1 << nbits, (5, 384)).astype(np.uint8)
    packed = cc.pack_codes(codes, nbits)
    assert np.array_equal(cc.unpack_codes(packed, nbits), codes)
    for h in range(2):
        for s in range(24):
            chunk = packed[:, 24 * nbits * h + nbits * s: 24 * nbits * h + nbits * (s + 1)].astype(np.uint64)
            word = sum(chunk[:, b] << np.uint64(8 * b) for b in range(nbits))
            for e in range(8):
                got = (word >> np.uint64(nbits * e)) & np.uint64(full)
                assert np.array_equal(got, codes[:, 16 * s + 8 * h + e])


@pytest.mark.parametrize("nbits", [2, 4])
def test_bucket_rule_ties_extremes_and_nan(nbits):
    L = 1 << nbits
    cut = (np.arange(1, L, dtype=np.float32) - L / 2) / np.float32(8)           # exact in bf16 and fp32
    w = (np.arange(L, dtype=np.float32) - (L - 1) / 2) / np.float32(8)
    cen = np.zeros((1, 384), np.uint16)
    x = np.zeros((1, 384), np.float32)
    x[0, : L - 1] = cut                               # on a cutoff: the lower bucket
    x[0, L - 1: 2 * L - 2] = cut + np.float32(2.0 ** -7)   # just above it: the upper bucket
    x[0, 2 * L - 2] = -1e30
    x[0, 2 * L - 1] = 1e30
    x[0, 2 * L] = np.inf
    x[0, 2 * L + 1] = -np.inf
    x[0, 2 * L + 2] = np.nan
    tok = lc.bf16_bits(np.where(np.isnan(x), 0, x))
    tok[0, 2 * L + 2] = 0x7FC0                        # a bf16 NaN
    cid, scale, packed, dec = cc.compress_rows(tok, [0], cen, cut, w, nbits)
    codes = cc.unpack_codes(packed, nbits)[0]
    assert codes[: L - 1].tolist() == list(range(L - 1))
    assert codes[L - 1: 2 * L - 2].tolist() == list(range(1, L))
    assert codes[2 * L - 2: 2 * L + 3].tolist() == [0, L - 1, L - 1, 0, 0]
    assert np.array_equal(lc.bf16_values(dec)[0], w[codes])   # centroid 0: dec is the bucket's weight (exact in bf16)
    assert cid.tolist() == [0] and np.isfinite(scale).all()
    assert np.array_equal(cc.decode_rows(cid, packed, cen, w, nbits), dec)
    # an assignment outside [0, C) is clamped, in compress and in decode
    cen3 = lc.unit_token_bits(np.random.default_rng(1), 3)
    a = cc.compress_rows(np.repeat(tok, 2, axis=0), [-5, 99], cen3, cut, w, nbits)
    assert a[0].tolist() == [0, 2]
    assert np.array_equal(cc.decode_rows([-1, 7], a[2], cen3, w, nbits), a[3])


def test_scale_is_the_pack_arithmetic_on_dec_and_floors_at_1e_12():
    rng = np.random.default_rng(5)
    cen, cut, w = cc.random_codec(rng, 7, 2)
    tok = lc.unit_token_bits(rng, 9)
    cid, scale, packed, dec = cc.compress_rows(tok, cc.assign_rows(tok, cen), cen, cut, w, 2)
    d = lc.bf16_values(dec).astype(np.float64)
    assert np.abs(scale * np.sqrt((d * d).sum(axis=1)) - 1).max() < 1e-6
    zero = cc.compress_rows(np.zeros((1, 384), np.uint16), [0], np.zeros((1, 384), np.uint16),
                            np.float32([-1, 0, 1]), np.float32([-2, 0, 0.5, 2]), 2)
    assert not zero[3].any() and zero[1][0] == np.float32(1.0) / np.float32(1e-12)


@pytest.mark.parametrize("nbits", [2, 4])
def test_store_files_round_trip(tmp_path, nbits):
    from semantic_search_kd_amd import late

    rng = np.random.default_rng(7)
    cen, cut, w = cc.random_codec(rng, 11, nbits)
    tok, lims = lc.sweep_store(seed=9, n_rows=30)
    cid, scale, packed, _ = cc.compress_rows(tok, cc.assign_rows(tok, cen), cen, cut, w, nbits)
    late.save_compressed_store(tmp_path, cid, scale, packed, cen, cut, w, lims, {"max_doc_tokens": 180, "max_query_tokens": 32})
    meta = json.loads((tmp_path / "late.json").read_text())
    assert meta["nbits"] == nbits and meta["n_centroids"] == 11 and meta["n_tokens"] == tok.shape[0] and meta["ntotal"] == 30
    assert (tmp_path / "late_codes.u8").stat().st_size == tok.shape[0] * 48 * nbits
    assert (tmp_path / "late_codec_centroids.bf16").stat().st_size == 11 * 768
    for name in late.COMPRESSED_FILES:
        assert (tmp_path / name).exists(), name
    assert not (tmp_path / "late_tokens.bf16").exists() and not list(tmp_path.glob("*.pkl"))
    assert late.is_late_dir(tmp_path) and late.stored_nbits(tmp_path) == nbits
    got = late.load_compressed_store(tmp_path)
    for a, b in zip(got[:7], (cid, scale, packed, cen, cut, w, lims)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert late.store_bytes(10, nbits) == 10 * (104 if nbits == 2 else 200) and late.store_bytes(10) == 7680
    assert late.codec_bytes(11, nbits) == 11 * 768 + 4 * (2 * (1 << nbits) - 1)
    # a truncated code file is refused; a bf16 directory (no "nbits") reads as uncompressed
    (tmp_path / "late_codes.u8").write_bytes(b"\0" * 5)
    with pytest.raises(ValueError, match="late_codes.u8"):
        late.load_compressed_store(tmp_path)
    plain = tmp_path / "plain"
    late.save_store(plain, tok, lims, {})
    assert late.stored_nbits(plain) == 0 and np.array_equal(late.load_store(plain)[0], tok)


def test_check_codec_refusals():
    from semantic_search_kd_amd import late

    rng = np.random.default_rng(11)
    cen, cut, w = cc.random_codec(rng, 3, 2)
    bits, c2, w2, nbits = late.check_codec(cen, cut, w)
    assert nbits == 2 and np.array_equal(bits, cen) and np.array_equal(c2, cut) and np.array_equal(w2, w)
    assert late.check_codec(lc.bf16_values(cen), cut, w)[0].tolist() == cen.tolist()      # fp32 centroids round to bf16
    assert late.check_codec(*cc.random_codec(rng, 1, 4))[3] == 4
    bad_w = w.copy()
    bad_w[1] = np.inf
    nan_cut = cut.copy()
    nan_cut[0] = np.nan
    nan_cen = cen.copy()
    nan_cen[0, 0] = 0x7F80
    for what, args in (("unsorted cutoffs", (cen, cut[::-1].copy(), w)), ("non-finite weights", (cen, cut, bad_w)),
                       ("non-finite cutoffs", (cen, nan_cut, w)), ("non-finite centroids", (nan_cen, cut, w)),
                       ("C = 0", (cen[:0], cut, w)), ("C > 65 536", (np.zeros((65537, 384), np.uint16), cut, w)),
                       ("centroid width", (cen[:, :383], cut, w)), ("centroid rank", (cen[0], cut, w)),
                       ("cutoff count", (cen, cut[:2], w)), ("weight count", (cen, cut, w[:3])),
                       ("8 weights", (cen, np.arange(7, dtype=np.float32), np.arange(8, dtype=np.float32)))):
        with pytest.raises(ValueError):
            late.check_codec(*args)
        assert what
    with pytest.raises(ValueError):
        late.store_bytes(10, 3)
    assert late.default_n_centroids(1 << 20) == 16384 and late.default_n_centroids(100) == 100
    assert late.default_n_centroids(10 ** 9) == 65536 and late.default_n_centroids(1 << 20, 1000) == 1000


@pytest.mark.parametrize("nbits,n_centroids", [(2, 1), (2, 16), (4, 1), (4, 16)])
def test_separated_family_keeps_its_fp64_order_under_compression(nbits, n_centroids):
    """A sanity condition on the restatement: with a codec fitted to the sweep's store, the compressed fp64 ranking of
    the separated family is the uncompressed one and neighbouring scores stay more than 0.5 apart."""
    store, _ = lc.sweep_store()
    cen, cut, w = cc.fit_codec(store[::4], n_centroids, nbits)
    q_bits, q_lims, tok, lims, cand, m = lc.separated_family()
    cid, scale, packed, dec = cc.compress_rows(tok, cc.assign_rows(tok, cen), cen, cut, w, nbits)
    plain = lc.Reference(q_bits, q_lims, tok, lims).s64[0]
    comp = cc.ReferenceC(q_bits, q_lims, dec, scale, lims)
    assert np.array_equal(np.argsort(-comp.s64[0], kind="stable"), np.argsort(-plain, kind="stable"))
    gaps = -np.diff(np.sort(comp.s64[0])[::-1])
    assert gaps.min() > 0.5, gaps.min()
    assert gaps.min() > 100 * comp.E.max()
    # the pair reference is the table's entry
    r = 3
    assert abs(cc.s64c(q_bits, dec[lims[r]: lims[r + 1]], scale[lims[r]: lims[r + 1]]) - comp.s64[0, r]) < 1e-12
    t = lc.bf16_values(tok).astype(np.float64)
    d = lc.bf16_values(dec).astype(np.float64) * scale[:, None]
    cos = (t * d).sum(axis=1) / np.sqrt((t * t).sum(axis=1))
    assert cos.min() > (0.75 if nbits == 2 else 0.9)


def test_header_declares_the_codec_symbols():
    from semantic_search_kd_amd import _native

    for name in ("sskd_latec_compress", "sskd_latec_rerank", "sskd_latec_rerank_plan",
                 "sskd_latec_rerank_workspace_bytes"):
        assert name in _native.SIGNATURES


def test_plan_and_refusals_need_no_device(native_lib):
    import ctypes as C

    wg, th, lds, chunk = (C.c_int() for _ in range(4))
    for nbits in (2, 4):
        assert native_lib.sskd_latec_rerank_plan(1024, 32, 100, 10, nbits, wg, th, lds, chunk) == 0
        assert th.value == 256 and lds.value == 24576 + 64 and wg.value >= 1024 and chunk.value % 4 == 0
    assert native_lib.sskd_latec_rerank_plan(3, 128, 7, 7, 2, wg, th, lds, chunk) == 0 and lds.value == 4 * 24576 + 64
    assert native_lib.sskd_latec_rerank_plan(1, 32, 100, 10, 3, wg, th, lds, chunk) == 1
    assert native_lib.sskd_latec_rerank_plan(1, 129, 100, 10, 2, wg, th, lds, chunk) == 1
    assert native_lib.sskd_latec_rerank_plan(1, 32, 10, 11, 2, wg, th, lds, chunk) == 1
    assert native_lib.sskd_latec_rerank_workspace_bytes(3, 100) == native_lib.sskd_late_rerank_workspace_bytes(3, 100) > 0
    # refused before any device call: nbits, C, a range outside the store, null pointers
    assert native_lib.sskd_latec_compress(None, None, 0, None, 1, None, None, 3, None, None, None, 0, 0, None) == 1
    assert native_lib.sskd_latec_compress(None, None, 0, None, 0, None, None, 2, None, None, None, 0, 0, None) == 1
    assert native_lib.sskd_latec_compress(None, None, 5, None, 1, None, None, 2, None, None, None, 3, 7, None) == 1
    assert native_lib.sskd_latec_compress(None, None, 5, None, 1, None, None, 2, None, None, None, 0, 5, None) == 1
    assert native_lib.sskd_latec_compress(None, None, 0, None, 1, None, None, 2, None, None, None, 0, 0, None) == 0   # n = 0
