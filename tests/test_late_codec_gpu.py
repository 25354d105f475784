"""The compressed token store on the MI355X: ``sskd_latec_compress`` against its NumPy restatement (bits), the
compressed MaxSim scores against the fp64 reference ``s64c`` inside the derived band ``E_c``, the ranking in its
tolerant and exact forms, independence of a score from everything but the pair and the codec, and a store with corrupt
centroid ids.

The sweep prints ``max |score - s64c| / E_c`` (DESIGN section 22 records it)."""
import numpy as np
import pytest
import torch

import late_cases as lc
import late_codec_cases as cc
from capi_helpers import stream
from semantic_search_kd_amd import FAISSIndexBuilder, LateInteractionIndex

pytestmark = pytest.mark.gpu

DIM = lc.DIM
SENTINEL = 0xA5


def _dev(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a).cuda()


def _flat(n_rows: int, gpu, id_offset: int = 0) -> FAISSIndexBuilder:
    rows = np.random.default_rng(5).standard_normal((n_rows, DIM)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device=str(gpu), id_offset=id_offset)
    flat.build_from_embeddings(rows)
    return flat


class Store:
    """A token store compressed by the RESTATEMENT (so the re-rank tests stand without the compress kernel) and held by a
    ``LateInteractionIndex``; ``dec`` and ``scale`` are what the reference reads."""

    def __init__(self, gpu, tok, lims, codec, nbits, id_offset=0, cid_override=None):
        self.cen, self.cut, self.w = codec
        self.nbits, self.lims, self.n = nbits, lims, lims.size - 1
        self.cid, self.scale, self.codes, _ = cc.compress_rows(tok, cc.assign_rows(tok, self.cen), *codec, nbits)
        if cid_override is not None:
            self.cid = cid_override(self.cid)
        self.dec = cc.decode_rows(self.cid, self.codes, self.cen, self.w, nbits)     # (clamps a cid out of range)
        self.late = LateInteractionIndex(_flat(self.n, gpu, id_offset))
        self.late.set_codec(*codec)
        self.late.set_compressed(self.cid, self.scale, self.codes, lims)

    def reference(self, q_bits, q_lims):
        return cc.ReferenceC(q_bits, q_lims, self.dec, self.scale, self.lims)

    def rerank(self, q_bits, q_lims, cand, k):
        D, I, raw = self.late.rerank_device(q_bits, q_lims, torch.from_numpy(cand).cuda(), k, return_raw=True)
        torch.cuda.synchronize()
        return D.cpu().numpy(), I.cpu().numpy(), raw.cpu().numpy()


def _codec(n_centroids, nbits, seed=31):
    return cc.random_codec(np.random.default_rng(seed + n_centroids + nbits), n_centroids, nbits)


_worlds = {}


@pytest.fixture
def world(gpu, request):
    """The sweep's store under (nbits, C), compressed once and left unchanged."""
    key = request.param
    if key not in _worlds:
        tok, lims = lc.sweep_store()
        _worlds[key] = Store(gpu, tok, lims, _codec(key[1], key[0]), key[0])
        _worlds[key].big = lc.big_rows(lims)
    return _worlds[key]


WORLDS = [(2, 1), (2, 300), (4, 1), (4, 300)]
world_ids = lambda k: f"b{k[0]}-C{k[1]}"   # noqa: E731


def _assert_in_band(raw, ref, cand, id_offset=0):
    want = ref.of_candidates(ref.s64, cand, id_offset)
    E = ref.of_candidates(ref.E, cand, id_offset, fill=0.0)
    absent = np.isneginf(want)
    assert np.array_equal(np.isneginf(raw), absent), "absent candidates (-1, no tokens) must score -inf and only they"
    err = np.abs(raw[~absent].astype(np.float64) - want[~absent])
    ratio = float((err / E[~absent]).max()) if err.size else 0.0
    print(f"max |score - s64c| / E_c = {ratio:.4f} over {err.size} scores")
    assert (err <= E[~absent]).all(), f"max |score - s64c| / E_c = {ratio:.4f}"
    return ratio


# ------------------------------------------------------------------------------------------------ compress
def _compress(lib, tok, assign, codec, nbits, row0=0, spare=0):
    """The kernel on ``tok`` into rows ``row0 ..`` of a store of ``row0 + n + spare`` sentinel rows."""
    cen, cut, w = codec
    n, nb = tok.shape[0], 48 * nbits
    total = row0 + n + spare
    cid = torch.full((total,), -77, dtype=torch.int32, device="cuda")
    scale = torch.full((total,), -3.0, dtype=torch.float32, device="cuda")
    codes = torch.full((total, nb), SENTINEL, dtype=torch.uint8, device="cuda")
    keep = (_dev(tok), _dev(np.asarray(assign, np.int64)), _dev(cen), _dev(cut), _dev(w))
    rc = lib.sskd_latec_compress(keep[0].data_ptr(), keep[1].data_ptr(), n, keep[2].data_ptr(), cen.shape[0], keep[3].data_ptr(),
                                 keep[4].data_ptr(), nbits, cid.data_ptr(), scale.data_ptr(), codes.data_ptr(), row0, total, stream())
    torch.cuda.synchronize()
    return rc, cid.cpu().numpy(), scale.cpu().numpy(), codes.cpu().numpy()


@pytest.mark.parametrize("nbits", [2, 4])
@pytest.mark.parametrize("n_centroids", [1, 3, 300])
def test_compress_bits_equal_the_restatement(gpu, native_lib, nbits, n_centroids):
    rng = np.random.default_rng(200 + n_centroids)
    codec = _codec(n_centroids, nbits)
    for n in (1, 5, 64, 257):
        # tokens near their centroid (small residuals, every bucket in use) and plain unit tokens (saturated buckets)
        tok = lc.unit_token_bits(rng, n)
        assign = cc.assign_rows(tok, codec[0])
        near = lc.bf16_values(codec[0][assign]) + rng.standard_normal((n, DIM)).astype(np.float32) * np.float32(DIM ** -0.5)
        tok[::2] = lc.bf16_bits(near)[::2]
        row0, spare = (0, 0) if n == 1 else (3, 2)
        rc, cid, scale, codes = _compress(native_lib, tok, assign, codec, nbits, row0, spare)
        assert rc == 0
        want = cc.compress_rows(tok, assign, *codec, nbits)
        rows = slice(row0, row0 + n)
        assert np.array_equal(cid[rows], want[0]), f"n={n}: cid"
        assert np.array_equal(codes[rows], want[2]), f"n={n}: codes"
        assert np.array_equal(scale[rows].view(np.uint32), want[1].view(np.uint32)), f"n={n}: scale"
        assert len(set(cc.unpack_codes(want[2], nbits).reshape(-1).tolist())) == 1 << nbits, "the case must use every bucket"
        # the sentinel rows on either side are untouched
        for lo, hi in ((0, row0), (row0 + n, row0 + n + spare)):
            assert (cid[lo:hi] == -77).all() and (scale[lo:hi] == -3.0).all() and (codes[lo:hi] == SENTINEL).all()


@pytest.mark.parametrize("nbits", [2, 4])
def test_compress_cutoff_ties_zero_token_and_clamped_assignments(gpu, native_lib, nbits):
    L = 1 << nbits
    rng = np.random.default_rng(7)
    cut = (np.arange(1, L, dtype=np.float32) - L / 2) / np.float32(8)
    w = (np.arange(L, dtype=np.float32) - (L - 1) / 2) / np.float32(8)
    w[L // 2 - 1] = 0.0                                   # the bucket of r = 0 (cutoffs strictly below 0: L / 2 - 1)
    cen = np.concatenate([np.zeros((1, DIM), np.uint16), lc.bf16_bits(rng.integers(-4, 5, (2, DIM)).astype(np.float32) / 8)])
    codec = (cen, cut, w)
    # row r: residuals exactly on cutoffs (and one bf16 step above / below them) around centroid r % 3; centroid
    # columns are multiples of 1/8, so t = c + cutoff is exact in bf16 and r = t - c is the cutoff again
    grid = np.concatenate([cut, cut + np.float32(2.0 ** -6), cut - np.float32(2.0 ** -6), [-9.0, 9.0]]).astype(np.float32)
    res = grid[rng.integers(0, grid.size, (6, DIM))]
    res[:, : grid.size] = grid
    assign = np.arange(6) % 3
    tok = lc.bf16_bits(lc.bf16_values(cen[assign]) + res)
    assert np.array_equal(lc.bf16_values(tok) - lc.bf16_values(cen[assign]), res), "the case must place residuals exactly"
    tok = np.concatenate([tok, np.zeros((1, DIM), np.uint16), tok[:3]])      # + an all-zero token on the zero centroid
    given = np.concatenate([assign, [0], [-1, 3, 2 ** 40]])                  # + assignments outside [0, 3): clamped
    rc, cid, scale, codes = _compress(native_lib, tok, given, codec, nbits)
    assert rc == 0
    want = cc.compress_rows(tok, given, *codec, nbits)
    assert want[0].tolist() == [0, 1, 2, 0, 1, 2, 0, 0, 2, 2]
    on_cut = cc.unpack_codes(want[2], nbits)[0, : L - 1]
    assert on_cut.tolist() == list(range(L - 1)), "a residual on a cutoff falls in the lower bucket"
    assert not want[3][6].any() and want[1][6] == np.float32(1.0) / np.float32(1e-12), "the 1e-12 floor decides"
    assert np.array_equal(cid, want[0]) and np.array_equal(codes, want[2])
    assert np.array_equal(scale.view(np.uint32), want[1].view(np.uint32))


def test_compress_refusals_leave_the_outputs_untouched(gpu, native_lib):
    lib = native_lib
    rng = np.random.default_rng(9)
    codec = _codec(3, 2)
    tok = lc.unit_token_bits(rng, 5)
    t, a, cen, cut, w = _dev(tok), _dev(np.zeros(5, np.int64)), _dev(codec[0]), _dev(codec[1]), _dev(codec[2])
    big = torch.zeros(8 + 3 * DIM, dtype=torch.bfloat16, device="cuda")

    def call(nbits=2, C=3, n=5, row0=0, n_store=5, cen_ptr=cen.data_ptr(), codes_off=0):
        cid = torch.full((16,), -77, dtype=torch.int32, device="cuda")
        scale = torch.full((16,), -3.0, dtype=torch.float32, device="cuda")
        codes = torch.full((16 * 192 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = lib.sskd_latec_compress(t.data_ptr(), a.data_ptr(), n, cen_ptr, C, cut.data_ptr(), w.data_ptr(), nbits, cid.data_ptr(),
                                     scale.data_ptr(), codes.data_ptr() + codes_off, row0, n_store, stream())
        torch.cuda.synchronize()
        return rc, bool((cid == -77).all() and (scale == -3.0).all() and (codes == SENTINEL).all())

    for what, args in (("nbits = 3", dict(nbits=3)), ("nbits = 8", dict(nbits=8)), ("C = 0", dict(C=0)), ("C > 65 536", dict(C=65537)),
                       ("n < 0", dict(n=-1)), ("rows past the store", dict(row0=1)), ("row0 < 0", dict(row0=-1, n_store=9)),
                       ("misaligned centroids", dict(cen_ptr=big.data_ptr() + 2)), ("misaligned codes", dict(codes_off=4)),
                       ("null centroids", dict(cen_ptr=None))):
        rc, intact = call(**args)
        assert rc == 1, what
        assert intact, f"{what}: something was written"
    rc, intact = call(n=0)
    assert rc == 0 and intact, "n = 0 is a successful no-op"
    rc, intact = call()
    assert rc == 0 and not intact


# ------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("shape", lc.SWEEP, ids=lambda s: f"nq{s[0]}-R{s[2]}")
@pytest.mark.parametrize("world", WORLDS, indirect=True, ids=world_ids)
def test_scores_lie_within_the_band_and_rank_in_order(world, shape):
    nq, tqs, R = shape
    rng = np.random.default_rng(100 + R)
    q_bits, q_lims = lc.queries(rng, tqs)
    must = np.concatenate([world.big[:12], [7]])     # every Td of the sweep and the row without tokens
    cand = lc.candidates(rng, nq, R, world.n, must=must)
    ref = world.reference(q_bits, q_lims)
    raws = []
    for k in sorted({1, min(10, R), R}):
        D, I, raw = world.rerank(q_bits, q_lims, cand, k)
        lc.check_ranking(D, I, raw, cand, k)
        assert not (I == 7).any(), "a row without tokens was returned"
        raws.append(raw)
    assert all(np.array_equal(r.view(np.uint32), raws[0].view(np.uint32)) for r in raws), "raw scores depend on k"
    _assert_in_band(raws[0], ref, cand)


def _family_store(gpu, tok, lims, nbits, n_centroids, fit=False, **kw):
    codec = cc.fit_codec(lc.sweep_store()[0][::4], n_centroids, nbits) if fit else _codec(n_centroids, nbits)
    return Store(gpu, tok, lims, codec, nbits, **kw)


@pytest.mark.parametrize("nbits,n_centroids", [(2, 1), (2, 300), (4, 1), (4, 300)])
def test_best_token_in_the_last_partial_tile(gpu, nbits, n_centroids):
    q_bits, q_lims, tok, lims, cand = lc.last_tile_family()
    st = _family_store(gpu, tok, lims, nbits, n_centroids)
    D, I, raw = st.rerank(q_bits, q_lims, cand, cand.shape[1])
    _assert_in_band(raw, st.reference(q_bits, q_lims), cand)
    lc.check_ranking(D, I, raw, cand, cand.shape[1])


@pytest.mark.parametrize("nbits", [2, 4])
def test_masked_rows_and_columns_are_not_scored(gpu, nbits):
    """Every true product is negative: a masked row that counted - as zeros, as a neighbour's row, or under a neighbour's
    (or an unset) scale - would win the max.  One zero centroid and tables that reach the tokens' range keep every
    decoded column negative, so the property survives the compression."""
    q_bits, q_lims, tok, lims, cand = lc.negative_family()
    vals = lc.bf16_values(tok)
    L = 1 << nbits
    cut = np.quantile(vals, np.arange(1, L) / L).astype(np.float32)
    w = np.quantile(vals, (np.arange(L) + 0.5) / L).astype(np.float32)
    st = Store(gpu, tok, lims, (np.zeros((1, DIM), np.uint16), cut, w), nbits)
    assert (lc.bf16_values(st.dec) < 0).all()
    ref = st.reference(q_bits, q_lims)
    assert (ref.s64 < -0.5).all()
    D, I, raw = st.rerank(q_bits, q_lims, cand, 3)
    assert (raw < -0.5).all(), "a zero-scored padding row or column lifted a score"
    _assert_in_band(raw, ref, cand)
    lc.check_ranking(D, I, raw, cand, 3)


@pytest.mark.parametrize("nbits,n_centroids", [(2, 1), (2, 16), (4, 1), (4, 16)])
def test_exact_ranking_on_the_separated_family(gpu, nbits, n_centroids):
    q_bits, q_lims, tok, lims, cand, m = lc.separated_family()
    st = _family_store(gpu, tok, lims, nbits, n_centroids, fit=True)
    ref = st.reference(q_bits, q_lims)
    R = cand.shape[1]
    D, I, raw = st.rerank(q_bits, q_lims, cand, R)
    _assert_in_band(raw, ref, cand)
    assert np.array_equal(I[0], np.argsort(-ref.s64[0], kind="stable"))
    D10, I10, _ = st.rerank(q_bits, q_lims, cand, 10)
    assert np.array_equal(I10[0], I[0, :10]) and np.array_equal(D10.view(np.uint32), D[:, :10].view(np.uint32))


@pytest.mark.parametrize("world", [(2, 300), (4, 300)], indirect=True, ids=world_ids)
def test_fewer_valid_candidates_than_k_pads(world):
    rng = np.random.default_rng(41)
    q_bits, q_lims = lc.queries(rng, [5, 32])
    cand = np.full((2, 12), -1, dtype=np.int64)
    cand[0, [3, 8]] = [world.big[0], 7]                 # one real candidate and the row without tokens
    cand[1, :4] = [world.n + 5, world.big[1], 2, -9]     # an id outside the store, two real ones, a negative id
    D, I, raw = world.rerank(q_bits, q_lims, cand, 10)
    lc.check_ranking(D, I, raw, cand, 10)
    assert (I[0] >= 0).sum() == 1 and I[0, 0] == world.big[0]
    assert sorted(I[1, :2].tolist()) == sorted([int(world.big[1]), 2]) and (I[1, 2:] == -1).all()
    _assert_in_band(raw, world.reference(q_bits, q_lims), cand)


@pytest.mark.parametrize("world", [(2, 300), (4, 1)], indirect=True, ids=world_ids)
def test_score_bits_depend_on_the_pair_alone(world):
    """A fixed (q, c): alone, in a batch of 67, first and last of a list of 200, two values of k, a repeated call."""
    rng = np.random.default_rng(43)
    q_bits, q_lims = lc.queries(rng, [(33, 5, 32, 1)[i % 4] for i in range(67)])
    bits = set()
    for qi, row in ((0, int(world.big[3])), (1, int(world.big[5])), (66, 3)):
        one_q = q_bits[q_lims[qi]: q_lims[qi + 1]]
        one_lims = np.array([0, one_q.shape[0]], np.int64)
        seen = []
        for _ in range(2):
            seen.append(world.rerank(one_q, one_lims, np.array([[row]], np.int64), 1)[2][0, 0])
        for pos, k in ((0, 1), (199, 10)):
            cand = lc.candidates(rng, 67, 200, world.n)
            cand[cand == row] = -1
            cand[qi, pos] = row
            seen.append(world.rerank(q_bits, q_lims, cand, k)[2][qi, pos])
        words = {np.float32(s).view(np.uint32).item() for s in seen}
        assert len(words) == 1, f"pair ({qi}, {row}): {len(words)} different score bit patterns {seen}"
        bits |= words
    assert len(bits) == 3


@pytest.mark.parametrize("nbits", [2, 4])
def test_id_offset_is_subtracted(gpu, nbits):
    q_bits, q_lims, tok, lims, cand = lc.last_tile_family()
    base = _family_store(gpu, tok, lims, nbits, 3).rerank(q_bits, q_lims, cand, 4)
    off = 1000
    shifted = _family_store(gpu, tok, lims, nbits, 3, id_offset=off)
    D, I, raw = shifted.rerank(q_bits, q_lims, cand + off, 4)
    assert np.array_equal(raw.view(np.uint32), base[2].view(np.uint32))
    assert np.array_equal(I, base[1] + off) and np.array_equal(D.view(np.uint32), base[0].view(np.uint32))
    _, I_low, raw_low = shifted.rerank(q_bits, q_lims, cand, 4)       # ids below the offset are no candidates
    assert np.isneginf(raw_low).all() and (I_low == -1).all()


@pytest.mark.parametrize("nbits", [2, 4])
def test_corrupt_centroid_ids_are_clamped_not_followed(gpu, nbits):
    """A store whose cid array holds values outside [0, C): the kernel reads them clamped into range, so the call
    completes and the scores are the restatement's on the clamped ids."""
    q_bits, q_lims, tok, lims, cand = lc.last_tile_family()

    def corrupt(cid):
        bad = cid.copy()
        bad[::3] = np.array([-1, 300, 2 ** 31 - 1, -2 ** 31, 5], np.int32)[np.arange(bad[::3].size) % 5]
        return bad

    st = _family_store(gpu, tok, lims, nbits, 5, cid_override=corrupt)
    assert (st.cid < 0).any() and (st.cid >= 5).any()
    D, I, raw = st.rerank(q_bits, q_lims, cand, cand.shape[1])
    _assert_in_band(raw, st.reference(q_bits, q_lims), cand)
    lc.check_ranking(D, I, raw, cand, cand.shape[1])


def test_rerank_refusals_leave_the_outputs_untouched(gpu, native_lib):
    lib = native_lib
    rng = np.random.default_rng(67)
    tok, lims = lc.sweep_store(seed=9, n_rows=40)
    st = Store(gpu, tok, lims, _codec(3, 2), 2)
    late = st.late
    R, k, nq = 8, 4, 2
    qt = _dev(lc.queries(rng, [130, 5])[0])
    cand = torch.from_numpy(lc.candidates(rng, nq, R, st.n)).cuda()
    need = int(lib.sskd_latec_rerank_workspace_bytes(nq, R))

    def call(lims_=(0, 5, 10), R_=R, k_=k, nbits=2, C=3, codes_off=0, cen_off=0, raw=True, ws_bytes=None):
        host = np.asarray(lims_, np.int64)
        dev = torch.from_numpy(host).cuda()
        outs = [torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda") for n in (nq * 16 * 4, nq * 16 * 8, nq * 16 * 4)]
        ws = torch.full((need + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = lib.sskd_latec_rerank(qt.data_ptr(), host.ctypes.data, dev.data_ptr(), nq, late.cid.data_ptr(), late.scale.data_ptr(),
                                   late.codes.data_ptr() + codes_off, nbits, late.centroids.data_ptr() + cen_off, C,
                                   late.weights.data_ptr(), late._lims_dev.data_ptr(), late.ntotal, late.n_tokens, cand.data_ptr(),
                                   R_, k_, 0, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr() if raw else None,
                                   ws.data_ptr(), need if ws_bytes is None else ws_bytes, stream())
        torch.cuda.synchronize()
        return rc, all(bool((b == SENTINEL).all()) for b in outs + [ws])

    for what, args in (("nbits = 3", dict(nbits=3)), ("nbits = 0", dict(nbits=0)), ("C = 0", dict(C=0)), ("C > 65 536", dict(C=65537)),
                       ("Tq = 129", dict(lims_=[0, 129, 134])), ("Tq = 0", dict(lims_=[0, 5, 5])),
                       ("k > R", dict(k_=R + 1)), ("k = 0", dict(k_=0)), ("R > 1024", dict(R_=1025, k_=1)),
                       ("misaligned codes", dict(codes_off=8)), ("misaligned centroids", dict(cen_off=2)),
                       ("a short workspace", dict(raw=False, ws_bytes=need - 1))):
        rc, intact = call(**args)
        assert rc == (2 if what == "a short workspace" else 1), what     # SSKD_ERR_WORKSPACE / SSKD_ERR_INVALID
        assert intact, f"{what}: something was written"
    rc, intact = call()
    assert rc == 0 and not intact
    rc, intact = call(raw=False)
    assert rc == 0 and not intact
