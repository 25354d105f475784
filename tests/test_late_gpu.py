"""Late interaction on the MI355X: the pack kernel against its NumPy restatement (bits), the MaxSim scores against the
fp64 reference inside the derived band E, the ranking in its tolerant and exact forms, independence of a score from
everything but the two token lists, and the Python layer (search, compact, save / load, graph capture, refusals).

The sweep prints ``max |score - s64| / E`` (DESIGN section 21 records it)."""

import numpy as np
import pytest
import torch

import late_cases as lc
from capi_helpers import stream
from semantic_search_kd_amd import FAISSIndexBuilder, GraphIndex, LateInteractionIndex, _native, late as late_mod

pytestmark = pytest.mark.gpu

DIM = lc.DIM
SENTINEL = 0xA5


def _bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _flat(n_rows: int, gpu, seed: int = 5, id_offset: int = 0) -> FAISSIndexBuilder:
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n_rows, DIM)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device=str(gpu), id_offset=id_offset)
    flat.build_from_embeddings(rows)
    return flat


def _late(tok_bits, tok_lims, gpu, id_offset: int = 0) -> LateInteractionIndex:
    late = LateInteractionIndex(_flat(tok_lims.size - 1, gpu, id_offset=id_offset))
    late.set_tokens(tok_bits, tok_lims)
    return late


def _rerank(late, q_bits, q_lims, cand, k):
    D, I, raw = late.rerank_device(q_bits, q_lims, torch.from_numpy(cand).cuda(), k, return_raw=True)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), raw.cpu().numpy()


class World:
    """The sweep's store on the device, computed once and left unchanged."""

    def __init__(self, gpu):
        self.tok, self.lims = lc.sweep_store()
        self.n = self.lims.size - 1
        self.big = lc.big_rows(self.lims)
        self.late = _late(self.tok, self.lims, gpu)


@pytest.fixture(scope="module")
def world(gpu):
    return World(gpu)


def _assert_in_band(raw, ref, cand, id_offset=0):
    want = ref.of_candidates(ref.s64, cand, id_offset)
    E = ref.of_candidates(ref.E, cand, id_offset, fill=0.0)
    absent = np.isneginf(want)
    assert np.array_equal(np.isneginf(raw), absent), "absent candidates (-1, no tokens) must score -inf and only they"
    err = np.abs(raw[~absent].astype(np.float64) - want[~absent])
    ratio = float((err / E[~absent]).max()) if err.size else 0.0
    print(f"max |score - s64| / E = {ratio:.4f} over {err.size} scores")
    assert (err <= E[~absent]).all(), f"max |score - s64| / E = {ratio:.4f}"
    return ratio


# ------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("case", lc.pack_cases(), ids=lambda c: c[0])
def test_pack_bits_equal_the_restatement(gpu, case):
    _, hidden, lengths = case
    want, lims = lc.pack_rows(hidden, lengths)
    B = hidden.shape[0]
    # the texts are written in REVERSE order behind 3 spare rows: the offsets, not the batch order, place them
    spare = 3
    offsets = spare + (lims[-1] - lims[1:])
    out = torch.full((spare + int(lims[-1]) + 2, DIM), -3.0, dtype=torch.bfloat16, device="cuda")
    late_mod.pack_tokens(_bf16(hidden), lengths, offsets, out)
    torch.cuda.synchronize()
    got = _bits(out)
    untouched = _bits(torch.full((1, DIM), -3.0, dtype=torch.bfloat16, device="cuda"))[0]
    for b in range(B):
        assert np.array_equal(got[offsets[b]: offsets[b] + lengths[b]], want[lims[b]: lims[b + 1]]), f"text {b}"
    assert (got[:spare] == untouched).all() and (got[spare + int(lims[-1]):] == untouched).all(), "padding was written"


def test_pack_refuses_bad_shapes_and_skips_rows_outside_the_store(gpu, native_lib):
    _, hidden, lengths = lc.pack_cases()[4]
    h = _bf16(hidden)
    out = torch.full((4, DIM), -3.0, dtype=torch.bfloat16, device="cuda")
    ln = torch.from_numpy(lengths).cuda()
    off = torch.tensor([2, -40, 1000], dtype=torch.int64, device="cuda")[: hidden.shape[0]].contiguous()
    assert native_lib.sskd_late_pack_tokens(h.data_ptr(), ln.data_ptr(), off.data_ptr(), hidden.shape[0], 0, 4, out.data_ptr(), stream()) == 1
    assert native_lib.sskd_late_pack_tokens(None, ln.data_ptr(), off.data_ptr(), hidden.shape[0], hidden.shape[1], 4, out.data_ptr(), stream()) == 1
    # offsets outside [0, n_tokens) write nothing; the one inside writes only rows below n_tokens
    _native.check(native_lib.sskd_late_pack_tokens(h.data_ptr(), ln.data_ptr(), off.data_ptr(), hidden.shape[0], hidden.shape[1],
                                                   4, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert (out[:2].float() == -3.0).all()


# ------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("shape", lc.SWEEP, ids=lambda s: f"nq{s[0]}-R{s[2]}")
def test_scores_lie_within_the_band_and_rank_in_order(world, shape):
    nq, tqs, R = shape
    rng = np.random.default_rng(100 + R)
    q_bits, q_lims = lc.queries(rng, tqs)
    # the long rows (every Td of the sweep) and the row without tokens come first, so every list mixes them
    must = np.concatenate([world.big[:12], [7]])     # (cut to R by the generator: R = 1 scores one long row)
    cand = lc.candidates(rng, nq, R, world.n, must=must)
    ref = lc.Reference(q_bits, q_lims, world.tok, world.lims)
    raws = []
    for k in sorted({1, min(10, R), R}):
        D, I, raw = _rerank(world.late, q_bits, q_lims, cand, k)
        lc.check_ranking(D, I, raw, cand, k)
        assert not (I == 7).any(), "a row without tokens was returned"
        raws.append(raw)
    assert all(np.array_equal(r.view(np.uint32), raws[0].view(np.uint32)) for r in raws), "raw scores depend on k"
    _assert_in_band(raws[0], ref, cand)


def test_best_token_in_the_last_partial_tile(gpu):
    q_bits, q_lims, tok, lims, cand = lc.last_tile_family()
    ref = lc.Reference(q_bits, q_lims, tok, lims)
    D, I, raw = _rerank(_late(tok, lims, gpu), q_bits, q_lims, cand, cand.shape[1])
    _assert_in_band(raw, ref, cand)
    lc.check_ranking(D, I, raw, cand, cand.shape[1])


def test_masked_rows_and_columns_are_not_scored(gpu):
    q_bits, q_lims, tok, lims, cand = lc.negative_family()
    ref = lc.Reference(q_bits, q_lims, tok, lims)
    D, I, raw = _rerank(_late(tok, lims, gpu), q_bits, q_lims, cand, 3)
    assert (raw < -0.5).all(), "a zero-scored padding row or column lifted a score"
    _assert_in_band(raw, ref, cand)
    lc.check_ranking(D, I, raw, cand, 3)


def test_exact_ranking_on_the_separated_family(gpu):
    q_bits, q_lims, tok, lims, cand, m = lc.separated_family()
    ref = lc.Reference(q_bits, q_lims, tok, lims)
    R = cand.shape[1]
    D, I, raw = _rerank(_late(tok, lims, gpu), q_bits, q_lims, cand, R)
    _assert_in_band(raw, ref, cand)
    assert np.array_equal(I[0], np.argsort(-ref.s64[0], kind="stable"))
    D10, I10, _ = _rerank(_late(tok, lims, gpu), q_bits, q_lims, cand, 10)
    assert np.array_equal(I10[0], I[0, :10]) and np.array_equal(D10.view(np.uint32), D[:, :10].view(np.uint32))


def test_fewer_valid_candidates_than_k_pads(world):
    rng = np.random.default_rng(41)
    q_bits, q_lims = lc.queries(rng, [5, 32])
    cand = np.full((2, 12), -1, dtype=np.int64)
    cand[0, [3, 8]] = [world.big[0], 7]                 # one real candidate and the row without tokens
    cand[1, :4] = [world.n + 5, world.big[1], 2, -9]     # an id outside the store, two real ones, a negative id
    D, I, raw = _rerank(world.late, q_bits, q_lims, cand, 10)
    lc.check_ranking(D, I, raw, cand, 10)
    assert (I[0] >= 0).sum() == 1 and I[0, 0] == world.big[0]
    assert sorted(I[1, :2].tolist()) == sorted([int(world.big[1]), 2]) and (I[1, 2:] == -1).all()
    ref = lc.Reference(q_bits, q_lims, world.tok, world.lims)
    _assert_in_band(raw, ref, cand)


def test_score_bits_depend_on_the_pair_alone(world):
    """A fixed (q, c): alone, in a batch of 67, first and last of a list of 200, two values of k, a repeated call."""
    rng = np.random.default_rng(43)
    q_bits, q_lims = lc.queries(rng, [(33, 5, 32, 1)[i % 4] for i in range(67)])
    bits = set()
    for qi, row in ((0, int(world.big[3])), (1, int(world.big[5])), (66, 3)):
        one_q = q_bits[q_lims[qi]: q_lims[qi + 1]]
        one_lims = np.array([0, one_q.shape[0]], np.int64)
        seen = []
        # nq = 1, R = 1 (twice), then nq = 67 with the pair first / last of R = 200 under two k
        for _ in range(2):
            seen.append(_rerank(world.late, one_q, one_lims, np.array([[row]], np.int64), 1)[2][0, 0])
        for pos, k in ((0, 1), (199, 10)):
            cand = lc.candidates(rng, 67, 200, world.n)
            cand[cand == row] = -1
            cand[qi, pos] = row
            seen.append(_rerank(world.late, q_bits, q_lims, cand, k)[2][qi, pos])
        words = {np.float32(s).view(np.uint32).item() for s in seen}
        assert len(words) == 1, f"pair ({qi}, {row}): {len(words)} different score bit patterns {seen}"
        bits |= words
    assert len(bits) == 3


def test_id_offset_is_subtracted(gpu):
    q_bits, q_lims, tok, lims, cand = lc.last_tile_family()
    base = _rerank(_late(tok, lims, gpu), q_bits, q_lims, cand, 4)
    off = 1000
    D, I, raw = _rerank(_late(tok, lims, gpu, id_offset=off), q_bits, q_lims, cand + off, 4)
    assert np.array_equal(raw.view(np.uint32), base[2].view(np.uint32))
    assert np.array_equal(I, base[1] + off) and np.array_equal(D.view(np.uint32), base[0].view(np.uint32))
    # ids below the offset are no candidates
    _, I_low, raw_low = _rerank(_late(tok, lims, gpu, id_offset=off), q_bits, q_lims, cand, 4)
    assert np.isneginf(raw_low).all() and (I_low == -1).all()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_search_is_first_stage_then_rerank(world):
    rng = np.random.default_rng(47)
    late, flat = world.late, world.late.flat
    nq = 5
    q_bits, q_lims = lc.queries(rng, [5, 32, 33, 1, 17])
    q_emb = rng.standard_normal((nq, DIM)).astype(np.float32)
    q_emb /= np.linalg.norm(q_emb, axis=1, keepdims=True)
    qd = torch.from_numpy(q_emb).cuda()
    graph = GraphIndex(flat=flat, M=8, ef=64)
    graph.build_graph()
    allow = np.ones(world.n, dtype=bool)
    allow[::3] = False
    first_ids = flat.search_device(qd, 50)[1].cpu().numpy()
    removed = int(first_ids[0, 0])
    assert flat.remove_ids([removed]) == 1
    try:
        for stage, kw in ((None, {}), (None, {"allow": allow}), (graph, {"ef": 64, "allow": allow})):
            D, I = late.search(q_emb, q_bits, q_lims, k=10, candidates=50, first_stage=stage, **kw)
            first = (flat if stage is None else stage).search_device(qd, k=50, **kw)[1]
            D2, I2 = late.rerank_device(q_bits, q_lims, first, 10)
            assert np.array_equal(I, I2.cpu().numpy()) and np.array_equal(D.view(np.uint32), D2.cpu().numpy().view(np.uint32))
            assert not (I == removed).any(), "a removed row was returned"
            if "allow" in kw:
                assert allow[I[I >= 0]].all(), "a row outside the allow mask was returned"
            assert (I[:, 0] >= 0).all()
        with pytest.raises(ValueError):
            late.search(q_emb, q_bits, q_lims, k=10, candidates=5)
    finally:
        world.late = _late(world.tok, world.lims, flat.device)   # later tests get an index without tombstones


def test_search_over_the_hybrid_first_stage(world):
    from semantic_search_kd_amd import BM25Index, HybridIndex

    rng = np.random.default_rng(49)
    late, flat = world.late, world.late.flat
    texts = [f"w{r % 37} w{r % 11} w{r % 5} common" for r in range(world.n)]
    bm25 = BM25Index(device=str(flat.device))
    bm25.build_from_texts([f"doc_{r}" for r in range(world.n)], texts)
    hybrid = HybridIndex(flat, bm25, depth=50)
    q_bits, q_lims = lc.queries(rng, [5, 32])
    q_emb = rng.standard_normal((2, DIM)).astype(np.float32)
    q_emb /= np.linalg.norm(q_emb, axis=1, keepdims=True)
    q_texts = ["w3 w4 common", "w30 w7"]
    D, I = late.search(q_emb, q_bits, q_lims, k=10, candidates=60, first_stage=hybrid, query_texts=q_texts, depth=50)
    first = hybrid.search_device(q_texts, torch.from_numpy(q_emb).cuda(), k=60, depth=50)[1]
    D2, I2 = late.rerank_device(q_bits, q_lims, first, 10)
    assert np.array_equal(I, I2.cpu().numpy()) and np.array_equal(D.view(np.uint32), D2.cpu().numpy().view(np.uint32))
    assert (I[:, 0] >= 0).all()


def test_compact_keeps_the_survivors_scores(gpu):
    rng = np.random.default_rng(53)
    tok, lims = lc.sweep_store(seed=9, n_rows=120)
    late = _late(tok, lims, gpu)
    q_bits, q_lims = lc.queries(rng, [5, 33])
    cand = np.tile(np.arange(120, dtype=np.int64), (2, 1))
    before = _rerank(late, q_bits, q_lims, cand, 10)[2]
    gone = [0, 7, 24, 25, 119]
    assert late.flat.remove_ids(gone) == len(gone)
    kept = late.flat.compact()
    late.compact(kept)
    assert late.ntotal == late.flat.ntotal == 120 - len(gone)
    after = _rerank(late, q_bits, q_lims, np.tile(np.arange(kept.size, dtype=np.int64), (2, 1)), 10)[2]
    assert np.array_equal(after.view(np.uint32), before[:, kept].view(np.uint32))


def test_add_tokens_appends_and_a_short_store_is_refused(gpu):
    tok, lims = lc.sweep_store(seed=9, n_rows=60)
    flat = _flat(40, gpu)
    late = LateInteractionIndex(flat)
    late.set_tokens(tok[: lims[40]], lims[:41])
    rng = np.random.default_rng(3)
    extra = rng.standard_normal((20, DIM)).astype(np.float32)
    flat.add(extra / np.linalg.norm(extra, axis=1, keepdims=True))
    q_bits, q_lims = lc.queries(rng, [5])
    cand = torch.arange(60, dtype=torch.int64, device="cuda")[None, :]
    with pytest.raises(RuntimeError, match="token store covers 40 rows"):
        late.rerank_device(q_bits, q_lims, cand, 5)
    late.add_tokens(tok[lims[40]:], lims[40:] - lims[40])
    whole = _late(tok, lims, gpu)
    a = _rerank(late, q_bits, q_lims, cand.cpu().numpy(), 5)
    b = _rerank(whole, q_bits, q_lims, cand.cpu().numpy(), 5)
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def test_save_load_returns_the_same_bits(gpu, tmp_path):
    rng = np.random.default_rng(59)
    tok, lims = lc.sweep_store(seed=9, n_rows=120)
    late = _late(tok, lims, gpu)
    q_bits, q_lims = lc.queries(rng, [32, 7])
    cand = lc.candidates(rng, 2, 64, 120)
    before = _rerank(late, q_bits, q_lims, cand, 10)
    late.save(tmp_path)
    assert late_mod.is_late_dir(tmp_path)
    again = LateInteractionIndex(late.flat)
    again.load(tmp_path)
    assert np.array_equal(again.tokens_numpy(), tok) and np.array_equal(again.lims, lims)
    after = _rerank(again, q_bits, q_lims, cand, 10)
    assert np.array_equal(after[1], before[1])
    assert np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32))
    assert np.array_equal(after[2].view(np.uint32), before[2].view(np.uint32))
    with pytest.raises(ValueError, match="rows"):
        LateInteractionIndex(_flat(119, gpu)).load(tmp_path)


def test_graph_capture_and_replay_equals_eager(world):
    rng = np.random.default_rng(61)
    q_bits, q_lims = lc.queries(rng, [5, 32, 33])
    cand = torch.from_numpy(lc.candidates(rng, 3, 65, world.n, must=world.big[:6])).cuda()
    queries = world.late.prepare_queries(q_bits, q_lims)
    eager_D, eager_I = world.late.rerank_device(queries, None, cand, 10)     # also sizes the workspace before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            D, I = world.late.rerank_device(queries, None, cand, 10)
    torch.cuda.current_stream().wait_stream(side)
    D.fill_(0)
    I.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(I, eager_I) and torch.equal(D.view(torch.int32), eager_D.view(torch.int32))


def test_invalid_arguments_are_refused_before_anything_is_enqueued(world, native_lib):
    lib, late = native_lib, world.late
    rng = np.random.default_rng(67)
    R, k, nq = 8, 4, 2
    q_bits, _ = lc.queries(rng, [130, 5])
    qt = _bf16(q_bits)
    cand = torch.from_numpy(lc.candidates(rng, nq, R, world.n)).cuda()
    big_cand = torch.zeros((nq, 1025), dtype=torch.int64, device="cuda")

    def call(lims, R_=R, k_=k, cand_=cand):
        host = np.asarray(lims, np.int64)
        dev = torch.from_numpy(host).cuda()
        outs = [torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda") for n in (nq * 1025 * 4, nq * 1025 * 8, nq * 1025 * 4)]
        ws = torch.full((nq * 1025 * 4 + 256,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = lib.sskd_late_rerank(qt.data_ptr(), host.ctypes.data, dev.data_ptr(), nq, late.tokens.data_ptr(),
                                  late._lims_dev.data_ptr(), late.ntotal, late.n_tokens, cand_.data_ptr(), R_, k_, 0,
                                  outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr(), ws.numel(), stream())
        torch.cuda.synchronize()
        return rc, all(bool((b == SENTINEL).all()) for b in outs + [ws])

    for what, args in (("Tq = 0", dict(lims=[0, 5, 5])), ("Tq > 128", dict(lims=[0, 129, 134])),
                       ("lims not ascending", dict(lims=[0, 8, 3])), ("negative start", dict(lims=[-1, 4, 9])),
                       ("R > 1024", dict(lims=[0, 5, 10], R_=1025, cand_=big_cand)),
                       ("k > R", dict(lims=[0, 5, 10], k_=R + 1)), ("k = 0", dict(lims=[0, 5, 10], k_=0))):
        rc, intact = call(**args)
        assert rc == 1, what
        assert intact, f"{what}: something was written"
    rc, intact = call([0, 5, 10])
    assert rc == 0 and not intact
    # the Python layer refuses the same before it reaches the library
    with pytest.raises((ValueError, _native.NativeError)):
        late.rerank_device(q_bits[:10], [0, 8, 3], cand, k)
    with pytest.raises(_native.NativeError):
        late.rerank_device(q_bits[:134], [0, 129, 134], cand, k)
    with pytest.raises(_native.NativeError):
        late.rerank_device(q_bits[:10], [0, 5, 10], cand, R + 1)
