"""Candidate generation from the compressed store on the MI355X: the centroid scores inside their band and independent
of their batch-mates, ``sskd_plaid_candidates`` against the NumPy restatement on the device's own S and on hand-made S
(ids exactly, ``cand_A`` by bits, ``n_cand`` exactly), the anchor (every centroid probed: ``search_tokens`` is the re-rank
of all rows, bit for bit) and the recall gate on the clustered family.

The band test prints ``max |S - s64| / band`` (DESIGN section 23 records it)."""
import numpy as np
import pytest
import torch

import late_cases as lc
import late_codec_cases as cc
import plaid_cases as pc
from capi_helpers import stream
from semantic_search_kd_amd import FAISSIndexBuilder, LateInteractionIndex

pytestmark = pytest.mark.gpu

DIM = lc.DIM
GUARD = 64


def _dev(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def _flat(n_rows: int, gpu, id_offset: int = 0) -> FAISSIndexBuilder:
    rows = np.random.default_rng(5).standard_normal((n_rows, DIM)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device=str(gpu), id_offset=id_offset)
    flat.build_from_embeddings(rows)
    return flat


class World:
    """A token store compressed by the RESTATEMENT, its lists built by the RESTATEMENT, held by a ``LateInteractionIndex``
    (so the C-ABI tests stand without the compress kernel and without ``build_centroid_lists``)."""

    def __init__(self, gpu, tok, lims, codec, nbits=2, id_offset=0, cid_override=None):
        self.cen, self.cut, self.w = codec
        self.C, self.lims, self.n = self.cen.shape[0], lims, lims.size - 1
        self.cid, self.scale, self.codes, _ = cc.compress_rows(tok, cc.assign_rows(tok, self.cen), *codec, nbits)
        if cid_override is not None:
            self.cid = cid_override(self.cid)
        self.list_lims, self.list_rows = pc.build_lists_ref(self.cid, lims, self.C)
        self.late = LateInteractionIndex(_flat(self.n, gpu, id_offset))
        self.late.set_codec(*codec)
        self.late.set_compressed(self.cid, self.scale, self.codes, lims)
        self.late.list_lims, self.late.list_rows = _dev(self.list_lims), _dev(self.list_rows)
        self.id_offset = id_offset

    def ref(self, S, q_lims, nprobe, R, allowed=None):
        return pc.candidates_ref(S, q_lims, self.cid, self.lims, self.list_lims, self.list_rows, self.C, nprobe, R, allowed,
                                 self.id_offset)


def _codec(n_centroids, nbits=2, seed=31):
    return cc.random_codec(np.random.default_rng(seed + n_centroids + nbits), n_centroids, nbits)


_worlds = {}


def _world(gpu, C_):
    if C_ not in _worlds:
        tok, lims = lc.sweep_store()
        _worlds[C_] = World(gpu, tok, lims, _codec(C_))
    return _worlds[C_]


def centroid_scores(lib, cen_bits, q_bits, ld=None):
    """The kernel's S as NumPy fp32 ``[C, ld]``; the columns past the tokens keep a sentinel."""
    C_, T = cen_bits.shape[0], q_bits.shape[0]
    ld = T if ld is None else ld
    S = torch.full((C_ * ld + 2 * GUARD,), -12345.0, dtype=torch.float32, device="cuda")
    q, cen = _dev(q_bits), _dev(cen_bits)
    rc = lib.sskd_plaid_centroid_scores(q.data_ptr(), T, cen.data_ptr(), C_, S.data_ptr() + 4 * GUARD, ld, stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.sskd_last_error()
    host = S.cpu().numpy()
    assert (host[:GUARD] == -12345.0).all() and (host[GUARD + C_ * ld:] == -12345.0).all(), "S was written outside [C, ld]"
    return host[GUARD: GUARD + C_ * ld].reshape(C_, ld)


class _Lent:
    """a caller's ``(pointer, bytes)`` workspace behind the two tensor methods ``candidates`` uses"""

    def __init__(self, ptr, nbytes):
        self._ptr, self._n = int(ptr), int(nbytes)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n


def candidates(lib, world, S, q_lims, nprobe, R, mask_words=None, ws_bytes=None, expect=0, ws=None, **override):
    """``sskd_plaid_candidates`` on host ``S`` with guarded outputs: ``(rc, cand_I, cand_A, n_cand, intact)`` - ``intact``
    says that nothing but the outputs proper was written (and with ``expect != 0``: nothing at all).  ``ws``: the caller's
    ``(pointer, bytes)`` workspace instead of a fresh buffer."""
    late = world.late
    q_lims = np.ascontiguousarray(q_lims, np.int64)
    nq = q_lims.size - 1
    S_dev, lims_dev = _dev(np.ascontiguousarray(S, np.float32)), _dev(q_lims)
    need = int(lib.sskd_plaid_candidates_workspace_bytes(max(nq, 1), world.n, min(max(nprobe, 1), 32)))
    if ws is not None:
        ws = _Lent(*ws)
    else:
        ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 256), dtype=torch.uint8, device="cuda")
    cells = max(nq, 1) * max(min(R, 1024), 1)
    I = torch.full((cells + 2 * GUARD,), -777, dtype=torch.int64, device="cuda")
    A = torch.full((cells + 2 * GUARD,), -555.0, dtype=torch.float32, device="cuda")
    N = torch.full((max(nq, 1) + 2 * GUARD,), -333, dtype=torch.int32, device="cuda")
    mask = None if mask_words is None else _dev(mask_words)
    args = dict(ld=S.shape[1], nq=nq, C=world.C, n_rows=world.n, n_tokens=late.n_tokens, n_list=int(world.list_rows.size),
                nprobe=nprobe, R=R, id_offset=world.id_offset, ws_bytes=ws.numel() if ws_bytes is None else ws_bytes)
    args.update(override)
    rc = lib.sskd_plaid_candidates(
        S_dev.data_ptr(), args["ld"], q_lims.ctypes.data, lims_dev.data_ptr(), args["nq"], args["C"], late.cid.data_ptr(),
        late._lims_dev.data_ptr(), args["n_rows"], args["n_tokens"], late.list_lims.data_ptr(), late.list_rows.data_ptr(),
        args["n_list"], None if mask is None else mask.data_ptr(), args["nprobe"], args["R"], args["id_offset"],
        I.data_ptr() + 8 * GUARD, A.data_ptr() + 4 * GUARD, N.data_ptr() + 4 * GUARD, ws.data_ptr(), args["ws_bytes"], stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, lib.sskd_last_error())
    Ih, Ah, Nh = I.cpu().numpy(), A.cpu().numpy(), N.cpu().numpy()
    body = slice(GUARD, GUARD + cells)
    intact = all(((x[:GUARD] == s).all() and (x[GUARD + m:] == s).all())
                 for x, s, m in ((Ih, -777, cells), (Ah, -555.0, cells), (Nh, -333, max(nq, 1))))
    if expect != 0:
        intact = intact and (Ih[body] == -777).all() and (Ah[body] == -555.0).all() and (Nh[GUARD: GUARD + max(nq, 1)] == -333).all()
        return rc, None, None, None, bool(intact)
    return rc, Ih[body].reshape(nq, -1), Ah[body].reshape(nq, -1), Nh[GUARD: GUARD + nq], bool(intact)


def assert_matches(got, want, what=""):
    _, I, A, N, intact = got
    assert intact, f"{what}: written outside the outputs"
    assert np.array_equal(N, want[2]), f"{what}: n_cand {N.tolist()} != {want[2].tolist()}"
    assert np.array_equal(I, want[0]), f"{what}: candidate ids differ"
    assert np.array_equal(A.view(np.uint32), want[1].view(np.uint32)), f"{what}: cand_A differs in bits"


# ------------------------------------------------------------------------------------------------ S
BATCHES = {1: [[1], [5], [32], [33], [128]], 3: [[5, 32, 33], [128, 1, 33]], 67: [[(1, 5, 32, 33, 128)[i % 5] for i in range(67)]]}


@pytest.mark.parametrize("nq", [1, 3, 67])
@pytest.mark.parametrize("n_centroids", [1, 3, 300])
def test_centroid_scores_lie_within_the_band(gpu, native_lib, n_centroids, nq):
    rng = np.random.default_rng(300 + n_centroids + nq)
    cen = _codec(n_centroids)[0]
    worst = 0.0
    for tqs in BATCHES[nq]:
        q_bits, _ = lc.queries(rng, tqs)
        q_bits[0] = lc.bf16_bits(lc.bf16_values(q_bits[0]) * np.float32(3.0))      # a token that is not a unit vector
        T = q_bits.shape[0]
        S = centroid_scores(native_lib, cen, q_bits, ld=T + (7 if nq == 3 else 0))
        assert (S[:, T:] == -12345.0).all(), "columns past the tokens were written"
        err = np.abs(S[:, :T].astype(np.float64) - pc.centroid_scores64(cen, q_bits))
        band = pc.band_S(cen, q_bits)
        worst = max(worst, float((err / band).max()))
        assert (err <= band).all(), f"Tq={tqs}: max |S - s64| / band = {(err / band).max():.4f}"
    print(f"C={n_centroids} nq={nq}: max |S - s64| / band = {worst:.4f}")


def test_a_score_does_not_depend_on_its_batch_mates(gpu, native_lib):
    rng = np.random.default_rng(47)
    cen = _codec(300)[0]
    q_bits, q_lims = lc.queries(rng, [(33, 5, 32, 1, 128)[i % 5] for i in range(67)])
    whole = centroid_scores(native_lib, cen, q_bits)
    for q in (0, 1, 4, 66):
        alone = centroid_scores(native_lib, cen, q_bits[q_lims[q]: q_lims[q + 1]])
        assert np.array_equal(alone.view(np.uint32), whole[:, q_lims[q]: q_lims[q + 1]].view(np.uint32)), f"query {q}"
    # and not on the centroids around it: the first 3 centroids alone
    few = centroid_scores(native_lib, cen[:3], q_bits[:40])
    assert np.array_equal(few.view(np.uint32), whole[:3, :40].view(np.uint32))


# ------------------------------------------------------------------------------------------------ candidates on the device's S
_scores = {}
MIXED = [1, 5, 32, 33, 128, 64, 2]


def _sweep_scores(lib, world, key, tqs, seed):
    if (world.C, key) not in _scores:
        q_bits, q_lims = lc.queries(np.random.default_rng(seed), tqs)
        _scores[(world.C, key)] = (centroid_scores(lib, world.cen, q_bits), q_lims)
    return _scores[(world.C, key)]


@pytest.mark.parametrize("R", [1, 7, 64, 1024])
@pytest.mark.parametrize("nprobe", [1, 2, 4, 32])
@pytest.mark.parametrize("n_centroids", [3, 300])
def test_candidates_equal_the_restatement_on_the_devices_own_scores(gpu, native_lib, n_centroids, nprobe, R):
    world = _world(gpu, n_centroids)
    nprobe = min(nprobe, n_centroids)
    S, q_lims = _sweep_scores(native_lib, world, "mixed", MIXED, 500)
    want = world.ref(S, q_lims, nprobe, R)
    assert_matches(candidates(native_lib, world, S, q_lims, nprobe, R), want, f"C={n_centroids} nprobe={nprobe} R={R}")
    if R == 1024 and n_centroids == 300:
        assert (want[2] > 64).any() and (want[2] < 1024).any(), "the case must cut some queries and pad others"


def test_candidates_for_a_batch_of_67_queries_and_one_centroid(gpu, native_lib):
    world = _world(gpu, 300)
    S, q_lims = _sweep_scores(native_lib, world, "67", [(1, 5, 32, 33)[i % 4] for i in range(67)], 501)
    assert_matches(candidates(native_lib, world, S, q_lims, 2, 64), world.ref(S, q_lims, 2, 64), "nq=67")
    one = _world(gpu, 1)
    S, q_lims = _sweep_scores(native_lib, one, "one", [5, 33], 502)
    want = one.ref(S, q_lims, 1, 1024)
    assert (want[2] == one.n - 1).all(), "one centroid lists every row that has tokens"
    assert_matches(candidates(native_lib, one, S, q_lims, 1, 1024), want, "C=1")


@pytest.mark.parametrize("nprobe,R", [(1, 7), (4, 64), (32, 1024)])
def test_candidates_do_not_depend_on_the_alignment_of_the_scores(gpu, native_lib, nprobe, R):
    """The same scores at a leading dimension that is a multiple of 4 and at one that is not, queries that begin on and
    off multiples of 4 columns, blocks that end inside a run of 4 columns: always the restatement's bits."""
    world = _world(gpu, 300)
    tqs = [32, 4, 128, 36, 8, 64, 5, 3, 33, 7]                  # begins 0 .. 272 aligned, then 277, 280 (aligned), 313
    q_bits, q_lims = lc.queries(np.random.default_rng(503), tqs)
    T = int(q_lims[-1])
    assert T == 320 and [int(b) % 4 for b in q_lims[:-1]] == [0, 0, 0, 0, 0, 0, 0, 1, 0, 1]
    S = centroid_scores(native_lib, world.cen, q_bits, ld=T + 4)
    want = world.ref(S, q_lims, nprobe, R)
    assert_matches(candidates(native_lib, world, S, q_lims, nprobe, R), want, "ld % 4 == 0")
    # the same scores at a leading dimension that is no multiple of 4
    odd = np.full((300, T + 1), -12345.0, np.float32)
    odd[:, :T] = S[:, :T]
    assert_matches(candidates(native_lib, world, odd, q_lims, nprobe, R), want, "ld % 4 == 1")
    # hand-made scores with ties, on the store of tripled documents
    tripled = _tripled_world(gpu)
    lims2 = np.array([0, 4, 12, 44, 47], np.int64)
    S2 = (np.random.default_rng(504).integers(-2, 3, (8, 48)) / 4).astype(np.float32)
    S2[5] = S2[2]
    S2[[1, 6], 9] = np.nan
    S2[:, 45] = -np.inf
    np_, R_ = min(nprobe, 8), R
    assert_matches(candidates(native_lib, tripled, S2, lims2, np_, R_), tripled.ref(S2, lims2, np_, R_), "hand-made, aligned")


def test_a_workspace_of_one_query_runs_the_batch_in_chunks(gpu, native_lib):
    world = _world(gpu, 300)
    S, q_lims = _sweep_scores(native_lib, world, "mixed", MIXED, 500)
    one = int(native_lib.sskd_plaid_candidates_workspace_bytes(1, world.n, 4))
    want = world.ref(S, q_lims, 4, 64)
    for ws_bytes in (one, 2 * one + 1000):
        assert_matches(candidates(native_lib, world, S, q_lims, 4, 64, ws_bytes=ws_bytes), want, f"workspace {ws_bytes}")
    rc, *_, intact = candidates(native_lib, world, S, q_lims, 4, 64, ws_bytes=one - 1, expect=2)
    assert intact, "a short workspace: something was written"


# ------------------------------------------------------------------------------------------------ hand-made S
def _tripled_world(gpu):
    """40 documents stored three times each (rows r, r + 40, r + 80 hold the same tokens), 8 centroids, centroid ids
    drawn so that documents share centroid sets."""
    if "tripled" not in _worlds:
        rng = np.random.default_rng(61)
        td = rng.integers(1, 9, 40)
        td[3], td[17] = 1, 70                               # a one-token document and one longer than 64 tokens
        one_lims = np.concatenate([[0], np.cumsum(td)])
        cid_one = rng.integers(0, 8, int(one_lims[-1])).astype(np.int32)
        cid_one[one_lims[17]: one_lims[18]] = rng.integers(0, 3, 70)
        lims = np.concatenate([[0], np.cumsum(np.tile(td, 3))]).astype(np.int64)
        tok = lc.unit_token_bits(rng, int(lims[-1]))
        _worlds["tripled"] = World(gpu, tok, lims, _codec(8), cid_override=lambda _: np.tile(cid_one, 3))
    return _worlds["tripled"]


def test_exact_ties_across_centroids_and_documents_fall_to_the_lower_row(gpu, native_lib):
    world = _tripled_world(gpu)
    rng = np.random.default_rng(62)
    q_lims = np.array([0, 4, 9, 41], np.int64)
    S = (rng.integers(-2, 3, (8, 41)) / 4).astype(np.float32)       # few distinct values: ties across centroids
    S[5] = S[2]                                                      # two centroids that tie for every token
    for nprobe, R in ((1, 120), (2, 7), (8, 64), (8, 1024)):
        want = world.ref(S, q_lims, nprobe, R)
        assert_matches(candidates(native_lib, world, S, q_lims, nprobe, R), want, f"nprobe={nprobe} R={R}")
    # the three copies of a document tie exactly and come out in row order
    I, A, _ = world.ref(S, q_lims, 8, 1024)
    assert (I[0, :120] >= 0).all()
    for q in range(3):
        for p in range(0, 120, 1):
            same = np.flatnonzero((A[q, :120] == A[q, p]))
            assert np.array_equal(I[q, same], np.sort(I[q, same]))
    assert len(set(A[0, :120].tolist())) <= 40


def test_minus_infinity_columns_nan_entries_and_short_candidate_lists(gpu, native_lib):
    world = _tripled_world(gpu)
    rng = np.random.default_rng(63)
    q_lims = np.array([0, 3, 8, 10, 13], np.int64)
    S = rng.standard_normal((8, 13)).astype(np.float32)
    S[:, 1] = -np.inf                                               # query 0: a token nothing matches - every approx is -inf
    S[[0, 3, 6], 4] = np.nan                                        # query 1: NaN entries (never probed, ignored by the max)
    S[:, 6] = np.nan                                                #          and a token that is NaN everywhere
    S[:, 8] = -np.inf
    S[4, 8] = 1.0                                                   # query 2: its first token matches centroid 4 alone
    S[2, 11] = np.inf                                               # query 3: +inf is a score like any other
    for nprobe, R in ((1, 16), (2, 200), (8, 1024)):
        want = world.ref(S, q_lims, nprobe, R)
        got = candidates(native_lib, world, S, q_lims, nprobe, R)
        assert_matches(got, want, f"nprobe={nprobe} R={R}")
        assert want[2][0] > 0 and (want[0][0] == -1).all(), "query 0 has candidates and every one is dropped"
        assert (want[0][1] == -1).all(), "a token that is NaN everywhere leaves every approx at -inf"
    want = world.ref(S, q_lims, 1, 1024)
    # query 2: only the documents that own a token of centroid 4 survive, fewer than there are candidates and than R
    assert 0 < (want[0][2] >= 0).sum() < want[2][2] <= 120
    assert np.isposinf(want[1][3, 0])


# ------------------------------------------------------------------------------------------------ stores and filters
def test_corrupt_centroid_ids_are_clamped_not_followed(gpu, native_lib):
    tok, lims = lc.sweep_store(seed=9, n_rows=90)

    def corrupt(cid):
        bad = cid.copy()
        bad[::3] = np.array([-1, 300, 2 ** 31 - 1, -2 ** 31, 5], np.int32)[np.arange(bad[::3].size) % 5]
        return bad

    world = World(gpu, tok, lims, _codec(5), cid_override=corrupt)
    assert (world.cid < 0).any() and (world.cid >= 5).any()
    q_bits, q_lims = lc.queries(np.random.default_rng(71), [5, 33])
    S = centroid_scores(native_lib, world.cen, q_bits)
    for nprobe in (1, 5):
        assert_matches(candidates(native_lib, world, S, q_lims, nprobe, 128), world.ref(S, q_lims, nprobe, 128), f"nprobe={nprobe}")


def test_allow_mask_all_clear_mask_and_id_offset(gpu, native_lib):
    world = _world(gpu, 300)
    S, q_lims = _sweep_scores(native_lib, world, "mixed", MIXED, 500)
    rng = np.random.default_rng(72)
    allowed = rng.random(world.n) < 0.4
    want = world.ref(S, q_lims, 4, 64, allowed)
    assert_matches(candidates(native_lib, world, S, q_lims, 4, 64, mask_words=pc.mask_words(allowed)), want, "allow-mask")
    assert not np.isin(want[0][want[0] >= 0], np.flatnonzero(~allowed)).any()
    # the bits past n_rows are ignored
    words = pc.mask_words(allowed).copy()
    words[-1] |= np.uint32(0xFFFFFFFF) << np.uint32(world.n % 32)
    assert_matches(candidates(native_lib, world, S, q_lims, 4, 64, mask_words=words), want, "bits past n_rows")
    none = np.zeros(world.n, bool)
    got = candidates(native_lib, world, S, q_lims, 4, 64, mask_words=pc.mask_words(none))
    assert_matches(got, world.ref(S, q_lims, 4, 64, none), "all-clear mask")
    assert (got[1] == -1).all() and np.isneginf(got[2]).all() and (got[3] == 0).all()
    # id_offset
    tok, lims = lc.sweep_store(seed=9, n_rows=90)
    shifted = World(gpu, tok, lims, _codec(5), id_offset=1000)
    q_bits, q_lims2 = lc.queries(np.random.default_rng(73), [5, 33])
    S2 = centroid_scores(native_lib, shifted.cen, q_bits)
    want = shifted.ref(S2, q_lims2, 2, 32)
    assert want[0][want[0] >= 0].min() >= 1000
    assert_matches(candidates(native_lib, shifted, S2, q_lims2, 2, 32), want, "id_offset")


def test_a_removed_row_is_no_candidate(gpu, native_lib):
    tok, lims = lc.sweep_store(seed=9, n_rows=90)
    world = World(gpu, tok, lims, _codec(5))
    q_bits, q_lims = lc.queries(np.random.default_rng(74), [5, 33])
    before = world.late.candidates_device(q_bits, q_lims, nprobe=5, ndocs=128)
    gone = sorted({int(before[0][0, 0]), int(before[0][1, 1]), 24})
    world.late.flat.remove_ids(np.asarray(gone, np.int64))
    cand_I, cand_A, n_cand, S = world.late.candidates_device(q_bits, q_lims, nprobe=5, ndocs=128, return_scores=True)
    torch.cuda.synchronize()
    allowed = np.ones(world.n, bool)
    allowed[gone] = False
    want = world.ref(S.cpu().numpy(), q_lims, 5, 128, allowed)
    assert np.array_equal(cand_I.cpu().numpy(), want[0]) and np.array_equal(n_cand.cpu().numpy(), want[2])
    assert np.array_equal(cand_A.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    assert not np.isin(cand_I.cpu().numpy(), gone).any()
    # and a per-call filter on top of the removal
    allow = np.flatnonzero(np.arange(world.n) % 2 == 0)
    cand_I = world.late.candidates_device(q_bits, q_lims, nprobe=5, ndocs=128, allow=allow)[0].cpu().numpy()
    allowed &= np.arange(world.n) % 2 == 0
    assert np.array_equal(cand_I, world.ref(S.cpu().numpy(), q_lims, 5, 128, allowed)[0])


def test_refusals_leave_the_outputs_untouched(gpu, native_lib):
    world = _world(gpu, 300)
    S, q_lims = _sweep_scores(native_lib, world, "mixed", MIXED, 500)
    T = int(q_lims[-1])
    for what, args in (("C = 0", dict(C=0)), ("C > 65 536", dict(C=65537)), ("nprobe = 0", dict(nprobe=0)), ("nprobe = 33", dict(nprobe=33)),
                       ("R = 0", dict(R=0)), ("R = 1025", dict(R=1025)), ("ld < tokens", dict(ld=T - 1)), ("n_rows < 0", dict(n_rows=-1)),
                       ("n_list < 0", dict(n_list=-1)), ("n_list > n_tokens", dict(n_list=world.late.n_tokens + 1)),
                       ("id_offset < 0", dict(id_offset=-1)), ("nq < 0", dict(nq=-1))):
        rc, *_, intact = candidates(native_lib, world, S, q_lims, args.pop("nprobe", 2), args.pop("R", 16), expect=1, **args)
        assert intact, f"{what}: something was written"
    long_lims = np.array([0, 129], np.int64)
    rc, *_, intact = candidates(native_lib, world, S, long_lims, 2, 16, expect=1)
    assert intact, "Tq = 129: something was written"
    rc, *_, intact = candidates(native_lib, world, S, np.array([0, 5, 5], np.int64), 2, 16, expect=1)
    assert intact, "Tq = 0: something was written"


# ------------------------------------------------------------------------------------------------ anchor and gate
@pytest.mark.parametrize("n_centroids", [1, 3])
def test_with_every_centroid_probed_search_tokens_is_the_rerank_of_all_rows(gpu, n_centroids):
    tok, lims = lc.sweep_store(seed=8, n_rows=1000)
    world = World(gpu, tok, lims, _codec(n_centroids))
    q_bits, q_lims = lc.queries(np.random.default_rng(81), [5, 32, 33, 128, 1])
    D, I, cand_I, cand_A, n_cand = world.late.search_tokens(q_bits, q_lims, k=10, nprobe=n_centroids, ndocs=1024,
                                                            return_candidates=True)
    everything = np.tile(np.arange(1000, dtype=np.int64), (5, 1))
    D_all, I_all = world.late.rerank(q_bits, q_lims, everything, 10)
    assert (n_cand == 999).all(), "every row but the one without tokens is a candidate"
    assert np.array_equal(I, I_all) and np.array_equal(D.view(np.uint32), D_all.view(np.uint32))
    assert (np.sort(cand_I[:, :999], axis=1) == np.delete(np.arange(1000), 7)[None, :]).all() and (cand_I[:, 999:] == -1).all()


def test_recall_gate_on_the_clustered_family(gpu):
    """recall@10 >= 0.97 against the exhaustive compressed MaxSim: the gate ``validate()`` holds the other indexes to.  The
    restatement alone reaches 1.000 on this family on the CPU (``plaid_cases.recall_ref``; 0.991 at ``ndocs = 64``)."""
    fam = pc.clustered_family()
    cid, scale, codes, _ = pc.compress_family(fam)
    late = LateInteractionIndex(_flat(fam["lims"].size - 1, gpu))
    late.set_codec(*fam["codec"])
    late.set_compressed(cid, scale, codes, fam["lims"])
    late.build_centroid_lists()
    recall = late.validate_tokens(fam["q_bits"], fam["q_lims"], k=10, nprobe=2, ndocs=256)
    D, I, cand_I, cand_A, n_cand = late.search_tokens(fam["q_bits"], fam["q_lims"], k=10, nprobe=2, ndocs=256, return_candidates=True)
    print(f"recall@10 = {recall:.4f}, mean n_cand = {n_cand.mean():.1f} of {late.ntotal} rows")
    assert recall >= 0.97
    assert (I[:, 0] == fam["source"]).mean() >= 0.97, "a query drawn from a document finds it first"
