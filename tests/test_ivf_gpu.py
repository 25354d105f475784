"""IVF index on the GPU: which rows are looked at is approximate, every score and every order is exact.

The oracle of a search is ``oracle.topk_of_scores`` over ``oracle.scores_fma`` (the scan's fma order, in C) with every
row outside the probed lists - and every filtered or removed row - set to -inf: the results are compared with
``np.array_equal``, scores by their bits.  With every list probed the oracle is the plain exact search."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import small_kernel_cases as kc
from capi_helpers import stream
from oracle import search as oracle
from semantic_search_kd_amd import FAISSIndexBuilder, IVFIndex, _native, ivf as ivf_mod

pytestmark = pytest.mark.gpu

N, DIM, NLIST = 3001, 384, 16   # 3001 rows: a ragged last tile


def _flat(corpus, gpu):
    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu))
    index.build_from_embeddings(corpus)
    return index


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got, ref, what):
    assert np.array_equal(got[1], ref[1]), f"{what}: ids differ"
    assert np.array_equal(_bits(got[0]), _bits(ref[0])), f"{what}: scores differ"


def _probed_rows(probe_row, offsets, rows, n):
    ok = np.zeros(n, dtype=np.bool_)
    for l in probe_row:
        if l >= 0:
            ok[rows[offsets[l]:offsets[l + 1]]] = True
    return ok


def _ivf_oracle(scores, probe, offsets, rows, k, extra=None):
    s = np.array(scores, dtype=np.float32)
    for i in range(s.shape[0]):
        ok = _probed_rows(probe[i], offsets, rows, s.shape[1])
        if extra is not None:
            ok &= extra
        s[i, ~ok] = -np.inf
    return oracle.topk_of_scores(s, k)


def _probe_host(index, q, nprobe):
    return index.probe_device(torch.from_numpy(np.ascontiguousarray(q)).to(index.device), nprobe).cpu().numpy()


@pytest.fixture(scope="module")
def world(gpu):
    corpus = oracle.seeded_unit_rows(N, DIM, 1)
    queries = oracle.seeded_unit_rows(200, DIM, 2)
    centroids = oracle.seeded_unit_rows(NLIST, DIM, 4)
    assignment = np.random.default_rng(3).integers(0, NLIST, size=N)
    flat = _flat(corpus, gpu)
    index = IVFIndex.from_assignment(flat, centroids, assignment)
    offsets, rows = ivf_mod.csr_from_assignment(assignment, NLIST)
    return SimpleNamespace(corpus=corpus, queries=queries, centroids=centroids, assignment=assignment, flat=flat,
                           index=index, offsets=offsets, rows=rows, scores=oracle.scores_fma(queries, corpus))


# ------------------------------------------------------------------------------------------- the bit contract
@pytest.mark.parametrize("k", [1, 10, 100, 256])
@pytest.mark.parametrize("nq", [1, 65, 200])
def test_full_probe_equals_the_exact_search(world, nq, k):
    q = world.queries[:nq]
    got = world.index.search(q, k, nprobe=NLIST)
    assert world.index.last_search_path == "ivf"
    _same(got, oracle.topk_of_scores(world.scores[:nq], k), "oracle")
    _same(got, world.flat.search(q, k), "flat.search")


def test_lists_on_the_device_are_the_host_csr(world):
    offsets, rows = world.index.lists_numpy()
    assert np.array_equal(offsets, world.offsets) and np.array_equal(rows, world.rows)
    assert world.index.max_list_rows == int(np.diff(world.offsets).max()) and world.index.nlist == NLIST


@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("nprobe", [1, 4])
def test_partial_probe(world, nprobe, k):
    q = world.queries[:65]
    probe = _probe_host(world.index, q, nprobe)
    # the probed lists are the top-nprobe centroids under the search's rank order
    assert np.array_equal(probe, oracle.topk_of_scores(oracle.scores_fma(q, world.centroids), nprobe)[1])
    got = world.index.search(q, k, nprobe=nprobe)
    _same(got, _ivf_oracle(world.scores[:65], probe, world.offsets, world.rows, k), f"nprobe={nprobe} k={k}")
    held = np.array([_probed_rows(p, world.offsets, world.rows, N).sum() for p in probe])
    if nprobe == 1 and k == 256:
        assert (held < k).all()   # one list of ~190 rows: fewer rows than k
    for i, h in enumerate(held):  # slots beyond the probed rows are (-FLT_MAX, -1)
        assert (got[1][i, min(h, k):] == -1).all() and (got[0][i, min(h, k):] == oracle.NEG_PAD).all()
        assert (got[1][i, :min(h, k)] >= 0).all()


@pytest.mark.parametrize("nq", [1, 64, 65])
@pytest.mark.parametrize("nprobe", [10, 11, 13, 16])
def test_probe_is_the_exact_coarse_search_on_both_routes(world, nq, nprobe):
    """Up to 64 queries probing 11 .. 32 lists take the list scan over the centroids, everything else the flat search
    over them: the same lists in the same order either way, and the same results."""
    q = world.queries[:nq]
    want = oracle.topk_of_scores(oracle.scores_fma(q, world.centroids), nprobe)[1]
    assert np.array_equal(_probe_host(world.index, q, nprobe), want)
    flat_route = world.index.quantizer.search_device(torch.from_numpy(q.copy()).cuda(), nprobe, normalize_queries=False)[1]
    assert np.array_equal(flat_route.cpu().numpy(), want)
    _same(world.index.search(q, 10, nprobe=nprobe), _ivf_oracle(world.scores[:nq], want, world.offsets, world.rows, 10),
          f"nq={nq} nprobe={nprobe}")


def _awkward(name):
    rng = np.random.default_rng(17)
    if name == "five_empty":
        live = np.array([0, 1, 3, 4, 6, 8, 9, 11, 12, 14, 15])   # 2, 5, 7, 10, 13 stay empty
        return 16, live[rng.integers(0, live.size, size=N)]
    if name == "skewed_90":
        return 16, np.where(rng.random(N) < 0.9, 5, rng.integers(0, 16, size=N))
    if name == "tiny_1_31_32_33":
        a = np.empty(N, dtype=np.int64)
        order = rng.permutation(N)
        cuts = np.cumsum([0, 1, 31, 32, 33])
        for l in range(4):
            a[order[cuts[l]:cuts[l + 1]]] = l
        a[order[cuts[4]:]] = 4 + rng.integers(0, 2, size=N - cuts[4])
        return 6, a
    if name == "tiny_64_65":   # exactly two chunks of 32 rows, and one row into a third
        a = np.empty(N, dtype=np.int64)
        order = rng.permutation(N)
        a[order[:64]] = 0
        a[order[64:129]] = 1
        a[order[129:]] = 2 + rng.integers(0, 2, size=N - 129)
        return 4, a
    if name == "nlist_1":
        return 1, np.zeros(N, dtype=np.int64)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["five_empty", "skewed_90", "tiny_1_31_32_33", "tiny_64_65", "nlist_1"])
def test_awkward_lists(world, name, native_lib):
    nlist, assignment = _awkward(name)
    offsets, rows = ivf_mod.csr_from_assignment(assignment, nlist)
    sizes = np.diff(offsets)
    if name == "five_empty":
        assert (sizes == 0).sum() == 5
    if name == "skewed_90":
        assert sizes[5] > 0.88 * N
    if name == "tiny_1_31_32_33":
        assert sizes[:4].tolist() == [1, 31, 32, 33]
    index = IVFIndex.from_assignment(world.flat, oracle.seeded_unit_rows(nlist, DIM, 23), assignment)
    for nq in (1, 65):   # one query: its parts cut through the middle of a list
        q = world.queries[:nq]
        for k in (10, 100):
            _same(index.search(q, k, nprobe=nlist), oracle.topk_of_scores(world.scores[:nq], k), f"{name} full nq={nq} k={k}")
            for nprobe in sorted({1, min(3, nlist)}):
                probe = _probe_host(index, q, nprobe)
                assert np.array_equal(probe, oracle.topk_of_scores(oracle.scores_fma(q, index.centroids_numpy()), nprobe)[1])
                _same(index.search(q, k, nprobe=nprobe), _ivf_oracle(world.scores[:nq], probe, offsets, rows, k),
                      f"{name} nprobe={nprobe} nq={nq} k={k}")
    if name == "five_empty":   # a query whose only probed list is empty: nothing but padding
        empty_first = oracle.l2_normalize_rows(index.centroids_numpy()[[2]])
        D, I = index.search(empty_first, 5, nprobe=1)
        assert _probe_host(index, empty_first, 1)[0, 0] == 2
        assert (I == -1).all() and (D == oracle.NEG_PAD).all()
    if name == "tiny_64_65":   # each small list probed alone with k = 256: few parts, and one part that walks every chunk
        assert sizes[:2].tolist() == [64, 65]
        lib, k = native_lib, 256
        d_off, d_rows = torch.from_numpy(offsets).cuda(), torch.from_numpy(rows).cuda()
        for l in (0, 1):
            own = index.centroids_numpy()[[l]]   # a unit row: its own list scores 1.0 and is probed first
            probe = _probe_host(index, own, 1)
            assert probe[0, 0] == l
            ref = _ivf_oracle(oracle.scores_fma(own, world.corpus), probe, offsets, rows, k)
            assert (ref[1][0] >= 0).sum() == sizes[l]
            _same(index.search(own, k, nprobe=1), ref, f"{name} list {l} alone")
            _same(index.search(own, k, nprobe=1), world.flat.search(own, k, allow=rows[offsets[l]:offsets[l + 1]]),
                  f"{name} list {l} alone vs flat.search")
            # through the C-ABI with the workspace of ONE part: that part walks the list's two (three) chunks itself
            parts = C.c_int(0)
            _native.check(lib.sskd_ivf_search_plan(1, 1, k, N, 1, C.byref(parts), None, None))
            assert parts.value == 1
            one = int(lib.sskd_ivf_search_workspace_bytes(1, 1, k, N, 1))
            q = torch.from_numpy(own.copy()).cuda()
            out_s = torch.empty((1, k), dtype=torch.float32, device="cuda")
            out_i = torch.empty((1, k), dtype=torch.int64, device="cuda")
            ws = torch.empty(one, dtype=torch.uint8, device="cuda")
            _native.check(lib.sskd_ivf_search(world.flat._tiled.data_ptr(), N, q.data_ptr(), 1,
                                              torch.from_numpy(probe).cuda().data_ptr(), 1, d_off.data_ptr(),
                                              d_rows.data_ptr(), nlist, k, 0, None, out_s.data_ptr(), out_i.data_ptr(),
                                              ws.data_ptr(), one, stream()))
            torch.cuda.synchronize()
            _same((out_s.cpu().numpy(), out_i.cpu().numpy()), ref, f"{name} list {l} alone, one part")


def test_capi_probe_with_minus_one_and_more_probes_than_a_prefix_block(world, native_lib):
    """Straight through the C-ABI: -1 entries and out-of-range list numbers are skipped, and 300 probes (more than the
    256 of one prefix block; lists beyond the 16 real ones are empty) still give the exact result."""
    lib = native_lib
    nlist, nq, k = 300, 3, 10
    offsets = np.concatenate([world.offsets, np.full(nlist - NLIST, N, dtype=np.int64)])
    rng = np.random.default_rng(5)
    probe = np.stack([rng.permutation(nlist) for _ in range(nq)]).astype(np.int64)
    probe[0, probe[0] == 7] = -1        # query 0 does not visit list 7
    probe[1, probe[1] == 3] = 1 << 40   # query 1 names a list that does not exist
    q = torch.from_numpy(world.queries[:nq].copy()).cuda()
    d_probe, d_off, d_rows = (torch.from_numpy(a).cuda() for a in (probe, offsets, world.rows))
    out_s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    out_i = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    need = int(lib.sskd_ivf_search_workspace_bytes(nq, nlist, k, N, int(np.diff(offsets).max())))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    _native.check(lib.sskd_ivf_search(world.flat._tiled.data_ptr(), N, q.data_ptr(), nq, d_probe.data_ptr(), nlist,
                                      d_off.data_ptr(), d_rows.data_ptr(), nlist, k, 0, None, out_s.data_ptr(),
                                      out_i.data_ptr(), ws.data_ptr(), need, stream()))
    torch.cuda.synchronize()
    ref = _ivf_oracle(world.scores[:nq], np.where(probe < nlist, probe, -1), offsets, world.rows, k)
    _same((out_s.cpu().numpy(), out_i.cpu().numpy()), ref, "capi")
    # a smaller workspace (the plan of lists of one row: fewer parts) gives the same bits
    small = int(lib.sskd_ivf_search_workspace_bytes(nq, nlist, k, N, 1))
    assert 0 < small < need
    _native.check(lib.sskd_ivf_search(world.flat._tiled.data_ptr(), N, q.data_ptr(), nq, d_probe.data_ptr(), nlist,
                                      d_off.data_ptr(), d_rows.data_ptr(), nlist, k, 0, None, out_s.data_ptr(),
                                      out_i.data_ptr(), ws.data_ptr(), small, stream()))
    torch.cuda.synchronize()
    _same((out_s.cpu().numpy(), out_i.cpu().numpy()), ref, "capi, fewer parts")


def test_ties_come_out_in_ascending_id_order(gpu):
    """40 vectors, each stored at three ids that land in three different lists."""
    n, nlist = 600, 16
    corpus = oracle.seeded_unit_rows(n, DIM, 31)
    base = oracle.seeded_unit_rows(40, DIM, 32)
    rng = np.random.default_rng(33)
    ids = rng.permutation(n)[:120].reshape(40, 3)
    assignment = rng.integers(0, nlist, size=n)
    for j in range(40):
        for t in range(3):
            corpus[ids[j, t]] = base[j]
            assignment[ids[j, t]] = (j + 5 * t) % nlist
    flat = _flat(corpus, gpu)
    index = IVFIndex.from_assignment(flat, oracle.seeded_unit_rows(nlist, DIM, 34), assignment)
    queries = np.concatenate([base[:24], oracle.seeded_unit_rows(8, DIM, 35)])
    scores = oracle.scores_fma(queries, corpus)
    for k in (3, 10, 100):
        got = index.search(queries, k, nprobe=nlist)
        _same(got, oracle.topk_of_scores(scores, k), f"ties k={k}")
        _same(got, flat.search(queries, k), f"ties k={k} vs flat")
    D, I = index.search(queries, 10, nprobe=nlist)
    for j in range(24):   # the query's own vector three times on top, ids ascending
        assert _bits(D[j, 0]) == _bits(D[j, 1]) == _bits(D[j, 2]) and I[j, :3].tolist() == sorted(ids[j].tolist())
    equal = _bits(D)[:, 1:] == _bits(D)[:, :-1]
    assert equal.sum() >= 48 and (I[:, 1:][equal] > I[:, :-1][equal]).all()
    # a partial probe keeps the order among the copies it reaches
    offsets, rows = ivf_mod.csr_from_assignment(assignment, nlist)
    probe = _probe_host(index, queries, 6)
    _same(index.search(queries, 10, nprobe=6), _ivf_oracle(scores, probe, offsets, rows, 10), "ties, partial")


# ---------------------------------------------------------------------------------------------------- filters
def test_filters_and_removed_rows(world, gpu):
    flat = _flat(world.corpus, gpu)
    index = IVFIndex.from_assignment(flat, world.centroids, world.assignment)
    rng = np.random.default_rng(41)
    removed = rng.permutation(N)[:150]
    assert index.remove_ids(removed) == 150
    live = np.ones(N, dtype=np.bool_)
    live[removed] = False
    q, k, nprobe = world.queries[:65], 10, 4
    probe = _probe_host(index, q, nprobe)
    few = np.zeros(N, dtype=np.bool_)
    few[rng.permutation(N)[:7]] = True
    cases = {"no filter": None, "half": rng.random(N) < 0.5, "one percent": rng.random(N) < 0.01,
             "none": np.zeros(N, dtype=np.bool_), "fewer than k": few}
    for name, allow in cases.items():
        extra = live if allow is None else (allow & live)
        got = index.search(q, k, nprobe=nprobe, allow=allow)
        _same(got, _ivf_oracle(world.scores[:65], probe, world.offsets, world.rows, k, extra), name)
        hit = got[1][got[1] >= 0]
        assert extra[hit].all(), f"{name}: a masked row was returned"
        full = index.search(q, k, nprobe=NLIST, allow=allow)
        _same(full, flat.search(q, k, allow=allow), f"{name}, every list")
    assert (index.search(q, k, nprobe=nprobe, allow=cases["none"])[1] == -1).all()
    # an id array and a prepared RowFilter are the same filter
    ids = np.flatnonzero(cases["half"])
    _same(index.search(q, k, nprobe=nprobe, allow=ids), index.search(q, k, nprobe=nprobe, allow=cases["half"]), "id array")
    _same(index.search(q, k, nprobe=nprobe, allow=flat.row_filter(cases["half"])),
          index.search(q, k, nprobe=nprobe, allow=cases["half"]), "RowFilter")


# ------------------------------------------------------------------------------------------ the centroid update
def test_list_sums_against_fsum(world, native_lib):
    assignment = world.assignment.copy()
    assignment[assignment == 9] = 10   # list 9 is empty
    offsets, rows = ivf_mod.csr_from_assignment(assignment, NLIST)
    d_off, d_rows = torch.from_numpy(offsets).cuda(), torch.from_numpy(rows).cuda()

    def run():
        out = torch.full((NLIST + 1, DIM), float("nan"), dtype=torch.float64, device="cuda")
        _native.check(native_lib.sskd_ivf_list_sums(world.flat._tiled.data_ptr(), N, d_off.data_ptr(), d_rows.data_ptr(),
                                                    NLIST, out.data_ptr(), stream()))
        torch.cuda.synchronize()
        return out.cpu().numpy()

    first, second = run(), run()
    assert np.isnan(first[NLIST]).all()                                   # nothing written past the last list
    assert np.array_equal(first[:NLIST].view(np.int64), second[:NLIST].view(np.int64))   # two calls, the same bits
    assert np.array_equal(first[9].view(np.int64), np.zeros(DIM, np.int64))   # the empty list: exactly +0.0
    worst = 0.0
    for l in range(NLIST):
        part = world.corpus[rows[offsets[l]:offsets[l + 1]]].astype(np.float64)
        if part.shape[0] == 0:
            continue
        ref = np.array([math.fsum(part[:, c]) for c in range(DIM)])
        # recursive fp64 summation of n_l terms: (n_l - 1) 2^-53 sum |x|
        bound = (part.shape[0] - 1) * 2.0 ** -53 * np.abs(part).sum(axis=0)
        err = np.abs(first[l] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), f"list {l}: error {err.max():.3e} above the bound"
    print(f"list_sums: worst error / bound = {worst:.3f}")


# ----------------------------------------------------------------------------------------------------- training
@pytest.fixture(scope="module")
def trained(gpu):
    corpus = oracle.seeded_unit_rows(5000, DIM, 5)
    index = IVFIndex(flat=_flat(corpus, gpu))
    index.train(nlist=32, iterations=5)
    return SimpleNamespace(corpus=corpus, index=index, centroids=index.centroids_numpy(), lists=index.lists_numpy())


def test_training_invariants(trained):
    offsets, rows = trained.lists
    assert trained.index.nlist == 32 and offsets.shape == (33,)
    ivf_mod.check_csr(offsets, rows, 5000)     # every row in exactly one list, ascending
    assignment = ivf_mod.assignment_from_csr(offsets, rows)
    # each row's list is the best centroid under the rank order (ties to the lower list)
    best = oracle.topk_of_scores(oracle.scores_fma(trained.corpus, trained.centroids), 1)[1][:, 0]
    assert np.array_equal(assignment, best)
    assert trained.index.max_list_rows == int(np.diff(offsets).max())
    # unit centroids, to the tolerance of sskd_l2_normalize_rows (test_small_kernels_gpu.py: relative, per element)
    rel = kc.l2_depth(DIM) * kc.U / 2 + kc.SQRT + kc.DIV + kc.U
    norms = np.sqrt((trained.centroids.astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(norms - 1.0) <= rel).all(), np.abs(norms - 1.0).max()


def test_training_is_deterministic_and_seeded(trained, gpu):
    again = IVFIndex(flat=trained.index.flat)
    again.train(nlist=32, iterations=5)
    assert np.array_equal(_bits(again.centroids_numpy()), _bits(trained.centroids))
    assert all(np.array_equal(a, b) for a, b in zip(again.lists_numpy(), trained.lists))
    other = IVFIndex(flat=trained.index.flat)
    other.train(nlist=32, iterations=5, seed=4321)
    assert not np.array_equal(_bits(other.centroids_numpy()), _bits(trained.centroids))
    assert not np.array_equal(other.lists_numpy()[1], trained.lists[1])
    # a training sample smaller than the index: still every row in a list, still its best centroid
    sampled = IVFIndex(flat=trained.index.flat)
    sampled.train(nlist=32, iterations=2, max_train_rows=1000)
    offsets, rows = sampled.lists_numpy()
    ivf_mod.check_csr(offsets, rows, 5000)
    best = oracle.topk_of_scores(oracle.scores_fma(trained.corpus, sampled.centroids_numpy()), 1)[1][:, 0]
    assert np.array_equal(ivf_mod.assignment_from_csr(offsets, rows), best)


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def test_recall_gate(gpu):
    """recall@10 >= 0.97 (recall_threshold of the reference's configs/index.yaml) against the index's own exact search,
    on clustered data: 64 unit centres, 20 000 rows unit(centre + N(0, I) / sqrt(384)), 500 queries unit(row + 0.5 N(0, I)
    / sqrt(384)) from 500 distinct rows; nlist 64, 10 iterations, nprobe 8."""
    rng = np.random.default_rng(0)
    centres = _unit(rng.standard_normal((64, DIM)))
    topic = rng.integers(0, 64, size=20000)
    rows = _unit(centres[topic] + rng.standard_normal((20000, DIM)) / np.sqrt(DIM))
    picked = rng.permutation(20000)[:500]
    queries = _unit(rows[picked] + 0.5 * rng.standard_normal((500, DIM)) / np.sqrt(DIM))
    index = IVFIndex(embedding_dim=DIM, metric="ip", device=str(gpu), nprobe=8)
    index.build_from_embeddings(rows, nlist=64, iterations=10)
    assert index.nlist == 64 and index.ntotal == 20000
    truth = index.flat.search(queries, 10)[1]
    recall = {p: ivf_mod.recall_at_k(index.search(queries, 10, nprobe=p)[1], truth) for p in (1, 8, 64)}
    print(f"recall@10: {recall}; empty lists: {int((np.diff(index.lists_numpy()[0]) == 0).sum())}")
    assert recall[64] == 1.0
    assert recall[8] >= 0.97
    validated = index.validate(num_queries=1000, k=10, seed=0)
    print(f"validate(): {validated:.4f}")
    assert validated >= 0.97


# ---------------------------------------------------------------------------------------------------- lifecycle
def test_add_assigns_the_new_rows_to_the_existing_centroids(world, gpu):
    index = IVFIndex(flat=_flat(world.corpus, gpu))
    index.train(nlist=NLIST, iterations=3)
    centroids = index.centroids_numpy()
    extra = oracle.seeded_unit_rows(500, DIM, 51)
    index.add(extra)
    assert index.ntotal == N + 500 and np.array_equal(_bits(index.centroids_numpy()), _bits(centroids))
    both = np.concatenate([world.corpus, extra])
    offsets, rows = index.lists_numpy()
    ivf_mod.check_csr(offsets, rows, N + 500)
    best = oracle.topk_of_scores(oracle.scores_fma(both, centroids), 1)[1][:, 0]
    assert np.array_equal(ivf_mod.assignment_from_csr(offsets, rows), best)
    # a new row finds itself in its own list, and the full-probe contract holds over all rows
    D, I = index.search(extra[:64], 1, nprobe=1)
    assert np.array_equal(I[:, 0], N + np.arange(64))
    q = world.queries[:65]
    _same(index.search(q, 10, nprobe=NLIST), oracle.topk_of_scores(oracle.scores_fma(q, both), 10), "after add")


def test_remove_then_compact(world, gpu):
    index = IVFIndex.from_assignment(_flat(world.corpus, gpu), world.centroids, world.assignment)
    gone = np.random.default_rng(61).permutation(N)[:400]
    index.remove_ids(gone)
    q = world.queries[:65]
    before = index.search(q, 10, nprobe=4)
    old_lists = index.lists_numpy()
    kept = index.compact()
    assert kept.size == N - 400 and index.ntotal == N - 400 and index.flat.n_removed == 0
    after = index.search(q, 10, nprobe=4)
    assert np.array_equal(_bits(after[0]), _bits(before[0]))
    assert np.array_equal(np.where(after[1] >= 0, kept[np.maximum(after[1], 0)], -1), before[1])
    ref_lists = ivf_mod.remap_lists(old_lists[0], old_lists[1], kept)
    assert all(np.array_equal(a, b) for a, b in zip(index.lists_numpy(), ref_lists))
    _same(index.search(q, 10, nprobe=NLIST), index.flat.search(q, 10), "after compact, every list")


def test_save_load(world, tmp_path):
    q = world.queries[:65]
    before = world.index.search(q, 10, nprobe=4)
    world.index.save(tmp_path)
    for name in ("index.faiss", "doc_ids.json", "ivf_centroids.npy", "ivf_list_offsets.npy", "ivf_list_rows.npy", "ivf.json"):
        assert (tmp_path / name).exists(), name
    again = IVFIndex(embedding_dim=DIM, metric="ip", device=str(world.flat.device))
    again.load(tmp_path)
    assert again.nlist == NLIST and again.ntotal == N and again.nprobe == world.index.nprobe
    _same(again.search(q, 10, nprobe=4), before, "after load")
    # the flat loader ignores the extra files and still answers exactly
    plain = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(world.flat.device))
    plain.load(tmp_path)
    _same(plain.search(q, 10), oracle.topk_of_scores(world.scores[:65], 10), "FAISSIndexBuilder.load")


def test_search_device_under_graph_capture(world):
    q = torch.from_numpy(world.queries[:8].copy()).cuda()
    ref = world.index.search(world.queries[:8], 10, nprobe=4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = world.index.search_device(q, 10, nprobe=4)   # sizes the workspaces
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = world.index.search_device(q, 10, nprobe=4)
    g.replay()
    torch.cuda.synchronize()
    for name, got in (("eager", eager), ("graph", captured)):
        _same(tuple(t.cpu().numpy() for t in got), ref, name)


def test_python_argument_checks(world):
    q = world.queries[:2]
    for bad in (0, 257):
        with pytest.raises(ValueError):
            world.index.search(q, bad)
    with pytest.raises(ValueError):
        world.index.search(q, 10, nprobe=0)
    _same(world.index.search(q, 10, nprobe=10 ** 6), world.index.search(q, 10, nprobe=NLIST), "nprobe above nlist")
    fresh = IVFIndex(flat=world.flat)
    with pytest.raises(RuntimeError):
        fresh.search(q, 10)   # no lists yet
