"""Range search on the MI355X: every allowed row scoring above a per-query threshold (faiss ``range_search``).

The oracle: the fma-order scores of every row (``oracle.search.scores_fma``) with masked rows set to -inf; query q
returns ``flatnonzero(s > thr_q)`` ordered by ``lexsort((rows, -s))``.  Every comparison is bit-equal on lims, D
and I.
"""
import numpy as np
import pytest
import torch

from capi_helpers import stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import _native
from test_filtered_search_gpu import _masks

DIM = 384


def _ref_from_scores(s, thr, id_offset=0):
    lims, D, I = [0], [], []
    for q in range(s.shape[0]):
        row = s[q]
        sel = np.flatnonzero(row > thr[q])
        sel = sel[np.lexsort((sel, -row[sel].astype(np.float64)))]
        D.append(row[sel])
        I.append(sel.astype(np.int64) + id_offset)
        lims.append(lims[-1] + sel.size)
    return (np.array(lims, np.int64), np.concatenate(D).astype(np.float32) if D else np.zeros(0, np.float32),
            np.concatenate(I) if I else np.zeros(0, np.int64))


def _ref(queries, corpus, thr, allowed=None, id_offset=0):
    s = oracle.scores_fma(queries, corpus)
    if allowed is not None:
        s[:, ~allowed] = -np.inf
    return _ref_from_scores(s, thr, id_offset)


def _same(got, ref, what=""):
    lims, D, I = got
    assert np.array_equal(lims, ref[0]), (what, np.flatnonzero(lims != ref[0])[:5])
    assert np.array_equal(I, ref[2]), what
    assert np.array_equal(D.view(np.uint32), ref[1].view(np.uint32)), what


def _index(corpus, gpu, id_offset=0):
    from semantic_search_kd_amd import FAISSIndexBuilder

    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu), id_offset=id_offset)
    index.build_from_embeddings(corpus)
    return index


def _spread_thresholds(s):
    """per-query thresholds that return 0, 1, ~10, ~1 %, ~50 % and all rows, in turn"""
    n = s.shape[1]
    wanted = [0, 1, 10, max(1, n // 100), n // 2, n]
    thr = np.empty(s.shape[0], np.float32)
    for q in range(s.shape[0]):
        c = min(wanted[q % len(wanted)], n)
        desc = np.sort(s[q])[::-1]
        thr[q] = -np.inf if c >= n else desc[c]
    return thr


@pytest.mark.gpu
@pytest.mark.parametrize("n,nq", [(1, 1), (31, 3), (33, 5), (3001, 200), (5000, 100), (20000, 64)])
def test_range_search_shapes_and_thresholds(gpu, n, nq):
    corpus = oracle.seeded_unit_rows(n, DIM, n + 5)
    queries = oracle.seeded_unit_rows(nq, DIM, nq + 9)
    s = oracle.scores_fma(queries, corpus)
    thr = _spread_thresholds(s)
    index = _index(corpus, gpu, id_offset=7)
    got = index.range_search(queries, thr)
    ref = _ref_from_scores(s, thr, 7)
    _same(got, ref, (n, nq))
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64
    # a scalar threshold is every query's
    got = index.range_search(queries, float(np.median(s)))
    _same(got, _ref_from_scores(s, np.full(nq, np.float32(np.median(s))), 7), "scalar")


@pytest.mark.gpu
def test_range_search_boundary_ties_nan_and_id_offset(gpu, native_lib):
    lib = native_lib
    corpus = oracle.seeded_unit_rows(300, DIM, 3)
    corpus[17] = corpus[5]            # duplicates tie: ids ascending
    corpus[40] = corpus[5]
    corpus[99] = np.nan               # a NaN row is never returned
    queries = oracle.seeded_unit_rows(4, DIM, 4)
    queries[0] = corpus[5]
    s = oracle.scores_fma(queries, corpus)
    x = s[1, 123]
    thr = np.array([-np.inf, x, np.nextafter(x, -np.inf, dtype=np.float32), np.nan], np.float32)
    index = _index(corpus, gpu)
    got = index.range_search(queries, thr)
    ref = _ref_from_scores(s, thr)
    _same(got, ref)
    lims, D, I = got
    q0 = I[lims[0]:lims[1]]
    assert 99 not in q0 and lims[1] - lims[0] == 299
    assert q0[:3].tolist() == [5, 17, 40]            # equal scores come back in id order
    assert 123 not in I[lims[1]:lims[2]]               # a threshold equal to the score excludes the row
    assert 123 in I[lims[2]:lims[3]]                   # one ulp below includes it
    assert lims[4] == lims[3]                          # a NaN threshold returns nothing

    # the C-ABI with an id offset
    tiled = tile_corpus(lib, corpus)
    got = _capi(lib, tiled, corpus.shape[0], queries, thr, max_results=int(ref[0][-1]), id_offset=1000)
    _same(got[:3], _ref_from_scores(s, thr, 1000), "capi")


def _capi(lib, tiled, n, queries, thr, max_results, id_offset=0, buf=None, null_outputs=False, mask=None):
    """direct C-ABI call; outputs of `buf` entries (default max_results) pre-filled with a sentinel"""
    nq = queries.shape[0]
    buf = max_results if buf is None else buf
    q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(thr, np.float32)).cuda()
    lims = torch.full((nq + 1,), -3, dtype=torch.int64, device="cuda")
    sc = torch.full((max(buf, 1),), 12345.0, dtype=torch.float32, device="cuda")
    ids = torch.full((max(buf, 1),), -77, dtype=torch.int64, device="cuda")
    ws_b = int(lib.sskd_index_range_search_workspace_bytes(n, nq, max_results))
    ws = torch.empty(max(ws_b, 1), dtype=torch.uint8, device="cuda")
    _native.check(lib.sskd_index_range_search(
        tiled.data_ptr(), n, q.data_ptr(), nq, t.data_ptr(), id_offset, None if mask is None else mask.data_ptr(),
        lims.data_ptr(), None if null_outputs else sc.data_ptr(), None if null_outputs else ids.data_ptr(), max_results,
        ws.data_ptr(), ws.numel(), stream()))
    torch.cuda.synchronize()
    L = lims.cpu().numpy()
    total = int(L[-1])
    keep = min(total, buf) if total <= max_results else 0
    return L, sc.cpu().numpy()[:keep], ids.cpu().numpy()[:keep], sc.cpu().numpy(), ids.cpu().numpy()


_PAST_ONE_SCAN_BLOCK = {}


def _past_one_scan_block():
    """64 rows x 8 193 queries, computed once: the scores and thresholds that return 0, 1, 5, all 64, 2, 0 and 17 rows
    in turn, so the counts the lims scan adds up differ from query to query"""
    if not _PAST_ONE_SCAN_BLOCK:
        corpus = oracle.seeded_unit_rows(64, DIM, 71)
        queries = oracle.seeded_unit_rows(8193, DIM, 72)
        s = oracle.scores_fma(queries, corpus)
        desc = -np.sort(-s, axis=1)
        want = np.array([0, 1, 5, 64, 2, 0, 17])[np.arange(8193) % 7]
        thr = np.where(want >= 64, -np.inf, desc[np.arange(8193), np.minimum(want, 63)]).astype(np.float32)
        _PAST_ONE_SCAN_BLOCK.update(corpus=corpus, queries=queries, s=s, thr=thr)
    return _PAST_ONE_SCAN_BLOCK


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [4095, 4096, 4097, 8193])
def test_range_search_lims_past_one_scan_block(gpu, native_lib, nq):
    """The CSR build scans 4 096 queries per workgroup: one block not full, one exactly full, one query into a second
    block, one into a third - the block offsets, the carry over the block sums and the total in ``lims[nq]``."""
    c = _past_one_scan_block()
    s, thr = c["s"][:nq], c["thr"][:nq]
    ref = _ref_from_scores(s, thr, 500)
    counts = np.diff(ref[0])
    assert (counts == 0).any() and (counts == 64).any() and len(set(counts.tolist())) >= 6
    tiled = tile_corpus(native_lib, c["corpus"])
    total = int(ref[0][-1])
    got = _capi(native_lib, tiled, 64, c["queries"][:nq], thr, max_results=total, id_offset=500)
    _same(got[:3], ref, nq)
    # count-only: the same lims
    got = _capi(native_lib, tiled, 64, c["queries"][:nq], thr, max_results=0, null_outputs=True)
    assert np.array_equal(got[0], ref[0])


@pytest.mark.gpu
def test_range_search_masks_and_removed_rows(gpu):
    n, nq = 3001, 37
    rng = np.random.default_rng(11)
    corpus = oracle.seeded_unit_rows(n, DIM, 21)
    queries = oracle.seeded_unit_rows(nq, DIM, 22)
    s = oracle.scores_fma(queries, corpus)
    thr = _spread_thresholds(s)
    index = _index(corpus, gpu)
    for name, allowed in _masks(n, 10, rng).items():
        _same(index.range_search(queries, thr, allow=allowed), _ref(queries, corpus, thr, allowed), name)
    removed = rng.choice(n, 400, replace=False)
    index.remove_ids(removed)
    live = np.ones(n, bool)
    live[removed] = False
    _same(index.range_search(queries, thr), _ref(queries, corpus, thr, live), "removed")
    allow = rng.random(n) < 0.5
    _same(index.range_search(queries, thr, allow=allow), _ref(queries, corpus, thr, allow & live), "allow+removed")
    _same(index.range_search(queries, thr, allow=np.flatnonzero(allow)), _ref(queries, corpus, thr, allow & live), "ids")


@pytest.mark.gpu
def test_range_search_overflow_keeps_lims_exact_and_writes_nothing_past_capacity(gpu, native_lib):
    lib = native_lib
    n, nq = 5000, 50
    corpus = oracle.seeded_unit_rows(n, DIM, 31)
    queries = oracle.seeded_unit_rows(nq, DIM, 32)
    s = oracle.scores_fma(queries, corpus)
    thr = _spread_thresholds(s)
    ref = _ref_from_scores(s, thr)
    total = int(ref[0][-1])
    assert total > 1000
    tiled = tile_corpus(lib, corpus)
    for cap in (1, 997, total - 1):
        L, _, _, sc_all, ids_all = _capi(lib, tiled, n, queries, thr, max_results=cap, buf=cap + 4096)
        assert np.array_equal(L, ref[0]), cap
        assert (sc_all[cap:] == 12345.0).all() and (ids_all[cap:] == -77).all(), cap
    got = _capi(lib, tiled, n, queries, thr, max_results=total, buf=total + 64)
    _same(got[:3], ref, "exact capacity")
    assert (got[3][total:] == 12345.0).all() and (got[4][total:] == -77).all()
    L = _capi(lib, tiled, n, queries, thr, max_results=0, null_outputs=True)[0]     # count only
    assert np.array_equal(L, ref[0])
    # the Python wrapper grows its buffer from a tiny capacity with one retry
    index = _index(corpus, gpu)
    index.range_capacity = 3
    _same(index.range_search(queries, thr), ref, "wrapper")
    assert index.range_capacity == total
    # empty shapes
    assert index.range_search(np.zeros((0, DIM), np.float32), 0.5)[0].tolist() == [0]


def _aniso(n, nq, seed):
    rng = np.random.default_rng(seed)
    common = rng.standard_normal(DIM).astype(np.float32)
    common /= np.linalg.norm(common)
    centres = rng.standard_normal((64, DIM)).astype(np.float32) / np.sqrt(DIM)
    def draw(m):
        x = 2.0 * common + 0.5 * centres[rng.integers(0, 64, m)] + rng.standard_normal((m, DIM)).astype(np.float32) / np.sqrt(DIM)
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    return draw(n), draw(nq)


@pytest.mark.gpu
def test_range_search_long_segments(gpu):
    # thr = -inf over 50 000 rows: segments longer than one LDS sort (chunks + merge passes)
    n = 50_000
    corpus = oracle.seeded_unit_rows(n, DIM, 41)
    queries = oracle.seeded_unit_rows(3, DIM, 42)
    index = _index(corpus, gpu)
    thr = np.full(3, -np.inf, np.float32)
    _same(index.range_search(queries, thr), _ref(queries, corpus, thr), "-inf")
    # anisotropic e5-like rows (mean pairwise cosine ~0.8): one threshold returns >= 30 % of the rows
    rows, q = _aniso(40_000, 256, 43)
    s = oracle.scores_fma(q, rows)
    assert 0.7 < float((rows[:512] @ rows[512:1024].T).mean()) < 0.9
    t = np.float32(np.quantile(s[:16], 0.6))
    thr = np.full(256, t, np.float32)
    ref = _ref_from_scores(s, thr)
    counts = np.diff(ref[0])
    assert counts.mean() >= 0.3 * rows.shape[0] and counts.max() > 16384 and (counts < 16384).any()
    index = _index(rows, gpu)
    _same(index.range_search(q, thr), ref, "anisotropic")


@pytest.mark.gpu
def test_range_search_full_size_matches_topk_prefix(gpu):
    from semantic_search_kd_amd import FAISSIndexBuilder

    n, nq = 1_000_000, 64
    gen = torch.Generator(device="cuda").manual_seed(77)
    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device="cuda:0", id_offset=5)
    index.reserve(n)
    for lo in range(0, n, 1 << 18):
        rows = torch.randn((min(1 << 18, n - lo), DIM), generator=gen, device="cuda", dtype=torch.float32)
        index.add(rows / rows.norm(dim=1, keepdim=True))
    q = torch.randn((nq, DIM), generator=gen, device="cuda", dtype=torch.float32)
    q /= q.norm(dim=1, keepdim=True)
    qh = q.cpu().numpy()
    S, I = index.search(qh, 256)
    thr = S[:, 199].copy()
    lims, D, R = index.range_search(qh, thr)
    for j in range(nq):
        keep = S[j] > thr[j]
        assert np.array_equal(R[lims[j]:lims[j + 1]], I[j][keep]), j
        assert np.array_equal(D[lims[j]:lims[j + 1]], S[j][keep]), j
    corpus = index.to_numpy()
    sample = [0, 17, 40, 63]
    ref = _ref(qh[sample], corpus, thr[sample], id_offset=5)
    got_l = np.concatenate([[0], np.cumsum([lims[j + 1] - lims[j] for j in sample])])
    got_D = np.concatenate([D[lims[j]:lims[j + 1]] for j in sample])
    got_I = np.concatenate([R[lims[j]:lims[j + 1]] for j in sample])
    _same((got_l, got_D, got_I), ref, "sampled")


@pytest.mark.gpu
def test_range_search_device_replays_in_a_graph(gpu):
    n, nq = 20_000, 96
    corpus = oracle.seeded_unit_rows(n, DIM, 51)
    queries = oracle.seeded_unit_rows(nq, DIM, 52)
    s = oracle.scores_fma(queries, corpus)
    thr_h = _spread_thresholds(s)
    thr_h[thr_h == -np.inf] = np.float32(0.0)
    ref = _ref_from_scores(s, thr_h)
    index = _index(corpus, gpu)
    q = torch.from_numpy(queries).cuda()
    thr = torch.from_numpy(thr_h).cuda()
    cap = int(ref[0][-1]) + 100
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = index.range_search_device(q, thr, max_results=cap, normalize_queries=False)   # sizes the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lims, sc, ids = index.range_search_device(q, thr, max_results=cap, normalize_queries=False)
    g.replay()
    torch.cuda.synchronize()
    total = int(ref[0][-1])
    for got in (eager, (lims, sc, ids)):
        L, D, I = (t.cpu().numpy() for t in got)
        _same((L, D[:total], I[:total]), ref, "graph")


@pytest.mark.gpu
def test_near_duplicates_small_against_the_oracle(gpu):
    n = 4096
    rng = np.random.default_rng(61)
    C = oracle.seeded_unit_rows(n, DIM, 61)
    plants = [(3, 2000), (999, 1000), (1500, 4095), (10, 20), (20, 30)]   # (10, 20, 30): a triple
    for a, b in plants:
        x = C[a] + 0.05 * rng.standard_normal(DIM).astype(np.float32) / np.sqrt(DIM)
        C[b] = x / np.linalg.norm(x)
    index = _index(C, gpu)
    index.remove_ids([1000])
    thr = 0.9
    pairs, scores = index.near_duplicates(thr, batch_size=1000)
    S = oracle.scores_fma(C, C)
    live = np.ones(n, bool)
    live[1000] = False
    ok = (S > thr) & np.triu(np.ones((n, n), bool), 1) & live[:, None] & live[None, :]
    i, j = np.nonzero(ok)
    sv = S[i, j]
    order = np.lexsort((j, -sv.astype(np.float64), i))
    assert np.array_equal(pairs, np.stack([i[order], j[order]], 1).astype(np.int64))
    assert np.array_equal(scores.view(np.uint32), sv[order].view(np.uint32))
    assert {(10, 20), (20, 30), (10, 30)} <= set(map(tuple, pairs.tolist()))
    assert not (pairs == 1000).any() and len(pairs) == 5
    assert np.array_equal(S, S.T)     # the oracle's symmetry the kernel relies on


@pytest.mark.gpu
def test_near_duplicates_across_batches_at_200k(gpu):
    n, bs = 200_000, 4096
    rng = np.random.default_rng(71)
    C = rng.standard_normal((n, DIM)).astype(np.float32)
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    plants = [(bs - 1, bs), (0, n - 1), (2 * bs - 1, 3 * bs + 5), (12345, 12346), (77_777, 150_000)]
    for a, b in plants:
        x = C[a] + 0.05 * rng.standard_normal(DIM).astype(np.float32) / np.sqrt(DIM)
        C[b] = x / np.linalg.norm(x)
    index = _index(C, gpu, id_offset=100)
    pairs, scores = index.near_duplicates(0.8, batch_size=bs)
    want = sorted((a + 100, b + 100) for a, b in plants)
    assert sorted(map(tuple, pairs.tolist())) == want
    assert pairs[:, 0].tolist() == sorted(pairs[:, 0].tolist())
    for (a, b), sc in zip(pairs.tolist(), scores):
        assert sc == oracle.scores_fma(C[a - 100:a - 99], C[b - 100:b - 99])[0, 0]
        assert sc > 0.95
