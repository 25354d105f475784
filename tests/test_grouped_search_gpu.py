"""Grouped search on the MI355X: the top-k distinct groups by their best row (``include/sskd_amd.h``).

The oracle (``grouped_cases.py``): the fma-order scores of every row, masked rows at -inf, ``search``'s full ranking
walked keeping the first row of every group.  Every comparison is bit-equal on D, I and G.  Shapes are the smallest
at which the path can go wrong: a tile is 32 rows, a collapse step 64 ranks, a chained pass 32 results.
"""
import numpy as np
import pytest
import torch

import grouped_cases as gc
import ranking_walk_cases as rw
from capi_helpers import stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import _native
from semantic_search_kd_amd.index import mask_words

DIM = gc.DIM
K_MAX = _native.SSKD_K_MAX
SENT_S, SENT_I, SENT_G = 12345.0, -77, -55


def _index(corpus, gpu, groups=None, id_offset=0):
    from semantic_search_kd_amd import FAISSIndexBuilder

    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu), id_offset=id_offset)
    index.build_from_embeddings(np.array(corpus), groups=None if groups is None else list(groups))
    return index


def _capi(lib, tiled, n, queries, k, k_rows, groups, id_offset=0, allowed=None):
    """direct C-ABI call into sentinel-filled outputs ONE ROW LONGER than the call's; returns host arrays
    ``(D, I, G, counts, unproved, n_unproved)`` of the call's rows after checking the extra row is untouched"""
    nq = queries.shape[0]
    q = torch.from_numpy(np.array(queries, np.float32)).cuda()       # (copies: the shared cases are read-only)
    rg = torch.from_numpy(np.array(groups, np.int32)).cuda()
    mask = None if allowed is None else torch.from_numpy(mask_words(allowed, n).view(np.int32)).cuda()
    sc = torch.full((nq + 1, k), SENT_S, dtype=torch.float32, device="cuda")
    ids = torch.full((nq + 1, k), SENT_I, dtype=torch.int64, device="cuda")
    gr = torch.full((nq + 1, k), SENT_G, dtype=torch.int32, device="cuda")
    cnt = torch.full((nq + 1,), SENT_G, dtype=torch.int32, device="cuda")
    unp = torch.full((nq + 1,), SENT_G, dtype=torch.int32, device="cuda")
    nun = torch.full((1,), SENT_G, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(int(lib.sskd_index_search_grouped_workspace_bytes(n, nq, k, k_rows)), 1), dtype=torch.uint8, device="cuda")
    _native.check(lib.sskd_index_search_grouped(
        tiled.data_ptr(), n, q.data_ptr(), nq, k, k_rows, id_offset, None if mask is None else mask.data_ptr(),
        rg.data_ptr(), sc.data_ptr(), ids.data_ptr(), gr.data_ptr(), cnt.data_ptr(), unp.data_ptr(), nun.data_ptr(),
        ws.data_ptr(), ws.numel(), stream()))
    torch.cuda.synchronize()
    sc, ids, gr, cnt, unp = (t.cpu().numpy() for t in (sc, ids, gr, cnt, unp))
    assert (sc[nq] == np.float32(SENT_S)).all() and (ids[nq] == SENT_I).all() and (gr[nq] == SENT_G).all()
    assert cnt[nq] == SENT_G and unp[nq] == SENT_G, "wrote past the last query"
    return sc[:nq], ids[:nq], gr[:nq], cnt[:nq], unp[:nq].astype(bool), int(nun.item())


def _check_against(got, ref):
    """proved queries equal the oracle; unproved ones its prefix of length count, then padding"""
    D, I, G, cnt, unp, n_unp = got
    rD, rI, rG, rcnt, runp = ref
    assert np.array_equal(unp, runp), np.flatnonzero(unp != runp)[:5]
    assert n_unp == int(runp.sum())
    assert np.array_equal(cnt, rcnt)
    gc.same((D, I, G), (rD, rI, rG))      # the oracle at this k_rows pads behind its own count
    for q in np.flatnonzero(unp):          # ... which for an unproved query is a prefix of the full answer
        assert cnt[q] < D.shape[1] and (I[q, cnt[q]:] == -1).all() and (G[q, cnt[q]:] == -1).all()
        assert (D[q, cnt[q]:] == gc.NEG_PAD).all()


# ---------------------------------------------------------------------------------------------------------------------
# singletons reproduce search
# ---------------------------------------------------------------------------------------------------------------------
_singleton_indexes = {}


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 3, 70])
@pytest.mark.parametrize("n", [1, 31, 33, 1000])
def test_singleton_groups_reproduce_search(gpu, n, nq):
    if n not in _singleton_indexes:
        _singleton_indexes[n] = _index(oracle.seeded_unit_rows(n, DIM, 400 + n), gpu, id_offset=5)
    index = _singleton_indexes[n]
    q = torch.from_numpy(oracle.seeded_unit_rows(nq, DIM, 410 + nq)).cuda()
    for k in (1, 10, 33):
        rs, ri = index.search_device(q, k)
        s, i, g, unproved = index.search_grouped_device(q, k)
        rs, ri, s, i, g, unproved = (t.cpu().numpy() for t in (rs, ri, s, i, g, unproved))
        assert not unproved.any()
        assert np.array_equal(i, ri) and np.array_equal(s.view(np.uint32), rs.view(np.uint32)), (n, nq, k)
        assert np.array_equal(g, np.where(i >= 0, i - 5, -1)), "G is the local row"
        assert np.array_equal(index.last_group_counts.cpu().numpy(), np.minimum(n, k).repeat(nq))
    D, I, G = index.search_grouped(q.cpu().numpy(), 10)      # the host route agrees
    assert index.last_search_path == "grouped:counted"
    rs, ri = index.search(q.cpu().numpy(), 10)
    assert np.array_equal(I, ri) and np.array_equal(D.view(np.uint32), rs.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI at every k_rows that takes another path
# ---------------------------------------------------------------------------------------------------------------------
_tiled = {}


def _case(lib, name):
    if name not in _tiled:
        data = gc.runs_of_three() if name == "runs3" else gc.random_groups()
        _tiled[name] = (tile_corpus(lib, np.array(data[0])),) + tuple(data)
    return _tiled[name]


@pytest.mark.gpu
@pytest.mark.parametrize("k_rows", ["k", 32, 33, 64, 65, 200])
@pytest.mark.parametrize("name,k,nq", [("runs3", 10, 70), ("random", 31, 70), ("random", 31, 3)])
def test_capi_unproved_matches_the_oracle_statement(gpu, native_lib, name, k, nq, k_rows):
    tiled, corpus, queries, groups, scores = _case(native_lib, name)
    k_rows = k if k_rows == "k" else k_rows
    got = _capi(native_lib, tiled, corpus.shape[0], queries[:nq], k, k_rows, groups)
    ref = gc.expected(scores[:nq], groups, k, k_rows=k_rows)
    _check_against(got, ref)
    full = gc.expected(scores[:nq], groups, k)
    for q in range(nq):                     # what an unproved query did write is the exact beginning of the answer
        c = got[3][q]
        assert np.array_equal(got[1][q, :c], full[1][q, :c]) and np.array_equal(got[2][q, :c], full[2][q, :c])
    if name == "runs3" and k_rows >= (k - 1) * 3 + 1:
        assert not got[4].any(), "(k - 1) m + 1 rows always hold k groups"
    if k_rows == k:
        assert got[4].any(), "the case is meant to leave some query unproved at k_rows = k"


@pytest.mark.gpu
def test_capi_id_offset_shifts_ids_not_groups(gpu, native_lib):
    tiled, corpus, queries, groups, scores = _case(native_lib, "runs3")
    got = _capi(native_lib, tiled, corpus.shape[0], queries[:5], 10, 32, groups, id_offset=1_000_000_007)
    base = gc.expected(scores[:5], groups, 10, k_rows=32)
    ref = gc.expected(scores[:5], groups, 10, id_offset=1_000_000_007, k_rows=32)
    _check_against(got, ref)
    assert np.array_equal(got[1], base[1] + 1_000_000_007) and np.array_equal(got[2], base[2])


@pytest.mark.gpu
@pytest.mark.parametrize("k_rows", rw.WIDTHS)
def test_capi_walk_with_the_first_pad_on_both_sides_of_the_step(gpu, native_lib, k_rows):
    """The row ranking this kernel walks is written by the exact search inside the same call, so its padding is always
    a suffix of -1: the first -1 stands at rank 0, 63 (last lane of step one), 64 (first lane of step two) or nowhere
    by allowing 0, 63, 64 or all of the 200 rows.  (A negative id other than -1, an id outside the index or a row behind
    the padding cannot reach this kernel through the C-ABI: see the table in ``csrc/ranking_walk.h``.)"""
    n, nq = 200, rw.NQ
    corpus = oracle.seeded_unit_rows(n, DIM, 441)
    queries = oracle.seeded_unit_rows(nq, DIM, 442)
    scores = oracle.scores_fma(queries, corpus)
    groups = (np.arange(n) // 3).astype(np.int32)
    tiled = tile_corpus(native_lib, corpus)
    rng = np.random.default_rng(443)
    for n_allowed in (0, 63, 64, n):
        allowed = np.zeros(n, bool)
        allowed[rng.permutation(n)[:n_allowed]] = True
        # k = k_rows too, except where the ranking is full to its last rank with nothing behind it: the kernel meets no
        # -1 there and reports such a query as unproved (the safe answer), the oracle knows that no row is left
        for k in sorted({min(10, k_rows)} | ({k_rows} if n_allowed != k_rows else set())):
            got = _capi(native_lib, tiled, n, queries, k, k_rows, groups, id_offset=1000,
                        allowed=None if n_allowed == n else allowed)
            ref = gc.expected(scores, groups, k, allowed, 1000, k_rows)
            _check_against(got, ref)
            if n_allowed < k_rows:
                assert not got[4].any(), "a -1 inside the ranking proves the answer"
            if n_allowed == 0:
                assert (got[3] == 0).all() and (got[1] == -1).all()


# ---------------------------------------------------------------------------------------------------------------------
# ties, k reached inside a step, fewer groups than k
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ties_across_the_step_boundary_and_between_groups(gpu, native_lib):
    corpus, queries, groups, scores, (same_lo, same_hi, diff_lo, diff_hi) = gc.scaled_copies()
    order, _ = gc.ranking(scores[0])
    assert order[63] == same_lo and order[64] == same_hi and groups[same_lo] == groups[same_hi]
    assert scores[0, same_lo] == scores[0, same_hi] and scores[0, diff_lo] == scores[0, diff_hi]
    tiled = tile_corpus(native_lib, np.array(corpus))
    got = _capi(native_lib, tiled, corpus.shape[0], queries, 100, 128, groups)
    _check_against(got, gc.expected(scores, groups, 100, k_rows=128))
    I, G = got[1][0], got[2][0]
    assert I[63] == same_lo and same_hi not in I, "the duplicate at rank 64 falls to the group kept at rank 63"
    assert (G == groups[same_lo]).sum() == 1
    p, q = int(np.flatnonzero(I == diff_lo)[0]), int(np.flatnonzero(I == diff_hi)[0])
    assert q == p + 1 and G[p] != G[q], "equal scores in two groups: both stay, the lower row first"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 63, 64, 65])
def test_k_reached_inside_a_step_writes_nothing_further(gpu, native_lib, k):
    tiled, corpus, queries, groups, scores = _case(native_lib, "runs3")
    got = _capi(native_lib, tiled, corpus.shape[0], queries[:3], k, 200, groups)   # the helper checks the row behind
    _check_against(got, gc.expected(scores[:3], groups, k, k_rows=200))
    assert (got[3] == k).all() and not got[4].any()


@pytest.mark.gpu
def test_fewer_groups_than_k_is_proved_by_exhaustion(gpu):
    corpus = oracle.seeded_unit_rows(100, DIM, 431)
    queries = oracle.seeded_unit_rows(2, DIM, 432)
    groups = np.zeros(100, np.int32)
    index = _index(corpus, gpu, groups=["only"] * 100)
    ref = gc.expected(oracle.scores_fma(queries, corpus), groups, 5)
    q = torch.from_numpy(queries).cuda()
    s, i, g, unproved = index.search_grouped_device(q, 5, k_rows=128)
    assert not unproved.cpu().numpy().any() and index.last_group_counts.cpu().tolist() == [1, 1]
    assert int(index.last_group_n_unproved.item()) == 0
    gc.same((s.cpu().numpy(), i.cpu().numpy(), g.cpu().numpy()), ref)
    s, i, g, unproved = index.search_grouped_device(q, 5)          # 32 of the 100 rows: one group, rows remain
    assert unproved.cpu().numpy().all() and index.last_group_counts.cpu().tolist() == [1, 1]
    assert int(index.last_group_n_unproved.item()) == 2
    gc.same(index.search_grouped(queries, 5), ref)
    assert (ref[1][:, 1:] == -1).all() and "mask" not in index.last_search_path
    assert index.group_key(ref[2][0]) == ["only", None, None, None, None]


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_masks_lower_a_document_they_do_not_drop_it(gpu):
    corpus, queries, groups, scores = gc.runs_of_three()
    n, nq, k = corpus.shape[0], 8, 10
    queries = queries[:nq].copy()
    queries[0] = corpus[groups == 100].sum(0)               # query 0 asks for document 100: its three chunks lead
    queries[0] /= np.linalg.norm(queries[0])
    scores = oracle.scores_fma(queries, corpus)
    index = _index(corpus, gpu, groups=[f"doc{g}" for g in groups])
    full = gc.expected(scores, groups, k)
    gc.same(index.search_grouped(queries, k), full, "no mask")
    assert index.last_search_path == "grouped:counted" and index.max_group_size == 3

    top_doc, top_row = int(full[2][0, 0]), int(full[1][0, 0])
    assert top_doc == 100
    allow = np.ones(n, bool)
    allow[top_row] = False                                  # the best chunk of query 0's top document
    got = index.search_grouped(queries, k, allow=allow)
    gc.same(got, gc.expected(scores, groups, k, allowed=allow), "best chunk masked")
    siblings = np.flatnonzero((groups == top_doc) & allow)
    second = siblings[np.lexsort((siblings, -scores[0, siblings].astype(np.float64)))][0]
    where = np.flatnonzero(got[2][0] == top_doc)
    assert where.size == 1, "the document stays"
    assert got[1][0, where[0]] == second and got[0][0, where[0]] == scores[0, second]

    allow = groups != top_doc                               # the whole document
    got = index.search_grouped(queries, k, allow=allow)
    gc.same(got, gc.expected(scores, groups, k, allowed=allow), "document masked")
    assert top_doc not in got[2][0]

    none = np.zeros(n, bool)
    got = index.search_grouped(queries, k, allow=none)
    gc.same(got, gc.expected(scores, groups, k, allowed=none), "all masked")
    assert (got[1] == -1).all() and (got[2] == -1).all() and (got[0] == gc.NEG_PAD).all()

    rng = np.random.default_rng(441)
    removed = np.unique(np.concatenate([full[1][:, 0], rng.choice(n, 300, replace=False)]))   # every query's best row
    index.remove_ids(removed)
    allow = rng.random(n) < 0.6
    live = np.ones(n, bool)
    live[removed] = False
    gc.same(index.search_grouped(queries, k), gc.expected(scores, groups, k, allowed=live), "removed")
    gc.same(index.search_grouped(queries, k, allow=allow), gc.expected(scores, groups, k, allowed=live & allow), "removed + allow")


# ---------------------------------------------------------------------------------------------------------------------
# one group larger than every row count the search can rank
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_flood_finishes_through_the_mask_route(gpu):
    corpus, query, groups, scores = gc.one_big_group(1100, 400, 451)
    query = np.array(query)                                  # (the shared cases are read-only)
    index = _index(corpus, gpu, groups=list(groups))
    ref = gc.expected(scores, groups, 3)
    assert ref[2][0, 0] == 0 and (ref[2][0, 1:] > 0).all()
    s, i, g, unproved = index.search_grouped_device(torch.from_numpy(np.array(query)).cuda(), 3, k_rows=K_MAX)
    assert unproved.cpu().tolist() == [1] and index.last_group_counts.cpu().tolist() == [1]
    assert int(index.last_group_n_unproved.item()) == 1
    assert g.cpu().tolist() == [[0, -1, -1]] and i.cpu().numpy()[0, 0] == ref[1][0, 0]
    gc.same(index.search_grouped(query, 3), ref)
    assert index.last_search_path.endswith("+mask"), index.last_search_path
    # a filter of the caller's survives the route's own masking
    allow = np.ones(corpus.shape[0], bool)
    allow[[int(ref[1][0, 0]), int(ref[1][0, 1])]] = False
    gc.same(index.search_grouped(query, 3, allow=allow), gc.expected(scores, groups, 3, allowed=allow), "flood + allow")


@pytest.mark.gpu
def test_doubling_answers_a_hundred_near_copies_without_the_mask_route(gpu):
    corpus, query, groups, scores = gc.one_big_group(100, 400, 461)
    query = np.array(query)
    index = _index(corpus, gpu, groups=list(groups))
    gc.same(index.search_grouped(query, 5), gc.expected(scores, groups, 5))
    assert index.last_search_path == "grouped:doubled128", index.last_search_path


# ---------------------------------------------------------------------------------------------------------------------
# product round trip
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_groups_survive_save_load_add_and_append(gpu, tmp_path):
    from semantic_search_kd_amd import FAISSIndexBuilder

    corpus, queries, groups, scores = gc.runs_of_three()
    queries, scores = queries[:6], scores[:6]
    n, k = corpus.shape[0], 10
    keys = [f"doc{g}" for g in groups]
    index = _index(corpus, gpu, groups=keys)
    ref = gc.expected(scores, groups, k)
    index.save(tmp_path / "a")
    assert (tmp_path / "a" / "groups.npy").exists() and (tmp_path / "a" / "group_keys.json").exists()
    loaded = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu))
    loaded.load(tmp_path / "a")
    got = loaded.search_grouped(queries, k)
    gc.same(got, ref, "after load")
    assert loaded.group_key(got[2][0]) == [keys[i] for i in got[1][0]]
    assert loaded.group_keys == index.group_keys and np.array_equal(loaded.row_groups(), groups)

    # add: with keys (a known key joins its group, also across the call), then without (singletons)
    half = 1000                                             # cuts document 333 in two
    grown = _index(corpus[:half], gpu, groups=keys[:half])
    grown.add(corpus[half:1500], groups=keys[half:1500])
    assert np.array_equal(grown.row_groups(), groups[:1500])
    grown.add(corpus[1500:])
    want = np.concatenate([groups[:1500], groups[1499] + 1 + np.arange(n - 1500)]).astype(np.int32)
    assert np.array_equal(grown.row_groups(), want) and grown.group_key(int(want[-1])) is None
    gc.same(grown.search_grouped(queries, k), gc.expected(scores, want, k), "after add")

    # append: the second part's groups are numbered behind the first's, equal keys are not merged
    first = _index(corpus[:half], gpu, groups=keys[:half])
    _index(corpus[half:], gpu, groups=keys[half:]).save(tmp_path / "b")
    first.load(tmp_path / "b", append=True)
    want = np.concatenate([groups[:half], groups[half:] - groups[half] + groups[half - 1] + 1]).astype(np.int32)
    assert np.array_equal(first.row_groups(), want)
    assert first.group_keys.count("doc333") == 2
    gc.same(first.search_grouped(queries, k), gc.expected(scores, want, k), "after append")

    # an index without groups writes no group files, and takes stale ones away
    plain = _index(corpus[:100], gpu)
    plain.save(tmp_path / "c")
    assert sorted(p.name for p in (tmp_path / "c").iterdir()) == ["doc_ids.json", "index.faiss"]
    plain.save(tmp_path / "a")
    assert not (tmp_path / "a" / "groups.npy").exists() and not (tmp_path / "a" / "group_keys.json").exists()
    # set_groups on stored rows
    plain.set_groups(keys[:100])
    assert np.array_equal(plain.row_groups(), groups[:100]) and plain.n_groups == 34
    gc.same(plain.search_grouped(queries, k), gc.expected(oracle.scores_fma(queries, corpus[:100]), groups[:100], k))
    gc.same(plain.index.search_grouped(queries, k), gc.expected(oracle.scores_fma(queries, corpus[:100]), groups[:100], k))


# ---------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_grouped_search_device_under_graph_capture(gpu):
    corpus, queries, groups, scores = gc.runs_of_three()
    index = _index(corpus, gpu, groups=list(groups))
    keep = np.random.default_rng(471).random(corpus.shape[0]) < 0.7
    flt = index.row_filter(keep)
    ref = gc.expected(scores, groups, 10, allowed=keep, k_rows=28)
    q = torch.from_numpy(np.array(queries)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = index.search_grouped_device(q, 10, allow=flt)       # sizes the workspace, uploads the row groups
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = index.search_grouped_device(q, 10, allow=flt)
    g.replay()
    torch.cuda.synchronize()
    for got in (eager, captured):
        s, i, gr, unproved = (t.cpu().numpy() for t in got)
        assert not unproved.any()
        gc.same((s, i, gr), ref, "graph")
