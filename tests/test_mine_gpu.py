"""Hard-negative mining on the MI355X: ``sskd_index_mine_select`` behind ``FAISSIndexBuilder.mine_negatives`` and
``ANCEMiner.mine_from_index`` (``include/sskd_amd.h``).

The oracle (``mine_cases.py``): the project's own ``select_adversarial``, applied on the host to the ranking ``search``
returned on the GPU, with the positive scores from ``sskd_similarity`` over the stored rows - what
``ANCEMiner._mine_from_index_host`` computes.  Every comparison is exact: ids, scores as bits, counts.  Shapes are the
smallest at which the kernel can go wrong: a round is 64 ranks / 64 positives, a workgroup holds several waves, the
screened search needs 2 048 rows and 64 queries.  One index per corpus and module.
"""
import zlib

import numpy as np
import pytest
import torch

import mine_cases as mc
import ranking_walk_cases as rw
from capi_helpers import stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import _native

DIM = mc.DIM
OFFSET = 1_000_000_007
SENT_S, SENT_I, SENT_C = 12345.0, -77, -55

_indexes = {}
_similarity = {}


def _index(gpu, name, corpus, **kwargs):
    from semantic_search_kd_amd import FAISSIndexBuilder

    if name not in _indexes:
        index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu), id_offset=kwargs.pop("id_offset", 0))
        index.build_from_embeddings(np.array(corpus), **kwargs)
        _indexes[name] = index
    return _indexes[name]


def _scores(lib, name, index, queries):
    """sskd_similarity of every query against the stored rows: the positive scores of the oracle"""
    if name not in _similarity:
        rows = torch.from_numpy(index.to_numpy()).cuda()
        q = torch.from_numpy(np.array(queries, np.float32)).cuda()
        out = torch.empty((q.shape[0], rows.shape[0]), dtype=torch.float32, device="cuda")
        _native.check(lib.sskd_similarity(q.data_ptr(), q.shape[0], rows.data_ptr(), rows.shape[0], DIM, out.data_ptr(), stream()))
        _similarity[name] = out.cpu().numpy()
    return _similarity[name]


def _ranking(index, queries, search_k, allow=None):
    """the ranking ``search`` returns on the GPU, in local rows"""
    D, I = index.search(np.array(queries), search_k, allow=allow)
    return D, np.where(I >= 0, I - index.id_offset, -1)


def _host(got):
    return tuple(t.cpu().numpy() for t in got)


# ---------------------------------------------------------------------------------------------------------------------
# rounds of 64 ranks and of 64 positives, top_k inside a round, padding, counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("margin", [0.1, 0.05, 0.0])
@pytest.mark.parametrize("search_k", [1, 64, 65, 100])
def test_mixed_positives_at_every_round_boundary(gpu, native_lib, search_k, margin):
    corpus, queries, _, lims, rows = mc.mixed()
    index = _index(gpu, "mixed", corpus)
    S = _scores(native_lib, "mixed", index, queries)
    D, I = _ranking(index, queries, search_k)
    for top_k in sorted({1, min(5, search_k), search_k}):
        ref = mc.expected(D, I, lims, rows, S, margin, top_k)
        got = index.mine_negatives(np.array(queries), (lims, rows), top_k=top_k, search_k=search_k, margin=margin)
        mc.same(got, ref, (search_k, margin, top_k))
    if search_k == 100:
        ref = mc.expected(D, I, lims, rows, S, margin, 5)
        if margin == 0.1:
            assert (ref[2] > 5).any(), "counts above top_k are reported"
        elif margin == 0.05:
            assert len(set(ref[2].tolist())) > 10, "the threshold falls inside the window"
        else:
            assert ((ref[2] > 0) & (ref[2] < 5)).any() and (ref[1] == -1).any(), "fewer survivors than top_k: padding"
        # the list form, unsorted and with repeats, is the same call
        lists = [rows[lims[q]:lims[q + 1]][::-1].tolist() * 2 for q in range(70)]
        mc.same(index.mine_negatives(np.array(queries), lists, top_k=5, search_k=100, margin=margin), ref, "lists")


@pytest.mark.gpu
def test_capi_writes_nothing_past_top_k_or_the_last_query(gpu, native_lib):
    corpus, queries, _, lims, rows = mc.mixed()
    index = _index(gpu, "mixed", corpus)
    S = _scores(native_lib, "mixed", index, queries)
    nq, search_k, top_k = 70, 100, 5
    q = torch.from_numpy(np.array(queries)).cuda()
    rs, ri = index.search_device(q, search_k)
    # outputs one query longer than the call's (the row stride is top_k, so there is no guard column: a write past
    # top_k inside query q would land in query q + 1's row and show in the exact comparison, and behind the last query
    # - whose count is above top_k - in the sentinels)
    sc = torch.full((nq * top_k + top_k,), SENT_S, dtype=torch.float32, device="cuda")
    ids = torch.full((nq * top_k + top_k,), SENT_I, dtype=torch.int64, device="cuda")
    cnt = torch.full((nq + 1,), SENT_C, dtype=torch.int32, device="cuda")
    mp = torch.full((nq + 1,), SENT_S, dtype=torch.float32, device="cuda")
    # the device form takes the positives in any order: the best one goes last (the second round of 65 positives)
    lists = [rows[lims[j]:lims[j + 1]] for j in range(nq)]
    lists = [x[np.argsort(S[j, x], kind="stable")] for j, x in enumerate(lists)]
    dl, dr = (torch.from_numpy(a).cuda() for a in mc.csr(lists))
    _native.check(native_lib.sskd_index_mine_select(
        index._tiled.data_ptr(), index.ntotal, q.data_ptr(), nq, rs.data_ptr(), ri.data_ptr(), search_k, dl.data_ptr(),
        dr.data_ptr(), None, 0.1, top_k, OFFSET, sc.data_ptr(), ids.data_ptr(), cnt.data_ptr(), mp.data_ptr(), stream()))
    torch.cuda.synchronize()
    sc, ids, cnt, mp = (t.cpu().numpy() for t in (sc, ids, cnt, mp))
    assert (sc[nq * top_k:] == np.float32(SENT_S)).all() and (ids[nq * top_k:] == SENT_I).all()
    assert cnt[nq] == SENT_C and mp[nq] == np.float32(SENT_S), "wrote past the last query"
    ref = mc.expected(rs.cpu().numpy(), ri.cpu().numpy(), lims, rows, S, 0.1, top_k, id_offset=OFFSET)
    mc.same((sc[: nq * top_k].reshape(nq, top_k), ids[: nq * top_k].reshape(nq, top_k), cnt[:nq], mp[:nq]), ref, "capi")
    assert (ref[2] > top_k).any()


@pytest.mark.gpu
def test_id_offset_shifts_the_ids_out_not_the_positives_in(gpu, native_lib):
    corpus, queries, _, lims, rows = mc.mixed()
    base = _index(gpu, "mixed", corpus)
    index = _index(gpu, "mixed+offset", corpus, id_offset=OFFSET)
    S = _scores(native_lib, "mixed", base, queries)
    D, I = _ranking(index, queries, 100)
    ref = mc.expected(D, I, lims, rows, S, 0.1, 5, id_offset=OFFSET)
    got = index.mine_negatives(np.array(queries), (lims, rows), top_k=5, search_k=100, margin=0.1)
    mc.same(got, ref, "offset")
    plain = base.mine_negatives(np.array(queries), (lims, rows), top_k=5, search_k=100, margin=0.1)
    assert np.array_equal(got[1], np.where(plain[1] >= 0, plain[1] + OFFSET, -1)) and np.array_equal(got[2], plain[2])


# ---------------------------------------------------------------------------------------------------------------------
# the walk itself, on hand-made rankings
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("width", rw.WIDTHS)
def test_capi_walk_ends_on_any_negative_id_and_cuts_the_lanes_behind_it(gpu, native_lib, width):
    """This kernel's row of the table in ``csrc/ranking_walk.h``: ANY negative id ends the ranking (the other walks
    skip -9 and end on -1 alone), ids at or above ``n_rows`` are skipped, nothing behind the end is kept."""
    n, nq = 200, rw.NQ
    corpus = oracle.seeded_unit_rows(n, DIM, 661)
    queries = oracle.seeded_unit_rows(nq, DIM, 662)
    S = oracle.scores_fma(queries, corpus)
    I = rw.ids(n, width)
    D = rw.descending_scores(width, low=-0.5, high=0.9)
    # one positive per query: the row at rank 1 (rank 0 of a one-wide ranking) where that is a row, else row 7
    pos = [int(I[q, min(1, width - 1)]) for q in range(nq)]
    pos = [r if 0 <= r < n else 7 for r in pos]
    lims, rows = mc.csr([[r] for r in pos])
    groups = (np.arange(n) // 3).astype(np.int32)
    tiled = tile_corpus(native_lib, corpus)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dq, ds, di, dl, dr, dg = d(queries), d(D), d(I), d(lims), d(rows), d(groups)
    for by_group in (False, True):
        for margin in (10.0, 0.3):
            for top_k in sorted({1, min(5, width), width}):
                sc = torch.full((nq + 1, top_k), SENT_S, dtype=torch.float32, device="cuda")
                ids = torch.full((nq + 1, top_k), SENT_I, dtype=torch.int64, device="cuda")
                cnt = torch.full((nq + 1,), SENT_C, dtype=torch.int32, device="cuda")
                mp = torch.full((nq + 1,), SENT_S, dtype=torch.float32, device="cuda")
                _native.check(native_lib.sskd_index_mine_select(
                    tiled.data_ptr(), n, dq.data_ptr(), nq, ds.data_ptr(), di.data_ptr(), width, dl.data_ptr(),
                    dr.data_ptr(), dg.data_ptr() if by_group else None, margin, top_k, OFFSET, sc.data_ptr(),
                    ids.data_ptr(), cnt.data_ptr(), mp.data_ptr(), stream()))
                torch.cuda.synchronize()
                sc, ids, cnt, mp = (t.cpu().numpy() for t in (sc, ids, cnt, mp))
                assert (sc[nq] == np.float32(SENT_S)).all() and (ids[nq] == SENT_I).all()
                assert cnt[nq] == SENT_C and mp[nq] == np.float32(SENT_S), "wrote past the last query"
                ref = [mc.walk(D[q], I[q], [pos[q]], S[q, pos[q]], margin, top_k, groups if by_group else None, OFFSET,
                               n_rows=n) for q in range(nq)]
                ref = (np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]),
                       np.array([r[2] for r in ref], np.int32), np.array([r[3] for r in ref], np.float32))
                mc.same((sc[:nq], ids[:nq], cnt[:nq], mp[:nq]), ref, (width, by_group, margin, top_k))
                if margin == 10.0 and not by_group:
                    # every walked row but the positive survives: the counts say where each walk ended
                    ended = [int(np.flatnonzero(I[q] < 0)[0]) if (I[q] < 0).any() else width for q in range(nq)]
                    walked = [sum(1 for r in I[q, :ended[q]] if r < n and r != pos[q]) for q in range(nq)]
                    assert ref[2].tolist() == walked
                    if width >= 63:
                        assert ended[1] == 3 and ended[2] == 63 and ended[4] == 2, "-9 ends this walk"
                        assert ref[2][4] == 1 and ref[2][0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# threshold ties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_copies_of_a_positive_sit_on_the_threshold(gpu, native_lib):
    corpus, queries, _, lims, rows, copies = mc.duplicates()
    index = _index(gpu, "duplicates", corpus)
    S = _scores(native_lib, "duplicates", index, queries)
    D, I = _ranking(index, queries, 100)
    got = {}
    for margin in (0.0, -1e-9, 0.1):
        got[margin] = index.mine_negatives(np.array(queries), (lims, rows), top_k=100, search_k=100, margin=margin)
        mc.same(got[margin], mc.expected(D, I, lims, rows, S, margin, 100), margin)
    for q in (0, 1):
        assert set(copies[q]) <= set(got[0.0][1][q].tolist()), "margin=0.0: exactly on max_pos is kept"
        assert not set(copies[q]) & set(got[-1e-9][1][q].tolist()), "margin=-1e-9: dropped, in fp64"
        assert got[0.0][2][q] == got[-1e-9][2][q] + 3
    assert got[-1e-9][2][0] == 0 and (got[-1e-9][1][0] == -1).all()


@pytest.mark.gpu
def test_margin_decides_in_fp64_not_fp32(gpu, native_lib):
    corpus, queries, _, lims, rows, (d32, drounded) = mc.threshold_neighbours()
    index = _index(gpu, "neighbours", corpus)
    S = _scores(native_lib, "neighbours", index, queries)
    D, I = _ranking(index, queries, 150)
    got = index.mine_negatives(np.array(queries), (lims, rows), top_k=150, search_k=150, margin=0.1)
    mc.same(got, mc.expected(D, I, lims, rows, S, 0.1, 150), "neighbours")
    in64, in32, rounded = mc.decisions(S[0], S[0, 0], 0.1)
    kept = set(got[1][0, : got[2][0]].tolist())
    assert kept == set((1 + np.flatnonzero(in64[1:])).tolist())
    assert (in64 != in32)[1:130].any() and (in64 != rounded)[1:130].any(), "the case must tell the arithmetics apart"


# ---------------------------------------------------------------------------------------------------------------------
# groups, hidden rows, search paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_by_group_drops_the_sibling_chunks_of_a_positive(gpu, native_lib):
    corpus, queries, _, groups, lims, rows = mc.chunked()
    index = _index(gpu, "chunked", corpus, groups=groups.tolist())
    S = _scores(native_lib, "chunked", index, queries)
    D, I = _ranking(index, queries, 100)
    on = index.mine_negatives(np.array(queries), (lims, rows), top_k=10, search_k=100, margin=0.8, by_group=True)
    off = index.mine_negatives(np.array(queries), (lims, rows), top_k=10, search_k=100, margin=0.8)
    mc.same(on, mc.expected(D, I, lims, rows, S, 0.8, 10, groups), "by_group")
    mc.same(off, mc.expected(D, I, lims, rows, S, 0.8, 10), "rows")
    pos_group = groups[rows]
    siblings_off = sum(int((groups[off[1][q][off[1][q] >= 0]] == pos_group[q]).sum()) for q in range(70))
    siblings_on = sum(int((groups[on[1][q][on[1][q] >= 0]] == pos_group[q]).sum()) for q in range(70))
    assert siblings_on == 0 and siblings_off >= 70, (siblings_on, siblings_off)
    # no groups set: every row is its own group, by_group changes nothing
    mixed = _index(gpu, "mixed", mc.mixed()[0])
    _, mq, _, ml, mr = mc.mixed()
    a = mixed.mine_negatives(np.array(mq), (ml, mr), by_group=True)
    mc.same(a, mixed.mine_negatives(np.array(mq), (ml, mr)), "no groups")


@pytest.mark.gpu
def test_hidden_rows_never_come_back_but_a_hidden_positive_still_scores(gpu, native_lib):
    corpus, queries, _, lims, rows = mc.mixed()
    index = _index(gpu, "mixed+removed", corpus)
    S = _scores(native_lib, "mixed", _index(gpu, "mixed", corpus), queries)
    has_pos = np.flatnonzero(np.diff(lims) == 1)
    # the single positive of these queries is their rank-2 row: remove it, and the best row of every query
    D, I = _ranking(index, queries, 3)
    removed = np.unique(np.concatenate([rows[lims[has_pos]], I[:, 0]]))
    if index.n_removed == 0:
        index.remove_ids(removed)
    allow = np.random.default_rng(641).random(corpus.shape[0]) < 0.7
    hidden = set(removed.tolist()) | set(np.flatnonzero(~allow).tolist())
    for flt in (None, allow):
        D, I = _ranking(index, queries, 100, allow=flt)
        got = index.mine_negatives(np.array(queries), (lims, rows), top_k=100, search_k=100, margin=0.1, allow=flt)
        mc.same(got, mc.expected(D, I, lims, rows, S, 0.1, 100), "hidden")
        out = set(got[1][got[1] >= 0].tolist())
        assert not out & (set(removed.tolist()) if flt is None else hidden)
        for q in has_pos:
            assert got[3][q] == S[q, rows[lims[q]]], "a removed positive still sets max_pos"


@pytest.mark.gpu
def test_screened_and_exact_search_give_the_same_negatives(gpu, native_lib):
    corpus, queries, _, lims, rows = mc.mixed()
    index = _index(gpu, "mixed", corpus)
    S = _scores(native_lib, "mixed", index, queries)
    q = torch.from_numpy(np.array(queries)).cuda()
    dl, dr = torch.from_numpy(np.array(lims)).cuda(), torch.from_numpy(np.array(rows)).cuda()
    assert index.screening
    screened = _host(index.mine_negatives_device(q, dl, dr, top_k=5, search_k=10, margin=0.1))
    assert index.last_status is not None, "10 results for 70 queries over 2 083 rows take the screened path"
    index.screening = False
    try:
        exact = _host(index.mine_negatives_device(q, dl, dr, top_k=5, search_k=10, margin=0.1))
        assert index.last_status is None
    finally:
        index.screening = True
    D, I = _ranking(index, queries, 10)
    ref = mc.expected(D, I, lims, rows, S, 0.1, 5)
    mc.same(screened, ref, "screened")
    mc.same(exact, ref, "exact")


@pytest.mark.gpu
def test_graph_capture_and_replay_equal_the_eager_call(gpu, native_lib):
    corpus, queries, _, lims, rows = mc.mixed()
    index = _index(gpu, "mixed", corpus)
    S = _scores(native_lib, "mixed", index, queries)
    D, I = _ranking(index, queries, 100)
    ref = mc.expected(D, I, lims, rows, S, 0.1, 5)
    q = torch.from_numpy(np.array(queries)).cuda()
    dl, dr = torch.from_numpy(np.array(lims)).cuda(), torch.from_numpy(np.array(rows)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = index.mine_negatives_device(q, dl, dr, top_k=5, search_k=100, margin=0.1)   # sizes the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = index.mine_negatives_device(q, dl, dr, top_k=5, search_k=100, margin=0.1)
    g.replay()
    torch.cuda.synchronize()
    mc.same(_host(eager), ref, "eager")
    mc.same(_host(captured), ref, "graph")


# ---------------------------------------------------------------------------------------------------------------------
# ANCEMiner
# ---------------------------------------------------------------------------------------------------------------------
class _WordStudent:
    """Stand-in student: a text embeds as the normalised sum of its words' seeded vectors, so texts sharing words score
    high; ``compute_similarity`` is the product's (``sskd_similarity``)."""

    device = "cuda:0"

    def __init__(self, lib):
        self.lib = lib
        self._words = {}

    def _word(self, w):
        if w not in self._words:
            g = np.random.Generator(np.random.PCG64(zlib.crc32(w.encode())))
            self._words[w] = g.standard_normal(DIM)
        return self._words[w]

    def _emb(self, texts):
        out = np.stack([np.sum([self._word(w) for w in t.split()] or [self._word("")], axis=0) for t in texts])
        return (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(np.float32)

    encode_queries = encode_documents = lambda self, texts, **kw: self._emb(list(texts))

    def compute_similarity(self, q, d):
        qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        dd = torch.from_numpy(np.ascontiguousarray(d, np.float32)).cuda()
        out = torch.empty((qd.shape[0], dd.shape[0]), dtype=torch.float32, device="cuda")
        _native.check(self.lib.sskd_similarity(qd.data_ptr(), qd.shape[0], dd.data_ptr(), dd.shape[0], DIM, out.data_ptr(), stream()))
        return out.cpu().numpy()


@pytest.mark.gpu
def test_ance_miner_equals_its_host_loop(gpu, native_lib):
    from semantic_search_kd_amd import ANCEMiner

    rng = np.random.default_rng(651)
    words = [f"w{i}" for i in range(60)]
    texts = [" ".join(rng.choice(words, size=int(rng.integers(3, 9)))) for _ in range(400)]
    ids = [f"d{i}" for i in range(400)]
    ids[123], texts[123] = ids[7], texts[7]           # one doc id on two rows (the same text)
    queries = [" ".join(rng.choice(words, size=4)) for _ in range(70)]
    positives = [[ids[int(j)] for j in rng.choice(400, size=int(rng.integers(0, 4)), replace=False)] for _ in queries]
    positives[0] = ["d7", "not-in-the-corpus"]
    positives[1] = []
    index = None
    for margin in (0.1, 0.0):
        miner = ANCEMiner(_WordStudent(native_lib), margin=margin)
        miner.refresh(ids, texts)
        for top_k, search_k in ((5, 100), (3, 64), (5, 1000)):
            got = miner.mine_from_index(queries, positives, top_k=top_k, search_k=search_k)
            want = miner._mine_from_index_host(queries, positives, top_k=top_k, search_k=search_k)
            assert got == want, (margin, top_k, search_k)
            assert all("d7" not in neg for neg, pos in zip(got, positives) if "d7" in pos)
        assert any(got) and (margin != 0.0 or any(len(x) < 5 for x in got))
        index = miner._index
    # the device form: the same rows, nothing leaves HBM
    q = torch.from_numpy(miner.student.encode_queries(queries)).cuda()
    lists = [[r for d in pos for r in miner._rows_of_id.get(d, ())] for pos in positives]
    lims, rows = mc.csr([sorted(x) for x in lists])
    D, I, counts, max_pos = miner.mine_from_index_device(q, torch.from_numpy(lims).cuda(), torch.from_numpy(rows).cuda())
    assert I.is_cuda and [[ids[r] for r in row if r >= 0] for row in I.cpu().tolist()] == miner.mine_from_index(queries, positives)
    assert miner.mine_from_index([], []) == [] and index.ntotal == 400
