"""``sskd_range_merge_packed`` on the MI355X: the merge of per-shard range results, through the C-ABI alone.

The inputs are real per-shard outputs: one corpus is cut into W shards, ``sskd_index_range_search`` runs on each with
``id_offset`` = the shard's first global row, the results are packed into records of a common capacity and merged.  The
reference is ONE ``sskd_index_range_search`` over the whole corpus: lims, D and I must be bit-equal."""

import numpy as np
import pytest
import torch

from capi_helpers import stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import _native
from semantic_search_kd_amd.dist import range_record_bytes, range_record_views
from test_range_search_gpu import _past_one_scan_block, _ref_from_scores

DIM = 384
OFFSET = 11   # global id of the corpus' row 0: every shard's id_offset is OFFSET + its first row


def _range(lib, corpus, lo, hi, q, thr):
    """one shard's exact-size sskd_index_range_search output (count-only call, then the full call)"""
    n = hi - lo
    tiled = tile_corpus(lib, corpus[lo:hi]) if n else torch.empty(1, dtype=torch.float32, device="cuda")
    nq = q.shape[0]
    lims = torch.empty(nq + 1, dtype=torch.int64, device="cuda")

    def call(scores, ids, max_results):
        ws = torch.empty(max(int(lib.sskd_index_range_search_workspace_bytes(n, nq, max_results)), 1), dtype=torch.uint8,
                         device="cuda")
        _native.check(lib.sskd_index_range_search(tiled.data_ptr(), n, q.data_ptr(), nq, thr.data_ptr(), OFFSET + lo, None,
                                                  lims.data_ptr(), scores, ids, max_results, ws.data_ptr(), ws.numel(),
                                                  stream()))

    call(None, None, 0)
    total = int(lims[-1].item())
    scores = torch.empty(total, dtype=torch.float32, device="cuda")
    ids = torch.empty(total, dtype=torch.int64, device="cuda")
    if total:
        call(scores.data_ptr(), ids.data_ptr(), total)
    return lims, scores, ids


def _pack(lib, runs, nq, cap):
    rec = int(lib.sskd_range_record_bytes(nq, cap))
    assert rec == range_record_bytes(nq, cap) and rec % 16 == 0
    buf = torch.full((len(runs) * rec,), 0x7F, dtype=torch.uint8, device="cuda")   # padding holds junk
    for r, (lims, scores, ids) in enumerate(runs):
        l, s, i = range_record_views(buf[r * rec : (r + 1) * rec], nq, cap)
        l.copy_(lims)
        s[: scores.numel()].copy_(scores)
        i[: ids.numel()].copy_(ids)
    return buf


SENTINEL_ID, SENTINEL_BITS = -7, 0x7FC00ABC


def _merge(lib, buf, w, nq, cap, max_results, room=None, outputs=True, ws=None):
    """-> (lims, scores, ids) host arrays of ``room`` entries (default max_results + 5); untouched slots keep sentinels.
    ``ws``: the caller's ``(pointer, bytes)`` workspace instead of a fresh buffer of the reported size."""
    room = max_results + 5 if room is None else room
    lims = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
    out_s = torch.full((room,), SENTINEL_BITS, dtype=torch.int32, device="cuda")
    out_i = torch.full((room,), SENTINEL_ID, dtype=torch.int64, device="cuda")
    if ws is None:
        own = torch.empty(max(int(lib.sskd_range_merge_workspace_bytes(w, nq, max_results)), 1), dtype=torch.uint8, device="cuda")
        ws = (own.data_ptr(), own.numel())
    _native.check(lib.sskd_range_merge_packed(buf.data_ptr(), w, nq, cap, lims.data_ptr(),
                                              out_s.data_ptr() if outputs else None, out_i.data_ptr() if outputs else None,
                                              max_results, ws[0], ws[1], stream()))
    torch.cuda.synchronize()
    return lims.cpu().numpy(), out_s.cpu().numpy().view(np.float32), out_i.cpu().numpy()


def _case(n, nq, seed):
    """seeded unit rows with: 3 copies of row 100 in different places (equal scores across shards, ordered by id), a
    row scoring exactly +0.0 and one scoring -0.0 against the last query (e_0), and queries near row 100"""
    corpus = oracle.seeded_unit_rows(n, DIM, seed)
    queries = oracle.seeded_unit_rows(nq, DIM, seed + 1)
    for at in (n // 2 + 3, n - 4, n // 5):
        corpus[at] = corpus[100]
    queries[: nq // 3] = corpus[100] + 0.05 * queries[: nq // 3]
    queries[: nq // 3] /= np.linalg.norm(queries[: nq // 3], axis=1, keepdims=True)
    pos = np.full(DIM, 1 / np.sqrt(DIM - 1), np.float32)
    pos[0] = 0.0
    corpus[300] = pos
    corpus[n - 300] = -pos            # first component -0.0, the rest negative: every product of e_0 is -0.0
    queries[-1] = 0.0
    queries[-1, 0] = 1.0
    return corpus, queries


def _thresholds(s):
    """per query: nothing, 1, ~10, ~1 %, ~50 %, every row, NaN, in turn; the e_0 query takes every row >= 0"""
    n = s.shape[1]
    thr = np.empty(s.shape[0], np.float32)
    for q in range(s.shape[0]):
        desc = np.sort(s[q])[::-1]
        thr[q] = [desc[0], desc[1], desc[min(10, n - 1)], desc[max(n // 100, 1)], desc[n // 2], -np.inf, np.nan][q % 7]
    thr[-1] = -1e-30
    return thr


def _sharded_vs_single(lib, corpus, queries, thr, cuts, extra_cap=3):
    q = torch.from_numpy(queries).cuda()
    t = torch.from_numpy(thr).cuda()
    nq = len(queries)
    runs = [_range(lib, corpus, a, b, q, t) for a, b in zip(cuts, cuts[1:])]
    ref = [x.cpu().numpy() for x in _range(lib, corpus, 0, len(corpus), q, t)]
    cap = max(int(r[0][-1].item()) for r in runs) + extra_cap
    buf = _pack(lib, runs, nq, cap)
    return buf, cap, ref


def _same(got, ref, total, what):
    lims, D, I = got
    assert np.array_equal(lims, ref[0]), (what, np.flatnonzero(lims != ref[0])[:5])
    assert np.array_equal(I[:total], ref[2]), what
    assert np.array_equal(D[:total].view(np.uint32), ref[1].view(np.uint32)), what
    assert (I[total:] == SENTINEL_ID).all() and (D[total:].view(np.uint32) == SENTINEL_BITS).all(), what


CUTS = {
    1: [0, 3001],
    2: [0, 1500, 3001],
    3: [0, 1234, 1234, 3001],                                     # an empty middle shard
    8: [0, 0, 500, 500, 1200, 2000, 2990, 3001, 3001],           # empty first, middle and last shards
}


@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 2, 3, 8])
def test_range_merge_equals_one_range_search(gpu, native_lib, w):
    lib = native_lib
    cuts = CUTS[w]
    corpus, queries = _case(3001, 50, 17)
    s = oracle.scores_fma(queries, corpus)
    thr = _thresholds(s)
    buf, cap, ref = _sharded_vs_single(lib, corpus, queries, thr, cuts)
    total = int(ref[0][-1])
    got = _merge(lib, buf, len(cuts) - 1, len(queries), cap, total)
    _same(got, ref, total, w)
    # the cases the test is meant to hold: empty queries, ties across shards, a signed zero
    counts = np.diff(ref[0])
    assert (counts == 0).any() and (counts == 3001).any()
    tied = ref[2][ref[0][2] : ref[0][3]]   # query 2 (near row 100) takes its top ~10
    assert {OFFSET + 100, OFFSET + 3001 // 2 + 3, OFFSET + 3001 - 4, OFFSET + 3001 // 5} <= set(tied.tolist())
    last = ref[1][ref[0][-2] :]
    assert (last == 0).any(), "the e_0 query matches its zero-score rows"
    # a merge with room to spare writes nothing past the total; the count-only call (NULL outputs) gives the same lims
    _same(_merge(lib, buf, len(cuts) - 1, len(queries), cap, total + 100, room=total + 105), ref, total, "room")
    lims, _, _ = _merge(lib, buf, len(cuts) - 1, len(queries), cap, 0, room=1, outputs=False)
    assert np.array_equal(lims, ref[0])
    # overflow: lims exact, nothing written at all
    lims, D, I = _merge(lib, buf, len(cuts) - 1, len(queries), cap, total - 1)
    assert np.array_equal(lims, ref[0])
    assert (I == SENTINEL_ID).all() and (D.view(np.uint32) == SENTINEL_BITS).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [[0, 30, 64], [0, 20, 20, 64]])
@pytest.mark.parametrize("nq", [4095, 4096, 4097, 8193])
def test_range_merge_lims_past_one_scan_block(gpu, native_lib, nq, cuts):
    """The merged lims come from a scan of 4 096 queries per workgroup: one block not full, one exactly full, one query
    into a second block, one into a third, with 2 and 3 runs of small capacity.  The reference is the host's range
    search of the whole 64-row corpus (``test_range_search_gpu._ref_from_scores`` over its 8 193 x 64 score matrix)."""
    c = _past_one_scan_block()
    thr = c["thr"][:nq]
    ref = _ref_from_scores(c["s"][:nq], thr, OFFSET)
    counts = np.diff(ref[0])
    assert (counts == 0).any() and (counts == 64).any() and len(set(counts.tolist())) >= 6
    q = torch.from_numpy(c["queries"][:nq]).cuda()
    t = torch.from_numpy(thr).cuda()
    runs = [_range(native_lib, c["corpus"], a, b, q, t) for a, b in zip(cuts, cuts[1:])]
    cap = max(int(r[0][-1].item()) for r in runs) + 3
    buf = _pack(native_lib, runs, nq, cap)
    total = int(ref[0][-1])
    _same(_merge(native_lib, buf, len(runs), nq, cap, total), ref, total, (nq, cuts))
    lims, _, _ = _merge(native_lib, buf, len(runs), nq, cap, 0, room=1, outputs=False)
    assert np.array_equal(lims, ref[0])


@pytest.mark.gpu
def test_range_merge_lims_past_256_scan_blocks(gpu, native_lib):
    """256 x 4 096 + 1 queries: the one workgroup that scans the block sums takes 256 of them per trip, so the last
    query's block is the first of its SECOND trip and its offset is the carry of the first.  Two runs of 8.4 MB of
    lims and six records: three queries (the first block, block 200, the last query) hold them."""
    nq, cap = 256 * 4096 + 1, 4
    at = [5, 200 * 4096 + 17, nq - 1]
    # run -> query -> [(score, id)], each list in rank order
    held = [{at[0]: [(0.5, 9), (0.25, 4)], at[2]: [(1.0, 70)]},
            {at[0]: [(0.5, 3)], at[1]: [(2.0, 8)], at[2]: [(1.5, 6)]}]
    rec = range_record_bytes(nq, cap)
    buf = torch.zeros(2 * rec, dtype=torch.uint8, device="cuda")
    for r, per_query in enumerate(held):
        lv, sv, iv = range_record_views(buf[r * rec : (r + 1) * rec], nq, cap)
        counts = torch.zeros(nq, dtype=torch.int64)
        flat = []
        for qq in sorted(per_query):
            counts[qq] = len(per_query[qq])
            flat += per_query[qq]
        lims = torch.zeros(nq + 1, dtype=torch.int64)
        lims[1:] = torch.cumsum(counts, 0)
        lv.copy_(lims)
        sv[: len(flat)].copy_(torch.tensor([x[0] for x in flat], dtype=torch.float32))
        iv[: len(flat)].copy_(torch.tensor([x[1] for x in flat], dtype=torch.int64))
    lims, D, I = _merge(native_lib, buf, 2, nq, cap, 6)
    want = np.zeros(nq + 1, np.int64)
    want[at[0] + 1:] += 3
    want[at[1] + 1:] += 1
    want[at[2] + 1:] += 2
    assert np.array_equal(lims, want), np.flatnonzero(lims != want)[:5]
    assert lims[nq - 1] == 4 and lims[nq] == 6
    assert I[:6].tolist() == [3, 9, 4, 8, 6, 70] and D[:6].tolist() == [0.5, 0.5, 0.25, 2.0, 1.5, 1.0]
    assert (I[6:] == SENTINEL_ID).all()


@pytest.mark.gpu
def test_range_merge_segments_longer_than_the_lds_sort(gpu, native_lib):
    """a query matching every row: segments of 40 000 keys (> 16 384) in the single call and 13 000+ per run"""
    corpus, queries = _case(40000, 4, 5)
    s = oracle.scores_fma(queries, corpus)
    thr = np.array([-np.inf, np.median(s[1]), np.nan, -1e-30], np.float32)
    cuts = [0, 13001, 26500, 40000]
    buf, cap, ref = _sharded_vs_single(native_lib, corpus, queries, thr, cuts, extra_cap=0)
    total = int(ref[0][-1])
    assert ref[0][1] == 40000 and ref[0][3] == ref[0][2]
    _same(_merge(native_lib, buf, 3, 4, cap, total), ref, total, "long")


@pytest.mark.gpu
def test_range_merge_orders_signed_zeros_and_ties(gpu, native_lib):
    """hand-made records: +0.0 ranks before -0.0 whatever the ids; equal scores go by id across runs"""
    nq, cap = 2, 3
    runs = [
        ([0, 1, 3], [0.0, 0.5, -0.0], [9, 4, 6]),
        ([0, 1, 3], [-0.0, 0.5, 0.0], [1, 3, 8]),
        ([0, 0, 0], [], []),
    ]
    rec = range_record_bytes(nq, cap)
    buf = torch.zeros(len(runs) * rec, dtype=torch.uint8, device="cuda")
    for r, (l, s, i) in enumerate(runs):
        lv, sv, iv = range_record_views(buf[r * rec : (r + 1) * rec], nq, cap)
        lv.copy_(torch.tensor(l))
        sv[: len(s)].copy_(torch.tensor(s, dtype=torch.float32))
        iv[: len(i)].copy_(torch.tensor(i, dtype=torch.int64))
    lims, D, I = _merge(native_lib, buf, len(runs), nq, cap, 6)
    assert lims.tolist() == [0, 2, 6]
    assert I[:6].tolist() == [9, 1, 3, 4, 8, 6]
    assert D[:6].tolist() == [0.0, 0.0, 0.5, 0.5, 0.0, 0.0]
    assert np.signbit(D[:6]).tolist() == [False, True, False, False, False, True]


@pytest.mark.gpu
def test_range_merge_no_queries_and_argument_errors(gpu, native_lib):
    lib = native_lib
    nq, cap = 4, 8
    rec = range_record_bytes(nq, cap)
    buf = torch.zeros(2 * rec, dtype=torch.uint8, device="cuda")
    lims = torch.full((nq + 1,), -5, dtype=torch.int64, device="cuda")
    out_s = torch.empty(16, dtype=torch.float32, device="cuda")
    out_i = torch.empty(16, dtype=torch.int64, device="cuda")
    need = int(lib.sskd_range_merge_workspace_bytes(2, nq, 16))
    assert need > 0 and int(lib.sskd_range_merge_workspace_bytes(2, 0, 16)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = stream()

    def call(records=buf.data_ptr(), n_runs=2, nq_=nq, cap_=cap, lims_=lims.data_ptr(), s=out_s.data_ptr(),
             i=out_i.data_ptr(), max_results=16, ws_=ws.data_ptr(), ws_bytes=need):
        return lib.sskd_range_merge_packed(records, n_runs, nq_, cap_, lims_, s, i, max_results, ws_, ws_bytes, st)

    invalid, workspace = 1, 2
    assert call(n_runs=0) == invalid
    assert call(n_runs=65536) == invalid
    assert call(nq_=-1) == invalid
    assert call(cap_=-1) == invalid
    assert call(max_results=-1) == invalid
    assert call(records=None) == invalid
    assert call(lims_=None) == invalid
    assert call(records=buf.data_ptr() + 4) == invalid
    assert call(s=None) == invalid and call(i=None) == invalid
    assert call(ws_bytes=need - 1) == workspace
    assert call(ws_=None) == workspace
    assert b"workspace" in lib.sskd_last_error()
    torch.cuda.synchronize()
    assert (lims.cpu() == -5).all(), "a refused call wrote lims"
    # the valid call over two empty records: zero lims; nq = 0 writes lims[0] only and needs no workspace
    assert call() == 0
    torch.cuda.synchronize()
    assert lims.cpu().tolist() == [0] * (nq + 1)
    lims.fill_(-5)
    assert call(nq_=0, ws_=None, ws_bytes=0, s=None, i=None, max_results=0) == 0
    torch.cuda.synchronize()
    assert lims.cpu().tolist() == [0] + [-5] * nq
