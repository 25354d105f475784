"""The index kernels past their 32-bit offset boundaries, on the MI355X (cases and references: ``high_rows_cases``;
that the cases can fail is shown on the CPU by ``test_high_rows_host.py``).

The index is ``torch.zeros`` of the full size with a few dozen planted rows on both sides of every boundary; every
comparison is bit for bit against the compressed references.  A kernel that reads a high row through a truncated
offset lands on zeros (or outside the buffer): a planted score turns into 0 and the comparison fails.  Twelve booster
rows in the first tiles (``high_rows_cases.BOOSTER_ROWS``) give the screened search a pruning bound above its error
band; the screened tests assert that not every query took the in-call exact scan.

Tier 1: 5 600 021 rows (8.0 GiB + a 4.0 GiB sidecar), boundaries A = row 1 398 101 (2^31 bytes), B = 2 796 202 (2^32
bytes), C = 5 592 405 (2^31 floats).  Tier 2: 22 400 021 rows (32.0 GiB), adds D = 11 184 810 (2^32 floats) and
E = 22 369 621 (2^31 float4).  The two are never resident together; tier 2 is skipped only when less than 40 GB are free.

Which planted rows an entry point READS, by boundary ("x": every planted row on both sides of it) - the table the
tests below implement, one test per line:

    entry point                                   A  B  C  D  E   how the rows are reached
    --------------------------------------------  -- -- -- -- --  --------------------------------------------------
    sskd_index_add_rows (high dst_row0)           x  x  x  x  x   the fixture writes every planted block through it
    sskd_index_get_rows                           x  x  x  x  x   row0 before, n_rows across every boundary
    sskd_l2_normalize_rows                        x  x  x  .  .   in place on the compacted copy (and on the last tiles)
    sskd_similarity (nd = n)                      x  x  x  .  .   every column
    sskd_index_search, _ex, k = 10 and 100        x  x  x  x  x   whole scan; every planted row leads a query
    sskd_index_search_onepass                     x  x  x  x  x   whole scan
    sskd_index_search_screened, _claim (0 / 1)    x  x  x  .  .   sidecar scan + exact re-scoring gathers
    sskd_index_search_filtered, _screened_, _onepass_filtered
                                                  x  x  x  x* x*  mask words of the high tiles (* exact scan only)
    sskd_index_range_search                       x  x  x  x  x   whole scan, per-query thresholds
    sskd_index_search_grouped                     x  x  x  .  .   whole scan + d_row_group of the high rows
    sskd_row_mask_rank + sskd_index_compact_rows  x  x  x  .  .   source and destination both cross
    sskd_ivf_search                               x  x  x  x  x   RowStage gathers of the lists around each boundary
    sskd_ivf_list_sums                            x  x  x  .  .   every list
    sskd_pq_encode, sskd_pq_code_sums             x  x  x  .  .   every row encoded; group lists name every planted row
    sskd_pq_search (refine = 64)                  x  x  x  .  .   ADC scan of the codes, RowStage gathers of the candidates
    sskd_graph_search                             x  x  x  x  x   RowStage gathers along a ring over the planted rows
    sskd_graph_link                               x  x  x  .  .   touched rows on both sides
    sskd_index_mine_select                        x  x  x  x  x   positives
    sskd_hybrid_fuse (linear)                     x  x  x  x  x   rows the dense list lacks
    sskd_prf_rocchio                              x  x  x  x  x   feedback rows
    sskd_mmr_select                               x  x  x  x  x   candidate rows
    sskd_late_pack_tokens, sskd_late_rerank       token store of 5 600 021 tokens: 2^31 bytes, 2^32 bytes = 2^31 elements

id_offset = 2^40 + 7 goes through every entry point above that takes one (``test_tier1_id_offset``).
What is still not covered, and the size it would need: DESIGN.md, "High-row coverage".
"""
import ctypes as C

import numpy as np
import pytest
import torch

import high_rows_cases as hr
from capi_helpers import stream
from oracle import search as oracle
from semantic_search_kd_amd import _native

pytestmark = pytest.mark.gpu

DIM, TILE = hr.DIM, hr.TILE
TIER2_MIN_FREE = 40 * 10 ** 9
SENT_S, SENT_I = 12345.0, -77


def _dev(a):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_topk(got, ref, what):
    assert np.array_equal(got[1], ref[1]), (what, "ids", np.argwhere(got[1] != ref[1])[:3].tolist(),
                                            got[1][got[1] != ref[1]][:3].tolist(), ref[1][got[1] != ref[1]][:3].tolist())
    assert np.array_equal(_bits(got[0]), _bits(ref[0])), (what, "scores", np.argwhere(_bits(got[0]) != _bits(ref[0]))[:3].tolist())


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")


def _outs(nq, k):
    return (torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda"),
            torch.full((nq, k), -7, dtype=torch.int64, device="cuda"))


def _nonzero_rows(buf, n_rows, width):
    """row numbers of a device matrix ``[n_rows, width]`` of 4-byte words that hold a non-zero word, found on the
    device a million rows at a time (the temporary is one byte per word of the chunk)"""
    words = buf.view(-1).view(torch.int32)[: n_rows * width].view(n_rows, width)
    found = []
    for lo in range(0, n_rows, 1 << 20):
        hit = (words[lo: lo + (1 << 20)] != 0).any(dim=1).nonzero().flatten()
        if hit.numel():
            found.append(hit + lo)
    return torch.cat(found).cpu().numpy() if found else np.zeros(0, np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the tiers on the device
# ---------------------------------------------------------------------------------------------------------------------
class Tier:
    """The zeroed buffer with the planted rows written through ``sskd_index_add_rows`` in 32-row blocks at their
    ``dst_row0``, the queries, and (tier 1) the bf16 sidecar."""

    def __init__(self, lib, which, sidecar):
        self.lib, self.which, self.sp = lib, which, hr.tier(which)
        sp = self.sp
        self.n = sp.n
        assert int(lib.sskd_index_tiled_bytes(sp.n)) == sp.padded * hr.ROW_BYTES
        self.tiled = torch.zeros(sp.padded * DIM, dtype=torch.float32, device="cuda")
        for row0, block in sp.blocks():
            d = _dev(block)
            _native.check(lib.sskd_index_add_rows(d.data_ptr(), min(TILE, sp.n - row0), 0, self.tiled.data_ptr(), row0, stream()))
        torch.cuda.synchronize()
        self.queries = hr.main_queries(sp)
        self.q = _dev(self.queries)
        self.bf = None
        if sidecar:
            self.bf = torch.empty(int(lib.sskd_index_bf16_bytes(sp.n)), dtype=torch.uint8, device="cuda")
            _native.check(lib.sskd_index_make_bf16(self.tiled.data_ptr(), sp.n, self.bf.data_ptr(), stream()))
            torch.cuda.synchronize()
        self.cache = {}

    def mask(self, cleared):
        """device mask words: all ones but the ``cleared`` rows"""
        words = torch.full((-(-self.n // 32),), -1, dtype=torch.int32, device="cuda")
        at, vals = hr.mask_edits(self.n, cleared)
        words[_dev(at)] = _dev(vals)
        return words

    def drop(self):
        self.tiled = self.bf = self.q = None
        self.cache.clear()
        torch.cuda.empty_cache()


_resident = {}


def _make(lib, which, sidecar):
    for other in list(_resident):          # the two tiers are never resident together
        _resident.pop(other).drop()
    torch.cuda.empty_cache()
    _resident[which] = Tier(lib, which, sidecar)
    return _resident[which]


@pytest.fixture(scope="module")
def tier1(gpu, native_lib):
    T = _make(native_lib, 1, sidecar=True)
    yield T
    T.drop()
    _resident.pop(1, None)


@pytest.fixture(scope="module")
def tier2(gpu, native_lib):
    for other in list(_resident):
        _resident.pop(other).drop()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < TIER2_MIN_FREE:
        reason = f"tier 2 needs 40 GB of free device memory, {free / 1e9:.1f} GB are free"
        print(reason)
        pytest.skip(reason)
    T = _make(native_lib, 2, sidecar=False)
    yield T
    T.drop()
    _resident.pop(2, None)


# ---------------------------------------------------------------------------------------------------------------------
# the calls (shared by the tiers and by the id_offset test)
# ---------------------------------------------------------------------------------------------------------------------
def run_writers_readers(T):
    sp, lib = T.sp, T.lib
    # the whole buffer, compared on the device: non-zero exactly in the planted rows, which hold the planted bits
    nz = _nonzero_rows(T.tiled, sp.padded, DIM)
    assert np.array_equal(nz, sp.rows), ("non-zero rows", np.setxor1d(nz, sp.rows)[:8].tolist())
    got = T.tiled.view(sp.padded, DIM)[_dev(sp.rows)].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(sp.values)), "planted bits"
    # get_rows: from 40 rows before every boundary, 100 rows across it; and the ragged tail
    for b in sp.boundaries + (sp.n - 60,):
        row0, cnt = b - 40, min(100, sp.n - (b - 40))
        out = torch.full((cnt + 1, DIM), SENT_S, dtype=torch.float32, device="cuda")
        _native.check(lib.sskd_index_get_rows(T.tiled.data_ptr(), row0, cnt, out.data_ptr(), stream()))
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        want = np.zeros((cnt, DIM), np.float32)
        inside = (sp.rows >= row0) & (sp.rows < row0 + cnt)
        want[sp.rows[inside] - row0] = sp.values[inside]
        assert inside.sum() >= 3 and np.array_equal(_bits(out[:cnt]), _bits(want)), ("get_rows", b)
        assert (out[cnt] == np.float32(SENT_S)).all(), "get_rows wrote past its last row"


def run_exact(T, entry, k, id_offset=0, cleared=None, queries=None, tuning=None):
    """one exact-family entry point over the main queries (or ``queries``): host (scores, ids)"""
    lib, n = T.lib, T.n
    q = T.q if queries is None else _dev(queries)
    nq = q.shape[0]
    mask = None if cleared is None else T.mask(cleared)
    mp = None if mask is None else mask.data_ptr()
    out_s, out_i = _outs(nq, k)
    tn = None if tuning is None else _native.SearchTuning(*tuning)
    tp = None if tn is None else C.byref(tn)
    if entry == "search":
        ws = _ws(lib.sskd_index_search_workspace_bytes(n, nq, k))
        rc = lib.sskd_index_search(T.tiled.data_ptr(), n, q.data_ptr(), nq, k, id_offset, out_s.data_ptr(), out_i.data_ptr(),
                                   ws.data_ptr(), ws.numel(), stream())
    elif entry == "search_ex":
        ws = _ws(lib.sskd_index_search_workspace_bytes_ex(n, nq, k, tp))
        rc = lib.sskd_index_search_ex(T.tiled.data_ptr(), n, q.data_ptr(), nq, k, id_offset, out_s.data_ptr(), out_i.data_ptr(),
                                      ws.data_ptr(), ws.numel(), stream(), tp, None, None)
    elif entry == "search_filtered":
        ws = _ws(lib.sskd_index_search_workspace_bytes_ex(n, nq, k, tp))
        rc = lib.sskd_index_search_filtered(T.tiled.data_ptr(), n, q.data_ptr(), nq, k, id_offset, mp, out_s.data_ptr(),
                                            out_i.data_ptr(), ws.data_ptr(), ws.numel(), stream(), tp, None, None)
    elif entry in ("onepass", "onepass_filtered"):
        assert nq <= 64
        flag = torch.full((1,), 9, dtype=torch.int32, device="cuda")
        ws = _ws(lib.sskd_index_search_onepass_workspace_bytes(n, nq, k))
        if entry == "onepass":
            rc = lib.sskd_index_search_onepass(T.tiled.data_ptr(), n, q.data_ptr(), nq, k, id_offset, out_s.data_ptr(),
                                               out_i.data_ptr(), flag.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        else:
            rc = lib.sskd_index_search_onepass_filtered(T.tiled.data_ptr(), n, q.data_ptr(), nq, k, id_offset, mp,
                                                        out_s.data_ptr(), out_i.data_ptr(), flag.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), stream())
        _native.check(rc)
        torch.cuda.synchronize()
        assert int(flag.item()) == 0, (entry, "the one-pass proof did not hold", int(flag.item()))
    else:
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        ws = _ws(lib.sskd_index_search_screened_workspace_bytes(n, nq, k))
        assert ws.numel() > 1, "the screened path refuses this shape"
        head = (T.tiled.data_ptr(), T.bf.data_ptr(), n, q.data_ptr(), nq, k, id_offset)
        tail = (out_s.data_ptr(), out_i.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), stream(), None, None)
        if entry == "screened":
            rc = lib.sskd_index_search_screened(*head, *tail)
        elif entry == "screened_filtered":
            rc = lib.sskd_index_search_screened_filtered(*head, mp, *tail)
        else:
            rc = lib.sskd_index_search_screened_claim(*head, mp, {"screened_dealt": 0, "screened_claimed": 1}[entry], *tail)
        _native.check(rc)
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        print(f"{entry}: {int(st[1])} of {nq} queries took the exact fallback")
        assert st[0] == 0 and 0 <= st[1] < nq, (entry, "every query fell back: nothing was screened", st.tolist())
    _native.check(rc)
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


UNFILTERED = ("search", "search_ex", "onepass", "screened", "screened_dealt", "screened_claimed")
FILTERED = ("search_filtered", "screened_filtered", "onepass_filtered")
EX_TUNING = (64, 0, 1)       # 64 queries per block, the shared pools forced on: not the built-in plan of this shape


def check_scans(T, entries, id_offset=0):
    sp = T.sp
    ref = hr.topk_ref(sp, T.queries, hr.K, id_offset)
    cleared = hr.masked_rows(sp)
    ref_masked = hr.topk_ref(sp, T.queries, hr.K, id_offset, allowed=hr.allow_all_but(cleared))
    for entry in entries:
        filtered = entry in FILTERED
        nq = 64 if entry.startswith("onepass") else hr.NQ
        got = run_exact(T, entry, hr.K, id_offset, cleared if filtered else None,
                        queries=None if nq == hr.NQ else T.queries[:nq], tuning=EX_TUNING if entry == "search_ex" else None)
        want = ref_masked if filtered else ref
        _same_topk(got, (want[0][:nq], want[1][:nq]), (entry, id_offset))
        if filtered:
            assert not np.isin(got[1] - id_offset, cleared).any(), (entry, "a cleared row was returned")


def check_range(T, id_offset=0):
    sp, lib, n = T.sp, T.lib, T.n
    thr = hr.range_thresholds(sp, T.queries)
    ref = hr.range_ref(sp, T.queries, thr, id_offset)
    total = int(ref[0][-1])
    room = total + 64
    lims = torch.full((hr.NQ + 1,), -3, dtype=torch.int64, device="cuda")
    sc = torch.full((room,), SENT_S, dtype=torch.float32, device="cuda")
    ids = torch.full((room,), SENT_I, dtype=torch.int64, device="cuda")
    ws = _ws(lib.sskd_index_range_search_workspace_bytes(n, hr.NQ, total))
    _native.check(lib.sskd_index_range_search(T.tiled.data_ptr(), n, T.q.data_ptr(), hr.NQ, _dev(thr).data_ptr(), id_offset, None,
                                              lims.data_ptr(), sc.data_ptr(), ids.data_ptr(), total, ws.data_ptr(), ws.numel(),
                                              stream()))
    torch.cuda.synchronize()
    lims, sc, ids = lims.cpu().numpy(), sc.cpu().numpy(), ids.cpu().numpy()
    assert np.array_equal(lims, ref[0]), ("lims", np.flatnonzero(lims != ref[0])[:5].tolist())
    assert np.array_equal(ids[:total], ref[2]) and np.array_equal(_bits(sc[:total]), _bits(ref[1])), "range results"
    assert (sc[total:] == np.float32(SENT_S)).all() and (ids[total:] == SENT_I).all(), "written past the results"
    for j in range(hr.NQ):
        seg = ids[lims[j]: lims[j + 1]]
        assert np.unique(seg).size == seg.size, (j, "an id appears twice")


def check_grouped(T, id_offset=0):
    sp, lib, n = T.sp, T.lib, T.n
    k, kr, nq = hr.K, hr.GROUPED_K_ROWS, hr.NQ
    ref = hr.grouped_ref(sp, T.queries, k, kr, id_offset)
    groups = (torch.arange(n, dtype=torch.int32, device="cuda") // TILE).contiguous()
    groups[_dev(sp.rows)] = _dev(hr.planted_groups(sp)[1])
    sc = torch.full((nq, k), SENT_S, dtype=torch.float32, device="cuda")
    ids = torch.full((nq, k), SENT_I, dtype=torch.int64, device="cuda")
    gr = torch.full((nq, k), -55, dtype=torch.int32, device="cuda")
    cnt, unp = (torch.full((nq,), -55, dtype=torch.int32, device="cuda") for _ in range(2))
    nun = torch.full((1,), -55, dtype=torch.int32, device="cuda")
    ws = _ws(lib.sskd_index_search_grouped_workspace_bytes(n, nq, k, kr))
    _native.check(lib.sskd_index_search_grouped(T.tiled.data_ptr(), n, T.q.data_ptr(), nq, k, kr, id_offset, None, groups.data_ptr(),
                                                sc.data_ptr(), ids.data_ptr(), gr.data_ptr(), cnt.data_ptr(), unp.data_ptr(),
                                                nun.data_ptr(), ws.data_ptr(), ws.numel(), stream()))
    torch.cuda.synchronize()
    import grouped_cases as gc

    gc.same((sc.cpu().numpy(), ids.cpu().numpy(), gr.cpu().numpy()), ref[:3], ("grouped", id_offset))
    assert np.array_equal(cnt.cpu().numpy(), ref[3]) and np.array_equal(unp.cpu().numpy().astype(bool), ref[4])
    assert int(nun.item()) == int(ref[4].sum())
    assert (ref[2][:, 0] >= sp.padded // TILE).all(), "every query is led by a planted group"


def check_ivf(T, id_offset=0):
    sp, lib, n = T.sp, T.lib, T.n
    nq, k, nprobe = hr.NQ, hr.IVF_K, 4
    offsets, _ = hr.ivf_lists(sp)
    nlist = offsets.size - 1
    probe = hr.ivf_probes(sp, nq, nprobe)
    ref = hr.ivf_ref(sp, T.queries, probe, k, id_offset)
    if "list_rows" not in T.cache:
        T.cache["list_rows"] = torch.arange(n, dtype=torch.int32, device="cuda")
    d_off, d_probe = _dev(offsets), _dev(probe)
    out_s, out_i = _outs(nq, k)
    need = int(lib.sskd_ivf_search_workspace_bytes(nq, nprobe, k, n, 2 * hr.IVF_LIST_HALF))
    ws = _ws(need)
    _native.check(lib.sskd_ivf_search(T.tiled.data_ptr(), n, T.q.data_ptr(), nq, d_probe.data_ptr(), nprobe, d_off.data_ptr(),
                                      T.cache["list_rows"].data_ptr(), nlist, k, id_offset, None, out_s.data_ptr(),
                                      out_i.data_ptr(), ws.data_ptr(), need, stream()))
    torch.cuda.synchronize()
    _same_topk((out_s.cpu().numpy(), out_i.cpu().numpy()), ref, ("ivf", id_offset))
    assert set(sp.high_rows().tolist()) <= set((ref[1][ref[1] >= 0] - id_offset).tolist()), "a high planted row no probe reaches"


def check_graph_search(T, id_offset=0):
    sp, lib, n = T.sp, T.lib, T.n
    nq, k, ef, width, M, n_seeds = hr.NQ, hr.K, 32, 4, hr.GRAPH_M, 4
    # seeds on the low side: the first planted rows (and one -1); the walk must cross every boundary to reach its answer
    seeds_c = np.tile(np.array([0, 1, -1, 2], np.int64), (nq, 1))
    (want_s, want_c, want_it), c = hr.graph_ref(sp, T.queries, seeds_c, k, ef, width)
    if "graph" not in T.cache:
        g = torch.full((n, M), -1, dtype=torch.int32, device="cuda")
        g[_dev(sp.rows)] = _dev(hr.graph_edges(sp, M))
        T.cache["graph"] = g
    seeds = _dev(c.ids(seeds_c))
    out_s, out_i = _outs(nq, k)
    its = torch.full((nq,), -5, dtype=torch.int32, device="cuda")
    _native.check(lib.sskd_graph_search(T.tiled.data_ptr(), n, T.cache["graph"].data_ptr(), M, T.q.data_ptr(), nq, seeds.data_ptr(),
                                        n_seeds, None, 0, k, ef, width, ef, id_offset, None, out_s.data_ptr(), out_i.data_ptr(),
                                        its.data_ptr(), stream()))
    torch.cuda.synchronize()
    want_i = c.ids(want_c, id_offset)
    _same_topk((out_s.cpu().numpy(), out_i.cpu().numpy()), (want_s, want_i), ("graph_search", id_offset))
    assert np.array_equal(its.cpu().numpy(), want_it), "iteration counts"
    assert set(sp.high_rows().tolist()) <= set((want_i[want_i >= 0] - id_offset).tolist()), "a high planted row no walk returns"


def _ranking(T):
    if "rank" not in T.cache:
        T.cache["rank"] = hr.rank_lists(T.sp, T.queries)
    return T.cache["rank"]


def check_mine(T, id_offset=0):
    import mine_cases as mc

    sp, lib, n = T.sp, T.lib, T.n
    S, I, c, full = _ranking(T)
    nq, search_k, top_k, margin = hr.NQ, hr.RANK_K, 5, 0.1
    # two positives per query, high planted rows among them for every query, one of them perhaps in the ranking
    lists = [sp.rows[[(q + 5) % sp.P, (q + 20) % sp.P]] for q in range(nq)]
    lims, rows = mc.csr(lists)
    lims_c, rows_c = mc.csr([c.numbers(x) for x in lists])
    ref = mc.expected(S, c.numbers(I), lims_c, rows_c, full, margin, top_k)
    ref = (ref[0], c.ids(ref[1], id_offset), ref[2], ref[3])
    sc = torch.full((nq, top_k), SENT_S, dtype=torch.float32, device="cuda")
    ids = torch.full((nq, top_k), SENT_I, dtype=torch.int64, device="cuda")
    cnt = torch.full((nq,), -55, dtype=torch.int32, device="cuda")
    mp = torch.full((nq,), SENT_S, dtype=torch.float32, device="cuda")
    d_s, d_i, d_l, d_r = _dev(S), _dev(I), _dev(lims), _dev(rows)
    _native.check(lib.sskd_index_mine_select(T.tiled.data_ptr(), n, T.q.data_ptr(), nq, d_s.data_ptr(), d_i.data_ptr(), search_k,
                                             d_l.data_ptr(), d_r.data_ptr(), None, margin, top_k, id_offset, sc.data_ptr(),
                                             ids.data_ptr(), cnt.data_ptr(), mp.data_ptr(), stream()))
    torch.cuda.synchronize()
    mc.same((sc.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy(), mp.cpu().numpy()), ref, ("mine", id_offset))
    assert (ref[3] != 0).all(), "every query's max_pos is a planted score"


def check_hybrid(T, id_offset=0):
    import hybrid_cases as hc

    sp, lib, n = T.sp, T.lib, T.n
    S, I, c, full = _ranking(T)
    nq, kd, kb, k = hr.NQ, hr.RANK_K, 8, 12
    # the BM25 side names eight other planted rows: the kernel scores them densely (the gather)
    J = np.stack([sp.rows[(q + 10 + 3 * np.arange(kb)) % sp.P] for q in range(nq)]).astype(np.int64)
    B = np.tile(np.linspace(9.0, 2.0, kb), (nq, 1))
    # a BM25 index of one term whose posting list holds every fourth planted row (ascending), weight 0.5 + i / 8
    post_rows = sp.rows[::4].astype(np.int32)
    post_w = 0.5 + np.arange(post_rows.size) / 8.0
    idf = np.array([1.5])
    full_bm25 = np.zeros((nq, c.rows.size))
    full_bm25[:, c.numbers(post_rows.astype(np.int64))] = 0.0 + idf[0] * post_w
    want = hc.fuse_batch(S, c.numbers(I), B, c.numbers(J), n_rows=c.rows.size, k=k, method="linear", ws=0.7, wb=0.3,
                         full_dense=full, full_bm25=full_bm25)
    want = (want[0], c.ids(want[1], id_offset)) + want[2:]
    tables = [_dev(x) for x in (np.array([0, post_rows.size], np.int64), post_rows, post_w, idf,
                                np.arange(nq + 1, dtype=np.int64), np.zeros(nq, np.int32))]
    d_s, d_i, d_b, d_j = _dev(S), _dev(I), _dev(B), _dev(J)
    out_s = torch.full((nq, k), 7.0, dtype=torch.float64, device="cuda")
    out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    out_c = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    out_d = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda")
    out_b = torch.full((nq, k), 7.0, dtype=torch.float64, device="cuda")
    _native.check(lib.sskd_hybrid_fuse(
        T.tiled.data_ptr(), n, T.q.data_ptr(), d_s.data_ptr(), d_i.data_ptr(), kd, tables[0].data_ptr(), tables[1].data_ptr(),
        tables[2].data_ptr(), tables[3].data_ptr(), 1, tables[4].data_ptr(), tables[5].data_ptr(), d_b.data_ptr(), d_j.data_ptr(),
        kb, None, 1, 0.7, 0.3, 60.0, nq, k, id_offset, out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr(), out_d.data_ptr(),
        out_b.data_ptr(), stream()))
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in (out_s, out_i, out_d, out_b, out_c))
    hc.assert_same(got, want, f"hybrid linear, id_offset {id_offset}")


def check_rocchio(T):
    import expand_cases as ec

    sp, lib, n = T.sp, T.lib, T.n
    S, I, c, _ = _ranking(T)
    nq, kd = hr.NQ, hr.RANK_K
    for weighting, code in (("uniform", 0), ("score", 1)):
        want = ec.rocchio_batch(T.queries, S, c.numbers(I), c.corpus, fb_docs=kd, alpha=1.0, beta=0.75, weighting=weighting)
        out = torch.full((nq, DIM), float("nan"), dtype=torch.float32, device="cuda")
        counts = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        d_s, d_i = _dev(S), _dev(I)
        _native.check(lib.sskd_prf_rocchio(T.tiled.data_ptr(), n, T.q.data_ptr(), nq, d_s.data_ptr(), d_i.data_ptr(), kd, kd,
                                           1.0, 0.75, code, out.data_ptr(), counts.data_ptr(), stream()))
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), want[1]), (weighting, "counts")
        assert np.array_equal(ec.bits32(out.cpu().numpy()), ec.bits32(want[0])), (weighting, "query bits differ")


def check_mmr(T, id_offset=0):
    import mmr_cases as mm

    sp, lib, n = T.sp, T.lib, T.n
    S, I, c, _ = _ranking(T)
    nq, fetch_k, k = hr.NQ, hr.RANK_K, 8
    want = mm.mmr_batch(S, c.numbers(I), c.corpus, k=k, lam=0.5, dup_threshold=np.inf)
    want = (want[0], c.ids(want[1], id_offset)) + want[2:]
    D = torch.full((nq, k), SENT_S, dtype=torch.float32, device="cuda")
    J = torch.full((nq, k), SENT_I, dtype=torch.int64, device="cuda")
    V = torch.full((nq, k), 7.0, dtype=torch.float64, device="cuda")
    R = torch.full((nq, k), SENT_S, dtype=torch.float32, device="cuda")
    counts = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
    d_s, d_i = _dev(S), _dev(I)
    _native.check(lib.sskd_mmr_select(T.tiled.data_ptr(), n, d_s.data_ptr(), d_i.data_ptr(), nq, fetch_k, 0.5, float("inf"), k,
                                      id_offset, D.data_ptr(), J.data_ptr(), V.data_ptr(), R.data_ptr(), counts.data_ptr(), stream()))
    torch.cuda.synchronize()
    mm.same(tuple(t.cpu().numpy() for t in (D, J, V, R, counts)), want, f"mmr, id_offset {id_offset}")


# ---------------------------------------------------------------------------------------------------------------------
# tier 1
# ---------------------------------------------------------------------------------------------------------------------
def test_tier1_writers_and_readers(tier1):
    run_writers_readers(tier1)


def test_tier1_similarity_over_the_whole_index(tier1):
    T, sp = tier1, tier1.sp
    nq = 33
    out = torch.empty((nq, sp.n), dtype=torch.float32, device="cuda")
    _native.check(T.lib.sskd_similarity(T.q.data_ptr(), nq, T.tiled.data_ptr(), sp.n, DIM, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    want = oracle.scores_fma(T.queries[:nq], sp.values)
    assert (want != 0).all()
    cols = (out.view(torch.int32) != 0).any(dim=0).nonzero().flatten().cpu().numpy()
    assert np.array_equal(cols, sp.rows), ("non-zero columns", np.setxor1d(cols, sp.rows)[:8].tolist())
    assert np.array_equal(_bits(out[:, _dev(sp.rows)].cpu().numpy()), _bits(want))


def test_tier1_exact_and_screened_scans(tier1):
    check_scans(tier1, UNFILTERED)
    # the exact scan at k = 100: chained passes, and a tail of the lowest zero rows
    ref = hr.topk_ref(tier1.sp, tier1.queries, 100)
    _same_topk(run_exact(tier1, "search", 100), ref, "search k=100")
    # ties: four positive planted rows, then the six lowest rows that are not planted
    ties = hr.ties_queries(tier1.sp)
    got = run_exact(tier1, "search", hr.K, queries=ties)
    _same_topk(got, hr.topk_ref(tier1.sp, ties, hr.K), "ties")
    assert (got[1][:, hr.TIES_POSITIVE:] == np.array([2, 3, 4, 5, 6, 7])).all()


def test_tier1_filtered_scans(tier1):
    check_scans(tier1, FILTERED)


def test_tier1_range_search(tier1):
    check_range(tier1)


def test_tier1_grouped_search(tier1):
    check_grouped(tier1)


def test_tier1_ivf_search_and_list_sums(tier1):
    T, sp = tier1, tier1.sp
    check_ivf(T)
    offsets, _ = hr.ivf_lists(sp)
    nlist = offsets.size - 1
    sums = torch.full((nlist + 1, DIM), float("nan"), dtype=torch.float64, device="cuda")
    _native.check(T.lib.sskd_ivf_list_sums(T.tiled.data_ptr(), sp.n, _dev(offsets).data_ptr(), T.cache["list_rows"].data_ptr(),
                                           nlist, sums.data_ptr(), stream()))
    torch.cuda.synchronize()
    sums = sums.cpu().numpy()
    assert np.isnan(sums[nlist]).all()
    # one fp64 accumulator per element from +0.0 in CSR order: a zero row adds +0.0 and changes no bit, so the sum is the
    # planted rows of the list added in row order
    for l in range(nlist):
        want = np.zeros(DIM, np.float64)
        for i in np.flatnonzero((sp.rows >= offsets[l]) & (sp.rows < offsets[l + 1])):
            want = want + sp.values[i].astype(np.float64)
        assert np.array_equal(sums[l].view(np.int64), want.view(np.int64)), ("list", l)


def test_tier1_graph_search_and_link(tier1):
    import graph_insert_cases as gi

    T, sp = tier1, tier1.sp
    check_graph_search(T)
    # link: every third planted row is touched; its incoming edges are four other planted rows from across the index
    M, H = hr.GRAPH_M, hr.GRAPH_M // 2
    touched_c = np.arange(0, sp.P, 3)
    incoming_c = np.stack([(t + np.array([11, 17, 23, 29])) % sp.P for t in touched_c])
    c = hr.Compressed(sp.rows, sp.values)
    adj_c = c.numbers(hr.graph_edges(sp, M)).astype(np.int32)
    want_c = gi.link_ref(sp.values, adj_c, sp.P, touched_c, incoming_c)
    g = T.cache["graph"].clone()
    touched = _dev(sp.rows[touched_c].astype(np.int32))
    incoming = _dev(sp.rows[incoming_c].astype(np.int32))
    _native.check(T.lib.sskd_graph_link(T.tiled.data_ptr(), g.data_ptr(), sp.n, sp.n, M, touched.data_ptr(), incoming.data_ptr(),
                                        touched_c.size, stream()))
    torch.cuda.synchronize()
    got = g[_dev(sp.rows)].cpu().numpy()
    assert np.array_equal(got, c.ids(want_c).astype(np.int32)), "relinked rows"
    assert (want_c[touched_c] != adj_c[touched_c]).any(), "the link changed nothing"
    g[_dev(sp.rows)] = -1
    assert bool((g == -1).all()), "a row that was not named was written"
    del g


def check_pq(T, id_offset=0):
    """sskd_pq_encode over the whole index, sskd_pq_code_sums over lists that name every planted row, sskd_pq_search
    with refine over the lists of ``check_ivf``"""
    import pq_cases as pc

    sp, lib, n, m = T.sp, T.lib, T.n, hr.PQ_M
    if "pq" not in T.cache:
        cb = hr.pq_codebooks(sp)
        codes, zero_code = hr.pq_codes(sp, cb)
        assert (codes != zero_code).any(1).all(), "a planted row that encodes like a zero row would hide a misread"
        d_cb = _dev(cb)
        out = torch.full(((n + 1) * m,), 0xAB, dtype=torch.uint8, device="cuda")
        _native.check(lib.sskd_pq_encode(T.tiled.data_ptr(), n, None, None, 0, d_cb.data_ptr(), m, out.data_ptr(), stream()))
        torch.cuda.synchronize()
        assert bool((out[n * m:] == 0xAB).all()), "codes written past the last row"
        want = _dev(zero_code).repeat(n, 1)
        want[_dev(sp.rows)] = _dev(codes)
        got = out[: n * m].view(n, m)
        assert torch.equal(got, want), ("codes", (got != want).any(1).nonzero().flatten()[:8].tolist())
        del want
        T.cache["pq"] = (cb, codes, zero_code, d_cb, got)
    cb, codes, zero_code, d_cb, d_codes = T.cache["pq"]
    if id_offset == 0:
        offsets, writes, listed = hr.pq_code_lists(sp, codes, zero_code)
        want_s, want_c = hr.pq_code_sums_ref(sp, codes, zero_code, listed)
        group_rows = torch.zeros(m * n, dtype=torch.int32, device="cuda")
        for at, rows in writes:
            group_rows[at: at + rows.size] = _dev(rows)
        dsub = DIM // m
        sums = torch.full((m * 256 * dsub + 8,), float("nan"), dtype=torch.float64, device="cuda")
        counts = torch.full((m * 256 + 8,), -7, dtype=torch.int64, device="cuda")
        _native.check(lib.sskd_pq_code_sums(T.tiled.data_ptr(), n, None, None, 0, _dev(offsets).data_ptr(), group_rows.data_ptr(), m,
                                            sums.data_ptr(), counts.data_ptr(), stream()))
        torch.cuda.synchronize()
        sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
        assert np.isnan(sums[m * 256 * dsub:]).all() and (counts[m * 256:] == -7).all()
        assert np.array_equal(counts[: m * 256].reshape(m, 256), want_c), "code counts"
        assert np.array_equal(pc.bits64(sums[: m * 256 * dsub].reshape(m, 256, dsub)), pc.bits64(want_s)), "code sums"
        del group_rows
    # the search: the probes of check_ivf, every probe score 0.0, refine = 64
    nq, k, R, nprobe = hr.NQ, hr.K, hr.PQ_REFINE, 4
    offsets, _ = hr.ivf_lists(sp)
    nlist = offsets.size - 1
    probe = hr.ivf_probes(sp, nq, nprobe)
    probe_scores = np.zeros(probe.shape, np.float32)
    ref = hr.pq_search_ref(sp, T.queries, probe, probe_scores, cb, codes, zero_code, k, R, id_offset)
    if "list_rows" not in T.cache:
        T.cache["list_rows"] = torch.arange(n, dtype=torch.int32, device="cuda")
    out_s, out_i = _outs(nq, k)
    out_c = torch.full((nq, R), -7, dtype=torch.int64, device="cuda")
    need = int(lib.sskd_pq_search_workspace_bytes(nq, nprobe, k, R, m, n, 2 * hr.IVF_LIST_HALF))
    assert need > 0
    ws = _ws(need)
    d_probe, d_ps, d_off = _dev(probe), _dev(probe_scores), _dev(offsets)
    _native.check(lib.sskd_pq_search(T.tiled.data_ptr(), n, T.q.data_ptr(), nq, d_probe.data_ptr(), d_ps.data_ptr(), nprobe,
                                     d_off.data_ptr(), T.cache["list_rows"].data_ptr(), nlist, d_codes.data_ptr(), d_cb.data_ptr(), m,
                                     k, R, id_offset, None, out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr(), ws.data_ptr(),
                                     need, stream()))
    torch.cuda.synchronize()
    assert np.array_equal(out_c.cpu().numpy(), ref[2]), ("pq candidates", id_offset)
    _same_topk((out_s.cpu().numpy(), out_i.cpu().numpy()), ref[:2], ("pq_search", id_offset))
    assert set(sp.high_rows().tolist()) <= set((ref[1][ref[1] >= 0] - id_offset).tolist()), "a high planted row no query returns"


def test_tier1_pq_encode_code_sums_and_refined_search(tier1):
    check_pq(tier1)


def test_tier1_gathers(tier1):
    check_mine(tier1)
    check_hybrid(tier1)
    check_rocchio(tier1)
    check_mmr(tier1)


def test_tier1_id_offset(tier1):
    """id_offset = 2^40 + 7 through every entry point that takes one: each id is row + offset exactly"""
    off = hr.ID_OFFSET
    check_scans(tier1, UNFILTERED + FILTERED, off)
    check_range(tier1, off)
    check_grouped(tier1, off)
    check_ivf(tier1, off)
    check_graph_search(tier1, off)
    check_pq(tier1, off)
    check_mine(tier1, off)
    check_hybrid(tier1, off)
    check_mmr(tier1, off)


def test_tier1_compaction_and_normalise(tier1):
    """the source and the destination both cross the boundaries; the sidecar is freed first"""
    T, sp, lib = tier1, tier1.sp, tier1.lib
    T.bf = None
    T.cache.clear()
    torch.cuda.empty_cache()
    drops = hr.compaction_drops(sp)
    new_rows, values, n_live = hr.compacted(sp, drops)
    assert 1000 <= drops.size < 1100 and 0 < new_rows.size < sp.P
    for b in sp.boundaries:
        assert (new_rows < b - drops.size).any() and (new_rows > b).any()
    padded_live = -(-n_live // TILE) * TILE
    assert int(lib.sskd_index_padded_rows(n_live)) == padded_live
    mask = T.mask(drops)
    n_words = mask.numel()
    prefix = torch.full((n_words + 1,), -7, dtype=torch.int64, device="cuda")
    dst = torch.full(((padded_live + TILE) * DIM,), SENT_I, dtype=torch.int32, device="cuda")
    _native.check(lib.sskd_row_mask_rank(mask.data_ptr(), sp.n, prefix.data_ptr(), stream()))
    _native.check(lib.sskd_index_compact_rows(T.tiled.data_ptr(), sp.n, mask.data_ptr(), prefix.data_ptr(), dst.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert int(prefix[-1].item()) == n_live
    # the prefix at the words of the dropped rows: an exclusive count of what lives before
    at = np.unique(drops >> 5)
    want_prefix = 32 * at - np.searchsorted(drops, 32 * at)
    assert np.array_equal(prefix[_dev(at)].cpu().numpy(), want_prefix)
    assert bool((dst[padded_live * DIM:] == SENT_I).all()), "written behind the last destination tile"
    nz = _nonzero_rows(dst, padded_live, DIM)
    assert np.array_equal(nz, new_rows), ("surviving planted rows", np.setxor1d(nz, new_rows)[:8].tolist())
    got = dst[: padded_live * DIM].view(padded_live, DIM)[_dev(new_rows)].view(torch.float32).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(values))
    # the source is only read
    assert np.array_equal(_nonzero_rows(T.tiled, sp.padded, DIM), sp.rows)
    # sskd_l2_normalize_rows in place on the compacted copy, across the same boundaries: the planted rows are normalised
    # (to the tolerance of the kernel's own test in test_search_gpu.py), zero rows stay zero
    scaled = int(new_rows[-1])
    x = dst[: padded_live * DIM].view(torch.float32).view(padded_live, DIM)
    x[scaled] *= 2.0
    _native.check(lib.sskd_l2_normalize_rows(x.data_ptr(), n_live, DIM, stream()))
    torch.cuda.synchronize()
    assert np.array_equal(_nonzero_rows(dst, padded_live, DIM), new_rows)
    got = x[_dev(new_rows)].cpu().numpy()
    src = values.copy()
    src[-1] *= 2.0
    np.testing.assert_allclose(got, oracle.l2_normalize_rows(src), rtol=0, atol=2e-7)
    # and on a copy of the last 64 tiles of the index with a planted row scaled by 2
    tail = T.tiled[(sp.padded - 64 * TILE) * DIM:].clone().view(64 * TILE, DIM)
    local = sp.rows[sp.rows >= sp.padded - 64 * TILE] - (sp.padded - 64 * TILE)
    tail[int(local[0])] *= 2.0
    want = oracle.l2_normalize_rows(tail.cpu().numpy())
    _native.check(lib.sskd_l2_normalize_rows(tail.data_ptr(), 64 * TILE - 11, DIM, stream()))
    torch.cuda.synchronize()
    np.testing.assert_allclose(tail.cpu().numpy(), want, rtol=0, atol=2e-7)
    assert local.size >= 3 and np.array_equal(np.flatnonzero(np.abs(want).sum(1)), local)
    del dst, x, tail


# ---------------------------------------------------------------------------------------------------------------------
# the token store of the late interaction
# ---------------------------------------------------------------------------------------------------------------------
def test_token_store_across_its_boundaries(gpu, native_lib):
    import late_cases as lc
    from test_late_gpu import _assert_in_band

    for other in list(_resident):          # (the tiers are not needed here: 4.0 GiB of tokens stand alone)
        _resident.pop(other).drop()
    lib = native_lib
    docs = hr.token_documents()
    B, S = docs.lengths.size, int(docs.lengths.max())
    hidden = lc.bf16_bits(docs.rng.standard_normal((B, S, DIM)).astype(np.float32))
    want_tok, want_lims = lc.pack_rows(hidden, docs.lengths)
    store = torch.zeros((docs.n_tokens, DIM), dtype=torch.bfloat16, device="cuda")
    d_h, d_len, d_off = _dev(hidden), _dev(docs.lengths), _dev(docs.offsets)
    _native.check(lib.sskd_late_pack_tokens(d_h.data_ptr(), d_len.data_ptr(), d_off.data_ptr(), B, S, docs.n_tokens,
                                            store.data_ptr(), stream()))
    torch.cuda.synchronize()
    token_rows = np.concatenate([np.arange(o, o + l) for o, l in docs.spans])
    nz = _nonzero_rows(store, docs.n_tokens, DIM // 2)
    assert np.array_equal(nz, token_rows), ("non-zero tokens", np.setxor1d(nz, token_rows)[:8].tolist())
    got = store[_dev(token_rows)].view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want_tok), "packed token bits"
    # re-rank: every document, the empty last row, a -1 and an id outside the store; document d is store row 2 d + 1
    rng = np.random.default_rng(77)
    q_bits, q_lims = lc.queries(rng, [5, 33, 128])
    nq, k = 3, 10
    empty_c, empty_row = B, docs.n_rows - 1
    cand_c = np.stack([np.concatenate([rng.permutation(B), [empty_c, -1, B + 5]]) for _ in range(nq)]).astype(np.int64)
    R = cand_c.shape[1]
    cand = np.where(cand_c < 0, -1, np.where(cand_c < B, 2 * cand_c + 1, np.where(cand_c == empty_c, empty_row, docs.n_rows + 9)))
    ref = lc.Reference(q_bits, q_lims, want_tok, np.concatenate([want_lims, want_lims[-1:]]))
    d_q, d_ql, d_tl, d_c = _dev(q_bits), _dev(q_lims), _dev(docs.tok_lims), _dev(cand)
    for id_offset in (0, hr.ID_OFFSET):
        d_c = _dev(np.where(cand >= 0, cand + id_offset, -1))
        D = torch.full((nq, k), SENT_S, dtype=torch.float32, device="cuda")
        I = torch.full((nq, k), SENT_I, dtype=torch.int64, device="cuda")
        raw = torch.full((nq, R), SENT_S, dtype=torch.float32, device="cuda")
        _native.check(lib.sskd_late_rerank(d_q.data_ptr(), q_lims.ctypes.data, d_ql.data_ptr(), nq, store.data_ptr(), d_tl.data_ptr(),
                                           docs.n_rows, docs.n_tokens, d_c.data_ptr(), R, k, id_offset, D.data_ptr(), I.data_ptr(),
                                           raw.data_ptr(), None, 0, stream()))
        torch.cuda.synchronize()
        D, I, raw = D.cpu().numpy(), I.cpu().numpy(), raw.cpu().numpy()
        _assert_in_band(raw, ref, cand_c)
        lc.check_ranking(D, I, raw, np.where(cand >= 0, cand + id_offset, -1), k)
        if id_offset == 0:
            first = raw
        else:
            assert np.array_equal(_bits(raw), _bits(first)), "a score depends on the two token lists alone"
    del store
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# tier 2: the entry points that need nothing but the index and small side arrays
# ---------------------------------------------------------------------------------------------------------------------
def test_tier2_writers_and_readers(tier2):
    run_writers_readers(tier2)


def test_tier2_scans(tier2):
    check_scans(tier2, ("search", "onepass", "search_filtered", "onepass_filtered"))
    _same_topk(run_exact(tier2, "search", 100), hr.topk_ref(tier2.sp, tier2.queries, 100), "search k=100")
    check_range(tier2)


def test_tier2_ivf_and_graph_search(tier2):
    check_ivf(tier2)
    check_graph_search(tier2)


def test_tier2_gathers(tier2):
    check_mine(tier2)
    check_hybrid(tier2)
    check_rocchio(tier2)
    check_mmr(tier2)
