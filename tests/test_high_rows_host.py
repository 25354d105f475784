"""The high-row cases, checked on the CPU: they CAN fail (``high_rows_cases``; the GPU side is
``test_high_rows_gpu.py``).

1. every boundary of a tier has planted rows strictly before, on and strictly after it;
2. a planted row read through any 32-bit truncation of its offset that wraps at that row lands outside the buffer or on
   bytes that differ from the row - no alias spot was planted by accident;
3. every main query has at least k + 2 planted rows scoring above 0 (its top k holds no zero row), every high planted
   row is in some query's top k, and the ties case has exactly four positive planted rows;
4. every range threshold lies above 0 and strictly between two neighbouring planted scores of its query;
5. the compressed references equal the oracle run on a DENSE corpus, at a miniature of the same construction;
6. every workspace and plan query that takes ``n_rows`` answers sensibly at the tiers' sizes and at 2^31 - 65 rows.

No real kernel is broken to show sensitivity: 2 and 3 are the argument.
"""
import ctypes as C

import numpy as np
import pytest

import grouped_cases as gc
import high_rows_cases as hr
from oracle import search as oracle
from semantic_search_kd_amd import _native

TIERS = [pytest.param(1, id="tier1"), pytest.param(2, id="tier2")]


# ------------------------------------------------------------------------------------------------ 1: the plants
@pytest.mark.parametrize("which", TIERS)
def test_every_boundary_has_planted_rows_before_on_and_after_it(which):
    sp = hr.tier(which)
    bounds = hr.TIER1_BOUNDARIES if which == 1 else hr.TIER2_BOUNDARIES
    assert sp.boundaries == tuple(b for b, _ in bounds) and sp.n % 32 == 21 and sp.boundaries[-1] < sp.n - 64
    planted = set(sp.rows.tolist())
    for b in sp.boundaries:
        # the straddling row holds the first byte that a 32-bit product cannot express
        assert b * hr.ROW_BYTES < (b + 1) * hr.ROW_BYTES and any(
            b * hr.ROW_BYTES < (1 << e) < (b + 1) * hr.ROW_BYTES for e in (31, 32, 33, 34, 35)), b
        assert {b - 2, b - 1, b, b + 1, b + 2, b + 3} <= planted
        t = b // 32
        assert {32 * t, 32 * t + 31, 32 * t + 32, 32 * t + 63} <= planted
    assert {0, 1, 31, 32, sp.n - 22, sp.n - 21, sp.n - 1} <= planted
    assert sp.rule_rows.size <= hr.NQ, "every rule row must lead one of the main queries"
    assert np.array_equal(sp.rule_rows, hr.plant_rows(sp.n, sp.boundaries)) and sp.P == sp.rule_rows.size + 12
    assert len({v.tobytes() for v in sp.values}) == sp.P and (np.abs(sp.values).sum(1) > 1).all()
    # the writer's blocks hold exactly the planted rows
    blocks = sp.blocks()
    assert sum(int((np.abs(blk).sum(1) > 0).sum()) for _, blk in blocks) == sp.P
    for row0, blk in blocks:
        assert row0 % 32 == 0 and blk.shape == (32, hr.DIM)
        for r in np.flatnonzero(np.abs(blk).sum(1) > 0):
            assert np.array_equal(blk[r], sp.values[np.searchsorted(sp.rows, row0 + r)])


def test_the_token_store_boundaries():
    assert [b for b, _ in hr.TOKEN_BOUNDARIES] == [2_796_202, 5_592_405]
    for (b, _), e in zip(hr.TOKEN_BOUNDARIES, (31, 32)):
        assert b * hr.TOKEN_BYTES < (1 << e) < (b + 1) * hr.TOKEN_BYTES
    docs = hr.token_documents()
    covered = np.zeros(0, np.int64)
    for off, ln in docs.spans:
        covered = np.concatenate([covered, np.arange(off, off + ln)])
    assert np.unique(covered).size == covered.size and covered.max() == hr.TOKEN_N - 1
    for b, _ in hr.TOKEN_BOUNDARIES:
        assert {b - 1, b, b + 1}.issubset(covered.tolist())
        assert any(off < b < off + ln - 1 for off, ln in docs.spans), "a document must straddle the boundary"
    assert (np.diff(docs.tok_lims) >= 0).all() and docs.tok_lims[0] == 0 and docs.tok_lims[-1] == hr.TOKEN_N
    assert np.array_equal(docs.tok_lims[docs.doc_rows], docs.offsets)
    assert np.array_equal(docs.tok_lims[docs.doc_rows + 1] - docs.offsets, docs.lengths)


# ------------------------------------------------------------------------------------------------ 2: truncation
@pytest.mark.parametrize("which", TIERS)
def test_a_truncated_offset_never_lands_on_the_planted_bytes(which):
    sp = hr.tier(which)
    models = hr.truncation_models()
    assert len(models) == 6
    wrapped = {name: 0 for name in models}
    for i, r in enumerate(sp.rows.tolist()):
        true = r * hr.ROW_BYTES
        for name, f in models.items():
            off = f(r)
            if off == true:
                continue
            wrapped[name] += 1
            got = hr.bytes_at(sp.rows, sp.values, sp.padded, off, hr.ROW_BYTES)
            assert got is None or not np.array_equal(got, sp.values[i].view(np.uint8)), (name, r, off)
        assert hr.bytes_at(sp.rows, sp.values, sp.padded, true, hr.ROW_BYTES).tobytes() == sp.values[i].tobytes()
    # each model the tier can reach wraps at some planted row: the three byte / float models in tier 1, five in tier 2
    reach = {1: ["byte offset as int32", "byte offset as uint32", "float offset as int32"],
             2: ["byte offset as int32", "byte offset as uint32", "float offset as int32", "float offset as uint32",
                 "float4 offset as int32"]}[which]
    for name in reach:
        assert wrapped[name] >= 4, (name, wrapped)
    if which == 1:
        assert wrapped["float offset as uint32"] == 0 and wrapped["float4 offset as int32"] == 0
    # and every planted row past a boundary is wrapped by the model of that boundary
    for b, name in zip(sp.boundaries, reach):
        for r in sp.rows[sp.rows > b].tolist():
            assert models[name](r) != r * hr.ROW_BYTES, (name, r)
        assert models[name](b) == b * hr.ROW_BYTES, "the straddling row's first byte is still addressed correctly"


def test_a_truncated_token_offset_never_lands_on_a_planted_token():
    docs = hr.token_documents()
    rows = np.concatenate([np.arange(off, off + ln) for off, ln in docs.spans])
    values = np.random.default_rng(3).integers(1, 1 << 15, size=(rows.size, hr.DIM)).astype(np.uint16)
    models = hr.truncation_models(hr.TOKEN_BYTES)
    wrapped = {name: 0 for name in models}
    padded = hr.TOKEN_N
    for i, r in enumerate(rows.tolist()):
        for name, f in models.items():
            off = f(r)
            if off == r * hr.TOKEN_BYTES:
                continue
            wrapped[name] += 1
            got = hr.bytes_at(rows, values, padded, off, hr.TOKEN_BYTES)
            assert got is None or not np.array_equal(got, values[i].view(np.uint8)), (name, r)
    assert wrapped["byte offset as int32"] > 100 and wrapped["byte offset as uint32"] > 20
    assert wrapped["element offset as int32"] > 20 and wrapped["uint4 offset as int32"] == 0


# ------------------------------------------------------------------------------------------------ 3: the queries
@pytest.mark.parametrize("which", TIERS)
def test_main_queries_fill_their_top_k_with_planted_rows_and_reach_every_planted_row(which):
    sp = hr.tier(which)
    q = hr.main_queries(sp)
    assert q.shape == (hr.NQ, hr.DIM) and hr.NQ >= 64
    s = hr.planted_scores(sp, q)
    positive = (s > 0).sum(1)
    assert positive.min() >= hr.K + 2, positive.min()
    D, I = hr.topk_ref(sp, q, hr.K)
    assert np.isin(I, sp.rows).all() and (D > 0).all(), "no zero row in a main query's top k"
    assert set(sp.rule_rows.tolist()) <= set(I.ravel().tolist()), "a rule row no query returns would go unread"
    assert np.array_equal(I[np.arange(sp.rule_rows.size), 0], sp.rule_rows), "query j is led by rule row j"
    # the boosters: in the first 64 tiles (the screened search's bound-only sample), in twelve different buckets of
    # (row mod 32), every score against every main query well above the screening band (2^-7 |q| max |row| < 0.008) and
    # below the query's tenth best score - the bound they give prunes the zero rows and no booster enters a top 10
    boosters = sp.rows[sp.booster]
    assert boosters.size == 12 and boosters.max() < 64 * 32 and np.unique(boosters % 32).size == 12
    sb = s[:, sp.booster]
    assert sb.min() > 0.04 and (sb.max(1) < D[:, hr.K - 1]).all(), (sb.min(), sb.max(), D[:, hr.K - 1].min())
    assert not np.isin(I, boosters).any()
    assert (np.sort(sb, axis=1)[:, 2] > 0.04).all(), "the tenth largest of the twelve booster scores is the bound"
    # the masked form: the cleared rows vanish and nothing else does
    cleared = hr.masked_rows(sp)
    assert np.isin(cleared, sp.rows).all() and cleared.size == 4 * len(sp.boundaries)
    Dm, Im = hr.topk_ref(sp, q, hr.K, allowed=hr.allow_all_but(cleared))
    assert not np.isin(Im, cleared).any() and np.isin(Im, sp.rows).all()
    assert (Im != I).any()
    # k = 100 runs past the planted rows into the zeros: the tail is the lowest rows that are not planted
    D100, I100 = hr.topk_ref(sp, q, 100)
    for j in range(hr.NQ):
        npos = int(positive[j])
        assert (D100[j, :npos] > 0).all() and (D100[j, npos:] == 0).all()
        assert np.array_equal(I100[j, npos:], sp.zero_rows(100)[: 100 - npos])
        assert I100[j, npos] == 2 and I100[j, npos + 1] == 3


def test_the_ties_case_has_exactly_four_positive_planted_rows():
    sp = hr.tier(1)
    q = hr.ties_queries(sp)
    s = hr.planted_scores(sp, q)
    assert ((s > 0).sum(1) == hr.TIES_POSITIVE).all() and (s != 0).all()
    D, I = hr.topk_ref(sp, q, hr.K)
    want_tail = sp.zero_rows(hr.K - hr.TIES_POSITIVE)
    assert want_tail.tolist() == [2, 3, 4, 5, 6, 7]
    for j in range(q.shape[0]):
        assert np.isin(I[j, :4], sp.rows).all() and (D[j, :4] > 0).all()
        assert (I[j, :4] > sp.boundaries[0]).all(), "the four positive rows all lie past the first boundary"
        assert np.array_equal(I[j, 4:], want_tail) and (D[j, 4:] == 0).all() and not np.signbit(D[j, 4:]).any()
        negative = sp.rows[s[j] < 0]
        assert negative.size == sp.P - 4 and not np.isin(I[j], negative).any(), "the boosters score below 0 here too"


# ------------------------------------------------------------------------------------------------ 4: thresholds
@pytest.mark.parametrize("which", TIERS)
def test_range_thresholds_separate_two_planted_scores_above_zero(which):
    sp = hr.tier(which)
    q = hr.main_queries(sp)
    thr = hr.range_thresholds(sp, q)
    s = hr.planted_scores(sp, q)
    assert thr.dtype == np.float32 and (thr > 0).all()
    for j in range(hr.NQ):
        above, below = s[j][s[j] > thr[j]], s[j][s[j] < thr[j]]
        assert above.size == 1 + j % 12 and above.size + below.size == sp.P, "no score equals its threshold"
        assert below.max() > 0, "the neighbour below is a planted score too, not the zero rows"
    lims, S, I = hr.range_ref(sp, q, thr)
    assert np.array_equal(np.diff(lims), 1 + np.arange(hr.NQ) % 12)
    assert set(sp.high_rows().tolist()) <= set(I.tolist()), "every high planted row is in some query's range result"
    for j in range(hr.NQ):
        seg = I[lims[j]: lims[j + 1]]
        assert np.unique(seg).size == seg.size


# ------------------------------------------------------------------------------------------------ 5: the miniature
def test_the_compressed_references_equal_the_oracle_on_a_dense_miniature():
    sp = hr.miniature()
    dense = sp.dense()
    assert sp.n % 32 == 21 and 2000 < sp.n < 5000 and sp.rule_rows.size <= hr.NQ
    assert {0, 1, 31, 32, sp.n - 22, sp.n - 21, sp.n - 1, 290 - 2, 290 + 3, 288, 288 + 63} <= set(sp.rows.tolist())
    q = np.concatenate([hr.main_queries(sp), hr.ties_queries(sp)])
    scores = oracle.scores_fma(q, dense)
    cleared = hr.masked_rows(sp)
    allowed = np.ones(sp.n, bool)
    allowed[cleared] = False
    for k in (1, hr.K, 100):
        for off in (0, hr.ID_OFFSET):
            want = oracle.topk_fma(q, dense, k, off)
            got = hr.topk_ref(sp, q, k, off)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (k, off)
        masked = scores.copy()
        masked[:, ~allowed] = -np.inf
        want = oracle.topk_of_scores(masked, k, 5)
        got = hr.topk_ref(sp, q, k, 5, allowed=hr.allow_all_but(cleared))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), k
    # range: every row above the threshold, by the dense scores
    main = q[: hr.NQ]
    thr = hr.range_thresholds(sp, main)
    lims, S, I = hr.range_ref(sp, main, thr, 5)
    for j in range(hr.NQ):
        hit = np.flatnonzero(scores[j] > thr[j])
        order = hit[np.lexsort((hit, -scores[j, hit].astype(np.float64)))]
        assert np.array_equal(I[lims[j]: lims[j + 1]], order + 5) and np.array_equal(S[lims[j]: lims[j + 1]], scores[j, order])
    # grouped: the restatement on the dense corpus
    base, pg = hr.planted_groups(sp)
    groups = (np.arange(sp.n) // 32).astype(np.int32)
    groups[sp.rows] = pg
    want = gc.expected(scores[: hr.NQ], groups, hr.K, None, 5, hr.GROUPED_K_ROWS)
    got = hr.grouped_ref(sp, main, hr.K, hr.GROUPED_K_ROWS, 5)
    gc.same(got, want, "grouped")
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]) and not want[4].any()
    # IVF: the exact top-k among the rows of the probed lists
    offsets, small = hr.ivf_lists(sp)
    probe = hr.ivf_probes(sp, hr.NQ)
    S_ivf, I_ivf = hr.ivf_ref(sp, main, probe, hr.K, 5)
    for j in range(hr.NQ):
        inside = np.zeros(sp.n, bool)
        for l in probe[j]:
            inside[offsets[l]: offsets[l + 1]] = True
        s = scores[j: j + 1].copy()
        s[:, ~inside] = -np.inf
        d, i = oracle.topk_of_scores(s, hr.K, 5)
        assert np.array_equal(I_ivf[j], i[0]) and np.array_equal(S_ivf[j].view(np.uint32), d[0].view(np.uint32)), j
    # compaction: the new numbers of the surviving planted rows
    drops = hr.compaction_drops(sp, 100)
    new_rows, values, n_live = hr.compacted(sp, drops)
    keep = np.ones(sp.n, bool)
    keep[drops] = False
    packed = dense[keep]
    assert packed.shape[0] == n_live and np.array_equal(packed[new_rows], values)
    assert int((np.abs(packed).sum(1) > 0).sum()) == new_rows.size and 0 < new_rows.size < sp.P


def test_the_gather_rank_lists_name_every_high_planted_row():
    for which in (1, 2):
        sp = hr.tier(which)
        S, I, c, full = hr.rank_lists(sp, hr.main_queries(sp))
        assert set(sp.rows.tolist()) <= set(I.ravel().tolist())
        zero_named = np.setdiff1d(I[I >= 0], sp.rows)
        assert zero_named.size == 3 and zero_named.min() > sp.boundaries[-1], "zero rows from the high end of the index"
        assert (I >= 0).all() and (np.diff(S.astype(np.float64), axis=1) <= 0).all()
        graph = hr.graph_edges(sp)
        assert np.isin(graph[graph >= 0], sp.rows).all() and (graph[:, :6] >= 0).all()


# ------------------------------------------------------------------------------------------------ 6: size queries
SIZES = (hr.TIER1_N - 1, hr.TIER1_N, hr.TIER2_N, (1 << 31) - 65)


def _plan(fn, *args, outs=3, out_type=C.c_int):
    vals = [out_type(-1) for _ in range(outs)]
    rc = fn(*args, *[C.byref(v) for v in vals])
    return rc, [v.value for v in vals]


def test_workspace_and_plan_queries_at_high_row_counts(native_lib):
    lib = native_lib
    tn = _native.SearchTuning(64, 0, 1)
    sizes = {
        "search": lambda n: lib.sskd_index_search_workspace_bytes(n, hr.NQ, hr.K),
        "search k=100": lambda n: lib.sskd_index_search_workspace_bytes(n, hr.NQ, 100),
        "search_ex": lambda n: lib.sskd_index_search_workspace_bytes_ex(n, hr.NQ, hr.K, C.byref(tn)),
        "onepass": lambda n: lib.sskd_index_search_onepass_workspace_bytes(n, 64, hr.K),
        "screened": lambda n: lib.sskd_index_search_screened_workspace_bytes(n, hr.NQ, hr.K),
        "range": lambda n: lib.sskd_index_range_search_workspace_bytes(n, hr.NQ, 1000),
        "grouped": lambda n: lib.sskd_index_search_grouped_workspace_bytes(n, hr.NQ, hr.K, hr.GROUPED_K_ROWS),
        "bm25": lambda n: lib.sskd_bm25_search_workspace_bytes(n, 4, hr.K),
        "ivf": lambda n: lib.sskd_ivf_search_workspace_bytes(hr.NQ, 4, hr.K, n, 192),
        "pq": lambda n: lib.sskd_pq_search_workspace_bytes(hr.NQ, 4, hr.K, 32, 8, n, 192),
        "plaid": lambda n: lib.sskd_plaid_candidates_workspace_bytes(4, n, 4),
    }
    for name, size in sizes.items():
        got = [int(size(n)) for n in SIZES]
        assert all(0 < g < 1 << 48 for g in got), (name, got)
        assert got == sorted(got), (name, "a size query shrinks as n_rows grows", got)
    # the same queries refuse a shard of 2^31 - 64 rows or more with a zero size (where they refuse at all)
    plans = {
        "search_plan": lambda n: _plan(lib.sskd_index_search_plan, n, hr.NQ, hr.K, outs=5),
        "search_plan_ex": lambda n: _plan(lib.sskd_index_search_plan_ex, n, hr.NQ, hr.K, C.byref(tn), outs=5),
        "screened_plan": lambda n: _plan(lib.sskd_index_search_screened_plan, n, hr.NQ, hr.K, outs=3),
        "screened_plan_claims": lambda n: _plan(lib.sskd_index_search_screened_plan_claims, n, hr.NQ, hr.K, outs=1),
        "bm25_plan": lambda n: _plan(lib.sskd_bm25_search_plan, n, 4, hr.K, outs=3),
        "ivf_plan": lambda n: _plan(lib.sskd_ivf_search_plan, hr.NQ, 4, hr.K, n, 192, outs=3),
    }
    for name, plan in plans.items():
        for n in SIZES:
            rc, vals = plan(n)
            assert rc == 0, (name, n, lib.sskd_last_error())
            assert all(0 <= v < 1 << 30 for v in vals), (name, n, vals)
            assert any(v > 0 for v in vals) or name == "screened_plan_claims", (name, n, vals)
    # the scan plans cover the index: slices x waves (x passes) never drop below one tile each, and the number of
    # slices does not shrink as the index grows
    slices = [plans["search_plan"](n)[1][2] for n in SIZES]
    assert slices == sorted(slices) and slices[0] >= 1, slices
    parts, chunk, cap, ws = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    for n in SIZES:
        assert lib.sskd_pq_search_plan(hr.NQ, 4, hr.K, 32, 8, n, 192, C.byref(parts), C.byref(chunk), C.byref(cap), C.byref(ws)) == 0
        assert parts.value >= 1 and 0 < ws.value < 1 << 48
        need, wgs, th, x = C.c_size_t(0), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        have = int(lib.sskd_plaid_candidates_workspace_bytes(4, n, 4))
        assert lib.sskd_plaid_candidates_plan(4, 32, 64, n, 4, 16, have, C.byref(need), C.byref(wgs), C.byref(th), C.byref(x)) == 0
        assert 0 < need.value <= have and wgs.value >= 1
    assert int(lib.sskd_index_tiled_bytes(hr.TIER2_N)) == (hr.TIER2_N + 11) * hr.ROW_BYTES
    assert int(lib.sskd_index_bf16_bytes(hr.TIER1_N)) == (hr.TIER1_N + 11) // 32 * oracle.SIDECAR_TILE_BYTES + oracle.SIDECAR_NORM_BYTES
    assert int(lib.sskd_row_mask_words(hr.TIER2_N)) == (hr.TIER2_N + 31) // 32
