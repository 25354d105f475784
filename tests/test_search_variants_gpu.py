"""Every compiled variant of the exact, range and screened scans, launched and held to its reference bit for bit.

``search_variant_cases`` names the variants and the smallest call that reaches each; ``test_search_variants_host.py``
checks those claims against the library's plans on the CPU.  This file adds a GPU case only for a variant that no other
test launches; where an existing test already holds a variant to the oracle, the table names it.

``scan_topk_kernel<K, QB, 8, HAS_UB, POOLS, MASKED>`` - reference ``oracle.topk_of_scores(oracle.scores_fma(q, corpus), k)``,
masked rows at -inf.  (K, QB, POOLS, HAS_UB) -> unmasked | masked; ``[name]`` is ``test_exact_scan_variant[name-...]`` here:

  (10, 1, off, no)   test_search_gpu.py::test_search_bit_exact_vs_oracle[31-3-5]           | [k10_qb1-masked], [k10_qb1_three_blocks-masked]
  (10, 2, off, no)   test_search_gpu.py::test_search_bit_exact_vs_oracle[1003-65-10]       | test_filtered_search_gpu.py::test_filtered_search_every_path_every_mask[5000-100-10-single]
  (10, 1, on,  no)   [k10_qb1_pools-unmasked]                                              | [k10_qb1_pools-masked]
  (10, 2, on,  no)   test_search_gpu.py::test_search_tuning_struct_changes_plan_not_results | [k10_qb2_pools-masked]
  (10, 1, off, yes)  test_search_gpu.py::test_large_k_chained_passes[100]                  | [k100_qb1-masked]
  (10, 2, off, yes)  test_search_gpu.py::test_online_shapes_few_queries_many_slices[64-100] | [k100_qb2-masked]
  (10, 1, on,  yes)  [k100_qb1_pools-unmasked]                                             | [k100_qb1_pools-masked]
  (10, 2, on,  yes)  [k100_qb2_pools-unmasked]                                             | [k100_qb2_pools-masked]
  (16, 1, on,  no)   [k16_qb1-unmasked]                                                    | [k16_qb1-masked]
  (16, 2, on,  no)   test_search_gpu.py::test_search_bit_exact_vs_oracle[4099-97-16]       | [k16_qb2-masked]
  (32, 1, on,  no)   test_search_gpu.py::test_search_bit_exact_vs_oracle[5000-7-32]        | test_filtered_search_gpu.py::...[3001-200-100-chained]
  (32, 1, on,  yes)  test_search_gpu.py::test_online_shapes_few_queries_many_slices[65-100] | test_filtered_search_gpu.py::...[3001-200-100-chained]
  (16, 1, on,  yes), (16, 2, on, yes)   compiled, unreachable: 11 <= k <= 16 is one pass, k > 32 chains K = 10 or K = 32

``range_scan_kernel<QB, 8, MASKED>`` - reference and sentinel tail as in ``test_range_search_gpu.py``:

  (1, unmasked)  test_range_search_gpu.py::test_range_search_shapes_and_thresholds[31-3]
  (2, unmasked)  test_range_search_gpu.py::test_range_search_shapes_and_thresholds[3001-200]
  (1, masked)    test_range_scan_variant[range_qb1-masked]
  (2, masked)    test_range_search_gpu.py::test_range_search_masks_and_removed_rows

``screen_append_kernel`` (QB, LIGHT, MASKED, tiles claimed / dealt) - reference: the bits of the exact scan
(``sskd_index_search`` / ``_filtered``) on the same inputs; ``[name]`` is ``test_screened_variant[name-...]`` here:

  (2, light, unmasked)  claimed test_screen_tile_claim_gpu.py::test_every_tile_is_screened_once[127-2049-...], dealt
                        test_screened_gpu.py::test_screened_equals_exact_bits[2049-65-10]
  (2, light, masked)    [screen_qb2-masked], claimed and dealt
  (4, light, unmasked)  claimed test_screen_tile_claim_gpu.py::...[383-4099-...], dealt test_screened_equals_exact_bits[20000-300-10]
  (4, light, masked)    claimed test_screen_tile_claim_gpu.py::test_mask_word_follows_the_tile[256-6007-...], dealt
                        test_filtered_search_gpu.py::test_filtered_search_every_path_every_mask[6007-256-10-+screened]
  (5, light, unmasked)  claimed test_screen_tile_claim_gpu.py::...[16479-32771-...], dealt [screen_qb5-unmasked]
  (5, light, masked)    claimed test_screen_tile_claim_gpu.py::test_mask_word_follows_the_tile[16479-32771-...], dealt [screen_qb5-masked]
  (4, long,  both)      [screen_qb4_long_slice-unmasked], [screen_qb4_long_slice-masked], claimed and dealt
  (5, long,  unmasked)  claimed test_screen_tile_claim_gpu.py::...[32799-127001-...], dealt [screen_qb5_long_slice-unmasked]
  (5, long,  masked)    claimed test_filtered_search_gpu.py::test_screened_full_size_half_mask_equals_a_subindex, dealt
                        [screen_qb5_long_slice-masked]
  (2, long,  both)      NOT RUN by any test: fewer than 256 queries get 42 slices, so a slice of more than 3 960 tiles
                        needs more than 5.3 M rows
"""
import numpy as np
import pytest
import torch

import search_variant_cases as sv
from capi_helpers import stream
from oracle import search as oracle
from semantic_search_kd_amd import FAISSIndexBuilder, _native
from test_filtered_search_gpu import _masks
from test_range_search_gpu import _capi, _ref_from_scores, _same as _same_range, _spread_thresholds
from test_screen_tile_claim_gpu import K as SCREEN_K, Searches, assert_same

pytestmark = pytest.mark.gpu

DIM = 384
MASKS = ("half", "whole_tiles", "fewer_than_k")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def worlds(gpu):
    """n -> (index, 70 queries, their fma-order scores against every row); computed once, never modified"""
    out = {}
    queries = oracle.seeded_unit_rows(70, DIM, 9002)
    for n in sorted({c.n for c in sv.SCAN_CASES} | {c.n for c in sv.RANGE_CASES}):
        corpus = oracle.seeded_unit_rows(n, DIM, 9000 + n)
        index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu))
        index.build_from_embeddings(corpus)
        scores = oracle.scores_fma(queries, corpus)
        scores.setflags(write=False)
        out[n] = (index, queries, scores)
    return out


def _allow_masks(n, k, masked, seed):
    if not masked:
        return {"unmasked": None}
    every = _masks(n, k, np.random.default_rng(seed))
    return {name: every[name] for name in MASKS}


# ------------------------------------------------------------------------------------------------ the exact scan
@pytest.mark.parametrize("case, masked", sv.scan_runs(), ids=lambda v: v.name if isinstance(v, sv.ScanCase) else
                         ("masked" if v else "unmasked"))
def test_exact_scan_variant(worlds, case, masked):
    index, queries, scores = worlds[case.n]
    q = torch.from_numpy(queries[:case.nq]).cuda()
    index.search_tuning = _native.SearchTuning(*case.tuning)   # an explicit tuning also keeps the screened path out
    try:
        for name, allowed in _allow_masks(case.n, case.k, masked, case.n + case.nq + case.k).items():
            s = scores[:case.nq].copy()
            if allowed is not None:
                s[:, ~allowed] = -np.inf
            ref_s, ref_i = oracle.topk_of_scores(s, case.k)
            got_s, got_i = index.search_device(q, case.k, normalize_queries=False, allow=allowed)
            torch.cuda.synchronize()
            assert index.last_status is None   # the exact scan answered
            assert np.array_equal(got_i.cpu().numpy(), ref_i), (case.name, name)
            assert np.array_equal(_bits(got_s.cpu().numpy()), _bits(ref_s)), (case.name, name)
            if name == "fewer_than_k":
                assert (ref_i[:, max(1, case.k // 2):] == -1).all()   # the tail is padding
    finally:
        index.search_tuning = None


# ------------------------------------------------------------------------------------------------ the range scan
@pytest.mark.parametrize("case, masked", sv.range_runs(), ids=lambda v: v.name if isinstance(v, sv.RangeCase) else
                         ("masked" if v else "unmasked"))
def test_range_scan_variant(worlds, native_lib, case, masked):
    index, queries, scores = worlds[case.n]
    q = queries[:case.nq]
    thr = _spread_thresholds(scores[:case.nq])
    for name, allowed in _allow_masks(case.n, 10, masked, case.n + case.nq).items():
        s = scores[:case.nq].copy()
        mask = None
        if allowed is not None:
            s[:, ~allowed] = -np.inf
            mask = index.search_mask(allowed)
        ref = _ref_from_scores(s, thr)
        total = int(ref[0][-1])
        got = _capi(native_lib, index._tiled, case.n, q, thr, max_results=total, buf=total + 64, mask=mask)
        _same_range(got[:3], ref, (case.name, name))
        assert (got[3][total:] == 12345.0).all() and (got[4][total:] == -77).all()   # nothing past the last record


# --------------------------------------------------------------------------------------------- the screened search
_screen_base = {}


def _screen_corpus(n):
    if "c" not in _screen_base:
        rows = oracle.seeded_unit_rows(max(case.n for case in sv.SCREEN_CASES), DIM, 7071)
        rows.setflags(write=False)
        _screen_base["c"] = rows
    return _screen_base["c"][:n]


def _screened(run, claim):
    out_s, out_i = run._out()
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    _native.check(run.lib.sskd_index_search_screened_claim(
        run.tiled.data_ptr(), run.bf.data_ptr(), run.n, run.q.data_ptr(), run.nq, SCREEN_K, 0,
        None if run.mask is None else run.mask.data_ptr(), int(claim), out_s.data_ptr(), out_i.data_ptr(), status.data_ptr(),
        run.ws.data_ptr(), run.ws.numel(), stream(), None, None))
    torch.cuda.synchronize()
    assert status.cpu().numpy()[0] == 0
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def _screen_groups():
    groups = {}
    for case, masked, claimed in sv.screen_runs():
        groups.setdefault((case, masked), []).append(claimed)
    return [(case, masked, tuple(claims)) for (case, masked), claims in groups.items()]


@pytest.mark.parametrize("case, masked, claims", _screen_groups(), ids=lambda v: v.name if isinstance(v, sv.ScreenCase) else
                         ("masked" if v is True else "unmasked" if v is False else "+".join("claimed" if c else "dealt" for c in v)))
def test_screened_variant(gpu, native_lib, case, masked, claims):
    corpus = _screen_corpus(case.n)
    queries = oracle.seeded_unit_rows(case.nq, DIM, 7100 + case.nq)
    planted = (np.arange(case.nq, dtype=np.int64) * 23) % case.n   # a near neighbour per query: the top rank is not trivial
    queries[:] = corpus[planted] + np.float32(0.02) * queries
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    allowed = (np.random.default_rng(case.n + case.nq).random(case.n) < 0.5) if masked else None
    run = Searches(native_lib, corpus, queries, allowed)
    want = run.exact()
    for claimed in claims:
        got = _screened(run, claimed)
        assert_same(got, want)
        if masked:
            assert allowed[got[1]].all()
            kept = allowed[planted]
            assert (got[1][kept, 0] == planted[kept]).all()
