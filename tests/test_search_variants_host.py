"""The variant table of ``search_variant_cases`` against the library's own plans (no GPU: the plan queries are host code).

Every row claims which compiled variant its call launches.  The claim is checked here from ``sskd_index_search_plan_ex``
/ ``sskd_index_search_screened_plan`` and the documented dispatch rule, so a later change to a plan rule that silently
moves a row to another variant - and with it shrinks what the GPU tests cover - fails here."""
import ctypes as C

import pytest

import search_variant_cases as sv
from semantic_search_kd_amd import _native


def _scan_plan(lib, n, nq, k, tuning):
    tn = _native.SearchTuning(*tuning)
    qpb, passes, slices, waves, scan_passes = (C.c_int(-1) for _ in range(5))
    _native.check(lib.sskd_index_search_plan_ex(n, nq, k, C.byref(tn), C.byref(qpb), C.byref(passes), C.byref(slices),
                                                C.byref(waves), C.byref(scan_passes)))
    assert waves.value == sv.SCAN_WAVES
    return qpb.value, scan_passes.value, sv.ceil_div(sv.ceil_div(n, sv.TILE_ROWS), slices.value)


def _screen_plan(lib, n, nq):
    qpb, passes, slices, claims = (C.c_int(-1) for _ in range(4))
    if lib.sskd_index_search_screened_plan(n, nq, 10, C.byref(qpb), C.byref(passes), C.byref(slices)) != 0:
        return None
    _native.check(lib.sskd_index_search_screened_plan_claims(n, nq, 10, C.byref(claims)))
    tps = sv.ceil_div(sv.ceil_div(n, sv.TILE_ROWS), slices.value)
    return qpb.value // 32, tps <= sv.SCREEN_LIGHT_MAX_TILES_PER_SLICE, slices.value, tps, bool(claims.value)


# ------------------------------------------------------------------------------------------------ the exact scan
@pytest.mark.parametrize("case", sv.SCAN_CASES, ids=lambda c: c.name)
def test_scan_case_reaches_the_arms_it_names(native_lib, case):
    qpb, passes, tps = _scan_plan(native_lib, case.n, case.nq, case.k, case.tuning)
    assert (qpb, passes, tps) == (case.queries_per_block, case.scan_passes, case.tiles_per_slice)
    assert sv.scan_arms(case.k, case.nq, qpb, passes, tps, case.tuning[2]) == case.arms
    assert case.n % sv.TILE_ROWS != 0 and 1000 <= case.n <= 20003   # a ragged last tile, a corpus of a few thousand rows
    # the untuned call and the call with an all-zero tuning struct are planned alike
    if case.tuning == (0, 0, 0):
        plain = [C.c_int(-1) for _ in range(5)]
        _native.check(native_lib.sskd_index_search_plan(case.n, case.nq, case.k, *[C.byref(x) for x in plain]))
        assert (plain[0].value, plain[4].value) == (qpb, passes)


def test_every_compiled_scan_arm_is_reached_or_explained():
    reached = set().union(*(c.arms for c in sv.SCAN_CASES))
    assert reached | set(sv.UNREACHABLE_ARMS) == set(sv.COMPILED_ARMS) and not reached & set(sv.UNREACHABLE_ARMS)
    assert len(sv.COMPILED_ARMS) * 2 == 28   # x MASKED
    # every reached arm runs masked and unmasked: in a new case, or in the existing test the table names
    new = {(arm, masked) for case, masked in sv.scan_runs() for arm in case.arms}
    for arm in reached:
        assert (arm, False) in new or arm in sv.SCAN_ELSEWHERE_UNMASKED, arm
        assert (arm, True) in new or arm in sv.SCAN_ELSEWHERE_MASKED, arm


@pytest.mark.parametrize("elsewhere", [sv.SCAN_ELSEWHERE_UNMASKED, sv.SCAN_ELSEWHERE_MASKED], ids=["unmasked", "masked"])
def test_the_existing_tests_the_table_names_still_reach_their_arms(native_lib, elsewhere):
    for arm, (test, n, nq, k, tuning) in elsewhere.items():
        qpb, passes, tps = _scan_plan(native_lib, n, nq, k, tuning)
        assert arm in sv.scan_arms(k, nq, qpb, passes, tps, tuning[2]), test


def test_no_call_reaches_the_arms_listed_as_unreachable(native_lib):
    """K = 16 with an upper bound: whatever k, nq and tuning, a plan with K = 16 has one pass"""
    for k in list(range(1, 70)) + [100, 256, 1000, 2048]:
        for nq in (1, 32, 33, 64, 65, 200):
            for tuning in ((0, 0, 0), (32, 0, 1), (64, 0, -1)):
                qpb, passes, tps = _scan_plan(native_lib, 20003, nq, k, tuning)
                assert not sv.scan_arms(k, nq, qpb, passes, tps, tuning[2]) & set(sv.UNREACHABLE_ARMS), (k, nq, tuning)


# ------------------------------------------------------------------------------------------------ the range scan
def test_range_cases_and_the_tests_named_for_them(native_lib):
    assert {(c.QB, m) for c in sv.RANGE_CASES for m in (False, True)} == {(1, False), (1, True), (2, False), (2, True)}
    for case in sv.RANGE_CASES:
        assert _scan_plan(native_lib, case.n, case.nq, 10, (0, 0, 0))[0] == 32 * case.QB and case.n % sv.TILE_ROWS != 0
    for (QB, _), (test, n, nq) in sv.RANGE_ELSEWHERE.items():
        assert _scan_plan(native_lib, n, nq, 10, (0, 0, 0))[0] == 32 * QB, test
    assert [(c.QB, m) for c, m in sv.range_runs()] == [(1, True)]


# --------------------------------------------------------------------------------------------- the screened search
@pytest.mark.parametrize("case", sv.SCREEN_CASES, ids=lambda c: c.name)
def test_screen_case_plans_the_variant_it_names(native_lib, case):
    assert _screen_plan(native_lib, case.n, case.nq) == (case.QB, case.light, case.n_slices, case.tiles_per_slice, case.claims)
    assert case.n % sv.TILE_ROWS != 0 and case.n >= 2048 and case.nq >= 64 and case.n < 200_000


def test_the_light_screen_cases_are_the_smallest_that_plan_their_queries_per_block(native_lib):
    """rows ascending over the grid, then queries ascending: the first shape that plans each QB"""
    first = {}
    for n in sv.SCREEN_GRID_ROWS:
        for nq in range(64, 20000):
            got = _screen_plan(native_lib, n, nq)
            if got is not None and got[0] not in first:
                first[got[0]] = (n, nq)
        if len(first) == 3:
            break
    assert first == {c.QB: (c.n, c.nq) for c in sv.SCREEN_CASES if c.light}


def test_every_screen_variant_is_run_named_or_listed_as_untested(native_lib):
    new = {(c.QB, c.light, masked, claimed) for c, masked, claimed in sv.screen_runs()}
    every = {(QB, light, masked, claimed) for QB in (2, 4, 5) for light in (True, False) for masked in (False, True)
             for claimed in (False, True)}
    assert new | set(sv.SCREEN_ELSEWHERE) | set(sv.SCREEN_UNTESTED) == every
    assert not new & set(sv.SCREEN_ELSEWHERE) and not (new | set(sv.SCREEN_ELSEWHERE)) & set(sv.SCREEN_UNTESTED)
    for (QB, light, _, claimed), (test, n, nq) in sv.SCREEN_ELSEWHERE.items():
        got = _screen_plan(native_lib, n, nq)
        assert got[:2] == (QB, light), test
        # the tile-claim tests force claiming where the plan deals; every other test named takes the plan's choice
        assert got[4] == claimed or "test_screen_tile_claim_gpu" in test, test
    # QB = 2 never gets a long slice below 200 000 rows
    for nq in (64, 127, 255):
        for n in (127001, 199999):
            assert _screen_plan(native_lib, n, nq)[:2] == (2, True)
