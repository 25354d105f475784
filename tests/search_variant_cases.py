"""Every compiled variant of the exact, range and screened scans, and the smallest call that reaches it.  No GPU needed.

The search kernels are families of template instances picked at run time.  A variant is identified here by the plan
queries of the C-ABI and the dispatch rule documented in the sources, nothing else:

* ``scan_topk_kernel<K, QB, 8, HAS_UB, POOLS, MASKED>`` (``csrc/search.hip``, ``make_plan`` + ``dispatch_scan_as``):
  K is 10, 16 or 32 by ``min(k, 32)``, and 10 for ``k > 32`` with at most 64 queries; a search of ``ceil(k / K)``
  passes, of which every pass but the first has ``HAS_UB``; QB is 2 for more than 32 queries (or what
  ``sskd_search_tuning.queries_per_block`` says) and always 1 for K = 32; POOLS is a template choice only for K = 10
  (``pruning_pools``, or slices of at least 192 tiles) - K = 16 and K = 32 are compiled with the pools alone; MASKED is
  "a row mask was given".  Seven (K, QB, POOLS) triples x HAS_UB x MASKED = 28 instances.
* ``range_scan_kernel<QB, 8, MASKED>`` (``csrc/range.hip``): QB of the untuned k = 10 plan, MASKED as above: 4 instances.
* ``screen_append_kernel<10, QB, 12, LIGHT, .., MASKED>`` (``csrc/screen.hip``, ``screen_plan``): QB 2 below 256 queries,
  else 4 or 5 by the cost model; LIGHT for slices of at most 330 x 12 tiles; the tiles of a slice are claimed or dealt
  (a run-time switch, forced either way by ``sskd_index_search_screened_claim``): 12 instances x 2.

``test_search_variants_host.py`` holds every row below to the library's own plan, so a change to a plan rule that moves
a row to another variant fails on the CPU; ``test_search_variants_gpu.py`` runs the rows against the oracle.
"""
from collections import namedtuple

TILE_ROWS, SCAN_WAVES, K_PASS = 32, 8, 32
POOLS_AUTO_MIN_TILES_PER_SLICE = 24 * SCAN_WAVES
SCREEN_WAVES, SCREEN_LIGHT_MAX_TILES_PER_SLICE = 12, 330 * 12


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the exact scan
Arm = namedtuple("Arm", "K QB pools has_ub")

# the seven (K, QB, POOLS) triples dispatch_scan_as can name, each compiled with and without HAS_UB (and MASKED)
COMPILED_ARMS = [Arm(K, QB, pools, ub) for K, QB, pools in
                 ((10, 1, False), (10, 2, False), (10, 1, True), (10, 2, True), (16, 1, True), (16, 2, True), (32, 1, True))
                 for ub in (False, True)]

UNREACHABLE_ARMS = {
    Arm(16, 1, True, True): "K = 16 serves 11 <= k <= 16, always one pass; k > 32 chains K = 10 or K = 32 passes",
    Arm(16, 2, True, True): "as above: no second pass ever runs with K = 16",
}


def scan_arms(k, nq, queries_per_block, scan_passes, tiles_per_slice, pruning_pools):
    """The arms a call launches, from the plan the library reports and the dispatch rule: the first pass without an
    upper bound, every later pass with one."""
    kk = min(k, K_PASS)
    K = 10 if kk <= 10 else (16 if kk <= 16 else 32)
    if k > K_PASS and nq <= 64:
        K = 10
    assert scan_passes == ceil_div(k, K), (scan_passes, k, K)
    QB = queries_per_block // 32
    assert QB in (1, 2) and not (K == 32 and QB == 2)
    pools = K != 10 or (pruning_pools > 0 if pruning_pools else tiles_per_slice >= POOLS_AUTO_MIN_TILES_PER_SLICE)
    return {Arm(K, QB, pools, False)} | ({Arm(K, QB, pools, True)} if scan_passes > 1 else set())


# tuning = (queries_per_block, target_workgroups, pruning_pools) of sskd_search_tuning; the last three columns are the
# claims test_search_variants_host.py checks against sskd_index_search_plan_ex.  3 001 = 93 tiles + 25 rows and
# 20 003 = 625 tiles + 3 rows: a ragged last tile in every row.  Forcing the pools on 20 003 rows with 8 workgroups per
# query block gives slices of 79 tiles, ten per wave, so the pools see more than a tile or two.
ScanCase = namedtuple("ScanCase", "name n nq k tuning arms queries_per_block scan_passes tiles_per_slice")

A = Arm
SCAN_CASES = [
    ScanCase("k10_qb1", 3001, 3, 10, (0, 0, 0), {A(10, 1, False, False)}, 32, 1, 8),
    ScanCase("k10_qb2", 3001, 33, 10, (0, 0, 0), {A(10, 2, False, False)}, 64, 1, 8),
    ScanCase("k10_qb1_three_blocks", 3001, 70, 10, (32, 0, 0), {A(10, 1, False, False)}, 32, 1, 8),
    ScanCase("k10_qb1_pools", 20003, 3, 10, (0, 8, 1), {A(10, 1, True, False)}, 32, 1, 79),
    ScanCase("k10_qb2_pools", 20003, 70, 10, (0, 8, 1), {A(10, 2, True, False)}, 64, 1, 79),
    ScanCase("k100_qb1", 3001, 3, 100, (0, 0, 0), {A(10, 1, False, False), A(10, 1, False, True)}, 32, 10, 8),
    ScanCase("k100_qb2", 3001, 33, 100, (0, 0, 0), {A(10, 2, False, False), A(10, 2, False, True)}, 64, 10, 8),
    ScanCase("k100_qb1_pools", 20003, 3, 100, (0, 8, 1), {A(10, 1, True, False), A(10, 1, True, True)}, 32, 10, 79),
    ScanCase("k100_qb2_pools", 20003, 33, 100, (0, 8, 1), {A(10, 2, True, False), A(10, 2, True, True)}, 64, 10, 79),
    ScanCase("k16_qb1", 3001, 3, 16, (0, 0, 0), {A(16, 1, True, False)}, 32, 1, 8),
    ScanCase("k16_qb2", 3001, 33, 16, (0, 0, 0), {A(16, 2, True, False)}, 64, 1, 8),
    ScanCase("k32", 3001, 3, 32, (0, 0, 0), {A(32, 1, True, False)}, 32, 1, 8),
    ScanCase("k32_qb2_asked_for", 3001, 70, 32, (64, 0, 0), {A(32, 1, True, False)}, 32, 1, 8),   # K = 32 keeps QB = 1
    ScanCase("k100_K32", 3001, 70, 100, (0, 0, 0), {A(32, 1, True, False), A(32, 1, True, True)}, 32, 4, 8),
]

# Arms an EXISTING test already holds to the oracle, with the call that test makes: (test, n, nq, k, tuning).
# test_search_variants_host.py checks that the call still lands on the arm; the GPU test adds no case for these.
SCAN_ELSEWHERE_UNMASKED = {
    A(10, 1, False, False): ("test_search_gpu.py::test_search_bit_exact_vs_oracle[31-3-5]", 31, 3, 5, (0, 0, 0)),
    A(10, 2, False, False): ("test_search_gpu.py::test_search_bit_exact_vs_oracle[1003-65-10]", 1003, 65, 10, (0, 0, 0)),
    A(10, 2, True, False): ("test_search_gpu.py::test_search_tuning_struct_changes_plan_not_results", 20000, 130, 10, (64, 16, 1)),
    A(10, 1, False, True): ("test_search_gpu.py::test_large_k_chained_passes[100]", 3000, 5, 100, (0, 0, 0)),
    A(10, 2, False, True): ("test_search_gpu.py::test_online_shapes_few_queries_many_slices[64-100]", 150000, 64, 100, (0, 0, 0)),
    A(16, 2, True, False): ("test_search_gpu.py::test_search_bit_exact_vs_oracle[4099-97-16]", 4099, 97, 16, (0, 0, 0)),
    A(32, 1, True, False): ("test_search_gpu.py::test_search_bit_exact_vs_oracle[5000-7-32]", 5000, 7, 32, (0, 0, 0)),
    A(32, 1, True, True): ("test_search_gpu.py::test_online_shapes_few_queries_many_slices[65-100]", 150000, 65, 100, (0, 0, 0)),
}
SCAN_ELSEWHERE_MASKED = {
    A(10, 2, False, False): ("test_filtered_search_gpu.py::test_filtered_search_every_path_every_mask[5000-100-10-single]",
                             5000, 100, 10, (0, 0, 0)),
    A(32, 1, True, False): ("test_filtered_search_gpu.py::test_filtered_search_every_path_every_mask[3001-200-100-chained]",
                            3001, 200, 100, (0, 0, 0)),
    A(32, 1, True, True): ("test_filtered_search_gpu.py::test_filtered_search_every_path_every_mask[3001-200-100-chained]",
                           3001, 200, 100, (0, 0, 0)),
}


def scan_runs():
    """(case, masked) pairs that launch at least one arm no existing test launches"""
    runs = []
    for case in SCAN_CASES:
        for masked, elsewhere in ((False, SCAN_ELSEWHERE_UNMASKED), (True, SCAN_ELSEWHERE_MASKED)):
            if case.arms - set(elsewhere):
                runs.append((case, masked))
    return runs


# ------------------------------------------------------------------------------------------------ the range scan
# QB comes from the untuned k = 10 plan of (n, nq): 2 above 32 queries.
RangeCase = namedtuple("RangeCase", "name n nq QB")
RANGE_CASES = [RangeCase("range_qb1", 3001, 3, 1), RangeCase("range_qb2", 3001, 33, 2)]

# (QB, masked) -> the existing test and its (n, nq); QB = 1 under a mask is the one arm no test launched
RANGE_ELSEWHERE = {
    (1, False): ("test_range_search_gpu.py::test_range_search_shapes_and_thresholds[31-3]", 31, 3),
    (2, False): ("test_range_search_gpu.py::test_range_search_shapes_and_thresholds[3001-200]", 3001, 200),
    (2, True): ("test_range_search_gpu.py::test_range_search_masks_and_removed_rows", 3001, 37),
}


def range_runs():
    return [(case, masked) for case in RANGE_CASES for masked in (False, True) if (case.QB, masked) not in RANGE_ELSEWHERE]


# --------------------------------------------------------------------------------------------- the screened search
# The smallest shapes that plan each QB, found on the CPU with sskd_index_search_screened_plan over SCREEN_GRID_ROWS x
# nq = 64 .. 19 999 (test_search_variants_host.py repeats the search); the non-LIGHT form needs a slice of more than
# 3 960 tiles, which 127 001 rows in one slice give for 128 and for 160 queries per block.  claims: what the plan does
# on its own at that shape.
ScreenCase = namedtuple("ScreenCase", "name n nq QB light n_slices tiles_per_slice claims")
SCREEN_GRID_ROWS = (2049, 3001, 4099, 6007, 8201, 12001, 16401, 20003, 32771)
SCREEN_CASES = [
    ScreenCase("screen_qb2", 2049, 64, 2, True, 6, 11, False),
    ScreenCase("screen_qb4", 2049, 256, 4, True, 6, 11, False),
    ScreenCase("screen_qb5", 16401, 16385, 5, True, 2, 257, True),
    ScreenCase("screen_qb4_long_slice", 127001, 27226, 4, False, 1, 3969, True),
    ScreenCase("screen_qb5_long_slice", 127001, 32880, 5, False, 1, 3969, True),
]

# (QB, light, masked, claimed) -> the existing test that holds the variant to the exact scan, and its (n, nq)
SCREEN_ELSEWHERE = {
    (2, True, False, True): ("test_screen_tile_claim_gpu.py::test_every_tile_is_screened_once[127-2049-...]", 2049, 127),
    (2, True, False, False): ("test_screened_gpu.py::test_screened_equals_exact_bits[2049-65-10]", 2049, 65),
    (4, True, False, True): ("test_screen_tile_claim_gpu.py::test_every_tile_is_screened_once[383-4099-...]", 4099, 383),
    (4, True, False, False): ("test_screened_gpu.py::test_screened_equals_exact_bits[20000-300-10]", 20000, 300),
    (4, True, True, True): ("test_screen_tile_claim_gpu.py::test_mask_word_follows_the_tile[256-6007-...]", 6007, 256),
    (4, True, True, False): ("test_filtered_search_gpu.py::test_filtered_search_every_path_every_mask[6007-256-10-+screened]",
                             6007, 256),
    (5, True, False, True): ("test_screen_tile_claim_gpu.py::test_every_tile_is_screened_once[16479-32771-...]", 32771, 16479),
    (5, True, True, True): ("test_screen_tile_claim_gpu.py::test_mask_word_follows_the_tile[16479-32771-...]", 32771, 16479),
    (5, False, False, True): ("test_screen_tile_claim_gpu.py::test_every_tile_is_screened_once[32799-127001-...]", 127001, 32799),
    (5, False, True, True): ("test_filtered_search_gpu.py::test_screened_full_size_half_mask_equals_a_subindex", 1_000_000, 10_000),
}

# QB = 2 serves fewer than 256 queries: at most four query blocks, so the plan cuts the shard into its maximum of 42
# slices, and a slice of more than 3 960 tiles needs more than 5.3 M rows.  No shape under 200 000 rows reaches it and
# no existing test is that large with so few queries: these four variants are launched by NO test.
SCREEN_UNTESTED = [(2, False, masked, claimed) for masked in (False, True) for claimed in (False, True)]


def screen_runs():
    return [(case, masked, claimed) for case in SCREEN_CASES for masked in (False, True) for claimed in (True, False)
            if (case.QB, case.light, masked, claimed) not in SCREEN_ELSEWHERE]
