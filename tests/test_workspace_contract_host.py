"""The workspace contract's test machinery, checked on the CPU (``workspace_cases``; the GPU side is
``test_workspace_contract_gpu.py``).

* Completeness: every size query of ``_native``'s signature table has a case, so a new workspace-taking entry point
  without one fails here.
* Sharpness: ``guarded`` and ``check_fill`` run on CPU tensors against fake entry points written in torch.  One reads a
  workspace byte nobody wrote into its output, one writes a single byte past its workspace, one behaves.  No real
  kernel is broken to prove that the test can fail.
* The plan claims the cases rest on: the reduce-buffer shape of the exact search is the smallest whose plan leaves more
  than ``MERGE_DIRECT_MAX_LISTS`` lists per query, the scan rows taken from ``search_variant_cases`` exist, and the
  search-family worlds are what the module says they are.
"""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import search_variant_cases as sv
import workspace_cases as wc
from semantic_search_kd_amd import _native


# ------------------------------------------------------------------------------------------------ completeness
def _size_queries():
    return sorted(name for name in _native.SIGNATURES if name.endswith(("_workspace_bytes", "_workspace_bytes_ex")))


def test_every_size_query_has_a_case():
    queries = _size_queries()
    assert len(queries) == 17, queries
    assert sorted(wc.CASES) == queries
    for entry, shapes in wc.CASES.items():
        assert shapes, entry
        names = [s.name for s in shapes]
        assert len(set(names)) == len(names), (entry, names)
        for s in shapes:
            assert callable(s.setup) and isinstance(s.deterministic, bool) and isinstance(s.reference, str) and s.reference


def test_the_header_declares_the_same_size_queries_and_states_the_contract():
    header = (Path(__file__).resolve().parent.parent / "include" / "sskd_amd.h").read_text()
    declared = sorted(set(re.findall(r"^size_t (sskd_\w+_workspace_bytes(?:_ex)?)\(", header, flags=re.M)))
    assert declared == _size_queries()
    conventions = header[: header.index("#ifndef SSKD_AMD_H")]
    assert "may hold anything on entry" in conventions and "unspecified" in conventions


def test_the_shapes_the_issue_names_are_there():
    ex = {s.name for s in wc.CASES["sskd_index_search_workspace_bytes_ex"]}
    for row in ("k10_qb1", "k10_qb2", "k100_qb1", "k16_qb1", "k32", "k100_K32", "k10_qb1_pools"):
        assert {f"{row}-masked", f"{row}-unmasked"} <= ex, row
        assert row in {c.name for c in sv.SCAN_CASES}
    screened = {s.name for s in wc.CASES["sskd_index_search_screened_workspace_bytes"]}
    for c in sv.SCREEN_CASES:
        assert {f"{c.name}-dealt", f"{c.name}-claimed"} <= screened
    assert any(n.startswith("band_sweep_fallback") for n in screened)
    assert wc.FILLS == (0x00, 0xFF, 0x7F, "leftover") and wc.GUARD_BYTE not in wc.BYTE_FILLS


# ------------------------------------------------------------------------------------------------ the guard
@pytest.mark.parametrize("need", [0, 1, 255, 256, 4097])
def test_guarded_hands_out_exactly_need_bytes_between_two_guards(need):
    for fill in wc.BYTE_FILLS:
        g = wc.guarded(need, fill, "cpu")
        assert g.ptr % 256 == 0 and g.need == need and g.ptr == g.buf.data_ptr() + g.offset
        assert g.offset >= 4096 and g.buf.numel() - (g.offset + need) >= 4096
        assert g.intact()
        body = g.view()
        assert body.numel() == need and bool((body == fill).all())
        assert int((g.buf == wc.GUARD_BYTE).sum()) == g.buf.numel() - need
        body.fill_(0x11)                       # the call's own bytes are its to write
        assert g.intact()
    g = wc.guarded(need, 0x00, "cpu")
    g.buf[g.offset + need] = 0
    assert not g.intact(), "the first byte past the workspace"
    g = wc.guarded(need, 0x00, "cpu")
    g.buf[g.offset - 1] = 0
    assert not g.intact(), "the last byte before the workspace"
    g = wc.guarded(need, 0x00, "cpu")
    g.buf[-1] = 0
    assert not g.intact(), "the last guard byte"


# ------------------------------------------------------------------------------------------------ fake entry points
NEED = 1000
VALUES = torch.arange(8, dtype=torch.float32) - 20.0       # every true value is negative, like query 0 of the worlds


def _well_behaved(g):
    """uses its workspace the way a kernel should: writes a slot, then reads it"""
    ws = g.view()
    ws[:32] = torch.arange(32, dtype=torch.uint8)
    return (VALUES.numpy().copy(), ws[:32].numpy().astype(np.int64).copy())


def _reads_a_slot_nobody_wrote(g):
    """its output starts with ws[0], which this call never wrote"""
    out = VALUES.numpy().copy()
    out[0] = float(g.view()[0])
    return (out, np.arange(32, dtype=np.int64))


def _writes_one_byte_past_its_workspace(g):
    g.buf[g.offset + g.need] = 7
    return _well_behaved(g)


def _prior(g):
    g.view().fill_(0x33)          # what an earlier call on another world left behind


def _run_all(fake):
    base, problems = wc.check_fill("fake", "cpu", 0x00, fake, NEED, "cpu", prior=_prior)
    every = list(problems)
    for fill in wc.FILLS[1:]:
        every += wc.check_fill("fake", "cpu", fill, fake, NEED, "cpu", baseline=base, prior=_prior)[1]
    return every


def test_a_well_behaved_entry_point_passes_every_fill():
    assert _run_all(_well_behaved) == []


def test_reading_an_unwritten_slot_is_flagged_and_named():
    problems = _run_all(_reads_a_slot_nobody_wrote)
    assert problems, "a result that depends on the workspace's contents went unnoticed"
    assert len(problems) == 3, problems          # 0xFF, 0x7F and the leftover each give another value than 0x00
    for p, fill in zip(problems, ("0xFF", "0x7F", "leftover")):
        assert p.startswith(f"fake[cpu] fill={fill}:") and "output 0" in p and "element (0,)" in p, p


def test_a_reference_assertion_catches_the_zero_fill_too():
    """under 0x00 the stale slot reads 0.0, which beats every negative true value: only the reference sees that"""
    def reference(outs):
        assert np.array_equal(outs[0], VALUES.numpy()), "values differ from the reference"

    _, problems = wc.check_fill("fake", "cpu", 0x00, _reads_a_slot_nobody_wrote, NEED, "cpu", reference=reference)
    assert len(problems) == 1 and "the reference assertion fails" in problems[0] and "fill=0x00" in problems[0]
    assert wc.check_fill("fake", "cpu", 0x00, _well_behaved, NEED, "cpu", reference=reference)[1] == []


def test_one_byte_past_the_workspace_is_flagged():
    g = wc.guarded(NEED, 0x00, "cpu")
    _writes_one_byte_past_its_workspace(g)
    assert not g.intact()
    problems = _run_all(_writes_one_byte_past_its_workspace)
    assert len(problems) == 4 and all(f"byte {NEED} relative to a {NEED}-byte workspace was written" in p for p in problems), problems


def test_a_non_deterministic_entry_point_is_not_held_to_the_zero_run():
    calls = []

    def noisy(g):
        calls.append(1)
        return (np.array([float(len(calls))], np.float32),)

    base, _ = wc.check_fill("fake", "cpu", 0x00, noisy, NEED, "cpu")
    assert wc.check_fill("fake", "cpu", 0xFF, noisy, NEED, "cpu", baseline=base, deterministic=False)[1] == []
    assert len(wc.check_fill("fake", "cpu", 0xFF, noisy, NEED, "cpu", baseline=base, deterministic=True)[1]) == 1
    # a diagnostic word left out of the comparison
    assert wc.check_fill("fake", "cpu", 0xFF, noisy, NEED, "cpu", baseline=base, stable=lambda o: ())[1] == []


def test_first_difference_compares_bits():
    nan_a = np.array([np.nan, 1.0], np.float32)
    nan_b = nan_a.copy()
    assert wc.first_difference((nan_a,), (nan_b,)) is None                      # equal NaN patterns are equal
    nan_b.view(np.uint32)[0] ^= 1
    assert wc.first_difference((nan_a,), (nan_b,))[:2] == (0, (0,))              # another NaN payload is not
    assert wc.first_difference((np.array([0.0], np.float32),), (np.array([-0.0], np.float32),))[:2] == (0, (0,))
    a = np.zeros((3, 4), np.int64)
    b = a.copy()
    b[2, 1] = 5
    assert wc.first_difference((a, a), (a, b)) == (1, (2, 1), 0, 5)
    assert wc.first_difference((a,), (a.astype(np.int32),))[1] is None           # dtype or shape: no element to name
    assert wc.first_difference((a,), (a, a))[0] == 1


# ------------------------------------------------------------------------------------------------ plan claims
def test_the_reduce_buffer_shape_is_the_smallest_that_has_reduce_buffers(native_lib):
    """the exact search reduces its per-lane lists through the red_* buffers only above 64 lists per query"""
    lists = lambda n: wc.lists_per_query(native_lib, n, wc.REDUCE_NQ, wc.REDUCE_K)   # noqa: E731
    first = next(n for n in range(1, 5000) if lists(n) > wc.MERGE_DIRECT_MAX_LISTS)
    assert first == wc.REDUCE_MIN_ROWS and first % sv.TILE_ROWS != 0
    assert lists(first) == 80 and lists(first - 1) == wc.MERGE_DIRECT_MAX_LISTS
    shape = {s.name: s for s in wc.CASES["sskd_index_search_workspace_bytes"]}["reduce_buffers"]
    assert shape.deterministic
    # the workspace grows by the two ping-pong pairs exactly there
    ws = native_lib.sskd_index_search_workspace_bytes
    assert ws(first, wc.REDUCE_NQ, wc.REDUCE_K) - ws(first - 1, wc.REDUCE_NQ, wc.REDUCE_K) > 4 * 256
    # the scan rows borrowed from search_variant_cases all reduce as well (3 001 rows: 12 slices)
    for c in sv.SCAN_CASES:
        assert wc.lists_per_query(native_lib, c.n, c.nq, c.k, c.tuning) > wc.MERGE_DIRECT_MAX_LISTS or c.tuning[1], c.name


def test_the_graph_search_has_no_workspace(native_lib):
    for args in ((1, 1, 1, 1, 4, 1), (5, 10, 64, 4, 32, 16), (65, 256, 256, 8, 64, 256)):
        assert native_lib.sskd_graph_search_workspace_bytes(*args) == 0


def test_the_search_worlds_make_stale_values_visible():
    from oracle import search as oracle

    for n in (31, 1025, 3001):
        corpus, queries, corpus_big, queries_big = wc.world_arrays(n)
        assert n % 32 != 0 and corpus.shape == (n, wc.DIM) and queries.shape == (wc.WORLD_NQ, wc.DIM)
        norms = np.linalg.norm(corpus, axis=1)
        assert norms.max() / norms.min() > 1.2, "the corpus must not be normalised"
        s = oracle.scores_fma(queries, corpus)
        assert (s[0] < 0).all(), "query 0 points away from the corpus mean: every score is negative"
        assert (s[2:] > 0).any()
        assert oracle.scores_fma(queries_big[:3], corpus_big).min() > max(10.0, s.max())
    ks = {(s.name, s.reference) for s in wc.CASES["sskd_index_search_workspace_bytes"]}
    assert ("n1_k10", wc.ORACLE_BITS) in ks and ("n31_k10", wc.ORACLE_BITS) in ks     # k above the number of rows
