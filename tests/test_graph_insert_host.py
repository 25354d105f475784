"""Graph index, incremental insertion, host side (no GPU): the three exports are declared, bound and exported and refuse
bad arguments before anything is enqueued; the restatements of ``graph_insert_cases`` agree with ``graph_cases`` where the
rules coincide and keep their invariants on small hand-checked graphs; ``n_inserted`` survives ``graph.json``."""
import json
import re

import numpy as np
import pytest

import graph_cases as gc
import graph_insert_cases as gic
from conftest import REPO
from oracle import search as oracle
from semantic_search_kd_amd import GraphIndex, _native, graph

SSKD_ERR_INVALID = 1
DIM = 384
NEW = ("sskd_graph_insert_prune", "sskd_graph_merge_rows", "sskd_graph_link")
P = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused on the host


def test_the_three_symbols_are_declared_bound_and_exported(native_lib):
    header = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sskd_amd.h").read_text(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), f"{name} is not declared"
        assert name in _native.SIGNATURES and hasattr(native_lib, name)
    assert not [s for s in _native.SIGNATURES if s.startswith("sskd_graph_") and s.endswith("_workspace_bytes")
                and s != "sskd_graph_search_workspace_bytes"]   # no workspace, no new size query
    assert hasattr(GraphIndex, "insert")


# ------------------------------------------------------------------- refusal before anything is enqueued, through ctypes
@pytest.mark.parametrize("over, word", [
    (dict(M=5), "M=5"), (dict(M=66), "M=66"), (dict(M=2), "M=2"), (dict(K0=31), "knn_k=31"), (dict(K0=129), "knn_k=129"),
    (dict(n_old=-1), "n_old"), (dict(n_new=-1), "n_new"), (dict(graph_old=None), "null"), (dict(knn_new=None), "null"),
    (dict(fwd_new=None), "null"), (dict(n_old=(1 << 31) - 64), "int32"), (dict(n_old=(1 << 31) - 100, n_new=36), "int32"),
])
def test_insert_prune_refuses_bad_arguments(native_lib, over, word):
    a = dict(graph_old=P, n_old=1000, knn_new=P, n_new=100, K0=64, M=32, fwd_new=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_graph_insert_prune(*[a[key] for key in ("graph_old", "n_old", "knn_new", "n_new", "K0", "M", "fwd_new",
                                                                 "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_graph_insert_prune(P, 1000, None, 0, 64, 32, None, None) == 0   # no new rows: nothing to do


@pytest.mark.parametrize("over, word", [
    (dict(M=7), "M=7"), (dict(M=128), "M=128"), (dict(n_rows=-1), "n_rows"), (dict(row_base=-1), "row_base"),
    (dict(n_total=99), "n_total"), (dict(row_base=950), "n_total"), (dict(fwd=None), "null"), (dict(incoming=None), "null"),
    (dict(out=None), "null"), (dict(n_total=(1 << 31) - 64), "int32"),
])
def test_merge_rows_refuses_bad_arguments(native_lib, over, word):
    a = dict(fwd=P, incoming=P, n_rows=100, row_base=900, n_total=1000, M=32, out=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_graph_merge_rows(*[a[key] for key in ("fwd", "incoming", "n_rows", "row_base", "n_total", "M", "out",
                                                               "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_graph_merge_rows(None, None, 0, 1000, 1000, 32, None, None) == 0


@pytest.mark.parametrize("over, word", [
    (dict(M=9), "M=9"), (dict(M=66), "M=66"), (dict(n_old=-1), "n_old"), (dict(n_total=999), "n_total"),
    (dict(n_touched=-1), "n_touched"), (dict(tiled=None), "null"), (dict(graph=None), "null"), (dict(touched=None), "null"),
    (dict(incoming=None), "null"), (dict(tiled=P + 4), "aligned"), (dict(n_total=(1 << 31) - 64), "int32"),
])
def test_link_refuses_bad_arguments(native_lib, over, word):
    a = dict(tiled=P, graph=P, n_old=1000, n_total=1100, M=32, touched=P, incoming=P, n_touched=10, stream=None)
    a.update(over)
    rc = native_lib.sskd_graph_link(*[a[key] for key in ("tiled", "graph", "n_old", "n_total", "M", "touched", "incoming",
                                                         "n_touched", "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_graph_link(P, P, 1000, 1100, 32, None, None, 0, None) == 0      # nothing touched


# ------------------------------------------------------------------------------------------ the restatements
def _knn_of(corpus, K0):
    return gic.knn_new_ref(corpus, 0, K0)


def test_restatements_coincide_with_the_build_where_the_rules_do():
    n, K0, M = 50, 8, 4
    knn = _knn_of(oracle.seeded_unit_rows(n, DIM, 6), K0)
    det, fwd = gc.detours_ref(knn, M)
    assert det.max() > 0
    # nothing linked yet: every list is a k-NN list, which is the build's prune
    assert np.array_equal(gic.insert_prune_ref(np.empty((0, M), np.int32), knn, M), fwd)
    rev = gc.reverse_ref(fwd)
    assert np.array_equal(gic.merge_rows_ref(fwd, rev, 0, n), gc.merge_ref(fwd, rev))
    incoming_new, touched, incoming_old = gic.incoming_ref(fwd, 0)
    assert np.array_equal(incoming_new, rev) and touched.size == 0 and incoming_old.shape == (0, M // 2)
    # a list shorter than M and -1 entries
    small = _knn_of(oracle.seeded_unit_rows(5, DIM, 7), 8)
    assert np.array_equal(gic.insert_prune_ref(np.empty((0, 6), np.int32), small, 6), gc.detours_ref(small, 6)[1])


def test_insert_prune_looks_a_neighbour_up_in_its_own_table():
    """Hand-checked, M 4, K0 4, two linked rows and two new ones (ids 2 and 3)."""
    graph_old = np.array([[1, 3, -1, -1],        # N(0): width M
                          [0, -1, -1, -1]], np.int32)
    knn_new = np.array([[0, 3, 1, -1],           # L of row 2
                        [2, 1, 0, 2]], np.int32)  # L of row 3 (a repeat of 2 in the last place)
    fwd = gic.insert_prune_ref(graph_old, knn_new, 4)
    # row 2: 0 has no detour; 3: N(0)[:1] = [1] does not name it -> 0; 1: N(0)[:2] = [1, 3] names it (1 detour), and so
    # does N(3)[:2] = [2, 1] -> 2 detours
    assert fwd[0].tolist() == [0, 3, 1, -1]
    # row 3: 2 -> 0; 1: N(2)[:1] = [0] -> 0; 0: N(2)[:2] = [0, 3] names it, N(1)[:2] = [0, -1] names it -> 2;
    # the second 2: N(2) never names 2, N(1) no, N(0)[:3] = [1, 3, -1] no -> 0 detours, placed by j
    assert fwd[1].tolist() == [2, 1, 2, 0]


def test_merge_rows_uses_global_ids():
    fwd = np.array([[7, 5, 1, 6], [5, 9, 5, 0]], np.int32)        # rows 5 and 6 of 8
    incoming = np.array([[6, 1], [6, -1]], np.int32)
    out = gic.merge_rows_ref(fwd, incoming, 5, 8)
    assert out[0].tolist() == [7, 6, 1, -1]                       # row 5: its own id dropped, 6 once
    assert out[1].tolist() == [5, 0, -1, -1]                      # row 6: 9 is outside [0, 8), 6 is itself
    assert np.array_equal(gic.merge_rows_ref(fwd, incoming, 0, 2)[0], [1, -1, -1, -1])   # the same lists as rows 0, 1 of 2


def test_link_keeps_the_head_and_selects_the_rest_by_score():
    rng = np.random.default_rng(5)
    n0, b, M = 40, 12, 8
    h = M // 2
    rows = oracle.seeded_unit_rows(n0 + b, DIM, 8)
    graph_full = np.concatenate([gc.random_adjacency(n0, M, 9), np.full((b, M), -1, np.int32)])
    graph_full[3] = [5, 6, -1, -1, -1, -1, -1, -1]                # room, nothing evicted
    touched = np.array([1, 3, 7, 7, 45, 20, 19, -2], np.int32)    # a repeat, a new row, rows after a larger entry, a negative
    incoming = rng.integers(n0, n0 + b, size=(touched.size, h)).astype(np.int32)
    incoming[0] = [41, 41, 1, n0 + b]                             # a repeat, a self edge, out of range
    out = gic.link_ref(rows, graph_full, n0, touched, incoming)
    changed = [u for u in range(n0 + b) if not np.array_equal(out[u], graph_full[u])]
    assert set(changed) <= {1, 3, 7} and 3 in changed              # 20 follows 45 and 19 follows 20: left alone
    assert out[3].tolist()[:2] == [5, 6] and sorted(v for v in out[3][2:].tolist() if v >= 0) == sorted(set(incoming[1].tolist()))
    for t, u in ((0, 1), (1, 3), (2, 7)):
        old = [int(v) for v in graph_full[u]]
        adj = [v for i, v in enumerate(old) if 0 <= v < n0 + b and v != u and v not in old[:i]]
        row = out[u][out[u] >= 0].tolist()
        assert row[:len(adj[:h])] == adj[:h] and u not in row and len(set(row)) == len(row)   # head kept, no self, no repeat
        assert (out[u][len(row):] == -1).all()
        allowed = set(adj) | {int(v) for v in incoming[t] if 0 <= v < n0 + b}
        assert set(row) <= allowed
        pool = [v for v in allowed if v not in adj[:h] and v != u]
        assert len(row) == min(M, len(adj[:h]) + len(pool))
        # what follows the head is in rank order, and everything left out ranks after the last one kept
        s = {v: float(oracle.scores_fma(rows[u:u + 1], rows[[v]])[0, 0]) for v in pool}
        tail = row[len(adj[:h]):]
        assert tail == sorted(tail, key=lambda v: (-s[v], v))
        assert all((-s[v], v) > (-s[tail[-1]], tail[-1]) for v in pool if v not in tail)
        # the order inside incoming matters only through repeats: permuting it changes nothing
        shuffled = incoming.copy()
        shuffled[t] = shuffled[t][::-1]
        assert np.array_equal(gic.link_ref(rows, graph_full, n0, touched, shuffled)[u], out[u])


def test_link_ranks_nan_last_and_ties_by_id():
    n0, M = 6, 4
    rows = oracle.seeded_unit_rows(10, DIM, 12)
    rows[7] = rows[8]                      # an exact tie
    rows[9, 5] = np.nan
    graph_full = np.full((10, M), -1, np.int32)
    graph_full[0] = [1, 2, 9, 3]
    out = gic.link_ref(rows, graph_full, n0, np.array([0], np.int32), np.array([[8, 7]], np.int32))
    assert out[0].tolist()[:2] == [1, 2]
    s = oracle.scores_fma(rows[0:1], rows)[0]
    assert np.isnan(s[9]) and s[7] == s[8]
    ranked = sorted([3, 7, 8], key=lambda v: (-float(s[v]), v))
    assert out[0].tolist()[2:] == ranked[:2] and 9 not in out[0]
    # with room for everything the NaN row comes last
    graph_full[0] = [1, 9, -1, -1]
    assert gic.link_ref(rows, graph_full, n0, np.array([0], np.int32), np.array([[7, -1]], np.int32))[0].tolist() == [1, 9, 7, -1]
    graph_full[0] = [1, 2, 9, -1]
    assert gic.link_ref(rows, graph_full, n0, np.array([0], np.int32), np.array([[8, 7]], np.int32))[0].tolist()[2:] == [7, 8]
    graph_full[0] = [1, -1, -1, -1]
    assert gic.link_ref(rows, graph_full, n0, np.array([0], np.int32), np.array([[9, 8]], np.int32))[0].tolist() == [1, 8, 9, -1]


def test_entry_rows_after_an_insert():
    old = graph.entry_rows_of(100, 25)
    got = gic.entry_rows_after_insert_ref(old, 100, 10, 4)
    assert got.dtype == np.int32 and got[:25].tolist() == old.tolist() and got[25:].tolist() == [100, 103, 106]
    assert gic.entry_rows_after_insert_ref(old, 100, 1, 32)[25:].tolist() == [100]
    assert gic.entry_rows_after_insert_ref(old, 100, 10, 4, n_entry=50)[25:].tolist() == [100, 102, 104, 106, 108]
    assert gic.entry_rows_after_insert_ref(old, 100, 3, 4, n_entry=1000)[25:].tolist() == [100, 101, 102]   # at most b
    for b, n0, M, want in ((10, 100, 4, None), (1, 100, 32, None), (10, 100, 4, 50), (3, 100, 4, 1000), (2000, 50, 4, None),
                           (997, 19003, 32, 7)):
        e = graph.n_entry_of_insert(b, n0, M, want)
        assert e == gic.entry_rows_after_insert_ref(np.empty(0, np.int32), n0, b, M, want).size
        assert np.array_equal(gic.entry_rows_after_insert_ref(np.empty(0, np.int32), n0, b, M, want),
                              n0 + graph.entry_rows_of(b, e))


def test_whole_insert_restated_on_a_small_corpus():
    """20 rows + 9: the new rows' lists mix both tables, old rows are relinked, nothing else moves."""
    n0, b, K0, M = 20, 9, 8, 4
    corpus = oracle.seeded_unit_rows(n0 + b, DIM, 13)
    knn = _knn_of(corpus[:n0], K0)
    fwd = gc.detours_ref(knn, M)[1]
    graph_old = gc.merge_ref(fwd, gc.reverse_ref(fwd))
    r = gic.insert_ref(corpus, graph_old, graph.entry_rows_of(n0, 5), K0)
    assert r.knn_new.shape == (b, K0) and (r.knn_new >= n0).any() and (r.knn_new < n0).any()
    assert r.touched.size and (np.diff(r.touched) > 0).all() and r.touched.max() < n0
    untouched = np.setdiff1d(np.arange(n0), r.touched)
    assert np.array_equal(r.graph[untouched], graph_old[untouched])
    assert np.array_equal(r.graph[n0:], r.new_rows)
    for u, row in enumerate(r.graph):
        real = row[row >= 0]
        assert u not in real and np.unique(real).size == real.size and (real < n0 + b).all()
    for t, u in enumerate(r.touched):
        assert np.array_equal(r.graph[u][:M // 2], graph_old[u][:M // 2])
        assert set(r.graph[u].tolist()) <= set(graph_old[u].tolist()) | set(r.incoming_old[t].tolist())
    assert (r.graph[r.touched] >= n0).any()            # new rows did get linked into old ones
    assert r.entry_rows.tolist() == [0, 4, 8, 12, 16, 20, 23, 26]


# ------------------------------------------------------------------------------------------ graph.json
def test_n_inserted_round_trip(tmp_path):
    g = gc.ring_graph(30, 4)
    entry = graph.entry_rows_of(30, 8)
    graph.save_graph(tmp_path, g, entry, {"knn_k": 8, "ef": 64, "width": 4, "n_inserted": 7})
    meta = graph.load_graph(tmp_path)[2]
    assert meta["n_inserted"] == 7 and meta["format_version"] == graph.FORMAT_VERSION == 1
    graph.save_graph(tmp_path, g, entry, {"knn_k": 8, "ef": 64, "width": 4})
    assert "n_inserted" not in json.loads((tmp_path / "graph.json").read_text())
    assert int(graph.load_graph(tmp_path)[2].get("n_inserted", 0)) == 0
