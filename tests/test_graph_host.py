"""Graph index, host side (no GPU): the restatements of ``graph_cases`` against definitions one level plainer, the
files, the remap after ``compact``, the launch plan and the argument checks of ``sskd_graph_search`` /
``sskd_graph_prune`` / ``sskd_graph_merge`` through ctypes (a refused call returns before any HIP call)."""
import ctypes as C
import json

import numpy as np
import pytest

import graph_cases as gc
from oracle import search as oracle
from semantic_search_kd_amd import GraphIndex, graph

SSKD_ERR_INVALID = 1
DIM = 384


# ------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("width", [1, 4, 8])
def test_beam_search_on_a_ring_with_a_wide_beam_is_the_exact_search(width):
    """ef >= N on a connected graph: every row is reached and scored, so the result is the exact top-k."""
    n = 200
    corpus = oracle.seeded_unit_rows(n, DIM, 1)
    queries = oracle.seeded_unit_rows(7, DIM, 2)
    scores = oracle.scores_fma(queries, corpus)
    ring = gc.ring_graph(n, 4)
    seeds = np.full((7, 1), 17)
    for k in (1, 10, 200):
        got_s, got_i, iterations = gc.beam_search_batch_ref(scores, ring, seeds, 256, width, 256, k)
        ref_s, ref_i = oracle.topk_of_scores(scores, k)
        assert np.array_equal(got_i, ref_i) and np.array_equal(got_s.view(np.int32), ref_s.view(np.int32))
        assert (iterations >= -(-n // width)).all() and (iterations <= n).all()   # every row is expanded once
    # a mask: rows outside it are traversed and never returned
    allowed = np.random.default_rng(3).random(n) < 0.3
    got_s, got_i, _ = gc.beam_search_batch_ref(scores, ring, seeds, 256, width, 256, 10, allowed)
    ref_s, ref_i = oracle.topk_of_scores(np.where(allowed[None, :], scores, -np.inf), 10)
    assert np.array_equal(got_i, ref_i) and np.array_equal(got_s.view(np.int32), ref_s.view(np.int32))


def test_beam_search_stops_at_max_iterations_and_pads():
    n = 50
    corpus = oracle.seeded_unit_rows(n, DIM, 4)
    scores = oracle.scores_fma(oracle.seeded_unit_rows(1, DIM, 5), corpus)
    chain = np.full((n, 4), -1, dtype=np.int32)
    chain[:-1, 0] = np.arange(1, n)                       # 0 -> 1 -> 2 ...
    s, i, iterations = gc.beam_search_ref(lambda r: scores[0, r], chain, [0], 16, 1, 5, 10)
    assert iterations == 5 and sorted(i[i >= 0].tolist()) == [0, 1, 2, 3, 4, 5]
    assert (i[6:] == -1).all() and (s[6:] == gc.NEG_PAD).all()


def _detours_by_definition(knn):
    """The definition as a triple loop over (j, i, p), nothing shared with ``detours_ref``."""
    n, K0 = knn.shape
    det = np.full((n, K0), -1, dtype=np.int64)
    for u in range(n):
        for j in range(K0):
            w = knn[u][j]
            if w < 0 or w >= n or w == u:
                continue
            count = 0
            for i in range(j):
                v = knn[u][i]
                if v < 0 or v >= n or v == u:
                    continue
                hit = False
                for p in range(j):
                    if knn[v][p] == w:
                        hit = True
                count += hit
            det[u][j] = count
    return det


def _knn_of(corpus, K0):
    ids = oracle.topk_of_scores(oracle.scores_fma(corpus, corpus), K0 + 1)[1]
    out = np.empty((corpus.shape[0], K0), dtype=np.int32)
    for u, row in enumerate(ids):
        own = np.flatnonzero(row == u)
        out[u] = np.delete(row, own[0] if own.size else K0)
    return out


def test_detours_against_the_definition():
    n, K0, M = 50, 8, 4
    knn = _knn_of(oracle.seeded_unit_rows(n, DIM, 6), K0)
    det, fwd = gc.detours_ref(knn, M)
    want = _detours_by_definition(knn)
    assert np.array_equal(det, want) and want.max() > 0
    for u in range(n):
        order = sorted(range(K0), key=lambda j: (want[u, j], j))[:M]
        assert fwd[u].tolist() == [int(knn[u, j]) for j in order]
    # a list shorter than M (more neighbours asked for than rows exist): -1 padded, -1 entries skipped
    small = _knn_of(oracle.seeded_unit_rows(5, DIM, 7), 8)
    assert (small[:, 4:] == -1).all()
    det, fwd = gc.detours_ref(small, 6)
    assert np.array_equal(det, _detours_by_definition(small))
    assert (fwd[:, 4:] == -1).all() and (fwd[:, :4] >= 0).all()


def test_reverse_and_merge_restated():
    n, K0, M = 50, 8, 4
    knn = _knn_of(oracle.seeded_unit_rows(n, DIM, 6), K0)
    fwd = gc.detours_ref(knn, M)[1]
    rev = gc.reverse_ref(fwd)
    assert rev.shape == (n, M // 2)
    for v in range(n):
        named = sorted((int(np.flatnonzero(fwd[u, :M // 2] == v)[0]), u) for u in range(n) if v in fwd[u, :M // 2])
        assert rev[v][rev[v] >= 0].tolist() == [u for _, u in named[:M // 2]]
    g = gc.merge_ref(fwd, rev)
    for u in range(n):
        row = g[u][g[u] >= 0]
        assert u not in row and len(set(row.tolist())) == row.size                  # no self edge, no edge twice
        assert row[:M // 2].tolist() == fwd[u, :M // 2].tolist()                   # the best forward edges lead
        assert set(row.tolist()) <= set(fwd[u].tolist()) | set(rev[u].tolist())
        assert (g[u][row.size:] == -1).all()


# ------------------------------------------------------------------------------------------ entry rows, files, remap
def test_entry_rows():
    assert [graph.default_n_entry(n, 32) for n in (0, 1, 20, 32, 3001, 10 ** 6)] == [0, 1, 20, 32, 94, 31250]
    assert graph.entry_rows_of(10, 4).tolist() == [0, 2, 5, 7] and graph.entry_rows_of(3, 3).tolist() == [0, 1, 2]
    rows = graph.entry_rows_of(8_841_823, 2973)
    assert rows.dtype == np.int32 and rows[0] == 0 and (np.diff(rows) > 0).all() and rows[-1] < 8_841_823
    with pytest.raises(ValueError):
        graph.entry_rows_of(3, 4)
    for bad in (2, 3, 33, 66, 0):
        with pytest.raises(ValueError):
            graph.check_degree(bad)
    assert graph.check_degree(4) == 4 and graph.check_degree(64) == 64


def test_files_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    g = rng.integers(-1, 200, size=(200, 8)).astype(np.int32)
    entry = graph.entry_rows_of(200, 14)
    graph.save_graph(tmp_path, g, entry, {"knn_k": 16, "ef": 48, "width": 2})
    meta = json.loads((tmp_path / "graph.json").read_text())
    assert meta == {"knn_k": 16, "ef": 48, "width": 2, "M": 8, "format_version": 1}
    assert graph.is_graph_dir(tmp_path) and not graph.is_graph_dir(tmp_path / "nowhere")
    g2, e2, m2 = graph.load_graph(tmp_path)
    assert np.array_equal(g2, g) and g2.dtype == np.int32 and np.array_equal(e2, entry) and e2.dtype == np.int32
    assert m2 == meta
    # damaged files are noticed
    bad = g.copy()
    bad[3, 3] = 200
    np.save(tmp_path / "graph.npy", bad)
    with pytest.raises(ValueError):
        graph.load_graph(tmp_path)
    np.save(tmp_path / "graph.npy", g[:, :7])          # an odd degree
    with pytest.raises(ValueError):
        graph.load_graph(tmp_path)
    np.save(tmp_path / "graph.npy", g)
    np.save(tmp_path / "graph_entry_rows.npy", np.array([0, 200], np.int32))
    with pytest.raises(ValueError):
        graph.load_graph(tmp_path)
    np.save(tmp_path / "graph_entry_rows.npy", entry)
    (tmp_path / "graph.json").write_text(json.dumps({**meta, "format_version": 2}))
    with pytest.raises(ValueError):
        graph.load_graph(tmp_path)


@pytest.mark.parametrize("drop", ["some", "none", "all", "neighbours_of_0"])
def test_remap_graph_after_compact(drop):
    rng = np.random.default_rng(7)
    n, M = 300, 6
    g = rng.integers(0, n, size=(n, M)).astype(np.int32)
    g[rng.random((n, M)) < 0.2] = -1
    gone = {"some": rng.random(n) < 0.3, "none": np.zeros(n, bool), "all": np.ones(n, bool),
            "neighbours_of_0": np.isin(np.arange(n), g[0])}[drop]
    kept = np.flatnonzero(~gone).astype(np.int64)
    got = graph.remap_graph(g, kept)
    assert got.dtype == np.int32 and got.shape == (kept.size, M)
    assert np.array_equal(got, gc.remap_graph_ref(g, kept))
    if drop == "none":
        packed = np.array([sorted(r, key=lambda v: v < 0) for r in g.tolist()], dtype=np.int32)
        assert np.array_equal(got, packed)              # nothing renumbered: only packed to the left
    if drop == "neighbours_of_0" and not gone[0]:
        assert (got[0] == -1).all()


def test_exported():
    assert GraphIndex is graph.GraphIndex


# ------------------------------------------------------------------------------------- the plan, through ctypes
def _plan(lib, nq, k, ef, width, M, n_seeds):
    wgs, threads, lds, rows = (C.c_int(-1) for _ in range(4))
    rc = lib.sskd_graph_search_plan(nq, k, ef, width, M, n_seeds, C.byref(wgs), C.byref(threads), C.byref(lds), C.byref(rows))
    return rc, wgs.value, threads.value, lds.value, rows.value


@pytest.mark.parametrize("nq, k, ef, width, M, n_seeds", [
    (1, 10, 64, 4, 32, 32), (10_000, 1, 1, 1, 4, 1), (65, 256, 256, 8, 64, 256), (3, 16, 16, 2, 6, 16),
])
def test_plan_and_workspace(native_lib, nq, k, ef, width, M, n_seeds):
    rc, wgs, threads, lds, rows = _plan(native_lib, nq, k, ef, width, M, n_seeds)
    assert rc == 0 and wgs == nq and threads == 256 and rows == width * M
    assert 0 < 2 * lds <= 160 * 1024                     # two workgroups share a compute unit's LDS
    assert lds >= 32 * 97 * 16 + 384 * 4 + 2 * 2 * 256 * 8   # a chunk of rows, the query, T and R twice
    assert native_lib.sskd_graph_search_workspace_bytes(nq, k, ef, width, M, n_seeds) == 0   # the state is in LDS
    assert native_lib.sskd_graph_search_plan(nq, k, ef, width, M, n_seeds, None, None, None, None) == 0


@pytest.mark.parametrize("nq, k, ef, width, M, n_seeds", [
    (0, 10, 64, 4, 32, 32), (1, 0, 64, 4, 32, 32), (1, 65, 64, 4, 32, 32), (1, 10, 257, 4, 32, 32), (1, 10, 64, 0, 32, 32),
    (1, 10, 64, 9, 32, 32), (1, 10, 64, 4, 31, 32), (1, 10, 64, 4, 66, 32), (1, 10, 64, 4, 2, 32), (1, 10, 64, 4, 32, 0),
    (1, 10, 64, 4, 32, 257),
])
def test_plan_refuses(native_lib, nq, k, ef, width, M, n_seeds):
    assert _plan(native_lib, nq, k, ef, width, M, n_seeds)[0] == SSKD_ERR_INVALID
    assert native_lib.sskd_last_error()


# ------------------------------------------------------------------- refusal before anything is enqueued, through ctypes
P = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused on the host


def _search_args(**over):
    a = dict(tiled=P, n_rows=1000, graph=P, M=32, queries=P, nq=2, seeds=P, n_seeds=8, seed_rows=None, n_seed_rows=0, k=10,
             ef=64, width=4, max_iterations=64, id_offset=0, mask=None, out_s=P, out_i=P, out_it=None, stream=None)
    a.update(over)
    return [a[key] for key in ("tiled", "n_rows", "graph", "M", "queries", "nq", "seeds", "n_seeds", "seed_rows",
                               "n_seed_rows", "k", "ef", "width", "max_iterations", "id_offset", "mask", "out_s", "out_i",
                               "out_it", "stream")]


@pytest.mark.parametrize("over, word", [
    (dict(k=65), "k=65"), (dict(k=0), "k=0"), (dict(ef=257, k=10), "ef=257"), (dict(ef=0), "ef=0"), (dict(M=31), "M=31"),
    (dict(M=66), "M=66"), (dict(M=2), "M=2"), (dict(width=0), "width=0"), (dict(width=9), "width=9"),
    (dict(max_iterations=0), "max_iterations=0"), (dict(max_iterations=-3), "max_iterations"), (dict(n_seeds=0), "n_seeds=0"),
    (dict(n_seeds=257), "n_seeds=257"), (dict(n_rows=-1), "n_rows"), (dict(nq=-1), "nq"), (dict(id_offset=-1), "id_offset"),
    (dict(n_seed_rows=-1), "n_seed_rows"), (dict(n_rows=(1 << 31) - 64), "int32"),
    (dict(tiled=None), "null"), (dict(graph=None), "null"), (dict(queries=None), "null"), (dict(seeds=None), "null"),
    (dict(out_s=None), "null"), (dict(out_i=None), "null"), (dict(queries=P + 4), "aligned"), (dict(tiled=P + 8), "aligned"),
])
def test_search_refuses_bad_arguments(native_lib, over, word):
    rc = native_lib.sskd_graph_search(*_search_args(**over))
    assert rc == SSKD_ERR_INVALID
    assert word in native_lib.sskd_last_error().decode()


def test_search_with_no_queries_is_a_noop(native_lib):
    assert native_lib.sskd_graph_search(*_search_args(nq=0, queries=None, seeds=None, out_s=None, out_i=None)) == 0


@pytest.mark.parametrize("over, word", [
    (dict(M=5), "M=5"), (dict(M=66), "M=66"), (dict(K0=31), "knn_k=31"), (dict(K0=129), "knn_k=129"), (dict(n_rows=-1), "n_rows"),
    (dict(knn=None), "null"), (dict(fwd=None), "null"), (dict(n_rows=(1 << 31) - 64), "int32"),
])
def test_prune_refuses_bad_arguments(native_lib, over, word):
    a = dict(knn=P, n_rows=100, K0=64, M=32, fwd=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_graph_prune(*[a[key] for key in ("knn", "n_rows", "K0", "M", "fwd", "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_graph_prune(None, 0, 64, 32, None, None) == 0   # no rows: nothing to do


@pytest.mark.parametrize("over, word", [
    (dict(M=7), "M=7"), (dict(M=128), "M=128"), (dict(n_rows=-1), "n_rows"), (dict(fwd=None), "null"), (dict(rev=None), "null"),
    (dict(graph=None), "null"),
])
def test_merge_refuses_bad_arguments(native_lib, over, word):
    a = dict(fwd=P, rev=P, n_rows=100, M=32, graph=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_graph_merge(*[a[key] for key in ("fwd", "rev", "n_rows", "M", "graph", "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_graph_merge(None, None, 0, 32, None, None) == 0
