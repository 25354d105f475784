"""Near-duplicate clusters, the parts that need no GPU: the restatement of the rule against brute-force reachability,
``cluster_pairs`` against the restatement, the argument checks of the three C entry points, and the Python wrappers'
refusal of unknown rules before they touch a device."""
import numpy as np
import pytest

import dedup_cases as cases

NEW_SYMBOLS = ["sskd_dup_init", "sskd_dup_link", "sskd_dup_labels"]
A, B, C, D, E = (0x10_0000_0000 + k * 0x1_0000_0000 for k in range(5))   # never dereferenced: every call fails its checks
KEYS = ("parent", "degree", "rep", "size", "counts")


def _same(got, want, what):
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])


def test_restatement_equals_reachability_on_every_graph_of_five_vertices():
    groups = np.array([0, 1, 0, 1, 2])
    take = np.array([True, True, False, True, True])
    for edges in cases.all_graphs(5):
        for keep in (0, 1):
            _same(cases.restate(5, edges, keep=keep), cases.reach(5, edges, keep=keep), (edges, keep))
        for scope in (1, 2):
            _same(cases.restate(5, edges, take, groups, scope, 1), cases.reach(5, edges, take, groups, scope, 1),
                  (edges, scope))


def test_restatement_equals_reachability_on_random_graphs():
    rng = np.random.default_rng(7)
    for _ in range(300):
        n, edges, take, groups = cases.random_graph(rng)
        for scope in (0, 1, 2):
            for keep in (0, 1):
                _same(cases.restate(n, edges, take, groups, scope, keep), cases.reach(n, edges, take, groups, scope, keep),
                      (n, edges, scope, keep))


def test_the_tie_rule_of_densest():
    """A path 0 - 1 - 2 - 3: rows 1 and 2 share the largest degree, the smaller one is kept; first keeps row 0."""
    out = cases.restate(4, cases.path_edges(4), keep=1)
    assert out["rep"].tolist() == [1, 1, 1, 1] and out["parent"].tolist() == [0, 0, 0, 0] and out["size"].tolist() == [4, 0, 0, 0]
    assert cases.restate(4, cases.path_edges(4), keep=0)["rep"].tolist() == [0, 0, 0, 0]


def _as_restated(result, n, id_offset):
    """A ``DuplicateClusters`` in the restatement's terms: (labels as rows, clusters' (label, rep, size) triples)."""
    labels = np.where(result.labels >= 0, result.labels - id_offset, -1)
    return labels, result.representatives - id_offset, result.sizes


def _check_result(result, want, n, id_offset):
    labels, reps, sizes = _as_restated(result, n, id_offset)
    roots = np.flatnonzero(want["size"] > 0)
    assert np.array_equal(labels, want["parent"])
    assert np.array_equal(reps, want["rep"][roots]) and np.array_equal(sizes, want["size"][roots])
    assert (result.n_clusters, result.n_rows) == tuple(want["counts"])
    assert result.labels.dtype == result.representatives.dtype == result.sizes.dtype == np.int64


def test_cluster_pairs_equals_the_restatement():
    from semantic_search_kd_amd import cluster_pairs

    rng = np.random.default_rng(11)
    names = {0: "all", 1: "across_groups", 2: "within_groups"}
    for trial in range(200):
        n, edges, take, groups = cases.random_graph(rng)
        id_offset = 0 if trial % 2 else 1000
        pairs = np.array(edges, dtype=np.int64).reshape(-1, 2) + id_offset
        if trial % 3 == 0 and len(edges):   # pairs in either orientation, and a few outside the rows: ignored
            pairs = np.concatenate([pairs[:, ::-1], [[id_offset - 1, id_offset], [id_offset, id_offset + n]]])
        for scope in (0, 1, 2):
            for keep, keep_name in ((0, "first"), (1, "densest")):
                got = cluster_pairs(pairs, n, keep=keep_name, scope=names[scope], groups=groups, allow=take, id_offset=id_offset)
                _check_result(got, cases.restate(n, edges, take, groups, scope, keep), n, id_offset)
    empty = cluster_pairs(np.zeros((0, 2), dtype=np.int64), 3)
    assert empty.labels.tolist() == [0, 1, 2] and empty.sizes.tolist() == [1, 1, 1] and empty.n_clusters == 3
    assert cluster_pairs([], 0).n_clusters == 0
    dup = cluster_pairs([[0, 1], [1, 2], [4, 5]], 6, keep="densest")
    assert dup.duplicates().tolist() == [0, 2, 5] and dup.representative_of_rows().tolist() == [1, 1, 1, 3, 4, 4]


def test_cluster_pairs_argument_errors():
    from semantic_search_kd_amd import cluster_pairs

    with pytest.raises(ValueError, match="keep="):
        cluster_pairs([], 3, keep="last")
    with pytest.raises(ValueError, match="scope="):
        cluster_pairs([], 3, scope="groups")
    with pytest.raises(ValueError, match="needs groups"):
        cluster_pairs([], 3, scope="across_groups")
    with pytest.raises(ValueError, match="groups for"):
        cluster_pairs([], 3, scope="within_groups", groups=[0, 1])
    with pytest.raises(ValueError, match="allow"):
        cluster_pairs([], 3, allow=[True])


def test_dedup_symbols_are_declared_and_exported(native_lib):
    from semantic_search_kd_amd import _build, _native
    from test_capi_symbols import _declared_symbols

    declared = _declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(native_lib, name), name
    assert _build.SOURCES.count("dedup.hip") == 1


def _fails(native_lib, rc, text):
    assert rc == 1                                     # SSKD_ERR_INVALID
    msg = native_lib.sskd_last_error()
    assert msg and text in msg, msg


def test_dup_init_argument_errors(native_lib):
    init = native_lib.sskd_dup_init
    _fails(native_lib, init(-1, None, A, B, None), b"dup_init: n_rows < 0")
    _fails(native_lib, init(2**31 - 64, None, A, B, None), b"dup_init: shard too large")
    _fails(native_lib, init(10, None, None, B, None), b"dup_init: null pointer")
    _fails(native_lib, init(10, A, B, None, None), b"dup_init: null pointer")
    assert init(0, None, None, None, None) == 0        # nothing to do, before any pointer is looked at


def test_dup_link_argument_errors(native_lib):
    link = native_lib.sskd_dup_link
    ok = dict(lims=A, ids=B, nq=4, cap=100, row0=0, off=0, n=10, groups=None, scope=0, parent=C, degree=D, flag=E)

    def call(**change):
        a = {**ok, **change}
        return link(a["lims"], a["ids"], a["nq"], a["cap"], a["row0"], a["off"], a["n"], a["groups"], a["scope"],
                    a["parent"], a["degree"], a["flag"], None)

    _fails(native_lib, call(nq=-1), b"dup_link: nq < 0")
    _fails(native_lib, call(cap=-1), b"dup_link: max_results < 0")
    _fails(native_lib, call(n=-1), b"dup_link: n_rows < 0")
    _fails(native_lib, call(n=2**31 - 64), b"dup_link: shard too large")
    _fails(native_lib, call(scope=3), b"dup_link: scope=3")
    _fails(native_lib, call(scope=-1), b"dup_link: scope=-1")
    _fails(native_lib, call(scope=1), b"dup_link: scope=1 needs the row groups")
    _fails(native_lib, call(scope=2), b"dup_link: scope=2 needs the row groups")
    _fails(native_lib, call(row0=-1), b"dup_link: query rows")
    _fails(native_lib, call(row0=7), b"dup_link: query rows")          # 7 + 4 queries > 10 rows
    for name in ("lims", "parent", "degree", "flag"):
        _fails(native_lib, call(**{name: None}), b"dup_link: null pointer")
    _fails(native_lib, call(ids=None), b"dup_link: null ids")
    assert call(nq=0, lims=None, ids=None, parent=None, degree=None, flag=None) == 0
    assert call(nq=0, n=0, lims=None, ids=None, parent=None, degree=None, flag=None) == 0


def test_dup_labels_argument_errors(native_lib):
    labels = native_lib.sskd_dup_labels
    _fails(native_lib, labels(-1, A, B, 0, C, D, E, None), b"dup_labels: n_rows < 0")
    _fails(native_lib, labels(2**31 - 64, A, B, 0, C, D, E, None), b"dup_labels: shard too large")
    _fails(native_lib, labels(10, A, B, 2, C, D, E, None), b"dup_labels: keep=2")
    _fails(native_lib, labels(10, A, B, -1, C, D, E, None), b"dup_labels: keep=-1")
    for args in [(None, B, 0, C, D, E), (A, None, 0, C, D, E), (A, B, 0, None, D, E), (A, B, 0, C, None, E),
                 (A, B, 0, C, D, None)]:
        _fails(native_lib, labels(10, *args, None), b"dup_labels: null pointer")
    _fails(native_lib, labels(0, None, None, 0, None, None, None, None), b"dup_labels: null pointer")   # the counts are written


def _builder():
    from semantic_search_kd_amd import FAISSIndexBuilder

    return FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")   # the constructor touches no device


def test_wrappers_refuse_unknown_rules_before_the_device():
    index = _builder()
    index._n = 100                                     # nothing stored: any device work would fail differently
    for call in (index.duplicate_clusters, index.deduplicate):
        with pytest.raises(ValueError, match="keep='best'"):
            call(0.9, keep="best")
        with pytest.raises(ValueError, match="scope='groups'"):
            call(0.9, scope="groups")
        with pytest.raises(ValueError, match="batch_size=0"):
            call(0.9, batch_size=0)
    index.shard_info = {"rank": 0, "world_size": 2, "n_total": 200}
    with pytest.raises(ValueError, match="row-sharded"):
        index.deduplicate(0.9, compact=True)


def test_cli_refuses_dedup_on_the_sharded_build(tmp_path, capsys):
    from semantic_search_kd_amd.build_index_cli import main

    (tmp_path / "model").mkdir()
    (tmp_path / "corpus.parquet").write_bytes(b"")
    base = ["--model-path", str(tmp_path / "model"), "--data-path", str(tmp_path / "corpus.parquet"), "--output-dir",
            str(tmp_path / "out")]
    with pytest.raises(SystemExit):
        main(base + ["--shards", "1", "--dedup-threshold", "0.95"])
    assert "--dedup-threshold: clusters span shards" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(base + ["--dedup-keep", "densest"])
    assert "need --dedup-threshold" in capsys.readouterr().err


def test_package_exports_the_host_form():
    import semantic_search_kd_amd as pkg

    for name in ("DuplicateClusters", "cluster_pairs"):
        assert name in pkg.__all__ and hasattr(pkg, name)
