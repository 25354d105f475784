"""Near-duplicate clusters on the MI355X.

Kernel tests: hand-built CSR edge lists go straight into ``sskd_dup_link`` (no search involved) and every output -
``parent``, ``degree``, ``rep``, ``size``, the counts - is compared with the plain-Python restatement of
``dedup_cases`` by integer equality: the design links the larger root under the smaller, so the result is a function of
the edge set and not of the order the hardware takes the edges in.

End-to-end tests: ``duplicate_clusters`` / ``deduplicate`` over a corpus of noisy copies and one chain cluster, held to the
restatement fed with ``near_duplicates(threshold)`` of the SAME index - the device's own score bits, through the existing
call."""
import json

import numpy as np
import pytest
import torch

import dedup_cases as cases

pytestmark = pytest.mark.gpu
KEYS = ("parent", "degree", "rep", "size", "counts")
SENTINEL = -77


def _stream(gpu):
    return int(torch.cuda.current_stream(gpu).cuda_stream)


def _dev(a, gpu, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(gpu)


def _mask_words(take, gpu):
    n = len(take)
    flags = np.ones(32 * max(-(-n // 32), 1), dtype=bool)   # the bits past n stay set, as the index keeps them
    flags[:n] = take
    return torch.from_numpy(np.packbits(flags, bitorder="little").view("<u4").view(np.int32).copy()).to(gpu)


class Forest:
    """The device state of one clustering, with a guard word behind every array."""

    def __init__(self, lib, gpu, n, take=None):
        self.lib, self.gpu, self.n = lib, gpu, n
        self.buf = torch.full((4, n + 1), SENTINEL, dtype=torch.int32, device=gpu)
        self.parent, self.degree, self.rep, self.size = (self.buf[k] for k in range(4))
        self.counts = torch.full((3,), SENTINEL, dtype=torch.int32, device=gpu)
        self.flag = torch.zeros(2, dtype=torch.int32, device=gpu)
        self.flag[1] = SENTINEL
        mask = None if take is None else _mask_words(take, gpu)
        assert lib.sskd_dup_init(n, None if mask is None else mask.data_ptr(), self.parent.data_ptr(),
                                 self.degree.data_ptr(), _stream(gpu)) == 0

    def link(self, lims, ids, row0=0, id_offset=0, groups=None, scope=0, max_results=None):
        lims_d, ids_d = _dev(lims, self.gpu, np.int64), _dev(np.concatenate([ids, [0]]), self.gpu, np.int64)
        cap = len(ids) if max_results is None else max_results
        rc = self.lib.sskd_dup_link(lims_d.data_ptr(), ids_d.data_ptr(), len(lims) - 1, cap, row0, id_offset, self.n,
                                    None if groups is None else groups.data_ptr(), scope, self.parent.data_ptr(),
                                    self.degree.data_ptr(), self.flag.data_ptr(), _stream(self.gpu))
        assert rc == 0, self.lib.sskd_last_error()

    def labels(self, keep):
        assert self.lib.sskd_dup_labels(self.n, self.parent.data_ptr(), self.degree.data_ptr(), keep, self.rep.data_ptr(),
                                        self.size.data_ptr(), self.counts.data_ptr(), _stream(self.gpu)) == 0
        buf, counts = self.buf.cpu().numpy().astype(np.int64), self.counts.cpu().numpy().astype(np.int64)
        assert (buf[:, self.n] == SENTINEL).all() and counts[2] == SENTINEL      # nothing behind the outputs
        assert self.flag.cpu().tolist() == [0, SENTINEL]                          # no call overflowed
        n = self.n
        return {"parent": buf[0, :n], "degree": buf[1, :n], "rep": buf[2, :n], "size": buf[3, :n], "counts": counts[:2]}


def _same(got, want, what=""):
    for key in KEYS:
        bad = np.flatnonzero(got[key] != want[key])
        assert bad.size == 0, (what, key, bad[:5], got[key][bad[:5]], want[key][bad[:5]])


def _cluster(lib, gpu, n, calls, keep, take=None, groups=None, scope=0, id_offset=0):
    """Runs the link calls ``(row0, lims, ids)`` and the labels; returns the outputs and the edges the rows admit."""
    forest = Forest(lib, gpu, n, take)
    groups_d = None if groups is None else _dev(groups, gpu, np.int32)
    edges = []
    for row0, lims, ids in calls:
        forest.link(lims, ids, row0, id_offset, groups_d, scope)
        edges += cases.edges_of_csr(lims, ids, row0, id_offset, n)
    return forest.labels(keep), edges


# --------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_path_of_4097_rows_in_one_batch(gpu, native_lib, order):
    """Deep find chains, linked under the smaller root from both ends.  The kernel takes the rows of a batch in launch
    order, so the order is varied in what it can be: ascending = row k lists k + 1; descending = every row lists
    itself and both neighbours, largest first (the entries ``j <= i`` are ignored); shuffled = the path's vertices are
    renumbered by a fixed permutation, so consecutive rows are far apart on the path."""
    n = 4097
    edges = cases.path_edges(n)
    if order == "shuffled":
        edges = cases.relabel(edges, np.random.default_rng(5).permutation(n))
    lims, ids = cases.symmetric_csr(n, edges, descending=True) if order == "descending" else cases.upper_csr(n, edges)
    for keep in (0, 1):
        got, listed = _cluster(native_lib, gpu, n, [(0, lims, ids)], keep)
        assert sorted(listed) == sorted(edges)
        _same(got, cases.restate(n, edges, keep=keep), (order, keep))
    assert got["counts"].tolist() == [1, n] and got["size"][0] == n and (got["parent"] == 0).all()


@pytest.mark.parametrize("hub", [0, 5000, 10000])
def test_a_star_of_10000_leaves(gpu, native_lib, hub):
    """Every edge contends on one root: the hub's own row lists the leaves above it, the leaves below it list the hub."""
    n = 10001
    edges = cases.star_edges(hub, n)
    lims, ids = cases.upper_csr(n, edges)
    got, _ = _cluster(native_lib, gpu, n, [(0, lims, ids)], 1)
    _same(got, cases.restate(n, edges, keep=1), hub)
    assert (got["rep"] == hub).all() and got["degree"][hub] == n - 1 and got["size"][0] == n


def test_two_cliques_joined_by_a_later_call(gpu, native_lib):
    n = 128
    cliques = cases.clique_edges(range(0, 128, 2)) + cases.clique_edges(range(1, 128, 2))   # 64 even rows, 64 odd rows
    lims, ids = cases.symmetric_csr(n, cliques)
    separate, _ = _cluster(native_lib, gpu, n, [(0, lims, ids)], 0)
    _same(separate, cases.restate(n, cliques), "cliques")
    assert separate["counts"].tolist() == [2, n] and separate["size"][:2].tolist() == [64, 64]
    bridge = cases.csr_of([37], [[90]])
    for keep in (0, 1):
        joined, edges = _cluster(native_lib, gpu, n, [(0, lims, ids), (37, *bridge)], keep)
        _same(joined, cases.restate(n, edges, keep=keep), ("joined", keep))
        assert joined["counts"].tolist() == [1, n]
    assert joined["rep"][0] == 37            # 64 edges at rows 37 and 90, 63 elsewhere: the smaller of the two


def test_a_sparse_graph_in_uneven_batches_twice(gpu, native_lib):
    """20 000 rows, ~60 000 edges as a self-join lists them (every row lists itself and all its neighbours), cut at uneven
    boundaries; the larger batches launch more workgroups than the device has compute units."""
    n = 20000
    edges = cases.sparse_graph(n)
    cuts = [0, 1, 33, 1000, 4097, 9000, 9001, 15555, n]
    calls = [(lo, *cases.symmetric_csr(n, edges, lo, hi)) for lo, hi in zip(cuts, cuts[1:])]
    want = cases.restate(n, edges, keep=1)
    first, listed = _cluster(native_lib, gpu, n, calls, 1)
    assert len(listed) == len(edges)
    second, _ = _cluster(native_lib, gpu, n, calls[::-1], 1)        # the batches in the opposite order
    _same(first, want, "first")
    _same(second, first, "second")
    assert 1 < want["counts"][0] < n


def test_entries_that_are_not_edges(gpu, native_lib):
    """``j <= i``, ids outside the rows under a non-zero ``id_offset``, an endpoint cleared in the mask, and both scopes."""
    n, id_offset = 70, 1000
    rng = np.random.default_rng(3)
    take = rng.random(n) > 0.25
    groups = rng.integers(0, 4, size=n)
    # every row lists 12 ids drawn from [id_offset - 20, id_offset + n + 20): below the rows, j <= i, j > i, past the rows
    lists = [sorted(rng.integers(id_offset - 20, id_offset + n + 20, size=12).tolist()) for _ in range(n)]
    lists[5] += [id_offset + 5, 5, 2**40, -3]                       # itself, and ids far outside in both directions
    lims, ids = cases.csr_of(range(n), lists)
    edges = cases.edges_of_csr(lims, ids, 0, id_offset, n)
    assert 0 < len(edges) < len(ids) / 2
    for scope in (0, 1, 2):
        for mask in (None, take):
            got, _ = _cluster(native_lib, gpu, n, [(0, lims, ids)], 1, mask, groups, scope, id_offset)
            want = cases.restate(n, edges, mask, groups, scope, 1)
            _same(got, want, (scope, mask is None))
            if mask is not None:
                assert (got["parent"][~take] == -1).all() and (got["rep"][~take] == -1).all()
                assert (got["degree"][~take] == 0).all() and got["counts"][1] == take.sum()
    # the split of the batch must not matter either: two calls with a query_row0
    halves = [(0, *cases.csr_of(range(31), lists[:31])), (31, *cases.csr_of(range(31, n), lists[31:]))]
    got, _ = _cluster(native_lib, gpu, n, halves, 1, take, groups, 2, id_offset)
    _same(got, cases.restate(n, edges, take, groups, 2, 1), "halves")


def test_overflow_links_nothing_and_sets_the_flag(gpu, native_lib):
    n = 200
    edges = cases.path_edges(60) + cases.star_edges(100, n)[70:150]
    lims, ids = cases.upper_csr(n, edges)
    forest = Forest(native_lib, gpu, n)
    forest.link(*cases.upper_csr(n, cases.path_edges(40)))           # some state to keep
    before = forest.buf.clone()
    for cap in (len(ids) - 1, 0):
        forest.link(lims, ids, max_results=cap)                       # lims[nq] = len(ids) > cap
        assert forest.flag.cpu().tolist() == [1, SENTINEL]
        assert torch.equal(forest.buf, before)                        # parent and degree bit-identical
        forest.flag[0] = 0
    forest.flag[0] = 5
    forest.link(lims, ids, max_results=len(ids))                      # fits exactly: the flag is left alone
    assert forest.flag.cpu().tolist() == [5, SENTINEL]
    forest.flag[0] = 0
    _same(forest.labels(0), cases.restate(n, cases.path_edges(40) + edges), "after")


def test_empty_calls_are_no_ops(gpu, native_lib):
    forest = Forest(native_lib, gpu, 10)
    forest.link(*cases.upper_csr(10, [(1, 2), (2, 9)]))
    before = forest.buf.clone()
    forest.link(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), row0=4)          # nq = 0
    forest.link(np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int64), row0=7)          # three rows without entries
    assert torch.equal(forest.buf, before)
    _same(forest.labels(0), cases.restate(10, [(1, 2), (2, 9)]), "ten")
    empty = Forest(native_lib, gpu, 0)                                # n_rows = 0: nothing is written but the counts
    empty.link(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64))
    out = empty.labels(1)
    assert out["counts"].tolist() == [0, 0] and out["parent"].size == 0


def test_densest_ties_go_to_the_smaller_row(gpu, native_lib):
    """Component A = the path 3 - 7 - 5 - 9 (rows 5 and 7 share degree 2: 5 is kept, 3 is the label); component B = a star
    around row 20 with leaves 11 .. 14 plus the edge 11 - 12 (20 alone has the largest degree); row 0 is alone."""
    n = 24
    edges = [(3, 7), (5, 7), (5, 9), (11, 20), (12, 20), (13, 20), (14, 20), (11, 12)]
    got, _ = _cluster(native_lib, gpu, n, [(0, *cases.upper_csr(n, edges))], 1)
    _same(got, cases.restate(n, edges, keep=1), "ties")
    assert got["rep"][[3, 5, 7, 9]].tolist() == [5] * 4 and got["parent"][[3, 5, 7, 9]].tolist() == [3] * 4
    assert got["rep"][[11, 12, 13, 14, 20]].tolist() == [20] * 5 and got["rep"][0] == 0
    first, _ = _cluster(native_lib, gpu, n, [(0, *cases.upper_csr(n, edges))], 0)
    assert np.array_equal(first["rep"], first["parent"])


# ------------------------------------------------------------------------------------------------------ end to end
THRESHOLD = cases.E2E_THRESHOLD
OFFSETS = [0, 5000]


def _build(gpu, id_offset, removed=True):
    from semantic_search_kd_amd import FAISSIndexBuilder

    rows, family = cases.e2e_corpus()
    index = FAISSIndexBuilder(embedding_dim=384, metric="ip", device=str(gpu), id_offset=id_offset)
    index.build_from_embeddings(rows)
    if removed:
        index.remove_ids(id_offset + np.array([0, 17, 640, 1999, rows.shape[0] - 1]))
    return index, family


@pytest.fixture(scope="module")
def corpus(gpu):
    """id_offset -> (index with a few removed rows, family per row, near_duplicates' pairs as LOCAL rows, live per row)."""
    out = {}
    for id_offset in OFFSETS:
        index, family = _build(gpu, id_offset)
        pairs, _ = index.near_duplicates(THRESHOLD)
        live = np.ones(index.ntotal, dtype=bool)
        live[index.removed_rows()] = False
        out[id_offset] = (index, family, pairs - id_offset, live)
    assert np.array_equal(out[0][2], out[5000][2])
    return out


def _check(result, want, id_offset):
    roots = np.flatnonzero(want["size"] > 0)
    assert np.array_equal(result.labels, np.where(want["parent"] >= 0, want["parent"] + id_offset, -1))
    assert np.array_equal(result.representatives, want["rep"][roots] + id_offset)
    assert np.array_equal(result.sizes, want["size"][roots])
    assert (result.n_clusters, result.n_rows) == tuple(want["counts"])
    assert result.labels.dtype == result.representatives.dtype == result.sizes.dtype == np.int64


def test_the_corpus_is_what_the_tests_assume(corpus):
    index, family, pairs, live = corpus[0]
    n = index.ntotal
    assert 2048 <= n <= 4096 and pairs.shape[0] > n
    assert (family[pairs[:, 0]] == family[pairs[:, 1]]).all()          # no pair across families: well separated
    chain = np.flatnonzero(family == family.max())
    assert chain.size == 16
    in_chain = np.isin(pairs[:, 0], chain)
    assert in_chain.sum() < 16 * 15 // 2 - 20                          # the chain is no clique: its ends do not pair


@pytest.mark.parametrize("id_offset", OFFSETS)
@pytest.mark.parametrize("batch_size", [96, 257, 4096])
def test_duplicate_clusters_equals_near_duplicates_plus_union_find(corpus, id_offset, batch_size):
    """96: every batch starts on a tile boundary (the triangle path); 257: only every 32nd does (the full scan, and a mix);
    4096: the default, one batch."""
    index, family, pairs, live = corpus[id_offset]
    n = index.ntotal
    for keep, name in ((0, "first"), (1, "densest")):
        got = index.duplicate_clusters(THRESHOLD, keep=name, batch_size=batch_size)
        _check(got, cases.restate(n, pairs, live, keep=keep), id_offset)
    # the chain comes out as one cluster (its live rows), every family as one cluster
    chain = np.flatnonzero((family == family.max()) & live)
    assert np.unique(got.labels[chain]).size == 1 and got.labels[chain[0]] == chain.min() + id_offset
    assert got.n_clusters == np.unique(family[live]).size and got.n_rows == live.sum()
    assert (got.labels[~live] == -1).all()


@pytest.mark.parametrize("capacity", [1, 150, 400])
def test_a_tiny_capacity_takes_the_overflow_and_redo_path(corpus, capacity):
    """Batches of 96 rows list at least 96 entries (every row finds itself): capacity 1 overflows every batch, 150 and 400
    some of them.  An overflowed batch added nothing, so the degrees - and the densest rows - are those of one pass."""
    index, family, pairs, live = corpus[5000]
    index.dedup_capacity = capacity
    try:
        got = index.duplicate_clusters(THRESHOLD, keep="densest", batch_size=96)
    finally:
        index.dedup_capacity = 1 << 20
    _check(got, cases.restate(index.ntotal, pairs, live, keep=1), 5000)


def test_scopes_over_the_families(corpus):
    index, family, pairs, live = corpus[0]
    n = index.ntotal
    index.set_groups([int(f) for f in family])
    try:
        across = index.duplicate_clusters(THRESHOLD, scope="across_groups", batch_size=96)
        within = index.duplicate_clusters(THRESHOLD, scope="within_groups", keep="densest", batch_size=257)
    finally:
        index._reset_groups()
    _check(across, cases.restate(n, pairs, live, family, 1, 0), 0)
    assert across.n_clusters == across.n_rows == live.sum() and (across.sizes == 1).all()       # all singletons
    _check(within, cases.restate(n, pairs, live, keep=1), 0)                                      # the unscoped clusters


def test_allow_restricts_the_rows_taking_part(corpus):
    index, family, pairs, live = corpus[5000]
    n = index.ntotal
    allow = np.arange(n) % 2 == 0
    got = index.duplicate_clusters(THRESHOLD, keep="densest", allow=allow, batch_size=257)
    _check(got, cases.restate(n, pairs, live & allow, keep=1), 5000)       # the components of the induced graph
    assert (got.labels[~allow] == -1).all() and got.n_rows == (live & allow).sum()
    ids = 5000 + np.flatnonzero(allow)
    again = index.duplicate_clusters(THRESHOLD, keep="densest", allow=ids)   # the same filter as an id array
    assert np.array_equal(again.labels, got.labels) and np.array_equal(again.representatives, got.representatives)


@pytest.mark.parametrize("keep", ["first", "densest"])
def test_deduplicate_leaves_no_pair(gpu, keep):
    index, family = _build(gpu, 5000)
    gone_before = index.n_removed
    out = index.deduplicate(THRESHOLD, keep=keep, batch_size=1000)
    assert out.removed.size == out.n_rows - out.n_clusters and index.n_removed == gone_before + out.removed.size
    assert index.ntotal - index.n_removed == out.n_clusters
    assert not np.isin(out.representatives, out.removed).any() and out.kept is None
    pairs, scores = index.near_duplicates(THRESHOLD)
    assert pairs.shape == (0, 2) and scores.size == 0
    assert index.duplicate_clusters(THRESHOLD).n_clusters == out.n_clusters        # and all of them singletons now


def test_deduplicate_and_compact(gpu):
    index, family = _build(gpu, 5000)
    n = index.ntotal
    queries = cases.e2e_corpus(seed=99, n_originals=8, chain=2)[0][:16]
    plan = index.duplicate_clusters(THRESHOLD, keep="densest")                      # changes nothing: the survivors to be
    s_before, i_before = index.search(queries, k=10, allow=plan.representatives)
    doc_ids = list(index.doc_ids)
    out = index.deduplicate(THRESHOLD, keep="densest", compact=True)
    assert np.array_equal(out.representatives, plan.representatives) and np.array_equal(out.labels, plan.labels)
    assert index.ntotal == out.n_clusters and index.n_removed == 0
    assert np.array_equal(out.kept, np.sort(out.representatives))                   # kept: old ids of the new rows
    assert index.doc_ids == [doc_ids[i - 5000] for i in out.kept]
    s_after, i_after = index.search(queries, k=10)
    assert np.array_equal(s_after, s_before)                                        # the survivors' scores, bit for bit
    assert np.array_equal(out.kept[i_after - 5000], i_before)
    assert index.near_duplicates(THRESHOLD)[0].shape[0] == 0


def test_build_index_cli_dedup_threshold(gpu, tmp_path, capsys):
    import pandas as pd

    from semantic_search_kd_amd import BertConfig, FAISSIndexBuilder, StudentModel, synthetic_state_dict
    from semantic_search_kd_amd.build_index_cli import main as build_index_main
    from semantic_search_kd_amd.weights import save_model_dir
    from test_encoder_gpu import _vocab

    vocab = _vocab()
    cfg = BertConfig(vocab_size=len(vocab), num_hidden_layers=2)
    mdir = tmp_path / "model"
    save_model_dir(mdir, cfg, synthetic_state_dict(cfg))
    (mdir / "vocab.txt").write_text("\n".join(vocab))
    base = ["machine learning is a search of the vector index", "deep neural networks work", "hello world test document",
            "what is semantic search?", "the index of a document text", "how does a neural network work?"]
    texts = base + [base[1], base[4], base[1], "a text of its own", base[0]]
    corpus = tmp_path / "corpus.parquet"
    pd.DataFrame({"chunk_id": [f"chunk_{i}" for i in range(len(texts))], "text": texts}).to_parquet(corpus)
    threshold = 0.9995

    # the expectation, from the existing calls on the same rows
    ref = FAISSIndexBuilder(embedding_dim=384, metric="cosine", device="cuda:0")
    ref.build_from_parquet(model=StudentModel(str(mdir), device="cuda:0"), parquet_path=corpus, batch_size=4)
    pairs, _ = ref.near_duplicates(threshold)
    want = cases.restate(len(texts), pairs)
    n_clusters = int(want["counts"][0])
    assert n_clusters <= len(base) + 1                      # the repeated texts at least are found

    out = tmp_path / "index"
    capsys.readouterr()
    rc = build_index_main(["--model-path", str(mdir), "--data-path", str(corpus), "--output-dir", str(out), "--batch-size", "4",
                           "--device", "cuda:0", "--dedup-threshold", str(threshold), "--dedup-keep", "first"])
    assert rc == 0
    printed = capsys.readouterr().out
    assert f"De-duplication at {threshold}: {len(texts)} rows, {n_clusters} clusters, {len(texts) - n_clusters} rows dropped" in printed
    assert f"Total vectors: {n_clusters}" in printed
    survivors = np.flatnonzero(want["size"] > 0)
    assert json.loads((out / "doc_ids.json").read_text()) == [f"chunk_{i}" for i in survivors]
    loaded = FAISSIndexBuilder(embedding_dim=384, metric="cosine", device="cuda:0")
    loaded.load(out)
    assert loaded.ntotal == n_clusters and loaded.n_removed == 0
    assert np.array_equal(loaded.to_numpy(), ref.to_numpy()[survivors])
