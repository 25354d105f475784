"""Graph index on the GPU, incremental insertion: every step of ``GraphIndex.insert`` against its plain-Python
restatement (``graph_insert_cases``) by exact integer equality, the shapes where it can go wrong, the three exports
straight through the C-ABI on hand-made tables, the search over an inserted graph against ``beam_search_batch_ref``,
and the reference's recall gate (``recall_threshold: 0.97``) on graphs that grew by insertion."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import graph_cases as gc
import graph_insert_cases as gic
from oracle import search as oracle
from semantic_search_kd_amd import FAISSIndexBuilder, GraphIndex, _native, graph as graph_mod, ivf as ivf_mod

pytestmark = pytest.mark.gpu

N, N0, DIM, NQ = 3001, 2500, 384, 65   # 2 500 is no multiple of the 32-row tile: the flat add re-packs a partial tile


def _flat(corpus, gpu):
    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu))
    index.build_from_embeddings(corpus)
    return index


def _built(corpus, gpu, M, K0=None, **args):
    index = GraphIndex(flat=_flat(corpus, gpu), M=M, **args)
    index.build_graph(knn_k=K0)
    return index


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got, ref, what):
    assert np.array_equal(got[1], ref[1]), f"{what}: ids differ"
    assert np.array_equal(_bits(got[0]), _bits(ref[0])), f"{what}: scores differ"


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _graph_is_sound(g, n):
    for u, row in enumerate(g):
        real = row[row >= 0]
        assert u not in real and np.unique(real).size == real.size and (row[real.size:] == -1).all() and (real < n).all()


@pytest.fixture(scope="module")
def world(gpu):
    corpus = oracle.seeded_unit_rows(N, DIM, 1)
    queries = oracle.seeded_unit_rows(NQ, DIM, 2)
    return SimpleNamespace(corpus=corpus, queries=queries, scores=oracle.scores_fma(queries, corpus))


# ----------------------------------------------------------------------------- each step against its restatement
@pytest.mark.parametrize("M, K0", [(4, 8), (16, 32), (32, 64), (64, 128)])
def test_insert_steps_against_the_restatements(world, gpu, M, K0):
    index = _built(world.corpus[:N0], gpu, M, K0)
    old, old_entry = index.graph_numpy(), index.entry_rows_numpy()
    ref = gic.insert_ref(world.corpus, old, old_entry, K0)
    assert ref.touched.size and (ref.knn_new >= N0).any() and (ref.knn_new < N0).any()
    # step by step
    index.flat.add(world.corpus[N0:])
    with torch.cuda.device(index.device):
        knn = index.knn_device(K0, first=N0)
        fwd = index.insert_prune_device(index.graph, knn)
        incoming_new, touched, incoming_old = index.incoming_device(fwd, N0)
        full = torch.full((N + 1, M), 77, dtype=torch.int32, device=gpu)           # a guard row at the end
        full[:N0].copy_(index.graph)
        index.merge_rows_device(fwd, incoming_new, N0, full[N0:N])
        torch.cuda.synchronize()
        merged = full.cpu().numpy()
        index.link_device(full[:N], N0, touched, incoming_old)
        torch.cuda.synchronize()
    assert knn.dtype == torch.int32 and np.array_equal(knn.cpu().numpy(), ref.knn_new), "knn_new"
    assert np.array_equal(fwd.cpu().numpy(), ref.fwd_new), "sskd_graph_insert_prune"
    assert np.array_equal(incoming_new.cpu().numpy(), ref.incoming_new), "incoming, new targets"
    assert np.array_equal(touched.cpu().numpy(), ref.touched) and touched.dtype == torch.int32, "touched"
    assert np.array_equal(incoming_old.cpu().numpy(), ref.incoming_old), "incoming, old targets"
    assert np.array_equal(merged[N0:N], ref.new_rows) and np.array_equal(merged[:N0], old), "sskd_graph_merge_rows"
    linked = full.cpu().numpy()
    assert (linked[N] == 77).all() and (merged[N] == 77).all()
    assert np.array_equal(linked[:N], ref.graph), "sskd_graph_link"
    untouched = np.setdiff1d(np.arange(N0), ref.touched)
    assert untouched.size and np.array_equal(linked[untouched], old[untouched])     # bit-identical to before
    assert np.array_equal(linked[N0:N], ref.new_rows)
    # the whole call, twice from the same state
    first = None
    for _ in range(2):
        again = _built(world.corpus[:N0], gpu, M, K0)
        again.insert(world.corpus[N0:])
        got = (again.graph_numpy(), again.entry_rows_numpy())
        assert again.ntotal == N and again.n_inserted == N - N0 and again.n_entry == ref.entry_rows.size
        assert np.array_equal(got[0], ref.graph) and np.array_equal(got[1], ref.entry_rows)
        assert np.array_equal(_bits(again.entry.to_numpy()), _bits(world.corpus[ref.entry_rows]))
        first = first or got
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    _graph_is_sound(ref.graph, N)


# ------------------------------------------------------------------------------------ shapes where it can go wrong
@pytest.mark.parametrize("n0, b, M, K0", [(300, 1, 16, 32), (50, 2000, 4, 8), (10, 5, 16, 16)])
def test_insert_shapes(gpu, n0, b, M, K0):
    """One row; more new rows than linked ones; fewer rows than a list is long (lists and adjacency padded with -1)."""
    corpus = oracle.seeded_unit_rows(n0 + b, DIM, 80 + b)
    index = _built(corpus[:n0], gpu, M, K0)
    old = index.graph_numpy()
    ref = gic.insert_ref(corpus, old, index.entry_rows_numpy(), K0)
    if n0 + b <= K0:
        assert (ref.knn_new[:, n0 + b - 1:] == -1).all() and (ref.knn_new[:, :n0 + b - 1] >= 0).all()
        assert (old == -1).any()                                   # an old row with room: nothing is evicted from it
    index.insert(corpus[n0:])
    assert np.array_equal(index.graph_numpy(), ref.graph) and np.array_equal(index.entry_rows_numpy(), ref.entry_rows)
    _graph_is_sound(ref.graph, n0 + b)


def test_second_insert_on_top_of_the_first(world, gpu):
    """The neighbours of the second batch have their lists in BOTH tables: adjacency rows written by the build, by the
    first insert's merge and by its link step, and k-NN lists of the batch itself."""
    M, K0, a, c = 16, 32, 2000, 2500
    index = _built(world.corpus[:a], gpu, M, K0)
    r1 = gic.insert_ref(world.corpus[:c], index.graph_numpy(), index.entry_rows_numpy(), K0)
    r2 = gic.insert_ref(world.corpus, r1.graph, r1.entry_rows, K0)
    assert ((r2.knn_new >= a) & (r2.knn_new < c)).any() and (r2.knn_new < a).any() and (r2.knn_new >= c).any()
    assert (r2.touched >= a).any() and (r2.touched < a).any()      # rows of the first insert are relinked too
    index.insert(world.corpus[a:c])
    assert np.array_equal(index.graph_numpy(), r1.graph)
    index.insert(world.corpus[c:])
    assert np.array_equal(index.graph_numpy(), r2.graph) and np.array_equal(index.entry_rows_numpy(), r2.entry_rows)
    assert index.n_inserted == N - a


def test_identical_rows_ties_and_the_cap(gpu):
    """40 copies of one vector behind 150 rows that already hold 6 copies, K0 = 8: a new row is not among its own 9
    results, more than M / 2 new rows name one old row (kept by (position, source)), and the link step cuts through
    rows of equal score (kept by id)."""
    M, K0, n0, b = 8, 8, 150, 40
    corpus = oracle.seeded_unit_rows(n0 + b, DIM, 91)
    copies = [3, 40, 41, 77, 120, 149]
    corpus[copies] = corpus[3]
    corpus[n0:] = corpus[3]
    index = _built(corpus[:n0], gpu, M, K0)
    old = index.graph_numpy()
    ref = gic.insert_ref(corpus, old, index.entry_rows_numpy(), K0)
    own = oracle.topk_of_scores(oracle.scores_fma(corpus[n0:], corpus), K0 + 1)[1]
    assert (own != (n0 + np.arange(b))[:, None]).all(axis=1).any()             # absent from its own results
    heads = ref.fwd_new[:, :M // 2]
    named = np.bincount(heads[(heads >= 0) & (heads < n0)], minlength=n0)
    assert named.max() > M // 2                                                 # the cap has work to do
    tie_across_the_cut = False
    for t, u in enumerate(ref.touched):
        adj = [int(v) for v in old[u] if v >= 0]
        pool = adj[M // 2:] + [int(v) for v in ref.incoming_old[t] if v >= 0 and v not in adj]
        out = [int(v) for v in ref.graph[u] if v >= 0 and v not in adj[:M // 2]]
        s = oracle.scores_fma(corpus[u:u + 1], corpus)[0]
        tie_across_the_cut |= any(v not in out and s[v] == s[out[-1]] for v in pool)
    assert tie_across_the_cut
    index.insert(corpus[n0:])
    assert np.array_equal(index.graph_numpy(), ref.graph) and np.array_equal(index.entry_rows_numpy(), ref.entry_rows)


# -------------------------------------------------------------------------- the C-ABI on hand-made tables
def _wild(rng, shape, n):
    """Random ids in [0, n) with -1, out-of-range and negative entries mixed in."""
    a = rng.integers(0, n, size=shape).astype(np.int32)
    a[rng.random(shape) < 0.10] = -1
    wild = rng.random(shape) < 0.04
    a[wild] = rng.choice(np.array([n, n + 7, 2 ** 31 - 1, -5], dtype=np.int64), size=int(wild.sum())).astype(np.int32)
    return a


@pytest.mark.parametrize("M, K0", [(4, 4), (8, 24), (64, 128)])
def test_insert_prune_on_hand_made_tables(gpu, native_lib, M, K0):
    n0, b = 45, 38
    rng = np.random.default_rng(100 + M)
    graph_old, knn_new = _wild(rng, (n0, M), n0 + b), _wild(rng, (b, K0), n0 + b)
    knn_new[::3, 1] = (n0 + np.arange(b))[::3]                    # self edges
    knn_new[:, K0 - 1] = knn_new[:, 0]                            # repeats
    graph_old[:, M - 1] = graph_old[:, 1]
    out = torch.full((b + 1, M), 77, dtype=torch.int32, device=gpu)
    d_old, d_knn = _dev(graph_old, gpu), _dev(knn_new, gpu)
    _native.check(native_lib.sskd_graph_insert_prune(d_old.data_ptr(), n0, d_knn.data_ptr(), b, K0, M, out.data_ptr(),
                                                     _native.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[b] == 77).all()
    assert np.array_equal(out[:b], gic.insert_prune_ref(graph_old, knn_new, M))
    # nothing linked: the build's prune, bit for bit
    fwd = torch.empty((b, M), dtype=torch.int32, device=gpu)
    _native.check(native_lib.sskd_graph_insert_prune(None, 0, d_knn.data_ptr(), b, K0, M, fwd.data_ptr(),
                                                     _native.current_stream_ptr(gpu)))
    build = torch.empty((b, M), dtype=torch.int32, device=gpu)
    _native.check(native_lib.sskd_graph_prune(d_knn.data_ptr(), b, K0, M, build.data_ptr(), _native.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    assert np.array_equal(fwd.cpu().numpy(), build.cpu().numpy())
    assert np.array_equal(build.cpu().numpy(), gc.detours_ref(knn_new, M)[1])


def test_merge_rows_on_hand_made_tables(gpu, native_lib):
    n, M, base, total = 37, 8, 50, 90
    rng = np.random.default_rng(61)
    fwd, incoming = _wild(rng, (n, M), total + 2), _wild(rng, (n, M // 2), total + 2)
    fwd[:, 5] = fwd[:, 0]
    incoming[:, 1] = fwd[:, 2]
    fwd[::3, 1] = (base + np.arange(n))[::3]
    incoming[::4, 0] = np.arange(n)[::4]                          # the LOCAL row number is an ordinary id here
    out = torch.full((n + 1, M), 77, dtype=torch.int32, device=gpu)
    d_fwd, d_incoming = _dev(fwd, gpu), _dev(incoming, gpu)
    _native.check(native_lib.sskd_graph_merge_rows(d_fwd.data_ptr(), d_incoming.data_ptr(), n, base, total, M, out.data_ptr(),
                                                   _native.current_stream_ptr(gpu)))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[n] == 77).all()
    ref = gic.merge_rows_ref(fwd, incoming, base, total)
    assert np.array_equal(out[:n], ref)
    assert (ref >= n).any() and not np.array_equal(ref, gc.merge_ref(fwd, incoming))   # the old export could not serve this


@pytest.mark.parametrize("M", [4, 8, 32, 64])
def test_link_on_hand_made_tables(gpu, native_lib, M):
    """-1, out-of-range ids, self edges and repeats in graph and incoming; touched with an entry outside [0, n_old), a
    repeated entry and a step down; a row with room; more tied rows than places; a row holding NaN in the pool."""
    n0, b = 70, 50
    n1, h = n0 + b, M // 2
    rng = np.random.default_rng(200 + M)
    rows = oracle.seeded_unit_rows(n1, DIM, 95)
    rows[n0:n0 + 12] = rows[5]                                    # twelve rows of equal score to anyone
    rows[n0 + 20, 7] = np.nan
    flat = _flat(rows, gpu)
    graph = np.concatenate([gc.random_adjacency(n0, M, 300 + M), gc.random_adjacency(b, M, 301 + M)])
    graph[4] = -1
    graph[4, :2] = [9, 11]                                        # room
    graph[6, :h] = 20 + np.arange(h)                              # a full head,
    graph[6, h:] = (n0 + np.arange(M - h)) % n1                   # and in its pool tied rows already; more arrive
    graph[8, M - 1] = n0 + 20                                     # NaN already in the pool
    touched = np.array([2, 4, 6, 6, 8, n0 + 3, 10, 9, 12, -4, 2 ** 31 - 1, 30, 31], dtype=np.int32)
    incoming = _wild(rng, (touched.size, h), n1)
    inside = (incoming >= 0) & (incoming < n1)
    incoming[inside] = n0 + incoming[inside] % b
    incoming[0, 0] = 2                                            # a self edge
    incoming[1] = n0 + 20                                         # NaN, h times over
    incoming[2] = (n0 + 11 - np.arange(h)) % n1                   # tied rows in descending id order
    incoming[4, -1] = incoming[4, 0]
    incoming[12, 0] = n0 + 20
    full = torch.full((n1 + 1, M), 77, dtype=torch.int32, device=gpu)
    full[:n1].copy_(_dev(graph, gpu))
    d_touched, d_incoming = _dev(touched, gpu), _dev(incoming, gpu)
    for _ in range(2):                                            # linking what is linked changes nothing more
        _native.check(native_lib.sskd_graph_link(flat._tiled.data_ptr(), full.data_ptr(), n0, n1, M, d_touched.data_ptr(),
                                                 d_incoming.data_ptr(), touched.size, _native.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        out = full.cpu().numpy()
        assert (out[n1] == 77).all()
        ref = gic.link_ref(rows, graph, n0, touched, incoming)
        assert np.array_equal(out[:n1], ref)
        graph = ref
    # 10 and 30 follow a larger entry, 9 follows 10, n0 + 3 is no linked row: only these six rows may have changed
    rest = np.array(sorted(set(range(n1)) - {2, 4, 6, 8, 12, 31}))
    first = np.concatenate([gc.random_adjacency(n0, M, 300 + M), gc.random_adjacency(b, M, 301 + M)])
    assert np.array_equal(out[rest], first[rest])
    assert out[6, :h].tolist() == (20 + np.arange(h)).tolist()
    assert out[4].tolist() == [9, 11, n0 + 20] + [-1] * (M - 3)    # room: nothing evicted, the NaN row once
    tail = out[6, h:]
    assert (tail >= 0).all() and (np.diff(tail[np.isin(tail, n0 + np.arange(12))]) > 0).all()   # ties by ascending id


# ------------------------------------------------------------------------------------- searching after an insert
@pytest.fixture(scope="module")
def inserted(world, gpu):
    index = _built(world.corpus[:N0], gpu, 16)
    index.insert(world.corpus[N0:])
    return index


def _entry_seeds_ref(scores, entry_rows, ef):
    n_seed = min(ef, 32, entry_rows.size)
    return entry_rows[oracle.topk_of_scores(scores[:, entry_rows], n_seed)[1]]


def _search_ref(index, scores, k, ef, width, allowed=None):
    seeds = _entry_seeds_ref(scores, index.entry_rows_numpy(), ef)
    return gc.beam_search_batch_ref(scores, index.graph_numpy(), seeds, ef, width, ef, k, allowed)[:2]


@pytest.mark.parametrize("nq", [1, NQ])
def test_search_after_insert_equals_the_restatement(inserted, world, nq):
    for k, ef, width in ((10, 64, 4), (1, 16, 1)):
        got = inserted.search(world.queries[:nq], k, ef=ef, width=width)
        _same(got, _search_ref(inserted, world.scores[:nq], k, ef, width), f"nq={nq} ef={ef}")


def test_inserted_rows_find_themselves(inserted, world):
    D, I = inserted.search(world.corpus[N0:N0 + 64], 1, width=4)
    assert np.array_equal(I[:, 0], N0 + np.arange(64))


def test_allow_masks_and_removed_rows_after_insert(world, gpu):
    index = _built(world.corpus[:N0], gpu, 16)
    index.insert(world.corpus[N0:])
    rng = np.random.default_rng(51)
    removed = rng.permutation(N)[:300]
    assert index.remove_ids(removed) == 300
    live = np.ones(N, dtype=np.bool_)
    live[removed] = False
    half = rng.random(N) < 0.5
    for name, allowed, allow in (("removed", live, None), ("half", half & live, half)):
        got = index.search(world.queries, 10, ef=64, width=4, allow=allow)
        _same(got, _search_ref(index, world.scores, 10, 64, 4, allowed), name)
        assert allowed[got[1][got[1] >= 0]].all()
    # remove -> compact after an insert
    old = index.graph_numpy()
    kept = index.compact()
    assert kept.size == N - 300 and index.ntotal == N - 300
    assert np.array_equal(index.graph_numpy(), gc.remap_graph_ref(old, kept))
    assert np.array_equal(index.entry_rows_numpy(), graph_mod.entry_rows_of(N - 300, graph_mod.default_n_entry(N - 300, 16)))
    scores = oracle.scores_fma(world.queries, world.corpus[kept])
    _same(index.search(world.queries, 10, ef=64, width=4), _search_ref(index, scores, 10, 64, 4), "after compact")


def test_save_load_after_insert(inserted, world, tmp_path):
    before = inserted.search(world.queries, 10)
    inserted.save(tmp_path)
    again = GraphIndex(embedding_dim=DIM, metric="ip", device=str(inserted.device))
    again.load(tmp_path)
    assert again.ntotal == N and again.M == 16 and again.knn_k == 32 and again.n_inserted == inserted.n_inserted == N - N0
    assert np.array_equal(again.graph_numpy(), inserted.graph_numpy())
    assert np.array_equal(again.entry_rows_numpy(), inserted.entry_rows_numpy())
    _same(again.search(world.queries, 10), before, "after load")


def test_build_graph_after_inserts_is_a_fresh_build(world, gpu):
    index = _built(world.corpus[:2000], gpu, 16)
    assert index.n_inserted == 0
    index.insert(world.corpus[2000:N0])
    index.insert(world.corpus[N0:], groups=[f"g{i % 7}" for i in range(N - N0)])
    assert index.n_inserted == N - 2000 and index.ntotal == N
    index.insert(world.corpus[:0])                                 # no rows: nothing happens
    assert index.n_inserted == N - 2000 and index.ntotal == N
    index.build_graph()
    fresh = _built(world.corpus, gpu, 16)
    assert index.n_inserted == 0
    assert np.array_equal(index.graph_numpy(), fresh.graph_numpy())
    assert np.array_equal(index.entry_rows_numpy(), fresh.entry_rows_numpy())
    _same(index.search(world.queries, 10), fresh.search(world.queries, 10), "rebuilt")


def test_insert_surface(world, gpu):
    flat = _flat(world.corpus[:100], gpu)
    index = GraphIndex(flat=flat, M=8)
    with pytest.raises(RuntimeError):
        index.insert(world.corpus[100:110])                        # no graph yet
    index.build_graph()
    flat.add(world.corpus[100:110])                                # rows the graph does not cover
    with pytest.raises(RuntimeError):
        index.insert(world.corpus[110:120])
    # a fixed number of entry rows grows in proportion; an index from from_graph has no knn_k: K0 = min(2 M, 128)
    fixed = GraphIndex(flat=_flat(world.corpus[:100], gpu), M=8, n_entry=10)
    fixed.build_graph()
    fixed.insert(world.corpus[100:125])
    assert fixed.entry_rows_numpy().tolist() == gic.entry_rows_after_insert_ref(graph_mod.entry_rows_of(100, 10), 100, 25, 8,
                                                                                n_entry=10).tolist()
    assert fixed.n_entry == 13
    given = GraphIndex.from_graph(_flat(world.corpus[:100], gpu), gc.ring_graph(100, 8))
    assert given.knn_k is None
    ref = gic.insert_ref(world.corpus[:125], gc.ring_graph(100, 8), given.entry_rows_numpy(), 16)
    given.insert(world.corpus[100:125])
    assert np.array_equal(given.graph_numpy(), ref.graph) and np.array_equal(given.entry_rows_numpy(), ref.entry_rows)


# ----------------------------------------------------------------------------------------------- the recall gate
def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("case, n_build, batches", [
    ("random order", 16000, [2000, 2000]),
    ("sorted by topic", 16000, [2000, 2000]),
    ("fourfold growth", 5000, [1000] * 14 + [1, 1, 1, 997]),
])
def test_recall_gate_after_inserts(gpu, case, n_build, batches):
    """recall@10 >= 0.97 (recall_threshold of the reference's configs/index.yaml) on test_recall_gate's corpus - 64 unit
    centres, 20 000 rows, 500 noisy queries from 500 distinct rows, defaults M 32 / K0 64 / ef 64 - when part of the
    graph was inserted: of all queries, of the queries drawn from inserted rows alone, and validate().  Sorted by topic,
    every inserted row belongs to a cluster the graph has never seen.  The rebuilt graph's figures are printed beside."""
    rng = np.random.default_rng(0)
    centres = _unit(rng.standard_normal((64, DIM)))
    topic = rng.integers(0, 64, size=20000)
    rows = _unit(centres[topic] + rng.standard_normal((20000, DIM)) / np.sqrt(DIM))
    if case == "sorted by topic":
        rows = rows[np.argsort(topic, kind="stable")]
        assert not np.intersect1d(np.sort(topic)[:n_build], np.sort(topic)[n_build + 400:]).size
    picked = rng.permutation(20000)[:500]
    queries = _unit(rows[picked] + 0.5 * rng.standard_normal((500, DIM)) / np.sqrt(DIM))
    assert n_build + sum(batches) == 20000
    index = GraphIndex(embedding_dim=DIM, metric="ip", device=str(gpu))
    index.build_from_embeddings(rows[:n_build])
    lo = n_build
    for b in batches:
        index.insert(rows[lo:lo + b])
        lo += b
    assert index.ntotal == 20000 and index.M == 32 and index.knn_k == 64 and index.ef == 64
    assert index.n_inserted == 20000 - n_build
    truth = index.flat.search(queries, 10)[1]
    new = picked >= n_build
    assert new.sum() >= 50

    def figures(ix):
        found = ix.search(queries, 10)[1]
        return (ivf_mod.recall_at_k(found, truth), ivf_mod.recall_at_k(found[new], truth[new]),
                ix.validate(num_queries=1000, k=10, seed=0))

    got = figures(index)
    degree = (index.graph_numpy() >= 0).sum(axis=1)
    index.build_graph()
    rebuilt = figures(index)
    print(f"{case}: recall@10 all / inserted rows / validate(): inserted graph {got[0]:.4f} / {got[1]:.4f} / {got[2]:.4f}, "
          f"rebuilt {rebuilt[0]:.4f} / {rebuilt[1]:.4f} / {rebuilt[2]:.4f}; {int(new.sum())} queries from inserted rows, "
          f"minimum out-degree {int(degree.min())}")
    assert got[0] >= 0.97
    assert got[1] >= 0.97
    assert got[2] >= 0.97
