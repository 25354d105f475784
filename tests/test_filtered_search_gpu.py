"""Filtered search and document removal on the MI355X: a row allow-mask honoured by every search path.

The oracle: a filtered search returns the bits of a search over the allowed rows only, ids mapped back
(``allowed_rows[i]``), padding slots ``(-FLT_MAX, -1)`` - computed here as the fma-order scores of every row with the
masked rows set to -inf, which ``topk_of_scores`` skips exactly as the kernels do.
"""
import numpy as np
import pytest
import torch

from oracle import search as oracle

DIM = 384


def _ref(queries, corpus, allowed, k, id_offset=0):
    s = oracle.scores_fma(queries, corpus)
    s[:, ~allowed] = -np.inf
    return oracle.topk_of_scores(s, k, id_offset)


def _index(corpus, gpu):
    from semantic_search_kd_amd import FAISSIndexBuilder

    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu))
    index.build_from_embeddings(corpus)
    return index


def _masks(n, k, rng):
    """name -> bool allow array over n rows"""
    m = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "half": rng.random(n) < 0.5, "one_percent": rng.random(n) < 0.01}
    tiles = np.ones(n, bool)
    for t in range(0, (n + 31) // 32, 3):     # every third whole tile masked
        tiles[32 * t: 32 * t + 32] = False
    m["whole_tiles"] = tiles
    last = np.zeros(n, bool)
    last[(n - 1) // 32 * 32:] = True          # only the (ragged) last tile
    m["ragged_last_tile"] = last
    few = np.zeros(n, bool)
    few[rng.choice(n, max(1, k // 2), replace=False)] = True
    m["fewer_than_k"] = few
    return m


def _check(index, queries, corpus, allowed, k, path):
    s, i = index.search(queries, k, allow=allowed)
    ref_s, ref_i = _ref(queries, corpus, allowed, k)
    assert index.last_search_path.startswith(path) or index.last_search_path.endswith(path), index.last_search_path
    assert np.array_equal(i, ref_i), (path, np.argwhere(i != ref_i)[:5])
    assert np.array_equal(s, ref_s), path
    assert not np.isin(i[i >= 0], np.flatnonzero(~allowed)).any()
    return s, i


# (n rows, nq, k, expected path)
PATHS = [
    (5000, 100, 10, "single"),            # the exact scan, k <= 32 (run with screening off below)
    (3001, 200, 100, "chained"),
    (3001, 80, 1000, "chained"),
    (20_003, 3, 10, "onepass"),
    (20_003, 64, 256, "onepass"),
    (6_007, 256, 10, "+screened"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,nq,k,path", PATHS)
def test_filtered_search_every_path_every_mask(gpu, n, nq, k, path):
    rng = np.random.default_rng(n + nq + k)
    corpus = oracle.seeded_unit_rows(n, DIM, n)
    queries = oracle.seeded_unit_rows(nq, DIM, nq + 7)
    index = _index(corpus, gpu)
    if path == "single":
        index.screening = False
    for allowed in _masks(n, k, rng).values():
        _check(index, queries, corpus, allowed, k, path)   # (one-pass: proven, or "onepass-unproven+chained")
    # all allowed = the unfiltered call, bit for bit
    s0, i0 = index.search(queries, k)
    s1, i1 = index.search(queries, k, allow=np.ones(n, bool))
    assert np.array_equal(s0, s1) and np.array_equal(i0, i1)


@pytest.mark.gpu
def test_onepass_proof_fails_and_the_chained_fallback_keeps_the_mask(gpu):
    """k = 256 over a corpus whose best rows for the query crowd into few per-lane lists: the one-pass proof fails and
    the chained passes answer - with the same mask."""
    n = 40_000
    corpus = oracle.seeded_unit_rows(n, DIM, 3)
    q = oracle.seeded_unit_rows(1, DIM, 4)
    # 600 near-copies of the query on consecutive rows: the lists that see them fill with them and drop some
    corpus[1000:1600] = q + 0.05 * oracle.seeded_unit_rows(600, DIM, 5)
    corpus[1000:1600] /= np.linalg.norm(corpus[1000:1600], axis=1, keepdims=True)
    index = _index(corpus, gpu)
    allowed = np.random.default_rng(1).random(n) < 0.9   # dense enough that those lists still fill
    _check(index, q, corpus, allowed, 256, "onepass-unproven+chained")


@pytest.mark.gpu
def test_screened_mask_stress(gpu):
    n, nq, k = 8192, 256, 10
    corpus = oracle.seeded_unit_rows(n, DIM, 21)
    queries = oracle.seeded_unit_rows(nq, DIM, 22)
    index = _index(corpus, gpu)
    sample_rows = 64 * 32 if n // 32 // 8 >= 64 else (n // 32 // 8) * 32   # the sample phase's first tiles
    no_sample = np.ones(n, bool)
    no_sample[:sample_rows] = False
    only_sample = ~no_sample
    for allowed in (no_sample, only_sample):
        _check(index, queries, corpus, allowed, k, "+screened")
    # duplicate-heavy: 320 allowed copies of one row next to a quarter of the queries force the in-call fallback
    dup = corpus.copy()
    dup[3000:3000 + 320] = dup[77]
    q = queries.copy()
    for j in range(0, nq, 4):
        q[j] = dup[77] + 0.02 * q[j]
        q[j] /= np.linalg.norm(q[j])
    di = _index(dup, gpu)
    allowed = np.random.default_rng(2).random(n) < 0.9
    allowed[3000:3000 + 320] = True
    _check(di, q, dup, allowed, k, "+screened")
    assert int(di.last_status[1]) > 0
    # topic-sorted: rows sorted by their score for query 0, so scores ascend along the shard
    order = np.argsort(oracle.scores_fma(queries[:1], corpus)[0])
    ts = np.ascontiguousarray(corpus[order])
    ti = _index(ts, gpu)
    allowed = np.random.default_rng(3).random(n) < 0.5
    _check(ti, queries, ts, allowed, k, "+screened")


@pytest.mark.gpu
def test_screened_full_size_half_mask_equals_a_subindex(gpu):
    """1 M rows x 10 000 queries, 50 % mask: the filtered screened search equals the search of an index built from
    the allowed rows alone, ids mapped back."""
    n, nq, k = 1_000_000, 10_000, 10
    g = torch.Generator(device=gpu).manual_seed(7)
    corpus = torch.nn.functional.normalize(torch.randn(n, DIM, device=gpu, generator=g), dim=1)
    queries = torch.nn.functional.normalize(torch.randn(nq, DIM, device=gpu, generator=g), dim=1)
    allowed = torch.rand(n, device=gpu, generator=g) < 0.5
    index = _index(corpus, gpu)
    sub = _index(corpus[allowed].contiguous(), gpu)
    rows = torch.nonzero(allowed).reshape(-1)
    f = index.row_filter(allowed)
    s, i = index.search_device(queries, k, allow=f)
    assert index.last_status is not None                 # the screened path served it
    s2, i2 = sub.search_device(queries, k)
    torch.cuda.synchronize()
    assert torch.equal(s, s2)
    assert torch.equal(i, rows[i2])


@pytest.mark.gpu
def test_remove_add_search_save_load_round_trip(gpu, tmp_path):
    from semantic_search_kd_amd import FAISSIndexBuilder

    n, nq, k = 3000, 5, 20
    corpus = oracle.seeded_unit_rows(n + 500, DIM, 31)
    queries = oracle.seeded_unit_rows(nq, DIM, 32)
    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu), id_offset=0)
    index.build_from_embeddings(corpus[:n])
    _, top = index.search(queries, k)
    gone = np.unique(np.concatenate([top[:, :3].ravel(), [5, 6, 7]]))
    assert index.remove_ids(gone) == gone.size
    assert index.remove_ids(torch.from_numpy(gone[:2]).to(gpu)) == 0            # twice: no error, nothing new
    assert index.remove_ids([]) == 0
    with pytest.raises(ValueError):
        index.remove_ids([n])
    assert index.n_removed == gone.size and index.ntotal == n
    index.add(corpus[n:])                                                        # appended rows are live
    allowed = np.ones(n + 500, bool)
    allowed[gone] = False
    s, i = index.search(queries, k)
    ref = _ref(queries, corpus, allowed, k)
    assert np.array_equal(i, ref[1]) and np.array_equal(s, ref[0])
    # a per-call filter on top of the removals: allow AND NOT removed
    part = np.random.default_rng(4).random(n + 500) < 0.3
    s, i = index.search(queries, k, allow=part)
    ref = _ref(queries, corpus, allowed & part, k)
    assert np.array_equal(i, ref[1]) and np.array_equal(s, ref[0])
    index.save(tmp_path / "a")
    assert np.array_equal(np.load(tmp_path / "a" / "removed.npy"), gone)
    again = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu))
    again.load(tmp_path / "a")
    assert again.n_removed == gone.size
    s2, i2 = again.search(queries, k)
    ref = _ref(queries, corpus, allowed, k)
    assert np.array_equal(i2, ref[1]) and np.array_equal(s2, ref[0])
    # load(append=True): the second copy's tombstones are offset by the rows in front of it
    again.load(tmp_path / "a", append=True)
    both = np.concatenate([corpus, corpus])
    assert again.n_removed == 2 * gone.size
    s3, i3 = again.search(queries, k)
    ref = _ref(queries, both, np.concatenate([allowed, allowed]), k)
    assert np.array_equal(i3, ref[1]) and np.array_equal(s3, ref[0])
    # build / load(append=False) reset the tombstones
    again.build_from_embeddings(corpus[:n])
    assert again.n_removed == 0
    again.save(tmp_path / "a")
    assert not (tmp_path / "a" / "removed.npy").exists()
