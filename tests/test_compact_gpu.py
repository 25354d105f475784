"""Index compaction on the MI355X: the mask rank, the row compaction kernel, and ``FAISSIndexBuilder.compact()``.

The kernels are held to numpy statements of what they write (and of what they must leave alone: sentinels behind every
output).  The product is held to the guarantee that relates three indexes - A with tombstones, B = A after
``compact()``, C = a fresh index of the surviving rows: scores bit-equal across all three, ``I_B == I_C`` and
``I_A == kept[I_B - id_offset]``, for every search entry point and every path it takes.
"""
from functools import lru_cache

import numpy as np
import pytest
import torch

from oracle import search as oracle

DIM = 384
TILE = 32
SENTINEL = 0x5EA7BEEF


def _stream(gpu):
    return int(torch.cuda.current_stream(gpu).cuda_stream)


def _bits_to_words(live, garbage_tail=True):
    """bool per row -> uint32 mask words; the bits at or past len(live) are set (as the index keeps them) or clear"""
    n = live.size
    words = -(-n // 32)
    flags = np.full(32 * words, garbage_tail, dtype=bool)
    flags[:n] = live
    return np.packbits(flags, bitorder="little").view("<u4").copy()


def _popcounts(words, n_rows):
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(np.int64)
    bits[n_rows:] = 0
    return bits.reshape(-1, 32).sum(axis=1)


def _device_words(words, gpu):
    return torch.from_numpy(words.view(np.int32)).to(gpu)


# --------------------------------------------------------------------------------------------------------------- rank
def _rank_masks(n, rng):
    """name -> (bool per row, set the bits past n?)"""
    ragged = np.zeros(n, bool)
    ragged[(n - 1) // 32 * 32:] = True
    return {
        "all": (np.ones(n, bool), False),
        "none": (np.zeros(n, bool), False),
        "half": (rng.random(n) < 0.5, False),
        "ragged_last_word": (ragged, False),
        "garbage_past_n": (rng.random(n) < 0.5, True),
        "none_but_garbage_past_n": (np.zeros(n, bool), True),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 1000, 2_097_157])
def test_row_mask_rank_is_the_exclusive_cumsum_of_popcounts(gpu, native_lib, n):
    rng = np.random.default_rng(n)
    n_words = -(-n // 32)
    assert native_lib.sskd_row_mask_words(n) == n_words
    for name, (live, garbage) in _rank_masks(n, rng).items():
        words = _bits_to_words(live, garbage)
        want = np.concatenate([[0], np.cumsum(_popcounts(words, n))])
        prefix = torch.full((n_words + 1 + 8,), -7, dtype=torch.int64, device=gpu)
        assert native_lib.sskd_row_mask_rank(_device_words(words, gpu).data_ptr(), n, prefix.data_ptr(), _stream(gpu)) == 0
        got = prefix.cpu().numpy()
        assert np.array_equal(got[: n_words + 1], want), (name, np.flatnonzero(got[: n_words + 1] != want)[:5])
        assert got[n_words] == live.sum(), name
        assert (got[n_words + 1:] == -7).all(), name               # nothing behind the live count
        # the renumbering it defines: monotone, 0 .. n_live-1 over the live rows
        rows = np.flatnonzero(live)[:: max(1, live.sum() // 50)]
        w = words[rows >> 5].astype(np.uint64)
        below = np.array([bin(int(x) & ((1 << int(r & 31)) - 1)).count("1") for x, r in zip(w, rows)], dtype=np.int64)
        assert np.array_equal(got[rows >> 5] + below, np.searchsorted(np.flatnonzero(live), rows)), name


# --------------------------------------------------------------------------------------------------------- compaction
def _compact_masks(n, rng):
    tiles = np.ones(n, bool)
    for t in range(0, -(-n // 32), 3):         # every third whole tile removed
        tiles[32 * t: 32 * t + 32] = False
    first, last, ragged = np.ones(n, bool), np.ones(n, bool), np.zeros(n, bool)
    first[0] = False
    last[n - 1] = False
    ragged[(n - 1) // 32 * 32:] = True
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "half": rng.random(n) < 0.5,
            "one_percent": rng.random(n) < 0.01, "ninety_nine_percent": rng.random(n) < 0.99, "whole_tiles": tiles,
            "first_removed": first, "last_removed": last, "ragged_tail_only": ragged}


@lru_cache(maxsize=None)
def _source(n):
    """uint32 [padded rows, 384]: random bit patterns (NaNs, infinities and denormals among them), a few rows of chosen
    special values, and non-zero words in the padding rows, which no call may copy."""
    rng = np.random.default_rng(1000 + n)
    padded = -(-n // TILE) * TILE
    src = rng.integers(0, 2**32, size=(padded, DIM), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF],
                       dtype=np.uint32)                                  # NaNs, +-inf, -0.0, +0.0, denormals
    for r in {0, n // 2, n - 1}:
        src[r] = np.resize(special, DIM)
    src[n:] = 0xBAD0BAD0
    src.setflags(write=False)
    return src


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 95, 1000, 4099])
def test_compact_rows_moves_live_rows_pads_with_zeros_and_writes_nothing_else(gpu, native_lib, n):
    rng = np.random.default_rng(n)
    src = _source(n)
    d_src = torch.from_numpy(src.view(np.int32).copy()).to(gpu)
    n_words = -(-n // 32)
    for name, live in _compact_masks(n, rng).items():
        n_live = int(live.sum())
        padded_live = -(-n_live // TILE) * TILE
        assert native_lib.sskd_index_padded_rows(n_live) == padded_live
        d_mask = _device_words(_bits_to_words(live), gpu)                # bits past n set, as the index keeps them
        prefix = torch.empty(n_words + 1, dtype=torch.int64, device=gpu)
        dst = torch.full(((padded_live + TILE), DIM), SENTINEL, dtype=torch.int32, device=gpu)
        assert native_lib.sskd_row_mask_rank(d_mask.data_ptr(), n, prefix.data_ptr(), _stream(gpu)) == 0
        assert native_lib.sskd_index_compact_rows(d_src.data_ptr(), n, d_mask.data_ptr(), prefix.data_ptr(),
                                                  dst.data_ptr(), _stream(gpu)) == 0
        got = dst.cpu().numpy().view(np.uint32)
        assert int(prefix[-1]) == n_live, name
        assert np.array_equal(got[:n_live], src[:n][live]), (name, np.flatnonzero((got[:n_live] != src[:n][live]).any(1))[:5])
        assert not got[n_live:padded_live].any(), name                   # the tail of the last tile: zeros
        assert (got[padded_live:] == SENTINEL).all(), name               # behind it: untouched
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src)      # the source is only read


# ------------------------------------------------------------------------------------------------------------ product
N, NQ = 5000, 70
THRESHOLD = 0.12


@lru_cache(maxsize=None)
def _corpus():
    """Documents of 3 consecutive chunks that resemble each other, so a query's best rows cluster by document."""
    docs = oracle.seeded_unit_rows(-(-N // 3), DIM, 401)
    groups = np.arange(N) // 3
    corpus = docs[groups] + 0.5 * oracle.seeded_unit_rows(N, DIM, 402)
    corpus = (corpus / np.linalg.norm(corpus, axis=1, keepdims=True)).astype(np.float32)
    queries = oracle.seeded_unit_rows(NQ, DIM, 403)
    keys = [f"doc{g}" for g in groups]
    chunk_ids = [f"doc{g}_{r % 3}" for r, g in enumerate(groups)]
    for a in (corpus, queries):
        a.setflags(write=False)
    return corpus, queries, keys, chunk_ids


def _builder(gpu, id_offset=0):
    from semantic_search_kd_amd import FAISSIndexBuilder

    return FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu), id_offset=id_offset)


def _all_searches(index, queries):
    """name -> the result tuple of every entry point and path, as NumPy; checks that each call took the path it is
    here for."""
    out = {}
    for k in (1, 10, 33):
        out[f"search_k{k}"] = index.search(queries, k)
        want = "chained" if k > 32 else "single+screened"
        assert index.last_search_path == want, (k, index.last_search_path)
    index.screening = False
    out["search_exact_scan"] = index.search(queries, 10)
    assert index.last_search_path == "single"
    index.screening = True
    out["search_onepass"] = index.search(queries[:1], 10)
    assert index.last_search_path == "onepass"
    out["range"] = index.range_search(queries, THRESHOLD)
    for k in (10, 33):
        out[f"grouped_k{k}"] = index.search_grouped(queries, k)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Case:
    pass


@pytest.fixture(scope="module", params=[0, 70_000], ids=["id_offset_0", "id_offset_70000"])
def abc(request, gpu, native_lib):
    """A, then B = A compacted, and C = a fresh index of the surviving rows, each with the results of every search."""
    off = request.param
    corpus, queries, keys, chunk_ids = _corpus()
    a = _builder(gpu, off)
    a.build_from_embeddings(corpus, doc_ids=chunk_ids, groups=keys)
    a.doc_texts = {cid: f"text of {cid}" for cid in chunk_ids}
    _, top = a.search(queries[:2], 1)
    best0, best1 = int(top[0, 0]) - off, int(top[1, 0]) - off
    lost_best = best0                                           # a document that loses only its best chunk
    whole_doc = best1 // 3 if best1 // 3 != best0 // 3 else best1 // 3 + 1   # a document removed entirely
    rng = np.random.default_rng(404)
    gone = rng.random(N) < 0.30
    gone[3 * (lost_best // 3): 3 * (lost_best // 3) + 3] = False
    gone[lost_best] = True
    gone[3 * whole_doc: 3 * whole_doc + 3] = True
    gone[64:96] = True                                          # one whole tile
    gone[N - 1] = True                                          # the last row
    if (N - gone.sum()) % 32 == 0:                              # the add-after-compact test needs a ragged tail
        gone[np.flatnonzero(~gone)[100]] = True
    gone = np.flatnonzero(gone)

    c = _Case()
    c.off, c.gone, c.whole_doc, c.lost_best = off, gone, whole_doc, lost_best
    c.kept_rows = np.setdiff1d(np.arange(N), gone)
    assert a.remove_ids(gone + off) == gone.size
    c.stale_filter = a.row_filter(np.ones(N, bool))
    c.a_rows = a.to_numpy()
    c.a_capacity = a._tiled.numel()
    c.a_group_keys = list(a.group_keys)
    c.res_a = _all_searches(a, queries)
    c.a_buffer = a._tiled
    c.kept = a.compact()
    c.b = a                                                     # A is B from here on
    c.res_b = _all_searches(c.b, queries)
    c.c = _builder(gpu, off)
    c.c.build_from_embeddings(c.a_rows[c.kept - off], doc_ids=[chunk_ids[r] for r in c.kept - off],
                              groups=[keys[r] for r in c.kept - off])
    c.res_c = _all_searches(c.c, queries)
    return c


@pytest.mark.gpu
def test_kept_and_the_state_after_compact(abc, native_lib):
    c, b = abc, abc.b
    corpus, _, keys, chunk_ids = _corpus()
    assert c.kept.dtype == np.int64 and np.array_equal(c.kept, c.kept_rows + c.off)
    assert (np.diff(c.kept) > 0).all()
    n_live = c.kept.size
    assert n_live % 32 != 0
    assert b.ntotal == n_live and b.n_removed == 0 and b.id_offset == c.off and b.index.ntotal == n_live
    assert b.removed_rows().size == 0
    assert b.doc_ids == [chunk_ids[r] for r in c.kept_rows]
    assert b.doc_texts == {chunk_ids[r]: f"text of {chunk_ids[r]}" for r in c.kept_rows}
    # the capacity is given back: exactly the padded live rows
    assert b._tiled.numel() == native_lib.sskd_index_padded_rows(n_live) * DIM < c.a_capacity
    assert b._tiled is not c.a_buffer
    # the stored rows are the surviving rows, bit for bit, and A's rows were the corpus
    assert np.array_equal(_bits(c.a_rows), _bits(corpus))
    assert np.array_equal(_bits(b.to_numpy()), _bits(corpus[c.kept_rows]))
    # group numbers do not change; the emptied document stays as an empty group
    assert b.group_keys == c.a_group_keys and b.n_groups == len(c.a_group_keys)
    assert np.array_equal(b.row_groups(), (np.arange(N) // 3)[c.kept_rows])
    assert b._rows_of_groups([c.whole_doc]).size == 0
    assert b.max_group_size == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["search_k1", "search_k10", "search_k33", "search_exact_scan", "search_onepass"])
def test_search_guarantee(abc, name):
    (da, ia), (db, ib), (dc, ic) = abc.res_a[name], abc.res_b[name], abc.res_c[name]
    assert np.array_equal(_bits(da), _bits(db)) and np.array_equal(_bits(db), _bits(dc))
    assert np.array_equal(ib, ic)
    hit = ib >= 0
    assert hit.all() and np.array_equal(ia, abc.kept[ib - abc.off])
    assert not np.isin(ia, abc.gone + abc.off).any()


@pytest.mark.gpu
def test_range_search_guarantee(abc):
    (la, da, ia), (lb, db, ib), (lc, dc, ic) = abc.res_a["range"], abc.res_b["range"], abc.res_c["range"]
    assert la[-1] > NQ                                           # the threshold selects something
    assert np.array_equal(la, lb) and np.array_equal(lb, lc)
    assert np.array_equal(_bits(da), _bits(db)) and np.array_equal(_bits(db), _bits(dc))
    assert np.array_equal(ib, ic) and np.array_equal(ia, abc.kept[ib - abc.off])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grouped_k10", "grouped_k33"])
def test_search_grouped_guarantee(abc, name):
    (da, ia, ga), (db, ib, gb), (dc, ic, gc) = abc.res_a[name], abc.res_b[name], abc.res_c[name]
    assert np.array_equal(_bits(da), _bits(db)) and np.array_equal(_bits(db), _bits(dc))
    assert np.array_equal(ib, ic)
    assert (ib >= 0).all() and np.array_equal(ia, abc.kept[ib - abc.off])
    # G values are unchanged by the compaction; the fresh index numbers its groups anew but means the same documents
    assert np.array_equal(ga, gb)
    assert abc.b.group_key(gb) == abc.c.group_key(gc)
    assert not (gb == abc.whole_doc).any()                       # the document removed entirely is gone ...
    q0 = gb[0] == abc.lost_best // 3                             # ... the one that lost its best chunk still answers
    if q0.any():
        assert ia[0][q0][0] - abc.off != abc.lost_best and (ia[0][q0][0] - abc.off) // 3 == abc.lost_best // 3


@pytest.mark.gpu
def test_a_filter_prepared_before_the_compaction_is_refused(abc):
    _, queries, _, _ = _corpus()
    with pytest.raises(ValueError, match="prepared for"):
        abc.b.search(queries, 10, allow=abc.stale_filter)
    fresh = abc.b.row_filter(np.ones(abc.b.ntotal, bool))
    d, i = abc.b.search(queries, 10, allow=fresh)
    assert np.array_equal(i, abc.res_b["search_k10"][1]) and np.array_equal(_bits(d), _bits(abc.res_b["search_k10"][0]))


@pytest.mark.gpu
def test_save_after_compact_writes_only_the_survivors(abc, gpu, tmp_path):
    _, queries, _, _ = _corpus()
    (tmp_path / "removed.npy").write_bytes(b"left over from an earlier save")
    abc.b.save(tmp_path)
    assert not (tmp_path / "removed.npy").exists()
    from semantic_search_kd_amd.index import read_flat_ip

    assert read_flat_ip(tmp_path / "index.faiss").shape == (abc.kept.size, DIM)
    again = _builder(gpu)
    again.load(tmp_path)
    assert again.ntotal == abc.kept.size and again.n_removed == 0 and again.id_offset == abc.off
    assert again.doc_ids == abc.b.doc_ids and again.group_keys == abc.b.group_keys
    for k, name in ((10, "search_k10"), (33, "search_k33")):
        d, i = again.search(queries, k)
        assert np.array_equal(i, abc.res_b[name][1]) and np.array_equal(_bits(d), _bits(abc.res_b[name][0]))
    d, i, g = again.search_grouped(queries, 10)
    assert np.array_equal(i, abc.res_b["grouped_k10"][1]) and np.array_equal(g, abc.res_b["grouped_k10"][2])


@pytest.mark.gpu
def test_no_removals_is_the_identity_and_keeps_the_buffer(gpu):
    corpus, _, _, _ = _corpus()
    index = _builder(gpu, 11)
    index.build_from_embeddings(corpus[:100])
    buffer, handle = index._tiled, index.index
    kept = index.compact()
    assert kept.dtype == np.int64 and np.array_equal(kept, 11 + np.arange(100))
    assert index._tiled is buffer and index.index is handle and index.ntotal == 100
    assert np.array_equal(index.index.compact(), kept)           # the handle forwards


@pytest.mark.gpu
def test_add_after_compact_repacks_the_ragged_tail(gpu):
    """The zero padding behind the last live row is what ``add`` relies on: 1 000 rows, 337 removed (663 = 20 tiles +
    23), 10 rows added, compared with a fresh build of the same 673 rows."""
    corpus, queries, keys, _ = _corpus()
    rng = np.random.default_rng(405)
    gone = np.sort(rng.choice(1000, 337, replace=False))
    kept_rows = np.setdiff1d(np.arange(1000), gone)
    index = _builder(gpu)
    index.build_from_embeddings(corpus[:1000], groups=keys[:1000])
    index.remove_ids(gone)
    assert np.array_equal(index.compact(), kept_rows) and index.ntotal % 32 == 23
    index.add(corpus[4000:4010], groups=keys[4000:4010])
    rows = np.concatenate([corpus[kept_rows], corpus[4000:4010]])
    fresh = _builder(gpu)
    fresh.build_from_embeddings(rows, groups=[keys[r] for r in kept_rows] + keys[4000:4010])
    assert index.ntotal == 673 and np.array_equal(_bits(index.to_numpy()), _bits(rows))
    for q, k in ((queries, 10), (queries, 33), (queries[:1], 10)):
        d, i = index.search(q, k)
        d2, i2 = fresh.search(q, k)
        assert np.array_equal(i, i2) and np.array_equal(_bits(d), _bits(d2))
    d, i, g = index.search_grouped(queries, 10)
    d2, i2, g2 = fresh.search_grouped(queries, 10)
    assert np.array_equal(i, i2) and np.array_equal(_bits(d), _bits(d2)) and index.group_key(g) == fresh.group_key(g2)
    # removal and compaction work again on the grown index
    index.remove_ids([672])
    assert np.array_equal(index.compact(), np.arange(672)) and index.ntotal == 672


@pytest.mark.gpu
def test_remove_everything_then_add(gpu):
    corpus, queries, keys, chunk_ids = _corpus()
    index = _builder(gpu, 5)
    index.build_from_embeddings(corpus[:100], doc_ids=chunk_ids[:100], groups=keys[:100])
    index.doc_texts = {cid: cid for cid in chunk_ids[:100]}
    index.remove_ids(5 + np.arange(100))
    kept = index.compact()
    assert kept.size == 0 and kept.dtype == np.int64
    assert index.ntotal == 0 and index.n_removed == 0 and index.doc_ids == [] and index.doc_texts == {}
    assert index.n_groups == 34 and index.max_group_size == 1
    d, i = index.search(queries[:3], 5)
    assert (i == -1).all()
    index.add(corpus[200:250], groups=keys[200:250])
    fresh = _builder(gpu, 5)
    fresh.build_from_embeddings(corpus[200:250])
    d, i = index.search(queries[:3], 5)
    d2, i2 = fresh.search(queries[:3], 5)
    assert index.ntotal == 50 and np.array_equal(i, i2) and np.array_equal(_bits(d), _bits(d2))
