"""Index compaction, the parts that need no GPU: the two C-ABI entry points check their arguments before any launch,
``compact()`` refuses a piece of a row-sharded build, and the host bookkeeping (doc ids, texts, row groups) equals its
numpy statement - on a ``FAISSIndexBuilder`` that never touches the device."""
import numpy as np
import pytest

NEW_SYMBOLS = ["sskd_row_mask_rank", "sskd_index_compact_rows"]
ROW_BYTES = 384 * 4
SRC, MASK, PREFIX = 0x10_0000_0000, 0x20_0000_0000, 0x30_0000_0000   # never dereferenced: every call fails its checks


def test_compact_symbols_are_declared_and_exported(native_lib):
    from semantic_search_kd_amd import _native
    from test_capi_symbols import _declared_symbols

    declared = _declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.SIGNATURES and hasattr(native_lib, name), name
    assert native_lib.sskd_abi_version() == 1


def _fails(native_lib, rc, text):
    assert rc != 0
    msg = native_lib.sskd_last_error()
    assert msg and text in msg, msg


def test_row_mask_rank_argument_errors(native_lib):
    rank = native_lib.sskd_row_mask_rank
    _fails(native_lib, rank(MASK, -1, PREFIX, None), b"row_mask_rank: n_rows < 0")
    _fails(native_lib, rank(None, 10, PREFIX, None), b"row_mask_rank: null pointer")
    _fails(native_lib, rank(MASK, 10, None, None), b"row_mask_rank: null pointer")
    _fails(native_lib, rank(MASK, 2**31, PREFIX, None), b"row_mask_rank: shard too large")
    assert rank(None, 0, None, None) == 0          # nothing to rank: a no-op, before any pointer is looked at


def test_index_compact_rows_argument_errors(native_lib):
    compact = native_lib.sskd_index_compact_rows
    n = 100                                        # 4 tiles = 128 stored rows
    dst = SRC + 128 * ROW_BYTES                    # right behind the source: fine as far as the checks go
    _fails(native_lib, compact(SRC, -1, MASK, PREFIX, dst, None), b"index_compact_rows: n_rows < 0")
    for args in [(None, n, MASK, PREFIX, dst), (SRC, n, None, PREFIX, dst), (SRC, n, MASK, None, dst),
                 (SRC, n, MASK, PREFIX, None)]:
        _fails(native_lib, compact(*args, None), b"index_compact_rows: null pointer")
    _fails(native_lib, compact(SRC, 2**31, MASK, PREFIX, dst, None), b"index_compact_rows: shard too large")
    # overlap: in place, a destination inside the source (first byte, last row), a source inside the destination's
    # first tile
    for bad in [SRC, SRC + ROW_BYTES, SRC + 127 * ROW_BYTES, SRC - ROW_BYTES, SRC - 31 * ROW_BYTES]:
        _fails(native_lib, compact(SRC, n, MASK, PREFIX, bad, None), b"source and destination overlap")
    assert compact(None, 0, None, None, None, None) == 0


def _builder():
    from semantic_search_kd_amd import FAISSIndexBuilder

    return FAISSIndexBuilder(embedding_dim=384, metric="ip", device="cuda:0")   # the constructor touches no device


def test_compact_refuses_a_row_shard():
    index = _builder()
    index.shard_info = {"rank": 1, "world_size": 2, "n_total": 100}
    index.id_offset = 50
    with pytest.raises(ValueError, match="row-sharded"):
        index.compact()
    from semantic_search_kd_amd.index import IndexHandle

    with pytest.raises(ValueError, match="row-sharded"):
        IndexHandle(index).compact()


def test_nothing_removed_is_the_identity_without_a_device():
    index = _builder()
    index._n, index.id_offset = 7, 1000
    assert np.array_equal(index.compact(), 1000 + np.arange(7))
    assert index.compact().dtype == np.int64 and index.ntotal == 7


def test_kept_rows_is_the_complement():
    from semantic_search_kd_amd.index import _kept_rows

    assert np.array_equal(_kept_rows(6, np.array([0, 3, 5])), [1, 2, 4])
    assert np.array_equal(_kept_rows(3, np.zeros(0, np.int64)), [0, 1, 2])
    assert _kept_rows(3, np.arange(3)).size == 0 and _kept_rows(3, np.arange(3)).dtype == np.int64


def test_host_bookkeeping_matches_numpy():
    """12 rows in runs of 3 chunks per document (the last row without a key): documents 'a' .. 'd' are groups 0 .. 3, the
    keyless row is group 4.  Document 'b' goes entirely, 'c' loses one chunk, the keyless row goes."""
    n = 13
    keys = [k for k in "abcd" for _ in range(3)] + [None]
    index = _builder()
    index._n = n
    index.doc_ids = [f"{k}_{j}" for k in "abcd" for j in range(3)] + ["loose"]
    index.doc_texts = {cid: f"text of {cid}" for cid in index.doc_ids}
    index.doc_texts["orphan"] = "a text no row ever referred to"
    index.set_groups(keys)
    before = index.row_groups().copy()
    assert index.n_groups == 5 and index.max_group_size == 3
    assert np.array_equal(index._rows_of_groups([1]), [3, 4, 5])            # builds the CSR that must be dropped
    gone = np.array([3, 4, 5, 7, 12])
    kept = np.setdiff1d(np.arange(n), gone)
    old_ids, old_keys = list(index.doc_ids), list(index.group_keys)

    index._n = kept.size
    index._compact_host(kept)

    assert index.doc_ids == [old_ids[r] for r in kept]
    assert index.doc_texts == {old_ids[r]: f"text of {old_ids[r]}" for r in kept}   # pruned, the orphan included
    assert np.array_equal(index.row_groups(), before[kept]) and index.row_groups().dtype == np.int32
    # group numbers do not change; emptied groups stay as empty groups
    assert index.group_keys == old_keys and index.n_groups == 5
    assert index._group_of_key == {"a": 0, "b": 1, "c": 2, "d": 3}
    assert index.group_key(2) == "c" and index.group_key(1) == "b"
    assert index.max_group_size == 3
    new_groups = before[kept]
    for g in range(5):
        assert np.array_equal(index._rows_of_groups([g]), np.flatnonzero(new_groups == g)), g
    assert index._rows_of_groups([1]).size == 0 and index._rows_of_groups([4]).size == 0
    assert np.array_equal(index._rows_of_groups([2, 1, 0]), [3, 4, 0, 1, 2])            # old rows 6 and 8, then 0 1 2
    # a known key still joins its (now smaller, or empty) group
    index._extend_groups(kept.size, 2, ["b", "c"])
    assert np.array_equal(index.row_groups()[-2:], [1, 2]) and index.n_groups == 5

    # everything removed: empty arrays, and the largest group of nothing is 1 as for an empty index
    index._n = 0
    index._compact_host(np.zeros(0, np.int64))
    assert index.doc_ids == [] and index.doc_texts == {} and index.row_groups().size == 0
    assert index.max_group_size == 1 and index.n_groups == 5 and index._rows_of_groups([0, 1, 2, 3, 4]).size == 0


def test_host_bookkeeping_without_groups_or_texts():
    index = _builder()
    index._n = 5
    index.doc_ids = [f"doc_{i}" for i in range(5)]
    index._n = 3
    index._compact_host(np.array([0, 2, 4]))
    assert index.doc_ids == ["doc_0", "doc_2", "doc_4"] and index.doc_texts is None
    assert index.group_keys is None and np.array_equal(index.row_groups(), [0, 1, 2])   # still ungrouped: row = group


def test_rows_added_without_doc_ids_do_not_break_the_gather():
    """``add`` appends rows but no doc ids: ``doc_ids`` then covers only the first rows, and those keep theirs."""
    index = _builder()
    index.doc_ids = [f"doc_{i}" for i in range(4)]          # 4 ids, 7 rows: 3 were added later
    index.doc_texts = {f"doc_{i}": str(i) for i in range(4)}
    index._n = 4
    index._compact_host(np.array([1, 3, 4, 6]))
    assert index.doc_ids == ["doc_1", "doc_3"] and index.doc_texts == {"doc_1": "1", "doc_3": "3"}
