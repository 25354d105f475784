"""IVF index, host side (no GPU): the list arithmetic in NumPy, the files, the launch plan and the argument checks of
``sskd_ivf_search`` / ``sskd_ivf_list_sums`` through ctypes (a refused call returns before any HIP call)."""
import json

import numpy as np
import pytest

from semantic_search_kd_amd import IVFIndex, ivf

SSKD_ERR_INVALID = 1


# ------------------------------------------------------------------------------------------------ the CSR
@pytest.mark.parametrize("n, nlist, seed", [(3001, 16, 0), (100, 7, 1), (5, 1, 2), (0, 3, 3)])
def test_csr_from_assignment(n, nlist, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, nlist, size=n)
    if n > 50:
        a[a == 3] = 4   # an empty list in the middle
    offsets, rows = ivf.csr_from_assignment(a, nlist)
    assert offsets.dtype == np.int64 and rows.dtype == np.int32 and offsets.shape == (nlist + 1,) and rows.shape == (n,)
    assert offsets[0] == 0 and offsets[-1] == n and (np.diff(offsets) >= 0).all()
    assert np.array_equal(np.sort(rows), np.arange(n))          # every row exactly once
    for l in range(nlist):
        part = rows[offsets[l]:offsets[l + 1]]
        assert (a[part] == l).all() and (np.diff(part) > 0).all()   # the list's own rows, ascending
        assert part.size == int((a == l).sum())
    if n > 50:
        assert offsets[3] == offsets[4]                             # the empty list is two equal offsets
    ivf.check_csr(offsets, rows, n)
    assert np.array_equal(ivf.assignment_from_csr(offsets, rows), a)


def test_csr_rejects_bad_input():
    with pytest.raises(ValueError):
        ivf.csr_from_assignment([0, 1, 5], 4)
    with pytest.raises(ValueError):
        ivf.csr_from_assignment([0, -1], 4)
    with pytest.raises(ValueError):
        ivf.csr_from_assignment([0.5, 1.0], 4)
    with pytest.raises(ValueError):
        ivf.csr_from_assignment([0], 0)
    offsets, rows = ivf.csr_from_assignment([1, 0, 1, 0], 2)
    with pytest.raises(ValueError):
        ivf.check_csr(offsets, rows[::-1].copy(), 4)      # descending inside a list
    with pytest.raises(ValueError):
        ivf.check_csr(offsets, np.array([0, 0, 1, 3], np.int32), 4)   # a row twice
    with pytest.raises(ValueError):
        ivf.check_csr(np.array([0, 3, 2, 4]), rows, 4)    # offsets fall


def test_default_nlist():
    assert [ivf.default_nlist(n) for n in (0, 1, 2, 3001, 10 ** 6, 10 ** 12)] == [1, 1, 1, 55, 1000, 65536]


def _remap_restated(offsets, rows, kept):
    """The rule in plain Python: walk every list, drop rows that are gone, renumber the rest by position in kept."""
    new_number = {int(old): j for j, old in enumerate(kept)}
    out_rows, out_offsets = [], [0]
    for l in range(len(offsets) - 1):
        for r in rows[offsets[l]:offsets[l + 1]]:
            if int(r) in new_number:
                out_rows.append(new_number[int(r)])
        out_offsets.append(len(out_rows))
    return np.array(out_offsets, np.int64), np.array(out_rows, np.int32)


@pytest.mark.parametrize("drop", ["some", "none", "all", "one_list"])
def test_remap_lists_after_compact(drop):
    rng = np.random.default_rng(7)
    n, nlist = 500, 9
    a = rng.integers(0, nlist, size=n)
    offsets, rows = ivf.csr_from_assignment(a, nlist)
    gone = {"some": rng.random(n) < 0.3, "none": np.zeros(n, bool), "all": np.ones(n, bool), "one_list": a == 2}[drop]
    kept = np.flatnonzero(~gone).astype(np.int64)
    new_offsets, new_rows = ivf.remap_lists(offsets, rows, kept)
    ref_offsets, ref_rows = _remap_restated(offsets, rows, kept)
    assert np.array_equal(new_offsets, ref_offsets) and np.array_equal(new_rows, ref_rows)
    assert new_rows.dtype == np.int32 and new_offsets.dtype == np.int64
    ivf.check_csr(new_offsets, new_rows, kept.size)
    # the same lists as building from the surviving rows' assignment
    again = ivf.csr_from_assignment(a[kept], nlist)
    assert np.array_equal(new_offsets, again[0]) and np.array_equal(new_rows, again[1])


def test_files_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    centroids = rng.standard_normal((6, 384)).astype(np.float32)
    offsets, rows = ivf.csr_from_assignment(rng.integers(0, 6, size=200), 6)
    ivf.save_lists(tmp_path, centroids, offsets, rows, {"nprobe": 3, "seed": 99, "iterations": 4})
    meta = json.loads((tmp_path / "ivf.json").read_text())
    assert meta == {"nprobe": 3, "seed": 99, "iterations": 4, "nlist": 6, "format_version": 1}
    assert ivf.is_ivf_dir(tmp_path) and not ivf.is_ivf_dir(tmp_path / "nowhere")
    c2, o2, r2, m2 = ivf.load_lists(tmp_path)
    assert np.array_equal(c2.view(np.int32), centroids.view(np.int32)) and c2.dtype == np.float32
    assert np.array_equal(o2, offsets) and o2.dtype == np.int64 and np.array_equal(r2, rows) and r2.dtype == np.int32
    assert m2 == meta
    # a damaged file is noticed
    bad = rows.copy()
    bad[0] = bad[1]
    np.save(tmp_path / "ivf_list_rows.npy", bad)
    with pytest.raises(ValueError):
        ivf.load_lists(tmp_path)
    np.save(tmp_path / "ivf_list_rows.npy", rows)
    (tmp_path / "ivf.json").write_text(json.dumps({**meta, "format_version": 2}))
    with pytest.raises(ValueError):
        ivf.load_lists(tmp_path)


def test_recall_at_k():
    found = np.array([[1, 2, 3], [4, 5, -1], [7, 8, 9]])
    truth = np.array([[3, 2, 1], [4, 6, -1], [-1, -1, -1]])
    assert ivf.recall_at_k(found, truth) == pytest.approx((1.0 + 0.5 + 1.0) / 3)


def test_exported():
    assert IVFIndex is ivf.IVFIndex


# ------------------------------------------------------------------------------------- the plan, through ctypes
def _plan(lib, nq, nprobe, k, n_rows, max_list_rows):
    import ctypes as C

    parts, chunk, wgs = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = lib.sskd_ivf_search_plan(nq, nprobe, k, n_rows, max_list_rows, C.byref(parts), C.byref(chunk), C.byref(wgs))
    return rc, parts.value, chunk.value, wgs.value


@pytest.mark.parametrize("nq, nprobe, k, n_rows, longest", [
    (1, 32, 10, 1_000_000, 2000), (1, 1, 256, 3001, 400), (64, 32, 10, 1_000_000, 2000), (10_000, 128, 100, 1_000_000, 5000),
    (1, 16, 1, 3001, 2700), (200, 16, 256, 3001, 300), (1, 1, 1, 0, 0), (3, 65536, 10, 8_800_000, 1000),
])
def test_plan_and_workspace(native_lib, nq, nprobe, k, n_rows, longest):
    rc, parts, chunk, wgs = _plan(native_lib, nq, nprobe, k, n_rows, longest)
    assert rc == 0 and parts >= 1 and chunk >= 1 and wgs == parts * nq
    assert parts * k <= max(2048, k)          # the candidates of one query the merge is asked to read
    assert parts <= max(1, -(-min(n_rows, nprobe * longest) // chunk))   # no part shorter than a chunk by plan
    need = int(native_lib.sskd_ivf_search_workspace_bytes(nq, nprobe, k, n_rows, longest))
    assert need >= parts * nq * k * (4 + 8)   # one (float, int64) record per part, query and slot
    # any out pointer may be NULL
    assert native_lib.sskd_ivf_search_plan(nq, nprobe, k, n_rows, longest, None, None, None) == 0


def test_plan_spreads_a_single_query_and_not_a_batch(native_lib):
    assert _plan(native_lib, 1, 32, 10, 1_000_000, 2000)[1] >= 128      # one query spreads over the chip
    assert _plan(native_lib, 10_000, 32, 10, 1_000_000, 2000)[1] == 1   # a batch has one workgroup per query


@pytest.mark.parametrize("nq, nprobe, k, n_rows, longest", [
    (0, 1, 1, 10, 10), (1, 0, 1, 10, 10), (1, 65537, 1, 10, 10), (1, 1, 0, 10, 10), (1, 1, 257, 10, 10), (1, 1, 1, -1, 0),
    (1, 1, 1, 10, -1),
])
def test_plan_refuses(native_lib, nq, nprobe, k, n_rows, longest):
    assert _plan(native_lib, nq, nprobe, k, n_rows, longest)[0] == SSKD_ERR_INVALID
    assert native_lib.sskd_last_error()
    assert native_lib.sskd_ivf_search_workspace_bytes(nq, nprobe, k, n_rows, longest) == 0


# ------------------------------------------------------------------- refusal before anything is enqueued, through ctypes
P = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused on the host


def _search_args(**over):
    a = dict(tiled=P, n_rows=1000, queries=P, nq=2, probe=P, nprobe=4, offsets=P, rows=P, nlist=16, k=10, id_offset=0,
             mask=None, out_s=P, out_i=P, ws=P, ws_bytes=1 << 30, stream=None)
    a.update(over)
    return [a[key] for key in ("tiled", "n_rows", "queries", "nq", "probe", "nprobe", "offsets", "rows", "nlist", "k",
                               "id_offset", "mask", "out_s", "out_i", "ws", "ws_bytes", "stream")]


@pytest.mark.parametrize("over, word", [
    (dict(k=0), "k=0"), (dict(k=257), "k=257"), (dict(nprobe=0), "nprobe=0"), (dict(nprobe=17), "nprobe=17"),
    (dict(nlist=0), "nlist=0"), (dict(nlist=65537, nprobe=1), "nlist=65537"), (dict(n_rows=-1), "n_rows"),
    (dict(nq=-1), "nq"), (dict(nq=65536), "nq=65536"), (dict(id_offset=-1), "id_offset"),
    (dict(n_rows=(1 << 31) - 64), "int32"),
    (dict(tiled=None), "null"), (dict(queries=None), "null"), (dict(probe=None), "null"), (dict(offsets=None), "null"),
    (dict(rows=None), "null"), (dict(out_s=None), "null"), (dict(out_i=None), "null"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=16), "workspace"), (dict(ws_bytes=0), "workspace"),
    (dict(queries=P + 4), "aligned"), (dict(ws=P + 8), "aligned"),
])
def test_search_refuses_bad_arguments(native_lib, over, word):
    rc = native_lib.sskd_ivf_search(*_search_args(**over))
    assert rc == SSKD_ERR_INVALID
    assert word in native_lib.sskd_last_error().decode()


def test_search_with_no_queries_is_a_noop(native_lib):
    assert native_lib.sskd_ivf_search(*_search_args(nq=0, queries=None, probe=None, out_s=None, out_i=None, ws=None,
                                                    ws_bytes=0)) == 0


@pytest.mark.parametrize("over, word", [
    (dict(nlist=-1), "nlist"), (dict(nlist=65537), "nlist"), (dict(n_rows=-1), "n_rows"), (dict(offsets=None), "null"),
    (dict(sums=None), "null"), (dict(tiled=None), "null"), (dict(rows=None), "null"),
])
def test_list_sums_refuses_bad_arguments(native_lib, over, word):
    a = dict(tiled=P, n_rows=100, offsets=P, rows=P, nlist=4, sums=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_ivf_list_sums(*[a[key] for key in ("tiled", "n_rows", "offsets", "rows", "nlist", "sums", "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_ivf_list_sums(None, 0, None, None, 0, None, None) == 0   # no lists: nothing to do
