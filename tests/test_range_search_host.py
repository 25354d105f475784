"""Range search, host side (no GPU): workspace sizing, argument checks through ctypes, and the NumPy helpers
behind ``range_search`` / ``near_duplicates``."""
import ctypes as C

import numpy as np
import pytest

from semantic_search_kd_amd import _native
from semantic_search_kd_amd.index import pairs_from_ranges, range_thresholds

ERR_INVALID, ERR_WORKSPACE = 1, 2


def test_range_symbols_are_declared_and_bound(native_lib):
    for name in ("sskd_index_range_search_workspace_bytes", "sskd_index_range_search"):
        assert name in _native.SIGNATURES and hasattr(native_lib, name)


def test_workspace_is_monotone_and_safe_at_zero(native_lib):
    ws = native_lib.sskd_index_range_search_workspace_bytes
    assert ws(0, 0, 0) == 0 and ws(1000, 0, 10) == 0 and ws(0, 10, 10) == 0
    assert ws(-1, 10, 10) == 0 and ws(1000, -1, 10) == 0 and ws(1000, 10, -1) == 0
    for n in (1, 31, 33, 3001, 1_000_000):
        prev = 0
        for nq in (1, 2, 31, 32, 33, 64, 65, 97, 129, 193, 256, 257, 1000, 4096, 4097, 10_000, 100_000):
            cur = ws(n, nq, 100)
            assert cur >= prev > 0 or (prev == 0 and cur > 0), (n, nq, prev, cur)
            prev = cur
        prev = 0
        for mr in (0, 1, 10, 1000, 1 << 20, 1 << 26):
            cur = ws(n, 64, mr)
            assert cur >= prev, (n, mr, prev, cur)
            prev = cur
    # the pool holds max_results records at least (8 B key + 4 B query each)
    assert ws(1_000_000, 10_000, 1 << 24) >= 12 * (1 << 24)


def _call(lib, n_rows=100, nq=4, max_results=16, lims=True, tiled=True, queries=True, thr=True, outs=True,
          ws_bytes=None, ws=True):
    buf = (C.c_byte * 64)()
    p = C.addressof(buf)
    if ws_bytes is None:
        ws_bytes = int(lib.sskd_index_range_search_workspace_bytes(max(n_rows, 0), max(nq, 0), max(max_results, 0)))
    return lib.sskd_index_range_search(
        p if tiled else None, n_rows, p if queries else None, nq, p if thr else None, 0, None,
        p if lims else None, p if outs else None, p if outs else None, max_results, p if ws else None, ws_bytes, None,
    )


@pytest.mark.parametrize(
    "kwargs,code",
    [
        (dict(nq=-1), ERR_INVALID),
        (dict(max_results=-1), ERR_INVALID),
        (dict(n_rows=-5), ERR_INVALID),
        (dict(lims=False), ERR_INVALID),
        (dict(lims=False, nq=0), ERR_INVALID),
        (dict(n_rows=(1 << 31) - 64), ERR_INVALID),
        (dict(n_rows=1 << 33), ERR_INVALID),
        (dict(tiled=False), ERR_INVALID),
        (dict(queries=False), ERR_INVALID),
        (dict(thr=False), ERR_INVALID),
        (dict(outs=False), ERR_INVALID),
        (dict(ws=False), ERR_WORKSPACE),
        (dict(ws_bytes=1), ERR_WORKSPACE),
    ],
)
def test_argument_errors_need_no_gpu(native_lib, kwargs, code):
    rc = _call(native_lib, **kwargs)
    assert rc == code, (kwargs, rc, native_lib.sskd_last_error())
    assert b"index_range_search" in native_lib.sskd_last_error()


def test_range_thresholds_broadcast():
    assert range_thresholds(0.5, 3).tolist() == [0.5, 0.5, 0.5]
    assert range_thresholds(np.float64(0.25), 2).dtype == np.float32
    assert range_thresholds([0.1], 4).shape == (4,)
    t = range_thresholds(np.array([0.1, -np.inf, np.nan]), 3)
    assert t.dtype == np.float32 and t[0] == np.float32(0.1) and np.isneginf(t[1]) and np.isnan(t[2])
    assert range_thresholds(np.zeros((2, 1)), 2).shape == (2,)
    with pytest.raises(ValueError):
        range_thresholds([0.1, 0.2], 3)


def test_pairs_from_ranges_keeps_upper_triangle_of_live_queries():
    # queries are ids 10, 11, 12, 13; query 12 is removed
    lims = np.array([0, 3, 5, 7, 9])
    ids = np.array([10, 12, 11,    11, 13,    10, 13,    13, 12])
    scores = np.array([1.0, 0.9, 0.8,   1.0, 0.7,   0.95, 0.6,   1.0, 0.6], np.float32)
    pairs, s = pairs_from_ranges(lims, scores, ids, np.arange(10, 14), np.array([True, True, False, True]))
    assert pairs.tolist() == [[10, 12], [10, 11], [11, 13]]
    assert s.tolist() == pytest.approx([0.9, 0.8, 0.7])
    assert pairs.dtype == np.int64 and s.dtype == np.float32
    empty_p, empty_s = pairs_from_ranges(np.zeros(3, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64),
                                         np.arange(2), np.ones(2, bool))
    assert empty_p.shape == (0, 2) and empty_s.shape == (0,)
