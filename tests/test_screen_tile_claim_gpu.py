"""The screening kernel's claimed tiles: every tile of a query block is screened exactly once, whoever takes it.

In the slice phase a wave takes chunks of 8 consecutive tiles: chunk ``w < 12`` of a slice is wave ``w``'s of the
slice's own workgroup, every further chunk goes to whoever draws it from the slice's cursor, and a wave whose slice is
exhausted draws from the sibling slices of its query block.  The planner claims only where slices are long and query
blocks many (``sskd_index_search_screened_plan_claims`` says which; other launches deal tile ``w + 12 i`` to wave ``w``).
EVERY case here runs claimed: where the plan claims, through ``sskd_index_search_screened`` itself (and the plan's
choice is asserted from the library); where it deals, through the test hook ``sskd_index_search_screened_claim`` with
claiming forced - the small geometries are where the edges of the scheme lie.  Geometry asserted through
``sskd_index_search_screened_plan``:

  (127, 2 049)          64 per block, LIGHT      6 slices x 11 tiles: two chunks (8 + 3 tiles) for twelve waves - ten
                                                 waves of every workgroup start with a draw; last slice 10 tiles   forced
  (383, 4 099)         128 per block, LIGHT      11 x 12, last slice 9: chunks cut by the slice end                forced
  (16 479, 32 771)     160 per block, LIGHT      2 x 513: 65 chunks, the last of ONE tile; siblings                plan
  (32 799, 127 001)    160 per block, non-LIGHT  1 x 3 969: 497 chunks, the last of one tile; no sibling           plan
  (20 000, 254 017)    160 per block, non-LIGHT  125 blocks x 2 slices of 3 970 (last 3 969): the bench kernel     plan
  (256, 6 007) + mask  128 per block, LIGHT, MASKED, 16 x 12: the mask word follows the claimed tile               forced
  (16 479, 32 771) + mask   160 per block, LIGHT, MASKED, 2 x 513                                                  plan

Every case demands the scores and ids of the exact scan (``sskd_index_search``, oracle-pinned elsewhere) bit for bit on
seeded unit rows.  A tile nobody takes loses the rows it holds; a tile taken twice appends its rows twice and shows as
a duplicated id.  So that neither can hide behind rows that would not have made the top k anyway, the two-slice LIGHT
case and the one-slice case plant one self-match per tile: query ``i < n_tiles`` is a copy of corpus row
``32 i + (i mod 32)`` and must return that row first.  Those two cases also run twice on ONE workspace: the cursors are
re-zeroed by the call itself, or the second call would find every slice exhausted past its first twelve chunks.
"""
import ctypes

import numpy as np
import pytest
import torch

from capi_helpers import stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import _native

pytestmark = pytest.mark.gpu

DIM, K = 384, 10
WAVES, CLAIM_TILES = 12, 8
LIGHT_MAX_TILES_PER_SLICE = 330 * WAVES
BASE_ROWS = 254_017

_base = {}


def base_corpus():
    """One seeded corpus for every case (a case uses its first n rows); never modified."""
    if "c" not in _base:
        c = oracle.seeded_unit_rows(BASE_ROWS, DIM, 6061)
        c.setflags(write=False)
        _base["c"] = c
    return _base["c"]


def plan(lib, n, nq):
    qpb, passes, slices = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _native.check(lib.sskd_index_search_screened_plan(n, nq, K, ctypes.byref(qpb), ctypes.byref(passes), ctypes.byref(slices)))
    tiles_per_slice = -(-(-(-n // 32)) // slices.value)
    return qpb.value, passes.value, slices.value, tiles_per_slice


def queries_for(corpus, nq, seed, planted):
    """seeded unit queries; with ``planted``, query i < n_tiles is a copy of row 32 i + (i mod 32) - one per tile"""
    q = oracle.seeded_unit_rows(nq, DIM, seed)
    rows = None
    if planted:
        n = corpus.shape[0]
        n_tiles = -(-n // 32)
        assert nq >= n_tiles
        i = np.arange(n_tiles)
        rows = np.minimum(32 * i + i % 32, n - 1)   # (the ragged last tile: its last row)
        q[:n_tiles] = corpus[rows]
    return q, rows


class Searches:
    """the screened search and the exact scan over one device copy of (corpus, queries, mask)"""

    def __init__(self, lib, corpus, queries, allowed=None, force_claim=False):
        self.lib, self.n, self.nq, self.force_claim = lib, corpus.shape[0], queries.shape[0], force_claim
        self.tiled = tile_corpus(lib, np.array(corpus))
        self.bf = torch.empty(int(lib.sskd_index_bf16_bytes(self.n)), dtype=torch.uint8, device="cuda")
        _native.check(lib.sskd_index_make_bf16(self.tiled.data_ptr(), self.n, self.bf.data_ptr(), stream()))
        self.q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
        self.mask = None
        if allowed is not None:
            flags = torch.from_numpy(allowed.astype(np.uint8)).cuda()
            self.mask = torch.empty(int(lib.sskd_row_mask_words(self.n)), dtype=torch.int32, device="cuda")
            _native.check(lib.sskd_row_mask_pack(flags.data_ptr(), self.n, self.mask.data_ptr(), stream()))
        need = int(lib.sskd_index_search_screened_workspace_bytes(self.n, self.nq, K))
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")   # ONE workspace for every screened call

    def _out(self):
        return (torch.full((self.nq, K), float("nan"), device="cuda"),
                torch.full((self.nq, K), -7, dtype=torch.int64, device="cuda"))

    def screened(self):
        out_s, out_i = self._out()
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        head = (self.tiled.data_ptr(), self.bf.data_ptr(), self.n, self.q.data_ptr(), self.nq, K, 0)
        tail = (out_s.data_ptr(), out_i.data_ptr(), status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream(), None, None)
        mask = None if self.mask is None else self.mask.data_ptr()
        if self.force_claim:
            _native.check(self.lib.sskd_index_search_screened_claim(*head, mask, 1, *tail))
        elif mask is None:
            _native.check(self.lib.sskd_index_search_screened(*head, *tail))
        else:
            _native.check(self.lib.sskd_index_search_screened_filtered(*head, mask, *tail))
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        assert st[0] == 0, st
        return out_s.cpu().numpy(), out_i.cpu().numpy()

    def exact(self):
        out_s, out_i = self._out()
        ws = torch.empty(int(self.lib.sskd_index_search_workspace_bytes(self.n, self.nq, K)), dtype=torch.uint8, device="cuda")
        head = (self.tiled.data_ptr(), self.n, self.q.data_ptr(), self.nq, K, 0)
        tail = (out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), stream())
        if self.mask is None:
            _native.check(self.lib.sskd_index_search(*head, *tail))
        else:
            _native.check(self.lib.sskd_index_search_filtered(*head, self.mask.data_ptr(), *tail, None, None, None))
        torch.cuda.synchronize()
        return out_s.cpu().numpy(), out_i.cpu().numpy()


def check_geometry(lib, n, nq, qpb, slices, tps, light, claimed):
    """the geometry named, and whether the PLAN claims (read from the library); returns (plan, force): claiming is
    forced through the test hook exactly where the plan would deal"""
    got = plan(lib, n, nq)
    assert (got[0], got[2], got[3]) == (qpb, slices, tps), got
    assert (tps <= LIGHT_MAX_TILES_PER_SLICE) == light
    claims = ctypes.c_int(-1)
    _native.check(lib.sskd_index_search_screened_plan_claims(n, nq, K, ctypes.byref(claims)))
    assert claims.value == int(claimed), claims.value
    return got, not claimed


def assert_same(got, want):
    assert np.array_equal(got[1], want[1]), np.argwhere(got[1] != want[1])[:5]
    assert np.array_equal(got[0], want[0])
    # a tile screened twice would hand the finalize kernel the same row twice
    srt = np.sort(got[1], axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()


# (nq, n_rows, queries per block, LIGHT, slices, tiles per slice, claimed by the plan, one self-match per tile + second call)
FORMS = [
    (127, 2_049, 64, True, 6, 11, False, False),
    (383, 4_099, 128, True, 11, 12, False, False),
    (16_479, 32_771, 160, True, 2, 513, True, True),
    (32_799, 127_001, 160, False, 1, 3_969, True, True),
    (20_000, 254_017, 160, False, 2, 3_970, True, False),
]


@pytest.mark.parametrize("nq,n,qpb,light,slices,tps,claimed,planted", FORMS)
def test_every_tile_is_screened_once(gpu, native_lib, nq, n, qpb, light, slices, tps, claimed, planted):
    got, force = check_geometry(native_lib, n, nq, qpb, slices, tps, light, claimed)
    if not claimed:
        assert tps < 2 * CLAIM_TILES * WAVES and tps % CLAIM_TILES != 0   # waves without a chunk of their own; a cut chunk
    if n == 254_017:
        assert got[1] == 125    # the bench kernel (160 queries, non-LIGHT) with a sibling slice to draw from
    if planted:
        assert tps % CLAIM_TILES == 1   # a last chunk of ONE tile: its successor is drawn and read on the spot
    corpus = base_corpus()[:n]
    queries, rows = queries_for(corpus, nq, 3000 + nq, planted)
    run = Searches(native_lib, corpus, queries, force_claim=force)
    first = run.screened()
    want = run.exact()
    assert_same(first, want)
    if planted:
        wrong = np.flatnonzero(first[1][: rows.size, 0] != rows)
        assert wrong.size == 0, wrong[:8]            # (the query's number is the tile that was skipped)
        again = run.screened()                       # same workspace: the call zeroes its own cursors
        assert np.array_equal(again[1], first[1]) and np.array_equal(again[0], first[0])


@pytest.mark.parametrize("nq,n,qpb,slices,tps,claimed", [(256, 6_007, 128, 16, 12, False), (16_479, 32_771, 160, 2, 513, True)])
def test_mask_word_follows_the_tile(gpu, native_lib, nq, n, qpb, slices, tps, claimed):
    """MASKED kernels: the allow-mask word is fetched per tile index, so it must be the word of the tile the wave
    actually took.  Every third row is masked, and with it the self-match of every query planted on such a row."""
    _, force = check_geometry(native_lib, n, nq, qpb, slices, tps, True, claimed)
    corpus = base_corpus()[:n]
    queries = oracle.seeded_unit_rows(nq, DIM, 4000 + nq)
    planted = (np.arange(nq, dtype=np.int64) * 23) % n
    queries[:] = corpus[planted] + np.float32(0.02) * queries
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    allowed = np.ones(n, bool)
    allowed[::3] = False
    run = Searches(native_lib, corpus, queries, allowed, force_claim=force)
    got, want = run.screened(), run.exact()
    assert_same(got, want)
    assert allowed[got[1]].all()
    kept = allowed[planted]
    assert (got[1][kept, 0] == planted[kept]).all() and not (got[1][~kept] == planted[~kept, None]).any()
