"""The screening kernel on v_mfma_f32_16x16x32_bf16: operand maps, the 32-entry runs of a 16-lane group, fp16 bounds.

The kernel multiplies 16-row blocks of a corpus tile (A) with 16-query blocks (B); lane ``l`` of a wave owns query
``l & 15`` of every query block and rows ``4 (l >> 4) + 0..3`` of every row block, appends to a run of 32 entries per
(query, slice, wave, 16-lane group), and keeps its pruning bounds as fp16 pairs rounded toward -inf.

* ``test_operand_maps``: the raw screen scores (``sskd_index_screen_scores``: the kernel's own staging, tile ring and MFMA
  loop) of 70 rows - two full tiles and a ragged one of 6 rows - against fp64 dot products of the values the sidecar
  holds.  Row ``r`` is a one-hot at column ``r mod 384`` over small seeded steps, query ``c`` weighs the 8-column group ``c``:
  a lane reading another row, another column group or another position inside a group changes a score by far more than
  the bound, which is the fp32 accumulation of 384 exact products, 384 x 2^-24 x sum |product|.  Equality is not
  asserted: the sidecar holds the rows minus their mean row, rounded to bf16, so the operands are not the small dyadic
  numbers of the corpus and the order in which the MFMA adds 32 products is not documented; the reference is fp64 over
  the decoded sidecar, and the test itself asserts that any two rows, and any two queries, differ by more than 100
  bounds in some score.
* ``test_full_path``: the whole search against the exact scan, bit for bit, tiles claimed and dealt, plain and with a
  mask that clears whole 16-row blocks, whole tiles and single rows.  2 080 rows x 200 queries is the 64-query kernel
  with a last block of 8 queries; the other shapes (the library's plan is asserted) reach the 128-query kernel with a
  last block of 40 and the 160-query kernel with one of 65, both with a ragged last tile.
* ``test_ascending_rows_fill_the_runs``: 4 096 rows in ascending order of their score for query 0, so that the bound
  trails the rows and every row passes it when it arrives: a 16-lane group sees 4 rows of each tile of its wave, its run
  of 32 fills, and the answer must still be the exact scan's - by compaction or by the in-call exact fallback.
* ``test_threshold_pack_rounds_down``: ``sskd_screen_threshold_roundtrip`` against the specification restated with
  numpy's float16: the largest fp16 at or below x; -inf below -65504, 65504 above 65504, denormals kept.
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


def _sidecar(lib, corpus):
    n = corpus.shape[0]
    tiled = tile_corpus(lib, np.array(corpus))
    bf = torch.empty(int(lib.sskd_index_bf16_bytes(n)), dtype=torch.uint8, device="cuda")
    _native.check(lib.sskd_index_make_bf16(tiled.data_ptr(), n, bf.data_ptr(), stream()))
    return tiled, bf


def test_operand_maps(gpu, native_lib):
    lib = native_lib
    n, nq = 70, 48
    rng = np.random.default_rng(70)
    r = np.arange(n)
    corpus = (rng.integers(0, 8, (n, DIM)) / 64.0).astype(np.float32)                 # small seeded steps of 1 / 64
    corpus[r, r % DIM] += 1.0                                                         # the one-hot
    queries = (rng.integers(0, 5, (nq, DIM)) / 64.0).astype(np.float32)
    for q in range(nq):
        queries[q, 8 * q: 8 * q + 8] = 1.0 + np.arange(8) / 8.0                       # column group q, every position its own weight
    assert np.array_equal(oracle.bf16_round(queries), queries)
    tiled, bf = _sidecar(lib, corpus)
    dq = torch.from_numpy(queries).cuda()
    padded = -(-n // 32) * 32
    out = torch.full((padded, 64), float("nan"), device="cuda")
    _native.check(lib.sskd_index_screen_scores(bf.data_ptr(), n, dq.data_ptr(), nq, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    side = oracle.sidecar_decode(bf.cpu().numpy(), n)                                 # what the device multiplies: c~, exactly
    ct, q64 = side.tiles.astype(np.float64), queries.astype(np.float64)
    want = ct @ q64.T
    bound = 384 * 2.0 ** -24 * (np.abs(ct) @ np.abs(q64).T)
    err = np.abs(got[:, :nq] - want)
    print("operand maps: max error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), np.argwhere(err > bound)[:8]
    assert not got[n:].any() and not got[:, nq:].any()                                # padding rows, padding queries
    # the case can tell the maps apart: rows, and queries, differ from each other by far more than the bound
    assert np.abs(want[:n, None, :] - want[None, :n, :]).max(2)[~np.eye(n, dtype=bool)].min() > 100 * bound.max()
    assert np.abs(want[:n, :, None] - want[:n, None, :]).max(0)[~np.eye(nq, dtype=bool)].min() > 100 * bound.max()


class _Run:
    def __init__(self, lib, corpus, queries, allowed=None):
        self.lib, self.n, self.nq = lib, corpus.shape[0], queries.shape[0]
        self.tiled, self.bf = _sidecar(lib, corpus)
        self.q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
        self.mask = None
        if allowed is not None:
            flags = torch.from_numpy(allowed.astype(np.uint8)).cuda()
            self.mask = torch.empty(int(lib.sskd_row_mask_words(self.n)), dtype=torch.int32, device="cuda")
            _native.check(lib.sskd_row_mask_pack(flags.data_ptr(), self.n, self.mask.data_ptr(), stream()))
        need = int(lib.sskd_index_search_screened_workspace_bytes(self.n, self.nq, K))
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def _out(self):
        return (torch.full((self.nq, K), float("nan"), device="cuda"),
                torch.full((self.nq, K), -7, dtype=torch.int64, device="cuda"))

    def screened(self, claim):
        out_s, out_i = self._out()
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        _native.check(self.lib.sskd_index_search_screened_claim(
            self.tiled.data_ptr(), self.bf.data_ptr(), self.n, self.q.data_ptr(), self.nq, K, 0,
            None if self.mask is None else self.mask.data_ptr(), claim, out_s.data_ptr(), out_i.data_ptr(),
            status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream(), None, None))
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        assert st[0] == 0, st
        return out_s.cpu().numpy(), out_i.cpu().numpy(), int(st[1])

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


def _queries_per_block(lib, n, nq):
    qpb, passes, slices = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _native.check(lib.sskd_index_search_screened_plan(n, nq, K, ctypes.byref(qpb), ctypes.byref(passes), ctypes.byref(slices)))
    return qpb.value


_data = {}


def _corpus_and_queries(n, nq):
    """seeded unit rows (one corpus for every shape: its first n rows); every fifth query sits next to a corpus row"""
    if "c" not in _data:
        c = oracle.seeded_unit_rows(16_403, DIM, 1632)
        c.setflags(write=False)
        _data["c"] = c
    corpus = _data["c"][:n]
    q = oracle.seeded_unit_rows(nq, DIM, 1600 + nq)
    near = np.arange(0, nq, 5)
    q[near] = corpus[(near * 37) % n] + np.float32(0.05) * q[near]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return corpus, q


def _block_mask(n):
    """clears whole 16-row blocks (both halves of a tile, in different tiles), a whole tile, and single rows"""
    allowed = np.ones(n, bool)
    allowed[32 * 3: 32 * 3 + 16] = False
    allowed[32 * 7 + 16: 32 * 8] = False
    allowed[32 * 11: 32 * 12] = False
    allowed[-5:] = False                       # the end of the last tile
    allowed[np.arange(1, n, 29)] = False
    return allowed


# (rows, queries, queries per block): the issue's shape; 128 per block, last block 40, ragged; 160 per block, last 65, ragged
FULL = [(2_080, 200, 64), (2_093, 296, 128), (16_403, 16_385, 160)]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("n,nq,qpb", FULL)
def test_full_path(gpu, native_lib, n, nq, qpb, masked):
    assert _queries_per_block(native_lib, n, nq) == qpb
    assert nq % qpb != 0
    corpus, queries = _corpus_and_queries(n, nq)
    allowed = _block_mask(n) if masked else None
    run = _Run(native_lib, corpus, queries, allowed)
    want = run.exact()
    for claim in (0, 1):
        got_s, got_i, fallback = run.screened(claim)
        print(f"rows {n} queries {nq} claim {claim} masked {masked}: exact_fallback_queries {fallback}")
        assert np.array_equal(got_i, want[1]), np.argwhere(got_i != want[1])[:5]
        assert np.array_equal(got_s, want[0])
        if masked:
            assert allowed[got_i].all()


def test_ascending_rows_fill_the_runs(gpu, native_lib):
    n, nq = 4_096, 64
    corpus, queries = _corpus_and_queries(n, nq)
    q0 = queries[0].astype(np.float64)
    order = np.argsort(corpus.astype(np.float64) @ q0, kind="stable")
    corpus = np.ascontiguousarray(corpus[order])
    run = _Run(native_lib, corpus, queries)
    want = run.exact()
    assert want[1][0, 0] == n - 1                      # the best row of the planted query arrives last
    for claim in (0, 1):
        got_s, got_i, fallback = run.screened(claim)
        print(f"ascending rows, claim {claim}: exact_fallback_queries {fallback}")
        assert np.array_equal(got_i, want[1]) and np.array_equal(got_s, want[0])


def _floor_fp16(x):
    """the specification: the largest fp16 value <= x, widened to fp32 (-inf below the fp16 range)"""
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)                       # to nearest: may land above x, or on +-inf
    above = h.astype(np.float32) > x
    with np.errstate(over="ignore"):                   # (-65504 steps down to -inf)
        h[above] = np.nextafter(h[above], np.float16(-np.inf))
    return h.astype(np.float32)


def test_threshold_pack_rounds_down(gpu, native_lib):
    rng = np.random.default_rng(1616)
    m = 10_000
    # what the kernel sees: screen scores minus a band, any sign, from far below the fp16 denormals (2^-24) to far above 65504
    x = (rng.choice([-1.0, 1.0], m) * rng.uniform(1.0, 2.0, m) * 2.0 ** rng.integers(-40, 40, m)).astype(np.float32)
    f16 = rng.integers(0, 1 << 16, 2_000).astype(np.uint16).view(np.float16)
    f16 = f16[np.isfinite(f16)].astype(np.float32)     # exact fp16 values, denormals among them: they stay
    special = np.array([0.0, -0.0, 65504.0, -65504.0, 65519.996, -65519.996, 65520.0, -65520.0, 1e30, -1e30, 3.4028235e38,
                        -3.4028235e38, np.inf, -np.inf, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 1e-8, -1e-8,
                        1e-30, -1e-30, 6.1e-5, -6.1e-5, 6.0975e-5, -6.0975e-5], np.float32)
    x = np.concatenate([x, f16, np.nextafter(f16, np.float32(np.inf)), np.nextafter(f16, np.float32(-np.inf)), special])
    dx = torch.from_numpy(x).cuda()
    out = torch.full_like(dx, float("nan"))
    _native.check(native_lib.sskd_screen_threshold_roundtrip(dx.data_ptr(), x.size, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = _floor_fp16(x)
    assert (want <= x).all()
    assert (got <= x).all(), x[~(got <= x)][:8]                                        # never upward, NaN included
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (x[got != want][:8], got[got != want][:8])
    assert (got[x < -65504.0] == -np.inf).all() and (got[(x > 65504.0) & np.isfinite(x)] == 65504.0).all()
    den = (np.abs(want) < 2.0 ** -14) & (want != 0)
    assert den.sum() > 100                                                             # denormal fp16 results were exercised
