"""The screening kernel's rolled append body: one take mask per query pair, one loop over its bits.

Behind the MFMAs of a tile a lane holds, per pair ``pr`` of 16-query blocks, the scores of two queries (block positions
``32 pr + n`` and ``32 pr + 16 + n``, ``n = lane & 15``; ``e = 0, 1``) against the eight tile rows of its lane group
``g = lane >> 4`` (rows ``4 g + i`` and ``16 + 4 g + i``, ``i < 4``; ``r = 0..7``).  Bit ``8 e + r`` of the pair's mask
says that row ``r`` reached query ``e``'s bound.  The kernels that offer every appended row to the pools (long slices)
append and offer the rows of both queries in ONE loop over the set bits; the LIGHT kernels (short slices) walk the
sixteen rows unrolled.  What can go wrong is a wrong value, row id, query or run picked for a bit, a bit lost or
walked twice, and the count of a run that crosses its capacity in the middle of the walk.  So the cases plant rows for
chosen ``(pr, g, n)`` and chosen bits into seeded unit rows (a random row scores about 0.05, a planted one above 0.98),
and run them through every instantiation:

* full mask: all eight rows of a lane group are near-copies of BOTH queries of a lane, with distinct descending
  perturbations - sixteen bits, all eight rows in both top tens, in a decided order; for every pair of the block size
  and every lane group, once in a tile that is some wave's first (``tiles_done == 0``: one pool offer per query) and,
  where a wave has more than one tile, once in a later one (an offer per row in the long-slice form);
* sparse masks: only ``r = 7`` of ``e = 1`` (the last bit), only ``r = 0`` of ``e = 0`` (the first), one row each in
  both queries;
* ragged end: every shape has ``n_rows % 32 != 0``; the last real row, next to the padding rows of its tile, is planted.
  No padding row (-inf) is returned and every id stays below ``n_rows``;
* row mask: the MASKED kernels with every other planted row masked off;
* the cap crossed inside the walk: 40 (and 36) equal rows in five tiles of ONE wave and ONE lane group, with tiles
  dealt (the unrolled walk) and with tiles claimed on one long slice (the rolled loop).

Geometries are those of ``tests/test_screen_tile_claim_gpu.py`` (asserted from the library's plan), so that every
instantiation of the kernel runs them; the two small ones run with tiles claimed and dealt.  Planted queries and a
stride of the others are held to ``oracle.topk_fma`` bit for bit; every query besides to the exact scan of the library
(held to the same oracle elsewhere).  No tolerance anywhere.
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
WAVES, CLAIM_TILES, CAP = 12, 8, 32
LIGHT_MAX_TILES_PER_SLICE = 330 * WAVES
BASE_ROWS = 254_017

_base = {}


def base_corpus():
    """One seeded corpus for every case (a case plants into a copy of its first n rows); never modified."""
    if "c" not in _base:
        c = oracle.seeded_unit_rows(BASE_ROWS, DIM, 7171)
        c.setflags(write=False)
        _base["c"] = c
    return _base["c"]


def plan(lib, n, nq):
    qpb, passes, slices, claims = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(-1)
    _native.check(lib.sskd_index_search_screened_plan(n, nq, K, ctypes.byref(qpb), ctypes.byref(passes), ctypes.byref(slices)))
    _native.check(lib.sskd_index_search_screened_plan_claims(n, nq, K, ctypes.byref(claims)))
    n_tiles = -(-n // 32)
    return qpb.value, slices.value, -(-n_tiles // slices.value), bool(claims.value)


def unit(v):
    return (v / np.linalg.norm(v)).astype(np.float32)


class Plants:
    """rows and queries planted into one corpus: which tile a pair's plants go to, which lanes are still free"""

    def __init__(self, corpus, queries, qpb, slices, tps, claimed, seed):
        self.c, self.q, self.qb = corpus, queries, qpb // 32
        self.rng = np.random.default_rng(seed)
        self.free = [list(range(16)) for _ in range(self.qb)]
        self.full, self.single = [], []   # (query, the rows it must return) / (query, its best row)
        n_tiles = -(-corpus.shape[0] // 32)
        # tiles whose place in their wave's order is known: a wave's first tile, or a later one.  Dealt: wave w takes
        # t_begin + w + 12 i.  Claimed: chunk w < 12 of 8 tiles is wave w's own (further chunks go to whoever draws them).
        self.first, self.later = [], []
        for s in range(slices):
            t_begin, t_end = s * tps, min((s + 1) * tps, n_tiles - 1)   # (the ragged last tile has a plant of its own)
            for j in range(t_end - t_begin):
                if claimed and j >= WAVES * CLAIM_TILES:
                    break
                is_first = j % CLAIM_TILES == 0 if claimed else j < WAVES
                (self.first if is_first else self.later).append(t_begin + j)
        # (spread over the slices and waves instead of the first ones found)
        self.first = self.first[:: max(1, len(self.first) // (2 * self.qb))]
        self.later = self.later[:: max(1, len(self.later) // (2 * self.qb))]

    def lane(self, pr):
        return self.free[pr].pop(0)

    def vec(self):
        return unit(self.rng.standard_normal(DIM))

    def plant_full(self, tile, pr):
        for g in range(4):
            n, u = self.lane(pr), self.vec()
            qa, qb = 32 * pr + n, 32 * pr + 16 + n
            self.q[qa] = u
            self.q[qb] = unit(u + np.float32(0.01) * self.vec())
            rows = [32 * tile + 16 * (r >> 2) + 4 * g + (r & 3) for r in range(8)]
            for r, row in enumerate(rows):
                self.c[row] = unit(u + np.float32(0.02 * (r + 1)) * self.vec())
            self.full += [(qa, rows), (qb, rows)]

    def plant_bits(self, tile, pr, g, bits):
        """one row per (e, r) of ``bits``, each next to its own query of one lane"""
        n = self.lane(pr)
        for e, r in bits:
            u, row = self.vec(), 32 * tile + 16 * (r >> 2) + 4 * g + (r & 3)
            self.q[32 * pr + 16 * e + n] = u
            self.c[row] = unit(u + np.float32(0.02) * self.vec())
            self.single.append((32 * pr + 16 * e + n, row))

    def plant_last_row(self):
        row, u = self.c.shape[0] - 1, self.vec()
        qi = 32 * 0 + 16 * 1 + self.lane(0)
        self.q[qi] = u
        self.c[row] = unit(u + np.float32(0.02) * self.vec())
        self.single.append((qi, row))

    def queries(self):
        return sorted({q for q, _ in self.full} | {q for q, _ in self.single})


def planted_case(n, nq, qpb, slices, tps, claimed, seed):
    corpus = np.array(base_corpus()[:n])
    queries = oracle.seeded_unit_rows(nq, DIM, seed)
    pl = Plants(corpus, queries, qpb, slices, tps, claimed, seed + 1)
    qb = qpb // 32
    assert len(pl.first) >= 2 * qb
    sparse_tiles = pl.later[qb: 2 * qb] if len(pl.later) >= 2 * qb else pl.first[qb: 2 * qb]
    for pr in range(qb):
        pl.plant_full(pl.first[pr], pr)
        if len(pl.later) >= qb:
            pl.plant_full(pl.later[pr], pr)
        t = sparse_tiles[pr]
        pl.plant_bits(t, pr, (pr + 0) % 4, [(1, 7)])
        pl.plant_bits(t, pr, (pr + 1) % 4, [(0, 0)])
        pl.plant_bits(t, pr, (pr + 2) % 4, [(0, 5), (1, 2)])
    pl.plant_last_row()
    return corpus, queries, pl


class Run:
    """the screened search (tiles claimed or dealt) and the exact scan over one device copy of (corpus, queries, mask)"""

    def __init__(self, lib, corpus, queries, allowed=None):
        self.lib, self.n, self.nq = lib, corpus.shape[0], queries.shape[0]
        self.tiled = tile_corpus(lib, corpus)
        self.bf = torch.empty(int(lib.sskd_index_bf16_bytes(self.n)), dtype=torch.uint8, device="cuda")
        _native.check(lib.sskd_index_make_bf16(self.tiled.data_ptr(), self.n, self.bf.data_ptr(), stream()))
        self.q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
        self.mask = None
        if allowed is not None:
            flags = torch.from_numpy(allowed.astype(np.uint8)).cuda()
            self.mask = torch.empty(int(lib.sskd_row_mask_words(self.n)), dtype=torch.int32, device="cuda")
            _native.check(lib.sskd_row_mask_pack(flags.data_ptr(), self.n, self.mask.data_ptr(), stream()))

    def _out(self):
        return (torch.full((self.nq, K), float("nan"), device="cuda"),
                torch.full((self.nq, K), -7, dtype=torch.int64, device="cuda"))

    def screened(self, claim):
        out_s, out_i = self._out()
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(self.lib.sskd_index_search_screened_workspace_bytes(self.n, self.nq, K)), dtype=torch.uint8, device="cuda")
        assert ws.numel() > 0
        _native.check(self.lib.sskd_index_search_screened_claim(
            self.tiled.data_ptr(), self.bf.data_ptr(), self.n, self.q.data_ptr(), self.nq, K, 0,
            None if self.mask is None else self.mask.data_ptr(), int(claim), out_s.data_ptr(), out_i.data_ptr(),
            status.data_ptr(), ws.data_ptr(), ws.numel(), stream(), None, None))
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


def oracle_rows(queries, corpus, allowed=None):
    """``oracle.topk_fma`` over the allowed rows (their order kept, so ties still go to the lower id)"""
    if allowed is None:
        return oracle.topk_fma(queries, corpus, K)
    keep = np.flatnonzero(allowed)
    s, i = oracle.topk_fma(queries, corpus[keep], K)
    return s, keep[i]


def check(run, claim, corpus, queries, pl, allowed=None):
    """the screened result against the oracle (planted queries + a stride) and the exact scan (every query)"""
    n, nq = corpus.shape[0], queries.shape[0]
    got_s, got_i, fallback = run.screened(claim)
    sel = sorted(set(pl.queries()) | set(range(0, nq, max(1, nq // 16))))
    ref_s, ref_i = oracle_rows(queries[sel], corpus, allowed)
    assert np.array_equal(got_i[sel], ref_i), [sel[j] for j in np.flatnonzero((got_i[sel] != ref_i).any(1))[:8]]
    assert np.array_equal(got_s[sel], ref_s)
    want = run.exact()
    assert np.array_equal(got_i, want[1]), np.argwhere(got_i != want[1])[:5]
    assert np.array_equal(got_s, want[0])
    assert np.isfinite(got_s).all() and (got_i >= 0).all() and (got_i < n).all()      # no padding row, no id past the end
    srt = np.sort(got_i, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                                          # no bit walked twice
    return got_i, fallback


# (nq, n_rows, queries per block, LIGHT, slices, tiles per slice, claimed by the plan)
FORMS = [
    (127, 2_049, 64, True, 6, 11, False),
    (383, 4_099, 128, True, 11, 12, False),
    (16_479, 32_771, 160, True, 2, 513, True),
    (32_799, 127_001, 160, False, 1, 3_969, True),
    (20_000, 254_017, 160, False, 2, 3_970, True),
]
CASES = [(*f, claim) for f in FORMS for claim in ((1,) if f[6] else (1, 0))]


@pytest.mark.parametrize("nq,n,qpb,light,slices,tps,claimed,claim", CASES)
def test_planted_masks(gpu, native_lib, nq, n, qpb, light, slices, tps, claimed, claim):
    """full masks (first and later tiles), sparse masks and the ragged end, in one search per geometry and tile order"""
    assert plan(native_lib, n, nq) == (qpb, slices, tps, claimed)
    assert (tps <= LIGHT_MAX_TILES_PER_SLICE) == light and n % 32 != 0
    corpus, queries, pl = planted_case(n, nq, qpb, slices, tps, bool(claim), 5000 + nq)
    # a later tile exists wherever a wave has more than one: everywhere but the two small geometries with tiles dealt
    assert (len(pl.full) == 16 * (qpb // 32)) == bool(claim or tps > WAVES)
    got_i, fallback = check(Run(native_lib, corpus, queries), claim, corpus, queries, pl)
    print(f"rows {n} queries {nq} claim {claim}: {len(pl.full)} full-mask queries, {len(pl.single)} single rows, exact_fallback_queries {fallback}")
    for q, rows in pl.full:
        assert list(got_i[q, :8]) == rows, (q, got_i[q], rows)       # all eight, in the order of their perturbations
    for q, row in pl.single:
        assert got_i[q, 0] == row, (q, got_i[q], row)


@pytest.mark.parametrize("nq,n,qpb,slices,tps,claimed", [(256, 6_007, 128, 16, 12, False), (16_479, 32_771, 160, 2, 513, True)])
def test_planted_masks_with_row_mask(gpu, native_lib, nq, n, qpb, slices, tps, claimed):
    """the MASKED kernels: every other planted row (odd r of a full mask, every second single row) is masked off"""
    assert plan(native_lib, n, nq) == (qpb, slices, tps, claimed)
    corpus, queries, pl = planted_case(n, nq, qpb, slices, tps, claimed, 6000 + nq)
    allowed = np.ones(n, bool)
    allowed[::7] = False
    for _, rows in pl.full:
        allowed[rows[0::2]] = True
        allowed[rows[1::2]] = False
    singles = [row for _, row in pl.single]
    allowed[singles[0::2]] = True
    allowed[singles[1::2]] = False
    got_i, fallback = check(Run(native_lib, corpus, queries, allowed), int(claimed), corpus, queries, pl, allowed)
    print(f"rows {n} queries {nq} masked: exact_fallback_queries {fallback}")
    assert allowed[got_i].all()
    for q, rows in pl.full:
        assert list(got_i[q, :4]) == rows[0::2], (q, got_i[q], rows)
        assert not np.isin(rows[1::2], got_i[q]).any()
    for j, (q, row) in enumerate(pl.single):
        assert (got_i[q, 0] == row) == (j % 2 == 0) and (j % 2 == 0 or row not in got_i[q])


@pytest.mark.parametrize("n,nq,claim", [(65_536, 1_024, 0), (127_001, 32_799, 1)], ids=["dealt-unrolled", "claimed-rolled"])
def test_cap_crossed_inside_the_loop(gpu, native_lib, n, nq, claim):
    """Tiles dealt (128 queries per block, LIGHT: the unrolled walk): wave w of a slice owns tiles t_begin + w + 12 i.
    Tiles claimed (160 per block, one long slice: the rolled loop): chunk w of eight consecutive tiles is wave w's own.
    Query A finds eight copies of its row in lane group 1 of five tiles of wave 3 - 40 equal rows, all inside the band,
    for one run of 32: the count stands at the cap when the fifth tile's walk starts.  Query B finds four in the first
    of five tiles of wave 7 (lane group 2) and eight in the others - 36, the cap crossed after the fourth bit of a walk.
    No compaction can help (equal scores), so both take the exact fallback inside the call and still return the oracle's
    bits: ten copies, lowest ids first."""
    qpb, slices, tps, claimed = plan(native_lib, n, nq)
    assert claimed == bool(claim) and (tps > LIGHT_MAX_TILES_PER_SLICE) == bool(claim)
    assert tps >= WAVES * CLAIM_TILES if claim else tps >= 4 * WAVES + 8, (slices, tps)
    corpus = np.array(base_corpus()[:n])
    queries = oracle.seeded_unit_rows(nq, DIM, 52)
    rng = np.random.default_rng(53)
    planted = []
    for qi, slice_, wave, g, first_rows in ((37, slices // 2, 3, 1, 8), (70, slices - 1, 7, 2, 4)):
        u = unit(rng.standard_normal(DIM))
        rows = []
        for i in range(5):
            t = slice_ * tps + (CLAIM_TILES * wave + i if claim else wave + WAVES * i)
            rows += [32 * t + 16 * (r >> 2) + 4 * g + (r & 3) for r in range(8 if i else first_rows)]
        corpus[rows] = u
        queries[qi] = unit(u + np.float32(0.02) * queries[qi])
        planted.append((qi, sorted(rows)))
        assert len(rows) > CAP and max(rows) < n - 32
    run = Run(native_lib, corpus, queries)
    got_s, got_i, fallback = run.screened(claim)
    print(f"cap crossed inside the walk, rows {n} claim {claim}: exact_fallback_queries {fallback}")
    assert fallback >= len(planted), fallback
    sel = [q for q, _ in planted] + list(range(0, nq, max(64, nq // 16)))
    ref_s, ref_i = oracle.topk_fma(queries[sel], corpus, K)
    assert np.array_equal(got_i[sel], ref_i) and np.array_equal(got_s[sel], ref_s)
    want = run.exact()
    assert np.array_equal(got_i, want[1]) and np.array_equal(got_s, want[0])
    for q, rows in planted:
        assert list(got_i[q]) == rows[:K]
