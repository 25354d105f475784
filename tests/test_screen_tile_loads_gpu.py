"""The screening kernel's tile loads on scalar bases ("Tile loads on scalar bases").

Every corpus tile load of the screening kernel takes its address as a wave-uniform 64-bit scalar base (tile, k-step and,
for the ring's last groups, the signed distance to the wave's NEXT tile) plus a 32-bit lane offset.  A base that is wrong
for one group of k-steps, one row block, or one kind of hop between tiles gives specific rows a wrong screen score: a
planted nearest neighbour in such a tile is then screened out, or the query goes to the exact fallback.  So every test
here demands the oracle's bits (``oracle.topk_fma``) on planted top-1 data, ``status[0] == 0`` and fewer fallback
queries than queries - a run in which every query was rescued by the exact fallback proves nothing and fails.

(a) ``test_every_form``: the shapes of tests/test_screen_readahead_gpu.py::FORMS - 64, 128 and 160 queries per block,
    LIGHT and not, tiles dealt and claimed - each through the plain AND the masked entry point (every seventh row
    disallowed: the masked instantiations are kernels of their own).
(b) ``test_backward_hop_between_slices``: the smallest geometry the plan itself CLAIMS with two slices, found with the
    host-side plan functions: 10 881 queries (86 blocks of 128; a launch claims from 32 blocks up, and 85 blocks are
    still cut into three slices) x 383 tiles (a slice claims from 192 tiles up, and 382 tiles make two slices of 191).
    Slice 0 holds 192 tiles, slice 1 the other 191, the last of them ragged: the waves of slice 1 run out first and
    steal chunks of slice 0, so their next tile lies BEHIND the one in hand and the ring's next-tile offset is negative.
    Planted neighbours sit in the first and last tile of both slices (the ragged final tile among them) and in the
    first and last tile of the chunk that slice 0 hands out last.
(c) ``test_ragged_tile_with_masked_slice_heads``: ``n_rows % 32 != 0`` together with a row mask that clears the first
    two tiles of every slice, at 64 and at 160 queries per block.

Offsets past 2^32 bytes are the business of tests/test_high_rows_gpu.py.
"""
import numpy as np
import pytest

from oracle import search as oracle
from test_screen_fragment_pipeline_gpu import DIM, K, LIGHT_MAX_TILES_PER_SLICE, base_corpus, plan, planted_queries
from test_screen_mfma16_gpu import _Run
from test_screen_readahead_gpu import FORMS
from test_screen_rolled_append_gpu import plan as plan_with_claims

pytestmark = pytest.mark.gpu


def plan_claims(lib, n, nq):
    return plan_with_claims(lib, n, nq)[3]


def _reference(queries, corpus, allowed):
    if allowed is None:
        return oracle.topk_fma(queries, corpus, K)
    scores = oracle.scores_fma(queries, corpus)
    scores[:, ~allowed] = -np.inf
    return oracle.topk_of_scores(scores, K)


def _check(run, claim, nq, rows, sel, ref, allowed, what):
    s, i, fallback = run.screened(claim)        # (asserts status[0] == 0)
    print(f"{what} claim {claim}: exact_fallback_queries {fallback} of {nq}")
    assert fallback < nq, "every query took the exact fallback: the screening kernel proved nothing"
    kept = np.ones(nq, bool) if allowed is None else allowed[rows]
    wrong = np.flatnonzero(kept & (i[:, 0] != rows))
    assert wrong.size == 0, (what, claim, wrong[:8], rows[wrong[:8]] // 32)     # (which tiles)
    assert not (i[~kept] == rows[~kept, None]).any()
    if allowed is not None:
        assert allowed[i].all() and np.isfinite(s).all()
    assert (s[kept, 0] > 0.99).all() and (s[:, 1] < 0.5).all()
    assert np.array_equal(i[sel], ref[1]), (what, claim, np.argwhere(i[sel] != ref[1])[:5])
    assert np.array_equal(s[sel], ref[0]), (what, claim)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("nq,n,qpb,light,slices,tps,claims,step", FORMS)
def test_every_form(gpu, native_lib, nq, n, qpb, light, slices, tps, claims, step, masked):
    assert n % 32 != 0 and nq % qpb != 0     # ragged last tile, padding queries in the last block
    assert plan(native_lib, n, nq) == (qpb, slices, tps)
    assert (tps <= LIGHT_MAX_TILES_PER_SLICE) == light
    corpus = base_corpus()[:n]
    queries, rows = planted_queries(corpus, nq, 1000 + nq)
    allowed = None
    if masked:
        allowed = np.ones(n, bool)
        allowed[3::7] = False
        assert 0 < (~allowed[rows]).sum() < nq // 2      # planted rows on both sides of the mask
    sel = np.arange(0, nq, step)
    if step > 1:   # the padded last block and every sub-block position of one block in full
        sel = np.unique(np.concatenate([sel, np.arange(nq - 1 - (nq - 1) % qpb, nq, 13), np.arange(0, qpb, 17)]))
    ref = _reference(queries[sel], corpus, allowed)
    run = _Run(native_lib, corpus, queries, allowed)
    for claim in claims:
        _check(run, claim, nq, rows, sel, ref, allowed, f"queries {nq} rows {n} masked {masked}")


def _planted_at(corpus, nq, seed, first_rows):
    """planted_queries, with the first queries moved onto the given rows"""
    queries, rows = planted_queries(corpus, nq, seed)
    m = len(first_rows)
    rows[:m] = first_rows
    q = corpus[rows[:m]] + np.float32(0.02) * oracle.seeded_unit_rows(m, DIM, seed + 1)
    queries[:m] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return queries, rows


def test_backward_hop_between_slices(gpu, native_lib):
    nq, n = 10_881, 382 * 32 + 13
    qpb, slices, tps = plan(native_lib, n, nq)
    assert (qpb, slices, tps) == (128, 2, 192) and plan_claims(native_lib, n, nq)
    # the smallest such geometry: one query block fewer is cut into three slices (too short to claim), and with one tile
    # fewer the two slices hold 191 tiles each and are dealt
    assert plan(native_lib, n, nq - 1)[1] == 3 and not plan_claims(native_lib, n, nq - 1)
    assert plan(native_lib, n - 32, nq) == (128, 2, 191) and not plan_claims(native_lib, n - 32, nq)
    n_tiles = -(-n // 32)
    assert n_tiles - tps < tps and n % 32 != 0            # the last slice is the shorter one, and ends ragged
    # first and last tile of either slice, the ragged final tile's last row, and the chunk of 8 tiles that slice 0
    # hands out last (its 24th) - wherever a hop can land or leave
    tiles = [0, tps - 1, tps, n_tiles - 1, tps - 8, tps - 2]
    special = [32 * t + r for t in tiles for r in (0, 17, 31) if 32 * t + r < n] + [n - 1]
    corpus = base_corpus()[:n]
    queries, rows = _planted_at(corpus, nq, 4242, np.array(special))
    sel = np.unique(np.concatenate([np.arange(len(special)), np.arange(0, nq, 97), np.arange(nq - 3, nq)]))
    ref = _reference(queries[sel], corpus, None)
    _check(_Run(native_lib, corpus, queries), -1, nq, rows, sel, ref, None, f"queries {nq} rows {n}, 2 slices")


@pytest.mark.parametrize("nq,n,qpb,slices,tps,step", [(127, 2_049, 64, 6, 11, 1), (16_479, 32_771, 160, 2, 513, 131)])
def test_ragged_tile_with_masked_slice_heads(gpu, native_lib, nq, n, qpb, slices, tps, step):
    assert n % 32 != 0 and plan(native_lib, n, nq) == (qpb, slices, tps)
    corpus = base_corpus()[:n]
    allowed = np.ones(n, bool)
    for sl in range(slices):
        allowed[sl * tps * 32: sl * tps * 32 + 64] = False     # the slice's first two tiles, whole
    heads = np.flatnonzero(~allowed)
    last = np.arange(n - n % 32, n)                            # the ragged tile stays allowed, and is aimed at
    queries, rows = _planted_at(corpus, nq, 9000 + nq, np.concatenate([heads[::29][:8], last]))
    lost = ~allowed[rows]
    assert lost.sum() >= 8 and allowed[rows[8: 8 + last.size]].all()
    sel = np.unique(np.concatenate([np.arange(8 + last.size), np.arange(0, nq, step)]))
    ref = _reference(queries[sel], corpus, allowed)
    _check(_Run(native_lib, corpus, queries, allowed), -1, nq, rows, sel, ref, allowed,
           f"queries {nq} rows {n}, heads of {slices} slices masked")
