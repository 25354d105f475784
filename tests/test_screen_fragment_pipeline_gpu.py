"""The screening kernel's query-fragment ring: every (sub-block, k-step) fragment reaches the MFMA it belongs to.

The kernel keeps its LDS fragment reads a few MFMAs ahead of their use in a small register ring.  A wrong (sub-block,
k-step) index in that ring gives a wrong screen score for specific queries of a block, so the cases are built so that it
cannot hide: query ``i`` is corpus row ``r_i`` plus 2 % noise, renormalised, with a different ``r_i`` per query.  Its
exact top-1 is then known (``r_i``, score ~ 0.9998, the rest of the corpus below 0.3) - a mis-indexed fragment drops it
from the appended set - and on top every checked query must equal ``oracle.topk_fma`` bit for bit, as
tests/test_screened_gpu.py demands.

Shapes: the smallest ``(nq, n_rows)`` with ``n_rows >= nq`` that ``sskd_index_search_screened_plan`` maps to each form
(asserted here; LIGHT = at most 330 tiles per wave, i.e. 3 960 per slice):

  (127, 2 049)        64 per block, LIGHT      2 blocks (last one 63 queries), 6 slices x 11 tiles: fewer tiles than waves
  (383, 4 099)       128 per block, LIGHT      3 blocks (last one 127), 11 slices x 12 tiles: one tile per wave
  (16 479, 32 771)   160 per block, LIGHT      103 blocks (last one 159), 2 slices x 513 tiles
  (27 359, 127 001)  128 per block, non-LIGHT  214 blocks (last one 95), 1 slice x 3 969 tiles
  (32 799, 127 001)  160 per block, non-LIGHT  205 blocks (last one 159), 1 slice x 3 969 tiles
  (256, 6 007)       128 per block, LIGHT, MASKED (the filtered entry point)

64 queries per block serve batches below 256 queries only, which the planner cuts into 42 slices whatever the corpus:
their non-LIGHT form needs 42 x 3 961 x 32 = 5.3 M rows (8 GB of fp32 rows) and is not run here; it is the same template
as the two non-LIGHT forms above with fewer sub-blocks.
At the three large shapes the planted top-1 is checked for EVERY query and the oracle's bits on a sample of them (a
stride through the batch, plus every 13th query of the padded last block and every 17th of the first), which keeps the
CPU reference at a second or two.
"""
import ctypes

import numpy as np
import pytest

from oracle import search as oracle
from semantic_search_kd_amd import FAISSIndexBuilder, _native
from test_screened_gpu import screened

pytestmark = pytest.mark.gpu

DIM, K = 384, 10
LIGHT_MAX_TILES_PER_SLICE = 330 * 12
BASE_ROWS = 127_001

_base = {}


def base_corpus():
    """One seeded corpus for every case (a case uses its first n rows); never modified."""
    if "c" not in _base:
        c = oracle.seeded_unit_rows(BASE_ROWS, DIM, 5150)
        c.setflags(write=False)
        _base["c"] = c
    return _base["c"]


def planted_queries(corpus, nq, seed):
    """query i = corpus[r_i] + 0.02 u_i, renormalised; r_i distinct (a stride coprime to n walks every row once)"""
    n = corpus.shape[0]
    assert nq <= n
    stride = next(s for s in range(int(n * 0.618), n) if np.gcd(s, n) == 1)
    rows = (7 + stride * np.arange(nq, dtype=np.int64)) % n
    assert np.unique(rows).size == nq
    q = corpus[rows] + np.float32(0.02) * oracle.seeded_unit_rows(nq, DIM, seed)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.ascontiguousarray(q, np.float32), rows


def plan(lib, n, nq):
    qpb, passes, slices = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _native.check(lib.sskd_index_search_screened_plan(n, nq, K, ctypes.byref(qpb), ctypes.byref(passes), ctypes.byref(slices)))
    tiles_per_slice = -(-(-(-n // 32)) // slices.value)
    return qpb.value, slices.value, tiles_per_slice


# (nq, n_rows, queries per block, LIGHT, slices, tiles per slice, oracle on every step-th query)
FORMS = [
    (127, 2_049, 64, True, 6, 11, 1),
    (383, 4_099, 128, True, 11, 12, 1),
    (16_479, 32_771, 160, True, 2, 513, 131),
    (27_359, 127_001, 128, False, 1, 3_969, 997),
    (32_799, 127_001, 160, False, 1, 3_969, 997),
]


@pytest.mark.parametrize("nq,n,qpb,light,slices,tps,step", FORMS)
def test_every_fragment_reaches_its_mfma(gpu, native_lib, nq, n, qpb, light, slices, tps, step):
    assert n % 32 != 0 and nq % qpb != 0     # ragged last tile, padding queries in the last block
    assert plan(native_lib, n, nq) == (qpb, slices, tps)
    assert (tps <= LIGHT_MAX_TILES_PER_SLICE) == light
    corpus = base_corpus()[:n]
    queries, rows = planted_queries(corpus, nq, 1000 + nq)
    s, i, st = screened(native_lib, corpus.copy(), queries, K)   # (the shared corpus is read-only; torch wants its own)
    assert st[0] == 0, st
    wrong = np.flatnonzero(i[:, 0] != rows)
    assert wrong.size == 0, (wrong[:8], wrong % qpb)            # (position inside the query block: which sub-block)
    assert (s[:, 0] > 0.99).all() and (s[:, 1] < 0.5).all()
    sel = np.arange(0, nq, step)
    if step > 1:   # the padded last block and every sub-block position of one block in full
        sel = np.unique(np.concatenate([sel, np.arange(nq - 1 - (nq - 1) % qpb, nq, 13), np.arange(0, qpb, 17)]))
    ref_s, ref_i = oracle.topk_fma(queries[sel], corpus, K)
    assert np.array_equal(i[sel], ref_i), np.argwhere(i[sel] != ref_i)[:5]
    assert np.array_equal(s[sel], ref_s)


def test_masked_form_takes_the_second_best_set(gpu, native_lib):
    """The filtered entry point: the planted row of every third query is masked out, so those queries must return the
    oracle's top k over the allowed rows - their own planted row gone, everything else as before."""
    nq, n = 256, 6_007
    assert plan(native_lib, n, nq) == (128, 16, 12)
    corpus = base_corpus()[:n]
    queries, rows = planted_queries(corpus, nq, 77)
    allowed = np.ones(n, bool)
    allowed[rows[::3]] = False
    index = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device=str(gpu))
    index.build_from_embeddings(np.array(corpus))
    s, i = index.search(queries, K, allow=allowed)
    assert index.last_search_path.endswith("+screened"), index.last_search_path
    scores = oracle.scores_fma(queries, corpus)
    scores[:, ~allowed] = -np.inf
    ref_s, ref_i = oracle.topk_of_scores(scores, K)
    assert np.array_equal(i, ref_i), np.argwhere(i != ref_i)[:5]
    assert np.array_equal(s, ref_s)
    masked_q = np.arange(0, nq, 3)
    assert not (i[masked_q] == rows[masked_q, None]).any()
    keep = np.setdiff1d(np.arange(nq), masked_q)
    # a kept query's planted row survives unless another query's masking took that very row (rows are distinct: never)
    assert (i[keep, 0] == rows[keep]).all()
