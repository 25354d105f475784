"""The screening kernel's fragment read-ahead and first test ("Fragment read-ahead and the first test").

The query-fragment ring of a wave runs a chosen number of LDS reads ahead of the MFMAs, per workgroup size.  The depth
may not change a result: a ring slot that is overwritten before its MFMAs have read it, or a tile whose ring starts in
the wrong slot, gives specific queries of a block a wrong screen score.  (The bounds' register form did not change with
the depth, so there is no register hook here: ``sskd_screen_threshold_roundtrip`` still describes it.)

(a) ``test_every_form_at_its_smallest_shape``: every form of the kernel at the smallest ``(nq, n_rows)`` the plan maps
    to it (asserted), cases of tests/test_screen_fragment_pipeline_gpu.py - query ``i`` is corpus row ``r_i`` plus 2 %
    noise, so its top-1 is known and a fragment that reaches the wrong MFMA drops it - and ``oracle.topk_fma`` bit for bit:

      (127, 2 049)       64 per block: 6 slices x 11 tiles, fewer tiles than waves - some waves have no tile at all
      (383, 4 099)       128 per block: 11 slices x 12 tiles, one tile per wave - every tile is a wave's last
      (16 479, 32 771)   160 per block, LIGHT
      (32 799, 127 001)  160 per block, non-LIGHT, its tiles claimed AND dealt (``sskd_index_search_screened_claim``)

    Each has a ragged last tile and a padded last query block.  At the two large shapes the planted top-1 is checked for
    every query and the oracle's bits on a stride through the batch plus the padded last block.
(b) ``test_masked_tiles_at_the_head_of_every_slice``: the filtered entry point at (256, 6 007) with the first two tiles
    of EVERY slice masked whole (the sample's tiles among them): their accumulators are -inf while the lanes' bounds are
    still "none".  A -inf row that passed a -inf bound would be appended and come back as a result (or crowd the
    allowed rows out of a run); the results must be the oracle's over the allowed rows.
"""
import numpy as np
import pytest

from oracle import search as oracle
from test_screen_fragment_pipeline_gpu import K, LIGHT_MAX_TILES_PER_SLICE, base_corpus, plan, planted_queries
from test_screen_mfma16_gpu import _Run

pytestmark = pytest.mark.gpu

# (nq, n_rows, queries per block, LIGHT, slices, tiles per slice, claim arguments, oracle on every step-th query)
FORMS = [
    (127, 2_049, 64, True, 6, 11, (-1,), 1),
    (383, 4_099, 128, True, 11, 12, (-1,), 1),
    (16_479, 32_771, 160, True, 2, 513, (-1,), 131),
    (32_799, 127_001, 160, False, 1, 3_969, (1, 0), 997),
]


@pytest.mark.parametrize("nq,n,qpb,light,slices,tps,claims,step", FORMS)
def test_every_form_at_its_smallest_shape(gpu, native_lib, nq, n, qpb, light, slices, tps, claims, step):
    assert n % 32 != 0 and nq % qpb != 0     # ragged last tile, padding queries in the last block
    assert plan(native_lib, n, nq) == (qpb, slices, tps)
    assert (tps <= LIGHT_MAX_TILES_PER_SLICE) == light
    corpus = base_corpus()[:n]
    queries, rows = planted_queries(corpus, nq, 1000 + nq)
    sel = np.arange(0, nq, step)
    if step > 1:   # the padded last block and every sub-block position of one block in full
        sel = np.unique(np.concatenate([sel, np.arange(nq - 1 - (nq - 1) % qpb, nq, 13), np.arange(0, qpb, 17)]))
    ref_s, ref_i = oracle.topk_fma(queries[sel], corpus, K)
    run = _Run(native_lib, corpus, queries)
    for claim in claims:
        s, i, fallback = run.screened(claim)
        print(f"queries {nq} rows {n} claim {claim}: exact_fallback_queries {fallback}")
        wrong = np.flatnonzero(i[:, 0] != rows)
        assert wrong.size == 0, (claim, wrong[:8], wrong % qpb)     # (position inside the query block: which sub-block)
        assert (s[:, 0] > 0.99).all() and (s[:, 1] < 0.5).all()
        assert np.array_equal(i[sel], ref_i), (claim, np.argwhere(i[sel] != ref_i)[:5])
        assert np.array_equal(s[sel], ref_s), claim


def test_masked_tiles_at_the_head_of_every_slice(gpu, native_lib):
    nq, n = 256, 6_007
    qpb, slices, tps = plan(native_lib, n, nq)
    assert (qpb, slices, tps) == (128, 16, 12)
    corpus = base_corpus()[:n]
    queries, rows = planted_queries(corpus, nq, 77)
    allowed = np.ones(n, bool)
    for sl in range(slices):
        first = sl * tps * 32
        if first < n:
            allowed[first: first + 64] = False   # the slice's first two tiles, whole
    allowed[-3:] = False                         # and the end of the ragged last tile
    assert (~allowed[:64]).all() and allowed.sum() > n // 2
    lost = ~allowed[rows]
    assert 10 < lost.sum() < nq // 2             # planted rows on both sides of the mask
    scores = oracle.scores_fma(queries, corpus)
    scores[:, ~allowed] = -np.inf
    ref_s, ref_i = oracle.topk_of_scores(scores, K)
    s, i, fallback = _Run(native_lib, corpus, queries, allowed).screened(-1)
    print(f"masked heads of {slices} slices: exact_fallback_queries {fallback}")
    assert allowed[i].all() and np.isfinite(s).all()
    assert np.array_equal(i, ref_i), np.argwhere(i != ref_i)[:5]
    assert np.array_equal(s, ref_s)
    assert (i[~lost, 0] == rows[~lost]).all() and not (i[lost] == rows[lost, None]).any()

