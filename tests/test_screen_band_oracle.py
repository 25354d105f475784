"""The screened search's band reference (oracle/search.py) on its own, without a GPU.

tests/test_screen_band_gpu.py holds the device's sidecar and band to this reference.  That is only worth something if
the reference itself satisfies the soundness inequality on every input family, if the layout helper is right, and if
the shared checks (tests/screen_band_cases.py) would notice a wrong reference: all three are asserted here, with an
fp32 emulation of the kernels' arithmetic standing in for the device.
"""
import numpy as np
import pytest

import screen_band_cases as cases
from oracle import search as oracle


def test_sidecar_layout_round_trip():
    n = 2049
    rng = np.random.default_rng(1)
    tiles = oracle.bf16_round(rng.standard_normal((n, 384)).astype(np.float32))
    words = np.array([3.0, 2.0, 1.0e-5], np.float32)
    colsum = rng.standard_normal(384).astype(np.float32)
    raw = oracle.sidecar_encode(tiles, words, colsum, 4.5, n)
    assert raw.dtype == np.uint8 and raw.size == 65 * 24576 + 4096
    side = oracle.sidecar_decode(raw, n)
    assert side.tiles.shape == (2080, 384)
    assert np.array_equal(side.tiles[:n], tiles) and not side.tiles[n:].any()
    assert np.array_equal(side.words, words) and np.array_equal(side.colsum, colsum) and side.absmax == 4.5
    # the stated addresses, spelled out: tile t, step s, lane l, element e <-> row 32 t + (l & 31), column 16 s + 8 (l >> 5) + e
    h = raw[: 65 * 24576].view(np.uint16)
    for t, s, l, e in [(0, 0, 0, 0), (3, 5, 40, 7), (64, 23, 63, 7), (64, 0, 0, 3), (17, 11, 31, 2)]:
        row, col = 32 * t + (l & 31), 16 * s + 8 * (l >> 5) + e
        want = tiles[row, col] if row < n else np.float32(0)
        assert h[((t * 24 + s) * 64 + l) * 8 + e] == (want.view(np.uint32) >> 16)
    block = raw[65 * 24576:]
    assert np.array_equal(block.view(np.int32)[:3], words.view(np.int32))
    assert np.array_equal(block.view(np.float32)[64:448], colsum)


@pytest.mark.parametrize("n", cases.SIZES_N)
@pytest.mark.parametrize("family", cases.FINITE_FAMILIES)
def test_reference_alone_is_sound(family, n):
    """(a)-(f) with the emulation as the device: the fp64 band covers the fp64 screening error plus the accumulation
    allowance on every family - the condition that makes the GPU assertions meaningful."""
    corpus = cases.corpus_of(family, n)
    queries = cases.queries_of(family, corpus, 65)
    side, _ = cases.emulate_sidecar(corpus)
    ex = cases.check_sidecar(corpus, side)
    e64 = oracle.band_expected(queries, ex.words)
    ratio, screen = cases.check_soundness(queries, corpus, ex, e64)
    assert 0.0 < ratio <= 1.0
    cases.check_band(queries, cases.emulate_band(queries, side.words), side.words)
    ref_s, ref_i = oracle.topk_fma(queries, corpus, 10)
    cases.check_candidates(screen, e64, ref_i, 10)


def test_families_are_what_they_claim():
    n = 2079
    c = cases.corpus_of("anisotropic", n)
    assert 0.7 < float((c[:512] @ c[512:1024].T).mean()) < 0.8
    c = cases.corpus_of("large_mean", n)
    ex = oracle.sidecar_expected(c, c.sum(0, dtype=np.float32))
    assert ex.words[1] < ex.words[0] / 100                                   # |c~| << |c|
    for fam, at in (("unnorm_first", 0), ("unnorm_last", n - 1)):
        c = cases.corpus_of(fam, n)
        assert int(np.linalg.norm(c, axis=1).argmax()) == at and at // 32 == (0 if at == 0 else n // 32)
    c = cases.corpus_of("unnorm_split", n)
    ex = oracle.sidecar_expected(c, c.sum(0, dtype=np.float32))
    big = int(np.linalg.norm(c, axis=1).argmax())
    worst = int(np.linalg.norm((ex.ct - ex.xc).astype(np.float64), axis=1).argmax())
    assert big in (n // 3, n // 3 + 1) and worst not in (n // 3, n // 3 + 1)
    c = cases.corpus_of("ties", n)
    assert (np.abs(oracle.bf16_round(c) - c)[c != 0] >= np.abs(c[c != 0]) * 2.0 ** -9).all()   # every element on a tie


def test_sweep_reference_is_sound_in_fp64():
    """The scale sweep's inputs: in fp64 nothing underflows, so the reference band is sound at every scale."""
    corpus = cases.corpus_of("unit", 2049)
    queries, m = cases.sweep_queries(70)
    assert set(m) == set(cases.SWEEP_M) and (np.linalg.norm(queries.astype(np.float64), axis=1) > 0).all()
    for scale in (1.0, 2.0 ** -70, 2.0 ** 60):
        c = (corpus.astype(np.float64) * scale).astype(np.float32)
        ex = oracle.sidecar_expected(c, c.sum(0, dtype=np.float32))
        cases.check_soundness(queries, c, ex, oracle.band_expected(queries, ex.words))


def test_band_check_notices_a_dropped_cross_term():
    """Sensitivity of (d): a reference without the |q| max|c~ - xc| term is far below the band a correct kernel reports."""
    corpus = cases.corpus_of("unit", 2049)
    queries = cases.queries_of("unit", corpus, 65)
    side, _ = cases.emulate_sidecar(corpus)
    eps2 = cases.emulate_band(queries, side.words)
    terms = oracle.band_terms(queries, side.words)
    cases.check_band(queries, eps2, side.words)
    wrong = terms.copy()
    wrong[:, 1] = 0.0
    with pytest.raises(AssertionError, match="band inflated"):
        cases.check_band(queries, eps2, side.words, terms=wrong)
    # and the other way round: a KERNEL that dropped it is below the right reference
    f = np.float32
    dropped = (f(2.0) * (terms[:, 0] + terms[:, 2]).astype(f) * f(1.0002) + f(1e-30)).astype(f)
    with pytest.raises(AssertionError, match="band below its formula"):
        cases.check_band(queries, dropped, side.words)


def test_word_check_notices_a_maximum_that_skips_the_last_tile():
    """Sensitivity of (c): the largest row sits in the partial last tile; a maximum over the full tiles only is caught,
    from either side."""
    n = 2079
    corpus = cases.corpus_of("unnorm_last", n)
    side, raw = cases.emulate_sidecar(corpus)
    ex = cases.check_sidecar(corpus, side)
    full = slice(0, (n // 32) * 32)
    short = oracle.row_norm2_max(corpus, ex.xc, ex.ct, full)
    assert short[0] < 0.9 * ex.words[0]
    with pytest.raises(AssertionError, match="norm words"):
        cases.check_sidecar(corpus, side, expected_words=short)
    broken = side._replace(words=short.astype(np.float32))
    with pytest.raises(AssertionError, match="norm words"):
        cases.check_sidecar(corpus, broken)
