"""The screened search's proof-carrying numbers, held to an fp64 reference: the sidecar sskd_index_make_bf16 writes
(bf16 tiles of the centred rows, column sums, the three norm maxima) and the per-query band eps2 = 2 e(q) that
screen_setup_kernel derives from it (read through the test hook sskd_index_screen_band).

"Bit-identical to the exact scan, nothing for the caller to check" rests on |screen(q, r) - q.(c_r - mu)| <= e(q) for
every query and row; tests/test_screened_gpu.py sees a band that is too narrow only when a true top-k row happens to
fall outside it.  Here the inequality itself is asserted - checks (a)-(f) of tests/screen_band_cases.py, whose bounds
come from the number formats - on unit, anisotropic, large-mean, unnormalised, bf16-tie and special-row corpora at
tile-boundary sizes, and, together with bit equality of the search against oracle.topk_fma, on queries and corpora
scaled far out of the ordinary range and on non-finite data, where the only other acceptable band is +inf (the query is
answered by the in-call exact scan and counted in status[1]).

Records, not gates (MI355X; every case prints its own under -s).  Largest left side of (e) over eps2 / 2, per family,
over all sizes: unit 0.19, anisotropic 0.21, large_mean 0.41, unnorm_first 0.18, unnorm_last 0.17, unnorm_split 0.17,
ties 0.20, zero_row 0.19, outlier_row 0.14 - Cauchy-Schwarz is loose on roundings that do not line up.  eps2 over the
worst-case cap (f): unit random data 0.43 .. 0.49 (0.42 of the rounding part, plus the accumulation slack, which the
cap holds too), ties 0.63 .. 0.81.
On the kernels as they were before the range rules of screen_setup_kernel (this file's hook only): (e) failed for
queries scaled by 2^-80 (left side 4e-28, eps2 / 2 = 5e-31) and, with the corpus scaled by 2^60, for 2^-80, 2^-100 and
2^-140; a NaN row of either sign gave a NaN band for every query, a +inf row for an all-zero query, a NaN query for
itself.  Queries at 2^-70 and the corpus at 2^-70 passed (e): the fused sums keep denormal squares.
"""
import numpy as np
import pytest
import torch

import screen_band_cases as cases
from capi_helpers import stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import _native

pytestmark = pytest.mark.gpu
K = 10


def run(lib, corpus, queries, k=K, search=True):
    """make the sidecar, read the band, and search on the SAME buffers: (Sidecar, eps2, scores, ids, status)"""
    n, nq = corpus.shape[0], queries.shape[0]
    tiled = tile_corpus(lib, corpus)
    bf = torch.empty(int(lib.sskd_index_bf16_bytes(n)), dtype=torch.uint8, device="cuda")
    _native.check(lib.sskd_index_make_bf16(tiled.data_ptr(), n, bf.data_ptr(), stream()))
    q = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).cuda()
    eps2 = torch.full((nq,), float("nan"), device="cuda")
    need = int(lib.sskd_index_screen_band_scratch_bytes(nq))
    assert need >= (11 * nq + 66) * 4
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    _native.check(lib.sskd_index_screen_band(bf.data_ptr(), n, q.data_ptr(), nq, eps2.data_ptr(), scratch.data_ptr(),
                                             scratch.numel(), stream()))
    torch.cuda.synchronize()
    side = oracle.sidecar_decode(bf.cpu().numpy(), n)
    if not search:
        return side, eps2.cpu().numpy(), None, None, None
    out_s = torch.full((nq, k), float("nan"), device="cuda")
    out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(lib.sskd_index_search_screened_workspace_bytes(n, nq, k)), dtype=torch.uint8, device="cuda")
    _native.check(lib.sskd_index_search_screened(tiled.data_ptr(), bf.data_ptr(), n, q.data_ptr(), nq, k, 0,
                                                 out_s.data_ptr(), out_i.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                                 ws.numel(), stream(), None, None))
    torch.cuda.synchronize()
    return side, eps2.cpu().numpy(), out_s.cpu().numpy(), out_i.cpu().numpy(), status.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("nq", cases.SIZES_NQ)
@pytest.mark.parametrize("n", cases.SIZES_N)
@pytest.mark.parametrize("family", cases.FINITE_FAMILIES)
def test_sidecar_and_band_against_fp64(gpu, native_lib, family, n, nq):
    """(a)-(f), the candidate criterion, and the screened call on the same buffers against the oracle."""
    corpus = cases.corpus_of(family, n)
    queries = cases.queries_of(family, corpus, nq)
    side, eps2, s, i, st = run(native_lib, corpus, queries)
    ex = cases.check_sidecar(corpus, side)                                      # (a) (b) (c)
    of_cap = cases.check_band(queries, eps2, side.words)                        # (d) (f)
    ratio, screen = cases.check_soundness(queries, corpus, ex, eps2)            # (e)
    print(f"band {family} n={n} nq={nq}: max lhs/(eps2/2) = {ratio:.4f}, eps2/cap = {of_cap.min():.4f} .. {of_cap.max():.4f}")
    ref_s, ref_i = oracle.topk_fma(queries, corpus, K)
    cases.check_candidates(screen, eps2, ref_i, K)
    assert st[0] == 0
    assert np.array_equal(i, ref_i) and same_bits(s, ref_s)


def test_band_probe_checks_its_arguments(gpu, native_lib):
    lib = native_lib
    assert lib.sskd_index_screen_band_scratch_bytes(0) == 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert lib.sskd_index_screen_band(None, 2048, buf.data_ptr(), 64, buf.data_ptr(), buf.data_ptr(), buf.numel(), stream()) == 1
    assert lib.sskd_index_screen_band(buf.data_ptr(), 2048, buf.data_ptr(), 0, buf.data_ptr(), buf.data_ptr(), buf.numel(), stream()) == 1
    assert lib.sskd_index_screen_band(buf.data_ptr(), 2048, buf.data_ptr(), 64, buf.data_ptr(), buf.data_ptr(), 16, stream()) == 2
    assert b"workspace" in lib.sskd_last_error()


def _out_of_range(lib, corpus, queries, label):
    """(e) or +inf; the oracle's bits; status[1] counts the queries without a band; no NaN-scoring row returned."""
    side, eps2, s, i, st = run(lib, corpus, queries)
    ref_s, ref_i = oracle.topk_fma(queries, corpus, K)
    inf = np.isposinf(eps2)
    print(f"band {label}: {int(inf.sum())} of {len(eps2)} queries without a band, status {st.tolist()}")
    assert not np.isnan(eps2).any(), ("NaN band", np.where(np.isnan(eps2))[0][:8])
    finite_rows = np.isfinite(corpus).all(1)
    if finite_rows.all() and np.isfinite(side.colsum).all():
        ex = oracle.sidecar_expected(corpus, side.colsum)
        assert np.array_equal(side.tiles[: corpus.shape[0]].view(np.uint32), ex.ct.view(np.uint32))
        fin_q = np.isfinite(queries).all(1)
        assert inf[~fin_q].all()
        ratio, _ = cases.check_soundness(queries[fin_q], corpus, ex, eps2[fin_q], allow_inf=True)
        print(f"band {label}: max lhs/(eps2/2) over the queries with a band = {ratio:.4f}")
    else:
        assert inf.all(), "a corpus that is not finite has no band"
    assert st[0] == 0
    assert np.array_equal(i, ref_i) and same_bits(s, ref_s), (np.where((i != ref_i).any(1))[0][:8],)
    assert st[1] >= inf.sum(), (st, int(inf.sum()))          # (a query with a band may still overflow its runs)
    scores = queries.astype(np.float64) @ corpus.astype(np.float64).T
    for qi in range(len(queries)):
        got = i[qi][i[qi] >= 0]
        assert not np.isnan(scores[qi, got]).any(), ("a NaN-scoring row was returned", qi)
    assert not np.isnan(s).any()
    return eps2, st


# every n of the issue's table (full tiles, one row past, a partial and a full last tile, many tiles) and every nq
OUT_OF_RANGE_SIZES = [(2048, 257), (2049, 65), (2079, 64), (2080, 257), (20011, 65), (20011, 257)]


@pytest.mark.parametrize("n,nq", OUT_OF_RANGE_SIZES)
@pytest.mark.parametrize("family", ["unit", "ties"])
def test_scale_sweep_of_the_queries(gpu, native_lib, family, n, nq):
    """Queries of norm 2^-m, m = 0 .. 140, in one batch: below ~1e-19 fp32 squares leave the normal range, below 3e-23
    they are all zero (|q| was measured as 0 there and the band collapsed to its 1e-30 floor)."""
    corpus = cases.corpus_of(family, n)
    queries, m = cases.sweep_queries(nq)
    if family == "ties":
        queries = (cases.queries_of("ties", corpus, nq).astype(np.float64) * 2.0 ** -m[:, None].astype(np.float64)).astype(np.float32)
    eps2, st = _out_of_range(native_lib, corpus, queries, f"query sweep {family} n={n} nq={nq}")
    assert np.isfinite(eps2[m <= 63]).all(), "small queries keep their band (tests/test_screened_gpu.py scales to 2^-63)"
    assert st[1] == np.isposinf(eps2).sum()      # random scores: no band of these holds 64 rows of one lane's share


@pytest.mark.parametrize("n,nq", OUT_OF_RANGE_SIZES)
@pytest.mark.parametrize("log2_scale", [-70, -35, 60])
def test_scale_sweep_of_the_corpus(gpu, native_lib, log2_scale, n, nq):
    """2^-70: every row's sum of squares underflows, no query may keep a band.  2^-35: just above the smallest corpus
    the set-up kernel accepts, the ordinary queries keep theirs.  2^60: squares near the top of the range."""
    corpus = (cases.corpus_of("unit", n).astype(np.float64) * 2.0 ** log2_scale).astype(np.float32)
    queries, m = cases.sweep_queries(nq)
    eps2, st = _out_of_range(native_lib, corpus, queries, f"corpus x 2^{log2_scale} n={n} nq={nq}")
    if log2_scale != -70:
        assert np.isfinite(eps2[m <= 40]).all()
    assert st[1] == np.isposinf(eps2).sum()


@pytest.mark.parametrize("n,nq,row", [(2048, 257, 0), (2079, 65, 2076), (2080, 64, 1000), (20011, 257, 20010)])
@pytest.mark.parametrize("what", ["nan_row_positive", "nan_row_negative", "inf_row", "nan_query"])
def test_non_finite_data(gpu, native_lib, what, n, nq, row):
    """The exact scan never selects a NaN score (tests/test_search_gpu.py test_special_values); the screened call must
    return the same bits.  NaNs are set through their bit pattern: the norm maxima are merged as integers, where a NaN
    with the sign bit set loses and one without it wins.  Query 3 is all zero: 0 x inf must not become a NaN band."""
    corpus = cases.corpus_of("unit", n)
    queries = cases.queries_of("unit", corpus, nq)
    queries[3] = 0.0
    if what.startswith("nan_row"):
        corpus.view(np.uint32)[row, 5] = 0x7FC00000 if what.endswith("positive") else 0xFFC00000
    elif what == "inf_row":
        corpus[row, 5] = np.inf
    else:
        queries.view(np.uint32)[7, 100] = 0xFFC00000
        queries.view(np.uint32)[8, 100] = 0x7FC00000
    eps2, st = _out_of_range(native_lib, corpus, queries, f"{what} n={n} nq={nq}")
    if what == "nan_query":
        # the zero query keeps the floor band; every row scores 0, its band holds all n rows: it falls back too
        assert np.isposinf(eps2).sum() == 2 and eps2[3] < 1e-29 and st[1] == 3
    else:
        assert np.isposinf(eps2).all() and st[1] == nq
