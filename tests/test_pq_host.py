"""IVF-PQ, host side (no GPU): the NumPy restatement of the definitions (``pq_cases``) against exact rational arithmetic,
the files, the launch plan and workspace through ctypes, and every refused argument (a refused call returns before any
HIP call)."""
import ctypes as C
import json
from fractions import Fraction

import numpy as np
import pytest

import pq_cases as pc
from semantic_search_kd_amd import IVFPQIndex, pq

SSKD_ERR_INVALID = 1
U64 = 2.0 ** -53   # fp64 unit roundoff
U32 = 2.0 ** -24


def _fr(a):
    return [Fraction(float(x)) for x in np.asarray(a).reshape(-1)]


# --------------------------------------------------------------------- the restatement against exact rationals
def _small(m):
    rng = np.random.default_rng(3)
    cb = pc.seeded_codebooks(m, 5, scale=0.1)
    rows = rng.standard_normal((6, pc.DIM)).astype(np.float32) * 0.1
    centroids = rng.standard_normal((3, pc.DIM)).astype(np.float32) * 0.05
    assign = np.array([0, 2, 1, 1, 0, 2])
    return m, cb, rows, centroids, assign


@pytest.fixture(scope="module")
def small():
    return _small(8)


def test_residual_is_one_fp32_subtraction(small):
    m, cb, rows, centroids, assign = small
    r = pc.residuals(rows, centroids, assign)
    assert r.dtype == np.float32
    for i in range(rows.shape[0]):
        for d in (0, 1, 200, 383):
            exact = Fraction(float(rows[i, d])) - Fraction(float(centroids[assign[i], d]))
            assert abs(Fraction(float(r[i, d])) - exact) <= abs(exact) * Fraction(U32)   # correctly rounded
    assert np.array_equal(pc.bits32(pc.residuals(rows)), pc.bits32(rows))


def test_encode_distance_and_argmin_against_rationals(small):
    m, cb, rows, centroids, assign = small
    dsub = pc.DIM // m
    r = pc.residuals(rows, centroids, assign)
    codes = pc.encode(r, cb)
    for i in range(3):
        for j in (0, m - 1):
            dist = pc.encode_distances(r[i:i + 1], cb, j)[0]
            rj = _fr(r[i, j * dsub:(j + 1) * dsub])
            exact = [sum((a - b) ** 2 for a, b in zip(rj, _fr(cb[j, c]))) for c in range(pc.CODES)]
            # dsub terms, each with three roundings, then dsub - 1 additions: (dsub + 2) u relative covers it
            for c in range(pc.CODES):
                assert abs(Fraction(float(dist[c])) - exact[c]) <= exact[c] * Fraction((dsub + 2) * U64)
            best = min(exact)
            assert exact[codes[i, j]] <= best * (1 + Fraction(2 * (dsub + 2) * U64))
            assert codes[i, j] == int(np.argmin(dist))


def test_encode_ties_go_to_the_lower_code(small):
    m, cb, rows, centroids, assign = small
    dup = cb.copy()
    dup[:, 200] = dup[:, 7]   # entry 200 repeats entry 7 in every subspace
    r = np.concatenate([dup[j, 200] for j in range(m)])[None, :]   # a row made of the duplicated entries
    assert (pc.encode(r, dup) == 7).all()


def test_code_sums_against_rationals(small):
    m, cb, rows, centroids, assign = small
    dsub = pc.DIM // m
    rng = np.random.default_rng(9)
    r = rng.standard_normal((40, pc.DIM)).astype(np.float32)
    codes = rng.integers(0, 5, size=(40, m)).astype(np.uint8)   # five codes used: the groups hold about eight rows
    sums, counts = pc.code_sums(r, codes, m)
    assert counts.sum(axis=1).tolist() == [40] * m and (counts[:, 5:] == 0).all() and (sums[:, 5:] == 0).all()
    for j in (0, m - 1):
        for c in range(5):
            member = np.flatnonzero(codes[:, j] == c)
            for d in (0, dsub - 1):
                col = _fr(r[member, j * dsub + d])
                bound = Fraction((len(col) - 1) * U64) * sum(abs(x) for x in col)
                assert abs(Fraction(float(sums[j, c, d])) - sum(col)) <= bound
            # one accumulator, ascending rows: the plain loop gives the same bits
            acc = np.float64(0.0)
            for i in member:
                acc = acc + np.float64(r[i, j * dsub])
            assert acc == sums[j, c, 0]
    new = pc.update_codebooks(cb, sums, counts)
    assert np.array_equal(pc.bits32(new[:, 5:]), pc.bits32(cb[:, 5:]))   # empty codes keep their entries
    assert new[0, 0, 0] == np.float32(sums[0, 0, 0] / counts[0, 0])


def test_lut_against_rationals(small):
    m, cb, rows, centroids, assign = small
    dsub = pc.DIM // m
    table = pc.lut(rows[:2], cb)
    assert table.shape == (2, m, pc.CODES) and table.dtype == np.float32
    for j in (0, 3, m - 1):
        for c in (0, 17, 255):
            qj, e = _fr(rows[1, j * dsub:(j + 1) * dsub]), _fr(cb[j, c])
            exact = sum(a * b for a, b in zip(qj, e))
            mag = sum(abs(a * b) for a, b in zip(qj, e))
            # the products are exact; dsub - 1 fp64 additions, then one rounding to fp32
            assert abs(Fraction(float(table[1, j, c])) - exact) <= Fraction((dsub - 1) * U64) * mag + abs(exact) * Fraction(U32)


def test_adc_chain_and_rank_order(small):
    m, cb, rows, centroids, assign = small
    rng = np.random.default_rng(13)
    table = pc.lut(rows[:1], cb)[0]
    codes = rng.integers(0, 256, size=(5, m)).astype(np.uint8)
    base = rng.standard_normal(5).astype(np.float32)
    s = pc.adc_scores(base, table, codes)
    for i in range(5):
        acc = np.float32(base[i])
        terms = [Fraction(float(base[i]))]
        for j in range(m):
            acc = np.float32(acc + table[j, codes[i, j]])
            terms.append(Fraction(float(table[j, codes[i, j]])))
        assert pc.bits32(acc) == pc.bits32(s[i])
        assert abs(Fraction(float(s[i])) - sum(terms)) <= Fraction(m * U32) * sum(abs(t) for t in terms)
    order = pc.rank_order(np.float32([1.0, 2.0, 2.0, -1.0, 2.0]), np.array([9, 8, 3, 1, 5]))
    assert order.tolist() == [2, 4, 1, 0, 3]   # score descending, then lower id
    ps, pi = pc.padded(np.float32([3.0, 1.0]), np.array([4, 2]), 4)
    assert pi.tolist() == [4, 2, -1, -1] and ps[2] == pc.NEG_PAD


def test_probed_rows_skip_bad_probes_and_hidden_rows():
    offsets = np.array([0, 2, 2, 5], np.int64)
    list_rows = np.array([3, 4, 0, 1, 2], np.int32)
    allowed = np.array([True, False, True, True, True])
    rows, base = pc.probed([2, -1, 7, 1, 0], np.float32([0.5, 9, 9, 9, 0.25]), offsets, list_rows, 3, allowed)
    assert rows.tolist() == [0, 2, 3, 4] and base.tolist() == [0.5, 0.5, 0.25, 0.25]


@pytest.mark.parametrize("check", [test_residual_is_one_fp32_subtraction, test_encode_distance_and_argmin_against_rationals,
                                   test_encode_ties_go_to_the_lower_code, test_code_sums_against_rationals,
                                   test_lut_against_rationals, test_adc_chain_and_rank_order], ids=lambda f: f.__name__)
def test_the_restatement_at_m_24(check):
    """the checks above at m = 24: dsub = 16, and an m that is not a power of two"""
    check(_small(24))


def test_the_world_of_m_96_has_no_tied_encoding_distance():
    """The GPU tests compare the codes of every m with ``pc.encode``.  At m = 96 an entry has four components only, so
    two entries at the same fp64 distance from a residual slice are conceivable; the lower-code rule would then carry the
    comparison instead of the arithmetic.  Checked for the codebook seed the GPU world of m = 96 uses
    (``test_pq_gpu.world_seed(96)`` = 196) and the seed of ``test_encode`` (106) on the 3 001-row world: the two smallest
    distances of every (row, subspace) differ.  Should a change of the world produce a tie, change the seed."""
    import test_pq_gpu as gpu_side
    from oracle import search as oracle

    m = 96
    assert gpu_side.world_seed(m) == 196
    corpus = oracle.seeded_unit_rows(gpu_side.N, pc.DIM, 1)
    centroids = (oracle.seeded_unit_rows(gpu_side.NLIST, pc.DIM, 4) * np.float32(0.25)).astype(np.float32)
    assignment = np.random.default_rng(3).integers(0, gpu_side.NLIST, size=gpu_side.N)
    resid = pc.residuals(corpus, centroids, assignment)
    for seed in (gpu_side.world_seed(m), 10 + m):
        cb = gpu_side._sample_codebooks(resid, m, seed)
        codes = pc.encode(resid, cb)
        for j in range(m):
            two = np.partition(pc.encode_distances(resid, cb, j), 1, axis=1)[:, :2]
            assert (two[:, 0] < two[:, 1]).all(), f"seed {seed}, subspace {j}: tied distances"
        # the sampled rows encode to their own entries at distance +0.0, a strict minimum
        pick = np.sort(np.random.default_rng(seed).permutation(gpu_side.N)[:pc.CODES])
        assert (codes[pick] == np.arange(pc.CODES, dtype=np.uint8)[:, None]).all()


# ------------------------------------------------------------------------------------------------ python side
def test_defaults_and_python_refusals():
    assert [pq.default_refine(k) for k in (1, 10, 25, 26, 64, 256)] == [100, 100, 100, 104, 256, 256]
    assert pq.check_refine(10, None) == 100 and pq.check_refine(10, 0) == 0 and pq.check_refine(10, 10) == 10
    for k, r in ((10, 9), (10, 257), (1, -1)):
        with pytest.raises(ValueError):
            pq.check_refine(k, r)
    # the value kept with an index is a floor, never a refusal: any k up to 256 is answered
    assert [pq.stored_refine(k, None) for k in (10, 64)] == [100, 256]
    assert [pq.stored_refine(k, 20) for k in (1, 20, 21, 100, 256)] == [20, 20, 21, 100, 256]
    assert pq.stored_refine(100, 0) == 0 and pq.stored_refine(200, 256) == 256
    for m in pq.PQ_M_ALLOWED:
        assert pq.check_m(m) == m and 384 % m == 0
    for m in (12, 0, 7, 128, 384):
        with pytest.raises(ValueError):
            pq.check_m(m)
    with pytest.raises(ValueError):
        pq.check_codebooks(np.zeros((8, 256, 47), np.float32), 8)
    assert IVFPQIndex is pq.IVFPQIndex
    # fewer than 256 training rows: refused before anything else is looked at
    from types import SimpleNamespace

    index = IVFPQIndex.__new__(IVFPQIndex)
    index.flat = SimpleNamespace(ntotal=255)
    with pytest.raises(ValueError, match="at least 256 rows"):
        index.train()


def test_files_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    cb = pc.seeded_codebooks(16, 1)
    codes = rng.integers(0, 256, size=(200, 16)).astype(np.uint8)
    pq.save_pq(tmp_path, cb, codes, {"refine": None, "seed": 7, "iterations": 3})
    meta = json.loads((tmp_path / "pq.json").read_text())
    assert meta == {"refine": None, "seed": 7, "iterations": 3, "m": 16, "nbits": 8, "format_version": 1}
    assert pq.is_pq_dir(tmp_path) and not pq.is_pq_dir(tmp_path / "nowhere")
    cb2, codes2, meta2 = pq.load_pq(tmp_path)
    assert np.array_equal(pc.bits32(cb2), pc.bits32(cb)) and cb2.dtype == np.float32
    assert np.array_equal(codes2, codes) and codes2.dtype == np.uint8 and meta2 == meta
    np.save(tmp_path / "pq_codes.npy", codes[:, :15])   # a damaged file is noticed
    with pytest.raises(ValueError):
        pq.load_pq(tmp_path)
    np.save(tmp_path / "pq_codes.npy", codes)
    for bad in ({"format_version": 2}, {"nbits": 4}, {"m": 12}):
        (tmp_path / "pq.json").write_text(json.dumps({**meta, **bad}))
        with pytest.raises(ValueError):
            pq.load_pq(tmp_path)
    with pytest.raises(ValueError):
        pq.save_pq(tmp_path, cb, codes[:, :8], {})


# ------------------------------------------------------------------------------------- the plan, through ctypes
def _plan(lib, nq, nprobe, k, refine, m, n_rows, longest):
    parts, rows, wgs, lut = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    rc = lib.sskd_pq_search_plan(nq, nprobe, k, refine, m, n_rows, longest, C.byref(parts), C.byref(rows), C.byref(wgs),
                                 C.byref(lut))
    return rc, parts.value, rows.value, wgs.value, lut.value


@pytest.mark.parametrize("nq, nprobe, k, refine, m, n_rows, longest", [
    (1, 32, 10, 100, 64, 1_000_000, 2000), (1, 128, 10, 256, 64, 1_000_000, 2000), (64, 32, 10, 100, 64, 1_000_000, 2000),
    (4096, 32, 10, 100, 96, 1_000_000, 2000), (1, 16, 1, 0, 8, 3001, 2700), (200, 16, 256, 256, 24, 3001, 300),
    (1, 1, 1, 0, 16, 0, 0), (3, 65536, 10, 40, 48, 8_800_000, 1000), (1, 1024, 256, 0, 32, 8_800_000, 9000),
])
def test_plan_and_workspace(native_lib, nq, nprobe, k, refine, m, n_rows, longest):
    rc, parts, part_rows, wgs, lut = _plan(native_lib, nq, nprobe, k, refine, m, n_rows, longest)
    cap = refine if refine else k
    assert rc == 0 and parts >= 1 and wgs == parts * nq and lut == nq * m * 1024
    assert parts * cap <= 4096                                   # the records of one query the refine step sorts
    # a part's code bytes are at least four times the LUT bytes its workgroup loads (1 KiB m), unless there is one part
    assert part_rows * m >= 4 * m * 1024
    assert parts == 1 or parts * part_rows <= min(n_rows, nprobe * longest)
    need = int(native_lib.sskd_pq_search_workspace_bytes(nq, nprobe, k, refine, m, n_rows, longest))
    assert need >= lut + parts * nq * cap * 8
    assert native_lib.sskd_pq_search_plan(nq, nprobe, k, refine, m, n_rows, longest, None, None, None, None) == 0


def test_plan_spreads_a_single_query_and_not_a_batch(native_lib):
    assert _plan(native_lib, 1, 128, 10, 100, 64, 1_000_000, 2000)[1] >= 16
    assert _plan(native_lib, 4096, 32, 10, 100, 64, 1_000_000, 2000)[1] == 1


@pytest.mark.parametrize("nq, nprobe, k, refine, m, n_rows, longest", [
    (0, 1, 1, 0, 64, 10, 10), (1, 0, 1, 0, 64, 10, 10), (1, 65537, 1, 0, 64, 10, 10), (1, 1, 0, 0, 64, 10, 10),
    (1, 1, 257, 0, 64, 10, 10), (1, 1, 10, 9, 64, 10, 10), (1, 1, 10, 257, 64, 10, 10), (1, 1, 10, -1, 64, 10, 10),
    (1, 1, 1, 0, 12, 10, 10), (1, 1, 1, 0, 0, 10, 10), (1, 1, 1, 0, 64, -1, 0), (1, 1, 1, 0, 64, 10, -1),
])
def test_plan_refuses(native_lib, nq, nprobe, k, refine, m, n_rows, longest):
    assert _plan(native_lib, nq, nprobe, k, refine, m, n_rows, longest)[0] == SSKD_ERR_INVALID
    assert native_lib.sskd_last_error()
    assert native_lib.sskd_pq_search_workspace_bytes(nq, nprobe, k, refine, m, n_rows, longest) == 0


# ------------------------------------------------------------------- refusal before anything is enqueued, through ctypes
P = 1 << 20   # a non-null, 16-byte aligned address that is never dereferenced: every case below is refused on the host

SEARCH_KEYS = ("tiled", "n_rows", "queries", "nq", "probe", "probe_scores", "nprobe", "offsets", "rows", "nlist", "codes",
               "codebooks", "m", "k", "refine", "id_offset", "mask", "out_s", "out_i", "out_c", "ws", "ws_bytes", "stream")


def _search_args(**over):
    a = dict(tiled=P, n_rows=1000, queries=P, nq=2, probe=P, probe_scores=P, nprobe=4, offsets=P, rows=P, nlist=16, codes=P,
             codebooks=P, m=64, k=10, refine=100, id_offset=0, mask=None, out_s=P, out_i=P, out_c=None, ws=P,
             ws_bytes=1 << 30, stream=None)
    a.update(over)
    return [a[key] for key in SEARCH_KEYS]


@pytest.mark.parametrize("over, word", [
    (dict(m=12), "m=12"), (dict(m=0), "m=0"), (dict(k=0), "k=0"), (dict(k=257, refine=0), "k=257"),
    (dict(refine=9), "refine=9"), (dict(refine=257), "refine=257"), (dict(refine=-1), "refine=-1"),
    (dict(nprobe=0), "nprobe=0"), (dict(nprobe=17), "nprobe=17"), (dict(nlist=0), "nlist=0"),
    (dict(nlist=65537, nprobe=1), "nlist=65537"), (dict(n_rows=-1), "n_rows"), (dict(nq=-1), "nq"),
    (dict(nq=65536), "nq=65536"), (dict(id_offset=-1), "id_offset"), (dict(n_rows=(1 << 31) - 64), "int32"),
    (dict(refine=0, out_c=P), "candidates"),
    (dict(tiled=None), "null"), (dict(queries=None), "null"), (dict(probe=None), "null"), (dict(probe_scores=None), "null"),
    (dict(offsets=None), "null"), (dict(rows=None), "null"), (dict(codes=None), "null"), (dict(codebooks=None), "null"),
    (dict(out_s=None), "null"), (dict(out_i=None), "null"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=16), "workspace"), (dict(ws_bytes=0), "workspace"),
    (dict(ws_bytes=2 * 64 * 1024), "workspace"),   # the LUT alone: no room for one part's records
    (dict(queries=P + 4), "aligned"), (dict(codes=P + 8), "aligned"), (dict(ws=P + 8), "aligned"),
])
def test_search_refuses_bad_arguments(native_lib, over, word):
    rc = native_lib.sskd_pq_search(*_search_args(**over))
    assert rc == SSKD_ERR_INVALID
    assert word in native_lib.sskd_last_error().decode()


def test_search_with_no_queries_is_a_noop(native_lib):
    assert native_lib.sskd_pq_search(*_search_args(nq=0, queries=None, probe=None, probe_scores=None, out_s=None,
                                                   out_i=None, ws=None, ws_bytes=0)) == 0


@pytest.mark.parametrize("over, word", [
    (dict(m=12), "m=12"), (dict(n=-1), "n < 0"), (dict(n=(1 << 31) - 64), "int32"), (dict(nlist=0), "nlist=0"),
    (dict(nlist=65537), "nlist=65537"), (dict(centroids=None), "centroids"), (dict(rows=None), "null"),
    (dict(codebooks=None), "null"), (dict(codes=None), "null"),
])
def test_encode_refuses_bad_arguments(native_lib, over, word):
    a = dict(rows=P, n=100, centroids=P, assign=P, nlist=4, codebooks=P, m=64, codes=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_pq_encode(*[a[key] for key in ("rows", "n", "centroids", "assign", "nlist", "codebooks", "m",
                                                        "codes", "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_pq_encode(None, 0, None, None, 0, None, 64, None, None) == 0   # no rows: nothing to do


@pytest.mark.parametrize("over, word", [
    (dict(m=12), "m=12"), (dict(n=-1), "n < 0"), (dict(nlist=0), "nlist=0"), (dict(centroids=None), "centroids"),
    (dict(offsets=None), "null"), (dict(sums=None), "null"), (dict(counts=None), "null"), (dict(rows=None), "null"),
    (dict(order=None), "null"),
])
def test_code_sums_refuses_bad_arguments(native_lib, over, word):
    a = dict(rows=P, n=100, centroids=P, assign=P, nlist=4, offsets=P, order=P, m=64, sums=P, counts=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_pq_code_sums(*[a[key] for key in ("rows", "n", "centroids", "assign", "nlist", "offsets", "order",
                                                           "m", "sums", "counts", "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()


@pytest.mark.parametrize("over, word", [
    (dict(m=12), "m=12"), (dict(nq=-1), "nq < 0"), (dict(nq=65536), "nq=65536"), (dict(queries=None), "null"),
    (dict(codebooks=None), "null"), (dict(lut=None), "null"),
])
def test_lut_refuses_bad_arguments(native_lib, over, word):
    a = dict(queries=P, nq=3, codebooks=P, m=64, lut=P, stream=None)
    a.update(over)
    rc = native_lib.sskd_pq_lut(*[a[key] for key in ("queries", "nq", "codebooks", "m", "lut", "stream")])
    assert rc == SSKD_ERR_INVALID and word in native_lib.sskd_last_error().decode()
    assert native_lib.sskd_pq_lut(None, 0, None, 64, None, None) == 0
