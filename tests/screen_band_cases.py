"""Inputs and checks shared by tests/test_screen_band_oracle.py (CPU) and tests/test_screen_band_gpu.py.

The checks take "device" values (sidecar bytes decoded by ``oracle.search.sidecar_decode``, the ``eps2`` of
``sskd_index_screen_band``) and hold them to the fp64 reference of ``oracle.search``.  The CPU tests feed them an fp32
emulation of the kernels' arithmetic instead, which is what makes the bounds checkable without a GPU and lets them
prove that a wrong reference would be caught.

Every bound comes from the number formats, not from what a kernel returned:

(b) a column sum of P fp32 terms added in any order is off by at most P 2^-24 sum|c_rj| (each of the < P additions
    rounds a partial sum that is at most sum|c|);
(c) a norm word is a sum of 384 non-negative fused terms, taken in fp32: at most 384 roundings of 2^-24 relative to
    the running sum, second order included 400 x 2^-24;
(d) the kernel claims eps2 >= E (rounded up) and multiplies by 1.0002: the fp32 norms are within 385 x 2^-24 / 2 of the
    fp64 ones, so eps2 <= 1.0003 E + 2e-30 (its additive floor is 1e-30);
(e) bf16 rounding (Cauchy-Schwarz) plus the accumulation allowance 3 x 384 x 2^-24 (1 + 2^-8)^2 |q| max(cn, cb) that
    csrc/screen.hip derives SCREEN_ACC_SLACK from must fit in eps2 / 2 together;
(f) the header's stated worst case, 2^-7 (1 + 2^-9) + 2e-4 relative to |q| max(cn, cb) on each side, 0.1 % headroom.
"""
import numpy as np

from oracle import search as oracle

DIM = 384
SIZES_N = (2048, 2049, 2079, 2080, 20011)
SIZES_NQ = (64, 65, 257)
SWEEP_M = (0, 40, 63, 70, 80, 100, 140)
FINITE_FAMILIES = ("unit", "anisotropic", "large_mean", "unnorm_first", "unnorm_last", "unnorm_split", "ties",
                   "zero_row", "outlier_row")


def tie(j, e=0):
    """midpoint between the bf16 neighbours (1 + j/128) 2^e and (1 + (j+1)/128) 2^e (tests/test_screened_gpu.py _tie)"""
    return np.float32((1.0 + (j + 0.5) / 128.0) * 2.0 ** e)


def _ties(rng, shape):
    j = rng.integers(0, 128, shape)
    e = rng.integers(-6, -2, shape)
    sign = rng.choice(np.array([-1.0, 1.0]), shape)
    return (sign * (1.0 + (j + 0.5) / 128.0) * 2.0 ** e).astype(np.float32)


def corpus_of(family: str, n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(1000 + seed)
    unit = oracle.seeded_unit_rows(n, DIM, 300 + seed)
    m = oracle.seeded_unit_rows(1, DIM, 301 + seed)[0]
    if family == "unit":
        c = unit
    elif family == "anisotropic":       # mean pairwise cosine 0.85^2 / (0.85^2 + 0.49^2) = 0.75
        c = 0.85 * m[None] + 0.49 * unit
        c /= np.linalg.norm(c, axis=1, keepdims=True)
    elif family == "large_mean":        # |c~| << |c|: fmaxf(cn, cb) and fl(c - mu) at work
        c = 30.0 * m[None] + unit
    elif family in ("unnorm_first", "unnorm_last"):
        c = unit * rng.uniform(0.1, 28.0, size=(n, 1))
        at = 0 if family == "unnorm_first" else n - 1    # n - 1: inside the partial last tile when n % 32 != 0
        c[at] = 30.0 * unit[at]
    elif family == "unnorm_split":
        # the row of the largest |c| is bf16-exact and the shard's mean is ~0, so its own |c~ - xc| is ~0: the largest
        # rounding error belongs to another row
        c = unit * rng.uniform(0.1, 28.0, size=(n, 1))
        a = oracle.bf16_round(unit[7]).astype(np.float64)
        a = oracle.bf16_round((a * (30.0 / np.linalg.norm(a))).astype(np.float32))
        a = (np.round(a.astype(np.float64) * 64) / 64).astype(np.float32)     # few significand bits: exact in bf16 and in sums
        a = oracle.bf16_round(a)
        ia, ib = n // 3, n // 3 + 1
        rest = np.ones(n, bool)
        rest[[ia, ib]] = False
        c[rest] -= c[rest].astype(np.float64).mean(0).astype(np.float32)[None]
        c[ia], c[ib] = a, -a
    elif family == "ties":
        # antisymmetric pairs: the column sums cancel, so centring leaves the ties (nearly) where they are
        half = _ties(rng, (n // 2, DIM))
        c = np.zeros((n, DIM), np.float32)
        c[0:2 * (n // 2):2], c[1:2 * (n // 2):2] = half, -half
    elif family == "zero_row":
        c = unit.copy()
        c[n // 2] = 0.0
        c[n - 1] = 0.0
    elif family == "outlier_row":
        c = unit.copy()
        c[n - 5] *= np.float32(1.0e6)
    else:
        raise KeyError(family)
    return np.ascontiguousarray(c, np.float32)


def queries_of(family: str, corpus: np.ndarray, nq: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(2000 + seed)
    n = corpus.shape[0]
    q = oracle.seeded_unit_rows(nq, DIM, 400 + seed)
    if family == "ties":
        q = _ties(rng, (nq, DIM))
        q[0, :] = tie(0)                        # every element rounds with the largest relative error bf16 has
        q[1, :192], q[1, 192:] = tie(0), tie(1)
    else:
        for i in range(0, nq, 5):               # planted neighbours: the top ranks are not noise
            r = corpus[(i * 131 + 3) % n]
            if np.linalg.norm(r) > 0:
                q[i] = r / np.linalg.norm(r) + 0.05 * q[i]
                q[i] /= np.linalg.norm(q[i])
    if family.startswith("unnorm"):
        q = q * rng.uniform(0.01, 100.0, size=(nq, 1))
    return np.ascontiguousarray(q, np.float32)


def sweep_queries(nq: int, seed: int = 0):
    """query i scaled by 2^-m, m = SWEEP_M[i % 7]: every scale several times in one batch"""
    q = oracle.seeded_unit_rows(nq, DIM, 500 + seed)
    m = np.array([SWEEP_M[i % len(SWEEP_M)] for i in range(nq)])
    return np.ascontiguousarray(q.astype(np.float64) * 2.0 ** -m[:, None].astype(np.float64), np.float32), m


# ---- fp32 emulation of the kernels (stand-in for the device on the CPU) ---------------------------------------------
def emulate_sidecar(corpus: np.ndarray):
    """What sskd_index_make_bf16 writes, up to summation order: (Sidecar, raw bytes)."""
    n = corpus.shape[0]
    colsum = corpus.sum(0, dtype=np.float32)
    ex = oracle.sidecar_expected(corpus, colsum)
    sq = lambda a: (a.astype(np.float32) ** 2).sum(1, dtype=np.float32).max()
    words = np.array([sq(corpus), sq(ex.ct), sq(ex.ct - ex.xc)], np.float32)
    raw = oracle.sidecar_encode(ex.ct, words, colsum, np.abs(corpus).max(), n)
    return oracle.sidecar_decode(raw, n), raw


def emulate_band(queries: np.ndarray, words) -> np.ndarray:
    """screen_setup_kernel's formula in fp32 (ordinary range only)."""
    q = np.ascontiguousarray(queries, np.float32)
    f = np.float32
    qn = np.sqrt((q * q).sum(1, dtype=f))
    d = oracle.bf16_round(q) - q
    qd = np.sqrt((d * d).sum(1, dtype=f))
    cn, cb, cd = np.sqrt(np.asarray(words, f))
    return (f(2.0) * (qd * cb + qn * cd + f(1.0e-4) * qn * max(cn, cb)) * f(1.0002) + f(1e-30)).astype(f)


# ---- the checks ------------------------------------------------------------------------------------------------------
def check_sidecar(corpus: np.ndarray, side: oracle.Sidecar, expected_words=None):
    """(a) tile values bit for bit and zero padding, (b) column sums, (c) norm words.  Returns the expectation."""
    n = corpus.shape[0]
    padded = -(-n // 32) * 32
    c64 = corpus.astype(np.float64)
    # (b)
    err = np.abs(side.colsum.astype(np.float64) - c64.sum(0))
    bound = padded * 2.0 ** -24 * np.abs(c64).sum(0)
    assert (err <= bound).all(), ("column sums", float((err - bound).max()))
    # (a): mu from the DEVICE's column sums makes the expectation exact whatever order the atomics took
    ex = oracle.sidecar_expected(corpus, side.colsum)
    assert side.tiles.shape == (padded, DIM)
    assert np.array_equal(side.tiles[:n].view(np.uint32), ex.ct.view(np.uint32)), "tile values differ from bf16(fl32(c - mu))"
    assert not side.tiles[n:].view(np.uint32).any(), "padding rows are not all-zero bits"
    # (c): from the decoded c~ and the test's xc
    want = oracle.row_norm2_max(corpus, ex.xc, side.tiles[:n]) if expected_words is None else expected_words
    got = side.words.astype(np.float64)
    rel = 400 * 2.0 ** -24
    assert (np.abs(got - want) <= rel * want).all(), ("norm words", got, want, np.abs(got - want) / np.maximum(want, 1e-300))
    assert float(side.absmax) == float(np.abs(corpus).max())
    return ex


def check_band(queries: np.ndarray, eps2: np.ndarray, words, terms=None):
    """(d) the formula, from both sides, and (f) the worst-case cap."""
    t = oracle.band_terms(queries, words) if terms is None else terms
    e64 = 2.0 * t.sum(1)
    eps = eps2.astype(np.float64)
    assert (eps >= e64).all(), ("band below its formula", float((eps / np.maximum(e64, 1e-300)).min()))
    assert (eps <= 1.0003 * e64 + 2e-30).all(), ("band inflated", float((eps / np.maximum(e64, 1e-300)).max()))
    qn = np.linalg.norm(queries.astype(np.float64), axis=1)
    cn, cb, _ = np.sqrt(np.asarray(words, np.float64))
    cap = 2 * (2.0 ** -7 * (1 + 2.0 ** -9) + 2e-4) * qn * max(cn, cb) * 1.001
    assert (eps <= cap).all(), ("band above the stated worst case", float((eps / np.maximum(cap, 1e-300)).max()))
    return eps / np.maximum(cap, 1e-300)


def soundness(queries, corpus, ex, eps2):
    """(e): per query, the largest left side over the live rows and the right side eps2 / 2 (fp64)."""
    q64 = queries.astype(np.float64)
    qt = oracle.bf16_round(queries).astype(np.float64)
    mu = ex.mu.astype(np.float64)
    screen = qt @ ex.ct.astype(np.float64).T
    true = q64 @ (corpus.astype(np.float64) - mu[None]).T
    w = oracle.row_norm2_max(corpus, ex.xc, ex.ct)
    allowance = oracle.SCREEN_ACC_NEEDED * np.linalg.norm(q64, axis=1) * np.sqrt(max(w[0], w[1]))
    lhs = np.abs(screen - true).max(1) + allowance
    return lhs, eps2.astype(np.float64) / 2.0, screen


def check_soundness(queries, corpus, ex, eps2, allow_inf=False):
    lhs, rhs, screen = soundness(queries, corpus, ex, eps2)
    ok = lhs <= rhs
    if allow_inf:
        ok |= np.isposinf(eps2)
    assert not np.isnan(eps2).any(), "NaN band"
    assert ok.all(), ("band narrower than the screening error", np.where(~ok)[0][:8], lhs[~ok][:8], rhs[~ok][:8])
    finite = np.isfinite(rhs) & (rhs > 0)
    return float((lhs[finite] / rhs[finite]).max()) if finite.any() else 0.0, screen


def check_candidates(screen64, eps2, ref_ids, k):
    """Every row of the exact top k has an fp64 screen score >= (k-th best fp64 screen score) - eps2."""
    kth = np.sort(screen64, axis=1)[:, -k]
    for q in range(screen64.shape[0]):
        if not np.isfinite(eps2[q]):
            continue
        got = screen64[q, ref_ids[q]]
        assert (got >= kth[q] - float(eps2[q])).all(), ("exact top-k row outside the candidate band", q)
