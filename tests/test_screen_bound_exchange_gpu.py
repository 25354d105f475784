"""The screening kernel's bound exchange: B buckets per query, the K-th largest of their maxima, one wave per exchange.

The workgroups of a query exchange a pruning bound through ``B = sskd_screen_bucket_count()`` words per query in global
memory: bucket ``row id mod B`` keeps the best screen score of its rows, and the exchanged bound is the 10th largest of
the B words (distinct buckets hold distinct rows, so ten words at or above ``v`` are ten distinct rows scoring at least
``v``).  What can go wrong:

* the selection returns a value ABOVE the true k-th largest - a "bound" above the k-th best score, rows of the top k
  pruned silently.  ``sskd_screen_bucket_bound`` runs the kernel's own load and selection over caller-given words and
  is held to ``numpy.partition`` with EQUALITY (never "at most": this is the only place a too-strong bound shows
  directly): random words, all empty, exactly k - 1 / k / k + 1 filled, all equal, duplicates across the k-th place,
  ``INT32_MAX`` and the images of negative scores; every k the hook serves;
* a bucket word that is not cleared between calls, or a bound taken from the wrong query / published to the wrong one:
  every whole search below runs on ONE workspace that starts as 0x7f bytes (an uncleared word is a huge bound) and is
  first used with the queries DOUBLED (every bucket then holds twice the score any row of the real call reaches: one
  stale word prunes everything); the real call follows, twice, and must return the same bits both times;
* rows lost at the edges of the rule: the ten best rows of a query all in ONE bucket (no global bound from them), in
  exactly ten buckets with two of them tied, twelve identical rows spread over the slices, rows in ascending order of
  their score, a mask that leaves fewer than k rows.

Whole searches are compared bit for bit with ``oracle.topk_fma`` - every query of the two small geometries; the
planted queries and a stride of the others on the large ones, where every query is besides held to the exact scan of
the library (itself held to the same oracle elsewhere) - with ``exact_fallback_queries`` printed.  Geometries whose plan
claims tiles run claimed; the others run through ``sskd_index_search_screened_claim`` both dealt and claimed.  No
tolerance anywhere.
"""
import numpy as np
import pytest
import torch

from capi_helpers import stream
from oracle import search as oracle
from semantic_search_kd_amd import _native
from test_screen_rolled_append_gpu import DIM, K, Run, base_corpus, oracle_rows, plan, unit

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


def ordered(x):
    """the kernel's monotone int32 image of a float32 score (float_to_ordered)"""
    b = np.asarray(x, np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF)).astype(np.int32)


def selection_cases(b, k, rng):
    rows = [rng.integers(INT_MIN, INT_MAX, (256, b), dtype=np.int64, endpoint=True)]            # random words
    sparse = rng.integers(INT_MIN, INT_MAX, (256, b), dtype=np.int64, endpoint=True)
    sparse[rng.random((256, b)) < 0.6] = INT_MIN                                                # random, mostly empty
    rows.append(sparse)
    rows.append(np.full((1, b), INT_MIN, np.int64))                                             # all empty
    for filled in (k - 1, k, k + 1):                                                            # exactly k - 1, k, k + 1 filled
        for _ in range(8):
            r = np.full(b, INT_MIN, np.int64)
            r[rng.permutation(b)[:filled]] = rng.integers(INT_MIN + 1, INT_MAX, filled, endpoint=True)
            rows.append(r[None])
    for v in (INT_MIN, INT_MIN + 1, -1, 0, 7, INT_MAX):                                         # all equal
        rows.append(np.full((1, b), v, np.int64))
    for lo, hi in ((k - 2, k), (k - 1, k + 1), (0, k), (k - 1, b), (0, b - 1)):                 # duplicates across the k-th place
        for _ in range(4):
            r = np.sort(rng.integers(-1000, 1000, b))[::-1].copy()
            r[max(lo, 0):hi] = r[max(lo, 0)]
            rows.append(rng.permutation(r)[None])
    scores = np.concatenate([-np.abs(rng.standard_normal((32, b))), rng.standard_normal((32, b))]).astype(np.float32)
    scores[:, :3] = [-0.0, 0.0, -np.inf]
    img = ordered(scores).astype(np.int64)                                                      # negative-score images
    img[::4, rng.integers(0, b)] = INT_MAX
    img[1::4, : k + 1] = INT_MAX                                                                # INT32_MAX, more than k of them
    rows.append(img)
    return np.concatenate(rows).astype(np.int32)


def test_bucket_bound_is_the_kth_largest(gpu, native_lib):
    lib = native_lib
    b = lib.sskd_screen_bucket_count()
    assert b >= 10 and b & (b - 1) == 0
    rng = np.random.default_rng(3210)
    for k in range(1, 11):
        words = selection_cases(b, k, rng)
        nq = words.shape[0]
        d_in = torch.from_numpy(words).cuda()
        d_out = torch.full((nq,), 12345, dtype=torch.int32, device="cuda")
        _native.check(lib.sskd_screen_bucket_bound(d_in.data_ptr(), nq, k, d_out.data_ptr(), stream()))
        torch.cuda.synchronize()
        want = np.partition(words, b - k, axis=1)[:, b - k]
        got = d_out.cpu().numpy()
        assert np.array_equal(got, want), (k, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    assert lib.sskd_screen_bucket_bound(None, 4, 10, None, stream()) == 1
    assert lib.sskd_screen_bucket_bound(d_in.data_ptr(), 4, 0, d_out.data_ptr(), stream()) == 1
    assert lib.sskd_screen_bucket_bound(d_in.data_ptr(), 4, 11, d_out.data_ptr(), stream()) == 1
    assert lib.sskd_screen_bucket_bound(None, 0, 10, None, stream()) == 0


class SharedWorkspaceRun(Run):
    """Every screened call of a case on ONE workspace: poisoned at first, then used once with the queries doubled."""

    def __init__(self, lib, corpus, queries, allowed=None):
        super().__init__(lib, corpus, queries, allowed)
        need = int(lib.sskd_index_search_screened_workspace_bytes(self.n, self.nq, K))
        assert need > 0
        self.ws = torch.full((need,), 0x7F, dtype=torch.uint8, device="cuda")
        self.q_real = self.q
        self.q = 2.0 * self.q_real
        self.screened(-1)
        self.q = self.q_real

    def screened(self, claim):
        out_s, out_i = self._out()
        status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        _native.check(self.lib.sskd_index_search_screened_claim(
            self.tiled.data_ptr(), self.bf.data_ptr(), self.n, self.q.data_ptr(), self.nq, K, 0,
            None if self.mask is None else self.mask.data_ptr(), int(claim), out_s.data_ptr(), out_i.data_ptr(),
            status.data_ptr(), self.ws.data_ptr(), self.ws.numel(), stream(), None, None))
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        assert st[0] == 0, st
        return out_s.cpu().numpy(), out_i.cpu().numpy(), int(st[1])


def claims_to_run(claimed):
    return (1,) if claimed else (0, 1)


def check_search(lib, corpus, queries, claimed, oracle_queries, allowed=None, what=""):
    """twice per tile order on one workspace: the same bits, the oracle's on ``oracle_queries``, the exact scan's on all"""
    run = SharedWorkspaceRun(lib, corpus, queries, allowed)
    sel = sorted(set(oracle_queries))
    ref_s, ref_i = oracle_rows(queries[sel], corpus, allowed)
    want = run.exact()
    got = None
    for claim in claims_to_run(claimed):
        for again in (0, 1):
            got_s, got_i, fallback = run.screened(claim)
            print(f"{what} rows {corpus.shape[0]} queries {queries.shape[0]} claim {claim} call {again + 1}: "
                  f"exact_fallback_queries {fallback}")
            assert np.array_equal(got_i[sel], ref_i), [sel[j] for j in np.flatnonzero((got_i[sel] != ref_i).any(1))[:8]]
            assert np.array_equal(got_s[sel], ref_s)
            assert np.array_equal(got_i, want[1]), np.argwhere(got_i != want[1])[:5]
            assert np.array_equal(got_s, want[0])
            got = got_i
    return got


def stride(nq, parts=16):
    return list(range(0, nq, max(1, nq // parts)))


# (nq, n_rows, queries per block, claimed by the plan, every query on the oracle)
PLAIN = [
    (127, 2_049, 64, False, True),        # 64 per block, LIGHT, many short slices
    (383, 4_099, 128, False, True),       # 128 per block, LIGHT
    (16_479, 32_771, 160, True, False),   # 160 per block, LIGHT, 2 slices
    (20_000, 254_017, 160, True, False),  # the bench kernel: 125 blocks x 2 slices
]


@pytest.mark.parametrize("nq,n,qpb,claimed,whole", PLAIN)
def test_search_matches_the_oracle(gpu, native_lib, nq, n, qpb, claimed, whole):
    assert plan(native_lib, n, nq)[0] == qpb and plan(native_lib, n, nq)[3] == claimed
    corpus = base_corpus()[:n]
    queries = oracle.seeded_unit_rows(nq, DIM, 8100 + nq)
    near = np.arange(0, nq, 5)                                   # every fifth query sits next to a corpus row
    queries[near] = corpus[(near * 37) % n] + np.float32(0.05) * queries[near]
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    check_search(native_lib, corpus, queries, claimed, range(nq) if whole else stride(nq) + list(near[:: max(1, len(near) // 8)]))


def test_search_with_row_mask(gpu, native_lib):
    nq, n = 256, 6_007
    assert plan(native_lib, n, nq)[0] == 128 and not plan(native_lib, n, nq)[3]
    corpus = base_corpus()[:n]
    queries = oracle.seeded_unit_rows(nq, DIM, 8400)
    allowed = np.ones(n, bool)
    allowed[::7] = False
    allowed[32 * 11: 32 * 12] = False                            # a whole tile
    allowed[32 * 40: 32 * 40 + 16] = False                       # half of one
    allowed[-5:] = False
    got_i = check_search(native_lib, corpus, queries, False, range(nq), allowed, "masked")
    assert allowed[got_i].all()


def planted_buckets(n, nq, b, seed):
    """three planted queries: ten best rows in ONE bucket; in exactly ten buckets, two tied; twelve identical rows"""
    corpus = np.array(base_corpus()[:n])
    queries = oracle.seeded_unit_rows(nq, DIM, seed)
    rng = np.random.default_rng(seed + 1)
    vec = lambda: unit(rng.standard_normal(DIM))
    qa, qb, qc = 3, nq // 2, nq - 1
    spread = lambda count, residue: [b * ((i * (n // b - 1)) // count) + residue for i in range(count)]
    expect = {}
    u = vec()                                                    # one bucket: ids = 0 mod B, spread over the slices
    ids = spread(10, 0)
    queries[qa] = u
    for j, row in enumerate(ids):
        corpus[row] = unit(u + np.float32(0.02 * (j + 1)) * vec())
    expect[qa] = ids
    u = vec()                                                    # ten buckets (residues 1..10), the fourth and fifth row tied
    ids = [row + j for j, row in enumerate(spread(10, 1))]
    queries[qb] = u
    for j, row in enumerate(ids):
        corpus[row] = unit(u + np.float32(0.02 * (j + 1)) * vec())
    corpus[ids[4]] = corpus[ids[3]]
    expect[qb] = ids
    u = vec()                                                    # identical rows in different slices (residue 11)
    ids = spread(12, 11)
    queries[qc] = u
    corpus[ids] = unit(u + np.float32(0.02) * vec())
    expect[qc] = ids[:10]
    flat = [r for rows in (spread(10, 0), [row + j for j, row in enumerate(spread(10, 1))], spread(12, 11)) for r in rows]
    assert len(set(flat)) == 32 and max(flat) < n
    return corpus, queries, expect


GEOMETRIES = [(383, 4_099, 128, False), (16_479, 32_771, 160, True)]


@pytest.mark.parametrize("nq,n,qpb,claimed", GEOMETRIES)
def test_planted_buckets(gpu, native_lib, nq, n, qpb, claimed):
    assert plan(native_lib, n, nq)[0] == qpb and plan(native_lib, n, nq)[3] == claimed
    b = native_lib.sskd_screen_bucket_count()
    corpus, queries, expect = planted_buckets(n, nq, b, 8500 + nq)
    got_i = check_search(native_lib, corpus, queries, claimed, list(expect) + stride(nq), None, "planted buckets")
    for q, rows in expect.items():
        assert list(got_i[q]) == rows, (q, got_i[q], rows)
        assert len({r % b for r in rows}) in (1, 10)


@pytest.mark.parametrize("nq,n,qpb,claimed", GEOMETRIES)
def test_ascending_rows(gpu, native_lib, nq, n, qpb, claimed):
    """rows in ascending order of their score for query 0: the bound trails the rows, every exchange publishes a new one"""
    corpus = base_corpus()[:n]
    queries = oracle.seeded_unit_rows(nq, DIM, 8600 + nq)
    order = np.argsort(corpus.astype(np.float64) @ queries[0].astype(np.float64), kind="stable")
    corpus = np.ascontiguousarray(corpus[order])
    got_i = check_search(native_lib, corpus, queries, claimed, [0] + stride(nq), None, "ascending")
    assert got_i[0, 0] == n - 1 and (got_i[0] >= n - 2 * K).all()   # (fp64 order of the sort, fp32 order of the result)


@pytest.mark.parametrize("nq,n,qpb,claimed", GEOMETRIES)
def test_mask_leaves_fewer_than_k_rows(gpu, native_lib, nq, n, qpb, claimed):
    corpus = base_corpus()[:n]
    queries = oracle.seeded_unit_rows(nq, DIM, 8700 + nq)
    keep = np.array([5, 32 * 9 + 31, n // 3, n // 2 + 1, n - 40, n - 33, n - 1])
    allowed = np.zeros(n, bool)
    allowed[keep] = True
    run = SharedWorkspaceRun(native_lib, corpus, queries, allowed)
    want = run.exact()
    sel = stride(nq)
    sc = oracle.scores_fma(queries[sel], np.ascontiguousarray(corpus[keep]))
    for claim in claims_to_run(claimed):
        for again in (0, 1):
            got_s, got_i, fallback = run.screened(claim)
            print(f"seven allowed rows, rows {n} queries {nq} claim {claim} call {again + 1}: exact_fallback_queries {fallback}")
            assert np.array_equal(got_i, want[1]) and np.array_equal(got_s, want[0])
            assert (got_i[:, 7:] == -1).all() and (np.sort(got_i[:, :7], axis=1) == keep).all()
            for j, q in enumerate(sel):
                rank = sorted(range(7), key=lambda r: (-sc[j, r], keep[r]))
                assert list(got_i[q, :7]) == list(keep[rank]) and np.array_equal(got_s[q, :7], sc[j, rank])
