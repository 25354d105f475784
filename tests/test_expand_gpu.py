"""The two expansion kernels on the MI355X against the checker (``expand_cases``), through the C-ABI: the same bits for
every query.

Rocchio runs over seeded unit rows (1 000 and 1 003 of them) with rankings the exact search wrote and hand-made ones.
RM3 runs over the reference test's five sentences, a Zipf corpus and hand-made corpora for the table's worst case, the
256-term cut, ties and masks; the CSR it writes goes back into ``sskd_bm25_search`` and must score as the checker's
expanded token list does.
"""
import numpy as np
import pytest
import torch

import bm25_cases as bc
import expand_cases as ec
import ranking_walk_cases as rw
from capi_helpers import capi_search, stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import BM25Index, _native
from semantic_search_kd_amd.expand import expanded_lims

pytestmark = pytest.mark.gpu

WEIGHTING = {"uniform": 0, "score": 1}


# ---------------------------------------------------------------------------------------------------- Rocchio
def capi_rocchio(lib, tiled, n_rows, Q, S, I, *, fb_docs, alpha, beta, weighting):
    nq, kd = I.shape
    d_q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    d_s = torch.from_numpy(np.ascontiguousarray(S, np.float32)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(I, np.int64)).cuda()
    out = torch.full((max(nq, 1), 384), float("nan"), dtype=torch.float32, device="cuda")[:nq]
    counts = torch.full((max(nq, 1),), -7, dtype=torch.int32, device="cuda")[:nq]
    _native.check(lib.sskd_prf_rocchio(tiled.data_ptr(), n_rows, d_q.data_ptr(), nq, d_s.data_ptr(), d_i.data_ptr(), kd,
                                       fb_docs, alpha, beta, WEIGHTING[weighting], out.data_ptr(), counts.data_ptr(),
                                       stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), counts.cpu().numpy()


def _same_rocchio(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: counts {got[1]} != {want[1]}"
    assert np.array_equal(ec.bits32(got[0]), ec.bits32(want[0])), f"{what}: query bits differ"


class DenseWorld:
    def __init__(self, lib, n, seed):
        self.n = n
        self.rows = oracle.seeded_unit_rows(n, 384, seed)
        self.tiled = tile_corpus(lib, self.rows)
        self.queries = oracle.seeded_unit_rows(65, 384, seed + 1)
        self.S, self.I = capi_search(lib, self.tiled, n, self.queries, 19)


@pytest.fixture(scope="module")
def dense_worlds(native_lib, gpu):
    return {n: DenseWorld(native_lib, n, 40 + n) for n in (1000, 1003)}


@pytest.mark.parametrize("n", [1000, 1003])
def test_rocchio_equals_the_checker(native_lib, dense_worlds, n):
    w = dense_worlds[n]
    S, I = w.S.copy(), w.I.copy()
    if n == 1003:   # the last row, in a tile that is not full, among the feedback
        for q in range(65):
            if 1002 not in I[q, :1]:
                I[q, 0] = 1002
    for nq in (1, 3, 65):
        for fb_docs in (1, 5, 16):
            for kd in (fb_docs, fb_docs + 3):
                for weighting in ("uniform", "score"):
                    kw = dict(fb_docs=fb_docs, alpha=1.0, beta=0.75, weighting=weighting)
                    got = capi_rocchio(native_lib, w.tiled, n, w.queries[:nq], S[:nq, :kd], I[:nq, :kd], **kw)
                    want = ec.rocchio_batch(w.queries[:nq], S[:nq, :kd], I[:nq, :kd], w.rows, **kw)
                    _same_rocchio(got, want, f"n={n} nq={nq} fb_docs={fb_docs} kd={kd} {weighting}")
                    assert (want[1] == fb_docs).all()
    assert (I[:, 0] == 1002).all() if n == 1003 else True


def test_rocchio_on_hand_made_rankings(native_lib, dense_worlds):
    w = dense_worlds[1003]
    n, kd = w.n, 8
    g = np.random.default_rng(7)
    nq = 7
    I = np.stack([g.permutation(n)[:kd] for _ in range(nq)]).astype(np.int64)
    S = -np.sort(-g.standard_normal((nq, kd)).astype(np.float32), axis=1)
    S[:, :3] = np.abs(S[:, :3]) + 0.1
    I[0, 2:] = -1                      # padded after two entries ...
    I[0, 4:6] = [5, 6]                 # ... rows behind the padding are never read
    I[1, :] = -1                       # all padding: the query comes back
    I[2, 2] = n                        # ids outside the index in the middle: skipped
    I[2, 3] = n + 12345
    I[2, 4] = -5                       # negative but not the padding id: skipped, the walk goes on
    S[3, :] = -np.abs(S[3, :])         # every score <= 0: the score weighting falls back to uniform
    S[3, 1] = 0.0
    S[4, 0] = -0.0
    S[5, 2:] = -1.0                    # positive and negative scores mixed
    Q = w.queries[:nq]
    for weighting in ("uniform", "score"):
        for fb_docs in (1, 5, 8):
            for alpha, beta in ((1.0, 0.75), (0.0, 1.0), (0.5, 0.0), (2.5, 0.3)):
                kw = dict(fb_docs=fb_docs, alpha=alpha, beta=beta, weighting=weighting)
                got = capi_rocchio(native_lib, w.tiled, n, Q, S, I, **kw)
                want = ec.rocchio_batch(Q, S, I, w.rows, **kw)
                _same_rocchio(got, want, f"hand-made fb_docs={fb_docs} {weighting} alpha={alpha} beta={beta}")
                assert np.array_equal(ec.bits32(got[0][1]), ec.bits32(Q[1]))     # m == 0: the input bits, whatever alpha
    assert want[1].tolist() == [2, 0, 5, 8, 8, 8, 8]
    # all scores <= 0 under "score" is the uniform result
    a = capi_rocchio(native_lib, w.tiled, n, Q[3:4], S[3:4], I[3:4], fb_docs=8, alpha=1.0, beta=0.75, weighting="score")
    b = capi_rocchio(native_lib, w.tiled, n, Q[3:4], S[3:4], I[3:4], fb_docs=8, alpha=1.0, beta=0.75, weighting="uniform")
    assert np.array_equal(ec.bits32(a[0]), ec.bits32(b[0]))
    # no queries: nothing is written, nothing fails
    out, counts = capi_rocchio(native_lib, w.tiled, n, Q[:0], S[:0], I[:0], fb_docs=5, alpha=1.0, beta=0.75,
                               weighting="uniform")
    assert out.shape == (0, 384) and counts.shape == (0,)


@pytest.mark.parametrize("width", rw.WIDTHS)
def test_rocchio_walk_at_the_round_boundaries(native_lib, dense_worlds, width):
    """The shared hand-made rankings over the first 200 rows: the first -1 at rank 0, 63, 64 and absent, rows behind
    it, ids outside the index and -9 before it (skipped: the walk goes on); ``fb_docs`` on both sides of the round."""
    w, n = dense_worlds[1003], 200
    I = rw.ids(n, width)
    S = rw.descending_scores(width, low=-0.2, high=0.9)
    Q = w.queries[:rw.NQ]
    end = rw.first_pad(I)
    for fb_docs in sorted({1, min(63, width), min(64, width), min(65, width), width}):
        for weighting in ("uniform", "score"):
            kw = dict(fb_docs=fb_docs, alpha=1.0, beta=0.75, weighting=weighting)
            got = capi_rocchio(native_lib, w.tiled, n, Q, S, I, **kw)
            want = ec.rocchio_batch(Q, S, I, w.rows[:n], **kw)
            _same_rocchio(got, want, f"walk width={width} fb_docs={fb_docs} {weighting}")
        kept = [int(((I[q, :min(end[q], fb_docs)] >= 0) & (I[q, :min(end[q], fb_docs)] < n)).sum()) for q in range(rw.NQ)]
        assert want[1].tolist() == kept
    if width >= 63:
        assert kept[4] == width - 1 and kept[0] == 0, "-9 is skipped and the walk goes on; a -1 at rank 0 ends it"


# ---------------------------------------------------------------------------------------------------- RM3
def mask_words(allowed):
    bits = np.zeros(-(-len(allowed) // 32) * 32, np.uint8)
    bits[: len(allowed)] = np.asarray(allowed, np.uint8)
    return torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy()).cuda()


class LexWorld:
    def __init__(self, texts, gpu):
        self.texts = texts
        self.lex = ec.Lexicon([bc.tokenize(t) for t in texts])
        self.index = BM25Index(device=str(gpu))
        self.index.build_from_texts([f"d{i}" for i in range(len(texts))], texts)
        self.n = len(texts)

    def ranking(self, queries, kb):
        b, j = self.index.search_device(queries, kb)
        return b.cpu().numpy(), j.cpu().numpy()

    def rm3(self, lib, queries, B, J, *, fb_docs, fb_terms, orig_repeat, max_df=0, allowed=None):
        """``sskd_prf_rm3`` on host rankings: ``(segments, sel_terms, sel_w, counts, fb, csr)``."""
        idx, post = self.index, self.index.bm25
        _, offsets, _, _, _ = idx._tables()
        fwd_lims, fwd_terms, fwd_p, n_fwd = idx.forward_tables()
        d_lims, d_terms, lims = idx.query_csr_host(queries)
        nq, kb = J.shape
        d_b = torch.from_numpy(np.ascontiguousarray(B, np.float64)).cuda()
        d_j = torch.from_numpy(np.ascontiguousarray(J, np.int64)).cuda()
        out_lims = expanded_lims(lims, orig_repeat, fb_terms)
        d_out_lims = torch.from_numpy(out_lims).cuda()
        out_terms = torch.full((int(out_lims[-1]) + 8,), -7, dtype=torch.int32, device="cuda")
        sel_t = torch.full((nq, fb_terms), -7, dtype=torch.int32, device="cuda")
        sel_w = torch.full((nq, fb_terms), 7.0, dtype=torch.float64, device="cuda")
        counts = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        fb = torch.full((nq,), -7, dtype=torch.int32, device="cuda")
        mask = None if allowed is None else mask_words(allowed)
        _native.check(lib.sskd_prf_rm3(
            fwd_lims.data_ptr(), fwd_terms.data_ptr(), fwd_p.data_ptr(), n_fwd, offsets.data_ptr(), post.corpus_size,
            post.n_terms, lims.ctypes.data, d_lims.data_ptr(), d_terms.data_ptr(), d_b.data_ptr(), d_j.data_ptr(), kb,
            None if mask is None else mask.data_ptr(), nq, fb_docs, fb_terms, orig_repeat, max_df,
            out_lims.ctypes.data, d_out_lims.data_ptr(), out_terms.data_ptr(), sel_t.data_ptr(), sel_w.data_ptr(),
            counts.data_ptr(), fb.data_ptr(), stream()))
        torch.cuda.synchronize()
        flat = out_terms.cpu().numpy()
        assert (flat[int(out_lims[-1]):] == -7).all()          # nothing behind the last segment was touched
        segments = [flat[out_lims[q]:out_lims[q + 1]].tolist() for q in range(nq)]
        return segments, sel_t.cpu().numpy(), sel_w.cpu().numpy(), counts.cpu().numpy(), fb.cpu().numpy(), \
            (d_out_lims, out_terms)

    def check(self, lib, queries, *, kb, fb_docs, fb_terms, orig_repeat, max_df=0, allowed=None, ranking=None, what=""):
        """The kernel against the checker for every query, then the written CSR through ``sskd_bm25_search`` against
        the checker's search of the expanded token list.  Returns the checker's selections."""
        lex = self.lex
        B, J = self.ranking(queries, kb) if ranking is None else ranking
        segments, sel_t, sel_w, counts, fb, csr = self.rm3(lib, queries, B, J, fb_docs=fb_docs, fb_terms=fb_terms,
                                                           orig_repeat=orig_repeat, max_df=max_df, allowed=allowed)
        k = min(20, self.n)
        again_s, again_i = (t.cpu().numpy() for t in self.index._search_csr(csr, len(queries), k))
        chosen_all = []
        for q, text in enumerate(queries):
            tokens = bc.tokenize(text)
            chosen, weights, n_fb = lex.select(tokens, B[q], J[q], fb_docs=fb_docs, fb_terms=fb_terms, max_df=max_df,
                                               allowed=allowed)
            tag = f"{what} query {q} ({text[:30]!r}) fb_docs={fb_docs} fb_terms={fb_terms} repeat={orig_repeat}"
            assert fb[q] == n_fb and counts[q] == len(chosen), tag
            pad = fb_terms - len(chosen)
            assert sel_t[q].tolist() == chosen + [-1] * pad, tag
            assert ec.bits64(sel_w[q]).tolist() == ec.bits64(np.array(weights + [0.0] * pad)).tolist(), tag
            assert segments[q] == lex.segment(tokens, chosen, fb_terms=fb_terms, orig_repeat=orig_repeat), tag
            rows, scores = lex.oracle.rank(lex.oracle.scores(lex.expanded_tokens(tokens, chosen, orig_repeat=orig_repeat)), k)
            assert again_i[q].tolist() == rows, tag
            assert ec.bits64(again_s[q]).tolist() == ec.bits64(np.array(scores)).tolist(), tag
            chosen_all.append(chosen)
        return chosen_all


@pytest.fixture(scope="module")
def five(gpu):
    return LexWorld(bc.FIVE_SENTENCES, gpu)


@pytest.fixture(scope="module")
def zipf(gpu):
    return LexWorld(bc.zipf_corpus(600, 300, 3), gpu)


def test_rm3_five_sentences(native_lib, five):
    chosen = five.check(native_lib, ["learning"], kb=5, fb_docs=5, fb_terms=10, orig_repeat=2, what="five")
    B, _ = five.ranking(["learning"], 5)
    assert (B[0] != 0.0).sum() == 3 and (B[0][3:] == 0.0).all()       # a ranking whose tail scores 0.0: not feedback
    words = [five.lex.words[t] for t in chosen[0]]
    assert len(words) == 10 and "learning" not in words and "machine" in words
    # fewer candidates than fb_terms: -1 padding
    chosen = five.check(native_lib, ["learning"], kb=5, fb_docs=1, fb_terms=64, orig_repeat=1, what="five, one row")
    assert 0 < len(chosen[0]) < 64
    # kb == fb_docs == 1, and a query nothing matches
    five.check(native_lib, ["learning", "zzz"], kb=1, fb_docs=1, fb_terms=1, orig_repeat=3, what="five, kb 1")


def _zipf_queries(world):
    lex = world.lex
    by_df = sorted(lex.words, key=lambda w: len(lex.oracle.postings[w]))
    rare, common = by_df[0], by_df[-1]
    return [bc.zipf_query(300, 1, 101), bc.zipf_query(300, 3, 102), bc.zipf_query(300, 40, 103), "",
            f"{common} {rare} {common} {common}", f"{rare} not-a-word {common}", rare]


def test_rm3_zipf_sweep(native_lib, zipf):
    queries = _zipf_queries(zipf)
    for fb_docs in (1, 5, 16):
        for fb_terms in (1, 10, 64):
            for orig_repeat in (1, 3):
                for kb in sorted({fb_docs, 16}):
                    zipf.check(native_lib, queries, kb=kb, fb_docs=fb_docs, fb_terms=fb_terms, orig_repeat=orig_repeat,
                               what=f"zipf kb={kb}")
    # one query at a time gives what the batch gives (the checker is per query; this is the launch geometry)
    zipf.check(native_lib, queries[2:3], kb=16, fb_docs=5, fb_terms=10, orig_repeat=2, what="zipf alone")


def test_rm3_max_df_and_masks(native_lib, zipf):
    queries = _zipf_queries(zipf)
    lex = zipf.lex
    # max_df = 1 excludes almost everything; max_df = rows / 4 is the default of the host layer
    chosen = zipf.check(native_lib, queries, kb=16, fb_docs=5, fb_terms=10, orig_repeat=2, max_df=1, what="max_df=1")
    assert all(lex.df(t) == 1 for c in chosen for t in c) and any(len(c) < 10 for c in chosen)
    zipf.check(native_lib, queries, kb=16, fb_docs=5, fb_terms=10, orig_repeat=2, max_df=zipf.n // 4, what="max_df=n/4")
    # a mask that hides the two best rows of every query (and every third row besides)
    B, J = zipf.ranking(queries, 32)
    allowed = np.ones(zipf.n, bool)
    allowed[::3] = False
    for q in range(len(queries)):
        allowed[J[q, :2][J[q, :2] >= 0]] = False
    plain = zipf.check(native_lib, queries, kb=32, fb_docs=5, fb_terms=10, orig_repeat=2, ranking=(B, J), what="no mask")
    masked = zipf.check(native_lib, queries, kb=32, fb_docs=5, fb_terms=10, orig_repeat=2, ranking=(B, J),
                        allowed=allowed.tolist(), what="masked")
    assert plain != masked
    # hand-made rankings: ids outside the index, padding in the middle, zeros of either sign, a list that is all padding
    g = np.random.default_rng(11)
    nq, kb = len(queries), 12
    J2 = np.stack([g.permutation(zipf.n)[:kb] for _ in range(nq)]).astype(np.int64)
    B2 = -np.sort(-g.uniform(0.5, 9.0, (nq, kb)), axis=1)
    J2[0, [1, 3]] = [zipf.n, -9]
    J2[1, 4:] = -1
    J2[1, 6:8] = [3, 4]
    B2[2, 2] = 0.0
    B2[2, 3] = -0.0
    J2[3, :] = -1
    B2[3, :] = -np.inf
    zipf.check(native_lib, queries, kb=kb, fb_docs=5, fb_terms=10, orig_repeat=2, ranking=(B2, J2), what="hand-made")


@pytest.fixture(scope="module")
def zipf200(gpu):
    return LexWorld(bc.zipf_corpus(200, 300, 5), gpu)


@pytest.mark.parametrize("width", rw.WIDTHS)
def test_rm3_walk_at_the_round_boundaries(native_lib, zipf200, width):
    """The shared hand-made rankings as BM25 rankings over 200 rows.  Ranks 3 .. 59 score 0.0 (no feedback), so round one
    leaves fewer than ``fb_docs`` = 16 survivors and the walk enters round two; it stops once 16 are found."""
    world, n = zipf200, 200
    queries = [bc.zipf_query(300, 1 + q, 120 + q) for q in range(rw.NQ)]
    J = rw.ids(n, width)
    B = rw.descending_scores(width, np.float64).copy()
    B[:, 3:60] = 0.0
    B[4, min(1, width - 1)] = -0.0
    allowed = np.ones(n, bool)
    allowed[::7] = False
    fb_docs = min(16, width)
    end = rw.first_pad(J)
    for a in (None, allowed.tolist()):
        world.check(native_lib, queries, kb=width, fb_docs=fb_docs, fb_terms=10, orig_repeat=2, ranking=(B, J),
                    allowed=a, what=f"walk width={width} mask={a is not None}")
    kept = [int(((J[q, :end[q]] >= 0) & (J[q, :end[q]] < n) & (B[q, :end[q]] != 0.0)).sum()) for q in range(rw.NQ)]
    fb = [len(world.lex.feedback(B[q], J[q], fb_docs)) for q in range(rw.NQ)]
    assert fb == [min(c, fb_docs) for c in kept]
    if width == 130:
        assert kept[:3] == [0, 4, 5] and fb[3] == 16 and kept[3] > 64, (kept, fb)


def _worst_case_texts():
    """16 rows of 256 distinct words twice each plus the shared query word once at the end: the cut keeps the 256 and
    drops the query word, so the table takes 16 x 256 = 4 096 disjoint candidates.  Row r repeats its first word r more
    times, so the rows differ in length and score.  40 short rows of other words around them."""
    big = []
    for r in range(16):
        own = [f"u{r}_{i}" for i in range(256)]
        big.append(" ".join(own + own + [own[0]] * r + ["zq"]))
    return bc.zipf_corpus(20, 50, 8) + big + bc.zipf_corpus(20, 50, 9)


def test_rm3_table_worst_case(native_lib, gpu):
    w = LexWorld(_worst_case_texts(), gpu)
    lex = w.lex
    rows, _ = lex.oracle.search("zq", 16)
    assert sorted(rows) == list(range(20, 36))
    assert sum(len(lex.fwd[r]) for r in rows) == 4096 and len(set().union(*(lex.fwd[r] for r in rows))) == 4096
    assert all(lex.term_id["zq"] not in lex.fwd[r] for r in rows)
    for fb_terms in (1, 64):
        chosen = w.check(native_lib, ["zq", "zq w0"], kb=16, fb_docs=16, fb_terms=fb_terms, orig_repeat=1, what="worst case")
        assert len(chosen[0]) == fb_terms
    # within one row the words weigh the same: the term id decides
    chosen = w.check(native_lib, ["zq"], kb=16, fb_docs=1, fb_terms=64, orig_repeat=2, what="worst case, one row")
    assert chosen[0][1:] == sorted(chosen[0][1:])


def test_rm3_cut_row_and_identical_rows(native_lib, gpu):
    long_row = " ".join(["zc"] + [f"v{i}" for i in range(400)])
    twin = "zc alpha beta gamma delta alpha"
    texts = bc.zipf_corpus(30, 40, 4) + [long_row, twin, twin] + bc.zipf_corpus(10, 40, 5)
    w = LexWorld(texts, gpu)
    lex = w.lex
    assert len(lex.tf[30]) == 401 and len(lex.fwd[30]) == 256
    chosen = w.check(native_lib, ["zc"], kb=8, fb_docs=3, fb_terms=64, orig_repeat=2, what="cut row")
    assert any(t in lex.fwd[30] for t in chosen[0])
    assert not any(lex.words[t] in {f"v{i}" for i in range(300, 400)} for t in chosen[0])   # cut from the row
    # the twins give beta, gamma and delta the same weight: ascending term ids
    chosen = w.check(native_lib, ["zc"], kb=8, fb_docs=2, fb_terms=4, orig_repeat=1, what="twins")
    names = [lex.words[t] for t in chosen[0]]
    assert names == ["alpha", "beta", "gamma", "delta"]


def test_rm3_no_queries(native_lib, five):
    idx = five.index
    _, offsets, _, _, _ = idx._tables()
    fwd_lims, fwd_terms, fwd_p, n_fwd = idx.forward_tables()
    rc = native_lib.sskd_prf_rm3(fwd_lims.data_ptr(), fwd_terms.data_ptr(), fwd_p.data_ptr(), n_fwd, offsets.data_ptr(),
                                 5, idx.bm25.n_terms, None, None, None, None, None, 5, None, 0, 5, 10, 2, 0, None, None,
                                 None, None, None, None, None, stream())
    assert rc == 0


# ---------------------------------------------------------------------------------------------------- bad arguments
P = 4096   # a non-null, 16-byte aligned "pointer": every check comes before the launch, nothing is read


def _rocchio_call(lib, **over):
    a = dict(d_tiled=P, n_rows=100, d_queries=P, nq=1, d_rank_scores=P, d_rank_ids=P, kd=10, fb_docs=5, alpha=1.0,
             beta=0.75, weighting=0, d_out_queries=P + 4096, d_out_counts=P, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return lib.sskd_prf_rocchio(*a.values()), lib.sskd_last_error().decode()


@pytest.mark.parametrize("over, names", [
    (dict(fb_docs=0), "fb_docs=0"),
    (dict(fb_docs=11), "fb_docs=11"),
    (dict(kd=1025, fb_docs=1025), "kd=1025"),
    (dict(kd=0, fb_docs=0), "kd=0"),
    (dict(alpha=-0.5), "alpha"),
    (dict(alpha=float("nan")), "alpha"),
    (dict(alpha=float("inf")), "alpha"),
    (dict(beta=-1.0), "beta"),
    (dict(beta=float("inf")), "beta"),
    (dict(weighting=2), "weighting=2"),
    (dict(weighting=-1), "weighting=-1"),
    (dict(n_rows=-1), "n_rows"),
    (dict(n_rows=(1 << 31) - 64), "n_rows"),
    (dict(nq=-1), "nq"),
    (dict(d_queries=None), "null"),
    (dict(d_rank_ids=None), "null"),
    (dict(d_out_counts=None), "null"),
    (dict(d_tiled=None), "null index"),
    (dict(d_tiled=P + 8), "16-byte aligned"),
    (dict(d_queries=P + 4), "16-byte aligned"),
    (dict(d_out_queries=P + 4096 + 8), "16-byte aligned"),
    (dict(d_out_queries=P), "alias"),
    (dict(d_out_queries=P + 1520), "alias"),
    (dict(nq=2, d_out_queries=P + 1536), "alias"),
])
def test_rocchio_refuses_invalid_arguments_before_the_launch(native_lib, over, names):
    rc, message = _rocchio_call(native_lib, **over)
    assert rc == 1, (rc, message)
    assert message.startswith("prf_rocchio:") and names in message, message


def _rm3_call(lib, host_q_lims=(0, 3), host_out_lims=(0, 16), **over):
    q_lims, out_lims = np.asarray(host_q_lims, np.int64), np.asarray(host_out_lims, np.int64)
    a = dict(d_fwd_lims=P, d_fwd_terms=P, d_fwd_p=P, n_fwd=1000, d_term_offsets=P, n_rows=100, n_terms=50,
             q_lims=q_lims.ctypes.data, d_q_lims=P, d_q_terms=P, d_rank_scores=P, d_rank_ids=P, kb=16, d_mask=None, nq=1,
             fb_docs=5, fb_terms=10, orig_repeat=2, max_df=0, out_lims=out_lims.ctypes.data, d_out_lims=P, d_out_terms=P,
             d_out_sel_terms=P, d_out_sel_w=P, d_out_counts=P, d_out_fb=P, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return lib.sskd_prf_rm3(*a.values()), lib.sskd_last_error().decode()


@pytest.mark.parametrize("over, names", [
    (dict(fb_docs=0), "fb_docs=0"),
    (dict(fb_docs=17, kb=32), "fb_docs=17"),
    (dict(fb_docs=6, kb=5), "fb_docs=6 > kb=5"),
    (dict(kb=0), "kb=0"),
    (dict(kb=257), "kb=257"),
    (dict(fb_terms=0), "fb_terms=0"),
    (dict(fb_terms=65), "fb_terms=65"),
    (dict(orig_repeat=0), "orig_repeat=0"),
    (dict(orig_repeat=9), "orig_repeat=9"),
    (dict(max_df=-1), "max_df"),
    (dict(n_rows=(1 << 31) - 64), "n_rows"),
    (dict(n_rows=-1), "n_rows"),
    (dict(n_terms=-1), "n_terms"),
    (dict(n_fwd=-1), "n_fwd"),
    (dict(nq=-1), "nq"),
    (dict(d_fwd_lims=None), "index table"),
    (dict(d_fwd_p=None), "index table"),
    (dict(d_term_offsets=None), "index table"),
    (dict(q_lims=None), "query table"),
    (dict(d_q_terms=None), "query table"),
    (dict(d_rank_scores=None), "ranking"),
    (dict(out_lims=None), "output"),
    (dict(d_out_sel_w=None), "output"),
    (dict(d_out_fb=None), "output"),
])
def test_rm3_refuses_invalid_arguments_before_the_launch(native_lib, over, names):
    rc, message = _rm3_call(native_lib, **over)
    assert rc == 1, (rc, message)
    assert message.startswith("prf_rm3:") and names in message, message


@pytest.mark.parametrize("q_lims, out_lims, names", [
    ((0, 3), (0, 15), "out segment of query 0"),          # one slot short
    ((0, 3), (0, 17), "out segment of query 0"),          # one too many
    ((3, 0), (0, 16), "q_lims decreases"),
    ((-1, 2), (0, 16), "start at >= 0"),
    ((0, 3), (-16, 0), "start at >= 0"),
])
def test_rm3_checks_the_segment_lengths_on_the_host(native_lib, q_lims, out_lims, names):
    rc, message = _rm3_call(native_lib, host_q_lims=q_lims, host_out_lims=out_lims)
    assert rc == 1 and names in message, (rc, message)
