"""``sskd_mmr_select`` on the MI355X against the checker (``mmr_cases``), through the C-ABI: the same bits for scores,
ids, mmr, red and counts.

The corpus is the clustered family at 60 centres x 20 copies plus 8 bit-identical twins (1 208 rows: cosine about 0.98
inside a cluster, so ``dup_threshold = 0.8`` kills and lists end early; the twins tie exactly).  Rankings come from the
oracle's exact search and from hand-made lists.  ``fetch_k`` decides which kernel serves a call (every row resident in
LDS up to 50 and up to 100 candidates, the 32-row stage above), so the sweep stands on both sides of both limits and the
other cases run at a resident and at a staged width.  Every output buffer is filled with a poison pattern before the
call, so padding that is not written shows as a difference."""
import numpy as np
import pytest
import torch

import mmr_cases as mc
import ranking_walk_cases as rw
from capi_helpers import stream, tile_corpus
from oracle import search as oracle
from semantic_search_kd_amd import _native

pytestmark = pytest.mark.gpu

INF = float("inf")
POISON_F32, POISON_I64, POISON_F64, POISON_I32 = 12345.5, -777, 54321.25, -7


def poisoned(nq, k):
    rows = max(nq, 1)
    return (torch.full((rows, k), POISON_F32, dtype=torch.float32, device="cuda")[:nq],
            torch.full((rows, k), POISON_I64, dtype=torch.int64, device="cuda")[:nq],
            torch.full((rows, k), POISON_F64, dtype=torch.float64, device="cuda")[:nq],
            torch.full((rows, k), POISON_F32, dtype=torch.float32, device="cuda")[:nq],
            torch.full((rows,), POISON_I32, dtype=torch.int32, device="cuda")[:nq])


def capi_mmr(lib, tiled, n_rows, S, I, *, k, lam, dup_threshold=INF, id_offset=0, optional=True):
    """The call on host rankings; ``optional`` False passes d_out_mmr and d_out_red as NULL (None comes back)."""
    nq, fetch_k = I.shape
    d_s = torch.from_numpy(np.ascontiguousarray(S, np.float32)).cuda()
    d_i = torch.from_numpy(np.ascontiguousarray(I, np.int64)).cuda()
    D, J, V, R, counts = poisoned(nq, k)
    _native.check(lib.sskd_mmr_select(tiled.data_ptr(), n_rows, d_s.data_ptr(), d_i.data_ptr(), nq, fetch_k, lam,
                                      dup_threshold, k, id_offset, D.data_ptr(), J.data_ptr(),
                                      V.data_ptr() if optional else None, R.data_ptr() if optional else None,
                                      counts.data_ptr(), stream()))
    torch.cuda.synchronize()
    if not optional:   # nothing was written where NULL was passed
        assert (V == POISON_F64).all() and (R == POISON_F32).all()
    return (D.cpu().numpy(), J.cpu().numpy(), V.cpu().numpy() if optional else None,
            R.cpu().numpy() if optional else None, counts.cpu().numpy())


class World:
    def __init__(self, lib):
        self.rows, self.row_c, self.queries = mc.clustered_family(centres=60, copies=20, twins=8)
        self.n = self.rows.shape[0]
        assert self.n == 1208
        self.tiled = tile_corpus(lib, self.rows)
        self.gram = oracle.scores_fma(self.rows, self.rows)      # computed once, shared, never written
        self.gram.setflags(write=False)
        assert np.array_equal(mc.bits32(self.gram), mc.bits32(self.gram.T))
        self.rank = {}

    def ranking(self, fetch_k):
        if fetch_k not in self.rank:
            self.rank[fetch_k] = mc.ranking(self.queries, self.rows, fetch_k)
        return self.rank[fetch_k]

    def want(self, S, I, **kw):
        return mc.mmr_batch(S, I, self.rows, gram=self.gram, **kw)


@pytest.fixture(scope="module")
def world(native_lib, gpu):
    return World(native_lib)


@pytest.mark.parametrize("fetch_k", [1, 31, 32, 33, 50, 51, 100, 101, 257, 1024])
def test_select_equals_the_checker(native_lib, world, fetch_k):
    w = world
    nq = 8 if fetch_k <= 257 else 3
    S, I = (x[:nq] for x in w.ranking(fetch_k))
    shortened = differs = 0
    for k in sorted({1, min(10, fetch_k), fetch_k}):
        for lam in (0.0, 0.3, 0.5, 1.0):
            for thr in (INF, 0.8, -1.0):
                kw = dict(k=k, lam=lam, dup_threshold=thr)
                want = w.want(S, I, **kw)
                got = capi_mmr(native_lib, w.tiled, w.n, S, I, **kw)
                mc.same(got, want, f"fetch_k={fetch_k} k={k} lambda={lam} threshold={thr}")
                shortened += int((want[4] < min(k, fetch_k)).any())
                differs += int(not np.array_equal(want[1], I[:, :k]))
                if thr == -1.0:
                    assert (want[4] == 1).all()
                if lam == 1.0 and thr == INF:
                    assert np.array_equal(want[1], I[:, :k])
    if fetch_k >= 31:
        assert shortened and differs          # the cases did exercise counts < k and a re-ordering


def test_twins_tie_exactly_and_the_earlier_position_wins(native_lib, world):
    w = world
    S, I = (x.copy() for x in w.ranking(50))
    for q in range(8):                        # twin 1200 + q of row 20 q: the same score, listed right behind it
        at = {int(r): j for j, r in enumerate(I[q])}
        assert at[1200 + q] == at[20 * q] + 1 and mc.bits32(S[q, at[20 * q]]) == mc.bits32(S[q, at[1200 + q]])
    swapped = I.copy()
    for q in range(0, 8, 2):
        at = {int(r): j for j, r in enumerate(I[q])}
        swapped[q, at[20 * q]], swapped[q, at[1200 + q]] = 1200 + q, 20 * q
    for ids in (I, swapped):
        for lam in (0.0, 0.5, 1.0):
            kw = dict(k=50, lam=lam)
            want = w.want(S, ids, **kw)
            mc.same(capi_mmr(native_lib, w.tiled, w.n, S, ids, **kw), want, f"twins lambda={lam}")
            for q in range(8):
                got_at = {int(r): j for j, r in enumerate(want[1][q])}
                lst_at = {int(r): j for j, r in enumerate(ids[q])}
                a, b = 20 * q, 1200 + q
                assert (got_at[a] < got_at[b]) == (lst_at[a] < lst_at[b])


@pytest.mark.parametrize("width", [12, 104])
def test_hand_made_lists(native_lib, world, width):
    """``width`` 104: the same lists padded with -1, so the staged kernel walks them."""
    w = world
    n, fetch_k = w.n, 12
    S, I = (x[:6, :fetch_k].copy() for x in w.ranking(50))
    I[0, 5:] = -1                      # an early -1 ...
    I[0, 7:9] = [3, 4]                 # ... rows behind it are never read
    I[1, 2] = n                        # ids outside the index in the middle: skipped
    I[1, 3] = n + 12345
    I[1, 6] = -5                       # negative but not the padding id: skipped, the walk goes on
    I[2, :] = -1                       # m = 0
    I[3, 3:] = -1                      # m = 3 < k
    I[4, 5] = I[4, 1]                  # a row twice (the caller's promise broken: safe, and what the rule says)
    I[4, 9] = I[4, 0]
    S = np.concatenate([S, np.full((6, width - fetch_k), mc.NEG_PAD, np.float32)], axis=1)
    I = np.concatenate([I, np.full((6, width - fetch_k), -1, np.int64)], axis=1)
    for k in (1, 10, 12):
        for lam, thr in ((0.5, INF), (0.3, 0.8), (0.0, INF), (1.0, -1.0)):
            for optional in (True, False):
                kw = dict(k=k, lam=lam, dup_threshold=thr, id_offset=7000)
                want = w.want(S, I, **kw)
                got = capi_mmr(native_lib, w.tiled, n, S, I, optional=optional, **kw)
                mc.same(got, want, f"hand-made k={k} lambda={lam} threshold={thr} optional={optional}")
    want = w.want(S, I, k=10, lam=0.5, id_offset=7000)
    assert want[4].tolist() == [5, 9, 0, 3, 10, 10]
    assert (want[1][want[1] >= 0] >= 7000).all() and (want[1][2] == -1).all()
    # a negative offset, and one past 2^32
    for off in (-5, (1 << 33) + 1):
        kw = dict(k=10, lam=0.5, id_offset=off)
        mc.same(capi_mmr(native_lib, w.tiled, n, S, I, **kw), w.want(S, I, **kw), f"id_offset={off}")


@pytest.mark.parametrize("width", rw.WIDTHS)
def test_walk_at_the_round_boundaries(native_lib, world, width):
    """The shared hand-made rankings over the first 200 rows of the world: the first -1 at rank 0, 63, 64 and absent,
    rows behind it, ids outside the index and -9 before it (skipped: the walk goes on).  Width 1 runs the kernel with
    50 resident rows, 63 .. 65 the one with 100, 130 the staged one."""
    w, n = world, 200
    I = rw.ids(n, width)
    S = rw.descending_scores(width, low=0.05, high=0.95)
    rows, gram = w.rows[:n], w.gram[:n, :n]
    for k in sorted({1, min(10, width), width}):
        for lam, thr in ((0.5, INF), (0.3, 0.8), (1.0, INF)):
            kw = dict(k=k, lam=lam, dup_threshold=thr, id_offset=7000)
            want = mc.mmr_batch(S, I, rows, gram=gram, **kw)
            mc.same(capi_mmr(native_lib, w.tiled, n, S, I, **kw), want, f"walk width={width} k={k} lambda={lam} thr={thr}")
    # lambda = 1 without a threshold selects every candidate in list order: the counts are what the walk kept
    end = rw.first_pad(I)
    kept = [int(((I[q, :end[q]] >= 0) & (I[q, :end[q]] < n)).sum()) for q in range(rw.NQ)]
    assert want[4].tolist() == kept
    if width >= 63:
        assert kept[4] == width - 1 and kept[0] == 0, "-9 is skipped and the walk goes on; a -1 at rank 0 ends it"


def test_one_query_alone_and_many_queries(native_lib, world):
    """The checker is per query; this is the launch geometry: 1 workgroup, and more workgroups than compute units."""
    w = world
    for fetch_k in (33, 100, 101):
        S, I = w.ranking(fetch_k)
        kw = dict(k=10, lam=0.5, dup_threshold=0.99)
        mc.same(capi_mmr(native_lib, w.tiled, w.n, S[5:6], I[5:6], **kw), w.want(S[5:6], I[5:6], **kw), "one query")
        reps = 80                                                    # 640 queries
        got = capi_mmr(native_lib, w.tiled, w.n, np.tile(S, (reps, 1)), np.tile(I, (reps, 1)), **kw)
        want = w.want(S, I, **kw)
        mc.same(got, tuple(np.tile(x, (reps, 1)) if x.ndim == 2 else np.tile(x, reps) for x in want),
                f"640 queries, fetch_k={fetch_k}")


def test_no_queries_is_a_no_op(native_lib, world):
    w = world
    D, J, V, R, counts = poisoned(1, 4)
    rc = native_lib.sskd_mmr_select(w.tiled.data_ptr(), w.n, None, None, 0, 8, 0.5, INF, 4, 0, D.data_ptr(),
                                    J.data_ptr(), V.data_ptr(), R.data_ptr(), counts.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert (D == POISON_F32).all() and (J == POISON_I64).all() and (counts == POISON_I32).all()
    got = capi_mmr(native_lib, w.tiled, w.n, np.zeros((0, 8), np.float32), np.zeros((0, 8), np.int64), k=4, lam=0.5)
    assert got[0].shape == (0, 4) and got[4].shape == (0,)


@pytest.mark.parametrize("fetch_k", [50, 101])
def test_graph_capture_and_two_replays_equal_the_eager_result(native_lib, world, fetch_k):
    w = world
    S, I = w.ranking(fetch_k)
    k, lam, thr = 10, 0.5, 0.97
    want = w.want(S, I, k=k, lam=lam, dup_threshold=thr)
    eager = capi_mmr(native_lib, w.tiled, w.n, S, I, k=k, lam=lam, dup_threshold=thr)
    mc.same(eager, want, "eager")
    d_s, d_i = torch.from_numpy(S).cuda(), torch.from_numpy(I).cuda()
    out = poisoned(8, k)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            _native.check(native_lib.sskd_mmr_select(w.tiled.data_ptr(), w.n, d_s.data_ptr(), d_i.data_ptr(), 8, fetch_k, lam,
                                                     thr, k, 0, *(t.data_ptr() for t in out), stream()))
    torch.cuda.current_stream().wait_stream(side)
    for replay in range(2):
        for t in out:
            t.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        mc.same(tuple(t.cpu().numpy() for t in out), eager, f"replay {replay}")


# ---------------------------------------------------------------------------------------------------- bad arguments
P = 4096   # a non-null, 16-byte aligned "pointer": every check comes before the launch, nothing is read


def _call(lib, **over):
    a = dict(d_tiled=P, n_rows=100, d_rank_scores=P, d_rank_ids=P, nq=1, fetch_k=50, lam=0.5, dup_threshold=INF, k=10,
             id_offset=0, d_out_scores=P, d_out_ids=P, d_out_mmr=P, d_out_red=P, d_out_counts=P, stream=None)
    assert not set(over) - set(a)
    a.update(over)
    return lib.sskd_mmr_select(*a.values()), lib.sskd_last_error().decode()


@pytest.mark.parametrize("over, names", [
    (dict(k=0), "k=0"),
    (dict(k=51), "k=51"),
    (dict(fetch_k=0, k=1), "fetch_k=0"),
    (dict(fetch_k=1025), "fetch_k=1025"),
    (dict(lam=-0.1), "lambda"),
    (dict(lam=1.0000001), "lambda"),
    (dict(lam=float("nan")), "lambda"),
    (dict(lam=float("inf")), "lambda"),
    (dict(dup_threshold=float("nan")), "dup_threshold"),
    (dict(n_rows=-1), "n_rows"),
    (dict(n_rows=(1 << 31) - 64), "n_rows"),
    (dict(nq=-1), "nq"),
    (dict(d_tiled=P + 8), "d_tiled"),
    (dict(d_tiled=None), "null index"),
    (dict(d_rank_scores=None), "null ranking"),
    (dict(d_rank_ids=None), "null ranking"),
    (dict(d_out_scores=None), "null output"),
    (dict(d_out_ids=None), "null output"),
    (dict(d_out_counts=None), "null output"),
])
def test_refuses_invalid_arguments_before_the_launch(native_lib, gpu, over, names):
    D, J, V, R, counts = poisoned(1, 64)
    ptrs = dict(d_out_scores=D.data_ptr(), d_out_ids=J.data_ptr(), d_out_mmr=V.data_ptr(), d_out_red=R.data_ptr(),
                d_out_counts=counts.data_ptr())
    ptrs.update(over)
    rc, message = _call(native_lib, **ptrs)
    torch.cuda.synchronize()
    assert rc == 1, (rc, message)
    assert message.startswith("mmr_select:") and names in message, message
    assert (D == POISON_F32).all() and (J == POISON_I64).all() and (V == POISON_F64).all()       # the outputs: untouched
    assert (R == POISON_F32).all() and (counts == POISON_I32).all()
