"""The workspace contract of the C-ABI, as data: fills, a guarded allocation, the comparison, and one case per size query.

Every entry point that takes scratch memory declares a ``*_workspace_bytes`` query in ``include/sskd_amd.h``.  The
contract (stated in the header's conventions block, audited buffer by buffer in DESIGN.md "Workspace contract"):

* a call's results do not depend on what its workspace held on entry;
* a call touches no byte outside ``[d_workspace, d_workspace + *_workspace_bytes(...))``.

``tests/test_workspace_contract_host.py`` (CPU) checks that every size query of ``_native``'s signature table has a case
here, that the guard and the comparison catch a fake entry point that breaks either clause, and the plan claims the
cases rest on.  ``tests/test_workspace_contract_gpu.py`` runs ``CASES`` x shapes x ``FILLS`` on the MI355X.

This module imports without a GPU: every world is built inside a shape's ``setup`` on first use, once, from fixed seeds.
The search-family worlds make a stale value visible: the corpus is unnormalised around a common mean, query 0 points
away from that mean (every true score of it is negative, so a zero-filled slot would win), ``n_rows`` is no multiple of
32 and some shapes ask for more results than there are rows.
"""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

DIM = 384

# ---------------------------------------------------------------------------------------------------------------------
# fills and the guarded allocation
# ---------------------------------------------------------------------------------------------------------------------
# 0x00: score 0.0, id 0, count 0 - beats every negative true score.  0xFF: NaN, id -1, a huge unsigned.  0x7F: 3.39e38,
# a finite float that wins any top-k, int 2139062143.  "leftover": what the same entry point left behind after a call
# on another world whose scores are all larger (the shape supplies that call as ``prior``).
BYTE_FILLS = (0x00, 0xFF, 0x7F)
FILLS = BYTE_FILLS + ("leftover",)
GUARD_BYTE = 0xA5          # a fifth value: neither a fill nor anything a kernel is likely to write


def fill_name(fill):
    return fill if isinstance(fill, str) else f"0x{fill:02X}"


class Guarded:
    """One uint8 allocation ``[guard][slack][need bytes at an aligned address][guard]``; everything outside the ``need``
    bytes holds ``GUARD_BYTE``.  ``ptr`` / ``need`` are what a call is given: exactly ``need`` bytes, never more."""

    def __init__(self, buf, offset, need):
        self.buf, self.offset, self.need = buf, int(offset), int(need)
        self.ptr = buf.data_ptr() + self.offset

    def view(self):
        return self.buf[self.offset: self.offset + self.need]

    def intact(self) -> bool:
        lo, hi = self.buf[: self.offset], self.buf[self.offset + self.need:]
        return bool((lo == GUARD_BYTE).all()) and bool((hi == GUARD_BYTE).all())


def guarded(need, fill, device, align=256, guard=4096) -> Guarded:
    import torch

    need = int(need)
    buf = torch.full((guard + align + need + guard,), GUARD_BYTE, dtype=torch.uint8, device=device)
    offset = guard + (-(buf.data_ptr() + guard)) % align
    g = Guarded(buf, offset, need)
    assert g.ptr % align == 0 and offset >= guard and buf.numel() - (offset + need) >= guard
    if need:
        g.view().fill_(int(fill))
    return g


class Borrowed:
    """``(pointer, bytes)`` behind the two tensor methods the Python layer uses on a workspace (``data_ptr``, ``numel``):
    lets a case hand a guarded workspace to an index object whose buffer ``_native.grown`` then keeps."""

    def __init__(self, ptr, nbytes):
        self._ptr, self._n = int(ptr), int(nbytes)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def first_difference(got, want):
    """None when two tuples of host arrays are equal BIT FOR BIT (NaN patterns and the sign of zero included), else
    ``(output number, element index, got value, wanted value)`` of the first difference."""
    if len(got) != len(want):
        return (min(len(got), len(want)), None, f"{len(got)} outputs", f"{len(want)} outputs")
    for o, (a, b) in enumerate(zip(got, want)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            return (o, None, f"{a.dtype}{a.shape}", f"{b.dtype}{b.shape}")
        if a.size == 0:
            continue
        ab = a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)
        bb = b.reshape(-1).view(np.uint8).reshape(b.size, b.dtype.itemsize)
        bad = np.flatnonzero((ab != bb).any(axis=1))
        if bad.size:
            at = int(bad[0])
            idx = tuple(int(x) for x in np.unravel_index(at, a.shape)) if a.ndim else ()
            return (o, idx, a.reshape(-1)[at], b.reshape(-1)[at])
    return None


def check_fill(entry, shape, fill, call, need, device, baseline=None, deterministic=True, reference=None, prior=None,
               sync=None, stable=None, expect_written=False):
    """One (entry point, shape, fill): run ``call(guarded)`` on a guarded workspace of exactly ``need`` bytes holding
    ``fill`` and return ``(outputs, problems)``.  ``problems`` is a list of messages, each naming the entry point, the
    shape, the fill and - for a comparison - the first differing output element:

    * a guard byte changed (checked after ``sync()``);
    * ``reference(outputs)`` raised an AssertionError;
    * ``deterministic`` and the outputs (``stable(outputs)`` where an entry point has a diagnostic word that may vary)
      differ in any bit from ``baseline`` (the outputs of the 0x00 run).

    ``"leftover"`` starts from zeros and runs ``prior(guarded)`` first.  ``expect_written``: a call given a non-empty
    workspace of 0xFF or 0x7F bytes that leaves every byte as it was did not use the buffer it was handed (a case that
    lends its workspace to an object of the Python layer would otherwise pass without testing anything)."""
    sync = sync or (lambda: None)
    tag = f"{entry}[{shape}] fill={fill_name(fill)}"
    g = guarded(need, 0x00 if fill == "leftover" else fill, device)
    problems = []
    if fill == "leftover":
        prior(g)
        sync()
        if not g.intact():
            problems.append(f"{tag}: the prior call wrote outside its {need}-byte workspace")
    outs = call(g)
    sync()
    if not g.intact():
        buf = g.buf.cpu().numpy()
        inside = np.zeros(buf.size, bool)
        inside[g.offset: g.offset + g.need] = True
        at = int(np.flatnonzero((buf != GUARD_BYTE) & ~inside)[0]) - g.offset
        problems.append(f"{tag}: byte {at} relative to a {need}-byte workspace was written")
    if expect_written and need and fill in (0xFF, 0x7F) and bool((g.view() == fill).all()):
        problems.append(f"{tag}: the call left all {need} bytes of its workspace untouched: it ran on another buffer")
    if reference is not None:
        try:
            reference(outs)
        except AssertionError as e:
            problems.append(f"{tag}: the reference assertion fails: {e}")
    if deterministic and baseline is not None:
        stable = stable or (lambda o: o)
        d = first_difference(stable(outs), stable(baseline))
        if d is not None:
            problems.append(f"{tag}: output {d[0]} differs from the 0x00 run, first at element {d[1]}: {d[2]!r} != {d[3]!r}")
    return outs, problems


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
# Shape: ``setup(lib) -> Run`` builds the inputs once (GPU); ``deterministic``: the entry point returns the same bits
# for the same inputs; ``reference``: the NAME of the assertion ``Run.check`` applies - the one the entry point's own
# test makes.  Run: ``need`` = the size query's answer, ``run(lib, ws_ptr, ws_bytes) -> tuple of host arrays``,
# ``prior(lib, ws_ptr, ws_bytes)`` = the same entry point on the larger-scoring world, ``check(outputs)``.
Shape = namedtuple("Shape", "name setup deterministic reference")
Run = namedtuple("Run", "need run prior check stable", defaults=(None,))   # stable(outputs): what must not differ in a bit

ORACLE_BITS = "bit-equal to the fma-order oracle (oracle.search)"
EXACT_SCAN_BITS = "bit-equal to sskd_index_search on the same inputs"
RESTATEMENT_BITS = "bit-equal to the NumPy restatement of the entry point's test"
FP64_TOLERANCE = "the fp64 / oracle tolerance of the entry point's test"

_prepared = {}


def prepared(entry, shape, lib) -> Run:
    """``shape.setup(lib)``, once per process"""
    key = (entry, shape.name)
    if key not in _prepared:
        _prepared[key] = shape.setup(lib)
    return _prepared[key]


def _torch():
    import torch

    return torch


def _stream():
    return int(_torch().cuda.current_stream().cuda_stream)


def _sync():
    _torch().cuda.synchronize()


def _dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    return torch.from_numpy(a).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_topk(got, ref, what=""):
    s, i = got[0], got[1]
    assert np.array_equal(i, ref[1]), (what, "ids", np.argwhere(i != ref[1])[:3].tolist())
    assert np.array_equal(_bits(s), _bits(ref[0])), (what, "scores", np.argwhere(_bits(s) != _bits(ref[0]))[:3].tolist())


# ------------------------------------------------------------------------------------------- the search-family worlds
WORLD_NQ = 70
_worlds = {}


def world_arrays(n, nq=WORLD_NQ):
    """``(corpus, queries, corpus_big, queries_big)``: unnormalised rows around a common mean ``2 m``; query 0 = -1.5 m
    (every score negative), query 1 nearly so, query 2 next to a row; the "big" world scores every pair above 10."""
    from oracle import search as oracle

    m = oracle.seeded_unit_rows(1, DIM, 7000)[0]
    rng = np.random.default_rng(7001 + n)
    rows = oracle.seeded_unit_rows(n, DIM, 7002 + n)
    corpus = (2.0 * m[None] + rows * rng.uniform(0.5, 3.0, size=(n, 1))).astype(np.float32)
    q = oracle.seeded_unit_rows(nq, DIM, 7003)
    queries = (q * rng.uniform(0.5, 2.0, size=(nq, 1))).astype(np.float32)
    queries[0] = -1.5 * m
    if nq > 1:
        queries[1] = -m + 0.1 * q[1]
    if nq > 2:
        queries[2] = corpus[n // 2] + 0.05 * q[2]
    corpus_big = (6.0 * m[None] + rows).astype(np.float32)
    queries_big = (3.0 * m[None] + 0.2 * q).astype(np.float32)
    return corpus, np.ascontiguousarray(queries), corpus_big, queries_big


def world(lib, n, nq=WORLD_NQ, seed_scores=True):
    """The device side of ``world_arrays`` plus the oracle's scores of every (query, row): built once per ``(n, nq)``."""
    key = (n, nq)
    if key not in _worlds:
        from capi_helpers import tile_corpus
        from oracle import search as oracle

        corpus, queries, corpus_big, queries_big = world_arrays(n, nq)
        w = SimpleNamespace(n=n, nq=nq, corpus=corpus, queries=queries, tiled=tile_corpus(lib, corpus), q=_dev(queries),
                            tiled_big=tile_corpus(lib, corpus_big), q_big=_dev(queries_big), scores=None, extra={})
        if seed_scores:
            w.scores = oracle.scores_fma(queries, corpus)
            w.scores.setflags(write=False)
            assert (w.scores[0] < 0).all(), "query 0 must score every row below zero"
            big = oracle.scores_fma(queries_big[:3], corpus_big)
            assert big.min() > 10 and big.min() > w.scores.max(), "the prior world must score above the world itself"
        _worlds[key] = w
    return _worlds[key]


def _allow_mask(n, kind, seed):
    """``(allowed bool [n], device mask words)``; kind: "half", or an int = that many allowed rows"""
    from semantic_search_kd_amd.index import mask_words

    rng = np.random.default_rng(seed)
    if kind == "half":
        allowed = rng.random(n) < 0.5
    else:
        allowed = np.zeros(n, bool)
        allowed[rng.choice(n, int(kind), replace=False)] = True
    return allowed, _dev(mask_words(allowed, n).view(np.uint32))


def _topk_reference(w, nq, k, allowed=None, id_offset=0):
    from oracle import search as oracle

    s = w.scores[:nq].copy()
    if allowed is not None:
        s[:, ~allowed] = -np.inf
    return oracle.topk_of_scores(s, k, id_offset)


# ------------------------------------------------------------------------------------------------------ exact search
REDUCE_MIN_ROWS, REDUCE_NQ, REDUCE_K = 1025, 3, 10     # 33 tiles -> 5 slices x 8 waves x 2 lists = 80 > 64 lists per query
MERGE_DIRECT_MAX_LISTS = 64


def lists_per_query(lib, n, nq, k, tuning=(0, 0, 0)):
    """per-lane lists the exact scan leaves per query: slices x waves x 2, from the library's own plan"""
    from semantic_search_kd_amd import _native

    tn = _native.SearchTuning(*tuning)
    qpb, passes, slices, waves, scan_passes = (C.c_int(-1) for _ in range(5))
    _native.check(lib.sskd_index_search_plan_ex(n, nq, k, C.byref(tn), C.byref(qpb), C.byref(passes), C.byref(slices),
                                                C.byref(waves), C.byref(scan_passes)))
    return slices.value * waves.value * 2


def _exact_shape(name, n, nq, k, tuning=None, mask=None):
    """``tuning`` None: ``sskd_index_search``; a triple: ``sskd_index_search_filtered`` with that tuning struct"""

    def setup(lib):
        from semantic_search_kd_amd import _native

        torch = _torch()
        w = world(lib, n)
        tn = None if tuning is None else _native.SearchTuning(*tuning)
        allowed, mask_dev = (None, None) if mask is None else _allow_mask(n, mask, n + nq + k)
        if tuning is None:
            need = int(lib.sskd_index_search_workspace_bytes(n, nq, k))
        else:
            need = int(lib.sskd_index_search_workspace_bytes_ex(n, nq, k, C.byref(tn)))
        ref = _topk_reference(w, nq, k, allowed, 5)
        if mask is not None and mask != "half":
            assert int(mask) < k and (ref[1][:, int(mask):] == -1).all(), "the mask must leave fewer than k rows"
        if n < k:
            assert (ref[1][:, n:] == -1).all()

        def run(lib, ptr, nbytes, tiled=None, q=None):
            tiled, q = w.tiled if tiled is None else tiled, w.q if q is None else q
            out_s = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
            out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            if tuning is None:
                rc = lib.sskd_index_search(tiled.data_ptr(), n, q.data_ptr(), nq, k, 5, out_s.data_ptr(), out_i.data_ptr(),
                                           ptr, nbytes, _stream())
            else:
                rc = lib.sskd_index_search_filtered(tiled.data_ptr(), n, q.data_ptr(), nq, k, 5,
                                                    None if mask_dev is None else mask_dev.data_ptr(), out_s.data_ptr(),
                                                    out_i.data_ptr(), ptr, nbytes, _stream(), C.byref(tn), None, None)
            _native.check(rc)
            _sync()
            return out_s.cpu().numpy(), out_i.cpu().numpy()

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, w.tiled_big, w.q_big),
                   lambda outs: _same_topk(outs, ref, name))

    return Shape(name, setup, True, ORACLE_BITS)


def _scan_case_shapes():
    import search_variant_cases as sv

    wanted = ("k10_qb1", "k10_qb2", "k100_qb1", "k16_qb1", "k32", "k100_K32", "k10_qb1_pools")
    rows = {c.name: c for c in sv.SCAN_CASES}
    shapes = []
    for name in wanted:
        c = rows[name]
        shapes.append(_exact_shape(f"{name}-unmasked", c.n, c.nq, c.k, c.tuning))
        shapes.append(_exact_shape(f"{name}-masked", c.n, c.nq, c.k, c.tuning, mask="half"))
    shapes.append(_exact_shape("k10_qb1-fewer_than_k", 3001, 3, 10, (0, 0, 0), mask=5))
    return shapes


# ---------------------------------------------------------------------------------------------------- one-pass search
def _onepass_shape(name, n, nq, k, mask=None):
    def setup(lib):
        from semantic_search_kd_amd import _native

        torch = _torch()
        w = world(lib, n)
        allowed, mask_dev = (None, None) if mask is None else _allow_mask(n, mask, n + nq + k + 1)
        need = int(lib.sskd_index_search_onepass_workspace_bytes(n, nq, k))
        ref = _topk_reference(w, nq, k, allowed, 5)

        def run(lib, ptr, nbytes, tiled=None, q=None):
            tiled, q = w.tiled if tiled is None else tiled, w.q if q is None else q
            out_s = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
            out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            flag = torch.full((1,), 9, dtype=torch.int32, device="cuda")
            _native.check(lib.sskd_index_search_onepass_filtered(
                tiled.data_ptr(), n, q.data_ptr(), nq, k, 5, None if mask_dev is None else mask_dev.data_ptr(),
                out_s.data_ptr(), out_i.data_ptr(), flag.data_ptr(), ptr, nbytes, _stream()))
            _sync()
            return out_s.cpu().numpy(), out_i.cpu().numpy(), flag.cpu().numpy()

        def check(outs):
            assert int(outs[2][0]) == 0, (name, "the one-pass proof did not hold", int(outs[2][0]))
            _same_topk(outs, ref, name)

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, w.tiled_big, w.q_big), check)

    return Shape(name, setup, True, ORACLE_BITS)


# ---------------------------------------------------------------------------------------------------- screened search
SCREEN_K = 10


def _screened_shape(name, n, nq, claim, mask=None, band_world=False):
    """``band_world``: the query scale sweep of ``screen_band_cases`` on unit rows - queries below 2^-96 get no band and
    are answered by the in-call exact scan (status[1] counts them)"""

    def setup(lib):
        from semantic_search_kd_amd import _native

        torch = _torch()
        k = SCREEN_K
        if band_world:
            key = ("band", n, nq)
            if key not in _worlds:
                import screen_band_cases as sb
                from capi_helpers import tile_corpus

                corpus = sb.corpus_of("unit", n)
                queries, _ = sb.sweep_queries(nq)
                _worlds[key] = SimpleNamespace(n=n, nq=nq, corpus=corpus, queries=queries, tiled=tile_corpus(lib, corpus),
                                               q=_dev(queries), tiled_big=tile_corpus(lib, 8.0 * corpus),
                                               q_big=_dev(np.abs(queries[::-1]) * 4.0 + 1.0), scores=None, extra={})
            w = _worlds[key]
        else:
            w = world(lib, n, nq, seed_scores=n * nq <= 4_000_000)
        for which, tiled in (("bf", w.tiled), ("bf_big", w.tiled_big)):
            if which not in w.extra:
                bf = torch.empty(int(lib.sskd_index_bf16_bytes(n)), dtype=torch.uint8, device="cuda")
                _native.check(lib.sskd_index_make_bf16(tiled.data_ptr(), n, bf.data_ptr(), _stream()))
                w.extra[which] = bf
        allowed, mask_dev = (None, None) if mask is None else _allow_mask(n, mask, n + nq)
        mask_ptr = None if mask_dev is None else mask_dev.data_ptr()
        need = int(lib.sskd_index_search_screened_workspace_bytes(n, nq, k))
        assert need > 0
        # the reference of the screened search's own tests: the exact scan's bits on the same inputs (computed once)
        rkey = ("exact", mask)
        if rkey not in w.extra:
            out_s = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
            out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            ws = torch.empty(int(lib.sskd_index_search_workspace_bytes(n, nq, k)), dtype=torch.uint8, device="cuda")
            _native.check(lib.sskd_index_search_filtered(w.tiled.data_ptr(), n, w.q.data_ptr(), nq, k, 5, mask_ptr,
                                                         out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                                                         _stream(), None, None, None))
            _sync()
            w.extra[rkey] = (out_s.cpu().numpy(), out_i.cpu().numpy())
            if w.scores is not None:
                _same_topk(w.extra[rkey], _topk_reference(w, nq, k, allowed, 5), "the exact scan itself")
            elif band_world:
                from oracle import search as oracle

                _same_topk(w.extra[rkey], oracle.topk_fma(w.queries, w.corpus, k, 5), "the exact scan itself")
        ref = w.extra[rkey]
        no_band = None
        if band_world:
            # as tests/test_screen_band_gpu.py: on random scores the fallback takes exactly the queries without a band
            if "no_band" not in w.extra:
                eps2 = torch.full((nq,), float("nan"), dtype=torch.float32, device="cuda")
                scratch = torch.empty(int(lib.sskd_index_screen_band_scratch_bytes(nq)), dtype=torch.uint8, device="cuda")
                _native.check(lib.sskd_index_screen_band(w.extra["bf"].data_ptr(), n, w.q.data_ptr(), nq, eps2.data_ptr(),
                                                         scratch.data_ptr(), scratch.numel(), _stream()))
                _sync()
                w.extra["no_band"] = int(np.isposinf(eps2.cpu().numpy()).sum())
            no_band = w.extra["no_band"]
            assert 1 <= no_band < nq, no_band

        def run(lib, ptr, nbytes, big=False):
            tiled, bf, q = (w.tiled_big, w.extra["bf_big"], w.q_big) if big else (w.tiled, w.extra["bf"], w.q)
            out_s = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
            out_i = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            _native.check(lib.sskd_index_search_screened_claim(
                tiled.data_ptr(), bf.data_ptr(), n, q.data_ptr(), nq, k, 5,
                None if mask_dev is None else mask_dev.data_ptr(),      # (the closure keeps the mask alive)
                int(claim), out_s.data_ptr(),
                out_i.data_ptr(), status.data_ptr(), ptr, nbytes, _stream(), None, None))
            _sync()
            return out_s.cpu().numpy(), out_i.cpu().numpy(), status.cpu().numpy()

        def check(outs):
            st = outs[2]
            assert st[0] == 0 and 0 <= st[1] <= nq, (name, st.tolist())
            if band_world:
                # the plan deals the tiles of so small a shape: then exactly the queries without a band fall back.  Forced
                # claiming may overflow more runs (a query with a band may still fall back), never fewer.
                assert st[1] == no_band if not claim else st[1] >= no_band, \
                    (name, "the fallback count against the number of queries without a band", st.tolist(), no_band)
            _same_topk(outs, ref, name)

        # status[1] counts the queries sent to the fallback.  Whether a run overflows depends on the pruning bound its
        # wave held when the rows came by, and the bound travels between workgroups as they happen to run: the count is
        # a cost diagnostic that may differ between two calls.  Scores, ids and status[0] may not.
        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, big=True), check,
                   lambda outs: (outs[0], outs[1], outs[2][:1]))

    return Shape(name, setup, True, EXACT_SCAN_BITS)


def _screen_case_shapes():
    import search_variant_cases as sv

    shapes = []
    for c in sv.SCREEN_CASES:
        for claim in (0, 1):
            shapes.append(_screened_shape(f"{c.name}-{'claimed' if claim else 'dealt'}", c.n, c.nq, claim))
    shapes.append(_screened_shape("screen_qb2-masked-dealt", 2049, 64, 0, mask="half"))
    shapes.append(_screened_shape("screen_qb2-masked-claimed", 2049, 64, 1, mask="half"))
    shapes.append(_screened_shape("band_sweep_fallback-dealt", 2049, 65, 0, band_world=True))
    shapes.append(_screened_shape("band_sweep_fallback-claimed", 2049, 65, 1, band_world=True))
    return shapes


# ------------------------------------------------------------------------------------------------------- range search
RANGE_SENT_S, RANGE_SENT_I = 12345.0, -77


def _range_shape(name, n, nq, over_cap):
    def setup(lib):
        from semantic_search_kd_amd import _native
        from test_range_search_gpu import _ref_from_scores, _same, _spread_thresholds

        from oracle import search as oracle

        torch = _torch()
        w = world(lib, n)

        def thresholds(s):
            """three queries: half the rows, 30 rows, every row; more: the spread of the range search's own test"""
            if s.shape[0] != 3:
                return _spread_thresholds(s)
            desc = -np.sort(-s, axis=1)
            return np.array([desc[0, n // 2], desc[1, 30], -np.inf], np.float32)

        thr = thresholds(w.scores[:nq])
        ref = _ref_from_scores(w.scores[:nq], thr, 5)
        total = int(ref[0][-1])
        assert total > 1000
        max_results = total - 1 if over_cap else total
        room = total + 64
        need = int(lib.sskd_index_range_search_workspace_bytes(n, nq, max_results))
        # the prior call: about as many results, every score above 10
        thr_dev, thr_big = _dev(thr), _dev(thresholds(oracle.scores_fma(world_arrays(n)[3][:nq], world_arrays(n)[2])))

        def run(lib, ptr, nbytes, big=False):
            lims = torch.full((nq + 1,), -3, dtype=torch.int64, device="cuda")
            sc = torch.full((room,), RANGE_SENT_S, dtype=torch.float32, device="cuda")
            ids = torch.full((room,), RANGE_SENT_I, dtype=torch.int64, device="cuda")
            _native.check(lib.sskd_index_range_search(
                (w.tiled_big if big else w.tiled).data_ptr(), n, (w.q_big if big else w.q).data_ptr(), nq,
                (thr_big if big else thr_dev).data_ptr(), 5, None, lims.data_ptr(), sc.data_ptr(), ids.data_ptr(), max_results,
                ptr, nbytes, _stream()))
            _sync()
            return lims.cpu().numpy(), sc.cpu().numpy(), ids.cpu().numpy()

        def check(outs):
            lims, sc, ids = outs
            assert np.array_equal(lims, ref[0]), (name, "lims", np.flatnonzero(lims != ref[0])[:5].tolist())
            written = 0 if over_cap else total
            if not over_cap:
                _same((lims, sc[:total], ids[:total]), ref, name)
            assert (sc[written:] == np.float32(RANGE_SENT_S)).all() and (ids[written:] == RANGE_SENT_I).all(), \
                (name, "written past the results" if not over_cap else "an overflowing call wrote results")

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, big=True), check)

    return Shape(name, setup, True, ORACLE_BITS)


def _range_merge_shape(name, overflow):
    def setup(lib):
        import test_range_merge_gpu as rm
        from test_range_search_gpu import _ref_from_scores, _same, _spread_thresholds

        n, nq, cut = 3001, 33, 1400
        w = world(lib, n)
        thr = _spread_thresholds(w.scores[:nq])
        ref = _ref_from_scores(w.scores[:nq], thr, rm.OFFSET)
        total = int(ref[0][-1])
        q, t = w.q[:nq].contiguous(), _dev(thr)
        runs = [rm._range(lib, w.corpus, lo, hi, q, t) for lo, hi in ((0, cut), (cut, n))]
        cap = max(int(r[0][-1].item()) for r in runs) + 3
        records = rm._pack(lib, runs, nq, cap)
        # the prior call: the same records with every score raised (another, larger-scoring pair of shards)
        big_runs = [(l, s + 100.0, i) for l, s, i in runs]
        records_big = rm._pack(lib, big_runs, nq, cap)
        max_results = total - 1 if overflow else total
        need = int(lib.sskd_range_merge_workspace_bytes(2, nq, max_results))

        def run(lib, ptr, nbytes, buf=records):
            return rm._merge(lib, buf, 2, nq, cap, max_results, room=total + 5, ws=(ptr, nbytes))

        def check(outs):
            lims, sc, ids = outs
            assert np.array_equal(lims, ref[0]), (name, "lims")
            written = 0 if overflow else total
            if not overflow:
                _same((lims, sc[:total], ids[:total]), ref, name)
            assert (sc[written:].view(np.int32) == rm.SENTINEL_BITS).all() and (ids[written:] == rm.SENTINEL_ID).all(), name

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, records_big), check)

    return Shape(name, setup, True, "bit-equal to one range search over the union (the fma-order oracle)")


# ----------------------------------------------------------------------------------------------------- grouped search
def _grouped_shape(name, n, nq, k, k_rows, n_groups, expect_unproved):
    """``n_groups`` None: runs of three consecutive rows (``k_rows`` None = the Python layer's default (k - 1) 3 + 1);
    else rows dealt at random to that many groups"""

    def setup(lib):
        import grouped_cases as gc
        from semantic_search_kd_amd import _native

        torch = _torch()
        w = world(lib, n)
        if n_groups is None:
            groups = (np.arange(n) // 3).astype(np.int32)
        else:
            groups = np.random.default_rng(7100 + n).integers(0, n_groups, n).astype(np.int32)
        kr = (k - 1) * 3 + 1 if k_rows is None else k_rows
        assert kr <= 32 or k_rows is not None
        rg = _dev(groups)
        need = int(lib.sskd_index_search_grouped_workspace_bytes(n, nq, k, kr))
        ref = gc.expected(w.scores[:nq], groups, k, None, 5, kr)
        assert bool(ref[4].any()) == expect_unproved, (name, ref[4])

        def run(lib, ptr, nbytes, big=False):
            sc = torch.full((nq, k), 12345.0, dtype=torch.float32, device="cuda")
            ids = torch.full((nq, k), -77, dtype=torch.int64, device="cuda")
            gr = torch.full((nq, k), -55, dtype=torch.int32, device="cuda")
            cnt = torch.full((nq,), -55, dtype=torch.int32, device="cuda")
            unp = torch.full((nq,), -55, dtype=torch.int32, device="cuda")
            nun = torch.full((1,), -55, dtype=torch.int32, device="cuda")
            _native.check(lib.sskd_index_search_grouped(
                (w.tiled_big if big else w.tiled).data_ptr(), n, (w.q_big if big else w.q).data_ptr(), nq, k, kr, 5, None,
                rg.data_ptr(), sc.data_ptr(), ids.data_ptr(), gr.data_ptr(), cnt.data_ptr(), unp.data_ptr(), nun.data_ptr(),
                ptr, nbytes, _stream()))
            _sync()
            return tuple(t.cpu().numpy() for t in (sc, ids, gr, cnt, unp, nun))

        def check(outs):
            D, I, G, cnt, unp, nun = outs
            assert np.array_equal(unp.astype(bool), ref[4]) and int(nun[0]) == int(ref[4].sum()), (name, "unproved")
            assert np.array_equal(cnt, ref[3]), (name, "counts")
            gc.same((D, I, G), ref[:3], name)

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, big=True), check)

    return Shape(name, setup, True, ORACLE_BITS)


# ---------------------------------------------------------------------------------------------------------------- BM25
def _bm25_shape(name, chunked):
    def setup(lib):
        import test_bm25_gpu as tb
        from semantic_search_kd_amd import _native

        torch = _torch()
        if "bm25" not in _worlds:
            _worlds["bm25"] = tb.Case("T+1", tb._tile_rows(lib), torch.device("cuda:0"))
        case = _worlds["bm25"]
        index, k = case.index, 10
        post = index._require_built()
        dev, offsets, rows, wts, idf = index._tables()
        queries = list(case.queries)
        nq = len(queries)
        d_lims, d_terms = index.query_csr(queries)
        # the prior call: every query is the commonest word many times over - the largest scores of the corpus
        p_lims, p_terms = index.query_csr([" ".join([case.common] * 8)] * nq)
        need = int(lib.sskd_bm25_search_workspace_bytes(case.n, 1 if chunked else nq, k))
        if not chunked:
            assert need == nq * int(lib.sskd_bm25_search_workspace_bytes(case.n, 1, k)), "the whole batch in one chunk"

        def run(lib, ptr, nbytes, lims=d_lims, terms=d_terms):
            scores = torch.full((nq, k), float("nan"), dtype=torch.float64, device=dev)
            ids = torch.full((nq, k), -7, dtype=torch.int64, device=dev)
            _native.check(lib.sskd_bm25_search(offsets.data_ptr(), rows.data_ptr(), wts.data_ptr(), idf.data_ptr(), post.corpus_size,
                                               post.n_terms, lims.data_ptr(), terms.data_ptr(), nq, k, scores.data_ptr(),
                                               ids.data_ptr(), ptr, nbytes, _stream()))
            _sync()
            return ids.cpu().numpy(), scores.cpu().numpy().view(np.int64)

        def check(outs):
            ids, bits = outs
            for qi in range(nq):
                want_ids, want_bits = case.expect(qi, k)
                assert np.array_equal(ids[qi], want_ids), (name, qi, ids[qi].tolist(), want_ids.tolist())
                assert np.array_equal(bits[qi], want_bits), (name, qi, "score bits")

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, p_lims, p_terms), check)

    return Shape(name, setup, True, "bit-equal to the dict-and-loop BM25 oracle (bm25_cases)")


# ------------------------------------------------------------------------------------------------------ IVF and IVF-PQ
def _ann_world(lib):
    """3 001 unnormalised rows in 16 random lists, a flat index over them, 65 queries (``world`` of the same size)"""
    if "ann" not in _worlds:
        from semantic_search_kd_amd import FAISSIndexBuilder, IVFIndex, ivf as ivf_mod
        from oracle import search as oracle

        n, nlist = 3001, 16
        w = world(lib, n)
        centroids = oracle.seeded_unit_rows(nlist, DIM, 7200)
        assignment = np.random.default_rng(7201).integers(0, nlist, size=n)
        flat = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device="cuda:0")
        flat.build_from_embeddings(w.corpus)
        flat_big = FAISSIndexBuilder(embedding_dim=DIM, metric="ip", device="cuda:0")
        flat_big.build_from_embeddings(world_arrays(n)[2])
        offsets, rows = ivf_mod.csr_from_assignment(assignment, nlist)
        _worlds["ann"] = SimpleNamespace(n=n, nlist=nlist, w=w, centroids=centroids, assignment=assignment, flat=flat,
                                         flat_big=flat_big, offsets=offsets, rows=rows,
                                         ivf=IVFIndex.from_assignment(flat, centroids, assignment),
                                         ivf_big=IVFIndex.from_assignment(flat_big, centroids, assignment))
    return _worlds["ann"]


def _ivf_shape(name, nq, k, nprobe):
    def setup(lib):
        from test_ivf_gpu import _ivf_oracle, _probe_host

        a = _ann_world(lib)
        q = a.w.q[:nq].contiguous()
        probe = _probe_host(a.ivf, a.w.queries[:nq], nprobe)
        ref = _ivf_oracle(a.w.scores[:nq], probe, a.offsets, a.rows, k)
        need = int(lib.sskd_ivf_search_workspace_bytes(nq, nprobe, k, a.n, a.ivf.max_list_rows))

        def run(lib, ptr, nbytes, index=None, queries=None):
            index = a.ivf if index is None else index
            index._workspace = lent = Borrowed(ptr, nbytes)      # IVFIndex passes the size query's answer, not the buffer's size
            try:
                s, i = index.search_device(q if queries is None else queries, k, nprobe=nprobe, normalize_queries=False)
                _sync()
                assert index._workspace is lent, (name, "the index did not run on the workspace it was lent")
            finally:
                index._workspace = None
            return s.cpu().numpy(), i.cpu().numpy()

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, a.ivf_big, a.w.q_big[:nq].contiguous()),
                   lambda outs: _same_topk(outs, ref, name))

    return Shape(name, setup, True, ORACLE_BITS)


def _pq_shape(name, nq, k, nprobe, refine):
    def setup(lib):
        import pq_cases as pc
        import test_pq_gpu as tp
        from semantic_search_kd_amd import IVFPQIndex

        a = _ann_world(lib)
        if "pq" not in a.__dict__:
            m = 8
            resid = pc.residuals(a.w.corpus, a.centroids, a.assignment)
            cb = tp._sample_codebooks(resid, m, 7300)
            a.pq = IVFPQIndex.from_codebooks(a.flat, a.centroids, a.assignment, cb)
            a.pq_big = IVFPQIndex.from_codebooks(a.flat_big, a.centroids, a.assignment, cb)
            a.pq_codes = pc.encode(resid, cb)
            assert np.array_equal(a.pq.codes_numpy(), a.pq_codes)
        queries = a.w.queries[:nq]
        q = a.w.q[:nq].contiguous()
        pw = SimpleNamespace(index=a.pq, offsets=a.offsets, rows=a.rows, codes=a.pq_codes)
        ranking = tp._rankings(pw, queries, nprobe, nlist=a.nlist)
        need = int(lib.sskd_pq_search_workspace_bytes(nq, nprobe, k, refine, a.pq.m, a.n, a.pq.max_list_rows))

        def run(lib, ptr, nbytes, index=None, qq=None):
            index = a.pq if index is None else index
            index._pq_workspace = lent = Borrowed(ptr, nbytes)
            try:
                out = index.search_device(q if qq is None else qq, k, nprobe=nprobe, refine=refine, normalize_queries=False,
                                          return_candidates=refine > 0)
                _sync()
                assert index._pq_workspace is lent, (name, "the index did not run on the workspace it was lent")
            finally:
                index._pq_workspace = None
            return tuple(t.cpu().numpy() for t in out)

        def check(outs):
            if refine == 0:
                tp._same(outs, tp._adc_result(ranking, k), name)
                return
            D, I, cand = outs
            for i in range(nq):
                want = ranking[i][1][:refine]
                assert np.array_equal(cand[i, :len(want)], want) and (cand[i, len(want):] == -1).all(), (name, i, "candidates")
                s = a.w.scores[i: i + 1].copy()
                keep = np.zeros(a.n, bool)
                keep[want] = True
                s[:, ~keep] = -np.inf
                from oracle import search as oracle

                _same_topk((D[i: i + 1], I[i: i + 1]), oracle.topk_of_scores(s, k), (name, i))

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, a.pq_big, a.w.q_big[:nq].contiguous()), check)

    return Shape(name, setup, True, RESTATEMENT_BITS)


# --------------------------------------------------------------------------------------------------------------- graph
def _graph_shape(name):
    """``sskd_graph_search`` keeps a query's whole state in LDS: the size query answers 0 and the call takes no
    workspace argument.  The case pins that down and runs the search beside a guarded zero-byte workspace."""

    def setup(lib):
        import graph_cases as gc
        import test_graph_gpu as tg

        a = _ann_world(lib)
        nq, k, ef, width, degree = 5, 10, 64, 4, 32
        need = int(lib.sskd_graph_search_workspace_bytes(nq, k, ef, width, degree, 16))
        adjacency = gc.random_adjacency(a.n, degree, 7400)
        index = tg._over(a.flat, adjacency)
        index_big = tg._over(a.flat_big, adjacency)
        seeds = np.random.default_rng(7401).integers(0, a.n, size=(nq, 16)).astype(np.int64)
        seeds[:, 3] = -1
        ref = gc.beam_search_batch_ref(a.w.scores[:nq], adjacency, seeds, ef, width, ef, k)

        def run(lib, ptr, nbytes, ix=index, queries=a.w.queries[:nq]):
            return tg._search(ix, queries, k, ef, width, ef, seeds)

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, index_big, world_arrays(a.n)[3][:nq]),
                   lambda outs: tg._check(outs, ref, name))

    return Shape(name, setup, True, RESTATEMENT_BITS)


# ---------------------------------------------------------------------------------------------------- late interaction
def _late_world(lib, compressed):
    key = "latec" if compressed else "late"
    if key not in _worlds:
        import late_cases as lc

        torch = _torch()
        rng = np.random.default_rng(7500)
        tok, lims = lc.sweep_store()
        n = lims.size - 1
        nq, R, k = 3, 100, 10
        q_bits, q_lims = lc.queries(rng, [5, 33, 128])
        cand = lc.candidates(rng, nq, R, n, must=np.concatenate([lc.big_rows(lims)[:12], [7]]))
        big_bits, _ = lc.queries(np.random.default_rng(7501), [5, 33, 128])
        if compressed:
            import test_late_codec_gpu as tc

            store = tc.Store(torch.device("cuda:0"), tok, lims, tc._codec(16, 2), 2)
            late = store.late
        else:
            import test_late_gpu as tl

            late = tl._late(tok, lims, torch.device("cuda:0"))
            store = None
        _worlds[key] = SimpleNamespace(lc=lc, tok=tok, lims=lims, n=n, nq=nq, R=R, k=k, q_bits=q_bits, q_lims=q_lims, cand=cand,
                                       big_bits=lc.bf16_bits(lc.bf16_values(big_bits) * np.float32(3.0)), late=late, store=store)
    return _worlds[key]


def _late_shape(name, compressed):
    """The re-rank uses its workspace only when the caller does not ask for the raw scores.  Reference: the raw scores
    of the SAME kernel written to the caller's buffer (no workspace involved) - held to the fp64 band by the entry
    point's own test - and the ranking check of that test on (D, I) against them."""

    def setup(lib):
        torch = _torch()
        w = _late_world(lib, compressed)
        lc, late = w.lc, w.late
        size = lib.sskd_latec_rerank_workspace_bytes if compressed else lib.sskd_late_rerank_workspace_bytes
        need = int(size(w.nq, w.R))
        cand = torch.from_numpy(w.cand).cuda()
        D0, I0, raw = late.rerank_device(w.q_bits, w.q_lims, cand, w.k, return_raw=True)
        _sync()
        D0, I0, raw = D0.cpu().numpy(), I0.cpu().numpy(), raw.cpu().numpy()
        lc.check_ranking(D0, I0, raw, w.cand, w.k)
        if compressed:
            import test_late_codec_gpu as tc

            tc._assert_in_band(raw, w.store.reference(w.q_bits, w.q_lims), w.cand)
        else:
            import test_late_gpu as tl

            tl._assert_in_band(raw, lc.Reference(w.q_bits, w.q_lims, w.tok, w.lims), w.cand)

        def run(lib, ptr, nbytes, q_bits=w.q_bits):
            late._workspace = lent = Borrowed(ptr, nbytes)
            try:
                D, I = late.rerank_device(q_bits, w.q_lims, cand, w.k)
                _sync()
                assert late._workspace is lent, (name, "the index did not run on the workspace it was lent")
            finally:
                late._workspace = None
            return D.cpu().numpy(), I.cpu().numpy()

        def check(outs):
            lc.check_ranking(outs[0], outs[1], raw, w.cand, w.k)
            assert first_difference(outs, (D0, I0)) is None, (name, "differs from the call that returns the raw scores")

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, w.big_bits), check)

    return Shape(name, setup, True, "the ranking check of the re-rank's test against the kernel's own raw scores")


def _plaid_shape(name, one_query):
    def setup(lib):
        import test_plaid_gpu as tp

        torch = _torch()
        if "plaid" not in _worlds:
            world_ = tp._world(torch.device("cuda:0"), 300)
            S, q_lims = tp._sweep_scores(lib, world_, "mixed", tp.MIXED, 500)
            _worlds["plaid"] = (world_, S, q_lims)
        world_, S, q_lims = _worlds["plaid"]
        nq, nprobe, R = q_lims.size - 1, 4, 64
        want = world_.ref(S, q_lims, nprobe, R)
        need = int(lib.sskd_plaid_candidates_workspace_bytes(1 if one_query else nq, world_.n, nprobe))
        S_big = (np.abs(S) * 4.0 + 8.0).astype(np.float32)

        def run(lib, ptr, nbytes, scores=S):
            rc, I, A, N, intact = tp.candidates(lib, world_, scores, q_lims, nprobe, R, ws=(ptr, nbytes))
            assert intact, (name, "written outside the outputs")
            return I, A, N

        def check(outs):
            tp.assert_matches((0,) + tuple(outs) + (True,), want, name)

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, S_big), check)

    return Shape(name, setup, True, RESTATEMENT_BITS)


# ---------------------------------------------------------------------------------------------------------- encoders
def _encoder_shape(name, case_name, packed):
    def setup(lib):
        import encoder_kernel_cases as kc
        import test_encoder_kernels_gpu as te
        from oracle import encoder_ops as eo

        case = [c for c in kc.ATTENTION_CASES if c["name"] == case_name][0]
        key = ("probe", case["kind"])
        if key not in _worlds:
            _worlds[key] = te.Probe(lib, case["kind"], 1)
        pr = _worlds[key]
        inp = kc.make_inputs(case)
        big = dict(inp)
        big["ids"] = np.where(inp["mask"] != 0, (inp["ids"].astype(np.int64) * 7 + 13) % kc.VOCAB, 0).astype(np.int32)
        B, S = case["B"], case["S"]
        need = int(lib.sskd_encoder_workspace_bytes(pr.ccfg(1), B, S))
        hid, _ = pr.run(inp, 1)                       # the same kernels on a workspace of their own
        fwd = pr.forward_packed if packed else pr.forward

        def run(lib, ptr, nbytes, x=inp):
            return (fwd(x, 1, True, ws=(ptr, nbytes)).numpy(),)

        def check(outs):
            import torch

            got = torch.from_numpy(outs[0])
            if packed:
                for row, lo, hi, dst in inp["table"].tolist():
                    wgt = np.zeros(S)
                    wgt[lo:hi] = 1
                    o = eo.pool(hid[row], wgt, True)
                    te._check(got[dst], o["ref"], o["T"], f"{name}: segment [{lo}, {hi}) of row {row}")
            else:
                for b in range(B):
                    o = eo.pool(hid[b], inp["mask"][b], True)
                    te._check(got[b], o["ref"], o["T"], f"{name}: row {b}")

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, big), check)

    return Shape(name, setup, True, FP64_TOLERANCE)


def _generic_shape(name, training):
    def setup(lib):
        from oracle import encoder as enc_oracle
        from semantic_search_kd_amd import BertConfig, _native, synthetic_state_dict
        from semantic_search_kd_amd.training import TrainableEncoder

        torch = _torch()
        cfg = BertConfig(vocab_size=600, hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                         max_position_embeddings=64)
        ids_h, mask_h = enc_oracle.synthetic_token_ids(5, 40, seed=31, vocab=600, lengths=[40, 33, 17, 8, 2])
        ids_big = np.where(mask_h != 0, (ids_h.astype(np.int64) * 7 + 3) % 600, 0).astype(ids_h.dtype)
        sd = synthetic_state_dict(cfg)
        model = TrainableEncoder(cfg, sd, "cuda:0")
        model._refresh_device_weights()
        model._attach_grads()
        ids, mask = _native.padded_ids_mask(ids_h, mask_h, model.device)
        idb, _ = _native.padded_ids_mask(ids_big, mask_h, model.device)
        B, S = ids.shape
        H = cfg.hidden_size
        probe = np.random.Generator(np.random.PCG64(5)).standard_normal((B, H)).astype(np.float32)
        dout = torch.from_numpy(probe).cuda()
        need = int(lib.sskd_generic_workspace_bytes(model.cfg_struct, B, S, training))
        t = {k_: torch.from_numpy(v).clone().requires_grad_(bool(training)) for k_, v in sd.items()}
        e = enc_oracle.embeddings_torch(t, ids_h, mask_h, cfg.num_hidden_layers, cfg.num_attention_heads)
        want_g = None
        if training:
            (e * torch.from_numpy(probe)).sum().backward()
            want_g = {k_: v.grad.numpy() for k_, v in t.items() if v.grad is not None}
        want_e = e.detach().numpy()

        def run(lib, ptr, nbytes, tokens=ids):
            out = torch.full((B, H), float("nan"), dtype=torch.float32, device="cuda")
            _native.check(lib.sskd_generic_forward(model.cfg_struct, model.w_struct, tokens.data_ptr(), mask.data_ptr(), B, S,
                                                   training, 1, 1, out.data_ptr(), ptr, nbytes, _stream()))
            if not training:
                _sync()
                return (out.cpu().numpy(),)
            model.flat_grad.zero_()
            _native.check(lib.sskd_generic_backward(model.cfg_struct, model.w_struct, model.g_struct, tokens.data_ptr(),
                                                    mask.data_ptr(), B, S, 1, dout.data_ptr(), ptr, nbytes, _stream()))
            _sync()
            return out.cpu().numpy(), model.flat_grad.cpu().numpy().copy()

        def cos(a, b):
            a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
            return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))

        def check(outs):
            emb = outs[0]
            assert np.isfinite(emb).all(), (name, "non-finite embeddings")
            worst = min(cos(emb[i], want_e[i]) for i in range(B))
            assert worst >= 0.999, (name, "embedding cosine", worst)
            if not training:
                return
            flat = outs[1]
            assert np.isfinite(flat).all(), (name, "non-finite gradients")
            top = max(np.abs(v).max() for v in want_g.values())
            for pname in model.names:
                o, shape = model._layout[pname]
                got, ref = flat[o: o + int(np.prod(shape))].reshape(shape), want_g[pname]
                if np.abs(ref).max() < 1e-6 * top:
                    assert np.abs(got).max() < 2e-2 * top, (name, pname)
                    continue
                assert cos(got, ref) >= 0.999, (name, pname, cos(got, ref))
                assert abs(np.linalg.norm(got) / np.linalg.norm(ref) - 1.0) < 0.03, (name, pname, "norm")

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, idb), check)

    # the backward accumulates weight gradients with float atomics: its bits depend on their order
    return Shape(name, setup, not training, FP64_TOLERANCE)


def _teacher_shape(name):
    def setup(lib):
        import sys

        from conftest import GOLDEN
        from semantic_search_kd_amd import TeacherModel, _native

        sys.path.insert(0, str(GOLDEN))
        from make_golden import teacher_case
        from test_teacher_gpu import LOGIT_ATOL

        gold = np.load(GOLDEN / "xlmr_small.npz")
        cfg, sd, ids, mask = teacher_case()
        teacher = TeacherModel("synthetic", "cuda:0", config=cfg, state_dict=sd)
        d_ids, _ = _native.padded_ids_mask(*teacher._to_device_i32(ids, mask), teacher.torch_device, pad_id=cfg.pad_token_id)
        Bp, Sp = -(-d_ids.shape[0] // 8) * 8, d_ids.shape[1]        # TeacherModel.score_token_ids pads the batch to 8 rows
        need = int(lib.sskd_teacher_workspace_bytes(teacher._cfg, Bp, Sp))
        ids_big = np.where(mask != 0, np.maximum((ids.astype(np.int64) * 5 + 11) % cfg.vocab_size, 4), ids).astype(ids.dtype)

        def run(lib, ptr, nbytes, tokens=ids):
            teacher._workspace = lent = Borrowed(ptr, nbytes)
            try:
                got = teacher.score_token_ids(tokens, mask)
                _sync()
                assert teacher._workspace is lent, (name, "the teacher did not run on the workspace it was lent")
            finally:
                teacher._workspace = None
            return (got.cpu().numpy(),)

        def check(outs):
            assert np.abs(outs[0] - gold["logits"]).max() <= LOGIT_ATOL, (name, outs[0].tolist(), gold["logits"].tolist())

        return Run(need, run, lambda lib, ptr, nbytes: run(lib, ptr, nbytes, ids_big), check)

    return Shape(name, setup, True, FP64_TOLERANCE)


# ---------------------------------------------------------------------------------------------------------------------
# one entry per size query of include/sskd_amd.h (test_workspace_contract_host.py holds the list to _native's table)
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "sskd_index_search_workspace_bytes": [
        _exact_shape("n1_k10", 1, 3, 10),
        _exact_shape("n31_k10", 31, 3, 10),
        _exact_shape("reduce_buffers", REDUCE_MIN_ROWS, REDUCE_NQ, REDUCE_K),
        _exact_shape("n31_k100_chained", 31, 33, 100),
    ],
    "sskd_index_search_workspace_bytes_ex": _scan_case_shapes(),
    "sskd_index_search_onepass_workspace_bytes": [
        _onepass_shape("nq1_k1", 3001, 1, 1),
        _onepass_shape("nq64_k256", 3001, 64, 256),
        _onepass_shape("n5_k10", 5, 3, 10),
        _onepass_shape("nq3_k10_masked", 3001, 3, 10, mask="half"),
    ],
    "sskd_index_search_screened_workspace_bytes": _screen_case_shapes(),
    "sskd_index_range_search_workspace_bytes": [
        _range_shape("nq3_under_cap", 3001, 3, False),
        _range_shape("nq33_under_cap", 3001, 33, False),
        _range_shape("nq3_over_cap", 3001, 3, True),
        _range_shape("nq33_over_cap", 3001, 33, True),
    ],
    "sskd_range_merge_workspace_bytes": [_range_merge_shape("two_runs", False), _range_merge_shape("two_runs_overflow", True)],
    "sskd_index_search_grouped_workspace_bytes": [
        _grouped_shape("default_k_rows", 3001, 33, 10, None, None, False),
        _grouped_shape("unproved", 3001, 3, 10, 12, 4, True),
    ],
    "sskd_bm25_search_workspace_bytes": [_bm25_shape("whole", False), _bm25_shape("one_query_chunks", True)],
    "sskd_ivf_search_workspace_bytes": [_ivf_shape("nq33_k10_nprobe4", 33, 10, 4), _ivf_shape("nq3_k256_nprobe1", 3, 256, 1)],
    "sskd_pq_search_workspace_bytes": [_pq_shape("adc", 9, 10, 4, 0), _pq_shape("refine100", 9, 10, 4, 100)],
    "sskd_graph_search_workspace_bytes": [_graph_shape("no_workspace")],
    "sskd_late_rerank_workspace_bytes": [_late_shape("nq3_R100", False)],
    "sskd_latec_rerank_workspace_bytes": [_late_shape("nq3_R100", True)],
    "sskd_plaid_candidates_workspace_bytes": [_plaid_shape("whole", False), _plaid_shape("one_query_chunks", True)],
    "sskd_encoder_workspace_bytes": [_encoder_shape("padded_ragged", "nkt3_spw2", False), _encoder_shape("packed", "packed", True)],
    "sskd_generic_workspace_bytes": [_generic_shape("forward_inference", 0), _generic_shape("forward_backward_training", 1)],
    "sskd_teacher_workspace_bytes": [_teacher_shape("xlmr_small")],
}


def all_runs():
    """``(entry, shape)`` pairs in table order"""
    return [(entry, shape) for entry, shapes in CASES.items() for shape in shapes]
