"""Isolated parity of the small kernels that sit on every product path, each through its C-ABI entry point on its own
inputs (tests/small_kernel_cases.py holds the inputs, the fp64 references and the derived bounds; none is calibrated on a
GPU result, and tests/test_small_kernel_cases.py shows on the CPU that each is tight enough to catch its planted defects):

  sskd_kd_loss                kd_loss_rows_kernel + kd_loss_finish_kernel      fp64 oracle/kd_losses.py, derived bound
  sskd_teacher_score (L = 0)  teacher_head_kernel on the encoder's own <s> state  fp64, derived bound
  sskd_pool_normalize         pool_normalize_kernel<fp32 / bf16>               fp64, derived bound
  sskd_similarity             similarity_kernel                                bit for bit oracle.scores_fma
  sskd_l2_normalize_rows      l2_normalize_rows_kernel                         fp64, derived bound
  sskd_index_add_rows(1)      index_add_rows_kernel (+ sskd_index_get_rows)    fp64, derived bound; padding exact zeros
  sskd_row_mask_*             pack / update / and / count                      numpy bit model

Every device output buffer ends in a canary tail of 64 elements that must come back unchanged.  A failure names the worst
element: index, got, reference, bound.
"""
import numpy as np
import pytest
import torch

import small_kernel_cases as kc
from capi_helpers import stream
from oracle import search as oracle
from semantic_search_kd_amd import _native

pytestmark = pytest.mark.gpu

TAIL = 64
CANARY = {torch.float32: -1234.5, torch.bfloat16: -1232.0, torch.int32: -1515870811, torch.int64: -6148914691236517206,
          torch.uint8: 0xA5}


def _buf(n, dtype=torch.float32, body=None):
    """n elements + the canary tail; the body starts as canary too (``body`` overrides), so 'wrote nothing' is visible."""
    t = torch.full((n + TAIL,), CANARY[dtype], dtype=dtype, device="cuda")
    if body is not None:
        t[:n] = torch.from_numpy(np.ascontiguousarray(body).reshape(-1)).to(dtype=dtype, device="cuda")
    return t


def _untouched(t, lo=None):
    """The canary tail (or everything from ``lo``) is unchanged."""
    lo = t.numel() - TAIL if lo is None else lo
    return bool((t[lo:] == CANARY[t.dtype]).all())


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _within(got, ref, bound, what):
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    bound = np.broadcast_to(bound, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    if bad.any():
        excess = np.where(bad, np.nan_to_num(err - bound, nan=np.inf), -1.0)
        idx = np.unravel_index(int(np.argmax(excess)), ref.shape)
        pytest.fail(f"{what}: {int(bad.sum())} of {ref.size} elements out of bound; worst at {idx}: got {got[idx]!r}, "
                    f"ref {ref[idx]!r}, bound {bound[idx]:.3e}")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# sskd_kd_loss
# ----------------------------------------------------------------------------------------------------------------------
def _kd_call(lib, s, t, T, tau, w, with_grad=True, B=None, D=None):
    """-> rc, losses [4], grad [B, D] or None; asserts the canary tails of all three buffers."""
    B0, D0 = s.shape
    ds, dt = _up(s), _up(t)
    losses, grad, rows = _buf(4), _buf(B0 * D0), _buf(3 * B0)
    rc = lib.sskd_kd_loss(ds.data_ptr(), dt.data_ptr(), B0 if B is None else B, D0 if D is None else D, T, tau, w[0], w[1], w[2],
                          losses.data_ptr(), grad.data_ptr() if with_grad else None, rows.data_ptr(), stream())
    torch.cuda.synchronize()
    assert _untouched(losses) and _untouched(grad) and _untouched(rows), "kd_loss wrote past a buffer"
    return rc, losses, grad


@pytest.mark.parametrize("B,D", kc.KD_SHAPES)
def test_kd_loss_against_fp64(gpu, native_lib, B, D):
    """The four losses and the gradient against oracle/kd_losses.py in fp64, for T in {1, 2, 4}, tau in {0.05, 1}, the
    default weights and each one-hot triple, in the training regime, with tied row maxima (the margin-MSE gradient of the
    maximum belongs to the FIRST maximal lane), with student = teacher / T (margin-MSE exactly 0) and at spread 1e3 with
    tau = 1e-3.  B = 1023 / 1024 / 1025 sit either side of the finish kernel's second stride, 2049 and 4100 reach the third
    and fifth.  Two calls are bit-equal (the header of csrc/kd_loss.hip promises a fixed order)."""
    for regime, T, tau, w in kc.kd_combos():
        s, t = kc.kd_inputs(B, D, regime, T)
        what = f"kd_loss B={B} D={D} {regime} T={T} tau={tau} w={w}"
        rc, losses, grad = _kd_call(native_lib, s, t, T, tau, w)
        _native.check(rc)
        got_l, got_g = losses[:4].cpu().numpy(), grad[:B * D].cpu().numpy().reshape(B, D)
        ref_l, ref_g = kc.kd_reference(s, t, T, tau, w)
        bound_l, bound_g = kc.kd_bound(s, t, T, tau, w)
        _within(got_l, ref_l, bound_l, what + " losses")
        _within(got_g, ref_g, bound_g, what + " gradient")
        if regime == "zero_mm":
            assert got_l[1] == 0.0, f"{what}: margin-MSE of student = teacher / T is {got_l[1]!r}"
        if D == 1:
            assert not got_l[1:].any() and not got_g.any(), f"{what}: one document has nothing to rank: {got_l}, {got_g.ravel()}"
        rc, losses2, grad2 = _kd_call(native_lib, s, t, T, tau, w)
        _native.check(rc)
        assert torch.equal(losses2.view(torch.int32), losses.view(torch.int32)), what + ": losses differ between two calls"
        assert torch.equal(grad2.view(torch.int32), grad.view(torch.int32)), what + ": gradient differs between two calls"


def test_kd_loss_without_gradient_and_bad_arguments(gpu, native_lib):
    """d_grad = NULL returns the same losses bit for bit (and touches no gradient buffer); n_docs = 65, batch = 0 and a
    zero temperature return an error code and leave d_losses alone."""
    s, t = kc.kd_inputs(5, 9, "cosine", 2.0)
    w = kc.KD_WEIGHTS[0]
    rc, with_g, _ = _kd_call(native_lib, s, t, 2.0, 0.05, w)
    _native.check(rc)
    rc, without, grad = _kd_call(native_lib, s, t, 2.0, 0.05, w, with_grad=False)
    _native.check(rc)
    assert torch.equal(with_g.view(torch.int32), without.view(torch.int32))
    assert _untouched(grad, 0)
    s65, t65 = np.zeros((2, 65), np.float32), np.zeros((2, 65), np.float32)
    for kw, (a, b, T) in (("n_docs=65", (s65, t65, 2.0)), ("batch=0", (s, t, 2.0)), ("temperature=0", (s, t, 0.0))):
        rc, losses, grad = _kd_call(native_lib, a, b, T, 0.05, w, B=0 if kw == "batch=0" else None)
        assert rc != 0, kw
        assert _untouched(losses, 0) and _untouched(grad, 0), f"{kw}: an error return wrote to its outputs"


# ----------------------------------------------------------------------------------------------------------------------
# teacher_head_kernel behind a zero-layer encoder
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.HEAD_CASES, ids=kc.head_name)
def test_teacher_head_against_fp64(gpu, native_lib, case):
    """layers = 0 isolates the head: sskd_generic_forward(pool = 0) returns the bf16 embedding-LayerNorm output, the very
    values the head reads, and sskd_teacher_score on the same inputs must give out_w . tanh(dense_w . h[b, 0] + dense_b) +
    out_b of THOSE values within the fp32 bound.  H = 32 leaves waves 8-15 idle, 352 half fills the second lane stride,
    S = 64 against S = 32 at H = 96 catches a token-0 stride of H; biases of order 1 and row-scaled dense_w catch a dropped
    bias and a row permutation.  Two calls are bit-equal (fixed-order reduction)."""
    H, S, B = case["H"], case["S"], case["B"]
    lib, m, W = native_lib, kc.head_model_inputs(case), kc.head_weights(case["H"])
    cfg = _native.GenericConfig(kc.HEAD_VOCAB, H, 0, case["heads"], 4 * H, S, 1, 1e-5, 0)
    keep = {k: _up(m[k]).to(torch.bfloat16).contiguous() for k in ("word", "pos", "type")}
    keep.update({k: _up(m[k]) for k in ("ln_g", "ln_b", "ids", "mask")})
    keep.update({k: _up(v) for k, v in W.items()})
    w = _native.GenericWeights()
    w.word_emb, w.pos_emb, w.type_emb = keep["word"].data_ptr(), keep["pos"].data_ptr(), keep["type"].data_ptr()
    w.emb_ln_g, w.emb_ln_b = keep["ln_g"].data_ptr(), keep["ln_b"].data_ptr()
    need = int(lib.sskd_generic_workspace_bytes(cfg, B, S, 0))
    assert need > 0 and int(lib.sskd_teacher_workspace_bytes(cfg, B, S)) == need
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    hid = _buf(B * S * H, torch.bfloat16)
    _native.check(lib.sskd_generic_forward(cfg, w, keep["ids"].data_ptr(), keep["mask"].data_ptr(), B, S, 0, 0, 0, hid.data_ptr(),
                                           ws.data_ptr(), ws.numel(), stream()))
    runs = []
    for _ in range(2):
        logits = _buf(B)
        _native.check(lib.sskd_teacher_score(cfg, w, keep["dense_w"].data_ptr(), keep["dense_b"].data_ptr(), keep["out_w"].data_ptr(),
                                             keep["out_b"].data_ptr(), keep["ids"].data_ptr(), keep["mask"].data_ptr(), B, S,
                                             logits.data_ptr(), ws.data_ptr(), ws.numel(), stream()))
        torch.cuda.synchronize()
        assert _untouched(logits)
        runs.append(logits[:B].cpu().numpy())
    assert _untouched(hid)
    hidden = hid[:B * S * H].float().cpu().numpy().reshape(B, S, H).astype(np.float64)
    assert np.isfinite(hidden).all() and np.abs(hidden[:, 0]).max() > 0.1
    if B > 1:
        assert np.abs(hidden[1, 0] - hidden[0, 0]).max() > 0.1, "the <s> states of the sequences must differ"
    o = kc.head_reference(hidden, W)
    _within(runs[0], o["ref"], kc.head_bound(o, W), f"teacher_head {kc.head_name(case)}")
    assert np.array_equal(_bits(runs[0]), _bits(runs[1])), "two calls differ"


# ----------------------------------------------------------------------------------------------------------------------
# sskd_pool_normalize
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("S", kc.POOL_S)
def test_pool_normalize_against_fp64(gpu, native_lib, S, bf16):
    """fp64 sum_t m_t h_t / max(sum_t m_t, 1e-9), then optionally / max(|e|, 1e-12), on the fp32 values or on the
    bf16-rounded ones.  S below, at and off the four token groups; prefix, scattered and last-token-only masks; an
    all-zero mask gives exactly 0.  The ``weighted`` masks hold integers in {0, 1, 2, 3}: the kernel weights by
    (float) mask[t], i.e. computes a WEIGHTED mean, which is what the formula in the header of csrc/pool.hip says; this
    test pins that behaviour (a caller that wants a 0 / 1 mask passes one)."""
    for B in kc.POOL_B:
        for mk in kc.POOL_MASKS:
            h, m = kc.pool_inputs(S, B, mk, bf16)
            dh = _up(h).to(torch.bfloat16) if bf16 else _up(h)
            dm = _up(m)
            for normalize in (0, 1):
                out = _buf(B * kc.POOL_H)
                _native.check(native_lib.sskd_pool_normalize(dh.data_ptr(), int(bf16), dm.data_ptr(), B, S, normalize, out.data_ptr(), stream()))
                torch.cuda.synchronize()
                assert _untouched(out)
                got = out[:B * kc.POOL_H].cpu().numpy().reshape(B, kc.POOL_H)
                o = kc.pool_reference(h, m, bool(normalize))
                _within(got, o["ref"], kc.pool_bound(o, S, bool(normalize)), f"pool S={S} B={B} {mk} bf16={bf16} normalize={normalize}")
                if mk == "zero":
                    assert not got.any(), "the mean of nothing must be exactly 0"
    out = _buf(kc.POOL_H)
    _native.check(native_lib.sskd_pool_normalize(dh.data_ptr(), int(bf16), dm.data_ptr(), 0, S, 1, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert _untouched(out, 0), "B = 0 wrote something"


# ----------------------------------------------------------------------------------------------------------------------
# sskd_similarity
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", kc.SIM_DIMS)
def test_similarity_bit_equal_to_the_oracle(gpu, native_lib, dim):
    """Every (nq, nd) around the 32 x 32 output block, bit for bit oracle.scores_fma; the rows the kernel clamps
    out-of-range lanes to (nq - 1, nd - 1) carry values 16 x larger than the rest."""
    for nq, nd in kc.SIM_PAIRS:
        q, d = kc.sim_inputs(nq, nd, dim)
        dq, dd, out = _up(q), _up(d), _buf(nq * nd)
        _native.check(native_lib.sskd_similarity(dq.data_ptr(), nq, dd.data_ptr(), nd, dim, out.data_ptr(), stream()))
        torch.cuda.synchronize()
        assert _untouched(out)
        got, want = out[:nq * nd].cpu().numpy().reshape(nq, nd), oracle.scores_fma(q, d)
        diff = _bits(got) != _bits(want)
        assert not diff.any(), (f"similarity nq={nq} nd={nd} dim={dim}: {int(diff.sum())} outputs differ, first at "
                                f"{tuple(np.argwhere(diff)[0])}: {got[diff][0]!r} vs {want[diff][0]!r}")


def test_similarity_bad_and_empty_shapes(gpu, native_lib):
    q, d = kc.sim_inputs(3, 5, 24)
    dq, dd = _up(q), _up(d)
    out = _buf(15)
    assert native_lib.sskd_similarity(dq.data_ptr(), 3, dd.data_ptr(), 5, 12, out.data_ptr(), stream()) != 0   # dim % 8 != 0
    _native.check(native_lib.sskd_similarity(dq.data_ptr(), 0, dd.data_ptr(), 5, 24, out.data_ptr(), stream()))
    _native.check(native_lib.sskd_similarity(dq.data_ptr(), 3, dd.data_ptr(), 0, 24, out.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert _untouched(out, 0)


# ----------------------------------------------------------------------------------------------------------------------
# sskd_l2_normalize_rows, sskd_index_add_rows(normalize = 1) + sskd_index_get_rows
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", kc.L2_DIMS)
def test_l2_normalize_rows_against_fp64(gpu, native_lib, dim):
    """In place, any dim, 1 to 70 rows (four rows per workgroup).  Zero rows stay bit-unchanged; rows of 1e-30 too: the
    fp32 sum of squares underflows to 0 and the row counts as a zero row, as in faiss' fp32 normalize_L2.  Rows of 1e25
    overflow the sum of squares to +inf, 1 / sqrtf(inf) = 0, and the row comes back as zeros: that is what the fp32
    expression x * (1 / sqrt(ss)) gives, pinned here as today's behaviour, not endorsed as a norm."""
    for n in kc.L2_ROWS:
        x, kind = kc.l2_inputs(n, dim)
        buf = _buf(n * dim, body=x)
        _native.check(native_lib.sskd_l2_normalize_rows(buf.data_ptr(), n, dim, stream()))
        torch.cuda.synchronize()
        assert _untouched(buf), "bytes after the last row changed"
        got = buf[:n * dim].cpu().numpy().reshape(n, dim)
        ref = kc.l2_reference(x)["ref"]
        rnd = kind == kc.KIND_RANDOM
        _within(got[rnd], ref[rnd], kc.l2_bound(ref[rnd], kc.l2_depth(dim)), f"l2_normalize n={n} dim={dim}")
        for k, name in ((kc.KIND_ZERO, "zero"), (kc.KIND_TINY, "1e-30")):
            assert np.array_equal(_bits(got[kind == k]), _bits(x[kind == k])), f"n={n} dim={dim}: a {name} row changed"
        assert np.array_equal(_bits(got[kind == kc.KIND_HUGE]), _bits(np.zeros_like(x[kind == kc.KIND_HUGE]))), \
            f"n={n} dim={dim}: a 1e25 row is not +0: {got[kind == kc.KIND_HUGE][:1, :4]}"


@pytest.mark.parametrize("n", kc.ADD_ROWS_N)
def test_index_add_rows_normalized_against_fp64(gpu, native_lib, n):
    """add(normalize = 1) then get: the fp64-normalised rows within the bound, a zero row stays zero, the padding rows of
    the last tile are exact zeros in the (row-major fp32) index buffer, get_rows returns the buffer's bits."""
    x, kind = kc.l2_inputs(n, 384, specials=False)
    padded = int(native_lib.sskd_index_padded_rows(n))
    assert padded == -(-n // 32) * 32 and int(native_lib.sskd_index_tiled_bytes(n)) == padded * 384 * 4
    dx, tiled, back = _up(x), _buf(padded * 384), _buf(n * 384)
    _native.check(native_lib.sskd_index_add_rows(dx.data_ptr(), n, 1, tiled.data_ptr(), 0, stream()))
    _native.check(native_lib.sskd_index_get_rows(tiled.data_ptr(), 0, n, back.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert _untouched(tiled) and _untouched(back)
    buf = tiled[:padded * 384].cpu().numpy().reshape(padded, 384)
    ref = kc.l2_reference(x)["ref"]
    _within(buf[:n], ref, kc.l2_bound(ref, kc.ADD_ROWS_DEPTH), f"index_add_rows n={n}")
    assert np.array_equal(_bits(buf[n:]), np.zeros((padded - n, 384), np.int32)), "padding rows are not exact zeros"
    if n > 1:
        assert kind[1] == kc.KIND_ZERO and not buf[1].any()
    assert np.array_equal(_bits(back[:n * 384].cpu().numpy().reshape(n, 384)), _bits(buf[:n]))


# ----------------------------------------------------------------------------------------------------------------------
# row masks
# ----------------------------------------------------------------------------------------------------------------------
def _words(t, n):
    return t[:n].cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", kc.MASK_ROWS)
def test_row_mask_kernels(gpu, native_lib, n):
    """pack (flag bytes 0, 1, 2, 255) = np.packbits little-endian, exactly sskd_row_mask_words(n) words written; update
    with duplicates, ids 0 and n - 1 and three ids out of range: set then clear follow the numpy bit model, *d_bad is the
    exact out-of-range count and a following call with n_ids = 0 resets it; and = a & b; count ignores the bits at and
    past n_rows even when all of them are set, and is 0 for n_rows = 0."""
    lib = native_lib
    words = int(lib.sskd_row_mask_words(n))
    assert words == kc.mask_words(n)
    flags = kc.mask_flags(n)
    dflags, packed = _up(flags), _buf(words, torch.int32)
    _native.check(lib.sskd_row_mask_pack(dflags.data_ptr(), n, packed.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert _untouched(packed), "pack wrote past sskd_row_mask_words(n) words"
    assert np.array_equal(_words(packed, words), kc.mask_pack_reference(flags))

    ids = kc.mask_ids(n)
    dids = _up(ids)
    mask = _buf(words, torch.int32, body=np.zeros(words, np.int32))
    model = np.zeros(words, np.uint32)
    for allow in (1, 0):
        bad = _buf(1, torch.int32)
        _native.check(lib.sskd_row_mask_update(mask.data_ptr(), n, dids.data_ptr(), len(ids), allow, bad.data_ptr(), stream()))
        torch.cuda.synchronize()
        model, n_bad = kc.mask_update_reference(model, n, ids, bool(allow))
        assert _untouched(mask) and _untouched(bad)
        assert np.array_equal(_words(mask, words), model), f"update allow={allow}"
        assert int(bad[0]) == n_bad == 3
        if allow:
            assert model.any()
    assert not model.any()
    _native.check(lib.sskd_row_mask_update(mask.data_ptr(), n, dids.data_ptr(), 0, 1, bad.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and _untouched(bad) and not _words(mask, words).any()

    a, b = kc.mask_dirty_tail(n), kc.mask_pack_reference(kc.mask_flags(n)[::-1].copy())
    da, db, out = _up(a.view(np.int32)), _up(b.view(np.int32)), _buf(words, torch.int32)
    _native.check(lib.sskd_row_mask_and(da.data_ptr(), db.data_ptr(), n, out.data_ptr(), stream()))
    count = _buf(1, torch.int64)
    _native.check(lib.sskd_row_mask_count(da.data_ptr(), n, count.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert _untouched(out) and np.array_equal(_words(out, words), a & b)
    assert _untouched(count) and int(count[0]) == kc.mask_count_reference(a, n)
    _native.check(lib.sskd_row_mask_count(da.data_ptr(), 0, count.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert int(count[0]) == 0 and _untouched(count)
