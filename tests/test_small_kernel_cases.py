"""CPU side of tests/test_small_kernels_gpu.py: the bounds of tests/small_kernel_cases.py are neither slack nor tuned.

1. For every kernel and case an fp32 numpy evaluation in the kernel's own order (lane assignment, butterflies, strided
   sums; ``*_emulate``) stays inside the bound of the fp64 reference.  The largest error / bound per kernel is printed
   (``python -m pytest -s``) and must not exceed 0.5: a bound that an ideal fp32 evaluation half fills would leave
   no room for the GPU's math library.
2. Every planted defect (``defect=`` of the references) leaves the bound on at least one case of its kernel.
3. The references agree with what pins them: oracle.scores_fma bit for bit, tests/golden/pool_norm.npz within its 2e-6,
   oracle/kd_losses.py itself for the KD losses.
"""
import numpy as np
import pytest

import small_kernel_cases as kc
from conftest import GOLDEN
from oracle import kd_losses as kd
from oracle import search as oracle

HALF = 0.5


def _report(kernel, worst, where):
    print(f"{kernel}: largest fp32-emulation error / bound = {worst:.3f} at {where}")
    assert worst <= HALF, f"{kernel}: error / bound = {worst:.3f} at {where}; re-derive the depth"


# ---- KD loss ---------------------------------------------------------------------------------------------------------
def _kd_ratio(got, ref, bound):
    return max(kc.ratio(got[0], ref[0], bound[0]), kc.ratio(got[1], ref[1], bound[1]))


@pytest.mark.parametrize("B,D", kc.KD_SHAPES)
def test_kd_emulation_inside_bound(B, D):
    worst, where = 0.0, None
    for regime, T, tau, w in kc.kd_combos():
        s, t = kc.kd_inputs(B, D, regime, T)
        r = _kd_ratio(kc.kd_emulate(s, t, T, tau, w), kc.kd_reference(s, t, T, tau, w), kc.kd_bound(s, t, T, tau, w))
        if r > worst:
            worst, where = r, (regime, T, tau, w)
    _report(f"kd_loss B={B} D={D}", worst, where)


def test_kd_reference_is_the_oracle():
    s, t = kc.kd_inputs(5, 9, "cosine", 2.0)
    losses, grad = kc.kd_reference(s, t, 2.0, 0.05, (0.6, 0.2, 0.2))
    out, g = kd.combined(s, t, 2.0, tuple(float(np.float32(x)) for x in (0.6, 0.2, 0.2)), float(np.float32(0.05)))
    assert np.array_equal(grad, g) and losses.tolist() == [out[k] for k in kc.KD_LOSS_NAMES]
    # the row quantities the bounds are built on restate the same losses
    o = kc._kd_rows64(s, t, 2.0, float(np.float32(0.05)))
    np.testing.assert_allclose([o["sum_r2"].sum() / 45, o["kl"].sum() / 5 * 4, o["nll"].sum() / 5], losses[1:], rtol=1e-12)


@pytest.mark.parametrize("defect,shapes", [
    ("last_tie", [(5, 9), (1, 64)]), ("T_not_T2", [(5, 9)]), ("mean_over_B", [(5, 9)]),
    ("drop_rows_1024", [(1024, 9), (1025, 9)]),
])
def test_kd_defects_leave_the_bound(defect, shapes):
    caught = []
    for (B, D) in shapes:
        for regime, T, tau, w in kc.kd_combos():
            if T == 1.0 and defect == "T_not_T2":
                continue                                        # T = T^2 there
            s, t = kc.kd_inputs(B, D, regime, T)
            if _kd_ratio(kc.kd_reference(s, t, T, tau, w, defect), kc.kd_reference(s, t, T, tau, w), kc.kd_bound(s, t, T, tau, w)) > 1:
                caught.append((B, D, regime, T, tau, w))
    print(f"kd defect {defect}: caught on {len(caught)} cases, first {caught[:1]}")
    assert caught
    if defect == "drop_rows_1024":
        assert all(B > 1024 for (B, *_rest) in caught), "B = 1024 has no second stride"
    if defect == "last_tie":
        assert all(c[2] == "ties" for c in caught)


# ---- teacher head ----------------------------------------------------------------------------------------------------
def test_head_emulation_inside_bound():
    worst, where = 0.0, None
    for c in kc.HEAD_CASES:
        W, hid = kc.head_weights(c["H"]), kc.head_cpu_hidden(c)
        o = kc.head_reference(hid, W)
        r = kc.ratio(kc.head_emulate(hid, W), o["ref"], kc.head_bound(o, W))
        if r > worst:
            worst, where = r, kc.head_name(c)
    _report("teacher_head", worst, where)


@pytest.mark.parametrize("defect", ["no_dense_b", "stride_H", "rows_ge_64"])
def test_head_defects_leave_the_bound(defect):
    caught = []
    for c in kc.HEAD_CASES:
        W, hid = kc.head_weights(c["H"]), kc.head_cpu_hidden(c)
        o = kc.head_reference(hid, W)
        if kc.ratio(kc.head_reference(hid, W, defect)["ref"], o["ref"], kc.head_bound(o, W)) > 1:
            caught.append(kc.head_name(c))
    print(f"head defect {defect}: caught on {caught}")
    assert caught
    if defect == "stride_H":
        assert all(not n.endswith("B1") for n in caught)
    if defect == "rows_ge_64":
        assert all(not n.startswith("H32_") for n in caught)


# ---- pool ------------------------------------------------------------------------------------------------------------
def _pool_cases():
    for S in kc.POOL_S:
        for B in kc.POOL_B:
            for mk in kc.POOL_MASKS:
                for bf16 in (False, True):
                    for normalize in (False, True):
                        yield S, B, mk, bf16, normalize


def test_pool_emulation_inside_bound():
    worst, where = 0.0, None
    for case in _pool_cases():
        S, B, mk, bf16, normalize = case
        h, m = kc.pool_inputs(S, B, mk, bf16)
        o = kc.pool_reference(h, m, normalize)
        got = kc.pool_emulate(h, m, normalize)
        if mk == "zero":
            assert not got.any() and not o["ref"].any()
        r = kc.ratio(got, o["ref"], kc.pool_bound(o, S, normalize))
        if r > worst:
            worst, where = r, case
    _report("pool_normalize", worst, where)


@pytest.mark.parametrize("defect", ["divide_by_S", "clamp_mask", "drop_tail_groups"])
def test_pool_defects_leave_the_bound(defect):
    caught = []
    for case in _pool_cases():
        S, B, mk, bf16, normalize = case
        h, m = kc.pool_inputs(S, B, mk, bf16)
        o = kc.pool_reference(h, m, normalize)
        if kc.ratio(kc.pool_reference(h, m, normalize, defect)["ref"], o["ref"], kc.pool_bound(o, S, normalize)) > 1:
            caught.append(case)
    print(f"pool defect {defect}: caught on {len(caught)} cases, first {caught[:1]}")
    assert caught
    if defect == "clamp_mask":
        assert all(c[2] == "weighted" for c in caught)
    if defect == "drop_tail_groups":
        assert all(c[0] % 4 != 0 for c in caught)


def test_pool_reference_matches_golden():
    gold = np.load(GOLDEN / "pool_norm.npz")
    g = np.random.Generator(np.random.PCG64(int(gold["seed"])))
    h = g.standard_normal((8, 64, 384), dtype=np.float32)
    mask = np.zeros((8, 64), np.int32)
    for b, n in enumerate(gold["lengths"]):
        mask[b, :n] = 1
    for normalize, key in ((True, "normalized"), (False, "pooled")):
        np.testing.assert_allclose(kc.pool_reference(h, mask, normalize)["ref"], gold[key], rtol=0, atol=2e-6)
        np.testing.assert_allclose(kc.pool_emulate(h, mask, normalize), gold[key], rtol=0, atol=2e-6)


# ---- similarity ------------------------------------------------------------------------------------------------------
def test_similarity_reference_is_the_oracle_chain():
    """Bit for bit oracle.scores_fma at 384 (and at the other widths: the C oracle takes any dim % 8 == 0)."""
    for dim in kc.SIM_DIMS:
        q, d = kc.sim_inputs(33, 31, dim)
        assert np.array_equal(kc.sim_reference(q, d).view(np.int32), oracle.scores_fma(q, d).view(np.int32)), dim


def test_fma32_is_a_correctly_rounded_fma():
    """a * b + c = 2^30 + 192 - 2^-40 lies just below an fp32 tie.  The fp64 sum rounds onto the tie, and rounding that to
    fp32 goes to even, the wrong neighbour; fma32 must give what one rounding gives."""
    a, b, c = np.float32(8 + 2.0 ** -20), np.float32(8 - 2.0 ** -20), np.float32(2.0 ** 30 + 128)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(2.0 ** 30 + 256)
    assert kc.fma32(a, b, c) == np.float32(2.0 ** 30 + 128)
    assert kc.fma32(-a, b, -c) == np.float32(-(2.0 ** 30 + 128))


def test_similarity_defect_changes_bits():
    changed = 0
    for dim in kc.SIM_DIMS:
        q, d = kc.sim_inputs(33, 31, dim)
        changed += int((kc.sim_reference(q, d, "swap_last_two").view(np.int32) != kc.sim_reference(q, d).view(np.int32)).sum())
    print(f"similarity defect swap_last_two: {changed} outputs change bits")
    assert changed > 0


# ---- l2 normalise / index add ----------------------------------------------------------------------------------------
def test_l2_emulation_inside_bound():
    worst, where = 0.0, None
    for dim in kc.L2_DIMS:
        for n in kc.L2_ROWS:
            x, kind = kc.l2_inputs(n, dim)
            got, ref = kc.l2_emulate(x), kc.l2_reference(x)["ref"]
            rnd = kind == kc.KIND_RANDOM
            r = kc.ratio(got[rnd], ref[rnd], kc.l2_bound(ref[rnd], kc.l2_depth(dim)))
            for k in (kc.KIND_ZERO, kc.KIND_TINY):
                assert np.array_equal(got[kind == k].view(np.int32), x[kind == k].view(np.int32))
            assert not got[kind == kc.KIND_HUGE].any()          # x * (1 / sqrt(inf)) = x * 0
            if r > worst:
                worst, where = r, (n, dim)
    _report("l2_normalize_rows", worst, where)
    worst, where = 0.0, None
    for n in kc.ADD_ROWS_N:
        x, kind = kc.l2_inputs(n, 384, specials=False)
        ref = kc.l2_reference(x)["ref"]
        r = kc.ratio(kc.add_rows_emulate(x), ref, kc.l2_bound(ref, kc.ADD_ROWS_DEPTH))
        if r > worst:
            worst, where = r, n
    _report("index_add_rows(normalize)", worst, where)


def test_l2_defect_leaves_the_bound():
    caught = []
    for dim in kc.L2_DIMS:
        x, kind = kc.l2_inputs(5, dim)
        rnd = kind == kc.KIND_RANDOM
        ref = kc.l2_reference(x)["ref"][rnd]
        if kc.ratio(kc.l2_reference(x, "ss_first_64")["ref"][rnd], ref, kc.l2_bound(ref, kc.l2_depth(dim))) > 1:
            caught.append(dim)
    print(f"l2 defect ss_first_64: caught at dim {caught}")
    assert caught == [d for d in kc.L2_DIMS if d > 64]


# ---- masks -----------------------------------------------------------------------------------------------------------
def test_mask_models():
    from semantic_search_kd_amd.index import mask_words

    caught = []
    for n in kc.MASK_ROWS:
        flags = kc.mask_flags(n)
        packed = kc.mask_pack_reference(flags)
        assert len(packed) == kc.mask_words(n)
        assert np.array_equal(packed, mask_words(flags != 0, n))      # the host packer of tests/test_row_filter.py
        ids = kc.mask_ids(n)
        on, bad = kc.mask_update_reference(np.zeros_like(packed), n, ids, True)
        assert bad == 3 and kc.mask_count_reference(on, n) == len(set(i for i in ids.tolist() if 0 <= i < n))
        off, bad = kc.mask_update_reference(on, n, ids, False)
        assert bad == 3 and not off.any()
        w = kc.mask_dirty_tail(n)
        if kc.mask_count_reference(w, n, "tail_unmasked") != kc.mask_count_reference(w, n):
            caught.append(n)
    print(f"mask count defect tail_unmasked: caught at n_rows {caught}")
    assert caught == [n for n in kc.MASK_ROWS if n % 32]
