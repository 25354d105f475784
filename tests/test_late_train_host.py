"""Training through MaxSim, no GPU: the NumPy restatements of the gradient kernels (tests/late_train_cases.py) agree with
fp64 within DERIVED bounds (the derivations stand next to ``sum_bound`` and ``pack_bwd64``), and the fp64 gather
formulation ``sum_i <q_i, d_arg(i)>`` under torch autograd reproduces the fp64 references - what the kernels compute is
MaxSim's subgradient at the argmax they are given."""
import numpy as np
import pytest
import torch

import late_cases as lc
import late_train_cases as tc


def _case_with_arg(shape):
    name, tqs, tds, R = shape
    q_bits, q_lims, d_bits, d_lims, cand = tc.random_case(1000 + R, tqs, tds, R)
    arg, _, _ = tc.argmax64(q_bits, q_lims, d_bits, d_lims, cand, tc.tq_stride(q_lims))
    g = np.random.default_rng(7).standard_normal(cand.shape).astype(np.float32) * np.float32(3.0)
    return q_bits, q_lims, d_bits, d_lims, cand, arg, g


@pytest.mark.parametrize("shape", tc.SHAPES, ids=lambda s: s[0])
def test_gradient_restatements_agree_with_fp64_within_the_derived_bound(shape):
    q_bits, q_lims, d_bits, d_lims, cand, arg, g = _case_with_arg(shape)
    for got, (ref, mag, n) in ((tc.dq_rows(d_bits, d_lims, q_lims, cand, arg, g), tc.dq64(d_bits, d_lims, q_lims, cand, arg, g)),
                               (tc.dd_rows(q_bits, q_lims, d_lims, cand, arg, g), tc.dd64(q_bits, q_lims, d_lims, cand, arg, g))):
        err = np.abs(got.astype(np.float64) - ref)
        bound = tc.sum_bound(mag, n)
        assert (err <= bound).all(), float((err - bound).max())
        assert not got[n == 0].any(), "a row without contributions is exact zeros"
        assert n.max() >= 1


def test_absent_pairs_never_enter_the_arithmetic():
    q_bits, q_lims, d_bits, d_lims, cand, arg, g = _case_with_arg(tc.SHAPES[1])
    absent = (arg[:, :, 0] < 0)
    assert absent.any() and not absent.all()
    poisoned = g.copy()
    poisoned[absent] = np.nan
    assert np.array_equal(tc.dq_rows(d_bits, d_lims, q_lims, cand, arg, g), tc.dq_rows(d_bits, d_lims, q_lims, cand, arg, poisoned))
    got = tc.dd_rows(q_bits, q_lims, d_lims, cand, arg, poisoned)
    assert np.isfinite(got).all() and np.array_equal(got, tc.dd_rows(q_bits, q_lims, d_lims, cand, arg, g))
    # the document nobody names (the last one) receives exact zeros
    assert not got[d_lims[-2]:].any()


def test_pack_backward_restatement_agrees_with_fp64_within_the_derived_bound():
    hidden, lengths, dtok = tc.pack_bwd_case()
    got = lc.bf16_values(tc.pack_bwd_rows(hidden, lengths, dtok)).astype(np.float64)
    ref, bound = tc.pack_bwd64(hidden, lengths, dtok)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    for b, L in enumerate(lengths):
        assert not got[b, L:].any()
    assert np.abs(got[0, 3]).max() > 0      # the zero row: n = 1e-12, dh = g / n


@pytest.mark.parametrize("shape", tc.SHAPES[1:3], ids=lambda s: s[0])
def test_autograd_of_the_gather_formulation_reproduces_the_fp64_references(shape):
    q_bits, q_lims, d_bits, d_lims, cand, arg, g = _case_with_arg(shape)
    q = torch.from_numpy(lc.bf16_values(q_bits).reshape(-1, tc.DIM).astype(np.float64)).requires_grad_(True)
    d = torch.from_numpy(lc.bf16_values(d_bits).reshape(-1, tc.DIM).astype(np.float64)).requires_grad_(True)
    scores = tc.gather_scores_torch(q, q_lims, d, d_lims, cand, arg)
    # the gather at the fp64 argmax IS MaxSim on every present pair
    ref = lc.Reference(q_bits, q_lims, d_bits, d_lims)
    want = ref.of_candidates(ref.s64, cand)
    present = np.isfinite(want)
    assert np.allclose(scores.detach().numpy()[present], want[present], rtol=0, atol=1e-12)
    (scores * torch.from_numpy(g.astype(np.float64))).sum().backward()
    for got, (want_g, mag, _) in ((q.grad.numpy(), tc.dq64(d_bits, d_lims, q_lims, cand, arg, g)),
                                  (d.grad.numpy(), tc.dd64(q_bits, q_lims, d_lims, cand, arg, g))):
        assert (np.abs(got - want_g) <= 1e-13 * (mag + 1e-300) * 64).all()


def test_pack_backward_is_the_derivative_of_the_normalisation():
    hidden, lengths, dtok = tc.pack_bwd_case()
    ref, _ = tc.pack_bwd64(hidden, lengths, dtok)
    lims = tc.lims_of(lengths)
    for b in (1, 2):
        L = int(lengths[b])
        x = torch.from_numpy(lc.bf16_values(hidden[b, :L]).reshape(L, tc.DIM).astype(np.float64)).requires_grad_(True)
        y = x / x.norm(dim=1, keepdim=True)
        (y * torch.from_numpy(dtok[lims[b]: lims[b + 1]].astype(np.float64))).sum().backward()
        # the reference divides by the pack's fp32 n, autograd by the fp64 norm: they differ by fp32's rounding of n, twice
        assert np.allclose(x.grad.numpy(), ref[b, :L], rtol=0, atol=4 * 2.0 ** -23 * np.abs(ref[b, :L]).max() + 1e-300)


def test_generated_families_hold_what_the_gpu_tests_rely_on():
    # separated: the fp64 gap between best and second best exceeds twice the per-dot term for every (q, c, i)
    q_bits, q_lims, d_bits, d_lims, cand = tc.separated_case()
    arg, best, second = tc.argmax64(q_bits, q_lims, d_bits, d_lims, cand, tc.tq_stride(q_lims))
    live = arg >= 0
    assert live.any() and (best[live] - second[live] > 2 * tc.dot_term(q_bits, d_bits)).all()
    # ties: the two copies are the maximum for query token 2, and fp64's first argmax is the earlier one
    q_bits, q_lims, d_bits, d_lims, cand, expect = tc.tie_case()
    arg, best, second = tc.argmax64(q_bits, q_lims, d_bits, d_lims, cand, 32)
    assert [int(arg[0, c, 2]) for c in range(cand.shape[1])] == expect
    assert (best[0, :, 2] == second[0, :, 2]).all()
    # the random shapes hold an absent entry, an id outside the batch, a duplicate, a shared and an unnamed document
    _, _, _, d_lims, cand = tc.random_case(5, [31, 32, 33], [1, 31, 32, 33, 65, 180], 5)
    nd = d_lims.size - 1
    assert (cand == -1).any() and (cand >= nd).any() and cand[0, 4] == cand[0, 0]
    assert nd - 1 not in cand and len(set(cand[:, 0]) & set(cand[:, 3])) >= 1
