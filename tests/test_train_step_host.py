"""CPU: the gate of the composed student step (tests/train_step_cases.py) before it is trusted on the GPU.

  * the faithful chain R (oracle/generic_step.py) is the same function as the exact reference E: its forward agrees with E's
    and its gradients pass the per-tensor gate of tests/test_training_gpu.py (cosine >= 0.999, norms within 3 %);
  * R', the chain with every plain product accumulated in fp32 over a permuted reduction order and added in fp32 into the
    start pattern - what another summation order alone does to a gradient - stays inside the gate on all six shapes and
    three entries, for three permutation seeds (the exact statement is below: the gate is statistical at its edge);
  * each of the eight planted wiring defects (``generic_step.DEFECTS``) fails it on every shape it applies to.

What the OLD per-tensor gate does with the same defects, measured here at the shapes of train_step_cases.CASES (it is
applied as its tests apply it: to buffers that start from zero; "norms" = cosine and 3 % norm, the encoder test;
"cosine" = cosine alone, the two KD-step tests before this change):

  store_not_add        passes both rules at every shape and entry: from a zeroed buffer storing and adding are the same
  scale_x2             passes the cosine rule at every shape and entry; the norm rule catches it
  one_row_stale        passes both rules at 3 of the 6 (shape, entry) pairs it applies to (student_tn pooled + normalise and
                       tokens, generic_splitk pooled); caught at the other 3
  tile_20pct           CAUGHT at every shape: 32 rows are 1/12 (H 384) to 1/4 (H 128) of dWo, and 1.2 x on 1/12 of a tensor
                       is a 5.8 % error, just past what cosine 0.999 admits (4.5 %).  It passes only where 32 rows are under
                       1/20 of the tensor, which no matrix of the student is
  short_sequence_lost  CAUGHT at every shape: these batches hold 41 to 323 tokens, and one token of T is 1 / sqrt(T) > 4.5 %
                       of a LayerNorm gradient (the pooled entries weigh a short sequence's tokens up further).  It passes
                       from about T > 500 tokens, i.e. at the KD step's real batch
  residual_dropped, db2_from_dx2, pos_offset_ignored   caught at every shape

So at these small shapes the old gate is blind to three of the eight; the new one sees all eight (worst slice RMS(G - R) / noise
per defect and case: 16 and more, against C = 2).

The gate's constant and R'.  With C = 1 neither R' (worst slice over six permutation seeds and the 18 cases: up to 1.5 at one
layer and 2.0 at two) nor the kernels pass.  A rounding that flips between two correct evaluations moves
a stored value by one bf16 ulp - 3.5 x the RMS of a rounding error - and the flips cascade: in student_tn a fifth of the
final hidden states differ between R and R'.  In a slice that one token dominates (a 1-token sequence under mean pooling)
a single flip is worth up to 2 x the slice's noise.  With C = 2, the ceiling, six seeds x 18 cases x 640 ... 14 800 slices
leave two slices above C: one row of layer 0's dW1 in student_tn / pooled without normalise at seeds 1 and 4, at 2.03 and
2.00 (that batch holds a 1-token sequence whose token outweighs the 64-token sequence's 64-fold).  So the gate can raise a
false alarm on a mere reordering, at a rate of about one slice in a million, in that slice class.  The R' test therefore
does not pick a seed: it runs seeds 0, 1 and 2 (1 is one of the two above) and asserts, per case and entry, that the median
over the seeds of the worst slice ratio is <= C and that in every seed at most one slice in 10 000 is above C.  The kernels
themselves are deterministic here (both runs identical).
"""
import pytest
import torch

import train_step_cases as tc
from oracle import generic_step

APPLICABLE = [(case, d) for case in tc.CASES for d in generic_step.DEFECTS
              if generic_step.defect_applies(d, tc.CASES[case][3], tc.pos_offset(case))]


def _added_in_fp32(start, grads):
    """buffers that held ``start`` after an fp32 addition of ``grads``"""
    return {k: start[k] + grads[k].float() for k in grads}


@pytest.mark.parametrize("case", ["no_layers", "xlmr_offset"])
def test_chain_is_the_same_function_as_the_exact_reference(case):
    for mode in tc.MODES:
        out_e, E, out_r, R = tc.references(case, mode)
        B = out_e.shape[0]
        cos = torch.nn.functional.cosine_similarity(out_r.reshape(B, -1), out_e.reshape(B, -1), dim=1)
        assert float(cos.min()) >= 0.9999, (case, mode, cos)
        assert set(R) == set(E)
        assert tc.old_gate(R, E, norms=True) == [], (case, mode)
        # and the chain puts structural zeros where the exact gradient has them
        for name, rows in tc.structural_zero_rows(case).items():
            assert not bool(R[name][rows].any()) and not bool(E[name][rows].any()), name
            assert bool(R[name][~rows].any(1).all()), name


SEEDS = (0, 1, 2)


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("case", list(tc.CASES))
def test_reordered_fp32_chain_stays_inside_the_gate(case, mode):
    start = tc.start_dict(case)
    R = tc.references(case, mode)[3]
    worst = []
    for seed in SEEDS:
        _, Rp = tc.faithful(case, mode, products=tc.permuted_fp32_products(seed))
        if tc.CASES[case][3]:
            assert any(not torch.equal(Rp[k], R[k]) for k in R)      # the order did change something
        res = tc.gate(case, mode, _added_in_fp32(start, Rp), start)
        worst.append(max(res.worst.values()))
        # nothing but slices near the edge of the noise rule may complain, and at most one slice in 10 000 does
        assert all("x noise" in b for b in res.bad), res.bad[:5]
        assert res.over <= 1e-4 * res.slices, (seed, res.bad[:5])
    print(f"{case} / {mode}: R' worst RMS(G - R) / noise per seed " + " ".join(f"{w:.2f}" for w in worst))
    assert sorted(worst)[len(worst) // 2] <= tc.C, worst
    # R itself, added in fp32: only the buffer's own rounding, far inside
    res = tc.gate(case, mode, _added_in_fp32(start, R), start)
    assert not res.bad and max(res.worst.values()) < 0.01, (res.bad[:3], max(res.worst.values()))


@pytest.mark.parametrize("case,defect", APPLICABLE)
def test_every_planted_defect_fails_the_gate(case, defect):
    start = tc.start_dict(case)
    for mode in tc.MODES:
        _, Rd = tc.faithful(case, mode, defect=defect, start=start)
        res = tc.gate(case, mode, _added_in_fp32(start, Rd), start)
        assert res.bad, (case, mode, defect, max(res.worst.values()))


def test_defects_apply_where_the_cases_say():
    seen = {d for _, d in APPLICABLE}
    assert seen == set(generic_step.DEFECTS) and len(generic_step.DEFECTS) == 8
    assert sum(d == "pos_offset_ignored" for _, d in APPLICABLE) == 1          # xlmr_offset alone
    assert sum(d in ("residual_dropped", "one_row_stale") for _, d in APPLICABLE) == 4   # the two 2-layer shapes
    with pytest.raises(ValueError):
        tc.faithful("no_layers", "tokens", defect="tile_20pct")
    with pytest.raises(ValueError):
        tc.faithful("no_layers", "tokens", defect="store_not_add")          # needs the start values


def test_what_the_old_per_tensor_gate_lets_through():
    """The record in the module docstring, re-measured (old gate on buffers that start from zero)."""
    passes = {}
    for case, defect in APPLICABLE:
        for mode in tc.MODES:
            E = tc.references(case, mode)[1]
            zero = {k: torch.zeros_like(v) for k, v in E.items()}
            _, Rd = tc.faithful(case, mode, defect=defect, start=zero)
            passes.setdefault(defect, []).append((not tc.old_gate(Rd, E, norms=True), not tc.old_gate(Rd, E, norms=False)))
    for defect, got in passes.items():
        print(f"{defect}: old gate passes {sum(a for a, _ in got)} (norms) / {sum(b for _, b in got)} (cosine) of {len(got)}")
    assert all(a and b for a, b in passes["store_not_add"])
    assert all(b and not a for a, b in passes["scale_x2"])
    assert any(a for a, _ in passes["one_row_stale"])
    for defect in ("tile_20pct", "short_sequence_lost", "residual_dropped", "db2_from_dx2", "pos_offset_ignored"):
        assert not any(a or b for a, b in passes[defect]), defect      # the finding: caught at these shapes
