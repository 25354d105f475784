"""The composed student step on the GPU (``sskd_generic_forward`` / ``_backward`` / ``_backward_hidden`` through
``TrainableEncoder``) against the rounding-faithful fp64 chain R, with the exact fp64 autograd E as the measure of what bf16
costs: the gate of tests/train_step_cases.py (every row, column and 32-block of every parameter gradient; exact zeros bit
for bit; norms within 3 %), which tests/test_train_step_host.py shows to pass a reordered R and to fail eight planted
wiring defects.

Six shapes (train_step_cases.CASES: the TN and the transpose + NT weight-gradient routes with one and two K slices, fused
attention backward at widths 32 and 64 and the materialised-score route, no layers, a position offset) x three entries
(pooled + L2 normalise, pooled, token states with a seeded bf16 ``dhidden``).  The gradient buffers start from a non-zero
pattern, so what is gated is what the step ADDED; each case runs twice into refilled buffers (the atomics reorder: both runs
must pass, bit equality is not asked).

Worst RMS(G - R) / noise measured on an MI355X per case, with C = 2 in force (train_step_cases.C says why): DESIGN.md 3.8.
"""
import pytest
import torch

import train_step_cases as tc

pytestmark = pytest.mark.gpu


def run_step(model, case: str, mode: str, start):
    """Fill the gradient buffers with ``start``, run one forward + backward, return (output, buffers after) on the CPU."""
    _, ids, mask, dout, dhidden = tc.inputs(case)
    model._attach_grads()                       # every p.grad a view of flat_grad: a backward then keeps their contents
    for name in model.names:
        model.p(name).grad.copy_(start[name])
    before = model.flat_grad.clone()
    if mode == "tokens":
        out = model.forward_tokens(ids, mask)
        out.backward(torch.from_numpy(dhidden).to(out.device, torch.bfloat16))
    else:
        out = model(ids, mask, normalize=mode == "pooled_norm")
        out.backward(torch.from_numpy(dout).to(out.device))
    torch.cuda.synchronize()
    assert not torch.equal(before, model.flat_grad)
    return out.detach().double().cpu(), {n: model.p(n).grad.detach().cpu().clone() for n in model.names}


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("case", list(tc.CASES))
def test_composed_step_lies_within_rounding_noise_of_the_faithful_chain(gpu, case, mode):
    from semantic_search_kd_amd.training import TrainableEncoder

    sd = tc.inputs(case)[0]
    out_e, _, out_r, R = tc.references(case, mode)
    start = tc.start_dict(case)
    model = TrainableEncoder(tc.config(case), sd, gpu, pos_offset=tc.pos_offset(case))
    assert set(model.names) == set(R)
    for run in range(2):
        out, after = run_step(model, case, mode, start)
        # forward: every sequence's output points where the exact one does, and lies within C x (R's own distance from E) of R
        B = out.shape[0]
        cos = torch.nn.functional.cosine_similarity(out.reshape(B, -1), out_e.reshape(B, -1), dim=1)
        assert float(cos.min()) >= 0.9999, (case, mode, cos)
        fwd = float((out - out_r).pow(2).mean().sqrt() / (out_r - out_e).pow(2).mean().sqrt())
        assert fwd <= tc.C, (case, mode, fwd)
        res = tc.gate(case, mode, after, start)
        print(f"\n{case} / {mode} run {run}: worst RMS(G - R) / noise {max(res.worst.values()):.2f} (C = {tc.C}; "
              f"{res.over} of {res.slices} slices above C, {res.fp32_slices} held to fp32 arithmetic); forward "
              f"RMS(out - R) / RMS(R - E) {fwd:.2f}\n{tc.table(res.worst)}")
        bad = res.bad
        assert not bad, f"{case} / {mode} run {run}: {len(bad)} violations, first: " + "; ".join(bad[:5])
