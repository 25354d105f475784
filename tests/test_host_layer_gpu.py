"""The Python layer above the encoder, teacher and trainer: what it shares between launches and how it fills the
C structs.

* ``encode_ragged`` issues every launch of a call on the current stream and lets them share ONE workspace and ONE pair
  of packed-row buffers: a call that needs several launches must equal the same launches run one by one.
* ``TrainableEncoder`` and ``TeacherModel`` fill ``GenericWeights`` / ``GenericGrads`` from one field table
  (``weights.LAYER_FIELDS`` / ``EMBEDDING_FIELDS``).  The field -> HF parameter map is restated here BY HAND, so a slip
  in the table (or in the struct field order it must agree with) shows as a pointer at the wrong tensor.
"""
import numpy as np
import pytest
import torch

from semantic_search_kd_amd import BertConfig, Mi355xSentenceEncoder, synthetic_state_dict
from semantic_search_kd_amd import encoder as encoder_module

# struct field -> HF parameter names (several: concatenated along dim 0), written out independently of weights.py
LAYER = {
    "wqkv": ["attention.self.query.weight", "attention.self.key.weight", "attention.self.value.weight"],
    "bqkv": ["attention.self.query.bias", "attention.self.key.bias", "attention.self.value.bias"],
    "wo": ["attention.output.dense.weight"],
    "bo": ["attention.output.dense.bias"],
    "ln1_g": ["attention.output.LayerNorm.weight"],
    "ln1_b": ["attention.output.LayerNorm.bias"],
    "w1": ["intermediate.dense.weight"],
    "b1": ["intermediate.dense.bias"],
    "w2": ["output.dense.weight"],
    "b2": ["output.dense.bias"],
    "ln2_g": ["output.LayerNorm.weight"],
    "ln2_b": ["output.LayerNorm.bias"],
}
EMBEDDINGS = {
    "word_emb": "embeddings.word_embeddings.weight",
    "pos_emb": "embeddings.position_embeddings.weight",
    "type_emb": "embeddings.token_type_embeddings.weight",
    "emb_ln_g": "embeddings.LayerNorm.weight",
    "emb_ln_b": "embeddings.LayerNorm.bias",
}
MATRICES = ("wqkv", "wo", "w1", "w2", "word_emb", "pos_emb", "type_emb")   # read as bf16; every other field is fp32


# ---------------------------------------------------------------------------------- encode_ragged, several launches
LAUNCH_TOKENS = 1024


@pytest.fixture(scope="module")
def enc_l2(gpu):
    return Mi355xSentenceEncoder.from_synthetic(BertConfig(num_hidden_layers=2), device="cuda:0")


def _sequences(lengths, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    lengths = np.asarray(lengths, np.int32)
    flat = g.integers(999, 30522, size=int(lengths.sum()), dtype=np.int64).astype(np.int32)
    cu = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=cu[1:])
    flat[cu[:-1]] = 101
    return flat, lengths, cu


def _launch_bounds(cu):
    """Sequence bounds of the launches ``encode_ragged`` cuts: the longest run of whole sequences whose tokens fit 97 %
    of the launch budget (at least one sequence)."""
    budget, n, bounds = int(LAUNCH_TOKENS * 0.97), cu.size - 1, [0]
    while bounds[-1] < n:
        s0 = bounds[-1]
        s1 = int(np.searchsorted(cu, cu[s0] + budget, side="right")) - 1
        bounds.append(min(max(s1, s0 + 1), n))
    return bounds


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["uniform", "ragged"])
def test_ragged_launches_on_shared_buffers_equal_launches_run_alone(enc_l2, monkeypatch, case):
    """Consecutive launches of one call reuse the workspace and the packed-row buffers with nothing but stream order
    between them.  Each launch's slice encoded by itself (a slice within the budget is ONE launch with the same packing
    plan), with the device idle in between, must give the same bits; so must a second run of the whole call."""
    monkeypatch.setattr(encoder_module, "LAUNCH_TOKENS", LAUNCH_TOKENS)
    if case == "uniform":
        flat, lengths, cu = _sequences([96] * 40, seed=11)
    else:
        flat, lengths, cu = _sequences(np.random.default_rng(5).integers(1, 257, size=60), seed=12)
    bounds = _launch_bounds(cu)
    if case == "uniform":
        assert bounds == [0, 10, 20, 30, 40]          # 960 <= int(1024 * 0.97) = 993 < 1056
    assert len(bounds) - 1 >= 4
    enc = enc_l2
    got = enc.encode_ragged(flat, lengths).clone()
    padded = enc.last_encode_stats["padded_tokens"]
    again = enc.encode_ragged(flat, lengths).clone()
    torch.cuda.synchronize()
    alone, padded_alone = [], 0.0
    for s0, s1 in zip(bounds[:-1], bounds[1:]):
        alone.append(enc.encode_ragged(flat[cu[s0] : cu[s1]], lengths[s0:s1]).clone())
        padded_alone += enc.last_encode_stats["padded_tokens"]
        torch.cuda.synchronize()
    assert padded == padded_alone                     # the same rows were launched: the bounds above are the call's
    assert torch.equal(got, torch.cat(alone))
    assert torch.equal(again, got)
    assert bool(torch.isfinite(got).all()) and got.shape == (lengths.size, 384)


# ---------------------------------------------------------------------------------- struct tables
def _field(struct, name) -> int:
    return int(getattr(struct, name) or 0)


@pytest.mark.gpu
def test_trainer_structs_point_at_the_flat_buffers_by_name(gpu):
    """Every pointer of ``w_struct`` / ``g_struct`` is ``base + element size x offset`` of the HF parameter it stands
    for: bf16 copy for the matrices, fp32 master for the vectors, the flat gradient for every gradient.  The offset of a
    name is where its ``nn.Parameter`` (checked against the state dict) lives in the flat master.  No forward runs."""
    from semantic_search_kd_amd.training import TrainableEncoder

    H, F, L = 64, 128, 2
    cfg = BertConfig(vocab_size=64, hidden_size=H, num_hidden_layers=L, num_attention_heads=2, intermediate_size=F,
                     max_position_embeddings=64)
    sd = synthetic_state_dict(cfg)
    model = TrainableEncoder(cfg, sd, "cuda:0")
    model._refresh_device_weights()
    torch.cuda.synchronize()

    def offset(name) -> int:
        q = model.p(name)
        assert np.array_equal(q.detach().cpu().numpy(), sd[name]), name
        byte = q.data_ptr() - model._flat.data_ptr()
        assert byte % 4 == 0 and 0 <= byte < 4 * model._flat.numel()
        assert model._layout[name][0] == byte // 4
        return byte // 4

    bf16, f32, grad = model._flat_bf16.data_ptr(), model._flat.data_ptr(), model._flat_grad.data_ptr()
    assert model.flat_grad is model._flat_grad
    seen = set()

    def check(w, g, field, names, where):
        offs = [offset(n) for n in names]
        sizes = [int(np.prod(sd[n].shape)) for n in names]
        assert all(offs[j + 1] == offs[j] + sizes[j] for j in range(len(names) - 1)), (where, field)   # q | k | v
        want_w = bf16 + 2 * offs[0] if field in MATRICES else f32 + 4 * offs[0]
        assert _field(w, field) == want_w, (where, field)
        assert _field(g, field) == grad + 4 * offs[0], (where, field)
        seen.update(names)

    for i in range(L):
        for field, suffixes in LAYER.items():
            check(model._layers_struct[i], model._g_layers[i], field, [f"encoder.layer.{i}.{s}" for s in suffixes],
                  f"layer {i}")
    for field, name in EMBEDDINGS.items():
        check(model.w_struct, model.g_struct, field, [name], "embeddings")
    assert seen == set(sd)
    # the backward's W^T operands: kept tensors [L, cols, rows] holding the bf16 matrices transposed
    assert len(model._keep) == 4
    for kept, field in zip(model._keep, ("wqkv", "wo", "w1", "w2")):
        for i in range(L):
            w = torch.cat([model.p(f"encoder.layer.{i}.{s}").detach() for s in LAYER[field]]).to(torch.bfloat16)
            assert kept.shape == (L, w.shape[1], w.shape[0]) and kept.is_contiguous(), field
            assert _field(model._layers_struct[i], field + "_t") == kept[i].data_ptr(), (i, field)
            assert torch.equal(kept[i], w.t()), (i, field)
    # ctypes keeps the arrays alive through these references only
    assert model.w_struct.layers[0].wqkv == model._layers_struct[0].wqkv
    assert model.g_struct.layers[L - 1].ln2_b == model._g_layers[L - 1].ln2_b


@pytest.mark.gpu
def test_teacher_struct_points_at_the_named_tensors(gpu):
    """Every pointer of the teacher's ``GenericWeights`` is a kept device tensor holding the HF parameter(s) it stands
    for: bf16 (torch's rounding) for the matrices, fp32 for the vectors and the classification head."""
    from semantic_search_kd_amd.teacher import TeacherConfig, TeacherModel, synthetic_teacher_state_dict

    L = 2
    cfg = TeacherConfig(vocab_size=64, hidden_size=64, num_hidden_layers=L, num_attention_heads=2, intermediate_size=128,
                        max_position_embeddings=66)
    sd = synthetic_teacher_state_dict(cfg)
    teacher = TeacherModel.from_synthetic(cfg, device="cuda:0")
    torch.cuda.synchronize()
    kept = {t.data_ptr(): t for t in teacher._keep}
    assert len(kept) == len(teacher._keep)
    used = set()

    def check(ptr, names, matrix, where):
        want = torch.cat([torch.from_numpy(sd[n]) for n in names])
        want = want.to(torch.bfloat16) if matrix else want
        got = kept[int(ptr or 0)]
        assert got.dtype == want.dtype and got.shape == want.shape, where
        assert torch.equal(got.cpu(), want), where
        used.update(names)

    for i in range(L):
        for field, suffixes in LAYER.items():
            check(getattr(teacher._layers[i], field), [f"encoder.layer.{i}.{s}" for s in suffixes], field in MATRICES,
                  (i, field))
            if field in MATRICES:
                assert not _field(teacher._layers[i], field + "_t")     # inference: no transposed copies
    for field, name in EMBEDDINGS.items():
        check(getattr(teacher._w, field), [name], field in MATRICES, field)
    for ptr, name in zip(teacher._head, ("classifier.dense.weight", "classifier.dense.bias",
                                         "classifier.out_proj.weight", "classifier.out_proj.bias")):
        check(ptr, [name], False, name)
    assert used == set(sd)
    assert teacher._w.layers[1].w2 == teacher._layers[1].w2
    assert (teacher._cfg.hidden, teacher._cfg.layers, teacher._cfg.pos_offset) == (64, L, cfg.pad_token_id + 1)
