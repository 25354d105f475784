"""A call the encoders refuse must have enqueued nothing.

Every case fills the workspace and the output buffers with a sentinel byte, makes a call that is refused for a reason
only the deep end of the call used to notice (the attention launcher, the layer loop), synchronises, and asserts the
return code (SSKD_ERR_INVALID), that every sentinel byte is intact, and - for the generic encoder - that the matching
size query returns 0.  Real, small device weights (vocabulary 64, 1-2 layers): a partial run would be harmless, only
visible."""
import ctypes as C

import numpy as np
import pytest
import torch

from capi_helpers import stream
from semantic_search_kd_amd import _native
from semantic_search_kd_amd.training import TrainableEncoder
from semantic_search_kd_amd.weights import BertConfig, DeviceWeights, synthetic_state_dict

pytestmark = pytest.mark.gpu

SSKD_ERR_INVALID = 1
SENTINEL = 0xA5


def _sentinel(nbytes: int) -> torch.Tensor:
    return torch.full((max(int(nbytes), 1),), SENTINEL, dtype=torch.uint8, device="cuda")


def _intact(*buffers: torch.Tensor) -> bool:
    torch.cuda.synchronize()
    return all(bool((b == SENTINEL).all()) for b in buffers)


def _tokens(B: int, S: int, vocab: int = 64, seed: int = 0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, vocab, size=(B, S)).astype(np.int32)
    mask = np.ones((B, S), np.int32)
    mask[0, S - 5:] = 0   # some padding
    return torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()


def _generic(hidden: int, heads: int, layers: int, max_positions: int) -> TrainableEncoder:
    cfg = BertConfig(vocab_size=64, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                     intermediate_size=2 * hidden, max_position_embeddings=max_positions)
    enc = TrainableEncoder(cfg, synthetic_state_dict(cfg), "cuda:0")
    enc._refresh_device_weights()
    return enc


def _generic_forward(lib, enc, ids, mask, training, out, ws):
    B, S = ids.shape
    return lib.sskd_generic_forward(enc.cfg_struct, enc.w_struct, ids.data_ptr(), mask.data_ptr(), B, S, training, 1, 1,
                                    out.data_ptr(), ws.data_ptr(), ws.numel(), stream())


def _teacher_score(lib, enc, ids, mask, out, ws):
    B, S = ids.shape
    H = enc.config.hidden_size
    head = torch.full((H * H + 2 * H + 1,), 0.01, dtype=torch.float32, device="cuda")
    p = head.data_ptr()
    return lib.sskd_teacher_score(enc.cfg_struct, enc.w_struct, p, p + 4 * H * H, p + 4 * (H * H + H), p + 4 * (H * H + 2 * H),
                                  ids.data_ptr(), mask.data_ptr(), B, S, out.data_ptr(), ws.data_ptr(), ws.numel(), stream())


def test_inference_head_width_96_is_refused_whole_and_training_still_serves_it(gpu, native_lib):
    lib = native_lib
    enc = _generic(hidden=192, heads=2, layers=1, max_positions=64)
    B, S = 2, 32
    ids, mask = _tokens(B, S)
    room = int(lib.sskd_generic_workspace_bytes(enc.cfg_struct, B, S, 1))   # the unfused route serves this shape
    assert room > 0
    ws, out = _sentinel(room), _sentinel(B * 192 * 4)
    assert _generic_forward(lib, enc, ids, mask, 0, out, ws) == SSKD_ERR_INVALID
    assert _intact(ws, out)
    assert int(lib.sskd_generic_workspace_bytes(enc.cfg_struct, B, S, 0)) == 0
    assert int(lib.sskd_teacher_workspace_bytes(enc.cfg_struct, B, S)) == 0
    # training: the unfused route serves head width 96 and must keep serving it
    assert _generic_forward(lib, enc, ids, mask, 1, out, ws) == _native.SSKD_OK
    torch.cuda.synchronize()
    emb = out.view(torch.float32).view(B, 192)
    assert bool(torch.isfinite(emb).all())
    assert torch.allclose(emb.norm(dim=1), torch.ones(B, device="cuda"), atol=1e-3)


def test_inference_s_times_width_over_lds_is_refused_whole(gpu, native_lib):
    lib = native_lib
    enc = _generic(hidden=256, heads=2, layers=1, max_positions=320)
    B, S = 1, 320   # S * DH = 40 960 > 36 864
    ids, mask = _tokens(B, S)
    room = int(lib.sskd_generic_workspace_bytes(enc.cfg_struct, B, S, 1))
    assert room > 0
    ws, out, logits = _sentinel(room), _sentinel(B * 256 * 4), _sentinel(B * 4)
    assert _generic_forward(lib, enc, ids, mask, 0, out, ws) == SSKD_ERR_INVALID
    assert _intact(ws, out)
    assert _teacher_score(lib, enc, ids, mask, logits, ws) == SSKD_ERR_INVALID
    assert _intact(ws, logits)
    assert int(lib.sskd_generic_workspace_bytes(enc.cfg_struct, B, S, 0)) == 0
    assert int(lib.sskd_teacher_workspace_bytes(enc.cfg_struct, B, S)) == 0


def test_backward_without_a_transposed_weight_is_refused_whole(gpu, native_lib):
    lib = native_lib
    enc = _generic(hidden=128, heads=4, layers=2, max_positions=64)
    B, S = 2, 32
    ids, mask = _tokens(B, S)
    ws = _sentinel(int(lib.sskd_generic_workspace_bytes(enc.cfg_struct, B, S, 1)))
    out = torch.empty((B, 128), dtype=torch.float32, device="cuda")
    assert _generic_forward(lib, enc, ids, mask, 1, out, ws) == _native.SSKD_OK
    torch.cuda.synchronize()
    saved = ws.clone()   # the forward's activations over the sentinel: the refused backward must not touch a byte
    enc.flat_grad.zero_()
    dout = torch.ones((B, 128), dtype=torch.float32, device="cuda")
    kept = enc._layers_struct[0].w1_t
    enc._layers_struct[0].w1_t = None
    try:
        rc = lib.sskd_generic_backward(enc.cfg_struct, enc.w_struct, enc.g_struct, ids.data_ptr(), mask.data_ptr(), B, S, 1,
                                       dout.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    finally:
        enc._layers_struct[0].w1_t = kept
    torch.cuda.synchronize()
    assert rc == SSKD_ERR_INVALID
    assert torch.equal(ws, saved)
    assert int(torch.count_nonzero(enc.flat_grad)) == 0


def test_encoder_384_null_layer_weight_is_refused_whole(gpu, native_lib):
    lib = native_lib
    cfg = BertConfig(vocab_size=64, num_hidden_layers=2, max_position_embeddings=64)
    weights = DeviceWeights(cfg, synthetic_state_dict(cfg), "cuda:0")
    weights.layers[1].wo = None
    B, S = 1, 32
    ids, mask = _tokens(B, S)
    ws = _sentinel(int(lib.sskd_encoder_workspace_bytes(weights.cstruct_cfg, B, S)))
    out = _sentinel(B * 384 * 4)
    rc = lib.sskd_encoder_forward(weights.cstruct_cfg, weights.struct, ids.data_ptr(), mask.data_ptr(), B, S, 1, out.data_ptr(),
                                  ws.data_ptr(), ws.numel(), stream())
    assert rc == SSKD_ERR_INVALID
    assert _intact(ws, out)
    # one packed row of two sequences (20 + 7 tokens of 32)
    lengths = np.array([20, 7], np.int32)
    table = np.zeros(8, np.int32)
    n_rows = C.c_int(0)
    _native.check(lib.sskd_pack_plan(lengths.ctypes.data, 2, S, table.ctypes.data, n_rows))
    assert n_rows.value == 1
    flat = ids.flatten()[:27].contiguous()
    cu = torch.tensor([0, 20, 27], dtype=torch.int32, device="cuda")
    d_table = torch.from_numpy(table).cuda()
    rows_ids = torch.empty((1, S), dtype=torch.int32, device="cuda")
    rows_seg = torch.empty((1, S), dtype=torch.int32, device="cuda")
    _native.check(lib.sskd_pack_tokens(flat.data_ptr(), cu.data_ptr(), d_table.data_ptr(), 2, 1, S, rows_ids.data_ptr(),
                                       rows_seg.data_ptr(), stream()))
    out2 = _sentinel(2 * 384 * 4)
    rc = lib.sskd_encoder_forward_packed(weights.cstruct_cfg, weights.struct, rows_ids.data_ptr(), rows_seg.data_ptr(), 1, S,
                                         d_table.data_ptr(), 2, 1, out2.data_ptr(), ws.data_ptr(), ws.numel(), stream())
    assert rc == SSKD_ERR_INVALID
    assert _intact(ws, out2)
