"""Training through MaxSim on the MI355X: sskd_latet_maxsim_fwd / _bwd_q / _bwd_d, sskd_latet_pack_tokens_bwd,
sskd_generic_backward_hidden and the Python surface (late_training.maxsim_scores, TrainableEncoder.forward_tokens,
StudentModel.encode_tokens_with_gradients).

Scores are held bit for bit to the re-rank's raw scores, the gradient kernels and the pack backward bit for bit to their
NumPy restatements (tests/late_train_cases.py, which tests/test_late_train_host.py holds to fp64), the argmax to the fp64
dots, the encoder gradients to CPU autograd over the oracle encoder at the device's own argmax."""
import ctypes as C

import numpy as np
import pytest
import torch

import late_cases as lc
import late_train_cases as tc
from capi_helpers import stream
from oracle import encoder as enc_oracle
from semantic_search_kd_amd import (BertConfig, CombinedKDLoss, FAISSIndexBuilder, LateInteractionIndex, StudentModel,
                                    TokenLayout, TokenStates, _native, late_training as lt, maxsim_scores,
                                    synthetic_state_dict)
from semantic_search_kd_amd.encoder import Mi355xSentenceEncoder, build_wordpiece_tokenizer
from semantic_search_kd_amd.training import GraphedStep, TrainableEncoder
from semantic_search_kd_amd.weights import EMBEDDING_FIELDS, LAYER_FIELDS, field_shape

pytestmark = pytest.mark.gpu

DIM = lc.DIM
SENTINEL = 0xA5
INVALID, UNSUPPORTED = 1, 4


def _bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                                                 np.ascontiguousarray(b, np.float32).view(np.uint32))


class Device:
    """A case on the device: packed tokens, layouts, candidates; forward run once."""

    def __init__(self, q_bits, q_lims, d_bits, d_lims, cand):
        self.host = (q_bits, q_lims, d_bits, d_lims, cand)
        self.q_tok, self.d_tok = _bf16(q_bits), _bf16(d_bits)
        self.ql, self.dl = TokenLayout(np.diff(q_lims), "cuda:0"), TokenLayout(np.diff(d_lims), "cuda:0")
        self.cand = torch.from_numpy(cand).cuda()
        scores, arg = lt.maxsim_forward(self.q_tok, self.ql, self.d_tok, self.dl, self.cand)
        torch.cuda.synchronize()
        self.scores, self.arg = scores.cpu().numpy(), arg.cpu().numpy()
        self.arg_dev = arg

    def grads(self, g: np.ndarray):
        gd = torch.from_numpy(np.ascontiguousarray(g, np.float32)).cuda()
        dq = lt.maxsim_grad_q(self.d_tok, self.dl, self.ql, self.cand, self.arg_dev, gd)
        dd = lt.maxsim_grad_d(self.q_tok, self.ql, self.dl, self.cand, self.arg_dev, gd)
        torch.cuda.synchronize()
        return dq.cpu().numpy(), dd.cpu().numpy()


def _chunk_of(native_lib, nq: int, max_tq: int, R: int) -> int:
    chunk = C.c_int()
    assert native_lib.sskd_late_rerank_plan(nq, max_tq, R, 1, None, None, None, C.byref(chunk)) == 0
    return chunk.value


def _shapes(native_lib):
    shapes = list(tc.SHAPES)
    tqs, tds = [31, 32, 33], [1, 31, 32, 33, 65, 180]
    over = [R for R in range(2, 200) if _chunk_of(native_lib, 3, 33, R) + 1 == R]
    assert over, "no R one larger than the plan's chunk below 200"
    shapes.append((f"nq3-R{over[-1]}-chunk+1", tqs, tds, over[-1]))
    return shapes


@pytest.fixture(scope="module")
def cases(gpu, native_lib):
    """Every random shape, forward run once, shared by the tests below and left unchanged."""
    return {name: Device(*tc.random_case(1000 + R, tqs, tds, R)) for name, tqs, tds, R in _shapes(native_lib)}


# ------------------------------------------------------------------------------------------------ 1. scores
def test_scores_are_the_rerank_raw_scores_bit_for_bit(gpu, cases):
    for name, dev in cases.items():
        q_bits, q_lims, d_bits, d_lims, cand = dev.host
        rows = np.random.default_rng(5).standard_normal((d_lims.size - 1, DIM)).astype(np.float32)
        flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device="cuda:0")
        flat.build_from_embeddings(rows / np.linalg.norm(rows, axis=1, keepdims=True))
        late = LateInteractionIndex(flat)
        late.set_tokens(d_bits, d_lims)
        _, _, raw = late.rerank_device(q_bits, q_lims, dev.cand, 1, return_raw=True)
        torch.cuda.synchronize()
        assert _same_bits(dev.scores, raw.cpu().numpy()), name
        nd = d_lims.size - 1
        absent = (cand < 0) | (cand >= nd)
        assert np.array_equal(np.isneginf(dev.scores), absent), name


# ------------------------------------------------------------------------------------------------ 2. argmax
def test_argmax_is_within_the_band_of_the_fp64_maximum(gpu, cases):
    for name, dev in cases.items():
        q_bits, q_lims, d_bits, d_lims, cand = dev.host
        nd = d_lims.size - 1
        q = lc.bf16_values(q_bits).reshape(-1, DIM).astype(np.float64)
        d = lc.bf16_values(d_bits).reshape(-1, DIM).astype(np.float64)
        _, best, _ = tc.argmax64(q_bits, q_lims, d_bits, d_lims, cand, dev.arg.shape[2])
        slack = 2 * tc.dot_term(q_bits, d_bits)
        assert dev.arg.shape == (cand.shape[0], cand.shape[1], tc.tq_stride(q_lims))
        for qq in range(cand.shape[0]):
            tq = int(q_lims[qq + 1] - q_lims[qq])
            for c in range(cand.shape[1]):
                j = int(cand[qq, c])
                a = dev.arg[qq, c]
                if j < 0 or j >= nd:
                    assert (a == -1).all(), (name, qq, c)
                    continue
                td = int(d_lims[j + 1] - d_lims[j])
                assert (a[tq:] == -1).all() and (a[:tq] >= 0).all() and (a[:tq] < td).all(), (name, qq, c)
                at = (q[q_lims[qq]: q_lims[qq + 1]] * d[d_lims[j] + a[:tq]]).sum(axis=1)
                assert (at >= best[qq, c, :tq] - slack).all(), (name, qq, c, float((best[qq, c, :tq] - at).max()))


def test_argmax_is_exact_on_the_separated_family_and_ties_go_to_the_smallest_index(gpu):
    case = tc.separated_case()
    dev = Device(*case)
    want, best, second = tc.argmax64(*case, dev.arg.shape[2])
    live = want >= 0
    assert (best[live] - second[live] > 2 * tc.dot_term(case[0], case[2])).all()   # (the host test asserts it too)
    assert np.array_equal(dev.arg, want)
    *tie, expect = tc.tie_case()
    dev = Device(*tie)
    assert [int(dev.arg[0, c, 2]) for c in range(len(expect))] == expect


# ------------------------------------------------------------------------------------------------ 3. gradient kernels
def test_gradient_kernels_equal_their_restatements_bit_for_bit(gpu, cases):
    for name, dev in cases.items():
        q_bits, q_lims, d_bits, d_lims, cand = dev.host
        g = np.random.default_rng(11).standard_normal(cand.shape).astype(np.float32) * np.float32(3.0)
        dq, dd = dev.grads(g)
        assert _same_bits(dq, tc.dq_rows(d_bits, d_lims, q_lims, cand, dev.arg, g)), name
        want_dd = tc.dd_rows(q_bits, q_lims, d_lims, cand, dev.arg, g)
        assert _same_bits(dd, want_dd), name
        chosen = np.zeros(int(d_lims[-1]), bool)
        for *_, drow in tc.contributions(q_lims, d_lims, cand, dev.arg):
            chosen[drow] = True
        assert not dd.view(np.uint32)[~chosen].any(), f"{name}: an unselected row of dD is not exact +0.0"
        if len(d_lims) > 2:
            assert not chosen[d_lims[-2]:].any()          # the document nobody names
        # a NaN in g at an absent pair changes nothing; two runs give identical bits
        absent = dev.arg[:, :, 0] < 0
        poisoned = g.copy()
        poisoned[absent] = np.nan
        dq2, dd2 = dev.grads(poisoned)
        assert _same_bits(dq, dq2) and _same_bits(dd, dd2), name
        assert np.isfinite(dq2).all() and np.isfinite(dd2).all()


# ------------------------------------------------------------------------------------------------ 4. pack backward
def test_pack_backward_equals_its_restatement_bit_for_bit(gpu, native_lib):
    hidden, lengths, dtok = tc.pack_bwd_case()
    B, S = hidden.shape[:2]
    lay = TokenLayout(lengths, "cuda:0")
    h = _bf16(hidden)
    out = torch.full((B, S, DIM), -3.0, dtype=torch.bfloat16, device="cuda")
    g = torch.from_numpy(dtok).cuda()
    _native.check(native_lib.sskd_latet_pack_tokens_bwd(h.data_ptr(), lay.lengths_dev.data_ptr(), lay.lims_dev.data_ptr(), B, S, DIM,
                                                       lay.n_tokens, g.data_ptr(), out.data_ptr(), stream()))
    torch.cuda.synchronize()
    got = _bits(out)
    assert np.array_equal(got, tc.pack_bwd_rows(hidden, lengths, dtok))
    for b, L in enumerate(lengths):
        assert not got[b, L:].any(), "padded positions are zeros"


# ------------------------------------------------------------------------------------------------ 5. backward from hidden states
def _op(lib, op, ptrs, ints):
    p = (C.c_void_p * len(ptrs))(*ptrs)
    n = (C.c_int64 * len(ints))(*ints)
    _native.check(lib.sskd_generic_op(op, p, len(ptrs), n, len(ints), None, 0, stream()))


@pytest.mark.parametrize("shape", [(64, 256), (128, 256)], ids=["whole", "two-halves"])
def test_backward_from_hidden_states_reproduces_the_pooled_backward(gpu, native_lib, shape):
    """sskd_generic_backward_hidden fed the bf16 output of the pool backward (the sskd_generic_op hook launches the very
    kernel sskd_generic_backward begins with) against sskd_generic_backward.  The weight-gradient sums are fp32 atomics:
    the tolerance per tensor is four times the run-to-run spread of sskd_generic_backward itself, measured here."""
    lib = native_lib
    B, S = shape
    cfg = BertConfig(vocab_size=2000, num_hidden_layers=2)
    H = cfg.hidden_size
    model = TrainableEncoder(cfg, synthetic_state_dict(cfg), "cuda:0")
    model._refresh_device_weights()
    rng = np.random.default_rng(3)
    lengths = [int(x) for x in rng.integers(2, S + 1, size=B)]
    lengths[0] = S
    ids_np, mask_np = enc_oracle.synthetic_token_ids(B, S, seed=9, vocab=2000, lengths=lengths)
    ids, mask = torch.from_numpy(ids_np).cuda().int(), torch.from_numpy(mask_np).cuda().int()
    dout = torch.from_numpy(rng.standard_normal((B, H)).astype(np.float32)).cuda()
    ws = torch.empty(int(lib.sskd_generic_workspace_bytes(model.cfg_struct, B, S, 1)), dtype=torch.uint8, device="cuda")
    st = stream()

    def forward(pool, out):
        _native.check(lib.sskd_generic_forward(model.cfg_struct, model.w_struct, ids.data_ptr(), mask.data_ptr(), B, S, 1, pool, 1,
                                               out.data_ptr(), ws.data_ptr(), ws.numel(), st))

    def pooled():
        model._flat_grad.zero_()
        forward(1, torch.empty((B, H), dtype=torch.float32, device="cuda"))
        _native.check(lib.sskd_generic_backward(model.cfg_struct, model.w_struct, model.g_struct, ids.data_ptr(), mask.data_ptr(),
                                                B, S, 1, dout.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return model._flat_grad.clone()

    a1, a2 = pooled(), pooled()
    model._flat_grad.zero_()
    hidden = torch.empty((B, S, H), dtype=torch.bfloat16, device="cuda")
    forward(0, hidden)
    emb = torch.empty((B, H), dtype=torch.float32, device="cuda")
    saved = torch.empty((B, H), dtype=torch.float32, device="cuda")
    dhidden = torch.empty((B, S, H), dtype=torch.bfloat16, device="cuda")
    _op(lib, _native.OP_POOL_FWD, [hidden.data_ptr(), mask.data_ptr(), emb.data_ptr(), saved.data_ptr()], [B, S, H, 1])
    _op(lib, _native.OP_POOL_BWD, [dout.data_ptr(), saved.data_ptr(), mask.data_ptr(), dhidden.data_ptr()], [B, S, H, 1])
    before = dhidden.clone()
    _native.check(lib.sskd_generic_backward_hidden(model.cfg_struct, model.w_struct, model.g_struct, ids.data_ptr(), mask.data_ptr(),
                                                   B, S, dhidden.data_ptr(), ws.data_ptr(), ws.numel(), st))
    got = model._flat_grad.clone()
    torch.cuda.synchronize()
    assert torch.equal(dhidden, before), "the caller's gradient is read in place and left unchanged"
    assert float(a1.abs().sum()) > 0
    # "per tensor" = per gradient tensor of the C-ABI's own table (sskd_generic_grads / sskd_generic_layer_grads: the fused
    # QKV weight and bias are ONE tensor each there, as the backward writes them)
    tensors = [(field, model._layout[names[0]][0], int(np.prod(field_shape(cfg, dims)))) for field, names, dims in EMBEDDING_FIELDS]
    for layer in range(cfg.num_hidden_layers):
        tensors += [(f"layers[{layer}].{field}", model._off(layer, names[0]), int(np.prod(field_shape(cfg, dims))) * len(names))
                    for field, names, dims in LAYER_FIELDS]
    assert sum(n for _, _, n in tensors) == model._flat_grad.numel()
    worst = 0.0
    for name, o, n in tensors:
        sl = slice(o, o + n)
        spread = float((a1[sl] - a2[sl]).abs().max())
        diff = float((got[sl] - a1[sl]).abs().max())
        scale = max(float(a1[sl].abs().max()), 1e-30)
        worst = max(worst, spread / scale)
        print(f"{name}: spread {spread:.3e}  hidden-vs-pooled {diff:.3e}  (max |grad| {scale:.3e})")
        assert diff <= 4 * spread, (name, diff, spread)
    print(f"B={B} S={S}: largest run-to-run spread / max |grad| over the tensors = {worst:.3e}")


# ------------------------------------------------------------------------------------------------ 6. end to end
def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-300))


def test_encoder_gradients_through_maxsim_match_oracle_autograd(gpu):
    cfg = BertConfig(vocab_size=2000, num_hidden_layers=2)
    sd = synthetic_state_dict(cfg)
    q_len, d_len = [12, 5], [60, 33, 32, 20, 7, 2]
    q_ids, q_mask = enc_oracle.synthetic_token_ids(2, 12, seed=51, vocab=2000, lengths=q_len)
    d_ids, d_mask = enc_oracle.synthetic_token_ids(6, 60, seed=52, vocab=2000, lengths=d_len)
    probe = np.random.Generator(np.random.PCG64(53)).standard_normal((2, 6)).astype(np.float32)
    model = TrainableEncoder(cfg, sd, "cuda:0")
    qs = TokenStates(model.forward_tokens(q_ids, q_mask), q_len)
    ds = TokenStates(model.forward_tokens(d_ids, d_mask), d_len)
    assert qs.hidden.requires_grad and qs.hidden.dtype == torch.bfloat16 and qs.hidden.shape == (2, 32, DIM)
    scores = maxsim_scores(qs, ds)
    assert scores.shape == (2, 6) and scores.dtype == torch.float32 and scores.requires_grad
    (scores * torch.from_numpy(probe).cuda()).sum().backward()
    # the device's own argmax (validated on its own above): a near-tie flipped by bf16 must not make this a test of luck
    with torch.no_grad():
        cand = torch.arange(6, device="cuda").unsqueeze(0).expand(2, 6).contiguous()
        raw, arg = lt.maxsim_forward(lt._pack(qs.hidden.detach(), qs.layout), qs.layout, lt._pack(ds.hidden.detach(), ds.layout),
                                     ds.layout, cand)
    assert torch.equal(raw / qs.layout.lengths_f32.unsqueeze(1), scores.detach())
    arg = arg.cpu().numpy()
    # oracle chain: encoder -> normalise -> gather at arg -> mean over the query's tokens -> CPU autograd
    t = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in sd.items()}

    def tokens(ids, mask, lengths):
        h = enc_oracle.bert_hidden_states_torch(t, ids, mask, cfg.num_hidden_layers, cfg.num_attention_heads)[-1]
        rows = torch.cat([h[b, :L] for b, L in enumerate(lengths)])
        return rows / rows.norm(dim=1, keepdim=True)

    q_lims, d_lims = tc.lims_of(q_len), tc.lims_of(d_len)
    so = tc.gather_scores_torch(tokens(q_ids, q_mask, q_len), q_lims, tokens(d_ids, d_mask, d_len), d_lims, cand.cpu().numpy(), arg)
    so = so / torch.tensor(q_len, dtype=so.dtype).unsqueeze(1)
    (so * torch.from_numpy(probe)).sum().backward()
    assert np.abs(scores.detach().cpu().numpy() - so.detach().numpy()).max() < 5e-3
    want = {k: v.grad.numpy() for k, v in t.items() if v.grad is not None}
    top = max(np.abs(v).max() for v in want.values())
    for name in model.names:
        got, ref = model.p(name).grad.cpu().numpy(), want[name]
        if np.abs(ref).max() < 1e-6 * top:  # mathematically zero (key biases): only rounding noise may show
            assert np.abs(got).max() < 2e-2 * top, name
            continue
        assert _cos(got, ref) >= 0.999, (name, _cos(got, ref))
        assert abs(np.linalg.norm(got) / np.linalg.norm(ref) - 1.0) < 0.03, name
    gw = model.p("embeddings.word_embeddings.weight").grad
    untouched = torch.ones(cfg.vocab_size, dtype=torch.bool)
    untouched[torch.from_numpy(np.concatenate([q_ids[q_mask.astype(bool)], d_ids[d_mask.astype(bool)]])).long()] = False
    assert not gw[untouched.cuda()].any()


# ------------------------------------------------------------------------------------------------ 7. KD step
WORDS = ["what", "is", "machine", "learning", "how", "does", "search", "work", "semantic", "the", "a", "of", "deep", "neural",
         "network", "vector", "index", "hello", "world", "test", "document", "text"]


def _vocab():
    return ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS + ["##s", "##ing", ".", "?"]


def _sentence(rng, n):
    return " ".join(WORDS[i] for i in rng.integers(0, len(WORDS), size=n))


def test_kd_step_through_maxsim_learns_and_replays_from_a_graph(gpu):
    vocab = _vocab()
    cfg = BertConfig(vocab_size=len(vocab), num_hidden_layers=2)
    rng = np.random.default_rng(61)
    query = [_sentence(rng, 6)]
    docs = [_sentence(rng, n) for n in (40, 31, 30, 22, 17, 9, 5, 2, 1)]
    teacher = torch.from_numpy(rng.standard_normal((1, 9)).astype(np.float32) * 3.0).cuda()

    enc = Mi355xSentenceEncoder.from_synthetic(cfg, device="cuda:0", tokenizer=build_wordpiece_tokenizer(vocab))
    student = StudentModel.from_encoder(enc, "e5-small-v2-synthetic")
    loss_fn = CombinedKDLoss()

    def step_loss():
        q = student.encode_tokens_with_gradients(query, 32)
        d = student.encode_tokens_with_gradients(docs, 180)
        return loss_fn(maxsim_scores(q, d, docs_per_query=9), teacher)["loss"]

    q = student.encode_tokens_with_gradients(query, 32)
    assert list(q.lengths) == [8] and q.hidden.shape == (1, 32, DIM)          # [CLS] 6 words [SEP]
    assert list(student.encode_tokens_with_gradients(docs, 20).lengths)[:2] == [20, 20]   # cut, [SEP] kept
    opt = torch.optim.AdamW(student.model.parameters(), lr=2e-4)
    first = None
    for _ in range(8):
        opt.zero_grad()
        loss = step_loss()
        loss.backward()
        opt.step()
        first = float(loss.detach()) if first is None else first
    assert float(loss.detach()) < first, (first, float(loss.detach()))

    # The captured step: forward_tokens on ids that keep their storage, layouts built before the capture.  The optimizer
    # takes part with lr = 0, so the parameters - and with them the forward's bits - are those of the eager step.
    model = TrainableEncoder(cfg, synthetic_state_dict(cfg), "cuda:0")
    tok_q, tok_d = enc.tokenize(query), enc.tokenize(docs)
    ids = [torch.from_numpy(x).cuda().int() for x in (tok_q["input_ids"], tok_q["attention_mask"], tok_d["input_ids"], tok_d["attention_mask"])]
    lay_q = TokenLayout(tok_q["attention_mask"].sum(axis=1), "cuda:0")
    lay_d = TokenLayout(tok_d["attention_mask"].sum(axis=1), "cuda:0")
    opt = torch.optim.AdamW(model.parameters(), lr=0.0, capturable=True)
    loss_fn = CombinedKDLoss()

    def step():
        opt.zero_grad(set_to_none=True)
        qs = TokenStates(model.forward_tokens(ids[0], ids[1]), lay_q)
        ds = TokenStates(model.forward_tokens(ids[2], ids[3]), lay_d)
        scores = maxsim_scores(qs, ds, docs_per_query=9)
        loss = loss_fn(scores, teacher)["loss"]
        loss.backward()
        opt.step()
        return scores.detach(), loss.detach()

    eager_scores, eager_loss = (x.clone() for x in step())
    runner = GraphedStep(step, warmup=1, modules=[model])
    model._flat_grad.zero_()
    scores, loss = runner()
    torch.cuda.synchronize()
    assert torch.equal(scores, eager_scores) and torch.isfinite(scores).all()
    assert torch.allclose(loss, eager_loss, rtol=1e-6, atol=0)
    assert float(model.flat_grad.abs().sum()) > 0, "the replay ran the backward"


def test_more_than_1024_candidates_are_scored_in_chunks(gpu):
    """R = 1030 names four documents over and over: the forward is the two chunks' forwards side by side (bit for bit),
    the backward hands every chunk its own columns of g.  The hidden-state gradient of the whole call is the bf16
    rounding of the fp32 sum of the chunks' token gradients, the two chunks run alone round separately: each of the three
    is within 2^-9 of its unrounded value element by element, so ||whole - (a + b)|| <= 2^-9 (||whole|| + ||a|| + ||b||)
    plus the pack backward's fp32 dot error (a few 1e-5 of the same norms); the gate is 2^-8 of that sum.  Columns of g
    handed to the wrong chunk would move the result by about ||b||, ten times the gate."""
    gen = torch.Generator(device="cuda").manual_seed(3)
    qh = torch.randn((1, 32, DIM), device="cuda", generator=gen).to(torch.bfloat16).requires_grad_(True)
    dh = torch.randn((4, 64, DIM), device="cuda", generator=gen).to(torch.bfloat16).requires_grad_(True)
    ql, dl = TokenLayout([9], "cuda:0"), TokenLayout([64, 33, 2, 40], "cuda:0")
    cand = (torch.arange(1030, device="cuda") % 5 - 1).view(1, 1030).contiguous()      # -1, 0, 1, 2, 3, -1, ...
    g = torch.randn((1, 1030), device="cuda", generator=gen)

    def run(cols):
        qh.grad = dh.grad = None
        s = maxsim_scores(TokenStates(qh, ql), TokenStates(dh, dl), cand=cand[:, cols].contiguous(), mean=False)
        (s * g[:, cols]).sum().backward()
        return s.detach(), qh.grad.float(), dh.grad.float()

    s, dq, dd = run(slice(0, 1030))
    sa, dqa, dda = run(slice(0, 1024))
    sb, dqb, ddb = run(slice(1024, 1030))
    assert torch.equal(s, torch.cat([sa, sb], dim=1))
    assert bool(torch.isneginf(s[0, ::5]).all()) and bool(torch.isfinite(s[0, 1::5]).all())
    for whole, a, b in ((dq, dqa, dqb), (dd, dda, ddb)):
        assert float(b.abs().max()) > 0 and bool(torch.isfinite(whole).all())
        gate = 2.0 ** -8 * float(whole.norm() + a.norm() + b.norm())
        assert float((whole - (a + b)).norm()) <= gate < 0.25 * float(b.norm())


# ------------------------------------------------------------------------------------------------ 8. refusals
def _sentinel(nbytes: int) -> torch.Tensor:
    return torch.full((max(int(nbytes), 1),), SENTINEL, dtype=torch.uint8, device="cuda")


def _intact(*buffers: torch.Tensor) -> bool:
    torch.cuda.synchronize()
    return all(bool((b == SENTINEL).all()) for b in buffers)


def test_refusals_come_before_anything_is_enqueued(gpu, native_lib):
    lib = native_lib
    q_bits, q_lims, d_bits, d_lims, cand = tc.random_case(77, [5, 33], [7, 40, 3], 5)
    q_tok, d_tok = _bf16(q_bits), _bf16(d_bits)
    ql, dl = TokenLayout(np.diff(q_lims), "cuda:0"), TokenLayout(np.diff(d_lims), "cuda:0")
    cd = torch.from_numpy(cand).cuda()
    nq, R, stride = 2, 5, 64
    scores, arg = _sentinel(nq * R * 4), _sentinel(nq * R * stride * 4)
    big_cand = torch.zeros((nq, 1025), dtype=torch.int64, device="cuda")

    def fwd(q_lims_host=ql.lims, n_q=ql.n_tokens, R_=R, cand_=cd, scores_=scores, stride_=stride, nq_=nq):
        return lib.sskd_latet_maxsim_fwd(q_tok.data_ptr(), q_lims_host.ctypes.data, ql.lims_dev.data_ptr(), nq_, n_q, d_tok.data_ptr(),
                                        dl.lims_dev.data_ptr(), dl.n, dl.n_tokens, cand_.data_ptr(), R_,
                                        None if scores_ is None else scores_.data_ptr(), arg.data_ptr(), stride_, stream())

    long_lims = np.array([0, 129], np.int64)
    assert fwd(q_lims_host=long_lims, n_q=129, nq_=1, stride_=160) == INVALID            # Tq > 128
    assert fwd(R_=1025, cand_=big_cand) == INVALID                                          # R > 1024
    assert fwd(scores_=None) == INVALID                                                     # a null pointer
    assert fwd(n_q=ql.n_tokens + 1) == INVALID                                              # lims do not end at the row count
    assert fwd(stride_=32) == INVALID                                                       # not the rounded-up largest Tq
    assert _intact(scores, arg)
    assert fwd(R_=0) == 0 and fwd(nq_=0) == 0 and _intact(scores, arg)                      # nothing to do: SSKD_OK, nothing launched

    g = torch.zeros((nq, R), dtype=torch.float32, device="cuda")
    real_arg = torch.full((nq, R, stride), -1, dtype=torch.int32, device="cuda")
    dq, dd = _sentinel(ql.n_tokens * DIM * 4), _sentinel(dl.n_tokens * DIM * 4)

    def bwd_q(n_q=ql.n_tokens, R_=R, g_=g, stride_=stride):
        return lib.sskd_latet_maxsim_bwd_q(d_tok.data_ptr(), dl.lims_dev.data_ptr(), dl.n, dl.n_tokens, ql.lims.ctypes.data,
                                          ql.lims_dev.data_ptr(), nq, n_q, cd.data_ptr(), R_, real_arg.data_ptr(), stride_,
                                          None if g_ is None else g_.data_ptr(), dq.data_ptr(), stream())

    order = torch.zeros(nq * R * stride, dtype=torch.int64, device="cuda")
    seg = torch.zeros(dl.n_tokens + 1, dtype=torch.int64, device="cuda")

    def bwd_d(n_q=ql.n_tokens, R_=R, order_=order, stride_=stride):
        return lib.sskd_latet_maxsim_bwd_d(q_tok.data_ptr(), ql.lims.ctypes.data, ql.lims_dev.data_ptr(), nq, n_q, R_, stride_,
                                          None if order_ is None else order_.data_ptr(), seg.data_ptr(), dl.n_tokens, g.data_ptr(),
                                          dd.data_ptr(), stream())

    assert bwd_q(R_=1025) == INVALID and bwd_q(g_=None) == INVALID and bwd_q(n_q=ql.n_tokens - 1) == INVALID
    assert bwd_q(stride_=128) == INVALID
    assert bwd_d(R_=1025) == INVALID and bwd_d(order_=None) == INVALID and bwd_d(n_q=ql.n_tokens - 1) == INVALID
    assert _intact(dq, dd)

    # the pack backward: H != 384 is not served, a null pointer and S = 0 are invalid
    hidden = torch.zeros((2, 8, DIM), dtype=torch.bfloat16, device="cuda")
    lay = TokenLayout([8, 3], "cuda:0")
    dtok = torch.zeros((11, DIM), dtype=torch.float32, device="cuda")
    out = _sentinel(2 * 8 * DIM * 2)

    def pack_bwd(H=DIM, S=8, dtok_=dtok):
        return lib.sskd_latet_pack_tokens_bwd(hidden.data_ptr(), lay.lengths_dev.data_ptr(), lay.lims_dev.data_ptr(), 2, S, H, 11,
                                             None if dtok_ is None else dtok_.data_ptr(), out.data_ptr(), stream())

    assert pack_bwd(H=256) == UNSUPPORTED and pack_bwd(S=0) == INVALID and pack_bwd(dtok_=None) == INVALID
    assert _intact(out)

    # the Python surface raises before it enqueues
    with pytest.raises(ValueError, match="384"):
        TokenStates(torch.zeros((1, 32, 256), dtype=torch.bfloat16, device="cuda"), [4])
    with pytest.raises(ValueError, match="no tokens"):
        TokenStates(torch.zeros((2, 32, DIM), dtype=torch.bfloat16, device="cuda"), [4, 0])
    long_q = TokenStates(torch.zeros((1, 160, DIM), dtype=torch.bfloat16, device="cuda"), [129])
    docs = TokenStates(torch.zeros((2, 32, DIM), dtype=torch.bfloat16, device="cuda"), [4, 2])
    with pytest.raises(ValueError, match="128"):
        maxsim_scores(long_q, docs)
    with pytest.raises(ValueError, match="docs_per_query"):
        maxsim_scores(docs, docs, docs_per_query=3)


def test_backward_hidden_refuses_a_null_gradient_before_it_enqueues(gpu, native_lib):
    lib = native_lib
    cfg = BertConfig(vocab_size=64, hidden_size=128, num_hidden_layers=1, num_attention_heads=4, intermediate_size=256,
                     max_position_embeddings=64)
    model = TrainableEncoder(cfg, synthetic_state_dict(cfg), "cuda:0")
    model._refresh_device_weights()
    B, S = 2, 32
    ids = torch.ones((B, S), dtype=torch.int32, device="cuda")
    ws = _sentinel(int(lib.sskd_generic_workspace_bytes(model.cfg_struct, B, S, 1)))
    model._flat_grad.zero_()
    rc = lib.sskd_generic_backward_hidden(model.cfg_struct, model.w_struct, model.g_struct, ids.data_ptr(), ids.data_ptr(), B, S,
                                          None, ws.data_ptr(), ws.numel(), stream())
    assert rc == INVALID and _intact(ws) and not model._flat_grad.any()
    # any H the generic encoder serves (here 128): forward_tokens -> backward from a hidden-state gradient
    h = model.forward_tokens(ids, ids)
    assert h.shape == (B, S, 128)
    h.float().square().sum().backward()     # an fp32 gradient: the backward hands bf16 to the kernels
    assert float(model.flat_grad.abs().sum()) > 0 and bool(torch.isfinite(model.flat_grad).all())
