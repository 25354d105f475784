"""Student forward / backward on the MI355X (BASELINE cfg 4): ``encode_with_gradients``.

The reference's KD step (src/kd/train.py:176-210) calls ``StudentModel.encode_with_gradients``
twice per query (query, then its positive + hard negatives), multiplies, applies
``CombinedKDLoss`` and lets torch autograd walk back through the sentence-transformers modules.
Here the encoder forward that saves its activations and the whole backward pass are HIP
(``sskd_generic_forward`` / ``sskd_generic_backward``, csrc/train.hip) behind ONE
``torch.autograd.Function``; torch holds the fp32 master parameters (what the optimizer updates)
and supplies device memory.  bf16 compute, fp32 accumulation and gradients.  No CPU path.

``TrainableEncoder.forward_tokens`` is the same pair without the pool (``sskd_generic_backward_hidden`` starts from the
gradient of the final hidden states): the encoder side of training through MaxSim (late_training.py).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _native
from .weights import EMBEDDING_FIELDS, LAYER_FIELDS, BertConfig, field_shape


def _pname(hf_name: str) -> str:
    return hf_name.replace(".", "__")


class _EncoderFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module: "TrainableEncoder", ids: torch.Tensor, mask: torch.Tensor, normalize: bool, *params):
        lib = _native.load()
        B, S = ids.shape
        module._check_autograd_contract()
        module._refresh_device_weights()
        need = int(lib.sskd_generic_workspace_bytes(module.cfg_struct, B, S, 1))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=ids.device)
        out = torch.empty((B, module.config.hidden_size), dtype=torch.float32, device=ids.device)
        with torch.cuda.device(ids.device):
            _native.check(lib.sskd_generic_forward(
                module.cfg_struct, module.w_struct, ids.data_ptr(), mask.data_ptr(), B, S, 1, 1, int(normalize),
                out.data_ptr(), ws.data_ptr(), ws.numel(), _native.current_stream_ptr(ids.device)))
        ctx.module, ctx.ws, ctx.normalize = module, ws, bool(normalize)
        ctx.save_for_backward(ids, mask)
        ctx.weights_version = module._weights_version
        return out

    @staticmethod
    def backward(ctx, dout):
        """The HIP backward ACCUMULATES (atomics / +=) straight into ``p.grad`` of every parameter - views of ONE flat fp32
        buffer that is zeroed with one memset when the gradients were ``None`` - and hands autograd ``None`` for them:
        no per-call set of ~150 zero-filled buffers (90 MB for e5-small, the dense 30522 x 384 word-embedding gradient
        included) and no ~150 accumulation kernels when a step calls the encoder more than once (the reference calls
        ``encode_with_gradients`` 2 x batch_size times per step, src/kd/train.py:176-210).

        RESTRICTION (checked in ``TrainableEncoder._check_autograd_contract``, which raises instead of returning wrong
        gradients): this is ``loss.backward()`` semantics only.  Parameter gradients are side effects on ``p.grad``, so
        ``torch.autograd.grad(..., params)``, ``backward(inputs=...)``, tensor / post-accumulate hooks on a parameter
        (DDP registers those) and ``requires_grad=False`` on a single parameter are NOT served - the forward refuses
        parameters that carry hooks or are frozen.  Data parallelism reduces the FLAT gradient buffer instead
        (``TrainableEncoder.flat_grad``: one all-reduce of one tensor)."""
        lib = _native.load()
        module: TrainableEncoder = ctx.module
        ids, mask = ctx.saved_tensors
        B, S = ids.shape
        if ctx.weights_version != module._weights_version:
            raise RuntimeError("parameters changed between forward and backward of encode_with_gradients")
        module._attach_grads()
        dout = dout.to(torch.float32).contiguous()
        with torch.cuda.device(ids.device):
            _native.check(lib.sskd_generic_backward(
                module.cfg_struct, module.w_struct, module.g_struct, ids.data_ptr(), mask.data_ptr(), B, S, int(ctx.normalize),
                dout.data_ptr(), ctx.ws.data_ptr(), ctx.ws.numel(), _native.current_stream_ptr(ids.device)))
        ctx.ws = None
        return (None, None, None, None) + (None,) * len(module.names)


class _EncoderTokensFunction(torch.autograd.Function):
    """``_EncoderFunction`` without the pool: ids -> the final hidden states bf16 ``[B, S, H]``
    (``sskd_generic_forward(training=1, pool=0)``), backward from their gradient (``sskd_generic_backward_hidden``).
    The autograd contract, the refusals and the ``p.grad`` side effects are ``_EncoderFunction``'s."""

    @staticmethod
    def forward(ctx, module: "TrainableEncoder", ids: torch.Tensor, mask: torch.Tensor, *params):
        lib = _native.load()
        B, S = ids.shape
        module._check_autograd_contract()
        module._refresh_device_weights()
        need = int(lib.sskd_generic_workspace_bytes(module.cfg_struct, B, S, 1))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=ids.device)
        out = torch.empty((B, S, module.config.hidden_size), dtype=torch.bfloat16, device=ids.device)
        with torch.cuda.device(ids.device):
            _native.check(lib.sskd_generic_forward(
                module.cfg_struct, module.w_struct, ids.data_ptr(), mask.data_ptr(), B, S, 1, 0, 0,
                out.data_ptr(), ws.data_ptr(), ws.numel(), _native.current_stream_ptr(ids.device)))
        ctx.module, ctx.ws = module, ws
        ctx.save_for_backward(ids, mask)
        ctx.weights_version = module._weights_version
        return out

    @staticmethod
    def backward(ctx, dhidden):
        lib = _native.load()
        module: TrainableEncoder = ctx.module
        ids, mask = ctx.saved_tensors
        B, S = ids.shape
        if ctx.weights_version != module._weights_version:
            raise RuntimeError("parameters changed between forward and backward of forward_tokens")
        module._attach_grads()
        dhidden = dhidden.to(torch.bfloat16).contiguous()   # bf16 or fp32 in, bf16 to the kernels
        with torch.cuda.device(ids.device):
            _native.check(lib.sskd_generic_backward_hidden(
                module.cfg_struct, module.w_struct, module.g_struct, ids.data_ptr(), mask.data_ptr(), B, S,
                dhidden.data_ptr(), ctx.ws.data_ptr(), ctx.ws.numel(), _native.current_stream_ptr(ids.device)))
        ctx.ws = None
        return (None, None, None) + (None,) * len(module.names)


class TrainableEncoder(nn.Module):
    """fp32 master parameters (HF ``BertModel`` names) + the bf16 device copies the kernels read.

    Every parameter is a VIEW of one flat fp32 buffer laid out the way the C-ABI wants it (per layer: Wq, Wk, Wv
    back to back = the fused [3H, H] QKV matrix, then their biases, ...), and every ``.grad`` a view of a second flat
    buffer with the same layout.  That makes the per-step housekeeping three launches instead of ~450: ONE cast of the
    flat master to bf16 + FOUR batched transposes (the backward's W^T operands, all 12 layers per launch) after an
    optimizer step, ONE memset of the gradients.  Optimizers see ordinary ``nn.Parameter``s."""

    def __init__(self, config: BertConfig, state_dict: Dict[str, np.ndarray], device, pos_offset: int = 0) -> None:
        super().__init__()
        _native.require_gpu()
        self.config = config
        self.device = torch.device(device)
        self.pos_offset = pos_offset
        H, F, L = config.hidden_size, config.intermediate_size, config.num_hidden_layers
        # ---- layout (element offsets into the flat buffers) ----
        layer_fields = [(n, field_shape(config, dims)) for _, names, dims in LAYER_FIELDS for n in names]
        self._field_off: Dict[str, int] = {}
        off = 0
        for suffix, shape in layer_fields:
            self._field_off[suffix] = off
            off += int(np.prod(shape))
        self._layer_stride = off
        layout: Dict[str, tuple] = {}
        for i in range(L):
            for suffix, shape in layer_fields:
                layout[f"encoder.layer.{i}.{suffix}"] = (i * self._layer_stride + self._field_off[suffix], shape)
        off = L * self._layer_stride
        for _, (name,), dims in EMBEDDING_FIELDS:
            shape = field_shape(config, dims)
            layout[name] = (off, shape)
            off += int(np.prod(shape))
        if H % 8 or F % 8:
            raise ValueError("hidden / intermediate sizes must be multiples of 8 (16-byte aligned bf16 rows)")
        self._layout, self._total = layout, off
        flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.names: List[str] = []
        for name, arr in state_dict.items():
            if name.endswith("position_ids") or name.startswith("pooler."):
                continue
            if name not in layout:
                raise KeyError(f"unexpected parameter {name!r}")
            o, shape = layout[name]
            if tuple(arr.shape) != tuple(shape):
                raise ValueError(f"{name}: shape {tuple(arr.shape)} != {tuple(shape)}")
            flat[o : o + int(np.prod(shape))] = torch.from_numpy(np.ascontiguousarray(arr, np.float32)).reshape(-1).to(self.device)
            self.names.append(name)
        missing = set(layout) - set(self.names)
        if missing:
            raise KeyError(f"state dict lacks {sorted(missing)[:3]} ...")
        self._flat = flat
        for name in self.names:   # parameters share the flat buffer's storage
            o, shape = layout[name]
            self.register_parameter(_pname(name), nn.Parameter(flat[o : o + int(np.prod(shape))].view(shape)))
        self._flat_grad = torch.zeros(off, dtype=torch.float32, device=self.device)
        self._flat_bf16 = torch.empty(off, dtype=torch.bfloat16, device=self.device)
        self.cfg_struct = _native.GenericConfig(
            config.vocab_size, config.hidden_size, config.num_hidden_layers, config.num_attention_heads,
            config.intermediate_size, config.max_position_embeddings, config.type_vocab_size,
            float(config.layer_norm_eps), pos_offset)
        self._weights_version = -1
        self._seen_versions: Optional[tuple] = None
        self._epoch = 0   # bumped by invalidate(): changes that torch's version counters do not see (HIP-graph replays)
        self._keep: list = []
        self.w_struct = None
        self.g_struct, self._g_layers = _native.GenericGrads(), (_native.GenericLayerGrads * max(L, 1))()
        self._point(self.g_struct, self._g_layers, self._flat_grad.data_ptr(), 4)

    def p(self, hf_name: str) -> nn.Parameter:
        return getattr(self, _pname(hf_name))

    @property
    def flat_grad(self) -> torch.Tensor:
        """every parameter's gradient in ONE fp32 tensor (the buffer all ``p.grad`` are views of): what a data-parallel
        trainer all-reduces after ``backward()`` - the backward writes gradients as side effects, so autograd hooks
        (DDP's mechanism) never fire"""
        return self._flat_grad

    def _check_autograd_contract(self) -> None:
        """The HIP backward hands autograd ``None`` for every parameter and writes ``p.grad`` itself: refuse the uses
        that would silently get no gradient."""
        for name in self.names:
            q = self.p(name)
            if not q.requires_grad:
                raise NotImplementedError(
                    f"{name}: requires_grad=False on a single parameter is not served by the fused backward "
                    "(it writes every gradient); freeze by leaving the parameter out of the optimizer")
            if getattr(q, "_backward_hooks", None) or getattr(q, "_post_accumulate_grad_hooks", None):
                raise NotImplementedError(
                    f"{name} carries autograd hooks (DistributedDataParallel?): the fused backward writes p.grad as a "
                    "side effect and hooks would never fire - all-reduce TrainableEncoder.flat_grad instead")

    def _off(self, layer: int, suffix: str) -> int:
        return layer * self._layer_stride + self._field_off[suffix]

    # -------------------------------------------------------------- device copies
    def invalidate(self) -> None:
        """Force the bf16 copies to be rebuilt at the next forward.  Needed only after parameters were changed through
        ``p.data`` / ``torch.no_grad`` tricks that do not bump the tensors' version counters (in-place optimizer steps
        do bump them and are picked up automatically) - and after REPLAYING a captured training step (GraphedStep): a
        replay updates the parameters on the device without touching torch's counters."""
        self._seen_versions = None
        self._epoch += 1

    def _refresh_device_weights(self) -> None:
        params = list(self.parameters())
        for q in params:   # a parameter re-pointed at foreign storage (load_state_dict copies in place and is fine)
            if q.untyped_storage().data_ptr() != self._flat.untyped_storage().data_ptr():
                raise RuntimeError("a parameter no longer lives in the flat master buffer (assign with p.data.copy_ / load_state_dict)")
        versions = tuple(q._version for q in params)
        if versions == self._seen_versions and self.w_struct is not None:
            return
        L = self.config.num_hidden_layers
        self._flat_bf16.copy_(self._flat)                                   # ONE cast kernel for all parameters
        w, layers, keep = _native.GenericWeights(), (_native.GenericLayerWeights * max(L, 1))(), []
        self._point(w, layers, self._flat_bf16.data_ptr(), 2, ndim=2)
        self._point(w, layers, self._flat.data_ptr(), 4, ndim=1)
        for field, names, dims in LAYER_FIELDS:   # the backward's W^T operands: [L, cols, rows], one launch for all layers
            if len(dims) == 2:
                rows, cols = field_shape(self.config, dims)
                rows *= len(names)
                wt = self._flat_bf16.as_strided((L, rows, cols), (self._layer_stride, cols, 1), self._field_off[names[0]])
                wt = wt.transpose(1, 2).contiguous()
                keep.append(wt)
                for i in range(L):
                    setattr(layers[i], field + "_t", wt[i].data_ptr())
        self.w_struct, self._layers_struct, self._keep = w, layers, keep
        self._seen_versions = versions
        self._weights_version += 1

    def _point(self, top, layers, base: int, size: int, ndim: Optional[int] = None) -> None:
        """Point the table's fields of ``top`` (GenericWeights / GenericGrads) and of its ``layers`` at
        ``base + size * offset`` of their (first) tensor in the flat layout; ``ndim`` restricts it to the matrices (2)
        or the vectors (1)."""
        top.layers = layers
        for field, names, dims in EMBEDDING_FIELDS:
            if ndim in (None, len(dims)):
                setattr(top, field, base + size * self._layout[names[0]][0])
        for i in range(self.config.num_hidden_layers):
            for field, names, dims in LAYER_FIELDS:
                if ndim in (None, len(dims)):
                    setattr(layers[i], field, base + size * self._off(i, names[0]))

    # -------------------------------------------------------------- gradients
    def _attach_grads(self) -> None:
        """Make every ``p.grad`` the matching view of the flat gradient buffer.  Gradients that were ``None`` (after
        ``zero_grad(set_to_none=True)`` or before the first step) start from ONE memset; gradients that already are our
        views keep their contents (autograd semantics: backward accumulates); foreign ``.grad`` tensors are folded in."""
        params = [self.p(n) for n in self.names]
        ours = [q.grad is not None and q.grad.untyped_storage().data_ptr() == self._flat_grad.untyped_storage().data_ptr()
                for q in params]
        if all(ours):
            return
        if not any(ours):
            self._flat_grad.zero_()
        for name, q, mine in zip(self.names, params, ours):
            if mine:
                continue
            o, shape = self._layout[name]
            view = self._flat_grad[o : o + int(np.prod(shape))].view(shape)
            if any(ours):
                view.zero_()                      # mixed state: this slot was dropped, the others are live
            if q.grad is not None:
                view.add_(q.grad)                 # a gradient somebody else put there
            q.grad = view

    # -------------------------------------------------------------- forward
    def forward(self, input_ids, attention_mask=None, normalize: bool = True) -> torch.Tensor:
        """ids / mask ``[B, S]`` -> embeddings ``[B, hidden]`` (fp32, on device, differentiable with
        respect to every parameter).  S is padded to a multiple of 32 here."""
        ids, mask = _native.padded_ids_mask(input_ids, attention_mask, self.device)
        params = [self.p(n) for n in self.names]
        return _EncoderFunction.apply(self, ids, mask, normalize, *params)

    def forward_tokens(self, input_ids, attention_mask=None) -> torch.Tensor:
        """ids / mask ``[B, S]`` -> the final hidden states bf16 ``[B, S', hidden]`` (S' = S padded to a multiple of 32;
        on device, differentiable with respect to every parameter; the gradient may be bf16 or fp32).  What
        ``late_training.maxsim_scores`` normalises into token vectors."""
        ids, mask = _native.padded_ids_mask(input_ids, attention_mask, self.device)
        params = [self.p(n) for n in self.names]
        return _EncoderTokensFunction.apply(self, ids, mask, *params)

    def state_dict_numpy(self) -> Dict[str, np.ndarray]:
        return {n: self.p(n).detach().cpu().numpy() for n in self.names}


def kd_step_scores(query_emb: torch.Tensor, doc_embs: torch.Tensor) -> torch.Tensor:
    """``torch.matmul(query_emb, doc_embs.T)[0]`` of the reference step (src/kd/train.py:189)."""
    return torch.matmul(query_emb, doc_embs.T)[0]


class GraphedStep:
    """ONE training step - every encoder forward, the loss, the backward pass and the optimizer update - captured into
    a HIP graph and replayed (reference step: src/kd/train.py:176-210).

    The KD step is ~800 short launches per 30 ms: replayed as one graph it no longer depends on how fast the host can
    issue them (round 3 measured 111-132 ms for the same 30 ms of kernels on a box whose host cores were busy).
    Nothing in the C-ABI allocates or synchronises, so every launch of a step is capturable; torch's caching allocator
    serves the step's temporaries from the graph's private pool.

    ``step_fn()`` runs one whole step on the CURRENT stream and returns a tensor (the loss) or a tuple of tensors; it
    must read its batch from tensors that keep their storage (``GraphedStep.copy_inputs`` / ``tensor.copy_``) and must
    not synchronise (no ``.item()``, no host reads).  The optimizer must be created with ``capturable=True``.
    ``opt.zero_grad(set_to_none=True)`` inside ``step_fn`` is fine: the gradient views are re-attached during capture
    and the memset of the flat gradient buffer is part of the graph."""

    def __init__(self, step_fn, warmup: int = 3, modules: Sequence["TrainableEncoder"] = ()) -> None:
        """``modules``: the ``TrainableEncoder``s the step trains.  A replay changes their parameters without bumping
        torch's version counters, so every replay marks them stale (``invalidate()``): the next EAGER forward - an
        evaluation between steps, ``Mi355xSentenceEncoder.encode`` - then re-casts the weights instead of using the bf16
        copies of one optimizer step ago."""
        _native.require_gpu()
        self._fn = step_fn
        self._modules = list(modules)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # warm-up off the default stream, as torch's capture rules ask
            for _ in range(max(int(warmup), 1)):
                step_fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = step_fn()
        self.steps_replayed = 0

    def __call__(self):
        self.graph.replay()
        self.steps_replayed += 1
        for m in self._modules:
            m.invalidate()
        return self.out

    @staticmethod
    def copy_inputs(static: Sequence[torch.Tensor], fresh: Sequence[torch.Tensor]) -> None:
        """copy the next batch into the tensors the captured step reads (same shapes)"""
        for dst, src in zip(static, fresh):
            if dst.shape != src.shape:
                raise ValueError(f"a captured step has fixed shapes: {tuple(dst.shape)} != {tuple(src.shape)}")
            dst.copy_(src, non_blocking=True)
