"""Training through MaxSim on the MI355X: token states -> the ``[nq, R]`` score matrix the KD losses take.

``score[q, c] = sum_i max_t <q_i, d_cand[q,c],t>`` over L2-normalised bf16 token vectors - the number
``LateInteractionIndex`` ranks by, bit for bit (``sskd_latet_maxsim_fwd`` is the re-rank's score kernel plus the argmax) -
behind ONE ``torch.autograd.Function`` that spans pack -> forward -> backward -> pack backward, all HIP
(csrc/late.hip, csrc/late_train.hip).  The fp32 token gradients stay inside the Function: autograd only ever sees the bf16
hidden states of ``TrainableEncoder.forward_tokens`` and their bf16 gradients.  Nothing synchronises with the host, so a
step built from these calls can be captured by ``training.GraphedStep`` (build the ``TokenLayout``s before the capture:
they upload the lengths).  ``hidden_size`` 384 only; everything else raises before anything is enqueued.  No CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _native

DIM = 384
TQ_MAX = 128
R_MAX = 1024


class TokenLayout:
    """The real-token counts of a batch of texts, on the host (validated there) and on the device (read by the kernels):
    ``lengths [B]``, ``lims [B + 1]`` = their running sum from 0.  Fixed for the life of a captured step."""

    def __init__(self, lengths, device) -> None:
        if isinstance(lengths, torch.Tensor):
            lengths = lengths.detach().cpu().numpy()
        self.lengths = np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int64)
        if self.lengths.size and int(self.lengths.min()) < 1:
            raise ValueError(f"text {int(np.argmin(self.lengths))} has no tokens: MaxSim needs at least one token per text")
        self.lims = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.device = torch.device(device)
        self.lengths_dev = torch.from_numpy(self.lengths.astype(np.int32)).to(self.device)
        self.lims_dev = torch.from_numpy(self.lims).to(self.device)
        self.lengths_f32 = self.lengths_dev.to(torch.float32)

    @property
    def n(self) -> int:
        return int(self.lengths.size)

    @property
    def n_tokens(self) -> int:
        return int(self.lims[-1])

    @property
    def longest(self) -> int:
        return int(self.lengths.max()) if self.lengths.size else 0


class TokenStates:
    """Final hidden states of a batch of texts, bf16 ``[B, S, 384]`` on the device (``TrainableEncoder.forward_tokens``;
    differentiable), and how many positions of every text are real tokens (``lengths``: a sequence, or a ``TokenLayout``
    built once and shared between steps)."""

    def __init__(self, hidden: torch.Tensor, lengths: Union[Sequence[int], np.ndarray, torch.Tensor, TokenLayout]) -> None:
        if hidden.dim() != 3 or hidden.dtype != torch.bfloat16 or not hidden.is_cuda:
            raise ValueError("hidden: expected a device bf16 [B, S, H] tensor")
        if hidden.shape[2] != DIM:
            raise ValueError(f"hidden size {hidden.shape[2]}: the late-interaction kernels are built for {DIM}")
        self.hidden = hidden
        self.layout = lengths if isinstance(lengths, TokenLayout) else TokenLayout(lengths, hidden.device)
        if self.layout.device != hidden.device:
            raise ValueError("the layout lives on another device than the hidden states")
        if self.layout.n != hidden.shape[0]:
            raise ValueError(f"{self.layout.n} lengths for {hidden.shape[0]} texts")
        if self.layout.longest > hidden.shape[1]:
            raise ValueError(f"a text of {self.layout.longest} tokens in hidden states of {hidden.shape[1]} positions")

    @property
    def lengths(self) -> np.ndarray:
        return self.layout.lengths


def _pack(hidden: torch.Tensor, lay: TokenLayout) -> torch.Tensor:
    out = torch.empty((lay.n_tokens, DIM), dtype=torch.bfloat16, device=hidden.device)
    B, S = hidden.shape[0], hidden.shape[1]
    _native.check(_native.load().sskd_late_pack_tokens(
        hidden.data_ptr(), lay.lengths_dev.data_ptr(), lay.lims_dev.data_ptr(), B, S, lay.n_tokens, out.data_ptr(),
        _native.current_stream_ptr(hidden.device)))
    return out


def _pack_bwd(hidden: torch.Tensor, lay: TokenLayout, dtok: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(hidden)
    B, S, H = hidden.shape
    _native.check(_native.load().sskd_latet_pack_tokens_bwd(
        hidden.data_ptr(), lay.lengths_dev.data_ptr(), lay.lims_dev.data_ptr(), B, S, H, lay.n_tokens, dtok.data_ptr(),
        out.data_ptr(), _native.current_stream_ptr(hidden.device)))
    return out


def maxsim_forward(q_tok: torch.Tensor, ql: TokenLayout, d_tok: torch.Tensor, dl: TokenLayout, cand: torch.Tensor):
    """``sskd_latet_maxsim_fwd`` over packed tokens: ``(scores fp32 [nq, R], arg int32 [nq, R, tq_stride])``, R <= 1024."""
    nq, R = cand.shape
    stride = -(-ql.longest // 32) * 32
    scores = torch.empty((nq, R), dtype=torch.float32, device=cand.device)
    arg = torch.empty((nq, R, stride), dtype=torch.int32, device=cand.device)
    _native.check(_native.load().sskd_latet_maxsim_fwd(
        q_tok.data_ptr(), ql.lims.ctypes.data, ql.lims_dev.data_ptr(), nq, ql.n_tokens, d_tok.data_ptr(),
        dl.lims_dev.data_ptr(), dl.n, dl.n_tokens, cand.data_ptr(), R, scores.data_ptr(), arg.data_ptr(), stride,
        _native.current_stream_ptr(cand.device)))
    return scores, arg


def maxsim_grad_q(d_tok: torch.Tensor, dl: TokenLayout, ql: TokenLayout, cand: torch.Tensor, arg: torch.Tensor,
                  g: torch.Tensor) -> torch.Tensor:
    """``sskd_latet_maxsim_bwd_q``: ``dQ`` fp32 ``[sum Tq, 384]``."""
    nq, R = cand.shape
    dq = torch.empty((ql.n_tokens, DIM), dtype=torch.float32, device=cand.device)
    _native.check(_native.load().sskd_latet_maxsim_bwd_q(
        d_tok.data_ptr(), dl.lims_dev.data_ptr(), dl.n, dl.n_tokens, ql.lims.ctypes.data, ql.lims_dev.data_ptr(), nq,
        ql.n_tokens, cand.data_ptr(), R, arg.data_ptr(), arg.shape[2], g.data_ptr(), dq.data_ptr(),
        _native.current_stream_ptr(cand.device)))
    return dq


def destination_segments(dl: TokenLayout, cand: torch.Tensor, arg: torch.Tensor):
    """The per-destination form of MaxSim's document gradient: contribution ``e = (q R + c) tq_stride + i`` goes to token
    row ``lims_d[cand[q, c]] + arg[q, c, i]`` (key ``sum Td`` when ``arg < 0``).  ``(order int64 [E], seg int64
    [sum Td + 1])``: the contributions stably sorted by key and where every row's run begins.  Device work only."""
    T = dl.n_tokens
    base = dl.lims_dev[cand.clamp(0, max(dl.n - 1, 0))]                     # arg >= 0 only where cand names a document
    key = torch.where(arg >= 0, base.unsqueeze(2) + arg.to(torch.int64), torch.full_like(base, T).unsqueeze(2))
    skey, order = torch.sort(key.reshape(-1), stable=True)
    seg = torch.searchsorted(skey, torch.arange(T + 1, dtype=torch.int64, device=cand.device))
    return order.contiguous(), seg.contiguous()


def maxsim_grad_d(q_tok: torch.Tensor, ql: TokenLayout, dl: TokenLayout, cand: torch.Tensor, arg: torch.Tensor,
                  g: torch.Tensor) -> torch.Tensor:
    """``sskd_latet_maxsim_bwd_d`` behind ``destination_segments``: ``dD`` fp32 ``[sum Td, 384]``."""
    nq, R = cand.shape
    order, seg = destination_segments(dl, cand, arg)
    dd = torch.empty((dl.n_tokens, DIM), dtype=torch.float32, device=cand.device)
    _native.check(_native.load().sskd_latet_maxsim_bwd_d(
        q_tok.data_ptr(), ql.lims.ctypes.data, ql.lims_dev.data_ptr(), nq, ql.n_tokens, R, arg.shape[2], order.data_ptr(),
        seg.data_ptr(), dl.n_tokens, g.data_ptr(), dd.data_ptr(), _native.current_stream_ptr(cand.device)))
    return dd


class _MaxSimFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q_hidden: torch.Tensor, d_hidden: torch.Tensor, ql: TokenLayout, dl: TokenLayout, cand: torch.Tensor):
        q_hidden, d_hidden = q_hidden.contiguous(), d_hidden.contiguous()
        with torch.cuda.device(q_hidden.device):
            q_tok, d_tok = _pack(q_hidden, ql), _pack(d_hidden, dl)
            chunks = []
            for lo in range(0, cand.shape[1], R_MAX):       # the kernels take R <= 1024 per call
                part = cand[:, lo: lo + R_MAX].contiguous()
                scores, arg = maxsim_forward(q_tok, ql, d_tok, dl, part)
                chunks.append((lo, part, arg, scores))
        ctx.ql, ctx.dl = ql, dl
        ctx.chunks = [(lo, part, arg) for lo, part, arg, _ in chunks]
        ctx.save_for_backward(q_hidden, d_hidden, q_tok, d_tok)
        return chunks[0][3] if len(chunks) == 1 else torch.cat([c[3] for c in chunks], dim=1)

    @staticmethod
    def backward(ctx, g):
        q_hidden, d_hidden, q_tok, d_tok = ctx.saved_tensors
        ql, dl = ctx.ql, ctx.dl
        g = g.to(torch.float32)
        dq = dd = None
        with torch.cuda.device(q_hidden.device):
            for lo, part, arg in ctx.chunks:
                gc = g[:, lo: lo + part.shape[1]].contiguous()
                if ctx.needs_input_grad[0]:
                    one = maxsim_grad_q(d_tok, dl, ql, part, arg, gc)
                    dq = one if dq is None else dq + one
                if ctx.needs_input_grad[1]:
                    one = maxsim_grad_d(q_tok, ql, dl, part, arg, gc)
                    dd = one if dd is None else dd + one
            # fp32 token gradients -> bf16 hidden-state gradients, without a pass through autograd's dtype cast
            dqh = _pack_bwd(q_hidden, ql, dq) if dq is not None else None
            ddh = _pack_bwd(d_hidden, dl, dd) if dd is not None else None
        return dqh, ddh, None, None, None


def maxsim_scores(q: TokenStates, d: TokenStates, cand: Optional[torch.Tensor] = None, docs_per_query: Optional[int] = None,
                  mean: bool = True) -> torch.Tensor:
    """Differentiable MaxSim, fp32 ``[nq, R]``: what ``CombinedKDLoss`` takes as student scores.

    ``cand=None`` scores every document of ``d`` for every query (in-batch negatives); ``docs_per_query=n`` scores query
    ``q`` against documents ``q n .. q n + n - 1`` (the reference step's layout: positive + hard negatives per query);
    an explicit device int64 ``[nq, R]`` table names documents of the batch (-1 or an id outside it: an absent pair, score
    ``-inf``, no gradient; a document may be named twice, both entries contribute).  ``mean`` divides by the query's
    token count, the normalisation ``/search`` applies.  Gradients reach ``q.hidden`` and ``d.hidden`` as bf16."""
    _native.require_gpu()
    if not isinstance(q, TokenStates) or not isinstance(d, TokenStates):
        raise TypeError("maxsim_scores takes TokenStates (StudentModel.encode_tokens_with_gradients)")
    dev = q.hidden.device
    if d.hidden.device != dev:
        raise ValueError("queries and documents live on different devices")
    ql, dl = q.layout, d.layout
    nq, nd = ql.n, dl.n
    if nq < 1 or nd < 1:
        raise ValueError("maxsim_scores needs at least one query and one document")
    if ql.longest > TQ_MAX:
        raise ValueError(f"a query of {ql.longest} tokens: at most {TQ_MAX} (cut it with max_tokens)")
    if cand is not None and docs_per_query is not None:
        raise ValueError("pass cand or docs_per_query, not both")
    if docs_per_query is not None:
        n = int(docs_per_query)
        if n < 1 or nq * n != nd:
            raise ValueError(f"docs_per_query={n}: {nq} queries need {nq * n} documents, there are {nd}")
        cand = torch.arange(nd, dtype=torch.int64, device=dev).view(nq, n)
    elif cand is None:
        cand = torch.arange(nd, dtype=torch.int64, device=dev).unsqueeze(0).expand(nq, nd).contiguous()
    else:
        if cand.dim() != 2 or cand.dtype != torch.int64 or cand.device != dev or cand.shape[0] != nq or cand.shape[1] < 1:
            raise ValueError(f"cand: expected a device int64 [{nq}, R >= 1] tensor")
        cand = cand.contiguous()
    scores = _MaxSimFunction.apply(q.hidden, d.hidden, ql, dl, cand)
    return scores / ql.lengths_f32.unsqueeze(1) if mean else scores
