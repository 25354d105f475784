"""``LateInteractionIndex``: token-level MaxSim re-ranking (ColBERT's late interaction) over the rows of a flat index.

The reference's ``configs/service.yaml`` carries ``features.enable_late_interaction`` (``.env.example``:
``ENABLE_LATE_INTERACTION``) with no code behind it, as it did ``features.enable_hybrid``; this is the code.

* The rows stay the ``FAISSIndexBuilder`` (``late.flat``).  Beside it lives the token store: one L2-normalised bf16
  ``[384]`` row per real token of every document (``[CLS]`` and ``[SEP]`` included, padding not), 768 B each, in CSR
  order - the tokens of row ``r`` are store rows ``lims[r] .. lims[r + 1] - 1``.
* ``score(q, c) = sum_i max_j <q_i, d_j>`` over the query's and the document's tokens (``include/sskd_amd.h``, "Late
  interaction": bf16 MFMA dot products, fp32 max, sequential fp32 sum).  A score's bits depend on the two token lists
  alone.  A first stage - the flat index or any index over the same rows - proposes ``candidates`` rows per query by
  their pooled vectors, ``rerank_device`` orders them by MaxSim: score descending, ties by lower id, ``(-inf, -1)``
  padding.  A row without tokens is no candidate.
* Row filters and removed rows are the first stage's business: what it does not return is not re-ranked.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native
from .index import FAISSIndexBuilder, _host_queries_to_device
from .overlay import read_versioned_json

DIM = _native.SSKD_DIM
LATE_TQ_MAX = 128
LATE_R_MAX = 1024
TOKEN_BYTES = DIM * 2
FORMAT_VERSION = 1


# ------------------------------------------------------------------ host-side helpers (NumPy, no GPU)
def check_lims(lims, n_rows: Optional[int] = None, n_tokens: Optional[int] = None) -> np.ndarray:
    """``lims`` as a contiguous int64 ``[n + 1]`` array; raises ``ValueError`` unless it starts at 0, never descends
    and - when given - has ``n_rows + 1`` entries and ends at ``n_tokens``."""
    a = np.ascontiguousarray(np.asarray(lims).astype(np.int64, copy=False)).reshape(-1)
    if a.size < 1 or a[0] != 0 or (a.size > 1 and (np.diff(a) < 0).any()):
        raise ValueError("lims must start at 0 and ascend")
    if n_rows is not None and a.size != n_rows + 1:
        raise ValueError(f"lims has {a.size} entries for {n_rows} rows (needs rows + 1)")
    if n_tokens is not None and a[-1] != n_tokens:
        raise ValueError(f"lims ends at {int(a[-1])}, there are {n_tokens} token rows")
    return a


def store_bytes(n_tokens: int) -> int:
    """HBM (and file) bytes of a store of ``n_tokens`` token rows: 768 B each."""
    return int(n_tokens) * TOKEN_BYTES


def save_store(out_dir: Union[str, Path], tokens_bf16_bits: np.ndarray, lims: np.ndarray, meta: dict) -> None:
    """Writes ``late.json``, ``late_token_lims.npy`` and ``late_tokens.bf16`` (the raw little-endian bf16 rows).
    ``tokens_bf16_bits``: uint16 ``[T, 384]``, the bf16 bit patterns."""
    bits = np.ascontiguousarray(tokens_bf16_bits, dtype=np.uint16).reshape(-1, DIM)
    lims = check_lims(lims, n_tokens=bits.shape[0])
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "late_token_lims.npy", lims)
    bits.tofile(out / "late_tokens.bf16")
    with open(out / "late.json", "w") as f:
        json.dump({**meta, "ntotal": int(lims.size - 1), "n_tokens": int(bits.shape[0]), "dim": DIM, "dtype": "bfloat16",
                   "format_version": FORMAT_VERSION}, f)


def load_store(index_dir: Union[str, Path]):
    """``(tokens uint16 [T, 384], lims int64 [n + 1], meta)`` as ``save_store`` wrote them, checked."""
    d = Path(index_dir)
    meta = read_versioned_json(d / "late.json", FORMAT_VERSION)
    if int(meta.get("dim", -1)) != DIM or meta.get("dtype") != "bfloat16":
        raise ValueError(f"{d / 'late.json'}: expected {DIM}-d bfloat16 tokens")
    lims = check_lims(np.load(d / "late_token_lims.npy"), n_rows=int(meta["ntotal"]), n_tokens=int(meta["n_tokens"]))
    bits = np.fromfile(d / "late_tokens.bf16", dtype=np.uint16)
    if bits.size != int(meta["n_tokens"]) * DIM:
        raise ValueError(f"{d / 'late_tokens.bf16'}: {bits.size * 2} bytes, late.json says {store_bytes(meta['n_tokens'])}")
    return bits.reshape(-1, DIM), lims, meta


def is_late_dir(index_dir: Union[str, Path]) -> bool:
    return (Path(index_dir) / "late.json").exists()


def _tokens_to_device(tokens, device) -> torch.Tensor:
    """fp32 / bf16 token rows, host or device -> contiguous device bf16 ``[T, 384]`` (fp32 is rounded to nearest even; a
    NumPy uint16 array is taken as bf16 bit patterns)."""
    if isinstance(tokens, torch.Tensor):
        t = tokens
    else:
        a = np.ascontiguousarray(tokens)
        if a.dtype == np.uint16:
            t = torch.from_numpy(a.view(np.int16)).view(torch.bfloat16)
        else:
            t = torch.from_numpy(a.astype(np.float32, copy=False))
    t = t.to(device=device).reshape(-1, DIM)
    if t.dtype != torch.bfloat16:
        t = t.to(torch.float32).to(torch.bfloat16)
    return t.contiguous()


class LateQueries:
    """Query tokens prepared for ``rerank_device``: device bf16 ``[sum Tq, 384]`` rows, their CSR bounds on the host
    (validated by the library before anything is enqueued) and on the device (read by the kernel).  Preparing them once
    lets ``rerank_device`` run without a copy, so inside a graph capture."""

    def __init__(self, tokens: torch.Tensor, lims_host: np.ndarray, lims_dev: torch.Tensor):
        self.tokens, self.lims_host, self.lims_dev = tokens, lims_host, lims_dev
        self.nq = int(lims_host.size - 1)


class LateInteractionIndex:
    """Token store + MaxSim re-rank over the rows of ``flat``."""

    def __init__(self, flat: FAISSIndexBuilder, max_doc_tokens: int = 180, max_query_tokens: int = 32) -> None:
        if max_doc_tokens < 2:
            raise ValueError(f"max_doc_tokens={max_doc_tokens} < 2")
        if max_query_tokens < 2 or max_query_tokens > LATE_TQ_MAX:
            raise ValueError(f"max_query_tokens={max_query_tokens} outside [2, {LATE_TQ_MAX}]")
        self.flat = flat
        self.device = flat.device
        self.max_doc_tokens = int(max_doc_tokens)
        self.max_query_tokens = int(max_query_tokens)
        self.tokens: Optional[torch.Tensor] = None       # device bf16 [n_tokens, 384]
        self.lims = np.zeros(1, dtype=np.int64)           # host int64 [rows + 1]
        self._lims_dev: Optional[torch.Tensor] = None
        self._workspace: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ properties
    @property
    def ntotal(self) -> int:
        """Rows the store covers (it serves searches once this equals ``flat.ntotal``)."""
        return int(self.lims.size - 1)

    @property
    def n_tokens(self) -> int:
        return int(self.lims[-1])

    @property
    def nbytes(self) -> int:
        return store_bytes(self.n_tokens)

    def _require_store(self) -> None:
        if self.tokens is None or self.ntotal != self.flat.ntotal:
            raise RuntimeError(f"the token store covers {self.ntotal} rows, the index holds {self.flat.ntotal}: call "
                               "set_tokens / add_tokens / build_from_texts (or load)")

    def tokens_numpy(self) -> np.ndarray:
        """Host copy of the store as bf16 bit patterns, uint16 ``[n_tokens, 384]``."""
        if self.tokens is None:
            return np.zeros((0, DIM), dtype=np.uint16)
        return self.tokens.view(torch.int16).cpu().numpy().view(np.uint16)

    # ------------------------------------------------------------------ filling the store
    def _install(self, tokens: torch.Tensor, lims: np.ndarray) -> None:
        with torch.cuda.device(self.device):
            self.tokens = tokens
            self.lims = lims
            self._lims_dev = torch.from_numpy(lims).to(self.device)

    def set_tokens(self, tokens, lims) -> None:
        """Pre-computed token vectors for rows ``0 .. flat.ntotal - 1``: ``tokens`` ``[T, 384]`` (NumPy fp32, NumPy uint16
        = bf16 bits, or a torch fp32 / bf16 tensor), ``lims`` ``[ntotal + 1]``.  The rows are stored as given (rounded to
        bf16), not normalised again."""
        t = _tokens_to_device(tokens, self.device)
        self._install(t, check_lims(lims, n_rows=self.flat.ntotal, n_tokens=t.shape[0]))

    def add_tokens(self, tokens, lims) -> None:
        """Appends the token vectors of the rows added with ``flat.add`` since: ``lims`` ``[new rows + 1]`` from 0."""
        t = _tokens_to_device(tokens, self.device)
        new = check_lims(lims, n_tokens=t.shape[0])
        if self.ntotal + new.size - 1 > self.flat.ntotal:
            raise ValueError(f"{self.ntotal} + {new.size - 1} rows of tokens for an index of {self.flat.ntotal} rows")
        with torch.cuda.device(self.device):
            both = t if self.tokens is None else torch.cat([self.tokens, t])
        self._install(both, np.concatenate([self.lims, self.lims[-1] + new[1:]]))

    def build_from_texts(self, student, texts: Sequence[str], batch_size: int = 64) -> None:
        """Encodes the documents of rows ``0 .. flat.ntotal - 1`` (``student``: a ``StudentModel``; the E5 passage prefix
        is applied as ``encode_documents`` applies it) and installs their tokens."""
        if len(texts) != self.flat.ntotal:
            raise ValueError(f"{len(texts)} texts for an index of {self.flat.ntotal} rows")
        tokens, lims = student.encode_tokens(list(texts), is_query=False, max_tokens=self.max_doc_tokens,
                                             batch_size=batch_size)
        self._install(tokens, lims)

    # ------------------------------------------------------------------ re-rank
    def prepare_queries(self, q_tokens, q_lims) -> LateQueries:
        """Uploads query tokens (as ``set_tokens`` takes them) and their bounds ``[nq + 1]`` once; the result is what
        ``rerank_device`` takes inside a graph capture."""
        if isinstance(q_tokens, LateQueries):
            return q_tokens
        lims = check_lims(q_lims)
        with torch.cuda.device(self.device):
            t = _tokens_to_device(q_tokens, self.device)
            if t.shape[0] != lims[-1]:
                raise ValueError(f"q_lims ends at {int(lims[-1])}, there are {t.shape[0]} query token rows")
            return LateQueries(t, lims, torch.from_numpy(lims).to(self.device))

    def rerank_device(self, q_tokens, q_lims, cand_I: torch.Tensor, k: int, return_raw: bool = False):
        """MaxSim re-rank of the candidates ``cand_I`` (device int64 ``[nq, R]``, global ids as a first stage returns
        them, -1 = none) to the best ``k``: device tensors ``(D fp32 [nq, k], I int64 [nq, k])``, and the ``[nq, R]`` raw
        scores in candidate order with ``return_raw``.  Everything is enqueued on the current stream with no host
        synchronisation once the queries are prepared (``q_tokens`` a ``LateQueries``, ``q_lims`` then unused)."""
        lib = _native.load()
        self._require_store()
        queries = self.prepare_queries(q_tokens, q_lims)
        if cand_I.dim() != 2 or cand_I.dtype != torch.int64 or not cand_I.is_cuda or cand_I.shape[0] != queries.nq:
            raise ValueError(f"cand_I: expected a device int64 [{queries.nq}, R] tensor")
        cand = cand_I.contiguous()
        nq, R, k = queries.nq, int(cand.shape[1]), int(k)
        D = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        I = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        raw = torch.empty((nq, R), dtype=torch.float32, device=self.device) if return_raw else None
        ws = None
        if raw is None:
            self._workspace = ws = _native.grown(self._workspace, int(lib.sskd_late_rerank_workspace_bytes(nq, R)), self.device)
        _native.check(lib.sskd_late_rerank(
            queries.tokens.data_ptr(), queries.lims_host.ctypes.data, queries.lims_dev.data_ptr(), nq,
            self.tokens.data_ptr(), self._lims_dev.data_ptr(), self.ntotal, self.n_tokens, cand.data_ptr(), R, k,
            self.flat.id_offset, D.data_ptr(), I.data_ptr(), None if raw is None else raw.data_ptr(),
            None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), _native.current_stream_ptr(self.device)))
        return (D, I, raw) if return_raw else (D, I)

    def rerank(self, q_tokens, q_lims, cand_I, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """``rerank_device`` for host candidates, returning NumPy."""
        with torch.cuda.device(self.device):
            cand = cand_I if isinstance(cand_I, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cand_I, dtype=np.int64))
            D, I = self.rerank_device(q_tokens, q_lims, cand.to(self.device), k)
            return D.cpu().numpy(), I.cpu().numpy()

    def search_device(self, q_emb: torch.Tensor, q_tokens, q_lims, k: int, candidates: int = 100, first_stage=None,
                      **first_stage_kw):
        """First stage, then MaxSim: ``first_stage`` (default: the flat index; an ``IVFIndex``, ``IVFPQIndex``,
        ``GraphIndex`` or ``HybridIndex`` over the same rows) is asked for ``candidates`` rows per query through its
        ``search_device`` (``first_stage_kw`` pass through: ``allow``, ``nprobe``, ``ef`` ...; a ``HybridIndex`` also
        needs ``query_texts``), and they are re-ranked to ``k``.  Device tensors ``(D, I)``."""
        first = self.flat if first_stage is None else first_stage
        candidates = int(candidates)
        if candidates < k or candidates > LATE_R_MAX:
            raise ValueError(f"candidates={candidates} outside [k={k}, {LATE_R_MAX}]")
        if "query_texts" in first_stage_kw:
            texts = first_stage_kw.pop("query_texts")
            _, ids = first.search_device(texts, q_emb, k=candidates, **first_stage_kw)
        else:
            _, ids = first.search_device(q_emb, k=candidates, **first_stage_kw)
        return self.rerank_device(q_tokens, q_lims, ids, k)

    def search(self, q_emb, q_tokens, q_lims, k: int = 10, candidates: int = 100, first_stage=None, **first_stage_kw
               ) -> Tuple[np.ndarray, np.ndarray]:
        """``search_device`` for host (or device) pooled query embeddings ``[nq, 384]``, returning NumPy ``(D, I)``."""
        with torch.cuda.device(self.device):
            qd = q_emb if isinstance(q_emb, torch.Tensor) else _host_queries_to_device(q_emb, self.device)
            D, I = self.search_device(qd, q_tokens, q_lims, k, candidates=candidates, first_stage=first_stage,
                                      **first_stage_kw)
            return D.cpu().numpy(), I.cpu().numpy()

    # ------------------------------------------------------------------ maintenance
    def compact(self, kept) -> None:
        """After ``flat.compact()``: ``kept`` is what it returned (the surviving OLD ids, ascending).  The surviving
        rows' tokens are gathered in their new order; their bits, and so their scores, stay."""
        old = np.asarray(kept, dtype=np.int64) - self.flat.id_offset
        if old.size and (old.min() < 0 or old.max() >= self.ntotal):
            raise ValueError(f"kept rows outside [0, {self.ntotal})")
        counts = self.lims[old + 1] - self.lims[old]
        lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        take = np.repeat(self.lims[old] - lims[:-1], counts) + np.arange(int(lims[-1]), dtype=np.int64)
        with torch.cuda.device(self.device):
            tokens = self.tokens[torch.from_numpy(take).to(self.device)].contiguous()
        self._install(tokens, lims)

    def save(self, output_dir: Union[str, Path]) -> None:
        """``late.json``, ``late_token_lims.npy`` and ``late_tokens.bf16`` beside the index's own files (which the
        index's ``save`` writes)."""
        if self.tokens is None:
            raise RuntimeError("save(): the token store is empty")
        save_store(output_dir, self.tokens_numpy(), self.lims,
                   {"max_doc_tokens": self.max_doc_tokens, "max_query_tokens": self.max_query_tokens})

    def load(self, index_dir: Union[str, Path]) -> None:
        """The store of ``index_dir`` over the rows ``self.flat`` already holds; a store over another number of rows
        raises ``ValueError``."""
        bits, lims, meta = load_store(index_dir)
        if lims.size - 1 != self.flat.ntotal:
            raise ValueError(f"{index_dir}: a token store over {lims.size - 1} rows, the index holds {self.flat.ntotal}")
        self.max_doc_tokens = int(meta.get("max_doc_tokens", self.max_doc_tokens))
        self.max_query_tokens = int(meta.get("max_query_tokens", self.max_query_tokens))
        self._install(_tokens_to_device(bits, self.device), lims)

    def cleanup(self) -> None:
        self.tokens = self._lims_dev = self._workspace = None
        self.lims = np.zeros(1, dtype=np.int64)


def pack_tokens(hidden: torch.Tensor, lengths, offsets, out: torch.Tensor) -> None:
    """``sskd_late_pack_tokens``: normalises the first ``lengths[b]`` positions of every text of ``hidden`` (device bf16
    ``[B, S, 384]``) into rows ``offsets[b] ..`` of ``out`` (device bf16 ``[T, 384]``) on the current stream."""
    device = hidden.device
    B, S = hidden.shape[0], hidden.shape[1]
    ln = _native.as_device_i32(lengths, device).contiguous()
    off = offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int64))
    off = off.to(device=device, dtype=torch.int64).contiguous()
    hidden = hidden.contiguous()
    _native.check(_native.load().sskd_late_pack_tokens(hidden.data_ptr(), ln.data_ptr(), off.data_ptr(), B, S, out.shape[0],
                                                       out.data_ptr(), _native.current_stream_ptr(device)))


def encode_tokens_device(encoder, texts: Sequence[str], max_tokens: int, batch_size: int = 64
                         ) -> Tuple[torch.Tensor, np.ndarray]:
    """``(tokens bf16 device [T, 384], lims int64 [n + 1])`` of ``texts``: tokenised (truncated to ``max_tokens`` keeping
    the closing ``[SEP]``), encoded in length-sorted padded batches through ``encoder.hidden_states`` and packed with
    ``sskd_late_pack_tokens``."""
    rows = _token_rows(encoder, texts, max_tokens)
    lengths = np.fromiter((len(r) for r in rows), np.int64, count=len(rows))
    lims = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    with torch.cuda.device(encoder.device):
        out = torch.empty((int(lims[-1]), DIM), dtype=torch.bfloat16, device=encoder.device)
        order = np.argsort(lengths, kind="stable")
        for lo in range(0, len(rows), batch_size):
            pick = order[lo: lo + batch_size]
            width = int(lengths[pick].max())
            ids = np.zeros((len(pick), width), np.int32)
            mask = np.zeros((len(pick), width), np.int32)
            for j, r in enumerate(pick):
                ids[j, : lengths[r]] = rows[r]
                mask[j, : lengths[r]] = 1
            pack_tokens(encoder.hidden_states(ids, mask), lengths[pick].astype(np.int32), lims[pick], out)
    return out, lims


def _token_rows(encoder, texts: Sequence[str], max_tokens: int):
    """WordPiece ids of every text (the encoder's own tokenizer and ``max_seq_length``), cut to ``max_tokens`` keeping
    the closing ``[SEP]``."""
    flat, lengths = encoder._tokenize_flat(list(texts))
    rows = np.split(np.asarray(flat, np.int32), np.cumsum(lengths)[:-1]) if len(lengths) else []
    return [r if len(r) <= max_tokens else np.concatenate([r[: max_tokens - 1], r[-1:]]) for r in rows]
