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
* With a codec (``train_codec`` / ``set_codec``) the store can be held compressed, as ColBERTv2 / PLAID hold theirs: per
  token the id of its nearest centroid, ``nbits`` in {2, 4} bits per column for the residual and one fp32 scale - 104 B
  or 200 B instead of 768 B.  ``sskd_latec_rerank`` decodes inside the MaxSim kernel; the rules are in
  ``include/sskd_amd.h``, "Compressed token store".  Without a codec nothing changes.
* With centroid lists over a compressed store (``build_centroid_lists``: list ``c`` = the rows that own a token of centroid
  ``c``) the store is a retriever of its own, as PLAID's first stages are: ``search_tokens`` scores every centroid against
  every query token, probes the ``nprobe`` best lists per token, orders the rows found by the centroid interaction
  ``sum_i max_j S[cid_j, t_i]`` and hands the best ``ndocs`` to the compressed MaxSim (``include/sskd_amd.h``, "Candidate
  generation").  Without lists nothing changes.
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
LATE_C_MAX = 65536
PLAID_NPROBE_MAX = 32
PLAID_S_BUDGET = 256 << 20     # bytes of centroid scores one chunk of queries may take
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


def store_bytes(n_tokens: int, nbits: int = 0) -> int:
    """HBM (and file) bytes of a store of ``n_tokens`` token rows: 768 B each as bf16 (``nbits = 0``); compressed, a
    4-byte centroid id, a 4-byte scale and ``48 * nbits`` code bytes - 104 B at 2 bits, 200 B at 4 (the codec itself:
    ``codec_bytes``)."""
    if nbits == 0:
        return int(n_tokens) * TOKEN_BYTES
    _check_nbits(nbits)
    return int(n_tokens) * (8 + code_bytes(nbits))


def _check_nbits(nbits) -> int:
    if nbits not in (2, 4):
        raise ValueError(f"nbits={nbits}: the compressed store takes 2 or 4 bits per column")
    return int(nbits)


def code_bytes(nbits: int) -> int:
    """Code bytes of one compressed token: 96 or 192."""
    return DIM * int(nbits) // 8


def codec_bytes(n_centroids: int, nbits: int) -> int:
    """Bytes of a codec: bf16 centroids, ``2^nbits - 1`` fp32 cutoffs, ``2^nbits`` fp32 weights."""
    return int(n_centroids) * TOKEN_BYTES + 4 * ((1 << nbits) - 1) + 4 * (1 << nbits)


def default_n_centroids(n_tokens: int, sample_tokens: Optional[int] = None) -> int:
    """The largest power of two ``<= 16 sqrt(n_tokens)``, at most 65 536 and at most the sample size."""
    c = 1
    while 2 * c <= 16.0 * float(np.sqrt(max(int(n_tokens), 1))) and 2 * c <= LATE_C_MAX:
        c *= 2
    return int(max(1, min(c, int(n_tokens) if sample_tokens is None else int(sample_tokens))))


def check_codec(centroids, cutoffs, weights):
    """A caller's codec, validated on the host: ``(centroid bf16 bits uint16 [C, 384], cutoffs fp32 [L - 1], weights
    fp32 [L], nbits)``.  ``centroids``: NumPy uint16 (bf16 bits), NumPy / torch floating point (rounded to bf16, nearest
    even).  Raises ``ValueError`` for a wrong shape, ``C`` outside [1, 65 536], ``L`` not 4 or 16, cutoffs that do not
    ascend, and anything not finite."""
    if isinstance(centroids, torch.Tensor):
        bits = centroids.detach().to(torch.float32).to(torch.bfloat16).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    else:
        a = np.asarray(centroids)
        if a.dtype == np.uint16:
            bits = np.ascontiguousarray(a)
        else:
            bits = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    if bits.ndim != 2 or bits.shape[1] != DIM:
        raise ValueError(f"centroids: expected [C, {DIM}], got {tuple(bits.shape)}")
    if not 1 <= bits.shape[0] <= LATE_C_MAX:
        raise ValueError(f"centroids: C={bits.shape[0]} outside [1, {LATE_C_MAX}]")
    if ((bits & 0x7F80) == 0x7F80).any():
        raise ValueError("centroids must be finite")
    cut = np.ascontiguousarray(np.asarray(cutoffs, dtype=np.float32))
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32))
    if w.ndim != 1 or w.size not in (4, 16):
        raise ValueError(f"weights: expected [4] (2 bits) or [16] (4 bits), got {tuple(w.shape)}")
    if cut.ndim != 1 or cut.size != w.size - 1:
        raise ValueError(f"cutoffs: expected [{w.size - 1}] for {w.size} weights, got {tuple(cut.shape)}")
    if not np.isfinite(w).all():
        raise ValueError("weights must be finite")
    if not np.isfinite(cut).all() or (np.diff(cut) < 0).any():
        raise ValueError("cutoffs must be finite and ascend")
    return bits, cut, w, 2 if w.size == 4 else 4


COMPRESSED_FILES = ("late_cid.npy", "late_scale.npy", "late_codes.u8", "late_codec_centroids.bf16", "late_codec_cutoffs.npy",
                    "late_codec_weights.npy")


def save_compressed_store(out_dir: Union[str, Path], cid, scale, codes, centroid_bits, cutoffs, weights, lims, meta: dict) -> None:
    """Writes ``late.json`` (with ``"nbits"`` and ``"n_centroids"``), ``late_token_lims.npy``, ``late_cid.npy``,
    ``late_scale.npy``, ``late_codes.u8`` (raw bytes) and ``late_codec_{centroids.bf16, cutoffs.npy, weights.npy}``."""
    cen, cut, w, nbits = check_codec(centroid_bits, cutoffs, weights)
    cid = np.ascontiguousarray(cid, dtype=np.int32).reshape(-1)
    scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
    codes = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1, code_bytes(nbits))
    lims = check_lims(lims, n_tokens=cid.size)
    if scale.size != cid.size or codes.shape[0] != cid.size:
        raise ValueError("cid, scale and codes must cover the same tokens")
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "late_token_lims.npy", lims)
    np.save(out / "late_cid.npy", cid)
    np.save(out / "late_scale.npy", scale)
    codes.tofile(out / "late_codes.u8")
    cen.tofile(out / "late_codec_centroids.bf16")
    np.save(out / "late_codec_cutoffs.npy", cut)
    np.save(out / "late_codec_weights.npy", w)
    with open(out / "late.json", "w") as f:
        json.dump({**meta, "ntotal": int(lims.size - 1), "n_tokens": int(cid.size), "dim": DIM, "dtype": "bfloat16",
                   "nbits": nbits, "n_centroids": int(cen.shape[0]), "format_version": FORMAT_VERSION}, f)


def load_compressed_store(index_dir: Union[str, Path]):
    """``(cid, scale, codes, centroid bits, cutoffs, weights, lims, meta)`` as ``save_compressed_store`` wrote them, checked."""
    d = Path(index_dir)
    meta = read_versioned_json(d / "late.json", FORMAT_VERSION)
    nbits = _check_nbits(int(meta.get("nbits", 0)))
    if int(meta.get("dim", -1)) != DIM:
        raise ValueError(f"{d / 'late.json'}: expected {DIM}-d tokens")
    n, C = int(meta["n_tokens"]), int(meta["n_centroids"])
    lims = check_lims(np.load(d / "late_token_lims.npy"), n_rows=int(meta["ntotal"]), n_tokens=n)
    cid = np.load(d / "late_cid.npy", allow_pickle=False)
    scale = np.load(d / "late_scale.npy", allow_pickle=False)
    codes = np.fromfile(d / "late_codes.u8", dtype=np.uint8)
    cen = np.fromfile(d / "late_codec_centroids.bf16", dtype=np.uint16)
    if cid.shape != (n,) or cid.dtype != np.int32 or scale.shape != (n,) or scale.dtype != np.float32:
        raise ValueError(f"{d}: late_cid.npy / late_scale.npy do not hold {n} int32 / fp32 entries")
    if codes.size != n * code_bytes(nbits):
        raise ValueError(f"{d / 'late_codes.u8'}: {codes.size} bytes, late.json says {n * code_bytes(nbits)}")
    if cen.size != C * DIM:
        raise ValueError(f"{d / 'late_codec_centroids.bf16'}: {cen.size * 2} bytes, late.json says {C * TOKEN_BYTES}")
    cen, cut, w, nb = check_codec(cen.reshape(-1, DIM), np.load(d / "late_codec_cutoffs.npy", allow_pickle=False),
                                  np.load(d / "late_codec_weights.npy", allow_pickle=False))
    if nb != nbits:
        raise ValueError(f"{d}: the codec's tables are for {nb} bits, late.json says {nbits}")
    return cid, scale, codes.reshape(-1, code_bytes(nbits)), cen, cut, w, lims, meta


LIST_FILES = ("late_list_lims.npy", "late_list_rows.npy")


def check_centroid_lists(list_lims, list_rows, n_centroids: int, n_rows: int, n_tokens: int):
    """Centroid lists as ``(int64 [C + 1], int32 [n_list])``; raises ``ValueError`` unless the bounds start at 0, ascend
    and end at the number of listed rows, there are at most ``n_tokens`` of those, every row lies in ``[0, n_rows)`` and
    the rows of a list ascend strictly."""
    lims = np.ascontiguousarray(np.asarray(list_lims)).reshape(-1)
    rows = np.ascontiguousarray(np.asarray(list_rows)).reshape(-1)
    if lims.dtype != np.int64 or rows.dtype != np.int32:
        raise ValueError("centroid lists: expected int64 bounds and int32 rows")
    if lims.size != n_centroids + 1 or lims[0] != 0 or (np.diff(lims) < 0).any() or lims[-1] != rows.size:
        raise ValueError(f"centroid lists: the bounds must ascend from 0 to {rows.size} over {n_centroids} lists")
    if rows.size > n_tokens:
        raise ValueError(f"centroid lists: {rows.size} listed rows for a store of {n_tokens} tokens")
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows):
        raise ValueError(f"centroid lists: rows outside [0, {n_rows})")
    if rows.size > 1:
        inner = np.ones(rows.size, dtype=bool)
        inner[lims[1:-1][lims[1:-1] < rows.size]] = False      # the first row of a list has no predecessor in it
        if (np.diff(rows) <= 0)[inner[1:]].any():
            raise ValueError("centroid lists: the rows of a list must ascend")
    return lims, rows


def save_centroid_lists(out_dir: Union[str, Path], list_lims, list_rows) -> None:
    """``late_list_lims.npy`` and ``late_list_rows.npy`` beside a compressed store, and ``"centroid_lists": true`` in its
    ``late.json``."""
    out = Path(out_dir)
    meta = read_versioned_json(out / "late.json", FORMAT_VERSION)
    np.save(out / "late_list_lims.npy", np.ascontiguousarray(list_lims, dtype=np.int64))
    np.save(out / "late_list_rows.npy", np.ascontiguousarray(list_rows, dtype=np.int32))
    with open(out / "late.json", "w") as f:
        json.dump({**meta, "centroid_lists": True}, f)


def has_centroid_lists(index_dir: Union[str, Path]) -> bool:
    """True when ``late.json`` of ``index_dir`` announces centroid lists."""
    d = Path(index_dir)
    return is_late_dir(d) and bool(read_versioned_json(d / "late.json", FORMAT_VERSION).get("centroid_lists", False))


def load_centroid_lists(index_dir: Union[str, Path]):
    """``(list_lims, list_rows)`` as ``save_centroid_lists`` wrote them, checked against the store's ``late.json``."""
    d = Path(index_dir)
    meta = read_versioned_json(d / "late.json", FORMAT_VERSION)
    return check_centroid_lists(np.load(d / "late_list_lims.npy", allow_pickle=False),
                                np.load(d / "late_list_rows.npy", allow_pickle=False), int(meta["n_centroids"]),
                                int(meta["ntotal"]), int(meta["n_tokens"]))


def stored_nbits(index_dir: Union[str, Path]) -> int:
    """``nbits`` of the store in ``index_dir``: 0 for the bf16 store (and for a directory written before compression)."""
    return int(read_versioned_json(Path(index_dir) / "late.json", FORMAT_VERSION).get("nbits", 0))


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
        self._chunks = {}      # search_tokens_device: token budget -> the batch cut into LateQueries that fit it


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
        # the codec (None: there is none) and the compressed store (None: the store, if any, is the bf16 one)
        self.nbits = 0
        self.centroids: Optional[torch.Tensor] = None    # device bf16 [C, 384]
        self.cutoffs: Optional[torch.Tensor] = None      # device fp32 [2^nbits - 1]
        self.weights: Optional[torch.Tensor] = None      # device fp32 [2^nbits]
        self.cid: Optional[torch.Tensor] = None          # device int32 [n_tokens]
        self.scale: Optional[torch.Tensor] = None        # device fp32 [n_tokens]
        self.codes: Optional[torch.Tensor] = None        # device uint8 [n_tokens, 48 nbits]
        self._quantizer: Optional[FAISSIndexBuilder] = None   # the centroids as fp32 rows, for the exact top-1 assignment
        # centroid lists over the compressed store (None: there are none): list c = the rows owning a token of centroid c
        self.list_lims: Optional[torch.Tensor] = None    # device int64 [C + 1]
        self.list_rows: Optional[torch.Tensor] = None    # device int32 [n_list]
        self._plaid_S: Optional[torch.Tensor] = None
        self._plaid_ws: Optional[torch.Tensor] = None

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
        """Bytes of the store held: the bf16 rows, or the compressed arrays plus the codec."""
        if self.compressed:
            return store_bytes(self.n_tokens, self.nbits) + codec_bytes(self.n_centroids, self.nbits)
        return store_bytes(self.n_tokens)

    @property
    def compressed(self) -> bool:
        """True when the compressed store is the one held (``compress()``, a compressing build, or such a directory)."""
        return self.cid is not None

    @property
    def n_centroids(self) -> int:
        return 0 if self.centroids is None else int(self.centroids.shape[0])

    def _require_store(self) -> None:
        if (self.tokens is None and self.cid is None) or self.ntotal != self.flat.ntotal:
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
            self.cid = self.scale = self.codes = None
            self.list_lims = self.list_rows = None
            self.lims = lims
            self._lims_dev = torch.from_numpy(lims).to(self.device)

    def _install_compressed(self, cid: torch.Tensor, scale: torch.Tensor, codes: torch.Tensor, lims: np.ndarray,
                            rebuild_lists: bool = False) -> None:
        """``rebuild_lists``: the centroid lists, when there were any, are built again over the new store (``add_tokens``,
        ``compact``); otherwise they are dropped with the store they described."""
        had = self.list_lims is not None
        with torch.cuda.device(self.device):
            self.tokens = None
            self.cid, self.scale, self.codes = cid.contiguous(), scale.contiguous(), codes.contiguous()
            self.lims = lims
            self._lims_dev = torch.from_numpy(lims).to(self.device)
            self.list_lims = self.list_rows = None
        if had and rebuild_lists:
            self.build_centroid_lists()

    def set_tokens(self, tokens, lims) -> None:
        """Pre-computed token vectors for rows ``0 .. flat.ntotal - 1``: ``tokens`` ``[T, 384]`` (NumPy fp32, NumPy uint16
        = bf16 bits, or a torch fp32 / bf16 tensor), ``lims`` ``[ntotal + 1]``.  The rows are stored as given (rounded to
        bf16), not normalised again."""
        t = _tokens_to_device(tokens, self.device)
        self._install(t, check_lims(lims, n_rows=self.flat.ntotal, n_tokens=t.shape[0]))

    def add_tokens(self, tokens, lims) -> None:
        """Appends the token vectors of the rows added with ``flat.add`` since: ``lims`` ``[new rows + 1]`` from 0.  With
        a codec installed and no bf16 store held (a compressed store, or none yet) they are compressed on arrival."""
        t = _tokens_to_device(tokens, self.device)
        new = check_lims(lims, n_tokens=t.shape[0])
        if self.ntotal + new.size - 1 > self.flat.ntotal:
            raise ValueError(f"{self.ntotal} + {new.size - 1} rows of tokens for an index of {self.flat.ntotal} rows")
        lims = np.concatenate([self.lims, self.lims[-1] + new[1:]])
        if self.centroids is not None and self.tokens is None:
            # a codec and no bf16 store: the new tokens are compressed on arrival
            with torch.cuda.device(self.device):
                cid, scale, codes = self._compress_tokens(t)
                if self.cid is not None:
                    cid, scale, codes = (torch.cat([a, b]) for a, b in ((self.cid, cid), (self.scale, scale), (self.codes, codes)))
            self._install_compressed(cid, scale, codes, lims, rebuild_lists=True)
            return
        with torch.cuda.device(self.device):
            both = t if self.tokens is None else torch.cat([self.tokens, t])
        self._install(both, lims)

    def build_from_texts(self, student, texts: Sequence[str], batch_size: int = 64, compress: Optional[int] = None,
                         train_texts: Optional[int] = None, encode_texts: int = 4096, **codec_args) -> None:
        """Encodes the documents of rows ``0 .. flat.ntotal - 1`` (``student``: a ``StudentModel``; the E5 passage prefix
        is applied as ``encode_documents`` applies it) and installs their tokens.

        ``compress`` = 2 or 4 builds the compressed store without the whole bf16 store ever existing: unless a codec of
        that width is installed, one is trained (``train_codec``'s rule, ``codec_args`` pass through) on the tokens of
        ``train_texts`` texts spread evenly over ``texts`` (default: ``max(1024, len(texts) // 16)``); then the texts are
        encoded and compressed ``encode_texts`` at a time."""
        if len(texts) != self.flat.ntotal:
            raise ValueError(f"{len(texts)} texts for an index of {self.flat.ntotal} rows")
        texts = list(texts)
        encode = lambda part: student.encode_tokens(part, is_query=False, max_tokens=self.max_doc_tokens,  # noqa: E731
                                                    batch_size=batch_size)
        if compress is None:
            tokens, lims = encode(texts)
            self._install(tokens, lims)
            return
        nbits = _check_nbits(compress)
        if self.centroids is None or self.nbits != nbits:
            m = min(len(texts), max(1024, len(texts) // 16) if train_texts is None else int(train_texts))
            if m < 1:
                raise ValueError("build_from_texts(compress=...): no texts to train the codec on")
            sample, _ = encode([texts[(i * len(texts)) // m] for i in range(m)])
            self._set_codec_device(*train_codec_tokens(sample, nbits=nbits, **codec_args))
            del sample
        parts, lims = [], [np.zeros(1, np.int64)]
        for lo in range(0, len(texts), max(1, int(encode_texts))):
            tokens, part_lims = encode(texts[lo: lo + max(1, int(encode_texts))])
            with torch.cuda.device(self.device):
                parts.append(self._compress_tokens(tokens))
            lims.append(lims[-1][-1] + part_lims[1:])
            del tokens
        with torch.cuda.device(self.device):
            cid, scale, codes = (torch.cat([p[i] for p in parts]) for i in range(3))
        self._install_compressed(cid, scale, codes, np.concatenate(lims).astype(np.int64))

    # ------------------------------------------------------------------ the codec and the compressed store
    def _set_codec_device(self, centroids: torch.Tensor, cutoffs: np.ndarray, weights: np.ndarray) -> None:
        """Installs a codec already validated: ``centroids`` device bf16 ``[C, 384]``."""
        if self.cid is not None:
            raise RuntimeError("the compressed store was written with the codec installed: it cannot be replaced")
        self.list_lims = self.list_rows = None
        with torch.cuda.device(self.device):
            self.centroids = centroids.contiguous()
            self.cutoffs = torch.from_numpy(np.ascontiguousarray(cutoffs, dtype=np.float32)).to(self.device)
            self.weights = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float32)).to(self.device)
            self.nbits = 2 if self.weights.numel() == 4 else 4
            self._quantizer = FAISSIndexBuilder(embedding_dim=DIM, index_type="Flat", metric="ip", device=str(self.device))
            self._quantizer.build_from_embeddings(self.centroids.to(torch.float32))     # metric "ip": stored as given

    def set_codec(self, centroids, cutoffs, weights) -> None:
        """A caller's codec (``check_codec`` validates it on the host): ``centroids`` ``[C, 384]``, ``cutoffs``
        ``[L - 1]`` ascending, ``weights`` ``[L]``, ``L`` = 4 (2 bits) or 16 (4 bits)."""
        bits, cut, w, _ = check_codec(centroids, cutoffs, weights)
        self._set_codec_device(_tokens_to_device(bits, self.device), cut, w)

    def train_codec(self, nbits: int = 2, n_centroids: Optional[int] = None, sample_tokens: Optional[int] = None,
                    iterations: int = 10, seed: int = 1234) -> None:
        """Trains a codec on the bf16 store held and installs it (``train_codec_tokens`` has the rule); the same
        inputs give the same codec bits."""
        if self.tokens is None or self.n_tokens < 1:
            raise RuntimeError("train_codec(): needs the bf16 token store (set_tokens / add_tokens / build_from_texts)")
        self._set_codec_device(*train_codec_tokens(self.tokens, nbits=nbits, n_centroids=n_centroids,
                                                   sample_tokens=sample_tokens, iterations=iterations, seed=seed))

    def codec_numpy(self):
        """Host copy of the codec: ``(centroid bf16 bits uint16 [C, 384], cutoffs fp32, weights fp32)``."""
        if self.centroids is None:
            raise RuntimeError("no codec is installed: call train_codec / set_codec (or load a compressed store)")
        return (self.centroids.view(torch.int16).cpu().numpy().view(np.uint16), self.cutoffs.cpu().numpy(),
                self.weights.cpu().numpy())

    def _compress_tokens(self, tokens: torch.Tensor, batch: int = 1 << 16):
        """``(cid, scale, codes)`` of device bf16 ``tokens`` under the codec installed: the exact top-1 search over the
        centroids in batches (ties to the lower id), then ``sskd_latec_compress``."""
        lib = _native.load()
        if self.centroids is None:
            raise RuntimeError("no codec is installed: call train_codec / set_codec")
        n = int(tokens.shape[0])
        cid = torch.empty(n, dtype=torch.int32, device=self.device)
        scale = torch.empty(n, dtype=torch.float32, device=self.device)
        codes = torch.empty((n, code_bytes(self.nbits)), dtype=torch.uint8, device=self.device)
        for lo in range(0, n, batch):
            part = tokens[lo: lo + batch]
            _, ids = self._quantizer.search_device(part.to(torch.float32), 1, normalize_queries=False)
            assign = ids[:, 0].contiguous()
            _native.check(lib.sskd_latec_compress(
                part.data_ptr(), assign.data_ptr(), part.shape[0], self.centroids.data_ptr(), self.n_centroids,
                self.cutoffs.data_ptr(), self.weights.data_ptr(), self.nbits, cid.data_ptr(), scale.data_ptr(),
                codes.data_ptr(), lo, n, _native.current_stream_ptr(self.device)))
        return cid, scale, codes

    def compress(self) -> None:
        """Compresses the bf16 store under the codec installed and frees it."""
        if self.tokens is None:
            raise RuntimeError("compress(): there is no bf16 token store" + (" (it is compressed already)" if self.compressed else ""))
        with torch.cuda.device(self.device):
            cid, scale, codes = self._compress_tokens(self.tokens)
        self._install_compressed(cid, scale, codes, self.lims)

    def set_compressed(self, cid, scale, codes, lims) -> None:
        """A compressed store computed elsewhere under the codec installed, for rows ``0 .. flat.ntotal - 1``: ``cid``
        int32 ``[T]``, ``scale`` fp32 ``[T]``, ``codes`` uint8 ``[T, 48 nbits]`` (NumPy), ``lims`` ``[ntotal + 1]``.  Stored
        as given: the kernel clamps a centroid id outside ``[0, C)``."""
        if self.centroids is None:
            raise RuntimeError("no codec is installed: call train_codec / set_codec")
        cid = np.ascontiguousarray(cid, dtype=np.int32).reshape(-1)
        scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(-1)
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        if scale.shape != cid.shape or codes.shape != (cid.size, code_bytes(self.nbits)):
            raise ValueError(f"expected cid [T], scale [T] and codes [T, {code_bytes(self.nbits)}]")
        lims = check_lims(lims, n_rows=self.flat.ntotal, n_tokens=cid.size)
        with torch.cuda.device(self.device):
            self._install_compressed(*(torch.from_numpy(a).to(self.device) for a in (cid, scale, codes)), lims)

    def compressed_numpy(self):
        """Host copies ``(cid int32 [n], scale fp32 [n], codes uint8 [n, 48 nbits])`` of the compressed store."""
        if not self.compressed:
            raise RuntimeError("the store is not compressed")
        return self.cid.cpu().numpy(), self.scale.cpu().numpy(), self.codes.cpu().numpy()

    def decoded_numpy(self):
        """For checking: ``(dec bf16 bits uint16 [n_tokens, 384], scale fp32 [n_tokens])``, the values the compressed
        re-rank multiplies (``dec = bf16(centroid + weights[code])``, a centroid id clamped into ``[0, C)``)."""
        if not self.compressed:
            raise RuntimeError("the store is not compressed")
        nbits, per = self.nbits, 8 // self.nbits
        with torch.cuda.device(self.device):
            packed = self.codes.to(torch.int32)
            by_pos = torch.empty((packed.shape[0], DIM), dtype=torch.int64, device=self.device)
            for i in range(per):
                by_pos[:, i::per] = (packed >> (nbits * i)) & ((1 << nbits) - 1)
            d = torch.arange(DIM, device=self.device)
            code = by_pos[:, 192 * ((d // 8) % 2) + 8 * (d // 16) + d % 8]
            cen = self.centroids[self.cid.to(torch.int64).clamp(0, self.n_centroids - 1)].to(torch.float32)
            dec = (cen + self.weights[code]).to(torch.bfloat16)
            return dec.view(torch.int16).cpu().numpy().view(np.uint16), self.scale.cpu().numpy()

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
        if raw is None:   # (the two stores ask for the same workspace: the raw scores)
            self._workspace = ws = _native.grown(self._workspace, int(lib.sskd_late_rerank_workspace_bytes(nq, R)), self.device)
        if self.compressed:
            call = lib.sskd_latec_rerank
            store = (self.cid.data_ptr(), self.scale.data_ptr(), self.codes.data_ptr(), self.nbits, self.centroids.data_ptr(),
                     self.n_centroids, self.weights.data_ptr())
        else:
            call, store = lib.sskd_late_rerank, (self.tokens.data_ptr(),)
        _native.check(call(
            queries.tokens.data_ptr(), queries.lims_host.ctypes.data, queries.lims_dev.data_ptr(), nq, *store,
            self._lims_dev.data_ptr(), self.ntotal, self.n_tokens, cand.data_ptr(), R, k, self.flat.id_offset, D.data_ptr(),
            I.data_ptr(), None if raw is None else raw.data_ptr(), None if ws is None else ws.data_ptr(),
            0 if ws is None else ws.numel(), _native.current_stream_ptr(self.device)))
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
        needs ``query_texts``), and they are re-ranked to ``k``.  Device tensors ``(D, I)``.

        ``first_stage="centroids"`` takes the candidates from the store's own centroid lists instead
        (``search_tokens_device`` with ``ndocs=candidates``; ``nprobe`` and ``allow`` pass through, ``q_emb`` is unused)."""
        if isinstance(first_stage, str):
            if first_stage != "centroids":
                raise ValueError(f"first_stage={first_stage!r}: the only first stage with a name is 'centroids'")
            return self.search_tokens_device(q_tokens, q_lims, k, ndocs=candidates, **first_stage_kw)
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
            by_lists = isinstance(first_stage, str)      # "centroids": the pooled embeddings are not used
            qd = q_emb if by_lists or isinstance(q_emb, torch.Tensor) else _host_queries_to_device(q_emb, self.device)
            D, I = self.search_device(qd, q_tokens, q_lims, k, candidates=candidates, first_stage=first_stage,
                                      **first_stage_kw)
            return D.cpu().numpy(), I.cpu().numpy()

    # ------------------------------------------------------------------ candidate generation from the store itself
    @property
    def has_centroid_lists(self) -> bool:
        return self.list_lims is not None

    def build_centroid_lists(self) -> None:
        """Builds the centroid lists of the compressed store on the device: list ``c`` holds, ascending and once each,
        the rows that own a token whose centroid id (clamped into ``[0, C)``) is ``c``.  Deterministic: the same store
        gives the same bits.  ``add_tokens`` and ``compact`` rebuild them, ``set_compressed`` and ``set_codec`` drop them."""
        if not self.compressed:
            raise RuntimeError("build_centroid_lists(): centroid lists index a compressed store - call compress() first "
                               "(or build / load a compressed store)")
        C, n = self.n_centroids, self.ntotal
        with torch.cuda.device(self.device):
            counts = torch.from_numpy(np.diff(self.lims)).to(self.device)
            row_of = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=self.device), counts)
            pairs = torch.unique(self.cid.to(torch.int64).clamp(0, C - 1) * max(n, 1) + row_of)      # sorted, distinct
            per_list = torch.bincount(pairs // max(n, 1), minlength=C)
            self.list_lims = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(per_list, 0)]).contiguous()
            self.list_rows = (pairs % max(n, 1)).to(torch.int32).contiguous()

    def centroid_lists_numpy(self):
        """Host copies ``(list_lims int64 [C + 1], list_rows int32)`` of the centroid lists."""
        if not self.has_centroid_lists:
            raise RuntimeError("there are no centroid lists: call build_centroid_lists()")
        return self.list_lims.cpu().numpy(), self.list_rows.cpu().numpy()

    @property
    def centroid_list_bytes(self) -> int:
        return 0 if not self.has_centroid_lists else 8 * int(self.list_lims.numel()) + 4 * int(self.list_rows.numel())

    def _token_chunks(self, queries: LateQueries):
        """``queries`` cut into runs of whole queries whose centroid scores fit ``PLAID_S_BUDGET`` (at least one query
        each).  The cut is made once per ``LateQueries`` and kept on it: the bounds of every run are uploaded here, so a
        later call with the same object enqueues no copy and can be captured into a graph."""
        budget = max(LATE_TQ_MAX, PLAID_S_BUDGET // (4 * max(self.n_centroids, 1)))
        if budget not in queries._chunks:
            lims = queries.lims_host
            if int(lims[-1] - lims[0]) <= budget and lims[0] == 0:
                queries._chunks[budget] = [(0, queries)]
            else:
                parts, a = [], 0
                while a < queries.nq:
                    b = max(a + 1, int(np.searchsorted(lims, lims[a] + budget, side="right")) - 1)
                    sub = np.ascontiguousarray(lims[a: b + 1] - lims[a])
                    parts.append((a, LateQueries(queries.tokens[int(lims[a]): int(lims[b])], sub,
                                                 torch.from_numpy(sub).to(self.device))))
                    a = b
                queries._chunks[budget] = parts
        return queries._chunks[budget]

    def prepare_token_queries(self, q_tokens, q_lims) -> LateQueries:
        """``prepare_queries`` plus the cut ``search_tokens_device`` makes of the batch: what that call takes inside a
        graph capture."""
        queries = self.prepare_queries(q_tokens, q_lims)
        self._token_chunks(queries)
        return queries

    def candidates_device(self, q_tokens, q_lims, nprobe: int = 2, ndocs: int = 256, allow=None, return_scores: bool = False):
        """The first stages alone, for a batch whose centroid scores fit one chunk: ``(cand_I int64 [nq, ndocs], cand_A
        fp32 [nq, ndocs], n_cand int32 [nq])`` on the device (and ``S`` fp32 ``[C, ld]``, a view of a buffer the next call
        overwrites, with ``return_scores``)."""
        lib = _native.load()
        self._require_store()
        if not self.has_centroid_lists:
            raise RuntimeError("there are no centroid lists: call build_centroid_lists() (a compressed store only)")
        queries = self.prepare_queries(q_tokens, q_lims)
        nq, R, nprobe = queries.nq, int(ndocs), int(nprobe)
        C = self.n_centroids
        if not 1 <= nprobe <= min(C, PLAID_NPROBE_MAX):
            raise ValueError(f"nprobe={nprobe} outside [1, min(C={C}, {PLAID_NPROBE_MAX})]")
        if not 1 <= R <= LATE_R_MAX:
            raise ValueError(f"ndocs={R} outside [1, {LATE_R_MAX}]")
        T = int(queries.lims_host[-1])
        ld = max(32, -(-T // 32) * 32)
        mask = self.flat.search_mask(allow)
        stream = _native.current_stream_ptr(self.device)
        self._plaid_S = _native.grown(self._plaid_S, 4 * C * ld, self.device)
        need = int(lib.sskd_plaid_candidates_workspace_bytes(nq, self.ntotal, nprobe))
        self._plaid_ws = _native.grown(self._plaid_ws, need, self.device)
        S, ws = self._plaid_S, self._plaid_ws
        cand_I = torch.empty((nq, R), dtype=torch.int64, device=self.device)
        cand_A = torch.empty((nq, R), dtype=torch.float32, device=self.device)
        n_cand = torch.empty((nq,), dtype=torch.int32, device=self.device)
        _native.check(lib.sskd_plaid_centroid_scores(queries.tokens.data_ptr(), T, self.centroids.data_ptr(), C, S.data_ptr(),
                                                     ld, stream))
        _native.check(lib.sskd_plaid_candidates(
            S.data_ptr(), ld, queries.lims_host.ctypes.data, queries.lims_dev.data_ptr(), nq, C, self.cid.data_ptr(),
            self._lims_dev.data_ptr(), self.ntotal, self.n_tokens, self.list_lims.data_ptr(), self.list_rows.data_ptr(),
            int(self.list_rows.numel()), None if mask is None else mask.data_ptr(), nprobe, R, self.flat.id_offset,
            cand_I.data_ptr(), cand_A.data_ptr(), n_cand.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        if return_scores:
            return cand_I, cand_A, n_cand, S[: 4 * C * ld].view(torch.float32).view(C, ld)
        return cand_I, cand_A, n_cand

    def search_tokens_device(self, q_tokens, q_lims, k: int, nprobe: int = 2, ndocs: int = 256, allow=None,
                             return_candidates: bool = False):
        """Retrieval from the token store alone: the centroid scores of every query token, ``nprobe`` lists per token,
        the ``ndocs`` best rows by centroid interaction (``candidates_device``), then ``rerank_device`` to ``k``.  Device
        tensors ``(D, I)``; ``return_candidates`` adds ``(cand_I, cand_A, n_cand)``.  ``allow`` takes what ``flat.search``
        takes; removed rows are hidden through the flat index's mask.  Queries run in chunks whose centroid scores stay
        under ``PLAID_S_BUDGET``.  No host synchronisation once the queries are prepared (``prepare_token_queries``)."""
        queries = self.prepare_queries(q_tokens, q_lims)
        k, ndocs = int(k), int(ndocs)
        if not 1 <= k <= ndocs:
            raise ValueError(f"k={k} outside [1, ndocs={ndocs}]")
        if allow is not None:
            allow = self.flat.row_filter(allow)         # prepared once, not per chunk
        outs = []
        for _, part in self._token_chunks(queries):
            cand = self.candidates_device(part, None, nprobe=nprobe, ndocs=ndocs, allow=allow)
            outs.append(self.rerank_device(part, None, cand[0], k) + (cand if return_candidates else ()))
        return outs[0] if len(outs) == 1 else tuple(torch.cat([o[i] for o in outs]) for i in range(len(outs[0])))

    def search_tokens(self, q_tokens, q_lims, k: int = 10, nprobe: int = 2, ndocs: int = 256, allow=None,
                      return_candidates: bool = False):
        """``search_tokens_device`` returning NumPy."""
        with torch.cuda.device(self.device):
            out = self.search_tokens_device(q_tokens, q_lims, k, nprobe=nprobe, ndocs=ndocs, allow=allow,
                                            return_candidates=return_candidates)
            return tuple(o.cpu().numpy() for o in out)

    def exhaustive_tokens(self, q_tokens, q_lims, k: int, rows_per_call: int = LATE_R_MAX) -> Tuple[np.ndarray, np.ndarray]:
        """The exact MaxSim top-``k`` over ALL rows, for checking: every row goes through ``rerank_device(return_raw=True)``
        in runs of at most 1 024 candidates, and the raw scores are ordered on the host (score descending, lower id)."""
        queries = self.prepare_queries(q_tokens, q_lims)
        n, nq = self.ntotal, queries.nq
        step = max(1, min(int(rows_per_call), LATE_R_MAX))
        raw = np.full((nq, n), -np.inf, dtype=np.float32)
        with torch.cuda.device(self.device):
            for lo in range(0, n, step):
                hi = min(n, lo + step)
                ids = torch.arange(lo, hi, dtype=torch.int64, device=self.device) + self.flat.id_offset
                raw[:, lo:hi] = self.rerank_device(queries, None, ids.repeat(nq, 1), 1, return_raw=True)[2].cpu().numpy()
        order = np.argsort(-raw, axis=1, kind="stable")[:, :k]
        D = np.take_along_axis(raw, order, axis=1)
        I = np.where(D > -np.inf, order + self.flat.id_offset, -1)
        if D.shape[1] < k:
            D = np.concatenate([D, np.full((nq, k - D.shape[1]), -np.inf, np.float32)], axis=1)
            I = np.concatenate([I, np.full((nq, k - I.shape[1]), -1, np.int64)], axis=1)
        return D, I.astype(np.int64)

    def validate_tokens(self, q_tokens, q_lims, k: int = 10, nprobe: int = 2, ndocs: int = 256) -> float:
        """Recall@``k`` of ``search_tokens`` against the exhaustive MaxSim over all rows (``exhaustive_tokens``): the
        share of the exhaustive top-``k`` that the search returns, averaged over the queries."""
        queries = self.prepare_queries(q_tokens, q_lims)
        _, got = self.search_tokens(queries, None, k, nprobe=nprobe, ndocs=ndocs)
        _, want = self.exhaustive_tokens(queries, None, k)
        hits = total = 0
        for g, w in zip(got, want):
            w = w[w >= 0]
            hits += int(np.isin(w, g).sum())
            total += int(w.size)
        return hits / max(total, 1)

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
            pick = torch.from_numpy(take).to(self.device)
            if self.compressed:
                self._install_compressed(self.cid[pick], self.scale[pick], self.codes[pick], lims, rebuild_lists=True)
                return
            tokens = self.tokens[pick].contiguous()
        self._install(tokens, lims)

    def save(self, output_dir: Union[str, Path]) -> None:
        """``late.json``, ``late_token_lims.npy`` and ``late_tokens.bf16`` beside the index's own files (which the
        index's ``save`` writes)."""
        meta = {"max_doc_tokens": self.max_doc_tokens, "max_query_tokens": self.max_query_tokens}
        if self.compressed:
            # the compressed store: late_cid.npy, late_scale.npy, late_codes.u8 and the codec's three files instead
            save_compressed_store(output_dir, *self.compressed_numpy(), *self.codec_numpy(), self.lims, meta)
            if self.has_centroid_lists:
                save_centroid_lists(output_dir, *self.centroid_lists_numpy())
            return
        if self.tokens is None:
            raise RuntimeError("save(): the token store is empty")
        save_store(output_dir, self.tokens_numpy(), self.lims, meta)

    def load(self, index_dir: Union[str, Path]) -> None:
        """The store of ``index_dir`` over the rows ``self.flat`` already holds; a store over another number of rows
        raises ``ValueError``.  Whichever store the directory holds is loaded: bf16 rows, or the compressed arrays
        with their codec (``"nbits"`` in ``late.json``)."""
        if stored_nbits(index_dir):
            cid, scale, codes, cen, cut, w, lims, meta = load_compressed_store(index_dir)
            if lims.size - 1 != self.flat.ntotal:
                raise ValueError(f"{index_dir}: a token store over {lims.size - 1} rows, the index holds {self.flat.ntotal}")
            self.max_doc_tokens = int(meta.get("max_doc_tokens", self.max_doc_tokens))
            self.max_query_tokens = int(meta.get("max_query_tokens", self.max_query_tokens))
            self.cid = None
            self._set_codec_device(_tokens_to_device(cen, self.device), cut, w)
            with torch.cuda.device(self.device):
                self._install_compressed(*(torch.from_numpy(a).to(self.device) for a in (cid, scale, codes)), lims)
                if meta.get("centroid_lists", False):
                    list_lims, list_rows = load_centroid_lists(index_dir)
                    self.list_lims = torch.from_numpy(list_lims).to(self.device)
                    self.list_rows = torch.from_numpy(list_rows).to(self.device)
            return
        bits, lims, meta = load_store(index_dir)
        if lims.size - 1 != self.flat.ntotal:
            raise ValueError(f"{index_dir}: a token store over {lims.size - 1} rows, the index holds {self.flat.ntotal}")
        self.max_doc_tokens = int(meta.get("max_doc_tokens", self.max_doc_tokens))
        self.max_query_tokens = int(meta.get("max_query_tokens", self.max_query_tokens))
        self._install(_tokens_to_device(bits, self.device), lims)

    def cleanup(self) -> None:
        self.tokens = self._lims_dev = self._workspace = None
        self.list_lims = self.list_rows = self._plaid_S = self._plaid_ws = None
        self.cid = self.scale = self.codes = self.centroids = self.cutoffs = self.weights = None
        if self._quantizer is not None:
            self._quantizer.cleanup()
        self._quantizer = None
        self.nbits = 0
        self.lims = np.zeros(1, dtype=np.int64)


def _sorted_quantiles(sorted_values: torch.Tensor, fractions) -> np.ndarray:
    """Quantiles of an ascending device fp32 vector by linear interpolation between neighbours, in fp64, as fp32."""
    n = int(sorted_values.numel())
    pos = np.asarray(fractions, dtype=np.float64) * (n - 1)
    lo = np.floor(pos).astype(np.int64)
    hi = np.minimum(lo + 1, n - 1)
    both = sorted_values[torch.from_numpy(np.concatenate([lo, hi])).to(sorted_values.device)].cpu().numpy().astype(np.float64)
    a, b = both[: lo.size], both[lo.size:]
    return (a + (b - a) * (pos - lo)).astype(np.float32)


def train_codec_tokens(tokens: torch.Tensor, nbits: int = 2, n_centroids: Optional[int] = None,
                       sample_tokens: Optional[int] = None, iterations: int = 10, seed: int = 1234,
                       residual_rows: int = 1 << 15):
    """A codec from device bf16 ``tokens`` ``[n, 384]``: ``(centroids device bf16 [C, 384], cutoffs fp32 [L - 1],
    weights fp32 [L])``, deterministic.

    The sample is ``sample_tokens`` rows spread evenly over ``tokens`` (default ``min(n, 256 C)``).  It is widened into a
    temporary flat index and ``IVFIndex.train`` runs its spherical k-means on it (its seeding, its update, ``iterations``
    of it); the centroids are rounded to bf16 and the sample is assigned again, against the rounded centroids.  ``cutoffs``
    and ``weights`` are the ``i / L`` and ``(i + 1/2) / L`` quantiles (ColBERTv2's rule) of the residuals
    ``fp32(t) - fp32(c)`` of at most ``residual_rows`` sample rows, again spread evenly.  ``C`` defaults to
    ``default_n_centroids``: the largest power of two ``<= 16 sqrt(n)``, at most 65 536 and at most the sample size."""
    from .ivf import IVFIndex

    nbits = _check_nbits(nbits)
    n = int(tokens.shape[0])
    if n < 1:
        raise ValueError("train_codec: no tokens")
    if sample_tokens is not None and not 1 <= int(sample_tokens) <= n:
        raise ValueError(f"sample_tokens={sample_tokens} outside [1, {n}]")
    C = default_n_centroids(n, sample_tokens) if n_centroids is None else int(n_centroids)
    m = min(n, 256 * C) if sample_tokens is None else int(sample_tokens)
    if not 1 <= C <= min(LATE_C_MAX, m):
        raise ValueError(f"n_centroids={C} outside [1, min({LATE_C_MAX}, sample of {m})]")
    device = tokens.device
    L = 1 << nbits
    with torch.cuda.device(device):
        pick = torch.from_numpy((np.arange(m, dtype=np.int64) * n) // m).to(device)
        sample = tokens[pick].to(torch.float32)
        flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="Flat", metric="ip", device=str(device))
        flat.build_from_embeddings(sample)
        ivf = IVFIndex(flat=flat)
        ivf.train(nlist=C, iterations=iterations, seed=seed, max_train_rows=m)
        centroids = torch.from_numpy(ivf.centroids_numpy()).to(device).to(torch.bfloat16).contiguous()
        keep = torch.from_numpy((np.arange(min(m, residual_rows), dtype=np.int64) * m) // min(m, residual_rows)).to(device)
        rows = sample[keep]
        ivf._set_centroids(centroids.to(torch.float32))
        assign = ivf._assign_device(rows)
        residual = (rows - centroids.to(torch.float32)[assign]).reshape(-1)
        ordered = torch.sort(residual).values
        cutoffs = _sorted_quantiles(ordered, np.arange(1, L) / L)
        weights = _sorted_quantiles(ordered, (np.arange(L) + 0.5) / L)
        ivf.cleanup()
    return centroids, cutoffs, weights


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
