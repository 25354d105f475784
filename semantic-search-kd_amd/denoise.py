"""Denoising of mined hard negatives: the trigram-set store, the text overlap and the rule's settings.

The reference's curriculum drops a mined passage whose teacher score is ``>= 0.7`` or whose text overlap with a positive
is ``> 0.8`` (configs/kd.yaml ``denoising:``; docs/guides/hyperparameter-tuning.md:107); the overlap is
``compute_text_overlap`` (src/utils/chunk.py:150-182): Jaccard similarity of the character 3-gram sets of the two texts
after ``.lower().strip()``.  Its miners never call it.  Here the sets live in HBM and the rule is one kernel
(``sskd_rank_denoise``, include/sskd_amd.h) between the search and the selection.

**Keys.**  A 3-gram of code points ``c0 c1 c2`` is the uint64 ``(c0 << 42) | (c1 << 21) | c2`` - collision-free because
code points are below 2^21 - and the set of a text is the ascending list of its distinct keys; a text of fewer than
three characters has the empty set.  Keys are stored raw, with no vocabulary: any text becomes a set without reference
to a corpus, ``append`` is a concatenation and nothing needs a global pass.  The price is 8 B per distinct 3-gram
(DESIGN.md 28 has the measured size).

``TrigramStore`` holds the sets of a corpus in CSR (``lims`` int64 ``[n + 1]``, ``keys`` uint64) and uploads them once
per device.  The device entry points trust a store; ``load`` is where a file is validated.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

LIMS_FILE = "trigram_lims.npy"
KEYS_FILE = "trigram_keys.npy"
_BUILD_CHUNK = 1 << 15      # texts per vectorised pass of build_from_texts (bounds the temporaries)


@dataclass(frozen=True)
class Denoising:
    """The reference's ``denoising:`` block.  ``None`` switches a rule off; any other value must be a finite float."""

    text_overlap_threshold: Optional[float] = 0.8
    teacher_score_threshold: Optional[float] = 0.7

    def __post_init__(self):
        for name in ("text_overlap_threshold", "teacher_score_threshold"):
            v = getattr(self, name)
            if v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise TypeError(f"Denoising.{name} must be a float or None, not {type(v).__name__}")
            v = float(v)
            if not math.isfinite(v):
                raise ValueError(f"Denoising.{name}={v} is not finite")
            object.__setattr__(self, name, v)


def _code_points(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """``(code points uint32, lens int64 [n])`` of the lowered, stripped texts, concatenated."""
    norm = [t.lower().strip() for t in texts]
    lens = np.fromiter((len(s) for s in norm), dtype=np.int64, count=len(norm))
    cps = np.frombuffer("".join(norm).encode("utf-32-le", "surrogatepass"), dtype="<u4")
    return cps, lens


_NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)     # pads a row of the sort matrix; no key reaches it (keys are below 2^63)


def _sets_of(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """CSR ``(lims int64 [n + 1], keys uint64)`` of the texts' trigram sets.  The texts become one UTF-32 buffer, the
    windows that do not cross a text boundary become keys, and the rows are sorted side by side: rows of similar length
    (the same power of two of windows) share one padded matrix and one ``sort(axis=1)`` - many short sorts instead of
    one (row, key) sort of the whole block, which took three times as long for the build as a whole."""
    n = len(texts)
    lims = np.zeros(n + 1, np.int64)
    if n == 0:
        return lims, np.zeros(0, np.uint64)
    cps, lens = _code_points(texts)
    starts = np.zeros(n, np.int64)
    np.cumsum(lens[:-1], out=starts[1:])
    n_win = np.maximum(lens - 2, 0)
    total = int(n_win.sum())
    if total == 0:
        return lims, np.zeros(0, np.uint64)
    first_win = np.zeros(n, np.int64)
    np.cumsum(n_win[:-1], out=first_win[1:])
    at = np.arange(total, dtype=np.int64) - np.repeat(first_win - starts, n_win)   # window w of row r starts at cps[at]
    c = cps.astype(np.uint64)
    keys = (c[at] << np.uint64(42)) | (c[at + 1] << np.uint64(21)) | c[at + 2]
    del at, c
    bucket = np.where(n_win > 0, np.ceil(np.log2(np.maximum(n_win, 1))).astype(np.int64), -1)
    bucket_of_window = np.repeat(bucket, n_win)
    sizes = np.zeros(n, np.int64)
    done = []
    for b in np.unique(bucket[bucket >= 0]):
        rows = np.flatnonzero(bucket == b)
        width = int(n_win[rows].max())
        mat = np.full((rows.size, width), _NO_KEY, np.uint64)
        mat[np.arange(width)[None, :] < n_win[rows][:, None]] = keys[bucket_of_window == b]
        mat.sort(axis=1)
        keep = mat != _NO_KEY
        keep[:, 1:] &= mat[:, 1:] != mat[:, :-1]
        sizes[rows] = keep.sum(axis=1)
        done.append((rows, mat[keep]))      # row-major: each row's distinct keys, ascending
    np.cumsum(sizes, out=lims[1:])
    out = np.empty(int(lims[-1]), np.uint64)
    for rows, kept in done:
        count = sizes[rows]
        before = np.cumsum(count) - count
        out[np.arange(kept.size, dtype=np.int64) + np.repeat(lims[rows] - before, count)] = kept
    return lims, out


def trigram_keys(text: str) -> np.ndarray:
    """The ascending uint64 key set of one text."""
    return _sets_of([text])[1]


def text_overlap(text1: str, text2: str) -> float:
    """The reference's ``compute_text_overlap`` (same signature, the same float bit for bit): Jaccard similarity of the
    two texts' character 3-gram sets after ``.lower().strip()``, 0.0 when either set is empty.  The small-input host
    form; a ranking is filtered by ``FAISSIndexBuilder.denoise_ranking_device``."""
    a, b = trigram_keys(text1), trigram_keys(text2)
    if a.size == 0 or b.size == 0:
        return 0.0
    inter = int(np.intersect1d(a, b, assume_unique=True).size)
    return inter / (int(a.size) + int(b.size) - inter)


compute_text_overlap = text_overlap


def _validate(lims: np.ndarray, keys: np.ndarray, what: str) -> None:
    if lims.ndim != 1 or lims.size < 1 or lims.dtype != np.int64:
        raise ValueError(f"{what}: lims must be a 1-d int64 array of n + 1 entries")
    if keys.ndim != 1 or keys.dtype != np.uint64:
        raise ValueError(f"{what}: keys must be a 1-d uint64 array")
    if lims[0] != 0:
        raise ValueError(f"{what}: lims must start at 0")
    if (np.diff(lims) < 0).any():
        raise ValueError(f"{what}: lims must never decrease")
    if int(lims[-1]) != keys.size:
        raise ValueError(f"{what}: lims must end at len(keys)={keys.size}, not {int(lims[-1])}")
    if keys.size > 1:
        bad = keys[1:] <= keys[:-1]
        bad[lims[1:-1][(lims[1:-1] > 0) & (lims[1:-1] < keys.size)] - 1] = False   # a set's first key against the set before
        if bad.any():
            raise ValueError(f"{what}: keys must strictly ascend within a set (key {int(np.flatnonzero(bad)[0]) + 1})")


class TrigramStore:
    """The trigram sets of ``n_sets`` texts, set ``i`` = ``keys[lims[i]:lims[i + 1]]`` ascending without repeats."""

    def __init__(self, lims: Optional[np.ndarray] = None, keys: Optional[np.ndarray] = None):
        self.lims = np.zeros(1, np.int64) if lims is None else lims
        self.keys = np.zeros(0, np.uint64) if keys is None else keys
        self._device = {}

    # ------------------------------------------------------------------ building
    @classmethod
    def build_from_texts(cls, texts: Sequence[str]) -> "TrigramStore":
        """Vectorised (``_sets_of``), one block of 32 768 texts at a time: no Python loop per text beyond ``lower().strip()``."""
        store = cls()
        store.append(texts)
        return store

    def append(self, texts: Sequence[str]) -> "TrigramStore":
        """The sets of ``texts`` as new sets ``n_sets, n_sets + 1, ...`` (the rows an ``add`` of their embeddings gets)."""
        texts = list(texts)
        parts_l, parts_k = [self.lims], [self.keys]
        base = int(self.lims[-1])
        for lo in range(0, len(texts), _BUILD_CHUNK):
            lims, keys = _sets_of(texts[lo : lo + _BUILD_CHUNK])
            parts_l.append(lims[1:] + base)
            parts_k.append(keys)
            base += keys.size
        self.lims = np.concatenate(parts_l)
        self.keys = np.concatenate(parts_k)
        self._device = {}
        return self

    def take(self, kept) -> "TrigramStore":
        """A new store of the sets ``kept`` (LOCAL rows, any order) - after ``kept = index.compact()``,
        ``store.take(kept - index.id_offset)`` is the store of the renumbered index."""
        kept = np.asarray(kept, dtype=np.int64).reshape(-1)
        if kept.size and (kept.min() < 0 or kept.max() >= self.n_sets):
            raise ValueError(f"take(): rows outside [0, {self.n_sets})")
        sizes = self.lims[kept + 1] - self.lims[kept]
        lims = np.zeros(kept.size + 1, np.int64)
        np.cumsum(sizes, out=lims[1:])
        src = np.arange(int(lims[-1]), dtype=np.int64) + np.repeat(self.lims[kept] - lims[:-1], sizes)
        return TrigramStore(lims, np.ascontiguousarray(self.keys[src]))

    # ------------------------------------------------------------------ files
    def save(self, directory) -> None:
        directory = Path(directory)
        directory.mkdir(parents=True, exist_ok=True)
        np.save(directory / LIMS_FILE, self.lims)
        np.save(directory / KEYS_FILE, self.keys)

    @classmethod
    def load(cls, directory) -> "TrigramStore":
        """Refuses files whose ``lims`` is not non-decreasing from 0, does not end at ``len(keys)``, or whose keys do
        not strictly ascend within a set: the kernels trust what is loaded."""
        directory = Path(directory)
        lims = np.load(directory / LIMS_FILE, allow_pickle=False)
        keys = np.load(directory / KEYS_FILE, allow_pickle=False)
        _validate(lims, keys, str(directory))
        return cls(np.ascontiguousarray(lims), np.ascontiguousarray(keys))

    # ------------------------------------------------------------------ reading
    @property
    def n_sets(self) -> int:
        return int(self.lims.size) - 1

    @property
    def nbytes(self) -> int:
        return int(self.lims.nbytes + self.keys.nbytes)

    def keys_of(self, i: int) -> np.ndarray:
        if not 0 <= i < self.n_sets:
            raise IndexError(f"set {i} outside [0, {self.n_sets})")
        return self.keys[self.lims[i] : self.lims[i + 1]]

    def device_arrays(self, device):
        """``(lims int64, keys)`` on ``device``, uploaded on first use.  The keys travel as the int64 view of their bits
        (at least one element, so that an empty store still has an address)."""
        import torch

        device = torch.device(device)
        if device not in self._device:
            keys = self.keys if self.keys.size else np.zeros(1, np.uint64)
            self._device[device] = (torch.from_numpy(self.lims).to(device),
                                    torch.from_numpy(keys.view(np.int64)).to(device))
        return self._device[device]


# ---------------------------------------------------------------------------------------------------------------------
# the device calls
# ---------------------------------------------------------------------------------------------------------------------
def overlap_pairs_device(store: TrigramStore, a, b, device=None):
    """``(inter int32, union int32, jaccard float64)`` device tensors of the set pairs ``(a[i], b[i])`` (device int32):
    ``sskd_overlap_pairs``, stream-ordered, no synchronisation."""
    import torch

    from . import _native

    lib = _native.load()
    device = a.device if device is None else torch.device(device)
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1:
            raise TypeError(f"overlap_pairs_device expects {name} as a 1-d int32 device tensor")
    if a.numel() != b.numel():
        raise ValueError(f"{a.numel()} and {b.numel()} set numbers do not pair up")
    n = a.numel()
    lims, keys = store.device_arrays(device)
    inter = torch.empty(n, dtype=torch.int32, device=device)
    union = torch.empty(n, dtype=torch.int32, device=device)
    jac = torch.empty(n, dtype=torch.float64, device=device)
    a, b = a.contiguous(), b.contiguous()
    with torch.cuda.device(device):
        _native.check(lib.sskd_overlap_pairs(lims.data_ptr(), keys.data_ptr(), store.n_sets, a.data_ptr(), b.data_ptr(), n,
                                             inter.data_ptr(), union.data_ptr(), jac.data_ptr(),
                                             _native.current_stream_ptr(device)))
    return inter, union, jac


def rank_denoise_device(rank_scores, rank_rows, pos_lims, pos_rows, denoising: Denoising,
                        trigrams: Optional[TrigramStore] = None, aux=None, diagnostics: bool = False):
    """``sskd_rank_denoise`` over device tensors (include/sskd_amd.h): ``rank_scores`` float32 / ``rank_rows`` int64
    ``[nq, search_k]`` in the store's set numbers, positives as ``(pos_lims int64 [nq + 1], pos_rows int32)``.  The
    overlap rule is on when ``denoising.text_overlap_threshold`` is set AND ``trigrams`` is given, the teacher rule when
    ``denoising.teacher_score_threshold`` is set AND ``aux`` (float32 ``[nq, search_k]``) is given.  Returns ``(scores,
    rows, aux_out or None, counts)``, and with ``diagnostics`` also ``(overlap float64, reason uint8)`` aligned with the
    input ranks.  Stream-ordered; nothing synchronises."""
    import torch

    from . import _native

    lib = _native.load()
    if not isinstance(denoising, Denoising):
        raise TypeError("denoising must be a Denoising")
    for name, t, dtype, dim in (("rank_scores", rank_scores, torch.float32, 2), ("rank_rows", rank_rows, torch.int64, 2),
                                ("pos_lims", pos_lims, torch.int64, 1), ("pos_rows", pos_rows, torch.int32, 1)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != dim:
            raise TypeError(f"denoise_ranking_device expects {name} as a {dim}-d {dtype} device tensor")
    if rank_scores.shape != rank_rows.shape:
        raise ValueError("rank_scores and rank_rows differ in shape")
    nq, search_k = rank_scores.shape
    if search_k < 1 or search_k > _native.SSKD_K_MAX:
        raise ValueError(f"search_k={search_k} outside [1, {_native.SSKD_K_MAX}]")
    if pos_lims.numel() != nq + 1:
        raise ValueError(f"pos_lims holds {pos_lims.numel()} entries for {nq} queries (needs nq + 1)")
    device = rank_scores.device
    use_overlap = denoising.text_overlap_threshold is not None and trigrams is not None
    use_aux = denoising.teacher_score_threshold is not None and aux is not None
    if use_aux:
        if not isinstance(aux, torch.Tensor) or not aux.is_cuda or aux.dtype != torch.float32 or aux.shape != rank_scores.shape:
            raise TypeError("denoise_ranking_device expects aux as a float32 device tensor shaped like the ranking")
        aux = aux.contiguous()
    rank_scores, rank_rows = rank_scores.contiguous(), rank_rows.contiguous()
    lims, rows = pos_lims.contiguous(), pos_rows.contiguous()
    out_s = torch.empty_like(rank_scores)
    out_i = torch.empty_like(rank_rows)
    out_a = torch.empty_like(rank_scores) if use_aux else None
    counts = torch.empty(nq, dtype=torch.int32, device=device)
    overlap = torch.empty((nq, search_k), dtype=torch.float64, device=device) if diagnostics else None
    reason = torch.empty((nq, search_k), dtype=torch.uint8, device=device) if diagnostics else None
    g_lims, g_keys = trigrams.device_arrays(device) if use_overlap else (None, None)
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(device):
        _native.check(lib.sskd_rank_denoise(
            ptr(g_lims), ptr(g_keys), trigrams.n_sets if use_overlap else 0, rank_scores.data_ptr(), rank_rows.data_ptr(),
            nq, search_k, lims.data_ptr(), rows.data_ptr() if rows.numel() else None, ptr(aux) if use_aux else None,
            denoising.teacher_score_threshold if use_aux else 0.0,
            denoising.text_overlap_threshold if use_overlap else 0.0, out_s.data_ptr(), out_i.data_ptr(), ptr(out_a),
            counts.data_ptr(), ptr(overlap), ptr(reason), _native.current_stream_ptr(device)))
    if diagnostics:
        return out_s, out_i, out_a, counts, overlap, reason
    return out_s, out_i, out_a, counts
