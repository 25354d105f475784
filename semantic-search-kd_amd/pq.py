"""``IVFPQIndex``: product-quantisation codes over the inverted lists, ADC list scan, exact re-ranking.

The PQ half of the reference's ``ivf_pq`` index type (``configs/index.yaml``: ``m: 64``, ``nbits: 8``) on top of
``IVFIndex``.  The codes decide WHICH rows of the probed lists get re-scored - 64 bytes per (row, query) through the
lists instead of 1 536 - and every score and order of the default result is still the exact scan's fp32 fma chain:

* ``search(q, k, refine=R)`` returns bit for bit what ``flat.search(q, k, allow=<the R candidates of q>)`` returns; the
  candidates are the ``R`` best probed rows by ADC score (asymmetric distance computation: query against codes).
  ``refine=0`` returns the top-``k`` by ADC with the ADC scores (the groundwork of a codes-only index).
* Rows are encoded by residual (row - centroid of its list), so ``<q, row> ~ <q, c_list> + sum_j lut[j][code_j]``: the
  look-up table does not depend on the list and the first term is the probe's own score.
* The arithmetic of every step (``include/sskd_amd.h``, "IVF-PQ") is sequential IEEE fp32 / fp64, so NumPy restates it
  bit for bit (``tests/pq_cases.py``).  Training is a k-means per subspace on the device, deterministic.
* ``codes_by_row`` (device uint8 ``[ntotal, m]``) is the master copy; ``codes_csr`` holds the same codes in the order of
  ``list_rows`` - a list is one contiguous byte range - and is re-derived by one gather whenever the lists change.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native
from .index import FAISSIndexBuilder, _host_queries_to_device
from .ivf import IVF_K_MAX, IVF_NLIST_MAX, IVFIndex, csr_from_assignment, load_lists
from .overlay import read_versioned_json

PQ_DIM = 384
PQ_NBITS = 8
PQ_CODES = 256
PQ_M_ALLOWED = (8, 16, 24, 32, 48, 64, 96)
PQ_REFINE_MAX = 256
PQ_MAX_BATCH = 4096            # queries per sskd_pq_search call: the LUT workspace is 1 KiB * m per query
PQ_MAX_TRAIN_ROWS = 65536
PQ_FORMAT_VERSION = 1


# ------------------------------------------------------------------ host side (NumPy, no GPU)
def check_m(m: int) -> int:
    if int(m) not in PQ_M_ALLOWED:
        raise ValueError(f"m={m} is not one of {PQ_M_ALLOWED}")
    return int(m)


def default_refine(k: int) -> int:
    """``min(256, max(100, 4 k))``"""
    return int(min(PQ_REFINE_MAX, max(100, 4 * int(k))))


def check_refine(k: int, refine: Optional[int]) -> int:
    """The ``refine`` a CALLER names for one search: None is ``default_refine(k)``, anything but 0 or ``k .. 256`` is
    refused."""
    r = default_refine(k) if refine is None else int(refine)
    if r != 0 and not int(k) <= r <= PQ_REFINE_MAX:
        raise ValueError(f"refine={r} is neither 0 nor in [k={k}, {PQ_REFINE_MAX}]")
    return r


def stored_refine(k: int, stored: Optional[int]) -> int:
    """The ``refine`` of a search whose caller names none, from the value kept with the index (the constructor's, or
    ``pq.json``'s): None is ``default_refine(k)``, 0 stays raw ADC, and a number is a FLOOR - ``min(256, max(k,
    stored))`` - so that an index tuned at k = 10 still answers any ``k <= 256``."""
    if stored is None:
        return default_refine(k)
    if int(stored) == 0:
        return 0
    return int(min(PQ_REFINE_MAX, max(int(k), int(stored))))


def check_codebooks(codebooks, m: int) -> np.ndarray:
    cb = np.ascontiguousarray(np.asarray(codebooks, dtype=np.float32))
    if cb.shape != (m, PQ_CODES, PQ_DIM // m):
        raise ValueError(f"expected codebooks [{m}, {PQ_CODES}, {PQ_DIM // m}], got {cb.shape}")
    return cb


def save_pq(out_dir: Union[str, Path], codebooks: np.ndarray, codes: np.ndarray, meta: dict) -> None:
    """Writes ``pq_codebooks.npy`` (fp32 ``[m, 256, dsub]``), ``pq_codes.npy`` (uint8 ``[n, m]``, row order) and
    ``pq.json``."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    m = int(np.asarray(codebooks).shape[0])
    cb = check_codebooks(codebooks, check_m(m))
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.ndim != 2 or codes.shape[1] != m:
        raise ValueError(f"expected codes [n, {m}], got {codes.shape}")
    np.save(out / "pq_codebooks.npy", cb)
    np.save(out / "pq_codes.npy", codes)
    with open(out / "pq.json", "w") as f:
        json.dump({**meta, "m": m, "nbits": PQ_NBITS, "format_version": PQ_FORMAT_VERSION}, f)


def load_pq(index_dir: Union[str, Path]):
    """``(codebooks, codes, meta)`` as ``save_pq`` wrote them; shapes and types are checked."""
    d = Path(index_dir)
    meta = read_versioned_json(d / "pq.json", PQ_FORMAT_VERSION)
    if int(meta.get("nbits", -1)) != PQ_NBITS:
        raise ValueError(f"{d / 'pq.json'}: nbits={meta.get('nbits')!r}, this build reads {PQ_NBITS}")
    m = check_m(meta["m"])
    cb = check_codebooks(np.load(d / "pq_codebooks.npy"), m)
    codes = np.load(d / "pq_codes.npy")
    if codes.dtype != np.uint8 or codes.ndim != 2 or codes.shape[1] != m:
        raise ValueError(f"{d}: expected uint8 codes [n, {m}], got {codes.dtype} {codes.shape}")
    return cb, np.ascontiguousarray(codes), meta


def is_pq_dir(index_dir: Union[str, Path]) -> bool:
    return (Path(index_dir) / "pq.json").exists()


# ------------------------------------------------------------------------------------------------ the index
class IVFPQIndex(IVFIndex):
    """``IVFIndex`` plus PQ codes: ``codebooks`` device fp32 ``[m, 256, dsub]``, ``codes_by_row`` / ``codes_csr`` device
    uint8 ``[ntotal, m]``."""

    def __init__(self, flat: Optional[FAISSIndexBuilder] = None, embedding_dim: int = 384, metric: str = "cosine",
                 device: Optional[str] = None, nlist: Optional[int] = None, nprobe: int = 32, m: int = 64,
                 refine: Optional[int] = None, pq_iterations: int = 10) -> None:
        super().__init__(flat=flat, embedding_dim=embedding_dim, metric=metric, device=device, nlist=nlist, nprobe=nprobe)
        if self.embedding_dim != PQ_DIM:
            raise ValueError(f"IVF-PQ is built for dim {PQ_DIM}, the index has {self.embedding_dim}")
        self.m = check_m(m)
        if refine is not None and not 0 <= int(refine) <= PQ_REFINE_MAX:
            raise ValueError(f"refine={refine} outside [0, {PQ_REFINE_MAX}]")
        self.refine = None if refine is None else int(refine)   # see stored_refine: None = the default, a number = a floor
        self.pq_iterations = int(pq_iterations)
        self.pq_seed = 1235
        self.codebooks: Optional[torch.Tensor] = None
        self.codes_by_row: Optional[torch.Tensor] = None
        self.codes_csr: Optional[torch.Tensor] = None
        self._pq_workspace: Optional[torch.Tensor] = None

    @property
    def dsub(self) -> int:
        return PQ_DIM // self.m

    def _centroid_rows(self) -> torch.Tensor:
        return self.quantizer._tiled[: self.nlist * PQ_DIM].view(self.nlist, PQ_DIM)

    def _require_pq(self) -> None:
        self._require_lists()
        n = self.flat.ntotal
        if (self.codebooks is None or self.codes_by_row is None or self.codes_csr is None
                or self.codes_by_row.shape[0] != n or self.codes_csr.shape[0] != n):
            raise RuntimeError("the PQ codes are not built for the rows held: call train() (or build_from_embeddings / load)")

    def codebooks_numpy(self) -> np.ndarray:
        return self.codebooks.cpu().numpy()

    def codes_numpy(self) -> np.ndarray:
        """Host copy of the codes in row order."""
        return self.codes_by_row.cpu().numpy()

    # ------------------------------------------------------------------ codes
    def _derive_csr(self) -> None:
        """``codes_csr`` = ``codes_by_row`` in ``list_rows`` order (one gather); skipped while the two disagree in size,
        as in the middle of ``add`` / ``compact``."""
        if self.codes_by_row is None or self.list_rows is None or self.codes_by_row.shape[0] != self.list_rows.numel():
            self.codes_csr = None
            return
        self.codes_csr = self.codes_by_row[self.list_rows.to(torch.int64)].contiguous()

    def _install(self, assign: torch.Tensor) -> None:
        super()._install(assign)
        self._derive_csr()

    def _from_host(self, centroids: np.ndarray, offsets: np.ndarray, rows: np.ndarray) -> None:
        super()._from_host(centroids, offsets, rows)
        self._derive_csr()

    def encode_device(self, rows: torch.Tensor, assign: Optional[torch.Tensor], codebooks: Optional[torch.Tensor] = None
                      ) -> torch.Tensor:
        """``sskd_pq_encode``: codes uint8 ``[n, m]`` of device fp32 ``rows`` ``[n, 384]``; ``assign`` (device int64
        ``[n]``) = the list of every row, whose centroid is subtracted first (None: the rows are encoded as given)."""
        lib = _native.load()
        cb = self.codebooks if codebooks is None else codebooks
        rows = rows.contiguous()
        n = rows.shape[0]
        codes = torch.empty((n, self.m), dtype=torch.uint8, device=self.device)
        if assign is not None:
            assign = assign.contiguous()
        _native.check(lib.sskd_pq_encode(
            rows.data_ptr() if n else None, n, self.quantizer._tiled.data_ptr() if assign is not None else None,
            None if assign is None else assign.data_ptr(), self.nlist if assign is not None else 0, cb.data_ptr(), self.m,
            codes.data_ptr() if n else None, _native.current_stream_ptr(self.device)))
        return codes

    def code_sums_device(self, rows: torch.Tensor, assign: Optional[torch.Tensor], codes: torch.Tensor
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
        """``sskd_pq_code_sums``: fp64 sums ``[m, 256, dsub]`` of the residuals grouped by code, and the int64 counts
        ``[m, 256]``.  The grouping is a stable sort per subspace (plumbing), so rows ascend within a code."""
        lib = _native.load()
        n, m = codes.shape
        by_sub = codes.t().contiguous().to(torch.int16)                                     # [m, n]
        order = torch.sort(by_sub, dim=1, stable=True).indices.to(torch.int32).contiguous()
        flat_codes = (by_sub.to(torch.int64) + PQ_CODES * torch.arange(m, device=self.device)[:, None]).view(-1)
        counts = torch.bincount(flat_codes, minlength=m * PQ_CODES).view(m, PQ_CODES)
        offsets = torch.zeros((m, PQ_CODES + 1), dtype=torch.int64, device=self.device)
        torch.cumsum(counts, 1, out=offsets[:, 1:])
        sums = torch.empty((m, PQ_CODES, self.dsub), dtype=torch.float64, device=self.device)
        out_counts = torch.empty((m, PQ_CODES), dtype=torch.int64, device=self.device)
        rows = rows.contiguous()
        _native.check(lib.sskd_pq_code_sums(
            rows.data_ptr() if n else None, n, self.quantizer._tiled.data_ptr() if assign is not None else None,
            None if assign is None else assign.contiguous().data_ptr(), self.nlist if assign is not None else 0,
            offsets.data_ptr(), order.data_ptr() if n else None, m, sums.data_ptr(), out_counts.data_ptr(),
            _native.current_stream_ptr(self.device)))
        return sums, out_counts

    def train_pq(self, seed: int = 1234, pq_iterations: Optional[int] = None) -> None:
        """k-means per subspace on the residuals of ``min(ntotal, 65 536)`` rows spread evenly, deterministic.  The
        first codebook entries are the residuals of the sample rows ``sorted(default_rng(seed + 1).permutation(n_train)
        [:256])``; an iteration encodes the sample, sums every code's residuals in ascending row order in fp64 and sets
        the entry to ``fl32(sum / count)``; an empty code keeps its entry.  Then ALL rows are encoded."""
        self._require_lists()
        n = self.flat.ntotal
        if n < PQ_CODES:
            raise ValueError(f"PQ training needs at least {PQ_CODES} rows, the index holds {n}")
        its = self.pq_iterations if pq_iterations is None else int(pq_iterations)
        if its < 0:
            raise ValueError(f"pq_iterations={its} < 0")
        n_train = min(n, PQ_MAX_TRAIN_ROWS)
        with torch.cuda.device(self.device):
            rows = self._rows_view()
            if n_train == n:
                sample, assign = rows, self._assign
            else:
                pick = torch.from_numpy((np.arange(n_train, dtype=np.int64) * n) // n_train).to(self.device)
                sample, assign = rows[pick], self._assign[pick]
            first = np.sort(np.random.default_rng(seed + 1).permutation(n_train)[:PQ_CODES])
            first = torch.from_numpy(first).to(self.device)
            resid = sample[first] - self._centroid_rows()[assign[first]]       # one fp32 subtraction per element
            cb = resid.view(PQ_CODES, self.m, self.dsub).permute(1, 0, 2).contiguous()
            for _ in range(its):
                codes = self.encode_device(sample, assign, cb)
                sums, counts = self.code_sums_device(sample, assign, codes)
                new = (sums / counts.clamp(min=1).to(torch.float64)[:, :, None]).to(torch.float32)
                cb = torch.where((counts > 0)[:, :, None], new, cb).contiguous()
            self.codebooks = cb
            self.codes_by_row = self.encode_device(rows, self._assign)
            self._derive_csr()
        self.pq_seed, self.pq_iterations = int(seed), its

    def train(self, nlist: Optional[int] = None, iterations: int = 10, seed: int = 1234,
              max_train_rows: Optional[int] = None, pq_iterations: Optional[int] = None) -> None:
        """The IVF train, then ``train_pq`` on the residuals, then every row is encoded."""
        if self.flat.ntotal < PQ_CODES:
            raise ValueError(f"PQ training needs at least {PQ_CODES} rows, the index holds {self.flat.ntotal}")
        self.codebooks = self.codes_by_row = self.codes_csr = None
        super().train(nlist=nlist, iterations=iterations, seed=seed, max_train_rows=max_train_rows)
        self.train_pq(seed=seed, pq_iterations=pq_iterations)

    @classmethod
    def from_codebooks(cls, flat: FAISSIndexBuilder, centroids, assignment, codebooks, codes=None, nprobe: int = 32,
                       refine: Optional[int] = None) -> "IVFPQIndex":
        """Lists and codebooks from a caller's arrays (externally trained quantisers): ``centroids`` / ``assignment``
        as ``IVFIndex.from_assignment`` takes them, ``codebooks`` fp32 ``[m, 256, 384 / m]``, ``codes`` uint8 ``[ntotal,
        m]`` in row order (None: the rows are encoded with the codebooks given)."""
        cb = np.asarray(codebooks, dtype=np.float32)
        if cb.ndim != 3:
            raise ValueError(f"expected codebooks [m, {PQ_CODES}, 384 / m], got {cb.shape}")
        index = cls(flat=flat, nprobe=nprobe, m=check_m(cb.shape[0]), refine=refine)
        cb = check_codebooks(cb, index.m)
        c = np.ascontiguousarray(np.asarray(centroids, dtype=np.float32))
        if c.ndim != 2 or c.shape[1] != flat.embedding_dim or not 1 <= c.shape[0] <= IVF_NLIST_MAX:
            raise ValueError(f"expected [1 .. {IVF_NLIST_MAX}, {flat.embedding_dim}] centroids, got {c.shape}")
        a = np.asarray(assignment).reshape(-1)
        if a.size != flat.ntotal:
            raise ValueError(f"{a.size} assignments for {flat.ntotal} rows")
        offsets, rows = csr_from_assignment(a, c.shape[0])
        index._from_host(c, offsets, rows)
        index._set_codes(cb, codes)
        return index

    def _set_codes(self, codebooks: np.ndarray, codes) -> None:
        with torch.cuda.device(self.device):
            self.codebooks = torch.from_numpy(codebooks).to(self.device)
            if codes is None:
                self.codes_by_row = self.encode_device(self._rows_view(), self._assign)
            else:
                c = np.ascontiguousarray(codes)
                if c.dtype != np.uint8 or c.shape != (self.flat.ntotal, self.m):
                    raise ValueError(f"expected uint8 codes [{self.flat.ntotal}, {self.m}], got {c.dtype} {c.shape}")
                self.codes_by_row = torch.from_numpy(c).to(self.device)
            self._derive_csr()

    # ------------------------------------------------------------------ building / mutation
    def add(self, embeddings, groups: Optional[Sequence] = None) -> None:
        """``IVFIndex.add``, then the new rows are encoded with the EXISTING codebooks."""
        self._require_pq()
        first = self.flat.ntotal
        old = self.codes_by_row
        super().add(embeddings, groups=groups)
        if self.flat.ntotal == first:
            return
        with torch.cuda.device(self.device):
            new = self.encode_device(self._rows_view()[first:], self._assign[first:])
            self.codes_by_row = torch.cat([old, new])
            self._derive_csr()

    def compact(self) -> np.ndarray:
        """``IVFIndex.compact``, then the surviving rows' codes (``codes_by_row[kept]``)."""
        self._require_pq()
        old, id_offset = self.codes_by_row, self.flat.id_offset
        kept = super().compact()
        with torch.cuda.device(self.device):
            self.codes_by_row = old[torch.from_numpy(np.asarray(kept, dtype=np.int64) - id_offset).to(self.device)].contiguous()
            self._derive_csr()
        return kept

    # ------------------------------------------------------------------ search
    def search_device(self, queries: torch.Tensor, k: int, *, nprobe: Optional[int] = None, refine: Optional[int] = None,
                      allow=None, normalize_queries: Optional[bool] = None, return_candidates: bool = False):
        """Top-k for device-resident queries: the probe WITH its scores, the LUT, the ADC scan of the probed lists'
        codes and the exact re-scoring of the ``refine`` best (0: the ADC top-k with ADC scores).  Without ``refine``
        the index's own value holds as a floor, ``min(256, max(k, self.refine))``, and when it has none the default
        ``min(256, max(100, 4 k))``.  Device tensors ``(scores [nq, k], ids [nq, k])`` padded with ``(-FLT_MAX, -1)`` - and the
        candidate ids ``[nq, refine]`` with ``return_candidates``.  Everything is enqueued on the current stream with
        no host synchronisation."""
        lib = _native.load()
        self._require_pq()
        k = int(k)
        if k < 1 or k > IVF_K_MAX:
            raise ValueError(f"k={k} outside [1, {IVF_K_MAX}]")
        refine = stored_refine(k, self.refine) if refine is None else check_refine(k, refine)
        if return_candidates and refine == 0:
            raise ValueError("return_candidates needs refine > 0")
        flat = self.flat
        nprobe = self._nprobe(nprobe)
        mask = flat.search_mask(allow)
        q = flat._prepare_queries(queries, normalize_queries, "search_device")
        nq = q.shape[0]
        scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        cand = torch.empty((nq, refine), dtype=torch.int64, device=self.device) if return_candidates else None
        n = flat.ntotal
        stream = _native.current_stream_ptr(self.device)
        for lo in range(0, nq, PQ_MAX_BATCH):
            qb = q[lo: lo + PQ_MAX_BATCH]
            b = qb.shape[0]
            probe_scores, probe = self._probe_scored(qb, nprobe)
            need = int(lib.sskd_pq_search_workspace_bytes(b, nprobe, k, refine, self.m, n, self.max_list_rows))
            self._pq_workspace = _native.grown(self._pq_workspace, need, self.device)
            _native.check(lib.sskd_pq_search(
                flat._tiled.data_ptr(), n, qb.data_ptr(), b, probe.data_ptr(), probe_scores.data_ptr(), nprobe,
                self.list_offsets.data_ptr(), self.list_rows.data_ptr(), self.nlist, self.codes_csr.data_ptr(),
                self.codebooks.data_ptr(), self.m, k, refine, flat.id_offset, None if mask is None else mask.data_ptr(),
                scores[lo: lo + b].data_ptr(), ids[lo: lo + b].data_ptr(),
                None if cand is None else cand[lo: lo + b].data_ptr(), self._pq_workspace.data_ptr(), need, stream))
        return (scores, ids, cand) if return_candidates else (scores, ids)

    def search(self, query_emb: np.ndarray, k: int = 10, *, nprobe: Optional[int] = None, refine: Optional[int] = None,
               allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(distances, indices)`` in ``FAISSIndexBuilder.search``'s form."""
        qd = _host_queries_to_device(query_emb, self.device)
        with torch.cuda.device(self.device):
            scores, ids = self.search_device(qd, k, nprobe=nprobe, refine=refine, allow=allow)
            self.last_search_path = "ivf_pq"
            return scores.cpu().numpy(), ids.cpu().numpy()

    def search_with_candidates(self, query_emb: np.ndarray, k: int = 10, *, nprobe: Optional[int] = None,
                               refine: Optional[int] = None, allow=None):
        """``search`` plus the candidate ids ``[nq, refine]`` (ADC rank order, -1 padded) that were re-scored."""
        qd = _host_queries_to_device(query_emb, self.device)
        with torch.cuda.device(self.device):
            out = self.search_device(qd, k, nprobe=nprobe, refine=refine, allow=allow, return_candidates=True)
            self.last_search_path = "ivf_pq"
            return tuple(t.cpu().numpy() for t in out)

    # ------------------------------------------------------------------ persistence
    def save(self, output_dir: Union[str, Path]) -> None:
        """``IVFIndex.save`` plus ``pq_codebooks.npy``, ``pq_codes.npy`` (row order) and ``pq.json``."""
        self._require_pq()
        super().save(output_dir)
        save_pq(output_dir, self.codebooks_numpy(), self.codes_numpy(),
                {"refine": self.refine, "seed": self.pq_seed, "iterations": self.pq_iterations})

    def load(self, index_dir: Union[str, Path]) -> None:
        self.flat.load(index_dir)
        self.load_lists(index_dir)

    def load_lists(self, index_dir: Union[str, Path]) -> None:
        """The IVF and PQ files of ``index_dir`` over the rows ``self.flat`` already holds.  Everything is read and
        checked before the index changes: a directory that does not fit leaves it as it was."""
        cb, codes, meta = load_pq(index_dir)
        centroids, offsets, rows, ivf_meta = load_lists(index_dir)
        n = self.flat.ntotal
        if codes.shape[0] != n or rows.size != n or centroids.shape[1] != self.embedding_dim:
            raise ValueError(f"{index_dir}: codes of {codes.shape[0]} rows and lists over {rows.size}, the index holds {n}")
        refine = meta.get("refine")
        if refine is not None and not 0 <= int(refine) <= PQ_REFINE_MAX:
            raise ValueError(f"{index_dir}: refine={refine!r} outside [0, {PQ_REFINE_MAX}]")
        self.m = int(meta["m"])
        self.codebooks = self.codes_by_row = self.codes_csr = None
        self._from_host(centroids, offsets, rows)
        self._set_codes(cb, codes)
        self.nprobe = int(ivf_meta.get("nprobe", self.nprobe))
        self.seed = int(ivf_meta.get("seed", self.seed))
        self.iterations = int(ivf_meta.get("iterations", self.iterations))
        self.refine = None if refine is None else int(refine)
        self.pq_seed = int(meta.get("seed", self.pq_seed))
        self.pq_iterations = int(meta.get("iterations", self.pq_iterations))

    def cleanup(self) -> None:
        super().cleanup()
        self.codebooks = self.codes_by_row = self.codes_csr = self._pq_workspace = None
