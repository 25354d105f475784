"""Search oracle (CPU) — TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

Two restatements of the reference's exact search, which must agree with each other:

``topk_blas``  the reference idiom verbatim: ``scores = q @ corpus.T`` (scripts/simple_eval.py:25,
               src/kd/eval.py:75) then ``np.argsort(scores)[::-1][:k]`` (src/kd/eval.py:86), made
               deterministic by the build's tie rule (equal scores: lower id first).
``topk_fma``   the same search with each score summed in the gfx950 kernel's fma order
               (plain C, ``oracle/csrc/oracle.c``) — comparable bit for bit with the HIP path.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np

from . import native

NEG_PAD = np.float32(-3.4028234663852886e38)  # faiss CMin<float>::neutral() = lowest()


def l2_normalize_rows(x: np.ndarray) -> np.ndarray:
    """``faiss.normalize_L2`` (configs/index.yaml:30): rows of zero norm are left untouched."""
    out = np.ascontiguousarray(x, dtype=np.float32).copy()
    native.load().oracle_l2_normalize_rows(out, out.shape[0], out.shape[1])
    return out


def scores_blas(q: np.ndarray, c: np.ndarray) -> np.ndarray:
    """``np.matmul(query_embs, corpus_embs.T)`` — scripts/simple_eval.py:25."""
    return np.matmul(np.asarray(q, np.float32), np.asarray(c, np.float32).T)


def scores_fma(q: np.ndarray, c: np.ndarray) -> np.ndarray:
    q = np.ascontiguousarray(q, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    out = np.empty((q.shape[0], c.shape[0]), np.float32)
    native.load().oracle_scores_fma(q, q.shape[0], c, c.shape[0], c.shape[1], out)
    return out


def topk_of_scores(scores: np.ndarray, k: int, id_offset: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Pure-numpy ``argsort(scores)[::-1][:k]`` with the tie rule, padded like faiss (-1 ids)."""
    scores = np.asarray(scores, np.float32)
    nq, n = scores.shape
    out_s = np.full((nq, k), NEG_PAD, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    ids = np.arange(n, dtype=np.int64)
    for i in range(nq):
        s = scores[i]
        valid = ~(np.isnan(s) | np.isneginf(s))
        # lexsort: last key is primary -> descending score, then ascending id
        order = np.lexsort((ids[valid], -s[valid].astype(np.float64)))[:k]
        sel = ids[valid][order]
        out_s[i, : len(sel)] = s[sel]
        out_i[i, : len(sel)] = sel + id_offset
    return out_s, out_i


def topk_blas(q: np.ndarray, c: np.ndarray, k: int, id_offset: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    if c.shape[0] == 0:
        nq = np.asarray(q).shape[0]
        return np.full((nq, k), NEG_PAD, np.float32), np.full((nq, k), -1, np.int64)
    return topk_of_scores(scores_blas(q, c), k, id_offset)


def topk_fma(q: np.ndarray, c: np.ndarray, k: int, id_offset: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    q = np.ascontiguousarray(q, np.float32)
    c = np.ascontiguousarray(c, np.float32).reshape(-1, q.shape[1])
    out_s = np.empty((q.shape[0], k), np.float32)
    out_i = np.empty((q.shape[0], k), np.int64)
    native.load().oracle_search_fma(q, q.shape[0], c, c.shape[0], q.shape[1], k, id_offset, out_s, out_i)
    return out_s, out_i


def topk_merge(scores: np.ndarray, ids: np.ndarray, k_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """Merge per-shard lists ``[n_lists, nq, k_in]`` into ``[nq, k_out]`` (after the all-gather)."""
    scores = np.ascontiguousarray(scores, np.float32)
    ids = np.ascontiguousarray(ids, np.int64)
    n_lists, nq, k_in = scores.shape
    out_s = np.empty((nq, k_out), np.float32)
    out_i = np.empty((nq, k_out), np.int64)
    native.load().oracle_topk_merge(scores, ids, n_lists, nq, k_in, k_out, out_s, out_i)
    return out_s, out_i


def pool_normalize(hidden: np.ndarray, mask: np.ndarray, normalize: bool = True) -> np.ndarray:
    """Masked mean-pool + L2-normalise (sentence-transformers Pooling(mean) + Normalize)."""
    hidden = np.ascontiguousarray(hidden, np.float32)
    mask = np.ascontiguousarray(mask, np.int32)
    B, S, H = hidden.shape
    out = np.empty((B, H), np.float32)
    native.load().oracle_pool_normalize(hidden, mask, B, S, H, int(normalize), out)
    return out


def near_tie_queries(scores_sorted: np.ndarray, gap: float = 2e-6) -> np.ndarray:
    """Queries whose consecutive oracle scores in the top (k+1) are closer than ``gap``.

    fp32 summation order differs between BLAS and the GPU; ranks inside such a gap are
    legitimately interchangeable (SURVEY.md §7 "exact-id parity").
    """
    d = scores_sorted[:, :-1] - scores_sorted[:, 1:]
    return np.where((d < gap).any(axis=1))[0]


def seeded_unit_rows(n: int, dim: int, seed: int) -> np.ndarray:
    """Synthetic corpus / query generator of BASELINE.md §4: N(0,1) rows, L2-normalised."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.standard_normal((n, dim), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32)


# --------------------------------------------------------------------------------------------------
# Screened search: the sidecar and the error band, restated on the CPU (fp64 where it matters).
#
# Sidecar layout (include/sskd_amd.h): ceil(n / 32) bf16 tiles of 24 576 bytes, then a 4 096-byte norm block.
# Tile t, k-step s (0..23), lane l (0..63), element e (0..7) holds row 32 t + (l & 31), column 16 s + 8 (l >> 5) + e
# of bf16(fl32(c - mu)), mu = fl32(colsum * fl32(1 / n)).  Norm block: int32 words 0..2 = the bit patterns of
# max |c|^2, max |c~|^2, max |c~ - fl32(c - mu)|^2, word 3 = the bit pattern of max |c_ij|, floats 64..447 = colsum.
# --------------------------------------------------------------------------------------------------
SIDECAR_TILE_BYTES = 24576
SIDECAR_NORM_BYTES = 4096
SIDECAR_COLSUM_OFF = 64                           # in floats
SCREEN_ACC_SLACK = float(np.float32(1.0e-4))      # the kernel's constant, as the fp32 it is compiled to
SCREEN_ACC_NEEDED = 3 * 384 * 2.0 ** -24 * (1 + 2.0 ** -8) ** 2   # what the source derives it from (6.9e-5)


class Sidecar(NamedTuple):
    tiles: np.ndarray     # fp32 [padded, 384]: the bf16 values, widened exactly
    words: np.ndarray     # fp32 [3]: max |c|^2, max |c~|^2, max |c~ - fl32(c - mu)|^2
    colsum: np.ndarray    # fp32 [384]
    absmax: np.float32    # max |c_ij|


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest even) -> fp32, torch's conversion."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def sidecar_decode(raw_bytes: np.ndarray, n_rows: int) -> Sidecar:
    raw = np.ascontiguousarray(raw_bytes, np.uint8)
    tiles = -(-n_rows // 32)
    assert raw.size == tiles * SIDECAR_TILE_BYTES + SIDECAR_NORM_BYTES, (raw.size, n_rows)
    h = raw[: tiles * SIDECAR_TILE_BYTES].view(np.uint16).reshape(tiles, 24, 2, 32, 8)   # [t][s][l >> 5][l & 31][e]
    h = h.transpose(0, 3, 1, 2, 4).reshape(tiles * 32, 384)                               # [row][16 s + 8 (l >> 5) + e]
    vals = (h.astype(np.uint32) << 16).view(np.float32)
    block = raw[tiles * SIDECAR_TILE_BYTES:]
    f = block.view(np.float32)
    return Sidecar(vals, f[:3].copy(), f[SIDECAR_COLSUM_OFF: SIDECAR_COLSUM_OFF + 384].copy(), f[3])


def sidecar_encode(tiles_f32: np.ndarray, words, colsum: np.ndarray, absmax, n_rows: int) -> np.ndarray:
    """Inverse of ``sidecar_decode`` (values must be bf16-representable): the bytes sskd_index_make_bf16 writes."""
    tiles = -(-n_rows // 32)
    vals = np.zeros((tiles * 32, 384), np.float32)
    vals[: tiles_f32.shape[0]] = tiles_f32
    bits = vals.view(np.uint32)
    assert not (bits & 0xFFFF).any(), "not bf16 values"
    h = (bits >> 16).astype(np.uint16).reshape(tiles, 32, 24, 2, 8).transpose(0, 2, 3, 1, 4)
    block = np.zeros(SIDECAR_NORM_BYTES // 4, np.float32)
    block[:3] = np.asarray(words, np.float32)
    block[3] = np.float32(absmax)
    block[SIDECAR_COLSUM_OFF: SIDECAR_COLSUM_OFF + 384] = colsum
    return np.concatenate([np.ascontiguousarray(h).reshape(-1).view(np.uint8), block.view(np.uint8)])


class SidecarExpected(NamedTuple):
    mu: np.ndarray        # fp32 [384]
    xc: np.ndarray        # fp32 [n, 384] = fl32(c - mu)
    ct: np.ndarray        # fp32 [n, 384] = bf16_rne(xc)
    words: np.ndarray     # fp64 [3]


def row_norm2_max(c: np.ndarray, xc: np.ndarray, ct: np.ndarray, rows=slice(None)) -> np.ndarray:
    """The three maxima over ``rows``, in fp64."""
    c64, xc64, ct64 = (np.asarray(a[rows], np.float64) for a in (c, xc, ct))
    return np.array([(c64 * c64).sum(1).max(), (ct64 * ct64).sum(1).max(), ((ct64 - xc64) ** 2).sum(1).max()])


def sidecar_expected(corpus: np.ndarray, colsum_f32: np.ndarray) -> SidecarExpected:
    c = np.ascontiguousarray(corpus, np.float32)
    inv_n = np.float32(1.0) / np.float32(c.shape[0])
    mu = (np.asarray(colsum_f32, np.float32) * inv_n).astype(np.float32)
    xc = (c - mu[None]).astype(np.float32)
    ct = bf16_round(xc)
    return SidecarExpected(mu, xc, ct, row_norm2_max(c, xc, ct))


def band_terms(queries: np.ndarray, words) -> np.ndarray:
    """fp64 [nq, 3]: |q~ - q| max|c~|, |q| max|c~ - fl(c - mu)|, SLACK |q| max(max|c|, max|c~|)."""
    q = np.ascontiguousarray(queries, np.float32)
    q64 = q.astype(np.float64)
    qn = np.sqrt((q64 * q64).sum(1))
    qd = np.sqrt(((bf16_round(q).astype(np.float64) - q64) ** 2).sum(1))
    cn, cb, cd = np.sqrt(np.asarray(words, np.float64))
    return np.stack([qd * cb, qn * cd, SCREEN_ACC_SLACK * qn * max(cn, cb)], axis=1)


def band_expected(queries: np.ndarray, words) -> np.ndarray:
    """E64[q] = 2 e(q): the full band width screen_setup_kernel rounds up into eps2[q]."""
    return 2.0 * band_terms(queries, words).sum(1)
