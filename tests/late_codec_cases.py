"""The compressed token store of late interaction: the codec restated bit for bit in NumPy, the fp64 reference, the
error band and a small host-side codec fit (no GPU).

* ``compress_rows`` restates ``sskd_latec_compress`` (``include/sskd_amd.h``, "Compressed token store"): per column
  ``r = fl32(t - c)``, ``code = searchsorted(cutoffs, r, "left")`` (NaN -> 0), ``dec = bf16_rn(fl32(c + weights[code]))``,
  ``scale = 1 / max(sqrt(ss), 1e-12)`` with ``ss`` in the pack kernel's order (``late_cases.sum_squares_rows``).
* ``pack_codes`` / ``unpack_codes`` are the byte order: column ``d = 16 s + 8 h + e`` sits at position ``192 h + 8 s + e``,
  ``nbits`` bits each, low bits first.
* ``decode_rows`` is what the re-rank kernel's A operand holds (a ``cid`` outside ``[0, C)`` is clamped into it).
* ``s64c`` is the score's reference: ``sum_i max_j <q_i, dec_j> * scale_j`` in fp64 on the stored values.
* ``band_c`` is the bound ``E_c = 1.01 (2 * 384 * Tq + Tq + Tq^2) 2^-24 Nq Nd``.

Token matrices travel as uint16 bf16 bit patterns, as in ``late_cases``.
"""
import numpy as np

import late_cases as lc

DIM = lc.DIM
C_MAX = 65536


# ------------------------------------------------------------------ byte order
def positions() -> np.ndarray:
    """``pos[d]`` = the position of column ``d``: ``d = 16 s + 8 h + e -> 192 h + 8 s + e``."""
    d = np.arange(DIM)
    s, h, e = d // 16, (d // 8) % 2, d % 8
    return 192 * h + 8 * s + e


def code_bytes(nbits: int) -> int:
    return DIM * nbits // 8            # 96 or 192


def pack_codes(codes: np.ndarray, nbits: int) -> np.ndarray:
    """``codes [n, 384]`` (column order, values below ``2^nbits``) -> uint8 ``[n, 48 nbits]``."""
    codes = np.asarray(codes).reshape(-1, DIM)
    per = 8 // nbits
    by_pos = np.zeros(codes.shape, dtype=np.uint32)
    by_pos[:, positions()] = codes
    out = np.zeros((codes.shape[0], code_bytes(nbits)), dtype=np.uint32)
    for i in range(per):
        out |= by_pos[:, i::per] << (nbits * i)
    return out.astype(np.uint8)


def unpack_codes(packed: np.ndarray, nbits: int) -> np.ndarray:
    """uint8 ``[n, 48 nbits]`` -> ``codes [n, 384]`` in column order."""
    packed = np.asarray(packed, dtype=np.uint8).reshape(-1, code_bytes(nbits)).astype(np.uint32)
    per = 8 // nbits
    by_pos = np.zeros((packed.shape[0], DIM), dtype=np.uint32)
    for i in range(per):
        by_pos[:, i::per] = (packed >> (nbits * i)) & ((1 << nbits) - 1)
    return by_pos[:, positions()].astype(np.uint8)


# ------------------------------------------------------------------ the codec
def _codec(centroid_bits, cutoffs, weights, nbits):
    cen = np.ascontiguousarray(centroid_bits, dtype=np.uint16).reshape(-1, DIM)
    cut = np.ascontiguousarray(cutoffs, dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    assert nbits in (2, 4) and cut.size == (1 << nbits) - 1 and w.size == 1 << nbits and 1 <= cen.shape[0] <= C_MAX
    return cen, cut, w


def decode_values(cid, codes, centroid_bits, weights) -> np.ndarray:
    """``dec`` bits from centroid ids (clamped into ``[0, C)``) and column-order codes."""
    cen = np.ascontiguousarray(centroid_bits, dtype=np.uint16).reshape(-1, DIM)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    c = lc.bf16_values(cen[np.clip(np.asarray(cid, np.int64), 0, cen.shape[0] - 1)])
    return lc.bf16_bits(c + w[np.asarray(codes, np.int64)])          # one fp32 addition, then nearest even


def scale_rows(dec_bits) -> np.ndarray:
    """fp32 ``1 / max(sqrt(ss), 1e-12)`` with ``ss`` the kernel's sum of squares of ``dec``."""
    with np.errstate(all="ignore"):
        ss = lc.sum_squares_rows(lc.bf16_values(dec_bits))
        return (np.float32(1.0) / np.maximum(np.sqrt(ss), np.float32(1e-12))).astype(np.float32)


def compress_rows(tok_bits, assign, centroid_bits, cutoffs, weights, nbits: int):
    """``sskd_latec_compress`` restated: ``(cid int32 [n], scale fp32 [n], codes uint8 [n, 48 nbits], dec bits [n, 384])``."""
    cen, cut, w = _codec(centroid_bits, cutoffs, weights, nbits)
    tok = np.ascontiguousarray(tok_bits, dtype=np.uint16).reshape(-1, DIM)
    cid = np.clip(np.asarray(assign, np.int64), 0, cen.shape[0] - 1).astype(np.int32)
    with np.errstate(all="ignore"):
        r = (lc.bf16_values(tok) - lc.bf16_values(cen[cid])).astype(np.float32)
    codes = np.where(np.isnan(r), 0, np.searchsorted(cut, r, side="left")).astype(np.uint8)
    dec = decode_values(cid, codes, cen, w)
    return cid, scale_rows(dec), pack_codes(codes, nbits), dec


def decode_rows(cid, packed, centroid_bits, weights, nbits: int) -> np.ndarray:
    """The ``dec`` bits of a compressed store (what the re-rank kernel multiplies)."""
    return decode_values(cid, unpack_codes(packed, nbits), centroid_bits, weights)


# ------------------------------------------------------------------ reference and band
def s64c(q_bits, dec_bits, scale) -> float:
    """``sum_i max_j <q_i, dec_j> * scale_j`` in fp64 on the stored values."""
    q = lc.bf16_values(q_bits).astype(np.float64)
    d = lc.bf16_values(dec_bits).astype(np.float64)
    return float(((q @ d.T) * np.asarray(scale, np.float64)[None, :]).max(axis=1).sum())


def band_c(tq: int, nq_norm, nd_norm):
    """``E_c = 1.01 (2 * 384 * Tq + Tq + Tq^2) 2^-24 Nq Nd``: section 21's band plus one rounding per query token for
    the multiplication by ``scale``."""
    return 1.01 * (2 * DIM * tq + tq + tq * tq) * 2.0 ** -24 * nq_norm * nd_norm


class ReferenceC:
    """``late_cases.Reference`` for a compressed store: fp64 scores ``s64`` and the band ``E`` of every (query, store
    row) pair, from the decoded values and the stored scales.  ``of_candidates`` as there."""

    of_candidates = lc.Reference.of_candidates

    def __init__(self, q_bits, q_lims, dec_bits, scale, tok_lims):
        q_lims, tok_lims = np.asarray(q_lims, np.int64), np.asarray(tok_lims, np.int64)
        nq, n = q_lims.size - 1, tok_lims.size - 1
        sc = np.asarray(scale, np.float64)
        d64 = lc.bf16_values(dec_bits).reshape(-1, DIM).astype(np.float64)
        dnorm = sc * np.sqrt((d64 * d64).sum(axis=1))
        self.row_norm = lc._segment_max(dnorm[None, :], tok_lims)[0]
        self.empty = tok_lims[1:] == tok_lims[:-1]
        self.s64 = np.full((nq, n), -np.inf)
        self.E = np.zeros((nq, n))
        for q in range(nq):
            qt = lc.bf16_values(q_bits[q_lims[q]: q_lims[q + 1]]).reshape(-1, DIM).astype(np.float64)
            best = lc._segment_max((qt @ d64.T) * sc[None, :], tok_lims)
            self.s64[q] = np.where(self.empty, -np.inf, best.sum(axis=0))
            qn = float(np.sqrt((qt * qt).sum(axis=1)).max())
            self.E[q] = np.where(self.empty, 0.0, band_c(qt.shape[0], qn, np.where(self.empty, 0.0, self.row_norm)))


# ------------------------------------------------------------------ a host-side codec (tests only)
def assign_rows(tok_bits, centroid_bits) -> np.ndarray:
    """Nearest centroid by inner product in fp64, ties to the lower id."""
    t = lc.bf16_values(tok_bits).astype(np.float64)
    c = lc.bf16_values(np.asarray(centroid_bits).reshape(-1, DIM)).astype(np.float64)
    return np.argmax(t @ c.T, axis=1).astype(np.int64)


def quantile_tables(residuals, nbits: int):
    """ColBERTv2's rule: ``cutoffs`` = the ``i / L`` quantiles (i = 1 .. L - 1), ``weights`` = the ``(i + 1/2) / L``
    quantiles (i = 0 .. L - 1) of the residuals, fp32."""
    L = 1 << nbits
    r = np.sort(np.asarray(residuals, np.float32).reshape(-1))
    cut = np.quantile(r, np.arange(1, L) / L).astype(np.float32)
    w = np.quantile(r, (np.arange(L) + 0.5) / L).astype(np.float32)
    return cut, w


def fit_codec(tok_bits, n_centroids: int, nbits: int, seed: int = 1, iterations: int = 4):
    """A small spherical k-means plus the quantile tables: ``(centroid bits [C, 384], cutoffs, weights)``."""
    rng = np.random.default_rng(seed)
    t = lc.bf16_values(tok_bits).astype(np.float64)
    cen = t[np.sort(rng.permutation(t.shape[0])[:n_centroids])].copy()
    for _ in range(iterations):
        a = np.argmax(t @ cen.T, axis=1)
        for c in range(n_centroids):
            if (a == c).any():
                m = t[a == c].sum(axis=0)
                cen[c] = m / max(np.linalg.norm(m), 1e-12)
    cen_bits = lc.bf16_bits(cen.astype(np.float32))
    a = assign_rows(tok_bits, cen_bits)
    res = lc.bf16_values(tok_bits) - lc.bf16_values(cen_bits[a])
    cut, w = quantile_tables(res, nbits)
    return cen_bits, cut, w


def random_codec(rng, n_centroids: int, nbits: int):
    """Unit random centroids and the quantile tables of a unit gaussian residual of 384 columns."""
    cen = lc.unit_token_bits(rng, n_centroids)
    L = 1 << nbits
    z = np.sort(rng.standard_normal(20000)).astype(np.float32) * np.float32(DIM ** -0.5)
    cut = np.quantile(z, np.arange(1, L) / L).astype(np.float32)
    w = np.quantile(z, (np.arange(L) + 0.5) / L).astype(np.float32)
    return cen, cut, w
