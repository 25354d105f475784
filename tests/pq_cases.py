"""The IVF-PQ definitions of ``include/sskd_amd.h`` restated in NumPy, step for step.

Every step is a sequence of single IEEE operations in a fixed order - fp32 subtractions for the residual, fp64 subtract /
multiply / add (no fma) for the encoding distance, sequential fp64 adds for the code sums and the look-up table, sequential
fp32 adds for the ADC score - and NumPy's element-wise float32 / float64 operations are those same operations, so the
device results are compared with ``np.array_equal`` on bits.  (``np.cumsum`` adds in index order; nothing here uses
``np.sum``, whose pairwise order is a different one.)"""
import numpy as np

DIM, CODES = 384, 256
NEG_PAD = np.float32(-np.finfo(np.float32).max)


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def residuals(rows, centroids=None, assign=None):
    """r = row - centroid[list(row)], one fp32 subtraction per element (no assignment: the rows themselves)."""
    rows = np.asarray(rows, np.float32)
    if assign is None:
        return rows.copy()
    return (rows - np.asarray(centroids, np.float32)[np.asarray(assign)]).astype(np.float32)


def encode_distances(resid, cb, j):
    """fp64 ``[n, 256]``: sum over d ascending from +0.0 of (r_d - cb[j][c][d])^2, subtract, multiply, add each rounded once"""
    dsub = cb.shape[2]
    r = np.asarray(resid, np.float32)[:, j * dsub:(j + 1) * dsub].astype(np.float64)
    c = cb[j].astype(np.float64)
    acc = np.zeros((r.shape[0], CODES), np.float64)
    for d in range(dsub):
        t = r[:, None, d] - c[None, :, d]
        t2 = t * t
        acc = acc + t2
    return acc


def encode(resid, cb):
    """uint8 ``[n, m]``: the argmin code per subspace, ties to the lower code (np.argmin keeps the first minimum)"""
    m = cb.shape[0]
    out = np.empty((np.asarray(resid).shape[0], m), np.uint8)
    for j in range(m):
        out[:, j] = np.argmin(encode_distances(resid, cb, j), axis=1)
    return out


def code_sums(resid, codes, m):
    """``(sums fp64 [m, 256, dsub], counts int64 [m, 256])``: one accumulator from +0.0 per element, rows ascending"""
    dsub = DIM // m
    r = np.asarray(resid, np.float32).astype(np.float64)
    sums = np.zeros((m, CODES, dsub), np.float64)
    counts = np.zeros((m, CODES), np.int64)
    for j in range(m):
        for c in np.unique(codes[:, j]):
            part = r[codes[:, j] == c, j * dsub:(j + 1) * dsub]   # boolean selection keeps ascending row order
            sums[j, c] = np.cumsum(part, axis=0)[-1]
            counts[j, c] = part.shape[0]
    return sums, counts


def update_codebooks(cb, sums, counts):
    """fl32(sum / count), the division in fp64; an empty code keeps its entry"""
    new = (sums / np.maximum(counts, 1)[:, :, None].astype(np.float64)).astype(np.float32)
    return np.where((counts > 0)[:, :, None], new, cb).astype(np.float32)


def lut(queries, cb):
    """fp32 ``[nq, m, 256]``: fl32 of the fp64 sum over d ascending of (double) q_d (double) cb[j][c][d]"""
    m, _, dsub = cb.shape
    q = np.asarray(queries, np.float32).astype(np.float64)
    out = np.empty((q.shape[0], m, CODES), np.float32)
    for j in range(m):
        c = cb[j].astype(np.float64)
        acc = np.zeros((q.shape[0], CODES), np.float64)
        for d in range(dsub):
            acc = acc + q[:, None, j * dsub + d] * c[None, :, d]
        out[:, j] = acc.astype(np.float32)
    return out


def adc_scores(base, lut_q, codes):
    """fp32 ``[n]``: s = base (the probe score of the row's list), then s = s + lut[j][code_j], j ascending, fp32 adds"""
    s = np.asarray(base, np.float32).copy()
    for j in range(codes.shape[1]):
        s = s + lut_q[j, codes[:, j]]
    assert s.dtype == np.float32
    return s


def rank_order(scores, ids):
    """indices that put (score, id) pairs into rank order: score descending, then lower id"""
    return np.lexsort((ids, -np.asarray(scores, np.float32)))


def probed(probe_row, probe_scores_row, offsets, list_rows, nlist, allowed=None):
    """``(rows, base)`` of the rows a query probes, in position order: -1 and out-of-range probes are skipped, rows that
    ``allowed`` (bool per row, or None) hides are dropped before anything is scored"""
    rows, base = [], []
    for l, s in zip(probe_row, probe_scores_row):
        if 0 <= l < nlist:
            part = list_rows[offsets[l]:offsets[l + 1]].astype(np.int64)
            rows.append(part)
            base.append(np.full(part.size, s, np.float32))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    base = np.concatenate(base) if base else np.zeros(0, np.float32)
    if allowed is not None:
        keep = allowed[rows]
        rows, base = rows[keep], base[keep]
    return rows, base


def adc_ranking(probe_row, probe_scores_row, offsets, list_rows, nlist, lut_q, codes_by_row, allowed=None):
    """``(scores, rows)`` of every probed row in ADC rank order"""
    rows, base = probed(probe_row, probe_scores_row, offsets, list_rows, nlist, allowed)
    s = adc_scores(base, lut_q, codes_by_row[rows])
    order = rank_order(s, rows)
    return s[order], rows[order]


def padded(scores, ids, k):
    """the first k of a ranking, padded with (-FLT_MAX, -1)"""
    out_s = np.full(k, NEG_PAD, np.float32)
    out_i = np.full(k, -1, np.int64)
    n = min(k, len(ids))
    out_s[:n], out_i[:n] = scores[:n], ids[:n]
    return out_s, out_i


def reconstruction_mse(resid, cb, codes):
    """mean squared error of the residuals against their code entries (float64, for the training test)"""
    m, _, dsub = cb.shape
    rec = np.concatenate([cb[j][codes[:, j]] for j in range(m)], axis=1).astype(np.float64)
    return float(((np.asarray(resid, np.float64) - rec) ** 2).sum(axis=1).mean())


def seeded_codebooks(m, seed, scale=0.05):
    return (np.random.default_rng(seed).standard_normal((m, CODES, DIM // m)) * scale).astype(np.float32)
