"""Late interaction held to EQUALITY: the world, the atom requests and the NumPy fp32 restatement of every kernel that
runs the MaxSim tile engine (no GPU, no library).

The kernels state that an element ``<q_i, d_j>`` is the chain of 24 MFMAs over those two rows alone.  So the ``atoms``
``a[i, j]`` - what ``sskd_late_rerank`` returns as the raw score of the one-token query ``i`` against the one-token
document ``j`` - are the very fp32 values every other call reduces, and the reductions are restated here in their one
documented order:

* bf16 store:       ``score = `` sequential fp32 sum from +0.0f over ``i`` ascending of ``max_j a[i, j]``;
* training forward: the same bits, and ``arg[i] = `` the smallest ``j`` with ``a[i, j]`` equal to the maximum;
* compressed store: the atoms of the DECODED rows, ``score = seq-sum_i max_j fp32(a[i, j] * scale[j])``;
* centroid scores:  ``S[c, t] = `` the atom of centroid row ``c`` against query token ``t``.

``host_atoms`` stands in for the atoms on the CPU (the fp64 dot product rounded to fp32), so that the restatement can be
held to the fp64 references and bands of ``late_cases`` / ``late_codec_cases`` without a device.
"""
import numpy as np

import late_cases as lc
import late_codec_cases as cc

DIM = lc.DIM
ATOM_R_MAX = lc.R_MAX                      # candidates of one atom call

TQS = (1, 31, 33, 96, 128)                 # the query pool: 1 .. 4 blocks of 32 tokens, partial blocks
TDS = (1, 31, 32, 33, 65, 180, 0)          # whole tiles, partial tiles, and (last) a row without tokens
# batches of pool queries: the largest Tq decides how many blocks the workgroup stages (1, 1, 2, 3, 4)
BATCHES = ((0,), (1, 0), (2, 1, 0), (3, 0, 2), (4, 3, 2, 1, 0))
R = 9                                      # the 7 rows, one -1 and one row twice: two chunks of 4 and a tail of 1
CENTROIDS = (3, 40)
EMPTY_ROW = len(TDS) - 1


class World:
    """One seeded world, built once and left unchanged: the query pool, the documents, a codec of 40 centroids per
    width and the candidate lists of every batch."""

    def __init__(self, seed: int = 41):
        rng = np.random.default_rng(seed)
        self.q_bits, self.q_lims = lc.queries(rng, TQS)
        self.d_lims = np.concatenate([[0], np.cumsum(TDS)]).astype(np.int64)
        d = lc.unit_token_bits(rng, int(self.d_lims[-1]))
        ql, dl = self.q_lims, self.d_lims
        # the best document token sits in the last, partial tile (Td = 33, 65): a copy of a query token
        d[dl[4] - 1] = self.q_bits[ql[2]]
        d[dl[5] - 1] = self.q_bits[ql[3] + 40]
        # exact ties: the same copy twice inside one tile, in either lane half (Td = 32: rows 5 and 17), and in two
        # tiles (Td = 180: rows 10 and 179) - the argmax is the smaller index
        d[dl[2] + 5] = d[dl[2] + 17] = self.q_bits[ql[1] + 3]
        d[dl[5] + 10] = d[dl[6] - 1] = self.q_bits[ql[4] + 100]
        self.d_bits = d
        self.codec = {nbits: cc.random_codec(np.random.default_rng(seed + nbits), max(CENTROIDS), nbits) for nbits in (2, 4)}
        rows = np.concatenate([np.arange(len(TDS)), [-1, 5]]).astype(np.int64)
        self.cand = [np.stack([rng.permutation(rows) for _ in batch]) for batch in BATCHES]

    def batch(self, b: int):
        """``(q_bits, q_lims, cand)`` of batch ``b``: the pool queries' tokens one after the other."""
        pool = BATCHES[b]
        bits = np.concatenate([self.q_bits[self.q_lims[k]: self.q_lims[k + 1]] for k in pool])
        lims = np.concatenate([[0], np.cumsum([TQS[k] for k in pool])]).astype(np.int64)
        return bits, lims, self.cand[b]


def atom_requests(n_q: int, n_d: int):
    """The calls that return every atom of ``n_q`` query tokens against ``n_d`` document tokens: every token its own
    one-token query / document (``q_lims = arange``, ``tok_lims = arange``), the documents in runs of at most 1 024
    candidates.  Yields ``(lo, hi, cand int64 [n_q, hi - lo])``; ``k = hi - lo`` and the raw scores are the atoms."""
    for lo in range(0, n_d, ATOM_R_MAX):
        hi = min(n_d, lo + ATOM_R_MAX)
        yield lo, hi, np.ascontiguousarray(np.broadcast_to(np.arange(lo, hi, dtype=np.int64), (n_q, hi - lo)))


def host_atoms(q_bits, d_bits) -> np.ndarray:
    """A stand-in for the atoms without a device: the fp64 dot products rounded once to fp32, ``[n_q, n_d]``."""
    q = lc.bf16_values(q_bits).reshape(-1, DIM).astype(np.float64)
    d = lc.bf16_values(d_bits).reshape(-1, DIM).astype(np.float64)
    return (q @ d.T).astype(np.float32)


def stride_of(tqs) -> int:
    """``tq_stride`` of the training forward: the batch's largest Tq rounded up to 32."""
    return 32 * ((max(tqs) + 31) // 32)


def maxsim(atoms, pool_lims, pool, d_lims, cand, scale=None):
    """The restatement.  ``atoms`` fp32 ``[pool tokens, document tokens]``, ``pool`` the batch's pool queries, ``cand``
    int64 ``[nq, R]``; with ``scale`` fp32 ``[document tokens]`` every atom is multiplied by its row's scale (one fp32
    rounding) before the max.  Returns ``(raw fp32 [nq, R], arg int32 [nq, R, stride])``: -inf and -1 for a candidate
    that is none (``-1``, outside the rows, a row without tokens), -1 for the token slots past a query's end."""
    atoms = np.ascontiguousarray(atoms, dtype=np.float32)
    n_rows = len(d_lims) - 1
    tqs = [int(pool_lims[k + 1] - pool_lims[k]) for k in pool]
    raw = np.full(cand.shape, -np.inf, dtype=np.float32)
    arg = np.full(cand.shape + (stride_of(tqs),), -1, dtype=np.int32)
    for q, k in enumerate(pool):
        for c, row in enumerate(cand[q]):
            if row < 0 or row >= n_rows or d_lims[row + 1] <= d_lims[row]:
                continue
            block = atoms[pool_lims[k]: pool_lims[k + 1], d_lims[row]: d_lims[row + 1]]
            if scale is not None:
                block = block * np.asarray(scale, np.float32)[None, d_lims[row]: d_lims[row + 1]]
            assert block.dtype == np.float32
            best = block.max(axis=1)
            arg[q, c, : tqs[q]] = block.argmax(axis=1)            # the first of equal maxima
            s = np.float32(0.0)
            for v in best:                                          # sequential, ascending, from +0.0f
                s = np.float32(s + v)
            raw[q, c] = s
    return raw, arg


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
