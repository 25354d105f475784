"""Hand-made padded rankings for the kernels that walk a first stage's ``[nq][width]`` ranking 64 ranks per round
(``csrc/ranking_walk.h`` holds the rule and the per-kernel table): mine, hybrid, MMR, Rocchio, RM3 and denoise.

Five queries, so the last workgroup of the one-wave-per-query kernels has idle waves, at the widths on both sides of the
64-rank round.  Every rank holds a distinct valid row first; then, where the width has room for them:

  query 0   the first -1 at rank 0; valid rows right behind it, in the same round and in the next one
  query 1   rows ``n_rows``, far above ``n_rows`` and -9 at ranks 1 .. 3, the first -1 at rank 63 (the last lane of
            round one), a valid row at rank 64 (the first lane of round two)
  query 2   ``n_rows`` at rank 10, a far id at rank 62, -9 at rank 63, the first -1 at rank 64 (first lane of round two),
            valid rows behind it in that round
  query 3   no -1 at all: ``n_rows`` at rank 0, a far id at rank 5, -9 at rank 66
  query 4   no -1 at all, one -9 at rank 2: a kernel that ends its walk on ANY negative id keeps two rows here, one that
            ends on -1 alone keeps ``width - 1``

-9 (a negative id that is not the padding id) and the valid rows behind the first -1 are where the kernels' rules differ.
"""
from functools import lru_cache

import numpy as np

WIDTHS = (1, 63, 64, 65, 130)
NQ = 5
FAR = (1 << 40) + 3


@lru_cache(maxsize=None)
def ids(n_rows, width, seed=0):
    """int64 ``[5, width]`` (read-only)"""
    assert n_rows >= width
    g = np.random.default_rng(1000 * width + seed)
    I = np.stack([g.permutation(n_rows)[:width] for _ in range(NQ)]).astype(np.int64)
    marks = {
        0: {0: -1},
        1: {1: n_rows, 2: FAR, 3: -9, 63: -1},
        2: {10: n_rows, 62: FAR, 63: -9, 64: -1},
        3: {0: n_rows, 5: FAR, 66: -9},
        4: {2: -9},
    }
    for q, at in marks.items():
        for rank, value in at.items():
            if rank < width:
                I[q, rank] = value
    I.setflags(write=False)
    return I


def first_pad(I):
    """rank of the first -1 of every query, the width where there is none"""
    return np.array([int(np.flatnonzero(row == -1)[0]) if (row == -1).any() else row.size for row in I])


def descending_scores(width, dtype=np.float32, seed=0, low=0.5, high=9.0):
    """``[5, width]`` strictly positive scores, descending per query"""
    g = np.random.default_rng(2000 * width + seed)
    return -np.sort(-g.uniform(low, high, (NQ, width)), axis=1).astype(dtype)
