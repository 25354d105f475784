"""Late interaction: the NumPy restatements, the fp64 reference, the error band and the case generators (no GPU).

* ``pack_rows`` restates ``sskd_late_pack_tokens`` bit for bit (the order of the sum of squares is the kernel's one
  documented order: ``include/sskd_amd.h``, "Late interaction").
* ``s64`` is the score's reference: ``sum_i max_j <q_i, d_j>`` in fp64 on the bf16 values actually stored.
* ``band`` is the derived bound ``E`` on ``|score - s64|``: ``1.01 (2 * 384 * Tq + Tq^2) 2^-24 Nq Nd``.
* ``emulate_f32`` is a sequential fp32 evaluation of the kernel's contract (fp32 dot accumulation, fp32 max, sequential
  fp32 sum): ONE admissible order, used to show on the CPU that the band holds the reference's own rounding.
* ``check_ranking`` is the tolerant ranking check: it holds ``(D, I)`` to the raw scores the kernel itself reported.

Token matrices travel as uint16 bf16 bit patterns (NumPy has no bf16).
"""
import numpy as np

DIM = 384
TQ_MAX = 128
R_MAX = 1024


# ------------------------------------------------------------------ bf16
def bf16_bits(x) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16), round to nearest even (finite input)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_values(bits) -> np.ndarray:
    """bf16 bit patterns -> the fp32 values they stand for."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


# ------------------------------------------------------------------ pack
def sum_squares_rows(x: np.ndarray) -> np.ndarray:
    """fp32 ``[n, 384]`` -> the kernel's sum of squares per row, fp32 ``[n]``: lane l < 48 chains its columns
    8 l .. 8 l + 7 from +0.0 (a bf16 square is exact in fp32, so the kernel's fma equals add(p, x * x)), lanes 48 .. 63
    hold +0.0, then the xor butterfly o = 32, 16, 8, 4, 2, 1 with ``p_l = p_l + p_(l ^ o)``."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, DIM)
    p = np.zeros((x.shape[0], 64), dtype=np.float32)
    lanes = x.reshape(-1, DIM // 8, 8)
    for j in range(8):
        p[:, : DIM // 8] = p[:, : DIM // 8] + lanes[:, :, j] * lanes[:, :, j]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, idx ^ o]
    return p[:, 0]


def normalize_rows_bits(x: np.ndarray) -> np.ndarray:
    """The pack arithmetic on fp32 rows holding bf16 values: ``x / max(sqrt(ss), 1e-12)`` in fp32 (IEEE sqrt and
    division), rounded to bf16 to nearest even.  uint16 ``[n, 384]``."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, DIM)
    with np.errstate(all="ignore"):
        denom = np.maximum(np.sqrt(sum_squares_rows(x)), np.float32(1e-12)).astype(np.float32)
        return bf16_bits(x / denom[:, None])


def pack_rows(hidden_bits: np.ndarray, lengths) -> tuple:
    """``sskd_late_pack_tokens`` restated: hidden bf16 bits ``[B, S, 384]`` and ``lengths [B]`` -> ``(token bits
    [T, 384], lims int64 [B + 1])``, the texts' real tokens in order."""
    lengths = np.asarray(lengths, dtype=np.int64)
    lims = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rows = [hidden_bits[b, : lengths[b]] for b in range(hidden_bits.shape[0])]
    real = np.concatenate(rows).reshape(-1, DIM) if rows else np.zeros((0, DIM), np.uint16)
    return normalize_rows_bits(bf16_values(real)), lims


def unit_token_bits(rng, n: int, scale: float = 1.0) -> np.ndarray:
    """n random rows, normalised by the pack arithmetic (so what a store holds), as bf16 bits."""
    x = bf16_values(bf16_bits(rng.standard_normal((n, DIM)).astype(np.float32) * np.float32(scale)))
    return normalize_rows_bits(x)


# ------------------------------------------------------------------ reference and band
def s64(q_bits: np.ndarray, d_bits: np.ndarray) -> float:
    """``sum_i max_j <q_i, d_j>`` in fp64 on the stored bf16 values."""
    q = bf16_values(q_bits).astype(np.float64)
    d = bf16_values(d_bits).astype(np.float64)
    return float((q @ d.T).max(axis=1).sum())


def band(tq: int, nq_norm: float, nd_norm: float) -> float:
    """``E = 1.01 (2 * 384 * Tq + Tq^2) 2^-24 Nq Nd``."""
    return 1.01 * (2 * DIM * tq + tq * tq) * 2.0 ** -24 * nq_norm * nd_norm


def _segment_max(dots: np.ndarray, lims: np.ndarray) -> np.ndarray:
    """``[Tq, T]`` dots -> ``[Tq, n_rows]`` max over every row's tokens (-inf for a row without tokens)."""
    n = lims.size - 1
    out = np.full((dots.shape[0], n), -np.inf, dtype=dots.dtype)
    full = np.flatnonzero(lims[1:] > lims[:-1])
    if full.size:
        # reduceat over the non-empty rows only: their starts ascend strictly and each segment ends where the next
        # non-empty row begins (empty rows own no columns)
        out[:, full] = np.maximum.reduceat(dots, lims[full], axis=1)
    return out


class Reference:
    """Per case: fp64 scores, the band and the fp32 emulation of every (query, store row) pair."""

    def __init__(self, q_bits, q_lims, tok_bits, tok_lims, emulate: bool = False):
        q_lims, tok_lims = np.asarray(q_lims, np.int64), np.asarray(tok_lims, np.int64)
        nq, n = q_lims.size - 1, tok_lims.size - 1
        d32 = bf16_values(tok_bits).reshape(-1, DIM)
        d64 = d32.astype(np.float64)
        dnorm = np.sqrt((d64 * d64).sum(axis=1))
        self.row_norm = _segment_max(dnorm[None, :], tok_lims)[0]          # Nd per row (-inf: no tokens)
        self.empty = tok_lims[1:] == tok_lims[:-1]
        self.s64 = np.full((nq, n), -np.inf)
        self.E = np.zeros((nq, n))
        self.f32 = np.full((nq, n), -np.inf, dtype=np.float32) if emulate else None
        for q in range(nq):
            qt32 = bf16_values(q_bits[q_lims[q]: q_lims[q + 1]]).reshape(-1, DIM)
            qt = qt32.astype(np.float64)
            tq = qt.shape[0]
            best = _segment_max(qt @ d64.T, tok_lims)
            self.s64[q] = np.where(self.empty, -np.inf, best.sum(axis=0))
            qn = float(np.sqrt((qt * qt).sum(axis=1)).max())
            self.E[q] = np.where(self.empty, 0.0, band(tq, qn, np.where(self.empty, 0.0, self.row_norm)))
            if emulate:
                acc = np.zeros((tq, d32.shape[0]), dtype=np.float32)
                for c in range(DIM):                                        # fp32 accumulation, columns ascending
                    acc = acc + qt32[:, c: c + 1] * d32[:, c][None, :]
                m = _segment_max(acc, tok_lims)
                s = np.zeros(n, dtype=np.float32)
                for i in range(tq):                                         # sequential fp32 sum from +0.0
                    s = s + np.where(self.empty, np.float32(0), m[i])
                self.f32[q] = np.where(self.empty, -np.inf, s)

    def of_candidates(self, table: np.ndarray, cand: np.ndarray, id_offset: int = 0, fill=-np.inf) -> np.ndarray:
        """``table [nq, n_rows]`` gathered at the candidates ``[nq, R]`` (global ids); ``fill`` where there is none."""
        n = table.shape[1]
        rows = cand - id_offset
        ok = (cand >= 0) & (rows >= 0) & (rows < n)
        safe = np.where(ok, rows, 0)
        got = np.take_along_axis(table, safe, axis=1)
        absent = ~ok | np.take_along_axis(np.broadcast_to(self.empty, table.shape), safe, axis=1)
        return np.where(absent, fill, got)


def emulate_f32(q_bits, d_bits) -> np.float32:
    """One pair through the fp32 emulation (host tests of single pairs)."""
    ref = Reference(q_bits, [0, len(q_bits)], d_bits, [0, len(d_bits)], emulate=True)
    return ref.f32[0, 0]


# ------------------------------------------------------------------ ranking
def check_ranking(D, I, raw, cand, k: int) -> None:
    """The tolerant form: ``(D, I)`` is the top-k of the kernel's OWN raw scores in the project's order."""
    D, I, raw, cand = np.asarray(D), np.asarray(I), np.asarray(raw), np.asarray(cand)
    nq, R = cand.shape
    assert D.shape == (nq, k) and I.shape == (nq, k)
    for q in range(nq):
        valid = np.isfinite(raw[q]) | (raw[q] == np.inf)
        assert not np.isnan(raw[q]).any()
        n_valid = int(valid.sum())
        got = int((I[q] >= 0).sum())
        assert got == min(k, n_valid), f"query {q}: {got} results for {n_valid} valid candidates, k={k}"
        assert (I[q, got:] == -1).all() and np.isneginf(D[q, got:]).all(), f"query {q}: padding is not (-inf, -1)"
        pos_of = {}
        for p in np.flatnonzero(valid):
            pos_of.setdefault(int(cand[q, p]), int(p))
        returned = set()
        for p in range(got):
            i = int(I[q, p])
            assert i in pos_of, f"query {q}: returned id {i} is not a valid candidate"
            assert i not in returned, f"query {q}: id {i} returned twice"
            returned.add(i)
            assert D[q, p].view(np.uint32) == raw[q, pos_of[i]].view(np.uint32), f"query {q}: D[{p}] is not the raw score of {i}"
            if p:
                assert D[q, p - 1] > D[q, p] or (D[q, p - 1] == D[q, p] and I[q, p - 1] < i), f"query {q}: order broken at {p}"
        if got == k:
            last_s, last_i = D[q, k - 1], int(I[q, k - 1])
            for i, p in pos_of.items():
                if i not in returned:
                    assert raw[q, p] < last_s or (raw[q, p] == last_s and i > last_i), \
                        f"query {q}: candidate {i} ({raw[q, p]}) beats the last result ({last_s}, {last_i})"


# ------------------------------------------------------------------ case generators
BIG_TD = (31, 32, 33, 64, 95, 180)


def sweep_store(seed: int = 7, n_rows: int = 1100):
    """The sweep's token store: ``(bits [T, 384], lims)`` over ``n_rows`` rows, about 4.8 k token rows.  Every 24th row
    has a length from ``BIG_TD`` in turn, the rest 1 or 2 tokens (1 024 DISTINCT candidates need many rows, a small
    store needs them short), and row 7 has none."""
    rng = np.random.default_rng(seed)
    td = np.array([BIG_TD[(r // 24) % len(BIG_TD)] if r % 24 == 0 else 1 + (r % 3 == 0) for r in range(n_rows)], np.int64)
    td[7] = 0
    lims = np.concatenate([[0], np.cumsum(td)]).astype(np.int64)
    return unit_token_bits(rng, int(lims[-1])), lims


def queries(rng, tqs):
    """Random unit query tokens: ``(bits [sum Tq, 384], lims)``."""
    lims = np.concatenate([[0], np.cumsum(np.asarray(tqs, np.int64))]).astype(np.int64)
    return unit_token_bits(rng, int(lims[-1])), lims


def candidates(rng, nq: int, R: int, n_rows: int, id_offset: int = 0, holes: bool = True, must=()):
    """int64 ``[nq, R]`` distinct global ids per query in random order: the rows of ``must`` first of all (then
    shuffled in), and with ``holes`` a few ``-1`` entries where R allows."""
    out = np.empty((nq, R), dtype=np.int64)
    must = np.asarray(list(must), dtype=np.int64)[:R]
    for q in range(nq):
        rest = np.setdiff1d(np.arange(n_rows), must)
        pick = np.concatenate([must, rng.permutation(rest)[: R - must.size]])
        row = rng.permutation(pick) + id_offset
        if holes and R >= 7:
            row[rng.permutation(R)[: max(1, R // 16)]] = -1
        out[q] = row
    return out


# (nq, Tq per query, R): every Tq, R and nq of the sweep appears, Tq mixed inside a batch
SWEEP = [
    (1, [1], 1),
    (3, [5, 32, 33], 7),
    (3, [64, 128, 1], 64),
    (1, [33], 65),
    (67, [(1, 5, 32, 33)[i % 4] for i in range(67)], 200),
    (3, [128, 64, 32], 1024),
]


def big_rows(lims) -> np.ndarray:
    """Rows of a store with more than 2 tokens (the ``BIG_TD`` rows of ``sweep_store``)."""
    lims = np.asarray(lims)
    return np.flatnonzero(lims[1:] - lims[:-1] > 2)


def last_tile_family(seed: int = 11):
    """The best document token sits in the last, PARTIAL tile: every document is random rows whose LAST row is a copy of
    one query token.  ``(q_bits, q_lims, tok_bits, tok_lims, cand)``, one query of 5 tokens, Td in {33, 65, 95, 180, 1}."""
    rng = np.random.default_rng(seed)
    q_bits, q_lims = queries(rng, [5])
    tds = [33, 65, 95, 180, 1, 34]
    lims = np.concatenate([[0], np.cumsum(tds)]).astype(np.int64)
    tok = unit_token_bits(rng, int(lims[-1]))
    for r in range(len(tds)):
        tok[lims[r + 1] - 1] = q_bits[r % 5]
    return q_bits, q_lims, tok, lims, np.arange(len(tds), dtype=np.int64)[None, :]


def negative_family(seed: int = 13, tqs=(5, 33, 1)):
    """Every true dot product is negative (query tokens in the positive orthant, document tokens in the negative), so a
    masked document row read as zeros - or as anything of a neighbour's that is less negative - would win the max, and
    the fp64 score is far from what a zero would make it.  Td covers partial tiles; the queries are short of a block,
    so query columns >= Tq exist in every tile, followed in memory by the NEXT query's tokens."""
    rng = np.random.default_rng(seed)
    q_lims = np.concatenate([[0], np.cumsum(tqs)]).astype(np.int64)
    q = np.abs(rng.standard_normal((int(q_lims[-1]), DIM))).astype(np.float32) + np.float32(0.05)
    q_bits = normalize_rows_bits(bf16_values(bf16_bits(q)))
    tds = [1, 31, 33, 95, 180, 64, 2]
    lims = np.concatenate([[0], np.cumsum(tds)]).astype(np.int64)
    d = -(np.abs(rng.standard_normal((int(lims[-1]), DIM))).astype(np.float32) + np.float32(0.05))
    # the rows after a document's last one belong to the next document: make every document's FIRST row its least
    # negative, so reading one row too many would also win
    for r in range(len(tds)):
        d[lims[r]] *= np.float32(0.25)
    tok = bf16_bits(d / np.float32(4.0))           # short rows (norm < 1): least negative = closest to zero
    cand = np.tile(np.arange(len(tds), dtype=np.int64), (len(tqs), 1))
    return q_bits, q_lims, tok, lims, cand


def separated_family(seed: int = 17, tq: int = 32, R: int = 20):
    """Candidate c holds copies of the first ``m_c`` query tokens, the ``m_c`` distinct: its score is about ``m_c`` plus
    ``Tq - m_c`` small maxima, so neighbouring scores are about 0.9 apart - far beyond the band - and the fp64 ranking
    is THE ranking.  ``(q_bits, q_lims, tok_bits, tok_lims, cand, m)``."""
    rng = np.random.default_rng(seed)
    q_bits, q_lims = queries(rng, [tq])
    m = rng.permutation(np.arange(1, tq + 1))[:R]
    lims = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    tok = np.concatenate([q_bits[:mc] for mc in m])
    return q_bits, q_lims, tok, lims, rng.permutation(R).astype(np.int64)[None, :], m


def pack_cases(seed: int = 19):
    """``(name, hidden bits [B, S, 384], lengths)`` for the pack kernel: S in {1, 31, 32, 33, 256}, lengths 1, S and
    mixed, an all-zero row (the 1e-12 floor), rows small enough that the floor decides, large and small magnitudes."""
    rng = np.random.default_rng(seed)
    out = []
    for S in (1, 31, 32, 33, 256):
        B = 3 if S > 1 else 2
        h = rng.standard_normal((B, S, DIM)).astype(np.float32)
        h[0] *= np.float32(1e15)                     # ss ~ 4e32 < FLT_MAX
        h[1] *= np.float32(2.0 ** -20)
        if S > 1:
            h[2, 0] = 0.0                            # all-zero token: 0 / 1e-12 = 0
            h[2, 1] *= np.float32(1e-14)             # sqrt(ss) ~ 2e-13 < 1e-12: the floor decides, no denormals
        for name, lengths in (("one", [1] * B), ("full", [S] * B), ("mixed", [S, max(1, S // 2), min(S, 2)][:B])):
            out.append((f"S{S}-{name}", bf16_bits(h), np.asarray(lengths, np.int32)))
    return out
