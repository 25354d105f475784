"""Shared cases of the denoising tests: the rule of include/sskd_amd.h ("Denoising of a ranking") restated in plain Python
(sets, loops, ``int / int``), a text generator and the key-set families the kernels are run on.  Nothing here imports
``semantic_search_kd_amd.denoise``: the store, the host overlap and the kernels are all checked against this file.
Everything is seeded, computed once and never modified.
"""
from functools import lru_cache

import numpy as np

NEG_PAD = np.float32(-3.4028234663852886e38)     # -FLT_MAX
LDS_CAP = 4096                                    # keys of a positive the kernel stages in LDS at most


# ---------------------------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------------------------
def trigram_keys_ref(text):
    """ascending uint64 keys of the distinct character 3-grams of ``text.lower().strip()``"""
    s = text.lower().strip()
    grams = set(s[i:i + 3] for i in range(len(s) - 2))
    return np.array(sorted((ord(g[0]) << 42) | (ord(g[1]) << 21) | ord(g[2]) for g in grams), dtype=np.uint64)


def jaccard_ref(a, b):
    """``(inter, union, value)`` of two key collections; the value is Python's ``int / int`` and 0.0 for an empty set"""
    a, b = set(int(x) for x in a), set(int(x) for x in b)
    inter = len(a & b)
    uni = len(a) + len(b) - inter
    return inter, uni, (inter / uni if a and b else 0.0)


def csr_of(sets):
    """key arrays as the store's CSR ``(lims int64, keys uint64)``"""
    lims = np.zeros(len(sets) + 1, np.int64)
    for i, s in enumerate(sets):
        lims[i + 1] = lims[i] + len(s)
    keys = np.concatenate([np.asarray(s, np.uint64) for s in sets]) if sets else np.zeros(0, np.uint64)
    return lims, keys.astype(np.uint64)


class Pairs:
    """jaccard values of a family of sets by set number, each pair computed once; a number outside the family is the
    empty set"""

    def __init__(self, sets):
        self.sets = [frozenset(int(x) for x in s) for s in sets]
        self.seen = {}

    def __call__(self, a, b):
        n = len(self.sets)
        if not (0 <= a < n and 0 <= b < n):
            return 0.0
        key = (a, b) if a <= b else (b, a)
        if key not in self.seen:
            A, B = self.sets[a], self.sets[b]
            inter = len(A & B)
            self.seen[key] = inter / (len(A) + len(B) - inter) if A and B else 0.0
        return self.seen[key]


def denoise_ref(jac, rank_scores, rank_ids, pos_lims, pos_rows, aux=None, aux_threshold=None, overlap_threshold=None):
    """The rule, one query and one rank at a time.  ``jac(a, b)``: the overlap of two set numbers (``Pairs``), or None
    for "no store"; ``aux`` None: teacher rule off.  Returns ``(scores, ids, aux_out, counts, overlap, reason)`` as the
    entry point writes them (``aux_out`` all NaN without ``aux``)."""
    rank_scores = np.asarray(rank_scores, np.float32)
    rank_ids = np.asarray(rank_ids, np.int64)
    nq, k = rank_ids.shape
    out_s = np.full((nq, k), NEG_PAD, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    out_a = np.full((nq, k), np.nan, np.float32)
    counts = np.zeros(nq, np.int32)
    overlap = np.zeros((nq, k), np.float64)
    reason = np.zeros((nq, k), np.uint8)
    for q in range(nq):
        pos = [int(r) for r in pos_rows[pos_lims[q]:pos_lims[q + 1]]]
        n = 0
        for r in range(k):
            row = int(rank_ids[q, r])
            if row == -1:
                break
            o = 0.0
            if jac is not None:
                for p in pos:
                    o = max(o, jac(row, p))
            why = 0
            if jac is not None and o > overlap_threshold:
                why |= 1
            if aux is not None and float(aux[q, r]) >= aux_threshold:      # float(): the comparison is in fp64
                why |= 2
            overlap[q, r], reason[q, r] = o, why
            if why == 0:
                out_s[q, n], out_i[q, n] = rank_scores[q, r], row
                if aux is not None:
                    out_a[q, n] = aux[q, r]
                n += 1
        counts[q] = n
    return out_s, out_i, out_a, counts, overlap, reason


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, ref, what=""):
    """ids and counts and reasons exactly, scores / aux / overlaps by their bits; a ``None`` on either side is skipped"""
    names = ("scores", "ids", "aux", "counts", "overlap", "reason")
    for name, g, r in zip(names, got, ref):
        if g is None or r is None:
            continue
        g = np.asarray(g)
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape)
        if g.dtype.kind == "f":
            assert np.array_equal(bits(g), bits(r)), (what, name, np.argwhere(bits(g) != bits(r))[:5])
        else:
            assert np.array_equal(g, r), (what, name, np.argwhere(g != r)[:5])


# ---------------------------------------------------------------------------------------------------------------------
# texts
# ---------------------------------------------------------------------------------------------------------------------
_WORDS = ("retrieval", "Dense", "passage", "İstanbul", "Straße", "groß", "ＦＵＬＬ", "naïve", "café", "日本語", "検索",
          "文書", "tab\tbed", "the", "of", "a", "Query", "MODEL", "ǅungla", "ΣΊΣΥΦΟΣ", "x", "to", "hard", "negative")


@lru_cache(maxsize=None)
def texts(n=120, seed=701):
    """Short texts over ASCII, ``İ`` / ``ß`` (lower() changes their length or not), combining marks, CJK and tabs; some
    empty, blank, or shorter than three characters; one of 6 000 characters over 64 symbols (more than 4 096 distinct
    3-grams: the route that searches a positive where it lies)."""
    rng = np.random.default_rng(seed)
    out = ["", "   ", "\t\n", "a", "ab", " ab ", "abc", "ABC ", "İ", "İİ", "ßßß", "aaa", "aaaa"]
    while len(out) < n - 1:
        k = int(rng.integers(1, 14))
        t = " ".join(_WORDS[int(i)] for i in rng.integers(0, len(_WORDS), k))
        if rng.random() < 0.2:
            t = "  " + t + "\t "
        out.append(t)
    symbols = [chr(c) for c in range(0x21, 0x21 + 64)]
    out.append("".join(symbols[int(i)] for i in rng.integers(0, 64, 6000)))
    return tuple(out)


def text_pairs():
    """the pairs of the golden file: every text with itself, its neighbour and a few random partners, and one-word edits"""
    t = texts()
    rng = np.random.default_rng(702)
    pairs = [(a, a) for a in t[:40]] + [(t[i], t[i + 1]) for i in range(len(t) - 2)]
    pairs += [(t[int(i)], t[int(j)]) for i, j in rng.integers(0, len(t) - 1, (150, 2))]
    for a in t[13:60]:
        words = a.split(" ")
        words[int(rng.integers(0, len(words)))] = "edit"
        pairs.append((a, " ".join(words)))
        pairs.append((a.upper(), "  " + a))
    return pairs


# ---------------------------------------------------------------------------------------------------------------------
# key-set families (no texts: exact sizes)
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 63, 64, 65, 4095, 4096, 4097, 6011)


def _keys(rng, n, lo=0):
    """n distinct keys as a key of three code points would look (below 2^63), ascending"""
    k = np.unique(rng.integers(lo, lo + (1 << 40), int(n * 1.1) + 8, dtype=np.int64).astype(np.uint64))
    assert k.size >= n
    return np.sort(rng.choice(k, n, replace=False))


@lru_cache(maxsize=None)
def sized_sets():
    """For every size s of SIZES three sets: a random one, an identical copy, and one sharing about half of it; then for
    every size a set disjoint from all others (keys from a separate range), then for every size a subset of that size
    of the largest random set (lists of different lengths that share keys).  Returns a tuple of uint64 arrays; sets
    ``3 i``, ``3 len(SIZES) + i`` and ``4 len(SIZES) + i`` have exactly ``SIZES[i]`` keys."""
    rng = np.random.default_rng(711)
    sets = []
    for s in SIZES:
        a = _keys(rng, s)
        half = rng.choice(a, s // 2, replace=False) if s else a
        other = _keys(rng, s - s // 2, lo=1 << 41)
        sets += [a, a.copy(), np.unique(np.concatenate([half, other]))]
    for s in SIZES:
        sets.append(_keys(rng, s, lo=(1 << 50) + (len(sets) << 42)))
    largest = sets[3 * (len(SIZES) - 1)]
    for s in SIZES:
        sets.append(np.sort(rng.choice(largest, s, replace=False)))
    for a in sets:
        a.setflags(write=False)
        assert (np.diff(a.astype(np.int64)) > 0).all()
    return tuple(sets)


@lru_cache(maxsize=None)
def family(n_small=400, seed=721):
    """The store of the ranking cases: ``n_small`` sets of 4 to 40 keys in 40 families (members of a family share most
    keys, so overlaps spread over (0, 1]), followed by the sets of ``sized_sets`` from size 4 095 up (positives and
    candidates longer than the LDS cap, and their copies).  Set 0 and set 1 are built for the threshold's edge:
    |set 0| = 5, set 1 = four of its keys, jaccard = 4 / 5.  Set 2 is empty.  Returns ``(sets, pairs)``."""
    rng = np.random.default_rng(seed)
    bases = [_keys(rng, 40, lo=f << 42) for f in range(40)]
    sets = []
    for i in range(n_small):
        base = bases[i % 40]
        m = int(rng.integers(4, 41))
        keep = np.sort(rng.choice(base, m, replace=False))
        if rng.random() < 0.5:
            keep = np.unique(np.concatenate([keep, _keys(rng, int(rng.integers(1, 6)), lo=(41 + i) << 42)]))
        sets.append(keep)
    edge = np.sort(bases[0][:5])
    sets[0], sets[1], sets[2] = edge, edge[:4].copy(), np.zeros(0, np.uint64)
    big = [s for s in sized_sets() if len(s) >= 4095]
    sets += big
    for a in sets:
        a.setflags(write=False)
    return tuple(sets), Pairs(sets)


def big_rows():
    """set numbers of ``family`` that exceed the LDS cap"""
    sets, _ = family()
    return [i for i, s in enumerate(sets) if len(s) > LDS_CAP]


@lru_cache(maxsize=None)
def ranking_case(nq, search_k, n_pos, seed=731):
    """A window over ``family``: random set numbers (repeats allowed - the rule is per rank), scores descending, and
    per query ``n_pos`` positives (random order, every third query one out of range, one of them longer than the LDS
    cap when ``n_pos >= 3``).  Sprinkled in: ids outside the store (too large, negative but not -1), a candidate that
    is a positive, and per query kind an early -1 (kind 1) or an all -1 window (kind 2, from query 2 on).  ``aux``
    float32 ``[nq, search_k]`` in [0, 1) with NaNs.  Returns ``(rank_scores, rank_ids, pos_lims, pos_rows, aux)``."""
    sets, _ = family()
    n = len(sets)
    rng = np.random.default_rng(seed + 1000 * nq + 10 * search_k + n_pos)
    ids = rng.integers(0, n, (nq, search_k)).astype(np.int64)
    scores = np.sort(rng.random((nq, search_k)).astype(np.float32), axis=1)[:, ::-1].copy()
    big = big_rows()
    lists = []
    for q in range(nq):
        pos = rng.integers(0, n, n_pos).tolist()
        if n_pos >= 3:
            pos[1] = big[q % len(big)]
        if n_pos and q % 3 == 2:
            pos[0] = n + 3
        lists.append(pos)
        # members of the positives' families, the positive itself, ids outside the store
        for j in range(0, search_k, 7):
            if pos and rng.random() < 0.6:
                p = pos[int(rng.integers(0, len(pos)))]
                ids[q, j] = (p % 40) + 40 * int(rng.integers(0, 10)) if p < 400 else p
        if search_k > 2:
            ids[q, search_k // 2] = n + 11
            ids[q, search_k // 3] = -7
            if pos:
                ids[q, search_k - 1] = pos[-1]
        if q % 4 == 1:
            ids[q, (search_k * 2) // 3:] = -1
        if q % 4 == 2 and q > 1:
            ids[q, :] = -1
    lims = np.zeros(nq + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=lims[1:])
    rows = np.array([r for x in lists for r in x], np.int32)
    aux = rng.random((nq, search_k)).astype(np.float32)
    aux[rng.random((nq, search_k)) < 0.1] = np.nan
    for a in (scores, ids, lims, rows, aux):
        a.setflags(write=False)
    return scores, ids, lims, rows, aux


# ---------------------------------------------------------------------------------------------------------------------
# the case the feature exists for: near-copies of the positives in the corpus
# ---------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def copies_case(n=300, nq=30, dim=384, seed=741):
    """300 short texts; 30 of them (rows 270 .. 299) are one-word edits of the positives of queries 0 .. 29 (positive of
    query q = row q).  Embeddings are given directly: random unit rows, each copy = its positive's vector plus small
    noise, each query = its positive's vector plus noise - so a copy ranks next to the positive and within any
    margin of it.  Returns ``(texts, corpus, queries, positives, copy_of)``, ``copy_of[q]`` = the row holding the copy."""
    rng = np.random.default_rng(seed)
    vocab = [f"w{i:03d}" for i in range(500)]
    docs = [" ".join(vocab[int(i)] for i in rng.integers(0, 500, 40)) for _ in range(n - nq)]
    copy_of = {}
    for q in range(nq):
        words = docs[q].split(" ")
        words[int(rng.integers(0, len(words)))] = "edited"
        copy_of[q] = len(docs)
        docs.append(" ".join(words))

    def unit(x):
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)

    corpus = unit(rng.standard_normal((n, dim)))
    for q in range(nq):
        corpus[copy_of[q]] = unit(corpus[q][None] + 0.05 * unit(rng.standard_normal((1, dim))))[0]
    queries = unit(corpus[:nq] + 0.3 * unit(rng.standard_normal((nq, dim))))
    corpus.setflags(write=False)
    queries.setflags(write=False)
    return tuple(docs), corpus, queries, [[q] for q in range(nq)], copy_of
