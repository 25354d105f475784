"""The checker of query expansion: the two rules of include/sskd_amd.h ("Query expansion") restated on the host, and the
corpora the tests run on.

Written from the definition, not from the product code (two HIP kernels behind ``expand.py``, a NumPy forward-index
builder in ``bm25.py``).

Rocchio, in NumPy float32 operations (each elementwise product and sum is rounded once, nothing is fused):

    feedback rows   the first fb_docs entries of the ranking up to the first id -1, ids outside [0, n_rows) skipped; m
    m == 0          the query comes back bit for bit
    uniform         b_i = beta / float32(m)
    score           s+_i = s_i if s_i > 0 else +0.0;  S = s+_1 + s+_2 + ... from +0.0;  S == 0 -> uniform;
                    b_i = beta * (s+_i / S)
    result          acc = alpha * q, then acc = acc + b_i * row_i in rank order

RM3, in Python floats (IEEE fp64, every operation rounded once) over ``bm25_cases.Oracle``:

    forward index   per row the distinct terms with p = tf / dl; at most 256 per row, largest tf first, ties to the lower
                    term id (term ids number the words in order of first appearance)
    feedback rows   the BM25 ranking up to the first id -1, skipping ids outside [0, n_rows), scores == 0.0 and rows the
                    mask hides; the first fb_docs survivors
    weights         S = s_1 + s_2 + ... from +0.0;  P_d = s_d / S;  w(t) = sum in rank order from +0.0 of p(t, d) * P_d
    candidates      terms of the feedback rows that are not among the query's tokens, df <= max_df when max_df > 0
    selection       the best fb_terms under (w descending, term id ascending)
    expanded query  the query's tokens orig_repeat times, then the selected words
"""
import random
from collections import Counter

import numpy as np

from bm25_cases import Oracle, float_bits, tokenize   # noqa: F401  (re-exported for the tests)

F32 = np.float32
ROW_TERMS = 256


# ---------------------------------------------------------------------------------------------------- Rocchio
def rocchio_query(q, scores, ids, rows, *, fb_docs, alpha, beta, weighting):
    """One query: ``q`` fp32 [dim], its ranking, the index rows fp32 [n, dim].  Returns ``(fp32 [dim], m)``."""
    q = np.asarray(q, F32)
    n_rows = rows.shape[0]
    fb = []
    for s, r in list(zip(scores, ids))[:fb_docs]:
        r = int(r)
        if r == -1:
            break
        if r < 0 or r >= n_rows:
            continue
        fb.append((F32(s), r))
    m = len(fb)
    if m == 0:
        return q.copy(), 0
    alpha, beta = F32(alpha), F32(beta)
    uniform = weighting == "uniform"
    if not uniform:
        plus = [s if s > 0 else F32(0.0) for s, _ in fb]
        total = F32(0.0)
        for s in plus:
            total = F32(total + s)
        if total == 0:
            uniform = True
    if uniform:
        b = [F32(beta / F32(m))] * m
    else:
        b = [F32(beta * F32(s / total)) for s in plus]
    acc = (alpha * q).astype(F32)
    for b_i, (_, r) in zip(b, fb):
        acc = (acc + (b_i * np.asarray(rows[r], F32)).astype(F32)).astype(F32)
    return acc, m


def rocchio_batch(Q, S, I, rows, **kw):
    out = [rocchio_query(Q[i], S[i], I[i], rows, **kw) for i in range(len(Q))]
    return (np.stack([o[0] for o in out]).astype(F32).reshape(len(Q), -1) if out else np.zeros((0, rows.shape[1]), F32),
            np.array([o[1] for o in out], np.int32))


# ---------------------------------------------------------------------------------------------------- RM3
class Lexicon:
    """``Oracle`` plus what RM3 reads: term ids, per-row term counts, the forward index after its cut."""

    def __init__(self, corpus):
        """``corpus``: token lists."""
        self.oracle = Oracle(corpus)
        self.words = list(self.oracle.postings)                 # term id -> word, in order of first appearance
        self.term_id = {w: i for i, w in enumerate(self.words)}
        self.n = len(corpus)
        self.dl = [len(doc) for doc in corpus]
        self.tf = [Counter(self.term_id[w] for w in doc) for doc in corpus]
        self.fwd = []                                           # row -> {term: p}, ascending term ids
        for row, tf in enumerate(self.tf):
            kept = sorted(tf.items(), key=lambda e: (-e[1], e[0]))[:ROW_TERMS]
            self.fwd.append({t: f / self.dl[row] for t, f in sorted(kept)})

    def df(self, t):
        return len(self.oracle.postings[self.words[t]])

    def ids(self, tokens):
        return [self.term_id[w] for w in tokens if w in self.term_id]

    def feedback(self, rank_scores, rank_ids, fb_docs, allowed=None):
        fb = []
        for s, r in zip(rank_scores, rank_ids):
            s, r = float(s), int(r)
            if r == -1:
                break
            if r < 0 or r >= self.n or s == 0.0 or (allowed is not None and not allowed[r]):
                continue
            fb.append((s, r))
            if len(fb) == fb_docs:
                break
        return fb

    def select(self, tokens, rank_scores, rank_ids, *, fb_docs, fb_terms, max_df=0, allowed=None):
        """``(selected term ids, their weights, feedback rows used)`` for one query given as tokens."""
        own = set(self.ids(tokens))
        fb = self.feedback(rank_scores, rank_ids, fb_docs, allowed)
        total = 0.0
        for s, _ in fb:
            total = total + s
        w = {}
        for s, r in fb:
            p_d = s / total
            for t, p in self.fwd[r].items():
                if t in own or (max_df > 0 and self.df(t) > max_df):
                    continue
                w[t] = w.get(t, 0.0) + p * p_d
        chosen = sorted(w, key=lambda t: (-w[t], t))[:fb_terms]
        return chosen, [w[t] for t in chosen], len(fb)

    def segment(self, tokens, chosen, *, fb_terms, orig_repeat):
        """The CSR segment the kernel writes for the query."""
        return self.ids(tokens) * orig_repeat + list(chosen) + [-1] * (fb_terms - len(chosen))

    def expanded_tokens(self, tokens, chosen, *, orig_repeat):
        return [w for w in tokens if w in self.term_id] * orig_repeat + [self.words[t] for t in chosen]

    def expand_and_search(self, text, top_k, *, fb_docs, fb_terms, orig_repeat, max_df=0, kb=None, allowed=None):
        """Search at ``kb`` (default ``fb_docs``), expand, search again: ``(rows, scores, chosen, weights)``."""
        tokens = tokenize(text)
        rows, scores = self.oracle.rank(self.oracle.scores(tokens), fb_docs if kb is None else kb)
        chosen, weights, _ = self.select(tokens, scores, rows, fb_docs=fb_docs, fb_terms=fb_terms, max_df=max_df,
                                         allowed=allowed)
        again = self.oracle.scores(self.expanded_tokens(tokens, chosen, orig_repeat=orig_repeat))
        rows2, scores2 = self.oracle.rank(again, top_k)
        return rows2, scores2, chosen, weights


def pad_ranking(rows, scores, k):
    """A ranking of fewer than ``k`` rows as ``sskd_bm25_search`` pads it."""
    rows, scores = list(rows), list(scores)
    return rows + [-1] * (k - len(rows)), scores + [float("-inf")] * (k - len(scores))


# ---------------------------------------------------------------------------------------------------- corpora
def topical_corpus(seed, topics=16, per_topic=32, topic_words=40, min_len=8, max_len=24, p_topic=0.4, common_cap=200):
    """``(texts, topic of every text)``: a word is ``t{topic}_{0..39}`` with probability 0.4, otherwise a common word
    ``c{j}`` with j Pareto(1)-distributed, capped at 200."""
    rng = random.Random(seed)
    texts, topic_of = [], []
    for topic in range(topics):
        for _ in range(per_topic):
            words = []
            for _ in range(rng.randint(min_len, max_len)):
                if rng.random() < p_topic:
                    words.append(f"t{topic}_{rng.randrange(topic_words)}")
                else:
                    words.append(f"c{min(int(rng.paretovariate(1.0)) - 1, common_cap)}")
            texts.append(" ".join(words))
            topic_of.append(topic)
    return texts, topic_of


def topical_queries(seed, n=64, topics=16, topic_words=40):
    """``(texts, topic of every query)``: two words of one topic plus one of ``c0 .. c4``."""
    rng = random.Random(seed + 1000)
    queries, topic_of = [], []
    for i in range(n):
        topic = i % topics
        a, b = rng.sample(range(topic_words), 2)
        queries.append(f"t{topic}_{a} t{topic}_{b} c{rng.randrange(5)}")
        topic_of.append(topic)
    return queries, topic_of


def clustered_family(seed, centres=64, per_centre=32, dim=384, row_noise=1.0, query_noise=4.5, queries_per_centre=4):
    """``(rows fp32 unit, centre of every row, queries fp32 unit, centre of every query)``: rows = centre + N(0, I) *
    row_noise / sqrt(dim), queries = centre + N(0, I) * query_noise / sqrt(dim), all L2-normalised."""
    g = np.random.default_rng(seed)

    def unit(x):
        return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)

    c = unit(g.standard_normal((centres, dim)))
    row_c = np.repeat(np.arange(centres), per_centre)
    rows = unit(c[row_c] + g.standard_normal((row_c.size, dim)) * (row_noise / np.sqrt(dim)))
    q_c = np.repeat(np.arange(centres), queries_per_centre)
    queries = unit(c[q_c] + g.standard_normal((q_c.size, dim)) * (query_noise / np.sqrt(dim)))
    return rows, row_c, queries, q_c


def bits32(x):
    return np.ascontiguousarray(x, F32).view(np.int32)


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)
