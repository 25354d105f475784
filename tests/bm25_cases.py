"""The checker of the BM25 index: BM25Okapi restated with dicts and loops in fp64, and the corpora the tests run on.

Written from the definition, not from the product code (which inverts the corpus with NumPy and scores on the GPU):

    idf(w)       = log(N - n_w + 0.5) - log(n_w + 0.5)                       n_w = documents containing w
    average_idf  = (idf summed left to right over the words in order of first appearance) / distinct words
    idf(w) < 0  -> epsilon * average_idf
    score(q, d)  = sum over the tokens t of q, in order, repeats counted again, of
                   idf(t) * (f * (k1 + 1) / (f + k1 * (1 - b + b * dl_d / avgdl)))      f = count of t in d
    ranking      = sorted(range(N), key=score, reverse=True)[:top_k]        (score descending, ties by ascending row)

Python floats are IEEE fp64 and every operation above is rounded once, so the values are the ones NumPy's elementwise
expression gives.  A token outside the vocabulary adds nothing; a document without the token adds idf * 0.0, which
never changes a sum that started at +0.0.
"""
import math
import random

K1, B, EPSILON = 1.5, 0.75, 0.25

# the reference test's corpus (its tests/test_bm25.py, data)
FIVE_SENTENCES = [
    "Machine learning is a subset of artificial intelligence.",
    "Deep learning uses neural networks with many layers.",
    "Natural language processing helps computers understand text.",
    "Computer vision enables machines to interpret images.",
    "Reinforcement learning trains agents through rewards.",
]


def tokenize(text):
    return text.lower().split()


class Oracle:
    def __init__(self, corpus, k1=K1, b=B, epsilon=EPSILON):
        """``corpus``: token lists."""
        self.k1, self.b, self.epsilon = k1, b, epsilon
        self.n = len(corpus)
        self.doc_len = [len(d) for d in corpus]
        self.avgdl = sum(self.doc_len) / self.n          # (ints: exact)
        self.postings = {}                               # word -> {row: f}, words in order of first appearance
        for row, doc in enumerate(corpus):
            for word in doc:
                rows = self.postings.setdefault(word, {})
                rows[row] = rows.get(row, 0) + 1
        self.idf = {}
        idf_sum = 0
        negative = []
        for word, rows in self.postings.items():
            n_w = len(rows)
            idf = math.log(self.n - n_w + 0.5) - math.log(n_w + 0.5)
            self.idf[word] = idf
            idf_sum += idf
            if idf < 0:
                negative.append(word)
        self.raw_idf = dict(self.idf)
        self.average_idf = idf_sum / len(self.idf) if self.idf else 0.0
        for word in negative:
            self.idf[word] = epsilon * self.average_idf

    def weight(self, f, row):
        k1, b = self.k1, self.b
        return f * (k1 + 1) / (f + k1 * (1 - b + b * self.doc_len[row] / self.avgdl))

    def scores(self, tokens):
        score = [0.0] * self.n
        for t in tokens:
            if t not in self.idf:
                continue
            idf = self.idf[t]
            for row, f in self.postings[t].items():
                score[row] = score[row] + idf * self.weight(f, row)
        return score

    def rank(self, scores, top_k):
        top = sorted(range(self.n), key=lambda i: scores[i], reverse=True)[:top_k]
        return top, [scores[i] for i in top]

    def search(self, text, top_k):
        return self.rank(self.scores(tokenize(text)), top_k)


def zipf_corpus(n_docs, vocab, seed, min_len=1, max_len=30):
    """``n_docs`` texts of ``min_len`` .. ``max_len`` words drawn from ``w0 .. w{vocab-1}`` with p(rank r) ~ 1 / (r + 1)."""
    rng = random.Random(seed)
    words = [f"w{r}" for r in range(vocab)]
    cum, total = [], 0.0
    for r in range(vocab):
        total += 1.0 / (r + 1)
        cum.append(total)
    docs = []
    for _ in range(n_docs):
        n = rng.randint(min_len, max_len)
        docs.append(" ".join(rng.choices(words, cum_weights=cum, k=n)))
    return docs


def zipf_query(vocab, n_tokens, seed):
    return zipf_corpus(1, vocab, seed, n_tokens, n_tokens)[0]


def float_bits(x):
    import struct

    return struct.unpack("<q", struct.pack("<d", x))[0]
