"""Near-duplicate clusters: case builders and the plain-Python restatement of the clustering rule (no GPU, no package code).

The rule (``include/sskd_amd.h``, near-duplicate clusters): rows that take part are vertices, an edge ``(i, j)``, ``i < j``,
counts when both rows take part and the scope rule over the row groups holds; a cluster is a connected component, its
label the smallest row; ``keep`` 0 keeps that row, ``keep`` 1 the row with the largest degree, ties to the smallest row.
``restate`` says that with a textbook union-find; ``reach`` says it again by brute-force reachability for tiny graphs.
"""
import itertools

import numpy as np


def scope_allows(scope, groups, i, j):
    """0: every pair, 1: only pairs of different groups, 2: only pairs of one group."""
    if scope == 0:
        return True
    return (groups[i] != groups[j]) if scope == 1 else (groups[i] == groups[j])


def restate(n, edges, take=None, groups=None, scope=0, keep=0):
    """``edges``: (i, j) row pairs, each listing counted once.  Returns int64 arrays ``parent`` (the smallest row of the
    row's component, -1 for a row that takes no part), ``degree``, ``rep``, ``size`` and ``counts`` = [components, rows]."""
    take = np.ones(n, dtype=bool) if take is None else np.asarray(take, dtype=bool)
    up = list(range(n))
    degree = [0] * n

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    for i, j in edges:
        i, j = int(i), int(j)
        if i == j or not (take[i] and take[j]) or not scope_allows(scope, groups, i, j):
            continue
        degree[i] += 1
        degree[j] += 1
        a, b = find(i), find(j)
        if a != b:
            up[max(a, b)] = min(a, b)
    parent = np.array([find(r) if take[r] else -1 for r in range(n)], dtype=np.int64)
    size = np.zeros(n, dtype=np.int64)
    rep = np.full(n, -1, dtype=np.int64)
    best = {}
    for r in range(n):
        if parent[r] < 0:
            continue
        root = int(parent[r])
        size[root] += 1
        if root not in best or (keep == 1 and degree[r] > degree[best[root]]):
            best[root] = r   # rows ascend: the first row of a component is its smallest, a tie keeps the earlier row
    for r in range(n):
        if parent[r] >= 0:
            rep[r] = best[int(parent[r])]
    counts = np.array([int((size > 0).sum()), int(take.sum())], dtype=np.int64)
    return {"parent": parent, "degree": np.array(degree, dtype=np.int64), "rep": rep, "size": size, "counts": counts}


def reach(n, edges, take=None, groups=None, scope=0, keep=0):
    """The same outputs from the transitive closure of the adjacency matrix (n <= 12 or so)."""
    take = np.ones(n, dtype=bool) if take is None else np.asarray(take, dtype=bool)
    adj = np.zeros((n, n), dtype=np.int64)
    degree = np.zeros(n, dtype=np.int64)
    for i, j in edges:
        if i != j and take[i] and take[j] and scope_allows(scope, groups, i, j):
            adj[i, j] = adj[j, i] = 1
            degree[i] += 1
            degree[j] += 1
    closure = ((adj + np.eye(n, dtype=np.int64)) > 0)
    for _ in range(max(n, 1)):
        closure = (closure.astype(np.int64) @ closure.astype(np.int64)) > 0
    parent = np.full(n, -1, dtype=np.int64)
    rep = np.full(n, -1, dtype=np.int64)
    size = np.zeros(n, dtype=np.int64)
    for r in range(n):
        if not take[r]:
            continue
        members = [m for m in range(n) if closure[r, m] and take[m]]
        parent[r] = min(members)
        if parent[r] == r:
            size[r] = len(members)
        rep[r] = min(members) if keep == 0 else min(members, key=lambda m: (-degree[m], m))
    counts = np.array([int((size > 0).sum()), int(take.sum())], dtype=np.int64)
    return {"parent": parent, "degree": degree, "rep": rep, "size": size, "counts": counts}


def all_graphs(n):
    """Every simple graph on ``n`` vertices as an edge list."""
    pairs = list(itertools.combinations(range(n), 2))
    for bits in range(1 << len(pairs)):
        yield [p for k, p in enumerate(pairs) if bits >> k & 1]


def random_graph(rng, n_max=12):
    """(n, edges, take, groups): a random graph with repeated edges, some rows out, three groups."""
    n = int(rng.integers(1, n_max + 1))
    m = int(rng.integers(0, 2 * n + 1))
    edges = [(int(a), int(b)) for a, b in rng.integers(0, n, size=(m, 2))]
    edges = [(min(a, b), max(a, b)) for a, b in edges if a != b]
    take = rng.random(n) > 0.2
    groups = rng.integers(0, 3, size=n)
    return n, edges, take, groups


# ----------------------------------------------------------------- CSR edge lists for sskd_dup_link
def csr_of(rows, lists):
    """(lims int64 [len(rows) + 1], ids int64) of one link call: ``lists[k]`` = the ids of query ``rows[k]``."""
    lims = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=lims[1:])
    ids = np.array([v for x in lists for v in x], dtype=np.int64)
    return lims, ids


def upper_csr(n, edges, lo=0, hi=None, id_offset=0):
    """Rows [lo, hi) as queries, each listing its larger neighbours (ascending), as ids."""
    hi = n if hi is None else hi
    lists = [[] for _ in range(hi - lo)]
    for i, j in edges:
        i, j = min(i, j), max(i, j)
        if lo <= i < hi:
            lists[i - lo].append(j + id_offset)
    for x in lists:
        x.sort()
    return csr_of(range(lo, hi), lists)


def symmetric_csr(n, edges, lo=0, hi=None, id_offset=0, descending=False):
    """What a self-join returns: rows [lo, hi) as queries, each listing itself and ALL its neighbours."""
    hi = n if hi is None else hi
    lists = [[r + id_offset] for r in range(lo, hi)]
    for i, j in edges:
        if lo <= i < hi:
            lists[i - lo].append(j + id_offset)
        if lo <= j < hi:
            lists[j - lo].append(i + id_offset)
    for x in lists:
        x.sort(reverse=descending)
    return csr_of(range(lo, hi), lists)


def edges_of_csr(lims, ids, query_row0, id_offset, n):
    """The entries of a link call that are edges as far as the rows go: j in [0, n), j > i.  One tuple per listing."""
    out = []
    for q in range(len(lims) - 1):
        i = query_row0 + q
        for t in range(int(lims[q]), int(lims[q + 1])):
            j = int(ids[t]) - id_offset
            if i < j < n:
                out.append((i, j))
    return out


def path_edges(n):
    return [(k, k + 1) for k in range(n - 1)]


def star_edges(hub, n):
    return [(min(hub, r), max(hub, r)) for r in range(n) if r != hub]


def clique_edges(rows):
    return list(itertools.combinations(sorted(rows), 2))


def relabel(edges, perm):
    return [(min(int(perm[a]), int(perm[b])), max(int(perm[a]), int(perm[b]))) for a, b in edges]


def sparse_graph(n=20000, m=60000, seed=20240917):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(np.sort(e, axis=1), axis=0)   # a self-join lists a pair once
    return [tuple(x) for x in e.tolist()]


# ----------------------------------------------------------------- the end-to-end corpus
E2E_THRESHOLD = 0.9
E2E_DIM = 384


def e2e_corpus(seed=4242, n_originals=560, chain=16):
    """Unit rows: ``n_originals`` well-separated random vectors (|cos| < 0.3 at 384 dimensions), each with 0 .. 7 noisy
    copies at cosine ~0.9998, and one chain of ``chain`` vectors stepped 0.2 rad along a great circle - neighbours score
    cos 0.2 = 0.98 and cos 0.4 = 0.92, both above the threshold 0.9, rows three steps apart cos 0.6 = 0.83 and the two
    ends cos 3.0 < 0, below it.  The rows are shuffled, so clusters straddle the batches.  Returns ``(rows float32 [n,
    384], family int32 [n])``: family = the original a row copies (the chain is one family)."""
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    originals = unit(rng.standard_normal((n_originals, E2E_DIM)))
    rows, family = [], []
    for k in range(n_originals):
        rows.append(originals[k])
        family.append(k)
        for _ in range(int(rng.integers(0, 8))):
            rows.append(unit(originals[k] + 0.02 * unit(rng.standard_normal(E2E_DIM))))
            family.append(k)
    e1 = unit(rng.standard_normal(E2E_DIM))
    e2 = rng.standard_normal(E2E_DIM)
    e2 = unit(e2 - (e2 @ e1) * e1)
    for s in range(chain):
        rows.append(np.cos(0.2 * s) * e1 + np.sin(0.2 * s) * e2)
        family.append(n_originals)
    rows, family = np.asarray(rows, dtype=np.float64), np.asarray(family, dtype=np.int32)
    order = rng.permutation(len(rows))
    return np.ascontiguousarray(rows[order], dtype=np.float32), np.ascontiguousarray(family[order])
