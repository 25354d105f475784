"""``DiverseIndex`` on the MI355X: over every dense first stage it equals the checker (``mmr_cases``) applied to that
stage's own ``fetch_k`` ranking - ids exact, scores, mmr and red by bit pattern.

One world, built once: the clustered family at 60 centres x 20 copies and its 8 queries, each between two centres -
1 200 unit rows under the inner product, so the index holds the rows bit for bit as the checker reads them and the
scores are cosines all the same."""
import numpy as np
import pytest
import torch

import mmr_cases as mc
from oracle import search as oracle
from semantic_search_kd_amd import (DiverseIndex, Diversity, ExpandedIndex, FAISSIndexBuilder, GraphIndex, IVFIndex,
                                    QueryExpansion)

pytestmark = pytest.mark.gpu

N = 1200


class World:
    def __init__(self, device):
        self.device = device
        self.rows, self.row_c, self.queries = mc.clustered_family(centres=60, copies=20)
        assert self.rows.shape == (N, 384)
        self.d_q = torch.from_numpy(self.queries).to(device)
        self.flat = self.new_flat()
        self.gram = oracle.scores_fma(self.rows, self.rows)       # computed once, shared, never written
        self.gram.setflags(write=False)

    def new_flat(self, **kw):
        flat = FAISSIndexBuilder(embedding_dim=384, metric="ip", device=str(self.device), **kw)
        flat.build_from_embeddings(self.rows)
        flat.doc_ids = [f"d{i}" for i in range(N)]
        return flat

    def want(self, stage, d: Diversity, k, id_offset=0, **kw):
        """The checker over ``stage``'s own ranking at the depth ``DiverseIndex`` fetches."""
        S, I = (t.cpu().numpy() for t in stage.search_device(self.d_q, d.depth(k), **kw)[:2])
        I = np.where(I < 0, I, I - id_offset)
        return mc.mmr_batch(S, I, self.rows, gram=self.gram, k=k, lam=d.lambda_mult, dup_threshold=d.threshold(),
                            id_offset=id_offset)


@pytest.fixture(scope="module")
def world(gpu):
    return World(gpu)


def _host(out):
    return tuple(t.cpu().numpy() for t in out)


SETTINGS = (Diversity(), Diversity(lambda_mult=0.3, fetch_k=33, dup_threshold=0.8), Diversity(lambda_mult=1.0, fetch_k=5))


def test_flat_index_equals_the_checker(world):
    w = world
    for d in SETTINGS:
        div = DiverseIndex(w.flat, d)
        for k in (1, 10):
            want = w.want(w.flat, d, k)
            got = _host(div.search_detailed_device(w.d_q, k))
            mc.same(got, want, f"flat {d} k={k}")
            D, I = div.search(w.queries, k)                       # search and search_device agree
            D2, I2 = _host(div.search_device(w.d_q, k))
            assert np.array_equal(I, I2) and np.array_equal(I, want[1]) and np.array_equal(mc.bits32(D), mc.bits32(D2))
            mc.same(div.search_detailed(w.queries, k), want, f"flat, NumPy form {d} k={k}")
    plain = w.flat.search(w.queries, 10)[1]
    got = DiverseIndex(w.flat).search(w.queries, 10)[1]
    for q in range(8):                                            # it does diversify: one cluster becomes three or more
        assert len(set(w.row_c[plain[q]])) == 1 and len(set(w.row_c[got[q]])) >= 3
    short = DiverseIndex(w.flat, SETTINGS[1]).search_detailed(w.queries, 10)
    assert (short[4] < 10).all() and (short[1][:, -1] == -1).all()
    # k above fetch_k fetches k; one [384] vector is one query
    d = Diversity(fetch_k=5)
    mc.same(_host(DiverseIndex(w.flat, d).search_detailed_device(w.d_q, 20)), w.want(w.flat, d, 20), "k > fetch_k")
    one = DiverseIndex(w.flat).search(w.queries[3], 10)
    assert one[1].shape == (1, 10) and np.array_equal(one[1][0], got[3])
    assert DiverseIndex(w.flat).ntotal == N and DiverseIndex(w.flat).doc_ids[5] == "d5"


def test_ivf_with_every_list_probed_equals_the_checker(world):
    w = world
    ivf = IVFIndex(flat=w.flat)
    ivf.train(nlist=8, iterations=3)
    for d in SETTINGS[:2]:
        want = w.want(ivf, d, 10, nprobe=8)
        mc.same(_host(DiverseIndex(ivf, d).search_detailed_device(w.d_q, 10, nprobe=8)), want, f"ivf {d}")
        mc.same(want, w.want(w.flat, d, 10), "ivf, nprobe = nlist, is the exact ranking")
    d = SETTINGS[0]
    mc.same(_host(DiverseIndex(ivf, d).search_detailed_device(w.d_q, 10, nprobe=2)), w.want(ivf, d, 10, nprobe=2),
            "ivf, nprobe = 2")


def test_graph_equals_the_checker_over_its_own_ranking(world):
    w = world
    graph = GraphIndex(flat=w.flat, M=16)
    graph.build_graph()
    d = Diversity(fetch_k=40, dup_threshold=0.9)
    mc.same(_host(DiverseIndex(graph, d).search_detailed_device(w.d_q, 10, ef=64)), w.want(graph, d, 10, ef=64), "graph")


def test_expanded_flat_equals_the_checker_over_the_expanded_ranking(world):
    w = world
    e = ExpandedIndex(w.flat, QueryExpansion(fb_docs=3))
    assert e.kind == "dense"
    for d in SETTINGS[:2]:
        div = DiverseIndex(e, d)
        mc.same(_host(div.search_detailed_device(w.d_q, 10)), w.want(e, d, 10), f"expanded flat {d}")
    assert div.ntotal == N and div.doc_ids is w.flat.doc_ids


def test_allow_and_removed_rows_never_appear(world):
    w = world
    flat = w.new_flat()
    d = Diversity(lambda_mult=0.4, fetch_k=40)
    div = DiverseIndex(flat, d)
    allow = np.ones(N, bool)
    allow[::3] = False
    got = _host(div.search_detailed_device(w.d_q, 10, allow=flat.row_filter(allow)))
    mc.same(got, w.want(flat, d, 10, allow=flat.row_filter(allow)), "allow")
    assert allow[got[1][got[1] >= 0]].all()
    best = w.flat.search(w.queries, 2)[1]
    assert div.remove_ids(np.unique(best)) == np.unique(best).size
    got = _host(div.search_detailed_device(w.d_q, 10))
    mc.same(got, w.want(flat, d, 10), "removed")
    assert not np.isin(got[1], best).any()
    both = div.search(w.queries, 10, allow=allow)[1]
    assert allow[both[both >= 0]].all() and not np.isin(both, best).any()


def test_flat_index_with_an_id_offset_returns_offset_ids(world):
    w = world
    flat = w.new_flat(id_offset=50_000)
    d = Diversity(dup_threshold=0.8)
    got = _host(DiverseIndex(flat, d).search_detailed_device(w.d_q, 10))
    want = w.want(flat, d, 10, id_offset=50_000)
    mc.same(got, want, "id_offset")
    base = w.want(w.flat, d, 10)
    assert np.array_equal(got[1], np.where(base[1] < 0, -1, base[1] + 50_000))
    assert (got[1][got[1] >= 0] >= 50_000).all()


def test_captured_search_replays_to_the_eager_result(world):
    w = world
    div = DiverseIndex(w.flat, Diversity(dup_threshold=0.97))
    static_q = w.d_q.clone()
    eager = div.search_device(static_q, 10)                      # also sizes the workspace before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            D, I = div.search_device(static_q, 10)
    torch.cuda.current_stream().wait_stream(side)
    D.fill_(0)
    I.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(I, eager[1]) and torch.equal(D.view(torch.int32), eager[0].view(torch.int32))


def test_search_route_with_the_flag_set_returns_the_diversified_ranking(world):
    """/search over a real flat index (the student is a stand-in that returns a family query): with the flag set the
    response is ``DiverseIndex``'s result, wrapped outermost around the query expansion when that is on too; with it
    unset the response is the plain ranking."""
    from unittest.mock import MagicMock

    from fastapi.testclient import TestClient

    from semantic_search_kd_amd.serve import app as app_module
    from semantic_search_kd_amd.serve.app import ServeSettings, app_state, create_app

    w = world
    emb = w.queries[2:3]

    def serve(**flags):
        for key, value in vars(app_module.AppState()).items():
            setattr(app_state, key, value)
        try:
            student = MagicMock()
            student.embedding_dim = 384
            student.encode_queries.return_value = emb
            app_state.student = student
            with TestClient(create_app(settings=ServeSettings(environment="test", **flags))) as client:
                app_state.index_builder, app_state.doc_ids = w.flat, w.flat.doc_ids
                r = client.post("/search", json={"query": "anything", "k": 10})
                assert r.status_code == 200, r.text
                body = r.json()
                return [x["doc_id"] for x in body["results"]], np.array([x["score"] for x in body["results"]], np.float32)
        finally:
            for key, value in vars(app_module.AppState()).items():
                setattr(app_state, key, value)

    d = Diversity(lambda_mult=0.4, fetch_k=40, dup_threshold=0.9)
    flags = dict(diversity_enabled=True, diversity_lambda=0.4, diversity_fetch_k=40, diversity_dup_threshold=0.9)
    D, I = DiverseIndex(w.flat, d).search(emb, 10)
    n = int((I[0] >= 0).sum())
    assert 2 <= n < 10                 # 40 candidates span two clusters of 20 or more: the cut-off shortens the response
    ids, scores = serve(**flags)
    assert ids == [f"d{r}" for r in I[0, :n]] and np.array_equal(mc.bits32(scores), mc.bits32(D[0, :n]))
    plain_ids, _ = serve()
    assert plain_ids == [f"d{r}" for r in w.flat.search(emb, 10)[1][0]] and plain_ids != ids
    x = QueryExpansion(fb_docs=3)
    D, I = DiverseIndex(ExpandedIndex(w.flat, x), d).search(emb, 10)
    ids, scores = serve(query_expansion_enabled=True, expansion_fb_docs=3, **flags)
    n = int((I[0] >= 0).sum())
    assert ids == [f"d{r}" for r in I[0, :n]] and np.array_equal(mc.bits32(scores), mc.bits32(D[0, :n]))
