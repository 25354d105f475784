"""The compressed token store through ``LateInteractionIndex``, ``build_index_cli --late-compress`` and the service:
``train_codec`` / ``set_codec`` / ``compress``, a compressing build, save and load, compact, search over two first
stages, ``add_tokens`` on a compressed store, graph capture, sizes."""
import json

import numpy as np
import pytest
import torch

import late_cases as lc
import late_codec_cases as cc
from semantic_search_kd_amd import FAISSIndexBuilder, GraphIndex, LateInteractionIndex, late as late_mod

pytestmark = pytest.mark.gpu

DIM = lc.DIM


def _flat(n_rows: int, gpu, seed: int = 5) -> FAISSIndexBuilder:
    rows = np.random.default_rng(seed).standard_normal((n_rows, DIM)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    flat = FAISSIndexBuilder(embedding_dim=DIM, index_type="HNSW", metric="ip", device=str(gpu))
    flat.build_from_embeddings(rows)
    return flat


def _compressed(gpu, tok, lims, nbits, n_centroids=16, flat=None):
    late = LateInteractionIndex(_flat(lims.size - 1, gpu) if flat is None else flat)
    late.set_tokens(tok, lims)
    late.set_codec(*cc.random_codec(np.random.default_rng(3), n_centroids, nbits))
    late.compress()
    return late


def _rerank(late, q_bits, q_lims, cand, k):
    D, I, raw = late.rerank_device(q_bits, q_lims, torch.from_numpy(cand).cuda(), k, return_raw=True)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), raw.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[1], b[1]) and all(np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32)) for i in (0, 2))


@pytest.mark.parametrize("nbits", [2, 4])
def test_compress_is_the_restatement_and_frees_the_bf16_store(gpu, nbits):
    tok, lims = lc.sweep_store(seed=9, n_rows=120)
    late = LateInteractionIndex(_flat(120, gpu))
    late.set_tokens(tok, lims)
    assert not late.compressed and late.nbytes == tok.shape[0] * 768
    with pytest.raises(RuntimeError, match="codec"):
        late.compress()
    codec = cc.random_codec(np.random.default_rng(3), 16, nbits)
    late.set_codec(*codec)
    rng = np.random.default_rng(1)
    q_bits, q_lims = lc.queries(rng, [5, 33])
    cand = lc.candidates(rng, 2, 64, 120)
    bare = LateInteractionIndex(late.flat)
    bare.set_tokens(tok, lims)
    assert _same(_rerank(late, q_bits, q_lims, cand, 10), _rerank(bare, q_bits, q_lims, cand, 10)), "a codec alone changes nothing"
    late.compress()
    assert late.compressed and late.tokens is None and late.nbits == nbits and late.n_centroids == 16
    n = tok.shape[0]
    assert late.nbytes == (104 if nbits == 2 else 200) * n + 16 * 768 + 4 * (2 * (1 << nbits) - 1)
    assert late.nbytes == late_mod.store_bytes(n, nbits) + late_mod.codec_bytes(16, nbits)
    cid, scale, codes = late.compressed_numpy()
    # the assignment is the exact top-1 over the centroids: the best fp64 inner product up to the fp32 search's rounding
    t64, c64 = lc.bf16_values(tok).astype(np.float64), lc.bf16_values(codec[0]).astype(np.float64)
    dots = t64 @ c64.T
    assert (dots[np.arange(n), cid] >= dots.max(axis=1) - 1e-5).all()
    want = cc.compress_rows(tok, cid, *codec, nbits)
    assert np.array_equal(codes, want[2]) and np.array_equal(scale.view(np.uint32), want[1].view(np.uint32))
    dec, sc = late.decoded_numpy()
    assert np.array_equal(dec, want[3]) and np.array_equal(sc, scale)
    got = _rerank(late, q_bits, q_lims, cand, 10)
    refc = cc.ReferenceC(q_bits, q_lims, dec, scale, lims)
    live = np.isfinite(got[2])
    assert (np.abs(got[2] - refc.of_candidates(refc.s64, cand))[live] <= refc.of_candidates(refc.E, cand, fill=0.0)[live]).all()
    lc.check_ranking(got[0], got[1], got[2], cand, 10)
    with pytest.raises(RuntimeError):
        late.compress()                                      # no bf16 store is left
    with pytest.raises(RuntimeError):
        late.set_codec(*codec)                               # the store was written with the codec installed
    with pytest.raises(ValueError):
        LateInteractionIndex(_flat(3, gpu)).set_codec(codec[0], codec[1][::-1].copy(), codec[2])


@pytest.mark.parametrize("nbits", [2, 4])
def test_save_load_compact_and_add_tokens(gpu, tmp_path, nbits):
    rng = np.random.default_rng(59)
    tok, lims = lc.sweep_store(seed=9, n_rows=120)
    late = _compressed(gpu, tok, lims, nbits)
    q_bits, q_lims = lc.queries(rng, [32, 7])
    cand = np.tile(np.arange(120, dtype=np.int64), (2, 1))
    before = _rerank(late, q_bits, q_lims, cand, 10)
    # ---- save / load: every array and every score
    late.save(tmp_path)
    meta = json.loads((tmp_path / "late.json").read_text())
    assert meta["nbits"] == nbits and meta["n_centroids"] == 16 and not (tmp_path / "late_tokens.bf16").exists()
    again = LateInteractionIndex(late.flat)
    again.load(tmp_path)
    assert again.compressed and again.nbits == nbits and np.array_equal(again.lims, lims)
    for a, b in zip(again.compressed_numpy() + again.codec_numpy(), late.compressed_numpy() + late.codec_numpy()):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert _same(_rerank(again, q_bits, q_lims, cand, 10), before)
    with pytest.raises(ValueError, match="rows"):
        LateInteractionIndex(_flat(119, gpu)).load(tmp_path)
    # ---- add_tokens on a compressed store: 100 rows, then the other 20 compressed on arrival
    flat = _flat(100, gpu)
    part = _compressed(gpu, tok[: lims[100]], lims[:101], nbits, flat=flat)
    extra = np.random.default_rng(5).standard_normal((120, DIM)).astype(np.float32)[100:]
    flat.add(extra / np.linalg.norm(extra, axis=1, keepdims=True))
    with pytest.raises(RuntimeError, match="token store covers 100 rows"):
        part.rerank_device(q_bits, q_lims, torch.from_numpy(cand).cuda(), 5)
    part.add_tokens(tok[lims[100]:], lims[100:] - lims[100])
    assert part.compressed and part.tokens is None
    for a, b in zip(part.compressed_numpy(), late.compressed_numpy()):
        assert np.array_equal(a, b)
    assert np.array_equal(_rerank(part, q_bits, q_lims, cand, 10)[2].view(np.uint32), before[2].view(np.uint32))
    # ---- compact: the survivors keep their bits
    gone = [0, 7, 24, 25, 119]
    assert late.flat.remove_ids(gone) == len(gone)
    kept = late.flat.compact()
    late.compact(kept)
    assert late.compressed and late.ntotal == late.flat.ntotal == 120 - len(gone)
    after = _rerank(late, q_bits, q_lims, np.tile(np.arange(kept.size, dtype=np.int64), (2, 1)), 10)[2]
    assert np.array_equal(after.view(np.uint32), before[2][:, kept].view(np.uint32))


def test_search_over_two_first_stages_and_graph_capture(gpu):
    rng = np.random.default_rng(47)
    tok, lims = lc.sweep_store(seed=9, n_rows=400)
    late = _compressed(gpu, tok, lims, 2)
    flat = late.flat
    q_bits, q_lims = lc.queries(rng, [5, 32, 33, 1, 17])
    q_emb = rng.standard_normal((5, DIM)).astype(np.float32)
    q_emb /= np.linalg.norm(q_emb, axis=1, keepdims=True)
    qd = torch.from_numpy(q_emb).cuda()
    graph = GraphIndex(flat=flat, M=8, ef=64)
    graph.build_graph()
    allow = np.ones(400, dtype=bool)
    allow[::3] = False
    removed = int(flat.search_device(qd, 50)[1].cpu().numpy()[0, 0])
    assert flat.remove_ids([removed]) == 1
    for stage, kw in ((None, {}), (None, {"allow": allow}), (graph, {"ef": 64, "allow": allow})):
        D, I = late.search(q_emb, q_bits, q_lims, k=10, candidates=50, first_stage=stage, **kw)
        first = (flat if stage is None else stage).search_device(qd, k=50, **kw)[1]
        D2, I2 = late.rerank_device(q_bits, q_lims, first, 10)
        assert np.array_equal(I, I2.cpu().numpy()) and np.array_equal(D.view(np.uint32), D2.cpu().numpy().view(np.uint32))
        assert not (I == removed).any(), "a removed row was returned"
        if "allow" in kw:
            assert allow[I[I >= 0]].all(), "a row outside the allow mask was returned"
        assert (I[:, 0] >= 0).all()
    # ---- graph capture and replay of rerank_device
    cand = torch.from_numpy(lc.candidates(rng, 5, 65, 400, must=lc.big_rows(lims)[:6])).cuda()
    queries = late.prepare_queries(q_bits, q_lims)
    eager_D, eager_I = late.rerank_device(queries, None, cand, 10)     # also sizes the workspace before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            D, I = late.rerank_device(queries, None, cand, 10)
    torch.cuda.current_stream().wait_stream(side)
    D.fill_(0)
    I.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(I, eager_I) and torch.equal(D.view(torch.int32), eager_D.view(torch.int32))


@pytest.mark.parametrize("nbits", [2, 4])
def test_train_codec_is_deterministic_and_follows_its_rule(gpu, nbits):
    tok, lims = lc.sweep_store(seed=9, n_rows=400)
    codecs = []
    for _ in range(2):
        late = LateInteractionIndex(_flat(400, gpu))
        late.set_tokens(tok, lims)
        late.train_codec(nbits=nbits, n_centroids=32, sample_tokens=1000, iterations=3, seed=7)
        codecs.append(late.codec_numpy())
    for a, b in zip(*codecs):
        assert a.dtype == b.dtype and np.array_equal(a, b), "the same inputs must give the same codec bits"
    cen, cut, w = codecs[0]
    L = 1 << nbits
    assert cen.shape == (32, DIM) and cut.shape == (L - 1,) and w.shape == (L,)
    late_mod.check_codec(cen, cut, w)
    assert (np.diff(np.concatenate([w[:1], np.stack([cut, w[1:]], axis=1).reshape(-1)])) >= 0).all(), "w0 <= c1 <= w1 <= ..."
    # the tables are the quantiles of the sample's residuals against the rounded centroids
    n = tok.shape[0]
    sample = tok[(np.arange(1000, dtype=np.int64) * n) // 1000]
    res = np.sort((lc.bf16_values(sample) - lc.bf16_values(cen[cc.assign_rows(sample, cen)])).reshape(-1))
    for i, c in enumerate(cut, 1):
        below = np.searchsorted(res, c, side="right") / res.size
        assert abs(below - i / L) < 2e-3
    # a default size, another seed, and the whole pipeline to scores
    late.compress()
    dec, scale = late.decoded_numpy()
    d = lc.bf16_values(dec).astype(np.float64) * scale[:, None]
    cos = (lc.bf16_values(tok).astype(np.float64) * d).sum(axis=1)
    assert cos.mean() > (0.65 if nbits == 2 else 0.9)
    auto = LateInteractionIndex(_flat(400, gpu))
    auto.set_tokens(tok, lims)
    auto.train_codec(nbits=nbits, iterations=1)
    assert auto.n_centroids == late_mod.default_n_centroids(n) == 512
    with pytest.raises(ValueError):
        auto.train_codec(nbits=3)
    with pytest.raises(ValueError):
        auto.train_codec(nbits=2, n_centroids=2000, sample_tokens=1000)


DOCS = ["machine learning search", "deep neural networks work", "hello world test document",
        "semantic text search index vector", "what does machine learning work how", "vector index"]


def test_compressing_build_cli_and_serve(gpu, tmp_path, monkeypatch, capsys):
    import pandas as pd
    from fastapi.testclient import TestClient

    from semantic_search_kd_amd import BertConfig, StudentModel, synthetic_state_dict
    from semantic_search_kd_amd.build_index_cli import main as build_index_main
    from semantic_search_kd_amd.serve import app as app_module
    from semantic_search_kd_amd.serve.app import ServeSettings, app_state, create_app
    from semantic_search_kd_amd.weights import save_model_dir
    from test_encoder_gpu import _vocab

    vocab = _vocab()
    cfg = BertConfig(vocab_size=len(vocab), num_hidden_layers=2)
    mdir = tmp_path / "e5-small-v2-synthetic"
    save_model_dir(mdir, cfg, synthetic_state_dict(cfg))
    (mdir / "vocab.txt").write_text("\n".join(vocab))
    corpus = tmp_path / "corpus.parquet"
    pd.DataFrame({"chunk_id": [f"chunk_{i}" for i in range(len(DOCS))], "text": DOCS}).to_parquet(corpus)
    student = StudentModel(str(mdir), device="cuda:0")

    # ---- compress() of a bf16 store equals the compressing build under the same codec, bit for bit
    codec = cc.random_codec(np.random.default_rng(3), 4, 2)
    a = LateInteractionIndex(_flat(len(DOCS), gpu), max_doc_tokens=7)
    a.build_from_texts(student, DOCS)
    tokens_bf16 = a.tokens_numpy()
    a.set_codec(*codec)
    a.compress()
    b = LateInteractionIndex(_flat(len(DOCS), gpu), max_doc_tokens=7)
    b.set_codec(*codec)
    b.build_from_texts(student, DOCS, compress=2, encode_texts=4)        # two batches of texts
    assert b.compressed and b.tokens is None and np.array_equal(a.lims, b.lims)
    for x, y in zip(a.compressed_numpy(), b.compressed_numpy()):
        assert np.array_equal(x, y)
    # without a codec installed the build trains one on the texts' own tokens
    c = LateInteractionIndex(_flat(len(DOCS), gpu), max_doc_tokens=7)
    c.build_from_texts(student, DOCS, compress=4, n_centroids=2, iterations=2)
    assert c.compressed and c.nbits == 4 and c.n_centroids == 2 and np.array_equal(c.lims, a.lims)

    # ---- build_index_cli --late-interaction --late-compress
    out = tmp_path / "index"
    common = ["--model-path", str(mdir), "--data-path", str(corpus), "--batch-size", "4", "--device", "cuda:0"]
    assert build_index_main(common + ["--output-dir", str(out), "--late-interaction", "--late-max-doc-tokens", "7",
                                      "--late-compress", "2"]) == 0
    printed = capsys.readouterr().out
    meta = json.loads((out / "late.json").read_text())
    n = meta["n_tokens"]
    assert meta["nbits"] == 2 and n == tokens_bf16.shape[0] and not (out / "late_tokens.bf16").exists()
    assert (out / "late_codes.u8").stat().st_size == 96 * n
    total = 104 * n + meta["n_centroids"] * 768 + 28
    assert f"{n} tokens, {total} bytes compressed to 2 bits over {meta['n_centroids']} centroids ({768 * n} bytes as bf16" in printed
    with pytest.raises(SystemExit):
        build_index_main(common + ["--output-dir", str(out), "--late-compress", "2"])
    with pytest.raises(SystemExit):
        build_index_main(common + ["--output-dir", str(out), "--late-interaction", "--late-compress", "3"])
    capsys.readouterr()

    # ---- the service loads whichever store the directory holds
    def reset():
        for k, v in vars(app_module.AppState()).items():
            setattr(app_state, k, v)

    try:
        monkeypatch.setenv("SEMANTIC_KD_FEATURES__ENABLE_LATE_INTERACTION", "true")
        monkeypatch.setenv("SEMANTIC_KD_LATE__CANDIDATES", "6")
        reset()
        app = create_app(student_model_path=str(mdir), device="cuda:0", settings=ServeSettings.from_env())
        q = "what is semantic search"
        with TestClient(app) as client:
            assert client.post("/index/load", params={"index_path": str(out)}).status_code == 200
            r = client.post("/search", json={"query": q, "k": 4})
            assert r.status_code == 200, r.text
            body, served, builder = r.json(), app_state.late, app_state.index_builder
        assert isinstance(served, LateInteractionIndex) and served.compressed and served.nbits == 2
        q_tokens, q_lims = student.encode_tokens([q], is_query=True, max_tokens=served.max_query_tokens)
        cand = builder.search(student.encode_queries([q]), k=6)[1]
        D, I = served.rerank(q_tokens, q_lims, cand, 4)
        assert [int(x["doc_id"].split("_")[1]) for x in body["results"]] == I[0].tolist()
        np.testing.assert_array_equal(np.float32([x["score"] for x in body["results"]]), D[0] / np.float32(int(q_lims[1])))
        dec, scale = served.decoded_numpy()
        q_bits = q_tokens.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        ref = cc.ReferenceC(q_bits, q_lims, dec, scale, served.lims)
        assert (np.abs(D[0].astype(np.float64) - ref.s64[0, I[0]]) <= ref.E[0, I[0]]).all()
    finally:
        reset()
