"""Serving through the inverted lists: an index built with ``--index-type ivf`` is retrieved through ``IVFIndex`` when
``SEMANTIC_KD_INDEX__INDEX_TYPE=ivf`` is set, with the unchanged response schema; without the variable nothing changes."""
import json
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
from fastapi.testclient import TestClient

from semantic_search_kd_amd import BertConfig, FAISSIndexBuilder, IVFIndex, synthetic_state_dict
from semantic_search_kd_amd.build_index_cli import main as build_index_main
from semantic_search_kd_amd.serve import app as app_module
from semantic_search_kd_amd.serve.app import ServeSettings, app_state, create_app
from semantic_search_kd_amd.weights import save_model_dir
from test_encoder_gpu import _vocab

pytestmark = pytest.mark.gpu

WORDS = ["machine", "learning", "search", "vector", "index", "deep", "neural", "networks", "work", "hello", "world",
         "test", "document", "semantic", "text", "what", "how", "does"]
SCHEMAS = json.loads((Path(__file__).resolve().parent / "golden" / "api_schemas.json").read_text())


def _docs(n=40):
    rng = np.random.default_rng(0)
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 8)))) for _ in range(n)]


def _reset_state():
    for k, v in vars(app_module.AppState()).items():
        setattr(app_state, k, v)


def test_ivf_build_cli_then_serve(gpu, tmp_path, monkeypatch, capsys):
    vocab = _vocab()
    cfg = BertConfig(vocab_size=len(vocab), num_hidden_layers=2)
    mdir = tmp_path / "e5-small-v2-synthetic"
    save_model_dir(mdir, cfg, synthetic_state_dict(cfg))
    (mdir / "vocab.txt").write_text("\n".join(vocab))
    docs = _docs()
    corpus = tmp_path / "corpus.parquet"
    pd.DataFrame({"chunk_id": [f"chunk_{i}" for i in range(len(docs))], "text": docs}).to_parquet(corpus)
    out = tmp_path / "index"
    common = ["--model-path", str(mdir), "--data-path", str(corpus), "--output-dir", str(out), "--batch-size", "8",
              "--device", "cuda:0", "--index-type", "ivf", "--nlist", "4"]
    assert build_index_main(common + ["--nprobe", "4"]) == 0          # every list probed: recall 1.0
    assert "recall@10 vs exact: 1.0000" in capsys.readouterr().out
    assert build_index_main(common + ["--nprobe", "1", "--recall-threshold", "1.01"]) == 1   # the gate can fail a build
    assert build_index_main(common + ["--nprobe", "2", "--recall-threshold", "0.0"]) == 0
    for name in ("index.faiss", "doc_ids.json", "texts.json", "ivf.json", "ivf_centroids.npy", "ivf_list_offsets.npy",
                 "ivf_list_rows.npy"):
        assert (out / name).exists(), name
    assert json.loads((out / "ivf.json").read_text())["nprobe"] == 2

    q = "what is semantic search"

    def serve(settings):
        _reset_state()
        app = create_app(student_model_path=str(mdir), device="cuda:0", settings=settings)
        with TestClient(app) as client:
            r = client.post("/index/load", params={"index_path": str(out)})
            assert r.status_code == 200 and r.json() == {"status": "loaded", "index_path": str(out), "num_documents": 40}
            r = client.post("/search", json={"query": q, "k": 5})
            assert r.status_code == 200
            emb = app_state.student.encode_queries([q])
            return r.json(), emb, app_state.ivf, app_state.index_builder

    try:
        # without the variable: the exact scan, as before
        monkeypatch.delenv("SEMANTIC_KD_INDEX__INDEX_TYPE", raising=False)
        settings = ServeSettings.from_env()
        settings.environment = "test"
        assert settings.index_type == "flat"
        body, emb, served_ivf, builder = serve(settings)
        assert served_ivf is None and isinstance(builder, FAISSIndexBuilder)
        exact_ids = builder.search(emb, k=5)[1][0]
        assert [x["doc_id"] for x in body["results"]] == [f"chunk_{i}" for i in exact_ids]

        # with it: the ids of IVFIndex.search, the same schema
        monkeypatch.setenv("SEMANTIC_KD_INDEX__INDEX_TYPE", "ivf")
        settings = ServeSettings.from_env()
        settings.environment = "test"
        assert settings.index_type == "ivf"
        body, emb, served_ivf, builder = serve(settings)
        assert isinstance(served_ivf, IVFIndex) and served_ivf.flat is builder and served_ivf.nprobe == 2
        assert served_ivf.last_search_path == "ivf"
        D, I = served_ivf.search(emb, k=5)
        assert [x["doc_id"] for x in body["results"]] == [f"chunk_{i}" for i in I[0] if i >= 0]
        np.testing.assert_array_equal(np.float32([x["score"] for x in body["results"]]), D[0][I[0] >= 0])
        assert set(body) == set(SCHEMAS["SearchResponse"]["properties"])
        assert body["total_results"] == len(body["results"]) and body["reranked"] is False
        for rank, item in enumerate(body["results"], 1):
            assert set(item) == set(SCHEMAS["SearchResult"]["properties"]) and item["rank"] == rank
            assert item["text"] == docs[int(item["doc_id"].split("_")[1])]
        # the lists restrict the rows: the results are the exact search over the probed lists' rows
        lists = served_ivf.lists_numpy()
        probe = served_ivf.probe_device(__import__("torch").from_numpy(emb).to(builder.device)).cpu().numpy()[0]
        allowed = np.concatenate([lists[1][lists[0][l]:lists[0][l + 1]] for l in probe])
        assert np.array_equal(builder.search(emb, k=5, allow=allowed.astype(np.int64))[1], I)
    finally:
        _reset_state()
