"""FastAPI application serving ``/search`` and ``/encode`` from the MI355X backend.

Route set, status codes and response shapes mirror the reference (src/serve/app.py:221-457):
``/``, ``/health``, ``/ready``, ``/live``, ``POST /search``, ``POST /encode``, ``POST /index/load``.
Glue semantics kept on purpose (src/serve/app.py:285-352): the query is encoded with
``encode_queries`` (E5 prefix), ``/encode`` uses plain ``encode``; ids < 0 or past ``doc_ids`` are
skipped *without* renumbering ranks; ``score = float(distance)``; results are trimmed to ``k``
after the optional rerank; any non-HTTP exception becomes a 500 ``{"error": "Search failed: ..."}``.
The reference's auth / rate-limit / logging middlewares (src/serve/middleware.py) are HTTP hygiene
outside the compute path and are not re-implemented here; they can be mounted in front unchanged.
"""
from __future__ import annotations

import json
import logging
import os
import time
from contextlib import asynccontextmanager
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional

import numpy as np
from fastapi import FastAPI, HTTPException, Request, status
from fastapi.responses import JSONResponse

logger = logging.getLogger("semantic_search_kd_amd.serve")

from ..index import FAISSIndexBuilder  # noqa: E402,F401
from ..late import LATE_R_MAX, PLAID_NPROBE_MAX
from ..sharded_index import open_index
from ..student import StudentModel
from .schemas import (
    EncodeRequest,
    EncodeResponse,
    ErrorResponse,
    HealthResponse,
    SearchRequest,
    SearchResponse,
    SearchResult,
)

VERSION = "1.1.0"  # API version of the reference this surface is wire-compatible with (app.py:41)


def _env_bool(value: Optional[str], default: bool) -> bool:
    """An environment flag as pydantic-settings reads one (the reference's loader): 1 / true / yes / on, any case."""
    if value is None or not value.strip():
        return default
    return value.strip().lower() in ("1", "true", "t", "yes", "y", "on")


@dataclass
class ServeSettings:
    """The few settings the path reads (reference: src/config.py:22-32,223-233; env prefix
    ``SEMANTIC_KD_`` with ``__`` nesting, src/config.py:275-279)."""

    student_model_name: str = "./artifacts/models/kd_student_production"
    student_device: Optional[str] = "cuda"
    index_dir: Optional[str] = None
    environment: str = "development"
    extra: Dict[str, Any] = field(default_factory=dict)
    # the ``hybrid:`` block of the reference's configs/service.yaml:43-49, names and defaults kept (the reference reads
    # the keys and has no code behind them): /search fuses the dense ranking with a BM25 ranking (hybrid.HybridIndex)
    hybrid_enabled: bool = False
    bm25_index_path: str = "./artifacts/indexes/bm25"
    bm25_weight: float = 0.3
    semantic_weight: float = 0.7
    fusion_method: str = "rrf"   # rrf (reciprocal rank fusion), linear
    # ``index_type`` of the reference's configs/index.yaml:4 (hnsw | ivf_pq | flat): "ivf" retrieves through the inverted
    # lists saved beside the index (ivf.IVFIndex), "ivf_pq" through the lists and their PQ codes (pq.IVFPQIndex), when
    # the directory holds them, "graph" through the k-NN graph saved beside the index (graph.GraphIndex); anything else
    # ("hnsw" included) is the exact scan
    index_type: str = "flat"
    # ``features.enable_late_interaction`` of the reference's configs/service.yaml (.env.example:
    # ENABLE_LATE_INTERACTION; read there, no code behind it): /search re-ranks the first stage's candidates by
    # token-level MaxSim over the token store saved beside the index (late.LateInteractionIndex)
    late_interaction_enabled: bool = False
    late_candidates: int = 100
    # where the candidates of the re-rank come from: "dense" (the first stage above) or "centroids" - the compressed token
    # store's own centroid lists (late.LateInteractionIndex.search_tokens, late_nprobe lists per query token), when the
    # directory holds them
    late_first_stage: str = "dense"
    late_nprobe: int = 2
    # ``features.enable_query_expansion`` of the reference's configs/service.yaml:108-113 (.env.example:
    # ENABLE_QUERY_EXPANSION; read there, no code behind it): /search wraps whatever first stage it resolves to in
    # pseudo-relevance feedback (expand.ExpandedIndex: Rocchio on the dense side, RM3 on the BM25 side)
    query_expansion_enabled: bool = False
    expansion_fb_docs: int = 5
    expansion_fb_terms: int = 10
    expansion_alpha: float = 1.0
    expansion_beta: float = 0.75
    expansion_orig_repeat: int = 2
    expansion_max_df_fraction: float = 0.25
    # diversified results (diversify.DiverseIndex; the reference has no such step): /search fetches diversity_fetch_k
    # candidates from the dense first stage and picks k of them by Maximal Marginal Relevance, dropping candidates whose
    # cosine to a picked row reaches diversity_dup_threshold (unset: no cut-off).  It wraps the dense stage outermost,
    # around the optional query expansion; with hybrid retrieval it is skipped (fused scores are not cosine relevance).
    # A late-interaction or teacher rerank that follows RE-ORDERS the diversified set by its own scores: the set is
    # MMR's, the order is the reranker's.
    diversity_enabled: bool = False
    diversity_lambda: float = 0.5
    diversity_fetch_k: int = 50
    diversity_dup_threshold: Optional[float] = None

    def diversity(self):
        """The ``Diversity`` /search applies, or None (the flag is off)."""
        if not self.diversity_enabled:
            return None
        from ..diversify import Diversity

        return Diversity(lambda_mult=self.diversity_lambda, fetch_k=self.diversity_fetch_k,
                         dup_threshold=self.diversity_dup_threshold)

    def query_expansion(self):
        """The ``QueryExpansion`` /search applies, or None (the flag is off)."""
        if not self.query_expansion_enabled:
            return None
        from ..expand import QueryExpansion

        return QueryExpansion(fb_docs=self.expansion_fb_docs, fb_terms=self.expansion_fb_terms,
                              alpha=self.expansion_alpha, beta=self.expansion_beta,
                              orig_repeat=self.expansion_orig_repeat, max_df_fraction=self.expansion_max_df_fraction)

    @staticmethod
    def from_env() -> "ServeSettings":
        e = os.environ
        return ServeSettings(
            student_model_name=e.get("SEMANTIC_KD_STUDENT__MODEL_NAME", ServeSettings.student_model_name),
            student_device=e.get("SEMANTIC_KD_STUDENT__DEVICE", "cuda"),
            index_dir=e.get("SEMANTIC_KD_INDEX__DIR"),
            environment=e.get("SEMANTIC_KD_ENVIRONMENT", "development"),
            hybrid_enabled=_env_bool(e.get("SEMANTIC_KD_HYBRID__ENABLED"), ServeSettings.hybrid_enabled),
            bm25_index_path=e.get("SEMANTIC_KD_HYBRID__BM25_INDEX_PATH", ServeSettings.bm25_index_path),
            bm25_weight=float(e.get("SEMANTIC_KD_HYBRID__BM25_WEIGHT", ServeSettings.bm25_weight)),
            semantic_weight=float(e.get("SEMANTIC_KD_HYBRID__SEMANTIC_WEIGHT", ServeSettings.semantic_weight)),
            fusion_method=e.get("SEMANTIC_KD_HYBRID__FUSION_METHOD", ServeSettings.fusion_method),
            index_type=(e.get("SEMANTIC_KD_INDEX__INDEX_TYPE") or ServeSettings.index_type).strip().lower(),
            late_interaction_enabled=_env_bool(e.get("SEMANTIC_KD_FEATURES__ENABLE_LATE_INTERACTION"),
                                               ServeSettings.late_interaction_enabled),
            late_candidates=int(e.get("SEMANTIC_KD_LATE__CANDIDATES") or ServeSettings.late_candidates),
            late_first_stage=(e.get("SEMANTIC_KD_LATE__FIRST_STAGE") or ServeSettings.late_first_stage).strip().lower(),
            late_nprobe=int(e.get("SEMANTIC_KD_LATE__NPROBE") or ServeSettings.late_nprobe),
            query_expansion_enabled=_env_bool(e.get("SEMANTIC_KD_FEATURES__ENABLE_QUERY_EXPANSION"),
                                              ServeSettings.query_expansion_enabled),
            expansion_fb_docs=int(e.get("SEMANTIC_KD_EXPANSION__FB_DOCS") or ServeSettings.expansion_fb_docs),
            expansion_fb_terms=int(e.get("SEMANTIC_KD_EXPANSION__FB_TERMS") or ServeSettings.expansion_fb_terms),
            expansion_alpha=float(e.get("SEMANTIC_KD_EXPANSION__ALPHA") or ServeSettings.expansion_alpha),
            expansion_beta=float(e.get("SEMANTIC_KD_EXPANSION__BETA") or ServeSettings.expansion_beta),
            expansion_orig_repeat=int(e.get("SEMANTIC_KD_EXPANSION__ORIG_REPEAT") or ServeSettings.expansion_orig_repeat),
            expansion_max_df_fraction=float(e.get("SEMANTIC_KD_EXPANSION__MAX_DF_FRACTION")
                                            or ServeSettings.expansion_max_df_fraction),
            diversity_enabled=_env_bool(e.get("SEMANTIC_KD_FEATURES__ENABLE_DIVERSITY"), ServeSettings.diversity_enabled),
            diversity_lambda=float(e.get("SEMANTIC_KD_DIVERSITY__LAMBDA") or ServeSettings.diversity_lambda),
            diversity_fetch_k=int(e.get("SEMANTIC_KD_DIVERSITY__FETCH_K") or ServeSettings.diversity_fetch_k),
            diversity_dup_threshold=(float(e["SEMANTIC_KD_DIVERSITY__DUP_THRESHOLD"])
                                     if (e.get("SEMANTIC_KD_DIVERSITY__DUP_THRESHOLD") or "").strip() else None),
        )

    def is_production(self) -> bool:
        return self.environment == "production"


class AppState:
    """Module-global holder of the duck-typed backend objects (reference: app.py:49-66)."""

    def __init__(self) -> None:
        self.student = None
        self.teacher = None
        self.index_builder = None
        self.doc_ids: Optional[List[str]] = None
        self.doc_texts: Optional[Dict[str, str]] = None
        self.settings: Optional[ServeSettings] = None
        self.ready: bool = False
        self.hybrid = None   # hybrid.HybridIndex over index_builder when hybrid retrieval is on and its BM25 index fits
        self.ivf = None      # ivf.IVFIndex / pq.IVFPQIndex over index_builder when the index type asks for it and the directory holds its files
        self.graph = None    # graph.GraphIndex over index_builder, likewise (index type "graph", graph.json)
        self.late = None     # late.LateInteractionIndex over index_builder when late interaction is on and the directory holds its store

    def is_ready(self) -> bool:
        return self.ready and self.student is not None


app_state = AppState()


def _load_index_dir(index_dir: Path) -> Dict[str, Any]:
    # a directory with a shards.json manifest opens as a row-sharded index (sharded_index.ShardedIndex: same
    # search / doc_ids surface, answered by every rank of the process group); anything else as one FAISSIndexBuilder
    builder = open_index(index_dir, app_state.student.embedding_dim, current=app_state.index_builder)
    app_state.index_builder = builder
    app_state.doc_ids = builder.doc_ids
    texts_path = index_dir / "texts.json"
    if texts_path.exists():
        with open(texts_path) as f:
            app_state.doc_texts = json.load(f)
    elif builder.doc_texts:
        app_state.doc_texts = builder.doc_texts
    app_state.hybrid = _load_hybrid(builder, app_state.settings)
    app_state.ivf = _load_ivf(builder, index_dir, app_state.settings)
    app_state.graph = _load_graph(builder, index_dir, app_state.settings)
    app_state.late = _load_late(builder, index_dir, app_state.settings)
    return {"status": "loaded", "index_path": str(index_dir), "num_documents": len(app_state.doc_ids)}


def _load_hybrid(builder, settings: Optional["ServeSettings"]):
    """The ``HybridIndex`` /search retrieves through, or None (dense-only): hybrid retrieval is off, the index is
    row-sharded (``ShardedIndex`` stays dense-only: fusing over shards needs the union across ranks), or the BM25
    index does not load or does not describe the dense index's rows - then a warning is logged and the service answers
    dense-only, the reference's rule for a teacher that fails to load (app.py:96-107)."""
    if settings is None or not settings.hybrid_enabled:
        return None
    if not isinstance(builder, FAISSIndexBuilder):
        logger.warning("Hybrid retrieval is enabled but the index is not a single-GPU dense index: serving dense-only")
        return None
    try:
        from ..bm25 import BM25Index
        from ..hybrid import HybridIndex

        bm25 = BM25Index(settings.bm25_index_path, device=str(builder.device))
        bm25.load()
        hybrid = HybridIndex(builder, bm25, semantic_weight=settings.semantic_weight, bm25_weight=settings.bm25_weight,
                             fusion_method=settings.fusion_method)
        if settings.diversity_enabled:
            logger.warning("Diversity is enabled but retrieval is hybrid: fused scores are not cosine relevance, "
                           "serving without the MMR step")
        return hybrid
    except Exception as exc:  # noqa: BLE001
        logger.warning("Failed to load the BM25 index (hybrid retrieval disabled, serving dense-only): %s", exc)
        return None


def _load_graph(builder, index_dir: Path, settings: Optional["ServeSettings"]):
    """The ``GraphIndex`` /search retrieves through, or None (the exact scan): the index type is not "graph", the
    directory holds no ``graph.json``, the index is row-sharded, or the files do not load - then a warning is logged
    and the service answers with the exact search."""
    if settings is None or settings.index_type != "graph":
        return None
    from ..graph import GraphIndex, is_graph_dir

    if not isinstance(builder, FAISSIndexBuilder) or not is_graph_dir(index_dir):
        logger.warning("Index type is graph but %s holds no graph over a single-GPU index: serving the exact scan", index_dir)
        return None
    try:
        graph = GraphIndex(flat=builder)
        graph.load_graph(index_dir)
        return graph
    except Exception as exc:  # noqa: BLE001
        logger.warning("Failed to load the graph (serving the exact scan): %s", exc)
        return None


def _load_late(builder, index_dir: Path, settings: Optional["ServeSettings"]):
    """The ``LateInteractionIndex`` /search re-ranks with, or None (the first stage's ranking is the answer, as without
    the feature): late interaction is off, the directory holds no ``late.json``, the index is row-sharded, or the store
    does not load or covers another number of rows - then a warning is logged and the service answers as before."""
    if settings is None or not settings.late_interaction_enabled:
        return None
    from ..late import LateInteractionIndex, is_late_dir

    if not isinstance(builder, FAISSIndexBuilder) or not is_late_dir(index_dir):
        logger.warning("Late interaction is enabled but %s holds no token store over a single-GPU index: serving "
                       "without it", index_dir)
        return None
    try:
        late = LateInteractionIndex(builder)
        late.load(index_dir)     # whichever store the directory holds: bf16 rows or the compressed arrays and their codec
        logger.info("Late-interaction token store: %d tokens, %d bytes%s", late.n_tokens, late.nbytes,
                    f" ({late.nbits}-bit residuals over {late.n_centroids} centroids)" if late.compressed else "")
        if settings.late_first_stage == "centroids":
            if late.has_centroid_lists:
                logger.info("Late interaction takes its candidates from the centroid lists (%d bytes, nprobe %d)",
                            late.centroid_list_bytes, settings.late_nprobe)
            else:
                logger.warning("SEMANTIC_KD_LATE__FIRST_STAGE is centroids but %s holds no centroid lists: the candidates "
                               "come from the dense first stage as before", index_dir)
        elif settings.late_first_stage != "dense":
            logger.warning("SEMANTIC_KD_LATE__FIRST_STAGE=%s is neither dense nor centroids: serving with dense",
                           settings.late_first_stage)
        return late
    except Exception as exc:  # noqa: BLE001
        logger.warning("Failed to load the late-interaction token store (serving without it): %s", exc)
        return None


def _load_ivf(builder, index_dir: Path, settings: Optional["ServeSettings"]):
    """The ``IVFIndex`` (index type "ivf") or ``IVFPQIndex`` ("ivf_pq") /search retrieves through, or None (the exact
    scan): the index type is neither, the directory holds no ``ivf.json`` (for "ivf_pq": no ``pq.json``), the index is
    row-sharded, or the files do not load - then a warning is logged and the service answers with the exact search."""
    if settings is None or settings.index_type not in ("ivf", "ivf_pq"):
        return None
    from ..ivf import IVFIndex, is_ivf_dir
    from ..pq import IVFPQIndex, is_pq_dir

    want_pq = settings.index_type == "ivf_pq"
    if not isinstance(builder, FAISSIndexBuilder) or not is_ivf_dir(index_dir) or (want_pq and not is_pq_dir(index_dir)):
        logger.warning("Index type is %s but %s holds no %s over a single-GPU index: serving the exact scan",
                       settings.index_type, index_dir, "inverted lists with PQ codes" if want_pq else "inverted lists")
        return None
    try:
        ivf = IVFPQIndex(flat=builder) if want_pq else IVFIndex(flat=builder)
        ivf.load_lists(index_dir)
        if want_pq and ivf.refine == 0:
            # an index saved with refine = 0 answers with raw ADC scores; the service's scores are exact inner products
            logger.warning("%s stores refine = 0 (raw ADC scores): serving with the default exact re-ranking", index_dir)
            ivf.refine = None
        return ivf
    except Exception as exc:  # noqa: BLE001
        logger.warning("Failed to load the inverted lists (serving the exact scan): %s", exc)
        return None


def create_app(
    student_model_path: Optional[str] = None,
    teacher_model_path: Optional[str] = None,
    index_dir: Optional[Path] = None,
    device: str = "cuda",
    settings: Optional[ServeSettings] = None,
) -> FastAPI:
    """Application factory with the reference's signature (app.py:124-130)."""
    settings = settings or ServeSettings.from_env()
    if student_model_path:
        settings.student_model_name = student_model_path
    if device:
        settings.student_device = device
    if index_dir:
        settings.index_dir = str(index_dir)

    @asynccontextmanager
    async def lifespan(app: FastAPI):
        app_state.settings = settings
        if app_state.student is None:
            app_state.student = StudentModel(model_name=settings.student_model_name, device=settings.student_device)
        if teacher_model_path and app_state.teacher is None:
            # reference: app.py:96-107 - a teacher that fails to load only disables reranking
            try:
                from ..teacher import TeacherModel

                app_state.teacher = TeacherModel(model_name=teacher_model_path, device=settings.student_device)
            except Exception as exc:  # noqa: BLE001
                logger.warning("Failed to load teacher model (reranking disabled): %s", exc)
        if settings.index_dir and app_state.index_builder is None and Path(settings.index_dir).exists():
            _load_index_dir(Path(settings.index_dir))
        app_state.ready = True
        yield
        app_state.ready = False

    app = FastAPI(title="Semantic Search API", version=VERSION, lifespan=lifespan)
    register_routes(app, settings)
    return app


def register_routes(app: FastAPI, settings: ServeSettings) -> None:
    @app.get("/", response_model=Dict[str, Any])
    async def root() -> Dict[str, Any]:
        return {
            "service": "Semantic Search API",
            "version": VERSION,
            "status": "running" if app_state.is_ready() else "starting",
            "environment": settings.environment,
        }

    @app.get("/health", response_model=HealthResponse)
    async def health() -> HealthResponse:
        return HealthResponse(
            status="healthy" if app_state.is_ready() else "unhealthy",
            model_loaded=app_state.student is not None,
            # a row-sharded index counts as loaded only while EVERY rank holds its shards and answers
            # (sharded_index.ShardedIndex.is_loaded)
            index_loaded=app_state.index_builder is not None and bool(getattr(app_state.index_builder, "is_loaded", True)),
            index_size=len(app_state.doc_ids) if app_state.doc_ids else 0,
            version=VERSION,
        )

    @app.get("/ready")
    async def readiness() -> Dict[str, bool]:
        if not app_state.is_ready():
            raise HTTPException(status_code=status.HTTP_503_SERVICE_UNAVAILABLE, detail="Service not ready")
        return {"ready": True}

    @app.get("/live")
    async def liveness() -> Dict[str, bool]:
        return {"alive": True}

    @app.post("/search", response_model=SearchResponse)
    async def search(request: SearchRequest) -> SearchResponse:
        t0 = time.time()
        if app_state.student is None:
            raise HTTPException(status_code=status.HTTP_503_SERVICE_UNAVAILABLE, detail="Student model not loaded")
        if app_state.index_builder is None:
            raise HTTPException(status_code=status.HTTP_503_SERVICE_UNAVAILABLE, detail="Search index not loaded")
        try:
            query_emb = app_state.student.encode_queries([request.query])
            k_retrieve = request.rerank_top_k if request.rerank else request.k
            hybrid = app_state.hybrid

            expansion = (app_state.settings or settings).query_expansion()
            if expansion is not None and not isinstance(app_state.index_builder, FAISSIndexBuilder):
                expansion = None   # (a row-sharded index: the feedback rows live on other ranks)

            def expanded(stage):
                # features.enable_query_expansion wraps whatever the first stage resolves to
                if expansion is None:
                    return stage
                from ..expand import ExpandedIndex

                return ExpandedIndex(stage, expansion)

            diversity = (app_state.settings or settings).diversity()
            if diversity is not None and not isinstance(app_state.index_builder, FAISSIndexBuilder):
                diversity = None   # (a row-sharded index: the candidates' rows live on other ranks)

            def diverse(stage):
                # diversity wraps the dense stage outermost: MMR over the (expanded) stage's own candidates; a late or
                # teacher rerank below re-orders the set it returns
                if diversity is None:
                    return stage
                from ..diversify import DiverseIndex

                return DiverseIndex(stage, diversity)

            def first_stage(k_first: int):
                if hybrid is not None and hybrid.dense is app_state.index_builder:
                    # both sides contribute at least k rows; the fused score is the result's score (no MMR step: warned
                    # about when the BM25 index was loaded)
                    depth = hybrid.clip_depth(max(hybrid.depth, k_first))
                    return expanded(hybrid).search([request.query], query_emb, k=min(k_first, 2 * depth), depth=depth)
                k_stage = k_first if diversity is None else diversity.depth(k_first)   # what the stage itself is asked for
                if app_state.ivf is not None and app_state.ivf.flat is app_state.index_builder and k_stage <= 256:
                    return diverse(expanded(app_state.ivf)).search(query_emb, k=k_first)
                if (app_state.graph is not None and app_state.graph.flat is app_state.index_builder
                        and k_stage <= app_state.graph.ef):
                    return diverse(expanded(app_state.graph)).search(query_emb, k=k_first)
                return diverse(expanded(app_state.index_builder)).search(query_emb, k=k_first)

            late = app_state.late
            if late is not None and late.flat is app_state.index_builder and k_retrieve <= LATE_R_MAX:
                # the first stage proposes, token-level MaxSim orders: score = MaxSim / Tq (1.0 = every query token
                # has an identical document token)
                live = app_state.settings or settings
                wanted = min(max(1, int(live.late_candidates), k_retrieve), LATE_R_MAX)
                q_tokens, q_lims = app_state.student.encode_tokens([request.query], is_query=True,
                                                                   max_tokens=late.max_query_tokens)
                if live.late_first_stage == "centroids" and late.has_centroid_lists:
                    # the token store retrieves by itself: centroid lists, centroid interaction, then MaxSim
                    nprobe = min(max(1, int(live.late_nprobe)), late.n_centroids, PLAID_NPROBE_MAX)
                    distances, indices = late.search_tokens(q_tokens, q_lims, k=k_retrieve, nprobe=nprobe, ndocs=wanted)
                else:
                    _, candidates = first_stage(wanted)
                    k_late = min(k_retrieve, candidates.shape[1])
                    distances, indices = late.rerank(q_tokens, q_lims, np.ascontiguousarray(candidates, dtype=np.int64), k_late)
                distances = distances / np.float32(q_lims[1] - q_lims[0])
            else:
                distances, indices = first_stage(k_retrieve)
            results: List[SearchResult] = []
            for rank, (dist, idx) in enumerate(zip(distances[0], indices[0]), 1):
                if idx < 0 or (app_state.doc_ids and idx >= len(app_state.doc_ids)):
                    continue
                doc_id = app_state.doc_ids[idx] if app_state.doc_ids else f"doc_{idx}"
                text = app_state.doc_texts.get(doc_id, "") if app_state.doc_texts else ""
                results.append(SearchResult(doc_id=doc_id, text=text, score=float(dist), rank=rank))
            reranked = False
            if request.rerank and app_state.teacher is not None and results:
                scores = app_state.teacher.score([[request.query, r.text] for r in results])
                for r, s in zip(results, scores):
                    r.score = float(s)
                results = sorted(results, key=lambda r: r.score, reverse=True)
                for pos, r in enumerate(results, 1):
                    r.rank = pos
                reranked = True
            results = results[: request.k]
            return SearchResponse(
                query=request.query,
                results=results,
                total_results=len(results),
                reranked=reranked,
                latency_ms=(time.time() - t0) * 1000,
            )
        except HTTPException:
            raise
        except Exception as exc:  # noqa: BLE001 - mirrors the reference's catch-all (app.py:356-361)
            raise HTTPException(
                status_code=status.HTTP_500_INTERNAL_SERVER_ERROR, detail=f"Search failed: {exc}"
            ) from exc

    @app.post("/encode", response_model=EncodeResponse)
    async def encode(request: EncodeRequest) -> EncodeResponse:
        t0 = time.time()
        if app_state.student is None:
            raise HTTPException(status_code=status.HTTP_503_SERVICE_UNAVAILABLE, detail="Model not loaded")
        try:
            emb = app_state.student.encode(request.texts, convert_to_numpy=True, normalize=request.normalize)
            return EncodeResponse(
                embeddings=emb.tolist(),
                dimension=emb.shape[1],
                num_texts=len(request.texts),
                latency_ms=(time.time() - t0) * 1000,
            )
        except Exception as exc:  # noqa: BLE001
            raise HTTPException(
                status_code=status.HTTP_500_INTERNAL_SERVER_ERROR, detail=f"Encoding failed: {exc}"
            ) from exc

    @app.post("/index/load")
    async def load_index(index_path: str) -> Dict[str, Any]:
        try:
            index_dir = Path(index_path)
            if not index_dir.exists():
                raise HTTPException(status_code=status.HTTP_404_NOT_FOUND, detail=f"Index not found: {index_path}")
            return _load_index_dir(index_dir)
        except HTTPException:
            raise
        except Exception as exc:  # noqa: BLE001
            raise HTTPException(
                status_code=status.HTTP_500_INTERNAL_SERVER_ERROR, detail=f"Failed to load index: {exc}"
            ) from exc

    @app.exception_handler(HTTPException)
    async def http_exception_handler(request: Request, exc: HTTPException) -> JSONResponse:
        return JSONResponse(status_code=exc.status_code, content=ErrorResponse(error=str(exc.detail)).model_dump())

    @app.exception_handler(Exception)
    async def general_exception_handler(request: Request, exc: Exception) -> JSONResponse:
        prod = app_state.settings.is_production() if app_state.settings else False
        return JSONResponse(
            status_code=status.HTTP_500_INTERNAL_SERVER_ERROR,
            content=ErrorResponse(error="Internal server error", detail=None if prod else str(exc)).model_dump(),
        )
