"""MI355X-native embedding-and-search path behind the semantic-search-kd API.

Drop-in for the reference's ``StudentModel`` (sentence-transformers encoder) and
``FAISSIndexBuilder`` (FAISS index) — reference: src/serve/app.py:21-23 — with the
arithmetic in hand-written gfx950 HIP kernels reached through the C-ABI in
``include/sskd_amd.h``.  The directory is named ``semantic-search-kd_amd``; import it
as ``semantic_search_kd_amd`` (the sibling alias package points here).
"""
from . import _native  # noqa: F401
from .index import FAISSIndexBuilder, IndexHandle, read_flat_ip, write_flat_ip  # noqa: F401

from .weights import BertConfig, synthetic_state_dict  # noqa: F401
from .encoder import Mi355xSentenceEncoder, build_wordpiece_tokenizer  # noqa: F401
from .student import StudentModel  # noqa: F401
from .losses import CombinedKDLoss, ContrastiveLoss, ListwiseKDLoss, MarginMSELoss  # noqa: F401
from .bm25 import BM25Index, build_bm25_index  # noqa: F401
from .hybrid import HybridIndex  # noqa: F401
from .expand import ExpandedIndex, QueryExpansion  # noqa: F401
from .diversify import DiverseIndex, Diversity  # noqa: F401
from .graph import GraphIndex  # noqa: F401
from .ivf import IVFIndex  # noqa: F401
from .pq import IVFPQIndex  # noqa: F401
from .late import LateInteractionIndex, is_late_dir  # noqa: F401
from .late_training import TokenLayout, TokenStates, maxsim_scores  # noqa: F401
from .evaluation import (  # noqa: F401
    KDEvaluator,
    compute_retrieval_metrics,
    evaluate_lists,
    evaluate_lists_device,
    expected_calibration_error,
    kendall_tau,
    mrr_at_k,
    ndcg_at_k,
    precision_at_k,
    recall_at_k,
)
from .mining import ANCEMiner, BM25Miner, TeacherMiner, build_mining_curriculum  # noqa: F401
from .denoise import Denoising, TrigramStore, compute_text_overlap, text_overlap  # noqa: F401
from .dedup import DuplicateClusters, cluster_pairs  # noqa: F401
from .teacher import TeacherConfig, TeacherModel  # noqa: F401
from .bench_support import bench_encode  # noqa: F401

Mi355xIndexBuilder = FAISSIndexBuilder

__all__ = [
    "ANCEMiner",
    "BM25Index",
    "BM25Miner",
    "build_bm25_index",
    "HybridIndex",
    "ExpandedIndex",
    "QueryExpansion",
    "DiverseIndex",
    "Diversity",
    "GraphIndex",
    "IVFIndex",
    "IVFPQIndex",
    "LateInteractionIndex",
    "is_late_dir",
    "TokenLayout",
    "TokenStates",
    "maxsim_scores",
    "KDEvaluator",
    "compute_retrieval_metrics",
    "evaluate_lists",
    "evaluate_lists_device",
    "expected_calibration_error",
    "kendall_tau",
    "mrr_at_k",
    "ndcg_at_k",
    "precision_at_k",
    "recall_at_k",
    "build_mining_curriculum",
    "Denoising",
    "TrigramStore",
    "compute_text_overlap",
    "text_overlap",
    "DuplicateClusters",
    "cluster_pairs",
    "TeacherMiner",
    "TeacherConfig",
    "TeacherModel",
    "CombinedKDLoss",
    "ContrastiveLoss",
    "ListwiseKDLoss",
    "MarginMSELoss",
    "StudentModel",
    "Mi355xSentenceEncoder",
    "FAISSIndexBuilder",
    "Mi355xIndexBuilder",
    "IndexHandle",
    "BertConfig",
    "synthetic_state_dict",
    "build_wordpiece_tokenizer",
    "read_flat_ip",
    "write_flat_ip",
]
