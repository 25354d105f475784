#!/usr/bin/env python3
"""Regenerates tests/golden/maxsim_small.json: what the REFERENCE'S OWN ``maxsim_aggregation`` (src/utils/chunk.py)
returns for the chunk scores of ``tests/grouped_cases.py::maxsim_pairs``.

The file holds data only: ``{"pairs": [[chunk_id, score], ...], "doc_scores": {doc_id: score}}``.  The reference
module imports ``transformers`` for its chunker; where that library is missing a stub module stands in (the
aggregation does not touch it), as ``make_golden.py`` does for the reference's other optional imports.

Usage:  SSKD_REFERENCE=<checkout of the reference project> python tests/golden/make_golden_grouped.py
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))          # tests/
sys.path.insert(0, str(HERE.parent.parent))   # repository root (oracle/)

from grouped_cases import maxsim_pairs  # noqa: E402


def _reference_chunk_module():
    ref = os.environ.get("SSKD_REFERENCE", "")
    path = Path(ref, "src", "utils", "chunk.py")
    if not (ref and path.is_file()):
        raise SystemExit("set SSKD_REFERENCE to a checkout of the reference project (the directory holding src/)")
    try:
        import transformers  # noqa: F401
    except Exception:
        stub = types.ModuleType("transformers")
        stub.AutoTokenizer = type("AutoTokenizer", (), {})
        sys.modules["transformers"] = stub
    spec = importlib.util.spec_from_file_location("ref_chunk", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    pairs = maxsim_pairs()
    doc_scores = _reference_chunk_module().maxsim_aggregation([(cid, score) for cid, score in pairs])
    out = HERE / "maxsim_small.json"
    out.write_text(json.dumps({"pairs": pairs, "doc_scores": doc_scores}, indent=1) + "\n")
    print(f"wrote {out}: {len(pairs)} chunk scores, {len(doc_scores)} documents")


if __name__ == "__main__":
    main()
