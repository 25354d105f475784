#!/usr/bin/env python3
"""Regenerates tests/golden/text_overlap.json: what the REFERENCE'S OWN ``compute_text_overlap``
(src/utils/chunk.py) returns for the text pairs of ``tests/denoise_cases.py``.

Recorded per pair: the two texts and the returned float as ``float.hex()`` (the bits, not a decimal rendering).  The
6 000-character text of the cases is left out (the file stays small; that text is for the kernels).  The file holds data
only.  The reference's module imports ``loguru`` (logging): where it is missing a stub stands in, as in
``make_golden_eval.py``.

Usage:  SSKD_REFERENCE=<checkout of the reference project> python tests/golden/make_golden_overlap.py
"""
from __future__ import annotations

import json
import os
import sys
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))          # tests/

import denoise_cases  # noqa: E402


def _reference_function():
    ref = os.environ.get("SSKD_REFERENCE", "")
    if not (ref and Path(ref, "src", "utils", "chunk.py").is_file()):
        raise SystemExit("set SSKD_REFERENCE to a checkout of the reference project (the directory holding src/)")
    sys.path.insert(0, ref)
    try:
        import loguru  # noqa: F401
    except Exception:
        stub = types.ModuleType("loguru")

        class _Silent:
            def __getattr__(self, name):
                return lambda *a, **k: None

        stub.logger = _Silent()
        sys.modules["loguru"] = stub
    from src.utils.chunk import compute_text_overlap

    return compute_text_overlap


def main() -> None:
    overlap = _reference_function()
    pairs = [(a, b) for a, b in denoise_cases.text_pairs() if len(a) < 1000 and len(b) < 1000]
    out = [{"a": a, "b": b, "overlap": float(overlap(a, b)).hex()} for a, b in pairs]
    path = HERE / "text_overlap.json"
    path.write_text(json.dumps(out, ensure_ascii=True, indent=0) + "\n")
    values = [float.fromhex(r["overlap"]) for r in out]
    print(f"wrote {path.name}: {len(out)} pairs, {path.stat().st_size / 1024:.1f} KiB; "
          f"{sum(v == 0.0 for v in values)} zeros, {sum(v == 1.0 for v in values)} ones, "
          f"{sum(v > 0.8 for v in values)} above 0.8")


if __name__ == "__main__":
    main()
