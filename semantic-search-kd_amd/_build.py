"""In-tree build of the gfx950 C-ABI library (``libsskd_amd.so``).

``hipcc --offload-arch=gfx950`` cross-compiles without a GPU, so this runs in the
CPU-only build container as well as on the MI355X box.  The shared object is
written next to this file (git-ignored, but it travels with the repo snapshot).
"""
from __future__ import annotations

import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
REPO_ROOT = PKG_DIR.parent
CSRC = PKG_DIR / "csrc"
INCLUDE = REPO_ROOT / "include"
OBJ_DIR = PKG_DIR / "build"
LIB_PATH = PKG_DIR / "libsskd_amd.so"

# search.hip and screen.hip first: they compile longest (the scan's and the screening kernel's instantiations)
SOURCES = ["search.hip", "screen.hip", "capi_common.hip", "index_rows.hip", "range.hip", "grouped.hip", "dedup.hip", "mine.hip", "denoise.hip", "bm25.hip", "hybrid.hip", "expand.hip", "mmr.hip", "eval.hip", "ivf.hip", "pq.hip", "graph.hip", "late.hip", "late_train.hip", "plaid.hip", "pool.hip", "encoder.hip", "kd_loss.hip", "tokenizer.hip", "generic.hip", "train.hip", "blaslt.hip", "testhooks.hip"]
HIPCC_FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-Wno-unused-result",
    "-Wno-unused-value",
    # keep scalar f32 VALU ops scalar: SLP-packed v_pk_* lose the free abs/neg source modifiers and
    # cost the in-order producer waves of the fused MLP ~25 % (measured)
    "-fno-slp-vectorize",
]


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(exe).exists():
        raise RuntimeError("hipcc not found: the MI355X backend needs the ROCm toolchain to build")
    return exe


def _newer(target: Path, deps) -> bool:
    if not target.exists():
        return False
    t = target.stat().st_mtime
    return all(t >= Path(d).stat().st_mtime for d in deps)


def _jobs() -> int:
    """Concurrent compiles: MAX_JOBS if set, else 8, at most 16 (never the machine's CPU count: a shared box shows all of them)."""
    return max(1, min(int(os.environ.get("MAX_JOBS") or 8), 16))


def build_native(force: bool = False, verbose: bool = False) -> Path:
    """Compile every stale HIP translation unit for gfx950, several at a time, and link the C-ABI library."""
    OBJ_DIR.mkdir(exist_ok=True)
    headers = list(CSRC.glob("*.h")) + list(INCLUDE.glob("*.h"))
    objs = []
    stale = []
    for name in SOURCES:
        src = CSRC / name
        if not src.exists():
            raise RuntimeError(f"missing source {src}")
        obj = OBJ_DIR / (src.stem + ".o")
        if force or not _newer(obj, [src, *headers]):
            stale.append([_hipcc(), *HIPCC_FLAGS, f"-I{INCLUDE}", f"-I{CSRC}", "-c", str(src), "-o", str(obj)])
        objs.append(obj)

    def compile_one(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    if stale:
        with ThreadPoolExecutor(max_workers=_jobs()) as pool:
            # every compile runs to its end; the first failure (in SOURCES order) is raised, its command in the exception
            for done in [pool.submit(compile_one, cmd) for cmd in stale]:
                done.result()
    if stale or force or not _newer(LIB_PATH, objs):
        # hipBLASLt: plain large-K library GEMMs of the teacher (csrc/blaslt.hip); everything else is this repo's kernels
        cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", str(LIB_PATH), *map(str, objs), "-lhipblaslt"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB_PATH


if __name__ == "__main__":
    print(build_native(force="--force" in os.sys.argv, verbose=True))
