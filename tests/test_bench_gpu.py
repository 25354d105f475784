"""``bench.py`` without ``--full``: only the headline search is set up, warmed up and timed."""
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

FULL_ONLY = ("cpu_baseline", "parity", "search_anisotropic", "search_locality", "search_cfg3", "encode", "teacher",
             "kd_step")


def test_plain_bench_runs_only_the_headline(gpu, native_lib, tmp_path):
    cmd = [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--corpus", "200000", "--queries", "2000",
           "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["unit"] == "queries/s" and line["higher_is_better"] is True and line["value"] > 0
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["dtype"] == "bf16 screen + f32 exact"
    assert line["roofline"]["kernel_ms"] > 0   # from the HIP events of the timed steps, no run of its own
    assert not [key for key in FULL_ONLY if key in line]
    scores = np.load(tmp_path / "search_scores.npy")
    ids = np.load(tmp_path / "search_ids.npy")
    assert scores.shape == ids.shape == (2000, 10)
    assert ((ids >= 0) & (ids < 200000)).all() and (np.diff(scores, axis=1) <= 0).all()
