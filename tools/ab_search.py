"""Same-box A/B of screened-search variants: ``python tools/ab_search.py lib_a.so lib_b.so ...`` loads every
library in ONE process and times the screening kernel (HIP events around it) alternately at the bench shape.
AB_STAMPS=1: every library listed was built with -DSSKD_SCREEN_STAMPS (tools/ab_build.py); the finish-time stamps of
its last call are read back from the tail of the workspace and summarised (use with AB_NOCHECK-style care: the stamp
stores are part of the timed kernel).  AB_CALLS=1 also prints every timed call of every library (block means against a
spread: profiles/readahead/README.md)."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
from semantic_search_kd_amd import _native  # noqa: E402

N, NQ, K = int(os.environ.get('AB_ROWS', 1_000_000)), int(os.environ.get('AB_NQ', 10_000)), 10
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(1)
corpus = torch.nn.functional.normalize(torch.randn((N, 384), generator=g, device=dev), dim=1)
queries = torch.nn.functional.normalize(torch.randn((NQ, 384), generator=g, device=dev), dim=1)
hip = C.CDLL("libamdhip64.so")
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
st = int(torch.cuda.current_stream(dev).cuda_stream)
names = ("sskd_index_tiled_bytes", "sskd_index_add_rows", "sskd_index_bf16_bytes", "sskd_index_make_bf16",
         "sskd_index_search_screened_workspace_bytes", "sskd_index_search_screened", "sskd_index_search_workspace_bytes",
         "sskd_index_search_profiled", "sskd_index_search_screened_plan")
EXACT = bool(os.environ.get("AB_EXACT"))   # time the plain exact fp32 scan instead of the screened search
ROUNDS = int(os.environ.get("AB_ROUNDS", 7))
libs, ref = [], None
for path in sys.argv[1:]:
    lib = C.CDLL(str(Path(path).resolve()))
    for n in names:
        fn = getattr(lib, n)
        fn.restype, fn.argtypes = _native.SIGNATURES[n]
    tiled = torch.empty(int(lib.sskd_index_tiled_bytes(N)) // 4, dtype=torch.float32, device=dev)
    assert lib.sskd_index_add_rows(corpus.data_ptr(), N, 0, tiled.data_ptr(), 0, st) == 0
    bf = torch.empty(int(lib.sskd_index_bf16_bytes(N)), dtype=torch.uint8, device=dev)
    assert lib.sskd_index_make_bf16(tiled.data_ptr(), N, bf.data_ptr(), st) == 0
    ws = torch.empty(int(lib.sskd_index_search_workspace_bytes(N, NQ, K) if EXACT else
                         lib.sskd_index_search_screened_workspace_bytes(N, NQ, K)), dtype=torch.uint8, device=dev)
    libs.append((Path(path).stem, lib, tiled, bf, ws))
out_s = torch.empty((NQ, K), device=dev)
out_i = torch.empty((NQ, K), dtype=torch.int64, device=dev)
status = torch.zeros(2, dtype=torch.int32, device=dev)
times = {n: [] for n, *_ in libs}
wall = {n: [] for n, *_ in libs}
fallbacks = {n: 0 for n, *_ in libs}
for r in range(ROUNDS):
    for n, lib, tiled, bf, ws in libs:
        a, b = C.c_void_p(), C.c_void_p()
        hip.hipEventCreate(C.byref(a)); hip.hipEventCreate(C.byref(b))
        torch.cuda.synchronize()
        import time
        t0 = time.perf_counter()
        if EXACT:
            rc = lib.sskd_index_search_profiled(tiled.data_ptr(), N, queries.data_ptr(), NQ, K, 0, out_s.data_ptr(),
                                                out_i.data_ptr(), ws.data_ptr(), ws.numel(), st, a, b)
        else:
            rc = lib.sskd_index_search_screened(tiled.data_ptr(), bf.data_ptr(), N, queries.data_ptr(), NQ, K, 0, out_s.data_ptr(),
                                                out_i.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st, a, b)
        assert rc == 0, rc
        torch.cuda.synchronize()
        wall[n].append((time.perf_counter() - t0) * 1e3)
        ms = C.c_float()
        hip.hipEventSynchronize(b); hip.hipEventElapsedTime(C.byref(ms), a, b)
        times[n].append(ms.value)
        if not EXACT:
            fallbacks[n] = max(fallbacks[n], int(status[1]))
        if ref is None:
            ref = (out_s.clone(), out_i.clone())
        if not os.environ.get('AB_NOCHECK'):
            assert torch.equal(out_i, ref[1]) and torch.equal(out_s, ref[0]) and int(status[0]) == 0, n
for n in times:
    print(f"{n}: screen kernel median {np.median(times[n][1:]):.3f} ms (min {np.min(times[n][1:]):.3f}, max {np.max(times[n][1:]):.3f}, mean {np.mean(times[n][1:]):.3f}); whole call {np.median(wall[n][1:]):.3f} ms"
          + ("" if EXACT else f"; exact-fallback queries {fallbacks[n]}"), flush=True)
if os.environ.get("AB_CALLS"):   # AB_CALLS=1: every timed call, for block means (the first call of a library is left out above)
    for n in times:
        print(f"{n}: calls " + " ".join(f"{t:.3f}" for t in times[n][1:]), flush=True)


def stamp_report(name, lib, ws, waves=12):
    """Finish times of the screening kernel's waves (s_memrealtime at entry / after the sample phase / after the tile
    loop, per wave, indexed by blockIdx), as shares of the launch = first entry .. last end."""
    qpb, passes, nsl = C.c_int(), C.c_int(), C.c_int()
    assert lib.sskd_index_search_screened_plan(N, NQ, K, C.byref(qpb), C.byref(passes), C.byref(nsl)) == 0
    nqb, nsl = passes.value, nsl.value
    wgs = nqb * nsl
    nbytes = wgs * waves * 3 * 8
    start = ws.numel() - ((nbytes + 255) & ~255)   # the carve's last block, 256-byte aligned
    s = ws[start:start + nbytes].view(torch.int64).cpu().numpy().reshape(wgs, waves, 3).astype(np.float64)
    b = np.arange(wgs)
    xcd = b & 7
    logical = xcd * (wgs >> 3) + np.minimum(xcd, wgs & 7) + (b >> 3)   # the kernel's XCD swizzle
    slice_, qblk = logical // nqb, logical % nqb
    t0, t1 = s[:, :, 0].min(), s[:, :, 2].max()
    L = t1 - t0
    if not 0 < L < 1e9:   # ten seconds of the 100 MHz clock: not a screening launch
        print(f"{name}: no stamps at the tail of the workspace (library built without -DSSKD_SCREEN_STAMPS?)")
        return
    end = s[:, :, 2]
    wg_end = end.max(axis=1)
    a = (end.max(axis=1) - end.min(axis=1)) / L
    qb_spread = np.array([np.ptp(wg_end[qblk == q]) for q in range(nqb)]) / L
    qb_end = np.array([wg_end[qblk == q].max() for q in range(nqb)])
    x_end = np.array([wg_end[xcd == x].max() for x in range(8) if (xcd == x).any()])
    x_mean = np.array([end[xcd == x].mean() for x in range(8) if (xcd == x).any()])
    sl_mean = np.array([end[slice_ == x].mean() for x in range(nsl)])
    print(f"{name}: stamps of {wgs} workgroups ({nqb} query blocks x {nsl} slices, {qpb.value} queries each) x {waves} waves; "
          f"launch {L / 100.0:.1f} us (100 MHz clock)")
    print(f"  (a) end-time spread among the {waves} waves of a workgroup / launch: mean {a.mean():.4f}  median {np.median(a):.4f}  max {a.max():.4f}")
    print(f"  (b) end-time spread among the workgroups of a query block / launch: mean {qb_spread.mean():.4f}  median {np.median(qb_spread):.4f}  max {qb_spread.max():.4f}")
    print(f"  (c) end-time spread among query blocks / launch: {np.ptp(qb_end) / L:.4f}; among XCDs (last wave of each): {np.ptp(x_end) / L:.4f}; "
          f"among XCDs (mean wave end): {np.ptp(x_mean) / L:.4f}; among slices (mean wave end): {np.ptp(sl_mean) / L:.4f}")
    print(f"  (d) mean wave lifetime / launch: {(end - s[:, :, 0]).mean() / L:.4f}   "
          f"(idle before entry {(s[:, :, 0] - t0).mean() / L:.4f}, idle after end {(t1 - end).mean() / L:.4f}; "
          f"sample phase {(s[:, :, 1] - s[:, :, 0]).mean() / L:.4f} of the launch)")
    print(f"      mean idle after end, split: inside the workgroup {((wg_end[:, None] - end).mean()) / L:.4f}, "
          f"workgroup to its query block's last {np.mean([ (wg_end[qblk == q].max() - wg_end[qblk == q]).mean() for q in range(nqb)]) / L:.4f}, "
          f"query block to the launch's last {(t1 - qb_end).mean() / L:.4f}", flush=True)


def appended_entries(lib, ws, waves=12, cap=32, runs=4):
    """mean number of rows a query's runs took in the last call (the counts follow the runs at the head of the carve)"""
    qpb, passes, nsl = C.c_int(), C.c_int(), C.c_int()
    assert lib.sskd_index_search_screened_plan(N, NQ, K, C.byref(qpb), C.byref(passes), C.byref(nsl)) == 0
    lists = nsl.value * waves * runs
    part = (NQ * lists * cap * 4 + 255) & ~255
    cnt = ws[2 * part:2 * part + NQ * lists * 4].view(torch.int32)
    # This mirrors the head of screen_carve (csrc/screen.hip: scores, ids, counts; SCREEN_CAP = 32 entries per run, 12
    # waves x 4 runs - one per 16-lane group - per slice).  A carve that moved would put other data here: a count is a number of rows of ONE
    # wave's tiles, so every word must lie in [0, rows] and their sum within the pairs screened - else refuse to print.
    assert 2 * part + NQ * lists * 4 <= ws.numel(), "workspace smaller than the carve this reader assumes"
    assert int(cnt.min()) >= 0 and int(cnt.max()) <= N and int(cnt.sum()) <= NQ * N, \
        "these are not run counts: screen_carve no longer starts with [scores][ids][counts]?"
    return float(cnt.sum()) / NQ


if os.environ.get("AB_ENTRIES") and not EXACT:   # AB_ENTRIES=1: appended entries per query of every library's last call
    for n, lib, tiled, bf, ws in libs:
        print(f"{n}: appended entries per query {appended_entries(lib, ws):.1f}", flush=True)
if os.environ.get("AB_STAMPS") and not EXACT:
    for n, lib, tiled, bf, ws in libs:
        stamp_report(n, lib, ws)
