"""Same-process A/B of two builds of the library on the calls that walk a ranking or build range lims, each call alone.

    python tools/ab_ranking_walk.py parent=/path/to/libsskd_amd.so new=semantic-search-kd_amd/libsskd_amd.so

Every named library is loaded into ONE process and bound with ``_native.SIGNATURES``; the inputs are made once (device
tensors, shared by all libraries); per leg the libraries take turns, round after round (A, B, A, B, ...), ``--iters``
back-to-back calls between two events per turn.  One JSON line per leg: median and min / max of the rounds per library,
and whether each later library's median lies inside the first one's min-max.  The outputs of the libraries are compared
bitwise once per leg.  Legs (shapes of the per-feature tools): mine select, hybrid fuse (rrf), MMR select
at 50 / 100 / 200 candidates, Rocchio, RM3, rank denoise, grouped search, range search, range merge.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from semantic_search_kd_amd import BM25Index, _native  # noqa: E402
from semantic_search_kd_amd.expand import expanded_lims  # noqa: E402

DIM = 384


def bind(path):
    lib = C.CDLL(str(path))
    for name, (res, args) in _native.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def stream():
    return int(torch.cuda.current_stream().cuda_stream)


def unit_rows(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((n, DIM), generator=g, device="cuda")
    return x / x.norm(dim=1, keepdim=True)


def ranking(nq, width, n_rows, seed, dtype=torch.float32):
    """random distinct-enough rows, descending positive scores, a -1 tail on every fourth query"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(0, n_rows, (nq, width), generator=g, device="cuda", dtype=torch.int64)
    ids[::4, (3 * width) // 4:] = -1
    s = torch.rand((nq, width), generator=g, device="cuda", dtype=torch.float64) + 0.01
    return torch.sort(s, dim=1, descending=True).values.to(dtype).contiguous(), ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="name=path, the reference build first")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    libs = [(s.split("=", 1)[0], bind(s.split("=", 1)[1])) for s in a.libs]
    lib0 = libs[0][1]
    n, nq = a.rows, a.queries
    st = stream()
    rows = unit_rows(n, 1)
    tiled = torch.zeros(int(lib0.sskd_index_tiled_bytes(n)) // 4, dtype=torch.float32, device="cuda")
    _native.check(lib0.sskd_index_add_rows(rows.data_ptr(), n, 0, tiled.data_ptr(), 0, st))
    queries = unit_rows(nq, 2)
    legs = []   # (name, call(lib) -> rc, outputs)

    def leg(name, outputs):
        def deco(fn):
            legs.append((name, fn, outputs))
        return deco

    # ---- mine select: search_k 100, top_k 5, 1 to 3 positives
    S100, I100 = ranking(nq, 100, n, 3)
    n_pos = torch.arange(nq) % 3 + 1
    pos_lims = torch.zeros(nq + 1, dtype=torch.int64)
    pos_lims[1:] = torch.cumsum(n_pos, 0)
    pos_rows = torch.randint(0, n, (int(pos_lims[-1]),), dtype=torch.int32).cuda()
    pos_lims = pos_lims.cuda()
    m_s, m_i = torch.empty((nq, 5), device="cuda"), torch.empty((nq, 5), dtype=torch.int64, device="cuda")
    m_c, m_p = torch.empty(nq, dtype=torch.int32, device="cuda"), torch.empty(nq, device="cuda")

    @leg("mine_select", (m_s, m_i, m_c, m_p))
    def _(lib):
        return lib.sskd_index_mine_select(tiled.data_ptr(), n, queries.data_ptr(), nq, S100.data_ptr(), I100.data_ptr(), 100,
                                          pos_lims.data_ptr(), pos_rows.data_ptr(), None, 0.5, 5, 0, m_s.data_ptr(),
                                          m_i.data_ptr(), m_c.data_ptr(), m_p.data_ptr(), st)

    # ---- hybrid fuse, rrf: depth 100 on both sides, k 10
    B100, J100 = ranking(nq, 100, n, 4, torch.float64)
    h_s = torch.empty((nq, 10), dtype=torch.float64, device="cuda")
    h_i = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
    h_c = torch.empty(nq, dtype=torch.int32, device="cuda")

    @leg("hybrid_fuse_rrf", (h_s, h_i, h_c))
    def _(lib):
        return lib.sskd_hybrid_fuse(None, n, None, S100.data_ptr(), I100.data_ptr(), 100, None, None, None, None, 0, None,
                                    None, B100.data_ptr(), J100.data_ptr(), 100, None, 0, 0.7, 0.3, 60.0, nq, 10, 0,
                                    h_s.data_ptr(), h_i.data_ptr(), h_c.data_ptr(), None, None, st)

    # ---- MMR select: 1 024 queries, the two resident kernels and the staged one
    for fetch_k in (50, 100, 200):
        Sf, If = ranking(1024, fetch_k, n, 5 + fetch_k)
        d_s = torch.empty((1024, 10), device="cuda")
        d_i = torch.empty((1024, 10), dtype=torch.int64, device="cuda")
        d_c = torch.empty(1024, dtype=torch.int32, device="cuda")

        @leg(f"mmr_select_fetch{fetch_k}", (d_s, d_i, d_c))
        def _(lib, Sf=Sf, If=If, d_s=d_s, d_i=d_i, d_c=d_c, fetch_k=fetch_k):
            return lib.sskd_mmr_select(tiled.data_ptr(), n, Sf.data_ptr(), If.data_ptr(), 1024, fetch_k, 0.5, float("inf"), 10,
                                       0, d_s.data_ptr(), d_i.data_ptr(), None, None, d_c.data_ptr(), st)

    # ---- Rocchio: 10 feedback rows of a depth-100 ranking
    r_q = torch.empty((nq, DIM), device="cuda")
    r_c = torch.empty(nq, dtype=torch.int32, device="cuda")

    @leg("prf_rocchio", (r_q, r_c))
    def _(lib):
        return lib.sskd_prf_rocchio(tiled.data_ptr(), n, queries.data_ptr(), nq, S100.data_ptr(), I100.data_ptr(), 100, 10,
                                    1.0, 0.75, 1, r_q.data_ptr(), r_c.data_ptr(), st)

    # ---- RM3 over a BM25 index of 20 000 synthetic texts, 1 024 queries, the index's own depth-100 ranking
    g = np.random.default_rng(6)
    words = np.array([f"w{i}" for i in range(5000)])
    zipf = 1.0 / np.arange(1, 5001)
    zipf /= zipf.sum()
    texts = [" ".join(words[g.choice(5000, int(g.integers(8, 40)), p=zipf)]) for _ in range(20_000)]
    qtexts = [" ".join(words[g.choice(5000, 4, p=zipf)]) for _ in range(1024)]
    bm = BM25Index(device="cuda:0")
    bm.build_from_texts([f"d{i}" for i in range(len(texts))], texts)
    _, offsets, _, _, _ = bm._tables()
    fwd_lims, fwd_terms, fwd_p, n_fwd = bm.forward_tables()
    q_dl, q_dt, q_lims = bm.query_csr_host(qtexts)
    Bq, Jq = bm.search_device(qtexts, 100)
    out_lims = expanded_lims(q_lims, 2, 10)
    d_out_lims = torch.from_numpy(out_lims).cuda()
    o_t = torch.empty(int(out_lims[-1]), dtype=torch.int32, device="cuda")
    o_st = torch.empty((1024, 10), dtype=torch.int32, device="cuda")
    o_sw = torch.empty((1024, 10), dtype=torch.float64, device="cuda")
    o_c, o_f = (torch.empty(1024, dtype=torch.int32, device="cuda") for _ in range(2))

    @leg("prf_rm3", (o_t, o_st, o_sw, o_c, o_f))
    def _(lib):
        return lib.sskd_prf_rm3(fwd_lims.data_ptr(), fwd_terms.data_ptr(), fwd_p.data_ptr(), n_fwd, offsets.data_ptr(),
                                bm.bm25.corpus_size, bm.bm25.n_terms, q_lims.ctypes.data, q_dl.data_ptr(), q_dt.data_ptr(),
                                Bq.data_ptr(), Jq.data_ptr(), 100, None, 1024, 10, 10, 2, 0, out_lims.ctypes.data,
                                d_out_lims.data_ptr(), o_t.data_ptr(), o_st.data_ptr(), o_sw.data_ptr(), o_c.data_ptr(),
                                o_f.data_ptr(), st)

    # ---- rank denoise: a store of `rows` sets of 32 sorted keys drawn from 4 096 values, both rules on
    keys = torch.sort(torch.randint(0, 4096, (n, 48), device="cuda", dtype=torch.int64), dim=1).values
    keep = torch.ones_like(keys, dtype=torch.bool)
    keep[:, 1:] = keys[:, 1:] != keys[:, :-1]
    g_lims = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    g_lims[1:] = torch.cumsum(keep.sum(1), 0)
    g_keys = keys[keep].contiguous()
    aux = torch.rand((nq, 100), device="cuda")
    dn_s, dn_i = torch.empty((nq, 100), device="cuda"), torch.empty((nq, 100), dtype=torch.int64, device="cuda")
    dn_c = torch.empty(nq, dtype=torch.int32, device="cuda")

    @leg("rank_denoise", (dn_s, dn_i, dn_c))
    def _(lib):
        return lib.sskd_rank_denoise(g_lims.data_ptr(), g_keys.data_ptr(), n, S100.data_ptr(), I100.data_ptr(), nq, 100,
                                     pos_lims.data_ptr(), pos_rows.data_ptr(), aux.data_ptr(), 0.7, 0.02, dn_s.data_ptr(),
                                     dn_i.data_ptr(), None, dn_c.data_ptr(), None, None, st)

    # ---- grouped search: documents of 3 rows, k 10, k_rows 32 (the row search and the collapse)
    groups = (torch.arange(n, dtype=torch.int32) // 3).cuda()
    gw = torch.empty(max(int(lib0.sskd_index_search_grouped_workspace_bytes(n, nq, 10, 32)), 1), dtype=torch.uint8, device="cuda")
    gr_s = torch.empty((nq, 10), device="cuda")
    gr_i = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
    gr_g = torch.empty((nq, 10), dtype=torch.int32, device="cuda")
    gr_c, gr_u = (torch.empty(nq, dtype=torch.int32, device="cuda") for _ in range(2))
    gr_n = torch.empty(1, dtype=torch.int32, device="cuda")

    @leg("search_grouped", (gr_s, gr_i, gr_g, gr_c, gr_u, gr_n))
    def _(lib):
        return lib.sskd_index_search_grouped(tiled.data_ptr(), n, queries.data_ptr(), nq, 10, 32, 0, None, groups.data_ptr(),
                                             gr_s.data_ptr(), gr_i.data_ptr(), gr_g.data_ptr(), gr_c.data_ptr(),
                                             gr_u.data_ptr(), gr_n.data_ptr(), gw.data_ptr(), gw.numel(), st)

    # ---- range search: about 10 matches per query; then the merge of 8 runs of that size
    thr = torch.full((nq,), 0.19, device="cuda")
    cap = 64 * nq
    rw = torch.empty(max(int(lib0.sskd_index_range_search_workspace_bytes(n, nq, cap)), 1), dtype=torch.uint8, device="cuda")
    rg_l = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
    rg_s, rg_i = torch.zeros(cap, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")

    @leg("range_search", (rg_l, rg_s, rg_i))
    def _(lib):
        return lib.sskd_index_range_search(tiled.data_ptr(), n, queries.data_ptr(), nq, thr.data_ptr(), 0, None,
                                           rg_l.data_ptr(), rg_s.data_ptr(), rg_i.data_ptr(), cap, rw.data_ptr(), rw.numel(), st)

    runs, per = 8, 16
    rec = int(lib0.sskd_range_record_bytes(nq, per * nq))
    buf = torch.zeros(runs * rec, dtype=torch.uint8, device="cuda")
    for r in range(runs):
        cnt = torch.randint(0, per + 1, (nq,), generator=torch.Generator().manual_seed(70 + r))
        lims = torch.zeros(nq + 1, dtype=torch.int64)
        lims[1:] = torch.cumsum(cnt, 0)
        total = int(lims[-1])
        seg = torch.repeat_interleave(torch.arange(nq), cnt)
        sc = torch.rand(total)
        order = torch.argsort(seg.double() * 2 - sc.double(), stable=True)   # per query, score descending
        view = buf[r * rec:(r + 1) * rec]
        view[: (nq + 1) * 8].view(torch.int64).copy_(lims)
        view[(nq + 1) * 8: (nq + 1) * 8 + total * 8].view(torch.int64).copy_(torch.arange(total) * runs + r)
        off = (nq + 1) * 8 + per * nq * 8
        view[off: off + total * 4].view(torch.float32).copy_(sc[order])
    mw = torch.empty(max(int(lib0.sskd_range_merge_workspace_bytes(runs, nq, runs * per * nq)), 1), dtype=torch.uint8, device="cuda")
    mg_l = torch.empty(nq + 1, dtype=torch.int64, device="cuda")
    mg_s = torch.zeros(runs * per * nq, device="cuda")
    mg_i = torch.zeros(runs * per * nq, dtype=torch.int64, device="cuda")

    @leg("range_merge", (mg_l, mg_s, mg_i))
    def _(lib):
        return lib.sskd_range_merge_packed(buf.data_ptr(), runs, nq, per * nq, mg_l.data_ptr(), mg_s.data_ptr(),
                                           mg_i.data_ptr(), runs * per * nq, mw.data_ptr(), mw.numel(), st)

    out = open(a.out, "w") if a.out else None
    for name, call, outputs in legs:
        images = []
        for _, lib in libs:   # warm-up and the bitwise comparison
            _native.check(call(lib))
            torch.cuda.synchronize()
            images.append([t.clone() for t in outputs])
        same = all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for other in images[1:] for x, y in zip(images[0], other))
        times = {k: [] for k, _ in libs}
        for _ in range(a.rounds):
            for k, lib in libs:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    call(lib)
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1) / a.iters)
        ref = times[libs[0][0]]
        line = {"leg": name, "same_bits": same}
        for k, _ in libs:
            line[k] = {"median_ms": round(statistics.median(times[k]), 5), "min_ms": round(min(times[k]), 5),
                       "max_ms": round(max(times[k]), 5)}
            if k != libs[0][0]:
                line[k]["inside_reference_range"] = bool(min(ref) <= statistics.median(times[k]) <= max(ref))
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()


if __name__ == "__main__":
    main()
