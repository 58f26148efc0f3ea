"""Cost of radial searches (sqe_index_range_search) on a 10 M x 1024 flat index.

Rows are seeded Gaussians; the queries are perturbed copies of rows.  Per query the thresholds are taken from a torch fp32
product (computed in row chunks) so that about 0, 10, 100, 1 k, 10 k and 100 k rows match; at batch 64 also -1 (every row).
Per case: wall time per call, host to host (median of 5 after one warm-up; 1 call for -1), the scan_ms / select_ms split from
the profiler (sqe_stats), the exact match counts, and the bf16 bytes the collect scans read per scan millisecond (one pass
over the rows per query group unless a query had more than 4096 candidates).  In the same run: the top-10 search of the same
index with scan_mode BF16_RESCORE and with the default int8 first pass.  Run it under `rocprofv3 --kernel-trace --stats`
for the kernel split.

usage (GPU box): python tools/range_bench.py [rows] [out.jsonl]   -> one JSON line per measurement"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from semantic_query_engine_amd import SCAN_BF16_RESCORE, SCAN_INT8_RESCORE, Context, VectorIndex

D, K = 1024, 10
ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else ""
CHUNK = 1 << 20
BATCHES = (1, 64, 1024)
TARGETS = (0, 10, 100, 1000, 10_000, 100_000)
MAX_HITS = 10
dev = torch.device("cuda", 0)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def chunk(c):
    g = torch.Generator(device=dev).manual_seed(1000 + c)
    return torch.randn((min(CHUNK, ROWS - c * CHUNK), D), generator=g, device=dev)


def timed(ctx, fn, reps):
    out = []
    for _ in range(reps):
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def profiled(ctx, fn):
    ctx.synchronize()
    ctx.stats_reset()
    ctx.set_profiling(True)
    fn()
    ctx.synchronize()
    st = ctx.stats()
    ctx.set_profiling(False)
    return st


def main():
    ctx = Context(0)
    idx = VectorIndex(ctx, D)
    idx.reserve(ROWS)
    for c in range((ROWS + CHUNK - 1) // CHUNK):
        x = chunk(c)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    # queries: perturbed copies of rows
    bmax = max(BATCHES)
    rng = np.random.default_rng(7)
    src = np.sort(rng.choice(ROWS, bmax, replace=False))
    gq = torch.Generator(device=dev).manual_seed(99)
    q = torch.empty((bmax, D), device=dev)
    for c in range((ROWS + CHUNK - 1) // CHUNK):
        sel = src[(src >= c * CHUNK) & (src < (c + 1) * CHUNK)]
        if sel.size:
            rows = torch.from_numpy(sel - c * CHUNK).to(dev)
            q[torch.from_numpy(np.searchsorted(src, sel)).to(dev)] = chunk(c)[rows]
    q = q + 1.5 * torch.randn((bmax, D), generator=gq, device=dev)
    # the best 100 001 fp32 cosines of every query, chunk by chunk
    qn = q / (q.norm(dim=1, keepdim=True) + 1e-9)
    top = None
    kk = max(TARGETS) + 1
    for c in range((ROWS + CHUNK - 1) // CHUNK):
        x = chunk(c)
        s = qn @ (x / (x.norm(dim=1, keepdim=True) + 1e-9)).T
        part = torch.topk(s, min(kk, s.shape[1]), dim=1).values
        top = part if top is None else torch.topk(torch.cat([top, part], 1), kk, dim=1).values
        del x, s
    top = top.cpu().numpy()
    thr = {}
    for t in TARGETS:
        thr[t] = (top[:, 0] + 0.01) if t == 0 else (top[:, t - 1] + top[:, t]) / 2
    cnt = torch.empty(bmax, dtype=torch.int64, device=dev)
    cos = torch.empty((bmax, max(MAX_HITS, K)), device=dev)
    ids = torch.empty((bmax, max(MAX_HITS, K)), dtype=torch.int64, device=dev)
    for b in BATCHES:
        qb = q[:b].contiguous()
        for mode, name in ((SCAN_BF16_RESCORE, "search_bf16"), (SCAN_INT8_RESCORE, "search_int8")):
            idx.set_option("scan_mode", mode)
            run = lambda: idx.search_device(qb.data_ptr(), b, K, cos.data_ptr(), ids.data_ptr())
            timed(ctx, run, 2)
            st = profiled(ctx, run)
            emit({"what": name, "rows": ROWS, "batch": b, "k": K, "wall_ms": round(statistics.median(timed(ctx, run, 5)), 3),
                  "scan_ms": round(st["scan_ms"], 3), "select_ms": round(st["select_ms"], 3), "sample_ms": round(st["sample_ms"], 3)})
        idx.set_option("scan_mode", SCAN_BF16_RESCORE)
        cases = [(t, thr[t][:b]) for t in TARGETS] + ([(-1, np.full(b, -1.0))] if b == 64 else [])
        for target, tv in cases:
            td = torch.from_numpy(np.ascontiguousarray(tv, np.float32)).to(dev)
            run = lambda: idx.range_search_device(qb.data_ptr(), b, td.data_ptr(), MAX_HITS, cnt.data_ptr(), cos.data_ptr(), ids.data_ptr())
            reps = 1 if target in (-1, 100_000) else 5
            if reps > 1:
                timed(ctx, run, 1)
            st = profiled(ctx, run)
            wall = statistics.median(timed(ctx, run, reps))
            counts = cnt[:b].cpu().numpy()
            bf16_bytes = ROWS * D * 2 * ((b + 1023) // 1024)
            emit({"what": "range", "rows": ROWS, "batch": b, "target_matches": target, "max_hits": MAX_HITS, "reps": reps,
                  "wall_ms": round(wall, 3), "scan_ms": round(st["scan_ms"], 3), "select_ms": round(st["select_ms"], 3),
                  "prep_ms": round(st["prep_ms"], 3), "matches_median": int(np.median(counts)), "matches_min": int(counts.min()),
                  "matches_max": int(counts.max()),
                  "first_pass_tb_per_s": round(bf16_bytes / (st["scan_ms"] * 1e-3) / 1e12, 3) if st["scan_ms"] > 0 else None})


if __name__ == "__main__":
    main()
