"""Cost of filtered searches (sqe_index_search_filtered) on a 10 M x 1024 flat index, top-10.

Allowed fractions 0.01 %, 0.1 %, 1 %, 10 %, 50 % and 100 % of the rows (random ids), at batch 1, 64 and 1024, next to
the unfiltered search of the same index.  Per case: wall time per call (median of 5 after one warm-up), and the device
time of the stages from the profiler (sqe_stats):
  * ids -> positions: the prep time of a call whose list names the same number of ids, all outside the index (the
    mark / popcount / scan / write kernels run, nothing is gathered);
  * gather: the rest of the prep time of the real call (the gather kernel, the zeroing of stale rows, the query
    normalisation), with the bytes it reads and writes: (4 dim + 2 dim) per row, read once and written once;
  * search: scan + select (+ collect) of the sub-index.
Each filtered result of batch 64 is checked against a fresh index of the allowed rows (fractions up to 10 %): the ids
must map back exactly and the cosines must be equal.  Run it under `rocprofv3 --kernel-trace --stats` for the kernel split.

usage (GPU box): python tools/filter_bench.py [rows] [out.jsonl]   -> one JSON line per measurement"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex

D, K = 1024, 10
ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else ""
CHUNK = 1 << 20
FRACTIONS = (0.0001, 0.001, 0.01, 0.1, 0.5, 1.0)
BATCHES = (1, 64, 1024)
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


def build(ctx, rows=None):
    """The index of all rows, or of the rows `rows` (ascending ids) only."""
    idx = VectorIndex(ctx, D)
    idx.reserve(ROWS if rows is None else max(rows.size, 1))
    for c in range((ROWS + CHUNK - 1) // CHUNK):
        x = chunk(c)
        if rows is not None:
            lo = c * CHUNK
            sel = rows[(rows >= lo) & (rows < lo + x.shape[0])] - lo
            x = x[torch.from_numpy(sel).to(dev)].contiguous()
        torch.cuda.synchronize()
        if x.shape[0]:
            idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    return idx


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
    a = build(ctx)
    gq = torch.Generator(device=dev).manual_seed(99)
    q_all = torch.randn((max(BATCHES), D), generator=gq, device=dev)
    cos = torch.empty((max(BATCHES), K), device=dev)
    ids = torch.empty((max(BATCHES), K), dtype=torch.int64, device=dev)
    rng = np.random.default_rng(5)
    for b in BATCHES:
        q = q_all[:b]
        run = lambda: a.search_device(q.data_ptr(), b, K, cos.data_ptr(), ids.data_ptr())
        timed(ctx, run, 2)
        st = profiled(ctx, run)
        emit({"what": "unfiltered", "rows": ROWS, "batch": b, "k": K, "wall_ms": round(statistics.median(timed(ctx, run, 5)), 3),
              "device_ms": round(st["prep_ms"] + st["scan_ms"] + st["select_ms"] + st["sample_ms"], 3)})
    for frac in FRACTIONS:
        m = max(1, int(round(frac * ROWS)))
        allowed = np.sort(rng.choice(ROWS, m, replace=False)) if m < ROWS else np.arange(ROWS)
        allow_d = torch.from_numpy(rng.permutation(allowed)).to(dev)
        outside_d = torch.arange(ROWS, ROWS + m, dtype=torch.int64, device=dev)      # same count, none in the index
        for b in BATCHES:
            q = q_all[:b]
            run = lambda: a.search_device(q.data_ptr(), b, K, cos.data_ptr(), ids.data_ptr(), filter_ptr=allow_d.data_ptr(), n_filter=m)
            none = lambda: a.search_device(q.data_ptr(), b, K, cos.data_ptr(), ids.data_ptr(), filter_ptr=outside_d.data_ptr(), n_filter=m)
            timed(ctx, run, 1)
            st0 = profiled(ctx, none)
            st = profiled(ctx, run)
            wall = statistics.median(timed(ctx, run, 5))
            gather_ms = max(st["prep_ms"] - st0["prep_ms"], 0.0)
            nbytes = 2 * m * (4 * D + 2 * D)
            emit({"what": "filtered", "rows": ROWS, "fraction": frac, "allowed": m, "batch": b, "k": K,
                  "wall_ms": round(wall, 3), "ids_to_positions_ms": round(st0["prep_ms"], 3), "gather_ms": round(gather_ms, 3),
                  "gather_bytes_read_plus_written": nbytes,
                  "gather_tb_per_s": round(nbytes / (gather_ms * 1e-3) / 1e12, 3) if gather_ms > 0 else None,
                  "search_ms": round(st["scan_ms"] + st["select_ms"] + st["sample_ms"], 3),
                  "device_ms": round(st["prep_ms"] + st["scan_ms"] + st["select_ms"] + st["sample_ms"], 3)})
        if frac <= 0.1:
            # exactness: the filtered search == an unfiltered search of a fresh index of the allowed rows (batch 64)
            b = 64
            q = q_all[:b]
            fa_c, fa_i = torch.empty((b, K), device=dev), torch.empty((b, K), dtype=torch.int64, device=dev)
            fb_c, fb_i = torch.empty_like(fa_c), torch.empty_like(fa_i)
            a.search_device(q.data_ptr(), b, K, fa_c.data_ptr(), fa_i.data_ptr(), filter_ptr=allow_d.data_ptr(), n_filter=m)
            ctx.synchronize()
            f = build(ctx, allowed)
            f.search_device(q.data_ptr(), b, K, fb_c.data_ptr(), fb_i.data_ptr())
            ctx.synchronize()
            ia, ib = fa_i.cpu().numpy(), fb_i.cpu().numpy()
            emit({"what": "check_vs_fresh", "fraction": frac, "allowed": m, "batch": b,
                  "same_ids": bool(np.array_equal(ia, np.where(ib >= 0, allowed[np.maximum(ib, 0)], -1))),
                  "same_cos": bool(torch.equal(fa_c, fb_c))})
            f.close()
            del f
        del allow_d, outside_d


if __name__ == "__main__":
    main()
