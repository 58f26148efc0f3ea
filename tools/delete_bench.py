"""Cost of sqe_index_delete on a 10 M x 1024 flat index, and what a search costs after it.

Three deletes, one after the other on the same index: the row with id 0 (every row moves), 1,000 random ids, 1 % of the
rows at random.  For each: wall time of the call, device time of the compaction (the ST_ADD stage events around the
block loop), bytes moved: (4 dim + pitch + 8) per moved row, read once and written once (the staged blocks of
compact.hip move a row twice, so their HBM traffic is twice that), the first batch-1024 search after it (it re-quantises the int8 tail) and the
steady search.  Then a fresh index of the same live rows is built and the two are searched alternately (batch 1024,
top-10): after the delete the index must search like the fresh one.  Run it under `rocprofv3 --kernel-trace --stats` for
the kernel split.

usage (GPU box): python tools/delete_bench.py [rows] [out.jsonl]   -> one JSON line per measurement"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex

D, K, B = 1024, 10, 1024
ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else ""
CHUNK = 1 << 20
PITCH = 2 * D + 128                                   # bytes of a row of the bf16 scan copy (api.hip: one 128-B pad line)
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


def build(ctx, live=None):
    idx = VectorIndex(ctx, D)
    idx.reserve(ROWS if live is None else live.size)
    for c in range((ROWS + CHUNK - 1) // CHUNK):
        x = chunk(c)
        if live is not None:
            lo = c * CHUNK
            sel = live[(live >= lo) & (live < lo + x.shape[0])] - lo
            x = x[torch.from_numpy(sel).to(dev)].contiguous()
        torch.cuda.synchronize()
        if x.shape[0]:
            idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    return idx


def search_ms(ctx, idx, q, cos, ids, reps):
    out = []
    for _ in range(reps):
        ctx.synchronize()
        t = time.perf_counter()
        idx.search_device(q.data_ptr(), B, K, cos.data_ptr(), ids.data_ptr())
        ctx.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ctx = Context(0)
    a = build(ctx)
    gq = torch.Generator(device=dev).manual_seed(99)
    q = torch.randn((B, D), generator=gq, device=dev)
    cos = torch.empty((B, K), device=dev)
    ids = torch.empty((B, K), dtype=torch.int64, device=dev)
    search_ms(ctx, a, q, cos, ids, 3)
    base = statistics.median(search_ms(ctx, a, q, cos, ids, 5))
    emit({"what": "search_before_deletes", "rows": ROWS, "batch": B, "k": K, "ms": round(base, 3)})
    rng = np.random.default_rng(5)
    for name in ("id_0", "1000_random", "1pct_random"):
        live = a.ids()
        if name == "id_0":
            drop = live[:1]
        elif name == "1000_random":
            drop = np.sort(rng.choice(live, 1000, replace=False))
        else:
            drop = np.sort(rng.choice(live, live.size // 100, replace=False))
        p0 = int(np.searchsorted(live, drop[0]))
        moved = live.size - p0 - drop.size                # live rows at or above the first deleted position
        ctx.stats_reset()
        ctx.set_profiling(True)
        ctx.synchronize()
        t = time.perf_counter()
        a.delete(drop)
        wall = (time.perf_counter() - t) * 1e3
        st = ctx.stats()
        ctx.set_profiling(False)
        first = search_ms(ctx, a, q, cos, ids, 1)[0]
        steady = statistics.median(search_ms(ctx, a, q, cos, ids, 5))
        nbytes = 2 * moved * (4 * D + PITCH + 8)           # read + written
        emit({"what": "delete", "case": name, "rows_before": int(live.size), "deleted": int(drop.size), "first_position": p0,
              "moved_rows": int(moved), "wall_ms": round(wall, 3), "compaction_device_ms": round(st["add_ms"], 3),
              "bytes_read_plus_written": int(nbytes), "tb_per_s": round(nbytes / (st["add_ms"] * 1e-3) / 1e12, 3) if st["add_ms"] > 0 else None,
              "first_search_ms": round(first, 3), "steady_search_ms": round(steady, 3)})
    # a fresh index of the same live rows, searched alternately with the one that had the deletes
    live = a.ids()
    b = build(ctx, live)
    assert len(b) == live.size
    ca, ia = torch.empty_like(cos), torch.empty_like(ids)
    cb, ib = torch.empty_like(cos), torch.empty_like(ids)
    a.search_device(q.data_ptr(), B, K, ca.data_ptr(), ia.data_ptr())
    b.search_device(q.data_ptr(), B, K, cb.data_ptr(), ib.data_ptr())
    ctx.synchronize()
    ia_h, ib_h = ia.cpu().numpy(), ib.cpu().numpy()
    same_ids = bool(np.array_equal(ia_h, np.where(ib_h >= 0, live[np.maximum(ib_h, 0)], -1)))
    max_dcos = float((ca - cb).abs().max().item())
    ta, tb = [], []
    for _ in range(10):
        ta += search_ms(ctx, a, q, cos, ids, 3)
        tb += search_ms(ctx, b, q, cos, ids, 3)
    emit({"what": "search_after_1pct_vs_fresh", "rows": int(live.size), "batch": B, "k": K, "same_ids": same_ids, "max_abs_dcos": max_dcos,
          "deleted_ms_median": round(statistics.median(ta), 3), "fresh_ms_median": round(statistics.median(tb), 3),
          "deleted_ms_min_max": [round(min(ta), 3), round(max(ta), 3)], "fresh_ms_min_max": [round(min(tb), 3), round(max(tb), 3)]})


if __name__ == "__main__":
    main()
