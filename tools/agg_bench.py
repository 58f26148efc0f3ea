"""Cost of field aggregations (sqe_index_aggregate_fields) on a 10 M-row flat index (dim 64: the vectors are never read).

Columns: SEL uniform 0 .. 999,999 (so `SEL < f * 1e6` selects the fraction f of the rows, and interval 1000 gives a 1,000-bucket
histogram), BOOL (2 values, 80 % ones), YEAR (35 values), CODE (3,000 values), ZIPF (100 k values, skewed), POS (every row its own).
Per predicate fraction 1 % / 21 % / 100 % and per point -- stats over one and over three columns, dense TERMS on 2 / 35 / 3,000
values, hash TERMS on the skewed and on the all-distinct column, the histogram -- one JSON line with
  wall_ms      median wall time of VectorIndex.aggregate_fields (after one warm-up)
  prep_ms / scan_ms / select_ms   device time of one call from the profiler: bitmap, stats + count passes, select + merge
  host_ms      (a) what a caller did before: match_fields(cap = count), get_field, np.unique / min / max on the host, one run
  match_ms     (b) device time of field_match_kernel alone over the same columns (count_fields with an exists clause per column)
and the answers of the device and of the host way are compared.

usage (GPU box): python tools/agg_bench.py [rows] [out.jsonl]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex

D = 64
ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else ""
CHUNK = 1 << 20
SEL, BOOL, YEAR, CODE, ZIPF, POS = range(6)
FRACTIONS = (0.01, 0.21, 1.0)
dev = torch.device("cuda", 0)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def build(ctx):
    idx = VectorIndex(ctx, D)
    idx.reserve(ROWS)
    for c in range((ROWS + CHUNK - 1) // CHUNK):
        g = torch.Generator(device=dev).manual_seed(1000 + c)
        x = torch.randn((min(CHUNK, ROWS - c * CHUNK), D), generator=g, device=dev)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    rng = np.random.default_rng(5)
    cols = {SEL: rng.integers(0, 1_000_000, ROWS), BOOL: (rng.random(ROWS) < 0.8).astype(np.int64), YEAR: rng.integers(1990, 2025, ROWS),
            CODE: rng.integers(0, 3000, ROWS), ZIPF: np.minimum(rng.zipf(1.3, ROWS), 100_000) * 7919, POS: np.arange(ROWS)}
    ids = np.arange(ROWS, dtype=np.int64)
    for f, col in cols.items():
        idx.set_field(f, ids, col.astype(np.int64))
    return idx, {f: col.astype(np.int64) for f, col in cols.items()}


def device_ms(ctx, fn):
    ctx.stats_reset()
    fn()
    st = ctx.stats()
    return {k: round(st[k], 4) for k in ("prep_ms", "scan_ms", "select_ms")}


def main():
    ctx = Context(0)
    t0 = time.perf_counter()
    idx, cols = build(ctx)
    emit({"what": "build", "rows": ROWS, "s": round(time.perf_counter() - t0, 1), "device": str(ctx.device_info())})
    ctx.set_profiling(True)
    points = [
        ("stats_1col", [(YEAR, "stats")]), ("stats_3col", [(YEAR, "stats"), (CODE, "stats"), (SEL, "stats")]),
        ("terms_dense_2", [(BOOL, "terms", 10)]), ("terms_dense_35", [(YEAR, "terms", 10)]), ("terms_dense_3000", [(CODE, "terms", 10)]),
        ("terms_hash_100k_skewed", [(ZIPF, "terms", 10)]), ("terms_hash_distinct", [(POS, "terms", 10)]),
        ("histogram_1000", [(SEL, "histogram", 1000, 0)]),
    ]
    for frac in FRACTIONS:
        pred = [] if frac == 1.0 else [(SEL, "range", None, int(frac * 1_000_000) - 1)]
        for name, aggs in points:
            run = lambda: idx.aggregate_fields(pred, aggs)                      # noqa: E731
            got = run()
            wall = []
            for _ in range(5):
                t = time.perf_counter()
                run()
                wall.append((time.perf_counter() - t) * 1e3)
            dms = device_ms(ctx, run)
            last = idx.aggregate_last()
            # (b) the match kernel alone over the same columns
            fields = sorted({a[0] for a in aggs})
            match = device_ms(ctx, lambda: idx.count_fields([[(f, "range", None, None) for f in fields]]))["scan_ms"]
            # (a) the host way, once: ids back, values back, NumPy
            t = time.perf_counter()
            count = int(idx.count_fields([pred])[0])
            ids = idx.match_fields([pred], count)[1][0]
            ok = got["selected"] == count
            for a, g in zip(aggs, got["aggs"]):
                v = idx.get_field(a[0], ids)
                if a[1] == "stats":
                    ok &= (g["count"], g["min"], g["max"], g["sum"]) == (v.size, int(v.min()), int(v.max()), int(v.sum()))
                elif a[1] == "terms":
                    u, c = np.unique(v, return_counts=True)
                    order = np.lexsort((u, -c))[:a[2]]
                    ok &= np.array_equal(g["keys"], u[order]) and np.array_equal(g["counts"], c[order]) and g["n_buckets"] == u.size
                else:
                    b = (v - a[3]) // a[2]
                    ok &= np.array_equal(g["counts"], np.bincount(b - b.min())) and g["keys"][0] == b.min() * a[2] + a[3]
            host_ms = (time.perf_counter() - t) * 1e3
            emit({"what": name, "fraction": frac, "selected": got["selected"], "wall_ms": round(statistics.median(wall), 3), **dms,
                  "match_ms": match, "host_ms": round(host_ms, 1), "same": bool(ok), "route": [r["route"] for r in last],
                  "slots": [r["slots"] for r in last], "select_blocks": [r["select_blocks"] for r in last]})


if __name__ == "__main__":
    main()
