"""Cost of field predicates (sqe_index_match_fields / search_where / search_where_each) on a 10 M x 1024 flat index, top-10.

One uniform field (values 0 .. 999,999, so `value < f * 1e6` selects the fraction f of the rows) and one tenant field.  Per
fraction 0.01 / 0.1 / 1 / 6 / 21 / 50 % and batch 1 / 64 / 1024, wall time per call (median after one warm-up) of
  where        VectorIndex.search_where(q, k, pred)                      -- the predicate evaluated on the device
  host_list    np.nonzero on a host copy of the column, then search(q, k, filter_ids=ids)   -- what a caller had to do before
  list_only    the same search with the list already built (the hand-over and the search, without np.nonzero)
  plain        search(q, k)
and the two filtered answers are compared bit for bit.  Then match_fields alone: the device time of field_match_kernel from
the profiler (sqe_stats scan_ms) and the bytes of the columns it reads, per second.  Then search_where_each with 64 queries
naming 64 tenants, against search_filtered_each over host-built lists, for tenants of 1.6 % and of 0.024 % of the rows.

usage (GPU box): python tools/fields_bench.py [rows] [out.jsonl]   -> one JSON line per measurement"""
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
FRACTIONS = (0.0001, 0.001, 0.01, 0.06, 0.21, 0.5)
BATCHES = (1, 64, 1024)
UNIFORM, TENANT, FINE = 0, 1, 2          # field slots: uniform 0..999,999; tenant of 64; tenant of 4,096
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
    return idx


def timed(fn, reps):
    fn()                                  # warm-up
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    ctx = Context(0)
    t0 = time.perf_counter()
    idx = build(ctx)
    rng = np.random.default_rng(7)
    cols = {UNIFORM: rng.integers(0, 1_000_000, ROWS), TENANT: rng.integers(0, 64, ROWS), FINE: rng.integers(0, 4096, ROWS)}
    ids = np.arange(ROWS, dtype=np.int64)
    t1 = time.perf_counter()
    for slot, col in cols.items():
        idx.set_field(slot, ids, col)
    emit({"what": "setup", "rows": ROWS, "dim": D, "build_s": round(t1 - t0, 1), "set_field_s_per_column": round((time.perf_counter() - t1) / 3, 2),
          "field_info": idx.field_info()})
    q_all = np.random.default_rng(8).standard_normal((1024, D)).astype(np.float32)

    # ---- search_where against the host-built list and the plain search
    for B in BATCHES:
        q = q_all[:B]
        reps = 5 if B <= 64 else 3
        plain = timed(lambda: idx.search(q, K), reps)
        emit({"what": "plain", "B": B, "ms": round(plain, 3)})
        for f in FRACTIONS:
            thr = int(f * 1_000_000)
            pred = [(UNIFORM, "range", None, thr - 1)]
            lst = np.nonzero(cols[UNIFORM] < thr)[0].astype(np.int64)
            got = idx.search_where(q, K, pred)
            want = idx.search(q, K, filter_ids=lst)
            same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
            where = timed(lambda: idx.search_where(q, K, pred), reps)
            host = timed(lambda: idx.search(q, K, filter_ids=np.nonzero(cols[UNIFORM] < thr)[0].astype(np.int64)), reps)
            only = timed(lambda: idx.search(q, K, filter_ids=lst), reps)
            emit({"what": "where", "B": B, "fraction": f, "selected": int(lst.size), "where_ms": round(where, 3), "host_list_ms": round(host, 3),
                  "list_only_ms": round(only, 3), "plain_ms": round(plain, 3), "bit_equal": same})

    # ---- match_fields alone: device time of the match kernel, bytes of the columns it reads
    ctx.set_profiling(True)
    some = list(range(0, 4096, 4))
    cases = {
        "1 range, 1 column": ([[(UNIFORM, "range", None, 9_999)]], 1),
        "8 ranges on 1 column": ([[(UNIFORM, "range", 1000 * j, 1000 * j + 9_999)] for j in range(8)], 1),
        "64 predicates, 2 columns": ([[(UNIFORM, "range", 1000 * j, 1000 * j + 9_999), (TENANT, "range", j, j)] for j in range(64)], 2),
        "1 IN of 1024 values": ([[(FINE, "in", some)]], 1),
        "3 columns, 3 clauses": ([[(UNIFORM, "range", None, 499_999), (TENANT, "in", [1, 5, 9], {"not_": True}), (FINE, "range", 100, 3000)]], 3),
    }
    for name, (preds, n_cols) in cases.items():
        idx.count_fields(preds)
        ms = []
        for _ in range(5):
            ctx.stats_reset()
            t = time.perf_counter()
            counts = idx.count_fields(preds)
            wall = (time.perf_counter() - t) * 1e3
            ms.append((ctx.stats()["scan_ms"], wall))
        kernel = statistics.median(m[0] for m in ms)
        emit({"what": "match_fields", "case": name, "predicates": len(preds), "columns": n_cols, "kernel_ms": round(kernel, 4),
              "column_bytes": ROWS * 8 * n_cols, "TB_per_s": round(ROWS * 8 * n_cols / (kernel * 1e-3) / 1e12, 3) if kernel > 0 else None,
              "call_wall_ms": round(statistics.median(m[1] for m in ms), 3), "count0": int(counts[0])})
    ctx.set_profiling(False)

    # ---- search_where_each: 64 queries, 64 tenants
    q = q_all[:64]
    for slot, tenants in ((TENANT, list(range(64))), (FINE, list(range(0, 4096, 64)))):
        preds = [[(slot, "range", t, t)] for t in tenants]
        lists = [np.nonzero(cols[slot] == t)[0].astype(np.int64) for t in tenants]
        got = idx.search_where_each(q, K, preds)
        want = idx.search_filtered_each(q, K, lists)
        same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
        each = timed(lambda: idx.search_where_each(q, K, preds), 3)
        host = timed(lambda: idx.search_filtered_each(q, K, [np.nonzero(cols[slot] == t)[0].astype(np.int64) for t in tenants]), 3)
        only = timed(lambda: idx.search_filtered_each(q, K, lists), 3)
        emit({"what": "where_each", "B": 64, "tenants": 64, "rows_per_tenant": int(np.mean([a.size for a in lists])), "where_each_ms": round(each, 3),
              "host_lists_ms": round(host, 3), "lists_only_ms": round(only, 3), "bit_equal": same})


if __name__ == "__main__":
    main()
