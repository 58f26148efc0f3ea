"""Cost of per-query filtered searches (sqe_index_search_filtered_each) on a 10 M x 1024 flat index, top-10.

  point    B in {64, 1024} queries, each with its own random list of 1,000 and of 10,000 rows: ONE
           search_filtered_each_device call ("each") next to a loop of B single-list search_device(filter_ptr=...) calls
           ("loop").  With --loop-only (a library built from the parent commit, chosen through SQE_LIB, has no
           per-query call) only the loop runs.  The B = 64 x 1,000 results of the two are compared.
  rows     1 query over 1 list of 10^3 .. 10^6 rows, direct against gathered, each forced by the options.
  queries  1 .. 1024 queries over one list of 10,000 rows, direct against gathered.
  rate     the B = 1024 x 1,000 call alone, a few times: run it under `rocprofv3 --kernel-trace --stats` for the
           scoring kernel's time; bytes of master rows read = B x rows x dim x 4.
Per case: wall time per call (median of 5 after one warm-up) and the profiler's stage times (sqe_stats).

usage (GPU box): python tools/filter_each_bench.py [--rows N] [--out file.jsonl] [--modes point,rows,queries] [--loop-only]
-> one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--out", default="")
ap.add_argument("--modes", default="point,rows,queries")
ap.add_argument("--loop-only", action="store_true")
ap.add_argument("--tag", default="")
args = ap.parse_args()

from semantic_query_engine_amd import _native

if args.loop_only:                                       # a library without the per-query call still binds
    for name in ("sqe_index_search_filtered_each", "sqe_index_search_filtered_each_device"):
        _native.SIGNATURES.pop(name, None)

from semantic_query_engine_amd import Context, VectorIndex

D, K = 1024, 10
ROWS = args.rows
CHUNK = 1 << 20
dev = torch.device("cuda", 0)
ALL_DIRECT = {"filter_each_direct_rows": 1 << 30, "filter_each_direct_queries": 1 << 30}
ALL_GATHERED = {"filter_each_direct_rows": 0}


def emit(rec):
    rec = {"lib": os.path.basename(os.path.dirname(_native.LIB_PATH)) + "/" + os.path.basename(_native.LIB_PATH), "tag": args.tag, **rec}
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
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


def timed(ctx, fn, reps=5, warm=1):
    out = []
    for i in range(warm + reps):
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(out), 3), [round(v, 3) for v in out]


def profiled(ctx, fn):
    ctx.synchronize()
    ctx.stats_reset()
    ctx.set_profiling(True)
    fn()
    ctx.synchronize()
    st = ctx.stats()
    ctx.set_profiling(False)
    return {key: round(st[key], 3) for key in ("prep_ms", "scan_ms", "select_ms")}


def distinct_ids(rng, rows):
    """`rows` distinct random ids in random order, without permuting the whole id range"""
    if rows * 4 >= ROWS:
        return rng.permutation(ROWS)[:rows]
    ids = np.unique(rng.integers(0, ROWS, rows + rows // 8 + 16))
    while ids.size < rows:
        ids = np.unique(np.concatenate([ids, rng.integers(0, ROWS, rows)]))
    return rng.permutation(ids)[:rows]


class Case:
    """n_lists random lists of `rows` ids each; query b names list list_of_query[b]"""

    def __init__(self, rng, b, n_lists, rows, loq=None):
        self.b, self.rows = b, rows
        ids = np.stack([distinct_ids(rng, rows) for _ in range(n_lists)])
        self.allow = torch.from_numpy(ids.astype(np.int64).reshape(-1)).to(dev)
        self.offsets = (np.arange(n_lists + 1, dtype=np.int64) * rows)
        self.loq = np.arange(b, dtype=np.int32) if loq is None else loq
        g = torch.Generator(device=dev).manual_seed(99)
        self.q = torch.randn((b, D), generator=g, device=dev)
        self.cos = torch.empty((b, K), device=dev)
        self.ids = torch.empty((b, K), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def each(self, idx):
        idx.search_filtered_each_device(self.q.data_ptr(), self.b, K, self.allow.data_ptr(), self.offsets, self.loq,
                                        self.cos.data_ptr(), self.ids.data_ptr())

    def loop(self, idx):
        qp, cp, ip, ap_ = self.q.data_ptr(), self.cos.data_ptr(), self.ids.data_ptr(), self.allow.data_ptr()
        for j in range(self.b):
            f = int(self.loq[j])
            idx.search_device(qp + j * D * 4, 1, K, cp + j * K * 4, ip + j * K * 8, filter_ptr=ap_ + int(self.offsets[f]) * 8,
                              n_filter=self.rows)

    def result(self, ctx):
        ctx.synchronize()
        return self.cos.cpu().numpy().copy(), self.ids.cpu().numpy().copy()


def options(idx, opts):
    for key, value in opts.items():
        idx.set_option(key, value)


def main():
    ctx = Context(0)
    idx = build(ctx)
    rng = np.random.default_rng(5)
    modes = args.modes.split(",")
    if "point" in modes:
        for b in (64, 1024):
            for rows in (1000, 10000):
                case = Case(rng, b, b, rows)
                rec = {"what": "point", "index_rows": ROWS, "batch": b, "list_rows": rows, "k": K}
                if not args.loop_only:
                    wall, all_ = timed(ctx, lambda: case.each(idx))
                    emit({**rec, "call": "each", "wall_ms": wall, "runs_ms": all_, **profiled(ctx, lambda: case.each(idx))})
                    got = case.result(ctx)
                wall, all_ = timed(ctx, lambda: case.loop(idx))
                emit({**rec, "call": "loop", "wall_ms": wall, "runs_ms": all_})
                if not args.loop_only and b == 64:
                    ref = case.result(ctx)
                    emit({**rec, "what": "check_each_vs_loop", "same_ids": bool(np.array_equal(got[1], ref[1])),
                          "same_cos": bool(np.array_equal(got[0], ref[0]))})
                del case
    if "rows" in modes and not args.loop_only:
        for rows in (1000, 3000, 10_000, 30_000, 100_000, 300_000, 1_000_000):
            case = Case(rng, 1, 1, rows)
            for route, opts in (("direct", ALL_DIRECT), ("gathered", ALL_GATHERED)):
                options(idx, opts)
                wall, all_ = timed(ctx, lambda: case.each(idx))
                emit({"what": "rows", "index_rows": ROWS, "batch": 1, "list_rows": rows, "route": route, "wall_ms": wall, "runs_ms": all_,
                      **profiled(ctx, lambda: case.each(idx))})
            del case
    if "queries" in modes and not args.loop_only:
        for nq in (1, 4, 16, 32, 64, 128, 256, 1024):
            case = Case(rng, nq, 1, 10_000, loq=np.zeros(nq, np.int32))
            for route, opts in (("direct", ALL_DIRECT), ("gathered", ALL_GATHERED)):
                options(idx, opts)
                wall, all_ = timed(ctx, lambda: case.each(idx))
                emit({"what": "queries", "index_rows": ROWS, "batch": nq, "list_rows": 10_000, "route": route, "wall_ms": wall, "runs_ms": all_,
                      **profiled(ctx, lambda: case.each(idx))})
            del case
    if "rate" in modes and not args.loop_only:
        options(idx, ALL_DIRECT)
        case = Case(rng, 1024, 1024, 1000)
        wall, all_ = timed(ctx, lambda: case.each(idx), reps=5, warm=2)
        emit({"what": "rate", "index_rows": ROWS, "batch": 1024, "list_rows": 1000, "wall_ms": wall, "runs_ms": all_,
              "master_bytes_read": 1024 * 1000 * D * 4})
    idx.close()


if __name__ == "__main__":
    main()
