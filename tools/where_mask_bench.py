"""The two routes of sqe_index_search_where side by side on the 10 M x 1024 flat index of tools/fields_bench.py.

One uniform field (values 0 .. 999,999, so `value < f * 1e6` selects the fraction f of the rows).  Per fraction 1 / 6 / 21 / 50 /
100 %, batch 1 / 64 / 1024 and k 3 / 10 / 100: the wall time per call of search_where with "where_route" = 1 (gather) and = 2
(mask) in ONE process, the two routes alternating over `--rounds` rounds, each round the median of `--reps` calls after one
warm-up, so that a route's own round-to-round spread stands next to the difference between the routes; the plain search at the
same k; what the mask route's read-back says (depth, first pass, swept); whether the two answers are bit-equal; and what the
automatic route picks.  Where the depth rule has no depth (sqe_where_depth == 0) a forced mask route sweeps nearly every query
over all rows: that point is measured at B = 1 only, to show what it costs, and skipped for larger batches.

Then the correlated case: a flag field refuses the 256 nearest rows of every fourth query, so a quarter of the batch is flagged
whatever the depth and goes through the sweep; swept queries and time per call of both routes at B = 64 and 1024, k = 10.

usage (GPU box): python tools/where_mask_bench.py [--rows N] [--out file.jsonl] [--rounds R] [--reps N] [--skip-correlated]
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--skip-correlated", action="store_true")
args = ap.parse_args()

from semantic_query_engine_amd import Context, VectorIndex, _native
from semantic_query_engine_amd.engine import where_depth

D = 1024
ROWS = args.rows
CHUNK = 1 << 20
FRACTIONS = (0.01, 0.06, 0.21, 0.5, 1.0)
BATCHES = (1, 64, 1024)
KS = (3, 10, 100)
UNIFORM, FLAG = 0, 1
GATHER, MASK = 1, 2
dev = torch.device("cuda", 0)


def emit(rec):
    rec = {"lib": os.path.basename(_native.LIB_PATH), "index_rows": ROWS, **rec}
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


def one_round(fn, reps):
    fn()                                  # warm-up
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def both_routes(idx, q, k, pred, mask_ok):
    """-> ({route: [round medians]}, the mask route's read-back, bit-equal)"""
    times = {GATHER: [], MASK: []}
    last, got = None, {}
    for _ in range(args.rounds):
        for route in (GATHER, MASK):
            if route == MASK and not mask_ok:
                continue
            idx.set_option("where_route", route)
            times[route].append(one_round(lambda: idx.search_where(q, k, pred), args.reps))
            got[route] = idx.search_where(q, k, pred)
            if route == MASK:
                last = idx.where_last()
    idx.set_option("where_route", 0)
    same = None
    if mask_ok:
        same = bool(np.array_equal(got[GATHER][0], got[MASK][0]) and np.array_equal(got[GATHER][1], got[MASK][1]))
    return times, last, same


def summary(ms):
    return {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "rounds": [round(v, 3) for v in ms]} if ms else None


def main():
    ctx = Context(0)
    idx = build(ctx)
    rng = np.random.default_rng(7)
    uniform = rng.integers(0, 1_000_000, ROWS)
    ids = np.arange(ROWS, dtype=np.int64)
    idx.set_field(UNIFORM, ids, uniform)
    q_all = np.random.default_rng(8).standard_normal((1024, D)).astype(np.float32)
    emit({"what": "setup", "dim": D, "rounds": args.rounds, "reps": args.reps})

    for B in BATCHES:
        q = q_all[:B]
        for k in KS:
            plain = [one_round(lambda: idx.search(q, k), args.reps) for _ in range(args.rounds)]
            for f in FRACTIONS:
                thr = int(f * 1_000_000)
                pred = [(UNIFORM, "range", None, thr - 1)]
                selected = int(np.count_nonzero(uniform < thr))
                rule = where_depth(k, selected, ROWS)
                mask_ok = rule > 0 or B == 1
                times, last, same = both_routes(idx, q, k, pred, mask_ok)
                idx.search_where(q, k, pred)                        # the automatic route
                auto = idx.where_last()
                emit({"what": "grid", "B": B, "k": k, "fraction": f, "selected": selected, "rule_depth": rule,
                      "gather": summary(times[GATHER]), "mask": summary(times[MASK]), "plain": summary(plain),
                      "mask_last": last, "bit_equal": same, "auto_route": auto["route"]})

    if args.skip_correlated:
        return
    # ---- the correlated case: the 256 nearest rows of every fourth query are refused
    k = 10
    for B in (64, 1024):
        q = q_all[:B]
        hot = np.arange(0, B, 4)
        _, near = idx.search(q[hot], 256)
        refused = np.unique(near[near >= 0])
        flag = np.zeros(ROWS, np.int64)
        flag[refused] = 1
        idx.set_field(FLAG, ids, flag)
        pred = [(FLAG, "range", 0, 0)]
        selected = ROWS - refused.size
        t0 = time.perf_counter()
        times, last, same = both_routes(idx, q, k, pred, True)
        emit({"what": "correlated", "B": B, "k": k, "flagged_queries": int(hot.size), "refused_rows": int(refused.size), "selected": selected,
              "rule_depth": where_depth(k, selected, ROWS), "gather": summary(times[GATHER]), "mask": summary(times[MASK]),
              "mask_last": last, "bit_equal": same, "case_s": round(time.perf_counter() - t0, 1)})


if __name__ == "__main__":
    main()
