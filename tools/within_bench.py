"""Radial, collapsed and MMR search within a row set on the 10 M x 1024 flat index of tools/where_mask_bench.py: the two routes
side by side, next to the unrestricted call of the same kind and to search_where alone.

One uniform field (values 0 .. 999,999, so `value < f * 1e6` selects the fraction f of the rows) and group keys of 4 rows each.
Per kind (radial at a threshold that leaves a few hundred matches a query, collapsed k = 10, MMR k = 10 over 40 candidates),
fraction 0.01 / 1 / 10 / 50 % and batch 1 / 64 / 1024: the wall time per host call of the restricted call on the gather route
("filter_gather_rows" raised to the whole index, so that it serves every fraction) and on the mask route ("within_route" 2;
MMR: "where_route" 1 / 2), the routes alternating over `--rounds` rounds in ONE process, each round the median of `--reps`
calls after one warm-up; the unrestricted call; search_where at the same k on the route it picks itself; what the read-back says
(depth of the collapsed first stage, swept queries); whether the two routes' answers are bit-equal.  Where the depth rule gives
the mask route of collapsed search no depth (sqe_where_depth == 0: it fetches 256 rows and sweeps nearly every query) the point
is measured at B = 1 only.

`--unchanged`: instead, the calls this change leaves as they were (search, range_search, search_collapsed, search_mmr,
search_where at 50 %) on the same index, with the package under `--root`: run it alternately on a checkout of the parent
commit and on this tree to compare them.

usage (GPU box): python tools/within_bench.py [--rows N] [--out file.jsonl] [--rounds R] [--reps N] [--unchanged] [--root DIR] [--tag T]
-> one JSON line per measurement"""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--out", default="")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--unchanged", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--tag", default="")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex, _native

D = 1024
ROWS = args.rows
CHUNK = 1 << 20
FRACTIONS = (0.0001, 0.01, 0.1, 0.5)
BATCHES = (1, 64, 1024)
K, MAX_HITS, MIN_COS, LAM = 10, 10, 0.115, 0.5
UNIFORM = 0
GATHER_ROWS_DEFAULT = 1 << 20        # "filter_gather_rows" as an index starts with it (include/sqe.h): restored after every point
GATHER, MASK = 1, 2
dev = torch.device("cuda", 0)


def emit(rec):
    rec = {"tag": args.tag, "lib": os.path.basename(_native.LIB_PATH), "index_rows": ROWS, **rec}
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


def summary(ms):
    return {"ms": round(statistics.median(ms), 3), "spread_ms": round(max(ms) - min(ms), 3), "rounds": [round(v, 3) for v in ms]} if ms else None


def same(a, b):
    return bool(all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b)))


def unchanged(idx, q_all, uniform):
    pred = [(UNIFORM, "range", None, 499_999)]
    for B in BATCHES:
        q = q_all[:B]
        calls = {"search": lambda: idx.search(q, K), "range_search": lambda: idx.range_search(q, MIN_COS, MAX_HITS),
                 "search_collapsed": lambda: idx.search_collapsed(q, K), "search_mmr": lambda: idx.search_mmr(q, K, lam=LAM),
                 "search_where_50pct": lambda: idx.search_where(q, K, pred)}
        for name, fn in calls.items():
            emit({"what": "unchanged", "call": name, "B": B, **summary([one_round(fn, args.reps) for _ in range(args.rounds)])})


def restricted(idx, kind, q, pred):
    if kind == "radial":
        return idx.range_search(q, MIN_COS, MAX_HITS, pred=pred)
    if kind == "collapsed":
        return idx.search_collapsed(q, K, pred=pred)
    return idx.search_mmr(q, K, lam=LAM, pred=pred)


def plain(idx, kind, q):
    if kind == "radial":
        return idx.range_search(q, MIN_COS, MAX_HITS)
    if kind == "collapsed":
        return idx.search_collapsed(q, K)
    return idx.search_mmr(q, K, lam=LAM)


def set_route(idx, kind, route):
    """gather: the whole index fits the scratch index; mask: forced"""
    if kind == "mmr":
        idx.set_option("where_route", route)
    else:
        idx.set_option("within_route", 2 if route == MASK else 0)
        idx.set_option("filter_gather_rows", max(ROWS, 256) if route == GATHER else 256)


def grid(idx, q_all, uniform):
    from semantic_query_engine_amd.engine import where_depth
    for kind in ("radial", "collapsed", "mmr"):
        for B in BATCHES:
            q = q_all[:B]
            t_plain = [one_round(lambda: plain(idx, kind, q), args.reps) for _ in range(args.rounds)]
            for f in FRACTIONS:
                thr = int(f * 1_000_000)
                pred = [(UNIFORM, "range", None, thr - 1)]
                selected = int(np.count_nonzero(uniform < thr))
                rule = where_depth(64 if kind == "collapsed" else 40, selected, ROWS) if kind != "radial" else -1
                mask_ok = kind == "radial" or rule > 0 or B == 1
                times, last, got = {GATHER: [], MASK: []}, {}, {}
                for _ in range(args.rounds):
                    for route in (GATHER, MASK):
                        if route == MASK and not mask_ok:
                            continue
                        set_route(idx, kind, route)
                        times[route].append(one_round(lambda: restricted(idx, kind, q, pred), args.reps))
                        got[route] = restricted(idx, kind, q, pred)
                        last[route] = idx.within_last()
                idx.set_option("where_route", 0)
                idx.set_option("within_route", 0)
                idx.set_option("filter_gather_rows", GATHER_ROWS_DEFAULT)
                t_where = [one_round(lambda: idx.search_where(q, K, pred), args.reps) for _ in range(args.rounds)]
                emit({"what": "grid", "kind": kind, "B": B, "fraction": f, "selected": selected, "rule_depth": rule,
                      "gather": summary(times[GATHER]), "mask": summary(times[MASK]), "plain": summary(t_plain),
                      "search_where": summary(t_where), "where_route": idx.where_last()["route"],
                      "gather_last": last.get(GATHER), "mask_last": last.get(MASK),
                      "bit_equal": same(got[GATHER], got[MASK]) if MASK in got else None})


def main():
    ctx = Context(0)
    t0 = time.perf_counter()
    idx = build(ctx)
    rng = np.random.default_rng(7)
    uniform = rng.integers(0, 1_000_000, ROWS)
    ids = np.arange(ROWS, dtype=np.int64)
    idx.set_field(UNIFORM, ids, uniform)
    idx.set_keys(ids, ids // 4)
    q_all = np.random.default_rng(8).standard_normal((1024, D)).astype(np.float32)
    emit({"what": "setup", "dim": D, "rounds": args.rounds, "reps": args.reps, "build_s": round(time.perf_counter() - t0, 1)})
    if args.unchanged:
        unchanged(idx, q_all, uniform)
    else:
        grid(idx, q_all, uniform)


if __name__ == "__main__":
    main()
