"""The entry points that take a row set (a field predicate and an allow-list), one after the other on one index: search_where and
its _device form, aggregate_fields, sort_fields, and the host and _device forms of range_search_where, search_collapsed_where and
search_mmr_where.

Without --time: ONE call of each on a 701-row index with three rows deleted, over a row set that has both a predicate and a list,
so that a kernel trace of the process lists every launch of the row-set layer; the answers' checksums are printed.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/rowset_calls.py --root <tree>` on two trees to compare kernel names and counts.

With --time: the wall time per call at B = 1 and B = 1024 on a --rows x --dim index for two row sets (a predicate that selects 1 %
of the rows; a predicate that selects 50 % behind a host list of 30 % of the ids), the median of --reps calls after one warm-up,
one JSON line per point.  Run it alternately with --root on two trees to compare them.

usage (GPU box): python tools/rowset_calls.py [--root DIR] [--time] [--rows N] [--dim D] [--reps N] [--out file.jsonl] [--tag T]"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--time", action="store_true")
ap.add_argument("--rows", type=int, default=2_000_000)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default="")
ap.add_argument("--tag", default="")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex

VALUE = 0                       # field slot: a uniform value in 0 .. 999
K, MAX_HITS, LAM = 10, 10, 0.5
dev = torch.device("cuda", 0)


def build(ctx, rows, dim, dels):
    idx = VectorIndex(ctx, dim)
    chunk = 1 << 20
    for c in range((rows + chunk - 1) // chunk):
        g = torch.Generator(device=dev).manual_seed(1000 + c)
        x = torch.randn((min(chunk, rows - c * chunk), dim), generator=g, device=dev)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    ids = np.arange(rows, dtype=np.int64)
    value = np.random.default_rng(7).integers(0, 1000, rows)
    idx.set_field(VALUE, ids, value)
    idx.set_keys(ids, ids // 4)
    if len(dels):
        idx.delete(np.asarray(dels, np.int64))
    return idx, value


def calls(idx, q, pred, allow, min_cos):
    """name -> a function that makes the call and returns its outputs as numpy arrays"""
    b = q.shape[0]
    qd = torch.from_numpy(q).to(dev)
    td = torch.full((b,), min_cos, dtype=torch.float32, device=dev)
    lam = np.full(b, LAM, np.float32)
    cd = torch.empty((b, K), dtype=torch.float32, device=dev)
    jd = torch.empty((b, K), dtype=torch.int64, device=dev)
    kd = torch.empty((b, K), dtype=torch.int64, device=dev)
    od = torch.empty((b, K), dtype=torch.float32, device=dev)
    nd = torch.empty(b, dtype=torch.int64, device=dev)
    rows, keep = idx._row_set(pred, None)
    ad = None
    if allow is not None:
        ad = torch.from_numpy(np.ascontiguousarray(allow, np.int64)).to(dev)
        rows = rows[:4] + (ad.data_ptr(), ad.shape[0])
    torch.cuda.synchronize()
    lib, h = idx.lib, idx.handle

    def device(fn, outs):
        def run():
            assert fn() == 0
            idx.ctx.synchronize()
            return [o.cpu().numpy() for o in outs]
        run.keep = (keep, ad)
        return run

    def aggregate():
        r = idx.aggregate_fields(pred, [(VALUE, "stats"), (VALUE, "terms", 5)], filter_ids=allow)
        return [np.array([r["selected"], r["aggs"][0]["sum"]]), r["aggs"][1]["keys"], r["aggs"][1]["counts"]]

    def sort():
        r = idx.sort_fields(pred, [(VALUE, "desc")], 16, filter_ids=allow)
        return [np.array([r["total"]]), r["ids"], r["values"]]

    return {
        "search_where": lambda: idx.search_where(q, K, pred, filter_ids=allow),
        "search_where_device": device(lambda: lib.sqe_index_search_where_device(h, qd.data_ptr(), b, K, *rows, cd.data_ptr(), jd.data_ptr()), (cd, jd)),
        "aggregate_fields": aggregate,
        "sort_fields": sort,
        "range_search_where": lambda: idx.range_search(q, min_cos, MAX_HITS, pred=pred, filter_ids=allow),
        "range_search_where_device": device(lambda: lib.sqe_index_range_search_where_device(h, qd.data_ptr(), b, td.data_ptr(), K, *rows, nd.data_ptr(),
                                                                                            cd.data_ptr(), jd.data_ptr()), (nd, cd, jd)),
        "search_collapsed_where": lambda: idx.search_collapsed(q, K, pred=pred, filter_ids=allow),
        "search_collapsed_where_device": device(lambda: lib.sqe_index_search_collapsed_where_device(h, qd.data_ptr(), b, K, *rows, cd.data_ptr(),
                                                                                                    jd.data_ptr(), kd.data_ptr()), (cd, jd, kd)),
        "search_mmr_where": lambda: idx.search_mmr(q, K, lam=LAM, pred=pred, filter_ids=allow),
        "search_mmr_where_device": device(lambda: lib.sqe_index_search_mmr_where_device(h, qd.data_ptr(), b, K, 0, lam.ctypes.data, 0, *rows,
                                                                                        cd.data_ptr(), jd.data_ptr(), od.data_ptr()), (cd, jd, od)),
    }


def checksum(outs):
    crc = 0
    for a in outs:
        crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    return crc


def emit(rec):
    line = json.dumps({"tag": args.tag, **rec})
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def once(ctx):
    idx, value = build(ctx, 701, 64, [3, 100, 650])
    rng = np.random.default_rng(8)
    q = rng.standard_normal((4, 64)).astype(np.float32)
    allow = rng.permutation(np.concatenate([np.arange(0, 701, 2), [3, 3, 900]]))
    for name, fn in calls(idx, q, [(VALUE, "range", 200, None)], allow, 0.05).items():
        emit({"what": "once", "call": name, "crc32": checksum(fn())})


def timed(ctx):
    t0 = time.perf_counter()
    idx, value = build(ctx, args.rows, args.dim, [])
    rng = np.random.default_rng(8)
    q_all = rng.standard_normal((1024, args.dim)).astype(np.float32)
    sets = {"pred_1pct": ([(VALUE, "range", None, 9)], None),
            "pred_50pct_list_30pct": ([(VALUE, "range", None, 499)], rng.permutation(args.rows)[: args.rows * 3 // 10].astype(np.int64))}
    emit({"what": "setup", "rows": args.rows, "dim": args.dim, "reps": args.reps, "build_s": round(time.perf_counter() - t0, 1)})
    for sname, (pred, allow) in sets.items():
        for B in (1, 1024):
            for name, fn in calls(idx, q_all[:B], pred, allow, 0.2).items():
                crc = checksum(fn())              # warm-up
                ms = []
                for _ in range(args.reps):
                    t = time.perf_counter()
                    fn()
                    ms.append((time.perf_counter() - t) * 1e3)
                emit({"what": "time", "set": sname, "B": B, "call": name, "ms": round(statistics.median(ms), 4),
                      "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "crc32": crc})


if __name__ == "__main__":
    ctx = Context(0)
    timed(ctx) if args.time else once(ctx)
