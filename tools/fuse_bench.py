"""Cost of fused multi-query searches (sqe_index_search_fused) on the MI355X, against the route they replace: the plain search
over all sub-queries, B x n hits pulled to the host, a merge by id in NumPy.

Rows are `centre[document] + g` (g Gaussian) with the document sizes of tests/golden/chunker.json repeated up to the row
count and shuffled; the m sub-queries of a logical query are `centre[one random document] + g`, so their lists overlap.
Per point (G, m, mode, n, k), in ONE process, the three routes taking turns inside every repeat (wall clock around calls that
return synchronised; median and range of `--repeats` rounds after `--warmup` rounds):

  fused_ms        search_fused (host entry point): queries in, [G, k] results out
  fused_dev_ms    search_fused_device + a stream synchronisation: the same without the host copies
  search_ms       search_device(q_sub, n) + a stream synchronisation, same Bs and depth: what the index could do before the merge
  host_route_ms   search (host entry point: [Bs, n] hits read back) + the NumPy merge below: the whole route without the feature
  merge_ms        the NumPy merge alone
  fuse_stage_ms   select_ms of one fused call minus select_ms of one plain search at that depth (sqe_stats): the fuse kernel
  equal           the fused call's ids and scores equal the NumPy merge of the library's own search, bit for bit

usage (GPU box): python tools/fuse_bench.py [--rows N] [--dim 1024] [--out file.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=0, help="0: 10 M if the device has the memory, else 1 M")
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default="")
ARGS = ap.parse_args()
dev = torch.device("cuda", 0)
CHUNK = 1 << 19
COUNTS = np.array(list(json.load(open(os.path.join(ROOT, "tests", "golden", "chunker.json")))["counts"].values()), np.int64)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as f:
            f.write(line + "\n")


def build(ctx, rows, dim, seed=5):
    reps = rows // int(COUNTS.sum()) + 1
    owner = np.repeat(np.arange(COUNTS.shape[0] * reps), np.tile(COUNTS, reps))[:rows]
    np.random.default_rng(seed).shuffle(owner)
    g = torch.Generator(device=dev).manual_seed(seed)
    centre = torch.randn((int(owner.max()) + 1, dim), generator=g, device=dev)
    own_d = torch.from_numpy(owner).to(dev)
    idx = VectorIndex(ctx, dim)
    idx.reserve(rows)
    for r0 in range(0, rows, CHUNK):
        x = centre[own_d[r0:r0 + CHUNK]] + torch.randn((min(CHUNK, rows - r0), dim), generator=g, device=dev)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    return idx, centre


def host_merge(cos, ids, m, k, mode, c=60):
    """The merge by id of [G m, n] hits on the host, vectorised per logical query -> (fused, ids, cos) [G, k]."""
    G, n = cos.shape[0] // m, cos.shape[1]
    terms = np.rint(2.0 ** 40 / (c + 1.0 + np.arange(n))).astype(np.uint64)
    fo, io, co = np.full((G, k), -np.inf, np.float32), np.full((G, k), -1, np.int64), np.full((G, k), -np.inf, np.float32)
    for g in range(G):
        gi, gc = ids[g * m:(g + 1) * m].reshape(-1), cos[g * m:(g + 1) * m].reshape(-1)
        ok = gi >= 0
        uniq, inv = np.unique(gi[ok], return_inverse=True)
        best = np.full(uniq.shape[0], -np.inf, np.float32)
        np.maximum.at(best, inv, gc[ok])
        if mode == "rrf":
            score = np.zeros(uniq.shape[0], np.uint64)
            np.add.at(score, inv, np.tile(terms, m)[ok])
            key, val = -score.astype(np.float64), (score.astype(np.float64) * 2.0 ** -40).astype(np.float32)
        else:
            key, val = -(best.astype(np.float64) + 0.0), best
        order = np.lexsort((uniq, key))[:k]
        t = order.shape[0]
        fo[g, :t], io[g, :t], co[g, :t] = val[order], uniq[order], best[order]
    return fo, io, co


def main():
    rows = ARGS.rows
    if rows == 0:
        free_b, _ = torch.cuda.mem_get_info()
        rows = 10_000_000 if free_b > 10_000_000 * ARGS.dim * 8 else 1_000_000
    ctx = Context(0)
    idx, centre = build(ctx, rows, ARGS.dim)
    g = torch.Generator(device=dev).manual_seed(6)
    emit({"what": "setup", "rows": rows, "dim": ARGS.dim, "device": ctx.device_info(), "warmup": ARGS.warmup, "repeats": ARGS.repeats})
    k, m = 10, 4
    for G in (1, 64, 256):
        bs = G * m
        own = torch.randint(0, centre.shape[0], (G,), generator=g, device=dev).repeat_interleave(m)
        qd = (centre[own] + torch.randn((bs, ARGS.dim), generator=g, device=dev)).contiguous()
        q = qd.cpu().numpy()
        off = np.arange(G + 1, dtype=np.int64) * m
        for mode, n in (("rrf", 40), ("max", 10)):
            cd = torch.empty((bs, n), device=dev)
            idd = torch.empty((bs, n), dtype=torch.int64, device=dev)
            of = torch.empty((G, k), device=dev)
            oi = torch.empty((G, k), dtype=torch.int64, device=dev)
            oc = torch.empty((G, k), device=dev)
            torch.cuda.synchronize()
            ts = {"fused_ms": [], "fused_dev_ms": [], "search_ms": [], "host_route_ms": [], "merge_ms": []}

            def clock(name, fn):
                t0 = time.perf_counter()
                out = fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
                return out

            def fused_dev():
                idx.search_fused_device(qd.data_ptr(), bs, k, of.data_ptr(), oi.data_ptr(), oc.data_ptr(), offsets=off, mode=mode, depth=n)
                ctx.synchronize()

            def search_dev():
                idx.search_device(qd.data_ptr(), bs, n, cd.data_ptr(), idd.data_ptr())
                ctx.synchronize()

            for r in range(ARGS.warmup + ARGS.repeats):
                if r == ARGS.warmup:
                    for v in ts.values():
                        v.clear()
                got = clock("fused_ms", lambda: idx.search_fused(q, k, offsets=off, mode=mode, depth=n))
                clock("search_ms", search_dev)
                t0 = time.perf_counter()
                cos, ids = idx.search(q, n)
                t1 = time.perf_counter()
                want = host_merge(cos, ids, m, k, mode)
                t2 = time.perf_counter()
                ts["host_route_ms"].append((t2 - t0) * 1e3)
                ts["merge_ms"].append((t2 - t1) * 1e3)
                clock("fused_dev_ms", fused_dev)
            equal = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))
            ctx.set_profiling(True)
            ctx.stats_reset()
            fused_dev()
            sf = ctx.stats()
            ctx.stats_reset()
            search_dev()
            ss = ctx.stats()
            ctx.set_profiling(False)
            rec = {"what": "point", "rows": rows, "G": G, "m": m, "Bs": bs, "mode": mode, "n": n, "k": k, "equal": bool(equal)}
            for name, v in ts.items():
                rec[name] = [statistics.median(v), min(v), max(v)]
            rec.update({"fused_select_ms": sf["select_ms"], "fused_scan_ms": sf["scan_ms"], "search_select_ms": ss["select_ms"],
                        "search_scan_ms": ss["scan_ms"], "fuse_stage_ms": sf["select_ms"] - ss["select_ms"],
                        "fuse_stage_share_of_fused_dev": (sf["select_ms"] - ss["select_ms"]) / max(statistics.median(ts["fused_dev_ms"]), 1e-9),
                        "host_route_over_fused": statistics.median(ts["host_route_ms"]) / max(statistics.median(ts["fused_ms"]), 1e-9)})
            emit(rec)


if __name__ == "__main__":
    main()
