"""Cost of collapsed searches (sqe_index_search_collapsed) on the MI355X.

Rows are `centre[document] + g` (g Gaussian) with the group sizes of tests/golden/chunker.json repeated up to the row count
and shuffled; queries are `centre[random document] + g`.  Wall time is host to host around the _device entry points, the
median of 5 calls after a warm-up; scan / select are the profiler's stage times and scan_calls its number of scan launches
(sqe_stats), which for a swept query batch is the number of row ranges walked plus the main scan.

  corpus    the 32,717-row corpus-shaped index at D = 1024, B = 1, k = 3 (the reference's call)
  stage_a   ROWS x 1024 FLAT, B = 1 / 64 / 1024, k = 10: automatic depth (64, bf16 scan) and collapse_depth = 20 (int8 pass),
            each against the plain search of the same depth -- of THIS library and, with --parent-lib, of the parent
            commit's library on an index of its own holding the same rows, alternating in the same process
  crowd     the same index with a 3,000-row crowd of one document; 8 and 1024 of 1024 queries aimed at it (stage B), next
            to the bf16 top-10 search and a radial search with about 100 matches
  share     queries of 1,024 that stage A completes at the automatic depth, per k, on the D = 256 corpus-shaped data

usage (GPU box): python tools/collapse_bench.py [--rows N] [--out file.jsonl] [--parent-lib libsqe_parent.so] [--only a,b]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from semantic_query_engine_amd import SCAN_BF16_RESCORE, SCAN_INT8_RESCORE, Context, VectorIndex

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--out", default="")
ap.add_argument("--parent-lib", default="")
ap.add_argument("--only", default="corpus,stage_a,crowd,share")
ARGS = ap.parse_args()
dev = torch.device("cuda", 0)
CHUNK = 1 << 20
COUNTS = np.array(list(json.load(open(os.path.join(ROOT, "tests", "golden", "chunker.json")))["counts"].values()), np.int64)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as f:
            f.write(line + "\n")


class ParentIndex:
    """The few entry points of another build of the library (the parent commit's) that the comparison needs."""

    def __init__(self, path, dim):
        self.lib = C.CDLL(path)
        for name in ("sqe_create", "sqe_index_create", "sqe_index_reserve", "sqe_index_add_device", "sqe_index_search_device",
                     "sqe_synchronize", "sqe_index_set_option"):
            getattr(self.lib, name).restype = C.c_int
        self.lib.sqe_index_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        self.lib.sqe_index_reserve.argtypes = [C.c_void_p, C.c_int64]
        self.lib.sqe_index_add_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self.lib.sqe_index_search_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self.ctx, self.idx = C.c_void_p(), C.c_void_p()
        ids = (C.c_int32 * 1)(0)
        assert self.lib.sqe_create(ids, 1, C.byref(self.ctx)) == 0
        assert self.lib.sqe_index_create(self.ctx, dim, 0, 0, C.byref(self.idx)) == 0

    def reserve(self, rows):
        assert self.lib.sqe_index_reserve(self.idx, rows) == 0

    def add_device(self, ptr, n):
        assert self.lib.sqe_index_add_device(self.idx, ptr, n) == 0
        assert self.lib.sqe_synchronize(self.ctx) == 0

    def set_option(self, key, value):
        assert self.lib.sqe_index_set_option(self.idx, key.encode(), float(value)) == 0

    def search_device(self, q_ptr, b, k, cos_ptr, id_ptr):
        assert self.lib.sqe_index_search_device(self.idx, q_ptr, b, k, 0, cos_ptr, id_ptr) == 0
        assert self.lib.sqe_synchronize(self.ctx) == 0


def layout(rows, seed):
    """document of every row (shuffled) for the corpus' group sizes repeated up to `rows` rows"""
    reps = rows // int(COUNTS.sum()) + 1
    counts = np.tile(COUNTS, reps)
    counts = counts[:int(np.searchsorted(np.cumsum(counts), rows)) + 1]
    owner = np.repeat(np.arange(counts.shape[0]), counts)[:rows]
    np.random.default_rng(seed).shuffle(owner)
    return owner


def build(ctx, rows, dim, seed, parent=None, crowd=0):
    """-> (index, parent index or None, centres on the device, owner, crowd centre)"""
    owner = layout(rows, seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    centre = torch.randn((int(owner.max()) + 1, dim), generator=g, device=dev)
    c0 = torch.randn(dim, generator=g, device=dev)
    idx = VectorIndex(ctx, dim)
    idx.reserve(rows + crowd)
    if parent:
        parent.reserve(rows + crowd)
    own_d = torch.from_numpy(owner).to(dev)
    for r0 in range(0, rows, CHUNK):
        x = centre[own_d[r0:r0 + CHUNK]] + torch.randn((min(CHUNK, rows - r0), dim), generator=g, device=dev)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        if parent:
            parent.add_device(x.data_ptr(), x.shape[0])
        del x
    keys = owner.astype(np.int64) * 7919 - 123_456_789
    if crowd:
        x = c0 + 1e-3 * torch.randn((crowd, dim), generator=g, device=dev)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), crowd)
        ctx.synchronize()
        if parent:
            parent.add_device(x.data_ptr(), crowd)
        keys = np.concatenate([keys, np.full(crowd, 1 << 50, np.int64)])
    idx.set_keys(np.arange(keys.shape[0]), keys)
    return idx, centre, c0


def queries(centre, b, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    pick = torch.randint(0, centre.shape[0], (b,), generator=g, device=dev)
    return (centre[pick] + torch.randn((b, centre.shape[1]), generator=g, device=dev)).contiguous()


def timed(ctx, fn, reps=5, warm=1):
    out = []
    for i in range(warm + reps):
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        if i >= warm:
            out.append((time.perf_counter() - t) * 1e3)
    return out


def alternating(ctx, fns, reps=5):
    """{name: fn} called in turn, reps rounds after one warm-up round -> {name: [ms]}"""
    out = {name: [] for name in fns}
    for i in range(reps + 1):
        for name, fn in fns.items():
            ctx.synchronize()
            t = time.perf_counter()
            fn()
            ctx.synchronize()
            if i:
                out[name].append((time.perf_counter() - t) * 1e3)
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


def med(v):
    return round(statistics.median(v), 4)


def compare_depths(ctx, idx, parent, q, b, k, what, rows):
    """collapsed search against the plain search of its depth, automatic depth and collapse_depth = 20"""
    cos = torch.empty((b, 256), device=dev)
    ids = torch.empty((b, 256), dtype=torch.int64, device=dev)
    keys = torch.empty((b, 256), dtype=torch.int64, device=dev)
    qb = q[:b].contiguous()
    torch.cuda.synchronize()
    for depth_opt in (0, 20):
        depth = depth_opt or max(64, 4 * k)
        idx.set_option("collapse_depth", depth_opt)
        fns = {"collapsed": lambda: idx.search_collapsed_device(qb.data_ptr(), b, k, cos.data_ptr(), ids.data_ptr(), keys.data_ptr()),
               "search": lambda: idx.search_device(qb.data_ptr(), b, depth, cos.data_ptr(), ids.data_ptr()),
               "search_again": lambda: idx.search_device(qb.data_ptr(), b, depth, cos.data_ptr(), ids.data_ptr())}
        if parent:
            fns["parent_search"] = lambda: parent.search_device(qb.data_ptr(), b, depth, cos.data_ptr(), ids.data_ptr())
        t = alternating(ctx, fns)
        st = profiled(ctx, fns["collapsed"])
        emit({"what": what, "rows": rows, "batch": b, "k": k, "depth": depth, "collapsed_ms": med(t["collapsed"]),
              "search_ms": med(t["search"]), "search_again_ms": med(t["search_again"]),
              "parent_search_ms": med(t["parent_search"]) if parent else None,
              "spread_ms": round(abs(statistics.median(t["search"]) - statistics.median(t["search_again"])), 4),
              "all_collapsed_ms": [round(v, 4) for v in t["collapsed"]], "swept": st["collapse_swept"],
              "int8_pass": st["i8_collected"] > 0, "scan_ms": round(st["scan_ms"], 3), "select_ms": round(st["select_ms"], 3),
              "sample_ms": round(st["sample_ms"], 3), "scan_calls": st["scan_calls"]})
    idx.set_option("collapse_depth", 0)


def main():
    only = set(ARGS.only.split(","))
    ctx = Context(0)
    emit({"what": "device", **ctx.device_info(), "rows": ARGS.rows, "parent_lib": bool(ARGS.parent_lib)})
    if "corpus" in only:
        parent = ParentIndex(ARGS.parent_lib, 1024) if ARGS.parent_lib else None
        idx, centre, _ = build(ctx, 32_717, 1024, 11, parent)
        compare_depths(ctx, idx, parent, queries(centre, 1, 12), 1, 3, "corpus", 32_717)
        idx.close()
    if "share" in only:
        idx, centre, _ = build(ctx, 32_717, 256, 13)
        q = queries(centre, 1024, 14).cpu().numpy()
        for k in (1, 3, 10, 64, 256):
            idx.search_collapsed(q, k)
            swept = ctx.stats()["collapse_swept"]
            emit({"what": "share", "rows": 32_717, "dim": 256, "batch": 1024, "k": k, "depth": min(256, max(64, 4 * k)),
                  "swept": swept, "stage_a_share": round(1 - swept / 1024, 4)})
        idx.close()
    if only & {"stage_a", "crowd"}:
        rows = ARGS.rows
        parent = ParentIndex(ARGS.parent_lib, 1024) if ARGS.parent_lib and "stage_a" in only else None
        idx, centre, c0 = build(ctx, rows, 1024, 15, parent, crowd=3000 if "crowd" in only else 0)
        q = queries(centre, 1024, 16)
        if "stage_a" in only:
            for b in (1, 64, 1024):
                compare_depths(ctx, idx, parent, q, b, 10, "stage_a", rows)
        if "crowd" in only:
            b, k = 1024, 10
            cos = torch.empty((b, k), device=dev)
            ids = torch.empty((b, k), dtype=torch.int64, device=dev)
            keys = torch.empty((b, k), dtype=torch.int64, device=dev)
            cnt = torch.empty(b, dtype=torch.int64, device=dev)
            idx.set_option("scan_mode", SCAN_BF16_RESCORE)
            run = lambda: idx.search_device(q.data_ptr(), b, k, cos.data_ptr(), ids.data_ptr())
            st = profiled(ctx, run)
            emit({"what": "search_bf16_top10", "rows": rows, "batch": b, "wall_ms": med(timed(ctx, run)), "scan_ms": round(st["scan_ms"], 3),
                  "select_ms": round(st["select_ms"], 3)})
            # a radial search with about 100 matches: the floor halfway between the 100th and 101st cosine of a deep search
            idx.search_device(q.data_ptr(), b, k, cos.data_ptr(), ids.data_ptr())
            deep = torch.empty((b, 128), device=dev)
            deep_i = torch.empty((b, 128), dtype=torch.int64, device=dev)
            idx.search_device(q.data_ptr(), b, 128, deep.data_ptr(), deep_i.data_ptr())
            ctx.synchronize()
            floor = ((deep[:, 99] + deep[:, 100]) / 2).contiguous()
            torch.cuda.synchronize()
            run = lambda: idx.range_search_device(q.data_ptr(), b, floor.data_ptr(), k, cnt.data_ptr(), cos.data_ptr(), ids.data_ptr())
            st = profiled(ctx, run)
            emit({"what": "range_100_matches", "rows": rows, "batch": b, "wall_ms": med(timed(ctx, run)), "scan_ms": round(st["scan_ms"], 3),
                  "select_ms": round(st["select_ms"], 3)})
            idx.set_option("scan_mode", SCAN_INT8_RESCORE)
            for aimed in (8, 1024):
                g = torch.Generator(device=dev).manual_seed(17)
                qq = q.clone()
                qq[:aimed] = c0 + 0.5 * torch.randn((aimed, 1024), generator=g, device=dev) + 0.5 * q[:aimed]
                torch.cuda.synchronize()
                run = lambda: idx.search_collapsed_device(qq.data_ptr(), b, k, cos.data_ptr(), ids.data_ptr(), keys.data_ptr())
                st = profiled(ctx, run)
                t = timed(ctx, run, reps=3)
                emit({"what": "crowd", "rows": rows, "batch": b, "k": k, "aimed_at_crowd": aimed, "wall_ms": med(t), "swept": st["collapse_swept"],
                      "scan_ms": round(st["scan_ms"], 3), "select_ms": round(st["select_ms"], 3), "sample_ms": round(st["sample_ms"], 3),
                      "scan_calls": st["scan_calls"], "crowd_first": int((keys[:aimed, 0] == (1 << 50)).sum().item())})
        idx.close()


if __name__ == "__main__":
    main()
