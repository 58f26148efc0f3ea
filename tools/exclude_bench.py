"""Cost of exclusion searches (sqe_index_search_excluding) on a 10 M x 1024 flat index, top-10, random per-query deny-lists.

  short    deny 5 ids per query at B = 1 / 64 / 1024: search_excluding_device ("excluding") next to the plain
           search_device at depth 15 ("plain": what stage A runs; the difference is the table build plus the drop kernel) and
           to the route such a request took before ("allow_list": search_device(filter_ptr=complement) -- ONE complement list
           shared by the whole batch, which flatters that route: per-query lists would cost it B calls).
  deep     deny 100 ids per query (deep class: depth 110, bf16 first pass) and deny 300 (k + len > 256: stage A at depth 256,
           then -- only for a query whose 256 hits were all denied -- the sweep) at B = 1 / 64, against "plain" at the same
           depth and "allow_list".  Random lists do not empty a query's top 256; "sweep" forces the sweep with
           exclude_depth = 10 and lists cut from each query's own top 10, which is what a sweep over 10 M rows costs.
Per case: wall time per call (median of 5 after one warm-up), the profiler's stage times (sqe_stats) and exclude_swept.
The answers of "excluding" and "allow_list" are compared where the lists are shared (B = 1).

usage (GPU box): python tools/exclude_bench.py [--rows N] [--out file.jsonl] [--modes short,deep,sweep]
-> one JSON line per measurement; for the kernel summary run `--modes short,sweep` under `rocprofv3 --kernel-trace --stats`"""
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
ap.add_argument("--modes", default="short,deep,sweep")
ap.add_argument("--tag", default="")
args = ap.parse_args()

from semantic_query_engine_amd import Context, VectorIndex, _native

D, K = 1024, 10
ROWS = args.rows
CHUNK = 1 << 20
dev = torch.device("cuda", 0)


def emit(rec):
    rec = {"lib": os.path.basename(_native.LIB_PATH), "tag": args.tag, "index_rows": ROWS, "k": K, **rec}
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
    return {key: round(st[key], 3) for key in ("prep_ms", "scan_ms", "select_ms", "sample_ms")}


class Case:
    """B queries, query b with its own deny-list of `n_deny` ids (random, or `lists` given)"""

    def __init__(self, rng, b, n_deny, lists=None):
        self.b, self.n_deny = b, n_deny
        ids = np.stack([rng.choice(ROWS, n_deny, replace=False) for _ in range(b)]) if lists is None else lists
        self.lists = ids.astype(np.int64)
        self.deny = torch.from_numpy(self.lists.reshape(-1)).to(dev)
        self.offsets = np.arange(b + 1, dtype=np.int64) * n_deny
        self.loq = np.arange(b, dtype=np.int32)
        # the route of before: the complement of list 0, shared by the batch
        keep = torch.ones(ROWS, dtype=torch.bool, device=dev)
        keep[self.deny[:n_deny]] = False
        self.allow = torch.nonzero(keep).reshape(-1).contiguous()
        g = torch.Generator(device=dev).manual_seed(99)
        self.q = torch.randn((b, D), generator=g, device=dev)
        self.cos = torch.empty((b, 256), device=dev)
        self.ids = torch.empty((b, 256), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

    def excluding(self, idx):
        idx.search_excluding_device(self.q.data_ptr(), self.b, K, self.deny.data_ptr(), self.offsets, self.loq, self.cos.data_ptr(),
                                    self.ids.data_ptr())

    def plain(self, idx, depth):
        idx.search_device(self.q.data_ptr(), self.b, depth, self.cos.data_ptr(), self.ids.data_ptr())

    def allow_list(self, idx):
        idx.search_device(self.q.data_ptr(), self.b, K, self.cos.data_ptr(), self.ids.data_ptr(), filter_ptr=self.allow.data_ptr(),
                          n_filter=int(self.allow.shape[0]))

    def result(self, ctx):
        ctx.synchronize()
        n = self.b * K
        return self.cos.reshape(-1)[:n].cpu().numpy().copy(), self.ids.reshape(-1)[:n].cpu().numpy().copy()


def measure(ctx, idx, case, what, depth):
    rec = {"what": what, "batch": case.b, "deny_per_query": case.n_deny}
    wall, runs = timed(ctx, lambda: case.excluding(idx))
    emit({**rec, "call": "excluding", "wall_ms": wall, "runs_ms": runs, **profiled(ctx, lambda: case.excluding(idx)),
          "exclude_swept": ctx.exclude_swept()})
    got = case.result(ctx)
    wall, runs = timed(ctx, lambda: case.plain(idx, depth))
    emit({**rec, "call": "plain", "depth": depth, "wall_ms": wall, "runs_ms": runs, **profiled(ctx, lambda: case.plain(idx, depth))})
    wall, runs = timed(ctx, lambda: case.allow_list(idx))
    emit({**rec, "call": "allow_list", "allowed_rows": int(case.allow.shape[0]), "wall_ms": wall, "runs_ms": runs,
          **profiled(ctx, lambda: case.allow_list(idx))})
    if case.b == 1:
        ref = case.result(ctx)
        emit({**rec, "what": "check_excluding_vs_allow_list", "same_ids": bool(np.array_equal(got[1], ref[1])),
              "same_cos": bool(np.array_equal(got[0], ref[0]))})


def main():
    ctx = Context(0)
    idx = build(ctx)
    rng = np.random.default_rng(5)
    modes = args.modes.split(",")
    if "short" in modes:
        for b in (1, 64, 1024):
            case = Case(rng, b, 5)
            measure(ctx, idx, case, "short", K + 5)
            del case
    if "deep" in modes:
        for n_deny, depth in ((100, K + 100), (300, 256)):
            for b in (1, 64):
                case = Case(rng, b, n_deny)
                measure(ctx, idx, case, "deep", depth)
                del case
    if "sweep" in modes:
        for b in (1, 64):
            probe = Case(rng, b, 5)
            probe.plain(idx, K)
            ctx.synchronize()
            own = probe.ids.reshape(-1)[:b * K].cpu().numpy().reshape(b, K)          # each query's own top 10
            del probe
            case = Case(rng, b, K, lists=own)
            idx.set_option("exclude_depth", K)
            measure(ctx, idx, case, "sweep", K)
            idx.set_option("exclude_depth", 0)
            del case
    idx.close()


if __name__ == "__main__":
    main()
