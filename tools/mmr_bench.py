"""Cost of MMR searches (sqe_index_search_mmr) on the MI355X, against the host formulation they replace.

Rows are `centre[document] + g` (g Gaussian) with the document sizes of tests/golden/chunker.json repeated up to the row
count and shuffled; queries are `centre[random document] + g`.  Per point (B, n, k), lambda = 0.5, all on one stream and
timed with events around the _device entry points, median and range of `--repeats` calls after `--warmup` calls:

  search_ms   the library's search_device at depth n alone
  mmr_ms      search_mmr_device(k, n)                      -> added_ms = mmr_ms - search_ms (Gram + select + index table)
  gram_ms     search_mmr_device(k = 1, n) - search_ms: the Gram stage plus ONE select step, an upper bound of the Gram
              kernel's time, so the fractions of the roofs derived from it are lower bounds
  torch_ms    the same added work in torch on the output of that search: a gather of the candidates' rows from an fp32
              normalised copy of the index, torch.bmm in fp32, and a k-step greedy loop batched over the queries
  ratio       torch_ms / added_ms (>= 1: the library's added stages are not slower)
  select_ms / scan_ms: the profiler's stage times of one MMR call (sqe_stats), for the split inside mmr_ms

Roofs of the Gram stage: 2 B n^2 dim FLOP against 155 TF (fp32 matrix rate) and B n dim 4 bytes against 8 TB/s (HBM).

usage (GPU box): python tools/mmr_bench.py [--rows N] [--dim 1024] [--out file.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=0, help="0: 10 M if the device has the memory, else 1 M")
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default="")
ARGS = ap.parse_args()
dev = torch.device("cuda", 0)
CHUNK = 1 << 19
COUNTS = np.array(list(json.load(open(os.path.join(ROOT, "tests", "golden", "chunker.json")))["counts"].values()), np.int64)
PEAK_TF, PEAK_HBM = 155e12, 8e12


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as f:
            f.write(line + "\n")


def build(ctx, rows, dim, seed=5):
    """-> (index, fp32 normalised copy of its rows on the device, document centres)"""
    reps = rows // int(COUNTS.sum()) + 1
    owner = np.repeat(np.arange(COUNTS.shape[0] * reps), np.tile(COUNTS, reps))[:rows]
    np.random.default_rng(seed).shuffle(owner)
    g = torch.Generator(device=dev).manual_seed(seed)
    centre = torch.randn((int(owner.max()) + 1, dim), generator=g, device=dev)
    own_d = torch.from_numpy(owner).to(dev)
    idx = VectorIndex(ctx, dim)
    idx.reserve(rows)
    xn = torch.empty((rows, dim), device=dev)
    for r0 in range(0, rows, CHUNK):
        x = centre[own_d[r0:r0 + CHUNK]] + torch.randn((min(CHUNK, rows - r0), dim), generator=g, device=dev)
        xn[r0:r0 + x.shape[0]] = x / (x.norm(dim=1, keepdim=True) + 1e-9)
        torch.cuda.synchronize()
        idx.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    return idx, xn, centre


def timed(fn, stream):
    """median, min, max (ms) of ARGS.repeats calls after ARGS.warmup calls, events on `stream`"""
    ts = []
    for i in range(ARGS.warmup + ARGS.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        if i >= ARGS.warmup:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def torch_added(xn, cos, ids, lam, k):
    """The host formulation of the added stages on the candidates (cos, ids) [B, n] of the library's search."""
    b, n = ids.shape
    rows = xn[ids.clamp_min(0)]                                   # [B, n, dim] gather of the master rows
    gram = torch.bmm(rows, rows.transpose(1, 2))
    pen = torch.zeros_like(cos)
    free = ids >= 0
    ar = torch.arange(b, device=cos.device)
    picks = torch.empty((b, k), dtype=torch.int64, device=cos.device)
    for t in range(k):
        obj = torch.where(free, lam * cos - (1.0 - lam) * pen, torch.full_like(cos, -float("inf")))
        i = obj.argmax(dim=1)
        picks[:, t] = i
        free[ar, i] = False
        s = gram[ar, :, i]
        pen = s if t == 0 else torch.maximum(pen, s)
    return ids.gather(1, picks)


def main():
    rows = ARGS.rows
    if rows == 0:
        free_b, _ = torch.cuda.mem_get_info()
        rows = 10_000_000 if free_b > 10_000_000 * ARGS.dim * 12 else 1_000_000      # master + copies + the torch copy
    ctx = Context(0)
    stream = torch.cuda.ExternalStream(ctx.stream)             # torch's work and the _device entry points share one stream
    idx, xn, centre = build(ctx, rows, ARGS.dim)
    g = torch.Generator(device=dev).manual_seed(6)
    emit({"what": "setup", "rows": rows, "dim": ARGS.dim, "device": ctx.device_info(), "warmup": ARGS.warmup, "repeats": ARGS.repeats})
    with torch.cuda.stream(stream):
        for b in (1, 64, 1024):
            q = centre[torch.randint(0, centre.shape[0], (b,), generator=g, device=dev)] + torch.randn((b, ARGS.dim), generator=g, device=dev)
            for n, k in ((32, 3), (64, 10), (256, 64)):
                cos = torch.empty((b, n), device=dev)
                ids = torch.empty((b, n), dtype=torch.int64, device=dev)
                oc = torch.empty((b, k), device=dev)
                oi = torch.empty((b, k), dtype=torch.int64, device=dev)
                om = torch.empty((b, k), device=dev)
                torch.cuda.synchronize()
                search = lambda: idx.search_device(q.data_ptr(), b, n, cos.data_ptr(), ids.data_ptr())
                mmr = lambda: idx.search_mmr_device(q.data_ptr(), b, k, oc.data_ptr(), oi.data_ptr(), om.data_ptr(), lam=0.5, n_cand=n)
                mmr1 = lambda: idx.search_mmr_device(q.data_ptr(), b, 1, oc.data_ptr(), oi.data_ptr(), om.data_ptr(), lam=0.5, n_cand=n)
                t_s = timed(search, stream)
                t_m = timed(mmr, stream)
                t_1 = timed(mmr1, stream)
                mmr()
                torch.cuda.synchronize()
                want = oi.clone()
                search()
                t_t = timed(lambda: torch_added(xn, cos, ids, 0.5, k), stream)
                same = float((torch_added(xn, cos, ids, 0.5, k) == want).all(dim=1).float().mean())
                ctx.set_profiling(True)
                ctx.stats_reset()
                mmr()
                st = ctx.stats()
                ctx.set_profiling(False)
                added = t_m[0] - t_s[0]
                gram = max(t_1[0] - t_s[0], 1e-6)
                flop, byts = 2.0 * b * n * n * ARGS.dim, 4.0 * b * n * ARGS.dim
                emit({"what": "point", "rows": rows, "B": b, "n": n, "k": k,
                      "search_ms": t_s, "mmr_ms": t_m, "mmr_k1_ms": t_1, "torch_added_ms": t_t,
                      "added_ms": added, "gram_ms_upper": gram, "ratio_torch_over_added": t_t[0] / max(added, 1e-6),
                      "gram_frac_of_fp32_roof_lower": flop / (gram * 1e-3) / PEAK_TF,
                      "gram_frac_of_hbm_roof_lower": byts / (gram * 1e-3) / PEAK_HBM,
                      "binding_roof": "fp32 matrix" if flop / PEAK_TF > byts / PEAK_HBM else "HBM",
                      "select_ms": st["select_ms"], "scan_ms": st["scan_ms"], "queries_equal_to_torch": same})


if __name__ == "__main__":
    main()
