#!/usr/bin/env python3
"""Headline benchmark: brute-force cosine k-NN queries/sec over 10M x 1024-d vectors, top-10.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Both forms work: started WITHOUT a torch.distributed environment and with --gpus N > 1, this script starts
its own N rank processes (a child `python -m torch.distributed.run`, before anything touches the GPU),
relays rank 0's JSON line and exits with the children's code.

One "step" = one pass of the hot path over one batch of B synthetic queries that are
already resident in HBM: sqe_index_search_device (query normalise + first-pass scan + fp32
re-score + exactness certificate + collect pass for uncertified queries) and, for N > 1, the
all-gather of per-shard top-k over RCCL plus the merge kernel.  The first pass of the headline
leg is the index's default, the int8 collect scan (--scan-mode int8: threshold pass on a row
sample, v_mfma_i32_16x16x64_i8 scan of a per-tile-scaled int8 copy); a second leg of the same
W + K steps runs the bf16 first pass on the same index and queries and is reported beside it
(`bf16_scan`, with --full).  Both legs return the exact fp32 top-k (recall and max |dcos| against
an independent torch fp32 scan are in the line of a --full run).  The 10M-row index is sharded row-wise across
the N ranks (strong scaling: the job is "answer B queries over the 10M-row index";
`--rows-per-gpu R` is the weak form of BASELINE.json's config 4, R rows on every rank, e.g.
8 x 10M = 80M rows).

Rank 0 prints ONE JSON line (see the task contract); `roofline` is for the scan kernel of the
headline leg (hipEvent-timed inside libsqe on the stream it runs on; `traffic` from the
committed PMC passes of that kernel), `cpu_baseline` is the NumPy oracle (OpenBLAS sgemm +
argpartition) on a bounded sample, `cpu_baseline_hnsw` the CPU HNSW the reference's index is.

A plain run sets up, warms up, times the K steps of the headline leg and prints the line.  Everything
else -- recall against the independent exact scan, the bf16 second leg, the clustered third leg, the
hipBLASLt GEMM reference and the CPU baselines -- runs only with --full.  --dump-outputs DIR writes what
the headline leg returned in its last timed step (DIR/cos.npy float32 [B, k], DIR/ids.npy float64 [B, k]);
the inputs are seeded, so two builds given the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

D = 1024
BLOCK_ROWS = 1 << 20          # DB is generated in blocks of 1M rows, seed = base + block
PEAK_BF16_TFLOPS = 2500.0     # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_I8_TOPS = 5000.0         # dense int8 MFMA: twice the bf16 rate per clock (MI355X_MICROARCH.md, matrix cores table)
PEAK_HBM_GBPS = 8000.0


def db_block(block: int, rows: int, device, seed: int = 1000, centres: "torch.Tensor | None" = None) -> torch.Tensor:
    """Block `block` of the synthetic DB: isotropic Gaussian rows, or with `centres` SURVEY 8(d)'s clustered set
    (row = a random centre + 0.3 x Gaussian noise: what text embeddings look like)."""
    g = torch.Generator(device=device).manual_seed(seed + block)
    x = torch.randn((rows, D), generator=g, device=device, dtype=torch.float32)
    if centres is not None:
        lab = torch.randint(0, centres.shape[0], (rows,), generator=g, device=device)
        x = centres[lab] + 0.3 * x
    if os.environ.get("SQE_BENCH_DATA") == "zeros":     # clock experiments only (DVFS note)
        x.zero_()
    return x


def make_queries(b: int, device, seed: int = 12345) -> torch.Tensor:
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn((b, D), generator=g, device=device, dtype=torch.float32)


def library_gemm_tflops(b: int, device) -> float:
    """What the vendor GEMM (torch.matmul -> hipBLASLt) sustains on this box on the scan's own GEMM shape,
    queries [b x 1024] x DB block [1M x 1024]^T, bf16 random operands, bf16 output, no top-k work: the
    practical MFMA ceiling under this chip's power management, reported beside the nominal 2.5 PFLOP/s."""
    n = 1 << 20
    g = torch.Generator(device=device).manual_seed(7)
    qm = torch.randn((b, D), generator=g, device=device).bfloat16()
    dbm = torch.randn((n, D), generator=g, device=device).bfloat16()
    out = torch.empty((b, n), dtype=torch.bfloat16, device=device)
    for _ in range(5):
        torch.matmul(qm, dbm.t(), out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        torch.matmul(qm, dbm.t(), out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    del qm, dbm, out
    torch.cuda.empty_cache()
    return 2.0 * b * n * D / ms / 1e9


def scan_source_hash(mode: str = "bf16") -> str:
    """sha256 over the sources of the scan kernels of `mode`: a PMC traffic figure is only quoted for the kernel it was
    measured on (tools/pmc_scan.sh records the same hash next to the bytes)."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "semantic_query_engine_amd", "csrc")
    names = ("common.h", "kernels.h", "scan_common.h", "scan.hip", "scan_pp.hip")
    if mode == "int8":
        names = ("common.h", "kernels.h", "scan_common.h", "scan_i8.hip", "quant.hip")
    for name in names:
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def committed_traffic(rows: int, b: int, mode: str = "bf16"):
    """(HBM bytes per scan launch, source file) from the committed rocprofv3 PMC passes (tools/pmc_scan.sh ->
    profiles/r*/pmc_traffic*.json) taken on this workload AND on the scan kernel sources of this tree;
    (None, reason) otherwise.  The figure is read from a committed file, not measured in this run."""
    import glob
    want = scan_source_hash(mode)
    stale = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_traffic*.json")), reverse=True):
        try:
            t = json.load(open(path))
        except (OSError, ValueError):
            continue
        if t.get("rows") == rows and t.get("batch") == b and t.get("scan_mode", "bf16") == mode:
            rel = os.path.relpath(path, ROOT)
            if t.get("scan_src_sha") == want:
                return float(t["hbm_bytes_per_launch"]), rel
            stale = stale or f"{rel} was measured on other scan sources ({t.get('scan_src_sha')} != {want})"
    return None, stale or "no committed PMC pass for this workload"


def cpu_baseline_hnsw(rows: int, b: int, k: int) -> dict:
    """What the reference's index actually is: HNSW m = 64, ef_construction = 500, cosine (main.py:272-276),
    here the CPU restatement oracle/hnsw.cpp on the host cores, built over a bounded sample of the
    synthetic DB (an HNSW over 10M x 1024 takes hours to build) and searched with the k-NN plugin's
    default ef_search = 100.  Not scaled to N = 10M: HNSW search cost grows ~log N, recall falls with N."""
    from oracle import retrieval as R
    from oracle.hnsw import HnswIndex
    rng = np.random.default_rng(7)
    x = rng.standard_normal((rows, D), dtype=np.float32)
    q = rng.standard_normal((b, D), dtype=np.float32)
    q[: b // 2] = x[rng.integers(0, rows, b // 2)] + 0.1 * q[: b // 2]       # planted neighbours, as in the GPU run
    # the GPU box hands a one-GPU job a CPU share of 16 whatever the affinity mask says: more threads than that only thrash
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 16))
    t0 = time.perf_counter()
    h = HnswIndex(x, m=64, ef_construction=500, seed=0, threads=cores)
    build_s = time.perf_counter() - t0
    h.search(q[:64], k, ef_search=100, threads=cores)
    t0 = time.perf_counter()
    _, ids = h.search(q, k, ef_search=100, threads=cores)
    dt = time.perf_counter() - t0
    nq = min(128, b)
    _, exact = R.exact_topk(h.xn, R.normalize_rows(q[:nq]), k)
    recall = float(np.mean([len(set(a.tolist()) & set(e.tolist())) / k for a, e in zip(ids[:nq], exact)]))
    return {"value": round(b / dt, 1), "unit": "queries/s", "cores": int(cores), "kind": "port",
            "sample": f"HNSW m=64 ef_construction=500 ef_search=100 over {rows} x {D} rows (not scaled to the full index), "
                      f"{b} queries in {dt:.3f}s, build {build_s:.1f}s",
            "recall_at_10": round(recall, 4), "build_s": round(build_s, 2), "rows": int(rows),
            "larger_build": "200000 rows (too long a build for the default run): 2,820 queries/s, recall@10 0.708, build 266 s "
                            "(profiles/r03_search/hnsw_200k.json); the 10 M-row index would be slower and less exact still"}


def cpu_baseline(sample_rows: int, b: int, n_total: int, k: int) -> dict:
    """NumPy oracle timed on the host cores, on a bounded sample of the same workload:
    fp32 normalise + Q @ X.T (OpenBLAS) + argpartition top-k over `sample_rows` rows,
    scaled linearly in N to the full index."""
    from oracle import retrieval as R
    rng = np.random.default_rng(7)
    x = rng.standard_normal((sample_rows, D), dtype=np.float32)
    q = rng.standard_normal((b, D), dtype=np.float32)
    xn = R.normalize_rows(x)
    # the box gives one GPU's job a share of the host (16 CPUs): OpenBLAS sized to the machine's
    # 256 hardware threads oversubscribes that share and runs several times slower
    threads = max(1, min(int(os.environ.get("SQE_CPU_THREADS", "16")), len(os.sched_getaffinity(0))))
    try:
        from threadpoolctl import threadpool_limits
        limiter = threadpool_limits(limits=threads)
    except Exception:
        limiter = None
        threads = os.cpu_count() or 1
    t0 = time.perf_counter()
    qn = R.normalize_rows(q)
    blk = 65536
    best = None
    for lo in range(0, sample_rows, blk):
        s = qn @ xn[lo:lo + blk].T
        part = np.argpartition(-s, k, axis=1)[:, :k]
        vals = np.take_along_axis(s, part, 1)
        cur = (vals, part + lo)
        if best is None:
            best = cur
        else:
            v = np.concatenate([best[0], cur[0]], 1)
            i = np.concatenate([best[1], cur[1]], 1)
            o = np.argpartition(-v, k, axis=1)[:, :k]
            best = (np.take_along_axis(v, o, 1), np.take_along_axis(i, o, 1))
    dt = time.perf_counter() - t0
    if limiter is not None:
        limiter.restore_original_limits()
    qps = b / (dt * (n_total / sample_rows))
    return {"value": round(qps, 3), "unit": "queries/s", "cores": int(threads), "kind": "port",
            "sample": f"numpy oracle (fp32 sgemm + argpartition top-{k}), {sample_rows} rows x {b} queries "
                      f"in {dt:.2f}s, scaled linearly to {n_total} rows"}


def exact_reference(q: torch.Tensor, n_total: int, row_lo: int, row_hi: int, k: int, device, seed: int = 1000, centres=None):
    """Independent exact top-k (torch fp32 matmul over regenerated blocks) for the recall check."""
    qn = q / (q.norm(dim=1, keepdim=True) + 1e-9)
    best_s = torch.full((q.shape[0], 0), -float("inf"), device=device)
    best_i = torch.zeros((q.shape[0], 0), dtype=torch.long, device=device)
    nblocks = (n_total + BLOCK_ROWS - 1) // BLOCK_ROWS
    for blk in range(nblocks):
        lo = blk * BLOCK_ROWS
        hi = min(n_total, lo + BLOCK_ROWS)
        if hi <= row_lo or lo >= row_hi:
            continue
        x = db_block(blk, hi - lo, device, seed, centres)
        a, b_ = max(lo, row_lo) - lo, min(hi, row_hi) - lo
        x = x[a:b_]
        xn = x / (x.norm(dim=1, keepdim=True) + 1e-9)
        s = qn @ xn.T
        ids = torch.arange(lo + a, lo + b_, device=device).expand_as(s)
        s = torch.cat([best_s, s], 1)
        ids = torch.cat([best_i, ids], 1)
        top = torch.topk(s, min(k, s.shape[1]), dim=1)
        best_s, best_i = top.values, torch.gather(ids, 1, top.indices)
        del x, xn, s, ids
    return best_s, best_i


def dump_outputs(out_dir: str, cos: torch.Tensor, ids: torch.Tensor) -> None:
    """--dump-outputs: the [B, k] cosines (float32) and global row ids (float64, exact below 2^53) of one step."""
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "cos.npy"), cos.detach().cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "ids.npy"), ids.detach().cpu().numpy().astype(np.float64))


def self_launch(n: int, argv) -> "int":
    """`python bench.py --gpus N` with no rank environment: run the N ranks as a CHILD torch.distributed.run
    (never an exec of this process), stdout/stderr inherited so rank 0's JSON line is this process's line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd).returncode


def dry_run(args, world: int, rank: int) -> None:
    """--dry: the launch plumbing only, on CPU (gloo): rank environment, process group, barrier-bracketed
    timed region, MAX over ranks, ONE JSON line from rank 0.  No GPU, no search: `value` is null.  The N > 1
    data path itself is covered by tests/test_sharded_cpu.py."""
    import torch.distributed as dist
    if world > 1 or "MASTER_ADDR" in os.environ:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    else:
        dist = None
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001 * (rank + 1))                      # uneven ranks: the MAX must be the slowest one's
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        rows = args.rows_per_gpu * world if args.rows_per_gpu > 0 else args.rows
        print(json.dumps({"metric": "k-NN queries/sec (dry run: launch plumbing only)", "value": None, "unit": "queries/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 4), "higher_is_better": True,
                          "scaling": "weak" if args.rows_per_gpu > 0 else "strong", "vs_baseline": None, "dtype": "bf16",
                          "data": "none", "dry": True,
                          "config": {"workload": "dry run", "rows": rows, "batch": args.batch, "parallelism": f"shard{world}"}}),
              flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=10_000_000, help="total index rows (all ranks)")
    ap.add_argument("--rows-per-gpu", type=int, default=0,
                    help="config 4 of BASELINE.json (weak scaling): every rank holds this many rows, the index is "
                         "N x as large (e.g. 10000000 -> 80M rows on 8 GPUs); overrides --rows")
    ap.add_argument("--batch", type=int, default=1024, help="queries per step")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--scan-mode", choices=["bf16", "int8"], default="int8",
                    help="first-pass scan type of the headline leg (sqe.h: SQE_SCAN_*); both return the exact fp32 top-k behind a "
                         "certificate.  With int8 (the default) a second, bf16 leg of the same K steps is timed afterwards and "
                         "reported beside it (`bf16_scan`); --no-second-leg skips it")
    ap.add_argument("--no-second-leg", action="store_true")
    ap.add_argument("--i8-sample", default="", help="int8 mode: 'step,m' of the threshold pass (default: the library's 50,32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-rows", type=int, default=400_000)
    ap.add_argument("--no-clustered-leg", action="store_true",
                    help="skip the third leg: the same search over SURVEY 8(d)'s clustered set (4096 centres, sigma 0.3), one GPU only")
    ap.add_argument("--cpu-hnsw-rows", type=int, default=100_000,
                    help="rows of the CPU HNSW baseline (0 = skip; the build is superlinear on Gaussian rows: 50 k rows take 20 s on "
                         "the GPU box's 16 cores, 100 k about 75 s, 200 k -- profiles/r03_search/hnsw_200k.json -- 266 s)")
    ap.add_argument("--recall-queries", type=int, default=64)
    ap.add_argument("--no-gemm-ref", action="store_true", help="skip the hipBLASLt GEMM reference timing")
    ap.add_argument("--force-collective", action="store_true",
                    help="rehearsal on a one-GPU box: launched through torch.distributed.run with ONE rank, take the "
                         "all-gather + merge path of the N > 1 search anyway")
    ap.add_argument("--dry", action="store_true",
                    help="CPU rehearsal of the launch plumbing (gloo, no GPU, no search): see dry_run()")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline leg: recall against an independent exact scan, the bf16 second leg, the clustered "
                         "third leg, the GEMM reference and the CPU baselines (the --no-* options above apply within it)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the headline leg's results of its last timed step to DIR/cos.npy (float32) and DIR/ids.npy (float64)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # nothing has touched the GPU yet (importing torch does not): start the ranks as children
        raise SystemExit(self_launch(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.dry:
        return dry_run(args, world, rank)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or (args.force_collective and "MASTER_ADDR" in os.environ):
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group("nccl", device_id=device)

    from semantic_query_engine_amd import Context, VectorIndex
    from semantic_query_engine_amd.sharded import ShardedSearcher

    ctx = Context(local_rank)
    if args.rows_per_gpu > 0:
        args.rows = args.rows_per_gpu * world
    n_total, b, k = args.rows, args.batch, args.k
    rows_per = (n_total + world - 1) // world
    row_lo, row_hi = rank * rows_per, min(n_total, (rank + 1) * rows_per)

    # ---- build this rank's shard in HBM (seeded blocks, never through host memory)
    idx = VectorIndex(ctx, D)
    idx.reserve(row_hi - row_lo)
    nblocks = (n_total + BLOCK_ROWS - 1) // BLOCK_ROWS
    for blk in range(nblocks):
        lo = blk * BLOCK_ROWS
        hi = min(n_total, lo + BLOCK_ROWS)
        if hi <= row_lo or lo >= row_hi:
            continue
        x = db_block(blk, hi - lo, device)
        a, e = max(lo, row_lo) - lo, min(hi, row_hi) - lo
        xs = x[a:e].contiguous()
        torch.cuda.synchronize()
        idx.add_device(xs.data_ptr(), xs.shape[0])
        ctx.synchronize()
        del x, xs
    assert len(idx) == row_hi - row_lo
    torch.cuda.empty_cache()

    q = make_queries(b, device)
    # plant true neighbours for half the queries so recall is non-trivial
    plant_rows = torch.arange(0, b // 2, device=device) * (n_total // max(b // 2, 1))
    for blk in range(nblocks):
        lo, hi = blk * BLOCK_ROWS, min(n_total, (blk + 1) * BLOCK_ROWS)
        sel = (plant_rows >= lo) & (plant_rows < hi)
        if sel.any():
            x = db_block(blk, hi - lo, device)
            qi = torch.nonzero(sel).flatten()
            q[qi] = x[plant_rows[qi] - lo] + 0.1 * q[qi]
            del x
    torch.cuda.synchronize()

    searcher = ShardedSearcher(ctx, idx, id_base=row_lo, dist=dist, world=world, device=device,
                               force_collective=args.force_collective)
    from semantic_query_engine_amd import SCAN_BF16_RESCORE, SCAN_INT8_RESCORE

    def step():
        return searcher.search(q, k)

    if args.i8_sample:
        st_, m_ = (int(v) for v in args.i8_sample.split(","))
        idx.set_option("i8_sample_step", st_)
        idx.set_option("i8_sample_m", m_)

    def timed_leg(mode: str):
        """W untimed warm-up steps, then EXACTLY K steps bracketed by barrier + synchronize, max over ranks."""
        idx.set_option("scan_mode", SCAN_INT8_RESCORE if mode == "int8" else SCAN_BF16_RESCORE)
        for _ in range(args.warmup):
            step()
        searcher.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.stats_reset()
        ctx.set_profiling(True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            cos, ids = step()
        searcher.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        st = ctx.stats()
        ctx.set_profiling(False)
        if dist is not None:
            t = torch.tensor([elapsed], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed, st, cos, ids

    # ---- correctness of what was timed (--full): recall@k vs an independent exact scan
    if args.full:
        nq = min(args.recall_queries, b)
        probe = torch.cat([torch.arange(0, nq // 2), torch.arange(b - (nq - nq // 2), b)]).to(device)
        ref_s, ref_i = exact_reference(q[probe], n_total, row_lo, row_hi, k, device)
        if dist is not None:
            gs = [torch.empty_like(ref_s) for _ in range(world)]
            gi = [torch.empty_like(ref_i) for _ in range(world)]
            dist.all_gather(gs, ref_s)
            dist.all_gather(gi, ref_i)
            s_all, i_all = torch.cat(gs, 1), torch.cat(gi, 1)
            top = torch.topk(s_all, k, dim=1)
            ref_s, ref_i = top.values, torch.gather(i_all, 1, top.indices)

        def check(cos, ids):
            got_i, got_s = ids[probe], cos[probe]
            hits = sum(len(set(a.tolist()) & set(r.tolist())) for a, r in zip(got_i.cpu(), ref_i.cpu()))
            return {"recall_at_10": round(hits / (nq * k), 4), "max_abs_dcos": float((got_s - ref_s).abs().max().item()),
                    "planted_top1_ok": bool((ids[: b // 2, 0] == plant_rows).all().item())}

    def describe(mode: str, elapsed: float, st: dict) -> dict:
        """queries/s, stage times and the roofline object of the leg's dominant kernel (the scan)."""
        used_i8 = mode == "int8" and st.get("i8_collected", 0) > 0
        ms_per_step = elapsed / args.steps * 1e3
        scan_ms = st["scan_ms"] / max(st["scan_calls"], 1)
        flops, bytes_ = float(st["scan_flops"]), float(st["scan_bytes"])
        tflops = flops / (scan_ms * 1e-3) / 1e12 if scan_ms > 0 else 0.0
        gbps = bytes_ / (scan_ms * 1e-3) / 1e9 if scan_ms > 0 else 0.0
        # binding roof: the scan needs max(flops/peak_mfma, bytes/peak_hbm) at best
        peak_mfma = PEAK_I8_TOPS if used_i8 else PEAK_BF16_TFLOPS
        t_mfma, t_hbm = flops / (peak_mfma * 1e12), bytes_ / (PEAK_HBM_GBPS * 1e9)
        if t_mfma >= t_hbm:
            roof = {"bound": "mfma", "achieved": round(tflops, 2), "peak": peak_mfma, "unit": "TOP/s" if used_i8 else "TFLOP/s",
                    "frac": round(tflops / peak_mfma, 4), "traffic": None}
        else:
            roof = {"bound": "hbm", "achieved": round(gbps, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                    "frac": round(gbps / PEAK_HBM_GBPS, 4), "traffic": None}
        # (dim 1024: batches <= 128 run the streaming kernel, one 256-query block the five-stage build of the ping-pong kernel)
        kernel = ("scan_i8_pp_kernel" if b > 256 else "scan_i8_pp_deep_kernel" if b > 128 else "scan_i8_stream_kernel") if used_i8 else \
                 ("scan_bf16_pp_kernel" if b > 128 else "scan_bf16_kernel")
        roof.update({"kernel": kernel, "kernel_ms": round(scan_ms, 4), "launches": int(st["scan_calls"]),
                     "algorithmic_flops_per_launch": flops, "algorithmic_bytes_per_launch": bytes_,
                     "hbm_gbps": round(gbps, 1), "mfma_tflops": round(tflops, 2)})
        if world == 1:
            roof["traffic"], roof["traffic_source"] = committed_traffic(n_total, b, "int8" if used_i8 else "bf16")
        stage = {"prep": round(st["prep_ms"] / args.steps, 4), "scan": round(scan_ms, 4),
                 "select_rescore": round(st["select_ms"] / args.steps, 4)}
        extra = {}
        if used_i8:
            stage["threshold_pass"] = round(st["sample_ms"] / args.steps, 4)
            extra["int8_last_step"] = {"keys_collected": int(st["i8_collected"]), "rows_rescored": int(st["i8_rescored"]),
                                       "overflows": int(st["i8_overflows"])}
        return {"used_i8": used_i8, "value": round(b * args.steps / elapsed, 1), "ms_per_step": round(ms_per_step, 4),
                "dtype": "i8" if used_i8 else "bf16", "stage_ms": stage, "roofline": roof,
                "uncertified_queries_last_step": int(st.get("uncertified", 0)), **extra}

    elapsed, st, cos, ids = timed_leg(args.scan_mode)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, cos, ids)
    head_check = check(cos, ids) if args.full else {}
    second = None
    if args.full and args.scan_mode == "int8" and not args.no_second_leg:
        e2, st2, cos2, ids2 = timed_leg("bf16")
        second = (e2, st2, check(cos2, ids2), bool(torch.equal(ids2, ids)), float((cos2 - cos).abs().max().item()))

    # ---- third leg (one GPU): the SAME search over SURVEY 8(d)'s clustered set -- 4096 Gaussian centres, rows and queries = a centre
    # + 0.3 x noise, ~2,400 rows per centre, all of them within the int8 bound of the query's 10th neighbour.  r03 answered this set at a
    # third of the headline rate (every certificate failed: int8 pass + bf16 pass); the anchored threshold (select_i8.hip) certifies it.
    clustered = None
    if args.full and world == 1 and args.scan_mode == "int8" and not args.no_clustered_leg:
        idx.close()
        torch.cuda.empty_cache()
        gc = torch.Generator(device=device).manual_seed(77)
        centres = torch.randn((4096, D), generator=gc, device=device)
        idx = VectorIndex(ctx, D)
        idx.reserve(n_total)
        for blk in range(nblocks):
            lo, hi = blk * BLOCK_ROWS, min(n_total, (blk + 1) * BLOCK_ROWS)
            x = db_block(blk, hi - lo, device, 5000, centres)
            torch.cuda.synchronize()
            idx.add_device(x.data_ptr(), hi - lo)
            ctx.synchronize()
            del x
        q = centres[torch.randint(0, 4096, (b,), generator=gc, device=device)] + 0.3 * torch.randn((b, D), generator=gc, device=device)
        searcher = ShardedSearcher(ctx, idx, id_base=0, dist=None, world=1, device=device, force_collective=False)
        e3, st3, cos3, ids3 = timed_leg("int8")
        ref_s, ref_i = exact_reference(q[probe], n_total, 0, n_total, k, device, 5000, centres)
        got_i, got_s = ids3[probe], cos3[probe]
        hits = sum(len(set(a.tolist()) & set(r.tolist())) for a, r in zip(got_i.cpu(), ref_i.cpu()))
        clustered = (e3, st3, {"recall_at_10": round(hits / (nq * k), 4), "max_abs_dcos": float((got_s - ref_s).abs().max().item())})

    if rank == 0:
        head = describe(args.scan_mode, elapsed, st)
        roof = head["roofline"]
        if args.full and roof["bound"] == "mfma" and world == 1 and not args.no_gemm_ref and not head["used_i8"]:
            lib = library_gemm_tflops(b, device)
            roof["library_gemm_tflops"] = round(lib, 1)
            roof["frac_of_library_gemm"] = round(roof["mfma_tflops"] / lib, 4)
        first_pass = "int8 collect scan (per-row-scaled int8 copy, sample-derived thresholds)" if head["used_i8"] else "bf16 scan with fused top-k filter"
        out = {
            "metric": f"k-NN queries/sec (brute-force cosine top-{k}, 1024-d, "
                      f"{n_total // 1_000_000}M vectors)" if n_total % 1_000_000 == 0 else
                      f"k-NN queries/sec (brute-force cosine top-{k}, 1024-d, {n_total} vectors)",
            "value": head["value"], "unit": "queries/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True,
            "scaling": "weak" if args.rows_per_gpu > 0 else "strong", "vs_baseline": None, "dtype": head["dtype"], "data": "synthetic",
            "config": {"workload": f"flat cosine top-{k}, N={n_total} x {D} fp32 ({first_pass} + fp32 re-score of the candidates, "
                                   f"exactness certified per query, bf16 collect pass for uncertified queries), "
                                   f"batch={b} queries/step, index row-sharded over {world} GPU(s)",
                       "rows": n_total, "dim": D, "batch": b, "k": k, "parallelism": f"shard{world}", "scan_mode": args.scan_mode},
            **head_check,
            "uncertified_queries_last_step": head["uncertified_queries_last_step"],
            "stage_ms": head["stage_ms"],
            "roofline": roof,
        }
        if "int8_last_step" in head:
            out["int8_last_step"] = head["int8_last_step"]
        if second is not None:
            e2, st2, chk2, same_ids, dcos = second
            leg = describe("bf16", e2, st2)
            if leg["roofline"]["bound"] == "mfma" and world == 1 and not args.no_gemm_ref:
                lib = library_gemm_tflops(b, device)
                leg["roofline"]["library_gemm_tflops"] = round(lib, 1)
                leg["roofline"]["frac_of_library_gemm"] = round(leg["roofline"]["mfma_tflops"] / lib, 4)
            leg.pop("used_i8")
            out["bf16_scan"] = {"note": f"second leg, same index, queries, K = {args.steps} steps after W = {args.warmup} warm-ups: the bf16 "
                                        "first pass (scan_mode = SQE_SCAN_BF16_RESCORE); not part of `value`",
                                **leg, **chk2, "ids_equal_to_headline_leg": same_ids, "max_abs_dcos_vs_headline_leg": dcos}
        if clustered is not None:
            e3, st3, chk3 = clustered
            leg = describe("int8", e3, st3)
            leg.pop("used_i8")
            out["clustered"] = {"note": f"third leg, same size, batch and options over SURVEY 8(d)'s clustered set (4096 Gaussian centres, rows and queries = "
                                        f"centre + 0.3 x noise), K = {args.steps} steps after W = {args.warmup} warm-ups; not part of `value`",
                                **leg, **chk3}
        if args.force_collective:
            out["config"]["rehearsal"] = "one-rank nccl group, all-gather + merge path forced"
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(args.cpu_sample_rows, b, n_total, k)
            if args.cpu_hnsw_rows > 0:
                out["cpu_baseline_hnsw"] = cpu_baseline_hnsw(args.cpu_hnsw_rows, b, k)
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
