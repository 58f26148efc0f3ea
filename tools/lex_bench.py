"""Cost of the lexical index (sqe_lex_*) and of the hybrid search (sqe_index_search_hybrid) on the MI355X.

Corpus: `--docs` documents (default 1 M) of about `--length` term occurrences (default 200; uniform in [length / 2, 3 length /
2]) over `--terms` terms (default 30522), term t drawn with probability ~ 1 / (t + 1).  Queries: `--qterms` terms each, drawn the
same way (so they hold the common terms whose runs are long).  One process; wall clock around calls that return synchronised;
median, min and max of `--repeats` rounds after `--warmup` rounds.  One JSON line per record:

  corpus    generation and put (host only: the bags are canonicalised and logged, nothing touches the device)
  rebuild   the first search after the puts: last_rebuild_ms (host compaction, upload, four kernels, one synchronisation) and
            the device bytes the index holds (hipMemGetInfo before the index exists and after the rebuild)
  search    per (B, query terms): search (host entry point), search_device + synchronise, scan_ms / select_ms of one call
            (sqe_stats), and host_ms_per_query: the NumPy/CSR evaluation of the same integer definition on this box's host
            (impacts from tests/lex_reference.py's formulas over a CSR by term, np.add.at per query term, lexsort), timed on the
            first `--host-queries` queries of the batch and checked bit for bit against the device's rows
  hybrid    per G: search_hybrid_device (one vector sub-query + the lexical list per group) + synchronise against
            search_fused_device of the same sub-queries alone on the same vector index (`--vec-rows` x `--dim`, random rows)

The chunk size is a compile-time constant: run once per library (SQE_LIB=.../libsqe_lex32768.so from `make LEX_CHUNK=32768`);
`--corpus-cache file.npy` lets the second run load the first run's draws.

usage (GPU box): python tools/lex_bench.py [--out file.jsonl] [--host-ref]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from semantic_query_engine_amd import Context, LexicalIndex, VectorIndex

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--length", type=int, default=200)
ap.add_argument("--terms", type=int, default=30522)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--host-ref", action="store_true", help="also time the NumPy/CSR evaluation on the host")
ap.add_argument("--host-queries", type=int, default=4)
ap.add_argument("--vec-rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--no-hybrid", action="store_true")
ap.add_argument("--corpus-cache", default="")
ap.add_argument("--out", default="")
ARGS = ap.parse_args()
dev = torch.device("cuda", 0)


def emit(rec):
    rec["lib"] = os.path.basename(os.environ.get("SQE_LIB", "libsqe.so"))
    line = json.dumps(rec)
    print(line, flush=True)
    if ARGS.out:
        with open(ARGS.out, "a") as f:
            f.write(line + "\n")


def draw(rng, cdf, n):
    return np.minimum(np.searchsorted(cdf, rng.random(n)), cdf.shape[0] - 1).astype(np.int32)


def med(v):
    return [statistics.median(v), min(v), max(v)]


def host_csr(lex_ids, offsets, terms, n_terms, k1=1.2, b=0.75):
    """The reference's impacts over a CSR by term, from the definition (include/sqe.h), vectorised."""
    n = offsets.shape[0] - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    key = row * n_terms + terms
    uniq, cnt = np.unique(key, return_counts=True)
    prow, pterm = uniq // n_terms, uniq % n_terms
    tf = np.minimum(cnt, 65535).astype(np.float64)
    dl = np.diff(offsets).astype(np.float64)
    avgdl = np.float64(offsets[-1]) / np.float64(n)
    df = np.bincount(pterm, minlength=n_terms)
    idf = np.zeros(n_terms, np.float64)
    for f in np.unique(df[df > 0]):
        idf[df == f] = math.log(1.0 + ((n - int(f)) + 0.5) / (int(f) + 0.5))
    norm = k1 * ((1.0 - b) + b * (dl / avgdl))
    imp = np.maximum(1.0, np.rint(idf[pterm] * (tf / (tf + norm[prow])) * 65536.0)).astype(np.uint64)
    order = np.argsort(pterm, kind="stable")
    start = np.concatenate([[0], np.cumsum(df)])
    return prow[order], imp[order], start


def host_search(csr, lex_ids, query, k):
    prow, imp, start = csr
    score = np.zeros(lex_ids.shape[0], np.uint64)
    for t in query:
        a, b = start[t], start[t + 1]
        np.add.at(score, prow[a:b], imp[a:b])
    hit = np.nonzero(score)[0]
    order = hit[np.lexsort((lex_ids[hit], -score[hit].astype(np.int64)))][:k]
    return (score[order].astype(np.float64) * 2.0 ** -16).astype(np.float32), lex_ids[order]


def main():
    rng = np.random.default_rng(1)
    p = 1.0 / np.arange(1, ARGS.terms + 1)
    cdf = np.cumsum(p / p.sum())
    t0 = time.perf_counter()
    lens = rng.integers(ARGS.length // 2, 3 * ARGS.length // 2 + 1, ARGS.docs)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if ARGS.corpus_cache and os.path.exists(ARGS.corpus_cache):
        terms = np.load(ARGS.corpus_cache)
    else:
        terms = draw(rng, cdf, int(offsets[-1]))
        if ARGS.corpus_cache:
            np.save(ARGS.corpus_cache, terms)
    t_gen = time.perf_counter() - t0
    ids = np.arange(ARGS.docs, dtype=np.int64)
    ctx = Context(0)
    free0, _ = torch.cuda.mem_get_info()
    lex = LexicalIndex(ctx, ARGS.terms)
    t0 = time.perf_counter()
    step = 100_000
    for lo in range(0, ARGS.docs, step):
        hi = min(ARGS.docs, lo + step)
        lex.put(ids[lo:hi], (offsets[lo:hi + 1] - offsets[lo], terms[offsets[lo]:offsets[hi]]))
    t_put = time.perf_counter() - t0
    emit({"what": "corpus", "docs": ARGS.docs, "occurrences": int(offsets[-1]), "terms": ARGS.terms, "generate_s": t_gen, "put_s": t_put,
          "device": ctx.device_info()})
    t0 = time.perf_counter()
    lex.search([[0]], 1)
    t_first = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    info = lex.info()
    emit({"what": "rebuild", "first_search_ms": t_first, "device_bytes": int(free0 - free1), **info})

    csr = None
    if ARGS.host_ref:
        t0 = time.perf_counter()
        csr = host_csr(ids, offsets, terms, ARGS.terms)
        emit({"what": "host_csr", "build_s": time.perf_counter() - t0, "postings": int(csr[0].shape[0])})

    qrng = np.random.default_rng(2)
    k = ARGS.k
    for nq in (4, 16):
        for B in (1, 64, 256):
            queries = [draw(qrng, cdf, nq) for _ in range(B)]
            sd = torch.empty((B, k), device=dev)
            idd = torch.empty((B, k), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            ts = {"search_ms": [], "search_dev_ms": []}

            def dev_call():
                lex.search_device(queries, k, sd.data_ptr(), idd.data_ptr())
                ctx.synchronize()

            for r in range(ARGS.warmup + ARGS.repeats):
                if r == ARGS.warmup:
                    for v in ts.values():
                        v.clear()
                t0 = time.perf_counter()
                got = lex.search(queries, k)
                ts["search_ms"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                dev_call()
                ts["search_dev_ms"].append((time.perf_counter() - t0) * 1e3)
            ctx.set_profiling(True)
            ctx.stats_reset()
            dev_call()
            st = ctx.stats()
            ctx.set_profiling(False)
            rec = {"what": "search", "B": B, "qterms": nq, "k": k, "chunk_rows": info["chunk_rows"], "scan_ms": st["scan_ms"],
                   "select_ms": st["select_ms"]}
            for name, v in ts.items():
                rec[name] = med(v)
            if csr is not None:
                hq = min(B, ARGS.host_queries)
                t0 = time.perf_counter()
                want = [host_search(csr, ids, queries[i], k) for i in range(hq)]
                rec["host_ms_per_query"] = (time.perf_counter() - t0) * 1e3 / hq
                rec["equal"] = all(np.array_equal(got[0][i][:w[0].shape[0]].view(np.uint8), w[0].view(np.uint8)) and
                                   np.array_equal(got[1][i][:w[1].shape[0]], w[1]) for i, w in enumerate(want))
            emit(rec)

    if ARGS.no_hybrid:
        return
    g = torch.Generator(device=dev).manual_seed(3)
    vec = VectorIndex(ctx, ARGS.dim)
    vec.reserve(ARGS.vec_rows)
    for r0 in range(0, ARGS.vec_rows, 1 << 18):
        x = torch.randn((min(1 << 18, ARGS.vec_rows - r0), ARGS.dim), generator=g, device=dev)
        torch.cuda.synchronize()
        vec.add_device(x.data_ptr(), x.shape[0])
        ctx.synchronize()
        del x
    for G in (1, 64, 256):
        qd = torch.randn((G, ARGS.dim), generator=g, device=dev).contiguous()
        queries = [draw(qrng, cdf, 4) for _ in range(G)]
        off = np.arange(G + 1, dtype=np.int64)
        outs = [torch.empty((G, k), device=dev) for _ in range(3)]
        oi = torch.empty((G, k), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ts = {"hybrid_dev_ms": [], "fused_dev_ms": []}

        def hybrid():
            vec.search_hybrid_device(lex, qd.data_ptr(), G, queries, k, outs[0].data_ptr(), oi.data_ptr(), outs[1].data_ptr(),
                                     outs[2].data_ptr(), offsets=off)
            ctx.synchronize()

        def fused():
            vec.search_fused_device(qd.data_ptr(), G, k, outs[0].data_ptr(), oi.data_ptr(), outs[1].data_ptr(), offsets=off, mode="rrf")
            ctx.synchronize()

        for r in range(ARGS.warmup + ARGS.repeats):
            if r == ARGS.warmup:
                for v in ts.values():
                    v.clear()
            for name, fn in (("hybrid_dev_ms", hybrid), ("fused_dev_ms", fused)):
                t0 = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        rec = {"what": "hybrid", "G": G, "k": k, "vec_rows": ARGS.vec_rows, "dim": ARGS.dim, "chunk_rows": info["chunk_rows"]}
        for name, v in ts.items():
            rec[name] = med(v)
        emit(rec)


if __name__ == "__main__":
    main()
