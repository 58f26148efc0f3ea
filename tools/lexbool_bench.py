"""Cost of the boolean lexical queries (sqe_lex_search_bool), of the match sets (sqe_lex_match) and of a k-NN search filtered
by a match set on the MI355X, beside sqe_lex_search on the same queries in the same run.

Corpus and queries are those of tools/lex_bench.py (same generators, same seeds): `--docs` documents (default 1 M) of about
`--length` term occurrences over `--terms` terms, term t with probability ~ 1 / (t + 1); queries of 4 and of 16 terms drawn the
same way.  One process; wall clock around calls that return synchronised; median, min and max of `--repeats` rounds after
`--warmup` rounds, the variants of one point alternated inside every round.  One JSON line per record:

  bool      per (B, query terms): search_device (plain), and search_bool_device with every role SHOULD, with every role MUST
            (operator and) and with every role SHOULD and min_should = 2, each + synchronise; scan_ms / select_ms of one call of
            each (sqe_stats); the mean number of matches of the AND and the min_should = 2 queries
  match     per (B, which): match_device + synchronise with cap = the largest count of the batch, for one FILTER term per query,
            rare (df of a few hundred) or common (in most documents); counts, scan_ms / select_ms
  filtered  one k-NN search (`--vec-rows` x `--dim`, random rows) filtered by the match set of an AND query: the match (host form:
            counts and ids back on the host), the search with filter_ids = those ids (the hand-over of the list is inside it) and
            the stages sqe_stats books for that search

usage (GPU box): python tools/lexbool_bench.py [--out file.jsonl]"""
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

from semantic_query_engine_amd import Context, LexicalIndex, VectorIndex
from semantic_query_engine_amd.engine import LEX_FILTER, LEX_MUST, LEX_SHOULD

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--length", type=int, default=200)
ap.add_argument("--terms", type=int, default=30522)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--vec-rows", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=1024)
ap.add_argument("--no-filtered", action="store_true")
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


def rounds(ctx, calls):
    """calls: name -> function that returns synchronised.  -> name -> [median, min, max] ms, and the stages of one more call."""
    ts = {name: [] for name in calls}
    for r in range(ARGS.warmup + ARGS.repeats):
        if r == ARGS.warmup:
            for v in ts.values():
                v.clear()
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    out = {}
    ctx.set_profiling(True)
    for name, fn in calls.items():
        ctx.stats_reset()
        fn()
        st = ctx.stats()
        out[name] = {"ms": med(ts[name]), "scan_ms": st["scan_ms"], "select_ms": st["select_ms"], "prep_ms": st["prep_ms"]}
    ctx.set_profiling(False)
    return out


def main():
    rng = np.random.default_rng(1)
    p = 1.0 / np.arange(1, ARGS.terms + 1)
    cdf = np.cumsum(p / p.sum())
    lens = rng.integers(ARGS.length // 2, 3 * ARGS.length // 2 + 1, ARGS.docs)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if ARGS.corpus_cache and os.path.exists(ARGS.corpus_cache):
        terms = np.load(ARGS.corpus_cache)
    else:
        terms = draw(rng, cdf, int(offsets[-1]))
        if ARGS.corpus_cache:
            np.save(ARGS.corpus_cache, terms)
    ids = np.arange(ARGS.docs, dtype=np.int64)
    ctx = Context(0)
    lex = LexicalIndex(ctx, ARGS.terms)
    step = 100_000
    for lo in range(0, ARGS.docs, step):
        hi = min(ARGS.docs, lo + step)
        lex.put(ids[lo:hi], (offsets[lo:hi + 1] - offsets[lo], terms[offsets[lo]:offsets[hi]]))
    lex.search([[0]], 1)
    info = lex.info()
    emit({"what": "corpus", "docs": ARGS.docs, "occurrences": int(offsets[-1]), "terms": ARGS.terms, "device": ctx.device_info(), **info})

    def sync(fn, *a):
        def call():
            fn(*a)
            ctx.synchronize()
        return call

    qrng = np.random.default_rng(2)
    k = ARGS.k
    for nq in (4, 16):
        for B in (1, 64, 256):
            queries = [draw(qrng, cdf, nq) for _ in range(B)]
            should, must = [[LEX_SHOULD] * nq] * B, [[LEX_MUST] * nq] * B
            sd = torch.empty((B, k), device=dev)
            idd = torch.empty((B, k), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            out = (k, sd.data_ptr(), idd.data_ptr())
            res = rounds(ctx, {"plain": sync(lex.search_device, queries, *out),
                               "bool_should": sync(lex.search_bool_device, queries, should, *out),
                               "bool_and": sync(lex.search_bool_device, queries, must, *out),
                               "bool_min2": sync(lex.search_bool_device, queries, should, *out, [2] * B)})
            same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8))
                       for a, b in zip(lex.search(queries, k), lex.search_bool(queries, should, k)))
            emit({"what": "bool", "B": B, "qterms": nq, "k": k, "should_equals_plain": same,
                  "and_matches_mean": float(lex.count(queries, must).mean()),
                  "min2_matches_mean": float(lex.count(queries, should, [2] * B).mean()), **res})

    occ = np.bincount(terms, minlength=ARGS.terms)                # occurrences, a stand-in for df
    rare = [int(t) for t in np.argsort(np.abs(occ - 300))[:256]]  # about 300 occurrences each
    for which, pick in (("rare", rare), ("common", list(range(256)))):
        for B in (1, 64):
            queries, roles = [[t] for t in pick[:B]], [[LEX_FILTER]] * B
            counts = lex.count(queries, roles)
            cap = int(counts.max())
            cd = torch.empty(B, dtype=torch.int64, device=dev)
            md = torch.empty((B, max(cap, 1)), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            res = rounds(ctx, {"match": sync(lex.match_device, queries, roles, None, cap, cd.data_ptr(), md.data_ptr()),
                               "count": sync(lex.match_device, queries, roles, None, 0, cd.data_ptr(), 0)})
            emit({"what": "match", "which": which, "B": B, "cap": cap, "count_mean": float(counts.mean()), "count_min": int(counts.min()), **res})
            del md

    if ARGS.no_filtered:
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
    q = torch.randn((1, ARGS.dim), generator=g, device=dev).cpu().numpy()
    for name, query in (("and_common", [0, 1]), ("and_mid", [40, 90]), ("rare", [rare[0]])):
        roles = [LEX_MUST] * len(query)
        got = {}

        def match():
            got["counts"], got["ids"] = lex.match([query], [roles])

        def search():
            got["hits"] = vec.search(q, k, filter_ids=got["ids"][0])

        def both():
            match()
            search()

        res = rounds(ctx, {"match": match, "search": search, "match_then_search": both})
        emit({"what": "filtered", "filter": name, "terms": query, "count": int(got["counts"][0]), "vec_rows": ARGS.vec_rows, "dim": ARGS.dim,
              "k": k, **res})


if __name__ == "__main__":
    main()
