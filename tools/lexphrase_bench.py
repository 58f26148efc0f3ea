"""Cost of the phrase queries (sqe_lex_search_phrase, sqe_lex_match_phrase) on the MI355X, beside the AND query of the same terms
through sqe_lex_search_bool (the floor: a phrase does that work and then verifies the order) and beside a host NumPy evaluation.

Corpus: that of tools/lex_bench.py (same generator, same seed): `--docs` documents (default 1 M) of about `--length` term
occurrences over `--terms` terms, term t with probability ~ 1 / (t + 1).  It is built twice, with bags only and with sequences
(sqe_lex_put_ordered): rebuild time and device bytes of both.  One process; wall clock around calls that return synchronised;
median, min and max of `--repeats` rounds after `--warmup` rounds, the variants of one point alternated inside every round.
One JSON line per record:

  corpus    per kind (bags, sequences): last_rebuild_ms of two rebuilds, postings, sequence words, device bytes of the index
  phrase    per (which, L, B): one MUST clause per query.  which = rare (adjacent words of random documents whose first term
            is rare) or common (the most common adjacent pair of the corpus, extended to the right by what follows it in the
            document where it occurs first: the worst case for the verification).  search_phrase_device, search_bool_device
            with every term MUST, match_phrase_device (cap = the largest count) and the count alone, each + synchronise;
            scan_ms / select_ms of one call of each; the mean matches of phrase and AND; host_numpy_ms: the sliding-window
            comparison of one query over the concatenated sequences in NumPy (match only, no scores)
  filtered  one k-NN search (`--vec-rows` x `--dim`, random rows) behind a phrase: match_phrase (host form), the search with
            filter_ids = those ids

SQE_LIB=.../libsqe_reverify.so (make PHRASE_REVERIFY=1) runs the same points on the build that verifies every scoring phrase a
second time when scoring; the field `lib` of each line says which library answered.

usage (GPU box): python tools/lexphrase_bench.py [--out file.jsonl]"""
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
from semantic_query_engine_amd.engine import LEX_MUST

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
        out[name] = {"ms": med(ts[name]), "scan_ms": st["scan_ms"], "select_ms": st["select_ms"]}
    ctx.set_profiling(False)
    return out


def build(ctx, ids, offsets, terms, ordered):
    lex = LexicalIndex(ctx, ARGS.terms)
    step = 100_000
    ms = []
    for again in range(2):                                        # the same documents twice: two rebuilds
        for lo in range(0, ARGS.docs, step):
            hi = min(ARGS.docs, lo + step)
            lex.put(ids[lo:hi], (offsets[lo:hi + 1] - offsets[lo], terms[offsets[lo]:offsets[hi]]), ordered=ordered)
        lex.search([[0]], 1)
        ms.append(lex.info()["last_rebuild_ms"])
    info = lex.info()
    n, p, t, c = info["documents"], info["postings"], ARGS.terms, info["chunks"]
    seq_words = int(offsets[-1]) if ordered else 0
    # ids, dl, fwd_off | fwd_term, fwd_tf, fwd_imp, postings | df, idf | table, cursor | seq_off, seq
    nbytes = 8 * n * 2 + 8 * (n + 1) + p * (4 + 2 + 4 + 8) + t * 12 + c * (2 * t + 1) * 4 + ((n + 1) * 8 + seq_words * 4 if ordered else 0)
    emit({"what": "corpus", "kind": "sequences" if ordered else "bags", "docs": ARGS.docs, "occurrences": int(offsets[-1]),
          "rebuild_ms": ms, "seq_words": seq_words, "index_bytes": nbytes, "device": ctx.device_info(), **info})
    return lex


def host_match(terms, left, phrase):
    """The start positions of the phrase over the concatenated sequences, as a mask; a window never leaves its document."""
    ok = left >= len(phrase)
    n = terms.shape[0]
    for j, t in enumerate(phrase):
        ok[:n - j] &= terms[j:] == t                              # (a window that would pass the end has left < L already)
    return ok


def main():
    rng = np.random.default_rng(1)
    p = 1.0 / np.arange(1, ARGS.terms + 1)
    cdf = np.cumsum(p / p.sum())
    lens = rng.integers(ARGS.length // 2, 3 * ARGS.length // 2 + 1, ARGS.docs)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    terms = draw(rng, cdf, int(offsets[-1]))
    ids = np.arange(ARGS.docs, dtype=np.int64)
    ctx = Context(0)
    build(ctx, ids, offsets, terms, False).close()
    lex = build(ctx, ids, offsets, terms, True)
    row_of = np.repeat(np.arange(ARGS.docs, dtype=np.int32), lens)
    left = (offsets[1:][row_of] - np.arange(terms.shape[0])).astype(np.int32)      # words of the row from this one on

    def sync(fn, *a):
        def call():
            fn(*a)
            ctx.synchronize()
        return call

    qrng = np.random.default_rng(2)
    k = ARGS.k
    # the most common adjacent pair inside one document; under this distribution it is made of the 16 most common terms
    inside = (left[:-1] >= 2) & (terms[:-1] < 16) & (terms[1:] < 16)
    pair = terms[:-1] * 16 + terms[1:]
    top = int(np.argmax(np.bincount(pair[inside], minlength=256)))
    first = int(np.nonzero(inside & (pair == top))[0][0])
    rare_starts = np.nonzero((terms >= 2000) & (left >= 4))[0]
    for which in ("rare", "common"):
        for L in (2, 4):
            for B in (1, 64, 256):
                if which == "common":                             # the same phrase B times: every workgroup at the worst case
                    at = first if left[first] >= L else int(np.nonzero(inside & (pair == top) & (left[:-1] >= L))[0][0])
                    phrases = [[int(t) for t in terms[at:at + L]]] * B
                else:
                    phrases = [[int(t) for t in terms[s:s + L]] for s in qrng.choice(rare_starts, B)]
                clause_q, clause_r = [[ph] for ph in phrases], [[LEX_MUST]] * B
                and_r = [[LEX_MUST] * L] * B
                sd = torch.empty((B, k), device=dev)
                idd = torch.empty((B, k), dtype=torch.int64, device=dev)
                counts = lex.count_phrase(clause_q, clause_r)
                cap = max(1, int(counts.max()))
                cd = torch.empty(B, dtype=torch.int64, device=dev)
                md = torch.empty((B, cap), dtype=torch.int64, device=dev)
                torch.cuda.synchronize()
                out = (k, sd.data_ptr(), idd.data_ptr())
                res = rounds(ctx, {"phrase": sync(lex.search_phrase_device, clause_q, clause_r, *out),
                                   "bool_and": sync(lex.search_bool_device, phrases, and_r, *out),
                                   "match_phrase": sync(lex.match_phrase_device, clause_q, clause_r, None, cap, cd.data_ptr(), md.data_ptr()),
                                   "count_phrase": sync(lex.match_phrase_device, clause_q, clause_r, None, 0, cd.data_ptr(), 0)})
                t0 = time.perf_counter()
                host_rows = np.unique(row_of[host_match(terms, left, phrases[0])]).shape[0]
                host_ms = (time.perf_counter() - t0) * 1e3
                emit({"what": "phrase", "which": which, "L": L, "B": B, "k": k, "phrase_matches_mean": float(counts.mean()),
                      "and_matches_mean": float(lex.count(phrases, and_r).mean()), "host_numpy_ms": host_ms,
                      "host_agrees": host_rows == int(counts[0]), **res})
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
    phrase = [int(t) for t in terms[first:first + 2]]
    got = {}

    def match():
        got["counts"], got["ids"] = lex.match_phrase([[phrase]], [[LEX_MUST]])

    def search():
        got["hits"] = vec.search(q, k, filter_ids=got["ids"][0])

    def both():
        match()
        search()

    res = rounds(ctx, {"match_phrase": match, "search": search, "match_then_search": both})
    emit({"what": "filtered", "phrase": phrase, "count": int(got["counts"][0]), "vec_rows": ARGS.vec_rows, "dim": ARGS.dim, "k": k, **res})


if __name__ == "__main__":
    main()
