"""Cost of sorting on fields (sqe_index_sort_fields) on a 10 M-row flat index (dim 64: the vectors are never read).

Columns: SEL uniform 0 .. 999,999 (so `SEL < f * 1e6` selects the fraction f of the rows), YEAR (35 distinct values), STAMP
(nearly unique: uniform below 2^40), SCORE (30 % missing).  Per predicate fraction 0.01 % / 1 % / 50 % / 100 %, per sort of 1 key
(YEAR desc: the k-th place always lies in a run of ties; STAMP asc: it never does) and of 3 keys (YEAR desc, SCORE asc missing
first, STAMP desc), per k 10 / 256, without and with a cursor (the last hit of the first page) one JSON line with
  wall_ms      median wall time of VectorIndex.sort_fields (after one warm-up)
  prep_ms / select_ms   device time of one call from the profiler: bitmap; slab + merge kernels
  last         the sqe_index_sort_last record of that call
  host_ms      what a caller did before, once: match_fields(cap = count), get_field per key, np.lexsort on the host
and the answers of the device and of the host way are compared.

usage (GPU box): python tools/sort_bench.py [rows] [out.jsonl]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from semantic_query_engine_amd import Context, VectorIndex
from semantic_query_engine_amd.engine import FIELD_NONE

D = 64
ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else ""
CHUNK = 1 << 20
SEL, YEAR, STAMP, SCORE = range(4)
FRACTIONS = (0.0001, 0.01, 0.5, 1.0)
dev = torch.device("cuda", 0)
U64 = np.uint64


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
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
    rng = np.random.default_rng(5)
    score = rng.integers(-(1 << 40), 1 << 40, ROWS)
    score[rng.random(ROWS) < 0.3] = FIELD_NONE
    cols = {SEL: rng.integers(0, 1_000_000, ROWS), YEAR: rng.integers(1990, 2025, ROWS), STAMP: rng.integers(0, 1 << 40, ROWS), SCORE: score}
    ids = np.arange(ROWS, dtype=np.int64)
    for f, col in cols.items():
        idx.set_field(f, ids, col.astype(np.int64))
    return idx


def image(v, desc, first):
    """the order image of include/sqe.h, as tests/sort_reference.py computes it"""
    b = v.view(U64) ^ U64(1 << 63)
    with np.errstate(over="ignore"):
        u = ((U64(0) - b) if first else ~b) if desc else (b if first else b - U64(1))
    return np.where(v == FIELD_NONE, U64(0) if first else U64(0xFFFFFFFFFFFFFFFF), u)


def host_way(idx, pred, sort, k, after):
    """today's route: every matching id and its values to the host, np.lexsort there"""
    count = int(idx.count_fields([pred])[0])
    ids = idx.match_fields([pred], count)[1][0]
    raw = [idx.get_field(key[0], ids) for key in sort]
    img = [image(v, key[1] == "desc", len(key) > 2 and key[2]["missing"] == "first") for key, v in zip(sort, raw)]
    keep = np.ones(ids.size, bool)
    if after is not None:
        cur = [image(np.array([FIELD_NONE if v is None else v], np.int64), key[1] == "desc", len(key) > 2 and key[2]["missing"] == "first")[0]
               for key, v in zip(sort, after[0])]
        gt, eq = np.zeros(ids.size, bool), np.ones(ids.size, bool)
        for u, c in zip(img, cur):
            gt |= eq & (u > c)
            eq &= u == c
        keep = gt | (eq & (ids > after[1]))
    pos = np.flatnonzero(keep)
    order = pos[np.lexsort((ids[pos],) + tuple(u[pos] for u in reversed(img)))[:k]]
    return count, ids[order], np.array([v[order] for v in raw], np.int64).T.reshape(order.size, len(sort))


def device_ms(ctx, fn):
    ctx.stats_reset()
    fn()
    st = ctx.stats()
    return {k: round(st[k], 4) for k in ("prep_ms", "select_ms")}


def main():
    ctx = Context(0)
    t0 = time.perf_counter()
    idx = build(ctx)
    emit({"what": "build", "rows": ROWS, "s": round(time.perf_counter() - t0, 1), "device": str(ctx.device_info())})
    ctx.set_profiling(True)
    sorts = [
        ("1key_35_values", [(YEAR, "desc")]),
        ("1key_nearly_unique", [(STAMP, "asc")]),
        ("3keys", [(YEAR, "desc"), (SCORE, "asc", {"missing": "first"}), (STAMP, "desc")]),
    ]
    for frac in FRACTIONS:
        pred = [] if frac == 1.0 else [(SEL, "range", None, int(frac * 1_000_000) - 1)]
        for name, sort in sorts:
            for k in (10, 256):
                first = idx.sort_fields(pred, sort, k)
                cursor = None
                if first["ids"].size:
                    cursor = ([None if v == FIELD_NONE else int(v) for v in first["values"][-1]], int(first["ids"][-1]))
                for after in (None, cursor):
                    if after is None and cursor is None and first["total"]:
                        continue
                    run = lambda: idx.sort_fields(pred, sort, k, after=after)         # noqa: E731
                    got = run()
                    wall = []
                    for _ in range(5):
                        t = time.perf_counter()
                        run()
                        wall.append((time.perf_counter() - t) * 1e3)
                    dms = device_ms(ctx, run)
                    last = idx.sort_last()
                    t = time.perf_counter()
                    count, ids, values = host_way(idx, pred, sort, k, after)
                    host_ms = (time.perf_counter() - t) * 1e3
                    ok = got["total"] == count and np.array_equal(got["ids"], ids) and np.array_equal(got["values"], values)
                    emit({"what": name, "fraction": frac, "k": k, "cursor": after is not None, "total": got["total"],
                          "wall_ms": round(statistics.median(wall), 3), **dms, "host_ms": round(host_ms, 1), "same": bool(ok), "last": last})


if __name__ == "__main__":
    main()
