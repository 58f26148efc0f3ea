"""NumPy / Python-int model of the field aggregations (include/sqe.h: sqe_index_aggregate_fields): what tests/test_agg_cpu.py
checks by hand and tests/test_agg_gpu.py compares the library with, bit for bit.  The row set is FieldModel.mask of
tests/fields_reference.py, ANDed with an allow-list of ids.  Pure integers; the sums are Python ints."""
import numpy as np

from tests.fields_reference import I64_MAX, NONE, FieldModel

MAX_BUCKETS = 16384


class TooManyBuckets(Exception):
    """A histogram with more than min(bucket_cap, 16384) buckets: the library answers SQE_ERR_INVALID, the stats stay valid."""

    def __init__(self, n_buckets, result):
        super().__init__(f"{n_buckets} buckets")
        self.n_buckets = n_buckets
        self.result = result


def _wrap64(x):
    return (int(x) + (1 << 63)) % (1 << 64) - (1 << 63)


def stats_of(values):
    """values: int64 [m], no NONE among them -> the five stats members, sum exact"""
    values = np.asarray(values, np.int64)
    if values.size == 0:
        return {"count": 0, "min": I64_MAX, "max": NONE, "sum": 0, "sum_lo": 0, "sum_hi": 0}
    ints = [int(v) for v in values]
    lo = sum(v & 0xFFFFFFFF for v in ints)
    hi = sum(v >> 32 for v in ints)
    assert (hi << 32) + lo == sum(ints)
    return {"count": len(ints), "min": min(ints), "max": max(ints), "sum": sum(ints), "sum_lo": lo, "sum_hi": hi}


def terms_of(values, size):
    """-> (keys, counts, n_buckets, other): the best `size` distinct values by (count desc, value asc)"""
    uniq, cnt = np.unique(np.asarray(values, np.int64), return_counts=True)
    order = np.lexsort((uniq, -cnt))[:size]
    keys, counts = uniq[order], cnt[order].astype(np.int64)
    return keys, counts, int(uniq.size), int(cnt.sum() - counts.sum())


def histogram_of(values, interval, offset):
    """-> (keys, counts, n_buckets): every bucket floor((v - offset) / interval) from the lowest occupied to the highest"""
    ints = [int(v) for v in np.asarray(values, np.int64)]
    if not ints:
        return np.empty(0, np.int64), np.empty(0, np.int64), 0
    b = [(v - offset) // interval for v in ints]            # Python ints: nothing wraps, // floors
    kmin, kmax = min(b), max(b)
    nb = kmax - kmin + 1
    if nb > MAX_BUCKETS:
        return None, None, nb
    counts = np.bincount(np.array([x - kmin for x in b], np.int64), minlength=nb).astype(np.int64)
    keys = np.array([_wrap64((kmin + i) * interval + offset) for i in range(nb)], np.int64)
    return keys, counts, nb


def aggregate(model: FieldModel, pred, aggs, filter_ids=None, bucket_cap=None):
    """What VectorIndex.aggregate_fields returns for the same arguments (aggs as pack_aggs takes tuples).  Raises TooManyBuckets
    (with the result that is still valid) where the library refuses."""
    mask = model.mask(pred)
    if filter_ids is not None:
        mask &= np.isin(model.ids, np.asarray(filter_ids, np.int64).reshape(-1))
    if bucket_cap is None:
        bucket_cap = MAX_BUCKETS if any(a[1] == "histogram" for a in aggs) else max([a[2] for a in aggs if a[1] == "terms"], default=0)
    out, too_many = [], None
    for a in aggs:
        field, kind = a[0], a[1]
        col = model.cols.get(field, np.full(model.ids.size, NONE, np.int64))
        vals = col[mask & (col != NONE)]
        r = stats_of(vals)
        del r["sum_lo"], r["sum_hi"]
        r.update(n_buckets=0, other=0, keys=np.empty(0, np.int64), counts=np.empty(0, np.int64))
        if kind == "terms":
            r["keys"], r["counts"], r["n_buckets"], r["other"] = terms_of(vals, a[2])
        elif kind == "histogram":
            keys, counts, nb = histogram_of(vals, a[2], a[3] if len(a) > 3 else 0)
            r["n_buckets"] = nb
            if nb > min(bucket_cap, MAX_BUCKETS):
                too_many = too_many or nb
            else:
                r["keys"], r["counts"] = keys, counts
        out.append(r)
    result = {"selected": int(mask.sum()), "aggs": out}
    if too_many:
        raise TooManyBuckets(too_many, result)
    return result


def same(got, want):
    """bit for bit: every member of every aggregation"""
    if got["selected"] != want["selected"] or len(got["aggs"]) != len(want["aggs"]):
        return False
    for g, w in zip(got["aggs"], want["aggs"]):
        for name in ("count", "min", "max", "sum", "n_buckets", "other"):
            if g[name] != w[name]:
                return False
        if not (np.array_equal(g["keys"], w["keys"]) and np.array_equal(g["counts"], w["counts"])):
            return False
    return True
