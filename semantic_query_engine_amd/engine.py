"""Thin object layer over the C ABI (include/sqe.h): Context, VectorIndex, LexicalIndex, CacheMatrix.

NumPy in / NumPy out for host callers; raw device pointers (``tensor.data_ptr()``) for
callers that already hold their data in HBM.  No arithmetic happens here.
"""
from __future__ import annotations

import ctypes as C
import threading
import weakref
from typing import Optional, Tuple

import numpy as np

from . import _native as N

INDEX_FLAT = 0
INDEX_IVF_FLAT = 1
SCAN_BF16_RESCORE = 0
SCAN_INT8_RESCORE = 2
FUSE_MODES = {"max": 0, "rrf": 1}      # SQE_FUSE_MAX / SQE_FUSE_RRF (VectorIndex.search_fused)
# buffers of the int8 first pass (VectorIndex.i8_read; include/sqe.h: SQE_I8_*)
KEY_NONE = -(1 << 63)      # SQE_KEY_NONE: a row without a group key (VectorIndex.set_keys / search_collapsed)
FIELD_NONE = -(1 << 63)    # SQE_FIELD_NONE: a row without a value in a field (VectorIndex.set_field / match_fields)
MAX_FIELDS = 8
FIELD_MAX_PREDS, FIELD_MAX_CLAUSES, FIELD_MAX_SET = 64, 8, 4096
FOP_RANGE, FOP_IN, FOP_NOT = 0, 1, 0x100
FIELD_DTYPE = np.dtype([("field", "<i4"), ("op", "<i4"), ("lo", "<i8"), ("hi", "<i8")])      # sqe_field_clause_t
# field aggregations (VectorIndex.aggregate_fields; include/sqe.h: SQE_AGG_*)
AGG_KINDS = {"stats": 0, "terms": 1, "histogram": 2}
AGG_ROUTE_NONE, AGG_ROUTE_DENSE, AGG_ROUTE_HASH = range(3)
AGG_MAX, AGG_MAX_SIZE, AGG_MAX_BUCKETS = 8, 256, 16384
AGG_DTYPE = np.dtype([("kind", "<i4"), ("field", "<i4"), ("size", "<i4"), ("pad", "<i4"), ("interval", "<i8"), ("offset", "<i8")])   # sqe_field_agg_t
AGG_RESULT_DTYPE = np.dtype([(name, "<i8") for name in ("count", "min", "max", "sum_lo", "sum_hi", "n_buckets", "other")])   # sqe_field_agg_result_t
I8_ROWS, I8_ROW_SCALES, I8_QUERIES, I8_THRESHOLDS, I8_LIST_COUNTS, I8_LISTS, I8_SAMPLE_BEST, I8_POOL_COUNTS, I8_POOLS = range(9)
I8_QUERIES_TILED = 9
(I8_THR_EFF, I8_SAMPLE_COS, I8_SAMPLE_IDS, I8_SELECT_COS, I8_SELECT_IDS, I8_SELECT_THR, I8_SELECT_TRACE) = range(10, 17)   # the last four: "i8_keep_select"
# the kernel of the last int8 collect launch (VectorIndex.i8_last()["kernel"]; include/sqe.h: SQE_I8_KERNEL_*)
(I8_KERNEL_PP, I8_KERNEL_DEEP, I8_KERNEL_STREAM_64_32, I8_KERNEL_STREAM_64_16, I8_KERNEL_STREAM_128_16, I8_KERNEL_STAGED_64,
 I8_KERNEL_STAGED_128) = range(1, 8)
# the last bf16 first pass (VectorIndex.scan_last / scan_read; include/sqe.h: SQE_SCAN_*)
SCAN_LISTS, SCAN_LIST_COUNTS, SCAN_BOUNDS, SCAN_COLLECT_THR, SCAN_UNC_COUNT, SCAN_UNC_IDS, SCAN_COLLECT_COUNTS, SCAN_COLLECT_KEYS = range(8)
SCAN_FAMILY_PINGPONG, SCAN_FAMILY_STAGED = range(2)

# scanned copies and measured residuals (VectorIndex.state_read; include/sqe.h: SQE_STATE_*)
STATE_SCAN_BF16, STATE_RESID_MAX, STATE_I8_RESID_MAX, STATE_QN, STATE_Q_RESID, STATE_Q8_RESID, STATE_Q8_SCALES = range(7)

# state of the last IVF search (VectorIndex.ivf_state / ivf_state_read; include/sqe.h: SQE_IVF_*)
(IVF_PROBES, IVF_PROBES_COS, IVF_STRIPS, IVF_ORDER, IVF_OFFSETS, IVF_TILE_OFF, IVF_SCAN_BF16, IVF_ROWS_F32, IVF_I8_ROWS,
 IVF_I8_ROW_SCALES, IVF_Q8, IVF_Q8_SCALES, IVF_QN, IVF_QB, IVF_THRESHOLDS, IVF_COUNTS, IVF_KEY_LISTS) = range(17)
# device state of a lexical index (LexicalIndex.state_read; include/sqe.h: SQE_LEX_*)
LEX_DF, LEX_IDF, LEX_IDS, LEX_DL, LEX_TABLE, LEX_POSTINGS, LEX_SEQ_OFF, LEX_SEQ = range(8)
IVF_COARSE_DENSE, IVF_COARSE_FLAT = range(2)
IVF_KERNEL_FP32, IVF_KERNEL_BF16_MFMA, IVF_KERNEL_I8_STAGED, IVF_KERNEL_I8_STREAM = range(4)
IVF_GRID_LIST, IVF_GRID_PAIR, IVF_GRID_PAIR_GRID, IVF_GRID_UNITS1, IVF_GRID_UNITS4, IVF_GRID_COLLECT = range(6)
IVF_QUEUED_STRIPS, IVF_QUEUED_SAMPLE, IVF_QUEUED_COLLECT, IVF_QUEUED_FALLBACK = 1, 2, 4, 8


def _f32(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _queries(q, dim: int, what: str = "queries") -> np.ndarray:
    """The query block of a search: contiguous float32 [B, dim]; one vector is a batch of one."""
    q = _f32(q)
    if q.ndim == 1:
        q = q[None]
    if q.shape[1] != dim:
        raise ValueError(f"expected [{'B' if what == 'queries' else 'Bs'}, {dim}] {what}, got {q.shape}")
    return q


def _pack_id_lists(lists, list_of_query, b: int, none_is_no_list: bool):
    """The id lists of ``b`` queries as the C ABI takes them -> (ids int64 [total], offsets int64 [n_lists + 1],
    list_of_query int32 [b], n_lists).  ``list_of_query=None`` is ``arange(b)`` and needs one list per query.  With
    ``none_is_no_list`` a ``None`` entry of ``lists`` is an empty list and every query that names it gets -1."""
    lists = list(lists)
    if list_of_query is None:
        if len(lists) != b:
            raise ValueError(f"{len(lists)} lists for {b} queries: pass list_of_query")
        loq = np.arange(b, dtype=np.int32)
    else:
        loq = np.array(list_of_query, dtype=np.int32).reshape(-1)
        if loq.shape[0] != b:
            raise ValueError(f"list_of_query has {loq.shape[0]} entries for {b} queries")
    if none_is_no_list:
        absent = np.array([ids is None for ids in lists], dtype=bool)
        if absent.any():
            named = (loq >= 0) & (loq < len(lists))
            loq[named & absent[np.clip(loq, 0, len(lists) - 1)]] = -1
        lists = [() if ids is None else ids for ids in lists]
    arrays = [np.ascontiguousarray(ids, dtype=np.int64).reshape(-1) for ids in lists]
    offsets = np.zeros(len(arrays) + 1, np.int64)
    if arrays:
        np.cumsum([a.shape[0] for a in arrays], out=offsets[1:])
    return (np.concatenate(arrays) if arrays else np.empty(0, np.int64)), offsets, loq, len(arrays)


def f64_image(x):
    """The order-preserving int64 image of doubles: a < b as doubles iff f64_image(a) < f64_image(b), with -0.0 mapped to +0.0
    (so both zeros are one value).  Total: infinities keep their place at the ends; every NaN lands beyond an infinity -- above
    +inf with the sign bit clear, below -inf with it set.  Float fields go through it, values and predicate bounds alike; no
    image equals FIELD_NONE (the lowest, a NaN of all ones, is FIELD_NONE + 1).  Scalar in, int out; array in, int64 array out."""
    a = np.asarray(x, dtype=np.float64)
    shape = a.shape
    a = np.atleast_1d(a) + 0.0                         # -0.0 + 0.0 == +0.0; everything else unchanged (NaN stays NaN)
    b = np.ascontiguousarray(a).view(np.int64)
    # a negative double is sign bit + magnitude m, m >= 1 now: its image is -m, at least FIELD_NONE + 1 (the NaN of all ones)
    img = np.where(b >= 0, b, np.int64(-(1 << 63)) - b).reshape(shape)
    return int(img) if img.ndim == 0 else img


def f64_from_image(img):
    """The inverse of ``f64_image``: the double whose image is ``img`` (the image of -0.0 and +0.0 gives +0.0; the image of a NaN
    gives a NaN).  Scalar in, float out; array in, float64 array out."""
    b = np.asarray(img, dtype=np.int64)
    shape = b.shape
    b = np.atleast_1d(b)
    # a non-negative image is the bit pattern itself; a negative one is -m for the magnitude m under the sign bit
    bits = np.where(b >= 0, b, np.int64(-(1 << 63)) - b)
    out = np.ascontiguousarray(bits).view(np.float64).reshape(shape)
    return float(out) if out.ndim == 0 else out


WHERE_ROUTE_NONE, WHERE_ROUTE_GATHER, WHERE_ROUTE_MASK = 0, 1, 2      # sqe.h: SQE_WHERE_ROUTE_*; the last two are "where_route" values


def where_depth(k: int, selected: int, live: int) -> int:
    """Rows the first stage of the mask route of ``search_where`` fetches when ``selected`` of ``live`` rows pass the predicate:
    the smallest d in [k, 256] with P[Binomial(d, selected / live) < k] <= 2^-10, 0 if there is none or selected < k
    (sqe_where_depth; host arithmetic, no device)."""
    return int(N.load().sqe_where_depth(int(k), int(selected), int(live)))


def pack_aggs(aggs):
    """Aggregations as the C ABI takes them -> AGG_DTYPE [n_aggs].  An aggregation is ``(field, "stats")``, ``(field, "terms",
    size)`` or ``(field, "histogram", interval, offset=0)``, or a dict ``{"field", "kind", "size" / "interval", "offset"}``.  The
    limits (1..8 aggregations, slots 0..7, 1 <= size <= 256, interval >= 1, 0 <= offset < interval) are checked here and again by
    the library."""
    aggs = list(aggs)
    if not 1 <= len(aggs) <= AGG_MAX:
        raise ValueError(f"{len(aggs)} aggregations in one call (between 1 and {AGG_MAX})")
    rows = []
    for a in aggs:
        if isinstance(a, dict):
            field, kind = a["field"], a["kind"]
            size, interval, offset = a.get("size", 10), a.get("interval", 1), a.get("offset", 0)
        else:
            a = tuple(a)
            field, kind = a[0], a[1]
            size = a[2] if kind == "terms" and len(a) > 2 else 10
            interval = a[2] if kind == "histogram" and len(a) > 2 else 1
            offset = a[3] if kind == "histogram" and len(a) > 3 else 0
        field = int(field)
        if not 0 <= field < MAX_FIELDS:
            raise ValueError(f"field slot {field} is outside 0..{MAX_FIELDS - 1}")
        if kind not in AGG_KINDS:
            raise ValueError(f"unknown aggregation kind {kind!r} (served: stats, terms, histogram)")
        if kind == "terms" and not 1 <= int(size) <= AGG_MAX_SIZE:
            raise ValueError(f"terms size {size} is outside 1..{AGG_MAX_SIZE}")
        if kind == "histogram" and not (int(interval) >= 1 and 0 <= int(offset) < int(interval)):
            raise ValueError(f"histogram needs interval >= 1 and 0 <= offset < interval, not {interval} and {offset}")
        rows.append((AGG_KINDS[kind], field, int(size) if kind == "terms" else 0, 0, int(interval) if kind == "histogram" else 0,
                     int(offset) if kind == "histogram" else 0))
    return np.array(rows, dtype=AGG_DTYPE)


SORT_DESC, SORT_MISSING_FIRST = 1, 2     # SQE_SORT_DESC, SQE_SORT_MISSING_FIRST
SORT_MAX_KEYS, SORT_MAX_K = 4, 256
SORT_DTYPE = np.dtype([("field", np.int32), ("flags", np.int32)])      # sqe_field_sort_t


def pack_sort(sort):
    """Sort keys as the C ABI takes them -> SORT_DTYPE [n_sort].  A key is ``(slot, "asc" | "desc")`` or ``(slot, order,
    {"missing": "first" | "last"})`` (default last, whatever the direction).  The limits (1..4 keys, slots 0..7, each named once)
    are checked here and again by the library."""
    sort = list(sort)
    if not 1 <= len(sort) <= SORT_MAX_KEYS:
        raise ValueError(f"{len(sort)} sort keys in one call (between 1 and {SORT_MAX_KEYS})")
    rows = []
    for key in sort:
        key = tuple(key)
        if not 2 <= len(key) <= 3:
            raise ValueError(f"a sort key is (slot, order) or (slot, order, {{'missing': ...}}), not {key!r}")
        field, order = int(key[0]), key[1]
        missing = key[2].get("missing", "last") if len(key) == 3 else "last"
        if not 0 <= field < MAX_FIELDS:
            raise ValueError(f"field slot {field} is outside 0..{MAX_FIELDS - 1}")
        if order not in ("asc", "desc"):
            raise ValueError(f"unknown sort order {order!r} (asc or desc)")
        if missing not in ("first", "last"):
            raise ValueError(f"unknown missing placement {missing!r} (first or last)")
        if any(r[0] == field for r in rows):
            raise ValueError(f"field slot {field} is named by two sort keys")
        rows.append((field, (SORT_DESC if order == "desc" else 0) | (SORT_MISSING_FIRST if missing == "first" else 0)))
    return np.array(rows, dtype=SORT_DTYPE)


def pack_predicates(preds):
    """Predicates as the C ABI takes them -> (clauses FIELD_DTYPE [n_clauses], pred_offsets int64 [n_preds + 1], set_values
    int64 [n_set]).  A predicate is a list of clauses ``(field, "range", lo, hi)`` / ``(field, "in", values)``, each with an
    optional trailing ``{"not_": True}`` or as a dict ``{"field", "op", "lo", "hi" / "values", "not_"}``; ``lo`` / ``hi`` None
    mean unbounded (never FIELD_NONE: an unbounded range is "exists").  The values of an "in" clause are sorted and deduplicated
    here.  The limits (64 predicates, 8 clauses each, 4,096 set values in all) are checked here and again by the library."""
    preds = list(preds)
    if len(preds) > FIELD_MAX_PREDS:
        raise ValueError(f"{len(preds)} predicates in one call (at most {FIELD_MAX_PREDS})")
    rows, offsets, sets, n_set = [], [0], [], 0
    for pred in preds:
        pred = list(pred)
        if len(pred) > FIELD_MAX_CLAUSES:
            raise ValueError(f"{len(pred)} clauses in one predicate (at most {FIELD_MAX_CLAUSES})")
        for cl in pred:
            if isinstance(cl, dict):
                field, op, not_ = cl["field"], cl["op"], bool(cl.get("not_", False))
                args = (cl.get("lo"), cl.get("hi")) if op == "range" else (cl["values"],)
            else:
                cl = tuple(cl)
                not_ = False
                if cl and isinstance(cl[-1], dict):
                    not_ = bool(cl[-1].get("not_", False))
                    cl = cl[:-1]
                field, op, args = cl[0], cl[1], cl[2:]
            field = int(field)
            if not 0 <= field < MAX_FIELDS:
                raise ValueError(f"field slot {field} is outside 0..{MAX_FIELDS - 1}")
            flag = FOP_NOT if not_ else 0
            if op == "range":
                lo, hi = (tuple(args) + (None, None))[:2]
                rows.append((field, FOP_RANGE | flag, FIELD_NONE + 1 if lo is None else int(lo), (1 << 63) - 1 if hi is None else int(hi)))
            elif op == "in":
                vals = np.unique(np.asarray(args[0], dtype=np.int64).reshape(-1))
                rows.append((field, FOP_IN | flag, n_set, n_set + vals.shape[0]))
                sets.append(vals)
                n_set += vals.shape[0]
            else:
                raise ValueError(f"unknown clause op {op!r}")
        offsets.append(len(rows))
    if n_set > FIELD_MAX_SET:
        raise ValueError(f"{n_set} set values in one call (at most {FIELD_MAX_SET})")
    clauses = np.array(rows, dtype=FIELD_DTYPE) if rows else np.empty(0, FIELD_DTYPE)
    return clauses, np.array(offsets, np.int64), (np.concatenate(sets) if sets else np.empty(0, np.int64))


EXCHANGE_AUTO, EXCHANGE_RCCL, EXCHANGE_COPY = 0, 1, 2


class Context:
    """One MI355X device (``device``: the local HIP ordinal -- the form used with one process per GPU), or
    ONE host process driving several (``devices=[0, 1, ...]``: flat indexes created on the context are
    sharded row-wise over them and searched with one exchange step, RCCL all-gather or peer copies;
    device pointers handed to the ``*_device`` calls are memory of ``devices[0]``).  Repeating a device id
    makes logical shards on one device (``exchange`` then has to be AUTO or COPY)."""

    def __init__(self, device: int = 0, devices=None, exchange: int = EXCHANGE_AUTO):
        self.lib = N.load()
        h = C.c_void_p()
        if devices is None:
            ids = (C.c_int32 * 1)(device)
            N.check(self.lib.sqe_create(ids, 1, C.byref(h)))
            self.devices = [device]
        else:
            self.devices = [int(d) for d in devices]
            ids = (C.c_int32 * len(self.devices))(*self.devices)
            N.check(self.lib.sqe_create_sharded(ids, len(self.devices), exchange, C.byref(h)))
        self.handle = h
        self.device = self.devices[0]
        self._children = weakref.WeakSet()      # indexes / caches that must die first

    def group_info(self) -> dict:
        """{"shards": P, "exchange": "rccl" | "copy", "devices": [...]} (one shard for a single-device context)."""
        n, ex = C.c_int32(), C.c_int32()
        devs = (C.c_int32 * 64)()
        N.check(self.lib.sqe_group_info(self.handle, C.byref(n), C.byref(ex), devs, 64))
        return {"shards": n.value, "exchange": {EXCHANGE_RCCL: "rccl", EXCHANGE_COPY: "copy"}.get(ex.value, "auto"),
                "devices": list(devs[:n.value])}

    def close(self) -> None:
        if getattr(self, "handle", None):
            for child in list(self._children):
                child.close()
            self.lib.sqe_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self) -> None:
        N.check(self.lib.sqe_synchronize(self.handle))

    @property
    def stream(self) -> int:
        return int(self.lib.sqe_stream(self.handle) or 0)

    def set_stream(self, hip_stream: int) -> None:
        """Enqueue on a caller-owned stream (e.g. ``torch.cuda.current_stream().cuda_stream``);
        0 restores the context's own stream."""
        N.check(self.lib.sqe_set_stream(self.handle, hip_stream or None))

    def device_info(self):
        name = C.create_string_buffer(128)
        cu = C.c_int32()
        mem = C.c_int64()
        N.check(self.lib.sqe_device_info(self.handle, name, 128, C.byref(cu), C.byref(mem)))
        return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}

    def set_profiling(self, on: bool) -> None:
        N.check(self.lib.sqe_set_profiling(self.handle, int(on)))

    def stats(self) -> dict:
        s = N.Stats()
        N.check(self.lib.sqe_stats(self.handle, C.byref(s)))
        out = {f: getattr(s, f) for f, _ in N.Stats._fields_}
        swept = C.c_int64()
        N.check(self.lib.sqe_collapse_swept(self.handle, C.byref(swept)))
        out["collapse_swept"] = int(swept.value)      # queries of the last collapsed search that the sweep answered
        return out

    def exclude_swept(self) -> int:
        """Queries of the last ``search_excluding`` that the sweep over all rows answered (sqe_exclude_swept)."""
        swept = C.c_int64()
        N.check(self.lib.sqe_exclude_swept(self.handle, C.byref(swept)))
        return int(swept.value)

    def stats_reset(self) -> None:
        N.check(self.lib.sqe_stats_reset(self.handle))

    # -- cache scan, one-shot (main.py:73-87)
    def cosine_best(self, mat: np.ndarray, q: np.ndarray) -> Tuple[float, int]:
        q = _f32(q).reshape(-1)
        mat = _f32(mat).reshape(-1, q.shape[0]) if mat.size else np.zeros((0, q.shape[0]), np.float32)
        sim = C.c_float()
        idx = C.c_int32()
        N.check(self.lib.sqe_cosine_best(self.handle, mat.ctypes.data, mat.shape[0], q.shape[0],
                                         q.ctypes.data, C.byref(sim), C.byref(idx)))
        return float(sim.value), int(idx.value)

    def cosine_all(self, mat: np.ndarray, q: np.ndarray) -> np.ndarray:
        q = _f32(q).reshape(-1)
        mat = _f32(mat).reshape(-1, q.shape[0])
        out = np.empty(mat.shape[0], np.float32)
        N.check(self.lib.sqe_cosine_all(self.handle, mat.ctypes.data, mat.shape[0], q.shape[0],
                                        q.ctypes.data, out.ctypes.data))
        return out

    def merge_topk_device(self, cos_parts_ptr: int, id_parts_ptr: int, part_stride_bytes: int,
                          P: int, B: int, k: int, cos_out_ptr: int, id_out_ptr: int) -> None:
        N.check(self.lib.sqe_merge_topk_device(self.handle, cos_parts_ptr, id_parts_ptr, part_stride_bytes,
                                               P, B, k, cos_out_ptr, id_out_ptr))


class VectorIndex:
    """Cosine index over ``dim``-d vectors held in HBM (fp32 master + bf16 scanned copy)."""

    def __init__(self, ctx: Context, dim: int = 1024, kind: int = INDEX_FLAT, nlist: int = 0):
        self.ctx = ctx
        self.lib = ctx.lib
        self.dim = dim
        h = C.c_void_p()
        N.check(self.lib.sqe_index_create(ctx.handle, dim, kind, nlist, C.byref(h)))
        self.handle = h
        ctx._children.add(self)

    @classmethod
    def load(cls, ctx: Context, path: str) -> "VectorIndex":
        """Read an index written by ``save`` (sqe_index_load): same rows, bit-identical results."""
        import struct
        with open(path, "rb") as f:
            head = f.read(24)
        if len(head) < 24 or head[:8] != b"SQEIDX01":
            raise N.SqeError(-6, f"{path}: not a saved index")
        _version, dim, _kind, _nlist = struct.unpack_from("<IIII", head, 8)
        self = cls.__new__(cls)
        self.ctx, self.lib, self.dim = ctx, ctx.lib, int(dim)
        h = C.c_void_p()
        N.check(self.lib.sqe_index_load(ctx.handle, path.encode(), C.byref(h)))
        self.handle = h
        ctx._children.add(self)
        return self

    def save(self, path: str) -> None:
        """Write the stored (normalised) rows, and the IVF centroids/assignments if trained, to a local file."""
        N.check(self.lib.sqe_index_save(self.handle, path.encode()))

    def close(self) -> None:
        if getattr(self, "handle", None):
            if self.ctx.handle:                 # a destroyed context already released the device
                self.lib.sqe_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        """Live rows (deleted rows are gone)."""
        n = C.c_int64()
        N.check(self.lib.sqe_index_count(self.handle, C.byref(n)))
        return int(n.value)

    @property
    def next_id(self) -> int:
        """The id the next added row gets (= rows ever added; ids are never reused)."""
        n = C.c_int64()
        N.check(self.lib.sqe_index_next_id(self.handle, C.byref(n)))
        return int(n.value)

    def ids(self) -> np.ndarray:
        """Live ids, ascending (int64 [len(self)])."""
        out = np.empty(len(self), np.int64)
        N.check(self.lib.sqe_index_ids(self.handle, out.ctypes.data, out.shape[0]))
        return out

    def delete(self, ids) -> None:
        """Remove the rows with these ids (sqe_index_delete): all must be live and distinct, else nothing is deleted."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if ids.size:
            N.check(self.lib.sqe_index_delete(self.handle, ids.ctypes.data, ids.shape[0]))

    def delete_last(self) -> dict:
        """The blocks the last delete of this index walked, staged and direct (sqe_index_delete_last)."""
        L = N.DeleteLast()
        N.check(self.lib.sqe_index_delete_last(self.handle, L))
        return {name: getattr(L, name) for name, _ in N.DeleteLast._fields_}

    def reserve(self, rows: int) -> None:
        N.check(self.lib.sqe_index_reserve(self.handle, rows))

    def set_option(self, key: str, value: float) -> None:
        N.check(self.lib.sqe_index_set_option(self.handle, key.encode(), float(value)))

    def add(self, x: np.ndarray) -> None:
        x = _f32(x)
        if x.size == 0:
            return
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected [n, {self.dim}] array, got {x.shape}")
        N.check(self.lib.sqe_index_add(self.handle, x.ctypes.data, x.shape[0]))

    def add_device(self, ptr: int, n: int) -> None:
        N.check(self.lib.sqe_index_add_device(self.handle, ptr, n))

    def update(self, rows: np.ndarray, x: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        x = _f32(x)
        if x.shape != (rows.shape[0], self.dim):
            raise ValueError(f"expected [{rows.shape[0]}, {self.dim}] array for {rows.shape[0]} rows, got {x.shape}")
        if rows.size:
            N.check(self.lib.sqe_index_update(self.handle, rows.ctypes.data, x.ctypes.data, rows.shape[0]))

    def get_rows(self, rows) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((rows.shape[0], self.dim), np.float32)
        if rows.size:
            N.check(self.lib.sqe_index_get_rows(self.handle, rows.ctypes.data, rows.shape[0], out.ctypes.data))
        return out

    # -- IVF-flat only
    def train(self, x: np.ndarray, iters: int = 20, seed: int = 0) -> None:
        """Spherical k-means on the sample ``x`` (host array), then (re)assignment of stored rows."""
        x = _f32(x)
        N.check(self.lib.sqe_index_train(self.handle, x.ctypes.data, x.shape[0], iters, seed))

    def train_device(self, ptr: int, n: int, iters: int = 20, seed: int = 0) -> None:
        N.check(self.lib.sqe_index_train_device(self.handle, ptr, n, iters, seed))

    def ivf_export(self, nlist: int) -> Tuple[np.ndarray, np.ndarray]:
        """-> (centroids float32 [nlist, dim], list id of every stored row int32 [count])."""
        cen = np.empty((nlist, self.dim), np.float32)
        asg = np.empty(len(self), np.int32)
        N.check(self.lib.sqe_index_ivf_export(self.handle, cen.ctypes.data, asg.ctypes.data))
        return cen, asg

    def ivf_state(self) -> dict:
        """Shapes and route of the last IVF search piece: which list-scan kernel and grid ran (sqe_index_ivf_state)."""
        st = N.IvfSearchState()
        N.check(self.lib.sqe_index_ivf_state(self.handle, st))
        return {name: getattr(st, name) for name, _ in N.IvfSearchState._fields_}

    def ivf_state_read(self, what: int, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        """`count` elements of `dtype` from a buffer of the last IVF search (sqe_index_ivf_state_read; what = IVF_*)."""
        out = np.empty(count, dtype)
        N.check(self.lib.sqe_index_ivf_state_read(self.handle, what, offset_bytes, out.ctypes.data, out.nbytes))
        return out

    def i8_last(self) -> dict:
        """What the last search answered by the int8 first pass launched (sqe_index_i8_last)."""
        L = N.I8Launch()
        N.check(self.lib.sqe_index_i8_last(self.handle, L))
        return {name: getattr(L, name) for name, _ in N.I8Launch._fields_}

    def i8_read(self, what: int, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        """`count` elements of `dtype` from one of the int8 pass's device buffers (sqe_index_i8_read; what = I8_*)."""
        out = np.empty(count, dtype)
        N.check(self.lib.sqe_index_i8_read(self.handle, what, offset_bytes, out.ctypes.data, out.nbytes))
        return out

    def scan_last(self) -> dict:
        """What the last search pass launched when the bf16 first pass answered it (sqe_index_scan_last)."""
        L = N.ScanLaunch()
        N.check(self.lib.sqe_index_scan_last(self.handle, L))
        return {name: getattr(L, name) for name, _ in N.ScanLaunch._fields_}

    def scan_read(self, what: int, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        """`count` elements of `dtype` from a buffer the last bf16 first pass left (sqe_index_scan_read; what = SCAN_*)."""
        out = np.empty(count, dtype)
        N.check(self.lib.sqe_index_scan_read(self.handle, what, offset_bytes, out.ctypes.data, out.nbytes))
        return out

    def state(self) -> dict:
        """Extents of what state_read / i8_read can copy out (sqe_index_state)."""
        st = N.IndexState()
        N.check(self.lib.sqe_index_state(self.handle, st))
        return {name: getattr(st, name) for name, _ in N.IndexState._fields_}

    def state_read(self, what: int, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        """`count` elements of `dtype` from a scanned copy or a measured residual (sqe_index_state_read; what = STATE_*)."""
        out = np.empty(count, dtype)
        N.check(self.lib.sqe_index_state_read(self.handle, what, offset_bytes, out.ctypes.data, out.nbytes))
        return out

    def scan_bf16(self) -> np.ndarray:
        """The bf16 scanned copy, de-pitched: uint16 [round_up(len, 256), dim] by row position (rows past len are zero)."""
        st = self.state()
        rows = (st["rows"] + 255) // 256 * 256
        raw = self.state_read(STATE_SCAN_BF16, np.uint16, rows * st["scan_pitch"] // 2)
        return np.ascontiguousarray(raw.reshape(rows, st["scan_pitch"] // 2)[:, :st["dim"]])

    def search(self, q: np.ndarray, k: int, nprobe: int = 0, filter_ids=None) -> Tuple[np.ndarray, np.ndarray]:
        """-> (cos [B,k] float32, ids [B,k] int64), best first, ties to the lowest id,
        (-inf, -1) padded.  ``filter_ids`` (array of ids, possibly empty): the exact top-k over those
        live rows only (sqe_index_search_filtered; ids that name no live row are skipped, nprobe is unused)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        cos = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        if b and filter_ids is not None:
            allow = np.ascontiguousarray(filter_ids, dtype=np.int64).reshape(-1)
            N.check(self.lib.sqe_index_search_filtered(self.handle, q.ctypes.data, b, k, allow.ctypes.data,
                                                       allow.shape[0], cos.ctypes.data, ids.ctypes.data))
        elif b:
            N.check(self.lib.sqe_index_search(self.handle, q.ctypes.data, b, k, nprobe,
                                              cos.ctypes.data, ids.ctypes.data))
        return cos, ids

    def search_device(self, q_ptr: int, b: int, k: int, cos_ptr: int, id_ptr: int, nprobe: int = 0,
                      filter_ptr=None, n_filter: int = 0) -> None:
        """Asynchronous on the context stream; all pointers are device pointers.  With ``filter_ptr`` (int64
        [n_filter] ids on the device) the filtered search, which synchronises the context stream once: the
        number of allowed rows plans the scan."""
        if filter_ptr is not None:
            N.check(self.lib.sqe_index_search_filtered_device(self.handle, q_ptr, b, k, filter_ptr, n_filter,
                                                              cos_ptr, id_ptr))
        else:
            N.check(self.lib.sqe_index_search_device(self.handle, q_ptr, b, k, nprobe, cos_ptr, id_ptr))

    def search_filtered_each(self, q: np.ndarray, k: int, lists, list_of_query=None) -> Tuple[np.ndarray, np.ndarray]:
        """Every query over its own allow-list, in one call -> (cos [B,k] float32, ids [B,k] int64) as ``search`` returns
        them.  ``lists`` is a sequence of id arrays; query b is answered over ``lists[list_of_query[b]]`` (default
        ``arange(B)``, which needs ``len(lists) == B``).  Row b equals ``search(q[b:b+1], k, filter_ids=lists[...])``
        (sqe_index_search_filtered_each)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        allow, offsets, loq, n_lists = _pack_id_lists(lists, list_of_query, b, False)
        cos = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        if b:
            N.check(self.lib.sqe_index_search_filtered_each(self.handle, q.ctypes.data, b, k, allow.ctypes.data, offsets.ctypes.data,
                                                            n_lists, loq.ctypes.data, cos.ctypes.data, ids.ctypes.data))
        return cos, ids

    def search_filtered_each_device(self, q_ptr: int, b: int, k: int, allow_ptr, offsets, list_of_query, cos_ptr: int,
                                    id_ptr: int) -> None:
        """Device pointers for the queries, the ids of all lists and the results; ``offsets`` (int64 [n_lists + 1]) and
        ``list_of_query`` (int32 [b]) are host arrays, free to reuse once the call returns.  Enqueued on the context
        stream; lists on the direct route read nothing back and synchronise nothing themselves (include/sqe.h)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        loq = np.ascontiguousarray(list_of_query, dtype=np.int32).reshape(-1)
        N.check(self.lib.sqe_index_search_filtered_each_device(self.handle, q_ptr, b, k, allow_ptr, offsets.ctypes.data,
                                                               offsets.shape[0] - 1, loq.ctypes.data, cos_ptr, id_ptr))

    def search_excluding(self, q: np.ndarray, k: int, lists, list_of_query=None) -> Tuple[np.ndarray, np.ndarray]:
        """Every query over all live rows EXCEPT its own deny-list, in one call -> (cos [B,k] float32, ids [B,k] int64) as
        ``search`` returns them.  ``lists`` is a sequence of id arrays, a ``None`` entry meaning "no list"; query b is answered
        outside ``lists[list_of_query[b]]`` (default ``arange(B)``, which needs ``len(lists) == B``; an entry of -1 names no
        list).  Row b is the exact ranking of ``search`` without the listed ids, first k (sqe_index_search_excluding)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        deny, offsets, loq, n_lists = _pack_id_lists(lists, list_of_query, b, True)
        cos = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        if b:
            N.check(self.lib.sqe_index_search_excluding(self.handle, q.ctypes.data, b, k, deny.ctypes.data, offsets.ctypes.data,
                                                        n_lists, loq.ctypes.data, cos.ctypes.data, ids.ctypes.data))
        return cos, ids

    def search_excluding_device(self, q_ptr: int, b: int, k: int, deny_ptr, offsets, list_of_query, cos_ptr: int, id_ptr: int) -> None:
        """Device pointers for the queries, the ids of all deny-lists and the results; ``offsets`` (int64 [n_lists + 1]) and
        ``list_of_query`` (int32 [b], -1 = no list) are host arrays, free to reuse once the call returns.  Enqueued on the
        context stream; the call synchronises the stream once after its first stage and once per row range of the sweep
        (include/sqe.h)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        loq = np.ascontiguousarray(list_of_query, dtype=np.int32).reshape(-1)
        N.check(self.lib.sqe_index_search_excluding_device(self.handle, q_ptr, b, k, deny_ptr, offsets.ctypes.data,
                                                           offsets.shape[0] - 1, loq.ctypes.data, cos_ptr, id_ptr))

    def _row_set(self, pred, filter_ids, device_list=None):
        """The row-set arguments of every call that takes one (sqe_index_search_where's): clauses, n_clauses, set values, n_set,
        allow-list, n_allow, and the arrays that must stay alive through the call.  ``device_list`` = (pointer or None, count):
        the list of a ``_device`` call, already on the device."""
        clauses, _, sets = pack_predicates([[] if pred is None else pred])
        allow = None if filter_ids is None else np.ascontiguousarray(filter_ids, dtype=np.int64).reshape(-1)
        if device_list is not None:
            ptr, count = device_list[0], -1 if device_list[0] is None else device_list[1]
        else:
            ptr, count = (None, -1) if allow is None else (allow.ctypes.data, allow.shape[0])
        return (clauses.ctypes.data, clauses.shape[0], sets.ctypes.data, sets.shape[0], ptr, count), (clauses, sets, allow)

    def range_search(self, q: np.ndarray, min_cos, max_hits: int = 10, pred=None, filter_ids=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Radial search -> (counts [B] int64, cos [B,max_hits] float32, ids [B,max_hits] int64).  counts[b] is the
        exact number of live rows whose fp32 cosine is >= min_cos[b] (a scalar applies to every query); the rows hold
        the best min(count, max_hits) of them, best first, ties to the lowest id, (-inf, -1) padded
        (sqe_index_range_search).  With ``pred`` and / or ``filter_ids`` only the rows of that row set (``search_where``'s)
        count and are returned (sqe_index_range_search_where)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(min_cos, np.float32), (b,)))
        counts = np.zeros(b, np.int64)
        cos = np.empty((b, max_hits), np.float32)
        ids = np.empty((b, max_hits), np.int64)
        if b and pred is None and filter_ids is None:
            N.check(self.lib.sqe_index_range_search(self.handle, q.ctypes.data, b, t.ctypes.data, max_hits, counts.ctypes.data,
                                                    cos.ctypes.data if max_hits else None, ids.ctypes.data if max_hits else None))
        elif b:
            rows, _keep = self._row_set(pred, filter_ids)
            N.check(self.lib.sqe_index_range_search_where(self.handle, q.ctypes.data, b, t.ctypes.data, max_hits, *rows, counts.ctypes.data,
                                                          cos.ctypes.data if max_hits else None, ids.ctypes.data if max_hits else None))
        return counts, cos, ids

    def range_search_device(self, q_ptr: int, b: int, min_cos_ptr: int, max_hits: int, count_ptr: int, cos_ptr, id_ptr) -> None:
        """Device pointers throughout (float32 thresholds [b], int64 counts [b], [b, max_hits] results; the result
        pointers may be None when max_hits == 0).  Enqueued on the context stream; the call reads the thresholds back
        and synchronises the stream to plan its passes (include/sqe.h)."""
        N.check(self.lib.sqe_index_range_search_device(self.handle, q_ptr, b, min_cos_ptr, max_hits, count_ptr, cos_ptr, id_ptr))


    # -- group keys and collapsed search (include/sqe.h: sqe_index_search_collapsed)
    def set_keys(self, ids, keys) -> None:
        """Give the live rows ``ids`` the int64 group keys ``keys`` (KEY_NONE removes a key; a repeated id keeps its last
        key).  Every id must be live, else nothing is written.  Keys are not part of a saved index."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1)
        if ids.shape != keys.shape:
            raise ValueError(f"{ids.shape[0]} ids but {keys.shape[0]} keys")
        if ids.size:
            N.check(self.lib.sqe_index_set_keys(self.handle, ids.ctypes.data, keys.ctypes.data, ids.shape[0]))

    def get_keys(self, ids) -> np.ndarray:
        """Group keys of the live rows ``ids`` (int64; KEY_NONE where none is set)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        out = np.empty(ids.shape[0], np.int64)
        if ids.size:
            N.check(self.lib.sqe_index_get_keys(self.handle, ids.ctypes.data, ids.shape[0], out.ctypes.data))
        return out

    def search_collapsed(self, q: np.ndarray, k: int, pred=None, filter_ids=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> (cos [B,k] float32, ids [B,k] int64, keys [B,k] int64): the k best groups of the exact ranking and each
        group's best row, best first; a row without a key is a group by itself; (-inf, -1, KEY_NONE) padded.  With ``pred``
        and / or ``filter_ids`` the ranking walked is that of the rows of that row set (``search_where``'s) only
        (sqe_index_search_collapsed_where)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        cos = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        keys = np.empty((b, k), np.int64)
        if b and pred is None and filter_ids is None:
            N.check(self.lib.sqe_index_search_collapsed(self.handle, q.ctypes.data, b, k, cos.ctypes.data, ids.ctypes.data,
                                                        keys.ctypes.data))
        elif b:
            rows, _keep = self._row_set(pred, filter_ids)
            N.check(self.lib.sqe_index_search_collapsed_where(self.handle, q.ctypes.data, b, k, *rows, cos.ctypes.data, ids.ctypes.data,
                                                              keys.ctypes.data))
        return cos, ids, keys

    def search_collapsed_device(self, q_ptr: int, b: int, k: int, cos_ptr: int, id_ptr: int, key_ptr: int) -> None:
        """Device pointers throughout, enqueued on the context stream; the call synchronises the stream once after its
        first stage and once per row range of the sweep (include/sqe.h)."""
        N.check(self.lib.sqe_index_search_collapsed_device(self.handle, q_ptr, b, k, cos_ptr, id_ptr, key_ptr))

    # -- MMR search (include/sqe.h: sqe_index_search_mmr)
    # -- numeric fields and field predicates (include/sqe.h: sqe_index_set_field, sqe_index_search_where)
    def set_field(self, field: int, ids, values) -> None:
        """Give the live rows ``ids`` the int64 ``values`` in field slot ``field`` (0..7; FIELD_NONE removes a value; a repeated
        id keeps its last value).  Every id must be live, else nothing is written.  Fields are not part of a saved index."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        values = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
        if ids.shape != values.shape:
            raise ValueError(f"{ids.shape[0]} ids but {values.shape[0]} values")
        N.check(self.lib.sqe_index_set_field(self.handle, int(field), ids.ctypes.data, values.ctypes.data, ids.shape[0]))

    def get_field(self, field: int, ids) -> np.ndarray:
        """Values of the live rows ``ids`` in field slot ``field`` (int64; FIELD_NONE where none is set)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        out = np.empty(ids.shape[0], np.int64)
        N.check(self.lib.sqe_index_get_field(self.handle, int(field), ids.ctypes.data, ids.shape[0], out.ctypes.data))
        return out

    def field_info(self) -> dict:
        """-> {"fields": slots that hold a column, "device_bytes": bytes of all columns}; zeros before the first set_field."""
        nf = C.c_int32()
        nb = C.c_int64()
        N.check(self.lib.sqe_index_field_info(self.handle, C.byref(nf), C.byref(nb)))
        return {"fields": nf.value, "device_bytes": nb.value}

    def match_fields(self, preds, cap: int) -> Tuple[np.ndarray, np.ndarray]:
        """-> (counts [P] int64, ids [P, cap] int64): per predicate (``pack_predicates``) the exact number of live rows it
        selects and its ``cap`` lowest ids ascending, -1 padded (sqe_index_match_fields)."""
        clauses, offsets, sets = pack_predicates(preds)
        p = offsets.shape[0] - 1
        counts = np.zeros(p, np.int64)
        ids = np.full((p, cap), -1, np.int64)
        N.check(self.lib.sqe_index_match_fields(self.handle, clauses.ctypes.data, offsets.ctypes.data, p, sets.ctypes.data,
                                                sets.shape[0], cap, counts.ctypes.data, ids.ctypes.data if cap else None))
        return counts, ids

    def count_fields(self, preds) -> np.ndarray:
        """The exact number of live rows each predicate selects (match_fields with cap 0)."""
        return self.match_fields(preds, 0)[0]

    def aggregate_fields(self, pred, aggs, filter_ids=None, bucket_cap: Optional[int] = None) -> dict:
        """Aggregations (``pack_aggs``) over the live rows predicate ``pred`` selects, also restricted to ``filter_ids`` when
        given -- the row set of ``search_where`` -> {"selected": its size, "aggs": [per aggregation {"count", "min", "max",
        "sum" (exact, a Python int), "n_buckets", "other", "keys", "counts"}]}, keys / counts int64 arrays trimmed of padding
        (empty for stats).  ``bucket_cap`` (default: what the call's aggregations can return at most) bounds the buckets of a
        histogram (sqe_index_aggregate_fields)."""
        rows, _keep = self._row_set(pred, filter_ids)
        packed = pack_aggs(aggs)
        n = packed.shape[0]
        if bucket_cap is None:
            bucket_cap = AGG_MAX_BUCKETS if np.any(packed["kind"] == AGG_KINDS["histogram"]) else int(packed["size"].max())
        bucket_cap = int(bucket_cap)
        selected = C.c_int64(0)
        res = np.zeros(n, AGG_RESULT_DTYPE)
        keys = np.full((n, max(bucket_cap, 0)), FIELD_NONE, np.int64)
        counts = np.zeros((n, max(bucket_cap, 0)), np.int64)
        N.check(self.lib.sqe_index_aggregate_fields(self.handle, *rows, packed.ctypes.data, n, bucket_cap, C.byref(selected), res.ctypes.data,
                                                    keys.ctypes.data if bucket_cap > 0 else None,
                                                    counts.ctypes.data if bucket_cap > 0 else None))
        out = []
        for j in range(n):
            r = res[j]
            if packed["kind"][j] == AGG_KINDS["terms"]:
                m = min(int(r["n_buckets"]), int(packed["size"][j]))
            else:
                m = int(r["n_buckets"])
            out.append({"count": int(r["count"]), "min": int(r["min"]), "max": int(r["max"]),
                        "sum": (int(r["sum_hi"]) << 32) + int(r["sum_lo"]), "n_buckets": int(r["n_buckets"]), "other": int(r["other"]),
                        "keys": keys[j, :m].copy(), "counts": counts[j, :m].copy()})
        return {"selected": selected.value, "aggs": out}

    def aggregate_last(self) -> list:
        """Test-only: per aggregation of the last ``aggregate_fields`` call {"route" (AGG_ROUTE_*), "select_blocks", "span",
        "slots", "occupied_blocks"} (sqe_index_aggregate_last; single-device indexes only)."""
        L = N.AggLast()
        N.check(self.lib.sqe_index_aggregate_last(self.handle, L))
        return [{name: getattr(L.agg[j], name) for name, _ in N.AggRoute._fields_ if name != "pad"} for j in range(L.n_aggs)]

    def sort_fields(self, pred, sort, k: int, filter_ids=None, after=None) -> dict:
        """The first ``k`` (1..256) rows, in the order of the sort keys (``pack_sort``), of the live rows predicate ``pred``
        selects, also restricted to ``filter_ids`` when given -- the row set of ``search_where`` -> {"total": its size, "ids"
        int64 [m], "values" int64 [m, n_sort]: the rows' raw values in the sort slots, FIELD_NONE where missing}, trimmed of
        padding.  ``after`` = (values, id) is a search_after cursor: one value per key, None for missing, and an id; only rows
        strictly after it in the order come back (sqe_index_sort_fields)."""
        rows, _keep = self._row_set(pred, filter_ids)
        packed = pack_sort(sort)
        n, k = packed.shape[0], int(k)
        if not 1 <= k <= SORT_MAX_K:
            raise ValueError(f"k {k} is outside 1..{SORT_MAX_K}")
        cursor, after_id = None, 0
        if after is not None:
            values, after_id = after
            values = list(values)
            if len(values) != n:
                raise ValueError(f"the cursor holds {len(values)} values for {n} sort keys")
            cursor = np.array([FIELD_NONE if v is None else int(v) for v in values], np.int64)
        total = C.c_int64(0)
        ids = np.full(k, -1, np.int64)
        vals = np.full((k, n), FIELD_NONE, np.int64)
        N.check(self.lib.sqe_index_sort_fields(self.handle, *rows, packed.ctypes.data, n, k, None if cursor is None else cursor.ctypes.data,
                                               int(after_id), C.byref(total), ids.ctypes.data, vals.ctypes.data))
        m = int(np.count_nonzero(ids >= 0))
        return {"total": total.value, "ids": ids[:m].copy(), "values": vals[:m].copy()}

    def sort_last(self) -> dict:
        """Test-only: of the last ``sort_fields`` call {"slabs", "slabs_occupied", "merge_levels", "fan_in", "candidates"}
        (sqe_index_sort_last; single-device indexes only)."""
        L = N.SortLast()
        N.check(self.lib.sqe_index_sort_last(self.handle, L))
        return {name: getattr(L, name) for name, _ in N.SortLast._fields_}

    def where_last(self) -> dict:
        """Test-only: of the last ``search_where`` call {"route" (WHERE_ROUTE_*), "depth", "first_pass_i8", "selected", "live",
        "swept"} (sqe_index_where_last; single-device indexes only)."""
        L = N.WhereLast()
        N.check(self.lib.sqe_index_where_last(self.handle, L))
        return {name: getattr(L, name) for name, _ in N.WhereLast._fields_ if name != "pad"}

    def within_last(self) -> dict:
        """Test-only: of the last restricted ``range_search`` / ``search_collapsed`` / ``search_mmr`` call {"kind" (1 radial,
        2 collapsed, 3 MMR), "route" (WHERE_ROUTE_*), "depth", "selected", "live", "swept"} (sqe_index_within_last;
        single-device indexes only)."""
        L = N.WithinLast()
        N.check(self.lib.sqe_index_within_last(self.handle, L))
        return {name: getattr(L, name) for name, _ in N.WithinLast._fields_ if name != "pad"}

    def match_fields_device(self, preds, cap: int, count_ptr: int, id_ptr) -> None:
        """Device pointers for the counts [P] and ids [P, cap]; enqueued on the context stream, nothing synchronises."""
        clauses, offsets, sets = pack_predicates(preds)
        N.check(self.lib.sqe_index_match_fields_device(self.handle, clauses.ctypes.data, offsets.ctypes.data, offsets.shape[0] - 1,
                                                       sets.ctypes.data, sets.shape[0], cap, count_ptr, id_ptr))

    def search_where(self, q: np.ndarray, k: int, pred, filter_ids=None) -> Tuple[np.ndarray, np.ndarray]:
        """The exact top-k over the live rows predicate ``pred`` selects -> (cos [B,k], ids [B,k]) as ``search`` returns them;
        ``filter_ids`` also restricts the rows to that id list.  Equal to ``search(q, k, filter_ids=<the selected ids>)``
        without the ids ever being on the host (sqe_index_search_where)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        rows, _keep = self._row_set(pred, filter_ids)
        cos = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        if b:
            N.check(self.lib.sqe_index_search_where(self.handle, q.ctypes.data, b, k, *rows, cos.ctypes.data, ids.ctypes.data))
        return cos, ids

    def search_where_device(self, q_ptr: int, b: int, k: int, pred, cos_ptr: int, id_ptr: int, filter_ptr=None, n_filter: int = 0) -> None:
        """Device pointers for the queries, the results and the optional id list; enqueued on the context stream, which the
        call synchronises once (the number of selected rows plans the scan)."""
        rows, _keep = self._row_set(pred, None, device_list=(filter_ptr, n_filter))
        N.check(self.lib.sqe_index_search_where_device(self.handle, q_ptr, b, k, *rows, cos_ptr, id_ptr))

    def search_where_each(self, q: np.ndarray, k: int, preds, pred_of_query=None) -> Tuple[np.ndarray, np.ndarray]:
        """Query b over the rows of ``preds[pred_of_query[b]]`` (default ``arange(B)``, which needs one predicate per query),
        in one call.  Row b equals ``search_where(q[b:b+1], k, preds[...])`` (sqe_index_search_where_each)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        clauses, offsets, sets = pack_predicates(preds)
        p = offsets.shape[0] - 1
        if pred_of_query is None:
            if p != b:
                raise ValueError(f"{p} predicates for {b} queries: pass pred_of_query")
            poq = np.arange(b, dtype=np.int32)
        else:
            poq = np.ascontiguousarray(pred_of_query, dtype=np.int32).reshape(-1)
            if poq.shape[0] != b:
                raise ValueError(f"pred_of_query has {poq.shape[0]} entries for {b} queries")
        cos = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        if b:
            N.check(self.lib.sqe_index_search_where_each(self.handle, q.ctypes.data, b, k, clauses.ctypes.data, offsets.ctypes.data, p,
                                                         sets.ctypes.data, sets.shape[0], poq.ctypes.data, cos.ctypes.data, ids.ctypes.data))
        return cos, ids

    def search_where_each_device(self, q_ptr: int, b: int, k: int, preds, pred_of_query, cos_ptr: int, id_ptr: int) -> None:
        """Device pointers for the queries and the results; the predicates and ``pred_of_query`` (int32 [b]) are host data.
        Enqueued on the context stream, which the call synchronises once for the counts."""
        clauses, offsets, sets = pack_predicates(preds)
        poq = np.ascontiguousarray(pred_of_query, dtype=np.int32).reshape(-1)
        N.check(self.lib.sqe_index_search_where_each_device(self.handle, q_ptr, b, k, clauses.ctypes.data, offsets.ctypes.data,
                                                            offsets.shape[0] - 1, sets.ctypes.data, sets.shape[0], poq.ctypes.data,
                                                            cos_ptr, id_ptr))

    def _mmr_lambda(self, lam, b: int) -> np.ndarray:
        lam = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, np.float32), (b,)))
        if b and not bool(np.all((lam >= 0) & (lam <= 1))):
            raise ValueError("lam must be in [0, 1]")
        return lam

    def search_mmr(self, q: np.ndarray, k: int, lam=0.5, n_cand: int = 0, nprobe: int = 0, pred=None,
                   filter_ids=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Maximal marginal relevance -> (cos [B,k] float32, ids [B,k] int64, mmr [B,k] float32) in selection order: the
        greedy choice of k rows among the exact top-``n_cand`` (0 = automatic, min(256, max(32, 4 k))) that maximises
        ``lam * cos - (1 - lam) * max similarity to the rows already chosen``; ``lam`` is a scalar or one value per query,
        1 = the plain top-k.  cos is the cosine ``search`` returns for the row, mmr the objective at the step that chose it;
        (-inf, -1, -inf) padded.  With ``pred`` and / or ``filter_ids`` the candidates are the exact top-``n_cand`` of that row
        set, ``search_where`` at that depth (sqe_index_search_mmr_where; ``nprobe`` is then not used)."""
        q = _queries(q, self.dim)
        b = q.shape[0]
        lam = self._mmr_lambda(lam, b)
        cos = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        mmr = np.empty((b, k), np.float32)
        if b and pred is None and filter_ids is None:
            N.check(self.lib.sqe_index_search_mmr(self.handle, q.ctypes.data, b, k, n_cand, lam.ctypes.data, nprobe,
                                                  cos.ctypes.data, ids.ctypes.data, mmr.ctypes.data))
        elif b:
            rows, _keep = self._row_set(pred, filter_ids)
            N.check(self.lib.sqe_index_search_mmr_where(self.handle, q.ctypes.data, b, k, n_cand, lam.ctypes.data, nprobe, *rows,
                                                        cos.ctypes.data, ids.ctypes.data, mmr.ctypes.data))
        return cos, ids, mmr

    def search_mmr_device(self, q_ptr: int, b: int, k: int, cos_ptr: int, id_ptr: int, mmr_ptr: int, lam=0.5, n_cand: int = 0,
                          nprobe: int = 0) -> None:
        """Device pointers for the queries and the three [b, k] outputs; ``lam`` (scalar or [b]) stays on the host.
        Enqueued on the context stream; nothing is read back and the stream is not synchronised."""
        lam = self._mmr_lambda(lam, b)
        self._mmr_lam = lam             # the copy of the weights is staged during the call; keep them until the next one anyway
        if b:
            N.check(self.lib.sqe_index_search_mmr_device(self.handle, q_ptr, b, k, n_cand, lam.ctypes.data, nprobe, cos_ptr, id_ptr,
                                                         mmr_ptr))

    # -- fused multi-query search (include/sqe.h: sqe_index_search_fused)
    def _fused_args(self, b: int, offsets, mode: str, weights):
        if mode not in FUSE_MODES:
            raise ValueError(f"mode must be 'rrf' or 'max', got {mode!r}")
        if offsets is None:
            offsets = np.array([0, b], np.int64)
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
            if offsets.shape[0] < 1 or int(offsets[-1]) != b:
                raise ValueError(f"offsets must hold G + 1 entries and end at the {b} rows of q")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            if weights.shape[0] != b:
                raise ValueError(f"{weights.shape[0]} weights for {b} sub-queries")
        return offsets, weights

    def search_fused(self, q: np.ndarray, k: int, offsets=None, mode: str = "rrf", weights=None, depth: int = 0, rank_constant: int = 60,
                     nprobe: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Several vectors for one question, one ranked list back -> (fused [G,k] float32, ids [G,k] int64, cos [G,k]
        float32).  Logical query g owns the rows ``q[offsets[g]:offsets[g+1]]`` (``offsets=None``: one group of all rows of
        ``q``), at most 32 of them.  Each sub-query's list is ``search(q_j, depth)`` (``depth`` 0 = automatic: k for "max",
        min(256, max(32, 4 k)) for "rrf"; sub-queries x depth <= 2048).  ``mode="rrf"``: reciprocal rank fusion, the sum of
        ``weights[j] / (rank_constant + rank)`` over the lists that hold the row, in exact integer arithmetic; ``mode="max"``:
        the row's best cosine (``weights`` must be None).  Ranked by the fused score, ties to the lowest id; cos is the row's
        best cosine as ``search`` returned it; (-inf, -1, -inf) padded."""
        q = _queries(q, self.dim, "sub-queries")
        offsets, weights = self._fused_args(q.shape[0], offsets, mode, weights)
        g = offsets.shape[0] - 1
        fused = np.empty((g, k), np.float32)
        ids = np.empty((g, k), np.int64)
        cos = np.empty((g, k), np.float32)
        if g:
            N.check(self.lib.sqe_index_search_fused(self.handle, q.ctypes.data, g, offsets.ctypes.data, k, depth, FUSE_MODES[mode],
                                                    rank_constant, None if weights is None else weights.ctypes.data, nprobe,
                                                    fused.ctypes.data, ids.ctypes.data, cos.ctypes.data))
        return fused, ids, cos

    def search_fused_device(self, q_ptr: int, bs: int, k: int, fused_ptr: int, id_ptr: int, cos_ptr: int, offsets=None, mode: str = "rrf",
                            weights=None, depth: int = 0, rank_constant: int = 60, nprobe: int = 0) -> None:
        """Device pointers for the ``bs`` sub-queries and the three [G, k] outputs; ``offsets`` and ``weights`` stay on the
        host, free to reuse once the call returns.  Enqueued on the context stream; nothing is read back and the stream is
        not synchronised."""
        offsets, weights = self._fused_args(bs, offsets, mode, weights)
        g = offsets.shape[0] - 1
        if g:
            N.check(self.lib.sqe_index_search_fused_device(self.handle, q_ptr, g, offsets.ctypes.data, k, depth, FUSE_MODES[mode],
                                                           rank_constant, None if weights is None else weights.ctypes.data, nprobe,
                                                           fused_ptr, id_ptr, cos_ptr))

    # -- hybrid search (include/sqe.h: sqe_index_search_hybrid)
    def _hybrid_args(self, b: int, q_terms, offsets, weights):
        qoff, qterms = _bags(q_terms)
        g = qoff.shape[0] - 1
        if offsets is None:
            if g != 1:
                raise ValueError("offsets=None means one group: pass one lexical query")
            offsets = np.array([0, b], np.int64)
        else:
            offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
            if offsets.shape[0] != g + 1 or int(offsets[-1]) != b:
                raise ValueError(f"offsets must hold {g + 1} entries, one group per lexical query, and end at the {b} rows of q")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            if weights.shape[0] != b + g:
                raise ValueError(f"{weights.shape[0]} weights for {b} sub-queries and {g} lexical lists")
        return qoff, qterms, offsets, weights

    def search_hybrid(self, lex: "LexicalIndex", q: np.ndarray, q_terms, k: int, offsets=None, weights=None, depth: int = 0,
                      rank_constant: int = 60, nprobe: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Reciprocal rank fusion of vector lists and one BM25 list per group -> (fused [G,k], ids [G,k], cos [G,k], bm25
        [G,k]).  Group g owns the rows ``q[offsets[g]:offsets[g+1]]`` (at most 31; none is fine) and the lexical query
        ``q_terms[g]`` (may be empty: no list).  ``weights``: the sub-queries' first, then one per group for its lexical list.
        cos is -inf for a row no vector list holds, bm25 -inf for a row the lexical list does not hold."""
        q = _f32(q).reshape(-1, self.dim)
        qoff, qterms, offsets, weights = self._hybrid_args(q.shape[0], q_terms, offsets, weights)
        g = offsets.shape[0] - 1
        fused = np.empty((g, k), np.float32)
        ids = np.empty((g, k), np.int64)
        cos = np.empty((g, k), np.float32)
        bm25 = np.empty((g, k), np.float32)
        if g:
            N.check(self.lib.sqe_index_search_hybrid(self.handle, lex.handle, q.ctypes.data, g, offsets.ctypes.data, qoff.ctypes.data,
                                                     qterms.ctypes.data, k, depth, rank_constant,
                                                     None if weights is None else weights.ctypes.data, nprobe, fused.ctypes.data,
                                                     ids.ctypes.data, cos.ctypes.data, bm25.ctypes.data))
        return fused, ids, cos, bm25

    def search_hybrid_device(self, lex: "LexicalIndex", q_ptr: int, bs: int, q_terms, k: int, fused_ptr: int, id_ptr: int, cos_ptr: int,
                             bm25_ptr: int, offsets=None, weights=None, depth: int = 0, rank_constant: int = 60, nprobe: int = 0) -> None:
        """Device pointers for the ``bs`` sub-queries and the four [G, k] outputs; everything else stays on the host."""
        qoff, qterms, offsets, weights = self._hybrid_args(bs, q_terms, offsets, weights)
        g = offsets.shape[0] - 1
        if g:
            N.check(self.lib.sqe_index_search_hybrid_device(self.handle, lex.handle, q_ptr, g, offsets.ctypes.data, qoff.ctypes.data,
                                                            qterms.ctypes.data, k, depth, rank_constant,
                                                            None if weights is None else weights.ctypes.data, nprobe, fused_ptr, id_ptr,
                                                            cos_ptr, bm25_ptr))


def _bags(bags) -> Tuple[np.ndarray, np.ndarray]:
    """A list of term-id sequences (or one flat pair already) -> (offsets [n + 1] int64, terms int32)."""
    if isinstance(bags, tuple) and len(bags) == 2:
        return (np.ascontiguousarray(bags[0], dtype=np.int64).reshape(-1), np.ascontiguousarray(bags[1], dtype=np.int32).reshape(-1))
    lens = [len(b) for b in bags]
    offsets = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    terms = np.concatenate([np.asarray(b, dtype=np.int32).reshape(-1) for b in bags]) if lens and offsets[-1] else np.zeros(0, np.int32)
    return offsets, np.ascontiguousarray(terms, dtype=np.int32)


LEX_SHOULD, LEX_MUST, LEX_FILTER, LEX_MUST_NOT = 0, 1, 2, 3      # roles of a term occurrence (include/sqe.h: SQE_LEX_SHOULD ..)


class LexicalIndex:
    """BM25 index over bags of term ids, held in HBM as a chunked inverted index of integer impacts (include/sqe.h:
    sqe_lex_*).  Documents are (int64 id, term ids); the analyzer that makes the term ids is the caller's."""

    def __init__(self, ctx: Context, n_terms: int, k1: float = 1.2, b: float = 0.75):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_terms = n_terms
        h = C.c_void_p()
        N.check(self.lib.sqe_lex_create(ctx.handle, n_terms, float(k1), float(b), C.byref(h)))
        self.handle = h
        ctx._children.add(self)

    def close(self) -> None:
        if getattr(self, "handle", None):
            if self.ctx.handle:
                self.lib.sqe_lex_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = C.c_int64()
        N.check(self.lib.sqe_lex_count(self.handle, C.byref(n)))
        return int(n.value)

    def count(self, queries=None, roles=None, min_should=None):
        """Without arguments the live documents; with boolean queries the number of matches of each (``match`` with ``cap`` 0)."""
        if queries is None:
            return len(self)
        return self.match(queries, roles, min_should, cap=0)[0]

    def put(self, ids, bags, ordered: bool = False) -> None:
        """Add or replace documents: ``bags`` is a list of term-id sequences (or an (offsets, terms) pair), one per id.  The
        ids of a call are distinct; a live id has its bag replaced; an empty bag is a document that never scores.
        ``ordered``: the terms of a document are kept as its sequence too (sqe_lex_put_ordered), which phrase clauses need;
        without it a document holds no phrase of two or more terms."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        offsets, terms = _bags(bags)
        if offsets.shape[0] != ids.shape[0] + 1:
            raise ValueError(f"{offsets.shape[0] - 1} bags for {ids.shape[0]} ids")
        if ids.size:
            put = self.lib.sqe_lex_put_ordered if ordered else self.lib.sqe_lex_put
            N.check(put(self.handle, ids.ctypes.data, offsets.ctypes.data, terms.ctypes.data, ids.shape[0]))

    def delete(self, ids) -> None:
        """Remove the documents with these ids; unknown ids are skipped."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if ids.size:
            N.check(self.lib.sqe_lex_delete(self.handle, ids.ctypes.data, ids.shape[0]))

    # The query tables of a call are a tuple of arrays (None: a null pointer) in the order of the C signature; _bool_args and
    # _phrase_args build them, _topk_host and _match_host are the host forms over any of the three query kinds.
    @staticmethod
    def _ptrs(tables):
        return tuple(None if a is None else a.ctypes.data for a in tables)

    @staticmethod
    def _min_should(min_should, b: int):
        if min_should is None:
            return None
        min_should = np.ascontiguousarray(min_should, dtype=np.int32).reshape(-1)
        if min_should.shape[0] != b:
            raise ValueError(f"{min_should.shape[0]} min_should values for {b} queries")
        return min_should

    def _topk_host(self, fn, tables, b: int, k: int) -> Tuple[np.ndarray, np.ndarray]:
        score = np.empty((b, k), np.float32)
        ids = np.empty((b, k), np.int64)
        N.check(fn(self.handle, *self._ptrs(tables), b, k, score.ctypes.data, ids.ctypes.data))
        return score, ids

    def _match_host(self, fn, tables, b: int, cap: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
        """``cap`` None: one counting call first, then the largest count of the batch."""
        args = (self.handle, *self._ptrs(tables), b)
        counts = np.zeros(b, np.int64)
        counted = cap is None
        if counted:
            N.check(fn(*args, 0, counts.ctypes.data, None))
            cap = int(counts.max()) if b else 0
        ids = np.empty((b, cap), np.int64)
        if cap or not counted:
            N.check(fn(*args, cap, counts.ctypes.data, ids.ctypes.data if cap else None))
        return counts, ids

    def search(self, queries, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """``queries``: a list of term-id sequences (at most 64 occurrences each; a repeated term counts each time) ->
        (scores [B,k] float32, ids [B,k] int64), best first, ties to the lowest id, (-inf, -1) padded."""
        tables = _bags(queries)
        return self._topk_host(self.lib.sqe_lex_search, tables, tables[0].shape[0] - 1, k)

    def search_device(self, queries, k: int, score_ptr: int, id_ptr: int) -> None:
        """The queries stay on the host; device pointers for the two [B, k] outputs.  Enqueued on the context stream; a search
        that finds the index unchanged reads nothing back and does not synchronise."""
        offsets, terms = _bags(queries)
        N.check(self.lib.sqe_lex_search_device(self.handle, offsets.ctypes.data, terms.ctypes.data, offsets.shape[0] - 1, k, score_ptr, id_ptr))

    def _bool_args(self, queries, roles, min_should):
        offsets, terms = _bags(queries)
        _, r = _bags(roles)
        r = np.ascontiguousarray(r, dtype=np.uint8)
        if r.shape[0] != terms.shape[0]:
            raise ValueError(f"{r.shape[0]} roles for {terms.shape[0]} term occurrences")
        b = offsets.shape[0] - 1
        return (offsets, terms, r, self._min_should(min_should, b)), b

    def search_bool(self, queries, roles, k: int, min_should=None) -> Tuple[np.ndarray, np.ndarray]:
        """Boolean queries (include/sqe.h: sqe_lex_search_bool): ``roles`` is shaped as ``queries``, one of LEX_SHOULD, LEX_MUST,
        LEX_FILTER, LEX_MUST_NOT per term occurrence; ``min_should`` one int per query (None: zeros).  -> the k best matches as
        ``search`` returns them; a match that only FILTER occurrences made scores 0.0 and ranks last."""
        tables, b = self._bool_args(queries, roles, min_should)
        return self._topk_host(self.lib.sqe_lex_search_bool, tables, b, k)

    def match(self, queries, roles, min_should=None, cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The match SET of each query (sqe_lex_match) -> (counts [B] int64, exact whatever ``cap`` is; ids [B, cap] int64: the
        lowest matching ids ascending, -1 padded).  ``cap`` None: the largest count of the batch (one counting call first)."""
        tables, b = self._bool_args(queries, roles, min_should)
        return self._match_host(self.lib.sqe_lex_match, tables, b, cap)

    def match_device(self, queries, roles, min_should, cap: int, count_ptr: int, id_ptr: int) -> None:
        """``match`` with device pointers for counts [B] and ids [B, cap]; enqueued on the context stream."""
        tables, b = self._bool_args(queries, roles, min_should)
        N.check(self.lib.sqe_lex_match_device(self.handle, *self._ptrs(tables), b, cap, count_ptr, id_ptr))

    def search_bool_device(self, queries, roles, k: int, score_ptr: int, id_ptr: int, min_should=None) -> None:
        """``search_bool`` with device pointers for the two [B, k] outputs; enqueued on the context stream."""
        tables, b = self._bool_args(queries, roles, min_should)
        N.check(self.lib.sqe_lex_search_bool_device(self.handle, *self._ptrs(tables), b, k, score_ptr, id_ptr))

    def _phrase_args(self, queries, roles, min_should):
        """``queries``: per query a list of clauses, each a sequence of term ids; ``roles``: per query one role per clause."""
        queries = [list(q) for q in queries]
        qoff = np.zeros(len(queries) + 1, np.int64)
        np.cumsum([len(q) for q in queries], out=qoff[1:])
        coff, terms = _bags([c for q in queries for c in q])
        _, r = _bags(roles)
        r = np.ascontiguousarray(r, dtype=np.uint8)
        if r.shape[0] != coff.shape[0] - 1:
            raise ValueError(f"{r.shape[0]} roles for {coff.shape[0] - 1} clauses")
        b = len(queries)
        return (qoff, coff, terms, r, self._min_should(min_should, b)), b

    def search_phrase(self, queries, roles, k: int, min_should=None) -> Tuple[np.ndarray, np.ndarray]:
        """Clause queries (include/sqe.h: sqe_lex_search_phrase): a query is a list of clauses, a clause a sequence of term
        ids that must occur next to each other in this order (one term: a plain occurrence); ``roles`` holds one role per
        clause.  -> the k best matches as ``search_bool`` returns them."""
        tables, b = self._phrase_args(queries, roles, min_should)
        return self._topk_host(self.lib.sqe_lex_search_phrase, tables, b, k)

    def search_phrase_device(self, queries, roles, k: int, score_ptr: int, id_ptr: int, min_should=None) -> None:
        """``search_phrase`` with device pointers for the two [B, k] outputs; enqueued on the context stream."""
        tables, b = self._phrase_args(queries, roles, min_should)
        N.check(self.lib.sqe_lex_search_phrase_device(self.handle, *self._ptrs(tables), b, k, score_ptr, id_ptr))

    def match_phrase(self, queries, roles, min_should=None, cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The match SET of each clause query (sqe_lex_match_phrase), as ``match`` returns it."""
        tables, b = self._phrase_args(queries, roles, min_should)
        return self._match_host(self.lib.sqe_lex_match_phrase, tables, b, cap)

    def match_phrase_device(self, queries, roles, min_should, cap: int, count_ptr: int, id_ptr: int) -> None:
        """``match_phrase`` with device pointers for counts [B] and ids [B, cap]; enqueued on the context stream."""
        tables, b = self._phrase_args(queries, roles, min_should)
        N.check(self.lib.sqe_lex_match_phrase_device(self.handle, *self._ptrs(tables), b, cap, count_ptr, id_ptr))

    def count_phrase(self, queries, roles, min_should=None) -> np.ndarray:
        """The number of matches of each clause query (``match_phrase`` with ``cap`` 0)."""
        return self.match_phrase(queries, roles, min_should, cap=0)[0]

    def info(self) -> dict:
        st = N.LexInfo()
        N.check(self.lib.sqe_lex_info(self.handle, C.byref(st)))
        return {f: getattr(st, f) for f, _ in N.LexInfo._fields_}

    def state_read(self, what: int, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        """``count`` elements of ``dtype`` of one buffer of the device index as the last rebuild left it (sqe_lex_state_read;
        test-only introspection)."""
        out = np.empty(count, dtype)
        N.check(self.lib.sqe_lex_state_read(self.handle, what, offset_bytes, out.ctypes.data, out.nbytes))
        return out


class CacheMatrix:
    """Resident cache matrix for the lfu_cache_get scan (main.py:73-87): slots hold raw
    embeddings; ``best(order, q)`` returns (sim, list position) of the first strict max."""

    def __init__(self, ctx: Context, capacity: int, dim: int = 1024):
        self.ctx = ctx
        self.lib = ctx.lib
        self.capacity, self.dim = capacity, dim
        h = C.c_void_p()
        N.check(self.lib.sqe_cache_create(ctx.handle, capacity, dim, C.byref(h)))
        self.handle = h
        self._lock = threading.Lock()
        ctx._children.add(self)

    def close(self) -> None:
        if getattr(self, "handle", None):
            if self.ctx.handle:
                self.lib.sqe_cache_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_slot(self, slot: int, vec: np.ndarray) -> None:
        vec = _f32(vec).reshape(-1)
        if vec.shape[0] != self.dim:            # the C side reads dim floats: never hand it a shorter buffer
            raise ValueError(f"cache embedding has {vec.shape[0]} values, the cache matrix holds {self.dim}-d rows")
        N.check(self.lib.sqe_cache_set_slot(self.handle, slot, vec.ctypes.data))

    def best(self, order, q: np.ndarray) -> Tuple[float, int]:
        order = np.ascontiguousarray(order, dtype=np.int32)
        q = _f32(q).reshape(-1)
        if q.shape[0] != self.dim:
            raise ValueError(f"query embedding has {q.shape[0]} values, the cache matrix holds {self.dim}-d rows")
        sim = C.c_float()
        pos = C.c_int32()
        N.check(self.lib.sqe_cache_best(self.handle, order.ctypes.data, order.shape[0], q.ctypes.data,
                                        C.byref(sim), C.byref(pos)))
        return float(sim.value), int(pos.value)
