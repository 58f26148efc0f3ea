"""NumPy stand-ins for the index behind the driver interface of tests/session_cases.py (DRIVER_METHODS).

``FakeIndex`` keeps what the library keeps behind its handle, in the same shape: rows, keys and field columns BY POSITION in
arrays of a capacity that only grows, a position -> id map that appears at the first delete, a delete that compacts the live
rows to the front and leaves the tail as it was, a second copy of the rows that the plain search takes its candidates from
before it scores them from the master (as the library's first pass reads the bf16 / int8 copy), one allow bitmap
that every row-set call reuses, and a scratch sub-index (rows and keys) that the gather route fills.  Faithful, it answers
every call as the model does.  With one of ``FAULTS`` it makes exactly one mistake of the kind such state invites; the checker
must see each (tests/test_session_cpu.py).  The faults live here only."""
import numpy as np

from oracle import retrieval as R
from tests import agg_reference, sort_reference
from tests.fields_reference import NONE, FieldModel, clause_holds, split_clause
from tests.fuse_reference import fuse_groups
from tests.mmr_reference import greedy
from tests.session_model import KEYS

FAULTS = (
    "keys_stay",                  # the key column does not follow the rows through a delete
    "field_tail",                 # a row added after set_field reads the value the previous occupant of its position left
    "bits_beyond_n",              # only the map words that hold live positions are cleared: words beyond a shrunken n survive
    "gather_leftover",            # rows of a larger earlier gather still count in a radial search over the sub-index
    "update_one_route",           # the copy the plain search takes its candidates from keeps the old vector of an updated row
    "deleted_resolves",           # a deleted id on a list resolves to the row that took its place in the id order
    "no_id_after_map",            # rows added once the id map exists get no entry in it
    "collapsed_inherits_keys",    # a collapsed search on the gather route reuses the keys the previous call gathered
)


def _round_up(a, b):
    return (a + b - 1) // b * b


class FakeIndex:
    def __init__(self, dim, fault=None):
        assert fault is None or fault in FAULTS
        self.dim, self.fault = dim, fault
        self.cap = self.n = self.next_id = 0
        self.X = np.zeros((0, dim), np.float32)            # the master rows
        self.X2 = np.zeros((0, dim), np.float32)           # the copy the plain search scans
        self.idmap = np.zeros(0, np.int64)
        self.has_map = False
        self.keys = None
        self.fields = {}
        self.bits = np.zeros(0, bool)
        self.sub_X = np.zeros((0, dim), np.float32)
        self.sub_n = 0
        self.sub_keys = None
        self.opts = {"filter_gather_rows": 1 << 40, "where_route": 0}
        self.version = 0                                   # counts the mutations: what the cached scores depend on
        self._cache = {}

    # ------------------------------------------------------------ storage
    def _grow(self, need):
        if need <= self.cap:
            return
        cap = _round_up(max(need, self.cap + self.cap // 2, 1024), 256)
        n = self.n

        def grown(old, fill, shape=()):
            new = np.full((cap,) + shape, fill, old.dtype)
            new[:n] = old[:n]
            return new
        self.X, self.X2 = grown(self.X, 0, (self.dim,)), grown(self.X2, 0, (self.dim,))
        self.idmap = grown(self.idmap, -7)
        if self.keys is not None:
            self.keys = grown(self.keys, NONE)
        self.fields = {f: grown(c, NONE) for f, c in self.fields.items()}
        bits = np.zeros(cap, bool)
        bits[:self.bits.size] = self.bits
        self.bits = bits
        self.cap = cap

    def __len__(self):
        return self.n

    def set_option(self, key, value):
        self.opts[key] = int(value)

    def ids(self):
        return self.idmap[:self.n].copy() if self.has_map else np.arange(self.n, dtype=np.int64)

    def _ids_of(self, pos):
        pos = np.asarray(pos, np.int64)
        if not self.has_map:
            return pos.copy()
        return np.where(pos >= 0, self.idmap[np.maximum(pos, 0)], -1)

    def _resolve(self, ids, strict=False):
        """positions of ids, -1 where an id names no live row"""
        ids = np.asarray(ids, np.int64).reshape(-1)
        n = self.n
        if not self.has_map:
            pos = np.where((ids >= 0) & (ids < n), ids, -1)
        else:
            p = np.searchsorted(self.idmap[:n], ids)
            hit = (p < n) & (self.idmap[np.minimum(p, max(n - 1, 0))] == ids) if n else np.zeros(ids.size, bool)
            if self.fault == "deleted_resolves" and not strict:
                # the lookup forgets to compare: an id between two live ones lands on the row that follows it
                hit |= (p > 0) & (p < n)
            pos = np.where(hit, p, -1)
        if strict and np.any(pos < 0):
            raise KeyError("an id is not live")
        return pos

    # ------------------------------------------------------------ mutations
    def add(self, x):
        x = np.asarray(x, np.float32).reshape(-1, self.dim)
        m = x.shape[0]
        if m == 0:
            return
        self._grow(self.n + m)
        pos = slice(self.n, self.n + m)
        self.X[pos] = self.X2[pos] = R.normalize_rows(x)
        if self.has_map and self.fault != "no_id_after_map":
            self.idmap[pos] = np.arange(self.next_id, self.next_id + m)
        if self.keys is not None:
            self.keys[pos] = NONE
        if self.fault != "field_tail":
            for col in self.fields.values():
                col[pos] = NONE
        self.n += m
        self.next_id += m
        self.version += 1

    def update(self, ids, x):
        pos = self._resolve(ids, True)
        xn = R.normalize_rows(np.asarray(x, np.float32).reshape(-1, self.dim))
        self.X[pos] = xn
        if self.fault != "update_one_route":
            self.X2[pos] = xn
        self.version += 1

    def delete(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        if ids.size == 0:
            return
        pos = self._resolve(ids, True)
        n = self.n
        if not self.has_map:
            self.idmap[:n] = np.arange(n)
            self.has_map = True
        keep = np.ones(n, bool)
        keep[pos] = False
        m = int(keep.sum())
        cols = [self.X, self.X2, self.idmap] + list(self.fields.values())
        if self.keys is not None and self.fault != "keys_stay":
            cols.append(self.keys)
        for a in cols:                                     # the live rows move to the front; the tail stays as it was
            a[:m] = a[:n][keep]
        self.n = m
        self.version += 1

    def _column(self, which):
        if which == KEYS:
            if self.keys is None:
                self.keys = np.full(self.cap, NONE, np.int64)
            return self.keys
        return self.fields.setdefault(which, np.full(self.cap, NONE, np.int64))

    def set_keys(self, ids, keys):
        self._set(KEYS, ids, keys)

    def set_field(self, slot, ids, values):
        self._set(int(slot), ids, values)

    def _set(self, which, ids, values):
        ids = np.asarray(ids, np.int64).reshape(-1)
        if ids.size == 0:
            return
        pos = self._resolve(ids, True)
        col = self._column(which)
        for p, v in zip(pos, np.asarray(values, np.int64).reshape(-1)):
            col[p] = v

    # ------------------------------------------------------------ read-backs
    def get_rows(self, ids):
        return self.X[self._resolve(ids, True)].copy()

    def get_keys(self, ids):
        pos = self._resolve(ids, True)
        return np.full(pos.size, NONE, np.int64) if self.keys is None else self.keys[pos].copy()

    def get_field(self, slot, ids):
        pos = self._resolve(ids, True)
        return self.fields[slot][pos].copy() if slot in self.fields else np.full(pos.size, NONE, np.int64)

    # ------------------------------------------------------------ row sets
    def _mask(self, pred):
        m = np.ones(self.n, bool)
        for cl in pred or []:
            field, op, args, not_ = split_clause(cl)
            col = self.fields[field][:self.n] if field in self.fields else np.full(self.n, NONE, np.int64)
            m &= clause_holds(col, op, args, not_)
        return m

    def _rowset(self, pred, filter_ids):
        """ascending positions of the row set, through the one bitmap every such call reuses"""
        n = self.n
        self.bits[:_round_up(n, 32) if self.fault == "bits_beyond_n" else self.bits.size] = False
        if filter_ids is not None:
            pos = self._resolve(filter_ids)
            self.bits[pos[pos >= 0]] = True
            if pred:
                self.bits[:n] &= self._mask(pred)
        else:
            self.bits[:n] = self._mask(pred)
        return np.flatnonzero(self.bits)

    def _gather(self, pos):
        """the rows at pos into the sub-index, which then holds exactly them -> how many it held before"""
        m = pos.size
        if self.sub_X.shape[0] < m:
            self.sub_X = np.zeros((_round_up(max(m, 1024), 256), self.dim), np.float32)
            self.sub_n = 0
        before = self.sub_n
        self.sub_X[:m] = self.X[pos]
        self.sub_n = m
        return before

    def _gather_chunks(self, pos):
        g = self.opts["filter_gather_rows"]
        for c0 in range(0, pos.size, g):
            self._gather(pos[c0:c0 + g])

    # ------------------------------------------------------------ scoring
    def _scores(self, q, X=None):
        """float32 [cap, B]: the cosine of every stored row (live or not) and every query, from float64 dot products"""
        X = self.X if X is None else X
        q = np.ascontiguousarray(q, np.float32)
        which = X is self.X2
        key = (q.tobytes(), self.version)
        if self._cache.get(which, (None, None))[0] != key:
            qn = R.normalize_rows(q).astype(np.float64).T
            S = np.empty((X.shape[0], q.shape[0]), np.float32)
            for r0 in range(0, X.shape[0], 8192):
                S[r0:r0 + 8192] = X[r0:r0 + 8192].astype(np.float64) @ qn
            self._cache[which] = (key, S)
        return self._cache[which][1]

    def _first_pass(self, q, depth):
        """What the plain search does before it scores: per query the positions of the max(64, 4 depth) best rows BY THE SCANNED
        COPY, ascending.  The caller scores them from the master, as the library re-scores its candidates in fp32: a copy
        that is stale for a row costs a candidate when the row's old vector ranked high, and misses the row when its new one does."""
        S2 = self._scores(q, self.X2)
        everything = np.arange(self.n, dtype=np.int64)
        return [np.sort(self._rank(everything, S2[:, b], max(64, 4 * depth))[0]) for b in range(S2.shape[1])]

    @staticmethod
    def _qn(q):
        return R.normalize_rows(np.asarray(q, np.float32)).astype(np.float64)

    @staticmethod
    def _rank(pos, s_all, depth=None):
        """-> (positions, float32 cosines) of the rows at pos for one query, best first, ties to the lowest position"""
        s = s_all[pos]
        if depth is not None and 0 < depth < pos.size:
            kth = np.partition(s, pos.size - depth)[pos.size - depth]
            near = np.flatnonzero(s >= kth)
            pos, s = pos[near], s[near]
        order = np.lexsort((pos, -s.astype(np.float64)))
        if depth is not None:
            order = order[:depth]
        return pos[order], s[order]

    def _topk(self, sets, q, k, X=None):
        S = self._scores(q, X)
        cos = np.full((S.shape[1], k), -np.inf, np.float32)
        ids = np.full((S.shape[1], k), -1, np.int64)
        for b in range(S.shape[1]):
            p, s = self._rank(sets(b), S[:, b], k)
            cos[b, :p.size], ids[b, :p.size] = s, self._ids_of(p)
        return cos, ids

    # ------------------------------------------------------------ the query kinds
    def search(self, q, k, nprobe=0, filter_ids=None):
        if filter_ids is None:
            cand = self._first_pass(q, k)
            return self._topk(lambda b: cand[b], q, k)
        pos = self._rowset([], filter_ids)
        self._gather_chunks(pos)
        return self._topk(lambda b: pos, q, k)

    def search_filtered_each(self, q, k, lists, list_of_query=None):
        loq = np.arange(len(lists)) if list_of_query is None else list_of_query
        sets = [np.unique(p[p >= 0]) for p in (self._resolve(l) for l in lists)]
        return self._topk(lambda b: sets[loq[b]], q, k)

    def search_excluding(self, q, k, lists, list_of_query=None):
        loq = np.arange(len(lists)) if list_of_query is None else list_of_query
        everything = np.arange(self.n, dtype=np.int64)
        sets = [everything if l is None else np.setdiff1d(everything, self._resolve(l)) for l in lists]
        return self._topk(lambda b: sets[loq[b]], q, k)

    def search_where(self, q, k, pred, filter_ids=None):
        pos = self._rowset(pred, filter_ids)
        if self.opts["where_route"] != 2:
            self._gather_chunks(pos)
        return self._topk(lambda b: pos, q, k)

    def search_where_each(self, q, k, preds, pred_of_query=None):
        poq = np.arange(len(preds)) if pred_of_query is None else pred_of_query
        sets = [np.flatnonzero(self._mask(p)) for p in preds]
        return self._topk(lambda b: sets[poq[b]], q, k)

    def _within(self, pred, filter_ids):
        """-> (positions, gathered, rows the sub-index held before) of a restricted radial / collapsed call"""
        if pred is None and filter_ids is None:
            return np.arange(self.n, dtype=np.int64), False, 0
        pos = self._rowset(pred, filter_ids)
        gathered = 0 < pos.size <= self.opts["filter_gather_rows"]
        return pos, gathered, self._gather(pos) if gathered else 0

    def range_search(self, q, min_cos, max_hits=10, pred=None, filter_ids=None):
        qn, S = self._qn(q), self._scores(q)
        b_ = qn.shape[0]
        t = np.broadcast_to(np.asarray(min_cos, np.float32), (b_,))
        pos, gathered, before = self._within(pred, filter_ids)
        counts = np.zeros(b_, np.int64)
        cos = np.full((b_, max_hits), -np.inf, np.float32)
        ids = np.full((b_, max_hits), -1, np.int64)
        for b in range(b_):
            p, s = self._rank(pos, S[:, b])
            hit = s >= t[b]
            counts[b] = hit.sum()
            if gathered and self.fault == "gather_leftover" and before > pos.size:
                left = (self.sub_X[pos.size:before].astype(np.float64) @ qn[b]).astype(np.float32)
                counts[b] += (left >= t[b]).sum()
            m = min(int(hit.sum()), max_hits)
            cos[b, :m], ids[b, :m] = s[:m], self._ids_of(p[:m])
        return counts, cos, ids

    def search_collapsed(self, q, k, pred=None, filter_ids=None):
        S = self._scores(q)
        pos, gathered, _ = self._within(pred, filter_ids)
        keys = np.full(pos.size, NONE, np.int64) if self.keys is None else self.keys[pos]
        if gathered and self.keys is not None:
            if self.fault == "collapsed_inherits_keys" and self.sub_keys is not None and self.sub_keys.size >= pos.size:
                keys = self.sub_keys[:pos.size]
            else:
                self.sub_keys = keys.copy()
        key_of = dict(zip(pos.tolist(), keys.tolist()))
        cos = np.full((S.shape[1], k), -np.inf, np.float32)
        ids = np.full((S.shape[1], k), -1, np.int64)
        out = np.full((S.shape[1], k), NONE, np.int64)
        for b in range(S.shape[1]):
            p, s = self._rank(pos, S[:, b])
            seen, j = set(), 0
            for pj, sj in zip(p.tolist(), s):
                key = key_of[pj]
                group = ("row", pj) if key == NONE else key
                if group in seen:
                    continue
                seen.add(group)
                cos[b, j], ids[b, j], out[b, j] = sj, self._ids_of([pj])[0], key
                j += 1
                if j == k:
                    break
        return cos, ids, out

    def search_mmr(self, q, k, lam=0.5, n_cand=0, nprobe=0, pred=None, filter_ids=None):
        qn = self._qn(q)
        n_cand = n_cand or min(256, max(32, 4 * k))
        lam = np.broadcast_to(np.asarray(lam, np.float32), (qn.shape[0],))
        if pred is None and filter_ids is None:
            cand = self._first_pass(q, n_cand)
        else:
            pos = self._rowset(pred, filter_ids)
            cand = [pos] * qn.shape[0]
            if self.opts["where_route"] != 2:
                self._gather_chunks(pos)
        S = self._scores(q)
        cos = np.full((qn.shape[0], k), -np.inf, np.float32)
        ids = np.full((qn.shape[0], k), -1, np.int64)
        obj = np.full((qn.shape[0], k), -np.inf, np.float32)
        for b in range(qn.shape[0]):
            p, s = self._rank(cand[b], S[:, b], n_cand)
            rows = self.X[p].astype(np.float64)
            order, objs, _ = greedy(s, rows @ rows.T, lam[b], k)
            m = order.size
            cos[b, :m], ids[b, :m], obj[b, :m] = s[order], self._ids_of(p[order]), objs.astype(np.float32)
        return cos, ids, obj

    def search_fused(self, q, k, offsets=None, mode="rrf", weights=None, depth=0, rank_constant=60, nprobe=0):
        depth = depth or (k if mode == "max" else min(256, max(32, 4 * k)))
        cos, ids = self.search(q, depth)
        offsets = np.array([0, len(q)], np.int64) if offsets is None else offsets
        return fuse_groups(cos, ids, offsets, k, mode, weights, rank_constant)

    # ------------------------------------------------------------ the integer calls
    def _field_model(self, pos):
        fm = FieldModel(0)
        fm.ids = self._ids_of(pos)
        fm.cols = {f: c[pos] for f, c in self.fields.items()}
        return fm

    def aggregate_fields(self, pred, aggs, filter_ids=None, bucket_cap=None):
        return agg_reference.aggregate(self._field_model(self._rowset(pred, filter_ids)), [], aggs, bucket_cap=bucket_cap)

    def sort_fields(self, pred, sort, k, filter_ids=None, after=None):
        total, ids, values = sort_reference.sort_fields(self._field_model(self._rowset(pred, filter_ids)), [], sort, k, after=after)
        return {"total": total, "ids": ids, "values": values}

    def match_fields(self, preds, cap):
        counts = np.zeros(len(preds), np.int64)
        ids = np.full((len(preds), cap), -1, np.int64)
        for j, pred in enumerate(preds):
            pos = np.flatnonzero(self._mask(pred))
            counts[j] = pos.size
            ids[j, :min(cap, pos.size)] = self._ids_of(pos[:cap])
        return counts, ids

    def count_fields(self, preds):
        return self.match_fields(preds, 0)[0]


def fill_twin(twin, model, gather_rows):
    """the model's live rows in ascending id order, with its keys and fields, into a fresh index (real or fake)"""
    twin.set_option("filter_gather_rows", gather_rows)
    n = len(model)
    if n == 0:
        return twin
    twin.add(model.raw())
    pos = np.arange(n, dtype=np.int64)
    if KEYS in model.fm.cols:
        keys = model.keys()
        if np.any(keys != NONE):
            twin.set_keys(pos[keys != NONE], keys[keys != NONE])
    for slot in model.slots():
        v = model.field(slot)
        if np.any(v != NONE):
            twin.set_field(slot, pos[v != NONE], v[v != NONE])
    return twin


def fake_twin(model):
    from tests.session_cases import GATHER_ROWS
    return fill_twin(FakeIndex(model.dim), model, GATHER_ROWS)
