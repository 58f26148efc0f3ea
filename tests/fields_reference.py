"""NumPy model of the numeric fields and field predicates (include/sqe.h: sqe_index_set_field, sqe_index_match_fields):
what tests/test_fields_cpu.py checks by hand and tests/test_fields_gpu.py compares the library with.  Pure integers."""
import numpy as np

NONE = -(1 << 63)
I64_MAX = (1 << 63) - 1


def clause_holds(values, op, args, not_=False):
    """bool [n]: the clause over a column (int64 [n], NONE where a row has no value)"""
    values = np.asarray(values, np.int64)
    has = values != NONE
    if op == "range":
        lo, hi = args
        lo = NONE + 1 if lo is None else int(lo)
        hi = I64_MAX if hi is None else int(hi)
        r = has & (values >= lo) & (values <= hi) if lo <= hi else np.zeros(values.shape, bool)
    elif op == "in":
        r = has & np.isin(values, np.asarray(args[0], np.int64))
    else:
        raise ValueError(op)
    return ~r if not_ else r


def split_clause(cl):
    cl = tuple(cl)
    not_ = False
    if cl and isinstance(cl[-1], dict):
        not_ = bool(cl[-1].get("not_", False))
        cl = cl[:-1]
    return int(cl[0]), cl[1], cl[2:], not_


class FieldModel:
    """The live ids of an index (ascending) and its field columns."""

    def __init__(self, n=0):
        self.ids = np.arange(n, dtype=np.int64)
        self.next_id = n
        self.cols = {}

    def add(self, count):
        self.ids = np.concatenate([self.ids, np.arange(self.next_id, self.next_id + count, dtype=np.int64)])
        for f in self.cols:
            self.cols[f] = np.concatenate([self.cols[f], np.full(count, NONE, np.int64)])
        self.next_id += count

    def _pos(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        pos = np.searchsorted(self.ids, ids)
        if ids.size and (np.any(pos >= self.ids.size) or np.any(self.ids[np.minimum(pos, self.ids.size - 1)] != ids)):
            raise KeyError("an id is not live")
        return pos

    def set_field(self, field, ids, values):
        pos = self._pos(ids)
        col = self.cols.setdefault(field, np.full(self.ids.size, NONE, np.int64))
        for p, v in zip(pos, np.asarray(values, np.int64).reshape(-1)):      # in order: the last of a repeated id wins
            col[p] = v

    def get_field(self, field, ids):
        pos = self._pos(ids)
        return self.cols[field][pos] if field in self.cols else np.full(pos.size, NONE, np.int64)

    def delete(self, ids):
        keep = np.ones(self.ids.size, bool)
        keep[self._pos(ids)] = False
        self.ids = self.ids[keep]
        for f in self.cols:
            self.cols[f] = self.cols[f][keep]

    def mask(self, pred):
        m = np.ones(self.ids.size, bool)
        for cl in pred:
            field, op, args, not_ = split_clause(cl)
            col = self.cols.get(field, np.full(self.ids.size, NONE, np.int64))
            m &= clause_holds(col, op, args, not_)
        return m

    def select(self, pred):
        """the ids the predicate selects, ascending"""
        return self.ids[self.mask(pred)]

    def match(self, preds, cap):
        """-> (counts [P], ids [P, cap]) as sqe_index_match_fields returns them"""
        counts = np.zeros(len(preds), np.int64)
        out = np.full((len(preds), cap), -1, np.int64)
        for j, pred in enumerate(preds):
            sel = self.select(pred)
            counts[j] = sel.size
            out[j, :min(cap, sel.size)] = sel[:cap]
        return counts, out
