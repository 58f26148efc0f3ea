"""The model of an index under a session of mutations (tests/session_cases.py): raw float32 rows by id, the live ids
ascending, next_id, the group keys and up to eight field columns.  The ids, keys and fields are a
tests.fields_reference.FieldModel (the keys are one more column of it).  It knows nothing of positions, capacities or
copies: whatever an index keeps behind its handle, this is what it must answer from.  NumPy only."""
import numpy as np

from oracle import retrieval as R
from tests.fields_reference import NONE, FieldModel

KEYS = "keys"                 # the FieldModel column that holds the group keys
MAX_FIELDS = 8


class SessionModel:
    def __init__(self, dim):
        self.dim = int(dim)
        self.rows = {}                       # id -> raw float32 [dim]
        self.fm = FieldModel(0)

    # ------------------------------------------------------------ what it holds
    @property
    def live(self):
        return self.fm.ids

    @property
    def next_id(self):
        return self.fm.next_id

    def __len__(self):
        return int(self.fm.ids.size)

    def is_live(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        return np.isin(ids, self.fm.ids)

    def raw(self, ids=None):
        """raw rows float32 [m, dim] of the live ids given (default: all, ascending)"""
        ids = self.live if ids is None else np.asarray(ids, np.int64).reshape(-1)
        if ids.size == 0:
            return np.empty((0, self.dim), np.float32)
        return np.stack([self.rows[int(i)] for i in ids]).astype(np.float32)

    def normalized(self, ids=None):
        return R.normalize_rows(self.raw(ids))

    def by_id(self):
        """normalised rows float32 [next_id, dim], zero where the id is not live: what gpu_util.assert_topk_matches indexes"""
        xn = np.zeros((max(self.next_id, 1), self.dim), np.float32)
        if len(self):
            xn[self.live] = self.normalized()
        return xn

    def keys(self, ids=None):
        ids = self.live if ids is None else ids
        return self.fm.get_field(KEYS, ids)

    def field(self, slot, ids=None):
        ids = self.live if ids is None else ids
        return self.fm.get_field(int(slot), ids)

    def slots(self):
        return sorted(f for f in self.fm.cols if f != KEYS)

    def select(self, pred=None, filter_ids=None):
        """the live ids of a row set, ascending: the predicate's rows that the list (when given) also names"""
        m = self.fm.mask([] if pred is None else pred)
        if filter_ids is not None:
            m &= np.isin(self.fm.ids, np.asarray(filter_ids, np.int64).reshape(-1))
        return self.fm.ids[m]

    # ------------------------------------------------------------ the five mutations
    def add(self, x):
        x = np.asarray(x, np.float32).reshape(-1, self.dim)
        first = self.next_id
        for j, row in enumerate(x):
            self.rows[first + j] = row.copy()
        self.fm.add(x.shape[0])
        return np.arange(first, first + x.shape[0], dtype=np.int64)

    def update(self, ids, x):
        ids = np.asarray(ids, np.int64).reshape(-1)
        x = np.asarray(x, np.float32).reshape(ids.size, self.dim)
        self.fm._pos(ids)                                    # every id is live
        for i, row in zip(ids, x):                           # in order: the last of a repeated id wins
            self.rows[int(i)] = row.copy()

    def delete(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        if np.unique(ids).size != ids.size:
            raise KeyError("an id is repeated")
        self.fm.delete(ids)
        for i in ids:
            del self.rows[int(i)]

    def set_keys(self, ids, keys):
        self.fm.set_field(KEYS, ids, keys)

    def set_field(self, slot, ids, values):
        slot = int(slot)
        if not 0 <= slot < MAX_FIELDS:
            raise ValueError(slot)
        self.fm.set_field(slot, ids, values)


__all__ = ["KEYS", "MAX_FIELDS", "NONE", "SessionModel"]
