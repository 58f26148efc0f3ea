"""NumPy model of sorting on fields (include/sqe.h: sqe_index_sort_fields) over a tests.fields_reference.FieldModel: what
tests/test_sort_cpu.py checks against a naive restatement and tests/test_sort_gpu.py compares the library with, bit for bit.
Also a NumPy stand-in of the slab / merge cascade of csrc/sort.hip (slab size, fan-in, levels), with the faults a kernel of
that shape could have, seeded on request: test_sort_cpu.py shows that each fails the property it belongs to.  Pure integers."""
import numpy as np

from tests.fields_reference import NONE

U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
TOP = np.uint64(1 << 63)


def split_key(key):
    """(slot, "asc" | "desc"[, {"missing": "first" | "last"}]) -> (slot, desc, first)"""
    key = tuple(key)
    return int(key[0]), key[1] == "desc", len(key) > 2 and key[2].get("missing", "last") == "first"


def image(values, desc, first):
    """uint64 [n]: the order image of raw values (NONE: missing); rows sort by it ascending"""
    v = np.asarray(values, np.int64).reshape(-1)
    b = v.view(np.uint64) ^ TOP
    with np.errstate(over="ignore"):
        if desc:
            u = (np.uint64(0) - b) if first else ~b
        else:
            u = b if first else b - np.uint64(1)
    return np.where(v == NONE, np.uint64(0) if first else U64_MAX, u)


def columns(model, sort):
    """raw values int64 [n_sort, n] and images uint64 [n_sort, n] of every live row, by position"""
    raw, img = [], []
    for key in sort:
        slot, desc, first = split_key(key)
        col = model.cols.get(slot, np.full(model.ids.size, NONE, np.int64))
        raw.append(col)
        img.append(image(col, desc, first))
    return np.array(raw, np.int64).reshape(len(sort), -1), np.array(img, np.uint64).reshape(len(sort), -1)


def cursor_images(sort, after):
    values, rid = after
    return [image([NONE if v is None else v], *split_key(key)[1:])[0] for key, v in zip(sort, values)], int(rid)


def after_mask(img, ids, cur, rid, strict=True):
    """bool [n]: the rows whose tuple (images, id) lies after the cursor's"""
    gt = np.zeros(ids.size, bool)
    eq = np.ones(ids.size, bool)
    for j, c in enumerate(cur):
        gt |= eq & (img[j] > c)
        eq &= img[j] == c
    return gt | (eq & ((ids > rid) if strict else (ids >= rid)))


def selected(model, pred, filter_ids):
    m = model.mask(pred)
    if filter_ids is not None:
        m &= np.isin(model.ids, np.asarray(filter_ids, np.int64))
    return m


def sort_fields(model, pred, sort, k, filter_ids=None, after=None):
    """-> (total, ids int64 [m], values int64 [m, n_sort]) as VectorIndex.sort_fields returns them"""
    raw, img = columns(model, sort)
    m = selected(model, pred, filter_ids)
    total = int(m.sum())
    if after is not None:
        cur, rid = cursor_images(sort, after)
        m &= after_mask(img, model.ids, cur, rid)
    pos = np.flatnonzero(m)
    order = np.lexsort((model.ids[pos],) + tuple(img[j][pos] for j in range(len(sort) - 1, -1, -1)))
    pos = pos[order[:k]]
    return total, model.ids[pos].copy(), raw[:, pos].T.copy()


def same(got, want):
    """a VectorIndex.sort_fields result against the model's triple, bit for bit"""
    return (got["total"] == want[0] and got["ids"].dtype == np.int64 and np.array_equal(got["ids"], want[1])
            and got["values"].shape == want[2].shape and np.array_equal(got["values"], want[2]))


# ------------------------------------------------------------------------------ the stand-in of the cascade
FAULTS = ("tie_dropped", "missing_is_max", "cursor_not_strict", "tie_by_candidate_order")


def _select(keys, wanted, fault):
    """keys: uint64 [n_levels, m], the last level unique -> the indices of the `wanted` first items in lexicographic order,
    found as the kernel finds them: level by level, a threshold, winners below it, the ties at it carried on"""
    m = keys.shape[1]
    alive = np.ones(m, bool)
    win = np.zeros(m, bool)
    if m <= wanted:
        return np.flatnonzero(alive)
    for level in range(keys.shape[0]):
        u = keys[level]
        live = np.sort(u[alive])
        T = live[wanted - 1] if live.size >= wanted else U64_MAX
        below, eq = alive & (u < T), alive & (u == T)
        win |= below
        if below.sum() + eq.sum() <= wanted:
            win |= eq
            break
        wanted -= int(below.sum())
        if fault == "tie_dropped":
            break                                         # the rows AT the threshold never reach the next level
        alive = eq
    return np.flatnonzero(win)


def cascade(model, pred, sort, k, filter_ids=None, after=None, slab=16384, fan_in=64, fault=None, seed=0):
    """The answer by the shape of csrc/sort.hip: a select per slab of `slab` positions, merges of `fan_in` lists until one is
    left, a final ranking.  Candidates leave every list in an arbitrary (seeded) order, as atomics hand out their slots.
    -> (total, ids, values, merge levels)"""
    rng = np.random.default_rng(seed)
    raw, img = columns(model, sort)
    if fault == "missing_is_max":
        img = np.minimum(img, U64_MAX - np.uint64(1))     # the image of "missing last" lands on the one of INT64_MAX ascending
    n, n_sort = model.ids.size, len(sort)
    m = selected(model, pred, filter_ids)
    total = int(m.sum())
    if after is not None:
        cur, rid = cursor_images(sort, after)
        if fault == "missing_is_max":
            cur = [min(c, U64_MAX - np.uint64(1)) for c in cur]
        m &= after_mask(img, model.ids, cur, rid, strict=fault != "cursor_not_strict")
    lists = []
    for p0 in range(0, max(n, 1), slab):
        pos = np.flatnonzero(m[p0:p0 + slab]) + p0
        keys = np.vstack([img[:, pos], pos.astype(np.uint64)[None, :]]).reshape(n_sort + 1, -1)
        lists.append(rng.permutation(pos[_select(keys, k, fault)]))
    levels = 0
    while True:
        groups = [np.concatenate(lists[g:g + fan_in]) for g in range(0, len(lists), fan_in)]
        levels += 1
        merged = []
        for pos in groups:
            keys = np.vstack([img[:, pos], pos.astype(np.uint64)[None, :]]).reshape(n_sort + 1, -1)
            merged.append(rng.permutation(pos[_select(keys, k, fault)]))
        lists = merged
        if len(lists) == 1:
            break
    pos = lists[0]
    tie = np.arange(pos.size) if fault == "tie_by_candidate_order" else pos
    pos = pos[np.lexsort((tie,) + tuple(img[j][pos] for j in range(n_sort - 1, -1, -1)))]
    return total, model.ids[pos].copy(), raw[:, pos].T.copy().reshape(pos.size, n_sort), levels
