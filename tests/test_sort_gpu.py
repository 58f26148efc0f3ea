"""Sorting on fields on the GPU (csrc/sort.hip: sqe_index_sort_fields) against the NumPy model of tests/sort_reference.py: keys,
directions and missing placements, ties down to the id, the extremes, the slabs and merge levels sqe_index_sort_last reports,
paging with the cursor, mutations, IVF, a device group of three logical shards and every refusal.  Integers only: every
comparison is bit for bit.  70,001 rows are four full slabs of 16,384 positions and a partial one; the columns are those of
tests/test_agg_gpu.py.  GPU only."""
import ctypes as C

import numpy as np
import pytest

from tests import sort_reference as S
from tests.fields_reference import I64_MAX, NONE, FieldModel

pytestmark = pytest.mark.gpu

N, DIM = 70_001, 64
# field slots: dense years, 30 % missing +-2^40, keyword codes, the row's position, values near +-2^62, a column the tests rewrite,
# a boolean, never set
YEAR, SCORE, CODE, POS, BIG, TMP, FLAG, UNSET = range(8)
ALL_IDS = np.arange(N, dtype=np.int64)
MODES = [("asc", "last"), ("asc", "first"), ("desc", "last"), ("desc", "first")]
PREDS = [
    [],
    [(YEAR, "range", 2010, 2019)],
    [(CODE, "in", list(range(0, 3000, 3)), {"not_": True})],
    [(YEAR, "range", 3000, None)],                      # selects nothing
]
ONE_PERCENT = [(CODE, "in", list(range(0, 3000, 100)))]


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2016)
    x = rng.standard_normal((N, DIM)).astype(np.float32)
    year = rng.integers(1990, 2025, N).astype(np.int64)
    score = rng.integers(-(1 << 40), 1 << 40, N).astype(np.int64)
    score[rng.random(N) < 0.3] = NONE
    code = rng.integers(0, 3000, N).astype(np.int64)
    big = (rng.integers(-(1 << 20), 1 << 20, N) + np.where(rng.random(N) < 0.7, 1 << 62, -(1 << 62))).astype(np.int64)
    flag = (rng.random(N) < 0.8).astype(np.int64)
    allow = rng.integers(-10, N + 10, 20_000).astype(np.int64)        # repeats, and ids that name no live row
    return {"x": x, "allow": allow, "cols": {YEAR: year, SCORE: score, CODE: code, POS: ALL_IDS.copy(), BIG: big, FLAG: flag}}


def _make(ctx, data, kind="flat"):
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd.engine import INDEX_IVF_FLAT
    if kind == "ivf":
        idx = VectorIndex(ctx, DIM, INDEX_IVF_FLAT, 16)
        idx.train(data["x"][:4096], iters=4)
    else:
        idx = VectorIndex(ctx, DIM)
    idx.add(data["x"])
    model = FieldModel(N)
    for f, col in data["cols"].items():
        idx.set_field(f, ALL_IDS, col)
        model.set_field(f, ALL_IDS, col)
    return idx, model


@pytest.fixture(scope="module")
def flat(ctx, data):
    return _make(ctx, data)


def _tmp(pair, col):
    """the column the test works on, in slot TMP of index and model"""
    idx, model = pair
    col = np.asarray(col, np.int64)
    idx.set_field(TMP, ALL_IDS, col)
    model.set_field(TMP, ALL_IDS, col)


def _key(slot, mode):
    return (slot, mode[0], {"missing": mode[1]})


def _check(pair, pred, sort, k, **kw):
    idx, model = pair
    got = idx.sort_fields(pred, sort, k, **kw)
    want = S.sort_fields(model, pred, sort, k, **kw)
    assert S.same(got, want), (pred, sort, k, kw, got["total"], want[0], got["ids"][:8], want[1][:8])
    return got


def _cursor(got, i=-1):
    """the cursor after hit i of a result"""
    return [None if v == NONE else int(v) for v in got["values"][i]], int(got["ids"][i])


# ---------------------------------------------------------------- 1. keys, directions, k
@pytest.mark.parametrize("slots", [(SCORE,), (YEAR, SCORE), (FLAG, YEAR, BIG), (FLAG, YEAR, CODE, SCORE)])
def test_keys_directions_and_k(flat, data, slots):
    for turn in range(4):             # key j takes mode (turn + j) % 4: every direction x missing placement at every key
        sort = [_key(s, MODES[(turn + j) % 4]) for j, s in enumerate(slots)]
        for k in (1, 10, 256):
            for pred in PREDS:
                got = _check(flat, pred, sort, k)
                assert got["ids"].size == min(k, got["total"])
            got = _check(flat, PREDS[1], sort, k, filter_ids=data["allow"])
            assert 0 < got["total"] < np.unique(data["allow"]).size
    idx, _ = flat
    for pred in PREDS:
        assert idx.sort_fields(pred, [(YEAR, "asc")], 1)["total"] == int(idx.count_fields([pred])[0])
    empty = _check(flat, [], [(YEAR, "asc")], 10, filter_ids=np.empty(0, np.int64))       # an empty list selects nothing
    assert empty["total"] == 0 and empty["ids"].size == 0 and empty["values"].shape == (0, 1)
    _check(flat, [], [(YEAR, "asc")], 10, filter_ids=[N, N + 5, -1])                       # no id is live


# ---------------------------------------------------------------- 2. ties
def test_ties_go_down_to_the_next_key_and_the_id(flat):
    _tmp(flat, np.full(N, 7, np.int64))
    for mode in MODES:
        # a constant column as key 0 sends everything to key 1
        _check(flat, [], [_key(TMP, mode), _key(SCORE, MODES[2])], 256)
        # 35 years, k = 256: the k-th place lies inside a run of ties, which the next key and then the id resolve
        _check(flat, [], [_key(YEAR, mode)], 256)
        _check(flat, [], [_key(YEAR, mode), _key(FLAG, mode)], 256)
        # all keys tie everywhere: the id order decides; a slot never set ties everywhere too
        got = _check(flat, [], [_key(TMP, mode), _key(UNSET, mode)], 256)
        assert np.array_equal(got["ids"], np.arange(256)) and np.all(got["values"][:, 1] == NONE)
        _check(flat, PREDS[1], [_key(UNSET, mode)], 10)
        got = _check(flat, PREDS[1], [_key(UNSET, mode), _key(YEAR, mode)], 10)
        _check(flat, PREDS[1], [_key(UNSET, mode), _key(YEAR, mode)], 256, after=_cursor(got))


# ---------------------------------------------------------------- 3. extremes
@pytest.mark.parametrize("mode", MODES)
def test_extremes_at_the_slab_and_wave_borders(flat, mode):
    at = [0, 31, 32767, 32768, N - 1]
    for values in ([I64_MAX, NONE + 1, NONE, I64_MAX, NONE + 1], [NONE, I64_MAX, NONE + 1, NONE, I64_MAX]):
        col = np.full(N, NONE, np.int64)
        col[1::2] = 5                                     # half the rows present and tied, the other half missing
        col[at] = values
        _tmp(flat, col)
        for k in (1, 3, 256):
            _check(flat, [], [_key(TMP, mode)], k)
        _check(flat, [(POS, "in", at + [7, 8])], [_key(TMP, mode)], 10)
        got = _check(flat, [(POS, "in", at + [7, 8])], [_key(TMP, mode), (YEAR, "asc")], 3)
        _check(flat, [(POS, "in", at + [7, 8])], [_key(TMP, mode), (YEAR, "asc")], 10, after=_cursor(got))
        for cur in ([I64_MAX], [NONE + 1], [None]):        # cursors AT the extremes, on rows and past them
            for rid in (-1, 31, N):
                _check(flat, [(POS, "in", at + [7, 8])], [_key(TMP, mode)], 10, after=(cur, rid))


# ---------------------------------------------------------------- 4. slabs, merge levels, sort_last
def test_slabs_and_merge_levels_are_reported(flat):
    idx, _ = flat
    sort = [(SCORE, "desc"), (YEAR, "asc")]
    one_slab = [(POS, "range", 20_000, 20_300)]
    per_slab = [(POS, "in", [5, 16_384 + 7, 32_768, 49_152 + 100, N - 1])]
    try:
        for fan, levels in ((64, 1), (2, 3), (3, 2)):
            idx.set_option("sort_fan_in", fan)
            _check(flat, one_slab, sort, 10)
            assert idx.sort_last() == {"slabs": 5, "slabs_occupied": 1, "merge_levels": levels, "fan_in": fan, "candidates": 10}
            _check(flat, per_slab, sort, 3)
            assert idx.sort_last() == {"slabs": 5, "slabs_occupied": 5, "merge_levels": levels, "fan_in": fan, "candidates": 5}
            _check(flat, PREDS[3], sort, 10)
            assert idx.sort_last() == {"slabs": 5, "slabs_occupied": 0, "merge_levels": levels, "fan_in": fan, "candidates": 0}
            got = _check(flat, [], sort, 256)
            assert idx.sort_last() == {"slabs": 5, "slabs_occupied": 5, "merge_levels": levels, "fan_in": fan, "candidates": 5 * 256}
            # the cursor leaves rows alive in some slabs only: the total still counts every selected row
            after = ([None, 2024], N - 20_000)
            got = _check(flat, [], [(SCORE, "asc"), (YEAR, "asc")], 256, after=after)
            assert got["total"] == N and idx.sort_last()["slabs_occupied"] == 2
    finally:
        idx.set_option("sort_fan_in", 64)
    from semantic_query_engine_amd._native import SqeError
    for bad in (1, 65):
        with pytest.raises(SqeError):
            idx.set_option("sort_fan_in", bad)


def test_fan_in_two_gives_the_bits_of_fan_in_64(flat):
    idx, _ = flat
    sort = [(YEAR, "desc", {"missing": "first"}), (FLAG, "asc"), (SCORE, "desc")]
    wide = [idx.sort_fields(p, sort, k) for p in PREDS[:3] for k in (10, 256)]
    try:
        idx.set_option("sort_fan_in", 2)
        narrow = [idx.sort_fields(p, sort, k) for p in PREDS[:3] for k in (10, 256)]
        assert idx.sort_last()["merge_levels"] == 3
    finally:
        idx.set_option("sort_fan_in", 64)
    for a, b in zip(wide, narrow):
        assert a["total"] == b["total"] and np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["values"], b["values"])


# ---------------------------------------------------------------- 5. paging
def _walk(idx, pred, sort, k, on_page=None):
    ids, after, pages = [], None, 0
    while True:
        got = idx.sort_fields(pred, sort, k, after=after)
        if got["ids"].size == 0:
            return ids, pages
        ids += got["ids"].tolist()
        after = _cursor(got)
        pages += 1
        if on_page is not None:
            on_page(pages, got)


def test_paging_visits_every_row_once_in_order(flat):
    idx, model = flat
    for sort in ([(YEAR, "desc"), (SCORE, "asc", {"missing": "first"})], [(FLAG, "asc")]):
        total, want, _ = S.sort_fields(model, ONE_PERCENT, sort, N)
        assert 500 < total < 900
        ids, pages = _walk(idx, ONE_PERCENT, sort, 7)
        assert ids == want.tolist() and pages == -(-total // 7)


def test_paging_survives_a_delete_of_the_cursor_row(ctx, data):
    pair = _make(ctx, data)
    idx, model = pair
    sort = [(YEAR, "asc"), (SCORE, "desc")]
    _, before, _ = S.sort_fields(model, ONE_PERCENT, sort, N)
    gone = []

    def delete_cursor_row(page, got):
        if page == 3:                                     # the row the cursor names, and the one that would come next
            rows = [int(got["ids"][-1]), int(before[21])]
            idx.delete(rows)
            model.delete(rows)
            gone.extend(rows)

    ids, _ = _walk(idx, ONE_PERCENT, sort, 7, delete_cursor_row)
    assert gone == [int(before[20]), int(before[21])]
    assert ids == [i for i in before.tolist() if i != gone[1]]      # the cursor's row was served, its successor never is
    _check(pair, ONE_PERCENT, sort, 256)


# ---------------------------------------------------------------- 6. mutations, an index without fields, IVF
def test_after_set_field_update_delete_and_add_the_answers_follow(ctx, data):
    pair = _make(ctx, data)
    idx, model = pair
    sort = [(YEAR, "desc"), (SCORE, "asc", {"missing": "first"}), (BIG, "asc")]
    rng = np.random.default_rng(3)
    rows = rng.choice(N, 500, replace=False).astype(np.int64)
    vals = rng.integers(1980, 2030, 500).astype(np.int64)
    vals[::7] = NONE
    idx.set_field(YEAR, rows, vals)
    model.set_field(YEAR, rows, vals)
    _check(pair, [], sort, 256)
    idx.update(rows[:50], data["x"][:50])                 # the vectors change, the values stay with their rows
    _check(pair, PREDS[2], sort, 256)
    gone = np.concatenate([np.arange(16_300, 16_500), [0, 5, N - 1]]).astype(np.int64)      # across a slab boundary: compaction
    idx.delete(gone)
    model.delete(gone)
    for pred in PREDS[:3]:
        got = _check(pair, pred, sort, 256)
    _check(pair, [], sort, 50, after=_cursor(got, 100))
    idx.add(data["x"][:300])
    model.add(300)
    new = np.arange(N, N + 300, dtype=np.int64)
    idx.set_field(YEAR, new, data["cols"][YEAR][:300] + 20)
    model.set_field(YEAR, new, data["cols"][YEAR][:300] + 20)
    for pred in PREDS[:2]:
        _check(pair, pred, sort, 256)
        _check(pair, pred, [(YEAR, "asc", {"missing": "first"}), (POS, "desc")], 256, filter_ids=np.arange(100, N + 300))


def test_index_without_fields_sorts_by_id(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, DIM)
    empty = idx.sort_fields([], [(YEAR, "asc")], 10)                 # an empty index
    assert empty["total"] == 0 and empty["ids"].size == 0
    assert idx.sort_last() == {"slabs": 0, "slabs_occupied": 0, "merge_levels": 0, "fan_in": 64, "candidates": 0}
    idx.add(data["x"][:5000])
    got = _check((idx, FieldModel(5000)), [], [(YEAR, "desc"), (CODE, "asc")], 256)
    assert np.array_equal(got["ids"], np.arange(256)) and np.all(got["values"] == NONE)
    assert idx.field_info() == {"fields": 0, "device_bytes": 0}


def test_ivf_index_gives_the_flat_answers(ctx, data, flat):
    ivf = _make(ctx, data, "ivf")
    sort = [(YEAR, "asc"), (SCORE, "desc", {"missing": "first"})]
    allow = np.arange(0, N, 3)
    for pred in PREDS[:3]:
        got = _check(ivf, pred, sort, 256, filter_ids=allow)
        again = flat[0].sort_fields(pred, sort, 256, filter_ids=allow)
        assert np.array_equal(got["ids"], again["ids"]) and np.array_equal(got["values"], again["values"]) and got["total"] == again["total"]


# ---------------------------------------------------------------- 7. device group
def test_device_group_of_three_shards_answers_as_the_single_index(data, flat):
    """logical shards on one device, as tests/test_group_gpu.py builds them: predicates, a routed allow-list, a cursor, a shard
    that holds no match, after a delete -- against the model and the single index"""
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    from semantic_query_engine_amd._native import SqeError
    single, _ = flat
    grp = VectorIndex(Context(devices=[0, 0, 0], exchange=EXCHANGE_COPY), DIM)
    grp.add(data["x"])
    model = FieldModel(N)
    for f, col in data["cols"].items():
        grp.set_field(f, ALL_IDS, col)
        model.set_field(f, ALL_IDS, col)
    pair = (grp, model)
    sorts = [[(YEAR, "desc"), (SCORE, "asc", {"missing": "first"})], [(FLAG, "asc"), (UNSET, "desc")], [(BIG, "desc", {"missing": "first"})]]
    for sort in sorts:
        for pred in PREDS:
            for k in (1, 10, 256):
                got = _check(pair, pred, sort, k)
                one = single.sort_fields(pred, sort, k)
                assert got["total"] == one["total"] and np.array_equal(got["ids"], one["ids"]) and np.array_equal(got["values"], one["values"])
        got = _check(pair, PREDS[1], sort, 10, filter_ids=data["allow"])
        _check(pair, PREDS[1], sort, 256, filter_ids=data["allow"], after=_cursor(got))           # a cursor inside a run of ties
        _check(pair, [], sort, 256, after=_cursor(got, 4))
    # rows of one shard only (ids = 1 mod 3): the other two shards hold no match
    one_shard = [(POS, "in", list(range(1, 3000, 3)))]
    got = _check(pair, one_shard, sorts[0], 256)
    assert np.all(got["ids"] % 3 == 1)
    _check(pair, one_shard, sorts[1], 7, after=([1, None], 1000))
    assert _check(pair, [], sorts[0], 5, filter_ids=np.empty(0, np.int64))["total"] == 0
    _check(pair, [], sorts[0], 5, filter_ids=[4, 7, 10])                                          # an allow-list that reaches one shard
    ids, pages = _walk(grp, ONE_PERCENT, sorts[0], 50)
    assert ids == S.sort_fields(model, ONE_PERCENT, sorts[0], N)[1].tolist()
    gone = np.concatenate([np.arange(32_700, 32_800), [0, 5, N - 1]]).astype(np.int64)
    grp.delete(gone)
    model.delete(gone)
    _check(pair, PREDS[1], sorts[0], 256)
    _check(pair, [], sorts[1], 256, after=([1, None], 32_750))                                    # a cursor on a deleted row
    with pytest.raises(SqeError) as e:
        grp.sort_last()
    assert e.value.code == -5


# ---------------------------------------------------------------- 8. refusals
def test_every_refusal_leaves_the_buffers_untouched(flat):
    from semantic_query_engine_amd.engine import FIELD_DTYPE, SORT_DTYPE
    idx, _ = flat
    ok_sort = [(YEAR, 0)]
    ok_clause = [(YEAR, 0, 2000, 2010)]

    def call(clauses=ok_clause, n_clauses=None, sets=(), n_set=None, allow=None, n_allow=-1, sort=ok_sort, n_sort=None, k=16, after=None,
             null=()):
        cl = np.array(clauses, dtype=FIELD_DTYPE)
        sv = np.array(sets, np.int64)
        so = np.array(sort, dtype=SORT_DTYPE)
        al = None if allow is None else np.array(allow, np.int64)
        af = None if after is None else np.array(after, np.int64)
        ids, vals, total = np.full(256, 77, np.int64), np.full((256, 4), 77, np.int64), C.c_int64(77)
        ptr = {"total": C.byref(total), "ids": ids.ctypes.data, "vals": vals.ctypes.data, "sort": so.ctypes.data}
        for name in null:
            ptr[name] = None
        rc = idx.lib.sqe_index_sort_fields(idx.handle, cl.ctypes.data, len(clauses) if n_clauses is None else n_clauses, sv.ctypes.data,
                                           len(sets) if n_set is None else n_set, None if al is None else al.ctypes.data, n_allow,
                                           ptr["sort"], len(sort) if n_sort is None else n_sort, k, None if af is None else af.ctypes.data, 0,
                                           ptr["total"], ptr["ids"], ptr["vals"])
        return rc, bool(total.value == 77 and np.all(ids == 77) and np.all(vals == 77))

    assert call() == (0, False)                                       # the well-formed call the cases below break one way each
    assert call(after=[2005]) == (0, False)
    bad = [
        dict(n_clauses=9), dict(n_clauses=-1), dict(clauses=[(8, 0, 0, 1)]), dict(clauses=[(0, 7, 0, 1)]),      # clauses
        dict(clauses=[(0, 1, 0, 2)], sets=[5, 5]), dict(clauses=[(0, 1, 0, 3)], sets=[1, 2]), dict(n_set=4097),
        dict(n_allow=-2), dict(n_allow=3, allow=None),                                                        # lists
        dict(n_sort=0), dict(n_sort=5, sort=[(j, 0) for j in range(5)]), dict(n_sort=-1), dict(null=("sort",)),
        dict(sort=[(8, 0)]), dict(sort=[(-1, 0)]), dict(sort=[(YEAR, 0), (8, 1)]),                            # slot
        dict(sort=[(YEAR, 0), (SCORE, 1), (YEAR, 2)]), dict(sort=[(CODE, 3), (CODE, 3)]),                     # a slot named twice
        dict(sort=[(YEAR, 4)]), dict(sort=[(YEAR, -1)]), dict(sort=[(YEAR, 1), (SCORE, 8)]),                  # flag bits
        dict(k=0), dict(k=257), dict(k=-5),
        dict(null=("total",)), dict(null=("ids",)), dict(null=("vals",)),
    ]
    for kw in bad:
        assert call(**kw) == (-1, True), kw
    assert idx.lib.sqe_index_sort_fields(None, None, 0, None, 0, None, -1, None, 1, 1, None, 0, None, None, None) == -1
    assert idx.lib.sqe_index_sort_last(idx.handle, None) == -1


def test_sort_last_needs_a_call(ctx):
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd._native import SqeError
    with pytest.raises(SqeError):
        VectorIndex(ctx, DIM).sort_last()
