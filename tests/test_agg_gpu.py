"""Field aggregations on the GPU (csrc/aggregate.hip: sqe_index_aggregate_fields) against the NumPy / Python-int model of
tests/agg_reference.py: stats, terms by the dense and by the hash route, histograms, the row set, mutations, IVF, a device group of
three logical shards and every refusal.  Integers only: every comparison is bit for bit, and sqe_index_aggregate_last is asserted wherever a route is named.
70,001 rows are two full 32,768-position bitmap blocks plus a partial one, as tests/test_fields_gpu.py.  GPU only."""
import ctypes as C

import numpy as np
import pytest

from tests import agg_reference as A
from tests.fields_reference import I64_MAX, NONE, FieldModel

pytestmark = pytest.mark.gpu

N, DIM = 70_001, 64
# field slots: dense years, 30 % missing +-2^40, keyword codes, the row's position, values near +-2^62, a column the tests rewrite,
# a boolean, never set
YEAR, SCORE, CODE, POS, BIG, TMP, FLAG, UNSET = range(8)
NONE_ROUTE, DENSE, HASH = 0, 1, 2
ALL_IDS = np.arange(N, dtype=np.int64)


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
    return {"x": x, "cols": {YEAR: year, SCORE: score, CODE: code, POS: ALL_IDS.copy(), BIG: big, FLAG: flag}}


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


def _check(pair, pred, aggs, routes=None, **kw):
    idx, model = pair
    got = idx.aggregate_fields(pred, aggs, **kw)
    want = A.aggregate(model, pred, aggs, **kw)
    last = idx.aggregate_last()
    print("selected", got["selected"], [(g["count"], g["n_buckets"], g["other"]) for g in got["aggs"]], [r["route"] for r in last])
    assert A.same(got, want), (got, want)
    if routes is not None:
        assert [r["route"] for r in last] == list(routes), last
    return got, last


PREDS = [
    [],
    [(YEAR, "range", 2010, 2019)],
    [(CODE, "in", list(range(0, 3000, 3)), {"not_": True})],
    [(YEAR, "range", 3000, None)],                      # selects nothing
]


# ---------------------------------------------------------------- 1. stats
@pytest.mark.parametrize("pred", PREDS)
def test_stats_every_column_shape(flat, pred):
    aggs = [(YEAR, "stats"), (SCORE, "stats"), (BIG, "stats"), (UNSET, "stats")]
    got, last = _check(flat, pred, aggs, routes=[NONE_ROUTE] * 4)
    idx, model = flat
    assert got["selected"] == int(idx.count_fields([pred])[0])
    unset = got["aggs"][3]                                                            # a slot never set
    assert (unset["count"], unset["min"], unset["max"], unset["sum"]) == (0, I64_MAX, NONE, 0)
    if not pred:
        assert abs(got["aggs"][2]["sum"]) > I64_MAX                                  # the sum of BIG leaves int64


def test_stats_extreme_values_and_eight_aggregations(flat):
    col = np.full(N, NONE, np.int64)
    col[[0, 31, 32767, 32768, N - 1]] = [I64_MAX, NONE + 1, I64_MAX, NONE + 1, -1]
    _tmp(flat, col)
    got, _ = _check(flat, [], [(TMP, "stats")])
    assert got["aggs"][0]["min"] == NONE + 1 and got["aggs"][0]["max"] == I64_MAX and got["aggs"][0]["sum"] == -1
    aggs = [(YEAR, "stats"), (SCORE, "stats"), (CODE, "stats"), (POS, "stats"), (BIG, "stats"), (FLAG, "stats"), (YEAR, "terms", 3),
            (TMP, "stats")]                                                           # eight, two of them on one column
    _check(flat, [(SCORE, "range", None, -1)], aggs)


# ---------------------------------------------------------------- 2. terms, dense route
@pytest.mark.parametrize("field, sizes", [(YEAR, (1, 10, 256)), (CODE, (1, 10, 256)), (FLAG, (1, 10))])
def test_terms_dense(flat, field, sizes):
    for size in sizes:            # 256 is above the 35 years' and the flag's distinct values, below the codes'
        for pred in PREDS[:3]:
            _check(flat, pred, [(field, "terms", size)], routes=[DENSE])
    _check(flat, PREDS[3], [(field, "terms", 10)], routes=[NONE_ROUTE])


def test_terms_span_threshold_takes_both_routes(flat, data):
    """a span of exactly 16,384 is dense; the same data with one outlier a step further is 16,385 and hashed: one answer"""
    rng = np.random.default_rng(7)
    col = rng.integers(-5000, -5000 + 16384, N).astype(np.int64)
    col[rng.random(N) < 0.1] = NONE
    col[[5, 40_000]] = [-5000, -5000 + 16383]
    _tmp(flat, col)
    dense, last = _check(flat, [], [(TMP, "terms", 10), (TMP, "terms", 256)], routes=[DENSE, DENSE])
    assert last[0]["span"] == 16384 and last[0]["slots"] == 16384 and last[0]["select_blocks"] == last[0]["occupied_blocks"] == 1
    col[40_000] = -5000 + 16384
    _tmp(flat, col)
    hashed, last = _check(flat, [], [(TMP, "terms", 10), (TMP, "terms", 256)], routes=[HASH, HASH])
    assert last[0]["span"] == 16385 and last[0]["slots"] == 131072 and last[0]["select_blocks"] == 8
    a, b = dense["aggs"][1], hashed["aggs"][1]
    assert a["count"] == b["count"] and abs(a["n_buckets"] - b["n_buckets"]) <= 1       # one row moved, nothing else


# ---------------------------------------------------------------- 3. terms, hash route
def test_terms_hash_all_distinct_ties_decide(flat):
    """POS: 70,001 distinct values, every count 1: the lowest `size` values win, found in many select blocks"""
    for size in (1, 10, 256):
        got, last = _check(flat, [], [(POS, "terms", size)], routes=[HASH])
        assert np.array_equal(got["aggs"][0]["keys"], np.arange(size)) and got["aggs"][0]["other"] == N - size
        assert last[0]["slots"] == 262144 and last[0]["select_blocks"] == last[0]["occupied_blocks"] == 16 and got["aggs"][0]["n_buckets"] == N
    _check(flat, [(POS, "range", 32760, 32775)], [(POS, "terms", 256)], routes=[DENSE])      # 16 values: size above them
    _check(flat, [(YEAR, "range", 2000, 2004)], [(POS, "terms", 7)], routes=[HASH])


def test_terms_hash_one_hot_slot_and_far_outliers(flat):
    col = np.full(N, 42, np.int64)
    col[[3, N - 2]] = [-(1 << 50), 1 << 50]
    _tmp(flat, col)
    got, _ = _check(flat, [], [(TMP, "terms", 5)], routes=[HASH])
    assert got["aggs"][0]["keys"].tolist() == [42, -(1 << 50), 1 << 50] and got["aggs"][0]["counts"].tolist() == [N - 2, 1, 1]


@pytest.mark.parametrize("shift", [32, 0])
def test_terms_hash_keys_differ_in_one_word_only(flat, shift):
    rng = np.random.default_rng(9)
    col = (rng.integers(0, 4096, N).astype(np.int64) << shift)
    if shift == 0:
        col[::1000] = 1 << 40                 # a far value on 71 rows keeps the low-word keys off the dense route
    _tmp(flat, col)
    _check(flat, [], [(TMP, "terms", 256), (TMP, "terms", 3)], routes=[HASH, HASH])
    _check(flat, PREDS[1], [(TMP, "terms", 256)], routes=[HASH])


def test_terms_hash_extreme_keys(flat):
    rng = np.random.default_rng(10)
    col = rng.choice(np.array([I64_MAX, NONE + 1, 0, -1, 1 << 62], np.int64), N)
    col[rng.random(N) < 0.2] = NONE
    _tmp(flat, col)
    _check(flat, [], [(TMP, "terms", 2), (TMP, "terms", 256)], routes=[HASH, HASH])


def test_terms_hash_candidates_from_many_select_blocks(flat, data):
    """the scores: ~49,000 distinct values scattered over the 8 select blocks of a 131,072-slot table, a few of them repeated
    so that the winners come by count from different blocks and the rest by value"""
    col = data["cols"][SCORE].copy()
    have = np.nonzero(col != NONE)[0]
    for j in range(40):
        col[have[1000 + 50 * j: 1000 + 50 * j + 2 + j % 5]] = col[have[j]]
    _tmp(flat, col)
    got, last = _check(flat, [], [(TMP, "terms", 64)], routes=[HASH])
    assert last[0]["select_blocks"] == 8 and last[0]["slots"] == 131072
    assert last[0]["occupied_blocks"] == 8                       # every one of the 8 blocks held keys and sent candidates to the merge
    assert got["aggs"][0]["counts"][0] > 1 and got["aggs"][0]["counts"][-1] == 1


# ---------------------------------------------------------------- 4. histograms
@pytest.mark.parametrize("interval, offset", [(1, 0), (5, 3), (1000, 7)])
def test_histogram_intervals_offsets_and_a_gap(flat, interval, offset):
    rng = np.random.default_rng(11)
    half = interval * 40
    col = np.where(rng.random(N) < 0.5, rng.integers(-3 * half, -2 * half, N), rng.integers(half, 2 * half, N)).astype(np.int64)
    col[rng.random(N) < 0.1] = NONE            # negative and positive values, an empty stretch of ~120 buckets in the middle
    _tmp(flat, col)
    for pred in PREDS[:2]:
        got, _ = _check(flat, pred, [(TMP, "histogram", interval, offset), (YEAR, "histogram", 5, 1)], routes=[DENSE, DENSE])
        assert np.any(got["aggs"][0]["counts"] == 0) and got["aggs"][0]["keys"][0] < 0 < got["aggs"][0]["keys"][-1]
    _check(flat, PREDS[3], [(TMP, "histogram", interval, offset)], routes=[NONE_ROUTE])


def _refused(pair, pred, aggs, **kw):
    from semantic_query_engine_amd._native import SqeError
    idx, model = pair
    with pytest.raises(A.TooManyBuckets) as want:
        A.aggregate(model, pred, aggs, **kw)
    with pytest.raises(SqeError) as e:
        idx.aggregate_fields(pred, aggs, **kw)
    assert e.value.code == -1 and str(want.value.n_buckets) in str(e.value)
    return want.value.result


def test_histogram_bucket_limits(flat):
    from semantic_query_engine_amd.engine import AGG_DTYPE, AGG_RESULT_DTYPE, pack_aggs
    idx, model = flat
    got, _ = _check(flat, [], [(YEAR, "histogram", 1, 0)], bucket_cap=35)                # n_buckets == bucket_cap passes
    assert got["aggs"][0]["n_buckets"] == 35
    want = _refused(flat, [], [(YEAR, "stats"), (YEAR, "histogram", 1, 0)], bucket_cap=34)
    # the refusal leaves the stats and the bucket count valid and writes no bucket
    packed = pack_aggs([(YEAR, "stats"), (YEAR, "histogram", 1, 0)])
    assert packed.dtype == AGG_DTYPE
    res = np.zeros(2, AGG_RESULT_DTYPE)
    keys, counts, sel = np.full((2, 34), 77, np.int64), np.full((2, 34), 77, np.int64), C.c_int64(-5)
    rc = idx.lib.sqe_index_aggregate_fields(idx.handle, None, 0, None, 0, None, -1, packed.ctypes.data, 2, 34, C.byref(sel), res.ctypes.data,
                                            keys.ctypes.data, counts.ctypes.data)
    assert rc == -1 and sel.value == N and np.all(keys == 77) and np.all(counts == 77)
    for j in range(2):
        assert (res[j]["count"], res[j]["min"], res[j]["max"]) == (want["aggs"][j]["count"], want["aggs"][j]["min"], want["aggs"][j]["max"])
    assert res[1]["n_buckets"] == 35 and res[0]["n_buckets"] == 0
    col = np.full(N, NONE, np.int64)
    col[[1, 50_000]] = [-10, -10 + 16383]
    _tmp(flat, col)
    got, last = _check(flat, [], [(TMP, "histogram", 1, 0)], routes=[DENSE])               # 16,384 buckets pass
    assert got["aggs"][0]["n_buckets"] == 16384 and last[0]["span"] == 16384
    col[50_000] += 1
    _tmp(flat, col)
    _refused(flat, [], [(TMP, "histogram", 1, 0)])                                       # 16,385 do not
    _check(flat, [], [(TMP, "histogram", 2, 1)], routes=[DENSE])
    col[[1, 50_000]] = [NONE + 1, I64_MAX]                                               # the widest span there is: nothing wraps
    _tmp(flat, col)
    _refused(flat, [], [(TMP, "histogram", 1, 0)])
    _refused(flat, [], [(TMP, "histogram", 1 << 40, 12345)])
    _check(flat, [], [(TMP, "histogram", 1 << 62, (1 << 62) - 1)], routes=[DENSE])


# ---------------------------------------------------------------- 5. the row set
def test_allow_list_and_predicate(flat):
    idx, model = flat
    rng = np.random.default_rng(12)
    allow = rng.integers(-10, N + 10, 20_000).astype(np.int64)        # repeats, and ids that name no live row
    aggs = [(YEAR, "terms", 10), (SCORE, "stats"), (POS, "terms", 4), (CODE, "histogram", 100, 50)]
    for pred in PREDS[:3]:
        got, _ = _check(flat, pred, aggs, filter_ids=allow, routes=[DENSE, NONE_ROUTE, HASH, DENSE])
        assert 0 < got["selected"] < np.unique(allow).size
    got, _ = _check(flat, [], aggs, filter_ids=np.empty(0, np.int64), routes=[NONE_ROUTE] * 4)       # an empty list selects nothing
    assert got["selected"] == 0 and all(g["count"] == 0 and g["keys"].size == 0 for g in got["aggs"])
    _check(flat, [], aggs, filter_ids=[N, N + 5, -1], routes=[NONE_ROUTE] * 4)                      # no id is live
    for pred in PREDS:
        assert idx.aggregate_fields(pred, [(YEAR, "stats")])["selected"] == int(idx.count_fields([pred])[0])


# ---------------------------------------------------------------- 6. mutations, an index without fields, IVF
def test_after_delete_and_add_the_answers_follow(ctx, data):
    pair = _make(ctx, data)
    idx, model = pair
    aggs = [(YEAR, "terms", 10), (POS, "terms", 5), (SCORE, "stats"), (CODE, "histogram", 7, 2), (BIG, "stats")]
    gone = np.concatenate([np.arange(32_700, 32_800), [0, 5, N - 1]]).astype(np.int64)       # across the bitmap block boundary
    idx.delete(gone)
    model.delete(gone)
    for pred in PREDS[:2]:
        _check(pair, pred, aggs)
    idx.add(data["x"][:300])
    model.add(300)
    new = np.arange(N, N + 300, dtype=np.int64)
    for f in (YEAR, POS):
        idx.set_field(f, new, data["cols"][f][:300] + 7)
        model.set_field(f, new, data["cols"][f][:300] + 7)
    for pred in PREDS[:2]:
        got, _ = _check(pair, pred, aggs, filter_ids=np.arange(100, N + 300))
    _check(pair, [], aggs)


def test_index_without_fields_answers_zeros_and_allocates_no_column(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, DIM)
    aggs = [(YEAR, "stats"), (YEAR, "terms", 10), (CODE, "histogram", 5, 0)]
    empty = idx.aggregate_fields([], aggs)                           # an empty index
    assert empty["selected"] == 0 and all(g["count"] == 0 and g["n_buckets"] == 0 and g["keys"].size == 0 for g in empty["aggs"])
    idx.add(data["x"][:5000])
    got, _ = _check((idx, FieldModel(5000)), [], aggs, routes=[NONE_ROUTE] * 3)
    assert got["selected"] == 5000 and got["aggs"][0]["min"] == I64_MAX and got["aggs"][0]["max"] == NONE
    assert idx.field_info() == {"fields": 0, "device_bytes": 0}


def test_ivf_index_gives_the_flat_answers(ctx, data, flat):
    ivf = _make(ctx, data, "ivf")
    aggs = [(YEAR, "terms", 10), (POS, "terms", 5), (SCORE, "stats"), (CODE, "histogram", 7, 2), (CODE, "terms", 256)]
    allow = np.arange(0, N, 3)
    for pred in PREDS[:3]:
        got, _ = _check(ivf, pred, aggs, filter_ids=allow, routes=[DENSE, HASH, NONE_ROUTE, DENSE, DENSE])
        assert A.same(got, flat[0].aggregate_fields(pred, aggs, filter_ids=allow))


def test_device_group_of_three_shards_answers_as_the_single_index(data, flat):
    """logical shards on one device, as tests/test_group_gpu.py builds them: STATS, HISTOGRAM and TERMS by both routes, under
    predicates and a routed allow-list, after a delete, against the model and the single index"""
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    from semantic_query_engine_amd._native import SqeError
    single, _ = flat
    grp = VectorIndex(Context(devices=[0, 0, 0], exchange=EXCHANGE_COPY), DIM)
    grp.add(data["x"])
    model = FieldModel(N)
    for f, col in data["cols"].items():
        if f != POS:
            grp.set_field(f, ALL_IDS, col)
            model.set_field(f, ALL_IDS, col)
    # the positions in runs of four: 17,501 distinct values, so that no shard holds more than 65,536 of them
    grp.set_field(POS, ALL_IDS, ALL_IDS // 4)
    model.set_field(POS, ALL_IDS, ALL_IDS // 4)
    aggs = [(YEAR, "stats"), (SCORE, "stats"), (BIG, "stats"), (UNSET, "stats"), (YEAR, "terms", 10), (CODE, "terms", 256),
            (POS, "terms", 7), (SCORE, "terms", 5)]                  # dense, dense, hash (ties decide), hash (30 % missing)
    hists = [(YEAR, "histogram", 5, 1), (CODE, "histogram", 100, 50), (SCORE, "histogram", 1 << 30, 12345), (FLAG, "terms", 2)]
    allow = np.random.default_rng(13).integers(-10, N + 10, 20_000).astype(np.int64)

    def check(pred, some, **kw):
        got = grp.aggregate_fields(pred, some, **kw)
        assert A.same(got, A.aggregate(model, pred, some, **kw)), (pred, kw)
        return got

    for pred in PREDS:
        g1, g2 = check(pred, aggs), check(pred, hists)
        s1 = single.aggregate_fields(pred, aggs[:6] + aggs[7:])         # (the single index's POS column differs: the other seven)
        assert A.same({"selected": g1["selected"], "aggs": g1["aggs"][:6] + g1["aggs"][7:]}, s1)
        assert A.same(g2, single.aggregate_fields(pred, hists))
    for pred in PREDS[:2]:
        check(pred, aggs, filter_ids=allow)
        check(pred, hists, filter_ids=allow)
    assert check([], aggs, filter_ids=np.empty(0, np.int64))["selected"] == 0
    gone = np.concatenate([np.arange(32_700, 32_800), [0, 5, N - 1]]).astype(np.int64)
    grp.delete(gone)
    model.delete(gone)
    check(PREDS[1], aggs)
    check([], hists, filter_ids=allow)
    # the refusals are the single index's, stats still valid; the record is single-device only
    with pytest.raises(A.TooManyBuckets) as want:
        A.aggregate(model, [], [(SCORE, "histogram", 1 << 20, 0)])
    with pytest.raises(SqeError) as e:
        grp.aggregate_fields([], [(SCORE, "histogram", 1 << 20, 0)])
    assert e.value.code == -1 and str(want.value.n_buckets) in str(e.value)
    with pytest.raises(SqeError) as e:
        grp.aggregate_last()
    assert e.value.code == -5


# ---------------------------------------------------------------- 7. refusals
def test_every_refusal_leaves_the_buffers_untouched(flat):
    from semantic_query_engine_amd.engine import AGG_DTYPE, AGG_RESULT_DTYPE, FIELD_DTYPE
    idx, _ = flat
    ok_agg = [(1, YEAR, 10, 0, 0, 0)]
    ok_clause = [(YEAR, 0, 2000, 2010)]

    def call(clauses=ok_clause, n_clauses=None, sets=(), n_set=None, allow=None, n_allow=-1, aggs=ok_agg, n_aggs=None, cap=16,
             null=()):
        cl = np.array(clauses, dtype=FIELD_DTYPE)
        sv = np.array(sets, np.int64)
        ag = np.array(aggs, dtype=AGG_DTYPE)
        al = None if allow is None else np.array(allow, np.int64)
        res = np.full(8, 77, AGG_RESULT_DTYPE)
        keys, counts, sel = np.full((8, 16), 77, np.int64), np.full((8, 16), 77, np.int64), C.c_int64(77)
        ptr = {"sel": C.byref(sel), "res": res.ctypes.data, "keys": keys.ctypes.data, "counts": counts.ctypes.data, "aggs": ag.ctypes.data}
        for name in null:
            ptr[name] = None
        rc = idx.lib.sqe_index_aggregate_fields(idx.handle, cl.ctypes.data, len(clauses) if n_clauses is None else n_clauses, sv.ctypes.data,
                                                len(sets) if n_set is None else n_set, None if al is None else al.ctypes.data, n_allow,
                                                ptr["aggs"], len(aggs) if n_aggs is None else n_aggs, cap, ptr["sel"], ptr["res"],
                                                ptr["keys"], ptr["counts"])
        untouched = sel.value == 77 and np.all(keys == 77) and np.all(counts == 77) and all(np.all(res[n] == 77) for n in res.dtype.names)
        return rc, untouched

    assert call() == (0, False)                                       # the well-formed call the cases below break one way each
    bad = [
        dict(n_clauses=9), dict(n_clauses=-1), dict(clauses=[(8, 0, 0, 1)]), dict(clauses=[(0, 7, 0, 1)]),      # clauses
        dict(clauses=[(0, 1, 0, 2)], sets=[5, 5]), dict(clauses=[(0, 1, 0, 3)], sets=[1, 2]), dict(n_set=4097),
        dict(n_allow=-2), dict(n_allow=3, allow=None),                                                        # lists
        dict(n_aggs=0), dict(n_aggs=9, aggs=ok_agg * 9), dict(null=("aggs",)),
        dict(aggs=[(3, YEAR, 10, 0, 0, 0)]), dict(aggs=[(-1, YEAR, 10, 0, 0, 0)]),                            # kind
        dict(aggs=[(0, 8, 0, 0, 0, 0)]), dict(aggs=[(1, -1, 10, 0, 0, 0)]),                                   # slot
        dict(aggs=[(1, YEAR, 0, 0, 0, 0)]), dict(aggs=[(1, YEAR, 257, 0, 0, 0)]), dict(aggs=[(1, YEAR, 17, 0, 0, 0)]),      # size
        dict(aggs=[(2, YEAR, 0, 0, 0, 0)]), dict(aggs=[(2, YEAR, 0, 0, 5, 5)]), dict(aggs=[(2, YEAR, 0, 0, 5, -1)]),      # interval, offset
        dict(cap=-1), dict(null=("sel",)), dict(null=("res",)), dict(null=("keys",)), dict(null=("counts",)),
        dict(aggs=ok_agg + [(2, YEAR, 0, 0, 0, 0)]),                                                          # the second one is bad
    ]
    for kw in bad:
        assert call(**kw) == (-1, True), kw
    assert idx.lib.sqe_index_aggregate_fields(None, None, 0, None, 0, None, -1, None, 1, 0, None, None, None, None) == -1
    assert idx.lib.sqe_index_aggregate_last(idx.handle, None) == -1


def test_aggregate_last_needs_a_call(ctx):
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd._native import SqeError
    with pytest.raises(SqeError):
        VectorIndex(ctx, DIM).aggregate_last()
