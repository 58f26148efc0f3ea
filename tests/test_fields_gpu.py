"""Numeric fields and field predicates on the GPU (csrc/fields.hip): sqe_index_set_field / get_field, sqe_index_match_fields,
sqe_index_search_where, sqe_index_search_where_each, against the NumPy model of tests/fields_reference.py and against the
filtered searches they must equal.  Everything is integers or reuses an existing search route: every comparison is bit for bit.
70,001 rows are two full 32,768-position bitmap blocks plus a partial one, and no multiple of 32 or 64.  GPU only."""
import ctypes as C
import filecmp

import numpy as np
import pytest

from tests.fields_reference import NONE, FieldModel

pytestmark = pytest.mark.gpu

N, DIM = 70_001, 64
YEAR, SCORE, CODE, POS, UNSET = 0, 1, 2, 3, 7       # field slots: dense, 30 % missing, keyword codes, the row's position, never set


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2015)
    x = rng.standard_normal((N, DIM)).astype(np.float32)
    q = rng.standard_normal((70, DIM)).astype(np.float32)
    q[:30] = x[rng.integers(0, N, 30)] + 0.1 * q[:30]
    year = rng.integers(1990, 2025, N).astype(np.int64)
    score = rng.integers(-(1 << 40), 1 << 40, N).astype(np.int64)
    score[rng.random(N) < 0.3] = NONE
    code = rng.integers(0, 3000, N).astype(np.int64)
    return {"x": x, "q": q, "cols": {YEAR: year, SCORE: score, CODE: code, POS: np.arange(N, dtype=np.int64)}}


def _fill(idx, model, cols, ids):
    for f, col in cols.items():
        idx.set_field(f, ids, col)
        model.set_field(f, ids, col)


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
    _fill(idx, model, data["cols"], np.arange(N, dtype=np.int64))
    return idx, model


@pytest.fixture(scope="module")
def flat(ctx, data):
    return _make(ctx, data)


@pytest.fixture(scope="module")
def ivf(ctx, data):
    return _make(ctx, data, "ivf")


IN_1024 = list(range(0, 3072, 3))
PREDS = [
    [(YEAR, "range", 2015, None)],
    [(YEAR, "range", None, 1999)],
    [(YEAR, "range", 2000, 2000)],
    [(CODE, "in", [17])],
    [(CODE, "in", IN_1024)],
    [(SCORE, "range", 0, None, {"not_": True})],                 # the rows without a score pass
    [(CODE, "in", IN_1024, {"not_": True})],
    [(YEAR, "range", 2010, 2020), (SCORE, "range", None, -1), (CODE, "in", [1, 5, 9, 2999], {"not_": True})],
    [],                                                          # every live row
    [(YEAR, "range", 2021, 2020)],                               # lo > hi: nothing
    [(YEAR, "range", 3000, None)],                               # nothing
    [(SCORE, "range", None, None)],                              # exists
    [(SCORE, "range", None, None, {"not_": True})],              # does not exist
    [(UNSET, "range", None, None)],                              # a slot never set holds for no row ...
    [(UNSET, "in", [1, 2], {"not_": True})],                     # ... and its negation for every row
    [(POS, "in", [0, 31, 32, 63, 64, 32767, 32768, N - 1])],
    [(POS, "range", 32760, 32775), (POS, "in", [32767, 32768, 40000])],
    [(SCORE, "in", [NONE])],                                     # a missing value is no value: nothing
]


def _check_match(idx, model, preds, cap):
    counts, ids = idx.match_fields(preds, cap)
    want_counts, want_ids = model.match(preds, cap)
    print("counts", counts.tolist())
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(ids, want_ids)


def _raw_match(idx, clauses, offsets, n_preds, sets, n_set, cap, counts, ids):
    from semantic_query_engine_amd.engine import FIELD_DTYPE
    clauses = np.array(clauses, dtype=FIELD_DTYPE)
    offsets = np.array(offsets, np.int64)
    sets = np.array(sets, np.int64)
    return idx.lib.sqe_index_match_fields(idx.handle, clauses.ctypes.data, offsets.ctypes.data, n_preds, sets.ctypes.data, n_set, cap,
                                          counts.ctypes.data, ids.ctypes.data)


# ---------------------------------------------------------------- 1. columns
def test_set_get_round_trip_and_refusals(flat, data):
    from semantic_query_engine_amd import VectorIndex  # noqa: F401
    from semantic_query_engine_amd._native import SqeError
    idx, model = flat
    all_ids = np.arange(N, dtype=np.int64)
    for f, col in data["cols"].items():
        assert np.array_equal(idx.get_field(f, all_ids), col)
    pick = np.array([N - 1, 0, 32768, 32767, 5], np.int64)
    assert np.array_equal(idx.get_field(SCORE, pick), data["cols"][SCORE][pick])
    assert np.all(idx.get_field(UNSET, pick) == NONE)                 # a slot never set
    assert np.all(idx.get_field(6, pick) == NONE)
    # a repeated id takes the last value; NONE removes one
    idx.set_field(5, [7, 9, 7, 11, 9], [1, 2, 3, 4, NONE])
    assert idx.get_field(5, [7, 9, 11, 8]).tolist() == [3, NONE, 4, NONE]
    before = idx.get_field(5, all_ids)
    for bad_ids, field in (([3, N, 4], 5), ([3, -1], 5), ([3], 8), ([3], -1)):
        with pytest.raises(SqeError) as e:
            idx.set_field(field, bad_ids, [99] * len(bad_ids))
        assert e.value.code == -1
    assert np.array_equal(idx.get_field(5, all_ids), before)          # nothing was written
    with pytest.raises(SqeError):
        idx.get_field(8, [0])
    with pytest.raises(SqeError):
        idx.get_field(0, [N])
    idx.set_field(5, all_ids[:12], np.full(12, NONE))                 # leave slot 5 empty for the other tests
    info = idx.field_info()
    assert info["fields"] == 5 and info["device_bytes"] >= 5 * 8 * N


# ---------------------------------------------------------------- 2. match_fields
def test_match_every_op_against_the_model(flat):
    idx, model = flat
    _check_match(idx, model, PREDS, 16)
    _check_match(idx, model, PREDS, N)               # every selected id
    assert np.array_equal(idx.count_fields(PREDS), model.match(PREDS, 0)[0])
    one = idx.match_fields([PREDS[15]], 10)
    assert one[0].tolist() == [8] and one[1][0].tolist() == [0, 31, 32, 63, 64, 32767, 32768, N - 1, -1, -1]


def test_match_64_predicates_in_one_call(flat):
    idx, model = flat
    rng = np.random.default_rng(64)
    preds = []
    for j in range(64):
        lo = int(rng.integers(1990, 2025))
        pred = [(YEAR, "range", lo, lo + int(rng.integers(0, 10)))]
        if j % 2:
            pred.append((CODE, "in", rng.integers(0, 3000, 60).tolist(), {"not_": bool(j % 4 == 1)}))
        if j % 3 == 0:
            pred.append((SCORE, "range", int(rng.integers(-(1 << 40), 0)), None, {"not_": bool(j % 2)}))
        preds.append(pred)
    _check_match(idx, model, preds, 100)
    _check_match(idx, model, preds[:63] + [[]], 3)


def test_match_invalid_tables_write_nothing(flat):
    idx, _ = flat
    rng = (0, 0, 0, 5)                                # a range clause on slot 0
    cases = {
        "65 predicates": ([rng] * 65, list(range(66)), 65, [0], 0, 4),
        "9 clauses": ([rng] * 9, [0, 9], 1, [0], 0, 4),
        "4097 set values": ([rng], [0, 1], 1, list(range(4097)), 4097, 4),
        "offsets start": ([rng, rng], [1, 2], 1, [0], 0, 4),
        "offsets decrease": ([rng, rng], [0, 2, 1], 2, [0], 0, 4),
        "slot 8": ([(8, 0, 0, 5)], [0, 1], 1, [0], 0, 4),
        "slot -1": ([(-1, 0, 0, 5)], [0, 1], 1, [0], 0, 4),
        "op 2": ([(0, 2, 0, 5)], [0, 1], 1, [0], 0, 4),
        "op 0x200": ([(0, 0x200, 0, 5)], [0, 1], 1, [0], 0, 4),
        "slice past the set": ([(0, 1, 0, 3)], [0, 1], 1, [1, 2], 2, 4),
        "slice negative": ([(0, 1, -1, 1)], [0, 1], 1, [1, 2], 2, 4),
        "slice reversed": ([(0, 1, 2, 1)], [0, 1], 1, [1, 2], 2, 4),
        "set equal": ([(0, 1, 0, 3)], [0, 1], 1, [1, 2, 2], 3, 4),
        "set descending": ([rng, (0, 1, 0, 2)], [0, 1, 2], 2, [2, 1], 2, 4),
        "cap < 0": ([rng], [0, 1], 1, [0], 0, -1),
        "n_preds < 0": ([rng], [0, 1], -1, [0], 0, 4),
    }
    for name, (clauses, offsets, n_preds, sets, n_set, cap) in cases.items():
        counts = np.full(80, 12345, np.int64)
        ids = np.full(80 * 4, 12345, np.int64)
        rc = _raw_match(idx, clauses, offsets, n_preds, sets, n_set, cap, counts, ids)
        assert rc == -1, name
        assert np.all(counts == 12345) and np.all(ids == 12345), name
    # and the valid neighbours pass: 64 predicates, 8 clauses, 4096 values
    counts = np.full(80, 12345, np.int64)
    ids = np.full(80 * 4, 12345, np.int64)
    assert _raw_match(idx, [rng] * 64, list(range(65)), 64, [0], 0, 4, counts, ids) == 0
    assert _raw_match(idx, [rng] * 8, [0, 8], 1, [0], 0, 4, counts, ids) == 0
    assert _raw_match(idx, [(2, 1, 0, 4096)], [0, 1], 1, list(range(4096)), 4096, 4, counts, ids) == 0
    assert counts[0] == N                              # every code lies in 0..2999


# ---------------------------------------------------------------- 3. growth, update, deletes, adds
@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_values_follow_their_rows(ctx, data, kind):
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd.engine import INDEX_IVF_FLAT
    x, cols = data["x"], data["cols"]
    if kind == "ivf":
        idx = VectorIndex(ctx, DIM, INDEX_IVF_FLAT, 16)
        idx.train(x[:4096], iters=4)
    else:
        idx = VectorIndex(ctx, DIM)
    model = FieldModel(0)
    n0 = 40_000
    idx.reserve(n0)
    idx.add(x[:n0])
    model.add(n0)
    first = np.arange(n0, dtype=np.int64)
    _fill(idx, model, {f: cols[f][:n0] for f in (YEAR, SCORE, CODE)}, first)
    idx.add(x[n0:])                                   # growth past the reserve
    model.add(N - n0)
    assert len(idx) == N
    assert np.array_equal(idx.get_field(YEAR, np.arange(N)), model.get_field(YEAR, np.arange(N)))       # new rows: no value
    rest = np.arange(n0, N, dtype=np.int64)
    _fill(idx, model, {f: cols[f][n0:] for f in (YEAR, SCORE)}, rest)        # CODE stays unset on the appended rows
    _fill(idx, model, {POS: cols[POS]}, np.arange(N, dtype=np.int64))        # a column allocated after the growth
    upd = np.array([0, 5, 32768, N - 1], np.int64)
    idx.update(upd, x[upd[::-1]].copy())              # vectors change, values stay
    rng = np.random.default_rng(3)
    dels = [np.concatenate([[0, N - 1], np.arange(32_760, 32_781), rng.choice(np.arange(100, 30_000), 300, replace=False)]),
            np.arange(1, 40)]                         # the first row, the last, a run across position 32,768; then the new first rows
    for d in dels:
        idx.delete(d)
        model.delete(d)
        idx.add(x[:200])
        model.add(200)
        new = model.ids[-200:]
        _fill(idx, model, {YEAR: np.arange(100, dtype=np.int64), CODE: np.full(100, 17, np.int64)}, new[::2])
    tail = model.ids[-5:]
    idx.delete(tail)                                  # the rows just added, the last row again
    model.delete(tail)
    live = idx.ids()
    assert np.array_equal(live, model.ids)
    for f in (YEAR, SCORE, CODE, POS, UNSET):
        assert np.array_equal(idx.get_field(f, live), model.get_field(f, live)), f
    preds = PREDS[:16] + [[(POS, "range", 32_700, 32_900)], [(YEAR, "range", 0, 199)]]
    _check_match(idx, model, preds, 50)
    _check_match(idx, model, preds, len(live))
    # the search sees the same rows
    sel = model.select(preds[0])
    want = idx.search(data["q"][:8], 10, filter_ids=sel)
    got = idx.search_where(data["q"][:8], 10, preds[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


# ---------------------------------------------------------------- 4. search_where
def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0])


@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_search_where_equals_the_filtered_search(flat, ivf, data, kind):
    idx, model = flat if kind == "flat" else ivf
    q, k = data["q"], 10
    for pred in (PREDS[0], PREDS[3], PREDS[7], PREDS[5], PREDS[8]):
        sel = model.select(pred)
        assert sel.size >= k
        _same(idx.search_where(q, k, pred), idx.search(q, k, filter_ids=sel))
    # with an allow-list: the intersection (the list holds repeats, dead and foreign ids)
    rng = np.random.default_rng(4)
    allow = np.concatenate([rng.integers(0, N, 20_000), [N, N + 5, -3, 0, 0, N - 1]]).astype(np.int64)
    sel = np.intersect1d(model.select(PREDS[0]), allow)
    _same(idx.search_where(q, k, PREDS[0], filter_ids=allow), idx.search(q, k, filter_ids=sel))
    cos, ids = idx.search_where(q, k, PREDS[0], filter_ids=np.empty(0, np.int64))
    assert np.all(ids == -1) and np.all(np.isneginf(cos))
    # no row at all: padding
    for pred in (PREDS[9], PREDS[13]):
        cos, ids = idx.search_where(q, k, pred)
        assert np.all(ids == -1) and np.all(np.isneginf(cos))
    # fewer than k rows
    sel = model.select(PREDS[15])
    assert sel.size == 8
    got = idx.search_where(q, k, PREDS[15])
    _same(got, idx.search(q, k, filter_ids=sel))
    assert np.all(got[1][:, 8:] == -1) and np.all(np.sort(got[1][:, :8], axis=1) == sel)
    # several gathered chunks merge
    idx.set_option("filter_gather_rows", 4096)
    try:
        for pred in (PREDS[0], PREDS[8]):
            _same(idx.search_where(q[:9], k, pred), idx.search(q[:9], k, filter_ids=model.select(pred)))
    finally:
        idx.set_option("filter_gather_rows", 1 << 20)
    _same(idx.search_where(q[:9], k, PREDS[0]), idx.search(q[:9], k, filter_ids=model.select(PREDS[0])))


def test_search_where_device_form(ctx, flat, data):
    import torch
    idx, model = flat
    q = torch.from_numpy(data["q"][:5]).cuda()
    cos = torch.empty((5, 10), dtype=torch.float32, device="cuda")
    ids = torch.empty((5, 10), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    idx.search_where_device(q.data_ptr(), 5, 10, PREDS[7], cos.data_ptr(), ids.data_ptr())
    ctx.synchronize()
    want = idx.search(data["q"][:5], 10, filter_ids=model.select(PREDS[7]))
    _same((cos.cpu().numpy(), ids.cpu().numpy()), want)
    counts = torch.empty(len(PREDS), dtype=torch.int64, device="cuda")
    out = torch.empty((len(PREDS), 7), dtype=torch.int64, device="cuda")
    idx.match_fields_device(PREDS, 7, counts.data_ptr(), out.data_ptr())
    ctx.synchronize()
    wc, wi = model.match(PREDS, 7)
    assert np.array_equal(counts.cpu().numpy(), wc) and np.array_equal(out.cpu().numpy(), wi)
    poq = np.arange(5, dtype=np.int32) % 3
    idx.search_where_each_device(q.data_ptr(), 5, 10, PREDS[:3], poq, cos.data_ptr(), ids.data_ptr())
    ctx.synchronize()
    _same((cos.cpu().numpy(), ids.cpu().numpy()), idx.search_filtered_each(data["q"][:5], 10, [model.select(p) for p in PREDS[:3]], poq))


# ---------------------------------------------------------------- 5. search_where_each
EACH_PREDS = [
    [(CODE, "in", [17, 18, 19])],                     # a short list: the direct route
    [(YEAR, "range", 2015, None)],                    # a long one: gathered
    [],                                               # the empty predicate: every row
    [(YEAR, "range", 1995, 1996)],                    # no query names this one
    [(YEAR, "range", 3000, None)],                    # selects nothing
]
EACH_OF_QUERY = np.array([(0, 1, 2, 4, 0, 0, 1)[b % 7] for b in range(70)], np.int32)


@pytest.mark.parametrize("direct_rows", [1 << 14, 0])
@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_search_where_each_equals_the_per_query_filtered_search(flat, ivf, data, kind, direct_rows):
    idx, model = flat if kind == "flat" else ivf
    q, k = data["q"], 10
    lists = [model.select(p) for p in EACH_PREDS]
    assert lists[0].size < 200 and lists[1].size > (1 << 14) and lists[2].size == N and lists[4].size == 0
    idx.set_option("filter_each_direct_rows", direct_rows)
    try:
        got = idx.search_where_each(q, k, EACH_PREDS, EACH_OF_QUERY)
        _same(got, idx.search_filtered_each(q, k, lists, EACH_OF_QUERY))
    finally:
        idx.set_option("filter_each_direct_rows", 1 << 14)
    assert np.all(got[1][EACH_OF_QUERY == 4] == -1)
    # one query, one predicate each
    _same(idx.search_where_each(q[:3], k, EACH_PREDS[:3]), idx.search_filtered_each(q[:3], k, lists[:3]))
    from semantic_query_engine_amd._native import SqeError
    with pytest.raises(SqeError):
        idx.search_where_each(q[:2], k, EACH_PREDS, [0, 5])


# ---------------------------------------------------------------- 6. device groups
def test_group_of_three_shards_answers_as_the_single_index(data):
    from semantic_query_engine_amd import Context, VectorIndex
    from semantic_query_engine_amd._native import SqeError
    from semantic_query_engine_amd.engine import EXCHANGE_COPY
    x, q, cols, k = data["x"], data["q"], data["cols"], 10
    sctx = Context(0)
    gctx = Context(devices=[0, 0, 0], exchange=EXCHANGE_COPY)
    single, group = VectorIndex(sctx, DIM), VectorIndex(gctx, DIM)
    model = FieldModel(N)
    all_ids = np.arange(N, dtype=np.int64)
    for idx in (single, group):
        idx.add(x)
        for f, col in cols.items():
            idx.set_field(f, all_ids, col)
        idx.set_field(5, [7, 9, 7, 11, 9], [1, 2, 3, 4, NONE])
    _fill(single, model, cols, all_ids)
    model.set_field(5, [7, 9, 7, 11, 9], [1, 2, 3, 4, NONE])
    with pytest.raises(SqeError):
        group.set_field(5, [3, N], [1, 1])
    with pytest.raises(SqeError):
        group.set_field(8, [3], [1])
    dels = np.concatenate([[0, N - 1], np.arange(32_760, 32_781)])
    for idx in (single, group, model):
        idx.delete(dels)
    live = model.ids
    assert np.array_equal(group.ids(), live)
    for f in (YEAR, SCORE, CODE, POS, 5, UNSET):
        assert np.array_equal(group.get_field(f, live), model.get_field(f, live)), f
    assert group.field_info()["fields"] == single.field_info()["fields"] == 5
    for cap in (0, 16, len(live)):
        gc, gi = group.match_fields(PREDS, cap)
        wc, wi = model.match(PREDS, cap)
        assert np.array_equal(gc, wc) and np.array_equal(gi, wi)
        sc, si = single.match_fields(PREDS, cap)
        assert np.array_equal(sc, wc) and np.array_equal(si, wi)
    for pred in (PREDS[0], PREDS[7], PREDS[15], PREDS[9]):
        _same(group.search_where(q, k, pred), single.search_where(q, k, pred))
        _same(group.search_where(q, k, pred), single.search(q, k, filter_ids=model.select(pred)))
    allow = np.random.default_rng(6).integers(0, N + 10, 20_000).astype(np.int64)
    _same(group.search_where(q, k, PREDS[0], filter_ids=allow), single.search_where(q, k, PREDS[0], filter_ids=allow))
    for direct_rows in (1 << 14, 0):
        for idx in (single, group):
            idx.set_option("filter_each_direct_rows", direct_rows)
        _same(group.search_where_each(q, k, EACH_PREDS, EACH_OF_QUERY), single.search_where_each(q, k, EACH_PREDS, EACH_OF_QUERY))
    _same(single.search_where_each(q, k, EACH_PREDS, EACH_OF_QUERY),
          single.search_filtered_each(q, k, [model.select(p) for p in EACH_PREDS], EACH_OF_QUERY))


# ---------------------------------------------------------------- 7. an index without fields is the index it was
def test_no_fields_no_bytes_and_the_same_file(ctx, data, tmp_path):
    from semantic_query_engine_amd import VectorIndex
    x = data["x"][:5000]
    plain, fielded = VectorIndex(ctx, DIM), VectorIndex(ctx, DIM)
    plain.add(x)
    fielded.add(x)
    assert plain.field_info() == {"fields": 0, "device_bytes": 0}
    plain.set_field(2, [1, 2], [NONE, NONE])          # removing what is not there allocates nothing
    assert plain.field_info() == {"fields": 0, "device_bytes": 0}
    fielded.set_field(0, np.arange(5000), np.arange(5000))
    fielded.set_field(4, [3], [9])
    assert fielded.field_info()["fields"] == 2
    plain.save(str(tmp_path / "plain.sqe"))
    fielded.save(str(tmp_path / "fielded.sqe"))
    assert filecmp.cmp(tmp_path / "plain.sqe", tmp_path / "fielded.sqe", shallow=False)
    loaded = VectorIndex.load(ctx, str(tmp_path / "fielded.sqe"))
    assert loaded.field_info() == {"fields": 0, "device_bytes": 0}
    assert np.all(loaded.get_field(0, [0, 1]) == NONE)


# ---------------------------------------------------------------- 8. end to end: the indexer and the shim
E2E_WORDS = ["aspirin", "fever", "pain", "gene", "cancer", "risk", "trial", "dose", "adult", "therapy", "tumor", "cohort"]


@pytest.fixture(scope="module")
def corpus():
    """2,000 chunks of 500 documents: a year each (one in nine without), a user, a few words, random vectors."""
    from oracle import wordpiece as WP
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    rng = np.random.default_rng(88)
    n = 2000
    docs = []
    for i in range(n):
        d = {"doc_id": f"d{i // 4}", "text": " ".join(rng.choice(E2E_WORDS, int(rng.integers(3, 8)))), "user_id": f"user{i % 13}"}
        if i % 9:
            d["year"] = int(2000 + (i * 7) % 24)
        docs.append(d)
    toks = WP.synthetic_vocab([" ".join(E2E_WORDS)], size=200)
    x = rng.standard_normal((n, DIM)).astype(np.float32)
    q = x[rng.integers(0, n, 13)] + 0.2 * rng.standard_normal((13, DIM)).astype(np.float32)
    return docs, x, q, WordPieceTokenizer(vocab_text="\n".join(toks) + "\n")


def _has_word(an, text, word):
    """`match` with operator and: every term of the query is a term of the document"""
    return set(an.query(word).tolist()) <= set(an.analyze([text])[0].tolist())


def _e2e_cases(an):
    year = lambda d: d.get("year")                            # noqa: E731
    return [
        ({"range": {"year": {"gte": 2015}}}, lambda d: year(d) is not None and year(d) >= 2015),
        ({"bool": {"filter": [{"range": {"year": {"gte": 2004, "lt": 2020}}}, {"term": {"doc_id": "d77"}}]}},
         lambda d: year(d) is not None and 2004 <= year(d) < 2020 and d["doc_id"] == "d77"),
        ({"bool": {"filter": [{"range": {"year": {"gte": 2004, "lt": 2020}}}, {"match": {"text": {"query": "gene", "operator": "and"}}}],
                   "must_not": [{"term": {"doc_id": "d3"}}]}},
         lambda d: year(d) is not None and 2004 <= year(d) < 2020 and _has_word(an, d["text"], "gene") and d["doc_id"] != "d3"),
        ({"bool": {"must_not": [{"exists": {"field": "year"}}], "filter": {"terms": {"user_id": ["user1", "user5", "nobody"]}}}},
         lambda d: year(d) is None and d["user_id"] in ("user1", "user5")),
    ]


def test_indexer_filters_equal_a_brute_force_selection(ctx, corpus):
    from semantic_query_engine_amd import retrieval as RT
    docs, x, q, tok = corpus
    client = RT.GpuSearchClient(ctx, dim=DIM)
    client.configure_fields("e2e", {"year": "long", "user_id": "keyword"})
    ix = RT.OpenSearchIndexer(client, "e2e")
    ix.add_embeddings(x[:1500], docs[:1500])
    RT.configure_analyzer(tok, max_len=64)
    try:
        an, idx = RT._analyzer, client.index("e2e")
        k = 10
        for n_docs in (1500, 2000):                           # the second round after an add: the new rows' values follow
            for flt, test in _e2e_cases(an):
                sel = np.array([i for i, d in enumerate(docs[:n_docs]) if test(d)], np.int64)
                assert sel.size > 0
                cos, ids = idx.vectors.search(q[:1], k, filter_ids=sel)
                hits = ix.search(q[:1], k, filter=flt)
                assert [(h["doc_id"], h["text"]) for h, _ in hits] == [(docs[i]["doc_id"], docs[i]["text"]) for i in ids[0] if i >= 0]
                assert [s for _, s in hits] == [float(1.0 / (2.0 - float(c))) for c, i in zip(cos[0], ids[0]) if i >= 0]
            # one term on user_id per query, in one call
            users = [f"user{b}" for b in range(12)] + ["nobody"]
            cos, ids = ix.search_batch(q, k, filters=[{"term": {"user_id": u}} for u in users])
            for b, u in enumerate(users):
                sel = np.array([i for i, d in enumerate(docs[:n_docs]) if d["user_id"] == u], np.int64)
                want = idx.vectors.search(q[b:b + 1], k, filter_ids=sel)
                assert np.array_equal(ids[b], want[1][0]) and np.array_equal(cos[b], want[0][0])
            ix.add_embeddings(x[1500:], docs[1500:])
        assert idx.vectors.field_info()["fields"] == 2
    finally:
        RT.configure_analyzer(None)


@pytest.mark.parametrize("per_query", [False, True])
def test_shim_knn_filter_equals_a_brute_force_selection(ctx, corpus, per_query):
    import json
    from fastapi.testclient import TestClient
    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim
    docs, x, q, tok = corpus
    RT.configure_analyzer(tok, max_len=64)
    try:
        an = RT._analyzer
        client = RT.GpuSearchClient(ctx, dim=DIM)
        with TestClient(shim.create_app(client, None, DIM, per_query_filters=per_query)) as c:
            props = {"year": {"type": "long"}, "user_id": {"type": "keyword"}, "embedding": {"type": "knn_vector", "dimension": DIM}}
            assert c.put("/e2e", json={"mappings": {"properties": props}}).status_code == 200
            lines = []
            for i, d in enumerate(docs):
                lines += [{"index": {"_index": "e2e", "_id": f"id{i}"}}, {**d, "embedding": x[i].tolist()}]
            r = c.post("/_bulk", content="\n".join(json.dumps(line) for line in lines) + "\n", headers={"content-type": "application/x-ndjson"})
            assert r.status_code == 200 and not r.json()["errors"]
            vectors = client.index("e2e").vectors
            cases = _e2e_cases(an) + [({"term": {"user_id": f"user{b}"}}, (lambda u: lambda d: d["user_id"] == u)(f"user{b}")) for b in range(3)]
            for j, (flt, test) in enumerate(cases):
                sel = np.array([i for i, d in enumerate(docs) if test(d)], np.int64)
                cos, ids = vectors.search(q[j:j + 1], 10, filter_ids=sel)
                body = {"size": 10, "query": {"knn": {"embedding": {"vector": q[j].tolist(), "k": 10, "filter": flt}}}}
                r = c.post("/e2e/_search", json=body)
                assert r.status_code == 200
                hits = r.json()["hits"]["hits"]
                assert [h["_id"] for h in hits] == [f"id{i}" for i in ids[0] if i >= 0] and hits
                assert [h["_score"] for h in hits] == [float(1.0 / (2.0 - float(cv))) for cv, i in zip(cos[0], ids[0]) if i >= 0]
            r = c.post("/e2e/_search", json={"size": 3, "query": {"knn": {"embedding": {"vector": q[0].tolist(), "k": 3, "filter": {"range": {"nope": {"gte": 1}}}}}}})
            assert r.status_code == 400
    finally:
        RT.configure_analyzer(None)
