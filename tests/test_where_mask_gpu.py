"""The mask route of sqe_index_search_where (csrc/where_mask.hip): the whole index searched at one depth, the hits masked by the
predicate's bitmap, the flagged queries swept.  Its answers are compared bit for bit with the gather route's and with the
filtered search over the ids the NumPy model of tests/fields_reference.py selects; the read-back (sqe_index_where_last) with what
the depth rule and a plain search of that depth predict.  70,001 rows are two full 32,768-position bitmap blocks plus a partial
one, and no multiple of 32 or 64.  GPU only."""
import numpy as np
import pytest

from tests.fields_reference import NONE, FieldModel

pytestmark = pytest.mark.gpu

N, DIM = 70_001, 64
YEAR, SCORE, CODE, POS = 0, 1, 2, 3                 # field slots: dense, 30 % missing, keyword codes, the row's position
GATHER, MASK = 1, 2                                 # "where_route" values = the routes where_last reports
EDGE_POSITIONS = [0, 31, 32, 63, 64, 32767, 32768, N - 1]
PREDS = {
    "range_29pct": [(YEAR, "range", 2015, None)],
    "three_clauses": [(YEAR, "range", 2010, 2020), (SCORE, "range", None, -1), (CODE, "in", [1, 5, 9, 2999], {"not_": True})],
    "negated_missing_pass": [(SCORE, "range", 0, None, {"not_": True})],
    "every_row": [],
    "no_row": [(YEAR, "range", 3000, None)],
    "edge_positions": [(POS, "in", EDGE_POSITIONS)],          # 8 rows: k = 10 and more end in padding
}
KS = (1, 10, 64, 100)
DEPTHS = (0, 63, 64, 65, 256)


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
    ids = np.arange(N, dtype=np.int64)
    for f, col in data["cols"].items():
        idx.set_field(f, ids, col)
        model.set_field(f, ids, col)
    return idx, model


@pytest.fixture(scope="module")
def flat(ctx, data):
    return _make(ctx, data)


@pytest.fixture(scope="module")
def deleted(ctx, data):
    """ids differ from positions: deletes across the boundary of the first bitmap block and at both ends"""
    idx, model = _make(ctx, data)
    dels = np.concatenate([[0, 1, N - 2, N - 1], np.arange(32_760, 32_781)])
    idx.delete(dels)
    model.delete(dels)
    return idx, model


def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


class Routed:
    """the index's routing options for the length of a block, the defaults afterwards"""

    def __init__(self, idx, route, depth=0):
        self.idx, self.route, self.depth = idx, route, depth

    def __enter__(self):
        self.idx.set_option("where_route", self.route)
        self.idx.set_option("where_mask_depth", self.depth)

    def __exit__(self, *exc):
        self.idx.set_option("where_route", 0)
        self.idx.set_option("where_mask_depth", 0)


def _expected_swept(idx, model, q, k, d, selected_ids):
    """the queries with fewer than k selected rows among their d nearest, unless those are all the rows there are"""
    live = len(model.ids)
    if d >= live:
        return 0
    _, near = idx.search(q, d)
    return int(np.count_nonzero(np.isin(near, selected_ids).sum(axis=1) < k))


def _three_routes(idx, model, q):
    from semantic_query_engine_amd.engine import where_depth
    live = len(model.ids)
    for name, pred in PREDS.items():
        sel = model.select(pred)
        for k in KS:
            want = idx.search(q, k, filter_ids=sel)
            with Routed(idx, GATHER):
                _same(idx.search_where(q, k, pred), want)
                last = idx.where_last()
                assert (last["route"], last["selected"], last["live"], last["depth"], last["swept"]) == \
                    (GATHER if len(sel) else 0, len(sel), live, 0, 0), (name, k, last)
            for depth in DEPTHS:
                with Routed(idx, MASK, depth):
                    got = idx.search_where(q, k, pred)
                    last = idx.where_last()
                print(f"[where mask] {name} k={k} where_mask_depth={depth}: {last}")
                _same(got, want)
                if len(sel) == 0:
                    assert (last["route"], last["selected"], last["depth"], last["swept"]) == (0, 0, 0, 0)
                    continue
                d = max(depth, k) if depth else (where_depth(k, len(sel), live) or 256)
                assert (last["route"], last["selected"], last["live"], last["depth"], last["first_pass_i8"]) == (MASK, len(sel), live, d, 0), \
                    (name, k, depth, last)
                assert last["swept"] == _expected_swept(idx, model, q, k, d, sel), (name, k, depth, last)
    assert np.all(idx.search_where(q, 10, PREDS["edge_positions"])[1][:, 8:] == -1)


# ---------------------------------------------------------------- 1. / 2. the three routes agree
def test_three_routes_agree_bit_for_bit(flat, data):
    _three_routes(flat[0], flat[1], data["q"])


def test_three_routes_agree_after_deletes(deleted, data):
    idx, model = deleted
    assert not np.array_equal(model.ids, np.arange(len(model.ids)))
    _three_routes(idx, model, data["q"])


# ---------------------------------------------------------------- 3. flagged queries
def test_flagged_queries_are_swept_and_exact(ctx):
    """3,000 rows within cosine 0.99 of four of the queries carry a year the predicate refuses; every other row is a random row
    below cosine 0.5 to those four queries, and the other queries are orthogonal to them.  The four queries find only refused
    rows at any depth up to 256 and are swept; nobody else is."""
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd.engine import where_depth
    rng = np.random.default_rng(33)
    n, near, k = 20_000, 3000, 10
    basis, _ = np.linalg.qr(rng.standard_normal((DIM, 4)))
    basis = basis.T                                               # four orthonormal query directions
    others = rng.standard_normal((n - near, DIM))
    high = ((others @ basis.T) / np.linalg.norm(others, axis=1, keepdims=True)).max(axis=1) > 0.45
    others[high] -= (others[high] @ basis.T) @ basis          # the few random rows that come near a query direction leave it
    close = np.repeat(basis, near // 4, axis=0) + 0.1 * rng.standard_normal((near, DIM)) / np.sqrt(DIM)
    cosines = np.einsum("ij,ij->i", close, np.repeat(basis, near // 4, axis=0)) / np.linalg.norm(close, axis=1)
    assert cosines.min() > 0.99
    order = rng.permutation(n)
    x = np.concatenate([close, others])[order].astype(np.float32)
    year = np.concatenate([np.full(near, 1990), np.full(n - near, 2010)])[order].astype(np.int64)
    q = rng.standard_normal((24, DIM))
    q -= (q @ basis.T) @ basis
    flagged = [2, 9, 16, 23]
    q[flagged] = basis
    q = q.astype(np.float32)
    unit = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    assert np.all((unit[year == 2010] @ basis.T.astype(np.float64)) < 0.5)
    idx = VectorIndex(ctx, DIM)
    idx.add(x)
    idx.set_field(YEAR, np.arange(n), year)
    pred = [(YEAR, "range", 2000, None)]
    sel = np.nonzero(year == 2010)[0]
    with Routed(idx, GATHER):
        want = idx.search_where(q, k, pred)
    _same(want, idx.search(q, k, filter_ids=sel))
    with Routed(idx, MASK):
        got = idx.search_where(q, k, pred)
        last = idx.where_last()
    print(f"[where mask] correlated predicate: {last}")
    assert last["route"] == MASK and last["depth"] == where_depth(k, n - near, n) and last["swept"] == 4
    _same(got, want)
    idx.close()


# ---------------------------------------------------------------- 4. the sweep halves a range
HEAD, RANDOM, TAIL = 300, 16_000, 5000
EPS_MAX = 0.005          # kernels.h scan_eps at K = 64 stays below this (tests/test_sweep_walk_gpu.py)


def test_sweep_halves_a_range(ctx):
    """300 refused copies of the query | 16,000 random rows | 5,000 selected copies.  Stage A at depth 10 finds refused rows only;
    the sweep fills its list from the random rows, doubles its range to 16,384 rows over them and then meets 4,916 copies of
    equal cosine in one range, more than the 4,096 keys a slot holds: the range is halved and collected again.  Ties go to the
    lowest id, so the answer is the first ten copies of the tail."""
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(7)
    v = rng.standard_normal(DIM)
    v /= np.linalg.norm(v)
    r = rng.standard_normal((RANDOM, DIM))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    assert (r @ v).max() < 1.0 - 4 * EPS_MAX
    x = np.concatenate([np.tile(v, (HEAD, 1)), r, np.tile(v, (TAIL, 1))]).astype(np.float32)
    v = v.astype(np.float32)
    n, k = len(x), 10
    idx = VectorIndex(ctx, DIM)
    idx.add(x)
    idx.set_field(YEAR, np.arange(n), np.concatenate([np.full(HEAD, 1990), np.full(RANDOM + TAIL, 2010)]))
    pred = [(YEAR, "range", 2000, None)]
    with Routed(idx, MASK, k):
        cos, ids = idx.search_where(v[None], k, pred)
        last = idx.where_last()
    assert (last["route"], last["depth"], last["swept"], last["selected"]) == (MASK, k, 1, RANDOM + TAIL)
    assert np.array_equal(ids[0], np.arange(HEAD + RANDOM, HEAD + RANDOM + k))
    _same((cos, ids), idx.search(v[None], k, filter_ids=np.arange(HEAD, n)))
    idx.close()


# ---------------------------------------------------------------- 5. allow-list AND predicate
def test_allow_list_and_predicate(deleted, data):
    idx, model = deleted
    q, k, pred = data["q"], 10, PREDS["range_29pct"]
    rng = np.random.default_rng(6)
    allow = rng.integers(0, N + 10, 40_000).astype(np.int64)        # repeats, deleted ids (0, 32,770, ...) and ids past the last
    allow[:6] = [0, 32_770, N - 1, N + 5, 17, 17]
    both = np.intersect1d(model.select(pred), allow)
    want = idx.search(q, k, filter_ids=both)
    for route in (GATHER, MASK):
        with Routed(idx, route):
            _same(idx.search_where(q, k, pred, filter_ids=allow), want)
            last = idx.where_last()
            assert last["route"] == route and last["selected"] == len(both)
            # zero clauses: the broad allow-list alone
            _same(idx.search_where(q, k, [], filter_ids=allow), idx.search(q, k, filter_ids=np.intersect1d(model.ids, allow)))
            cos, ids = idx.search_where(q, k, pred, filter_ids=np.zeros(0, np.int64))
            assert np.all(ids == -1) and np.all(np.isneginf(cos))
            assert idx.where_last()["route"] == 0 and idx.where_last()["selected"] == 0


# ---------------------------------------------------------------- 6. the device form on the caller's stream
def test_device_form_on_the_callers_stream(ctx, flat, data):
    import torch
    idx, model = flat
    pred, k, b = PREDS["three_clauses"], 10, 40
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream), Routed(idx, MASK):
            q = torch.from_numpy(data["q"][:b]).cuda().contiguous()
            cos = torch.empty((b, k), dtype=torch.float32, device="cuda")
            ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
            idx.search_where_device(q.data_ptr(), b, k, pred, cos.data_ptr(), ids.data_ptr())
            stream.synchronize()
            assert idx.where_last()["route"] == MASK
    finally:
        ctx.set_stream(0)
    _same((cos.cpu().numpy(), ids.cpu().numpy()), idx.search(data["q"][:b], k, filter_ids=model.select(pred)))


# ---------------------------------------------------------------- 7. device groups
def test_group_of_three_shards_equals_the_single_index(flat, data):
    from semantic_query_engine_amd import Context, VectorIndex
    from semantic_query_engine_amd._native import SqeError
    from semantic_query_engine_amd.engine import EXCHANGE_COPY
    single, model = flat
    q, k = data["q"], 10
    gctx = Context(devices=[0, 0, 0], exchange=EXCHANGE_COPY)
    group = VectorIndex(gctx, DIM)
    group.add(data["x"])
    ids = np.arange(N, dtype=np.int64)
    for f, col in data["cols"].items():
        group.set_field(f, ids, col)
    group.set_option("where_route", MASK)                      # forwarded to every shard, each of which routes for itself
    for name in ("range_29pct", "three_clauses", "edge_positions", "no_row"):
        pred = PREDS[name]
        _same(group.search_where(q, k, pred), single.search(q, k, filter_ids=model.select(pred)))
    allow = np.random.default_rng(6).integers(0, N + 10, 20_000).astype(np.int64)
    _same(group.search_where(q, k, PREDS["range_29pct"], filter_ids=allow),
          single.search(q, k, filter_ids=np.intersect1d(model.select(PREDS["range_29pct"]), allow)))
    with pytest.raises(SqeError):
        group.where_last()
    group.close()
    gctx.close()


# ---------------------------------------------------------------- 8. a large index: the int8 first pass stays on at a small depth
def test_large_index_keeps_the_int8_first_pass(ctx):
    """1,000,000 x 256, a 50 % predicate, forced mask: k = 3 runs at depth 18 through the int8 first pass (i8_last moves), k = 10
    at depth 38 through the bf16 scan.  A depth keeps the int8 pass while it is <= the place of the threshold sample, which is
    "i8_sample_m" = 20 as long as the sample has its 128 tiles; with the default "i8_sample_step" = 100 an index of 3,907 tiles
    samples more densely and at place 63 (search.hip: sample_plan), and depth 38 kept the int8 pass there (measured: first_pass_i8
    = 1 at depth 38), so the index samples every 30th tile here."""
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(12)
    n, d = 1_000_000, 256
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((64, d)).astype(np.float32)
    q[:32] = x[rng.integers(0, n, 32)] + 0.1 * q[:32]
    idx = VectorIndex(ctx, d)
    idx.set_option("i8_sample_step", 30)                             # 130 sampled tiles: the place stays at "i8_sample_m" = 20
    idx.add(x)
    half = (np.arange(n, dtype=np.int64) * 7919) % 2                 # alternating, so exactly 50 %
    idx.set_field(YEAR, np.arange(n), 2000 + half)
    pred = [(YEAR, "range", 2001, None)]
    sel = np.nonzero(half == 1)[0]
    idx.search(q[:1], 3)
    before = idx.i8_last()
    assert before["rows"] == n
    idx.set_option("where_route", MASK)
    for k, depth, i8 in ((3, 18, 1), (10, 38, 0)):
        got = idx.search_where(q, k, pred)
        last = idx.where_last()
        print(f"[where mask] 1 M x 256, 50 %, k={k}: {last}")
        assert (last["route"], last["selected"], last["live"], last["depth"], last["first_pass_i8"]) == (MASK, n // 2, n, depth, i8)
        if i8:
            after = idx.i8_last()
            assert after != before and after["B"] == 64 and after["k"] == depth
        _same(got, idx.search(q, k, filter_ids=sel))
    idx.close()


# ---------------------------------------------------------------- 9. where auto never masks
def test_auto_stays_with_gather(ctx, flat, data):
    from semantic_query_engine_amd.engine import where_depth
    idx, model = flat
    q, k = data["q"], 10
    broad, sel = PREDS["every_row"], model.ids

    def gathers(pred, kk, ids):
        _same(idx.search_where(q, kk, pred), idx.search(q, kk, filter_ids=ids))
        last = idx.where_last()
        assert last["route"] == GATHER and last["depth"] == 0 and last["selected"] == len(ids), last

    # the control: with the floor out of the way the same broad predicate takes the mask route under auto
    idx.set_option("where_mask_min_rows", 0)
    try:
        _same(idx.search_where(q, k, broad), idx.search(q, k, filter_ids=sel))
        assert idx.where_last()["route"] == MASK and idx.where_last()["depth"] == k
        idx.set_option("certify", 0)
        try:
            gathers(broad, k, sel)
        finally:
            idx.set_option("certify", 1)
        narrow = PREDS["edge_positions"]                              # 8 < k rows: the rule has no depth
        assert where_depth(k, 8, N) == 0
        gathers(narrow, k, model.select(narrow))
        tenth = [(CODE, "range", 0, 299)]                             # ~10 % of the rows, k = 64: no depth up to 256
        assert where_depth(64, len(model.select(tenth)), N) == 0
        gathers(tenth, 64, model.select(tenth))
        idx.set_option("where_mask_min_rows", N + 1)
        gathers(broad, k, sel)
    finally:
        idx.set_option("where_mask_min_rows", 1_000_000)


def test_ivf_always_gathers(ctx, data):
    idx, model = _make(ctx, data, "ivf")
    q, k, pred = data["q"], 10, PREDS["range_29pct"]
    with Routed(idx, MASK):
        _same(idx.search_where(q, k, pred), idx.search(q, k, filter_ids=model.select(pred)))
        assert idx.where_last()["route"] == GATHER
    idx.close()


def test_option_ranges_and_read_back_refusals(ctx, flat):
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd._native import SqeError
    idx = flat[0]
    for key, bad in (("where_route", 3), ("where_route", -1), ("where_mask_depth", 257), ("where_mask_depth", -1), ("where_mask_min_rows", -1)):
        with pytest.raises(SqeError):
            idx.set_option(key, bad)
    with pytest.raises(SqeError):
        VectorIndex(ctx, DIM).where_last()
    assert idx.lib.sqe_index_where_last(idx.handle, None) == -1
