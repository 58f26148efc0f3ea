"""Every consumer of a row set sees the same set (csrc/rowset.hip: rowset_map, rowset_positions).  A row set is the live rows a
field predicate selects, intersected with an optional allow-list; sqe_index_search_where, sqe_index_aggregate_fields,
sqe_index_sort_fields and the _where forms of radial and collapsed search all prepare it through the same two functions.  For
each set the expected ids S come from numpy, and every call must report exactly len(S) rows (and the sort exactly S's first
ids).  Two single indexes (701 rows; 33,001 rows: two 1,024-word blocks of the map, a partial last word) and a three-shard
logical group.  Everything is an integer: no tolerance.  GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 64
ID, YEAR = 0, 1                        # field slots: the row's id, a year with some values missing
NONE = -(1 << 63)
NQ, K = 3, 10


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _data(seed, n, dels):
    rng = np.random.default_rng(seed)
    year = rng.integers(2000, 2021, n).astype(np.int64)
    year[rng.random(n) < 0.1] = NONE
    return {"x": rng.standard_normal((n, DIM)).astype(np.float32), "q": rng.standard_normal((NQ, DIM)).astype(np.float32),
            "keys": (np.arange(n, dtype=np.int64) // 3) * 7 + 5, "year": year, "dels": np.asarray(dels, np.int64), "rng": rng}


def _build(ctx, d):
    from semantic_query_engine_amd import VectorIndex
    n = d["x"].shape[0]
    idx = VectorIndex(ctx, DIM)
    idx.add(d["x"])
    ids = np.arange(n, dtype=np.int64)
    idx.set_keys(ids, d["keys"])
    idx.set_field(ID, ids, ids)
    idx.set_field(YEAR, ids, d["year"])
    idx.delete(d["dels"])              # first of all: ids are not positions
    return idx


def _sets(d):
    """name -> (pred, filter_ids, S ascending)"""
    n, rng = d["x"].shape[0], d["rng"]
    live = np.setdiff1d(np.arange(n, dtype=np.int64), d["dels"])
    y = d["year"][live]
    since = live[(y != NONE) & (y >= 2009)]
    picked = live[rng.random(len(live)) < 0.4]
    # shuffled, with repeats, a deleted id and an id never given
    listed = rng.permutation(np.concatenate([picked, picked[:7], d["dels"][:1], np.array([n + 50], np.int64)]))
    p_since, p_none = [(YEAR, "range", 2009, None)], [(YEAR, "range", 3000, None)]
    return {"pred": (p_since, None, since),
            "list": ([], listed, picked),
            "both": (p_since, listed, np.intersect1d(since, picked)),
            "all_live": ([], None, live),
            "pred_selects_nothing": (p_none, None, live[:0]),
            "empty_list": (p_since, np.zeros(0, np.int64), live[:0])}


@pytest.fixture(scope="module", params=[(701, [3, 100, 650]), (33004, [0, 1023 * 32 + 5, 33003])], ids=["701", "33001"])
def world(ctx, request):
    n, dels = request.param
    d = _data(11 + n, n, dels)
    idx = _build(ctx, d)
    assert len(idx) == n - 3 and len(idx) % 32 != 0
    return {"d": d, "idx": idx, "sets": _sets(d)}


def _check_counts(idx, q, pred, allow, S, what):
    agg = idx.aggregate_fields(pred, [(ID, "stats")], filter_ids=allow)
    assert agg["selected"] == len(S), what
    srt = idx.sort_fields(pred, [(ID, "asc")], 16, filter_ids=allow)
    assert srt["total"] == len(S), what
    assert srt["ids"].tolist() == S[:16].tolist(), what
    _cos, ids = idx.search_where(q, K, pred, filter_ids=allow)
    assert np.isin(ids[ids >= 0], S).all() and np.count_nonzero(ids[0] >= 0) == min(K, len(S)), what
    counts, _cos, _ids = idx.range_search(q, -2.0, 4, pred=pred, filter_ids=allow)      # below every cosine: the size of the set
    assert counts.tolist() == [len(S)] * q.shape[0], what


@pytest.mark.parametrize("name", ["pred", "list", "both", "all_live", "pred_selects_nothing", "empty_list"])
def test_every_consumer_sees_the_same_set(world, name):
    idx, q = world["idx"], world["d"]["q"]
    pred, allow, S = world["sets"][name]
    assert (len(S) == 0) == (name in ("pred_selects_nothing", "empty_list"))
    _check_counts(idx, q, pred, allow, S, name)
    assert idx.within_last()["selected"] == len(S)                  # the radial call just made
    idx.search_where(q, K, pred, filter_ids=allow)
    assert idx.where_last()["selected"] == len(S)
    idx.search_collapsed(q, K, pred=pred, filter_ids=allow)
    assert idx.within_last()["selected"] == len(S)
    if allow is None:
        assert idx.count_fields([pred]).tolist() == [len(S)]


def test_a_logical_group_sees_the_same_sets():
    from semantic_query_engine_amd import EXCHANGE_COPY, Context
    d = _data(11 + 701, 701, [3, 100, 650])
    grp = _build(Context(devices=[0] * 3, exchange=EXCHANGE_COPY), d)
    for name, (pred, allow, S) in _sets(d).items():
        _check_counts(grp, d["q"], pred, allow, S, name)
