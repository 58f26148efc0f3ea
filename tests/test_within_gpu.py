"""Radial, collapsed and MMR search within a row set (csrc/within.hip: sqe_index_range_search_where, _search_collapsed_where,
_search_mmr_where).  The oracle of every case is the existing UNRESTRICTED call on a second index built from the same arrays in
the same order, with the same keys, from which every row outside the row set S was deleted (sqe_index_delete keeps ids stable):
ids, cosines, keys, counts and MMR scores are compared on their raw bits.  "filter_gather_rows" is 256 throughout, so a set of
300 or more rows takes the mask route and one of about 200 the gather route; every case reads the route back
(sqe_index_within_last).  GPU only."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM = 701, 64                       # no multiple of 32
ID, YEAR = 0, 1                        # field slots: the row's id, a year with some values missing
NONE = -(1 << 63)
GATHER, MASK = 1, 2                    # the routes within_last reports
RADIAL, COLLAPSED, MMR = 1, 2, 3       # its kinds
DELETED = [3, 100, 650]                # deleted before anything else: ids are not positions
GATHER_ROWS = 256


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _data(seed, n):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, DIM)).astype(np.float32)
    x[200] = x[101]                                       # equal cosines: ties go to the lowest id on every route
    q = rng.standard_normal((9, DIM)).astype(np.float32)
    q[:5] = x[rng.integers(0, n, 5)] + 0.3 * q[:5]
    keys = (np.arange(n, dtype=np.int64) // 3) * 7 + 5    # at most 3 rows a key: the top 256 of any set hold >= 64 groups
    keys[rng.random(n) < 0.05] = NONE
    year = rng.integers(2000, 2021, n).astype(np.int64)
    year[rng.random(n) < 0.1] = NONE
    return {"x": x, "q": q, "keys": keys, "year": year, "rng": rng}


def _build(ctx, d, keys=True, kind="flat", dels=DELETED, fields=True):
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd.engine import INDEX_IVF_FLAT
    n = d["x"].shape[0]
    if kind == "ivf":
        idx = VectorIndex(ctx, DIM, INDEX_IVF_FLAT, 8)
        idx.train(d["x"], iters=4, seed=1)
    else:
        idx = VectorIndex(ctx, DIM)
    idx.add(d["x"])
    ids = np.arange(n, dtype=np.int64)
    if keys:
        idx.set_keys(ids, d["keys"])
    if fields:
        idx.set_field(ID, ids, ids)
        idx.set_field(YEAR, ids, d["year"])
    if len(dels):
        idx.delete(np.asarray(dels, np.int64))
    idx.set_option("filter_gather_rows", GATHER_ROWS)
    return idx


def _live(d, dels=DELETED):
    return np.setdiff1d(np.arange(d["x"].shape[0], dtype=np.int64), np.asarray(dels, np.int64))


def _oracle(ctx, d, S, keys=True, kind="flat", dels=DELETED):
    """the index with every row outside S deleted"""
    idx = _build(ctx, d, keys=keys, kind=kind, dels=dels, fields=False)
    out = np.setdiff1d(_live(d, dels), S)
    if len(out):
        idx.delete(out)
    assert len(idx) == len(S)
    return idx


def _year_rows(d, live, lo, hi=None):
    y = d["year"][live]
    m = (y != NONE) & (y >= lo)
    if hi is not None:
        m &= y <= hi
    return live[m]


@pytest.fixture(scope="module")
def world(ctx):
    """the 701-row index, its row sets (name -> (pred, filter_ids, S, route)) and one oracle per set, built once"""
    d = _data(7, N)
    live = _live(d)
    edge = live[[0, 31, 32, 63, 64, len(live) - 1]]
    d["year"][edge[[0, 2, 4]]] = 2015                      # positions 0, 32, 64 pass every year range below ...
    d["year"][edge[[1, 3, 5]]] = 2001                      # ... positions 31, 63, n - 1 none of them
    rng = d["rng"]
    idx = _build(ctx, d)

    def listed(S, extra):
        """an allow-list for S: shuffled, with repeats, a deleted id and an id that was never given"""
        ids = np.concatenate([S, S[:5], np.asarray(extra, np.int64), np.array([DELETED[0], N + 50], np.int64)])
        return rng.permutation(ids)

    pick = lambda frac: live[rng.random(len(live)) < frac]
    sets = {}
    p_wide, p_mid, p_narrow = [(YEAR, "range", 2004, None)], [(YEAR, "range", 2009, None)], [(YEAR, "range", 2015, 2020)]
    sets["mask_pred"] = (p_mid, None, _year_rows(d, live, 2009))
    sets["gather_pred"] = (p_narrow, None, _year_rows(d, live, 2015, 2020))
    big = np.union1d(np.setdiff1d(pick(0.5), edge), edge[[1, 3, 5]])       # the list side takes the OTHER edge positions
    sets["mask_list"] = ([], listed(big, []), big)
    small = np.union1d(np.setdiff1d(pick(0.28), edge), edge[[1, 3]])
    sets["gather_list"] = ([], listed(small, []), small)
    wide = _year_rows(d, live, 2004)
    both = np.union1d(np.setdiff1d(wide[rng.random(len(wide)) < 0.7], edge), edge[[0, 4]])
    sets["mask_both"] = (p_wide, listed(both, np.setdiff1d(live, wide)[:40]), both)
    mid = _year_rows(d, live, 2009)
    both2 = np.union1d(np.setdiff1d(mid[rng.random(len(mid)) < 0.55], edge), edge[[2]])
    sets["gather_both"] = (p_mid, listed(both2, np.setdiff1d(live, mid)[:40]), both2)
    two = wide[wide % 5 != 0]
    sets["mask_two_clauses"] = (p_wide + [(ID, "in", live[live % 5 == 0], {"not_": True})], None, two)
    tiny = np.sort(rng.permutation(live)[:20])
    sets["gather_tiny"] = ([], tiny, tiny)
    out = {}
    for name, (pred, allow, S) in sets.items():
        route = MASK if name.startswith("mask") else GATHER
        assert (len(S) >= 300) if route == MASK else (len(S) <= GATHER_ROWS), (name, len(S))
        pos = np.searchsorted(live, S)
        hit = np.isin([0, 31, 32, 63, 64, len(live) - 1], pos)
        assert name == "gather_tiny" or (hit.any() and not hit.all()), name          # both sides of the set
        out[name] = (pred, allow, S, route)
    oracles = {name: _oracle(ctx, d, v[2]) for name, v in out.items()}
    return {"d": d, "idx": idx, "live": live, "sets": out, "oracles": oracles}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (what, j)


def _last(idx, kind, route, S, live):
    last = idx.within_last()
    assert (last["kind"], last["route"], last["selected"], last["live"]) == (kind, route, len(S), len(live)), last
    return last


class Option:
    def __init__(self, idx, key, value, back=0):
        self.idx, self.key, self.value, self.back = idx, key, value, back

    def __enter__(self):
        self.idx.set_option(self.key, self.value)

    def __exit__(self, *exc):
        self.idx.set_option(self.key, self.back)


ALL_SETS = ["mask_pred", "mask_list", "mask_both", "mask_two_clauses", "gather_pred", "gather_list", "gather_both", "gather_tiny"]


# ---------------------------------------------------------------- radial
@pytest.mark.parametrize("name", ALL_SETS)
def test_radial_equals_the_unrestricted_search_of_the_deleted_index(world, name):
    idx, q, live = world["idx"], world["d"]["q"], world["live"]
    pred, allow, S, route = world["sets"][name]
    orc = world["oracles"][name]
    b = q.shape[0]
    top = orc.search(q, 4)[0]
    few = np.nextafter(top[:, 2], np.float32(-1))          # a few matches: the best three (more where cosines tie)
    cases = {"none": np.full(b, 1.5, np.float32), "inf": np.full(b, np.inf, np.float32), "few": few, "exact": top[:, 0].copy(),
             "all": np.full(b, -1.0, np.float32), "mixed": np.where(np.arange(b) % 2 == 0, few, np.float32(-1.0)).astype(np.float32)}
    for cname, t in cases.items():
        for m in (0, 1, 10, 300):
            got = idx.range_search(q, t, m, pred=pred, filter_ids=allow)
            _last(idx, RADIAL, route, S, live)
            want = orc.range_search(q, t, m)
            _same(got, want, (name, cname, m))
            if cname == "all":
                assert np.all(got[0] == len(S))
            if cname in ("none", "inf"):
                assert np.all(got[0] == 0)
    assert np.all(idx.range_search(q, cases["few"], 10, pred=pred, filter_ids=allow)[0] >= 3)


def test_radial_walk_counts_exactly_the_row_set(ctx):
    """about 6,000 rows at threshold -1: a query holds more than 4,096 candidates and takes the walk over row ranges"""
    d = _data(11, 6007)
    dels = [0, 17, 4096]
    idx = _build(ctx, d, keys=False, dels=dels)
    live = _live(d, dels)
    S = _year_rows(d, live, 2003)
    assert len(S) > 4096
    orc = _oracle(ctx, d, S, keys=False, dels=dels)
    q = d["q"][:3]
    t = np.array([-1.0, -1.0, 0.2], np.float32)
    want = orc.range_search(q, t, 50)
    for route, rows in ((MASK, GATHER_ROWS), (GATHER, 8192)):
        with Option(idx, "filter_gather_rows", rows, GATHER_ROWS):
            got = idx.range_search(q, t, 50, pred=[(YEAR, "range", 2003, None)])
        last = _last(idx, RADIAL, route, S, live)
        assert last["swept"] == 2, last                       # the two queries at -1
        _same(got, want, route)
        assert got[0][0] == len(S) and got[0][1] == len(S)


# ---------------------------------------------------------------- collapsed
@pytest.mark.parametrize("name", ALL_SETS)
def test_collapsed_equals_the_unrestricted_search_of_the_deleted_index(world, name):
    from semantic_query_engine_amd.engine import where_depth
    idx, q, live = world["idx"], world["d"]["q"], world["live"]
    pred, allow, S, route = world["sets"][name]
    orc = world["oracles"][name]
    groups = len(np.unique(np.where(world["d"]["keys"][S] == NONE, -S - 1, world["d"]["keys"][S])))
    for k in (3, 10, 256):
        got = idx.search_collapsed(q, k, pred=pred, filter_ids=allow)
        last = _last(idx, COLLAPSED, route, S, live)
        kd = min(256, max(64, 4 * k))
        assert last["depth"] == (kd if route == GATHER else (where_depth(kd, len(S), len(live)) or 256)), last
        want = orc.search_collapsed(q, k)
        _same(got, want, (name, k))
        assert np.all((got[1] >= 0).sum(axis=1) == min(k, groups))          # k = 256 is above the groups of every set here
    for row in idx.search_collapsed(q, 10, pred=pred, filter_ids=allow)[1]:
        assert np.all(np.isin(row[row >= 0], S))


def test_collapsed_on_the_mask_route_where_the_set_is_small(world):
    """"within_route" 2: the 20-row set on the mask route; k above its groups ends in padding"""
    idx, q, live = world["idx"], world["d"]["q"], world["live"]
    pred, allow, S, _ = world["sets"]["gather_tiny"]
    orc = world["oracles"]["gather_tiny"]
    with Option(idx, "within_route", 2):
        for k in (3, 30):
            got = idx.search_collapsed(q, k, pred=pred, filter_ids=allow)
            last = _last(idx, COLLAPSED, MASK, S, live)
            assert last["depth"] == 256 and (k == 3 or last["swept"] == q.shape[0]), last       # 20 rows never hold 30 groups
            _same(got, orc.search_collapsed(q, k), k)
        got = idx.range_search(q, -1.0, 25, pred=pred, filter_ids=allow)
        _last(idx, RADIAL, MASK, S, live)
        _same(got, orc.range_search(q, -1.0, 25))
        assert np.all(got[0] == 20)


def test_collapsed_without_any_key(ctx, world):
    d, live = world["d"], world["live"]
    idx = _build(ctx, d, keys=False)
    for name in ("mask_pred", "gather_both"):
        pred, allow, S, route = world["sets"][name]
        orc = _oracle(ctx, d, S, keys=False)
        got = idx.search_collapsed(d["q"], 10, pred=pred, filter_ids=allow)
        _last(idx, COLLAPSED, route, S, live)
        _same(got, orc.search_collapsed(d["q"], 10), name)
        assert np.all(got[2] == NONE)
        _same(got[:2], orc.search(d["q"], 10), name)


@pytest.mark.parametrize("crowd_in_set", [True, False])
def test_collapsed_crowd_of_one_key_next_to_the_query(ctx, crowd_in_set):
    """300 near-identical rows of one key next to query 0: inside S the first stage sees one group, outside S all of its hits are
    denied; either way the query is swept"""
    d = _data(23, N)
    rng = np.random.default_rng(5)
    centre = rng.standard_normal(DIM).astype(np.float32)
    crowd = (centre[None] + 1e-3 * rng.standard_normal((300, DIM))).astype(np.float32)
    d["x"] = np.concatenate([d["x"], crowd])
    d["keys"] = np.concatenate([d["keys"], np.full(300, 99991, np.int64)])
    d["year"] = np.concatenate([d["year"], np.full(300, 2015 if crowd_in_set else 2001, np.int64)])
    d["q"][0] = centre
    idx = _build(ctx, d)
    live = _live(d)
    S = _year_rows(d, live, 2010)
    assert len(S) >= 300 and np.isin(np.arange(N, N + 300), S).all() == crowd_in_set
    orc = _oracle(ctx, d, S)
    got = idx.search_collapsed(d["q"], 10, pred=[(YEAR, "range", 2010, None)])
    last = _last(idx, COLLAPSED, MASK, S, live)
    assert 0 < last["depth"] < 300 and last["swept"] >= 1, last
    _same(got, orc.search_collapsed(d["q"], 10))
    assert (got[2][0, 0] == 99991) == crowd_in_set


def test_collapsed_and_radial_on_an_ivf_index(ctx, world):
    d, live = world["d"], world["live"]
    idx = _build(ctx, d, kind="ivf")
    q = d["q"]
    for name in ("mask_both", "gather_pred"):
        pred, allow, S, route = world["sets"][name]
        orc = _oracle(ctx, d, S, kind="ivf")
        got = idx.search_collapsed(q, 10, pred=pred, filter_ids=allow)
        last = _last(idx, COLLAPSED, route, S, live)
        if route == MASK:
            assert last["depth"] == 0 and last["swept"] == q.shape[0], last     # an IVF index sweeps every query
        _same(got, orc.search_collapsed(q, 10), name)
        got = idx.range_search(q, 0.1, 10, pred=pred, filter_ids=allow)
        _last(idx, RADIAL, route, S, live)
        _same(got, orc.range_search(q, 0.1, 10), name)


# ---------------------------------------------------------------- MMR
@pytest.mark.parametrize("where_route", [1, 2])
def test_mmr_equals_the_unrestricted_search_of_the_deleted_index(world, where_route):
    idx, q, live = world["idx"], world["d"]["q"], world["live"]
    b = q.shape[0]
    with Option(idx, "where_route", where_route):
        for name in ("mask_pred", "gather_list", "mask_both", "gather_tiny"):
            pred, allow, S, _ = world["sets"][name]
            orc = world["oracles"][name]
            route = where_route
            # lambda 1 is the plain ranking: search_where
            got = idx.search_mmr(q, 10, lam=1.0, pred=pred, filter_ids=allow)
            last = _last(idx, MMR, route, S, live)
            assert last["depth"] == 40 and last["route"] == idx.where_last()["route"], last
            _same(got[:2], idx.search_where(q, 10, pred, filter_ids=allow), name)
            _same(got, orc.search_mmr(q, 10, lam=1.0), name)
            # 20 rows under 32 candidates: M < n_cand
            for lam, n_cand, k in ((0.5, 32, 10), (0.3, 0, 5), (np.linspace(0, 1, b).astype(np.float32), 64, 12)):
                got = idx.search_mmr(q, k, lam=lam, n_cand=n_cand, pred=pred, filter_ids=allow)
                _last(idx, MMR, route, S, live)
                _same(got, orc.search_mmr(q, k, lam=lam, n_cand=n_cand), (name, n_cand))
                assert np.all((got[1] >= 0).sum(axis=1) == min(k, len(S)))


# ---------------------------------------------------------------- the ends of the row set
def test_empty_set_everything_and_an_empty_list(world):
    idx, q, live = world["idx"], world["d"]["q"], world["live"]
    for pred, allow in (([(YEAR, "range", 3000, None)], None), ([], np.empty(0, np.int64)), ([(YEAR, "range", 2010, None)], [DELETED[1]])):
        counts, cos, ids = idx.range_search(q, -1.0, 5, pred=pred, filter_ids=allow)
        _last(idx, RADIAL, 0, [], live)
        assert np.all(counts == 0) and np.all(ids == -1) and np.all(np.isneginf(cos))
        cos, ids, keys = idx.search_collapsed(q, 5, pred=pred, filter_ids=allow)
        last = _last(idx, COLLAPSED, 0, [], live)
        assert last["depth"] == 0 and last["swept"] == 0
        assert np.all(ids == -1) and np.all(np.isneginf(cos)) and np.all(keys == NONE)
        cos, ids, obj = idx.search_mmr(q, 5, pred=pred, filter_ids=allow)
        _last(idx, MMR, 0, [], live)
        assert np.all(ids == -1) and np.all(np.isneginf(cos)) and np.all(np.isneginf(obj))
    # zero clauses and no list select every live row: the unrestricted call on the same index
    for route, within_route in ((MASK, 0), (MASK, 2)):
        with Option(idx, "within_route", within_route):
            _same(idx.range_search(q, 0.1, 10, pred=[]), idx.range_search(q, 0.1, 10))
            _last(idx, RADIAL, route, live, live)
            _same(idx.search_collapsed(q, 10, pred=[]), idx.search_collapsed(q, 10))
            _last(idx, COLLAPSED, route, live, live)
    _same(idx.search_mmr(q, 10, pred=[]), idx.search_mmr(q, 10))
    _last(idx, MMR, GATHER, live, live)
    with Option(idx, "filter_gather_rows", 1 << 20, GATHER_ROWS):
        _same(idx.range_search(q, 0.1, 10, filter_ids=live), idx.range_search(q, 0.1, 10))
        _last(idx, RADIAL, GATHER, live, live)
        _same(idx.search_collapsed(q, 10, filter_ids=live), idx.search_collapsed(q, 10))
        _last(idx, COLLAPSED, GATHER, live, live)


def test_1025_queries_cross_a_pass_boundary(world):
    idx, live = world["idx"], world["live"]
    pred, allow, S, route = world["sets"]["mask_both"]
    orc = world["oracles"]["mask_both"]
    q = np.random.default_rng(3).standard_normal((1025, DIM)).astype(np.float32)
    t = np.where(np.arange(1025) % 3 == 0, 0.25, 0.05).astype(np.float32)
    got = idx.range_search(q, t, 7, pred=pred, filter_ids=allow)
    _last(idx, RADIAL, MASK, S, live)
    _same(got, orc.range_search(q, t, 7))
    got = idx.search_collapsed(q, 10, pred=pred, filter_ids=allow)
    _last(idx, COLLAPSED, MASK, S, live)
    _same(got, orc.search_collapsed(q, 10))
    got = idx.search_collapsed(q, 200, pred=pred, filter_ids=allow)      # more than the groups of S: every query of both passes is swept
    last = _last(idx, COLLAPSED, MASK, S, live)
    assert last["swept"] == 1025, last
    _same(got, orc.search_collapsed(q, 200))


def test_device_forms(world):
    import torch
    idx, q, live = world["idx"], world["d"]["q"], world["live"]
    dev = torch.device("cuda", 0)
    b, k = q.shape[0], 10
    qd = torch.from_numpy(q).to(dev)
    for name in ("mask_both", "gather_both"):
        pred, allow, S, route = world["sets"][name]
        rows, keep = idx._row_set(pred, None)
        ad = torch.from_numpy(np.ascontiguousarray(allow, np.int64)).to(dev)
        rows = rows[:4] + (ad.data_ptr(), ad.shape[0])
        cd = torch.empty((b, k), dtype=torch.float32, device=dev)
        jd = torch.empty((b, k), dtype=torch.int64, device=dev)
        kd = torch.empty((b, k), dtype=torch.int64, device=dev)
        od = torch.empty((b, k), dtype=torch.float32, device=dev)
        nd = torch.empty(b, dtype=torch.int64, device=dev)
        td = torch.full((b,), 0.1, dtype=torch.float32, device=dev)
        lam = np.full(b, 0.5, np.float32)
        torch.cuda.synchronize()
        assert idx.lib.sqe_index_range_search_where_device(idx.handle, qd.data_ptr(), b, td.data_ptr(), k, *rows, nd.data_ptr(), cd.data_ptr(),
                                                           jd.data_ptr()) == 0
        idx.ctx.synchronize()
        _same((nd.cpu().numpy(), cd.cpu().numpy(), jd.cpu().numpy()), idx.range_search(q, 0.1, k, pred=pred, filter_ids=allow), name)
        assert idx.lib.sqe_index_search_collapsed_where_device(idx.handle, qd.data_ptr(), b, k, *rows, cd.data_ptr(), jd.data_ptr(),
                                                               kd.data_ptr()) == 0
        idx.ctx.synchronize()
        _same((cd.cpu().numpy(), jd.cpu().numpy(), kd.cpu().numpy()), idx.search_collapsed(q, k, pred=pred, filter_ids=allow), name)
        assert idx.lib.sqe_index_search_mmr_where_device(idx.handle, qd.data_ptr(), b, k, 0, lam.ctypes.data, 0, *rows, cd.data_ptr(),
                                                         jd.data_ptr(), od.data_ptr()) == 0
        idx.ctx.synchronize()
        _same((cd.cpu().numpy(), jd.cpu().numpy(), od.cpu().numpy()), idx.search_mmr(q, k, pred=pred, filter_ids=allow), name)
        del keep


# ---------------------------------------------------------------- device groups
@pytest.mark.parametrize("P", [3])
def test_logical_shards_answer_as_the_single_index(world, P):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context
    d, q = world["d"], world["d"]["q"]
    one = world["idx"]
    grp = _build(Context(devices=[0] * P, exchange=EXCHANGE_COPY), d)
    for name in ("mask_pred", "mask_list", "mask_both", "gather_pred", "gather_both", "gather_tiny"):
        pred, allow, S, _ = world["sets"][name]
        for t, m in ((0.1, 10), (-1.0, 0), (-1.0, 40)):
            _same(grp.range_search(q, t, m, pred=pred, filter_ids=allow), one.range_search(q, t, m, pred=pred, filter_ids=allow), (name, t, m))
        for k in (3, 10):
            _same(grp.search_collapsed(q, k, pred=pred, filter_ids=allow), one.search_collapsed(q, k, pred=pred, filter_ids=allow), (name, k))
        for lam, n_cand in ((1.0, 0), (0.5, 32)):
            _same(grp.search_mmr(q, 10, lam=lam, n_cand=n_cand, pred=pred, filter_ids=allow),
                  one.search_mmr(q, 10, lam=lam, n_cand=n_cand, pred=pred, filter_ids=allow), (name, lam))
    # the _device forms on the group: leader-device memory, the allow-list read back and routed on the host; no list: a null pointer
    import torch
    dev = torch.device("cuda", 0)
    b, k = q.shape[0], 10
    qd = torch.from_numpy(q).to(dev)
    lam = np.full(b, 0.5, np.float32)
    for name in ("mask_both", "gather_both", "mask_pred"):
        pred, allow, S, _ = world["sets"][name]
        rows, keep = grp._row_set(pred, None)
        if allow is not None:
            ad = torch.from_numpy(np.ascontiguousarray(allow, np.int64)).to(dev)
            rows = rows[:4] + (ad.data_ptr(), ad.shape[0])
        cd = torch.empty((b, k), dtype=torch.float32, device=dev)
        jd = torch.empty((b, k), dtype=torch.int64, device=dev)
        kd = torch.empty((b, k), dtype=torch.int64, device=dev)
        od = torch.empty((b, k), dtype=torch.float32, device=dev)
        nd = torch.empty(b, dtype=torch.int64, device=dev)
        td = torch.full((b,), 0.1, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        assert grp.lib.sqe_index_range_search_where_device(grp.handle, qd.data_ptr(), b, td.data_ptr(), k, *rows, nd.data_ptr(), cd.data_ptr(),
                                                           jd.data_ptr()) == 0
        grp.ctx.synchronize()
        _same((nd.cpu().numpy(), cd.cpu().numpy(), jd.cpu().numpy()), one.range_search(q, 0.1, k, pred=pred, filter_ids=allow), name)
        assert grp.lib.sqe_index_search_collapsed_where_device(grp.handle, qd.data_ptr(), b, k, *rows, cd.data_ptr(), jd.data_ptr(),
                                                               kd.data_ptr()) == 0
        grp.ctx.synchronize()
        _same((cd.cpu().numpy(), jd.cpu().numpy(), kd.cpu().numpy()), one.search_collapsed(q, k, pred=pred, filter_ids=allow), name)
        assert grp.lib.sqe_index_search_mmr_where_device(grp.handle, qd.data_ptr(), b, k, 0, lam.ctypes.data, 0, *rows, cd.data_ptr(),
                                                         jd.data_ptr(), od.data_ptr()) == 0
        grp.ctx.synchronize()
        _same((cd.cpu().numpy(), jd.cpu().numpy(), od.cpu().numpy()), one.search_mmr(q, k, pred=pred, filter_ids=allow), name)
        del keep
    with pytest.raises(Exception):
        grp.within_last()                                    # single-device indexes only


# ---------------------------------------------------------------- argument errors
def test_argument_errors_write_nothing(ctx):
    from semantic_query_engine_amd import _native as N
    from semantic_query_engine_amd.engine import pack_predicates
    d = _data(31, 300)
    idx = _build(ctx, d, dels=[])
    lib, h = idx.lib, idx.handle
    last = N.WithinLast()
    assert C.sizeof(last) == 40
    assert lib.sqe_index_within_last(h, last) == -4       # SQE_ERR_STATE: no restricted search yet
    assert lib.sqe_index_within_last(h, None) == -1 and lib.sqe_index_within_last(None, last) == -1
    q = np.ascontiguousarray(d["q"][:2])
    t = np.array([0.1, 0.2], np.float32)
    lam = np.array([0.5, 0.5], np.float32)
    cos = np.full((2, 4), 7.0, np.float32)
    ids = np.full((2, 4), 7, np.int64)
    keys = np.full((2, 4), 7, np.int64)
    obj = np.full((2, 4), 7.0, np.float32)
    cnt = np.full(2, 7, np.int64)
    cl, _, sv = pack_predicates([[(YEAR, "range", 2010, None)]])
    nine = np.repeat(cl, 9)
    allow = np.arange(10, dtype=np.int64)
    P = lambda a: None if a is None else a.ctypes.data

    def radial(qq=q, tt=t, m=4, c=cl, nc=1, al=None, na=-1, n=cnt, co=cos, i=ids, b=2):
        return lib.sqe_index_range_search_where(h, P(qq), b, P(tt), m, P(c), nc, P(sv), 0, P(al), na, P(n), P(co), P(i))

    def collapsed(qq=q, k=4, c=cl, nc=1, al=None, na=-1, co=cos, i=ids, ke=keys, b=2):
        return lib.sqe_index_search_collapsed_where(h, P(qq), b, k, P(c), nc, P(sv), 0, P(al), na, P(co), P(i), P(ke))

    def mmr(qq=q, k=4, nc_=0, la=lam, c=cl, nc=1, al=None, na=-1, co=cos, i=ids, o=obj, b=2):
        return lib.sqe_index_search_mmr_where(h, P(qq), b, k, nc_, P(la), 0, P(c), nc, P(sv), 0, P(al), na, P(co), P(i), P(o))

    bad = [radial(qq=None), radial(tt=None), radial(n=None), radial(co=None), radial(i=None), radial(m=-1), radial(m=10001), radial(b=-1),
           radial(na=-2), radial(na=3), radial(c=nine, nc=9), radial(nc=-1), radial(tt=np.array([0.1, np.nan], np.float32)),
           collapsed(qq=None), collapsed(co=None), collapsed(i=None), collapsed(ke=None), collapsed(k=0), collapsed(k=257),
           collapsed(na=-2), collapsed(na=3), collapsed(c=nine, nc=9),
           mmr(qq=None), mmr(la=None), mmr(co=None), mmr(i=None), mmr(o=None), mmr(k=0), mmr(k=257), mmr(nc_=3), mmr(nc_=257),
           mmr(la=np.array([0.5, 1.5], np.float32)), mmr(na=-2), mmr(na=3), mmr(c=nine, nc=9),
           lib.sqe_index_range_search_where(None, P(q), 2, P(t), 4, P(cl), 1, P(sv), 0, None, -1, P(cnt), P(cos), P(ids))]
    assert bad == [-1] * len(bad), bad
    assert np.all(cos == 7.0) and np.all(ids == 7) and np.all(keys == 7) and np.all(obj == 7.0) and np.all(cnt == 7)
    assert lib.sqe_index_within_last(h, last) == -4       # still none
    # the good call of each kind, and max_hits 0 with null result buffers
    assert radial(al=allow, na=10) == 0 and collapsed(al=allow, na=10) == 0 and mmr(al=allow, na=10) == 0
    assert radial(m=0, co=None, i=None) == 0 and radial(b=0, qq=None, tt=None, n=None) == 0
    assert lib.sqe_index_within_last(h, last) == 0 and (last.kind, last.route, last.live) == (RADIAL, GATHER, 300)
    with pytest.raises(Exception):
        idx.set_option("within_route", 1)
