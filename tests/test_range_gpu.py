"""Radial search (sqe_index_range_search, range.hip): per query, every live row whose fp32 cosine is >= a threshold, the
exact count and the best max_hits of them.  Checked against a float64 NumPy product (counts exact except for rows whose
true cosine lies within 2e-6 of the threshold) and, bit for bit, against sqe_index_search: a row's cosine is the value
search returns for it.  GPU only."""
import numpy as np
import pytest

from oracle import retrieval as R

pytestmark = pytest.mark.gpu

N, D = 40_000, 256
TOL = 2e-6


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(21)
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((1500, D)).astype(np.float32)
    q[:600] = x[rng.integers(0, N, 600)] + 0.3 * q[:600]        # perturbed copies of rows: a few close rows each
    return x, q


@pytest.fixture(scope="module")
def index(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, D)
    idx.add(data[0])
    return idx


def _cos64(x, q):
    return R.normalize_rows(q).astype(np.float64) @ R.normalize_rows(x).astype(np.float64).T


def _check(counts, cos, ids, c64, t, live=None, id_of=None):
    """One radial result against the float64 product c64 [B, n] (columns = rows; `live` masks deleted ones, id_of maps a
    column to its id)."""
    b, m = cos.shape
    n = c64.shape[1]
    live = np.ones(n, bool) if live is None else live
    id_of = np.arange(n) if id_of is None else id_of
    col_of = {int(i): j for j, i in enumerate(id_of)}
    for i in range(b):
        ci = np.where(live, c64[i], -np.inf)
        ti = float(t[i])
        lo, hi = int(np.sum(ci >= ti + TOL)), int(np.sum(ci >= ti - TOL))
        assert lo <= counts[i] <= hi, (i, counts[i], lo, hi)
        v = min(int(counts[i]), m)
        assert np.all(ids[i, v:] == -1) and np.all(np.isneginf(cos[i, v:]))
        got = ids[i, :v]
        assert np.all(got >= 0) and np.unique(got).size == v
        assert np.all(cos[i, :v] >= np.float32(ti))
        cols = np.array([col_of[int(g)] for g in got], np.int64)
        assert np.all(live[cols])
        assert np.all(np.abs(cos[i, :v] - ci[cols]) <= TOL)
        # best first, ties to the lowest id
        if v > 1:
            assert np.all((cos[i, :v - 1] > cos[i, 1:v]) | ((cos[i, :v - 1] == cos[i, 1:v]) & (got[:-1] < got[1:])))
        # nothing clearly better was left out
        floor = ti if v < m else float(cos[i, v - 1])
        must = np.nonzero(ci >= floor + TOL)[0]
        assert set(id_of[must].tolist()) <= set(got.tolist()), i


def _thresholds(c64, ranks):
    """per query, a threshold halfway between the cosines of rank r and r + 1 (r < 0: -1)"""
    s = -np.sort(-c64, axis=1)
    t = np.empty(c64.shape[0], np.float32)
    for i, r in enumerate(ranks):
        t[i] = -1.0 if r < 0 else (s[i, r] + s[i, r + 1]) / 2
    return t


@pytest.mark.parametrize("B", [1, 64, 1024, 1500])
def test_mixed_thresholds(index, data, B):
    x, q = data
    qq = q[:B]
    c64 = _cos64(x, qq)
    ranks = np.array([0, 3, 250, 2000, -1, 9])[np.arange(B) % 6]
    t = _thresholds(c64, ranks)
    counts, cos, ids = index.range_search(qq, t, 100)
    _check(counts, cos, ids, c64, t)
    assert np.all(counts[ranks == -1] == N)
    # more matches than max_hits: the count does not depend on max_hits
    c2, _, _ = index.range_search(qq, t, 7)
    assert np.array_equal(c2, counts)


def test_scalar_threshold_and_none(index, data):
    x, q = data
    counts, cos, ids = index.range_search(q[:5], 1.5, 10)
    assert np.all(counts == 0) and np.all(ids == -1) and np.all(np.isneginf(cos))
    counts, _, ids = index.range_search(q[:3], -np.inf, 10)
    assert np.all(counts == N) and np.all(ids >= 0)
    counts, _, _ = index.range_search(q[:3], np.inf, 10)
    assert np.all(counts == 0)


def test_bit_exact_with_search(index, data):
    x, q = data
    qq = q[:64]
    scos, sids = index.search(qq, 256)
    c64 = _cos64(x, qq)
    t = _thresholds(c64, np.array([5, 100, 200, 30])[np.arange(64) % 4])
    counts, cos, ids = index.range_search(qq, t, 300)
    for i in range(64):
        sel = scos[i] >= t[i]
        v = int(sel.sum())
        assert counts[i] == v
        assert np.array_equal(ids[i, :v], sids[i, sel])
        assert np.array_equal(cos[i, :v].view(np.uint32), scos[i, sel].view(np.uint32))
    # inclusive boundary: t = a cosine search returned for row r puts r among the matches
    t2 = scos[:, 17].copy()
    counts, cos, ids = index.range_search(qq, t2, 256)
    for i in range(64):
        assert sids[i, 17] in ids[i]
        assert counts[i] >= 18


def test_tiny_budget_equals_large(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    big = VectorIndex(ctx, D)
    small = VectorIndex(ctx, D)
    small.set_option("range_key_budget", 4096)       # one query per group: many passes
    for v in (big, small):
        v.add(x[:20_000])
    qq = q[:5]
    c64 = _cos64(x[:20_000], qq)
    t = np.array([0.0, -1.0, 0.05, _thresholds(c64[3:4], [10])[0], 0.1], np.float32)   # ~10 k, 20 k, ~8 k candidates: row splits
    a = big.range_search(qq, t, 5000)
    b = small.range_search(qq, t, 5000)
    for u, w in zip(a, b):
        assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
    _check(*a, c64, t)
    assert a[0][1] == 20_000
    big.close()
    small.close()


def test_crowded_band(ctx):
    """thousands of near-identical rows straddle the threshold: the band is collected whole, the count is exact"""
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(22)
    base = rng.standard_normal(D).astype(np.float32)
    crowd = base + 2e-3 * rng.standard_normal((5000, D)).astype(np.float32)
    x = np.concatenate([rng.standard_normal((15_000, D)).astype(np.float32), crowd])
    x = x[rng.permutation(x.shape[0])]
    idx = VectorIndex(ctx, D)
    idx.add(x)
    qq = (base + 1e-3 * rng.standard_normal(D).astype(np.float32))[None]
    n_all, cos_all, ids_all = idx.range_search(qq, -np.inf, 10000)
    assert n_all[0] == x.shape[0]
    crowd_cos = cos_all[0, :5000]
    for t in (np.median(crowd_cos), crowd_cos[100], crowd_cos[4000]):
        counts, cos, ids = idx.range_search(qq, t, 10000)
        want = int(np.sum(cos_all[0] >= t))
        assert counts[0] == want
        assert np.array_equal(ids[0, :want], ids_all[0, :want])
        assert np.array_equal(cos[0, :want].view(np.uint32), cos_all[0, :want].view(np.uint32))
    idx.close()


def test_deletes_and_id_base(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    n = 12_000
    rng = np.random.default_rng(23)
    idx = VectorIndex(ctx, D)
    idx.add(x[:n])
    gone = np.sort(rng.choice(n, 3000, replace=False))
    idx.delete(gone)
    live = np.ones(n, bool)
    live[gone] = False
    qq = np.concatenate([x[gone[:8]], q[:8]])                  # queries sitting on deleted rows
    c64 = _cos64(x[:n], qq)
    t = np.array([0.2, 0.05, -1.0, 0.999] * 4, np.float32)
    counts, cos, ids = idx.range_search(qq, t, 500)
    _check(counts, cos, ids, c64, t, live=live)
    assert not np.isin(ids, gone).any()
    assert np.all(counts[t == -1.0] == n - gone.size)
    idx.close()
    based = VectorIndex(ctx, D)
    based.set_option("id_base", 1_000_000)
    based.add(x[:n])
    c2, cos2, ids2 = based.range_search(qq, t, 500)
    ref = VectorIndex(ctx, D)
    ref.add(x[:n])
    c3, cos3, ids3 = ref.range_search(qq, t, 500)
    assert np.array_equal(c2, c3) and np.array_equal(cos2, cos3)
    assert np.array_equal(ids2, np.where(ids3 >= 0, ids3 + 1_000_000, -1))
    based.close()
    ref.close()


def test_ivf_equals_flat(ctx, data, index):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    x, q = data
    ivf = VectorIndex(ctx, D, INDEX_IVF_FLAT, 64)
    ivf.add(x)
    ivf.train(x[:10_000], iters=5, seed=1)
    qq = q[:64]
    t = _thresholds(_cos64(x, qq), np.array([0, 40, 900, -1])[np.arange(64) % 4])
    a = ivf.range_search(qq, t, 1000)
    b = index.range_search(qq, t, 1000)
    for u, w in zip(a, b):
        assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
    ivf.close()


@pytest.mark.parametrize("P", [2, 3])
def test_group_equals_single_device(data, index, P):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, q = data
    gctx = Context(devices=[0] * P, exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    g.add(x)
    qq = q[:70]
    t = _thresholds(_cos64(x, qq), np.array([0, 12, 700, -1, 5000])[np.arange(70) % 5])
    a = g.range_search(qq, t, 800)
    b = index.range_search(qq, t, 800)
    for u, w in zip(a, b):
        assert np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
    c0, _, _ = g.range_search(qq, t, 0)
    assert np.array_equal(c0, b[0])
    g.close()
    gctx.close()


def test_counts_only_and_invalid(ctx, index, data):
    from semantic_query_engine_amd import VectorIndex, _native
    x, q = data
    t = np.array([0.1, 0.3, -1.0], np.float32)
    counts, cos, ids = index.range_search(q[:3], t, 0)
    full, _, _ = index.range_search(q[:3], t, 50)
    assert np.array_equal(counts, full) and cos.shape == (3, 0)
    lib = _native.load()
    c = np.zeros(3, np.int64)
    qq = np.ascontiguousarray(q[:3])
    assert lib.sqe_index_range_search(index.handle, qq.ctypes.data, 3, t.ctypes.data, 0, c.ctypes.data, None, None) == 0
    assert np.array_equal(c, counts)
    for bad_t, m in ((np.array([0.1, np.nan, 0.2], np.float32), 10), (t, 10001)):
        with pytest.raises(_native.SqeError) as e:
            index.range_search(q[:3], bad_t, m)
        assert e.value.code == -1                                        # SQE_ERR_INVALID
    assert lib.sqe_index_range_search(index.handle, qq.ctypes.data, 3, t.ctypes.data, -1, c.ctypes.data, None, None) == -1
    assert lib.sqe_index_range_search(index.handle, qq.ctypes.data, 3, t.ctypes.data, 5, c.ctypes.data, None, None) == -1
    assert lib.sqe_index_range_search(index.handle, qq.ctypes.data, 0, t.ctypes.data, 5, c.ctypes.data, None, None) == 0
    empty = VectorIndex(ctx, D)
    n0, c0, i0 = empty.range_search(q[:2], -1.0, 4)
    assert np.all(n0 == 0) and np.all(i0 == -1) and np.all(np.isneginf(c0))
    empty.close()


def test_device_entry_point(ctx, data, index):
    import torch
    x, q = data
    b, m = 50, 20
    t = _thresholds(_cos64(x, q[:b]), np.array([1, 30, -1])[np.arange(b) % 3])
    qd = torch.from_numpy(q[:b]).cuda()
    td = torch.from_numpy(t).cuda()
    nd = torch.empty(b, dtype=torch.int64, device="cuda")
    cd = torch.empty((b, m), dtype=torch.float32, device="cuda")
    idd = torch.empty((b, m), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    index.range_search_device(qd.data_ptr(), b, td.data_ptr(), m, nd.data_ptr(), cd.data_ptr(), idd.data_ptr())
    ctx.synchronize()
    hn, hc, hi = index.range_search(q[:b], t, m)
    assert np.array_equal(nd.cpu().numpy(), hn) and np.array_equal(cd.cpu().numpy(), hc) and np.array_equal(idd.cpu().numpy(), hi)


def test_int8_state_untouched(ctx):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    rng = np.random.default_rng(24)
    x = rng.standard_normal((20_000, 256)).astype(np.float32)
    q = rng.standard_normal((200, 256)).astype(np.float32)
    q[:50] = x[rng.integers(0, 20_000, 50)] + 0.1 * q[:50]
    idx = VectorIndex(ctx, 256)
    for key, val in (("scan_mode", SCAN_INT8_RESCORE), ("i8_min_rows", 0), ("i8_sample_step", 4), ("i8_sample_m", 64)):
        idx.set_option(key, val)
    idx.add(x)
    c0, i0 = idx.search(q, 10)
    last0 = idx.i8_last()
    assert last0["rows"] == 20_000
    counts, cos, ids = idx.range_search(q[:64], 0.2, 50)
    _check(counts, cos, ids, _cos64(x, q[:64]), np.full(64, 0.2, np.float32))
    assert idx.i8_last() == last0
    c1, i1 = idx.search(q, 10)
    assert np.array_equal(c0, c1) and np.array_equal(i0, i1)
    assert idx.i8_last() == last0
    idx.close()
