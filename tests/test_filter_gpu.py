"""Filtered search (sqe_index_search_filtered, filter.hip): the exact top-k over the live rows on an allow-list.  The
central check compares a filtered search of an index with an unfiltered search of a fresh index built from the allowed
rows alone: both normalise the same raw rows, so the ids must map back exactly and the cosines must be equal bit for bit.
Every case is also checked against the NumPy oracle.  GPU only."""
import threading

import numpy as np
import pytest

from oracle import retrieval as R
from tests.gpu_util import assert_topk_matches, exact_topk_fast

pytestmark = pytest.mark.gpu

N, D = 50_000, 256


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((1100, D)).astype(np.float32)
    q[:200] = x[rng.integers(0, N, 200)] + 0.1 * q[:200]       # queries with a clear nearest row
    return x, q


@pytest.fixture(scope="module")
def index(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, D)
    idx.add(data[0])
    return idx


def _fresh(ctx, x, allowed, q, k):
    from semantic_query_engine_amd import VectorIndex
    if allowed.size == 0:
        return np.full((q.shape[0], k), -np.inf, np.float32), np.full((q.shape[0], k), -1, np.int64)
    b = VectorIndex(ctx, x.shape[1])
    b.add(x[allowed])
    cos, ids = b.search(q, k)
    b.close()
    return cos, np.where(ids >= 0, allowed[np.maximum(ids, 0)], -1)


def _oracle_check(cos, ids, x, allowed, q, k, id_base=0):
    if allowed.size == 0:
        assert np.all(ids == -1) and np.all(np.isneginf(cos))
        return
    ref_cos, ref_pos = exact_topk_fast(x[allowed], q, k)
    ref_ids = np.where(ref_pos >= 0, allowed[np.maximum(ref_pos, 0)] + id_base, -1)
    xn = np.zeros((x.shape[0] + id_base, x.shape[1]), np.float32)
    xn[allowed + id_base] = R.normalize_rows(x[allowed])
    assert_topk_matches(cos, ids, ref_cos, ref_ids, xn, R.normalize_rows(q))


def _check(ctx, idx, x, q, k, filter_ids, allowed, id_base=0):
    """filtered search of idx == unfiltered search of a fresh index of x[allowed] (allowed: live ids, ascending)."""
    cos, ids = idx.search(q, k, filter_ids=filter_ids)
    assert cos.shape == (q.shape[0], k) and ids.shape == (q.shape[0], k)
    fc, fi = _fresh(ctx, x, allowed, q, k)
    assert np.array_equal(ids, np.where(fi >= 0, fi + id_base, -1))
    assert np.array_equal(cos, fc)
    _oracle_check(cos, ids, x, allowed, q, k, id_base)
    return cos, ids


@pytest.mark.parametrize("k", [1, 10, 256])
def test_allow_list_sizes_and_batches(ctx, data, index, k):
    x, q = data
    rng = np.random.default_rng(k)
    sizes = [0, 1, max(k - 1, 1), k, int(0.03 * N), N // 2, N]
    batches = [1, 64, 1024, 1100, 64, 1100, 1] if k != 1 else [1100, 1, 64, 1024, 1, 64, 1100]
    for size, b in zip(sizes, batches):
        allowed = np.sort(rng.choice(N, size, replace=False))
        _check(ctx, index, x, q[:b], k, rng.permutation(allowed), allowed)


def test_many_chunks_equal_one(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    rng = np.random.default_rng(3)
    allowed = np.sort(rng.choice(N, 20_000, replace=False))
    idx = VectorIndex(ctx, D)
    idx.add(x)
    one = idx.search(q[:300], 10, filter_ids=allowed)
    idx.set_option("filter_gather_rows", 1280)                  # 16 chunks
    many = _check(ctx, idx, x, q[:300], 10, allowed, allowed)
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])
    many256 = idx.search(q[:64], 256, filter_ids=allowed)
    idx.set_option("filter_gather_rows", 1 << 20)
    one256 = idx.search(q[:64], 256, filter_ids=allowed)
    assert np.array_equal(one256[0], many256[0]) and np.array_equal(one256[1], many256[1])


def test_no_stale_rows_after_a_larger_gather(ctx, data, index):
    x, q = data
    rng = np.random.default_rng(4)
    big = np.sort(rng.choice(N, 40_000, replace=False))
    _check(ctx, index, x, q[:64], 10, big, big)
    small = np.sort(rng.choice(N, 300, replace=False))
    _check(ctx, index, x, q[:64], 10, small, small)
    _check(ctx, index, x, q[:64], 256, small, small)          # k close to M: padding rows must not surface


def test_deleted_unknown_negative_repeated_ids(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    rng = np.random.default_rng(5)
    idx = VectorIndex(ctx, D)
    idx.add(x)
    drop = rng.choice(N, 5000, replace=False)
    idx.delete(drop)
    live = np.setdiff1d(np.arange(N), drop)
    want = np.sort(rng.choice(live, 3000, replace=False))
    junk = np.concatenate([want, want[:500], rng.choice(drop, 700), [-1, -5, N, N + 10, 2**40, -(2**40)]])
    junk = rng.permutation(junk)
    a = _check(ctx, idx, x, q[:128], 10, junk, want)
    b = idx.search(q[:128], 10, filter_ids=want)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # only non-live ids: all padding
    cos, ids = idx.search(q[:8], 5, filter_ids=np.concatenate([drop[:50], [-3, N + 1]]))
    assert np.all(ids == -1) and np.all(np.isneginf(cos))


def test_ties_go_to_lowest_allowed_id(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(6)
    base = rng.standard_normal((500, D)).astype(np.float32)
    x = np.concatenate([base, base, base])                     # row r, r + 500 and r + 1000 are the same
    idx = VectorIndex(ctx, D)
    idx.add(x)
    q = base[:40] + 0.01 * rng.standard_normal((40, D)).astype(np.float32)
    allowed = np.concatenate([np.arange(500, 1500)])           # the lowest copy excluded
    cos, ids = idx.search(q, 2, filter_ids=rng.permutation(allowed))
    assert np.array_equal(ids[:, 0], np.arange(40) + 500)
    assert np.array_equal(ids[:, 1], np.arange(40) + 1000)
    assert np.array_equal(cos[:, 0], cos[:, 1])


@pytest.mark.parametrize("with_deletes", [False, True])
def test_id_base(ctx, data, with_deletes):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    rng = np.random.default_rng(7)
    n = 20_000
    idx = VectorIndex(ctx, D)
    idx.add(x[:n])
    idx.set_option("id_base", 1_000_000)
    live = np.arange(n)
    if with_deletes:
        drop = rng.choice(n, 2000, replace=False)
        idx.delete(drop)
        live = np.setdiff1d(live, drop)
    allowed = np.sort(rng.choice(live, 4000, replace=False))
    _check(ctx, idx, x, q[:64], 10, allowed, allowed, id_base=1_000_000)


def test_ivf_is_exact_over_allowed_rows(ctx):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    rng = np.random.default_rng(8)
    n, d, k = 30_000, 128, 10
    cen = rng.standard_normal((200, d)).astype(np.float32)
    x = (cen[rng.integers(0, 200, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    q = (x[rng.integers(0, n, 48)] + 0.2 * rng.standard_normal((48, d))).astype(np.float32)
    idx = VectorIndex(ctx, d, INDEX_IVF_FLAT, 64)
    idx.add(x)
    idx.train(x, iters=8, seed=3)
    idx.search(q[:2], k, nprobe=4)
    drop = rng.choice(n, 3000, replace=False)
    idx.delete(drop)
    live = np.setdiff1d(np.arange(n), drop)
    allowed = np.sort(rng.choice(live, 5000, replace=False))
    _check(ctx, idx, x, q, k, allowed, allowed)


@pytest.mark.parametrize("P", [2, 3])
def test_group_equals_single_device(ctx, data, P):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, q = data
    rng = np.random.default_rng(9 + P)
    n = 12_007
    gctx = Context(devices=[0] * P, exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    s = VectorIndex(ctx, D)
    g.add(x[:n])
    s.add(x[:n])
    drop = rng.choice(n, 1500, replace=False)
    g.delete(drop)
    s.delete(drop)
    live = np.setdiff1d(np.arange(n), drop)
    filt = np.concatenate([rng.choice(live, 2500, replace=False), drop[:100], [-2, n + 3]])
    allowed = np.intersect1d(filt, live)
    for k, b in ((10, 64), (256, 5)):
        gc, gi = g.search(q[:b], k, filter_ids=filt)
        sc, si = _check(ctx, s, x, q[:b], k, filt, allowed)
        assert np.array_equal(gi, si) and np.array_equal(gc, sc)
    cos, ids = g.search(q[:4], 3, filter_ids=np.array([], np.int64))
    assert np.all(ids == -1)
    g.close()
    gctx.close()


def test_device_entry_point(ctx, data, index):
    import torch
    x, q = data
    rng = np.random.default_rng(10)
    allowed = np.sort(rng.choice(N, 1500, replace=False))
    b, k = 100, 10
    qd = torch.from_numpy(q[:b]).cuda()
    ad = torch.from_numpy(rng.permutation(allowed)).cuda()
    cos = torch.empty((b, k), dtype=torch.float32, device="cuda")
    ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    index.search_device(qd.data_ptr(), b, k, cos.data_ptr(), ids.data_ptr(), filter_ptr=ad.data_ptr(),
                        n_filter=ad.numel())
    ctx.synchronize()
    hc, hi = index.search(q[:b], k, filter_ids=allowed)
    assert np.array_equal(ids.cpu().numpy(), hi) and np.array_equal(cos.cpu().numpy(), hc)
    _oracle_check(hc, hi, x, allowed, q[:b], k)


def test_int8_parent_state_untouched(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(12)
    n, d, k = 1_000_000, 256, 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((256, d)).astype(np.float32)
    q[:64] = x[rng.integers(0, n, 64)] + 0.1 * q[:64]
    idx = VectorIndex(ctx, d)
    idx.add(x)
    c0, i0 = idx.search(q, k)
    last0 = idx.i8_last()
    assert last0["rows"] == n
    for size in (10, 20_000, 300_000):
        allowed = np.sort(rng.choice(n, size, replace=False))
        cos, ids = idx.search(q[:64], k, filter_ids=allowed)
        _oracle_check(cos, ids, x, allowed, q[:64], k)
    assert idx.i8_last() == last0
    c1, i1 = idx.search(q, k)
    assert np.array_equal(c0, c1) and np.array_equal(i0, i1)
    assert idx.i8_last() == last0
    idx.close()


def test_two_threads_equal_serial(ctx, data, index):
    x, q = data
    rng = np.random.default_rng(13)
    filters = [np.sort(rng.choice(N, s, replace=False)) for s in (50, 2000, 30_000)]
    jobs = [(q[i * 32:(i + 1) * 32], filters[i % 3] if i % 2 == 0 else None) for i in range(12)]
    serial = [index.search(qq, 10, filter_ids=f) for qq, f in jobs]
    out = [None] * len(jobs)
    errors = []

    def run(part):
        try:
            for i in range(part, len(jobs), 2):
                out[i] = index.search(jobs[i][0], 10, filter_ids=jobs[i][1])
        except Exception as e:          # pragma: no cover
            errors.append(e)

    ts = [threading.Thread(target=run, args=(p,)) for p in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors
    for a, b in zip(serial, out):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
