"""Per-query filtered search (sqe_index_search_filtered_each, filter_each.hip): every query of a call over its own
allow-list.  The central check: row b equals the single-list filtered search of query b alone over its list, bit for bit
in cosines and ids, whatever the route, the batch, the pass size or the index kind.  Every case is also checked against
the NumPy oracle.  GPU only."""
import numpy as np
import pytest

from oracle import retrieval as R
from tests.gpu_util import assert_topk_matches, exact_topk_fast

pytestmark = pytest.mark.gpu

N, DUP = 20_000, 5
ALL_DIRECT = {"filter_each_direct_rows": 1 << 20, "filter_each_direct_queries": 4096}
ALL_GATHERED = {"filter_each_direct_rows": 0}


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


_data = {}


def _rows(dim):
    """N Gaussian rows + DUP exact copies of existing rows (ties), and 320 queries, some next to a row"""
    if dim not in _data:
        rng = np.random.default_rng(1000 + dim)
        x = rng.standard_normal((N, dim)).astype(np.float32)
        x = np.concatenate([x, x[rng.choice(N, DUP, replace=False)]])
        q = rng.standard_normal((320, dim)).astype(np.float32)
        q[:100] = x[rng.integers(0, N, 100)] + 0.1 * q[:100]
        q[100:100 + DUP] = x[N:] + 0.01 * q[100:100 + DUP]         # the duplicated rows are the best hits of these
        _data[dim] = (x, q)
    return _data[dim]


_indexes = {}


def _index(ctx, dim):
    from semantic_query_engine_amd import VectorIndex
    if dim not in _indexes:
        idx = VectorIndex(ctx, dim)
        idx.add(_rows(dim)[0])
        _indexes[dim] = idx
    return _indexes[dim]


def _options(idx, opts):
    for key, value in opts.items():
        idx.set_option(key, value)


def _defaults(idx):
    _options(idx, {"filter_each_direct_rows": 1 << 14, "filter_each_direct_queries": 32, "filter_each_key_budget": 1 << 24})


def _oracle_check(cos, ids, x, lists, loq, q, k, live=None, id_base=0):
    """NumPy oracle per list over the live, distinct ids it names (tests/test_filter_gpu.py::_oracle_check)"""
    loq = np.asarray(loq)
    for f in np.unique(loq):
        rows = np.nonzero(loq == f)[0]
        allowed = np.unique(np.asarray(lists[f], np.int64))
        allowed = allowed[(allowed >= 0) & (allowed < x.shape[0])]
        if live is not None:
            allowed = np.intersect1d(allowed, live)
        if allowed.size == 0:
            assert np.all(ids[rows] == -1) and np.all(np.isneginf(cos[rows]))
            continue
        ref_cos, ref_pos = exact_topk_fast(x[allowed], q[rows], k)
        ref_ids = np.where(ref_pos >= 0, allowed[np.maximum(ref_pos, 0)] + id_base, -1)
        xn = np.zeros((x.shape[0] + id_base, x.shape[1]), np.float32)
        xn[allowed + id_base] = R.normalize_rows(x[allowed])
        assert_topk_matches(cos[rows], ids[rows], ref_cos, ref_ids, xn, R.normalize_rows(q[rows]))


def _single(idx, q, k, lists, loq):
    """what the single-list call answers for every query alone"""
    out = [idx.search(q[b:b + 1], k, filter_ids=np.asarray(lists[f], np.int64)) for b, f in enumerate(loq)]
    return np.concatenate([c for c, _ in out]), np.concatenate([i for _, i in out])


def _same(a, b):
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], b[0])


@pytest.mark.parametrize("k", [1, 10, 256])
@pytest.mark.parametrize("dim", [64, 192, 1024])
def test_list_sizes_and_k(ctx, dim, k):
    x, q = _rows(dim)
    idx = _index(ctx, dim)
    _defaults(idx)
    rng = np.random.default_rng(dim + k)
    sizes = [0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, 255, 256, 257, 1000, 5000, N + DUP]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    lists = [rng.permutation(N + DUP)[:s].astype(np.int64) for s in sizes]
    # the queries next to the duplicated rows see both copies in the long lists
    qq = np.concatenate([q[100:100 + DUP], q[:len(sizes) - DUP]])
    got = idx.search_filtered_each(qq, k, lists)
    assert got[0].shape == (len(sizes), k) and got[1].shape == (len(sizes), k)
    _same(got, _single(idx, qq, k, lists, range(len(sizes))))
    _oracle_check(got[0], got[1], x, lists, np.arange(len(sizes)), qq, k)
    _options(idx, ALL_DIRECT)                       # the list of all rows as well
    _same(idx.search_filtered_each(qq, k, lists), got)
    _defaults(idx)


def test_ties_go_to_the_lowest_id(ctx):
    x, q = _rows(192)
    idx = _index(ctx, 192)
    _defaults(idx)
    xn = R.normalize_rows(x)
    twins = [int(np.nonzero((xn[:N] == xn[N + j]).all(axis=1))[0][0]) for j in range(DUP)]
    lists = [np.array([N + j, twins[j], 7, 11], np.int64) for j in range(DUP)]
    cos, ids = idx.search_filtered_each(q[100:100 + DUP], 2, lists)
    assert np.array_equal(ids[:, 0], np.array(twins)) and np.array_equal(ids[:, 1], N + np.arange(DUP))
    assert np.array_equal(cos[:, 0], cos[:, 1])


def test_routes_agree(ctx):
    x, q = _rows(192)
    idx = _index(ctx, 192)
    rng = np.random.default_rng(21)
    lists = [rng.choice(N + DUP, s, replace=False).astype(np.int64) for s in (3000, 500, 7000, 900)]     # nobody names list 3
    loq = rng.permutation(np.array([0] * 88 + [1] * 6 + [2] * 6, np.int32))
    k = 10
    _options(idx, ALL_DIRECT)
    direct = idx.search_filtered_each(q[:100], k, lists, loq)
    _defaults(idx)
    _options(idx, ALL_GATHERED)
    gathered = idx.search_filtered_each(q[:100], k, lists, loq)
    _defaults(idx)
    _options(idx, {"filter_each_direct_queries": 8})            # list 0 (88 queries) is gathered, lists 1 and 2 are direct
    mixed = idx.search_filtered_each(q[:100], k, lists, loq)
    _defaults(idx)
    _same(direct, gathered)
    _same(direct, mixed)
    _same(direct, _single(idx, q[:100], k, lists, loq))
    _oracle_check(direct[0], direct[1], x, lists, loq, q[:100], k)


def test_several_passes_equal_one(ctx):
    x, q = _rows(192)
    idx = _index(ctx, 192)
    rng = np.random.default_rng(22)
    lists = [rng.choice(N + DUP, s, replace=False).astype(np.int64) for s in (1500, 5000, 0, 700, 4096, 3)]
    loq = rng.integers(0, len(lists), 60).astype(np.int32)
    _options(idx, ALL_DIRECT)
    one = idx.search_filtered_each(q[:60], 10, lists, loq)
    idx.set_option("filter_each_key_budget", 4096)              # the floor: a 5000-row list alone exceeds it
    many = idx.search_filtered_each(q[:60], 10, lists, loq)
    _defaults(idx)
    _same(one, many)
    _oracle_check(one[0], one[1], x, lists, loq, q[:60], 10)
    with pytest.raises(Exception):
        idx.set_option("filter_each_key_budget", 4095)


def test_batch_independence(ctx):
    x, q = _rows(192)
    idx = _index(ctx, 192)
    _defaults(idx)
    rng = np.random.default_rng(23)
    lists = [rng.choice(N + DUP, int(s), replace=False).astype(np.int64) for s in rng.integers(0, 600, 40)]
    loq = rng.integers(0, 40, 300).astype(np.int32)
    k = 10
    full = idx.search_filtered_each(q[:300], k, lists, loq)
    _oracle_check(full[0], full[1], x, lists, loq, q[:300], k)
    for b in rng.choice(300, 12, replace=False):
        alone = idx.search_filtered_each(q[b:b + 1], k, [lists[loq[b]]])
        assert np.array_equal(alone[0][0], full[0][b]) and np.array_equal(alone[1][0], full[1][b])
    perm = rng.permutation(40)                                  # new list f is old list perm[f]
    inv = np.argsort(perm)
    moved = idx.search_filtered_each(q[:300], k, [lists[p] for p in perm], inv[loq].astype(np.int32))
    _same(full, moved)


def test_id_rules(ctx):
    from semantic_query_engine_amd import VectorIndex
    x, q = _rows(192)
    rng = np.random.default_rng(24)
    idx = VectorIndex(ctx, 192)
    idx.add(x)
    drop = rng.choice(N, 2000, replace=False)
    idx.delete(drop)
    idx.set_option("id_base", 1000)
    live = np.setdiff1d(np.arange(N + DUP), drop)
    k = 10
    want = rng.choice(live, 400, replace=False)
    lists = [
        np.concatenate([want, np.full(300, want[0]), want[:50]]),                       # one id 300 times: more than k
        np.concatenate([rng.choice(live, 5, replace=False), drop[:300], [-1, -7, N + DUP, N + DUP + 9, 2**40, -(2**40)]]),
        np.concatenate([drop[:40], [-3, N + DUP]]),                                     # all dead
        np.full(20, live[3]),                                                           # one live row, repeated
    ]
    lists = [rng.permutation(a).astype(np.int64) for a in lists]
    loq = rng.integers(0, len(lists), 50).astype(np.int32)
    for opts in (ALL_DIRECT, ALL_GATHERED):
        _options(idx, opts)
        got = idx.search_filtered_each(q[:50], k, lists, loq)
        _defaults(idx)
        _same(got, _single(idx, q[:50], k, lists, loq))
        _oracle_check(got[0], got[1], x, lists, loq, q[:50], k, live=live, id_base=1000)
        for row in got[1]:
            hit = row[row >= 0]
            assert hit.size == np.unique(hit).size
        assert np.all(got[1][loq == 2] == -1) and np.all(np.isneginf(got[0][loq == 2]))
        assert np.all((got[1][loq == 3][:, 0] == live[3] + 1000) & (got[1][loq == 3][:, 1] == -1))
    idx.close()


def test_ivf_equals_flat(ctx):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    x, q = _rows(192)
    flat = _index(ctx, 192)
    _defaults(flat)
    rng = np.random.default_rng(25)
    ivf = VectorIndex(ctx, 192, INDEX_IVF_FLAT, 32)
    ivf.add(x)
    ivf.train(x, iters=4, seed=3)
    lists = [rng.choice(N + DUP, s, replace=False).astype(np.int64) for s in (2000, 64, 9000)]
    loq = rng.integers(0, 3, 40).astype(np.int32)
    _same(ivf.search_filtered_each(q[:40], 10, lists, loq), flat.search_filtered_each(q[:40], 10, lists, loq))
    ivf.close()


def test_group_equals_single_device(ctx):
    import torch
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, q = _rows(192)
    rng = np.random.default_rng(26)
    n = 12_007
    gctx = Context(devices=[0] * 3, exchange=EXCHANGE_COPY)
    g, s = VectorIndex(gctx, 192), VectorIndex(ctx, 192)
    drop = rng.choice(n, 1500, replace=False)
    for ix in (g, s):
        ix.add(x[:n])
        ix.delete(drop)
        ix.set_option("id_base", 500)
    live = np.setdiff1d(np.arange(n), drop)
    lists = [np.concatenate([rng.choice(live, 2500, replace=False), drop[:100], [-2, n + 3]]), rng.choice(live, 10, replace=False),
             np.array([], np.int64), np.concatenate([rng.choice(live, 300, replace=False)] * 2)]
    lists = [rng.permutation(a).astype(np.int64) for a in lists]
    b, k = 50, 10
    loq = rng.integers(0, len(lists), b).astype(np.int32)
    want = s.search_filtered_each(q[:b], k, lists, loq)
    _oracle_check(want[0], want[1], x[:n], lists, loq, q[:b], k, live=live, id_base=500)
    for opts in (ALL_DIRECT, ALL_GATHERED):
        _options(g, opts)
        _same(g.search_filtered_each(q[:b], k, lists, loq), want)
        qd = torch.from_numpy(q[:b]).cuda()
        ad = torch.from_numpy(np.concatenate(lists)).cuda()
        cos = torch.empty((b, k), dtype=torch.float32, device="cuda")
        ids = torch.empty((b, k), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        offsets = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
        g.search_filtered_each_device(qd.data_ptr(), b, k, ad.data_ptr(), offsets, loq, cos.data_ptr(), ids.data_ptr())
        gctx.synchronize()
        _same((cos.cpu().numpy(), ids.cpu().numpy()), want)
    for ix in (g, s):
        ix.close()
    gctx.close()


def test_device_form(ctx):
    import torch
    x, q = _rows(1024)
    idx = _index(ctx, 1024)
    _defaults(idx)
    rng = np.random.default_rng(27)
    lists = [rng.choice(N + DUP, s, replace=False).astype(np.int64) for s in (1500, 1, 0, 4000, 257)]
    b, k = 100, 10
    loq = rng.integers(0, len(lists), b).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
    qd = torch.from_numpy(q[:b]).cuda()
    ad = torch.from_numpy(np.concatenate(lists)).cuda()
    cos = torch.full((b, k), 7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((b, k), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    off2, loq2 = offsets.copy(), loq.copy()
    idx.search_filtered_each_device(qd.data_ptr(), b, k, ad.data_ptr(), off2, loq2, cos.data_ptr(), ids.data_ptr())
    off2[:] = -1                                                # the host arrays are not retained past return
    loq2[:] = 99
    ctx.synchronize()
    want = idx.search_filtered_each(q[:b], k, lists, loq)
    _same((cos.cpu().numpy(), ids.cpu().numpy()), want)
    _oracle_check(want[0], want[1], x, lists, loq, q[:b], k)


def test_owner_state_untouched_and_changes_seen(ctx):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    x, q = _rows(1024)
    rng = np.random.default_rng(28)
    idx = VectorIndex(ctx, 1024)
    idx.add(x[:N])
    idx.set_option("scan_mode", SCAN_INT8_RESCORE)
    idx.set_option("i8_min_rows", 0)
    idx.set_option("i8_sample_step", 8)                         # the int8 pass needs 1024 x step rows
    k = 10
    plain0 = idx.search(q[:256], k)
    last0 = idx.i8_last()
    assert last0["rows"] == N                                   # an int8 search ran
    lists = [rng.choice(N, s, replace=False).astype(np.int64) for s in (800, 3000, 50)]
    lists[0][:3] = [5, 6, 7]
    loq = rng.integers(0, 3, 64).astype(np.int32)
    for opts in (ALL_DIRECT, ALL_GATHERED):
        _options(idx, opts)
        idx.search_filtered_each(q[:64], k, lists, loq)
        _defaults(idx)
        assert idx.i8_last() == last0
        _same(idx.search(q[:256], k), plain0)
        assert idx.i8_last() == last0
    # rows added, updated and deleted between two calls are seen by the second
    idx.add(x[N:])                                              # ids N .. N + DUP - 1
    new = rng.standard_normal((1, 1024)).astype(np.float32)
    idx.update(np.array([5], np.int64), q[0:1] + 0.01 * new)    # row 5 becomes the best hit of query 0
    idx.delete(np.array([6], np.int64))
    lists[0] = np.concatenate([lists[0], N + np.arange(DUP)]).astype(np.int64)
    loq[0] = 0
    x2 = np.concatenate([x[:N], x[N:]])
    x2[5] = q[0] + 0.01 * new[0]
    live = np.setdiff1d(np.arange(N + DUP), [6])
    second = idx.search_filtered_each(q[:64], k, lists, loq)
    _oracle_check(second[0], second[1], x2, lists, loq, q[:64], k, live=live)
    assert second[1][0, 0] == 5 and not np.any(second[1] == 6)
    _same(second, _single(idx, q[:64], k, lists, loq))
    idx.close()


def test_invalid_arguments_write_nothing(ctx):
    from semantic_query_engine_amd import _native as NV
    x, q = _rows(64)
    idx = _index(ctx, 64)
    lib = idx.lib
    b, k = 4, 3
    qq = np.ascontiguousarray(q[:b])
    allow = np.arange(10, dtype=np.int64)
    good_off = np.array([0, 4, 10], np.int64)
    good_loq = np.array([0, 1, 1, 0], np.int32)

    def call(off=good_off, n_lists=2, loq=good_loq, kk=k, allow_p=allow.ctypes.data, q_p=qq.ctypes.data, null_out=False,
             null_loq=False, null_off=False, null_ids=False):
        cos = np.full((b, max(kk, 1)), 3.5, np.float32)
        ids = np.full((b, max(kk, 1)), 77, np.int64)
        rc = lib.sqe_index_search_filtered_each(idx.handle, q_p, b, kk, allow_p, None if null_off else off.ctypes.data, n_lists,
                                                None if null_loq else loq.ctypes.data, None if null_out else cos.ctypes.data,
                                                None if null_ids else ids.ctypes.data)
        return rc, cos, ids

    rc, cos, ids = call()
    assert rc == 0 and np.all(ids[:, 0] >= 0)
    bad = [
        dict(off=np.array([1, 4, 10], np.int64)),                # not starting at 0
        dict(off=np.array([0, 6, 4], np.int64)),                 # decreasing
        dict(n_lists=-1),
        dict(loq=np.array([0, 2, 1, 0], np.int32)),              # outside [0, n_lists)
        dict(loq=np.array([0, -1, 1, 0], np.int32)),
        dict(kk=0), dict(kk=257),
        dict(allow_p=None), dict(q_p=None), dict(null_out=True), dict(null_ids=True), dict(null_loq=True), dict(null_off=True),
        dict(n_lists=0),                                         # B > 0 queries but no list to name
    ]
    for kw in bad:
        rc, cos, ids = call(**kw)
        assert rc == -1, kw                                      # SQE_ERR_INVALID
        assert np.all(cos == 3.5) and np.all(ids == 77), kw
        with pytest.raises(NV.SqeError) as e:
            NV.check(rc)
        assert e.value.code == -1
    with pytest.raises(NV.SqeError):
        idx.search_filtered_each(qq, k, [allow[:4], allow[4:]], np.array([0, 5, 1, 0], np.int32))
    with pytest.raises(ValueError):
        idx.search_filtered_each(qq, k, [allow])                 # one list for four queries needs list_of_query
    # valid edge cases: no queries (with and without lists), an empty index
    empty_q = np.empty((0, 64), np.float32)
    assert idx.search_filtered_each(empty_q, k, [])[0].shape == (0, k)
    assert idx.search_filtered_each(empty_q, k, [allow], np.empty(0, np.int32))[1].shape == (0, k)
    from semantic_query_engine_amd import VectorIndex
    e = VectorIndex(ctx, 64)
    cos, ids = e.search_filtered_each(qq, k, [allow], np.zeros(b, np.int32))
    assert np.all(ids == -1) and np.all(np.isneginf(cos))
    e.close()
