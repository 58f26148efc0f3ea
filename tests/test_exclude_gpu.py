"""Exclusion k-NN search (sqe_index_search_excluding, exclude.hip): per query the exact top-k of the live rows that are not on
the query's deny-list.  GPU only.

Everything is compared bit for bit (cosines and ids) with what the library's own exact searches return:
  * the oracle of a list with k + len <= 256: ``search(q, k + len)`` with the listed ids removed, first k;
  * the oracle of any list: ``search(q, k, filter_ids=complement)`` (the route such a request took before).
With k + len > 256 the first oracle does not hold k rows, so those lists (every non-empty list at k = 256) are checked against
the second, and they are the queries the sweep answers: ``exclude_swept()`` counts exactly them.  The sweep is also checked
against a float64 NumPy ranking with the near-tie allowance of tests/test_collapse_gpu.py."""
import numpy as np
import pytest

from tests.test_collapse_gpu import NONE, compare, reference, same_bits

pytestmark = pytest.mark.gpu

N, D = 4096, 128
LENS = (0, 1, 7, 55, 246, 7, None)            # the deny-list length of each of the B = 7 queries; None: no list


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(41)
    return rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((1025, D)).astype(np.float32)


@pytest.fixture(scope="module")
def index(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, D)
    idx.add(data[0])
    return idx


@pytest.fixture(scope="module")
def top256(index, data):
    """ids [1025, 256] of the plain search at depth 256: what the lists are cut from"""
    return index.search(data[1], 256)[1]


def _lists(top, lens):
    return [None if n is None else top[b, :n].copy() for b, n in enumerate(lens)]


def oracle(idx, q, k, lists, loq=None, all_ids=None):
    """Row b by the oracles of the module docstring; a query without a list: ``search(q, k)``."""
    b = q.shape[0]
    loq = np.arange(b) if loq is None else np.asarray(loq)
    cos = np.full((b, k), -np.inf, np.float32)
    ids = np.full((b, k), -1, np.int64)
    for i in range(b):
        deny = None if loq[i] < 0 else lists[loq[i]]
        if deny is None:
            c, d = idx.search(q[i:i + 1], k)
        elif k + len(deny) <= 256:
            c, d = idx.search(q[i:i + 1], k + len(deny))
            keep = ~np.isin(d[0], deny) & (d[0] >= 0)
            c, d = c[:, keep][:, :k], d[:, keep][:, :k]
        else:
            live = idx.ids() if all_ids is None else all_ids
            c, d = idx.search(q[i:i + 1], k, filter_ids=np.setdiff1d(live, deny))
        cos[i, :c.shape[1]], ids[i, :d.shape[1]] = c[0], d[0]
    return cos, ids


def _swept_expected(k, lens):
    return sum(1 for n in lens if n and k + n > 256)


# ---------------------------------------------------------------- 1. the plain search with the denied rows dropped
@pytest.mark.parametrize("k", [1, 10, 256])
def test_equals_plain_search_minus_denied(ctx, data, index, top256, k):
    q = data[1][:7]
    lists = _lists(top256, LENS)
    got = index.search_excluding(q, k, lists)
    swept = ctx.exclude_swept()
    print(f"[exclude] k={k}: swept {swept} of 7")
    assert swept == _swept_expected(k, LENS) and (k == 256 or swept == 0)
    assert same_bits(got, oracle(index, q, k, lists))
    assert same_bits((got[0][6:], got[1][6:]), index.search(q[6:7], k))       # no list: the row of search
    for b, n in enumerate(LENS):                                              # the list really bites
        if n:
            assert not np.isin(got[1][b], lists[b]).any() and np.isin(index.search(q[b:b + 1], k)[1], lists[b]).any()
    # list_of_query = -1 names no list either, whatever the lists are
    loq = np.array([0, 1, 2, 3, 4, 5, -1], np.int32)
    assert same_bits(index.search_excluding(q, k, [top256[b, :n or 0] for b, n in enumerate(LENS)], loq), got)


# ---------------------------------------------------------------- 2. the sweep
@pytest.mark.parametrize("k", [1, 10])
def test_depth_gives_same_bits(ctx, data, index, top256, k):
    q = data[1][:7]
    lists = _lists(top256, LENS)
    auto = index.search_excluding(q, k, lists)
    assert ctx.exclude_swept() == 0
    for depth in (k, 64, 256):
        index.set_option("exclude_depth", depth)
        got = index.search_excluding(q, k, lists)
        swept = ctx.exclude_swept()
        index.set_option("exclude_depth", 0)
        print(f"[exclude] k={k} exclude_depth={depth}: swept {swept} of 7")
        assert same_bits(auto, got), (k, depth)
        assert (swept > 0) == (depth < 256)
    index.set_option("range_key_budget", 4096)               # one slot per sweep group
    index.set_option("exclude_depth", k)
    small = index.search_excluding(q, k, lists)
    index.set_option("exclude_depth", 0)
    index.set_option("range_key_budget", 1 << 25)
    assert same_bits(auto, small)


def test_sweep_against_filtered_search_and_float64(ctx, data, index, top256):
    x, q = data[0], data[1][:7]
    rng = np.random.default_rng(42)
    k = 10
    lists = [np.concatenate([top256[b], rng.integers(0, N, 100)]) for b in range(7)]
    got = index.search_excluding(q, k, lists)
    assert ctx.exclude_swept() == 7
    all_ids = np.arange(N)
    for b in range(7):
        allow = np.setdiff1d(all_ids, lists[b])
        assert same_bits((got[0][b:b + 1], got[1][b:b + 1]), index.search(q[b:b + 1], k, filter_ids=allow)), b
        ref = reference(x[allow], q[b:b + 1], np.full(allow.shape[0], NONE), allow, k)
        compare((got[0][b:b + 1], got[1][b:b + 1], np.full((1, k), NONE)), ref, k, f"sweep query {b}", cap=False)


# ---------------------------------------------------------------- 3. ties and ids
def test_ties_go_to_the_lowest_surviving_id(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(43)
    base = rng.standard_normal((64, D)).astype(np.float32)
    idx = VectorIndex(ctx, D)
    idx.add(np.concatenate([base, base, base]))              # row i, i + 64 and i + 128 are one vector
    lists = [np.array([i], np.int64) if i % 3 == 0 else np.array([i, i + 64], np.int64) if i % 3 == 1 else np.array([i + 64], np.int64)
             for i in range(64)]
    cos, ids = idx.search_excluding(base, 3, lists)
    assert ctx.exclude_swept() == 0
    assert same_bits((cos, ids), oracle(idx, base, 3, lists))
    for i in range(64):
        want = [[i + 64, i + 128], [i + 128], [i, i + 128]][i % 3]
        assert ids[i, :len(want)].tolist() == want and np.all(cos[i, :len(want)] == cos[i, 0])
    idx.close()


def test_id_rules_after_delete(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data[0], data[1][:16]
    idx = VectorIndex(ctx, D)
    idx.add(x)
    dead = np.arange(0, N, 3)
    idx.delete(dead)                                         # ids != positions from here on
    live = idx.ids()
    top = idx.search(q, 64)[1]
    clean = [top[b, :20].copy() for b in range(16)]
    messy = [np.concatenate([top[b, :20][::-1], dead[:5], [N, N + 77, 1 << 40, -1, -(1 << 40)], top[b, :20], top[b, :3]]) for b in range(16)]
    for k in (5, 10):
        want = oracle(idx, q, k, clean)
        assert same_bits(idx.search_excluding(q, k, clean), want)
        assert ctx.exclude_swept() == 0
        assert same_bits(idx.search_excluding(q, k, messy), want)
        for b in range(16):
            assert same_bits((want[0][b:b + 1], want[1][b:b + 1]), idx.search(q[b:b + 1], k, filter_ids=np.setdiff1d(live, clean[b])))
    deep = idx.search(q, 256)[1]
    got = idx.search_excluding(q, 10, [np.concatenate([deep[b], dead]) for b in range(16)])      # the sweep maps ids too
    assert ctx.exclude_swept() == 16
    for b in range(16):
        assert same_bits((got[0][b:b + 1], got[1][b:b + 1]), idx.search(q[b:b + 1], 10, filter_ids=np.setdiff1d(live, deep[b])))
    idx.set_option("id_base", 1000)                          # id_base is added to the answers, the deny ids stay local
    based = idx.search_excluding(q, 10, clean)
    idx.set_option("id_base", 0)
    want = oracle(idx, q, 10, clean)
    assert same_bits(based, (want[0], np.where(want[1] >= 0, want[1] + 1000, -1)))
    idx.close()


# ---------------------------------------------------------------- 4. padding
def test_padding_empty_index_and_no_queries(ctx, data, index):
    from semantic_query_engine_amd import VectorIndex
    q = data[1][:5]
    every = np.arange(N)
    cos, ids = index.search_excluding(q, 10, [every], np.zeros(5, np.int32))
    assert np.all(np.isneginf(cos)) and np.all(ids == -1)
    keep = np.array([5, 1000, 4095])
    cos, ids = index.search_excluding(q, 10, [np.setdiff1d(every, keep)], np.zeros(5, np.int32))
    assert same_bits((cos, ids), index.search(q, 10, filter_ids=keep))
    assert np.all(ids[:, :3] >= 0) and np.all(ids[:, 3:] == -1) and np.all(np.isneginf(cos[:, 3:]))
    empty = VectorIndex(ctx, D)
    cos, ids = empty.search_excluding(q, 4, [np.array([1, 2, 3])], np.zeros(5, np.int32))
    assert np.all(np.isneginf(cos)) and np.all(ids == -1)
    empty.close()
    cos, ids = index.search_excluding(np.zeros((0, D), np.float32), 3, [])
    assert cos.shape == (0, 3) and ids.shape == (0, 3)
    cos, ids = index.search_excluding(q, 3, [], np.full(5, -1, np.int32))      # no lists at all
    assert same_bits((cos, ids), index.search(q, 3))
    small = VectorIndex(ctx, D)                              # fewer rows than k + len: nothing to flag, padding behind the survivors
    small.add(data[0][:12])
    cos, ids = small.search_excluding(q, 10, [np.array([0, 3, 11, 11])], np.zeros(5, np.int32))
    assert ctx.exclude_swept() == 0
    assert same_bits((cos, ids), small.search(q, 10, filter_ids=np.setdiff1d(np.arange(12), [0, 3, 11])))
    small.close()


# ---------------------------------------------------------------- 5. batch independence
def test_batch_independence_across_the_pass(ctx, data, index, top256):
    q = data[1]
    rng = np.random.default_rng(44)
    k = 10
    lists = [top256[0, :3].copy(), top256[511, :40].copy(),
             np.concatenate([top256[2], np.setdiff1d(rng.permutation(N)[:400], top256[2])[:44]])]
    assert [len(a) for a in lists] == [3, 40, 300]
    loq = (np.arange(1025) % 3).astype(np.int32)
    loq[7::50] = -1
    assert loq[0] == 0 and loq[511] == 1 and loq[1023] == 0 and loq[1024] == 1 and loq[2] == 2
    cos, ids = index.search_excluding(q, k, lists, loq)
    swept = ctx.exclude_swept()                              # of the queries of the long list, those whose own top 256 it emptied
    print(f"[exclude] B=1025: swept {swept} of {int((loq == 2).sum())} queries of the list of 300")
    assert 1 <= swept <= int((loq == 2).sum())
    for b in (0, 2, 7, 511, 1023, 1024):
        one = index.search_excluding(q[b:b + 1], k, [lists[loq[b]]] if loq[b] >= 0 else [None])
        assert same_bits((cos[b:b + 1], ids[b:b + 1]), one), b
    assert not np.isin(ids[0], lists[0]).any() and not np.isin(ids[511], lists[1]).any() and not np.isin(ids[2], lists[2]).any()
    # every query of the two short lists and every query without one against the oracle: two searches of the whole batch
    c50, i50 = index.search(q, k + 40)
    for f in (-1, 0, 1):
        for b in np.flatnonzero(loq == f)[::17]:
            keep = np.ones(k + 40, bool) if f < 0 else ~np.isin(i50[b], lists[f])
            assert np.array_equal(ids[b], i50[b][keep][:k]) and np.array_equal(cos[b].view(np.uint32), c50[b][keep][:k].view(np.uint32)), b


# ---------------------------------------------------------------- 6. the int8 first pass stays on for the shallow class
def test_int8_first_pass_kept(ctx):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex, _native
    rng = np.random.default_rng(45)
    n, d, k = 8192, 256, 5
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((6, d)).astype(np.float32)
    q[:3] = x[[10, 4000, 8000]] + 0.1 * q[:3]
    idx = VectorIndex(ctx, d)
    idx.set_option("scan_mode", SCAN_INT8_RESCORE)
    idx.set_option("i8_min_rows", 0)
    idx.set_option("i8_sample_step", 4)                      # 32 tiles: the default step of 100 would leave no sample
    idx.add(x)
    plain = VectorIndex(ctx, d)                              # a bf16 index cuts the lists: no int8 search before the call
    plain.add(x)
    top = plain.search(q, 64)[1]
    lists = [top[b, :3 if b % 2 == 0 else 60].copy() for b in range(6)]
    with pytest.raises(_native.SqeError):
        idx.i8_last()                                        # no int8 search yet
    got = idx.search_excluding(q, k, lists)
    last = idx.i8_last()
    print(f"[exclude] int8: rows {last['rows']}, depth {last['k']}, swept {ctx.exclude_swept()}")
    assert last["rows"] == n and last["k"] == k + 3          # the shallow class: three queries at depth 8
    assert ctx.exclude_swept() == 0
    assert same_bits(got, oracle(idx, q, k, lists))
    idx.close()
    plain.close()


# ---------------------------------------------------------------- 7. IVF equals FLAT
def test_ivf_equals_flat(ctx, data, index, top256):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    x, q = data[0], data[1][:9]
    ivf = VectorIndex(ctx, D, INDEX_IVF_FLAT, 16)
    ivf.add(x)
    ivf.train(x, iters=5, seed=1)
    lens = (0, 1, 7, 55, 246, 256, None, 30, None)
    lists = _lists(top256, lens)
    for k in (10, 64):
        got = ivf.search_excluding(q, k, lists)
        assert ctx.exclude_swept() == 7                      # every query that names a list
        want = index.search_excluding(q, k, lists)
        named = [b for b, n in enumerate(lens) if n is not None]
        assert same_bits((got[0][named], got[1][named]), (want[0][named], want[1][named])), k
        for b in (6, 8):                                     # no list: the IVF index's own search
            assert same_bits((got[0][b:b + 1], got[1][b:b + 1]), ivf.search(q[b:b + 1], k))
    ivf.close()


# ---------------------------------------------------------------- 8. device groups
@pytest.mark.parametrize("P", [2, 3])
def test_group_equals_single_device(ctx, data, index, top256, P):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, q = data[0], data[1][:8]
    rng = np.random.default_rng(46)
    on_shard0 = [np.array([i for i in top256[b] if i % 6 == 0][:n], np.int64) for b, n in ((0, 5), (1, 30))]
    lists = on_shard0 + [top256[2, :7].copy(), top256[3, :100].copy(), np.concatenate([top256[4], rng.integers(0, N, 100)]),
                         np.array([-5, N + 3, 1 << 40], np.int64), None, top256[7, :246].copy()]
    gctx = Context(devices=[0] * P, exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    g.add(x)
    for k in (1, 10):
        want = index.search_excluding(q, k, lists)
        swept = ctx.exclude_swept()
        assert swept == 1                                    # the list of 356
        assert same_bits(g.search_excluding(q, k, lists), want), (P, k)
    g.set_option("exclude_depth", 10)                        # forwarded to every shard
    got = g.search_excluding(q, 10, lists)
    g.set_option("exclude_depth", 0)
    assert gctx.exclude_swept() > 0 and same_bits(got, index.search_excluding(q, 10, lists))      # summed over the shards
    g.close()
    gctx.close()


# ---------------------------------------------------------------- 9. the _device entry and the invalid arguments
def test_device_form(ctx, data, index, top256):
    import torch
    q = data[1][:7]
    for k, lens in ((10, LENS), (256, LENS)):
        lists = _lists(top256, lens)
        host = index.search_excluding(q, k, lists)
        swept = ctx.exclude_swept()
        arrays = [np.empty(0, np.int64) if a is None else a for a in lists]
        offsets = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrays])]).astype(np.int64)
        loq = np.array([-1 if a is None else b for b, a in enumerate(lists)], np.int32)
        qd = torch.from_numpy(q).cuda()
        dd = torch.from_numpy(np.concatenate(arrays)).cuda()
        cd = torch.empty((7, k), dtype=torch.float32, device="cuda")
        idd = torch.empty((7, k), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        index.search_excluding_device(qd.data_ptr(), 7, k, dd.data_ptr(), offsets, loq, cd.data_ptr(), idd.data_ptr())
        ctx.synchronize()
        assert same_bits(host, (cd.cpu().numpy(), idd.cpu().numpy())) and ctx.exclude_swept() == swept


def test_invalid_arguments_write_nothing(ctx, data, index):
    import torch
    from semantic_query_engine_amd import _native
    lib = _native.load()
    b, k = 3, 4
    q = np.ascontiguousarray(data[1][:b])
    deny = np.arange(10, dtype=np.int64)
    good_off = np.array([0, 4, 10], np.int64)
    good_loq = np.array([0, 1, -1], np.int32)
    cos = np.full((b, k), 7.5, np.float32)
    ids = np.full((b, k), -77, np.int64)

    def call(kk=k, bb=b, qp=q.ctypes.data, dp=deny.ctypes.data, off=good_off, n_lists=2, loq=good_loq, cp=cos.ctypes.data,
             ip=ids.ctypes.data, handle=index.handle):
        return lib.sqe_index_search_excluding(handle, qp, bb, kk, dp, None if off is None else off.ctypes.data, n_lists,
                                              None if loq is None else loq.ctypes.data, cp, ip)

    bad = [dict(kk=0), dict(kk=257), dict(bb=-1), dict(n_lists=-1), dict(off=np.array([1, 4, 10], np.int64)),
           dict(off=np.array([0, 6, 4], np.int64)), dict(loq=np.array([0, 2, 1], np.int32)), dict(loq=np.array([0, -2, 1], np.int32)),
           dict(qp=None), dict(cp=None), dict(ip=None), dict(loq=None), dict(off=None), dict(dp=None), dict(handle=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert np.all(cos == 7.5) and np.all(ids == -77), kw
    # the _device form checks the same before it touches the device
    qd = torch.from_numpy(q).cuda()
    dd = torch.from_numpy(deny).cuda()
    cd = torch.full((b, k), 7.5, dtype=torch.float32, device="cuda")
    idd = torch.full((b, k), -77, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for off, loq, kk in ((np.array([2, 4, 10], np.int64), good_loq, k), (good_off, np.array([0, 1, 2], np.int32), k), (good_off, good_loq, 300)):
        assert lib.sqe_index_search_excluding_device(index.handle, qd.data_ptr(), b, kk, dd.data_ptr(), off.ctypes.data, 2,
                                                     loq.ctypes.data, cd.data_ptr(), idd.data_ptr()) == -1
    ctx.synchronize()
    assert bool((cd == 7.5).all()) and bool((idd == -77).all())
    assert call() == 0 and call(bb=0) == 0 and np.all(ids[:, 0] >= 0)
    assert lib.sqe_exclude_swept(None, None) == -1
    with pytest.raises(_native.SqeError):
        index.set_option("exclude_depth", 257)
    with pytest.raises(ValueError):
        index.search_excluding(q, k, [deny])                 # one list for three queries needs list_of_query
    with pytest.raises(_native.SqeError):
        index.search_excluding(q, k, [deny], np.array([0, 0, 1], np.int32))


# ---------------------------------------------------------------- 10. the clause route
def test_clause_route(ctx):
    from semantic_query_engine_amd import retrieval as RT
    rng = np.random.default_rng(47)
    n_docs, chunks = 40, 5
    x = rng.standard_normal((n_docs * chunks, D)).astype(np.float32)
    docs = [{"doc_id": f"d{d}", "text": f"chunk {c} of {d}"} for d in range(n_docs) for c in range(chunks)]
    client = RT.GpuSearchClient(ctx, dim=D)
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x, docs)
    idx = client.index("idx")
    q = (x[[7, 50, 120, 199, 3]] + 0.3 * rng.standard_normal((5, D))).astype(np.float32)
    k = 6

    def hits_of(cos, ids):
        return [(idx.sources[int(r)]["text"], float(1.0 / (2.0 - float(c)))) for c, r in zip(cos, ids) if r >= 0]

    def by_allow_list(qq, clause):
        with idx.lock:
            allow = RT.filter_rows(idx, clause)
        cos, ids = idx.vectors.search(qq, k, filter_ids=allow)
        return cos, ids

    not_d1 = {"bool": {"must_not": [{"term": {"doc_id": "d1"}}]}}
    not_many = {"bool": {"must_not": [{"terms": {"doc_id": ["d10", "d24"]}}, {"ids": {"values": ["d0_3", "d39_199"]}}]}}
    only_d24 = {"term": {"doc_id": "d24"}}
    for clause, qq in ((not_d1, q[0:1]), (not_many, q[2:3]), (not_many, q[4:5])):
        want = by_allow_list(qq, clause)
        got = ix.search(qq, k=k, filter=clause)
        assert [(s["text"], sc) for s, sc in got] == hits_of(want[0][0], want[1][0]) and len(got) == k
    # exclude_ids: the direct form
    first = ix.search(q[0:1], k=k)
    shown = [f"{s['doc_id']}_{[d['text'] for d in docs].index(s['text'])}" for s, _ in first]
    nxt = ix.search(q[0:1], k=k, exclude_ids=shown + ["nope_1"])
    want = by_allow_list(q[0:1], {"bool": {"must_not": [{"ids": {"values": shown}}]}})
    assert [(s["text"], sc) for s, sc in nxt] == hits_of(want[0][0], want[1][0])
    assert not {s["text"] for s, _ in nxt} & {s["text"] for s, _ in first}
    both = ix.search(q[0:1], k=2 * k)
    assert [s["text"] for s, _ in both] == [s["text"] for s, _ in first] + [s["text"] for s, _ in nxt]
    with pytest.raises(ValueError):
        ix.search(q[0:1], k=k, filter=only_d24, exclude_ids=shown)
    # a batch: None, an allow clause and two must_not clauses, rows in request order
    filters = [not_d1, None, only_d24, not_many, not_d1]
    cos, ids = ix.search_batch(q, k=k, filters=filters)
    for b, flt in enumerate(filters):
        c1, i1 = idx.vectors.search(q[b:b + 1], k) if flt is None else by_allow_list(q[b:b + 1], flt)
        assert same_bits((cos[b:b + 1], ids[b:b + 1]), (c1, i1)), b
    with idx.lock:
        lists, loq, deny, doq = RT.resolve_routes(idx, filters)
    assert loq.tolist() == [-1, -1, 0, -1, -1] and doq.tolist() == [0, -1, -1, 1, 0] and len(lists) == 1 and len(deny) == 2
    assert deny[0].tolist() == [5, 6, 7, 8, 9] and deny[1].tolist() == sorted([3, 199] + list(range(50, 55)) + list(range(120, 125)))
