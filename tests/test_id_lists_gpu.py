"""The three searches that take id lists from the caller -- filtered (one allow-list), per-query filtered (an allow-list per
query) and exclusion (a deny-list per query) -- over the SAME lists: every list length around a power of two (the sizes of
the position sets), drawn three ways, with ids that name no row, a deleted id and every id three times over.  GPU only.

Everything is exact, cosines and ids bit for bit:
  * row b of ``search_filtered_each`` is ``search(q[b:b+1], k, filter_ids=list)``;
  * row b of ``search_excluding`` is the plain ``search`` at depth 256 without the denied ids, first k (k <= 10; the reference
    checks that it holds k rows or every live row), and at k = 256 ``search_filtered_each`` over the complement of the list;
  * the returned ids lie in list & live (outside the deny-list), and min(k, |list & live|) (min(k, live - |deny & live|))
    of them are no padding;
  * groups of 2 and 3 logical shards of device 0 give the single-device answers.
Three indexes: 4,096 rows without an id map; the same after deleting every third id (the first and the last among them), so
the map has holes at both ends; and one reduced to a single live row, where the binary search runs with n = 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D = 4096, 64
LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025)
KS = (1, 10, 256)
DELETED = {"full": np.empty(0, np.int64), "mapped": np.arange(0, N, 3), "one": np.delete(np.arange(N), 2000)}
assert DELETED["mapped"][0] == 0 and DELETED["mapped"][-1] == N - 1 and N - DELETED["mapped"].size == 2730
DIRECT = {"filter_each_direct_rows": 1 << 20, "filter_each_direct_queries": 4096}
DEFAULTS = {"filter_each_direct_rows": 1 << 14, "filter_each_direct_queries": 32}


def _make():
    rng = np.random.default_rng(2026)
    x = rng.standard_normal((N, D)).astype(np.float32)
    lists = []
    for n in LENS:
        start = int(rng.integers(0, N - 1025))
        for base in (np.arange(start, start + n), (start + 64 * np.arange(n)) % (N - 1), rng.permutation(N)[:n]):
            assert np.unique(base).size == n
            extra = [-1, N, N + 5, DELETED["mapped"][int(rng.integers(DELETED["mapped"].size))]]
            lists.append(rng.permutation(np.concatenate([base, extra, base, base]).astype(np.int64)))
    q = x[rng.integers(0, N, len(lists))] + 0.5 * rng.standard_normal((len(lists), D)).astype(np.float32)
    return x, q, lists


X, Q, LISTS = _make()
B = len(LISTS)


def _bits(a):
    return [np.ascontiguousarray(v).view(np.uint8) for v in a]


def same_bits(a, b):
    return len(a) == len(b) and all(u.shape == w.shape and np.array_equal(u, w) for u, w in zip(_bits(a), _bits(b)))


def _indexes(ctx):
    from semantic_query_engine_amd import VectorIndex
    out = {}
    for which, dead in DELETED.items():
        out[which] = VectorIndex(ctx, D)
        out[which].add(X)
        out[which].delete(dead)
        assert out[which].next_id == N and len(out[which]) == N - dead.size
    return out


@pytest.fixture(scope="module")
def single():
    from semantic_query_engine_amd import Context
    ctx = Context(0)
    yield ctx, _indexes(ctx)
    ctx.close()


@pytest.fixture(scope="module", params=[2, 3])
def group(request):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context
    ctx = Context(devices=[0] * request.param, exchange=EXCHANGE_COPY)
    yield ctx, _indexes(ctx)
    ctx.close()


def _each_single(idx, q, k, lists):
    out = [idx.search(q[b:b + 1], k, filter_ids=ids) for b, ids in enumerate(lists)]
    return np.concatenate([c for c, _ in out]), np.concatenate([i for _, i in out])


_ref = {}


def _reference(single, which, k):
    """(filtered rows, exclusion rows, live ids) of the single-device index, by the constructions of the module docstring;
    computed once per (index, k) and never written to"""
    if (which, k) not in _ref:
        idx = single[1][which]
        live = idx.ids()
        filt = _each_single(idx, Q, k, LISTS)
        if k < 256:
            c, d = idx.search(Q, 256)
            ex = np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int64)
            for b in range(B):
                keep = (d[b] >= 0) & ~np.isin(d[b], LISTS[b])
                assert live.size <= 256 or keep.sum() >= k          # the depth-256 ranking is enough
                m = min(k, int(keep.sum()))
                ex[0][b, :m], ex[1][b, :m] = c[b, keep][:m], d[b, keep][:m]
        else:
            ex = idx.search_filtered_each(Q, k, [np.setdiff1d(live, ids) for ids in LISTS])
        for v in filt + ex + (live,):
            v.flags.writeable = False
        _ref[(which, k)] = filt, ex, live
    return _ref[(which, k)]


def _check_sets(got_ids, k, live, allowed_of, what):
    for b in range(B):
        allowed = allowed_of(np.intersect1d(LISTS[b], live))
        hit = got_ids[b][got_ids[b] >= 0]
        assert np.isin(hit, allowed).all() and np.unique(hit).size == hit.size, (what, b)
        assert hit.size == min(k, allowed.size) and (got_ids[b, hit.size:] == -1).all(), (what, b, hit.size, allowed.size)


def _check_index(single, idx, which, k):
    """the three searches of `idx` (a single-device or a group index) against the single-device reference"""
    filt, ex, live = _reference(single, which, k)
    for opts in (DIRECT, DEFAULTS):
        for key, value in opts.items():
            idx.set_option(key, value)
        got = idx.search_filtered_each(Q, k, LISTS)
        assert same_bits(got, filt), opts
    _check_sets(got[1], k, live, lambda named: named, "filtered_each")
    got = idx.search_excluding(Q, k, LISTS)
    assert same_bits(got, ex)
    _check_sets(got[1], k, live, lambda named: np.setdiff1d(live, named), "excluding")
    return filt


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("which", list(DELETED))
def test_same_lists_through_all_three_searches(single, which, k):
    _check_index(single, single[1][which], which, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("which", list(DELETED))
def test_groups_give_the_single_device_answers(single, group, which, k):
    g = group[1][which]
    filt = _check_index(single, g, which, k)
    assert same_bits(_each_single(g, Q, k, LISTS), filt)


def test_group_routing_edges(single, group):
    """a list whose ids all live on one shard, a list without a live id, and an exclusion search without any list"""
    s, g = single[1]["mapped"], group[1]["mapped"]
    one_shard = np.arange(1, N, 6)[:300]                     # id % 2 == id % 3 == 1, none deleted
    no_live = np.concatenate([DELETED["mapped"][:50], [-1, N, N + 5]])
    assert not np.isin(one_shard, DELETED["mapped"]).any()
    lists, loq, q, k = [one_shard, no_live], [0, 1, 0, 1], Q[:4], 10
    want = s.search_filtered_each(q, k, lists, loq)
    assert (want[1][[1, 3]] == -1).all() and np.isin(want[1][[0, 2]], one_shard).all()
    assert same_bits(g.search_filtered_each(q, k, lists, loq), want)
    for f, ids in enumerate(lists):
        assert same_bits(g.search(q[f:f + 1], k, filter_ids=ids), (want[0][f:f + 1], want[1][f:f + 1]))
    want = s.search_excluding(q, k, lists, loq)
    assert same_bits((want[0][[1, 3]], want[1][[1, 3]]), s.search(q[[1, 3]], k)) and not np.isin(want[1][[0, 2]], one_shard).any()
    assert same_bits(g.search_excluding(q, k, lists, loq), want)
    none = [-1] * 4
    assert same_bits(g.search_excluding(q, k, [], none), s.search(q, k)) and same_bits(s.search_excluding(q, k, [], none), s.search(q, k))


def _device_forms(ctx, idx, k):
    """the `_device` entry points over LISTS (the single list: the longest random one) -> the three results"""
    import torch
    dev = torch.device("cuda", 0)
    offsets = np.concatenate([[0], np.cumsum([a.size for a in LISTS])]).astype(np.int64)
    loq = np.arange(B, dtype=np.int32)
    qd, ids = torch.from_numpy(Q).to(dev), torch.from_numpy(np.concatenate(LISTS)).to(dev)
    one = torch.from_numpy(LISTS[-1]).to(dev)
    out = [(torch.empty((B, k), dtype=torch.float32, device=dev), torch.empty((B, k), dtype=torch.int64, device=dev)) for _ in range(3)]
    torch.cuda.synchronize()
    idx.search_filtered_each_device(qd.data_ptr(), B, k, ids.data_ptr(), offsets, loq, out[0][0].data_ptr(), out[0][1].data_ptr())
    idx.search_excluding_device(qd.data_ptr(), B, k, ids.data_ptr(), offsets, loq, out[1][0].data_ptr(), out[1][1].data_ptr())
    idx.search_device(qd.data_ptr(), B, k, out[2][0].data_ptr(), out[2][1].data_ptr(), filter_ptr=one.data_ptr(), n_filter=LISTS[-1].size)
    ctx.synchronize()
    return [(c.cpu().numpy(), i.cpu().numpy()) for c, i in out]


def test_device_forms(single, group):
    k = 10
    filt, ex, _ = _reference(single, "mapped", k)
    want_one = single[1]["mapped"].search(Q, k, filter_ids=LISTS[-1])
    for ctx, indexes in (single, group):
        each, excl, one = _device_forms(ctx, indexes["mapped"], k)
        assert same_bits(each, filt) and same_bits(excl, ex) and same_bits(one, want_one)
