"""Row deletion (sqe_index_delete, compact.hip): the live rows are compacted in place keeping their order, an id map
(position -> id) translates search results, and ids are never reused.  Every search after a delete is compared with the
NumPy exact top-k over the live rows (ties to the lowest id) and, where it says most, with a fresh index built from the
live rows in id order.  GPU only."""
import os

import numpy as np
import pytest

from oracle import retrieval as R
from tests.gpu_util import assert_topk_matches, exact_topk_fast

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _live_oracle(x, live, q, k):
    """Exact top-k over the rows `live` (ascending ids) of x, ids mapped back."""
    ref_cos, ref_pos = R.knn_search(x[live], q, k)
    ref_ids = np.where(ref_pos >= 0, live[np.maximum(ref_pos, 0)], -1)
    return ref_cos, ref_ids


def _check_live(idx, x, live, q, k, id_base=0):
    cos, ids = idx.search(q, k)
    ref_cos, ref_ids = _live_oracle(x, live, q, k)
    ref_ids = np.where(ref_ids >= 0, ref_ids + id_base, -1)
    xn = np.zeros_like(x)
    xn[live] = R.normalize_rows(x[live])
    if id_base:
        xn = np.concatenate([np.zeros((id_base, x.shape[1]), np.float32), xn])
    assert_topk_matches(cos, ids, ref_cos, ref_ids, xn, R.normalize_rows(q))
    return cos, ids


def _fresh_equivalence(ctx, x, q, k, drop, options=()):
    from semantic_query_engine_amd import VectorIndex
    a = VectorIndex(ctx, x.shape[1])
    for key, v in options:
        a.set_option(key, v)
    a.add(x)
    a.search(q[:4], k)                                    # derived copies (int8) exist before the delete
    a.delete(drop)
    live = np.setdiff1d(np.arange(x.shape[0]), drop)
    assert len(a) == live.size and a.next_id == x.shape[0]
    assert np.array_equal(a.ids(), live)
    b = VectorIndex(ctx, x.shape[1])
    for key, v in options:
        b.set_option(key, v)
    b.add(x[live])
    ca, ia = a.search(q, k)
    cb, ib = b.search(q, k)
    assert np.array_equal(ia, np.where(ib >= 0, live[np.maximum(ib, 0)], -1))
    assert np.abs(ca - cb).max() <= 1e-6
    return a, live, ca, ia


def test_delete_equals_fresh_index_bf16(ctx):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((20000, 256)).astype(np.float32)
    q = rng.standard_normal((64, 256)).astype(np.float32)
    q[:16] = x[rng.integers(0, 20000, 16)] + 0.05 * q[:16]
    drop = rng.choice(20000, 2000, replace=False)
    a, live, ca, ia = _fresh_equivalence(ctx, x, q, 10, drop)
    _check_live(a, x, live, q, 10)
    assert not np.isin(ia, drop).any()


def test_delete_equals_fresh_index_int8(ctx):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE
    rng = np.random.default_rng(2)
    n, d, k = 300_000, 256, 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((200, d)).astype(np.float32)
    q[:50] = x[rng.integers(0, n, 50)] + 0.1 * q[:50]
    drop = rng.choice(n, n // 10, replace=False)
    opts = (("scan_mode", SCAN_INT8_RESCORE), ("i8_min_rows", 0))
    a, live, ca, ia = _fresh_equivalence(ctx, x, q, k, drop, opts)
    L = a.i8_last()                                      # the search after the delete ran the int8 first pass
    assert L["rows"] == live.size and L["B"] == 200
    ref_cos, ref_pos = exact_topk_fast(x[live], q, k)
    ref_ids = live[ref_pos]
    xn = np.zeros_like(x)
    xn[live] = R.normalize_rows(x[live])
    assert_topk_matches(ca, ia, ref_cos, ref_ids, xn, R.normalize_rows(q))


def test_adversarial_deletes(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(3)
    n, d, k = 6000, 128, 10
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((40, d)).astype(np.float32)
    idx = VectorIndex(ctx, d)
    idx.add(x)
    # every query's exact top-k goes: the next k come back
    _, top = R.knn_search(x, q, k)
    drop = np.unique(top)
    idx.delete(drop)
    live = np.setdiff1d(np.arange(n), drop)
    _check_live(idx, x, live, q, k)
    # B > 1024: the multi-pass path translates every pass
    qb = rng.standard_normal((1500, d)).astype(np.float32)
    _check_live(idx, x, live, qb, 5)
    # leave 3 live rows with k = 10: 3 hits, then padding
    keep = live[[7, 500, len(live) - 1]]
    idx.delete(np.setdiff1d(live, keep))
    assert len(idx) == 3 and np.array_equal(idx.ids(), keep)
    cos, ids = _check_live(idx, x, keep, q, k)
    assert np.all(ids[:, 3:] == -1) and np.all(np.isneginf(cos[:, 3:]))
    # delete everything: (-inf, -1), len 0, and a later add continues at next_id
    idx.delete(keep)
    assert len(idx) == 0 and idx.next_id == n
    cos, ids = idx.search(q, k)
    assert np.all(ids == -1) and np.all(np.isneginf(cos))
    idx.add(x[:5])
    assert np.array_equal(idx.ids(), np.arange(n, n + 5))
    cos, ids = idx.search(x[2:3], 1)
    assert ids[0, 0] == n + 2 and abs(cos[0, 0] - 1.0) < 1e-5


def test_duplicate_rows_tie_to_lowest_surviving_id(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3000, 128)).astype(np.float32)
    x[100] = x[1200] = x[2500] = x[40]
    idx = VectorIndex(ctx, 128)
    idx.add(x)
    cos, ids = idx.search(x[40:41] * 2.0, 4)
    assert ids[0].tolist()[:4] == [40, 100, 1200, 2500]
    idx.delete([40, 1200])
    cos, ids = idx.search(x[40:41] * 2.0, 4)
    assert ids[0, :2].tolist() == [100, 2500] and cos[0, 0] == cos[0, 1]


def test_id_base(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(5)
    x = rng.standard_normal((4000, 128)).astype(np.float32)
    q = rng.standard_normal((30, 128)).astype(np.float32)
    idx = VectorIndex(ctx, 128)
    idx.set_option("id_base", 1_000_000)
    idx.add(x)
    drop = rng.choice(4000, 700, replace=False)
    idx.delete(drop)                                     # ids are local: no id_base
    live = np.setdiff1d(np.arange(4000), drop)
    _check_live(idx, x, live, q, 10, id_base=1_000_000)


def test_interleaving_and_invalid_ids(ctx):
    from semantic_query_engine_amd import VectorIndex
    from semantic_query_engine_amd._native import SqeError
    rng = np.random.default_rng(6)
    d = 128
    x = rng.standard_normal((3000, d)).astype(np.float32)
    ref = {}                                             # id -> raw row
    idx = VectorIndex(ctx, d)
    idx.add(x[:1000]); ref.update({i: x[i] for i in range(1000)})
    idx.delete(np.arange(0, 1000, 3)); [ref.pop(i) for i in range(0, 1000, 3)]
    idx.add(x[1000:2000]); ref.update({i: x[i] for i in range(1000, 2000)})
    assert idx.next_id == 2000 and len(idx) == len(ref)
    upd = np.array([1, 1001, 998])
    new = rng.standard_normal((3, d)).astype(np.float32)
    idx.update(upd, new)
    for i, v in zip(upd, new):
        ref[int(i)] = v
    idx.delete(np.arange(1500, 1700)); [ref.pop(i) for i in range(1500, 1700)]
    live = np.array(sorted(ref))
    assert np.array_equal(idx.ids(), live) and len(idx) == live.size
    assert np.all(np.diff(idx.ids()) > 0)
    got = idx.get_rows(live)
    assert np.allclose(got, R.normalize_rows(np.stack([ref[i] for i in live])), atol=1e-6)
    before_ids, before_rows = idx.ids(), idx.get_rows(live)
    xr = np.zeros((2000, d), np.float32)
    for i, v in ref.items():
        xr[i] = v
    q = rng.standard_normal((20, d)).astype(np.float32)
    q[:3] = new * 2
    _check_live(idx, xr, live, q, 10)
    # deleted, never-assigned or repeated ids: SQE_ERR_INVALID and nothing changes
    for bad in ([0], [2000], [-1], [2, 2], [4, 1500]):
        with pytest.raises(SqeError) as e:
            idx.delete(bad)
        assert e.value.code == -1
    for bad in ([3], [5000]):
        with pytest.raises(SqeError):
            idx.update(np.array(bad), new[:1])
        with pytest.raises(SqeError):
            idx.get_rows(np.array(bad))
    assert np.array_equal(idx.ids(), before_ids) and np.array_equal(idx.get_rows(live), before_rows)
    assert idx.next_id == 2000


def test_ivf_with_deletes(ctx):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    rng = np.random.default_rng(7)
    n, d, k, nlist = 30000, 128, 10, 64
    cen = rng.standard_normal((200, d)).astype(np.float32)
    x = (cen[rng.integers(0, 200, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    q = (x[rng.integers(0, n, 48)] + 0.2 * rng.standard_normal((48, d))).astype(np.float32)
    idx = VectorIndex(ctx, d, INDEX_IVF_FLAT, nlist)
    idx.add(x[:20000])
    idx.train(x[:20000], iters=8, seed=3)
    idx.search(q[:2], k, nprobe=4)
    drop = rng.choice(20000, 3000, replace=False)
    idx.delete(drop)

    def check(live):
        centroids, assign = idx.ivf_export(nlist)
        assert assign.shape == (live.size,)
        xn, qn = R.normalize_rows(x[live]), R.normalize_rows(q)
        for nprobe in (1, 8):
            cos, ids = idx.search(q, k, nprobe=nprobe)
            ref_cos, ref_pos = R.ivf_search(xn, qn, centroids, assign, k, nprobe)
            ref_ids = np.where(ref_pos >= 0, live[np.maximum(ref_pos, 0)], -1)
            xfull = np.zeros((n, d), np.float32)
            xfull[live] = xn
            assert_topk_matches(cos, ids, ref_cos, ref_ids, xfull, qn)
        _, exact_pos = R.exact_topk(xn, qn, k)
        _, ids8 = idx.search(q, k, nprobe=8)
        assert R.recall_at_k(ids8, live[exact_pos]) >= 0.95

    live = np.setdiff1d(np.arange(20000), drop)
    check(live)
    idx.add(x[20000:])                                   # rows added after the delete get ids 20000 ..
    live = np.concatenate([live, np.arange(20000, n)])
    drop2 = live[rng.choice(live.size, 2000, replace=False)]
    idx.delete(drop2)
    live = np.setdiff1d(live, drop2)
    check(live)


@pytest.mark.parametrize("P", [2, 3])
def test_group_deletes(P, tmp_path):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    gctx = Context(devices=[0] * P, exchange=EXCHANGE_COPY)
    rng = np.random.default_rng(8 + P)
    n, d, k = 5003, 256, 10
    x = rng.standard_normal((n + 100, d)).astype(np.float32)
    q = rng.standard_normal((50, d)).astype(np.float32)
    idx = VectorIndex(gctx, d)
    idx.add(x[:n])
    drop = rng.choice(n, 800, replace=False)
    idx.delete(drop)
    live = np.setdiff1d(np.arange(n), drop)
    assert len(idx) == live.size and np.array_equal(idx.ids(), live) and idx.next_id == n
    _check_live(idx, x, live, q, k)
    # adds after deletes land on next_id % P: searched back by their global ids
    idx.add(x[n:n + 100])
    live = np.concatenate([live, np.arange(n, n + 100)])
    assert np.array_equal(idx.ids(), live)
    cos, ids = idx.search(x[n + 7:n + 8], 1)
    assert ids[0, 0] == n + 7
    assert np.allclose(idx.get_rows(live[[0, 5, -1]]), R.normalize_rows(x[live[[0, 5, -1]]]), atol=1e-6)
    idx.update(np.array([n + 7]), q[:1])
    cos, ids = idx.search(q[:1], 1)
    assert ids[0, 0] == n + 7
    x[n + 7] = q[0]
    _check_live(idx, x, live, q, k)
    with pytest.raises(Exception):
        idx.delete([int(drop[0])])
    # a group save with holes loads on a single device: same ids, same results
    p = str(tmp_path / "g.sqeidx")
    idx.save(p)
    from semantic_query_engine_amd import Context as C1
    one = VectorIndex.load(C1(0), p)
    assert np.array_equal(one.ids(), live) and one.next_id == n + 100
    c1, i1 = one.search(q, k)
    cg, ig = idx.search(q, k)
    assert np.array_equal(i1, ig) and np.array_equal(c1, cg)
    # ... and back onto a group
    back = VectorIndex.load(gctx, p)
    cb, ib = back.search(q, k)
    assert np.array_equal(ib, ig) and np.array_equal(cb, cg) and back.next_id == n + 100
    back.add(x[:1])
    assert back.ids()[-1] == n + 100


def test_persistence_with_holes(ctx, tmp_path):
    from semantic_query_engine_amd import VectorIndex, INDEX_IVF_FLAT
    rng = np.random.default_rng(9)
    x = rng.standard_normal((5000, 256)).astype(np.float32)
    q = rng.standard_normal((33, 256)).astype(np.float32)
    a = VectorIndex(ctx, 256)
    a.add(x)
    p1 = str(tmp_path / "v1.sqeidx")
    a.save(p1)                                           # no deletes: the version 1 file of the old size
    assert os.path.getsize(p1) == 64 + 5000 * 256 * 4
    assert int.from_bytes(open(p1, "rb").read()[8:12], "little") == 1
    a.delete(rng.choice(5000, 321, replace=False))
    a.delete([4999])
    p2 = str(tmp_path / "v2.sqeidx")
    a.save(p2)
    assert int.from_bytes(open(p2, "rb").read()[8:12], "little") == 2
    assert os.path.getsize(p2) == 64 + len(a) * 256 * 4 + 8 + len(a) * 8
    b = VectorIndex.load(ctx, p2)
    assert np.array_equal(a.ids(), b.ids()) and a.next_id == b.next_id == 5000
    ca, ia = a.search(q, 10)
    cb, ib = b.search(q, 10)
    assert np.array_equal(ia, ib) and np.array_equal(ca, cb)
    b.add(x[:2])
    assert b.ids()[-2:].tolist() == [5000, 5001]
    # IVF with holes
    cen = rng.standard_normal((64, 128)).astype(np.float32)
    xi = (cen[rng.integers(0, 64, 8000)] + 0.3 * rng.standard_normal((8000, 128))).astype(np.float32)
    iv = VectorIndex(ctx, 128, INDEX_IVF_FLAT, 32)
    iv.add(xi)
    iv.train(xi, iters=5, seed=1)
    iv.delete(np.arange(0, 8000, 7))
    p3 = str(tmp_path / "ivf.sqeidx")
    iv.save(p3)
    jv = VectorIndex.load(ctx, p3)
    assert np.array_equal(iv.ids(), jv.ids())
    c1, i1 = iv.search(xi[:20], 5, nprobe=4)
    c2, i2 = jv.search(xi[:20], 5, nprobe=4)
    assert np.array_equal(i1, i2) and np.array_equal(c1, c2)
    assert np.array_equal(iv.ivf_export(32)[1], jv.ivf_export(32)[1])
