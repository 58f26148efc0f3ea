"""Fused multi-query search (sqe_index_search_fused, fuse.hip): RRF and max-sim over the top-n of a group's sub-queries.  GPU only.

The definition is integer arithmetic, so every comparison here is bit for bit: search_fused(...) against
tests/fuse_reference.py applied to the library's OWN search(q_sub, n) output on the same index -- ids equal, fused and cos
equal as bytes.  No tolerance, no skipped case, and no call is repeated to look for nondeterminism."""
import numpy as np
import pytest

from . import fuse_reference as F

pytestmark = pytest.mark.gpu

D = 64
ROWS = 4096
CENTRES = 300
SEED = 7          # test_max_is_exact_top_k_of_the_raw_data: checked on the CPU with NumPy, see its docstring


def same_bits(a, b):
    return all(u.shape == w.shape and u.dtype == w.dtype and np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
               for u, w in zip(a, b))


def make_data(seed=SEED, dim=D):
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((CENTRES, dim)).astype(np.float32)
    owner = rng.integers(0, CENTRES, ROWS)
    x = centre[owner] + rng.standard_normal((ROWS, dim)).astype(np.float32)
    return x, centre, rng


def group_queries(centre, rng, centres_of_groups, m):
    """m sub-queries per group: the group's centre plus independent noise, so the lists of a group overlap partly."""
    c = np.repeat(np.asarray(centres_of_groups), m)
    return (centre[c] + 0.7 * rng.standard_normal((c.shape[0], centre.shape[1])).astype(np.float32)).astype(np.float32)


def depth_of(k, depth, mode):
    return depth if depth else (k if mode == "max" else min(256, max(32, 4 * k)))


def check(idx, q, offsets, k, mode, weights=None, depth=0, c=60, nprobe=0):
    """search_fused against the reference over the index's own search at the same depth; returns the library's answer."""
    got = idx.search_fused(q, k, offsets=offsets, mode=mode, weights=weights, depth=depth, rank_constant=c, nprobe=nprobe)
    off = np.array([0, q.shape[0]], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    if q.shape[0]:
        cos, ids = idx.search(q, depth_of(k, depth, mode), nprobe=nprobe)
    else:
        cos, ids = np.empty((0, 1), np.float32), np.empty((0, 1), np.int64)
    want = F.fuse_groups(cos, ids, off, k, mode, weights, c)
    assert np.array_equal(got[1], want[1]), (got[1][:2], want[1][:2])
    assert same_bits(got, want)
    return got


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    return make_data()


@pytest.fixture(scope="module")
def index(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, D)
    idx.add(data[0])
    return idx


WEIGHTED = (0.5, 2.0, 1.0, 64.0, 1e-3)


@pytest.mark.parametrize("m,n,k,mode,weights", [(1, 10, 10, "max", None), (3, 32, 10, "rrf", None), (8, 256, 64, "rrf", None),
                                                (32, 64, 64, "rrf", None), (8, 256, 256, "max", None), (5, 7, 7, "rrf", WEIGHTED)])
def test_cases(data, index, m, n, k, mode, weights):
    _, centre, _ = data
    rng = np.random.default_rng(100 + m)
    G = 3
    q = group_queries(centre, rng, [5, 17, 250], m)
    w = None if weights is None else np.tile(np.asarray(weights, np.float32), G)
    got = check(index, q, np.arange(G + 1) * m, k, mode, w, depth=n)
    assert np.all(got[1][:, 0] >= 0)


def test_ragged_groups_in_one_call(data, index):
    _, centre, rng0 = data
    rng = np.random.default_rng(200)
    offsets = np.array([0, 1, 4, 4, 12, 44], np.int64)
    cs = np.repeat([3, 40, 90, 200], [1, 3, 8, 32])
    q = (centre[cs] + 0.7 * rng.standard_normal((44, D)).astype(np.float32)).astype(np.float32)
    w = rng.uniform(0.1, 4.0, 44).astype(np.float32)
    for mode, wt in (("rrf", None), ("rrf", w), ("max", None)):
        got = check(index, q, offsets, 10, mode, wt, depth=40)
        assert np.all(got[1][2] == -1) and np.all(np.isneginf(got[0][2])) and np.all(np.isneginf(got[2][2]))      # the empty group
        assert np.all(got[1][[0, 1, 3, 4]] >= 0)


def test_identical_sub_queries_give_n_distinct_rows(data, index):
    _, centre, _ = data
    q = np.repeat(group_queries(centre, np.random.default_rng(201), [11], 1), 8, axis=0)
    fused, ids, cos = check(index, q, None, 32, "rrf", depth=32)
    assert np.array_equal(ids[0], index.search(q[:1], 32)[1][0])               # eight equal lists: n distinct rows, the list's own order
    # a sub-query repeated in MAX changes nothing
    assert same_bits(index.search_fused(q, 32, mode="max"), index.search_fused(q[:1], 32, mode="max"))


# 32 of the 300 centres whose 64 nearest rows overlap least (a greedy choice over make_data(SEED), made on the CPU in float64:
# 1850 distinct rows among the 2048)
SPREAD = [0, 1, 3, 5, 10, 20, 27, 33, 34, 35, 36, 51, 56, 59, 72, 82, 83, 89, 93, 110, 116, 135, 159, 183, 188, 227, 264, 279, 280, 284,
          287, 290]


def test_full_table(ctx, data, index):
    """32 sub-queries aimed at 32 different centres at depth 64: the distinct rows are near 2048, the table's limit (the 4096
    rows hold no 32 disjoint neighbourhoods of 64); then an index of 32 tight clusters of 64 rows, where they are exactly 2048."""
    from semantic_query_engine_amd import VectorIndex
    _, centre, _ = data
    q = np.ascontiguousarray(centre[SPREAD])
    distinct = np.unique(index.search(q, 64)[1]).size
    print(f"[fuse] full table: {distinct} distinct rows of 2048 entries")
    assert distinct >= 1800
    for mode, k in (("rrf", 64), ("max", 64), ("rrf", 1)):
        check(index, q, None, k, mode, depth=64)
    rng = np.random.default_rng(202)
    x2 = (np.repeat(centre[:32], 64, axis=0) + 0.1 * rng.standard_normal((2048, D)).astype(np.float32)).astype(np.float32)
    idx = VectorIndex(ctx, D)
    idx.add(x2[rng.permutation(2048)])
    q2 = np.ascontiguousarray(centre[:32])
    assert np.unique(idx.search(q2, 64)[1]).size == 2048
    for mode in ("rrf", "max"):
        got = check(idx, q2, None, 64, mode, depth=64)
        assert np.all(got[1] >= 0)
    idx.close()


def test_k_above_the_live_rows(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, centre, _ = data
    idx = VectorIndex(ctx, D)
    for arr in idx.search_fused(x[:3], 4):                                     # an empty index: all padding
        assert arr.shape == (1, 4) and np.all(arr == (-1 if arr.dtype == np.int64 else -np.inf))
    idx.add(x[:20])
    q = group_queries(centre, np.random.default_rng(203), [1, 2], 3)
    for mode in ("rrf", "max"):
        got = check(idx, q, [0, 3, 6], 32, mode, depth=64)
        assert np.all(got[1][:, :20] >= 0) and np.all(got[1][:, 20:] == -1)
    assert [a.shape for a in idx.search_fused(x[:0], 4, offsets=[0])] == [(0, 4)] * 3      # G = 0
    idx.close()


def test_one_sub_query_max_is_search(data, index):
    _, centre, _ = data
    q = group_queries(centre, np.random.default_rng(204), np.arange(130), 1)
    fused, ids, cos = index.search_fused(q, 10, offsets=np.arange(131), mode="max")
    want = index.search(q, 10)
    assert same_bits((fused, ids, cos), (want[0], want[1], want[0]))


def test_permutation_changes_no_bit(data, index):
    _, centre, _ = data
    rng = np.random.default_rng(205)
    q = group_queries(centre, rng, [77], 8)
    w = rng.uniform(0.1, 8.0, 8).astype(np.float32)
    p = rng.permutation(8)
    assert same_bits(check(index, q, None, 20, "rrf", w, depth=64), index.search_fused(q[p], 20, weights=w[p], depth=64))
    assert same_bits(check(index, q, None, 20, "max", depth=64), index.search_fused(q[p], 20, mode="max", depth=64))


def test_group_alone_and_inside_a_batch(data, index):
    _, centre, _ = data
    rng = np.random.default_rng(206)
    q = group_queries(centre, rng, rng.integers(0, CENTRES, 130), 4)
    w = rng.uniform(0.1, 8.0, 520).astype(np.float32)
    off = np.arange(131) * 4
    for mode, wt in (("rrf", w), ("max", None)):
        full = index.search_fused(q, 10, offsets=off, mode=mode, weights=wt, depth=40)
        for g in (0, 64, 129):
            alone = index.search_fused(q[4 * g:4 * g + 4], 10, mode=mode, weights=None if wt is None else wt[4 * g:4 * g + 4], depth=40)
            assert same_bits(alone, [a[g:g + 1] for a in full]), (mode, g)
    check(index, q, off, 10, "rrf", w, depth=40)


def test_device_entry(ctx, data, index):
    import torch
    _, centre, _ = data
    rng = np.random.default_rng(207)
    q = group_queries(centre, rng, rng.integers(0, CENTRES, 9), 5)
    off = np.arange(10) * 5
    w = rng.uniform(0.1, 8.0, 45).astype(np.float32)
    for mode, wt, k, n in (("rrf", w, 10, 0), ("max", None, 64, 64)):
        host = index.search_fused(q, k, offsets=off, mode=mode, weights=wt, depth=n)
        qd = torch.from_numpy(q).cuda()
        fd = torch.empty((9, k), dtype=torch.float32, device="cuda")
        idd = torch.empty((9, k), dtype=torch.int64, device="cuda")
        cd = torch.empty((9, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        index.search_fused_device(qd.data_ptr(), 45, k, fd.data_ptr(), idd.data_ptr(), cd.data_ptr(), offsets=off, mode=mode, weights=wt,
                                  depth=n)
        ctx.synchronize()
        assert same_bits(host, (fd.cpu().numpy(), idd.cpu().numpy(), cd.cpu().numpy()))


def test_large_id_base_and_deletes(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, centre, _ = data
    rng = np.random.default_rng(208)
    q = group_queries(centre, rng, [9, 99, 199], 6)
    off = [0, 6, 12, 18]
    idx = VectorIndex(ctx, D)
    idx.add(x)
    idx.set_option("id_base", 2 ** 40)
    got = check(idx, q, off, 20, "rrf", depth=64)
    assert got[1].min() >= 2 ** 40
    check(idx, q, off, 20, "max", depth=64)
    idx.set_option("id_base", 0)
    gone = np.unique(np.concatenate([np.arange(3, ROWS, 41), got[1][:, 0] - 2 ** 40]))[:100]      # 100 scattered rows, first hits among them
    assert gone.size == 100
    idx.delete(gone)
    for mode in ("rrf", "max"):
        after = check(idx, q, off, 20, mode, depth=64)
        assert not np.isin(after[1], gone).any() and np.isin(after[1], idx.ids()).all()             # live ids, not positions
    idx.close()


def test_ivf(ctx, data):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    x, centre, _ = data
    ivf = VectorIndex(ctx, D, INDEX_IVF_FLAT, 16)
    ivf.add(x)
    ivf.train(x, iters=5, seed=1)
    q = group_queries(centre, np.random.default_rng(209), [4, 44, 144], 4)
    for mode in ("rrf", "max"):
        check(ivf, q, [0, 4, 8, 12], 10, mode, depth=32, nprobe=4)
    ivf.close()


def test_int8_first_pass(ctx):
    """The int8 first pass needs dim >= 256 and more than 128 queries: an index of its own, 4096 x 256, sampled every 4th tile."""
    from semantic_query_engine_amd import VectorIndex
    x, centre, rng = make_data(seed=11, dim=256)
    idx = VectorIndex(ctx, 256)
    idx.add(x)
    for key, val in (("scan_mode", 2), ("i8_min_rows", 0), ("i8_sample_step", 4), ("i8_sample_m", 64)):
        idx.set_option(key, val)
    q = group_queries(centre, rng, rng.integers(0, CENTRES, 40), 5)
    off = np.arange(41) * 5
    got = idx.search_fused(q, 10, offsets=off, depth=16)
    last = idx.i8_last()                                                       # the lists came through the int8 first pass
    assert last["k"] == 16 and last["B"] == 200
    cos, ids = idx.search(q, 16)                                               # the index's own lists, by the same route
    assert same_bits(got, F.fuse_groups(cos, ids, off, 10, "rrf"))
    assert same_bits(idx.search_fused(q, 10, offsets=off, mode="max", depth=16), F.fuse_groups(cos, ids, off, 10, "max"))
    idx.close()


def test_device_group_equals_single_device(data, index):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, centre, _ = data
    rng = np.random.default_rng(210)
    gctx = Context(devices=[0] * 4, exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    g.add(x)
    offsets = np.array([0, 1, 4, 4, 12, 44], np.int64)
    q = group_queries(centre, rng, rng.integers(0, CENTRES, 44), 1)
    w = rng.uniform(0.1, 4.0, 44).astype(np.float32)
    for mode, wt, k, n in (("rrf", w, 10, 40), ("max", None, 64, 64), ("rrf", None, 1, 1)):
        a = g.search_fused(q, k, offsets=offsets, mode=mode, weights=wt, depth=n)
        assert same_bits(a, index.search_fused(q, k, offsets=offsets, mode=mode, weights=wt, depth=n)), (mode, k, n)
    assert same_bits(g.search_fused(q[:0], 3, offsets=[0, 0, 0]), index.search_fused(q[:0], 3, offsets=[0, 0, 0]))      # only empty groups
    g.close()
    gctx.close()


def max_reference_f64(x, q, offsets, k):
    """float64 top-k of max_j cos(q_j, x) per group from the raw data -> ids [G, k] and the gap between the k-th and the
    (k+1)-th value."""
    xn = x.astype(np.float64)
    xn /= np.linalg.norm(xn, axis=1, keepdims=True) + 1e-9
    qn = q.astype(np.float64)
    qn /= np.linalg.norm(qn, axis=1, keepdims=True) + 1e-9
    cos = qn @ xn.T
    G = len(offsets) - 1
    ids = np.empty((G, k), np.int64)
    gap = np.empty(G)
    for g in range(G):
        best = cos[offsets[g]:offsets[g + 1]].max(axis=0)
        order = np.lexsort((np.arange(best.shape[0]), -best))
        ids[g] = order[:k]
        gap[g] = best[order[k - 1]] - best[order[k]]
    return ids, gap


def test_max_is_exact_top_k_of_the_raw_data(data, index):
    """MAX against the raw data: the fused ids are the float64 top-k of max_j cos wherever the k-th and (k+1)-th float64
    values differ by more than the project's 2e-6 tie tolerance.  SEED was chosen so that no group of this case falls inside
    that band: checked on the CPU with NumPy (max_reference_f64 over make_data(SEED) and these queries; the smallest gap of
    the 64 groups is asserted below), so the cap on skipped groups is 0.  Values inside the top-k may lie closer than 2e-6
    to each other, so the ids are compared as sets per group."""
    x, centre, _ = data
    rng = np.random.default_rng(211)
    q = group_queries(centre, rng, rng.integers(0, CENTRES, 64), 4)
    off = np.arange(65) * 4
    want, gap = max_reference_f64(x, q, off, 10)
    print(f"[fuse] MAX exactness: smallest k / k+1 gap {gap.min():.3e}")
    assert gap.min() > 2e-6                                                    # no group is skipped
    _, ids, _ = index.search_fused(q, 10, offsets=off, mode="max")
    assert np.array_equal(np.sort(ids, axis=1), np.sort(want, axis=1))


def test_invalid_arguments_leave_outputs_untouched(data, index):
    from semantic_query_engine_amd import _native
    lib = _native.load()
    x, _, _ = data
    qq = np.ascontiguousarray(x[:40])
    f = np.full((2, 4), 7.0, np.float32)
    i = np.full((2, 4), 7, np.int64)
    c = np.full((2, 4), 7.0, np.float32)
    out = (f.ctypes.data, i.ctypes.data, c.ctypes.data)
    keep = []                                                                  # the host tables outlive the calls that read them

    def arr(v, dtype):
        keep.append(np.asarray(v, dtype))
        return keep[-1].ctypes.data

    off = arr([0, 3, 6], np.int64)
    ok_w = arr([1, 1, 1, 1, 1, 1], np.float32)
    h, qp = index.handle, qq.ctypes.data
    MAX, RRF = 0, 1
    #      idx q   G  offsets                      k    n    mode c      weights                                    nprobe
    bad = [(h, qp, 2, arr([1, 3, 6], np.int64),    4,   0,   RRF, 60,    None, 0, *out),                                    # does not start at 0
           (h, qp, 2, arr([0, 5, 3], np.int64),    4,   0,   RRF, 60,    None, 0, *out),                                    # decreases
           (h, qp, 2, arr([0, 33, 36], np.int64),  4,   8,   RRF, 60,    None, 0, *out),                                    # m_g > 32
           (h, qp, 2, arr([0, 3, 12], np.int64),   4,   256, RRF, 60,    None, 0, *out),                                    # 9 x 256 > 2048
           (h, qp, 2, off,                         0,   0,   RRF, 60,    None, 0, *out),                                    # k < 1
           (h, qp, 2, off,                         257, 0,   RRF, 60,    None, 0, *out),                                    # k > 256
           (h, qp, 2, off,                         4,   3,   RRF, 60,    None, 0, *out),                                    # n < k
           (h, qp, 2, off,                         4,   257, RRF, 60,    None, 0, *out),                                    # n > 256
           (h, qp, 2, off,                         4,   0,   MAX, 60,    ok_w, 0, *out),                                    # weights with MAX
           (h, qp, 2, off,                         4,   0,   RRF, 60,    arr([1, np.nan, 1, 1, 1, 1], np.float32), 0, *out),
           (h, qp, 2, off,                         4,   0,   RRF, 60,    arr([1, 1, 0, 1, 1, 1], np.float32), 0, *out),
           (h, qp, 2, off,                         4,   0,   RRF, 60,    arr([1, 1, 1, 1, 1, 64.5], np.float32), 0, *out),
           (h, qp, 2, off,                         4,   0,   RRF, 60,    arr([1, 1, -1, 1, 1, 1], np.float32), 0, *out),
           (h, qp, 2, off,                         4,   0,   RRF, 0,     None, 0, *out),                                    # c < 1
           (h, qp, 2, off,                         4,   0,   RRF, 10001, None, 0, *out),                                    # c > 10000
           (h, qp, 2, off,                         4,   0,   2,   60,    None, 0, *out),                                    # unknown mode
           (h, qp, 2, off,                         4,   0,   -1,  60,    None, 0, *out),
           (h, qp, -1, off,                        4,   0,   RRF, 60,    None, 0, *out),
           (h, qp, 2, None,                        4,   0,   RRF, 60,    None, 0, *out),
           (h, None, 2, off,                       4,   0,   RRF, 60,    None, 0, *out),
           (h, qp, 2, off,                         4,   0,   RRF, 60,    None, 0, None, out[1], out[2]),
           (h, qp, 2, off,                         4,   0,   RRF, 60,    None, 0, out[0], None, out[2]),
           (h, qp, 2, off,                         4,   0,   RRF, 60,    None, 0, out[0], out[1], None),
           (None, qp, 2, off,                      4,   0,   RRF, 60,    None, 0, *out)]
    for args in bad:
        assert lib.sqe_index_search_fused(*args) == -1, args[2:9]
        assert lib.sqe_index_search_fused_device(*args) == -1, args[2:9]
    assert np.all(f == 7.0) and np.all(i == 7) and np.all(c == 7.0)
    assert lib.sqe_index_search_fused(h, qp, 0, off, 4, 0, RRF, 60, None, 0, *out) == 0                                    # G = 0 writes nothing
    assert np.all(f == 7.0) and np.all(i == 7) and np.all(c == 7.0)
    assert lib.sqe_index_search_fused(h, qp, 2, off, 4, 0, RRF, 60, None, 0, *out) == 0
    assert same_bits((f, i, c), index.search_fused(qq[:6], 4, offsets=[0, 3, 6]))
    with pytest.raises(ValueError):
        index.search_fused(qq[:6], 4, mode="mean")
    with pytest.raises(ValueError):
        index.search_fused(qq[:6], 4, offsets=[0, 3, 7])
