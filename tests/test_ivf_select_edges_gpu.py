"""The IVF select kernels at small sizes, one case per path of ivf_select.hip, against oracle.ivf_search on the exported structure.

Every case asserts on the exported assignment the precondition that routes it to the path it is meant to reach (the gates
are in ivf_select.hip and ivf.hip: COLLECT_CAP = 1024 probed rows for ivf_select_kernel's sample fast path, nlist % 128 == 0 for the dense
probe select, IVF_LIST_CAP / 4 = 2048 probed rows for ivf_threshold_kernel's select, more than 512 (query, probe) pairs at
dim 256 with lists longer than one 256-row tile for the collect mode).  GPU only."""
import numpy as np
import pytest

from oracle import retrieval as R
from tests.gpu_util import assert_topk_matches

pytestmark = pytest.mark.gpu

# ivf_state(): include/sqe.h SQE_IVF_COARSE_*, SQE_IVF_KERNEL_*, SQE_IVF_GRID_*
BF16_LISTS = {"coarse": 1, "list_kernel": 1, "grid": 0}               # flat coarse index, bf16 MFMA list scan, one workgroup per list
BF16_LISTS_DENSE = {"coarse": 0, "list_kernel": 1, "grid": 0}         # dense coarse GEMM + ivf_probe_select_kernel
COLLECT = {"coarse": 1, "list_kernel": 3, "grid": 5, "fallback": 0}   # streaming int8 list scan in collect mode, answered by the lists

COLLECT_CAP = 1024       # ivf_select_kernel: more probed rows take the sample fast path
LIST_ALL = 2048          # ivf_threshold_kernel: up to IVF_LIST_CAP / 4 probed rows are listed whole
TILE = 256               # rows of a list-scan tile; the first tile of a list is the collect mode's sample


def _kp(k):
    return min(256, max(32, 4 * k))      # ivf.hip: ivf_search


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _data(n, d, b, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = (x[rng.integers(0, n, b)] + 0.3 * rng.standard_normal((b, d))).astype(np.float32)
    return x, q


def _index(ctx, x, nlist, seed):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    idx = VectorIndex(ctx, x.shape[1], INDEX_IVF_FLAT, nlist)
    idx.train(x, iters=6, seed=seed)
    idx.add(x)
    return idx


def _probed_rows(qn, centroids, assign, nprobe):
    """rows in the lists the oracle probes, per query"""
    cs = qn.astype(np.float64) @ centroids.astype(np.float64).T
    probes = np.argsort(-cs, axis=1, kind="stable")[:, :nprobe]
    return np.bincount(assign, minlength=centroids.shape[0])[probes].sum(1), probes


def _check(idx, x, q, nlist, k, nprobe, route):
    """route: fields of ivf_state() (what the host launched for this search) the case's preconditions promise"""
    centroids, assign = idx.ivf_export(nlist)
    xn, qn = R.normalize_rows(x), R.normalize_rows(q)
    cos, ids = idx.search(q, k, nprobe=nprobe)
    st = idx.ivf_state()
    assert {key: st[key] for key in route} == route, st
    ref_cos, ref_ids = R.ivf_search(xn, qn, centroids, assign, k, nprobe)
    assert_topk_matches(cos, ids, ref_cos, ref_ids, xn, qn)
    for row in ids:                                         # ids in a row are distinct
        live = row[row >= 0]
        assert np.unique(live).size == live.size
    return cos, ids


# ---------------------------------------------------------------- 1. ivf_select_kernel, general path
@pytest.fixture(scope="module")
def small(ctx):
    x, q = _data(500, 64, 24, seed=101)
    idx = _index(ctx, x, 8, seed=102)
    centroids, assign = idx.ivf_export(8)
    probed, _ = _probed_rows(R.normalize_rows(q), centroids, assign, 2)
    return idx, x, q, probed


@pytest.mark.parametrize("k", [10, 60, 256])
def test_general_path_select_all_and_padding(small, k):
    """At most 1,024 probed rows: the eight-pass select over the strips answers.  k = 10: kp = 40 keys of more probed rows (the
    select runs); k = 60: kp = 240 is at least the probed rows (everything is kept, no place is padded); k = 256: more places
    than probed rows (the tail is (-inf, -1))."""
    idx, x, q, probed = small
    assert probed.max() <= COLLECT_CAP
    if k == 10:
        sel = probed > _kp(k)
    elif k == 60:
        sel = (probed <= _kp(k)) & (probed >= k)
    else:
        sel = probed < k
    assert sel.sum() >= 4, (k, probed)
    cos, ids = _check(idx, x, q[sel], 8, k, 2, BF16_LISTS)
    assert np.array_equal((ids >= 0).sum(1), np.minimum(probed[sel], k))


# ---------------------------------------------------------------- 2. / 3. ivf_select_kernel, sample fast path and its misjudgement
def test_sample_fast_path(ctx):
    """More than 1,024 probed rows: the threshold from the sample (a four-pass select over 32-bit scores) leaves kp .. 1,024 keys,
    which are ranked at once."""
    x, q = _data(6000, 64, 16, seed=111)
    idx = _index(ctx, x, 8, seed=112)
    centroids, assign = idx.ivf_export(8)
    probed, _ = _probed_rows(R.normalize_rows(q), centroids, assign, 4)
    assert probed.min() > COLLECT_CAP, probed
    _check(idx, x, q, 8, 10, 4, BF16_LISTS)


def test_sample_fast_path_misjudged_by_ties(ctx):
    """2,000 bit-identical copies of one vector in one list: the sample's threshold is the copies' score, more than 1,024 keys
    reach it, and the general path answers over more than 256 tied scores (its select descends into the row bytes).  Any
    copy is a right answer; ids in a row stay distinct."""
    x, q = _data(6000, 64, 16, seed=111)
    rng = np.random.default_rng(113)
    idx = _index(ctx, x, 8, seed=112)
    v = rng.standard_normal(64).astype(np.float32)
    rows = rng.permutation(6000)[:2000]
    x[rows] = v
    idx.update(rows, x[rows])
    q[:4] = v + 0.01 * rng.standard_normal((4, 64)).astype(np.float32)
    centroids, assign = idx.ivf_export(8)
    home = np.unique(assign[rows])
    assert home.size == 1 and np.bincount(assign, minlength=8)[home[0]] > COLLECT_CAP
    probed, probes = _probed_rows(R.normalize_rows(q), centroids, assign, 4)
    assert all(home[0] in p for p in probes[:4])                      # the aimed queries probe the copies' list
    assert probed.min() > COLLECT_CAP
    cos, ids = _check(idx, x, q, 8, 10, 4, BF16_LISTS)
    assert np.all(np.isin(ids[:4], rows))


# ---------------------------------------------------------------- 4. ivf_probe_select_kernel
@pytest.fixture(scope="module")
def dense(ctx):
    x, q = _data(3000, 64, 16, seed=121)
    return _index(ctx, x, 128, seed=122), x, q


@pytest.mark.parametrize("nprobe", [1, 8, 100, 120, 128])
def test_dense_probe_select(dense, nprobe):
    """nlist = 128 takes the dense coarse GEMM and ivf_probe_select_kernel: the nprobe + 8 best of 128 lists by the select with
    its early exit (1, 8, 100), every list without a select once nprobe + 8 reaches nlist (120, 128)."""
    idx, x, q = dense
    nlist = 128
    assert nlist % 128 == 0 and nprobe + 8 <= 256            # ivf.hip: ivf_coarse_topk's dense gate
    assert (nprobe + 8 >= nlist) == (nprobe >= 120)
    _, assign = idx.ivf_export(nlist)
    assert np.count_nonzero(np.bincount(assign, minlength=nlist)) > 64      # the lists are in use: probes differ by query
    _check(idx, x, q, nlist, 10, nprobe, BF16_LISTS_DENSE)


# ---------------------------------------------------------------- 5. collect mode: ivf_threshold_kernel, ivf_select_list_kernel
def test_collect_mode_lists_everything(ctx):
    """640 (query, probe) pairs at dim 256 run the collect mode; 2,000 probed rows are at most IVF_LIST_CAP / 4, so the threshold
    is -inf, every row is listed and ivf_select_list_kernel selects kp of 2,000 keys."""
    n, d, nlist, nprobe, b = 2000, 256, 4, 4, 160
    x, q = _data(n, d, b, seed=131)
    idx = _index(ctx, x, nlist, seed=132)
    _, assign = idx.ivf_export(nlist)
    assert b * nprobe > 512 and nprobe <= 32
    assert np.bincount(assign, minlength=nlist).max() > TILE          # some list has a tile beyond the sample tile
    assert n <= LIST_ALL and nprobe == nlist                          # every query probes all n rows
    _check(idx, x, q, nlist, 10, nprobe, COLLECT)


@pytest.fixture(scope="module")
def collect_data():
    return _data(6000, 256, 80, seed=141)


def test_collect_mode_threshold_select(ctx, collect_data):
    """6,000 probed rows: ivf_threshold_kernel's four-pass select over the sample gives the threshold, the collect pass lists a
    few hundred keys, ivf_select_list_kernel selects kp of them."""
    n, nlist, nprobe = 6000, 8, 8
    x, q = collect_data
    idx = _index(ctx, x, nlist, seed=142)
    _, assign = idx.ivf_export(nlist)
    assert q.shape[0] * nprobe > 512 and nprobe <= 32
    assert np.bincount(assign, minlength=nlist).min() > TILE          # every list has tiles beyond the sample tile
    assert n > LIST_ALL and nprobe == nlist
    _check(idx, x, q, nlist, 10, nprobe, COLLECT)


def test_collect_mode_list_of_ties(ctx, collect_data):
    """1,500 bit-identical copies of one vector: the lists of the queries aimed at it hold more than 256 keys of one score (and
    fewer than the 8,192 a list holds), so ivf_select_list_kernel's select stops early only inside the row bytes."""
    n, nlist, nprobe = 6000, 8, 8
    x, q = (a.copy() for a in collect_data)
    rng = np.random.default_rng(143)
    idx = _index(ctx, x, nlist, seed=142)
    v = rng.standard_normal(256).astype(np.float32)
    rows = rng.permutation(n)[:1500]
    x[rows] = v
    idx.update(rows, x[rows])
    q[:4] = v + 0.01 * rng.standard_normal((4, 256)).astype(np.float32)
    _, assign = idx.ivf_export(nlist)
    assert q.shape[0] * nprobe > 512 and nprobe <= 32
    assert np.bincount(assign, minlength=nlist).max() > TILE
    assert np.unique(assign[rows]).size == 1 and 256 < rows.size < 8192 and nprobe == nlist
    cos, ids = _check(idx, x, q, nlist, 10, nprobe, COLLECT)
    assert np.all(np.isin(ids[:4], rows))
