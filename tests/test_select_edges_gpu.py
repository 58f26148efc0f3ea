"""The flat and filter-each select sites (block_select.h) at the key counts their other tests leave out: exactly as many keys
as wanted in select_rescore_kernel and collect_rescore_kernel, and more than 256 keys of one score in each_select_kernel.
GPU only."""
import numpy as np
import pytest

from oracle import retrieval as R
from tests.gpu_util import assert_topk_matches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _index(ctx, x):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, x.shape[1])
    idx.add(x)
    return idx


@pytest.mark.parametrize("n", [32, 64])
def test_flat_search_with_exactly_as_many_rows_as_kept(ctx, n):
    """k <= 32 keeps kp = 64 candidates (search.hip: auto_kp): with 64 rows select_rescore_kernel's select is asked for the 64th
    of exactly 64 keys, with 32 rows for more than there are (threshold 0).  k = n fills every place and pads none (k = 64 keeps
    128, again more than there are).  That all 64 rows reach the select as keys is assumed here, not asserted;
    test_forced_collect_with_about_k_rows[10] has n = k = kp and asserts its route."""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 256)).astype(np.float32)
    q = rng.standard_normal((6, 256)).astype(np.float32)
    idx = _index(ctx, x)
    xn, qn = R.normalize_rows(x), R.normalize_rows(q)
    for k in (10, n):
        cos, ids = idx.search(q, k)
        ref_cos, ref_ids = R.knn_search(x, q, k)
        assert_topk_matches(cos, ids, ref_cos, ref_ids, xn, qn)
        assert np.all(ids >= 0)


@pytest.mark.parametrize("n", [9, 10, 11])
def test_forced_collect_with_about_k_rows(ctx, n):
    """rescore_k = k = 10 leaves the first pass no margin (test_search_gpu.py::test_forced_collect_pass_is_exact).  With 10 or 11
    rows the union holds at least kp = 10 keys, every query fails its certificate and collect_rescore_kernel answers from the 10
    or 11 collected rows: exactly k keys (everything is kept) and one more (the select runs).  With 9 rows nothing was cut
    (threshold 0, no bound rose), the first pass is certified and pads one place; collect_rescore_kernel does not run."""
    k, b = 10, 7
    rng = np.random.default_rng(70 + n)
    x = rng.standard_normal((n, 256)).astype(np.float32)
    q = rng.standard_normal((b, 256)).astype(np.float32)
    idx = _index(ctx, x)
    idx.set_option("rescore_k", k)
    ctx.stats_reset()
    cos, ids = idx.search(q, k)
    unc = ctx.stats()["uncertified"]
    print(f"n = {n}: uncertified = {unc} of {b}")
    assert unc == (b if n >= k else 0)
    ref_cos, ref_ids = R.knn_search(x, q, k)
    assert_topk_matches(cos, ids, ref_cos, ref_ids, R.normalize_rows(x), R.normalize_rows(q))
    assert np.array_equal((ids >= 0).sum(1), np.full(b, min(n, k)))


@pytest.mark.parametrize("k", [10, 256])
def test_filter_each_list_of_identical_rows(ctx, k):
    """400 bit-identical rows in one allow-list: each_select_kernel's select meets more than 256 keys of one score and must descend
    into the row bytes; the k lowest ids win, as in the single-list search."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3000, 64)).astype(np.float32)
    copies = np.sort(rng.permutation(3000)[:400])
    x[copies] = x[copies[0]]
    idx = _index(ctx, x)
    others = np.setdiff1d(np.arange(3000), copies)
    lists = [rng.permutation(np.concatenate([copies, others[:300]])).astype(np.int64),      # 700 ids, 400 of them tied
             copies[::-1].astype(np.int64)]                                                # the 400 tied ones alone
    q = np.stack([x[copies[0]], x[copies[0]] * 2.0]).astype(np.float32)
    cos, ids = idx.search_filtered_each(q, k, lists)
    assert np.array_equal(ids, np.tile(copies[:k], (2, 1)))
    assert np.all(cos == cos[0, 0]) and abs(cos[0, 0] - 1.0) < 1e-5
    for b in range(2):
        c1, i1 = idx.search(q[b:b + 1], k, filter_ids=lists[b])
        assert np.array_equal(i1[0], ids[b]) and np.array_equal(c1[0], cos[b])
