"""The sweep walk (csrc/sweep.hip) that exclusion, collapsed and radial search share, driven through every branch on one index.

Row order of the index (dim 64): 300 copies of a unit vector v | 16 000 random unit rows | 8 200 more copies of v.  The query is
v.  A walk whose running list is full (threshold just under 1) meets nothing in the random stretch, so its range doubles past
8192 rows; the range that reaches the second block of copies then holds more than EXACT_CAP = 4096 rows of equal cosine, so it
must be halved and collected again.  Every copy has the same cosine bits and ties go to the lowest id, so the answers are known
in closed form -- provided no random row comes within the scan's error bound of cosine 1, which
``test_random_rows_stay_clear_of_the_query`` checks in float64 without a GPU.

That the halving branch ran cannot be seen from Python; profiles/sweep/NOTES.md shows it from the kernel trace of this file (more
collect scans than merges)."""
import numpy as np
import pytest

from tests.test_collapse_gpu import NONE

D = 64
HEAD, RANDOM, TAIL = 300, 16000, 8200
N = HEAD + RANDOM + TAIL
K = 10
KEY = 7
BASE = 1_000_000
DELETED = 5000                 # a random row: the index then has an id map
# kernels.h scan_eps at K = 64: (1 + dq) dx + dq + max(2e-4, K 2^-23), with dq, dx <= 2^-9 (bf16 rounding of a unit vector)
EPS_MAX = 0.005
CASES = ("default", "one_slot", "id_base", "id_map")


def make_rows():
    rng = np.random.default_rng(7)
    v = rng.standard_normal(D)
    v /= np.linalg.norm(v)
    r = rng.standard_normal((RANDOM, D))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    x = np.concatenate([np.tile(v, (HEAD, 1)), r, np.tile(v, (TAIL, 1))]).astype(np.float32)
    return x, v.astype(np.float32)


def test_random_rows_stay_clear_of_the_query():
    x, v = make_rows()
    r = x[HEAD:HEAD + RANDOM].astype(np.float64)
    cos = (r @ v.astype(np.float64)) / np.linalg.norm(r, axis=1) / np.linalg.norm(v.astype(np.float64))
    print(f"[sweep walk] largest cosine of a random row with the query: {cos.max():.4f}")
    assert cos.max() < 1.0 - 4 * EPS_MAX


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _build(ctx):
    from semantic_query_engine_amd import VectorIndex
    x, v = make_rows()
    idx = VectorIndex(ctx, D)
    idx.add(x)
    idx.set_keys(np.arange(HEAD), np.full(HEAD, KEY))
    return idx, v


@pytest.fixture(scope="module")
def plain(ctx):
    return _build(ctx)


@pytest.fixture(scope="module")
def mapped(ctx):
    idx, v = _build(ctx)
    idx.delete([DELETED])
    idx.set_option("id_base", BASE)
    return idx, v


@pytest.fixture(params=CASES)
def case(request, plain, mapped):
    """(index, query, id_base) of the case; the options of the shared index are put back afterwards"""
    name = request.param
    if name == "id_map":
        yield mapped[0], mapped[1], BASE
        return
    idx, v = plain
    if name == "one_slot":
        idx.set_option("range_key_budget", 4096)
    if name == "id_base":
        idx.set_option("id_base", BASE)
    yield idx, v, BASE if name == "id_base" else 0
    idx.set_option("range_key_budget", 1 << 25)
    idx.set_option("id_base", 0)


def _copy_cos(idx, v, base):
    """the cosine bits index.search returns for a copy of v (id 10)"""
    cos, ids = idx.search(v[None], 11)
    assert ids[0, 10] == 10 + base
    return cos[0, 10]


@pytest.mark.gpu
def test_exclusion(ctx, case):
    idx, v, base = case
    idx.set_option("exclude_depth", K)                       # stage A fetches ids 0..9, all denied: the query is swept
    try:
        cos, ids = idx.search_excluding(v[None], K, [np.arange(K)])
    finally:
        idx.set_option("exclude_depth", 0)
    assert ctx.exclude_swept() == 1
    assert np.array_equal(ids[0], np.arange(K, 2 * K) + base)
    assert np.array_equal(cos[0].view(np.uint32), np.full(K, _copy_cos(idx, v, base)).view(np.uint32))


@pytest.mark.gpu
def test_collapsed(ctx, case):
    idx, v, base = case
    cos, ids, keys = idx.search_collapsed(v[None], K)        # the 64 rows of stage A are one group
    assert ctx.stats()["collapse_swept"] == 1
    first_keyless = HEAD + RANDOM                            # ids are stable: the delete does not move them
    assert np.array_equal(ids[0], np.concatenate([[0], np.arange(first_keyless, first_keyless + K - 1)]) + base)
    assert np.array_equal(keys[0], np.concatenate([[KEY], np.full(K - 1, NONE)]))
    assert np.array_equal(cos[0].view(np.uint32), np.full(K, _copy_cos(idx, v, base)).view(np.uint32))


@pytest.mark.gpu
def test_range(ctx, case):
    idx, v, base = case
    counts, cos, ids = idx.range_search(v[None], 1.0 - EPS_MAX, K)
    assert counts[0] == HEAD + TAIL
    assert np.array_equal(ids[0], np.arange(K) + base)
    assert np.array_equal(cos[0].view(np.uint32), np.full(K, _copy_cos(idx, v, base)).view(np.uint32))
