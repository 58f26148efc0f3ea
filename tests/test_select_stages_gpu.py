"""The stages BEHIND the bf16 scan, on what a real search left: select_rescore_kernel (csrc/select.hip) and the tail
(csrc/exact.hip: compact_uncertified_kernel, collect_rescore_kernel) against oracle/select.py, which restates from the read-back
lists and bound table which rows are selected, their fp32 cosines bit for bit, the final order, the certificate's decision, the
collect threshold, and what the tail makes of the collected keys.  tests/test_scan_stages_gpu.py checks what comes BEFORE (the
lists, the table, the rows the collect pass gathers); the end-to-end tests cannot see a certificate that reads the wrong column
or drops eps, because on most data the answer still comes out right.  tests/test_select_stages_cpu.py shows on a NumPy emulation
that each stage of the checker can fail.

Every case asserts, before it compares, the plan (from the device's CU count), the launch form (n_chunks * kp > 4096: 1024 threads
and 16,384 LDS keys, else 256 and 4,096) and the key route (n_keys > 16,384 in the large form: the select walks the global lists)
from scan_last() and the counts it read.  Notes on what the cases can and cannot reach:
  * gfin > score(T) needs the scan's k-row bound to have emptied the lists (oracle/select.py, "A remark on gfin"): on the Gaussian
    cases at dim 128 every certificate is decided by score(T) or ties with it; test_certificate_under_the_k_row_bound (dim 1024,
    k = 1 and 10) is the case where gfin is the deciding term.  The report counts by_T / tie / by_gfin for every case.
  * m < k happens only on an index of fewer than k rows, where the union holds fewer than kp keys (T = 0) and the bound table is
    off (fewer than 64 chunks): unseen = -inf, so the kernel certifies the query -- nothing was cut, every row is in the answer --
    and the restated certificate (certified iff unseen == -inf or ...) agrees.  thr = -1 - eps needs m < k UNDER a bound; the
    CPU test reaches it with lists emptied by hand.
Measured figures: profiles/select_stages/NOTES.md."""
import numpy as np
import pytest

from oracle import scan as SC
from oracle import select as SL
from tests import scan_stage_cases as SCC
from tests import select_stage_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def cu(ctx):
    return ctx.device_info()["cu_count"]


# ------------------------------------------------------------------------------ forms and key routes
def test_small_form_at_its_upper_edge(ctx, cu):
    """n_chunks * kp == 4096 twice: 64 chunks x kp 64 (with id_base set) and 16 chunks x kp 256"""
    base = 1_000_000_007
    idx = C.make_index(ctx, C.gauss_rows(64 * 256, 128), id_base=base)
    rep, L, (cos, ids) = C.search_and_check(ctx, idx, C.gauss_queries(64, 128, 64 * 256), 10, 64, "form small 64x64 id_base", id_base=base)
    assert L["n_chunks"] * L["kp"] == 4096 and rep["form"] == "small" and ids.min() >= base
    idx.close()
    idx = C.make_index(ctx, C.gauss_rows(16 * 256, 128))
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(64, 128, 16 * 256), 100, 256, "form small 16x256")
    assert (L["n_chunks"], L["kp"], rep["form"], rep["n_keys_max"]) == (16, 256, "small", 4096)
    idx.close()


def test_large_form_just_past_the_edge(ctx, cu):
    n = 64 * 256 + 1
    idx = C.make_index(ctx, C.gauss_rows(n, 128))
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(64, 128, n), 10, 64, "form large 65x64")
    assert (L["n_chunks"], rep["form"], rep["route_lds"]) == (min(65, cu), "large", 64)
    idx.close()


@pytest.mark.parametrize("n,route", [(70_001, "global"), (10_000, "lds")])
def test_key_routes_of_the_large_form(ctx, cu, n, route):
    """kp = 256, k = 100: both bounds are off and every list fills, so 70,001 rows leave ~65,000 keys per query (the select walks
    the global lists) and 10,000 rows leave 10,000 (the LDS copy)."""
    B = 48
    idx = C.make_index(ctx, C.gauss_rows(n, 128))
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(B, 128, n), 100, 256, f"route {route} n={n}")
    assert rep["form"] == "large" and L["gshift"] < 0 and L["gshift_k"] < 0
    if route == "global":
        assert rep["route_global"] == B and rep["n_keys_min"] > SL.LARGE_KEYS
    else:
        assert rep["route_lds"] == B and rep["n_keys_max"] == n
    idx.close()


# ------------------------------------------------------------------------------ batch sizes
N_BATCH = 25_001            # 98 tiles: 85 chunks at three query blocks of a 256-CU part, 64 at four


@pytest.fixture(scope="module")
def index_batch(ctx):
    idx = C.make_index(ctx, C.gauss_rows(N_BATCH, 128))
    yield idx
    idx.close()


@pytest.mark.parametrize("B", [1, 64, 65, 300, 600, 1024])
def test_batch_sizes(ctx, cu, index_batch, B):
    rep, L, _ = C.search_and_check(ctx, index_batch, C.gauss_queries(B, 128, N_BATCH), 10, 0, f"batch B={B}")
    assert L["qblocks"] == {1: 1, 64: 1, 65: 1, 300: 2, 600: 3, 1024: 4}[B]
    if cu == 256:
        assert (L["n_chunks"], rep["form"]) == {1: (98, "large"), 64: (98, "large"), 65: (98, "large"), 300: (98, "large"),
                                                 600: (85, "large"), 1024: (64, "small")}[B]
    if B >= 600:                                                   # three and four query blocks: plans the scan tests never launch
        out = SC.check_first_pass(SCC.read_launch(index_batch, L))
        SCC.report(f"select-stages B={B}", L, out)


# ------------------------------------------------------------------------------ re-score
@pytest.mark.parametrize("dim", [64, 192, 256, 320, 1024])
def test_rescore_dims(ctx, dim):
    """48 idle lanes, three quarters of a trip, exactly one trip, a partial second trip, four trips; m = 50 selected rows: no
    multiple of 4 (the four-rows-per-step clamp) or of 64"""
    n = 3000 + dim % 7
    idx = C.make_index(ctx, C.gauss_rows(n, dim))
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(9, dim, n), 10, 50, f"rescore dim={dim}")
    assert L["kp"] == 50 and rep["m_lt_kp"] == 0 and rep["visible"] + rep["uncertified"] == 9
    idx.close()


@pytest.mark.parametrize("n", [1, 3, 37, 9])
def test_tiny_indexes(ctx, n):
    """m < kp (and m < k below ten rows): (-inf, -1) from place m on.  See the module docstring for why these queries are
    certified rather than sent to the collect pass."""
    idx = C.make_index(ctx, C.gauss_rows(n, 64))
    rep, L, (cos, ids) = C.search_and_check(ctx, idx, C.gauss_queries(5, 64, n), 10, 0, f"tiny n={n}")
    assert rep["m_lt_kp"] == 5 and rep["m_lt_k"] == (5 if n < 10 else 0)
    assert (ids[:, :min(n, 10)] >= 0).all() and (ids[:, n:] == -1).all() and np.isneginf(cos[:, n:]).all()
    assert rep["no_unseen"] == 5 and rep["certified"] == 5
    idx.close()


# ------------------------------------------------------------------------------ certificate
@pytest.fixture(scope="module")
def index_long(ctx):
    idx = C.make_index(ctx, SCC.rows_b("gauss", 200_001)[0])
    yield idx
    idx.close()


@pytest.mark.parametrize("B,k", [(64, 10), (100, 10), (100, 1)])
def test_certificate_on_the_long_index(ctx, index_long, B, k):
    """the scan tests' long index, where the table decides most drops of the scan: score(T) and gfin are both in force"""
    rep, L, _ = C.search_and_check(ctx, index_long, SCC.queries_b("gauss", B, 200_001), k, 0, f"long B={B} k={k}")
    assert L["gshift"] == 0 and rep["by_T"] + rep["tie"] + rep["by_gfin"] == B


@pytest.mark.parametrize("k", [1, 10])
def test_certificate_under_the_k_row_bound(ctx, cu, k):
    """dim 1024: a tile takes 16 K steps, so the k-row bound (k <= 16: the k-th largest of the 16 quad maxima, minus its slack)
    is applied inside a chunk's first filtered tile and the lists stay short."""
    n, B = 40_001, 64
    idx = C.make_index(ctx, C.gauss_rows(n, 1024))
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(B, 1024, n), k, 0, f"k-row bound dim=1024 k={k}")
    assert L["gshift"] == 0 and L["gshift_k"] == 2 and L["k_rows"] == k
    assert rep["by_gfin"] > 0 and rep["m_lt_kp"] > 0, "the case meant for certificates that gfin decides"
    idx.close()


@pytest.mark.parametrize("rescore_k,gshift", [(0, 0), (32, 1), (16, 2), (128, -1)])
def test_gshift_plans(ctx, cu, rescore_k, gshift):
    n = 64 * 256 + 1
    idx = C.make_index(ctx, C.gauss_rows(n, 128))
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(100, 128, n), 10, rescore_k, f"gshift={gshift}")
    if cu >= 65:
        assert L["gshift"] == gshift
    idx.close()


# ------------------------------------------------------------------------------ ties, the cap, partial failures
@pytest.mark.parametrize("n_same", [300, 5000])
def test_identical_rows(ctx, n_same):
    """Queries 0 and 3 sit on n_same bit-identical rows spread over all chunks: the lowest 64 are selected, the k-th cosine equals
    score(T) up to eps, so the certificate fails.  300 rows: the tail answers with the lowest ids.  5,000 rows are more than
    exact_cap: the first-pass answer stands and is the restated select answer."""
    x, q, same = C.tie_rows(n_same)
    idx = C.make_index(ctx, x)
    rep, L, (cos, ids) = C.search_and_check(ctx, idx, q, 10, 0, f"ties n_same={n_same}")
    d = SL.read_launch(idx, L)
    for b in (0, 3):
        ref = SL.select_reference(d, b)
        assert np.array_equal(ref["rows"], same[:64]) and not np.isposinf(d["thr"][b])
        assert np.array_equal(ids[b], same[:10])
    assert rep["over_cap"] == (2 if n_same > L["exact_cap"] else 0) and rep["uncertified"] >= 2
    idx.close()


def test_partial_failures(ctx):
    x, q, hard = C.partial_failures()
    idx = C.make_index(ctx, x)
    rep, L, _ = C.search_and_check(ctx, idx, q, 10, 0, "partial failures 5 of 64")
    from semantic_query_engine_amd import engine as E
    unc = idx.scan_read(E.SCAN_UNC_IDS, np.int32, L["uncertified"])
    assert set(hard.tolist()) <= set(unc.tolist()) and 5 <= rep["uncertified"] <= 8 and (np.diff(unc) > 0).all()
    counts = idx.scan_read(E.SCAN_COLLECT_COUNTS, np.int32, 64)
    assert (counts[:unc.size] > 0).all() and not counts[unc.size:].any()
    idx.close()


@pytest.mark.parametrize("dim", [64, 1024])
def test_decoys_above_the_true_neighbours(ctx, dim):
    """test_bound_gpu.py's layout (kp = 64, 157 and more chunks): for the three adversarial queries the scan ranks 600 decoys above
    the ten true neighbours by nearly the whole error bound, the selected rows are decoys, and only a certificate with the right
    unseen term and the full eps fails as it must; the threshold (k-th cosine of the DECOYS) - eps is what lets the tail find the
    true neighbours."""
    from tests import rounding_cases as RC
    case = RC.bf16_adversarial(dim)
    B = 64
    which = np.arange(B) % case["q"].shape[0]
    idx = C.make_index(ctx, case["x"])
    rep, L, (cos, ids) = C.search_and_check(ctx, idx, case["q"][which], RC.K_ADV, 0, f"decoys dim={dim}")
    hard = np.nonzero(which < case["n_adv"])[0]
    from semantic_query_engine_amd import engine as E
    unc = idx.scan_read(E.SCAN_UNC_IDS, np.int32, L["uncertified"])
    assert np.isin(hard, unc).all() and rep["thr_checked"] >= hard.size and rep["over_cap"] == 0
    d = SL.read_launch(idx, L)
    for b in hard.tolist():
        assert np.isin(SL.select_reference(d, b)["rows"], case["decoy_ids"][which[b]]).all(), "the selected rows are decoys"
        assert ids[b].tolist() == case["true_ids"][which[b]].tolist()
    idx.close()


@pytest.mark.parametrize("n,dim,B", [(20_001, 128, 200), (3_000, 1024, 65)])
def test_every_query_fails(ctx, n, dim, B):
    """rescore_k = k = 10 leaves the certificate no margin (test_scan_stages_gpu.py: test_collect_pass): every collect threshold
    and every answer of the tail is compared"""
    idx = C.make_index(ctx, C.gauss_rows(n, dim))
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(B, dim, n), 10, 10, f"every query fails n={n} dim={dim}")
    assert rep["uncertified"] == B and rep["thr_checked"] == B and rep["over_cap"] == 0 and rep["tail_keys"] >= 10 * B
    idx.close()


# ------------------------------------------------------------------------------ without the certificate
def test_without_the_certificate(ctx):
    """certify = 0 with rescore_k = 64 (kp unchanged): select's output is the final answer of every query"""
    n = 64 * 256 + 1
    idx = C.make_index(ctx, C.gauss_rows(n, 128), certify=0)
    rep, L, _ = C.search_and_check(ctx, idx, C.gauss_queries(100, 128, n), 10, 64, "certify=0", certify=False)
    assert L["kp"] == 64 and rep["visible"] == 100
    idx.close()


# ------------------------------------------------------------------------------ more than one pass
@pytest.mark.parametrize("B", [1025, 2049])
def test_more_than_one_pass(ctx, B):
    """Passes of 1,024 queries: the answer is that of the same queries searched in slices, bit for bit, and both are the exact
    top-k by the fp32 chain; scan_last() describes the last pass (one query); with rescore_k = k every query fails its
    certificate and the uncertified counts of the passes add up."""
    n, dim, k = 2000, 64, 10
    x = C.gauss_rows(n, dim)
    q = C.gauss_queries(B, dim, n)
    idx = C.make_index(ctx, x, rescore_k=k)
    ctx.stats_reset()
    cos, ids = idx.search(q, k)
    assert ctx.stats()["uncertified"] == B
    L = idx.scan_last()
    C.assert_plan(ctx, L, n, 1, k, k)
    assert L["B"] == 1 and L["uncertified"] == 1
    rep = SL.check_launch(idx, (cos[-1:], ids[-1:]), 0, L)
    assert rep["uncertified"] == 1
    master = idx.get_rows(idx.ids())
    for s0 in range(0, B, 1024):
        c2, i2 = idx.search(q[s0:s0 + 1024], k)
        assert np.array_equal(c2.view(np.uint32), cos[s0:s0 + 1024].view(np.uint32)) and np.array_equal(i2, ids[s0:s0 + 1024])
        from semantic_query_engine_amd import engine as E
        m = min(1024, B - s0)
        qn = idx.state_read(E.STATE_QN, np.float32, m * dim).reshape(m, dim)
        for b in range(m):
            sc = SL.chain_scores(master, None, qn[b])
            o = SL.rank_rows(sc, np.arange(n))[:k]
            assert np.array_equal(i2[b], o) and np.array_equal(c2[b].view(np.uint32), sc[o].view(np.uint32)), (s0, b)
    idx.close()
