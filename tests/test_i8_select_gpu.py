"""Stage tests of the int8 search: the thresholds (select_i8.hip: i8_sample_select_kernel; quant.hip: i8_thresholds_kernel), the
staged re-score, the certificate and collect_thr (select_i8_kernel), each against the restatement in oracle/i8_select.py.

tests/test_i8_gpu.py sees the final answer, which the bf16 fallback repairs whatever these stages did; here every launch runs with
the test-only option "i8_keep_select", and the checker reads the launch's own buffers -- sample, thresholds, lists and pools, what
select_i8_kernel wrote BEFORE the fallback, its per-query trace -- and says which stage broke.  tests/test_i8_select_cpu.py shows
that the checker fails on each kind of fault.  One pass per launch (B <= 300); every case prints its figures (pytest -s)."""
import json

import numpy as np
import pytest

from oracle import i8_select as S
from tests import i8_select_cases as C

pytestmark = pytest.mark.gpu

MARGIN, KEY_BUDGET = 0.25, 6144                        # the defaults of "i8_anchor_margin" / "i8_key_budget" (include/sqe.h)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def clustered():
    return C.clustered_case()


@pytest.fixture(scope="module")
def wide():
    """150 000 x 512 Gaussian rows, 260 queries (cases D and I)"""
    return C.gaussian_case(150_000, 512, 260, seed=150_260)


def _index(ctx, dim, step, m, keep=1, **options):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    idx = VectorIndex(ctx, dim)
    for key, val in dict(scan_mode=SCAN_INT8_RESCORE, i8_min_rows=0, i8_sample_step=step, i8_sample_m=m, i8_keep_select=keep, **options).items():
        idx.set_option(key, val)
    return idx


def _search_and_check(ctx, idx, q, k, name, margin=MARGIN, key_budget=KEY_BUDGET, id_base=0, final_ids=None, to_position=None):
    """one search through the int8 first pass, then the full checker and the exactness of the final answer -> (report, cos, ids)"""
    ctx.stats_reset()
    cos, ids = idx.search(q, k)
    st = ctx.stats()
    L = idx.i8_last()
    assert L["kernel"] != 0 and L["B"] == q.shape[0] and L["k"] == k, L        # the int8 path answered, in one pass
    rep = S.check_launch(idx, dict(margin=margin, key_budget=key_budget, id_base=id_base, final_ids=final_ids), final=(cos, ids), stats=st, L=L)
    if to_position is None and id_base:
        to_position = lambda i: i - id_base
    rep["worst_cos_err"] = max(rep["worst_cos_err"], S.check_final(rep, (cos, ids), to_position))
    print("i8_select", name, json.dumps(S.summary(rep)))
    return rep, cos, ids


# ------------------------------------------------------------------------------------------------------------------ A: Gaussian
@pytest.mark.parametrize("n,dim,b,k", [(60_000, 256, 300, 10), (50_003, 384, 129, 1), (40_000, 1024, 33, 64), (60_000, 512, 1, 10)])
def test_gaussian(ctx, n, dim, b, k):
    """Half of the queries planted on rows; 64- / 128- / 256-query blocks, k == m, a partial last tile"""
    x, q = C.gaussian_case(n, dim, b, seed=n + b)
    idx = _index(ctx, dim, step=4, m=64)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, k, f"A {n}x{dim} B{b} k{k}")
    assert rep["certified"] > 0 or k == 64             # (k == m: the threshold IS the k-th sample score, no query can certify)
    idx.close()


def test_keep_select_changes_no_answer_and_guards_its_buffers(ctx):
    """Answers with the option on and off are the same bits; without it the snapshot buffers are not readable, the others are"""
    from semantic_query_engine_amd import engine as E
    from semantic_query_engine_amd._native import SqeError
    x, q = C.clustered_case(n=30_000, b=70)                 # (uncertified queries too: the fallback's answers are part of the comparison)
    out = []
    for keep in (0, 1, 0):
        idx = _index(ctx, 256, step=4, m=64, keep=keep, i8_key_budget=1)
        idx.add(x)
        out.append(idx.search(q, 10))
        L = idx.i8_last()
        assert L["kernel"] != 0 and L["uncertified"] > 0
        assert idx.i8_read(E.I8_THR_EFF, np.float32, L["b_pad"]).size and idx.i8_read(E.I8_SAMPLE_COS, np.float32, L["B"] * L["sample_m"]).size
        for what, dt, cnt in ((E.I8_SELECT_COS, np.float32, L["B"] * 10), (E.I8_SELECT_IDS, np.int64, L["B"] * 10),
                              (E.I8_SELECT_THR, np.float32, L["b_pad"]), (E.I8_SELECT_TRACE, np.int32, L["B"] * 4)):
            if keep:
                assert idx.i8_read(what, dt, cnt).size == cnt
            else:
                with pytest.raises(SqeError, match="i8_keep_select"):
                    idx.i8_read(what, dt, cnt)
        if keep:                                              # switched off again on the same index: the old snapshot is not served
            idx.set_option("i8_keep_select", 0)
            idx.search(q, 10)
            with pytest.raises(SqeError, match="i8_keep_select"):
                idx.i8_read(E.I8_SELECT_TRACE, np.int32, 4)
        idx.close()
    for cos, ids in out[1:]:
        assert np.array_equal(cos.view(np.uint32), out[0][0].view(np.uint32)) and np.array_equal(ids, out[0][1])


# ------------------------------------------------------------------------------------------------------------------ B: clustered
@pytest.mark.parametrize("name,options", [("default", {}), ("budget1", {"i8_key_budget": 1}), ("margin0", {"i8_anchor_margin": 0}),
                                          ("margin4", {"i8_anchor_margin": 4})])
def test_clustered_anchor_on_and_off(ctx, clustered, name, options):
    """~2,000 rows inside the int8 error band of the k-th place: the anchored threshold collects the crowd; with key budget 1 the
    anchor is never used"""
    x, q = clustered
    idx = _index(ctx, 256, step=4, m=64, **options)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, 10, f"B clustered {name}", margin=options.get("i8_anchor_margin", MARGIN),
                                  key_budget=options.get("i8_key_budget", KEY_BUDGET))
    if name == "default":
        assert rep["anchored"] > 0
    if name == "budget1":
        assert rep["anchored"] == 0 and rep["uncertified"] > 0
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ C: negative thresholds
def test_queries_opposite_to_the_rows(ctx):
    """Every cosine is below -0.2, so is every threshold: thr_eff must still lie ABOVE thr_int * unit (the formula before this test
    multiplied by (1 + 1e-6), which rounds a negative product down: below the estimate of an uncollected row)"""
    x, q = C.opposite_case()
    idx = _index(ctx, 256, step=4, m=64)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, 10, "C opposite")
    d = rep["data"]
    assert (d["thr_int"][:100] < 0).all() and (d["thr_int"][:100].astype(np.float64) * S.units(d) < -0.1).all()
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ D: thresholds too high / too low
@pytest.mark.parametrize("step,m,k,margin", [(64, 1, 1, MARGIN), (4, 1, 1, 0.0), (1, 64, 10, MARGIN)])
def test_threshold_too_high_and_too_low(ctx, wide, step, m, k, margin):
    """(64, 1, 1) does not stay what it says: an index of 586 tiles samples at least 128 of them (search.hip: sample_plan), so the launch
    runs with step 4 and the 16th sample score -- asserted, so that a change of that plan shows here -- and every query certifies
    (44 of 260 anchored).  The threshold that IS too high is (4, 1, 1) with margin 0: the best sample score, anchored at c0 - eps8
    exactly; where the sample holds the best row of the index, thr_eff + eps8 lands on or above its cosine and the proof must fail."""
    x, q = wide
    idx = _index(ctx, 512, step=step, m=m, i8_anchor_margin=margin)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, k, f"D step{step} m{m} k{k} margin{margin}", margin=margin)
    L = rep["data"]["L"]
    assert (L["sample_step"], L["sample_m"]) == {64: (4, 16), 4: (4, 1), 1: (1, 64)}[step]
    if step == 4:
        assert rep["from_sample"] + rep["uncertified"] > 0
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ E: crowds
def test_crowd_overflows_the_estimate_buffer(ctx):
    """4,500 rows within 3e-3 of one centre, shuffled through the index: more rows qualify for a bf16 estimate than select_i8 holds"""
    x, q, pos = C.crowd_case()
    idx = _index(ctx, 512, step=4, m=64, i8_key_budget=0)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, 10, "E crowd shuffled", key_budget=0)
    tr = rep["data"]["trace"]
    assert (tr[:, 0] >= 4500).all() and (tr[:, 1] == S.RS_CAP).all() and (tr[:, 3] & S.F_OVERFLOW).all() and rep["uncertified"] == 8
    idx.close()


@pytest.mark.parametrize("crowd,past_cap", [(4500, False), (16000, True)])
def test_crowd_appended_in_one_call_uses_the_pool(ctx, crowd, past_cap):
    """The same crowd as one block of rows: a few chunks meet all of it, their lists fill and the rest goes to the query's pool;
    a larger crowd overflows the pool and the key buffer of select_i8 too"""
    x, q, pos = C.crowd_case(n=200_000, crowd=crowd, shuffled=False, seed=43)
    idx = _index(ctx, 512, step=4, m=64, i8_key_budget=0)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, 10, f"E crowd appended {crowd}", key_budget=0)
    d = rep["data"]
    assert d["pcnt"][:8].min() > 0, "the pool is not in use: the chunks are too short for this crowd"
    assert (d["pcnt"][:8] > d["L"]["pool_cap"]).all() == past_cap and (d["pcnt"][:8] > d["L"]["pool_cap"]).any() == past_cap
    assert (d["trace"][:, 3] & S.F_OVERFLOW).all()
    if past_cap:                                              # 21 full lists and a full pool: more than the 12,288 keys select_i8 holds
        assert (d["trace"][:, 0] == S.KEY_CAP).all()
    idx.close()


def test_clustered_every_tile_sampled_no_budget(ctx, clustered):
    """step 1, m 64, no key budget: every anchored query gathers its whole cluster (the largest count is printed; the key buffer of
    12,288 is not reached at this size, see profiles/i8_select/NOTES.md)"""
    x, q = clustered
    idx = _index(ctx, 256, step=1, m=64, i8_key_budget=0)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q[:64], 10, "E clustered step1 budget0", key_budget=0)
    assert rep["max_keys"] > 1000
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ F: ties
def test_bit_identical_rows(ctx):
    """600 copies of one row (which sets the scale of every tile it is in, so all copies score alike), a query on it: the top sample
    scores are one number, t is that number, sample and output name the lowest rows"""
    x, q, pos = C.ties_case()
    k, m = 10, 64
    idx = _index(ctx, 256, step=4, m=m)
    idx.add(x)
    rep, cos, ids = _search_and_check(ctx, idx, q, k, "F ties")
    d = rep["data"]
    score, row = S.sample_keys(d, 0)
    assert not S.sample_cut_crowded(score, m)
    assert score.size > m and (score[:m + 1] == score[0]).all() and np.isin(row[:m + 1], pos).all()      # more than m copies sampled, one score
    assert d["thr_int"][0] <= score[0]
    assert np.array_equal(d["sample_ids"][0, :k], row[:k]) and np.array_equal(row[:k], np.sort(row[score == score[0]])[:k])
    assert np.array_equal(d["sel_ids"][0], pos[:k]) and np.array_equal(ids[0], pos[:k]) and (cos[0] == cos[0, 0]).all()
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ G: short sample
@pytest.mark.parametrize("n,step", [(1100, 1), (4 * 1024 + 100, 4)])
def test_short_sample(ctx, n, step):
    """The smallest indexes the int8 pass admits (rows >= 1024 x step): four sampled tiles, 64 sample values per query for m = 64"""
    x, q = C.gaussian_case(n, 256, 20, seed=n)
    idx = _index(ctx, 256, step=step, m=64)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, 3, f"G n{n} step{step}")
    assert rep["data"]["L"]["sample_tiles"] == 4
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ H: bf16 threshold pass
@pytest.mark.parametrize("b", [300, 40])
def test_bf16_threshold_pass(ctx, b):
    x, q = C.gaussian_case(60_000, 256, b, seed=60_000 + b)
    idx = _index(ctx, 256, step=4, m=64, i8_sample_int8=0)
    idx.add(x)
    rep, _, _ = _search_and_check(ctx, idx, q, 10, f"H bf16 sample B{b}")
    assert rep["data"]["L"]["sample_int8"] == 0
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ I: ids
def test_id_base_and_deletes(ctx, wide):
    """select_i8 writes position + id_base; once rows were deleted it writes positions and the search maps them to ids.  The final
    answer is the bf16 route's bit for bit."""
    from semantic_query_engine_amd import SCAN_BF16_RESCORE
    x, q = wide
    base = 1_000_000
    idx = _index(ctx, 512, step=64, m=1, id_base=base)
    idx.add(x)
    _search_and_check(ctx, idx, q, 1, "I id_base", id_base=base)
    idx.delete(np.arange(0, x.shape[0], 7))
    live = idx.ids()
    assert live.size == x.shape[0] - (x.shape[0] + 6) // 7
    rep, cos, ids = _search_and_check(ctx, idx, q, 1, "I id_base + deletes", final_ids=lambda p: np.where(p >= 0, live[np.maximum(p, 0)] + base, -1),
                                      to_position=lambda i: np.searchsorted(live, i - base))
    idx.set_option("scan_mode", SCAN_BF16_RESCORE)
    cos16, ids16 = idx.search(q, 1)
    assert np.array_equal(cos.view(np.uint32), cos16.view(np.uint32)) and np.array_equal(ids, ids16)
    idx.close()
