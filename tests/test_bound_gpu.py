"""The error bound of the exactness certificate, row by row, on the library's own copies and its own measured residuals -- and
end to end on inputs built so that the bound is what finds the answer.

    |scan score - fp32 cosine| <= scan_eps(dq, dx, K)                                     (csrc/kernels.h)

Section A recomputes both sides in float64 from what the library holds (sqe_index_state_read, sqe_index_i8_read): est from the
scanned copies (bf16: <bf16 q, bf16 x>; int8: S0^2 sxi sqi <x8, q8>), true from the fp32 rows and queries, eps from the
MEASURED dq and dx.  Every (query, row) must satisfy |est - true| <= eps - acc_term: the accumulation term belongs to the
kernels' fp32 chains, which float64 does not have.  On Gaussian rows the two sides are a factor ~20 apart; the adversarial
builders of rounding_cases.py bring them within 0.85 (bf16) and 0.6 (int8), so a residual measured a little short fails here.

Section B searches those inputs.  For each adversarial query the bf16 scan ranks 600 decoys above the 10 true neighbours, every
candidate list fills with decoys, the certificate must fail, and only a collect threshold of (k-th cosine) - eps with a sound
eps reaches the true neighbours (the gap is 2.5e-4 of a 2e-3 bound).  The oracle is float64 over the library's fp32 rows."""
import os

import numpy as np
import pytest

from oracle import retrieval as R
from oracle import rounding as RD

from . import rounding_cases as RC
from .gpu_util import assert_topk_matches

pytestmark = pytest.mark.gpu
K = RC.K_ADV


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _bf16_index(ctx, x):
    from semantic_query_engine_amd import SCAN_BF16_RESCORE, VectorIndex
    idx = VectorIndex(ctx, x.shape[1])
    idx.set_option("scan_mode", SCAN_BF16_RESCORE)
    idx.add(x)
    return idx


def _i8_index(ctx, x):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    idx = VectorIndex(ctx, x.shape[1])
    idx.set_option("scan_mode", SCAN_INT8_RESCORE)
    idx.set_option("i8_min_rows", 0)
    idx.set_option("i8_sample_step", 1)
    idx.add(x)
    return idx


# ================================================================ A: the bound, row by row
def _bf16_bound(idx, B):
    """-> (err [rows, B], eps [B]) from the library's bf16 copy, fp32 rows, normalised queries and measured residuals"""
    from semantic_query_engine_amd import engine as E
    n, dim = len(idx), idx.dim
    xn = idx.get_rows(idx.ids())
    qn = idx.state_read(E.STATE_QN, np.float32, B * dim).reshape(B, dim)
    xb = RD.bf16_to_f32(idx.scan_bf16()[:n]).astype(np.float64)
    qb = RD.bf16_to_f32(RD.bf16_round(qn)).astype(np.float64)          # the query block is the same kernel's bf16 output
    dq = idx.state_read(E.STATE_Q_RESID, np.float32, B)
    dx = idx.state_read(E.STATE_RESID_MAX, np.float32, 1)[0]
    with np.errstate(all="ignore"):
        err = np.abs(xb @ qb.T - xn.astype(np.float64) @ qn.astype(np.float64).T)
    return err, RD.scan_eps(dq, dx, dim).astype(np.float64)


def _i8_bound(idx, B):
    from semantic_query_engine_amd import engine as E
    n, dim = len(idx), idx.dim
    st, L = idx.state(), idx.i8_last()
    assert st["last_i8"] == 1 and st["i8_rows"] == n and (L["B"], L["rows"]) == (B, n)
    tiles, stride, hs = (n + 255) // 256, st["i8_tile_stride"], dim // 64
    raw = idx.i8_read(E.I8_ROWS, np.int8, tiles * stride).reshape(tiles, stride)[:, :hs * 256 * 64].reshape(tiles, hs, 256, 64)
    x8 = np.ascontiguousarray(raw.transpose(0, 2, 1, 3)).reshape(tiles * 256, dim)[:n].astype(np.float64)
    sxi = idx.i8_read(E.I8_ROW_SCALES, np.uint32, tiles * 256)[:n].astype(np.float64)
    q8 = idx.i8_read(E.I8_QUERIES, np.int8, L["b_pad"] * L["q_pitch"]).reshape(L["b_pad"], L["q_pitch"])[:B, :dim].astype(np.float64)
    sqi = idx.state_read(E.STATE_Q8_SCALES, np.uint32, B).astype(np.float64)
    xn = idx.get_rows(idx.ids())
    qn = idx.state_read(E.STATE_QN, np.float32, B * dim).reshape(B, dim)
    dq = idx.state_read(E.STATE_Q8_RESID, np.float32, B)
    dx = idx.state_read(E.STATE_I8_RESID_MAX, np.float32, 1)[0]
    s0 = RD.i8_scale_unit(dim)
    with np.errstate(all="ignore"):
        est = s0 * s0 * sxi[:, None] * sqi[None, :] * (x8 @ q8.T)
        err = np.abs(est - xn.astype(np.float64) @ qn.astype(np.float64).T)
    return err, RD.scan_eps(dq, dx, dim).astype(np.float64), sxi


def _assert_bound(err, eps, dim, label):
    """every finite (row, query) within eps - acc_term; -> the tightness ratio max |est - true| / eps"""
    room = eps[None, :] - RD.acc_term(dim)
    ok = np.isnan(err) | (err <= room)                       # a NaN row has no score to bound: the fp32 re-score decides
    ratio = float(np.nanmax(err / eps[None, :]))
    print(f"{label}: max |est - true| {np.nanmax(err):.4e}, eps {np.nanmin(eps):.4e} .. {np.nanmax(eps):.4e}, ratio {ratio:.3f}")
    assert ok.all(), (label, np.argwhere(~ok)[:5], err[~ok][:5], room[0, np.nonzero(~ok)[1][:5]])
    return ratio


@pytest.mark.parametrize("dim,n", [(256, 1553), (1024, 1553), (8192, 1100)])
def test_bound_on_gaussian_and_edge_rows(ctx, dim, n):
    """Gaussian rows with the edge rows of test_copies_gpu.py mixed in, queries likewise: bf16 on all of them, int8 on the rows
    that quantise within "i8_max_resid"."""
    x, edge_pos = RC.copies_case(dim, n, seed=2)
    q, _ = RC.copies_case(dim, 70, seed=3, edges=False)
    q[:8] = RC.edge_rows(dim, seed=5)
    q[9] = x[100] * 3.0
    idx = _bf16_index(ctx, x)
    idx.search(q, K)
    err, eps = _bf16_bound(idx, 70)
    assert np.isnan(err[:, 5]).all() and np.isnan(err[edge_pos[5]]).all() and np.isfinite(np.delete(np.delete(err, 5, 1), edge_pos[5], 0)).all()
    _assert_bound(err, eps, dim, f"bf16 gaussian + edges dim {dim}")
    idx.close()
    keep = np.setdiff1d(np.arange(n), edge_pos[6:])          # without one_hot / one_large: they send the index to the bf16 scan
    q[6:8] = q[10:12]
    q[5] = q[12]                                             # ... and without the NaN query (no int8 residual to read)
    idx = _i8_index(ctx, x[keep])
    idx.search(q, K)
    err, eps, _ = _i8_bound(idx, 70)
    _assert_bound(err, eps, dim, f"int8 gaussian + edges dim {dim}")
    idx.close()


# ================================================================ B: end to end on the adversarial builders
class _Adv:
    """One adversarial index and its float64 oracle over the library's own fp32 rows."""

    def __init__(self, ctx, case, make_index):
        self.case = case
        self.x, self.q = case["x"], case["q"]
        self.idx = make_index(ctx, self.x)
        self.n = self.x.shape[0]
        self.xn = self.idx.get_rows(np.arange(self.n))
        self.qn = R.normalize_rows(self.q)
        # float64 scores of every distinct query: fp32 shortlist (everything within 1e-3 of the k-th), float64 over it
        self.s32 = self.qn @ self.xn.T
        self.n_adv = case["n_adv"]

    def batch(self, B):
        """B queries: the distinct ones tiled; -> (queries, index of each into the distinct ones)"""
        which = np.arange(B) % self.q.shape[0]
        return self.q[which], which

    def oracle(self, which, k, allowed=None):
        cos = np.full((which.size, k), -np.inf)
        ids = np.full((which.size, k), -1, np.int64)
        done = {}
        for i, b in enumerate(which):
            if b not in done:
                s = self.s32[b] if allowed is None else np.where(allowed, self.s32[b], -np.inf)
                kth = np.partition(s, -k)[-k]
                cand = np.nonzero(s >= kth - 1e-3)[0]
                s64 = self.xn[cand].astype(np.float64) @ self.qn[b].astype(np.float64)
                order = np.argsort(-s64, kind="stable")[:k]
                done[b] = (s64[order], cand[order])
            cos[i], ids[i] = done[b]
        return cos, ids

    def n_adversarial(self, which):
        return int((which < self.n_adv).sum())

    def check(self, cos, ids, which, allowed=None, idx_ids=None):
        ref_cos, ref_ids = self.oracle(which, K, allowed)
        assert_topk_matches(cos, ids, ref_cos, ref_ids, self.xn, self.qn[which], tol=2e-6)
        for i, b in enumerate(which):
            if b < self.n_adv:
                assert ids[i].tolist() == self.case["true_ids"][b].tolist(), (i, b)      # T, in order


@pytest.fixture(scope="module", params=[64, 1024])
def adv(request, ctx):
    a = _Adv(ctx, RC.bf16_adversarial(request.param), _bf16_index)
    yield a
    a.idx.close()


@pytest.mark.parametrize("B", [8, 100, 300])
def test_search_finds_the_true_neighbours_behind_the_decoys(ctx, adv, B):
    """all three query-block kernels (64, 128, 256 queries per workgroup); the certificate must fail for every adversarial query"""
    q, which = adv.batch(B)
    ctx.stats_reset()
    cos, ids = adv.idx.search(q, K)
    unc = ctx.stats()["uncertified"]
    print(f"dim {adv.idx.dim} B {B}: {unc} uncertified, {adv.n_adversarial(which)} adversarial queries")
    adv.check(cos, ids, which)
    assert unc >= adv.n_adversarial(which)


def test_bound_on_the_adversarial_rows(ctx, adv):
    q, which = adv.batch(adv.q.shape[0])
    adv.idx.search(q, K)
    err, eps = _bf16_bound(adv.idx, q.shape[0])
    ratio = _assert_bound(err, eps, adv.idx.dim, f"bf16 adversarial dim {adv.idx.dim}")
    assert ratio >= 0.85                                     # the library's own copies and residuals reach what the builder promises


def test_filtered_search_on_the_adversarial_rows(ctx, adv):
    c = adv.case
    allow = np.concatenate([c["true_ids"].ravel(), c["decoy_ids"].ravel(), c["background_ids"][::2]])
    allowed = np.zeros(adv.n, bool)
    allowed[allow] = True
    q, which = adv.batch(8)
    cos, ids = adv.idx.search(q, K, filter_ids=allow)
    adv.check(cos, ids, which, allowed)


def test_range_search_counts_exactly_the_true_neighbours(ctx, adv):
    c = adv.case
    q, which = adv.batch(adv.n_adv)
    true = np.stack([adv.xn[c["true_ids"][b]].astype(np.float64) @ adv.qn[b].astype(np.float64) for b in range(adv.n_adv)])
    min_cos = np.nextafter(true.min(axis=1).astype(np.float32), np.float32(-np.inf))       # min true(T), down one fp32 ulp
    counts, cos, ids = adv.idx.range_search(q, min_cos, max_hits=16)
    print(f"dim {adv.idx.dim}: radial counts {counts.tolist()}")
    assert counts.tolist() == [K] * adv.n_adv
    for b in range(adv.n_adv):
        assert ids[b, :K].tolist() == c["true_ids"][b].tolist() and np.all(ids[b, K:] == -1)


def _collapsed_oracle(adv, which, keys, k, depth=900):
    """the k best groups and each group's best row: float64 ranking of the `depth` best rows by fp32 score, first row of every key"""
    cos = np.full((which.size, k), -np.inf)
    ids = np.full((which.size, k), -1, np.int64)
    for i, b in enumerate(which):
        cand = np.sort(np.argpartition(-adv.s32[b], depth)[:depth])
        s64 = adv.xn[cand].astype(np.float64) @ adv.qn[b].astype(np.float64)
        seen, out = set(), []
        for j in np.argsort(-s64, kind="stable"):
            if keys[cand[j]] not in seen:
                seen.add(keys[cand[j]])
                out.append(j)
                if len(out) == k:
                    break
        cos[i, :len(out)], ids[i, :len(out)] = s64[out], cand[out]
    return cos, ids


def test_collapsed_search_sweeps_past_the_decoy_groups(ctx, adv):
    """Every true neighbour and every background row has a key of its own; the decoys share keys.

    With ALL decoys under one key and k = 10 (the layout first proposed for this test) the sweep never runs: the first stage
    of a collapsed search is itself the certified search, at depth 64, so it returns the 10 true neighbours and 54 decoys --
    11 groups, enough for k = 10 (measured: collapse_swept = 0, answer correct).  That search is kept below as a plain check.
    The sweep is reached with the decoys under TWO keys (D_0 .. D_299, D_300 .. D_599) and k = 12: the 64 rows of the first
    stage hold 11 groups, one short, and the sweep has to rebuild the answer from collect scans at (running 12th group cosine)
    - eps.  The 12th group is the second decoy key (best row D_300, cosine 0.87659), so the true neighbours (scan score 0.875)
    clear the final threshold by 4e-4 of a 2e-3 bound: a residual measured at half its value loses them."""
    from semantic_query_engine_amd import engine as E
    c = adv.case
    q, which = adv.batch(8)
    keys = np.arange(adv.n, dtype=np.int64) + 1000
    keys[c["decoy_ids"].ravel()] = 7
    try:
        adv.idx.set_keys(np.arange(adv.n), keys)
        cos, ids, got_keys = adv.idx.search_collapsed(q, K)
        print(f"dim {adv.idx.dim}: one decoy key, k = {K}: {ctx.stats()['collapse_swept']} queries swept")
        adv.check(cos, ids, which)                   # the plain top-k is the collapsed answer: T outranks the decoy group
        assert np.array_equal(got_keys, keys[ids])
        keys[c["decoy_ids"][:, 300:].ravel()] = 8
        adv.idx.set_keys(np.arange(adv.n), keys)
        k = K + 2
        cos, ids, got_keys = adv.idx.search_collapsed(q, k)
        swept = ctx.stats()["collapse_swept"]
        print(f"dim {adv.idx.dim}: two decoy keys, k = {k}: {swept} queries swept")
        ref_cos, ref_ids = _collapsed_oracle(adv, which, keys, k)
        assert_topk_matches(cos, ids, ref_cos, ref_ids, adv.xn, adv.qn[which], tol=2e-6)
        assert np.array_equal(got_keys, keys[ids])
        for i, b in enumerate(which):
            if b < adv.n_adv:
                assert ids[i].tolist() == c["true_ids"][b].tolist() + [c["decoy_ids"][b, 0], c["decoy_ids"][b, 300]]
        assert swept >= adv.n_adversarial(which) > 0
    finally:
        adv.idx.set_keys(np.arange(adv.n), np.full(adv.n, E.KEY_NONE, np.int64))


def test_saved_and_loaded_index_finds_them_too(ctx, adv, tmp_path):
    from semantic_query_engine_amd import SCAN_BF16_RESCORE, VectorIndex
    path = os.path.join(tmp_path, "adv.sqe")
    adv.idx.save(path)
    loaded = VectorIndex.load(ctx, path)
    loaded.set_option("scan_mode", SCAN_BF16_RESCORE)
    q, which = adv.batch(8)
    ctx.stats_reset()
    cos, ids = loaded.search(q, K)
    unc = ctx.stats()["uncertified"]
    adv.check(cos, ids, which)
    assert unc >= adv.n_adversarial(which)
    loaded.close()


def test_two_shard_group_finds_them_too(adv):
    from semantic_query_engine_amd import EXCHANGE_COPY, SCAN_BF16_RESCORE, Context, VectorIndex
    gctx = Context(devices=[0, 0], exchange=EXCHANGE_COPY)
    idx = VectorIndex(gctx, adv.idx.dim)
    idx.set_option("scan_mode", SCAN_BF16_RESCORE)
    idx.add(adv.x)
    q, which = adv.batch(8)
    gctx.stats_reset()
    cos, ids = idx.search(q, K)
    unc = gctx.stats()["uncertified"]
    adv.check(cos, ids, which)
    assert unc >= adv.n_adversarial(which)
    idx.close()
    gctx.close()


def test_int8_pass_finds_the_true_neighbours_behind_the_decoys(ctx):
    """dim 256, every tile scale pinned at 641: the int8 estimates rank 600 decoys above the 10 true neighbours (222 against 220
    units) with |est - true| at 0.85 of the int8 eps.

    With the default options the collect threshold is ANCHORED at (best true cosine of the sample) - 1.25 eps8, so the int8
    pass itself collects the true neighbours and its certificate holds by construction (measured: 0 uncertified) -- provided
    eps8 is sound: at half its value the anchor passes them by and the certificate still "holds".  The second search takes the
    anchor away ("i8_key_budget" below the crowd: the m-th sample score alone stands, above every true neighbour): there the
    int8 certificate must fail for every adversarial query and the bf16 collect pass supplies the answer."""
    a = _Adv(ctx, RC.i8_adversarial(), _i8_index)
    q, which = a.batch(a.q.shape[0])
    ctx.stats_reset()
    cos, ids = a.idx.search(q, K)
    st = ctx.stats()
    print(f"int8, anchored: {st['i8_collected']} keys collected, {st['uncertified']} uncertified, {a.n_adversarial(which)} adversarial queries")
    a.check(cos, ids, which)
    assert st["i8_collected"] > 0                            # the int8 path ran
    err, eps, sxi = _i8_bound(a.idx, q.shape[0])
    assert np.all(sxi == RC.I8_PIN_SXI)                      # the pin rows fix every tile's scale
    ratio = _assert_bound(err, eps, RC.I8_DIM, "int8 adversarial")
    assert ratio >= 0.6
    a.idx.set_option("i8_key_budget", 64)
    ctx.stats_reset()
    cos, ids = a.idx.search(q, K)
    st = ctx.stats()
    print(f"int8, no anchor: {st['i8_collected']} keys collected, {st['uncertified']} uncertified")
    a.check(cos, ids, which)
    assert st["i8_collected"] > 0
    assert st["uncertified"] >= a.n_adversarial(which)
    a.idx.close()
