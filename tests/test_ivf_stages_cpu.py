"""oracle/ivf.py against independent plain formulations on small inputs (no GPU): the restatements that
tests/test_ivf_stages_gpu.py holds the IVF kernels to must themselves be right."""
import math

import numpy as np
import pytest

from oracle import ivf as IV
from oracle import retrieval as R
from oracle import rounding as RD


def _rows(n, dim, seed):
    return R.normalize_rows(np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32))


# ---------------------------------------------------------------- int8 estimate
@pytest.mark.parametrize("dim", [256, 384, 1024, 1280])
def test_i8_strip_against_python_integers_and_true_cosine(dim):
    """The integer dot product by Python integers (no overflow, no rounding), the three float32 products one by one; and the
    estimate lies within scan_eps of the true cosine for the measured quantisation residuals."""
    xn, qn = _rows(40, dim, 1), _rows(3, dim, 2)
    sx, sq = RD.i8_row_scales(xn), RD.i8_row_scales(qn)
    x8, q8 = RD.i8_quantize(xn, sx), RD.i8_quantize(qn, sq)
    unit = np.float32(RD.i8_scale_unit(dim))
    dx = RD.i8_residual(xn, x8, sx).max()
    dq = RD.i8_residual(qn, q8, sq)
    for j in range(3):
        got = IV.i8_strip(x8, sx, q8[j], int(sq[j]), dim)
        assert got.dtype == np.float32 and got.shape == (40,)
        for r in range(40):
            acc = sum(int(a) * int(b) for a, b in zip(x8[r].tolist(), q8[j].tolist()))
            want = np.float32(np.float32(np.float32(acc) * np.float32(int(sx[r]))) * np.float32(np.float32(unit * unit) * np.float32(int(sq[j]))))
            assert got[r].view(np.uint32) == want.view(np.uint32)
        true = xn.astype(np.float64) @ qn[j].astype(np.float64)
        assert np.all(np.abs(got - true) <= RD.scan_eps(dq[j], dx, dim))


def test_i8_strip_rounds_large_accumulators_to_nearest_even():
    """dim 1280 with saturated rows: |acc| = 127^2 * 1280 > 2^24, the conversion to float32 rounds (ties to even)."""
    dim = 1280
    x8 = np.full((2, dim), 127, np.int8)
    x8[1, :3] = [126, 126, 127]                         # acc = 20645120 - 254: odd multiples of 1 above 2^24 are not representable
    q8 = np.full(dim, 127, np.int8)
    got = IV.i8_strip(x8, np.array([1, 1], np.uint32), q8, 1, dim)
    u2 = np.float32(np.float32(RD.i8_scale_unit(dim)) ** 2)
    for r, acc in enumerate((127 * 127 * dim, 127 * 127 * dim - 254)):
        assert acc > 1 << 24
        assert got[r] == np.float32(np.float32(float(acc)) * np.float32(1.0)) * u2
    acc = (1 << 24) + 1                                  # a tie: rounds to the even neighbour 2^24
    assert np.float64(acc).astype(np.float32) == np.float32(1 << 24)


# ---------------------------------------------------------------- tiled layout
def test_tiled_layout_by_a_per_element_loop():
    dim = 128
    lens = [0, 1, 255, 256, 257, 0, 3]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offsets[-1])
    rng = np.random.default_rng(3)
    order = rng.permutation(n).astype(np.int32)
    xn = _rows(n, dim, 4)
    tiled, scales, pos = IV.i8_rows_of_lists(xn, order, offsets)
    toff = IV.tile_offsets(offsets)
    assert toff.tolist() == [0, 0, 1, 2, 3, 5, 5, 6]
    assert tiled.shape == (6, (dim // 64) * 16384 + 2048) and scales.shape == (6 * 256,)
    sx = RD.i8_row_scales(xn)
    x8 = RD.i8_quantize(xn, sx)
    flat = tiled.reshape(-1)
    seen = np.zeros(flat.size, bool)
    for L, ln in enumerate(lens):
        for p in range(ln):
            row = order[offsets[L] + p]
            tile, r = toff[L] + p // 256, p % 256
            assert pos[offsets[L] + p] == tile * 256 + r
            assert scales[tile * 256 + r] == sx[row]
            for e in range(dim):
                at = tile * tiled.shape[1] + (e // 64) * 16384 + r * 64 + e % 64
                assert flat[at] == x8[row, e]
                seen[at] = True
    assert not flat[~seen].any()                        # nothing else is written
    assert np.array_equal(IV.untile(tiled, pos, dim), x8[order])


def test_scale_boundary_marks_only_near_integers():
    dim = 256
    xn = _rows(2000, dim, 5)
    b = IV.scale_boundary(xn)
    t = RD.i8_need(xn) / RD.i8_scale_unit(dim) * 1.000001
    assert b.sum() <= 4                                  # ~ 2 * 160 * 2.4e-7 per row
    assert np.all(np.abs(t[b] - np.rint(t[b])) < 1e-3)
    # a float32 evaluation of the same chain disagrees with float64 only on marked rows
    need32 = np.maximum(np.abs(xn).max(1) / np.float32(127), np.sqrt((xn * xn).sum(1, dtype=np.float32)) / np.float32(2800))
    s32 = np.ceil(need32 / np.float32(RD.i8_scale_unit(dim)) * np.float32(1.000001)).astype(np.int64)
    assert np.all((s32 == RD.i8_row_scales(xn)) | b)


# ---------------------------------------------------------------- bf16 estimate
def test_bf16_strip_is_the_dot_product_of_the_copies():
    xn, qn = _rows(20, 320, 6), _rows(1, 320, 7)
    xb, qb = RD.bf16_round(xn), RD.bf16_round(qn)[0]
    got = IV.bf16_strip(xb, qb)
    for r in range(20):
        want = math.fsum(float(a) * float(b) for a, b in zip(RD.bf16_to_f32(xb[r]).tolist(), RD.bf16_to_f32(qb).tolist()))
        assert abs(got[r] - want) < 1e-15
    assert np.all(np.abs(got - xn.astype(np.float64) @ qn[0].astype(np.float64)) < RD.scan_eps(RD.bf16_residual(qn)[0], RD.bf16_residual(xn).max(), 320))


# ---------------------------------------------------------------- collect mode
def test_collect_reference_keys_and_threshold_rank():
    rng = np.random.default_rng(8)
    est = [rng.standard_normal(300).astype(np.float32), rng.standard_normal(10).astype(np.float32)]
    est[0][5] = np.nan
    est[1][2] = est[0][7]                               # a tie across lists
    ids = [np.arange(300) + 1000, np.arange(10)]
    thr = float(np.sort(est[0][~np.isnan(est[0])])[-20])
    keys = IV.collect_reference(est, ids, thr)
    want = set()
    for e, r in zip(est, ids):
        for s, i in zip(e.tolist(), r.tolist()):
            if s == s and np.float32(s) >= np.float32(thr):
                bits = int(np.float32(s).view(np.uint32))
                o = (~bits & 0xFFFFFFFF) if bits & 0x80000000 else bits | 0x80000000
                want.add((o << 32) | (0xFFFFFFFF - i))
    assert set(keys.tolist()) == want and keys.size == len(want)
    assert np.all(np.diff(keys.astype(np.float64)) >= 0)
    everything = IV.collect_reference(est, ids, -np.inf)
    assert everything.size == 309                       # all but the NaN
    # the key order is (score desc, row asc)
    k = IV.make_keys(np.array([1.0, 1.0, -2.0, 0.0], np.float32), np.array([3, 4, 0, 0]))
    assert k[0] > k[1] > k[3] > k[2]
    # rank rule
    assert IV.collect_want(256 * 8, 2048, 40) == 0 and IV.collect_want(0, 9000, 40) == 0
    S, total, kp = 2048, 6000, 40
    t = 8.0 * kp * S / total
    w = IV.collect_want(S, total, kp)
    assert w == int(t + 3 * math.sqrt(t) + 2) and w < S
    assert IV.collect_want(100, 60000, 256) == min(100, int(8 * 256 * 100 / 60000 + 3 * math.sqrt(8 * 256 * 100 / 60000) + 2))
    sample = np.arange(100, dtype=np.float32)
    sample[10] = np.nan
    assert IV.threshold_rank_ok(sample, 90.0, 10)       # the 10th largest of 99 .. 0
    assert IV.threshold_rank_ok(sample, 90.0, 9) and IV.threshold_rank_ok(sample, 90.0, 11)
    assert not IV.threshold_rank_ok(sample, 90.0, 12) and not IV.threshold_rank_ok(sample, 90.0, 8)
    assert not IV.threshold_rank_ok(sample, 90.5, 10)   # not a sample score
    tied = np.array([5, 4, 4, 4, 1], np.float32)
    assert all(IV.threshold_rank_ok(tied, 4.0, w) for w in (1, 2, 3, 4, 5)) and not IV.threshold_rank_ok(tied, 4.0, 6)


# ---------------------------------------------------------------- k-means
def test_splitmix_and_picks():
    # splitmix64 from state 0: the published first outputs
    s, a = IV.splitmix(0)
    s, b = IV.splitmix(s)
    assert a == 0xE220A8397B1DCDAF and b == 0x6E789E6AA1B965F4
    for n, nlist, seed in ((16, 16, 0), (4000, 16, 7), (100, 3, 1 << 63)):
        p = IV.train_picks(n, nlist, seed)
        assert p.shape == (nlist,) and np.unique(p).size == nlist and p.min() >= 0 and p.max() < n
    assert sorted(IV.train_picks(16, 16, 3).tolist()) == list(range(16))          # n = nlist: every row is a pick
    assert not np.array_equal(IV.train_picks(4000, 16, 1), IV.train_picks(4000, 16, 2))


def test_kmeans_reference_unit_norm_empty_lists_and_fixed_point():
    rng = np.random.default_rng(9)
    cen = R.normalize_rows(rng.standard_normal((4, 32)).astype(np.float32))
    x = R.normalize_rows(cen[rng.integers(0, 4, 400)] + 0.05 * rng.standard_normal((400, 32)).astype(np.float32))
    # picks 0 and 1 are copies: in the first iteration list 1 loses every row to list 0 (ties go to the lowest id) and keeps its
    # centroid (afterwards centroid 0 has moved and the two copies are nearest to the one that stayed)
    x[1] = x[0]
    picks = np.array([0, 1, 2, 3])
    its = IV.kmeans_reference(x, picks, 3)
    assert len(its) == 3
    for it in its:
        assert np.allclose(np.linalg.norm(it["centroids"], axis=1), 1.0, atol=1e-12)
        assert it["counts"].sum() == 400 and np.all(it["gap"] >= 0)
    assert its[0]["counts"][1] == 0 and np.array_equal(its[0]["centroids"][1], x[1].astype(np.float64))
    assert its[1]["counts"][1] == 2 and set(np.flatnonzero(its[1]["assign"] == 1).tolist()) == {0, 1}
    # one step restated plainly
    c0 = x[picks].astype(np.float64)
    s = x.astype(np.float64) @ c0.T
    a = np.array([int(np.flatnonzero(row == row.max())[0]) for row in s])
    assert np.array_equal(its[0]["assign"], a)
    for c in (0, 2, 3):
        m = x[a == c].astype(np.float64).sum(0)
        assert np.allclose(its[0]["centroids"][c], m / np.linalg.norm(m), atol=1e-12)
        assert np.allclose(its[0]["abs_sums"][c], np.abs(x[a == c].astype(np.float64)).sum(0))
