"""The seeded builders of rounding_cases.py have the properties the GPU tests rely on, shown from the NumPy restatement
(oracle/rounding.py) alone: the bound holds row by row, the adversarial rows reach most of it in the direction that hides
true neighbours, and only a sound eps brings those neighbours back."""
import numpy as np
import pytest

from oracle import retrieval as R
from oracle import rounding as RD

from . import rounding_cases as RC

BF16_RATIO = 0.85     # largest |est - true| / eps the bf16 builder must reach
I8_RATIO = 0.6        # ... and the int8 builder


def test_bf16_round_matches_the_bit_rule():
    x = np.array([1.0, 1.00390625, 1.01171875, -0.4375 - 0.45 * 2.0 ** -9, 3e38, np.inf, 0.0, -0.0, 1e-40], np.float32)
    b = RD.bf16_round(x)
    # 1 + 2^-8 is the midpoint between 0x3F80 and 0x3F81: ties to even go down; 1 + 3 * 2^-8 is the next one: up to 0x3F82
    assert b[:3].tolist() == [0x3F80, 0x3F80, 0x3F82]
    assert RD.bf16_to_f32(b[3:4])[0] == np.float32(-0.4375)
    assert b[5] == 0x7F80 and b[6] == 0 and b[7] == 0x8000
    nan = np.array([0x7FC00001, 0xFF800001, 0x7F80FFFF], np.uint32).view(np.float32)
    assert RD.bf16_round(nan).tolist() == [0x7FC0, 0xFFC0, 0x7FC0]          # quiet, sign kept, never rounded into inf
    rng = np.random.default_rng(0)
    v = rng.standard_normal(100000).astype(np.float32)
    back = RD.bf16_to_f32(RD.bf16_round(v)).astype(np.float64)
    assert np.all(np.abs(back - v) <= np.abs(v.astype(np.float64)) * 2.0 ** -8)   # half an ulp of 8 significant bits
    assert np.array_equal(RD.bf16_round(RD.bf16_to_f32(RD.bf16_round(v))), RD.bf16_round(v))


def test_scan_eps_and_scale_unit():
    assert RD.i8_scale_unit(256) == pytest.approx(4.0 / (127 * 160 * 16), rel=1e-6)
    assert RD.acc_term(1024) == pytest.approx(2.0e-4, rel=1e-6) and RD.acc_term(8192) == pytest.approx(8192 * 2.0 ** -23 * 1.05, rel=1e-6)
    assert float(RD.scan_eps(0.0, 1.8e-3, 64)) == pytest.approx(1.8e-3 * 1.000001 + 2e-4, rel=1e-6)
    assert float(RD.scan_eps(1e-3, 2e-3, 1024)) == pytest.approx(1.001 * 2e-3 + 1e-3 + 2e-4, rel=1e-5)


def test_i8_restatement_properties():
    x, _ = RC.copies_case(256, 600, seed=1)
    xn = R.normalize_rows(x)
    sc = RD.i8_tile_scales(xn)
    x8 = RD.i8_quantize(xn, sc)
    fin = RD.i8_finite_rows(xn)
    s = sc.astype(np.float64) * RD.i8_scale_unit(256)
    assert np.all(np.abs(x8.astype(np.int32)) <= 127) and not x8[~fin].any()
    assert np.all(np.abs(xn[fin].astype(np.float64) / s[fin, None] - x8[fin]) <= 0.5 + 1e-4)
    assert np.all(127 * s[fin] >= np.abs(xn[fin]).max(axis=1))
    assert len(set(sc[:256].tolist())) == 1 and len(set(sc[512:].tolist())) == 1
    assert np.all(RD.i8_residual(xn, x8, sc)[fin] <= 0.5 * s[fin] * 16 + 1e-9)


@pytest.fixture(scope="module", params=[64, 1024])
def bf16_case(request):
    dim = request.param
    c = RC.bf16_adversarial(dim, n_background=3000)
    xn, qn = R.normalize_rows(c["x"]), R.normalize_rows(c["q"])
    xb, qb = RD.bf16_to_f32(RD.bf16_round(xn)).astype(np.float64), RD.bf16_to_f32(RD.bf16_round(qn)).astype(np.float64)
    est = xb @ qb.T
    true = xn.astype(np.float64) @ qn.astype(np.float64).T
    dx = np.float32(RD.bf16_residual(xn).max() * 1.0001)
    dq = (RD.bf16_residual(qn) * 1.0001).astype(np.float32)
    return dim, c, est, true, dq, dx


def test_bf16_builder_reaches_the_bound(bf16_case):
    dim, c, est, true, dq, dx = bf16_case
    assert np.array_equal(R.normalize_rows(c["q"]), c["q"]) and not dq.any()      # unit, bf16-exact queries: dq = 0
    eps = RD.scan_eps(dq, dx, dim).astype(np.float64)
    err = np.abs(est - true)
    assert np.all(err <= eps[None, :] - RD.acc_term(dim))                         # the bound itself, without its fp32-chain share
    ratio = (err / eps[None, :]).max()
    print(f"bf16 dim {dim}: dx {dx:.4e} eps {eps[0]:.4e} max |est - true| {err.max():.4e} ratio {ratio:.3f}")
    assert ratio >= BF16_RATIO
    for b in range(c["n_adv"]):
        t, d = c["true_ids"][b], c["decoy_ids"][b]
        assert (err[t, b] / eps[b]).min() >= BF16_RATIO                           # every true neighbour sits that deep
        assert np.all(est[t, b] < true[t, b])                                     # ... and is under-scored


def test_bf16_builder_hides_true_neighbours_from_an_unsound_eps(bf16_case):
    dim, c, est, true, dq, dx = bf16_case
    bg = c["background_ids"]
    assert true[bg].max() <= 0.5
    for b in range(c["n_adv"]):
        t, d = c["true_ids"][b], c["decoy_ids"][b]
        assert np.all(np.diff(true[t, b]) < -2.5e-6)                              # T in order, resolvable by the 2e-6 tie rule
        assert true[t, b].min() > true[d, b].max() + 1e-5                         # every T beats every D ...
        assert est[d, b].min() > est[t, b].max() + 5e-4                           # ... and every D outranks every T in the scan
        others = np.setdiff1d(np.arange(true.shape[0]), np.concatenate([t, d]))
        assert true[others, b].max() <= 0.5
        # the collect pass starts from the decoys: threshold = (10th best true cosine among them) - eps
        kth = np.sort(true[d, b])[-RC.K_ADV]
        assert kth - float(RD.scan_eps(dq[b], dx, dim)) < est[t, b].min()         # a sound eps collects every T
        assert kth - float(RD.scan_eps(dq[b], np.float32(0.8) * dx, dim)) > est[t, b].max()   # dx at 0.8 of its value loses them all


def test_bf16_builder_spreads_decoys_over_every_tile(bf16_case):
    dim, c, *_ = bf16_case
    tiles = (c["x"].shape[0] + 255) // 256
    for b in range(c["n_adv"]):
        assert np.unique(c["decoy_ids"][b] // 256).size == tiles
        assert np.unique(c["true_ids"][b] // 256).size >= RC.K_ADV // 2


@pytest.fixture(scope="module")
def i8_case():
    c = RC.i8_adversarial()
    xn, qn = R.normalize_rows(c["x"]), R.normalize_rows(c["q"])
    sx, sq = RD.i8_tile_scales(xn), RD.i8_row_scales(qn)
    x8, q8 = RD.i8_quantize(xn, sx), RD.i8_quantize(qn, sq)
    s0 = RD.i8_scale_unit(RC.I8_DIM)
    est = s0 * s0 * sx[:, None].astype(np.float64) * sq[None, :].astype(np.float64) * (x8.astype(np.float64) @ q8.astype(np.float64).T)
    true = xn.astype(np.float64) @ qn.astype(np.float64).T
    dx = np.float32(RD.i8_residual(xn, x8, sx).max() * 1.0001 + 1e-7)
    dq = (RD.i8_residual(qn, q8, sq) * 1.0001 + 1e-7).astype(np.float32)
    return c, sx, est, true, dq, dx


def test_i8_builder_reaches_the_bound(i8_case):
    c, sx, est, true, dq, dx = i8_case
    assert np.all(sx == RC.I8_PIN_SXI)                                            # the pin rows fix every tile's scale
    assert dx < 0.02                                                              # within "i8_max_resid": the int8 pass answers
    eps = RD.scan_eps(dq, dx, RC.I8_DIM).astype(np.float64)
    err = np.abs(est - true)
    assert np.all(err <= eps[None, :] - RD.acc_term(RC.I8_DIM))
    ratio = (err / eps[None, :]).max()
    print(f"int8: dx {dx:.4e} dq {dq[0]:.4e} eps {eps[0]:.4e} max |est - true| {err.max():.4e} ratio {ratio:.3f}")
    assert ratio >= I8_RATIO
    for b in range(c["n_adv"]):
        t, d = c["true_ids"][b], c["decoy_ids"][b]
        assert (err[t, b] / eps[b]).min() >= I8_RATIO and np.all(est[t, b] < true[t, b])
        assert np.all(np.diff(true[t, b]) < -2.5e-6)
        assert true[t, b].min() > true[d, b].max() + 1e-5
        assert est[d, b].min() > est[t, b].max() + 1e-3
        others = np.setdiff1d(np.arange(true.shape[0]), np.concatenate([t, d]))
        assert true[others, b].max() <= 0.5
