"""Seeded inputs for the tests of the scanned copies, the measured residuals and the error bound built on them
(test_rounding_cases_cpu.py, test_copies_gpu.py, test_bound_gpu.py), in the style of golden_cases.py.

Random rows round benignly: the errors of a dot product average out to ~1e-4 while the bound is ~2e-3.  The adversarial
builders below make every rounding of a row push its scan score the same way, so that |scan score - true cosine| reaches
most of scan_eps -- in the direction that hides true neighbours behind decoys.  test_rounding_cases_cpu.py asserts that
from the NumPy restatement (oracle/rounding.py) alone.
"""
import numpy as np

from oracle import rounding as RD

EDGE_NAMES = ("zero", "tiny_element", "scaled_1e-12", "scaled_1e15", "inf_sum_of_squares", "nan_element", "one_hot", "one_large")
K_ADV = 10            # true neighbours per adversarial query
N_DECOYS = 600        # more than MAX_KP = 256: they fill every candidate list


def edge_rows(dim, seed=3):
    """The eight edge rows of EDGE_NAMES, raw (before normalisation)."""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((len(EDGE_NAMES), dim)).astype(np.float32)
    e[0] = 0.0
    e[1] = 0.0; e[1, dim // 3] = 1e-20
    e[2] *= np.float32(1e-12)
    e[3] *= np.float32(1e15)
    e[4, 5] = 3e38                      # the sum of squares overflows to inf: the row normalises to zeros (and one NaN-free 0)
    e[5, dim - 1] = np.nan
    e[6] = 0.0; e[6, 7] = -2.5
    e[7, dim // 2] = 50.0 * np.abs(e[7]).max()
    return e


def copies_case(dim, rows, seed=0, edges=True):
    """Gaussian rows of mixed magnitude with the edge rows mixed in (first tile, a middle tile, the partial last tile).
    -> (x raw float32 [rows, dim], positions of the edge rows in EDGE_NAMES order)."""
    rng = np.random.default_rng(seed * 1000 + dim)
    x = (rng.standard_normal((rows, dim)) * rng.uniform(0.01, 50.0, (rows, 1))).astype(np.float32)
    pos = np.zeros(0, np.int64)
    if edges:
        pos = np.array([0, 5, rows // 2, rows // 2 + 1, rows // 2 + 7, rows - 3, rows - 2, rows - 1], np.int64)
        x[pos] = edge_rows(dim, seed + 3)
    return x, pos


# ------------------------------------------------------------------------------ bf16 builder
G = 0.4375            # a bf16 grid point in [0.25, 0.5)
U = 2.0 ** -9         # the bf16 ulp there


def _bf16_floor(v):
    """largest bf16-representable value <= v (v > 0)"""
    u = np.array([v], np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return float(u.view(np.float32)[0])


def _nested_mass(rem, snap, n=3):
    """n coordinates whose squares sum to rem: grid points (snap) taken greedily, the last one whatever is left"""
    out = []
    for _ in range(n - 1):
        m = snap(np.sqrt(rem))
        out.append(m)
        rem = max(rem - m * m, 0.0)
    out.append(np.sqrt(max(rem, 0.0)))
    return out


def _sparse_row(dim, block, active, mass_snap=_bf16_floor):
    """unit row: `active` on coordinates 8 block .. 8 block + 3, the rest of the norm on 8 block + 4 .. + 6"""
    row = np.zeros(dim, np.float64)
    a = np.asarray(active, np.float64)
    row[8 * block:8 * block + 4] = a
    row[8 * block + 4:8 * block + 7] = _nested_mass(1.0 - float((a * a).sum()), mass_snap)
    return row


def bf16_adversarial(dim, n_background=40000, n_adv=3, seed=1):
    """Rows and queries on which the bf16 scan ranks N_DECOYS decoys above the K_ADV true neighbours of each adversarial
    query, by nearly the whole error bound.

    Query b has 0.5 on the four active coordinates of its own block of 8 (unit norm, bf16-exact: dq = 0).  For the first
    n_adv queries:
      T_j (j < 10): active coordinates G + 0.45 U -- each rounds DOWN to G, the scan score loses 0.9 U = 1.76e-3 -- and
                    coordinate 0 raised by (10 - j) * 0.003 U, which orders the true cosines without crossing a rounding midpoint;
      D_j (j < 600): two active coordinates G + 0.55 U (round UP), two G + 0.34 U (round down; one lowered by j * 1e-6):
                    true cosine below every T, scan score G * 2 + U above every T.
    Background rows: two active coordinates of a random block, anywhere in [0.06, 0.47] (cosine <= 0.5 with every query),
    residual below T's.
    Adversarial rows are dealt out evenly over the whole index, so every tile and chunk holds decoys.
    -> dict(x [N, dim] float32, q [nq, dim] float32, true_ids [n_adv, 10] best first, decoy_ids [n_adv, 600], background_ids)."""
    nq = dim // 8
    assert 1 <= n_adv <= nq
    rng = np.random.default_rng(seed * 7919 + dim)
    q = np.zeros((nq, dim), np.float32)
    for b in range(nq):
        q[b, 8 * b:8 * b + 4] = 0.5
    adv = []                                              # (query, kind, j, row)
    for b in range(n_adv):
        for j in range(K_ADV):
            a = np.full(4, G + 0.45 * U)
            a[0] += (K_ADV - j) * 0.003 * U
            adv.append((b, 0, j, _sparse_row(dim, b, a)))
        for j in range(N_DECOYS):
            a = np.array([G + 0.55 * U, G + 0.55 * U, G + 0.34 * U, G + 0.34 * U - j * 1e-6])
            adv.append((b, 1, j, _sparse_row(dim, b, a)))
    order = rng.permutation(len(adv))
    n = n_background + len(adv)
    adv_pos = (np.arange(len(adv), dtype=np.int64) * n) // len(adv)        # evenly spaced, strictly increasing
    x = np.zeros((n, dim), np.float32)
    is_adv = np.zeros(n, bool)
    is_adv[adv_pos] = True
    true_ids = np.zeros((n_adv, K_ADV), np.int64)
    decoy_ids = np.zeros((n_adv, N_DECOYS), np.int64)
    for slot, i in enumerate(order):
        b, kind, j, row = adv[i]
        x[adv_pos[slot]] = row
        (decoy_ids if kind else true_ids)[b, j] = adv_pos[slot]
    bg = np.nonzero(~is_adv)[0]
    blocks = rng.integers(0, nq, bg.size)
    pairs = rng.integers(0, 4, (bg.size, 2))
    pairs[:, 1] = (pairs[:, 0] + 1 + pairs[:, 1] % 3) % 4                   # two distinct active coordinates
    # values all over [0.06, 0.47], each a bf16 grid point + up to 0.4 ulp: cosines spread over [0.06, 0.47] (a crowd inside
    # one error band would overflow the collect pass, which is another matter), residuals below those of T
    grid = RD.bf16_to_f32(RD.bf16_round(rng.uniform(0.06, 0.46, (bg.size, 2)).astype(np.float32))).astype(np.float64)
    vals = grid + rng.uniform(-0.4, 0.4, (bg.size, 2)) * 2.0 ** (np.floor(np.log2(grid)) - 7)
    for i, r in enumerate(bg):
        a = np.zeros(4)
        a[pairs[i]] = vals[i]
        x[r] = _sparse_row(dim, blocks[i], a)
    return {"x": x, "q": q, "true_ids": true_ids, "decoy_ids": decoy_ids, "background_ids": bg, "n_adv": n_adv}


# ------------------------------------------------------------------------------ int8 builder
I8_DIM = 256
I8_PIN_SXI = 641      # a row with a single 1.0 needs 1 / 127 = 640 S0: * 1.000001, rounded up


def _three_squares(t):
    """integers a >= b >= c >= 0 with a^2 + b^2 + c^2 == t (t is not of the form 4^a (8 b + 7)), else the nearest below"""
    for target in range(t, max(t - 8, 0), -1):
        a = int(np.sqrt(target))
        while a * a * 3 >= target:
            r = target - a * a
            b = int(np.sqrt(r))
            while b >= 0 and b * b * 2 >= r:
                c = int(round(np.sqrt(r - b * b)))
                if c * c == r - b * b and b <= a:
                    return a, b, c
                b -= 1
            a -= 1
    raise AssertionError(t)


def _i8_row(block, active_units, s):
    """unit-norm row on the grid of scale s: `active_units` (reals, in units of s) on the block's active coordinates, the rest
    of the norm on three coordinates that are whole multiples of s (so only the active coordinates carry rounding error)"""
    row = np.zeros(I8_DIM, np.float64)
    a = np.asarray(active_units, np.float64) * s
    row[8 * block:8 * block + 4] = a
    t = (1.0 - float((a * a).sum())) / (s * s)
    row[8 * block + 4:8 * block + 7] = np.array(_three_squares(int(round(t))), np.float64) * s
    return row


def i8_query(block, s0):
    """Unit query: v on the block's four active coordinates, one larger coordinate w (8 block + 7, where every row is zero)
    that fixes the query scale s_q so that w / s_q is almost a whole number and v / s_q has a fractional part of ~0.45: the
    query's own rounding then deflates the estimate as the rows' rounding does."""
    best = None
    for m in range(int(0.46 / (127.0 * s0)) + 1, 520):         # w > v needs w > 1 / sqrt(5): w sets the scale
        w = 127.0 * s0 * (m - 0.01)
        if w >= 0.95:
            break
        v = np.sqrt((1.0 - w * w) / 4.0)
        frac = (v / (m * s0)) % 1.0
        if best is None or abs(frac - 0.45) < best[0]:
            best = (abs(frac - 0.45), v, w)
        if abs(frac - 0.45) < 0.02:
            break                                            # the smallest w that does: v stays large
    _, v, w = best
    qv = np.zeros(I8_DIM, np.float64)
    qv[8 * block:8 * block + 4] = v
    qv[8 * block + 7] = w
    return qv.astype(np.float32)


def i8_adversarial(n_rows=4096 + 200, n_adv=3, seed=2):
    """dim 256.  Every 256-row tile holds one pin row (a single 1.0 on the last coordinate), which fixes the tile scale at
    sxi = 641, s = 641 S0 = 7.9e-3.  T_j: active coordinates (55.42 + dj) s, rounded DOWN to 55 s; D_j: two at 55.55 s
    (up to 56), two near 55.28 s (down): true cosine below T, int8 estimate 222 against 220 units.  Background: two active
    coordinates near 55 s.  Every row is sparse, so its residual (0.84 s = 6.6e-3) stays below "i8_max_resid"."""
    s0 = RD.i8_scale_unit(I8_DIM)
    s = I8_PIN_SXI * s0
    nq = I8_DIM // 8 - 1                                  # the last block holds the pin coordinate
    rng = np.random.default_rng(seed)
    q0 = i8_query(0, s0)
    q = np.stack([np.roll(q0, 8 * b) for b in range(nq)])
    x = np.zeros((n_rows, I8_DIM), np.float32)
    pins = np.arange(3, n_rows, 256)
    x[pins, I8_DIM - 1] = 1.0
    free = np.setdiff1d(np.arange(n_rows), pins)
    adv = []
    for b in range(n_adv):
        for j in range(K_ADV):
            a = np.full(4, 55.42)
            a[0] += (K_ADV - j) * 0.004
            adv.append((b, 0, j, _i8_row(b, a, s)))
        for j in range(N_DECOYS):
            adv.append((b, 1, j, _i8_row(b, [55.55, 55.55, 55.28, 55.28 - j * 2e-4], s)))
    assert len(adv) < free.size
    slots = free[(np.arange(len(adv), dtype=np.int64) * free.size) // len(adv)]
    order = rng.permutation(len(adv))
    true_ids = np.zeros((n_adv, K_ADV), np.int64)
    decoy_ids = np.zeros((n_adv, N_DECOYS), np.int64)
    for slot, i in enumerate(order):
        b, kind, j, row = adv[i]
        x[slots[slot]] = row
        (decoy_ids if kind else true_ids)[b, j] = slots[slot]
    bg = np.setdiff1d(free, slots)
    blocks = rng.integers(0, nq, bg.size)
    for i, r in enumerate(bg):
        a = np.zeros(4)
        c = rng.integers(0, 4)
        a[[c, (c + 1 + rng.integers(0, 3)) % 4]] = 55.0 + rng.uniform(-0.4, 0.4, 2)
        x[r] = _i8_row(blocks[i], a, s)
    return {"x": x, "q": q, "true_ids": true_ids, "decoy_ids": decoy_ids, "background_ids": bg, "pin_ids": pins, "n_adv": n_adv}
