"""The properties of oracle/scan.py can fail: a plain NumPy emulation of the bf16 scan's filter (fp32 scores, candidate lists,
bound table, both table bounds; no schedule -- the chunks simply take turns, tile by tile) passes P1 .. P5, and each seeded
fault of the kind the kernels could have fails at least one of them.  No GPU; tests/test_scan_stages_gpu.py applies the same
properties to what a real launch left behind."""
import numpy as np
import pytest

from oracle import rounding as RD
from oracle import scan as SC

CU = 256              # the plan of a 256-CU part
DIM = 64


def _normalise(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def emulate(x, q, k, fault=None, rescore_k=0):
    """One launch on normalised float32 rows x and queries q -> oracle.scan.Launch (with .s32, the emulation's own scores)."""
    n, K = x.shape
    B = q.shape[0]
    L = SC.expected_plan(n, B, k, CU, rescore_k)
    nt, nc, kp, trig = L["n_tiles"], L["n_chunks"], L["kp"], L["trig"]
    xb = np.zeros((nt * SC.TILE, K), np.uint16)
    xb[:n] = RD.bf16_round(x)
    qb = RD.bf16_round(q)
    S, delta = SC.scores(xb[:n], qb)
    slack = SC.slack_of(RD.bf16_residual(q).astype(np.float32), np.float32(RD.bf16_residual(x).max()), K)
    used_slack = slack
    if fault == "slack_eps":                                   # eps where 2 eps belongs
        eps = RD.scan_eps(RD.bf16_residual(q).astype(np.float32), np.float32(RD.bf16_residual(x).max()), K)
        used_slack = (eps * np.float32(1.000001) + np.float32(1e-6)).astype(np.float32)
    xf = RD.bf16_to_f32(xb).copy()
    if fault == "stale_piece":                                 # rows 8 .. 15 of tile 3, one 64-wide K step: still the piece of tile 2
        xf[3 * 256 + 8:3 * 256 + 16, 0:64] = xf[2 * 256 + 8:2 * 256 + 16, 0:64]
    s32 = xf @ RD.bf16_to_f32(qb).T                            # float32 accumulation
    bounds_on = L["gshift"] >= 0 or L["gshift_k"] >= 0
    table = np.zeros((L["b_pad"] // 64, 1, 64, 64), np.uint32)
    lists = [[np.zeros(0, np.uint64) for _ in range(B)] for _ in range(nc)]
    thr_s = np.full((nc, B), -np.inf, np.float32)
    thr_key = np.zeros((nc, B), np.uint64)
    cmax = np.zeros((nc, B), np.uint32)
    qs = np.arange(B)

    def publish(c, o):
        col = ((c + 1) if fault == "col_shift" else c) % 64
        cur = table[qs // 64, 0, col, qs % 64]
        table[qs // 64, 0, col, qs % 64] = np.maximum(cur, o)

    def compact(c, b):
        keys = np.sort(lists[c][b])[::-1]
        T = keys[kp - 1]
        lists[c][b] = keys[:kp].copy()
        if T > thr_key[c, b]:
            thr_key[c, b] = T
            thr_s[c, b] = SC.unpack_key(np.array([T]))[0][0]

    entries = [[*range(*SC.chunk_tile_range(nt, nc, c))] for c in range(nc)]
    for c in range(nc):
        entries[c] = [("boot", entries[c][0])] + [("tile", t) for t in entries[c][1:]] + [("tile", entries[c][0])]
    for e in range(max(len(v) for v in entries)):
        for c in range(nc):
            if e >= len(entries[c]):
                continue
            mode, t = entries[c][e]
            r0 = t * SC.TILE
            sc = s32[r0:r0 + SC.TILE]
            valid = np.arange(r0, r0 + SC.TILE) < n
            if mode == "boot":
                v = np.where(valid[:, None] | (fault == "pad_fold"), sc, -np.inf).max(axis=0) + np.float32(0.0)
                cmax[c] = np.maximum(cmax[c], SC.f32_orderable(v))
                publish(c, cmax[c])
                continue
            if bounds_on:
                cols = np.ascontiguousarray(table[:, 0].transpose(0, 2, 1)).reshape(-1, 64)[:B]
                b_kp, b_k = SC.table_bounds(cols, L["gshift"], L["gshift_k"], L["k_rows"], used_slack)
                best = np.maximum(b_kp, b_k).astype(np.float32)
                up = (SC.f32_orderable(best).astype(np.uint64) << np.uint64(32)) > thr_key[c]
                up &= best > -np.inf
                thr_key[c] = np.where(up, SC.f32_orderable(best).astype(np.uint64) << np.uint64(32), thr_key[c])
                thr_s[c] = np.where(up, best, thr_s[c])
            if fault == "pad_key":
                valid = np.ones(SC.TILE, bool)
            for b in range(B):
                m = (sc[:, b] >= thr_s[c, b]) & valid
                rows_in = r0 + np.nonzero(m)[0]
                if fault == "drop_row" and b == 0:
                    rows_in = rows_in[rows_in != DROPPED_ROW]
                if rows_in.size == 0:
                    continue
                keys = SC.pack_key(s32[rows_in, b], rows_in)
                lists[c][b] = np.concatenate([lists[c][b], keys])
                o = np.uint32(keys.max() >> np.uint64(32))
                if o > cmax[c, b]:
                    cmax[c, b] = o
                    col = ((c + 1) if fault == "col_shift" else c) % 64
                    table[b // 64, 0, col, b % 64] = max(table[b // 64, 0, col, b % 64], o)
                if lists[c][b].size >= trig:
                    compact(c, b)
    out = np.zeros((nc, L["b_pad"], SC.CAND_CAP), np.uint64)
    counts = np.zeros((nc, L["b_pad"]), np.int32)
    for c in range(nc):
        for b in range(B):
            if lists[c][b].size > kp:
                compact(c, b)
            counts[c, b] = lists[c][b].size
            out[c, b, :counts[c, b]] = lists[c][b]
    st = SC.Launch(L, out, counts, table, S, delta, slack)
    st.s32 = s32[:n]
    return st


DROPPED_ROW = 4000


def gauss_case(n=64 * 256 + 1, B=6, seed=0):
    """Gaussian rows; query 0 is row DROPPED_ROW plus noise, query 1 is near the single row of the last, partial tile."""
    rng = np.random.default_rng(seed)
    x = _normalise(rng.standard_normal((n, DIM)))
    q = rng.standard_normal((B, DIM))
    q[0] = x[DROPPED_ROW] + 0.02 * q[0]
    q[1] = x[n - 1] + 0.02 * q[1]
    q[2] = x[3 * 256 + 9] + 0.02 * q[2]                          # a row of the piece that "stale_piece" corrupts
    return x, _normalise(q)


def negative_case(n=64 * 256 + 1, B=4, seed=1):
    """rows that share a positive component, queries minus their mean direction: every real score is negative"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, DIM))
    x[:, 0] = np.abs(x[:, 0]) + 4.0
    x = _normalise(x)
    q = -x.mean(axis=0)[None, :] + 0.01 * rng.standard_normal((B, DIM))
    return x, _normalise(q)


def slack_case(seed=2):
    """k = 1: the k-row bound is the best score anywhere, L ~ 1 for query 0 (= row 5, first tile of chunk 0, published by the BOOT
    fold before any tile is filtered).  Twenty rows elsewhere sit 0.75 slack below it: above L - 2 eps, below L - eps."""
    rng = np.random.default_rng(seed)
    n = 64 * 256 + 1
    x = _normalise(rng.standard_normal((n, DIM)))
    q = _normalise(np.concatenate([x[5:6], rng.standard_normal((2, DIM))]))
    slack = float(SC.slack_of(RD.bf16_residual(q).astype(np.float32), np.float32(RD.bf16_residual(x).max()), DIM)[0])
    cos = 1.0 - 0.75 * slack
    near = 256 * np.arange(10, 30) + 100
    for r in near:
        o = rng.standard_normal(DIM)
        o -= (o @ x[5]) * x[5]
        x[r] = cos * x[5] + np.sqrt(1 - cos * cos) * o / np.linalg.norm(o)
    return _normalise(x), q, near


def check_all(st):
    return SC.check_first_pass(st)


# ------------------------------------------------------------------------------ the emulation passes
@pytest.fixture(scope="module")
def gauss():
    return gauss_case()


@pytest.fixture(scope="module")
def negative():
    return negative_case()


def test_helpers_round_trip():
    f = np.array([-np.inf, -1.5, -0.0, 0.0, 1e-30, 0.25, np.inf], np.float32)
    o = SC.f32_orderable(f)
    assert np.array_equal(SC.f32_from_orderable(o).view(np.uint32), f.view(np.uint32))
    assert (np.diff(o[[0, 1, 3, 4, 5, 6]].astype(np.int64)) > 0).all() and o.min() > 0
    key = SC.pack_key(np.array([0.5, 0.5, -0.25], np.float32), np.array([7, 3, 0]))
    sc, row, _ = SC.unpack_key(key)
    assert sc.tolist() == [0.5, 0.5, -0.25] and row.tolist() == [7, 3, 0]
    assert key[1] > key[0] > key[2]                              # higher score first, then the LOWER row
    assert [SC.chunk_tile_range(274, 256, c) for c in (0, 17, 18, 255)] == [(0, 2), (34, 36), (36, 37), (273, 274)]
    assert SC.chunk_row_starts(65, 65)[-1] == 65 * 256
    p = SC.expected_plan(70001, 100, 10, 256)
    assert (p["bn"], p["n_tiles"], p["n_chunks"], p["kp"], p["gshift"], p["gshift_k"], p["k_rows"], p["trig"]) == (128, 274, 256, 64, 0, 2, 10, 128)
    p = SC.expected_plan(70001, 300, 64, 256)
    assert (p["bn"], p["n_chunks"], p["kp"], p["gshift"], p["gshift_k"], p["k_rows"]) == (256, 128, 128, -1, 0, 0)
    p = SC.expected_plan(64 * 256, 300, 100, 256, rescore_k=256)
    assert (p["n_chunks"], p["n_tiles"], p["kp"], p["trig"], p["gshift"], p["gshift_k"]) == (64, 64, 256, 256, -1, -1)


def test_table_bounds_by_hand():
    cols = SC.f32_orderable(np.linspace(0.1, 0.73, 64, dtype=np.float32))[None, :]
    slack = np.array([0.01], np.float32)
    b_kp, b_k = SC.table_bounds(cols, 0, 2, 0, slack)
    assert b_kp[0] == np.float32(0.1) and b_k[0] == np.float32(np.float32(0.13) - np.float32(0.01))   # min of the quad maxima = column 3
    _, b_k3 = SC.table_bounds(cols, 0, 2, 3, slack)
    assert b_k3[0] == np.float32(np.linspace(0.1, 0.73, 64, dtype=np.float32)[55] - np.float32(0.01))   # third largest quad maximum
    cols[0, 9] = 0                                              # one column unpublished: no kp-row bound, quads still publish
    b_kp, b_k = SC.table_bounds(cols, 0, 2, 0, slack)
    assert b_kp[0] == -np.inf and b_k[0] > 0


@pytest.mark.parametrize("k", [10, 1, 40])
def test_emulation_passes(gauss, k):
    st = emulate(*gauss, k)
    assert st.bounds_on and st.L["n_chunks"] == 65
    out = check_all(st)
    assert out["p2"] <= 1.0 and out["keys"] > 0
    assert (st.counts[:, :6].sum(axis=0) < st.L["rows"] // 4).all(), "the bounds dropped most rows"


def test_emulation_passes_on_negative_scores(negative):
    st = emulate(*negative, 10)
    assert st.S.max() < 0
    check_all(st)


def test_emulation_passes_with_bounds_off(gauss):
    x, q = gauss
    st = emulate(x[:2 * 256 + 17], q, 100, rescore_k=256)
    assert not st.bounds_on and st.L["kp"] == 256 and st.L["n_chunks"] == 3
    out = check_all(st)
    assert out["keys"] == (2 * 256 + 17) * 6                     # every row of every chunk is in its list: P2 saw every score


# ------------------------------------------------------------------------------ each seeded fault fails a property
def test_stale_operand_piece_fails(gauss):
    x, q = gauss
    st = emulate(x[:8 * 256], q, 100, fault="stale_piece", rescore_k=256)      # every score is in a list: P2 sees it
    with pytest.raises(AssertionError, match="P2"):
        check_all(st)
    with pytest.raises(AssertionError, match="P2|P3|P4"):                       # and behind the bounds: a wrong BOOT maximum, key or drop
        check_all(emulate(x, q, 10, fault="stale_piece"))


def test_dropped_row_fails(gauss):
    with pytest.raises(AssertionError, match="P4"):
        check_all(emulate(*gauss, 10, fault="drop_row"))


def test_pad_row_as_key_fails(negative):
    with pytest.raises(AssertionError, match="P1 key names a row past the end"):
        check_all(emulate(*negative, 10, fault="pad_key"))


def test_pad_row_folded_into_the_table_fails(negative):
    st = emulate(*negative, 10, fault="pad_fold")
    SC.check_lists(st)
    SC.check_scores(st)
    with pytest.raises(AssertionError, match="P3 column above"):
        SC.check_table(st)


def test_row_id_off_by_16_fails(gauss):
    st = emulate(*gauss, 10)
    c, b = 7, 3
    sc, row, _ = SC.unpack_key(st.lists[c, b, :1])
    st.lists[c, b, :1] = SC.pack_key(sc, row + 16 if (row[0] % 256) < 240 else row - 16)
    with pytest.raises(AssertionError, match="P2"):
        check_all(st)


def test_duplicated_key_fails(gauss):
    st = emulate(*gauss, 10)
    c = int(np.argmax((st.counts[:, 4] > 0) & (st.counts[:, 4] < st.L["kp"])))
    n = st.counts[c, 4]
    assert 0 < n < st.L["kp"]
    st.lists[c, 4, n] = st.lists[c, 4, 0]
    st.counts[c, 4] = n + 1
    with pytest.raises(AssertionError, match="P1 a row twice"):
        check_all(st)


def test_column_credited_to_the_next_chunk_fails(gauss):
    st = emulate(*gauss, 10, fault="col_shift")
    SC.check_lists(st)
    SC.check_scores(st)
    with pytest.raises(AssertionError, match="P3"):
        SC.check_table(st)


def test_slack_of_one_eps_fails():
    x, q, near = slack_case()
    good = emulate(x, q, 1)
    assert good.L["k_rows"] == 1 and good.L["gshift_k"] == 2
    check_all(good)
    kept = SC.unpack_key(good.lists[10:30, 0, :64][np.arange(64)[None, :] < good.counts[10:30, 0, None]])[1]
    assert np.isin(near, kept).all(), "the rows between L - 2 eps and L - eps belong in the lists"
    with pytest.raises(AssertionError, match="P4"):
        check_all(emulate(x, q, 1, fault="slack_eps"))


def _emulate_collect(x, q, k, skip_partial_tile):
    n, K = x.shape
    B = q.shape[0]
    L = SC.expected_plan(n, B, k, CU, k)
    xb, qb = RD.bf16_round(x), RD.bf16_round(q)
    S, delta = SC.scores(xb, qb)
    s32 = RD.bf16_to_f32(xb) @ RD.bf16_to_f32(qb).T
    eps = RD.scan_eps(RD.bf16_residual(q).astype(np.float32), np.float32(RD.bf16_residual(x).max()), K)
    thr = (np.sort(s32, axis=0)[-k] - eps).astype(np.float32)
    thr[1::2] = np.inf                                          # every other query certified
    unc = np.nonzero(thr != np.inf)[0].astype(np.int32)
    keys = np.zeros((unc.size, SC.EXACT_CAP), np.uint64)
    counts = np.zeros(B, np.int32)
    last_full = n // 256 * 256
    for i, b in enumerate(unc):
        rows = np.nonzero(s32[:, b] >= thr[b])[0]
        if skip_partial_tile:
            rows = rows[rows < last_full]
        counts[i] = rows.size
        keys[i, :rows.size] = SC.pack_key(s32[rows, b], rows)
    return L, thr, unc, counts, keys, S, delta


def test_collect_emulation_passes_and_a_lost_partial_tile_fails(gauss):
    x, q = gauss
    x, q = x[:1000], q.copy()
    q[0] = x[995]                                               # its best row sits in the last, partial tile
    share, worst, over = SC.check_collect(*_emulate_collect(x, q, 10, False))
    assert over == 0 and worst <= 1.0
    with pytest.raises(AssertionError, match="P5 row at or above the threshold missing"):
        SC.check_collect(*_emulate_collect(x, q, 10, True))


def test_collect_rejects_unordered_ids_and_low_keys(gauss):
    x, q = gauss
    L, thr, unc, counts, keys, S, delta = _emulate_collect(x[:1000], q, 10, False)
    with pytest.raises(AssertionError, match="P5 unc_ids"):
        SC.check_collect(L, thr, unc[::-1], counts, keys, S, delta)
    low = int(np.argmin(S[:, 0]))
    keys[0, counts[0]:counts[0] + 1] = SC.pack_key(np.array([S[low, 0]], np.float32), np.array([low]))
    counts[0] += 1
    with pytest.raises(AssertionError, match="P5 key below the threshold"):
        SC.check_collect(L, thr, unc, counts, keys, S, delta)
