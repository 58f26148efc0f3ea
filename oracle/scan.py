"""float64 restatement of what ONE launch of the bf16 scan with the fused top-k filter leaves behind
(csrc/scan.hip, scan_pp.hip, scan_common.h), and of its collect pass.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  The scan keeps per (chunk, query) a candidate list and folds chunk
maxima into a small bound table; a row is dropped against a threshold that mixes the list's own kp-th key with two bounds
read from that table.  Everything here is stated on the FINAL state (lists, counts, table), so it holds for any schedule:
thresholds only rise, hence the final table bounds every threshold the kernel used.

    S     = Xb . Qb^T in float64 from the bf16 copies the kernel read
    delta = 1.05 * K * 2^-24 * (|Xb| . |Qb|^T)        one fp32 accumulation chain (half of kernels.h: scan_eps's term)

P1 .. P5 (check_lists, check_scores, check_table, check_drops, check_collect) raise AssertionError; each returns the
figures a test records.  "Within delta" always means the pair's own delta.
"""
from __future__ import annotations

import numpy as np

from oracle import rounding as RD

TILE = 256            # kernels.h: SCAN_BM
COLS = 64             # kernels.h: GMAX_COLS
CAND_CAP = 512
EXACT_CAP = 4096
MAX_KP = 256
UNDECIDED_CAP = 0.005


# ------------------------------------------------------------------------------ keys
def f32_orderable(f) -> np.ndarray:
    """common.h f32_orderable: float32 -> uint32 whose unsigned order is the float order."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def f32_from_orderable(o) -> np.ndarray:
    o = np.ascontiguousarray(o, dtype=np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)


def pack_key(score, row) -> np.ndarray:
    """common.h make_key: orderable(score) << 32 | (0xFFFFFFFF - row); the kernel packs score + 0.0f (no -0)."""
    s = np.asarray(score, dtype=np.float32) + np.float32(0.0)
    return (f32_orderable(s).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(row).astype(np.uint64))


def unpack_key(key):
    """-> (score float32, row int64, orderable uint32)"""
    key = np.asarray(key, dtype=np.uint64)
    o = (key >> np.uint64(32)).astype(np.uint32)
    row = (np.uint64(0xFFFFFFFF) - (key & np.uint64(0xFFFFFFFF))).astype(np.int64)
    return f32_from_orderable(o), row, o


# ------------------------------------------------------------------------------ the plan
def chunk_tile_range(n_tiles: int, n_chunks: int, c: int):
    """scan_common.h chunk_tile_range: tiles dealt out evenly, the first n_tiles % n_chunks chunks one longer."""
    base, rem = divmod(n_tiles, n_chunks)
    begin = c * base + min(c, rem)
    return begin, begin + base + (1 if c < rem else 0)


def chunk_row_starts(n_tiles: int, n_chunks: int) -> np.ndarray:
    """first row of each chunk, then n_tiles * 256: int64 [n_chunks + 1] (not clipped to the row count)."""
    return np.array([chunk_tile_range(n_tiles, n_chunks, c)[0] for c in range(n_chunks)] + [n_tiles], np.int64) * TILE


def auto_kp(k: int, rescore_k: int = 0) -> int:
    """search.hip auto_kp with the certificate on."""
    if rescore_k > 0:
        return min(MAX_KP, max(rescore_k, k))
    return 64 if k <= 32 else 128 if k <= 128 else k


def expected_plan(rows: int, B: int, k: int, cu_count: int, rescore_k: int = 0) -> dict:
    """scan.hip make_scan_plan + make_kernel_args (first pass, certificate on) for a batch of <= 1024 queries."""
    kp = auto_kp(k, rescore_k)
    bn = 256 if B > 128 else 128 if B > 64 else 64
    qblocks = (B + bn - 1) // bn
    n_tiles = (rows + TILE - 1) // TILE
    chunks = max(1, cu_count // qblocks)
    if chunks > n_tiles:
        chunks = max(n_tiles, 1)
    gshift = 2 if kp <= 16 else 1 if kp <= 32 else 0 if kp <= 64 else -1
    gshift_k = 2 if k <= 16 else 1 if k <= 32 else 0 if k <= 64 else -1
    if gshift_k <= gshift:
        gshift_k = -1
    k_rows = k if (gshift_k == 2 and k <= 16) else 0
    if chunks < COLS:
        gshift, gshift_k, k_rows = -1, -1, 0
    return {"rows": rows, "B": B, "k": k, "kp": kp, "bn": bn, "qblocks": qblocks, "b_pad": qblocks * bn, "n_tiles": n_tiles,
            "n_chunks": chunks, "tiles_per_chunk": (n_tiles + chunks - 1) // chunks if n_tiles else 0, "ngroups": 1,
            "trig": min(CAND_CAP - TILE, max(2 * kp, 128)), "gshift": gshift, "gshift_k": gshift_k, "k_rows": k_rows,
            "list_cap": CAND_CAP, "exact_cap": EXACT_CAP}


# ------------------------------------------------------------------------------ scores
def scores(xb: np.ndarray, qb: np.ndarray, block: int = 8192):
    """bf16 bit patterns xb [rows, K], qb [B, K] -> (S, delta) float64 [rows, B], in row blocks."""
    q = RD.bf16_to_f32(qb).astype(np.float64)
    K = q.shape[1]
    S = np.empty((xb.shape[0], q.shape[0]), np.float64)
    D = np.empty_like(S)
    qa, c = np.abs(q).T.copy(), 1.05 * K * 2.0 ** -24
    qt = q.T.copy()
    for r0 in range(0, xb.shape[0], block):
        x = RD.bf16_to_f32(xb[r0:r0 + block]).astype(np.float64)
        S[r0:r0 + block] = x @ qt
        D[r0:r0 + block] = c * (np.abs(x) @ qa)
    return S, D


def slack_of(q_resid, db_resid_max, K: int) -> np.ndarray:
    """scan_common.h filter_init: 2 eps * 1.000001 + 1e-6 in float32, from the measured residuals."""
    eps = RD.scan_eps(q_resid, db_resid_max, K)
    return (np.float32(2.0) * eps * np.float32(1.000001) + np.float32(1.0e-6)).astype(np.float32)


def table_bounds(cols: np.ndarray, gshift: int, gshift_k: int, k_rows: int, slack: np.ndarray):
    """scan_common.h refresh_apply on final table rows.  cols: uint32 [B, 64] (query, column), slack float32 [B].
    -> (kp-row bound, k-row bound minus slack) as float64 [B], -inf where a bound is off or a column it needs is unpublished."""
    cols = np.asarray(cols, dtype=np.uint32)
    B = cols.shape[0]
    b_kp = np.full(B, -np.inf)
    b_k = np.full(B, -np.inf)
    if gshift >= 0:
        o = cols.reshape(B, COLS >> gshift, 1 << gshift).max(axis=2).min(axis=1)
        b_kp = np.where(o != 0, f32_from_orderable(o).astype(np.float64), -np.inf)
    if gshift_k >= 0:
        gm = cols.reshape(B, COLS >> gshift_k, 1 << gshift_k).max(axis=2)
        if k_rows > 0:
            assert gshift_k == 2
            lk = -np.sort(-gm.astype(np.int64), axis=1)[:, k_rows - 1].astype(np.uint32)      # the k-th LARGEST quad maximum
        else:
            lk = gm.min(axis=1)
        lowered = (f32_from_orderable(lk) - np.asarray(slack, np.float32)).astype(np.float32)
        b_k = np.where(lk != 0, lowered.astype(np.float64), -np.inf)
    return b_kp, b_k


# ------------------------------------------------------------------------------ the state of one launch
class Launch:
    """What a launch left: L (sqe_index_scan_last / expected_plan keys), lists uint64 [n_chunks, b_pad, cap], counts int32
    [n_chunks, b_pad], table uint32 [b_pad / 64, ngroups, 64, 64] or None, and the reference S, delta [rows, B], slack [B]."""

    def __init__(self, L, lists, counts, table, S, delta, slack):
        self.L, self.lists, self.counts, self.table, self.S, self.delta, self.slack = L, lists, counts, table, S, delta, slack
        self.starts = chunk_row_starts(L["n_tiles"], L["n_chunks"])
        self.bounds_on = L["gshift"] >= 0 or L["gshift_k"] >= 0

    def live(self):
        """-> (chunk, query, score f32, row, orderable) of every key of the live queries' lists (counts clipped to kp)."""
        L = self.L
        kp, B = L["kp"], L["B"]
        cnt = np.clip(self.counts[:, :B], 0, kp)
        m = np.arange(kp)[None, None, :] < cnt[:, :, None]
        c, q, _ = np.nonzero(m)
        sc, row, o = unpack_key(self.lists[:, :B, :kp][m])
        return c, q, sc, row, o

    def table_cols(self) -> np.ndarray:
        """uint32 [B, 64]: the columns of each live query"""
        B = self.L["B"]
        t = self.table[:, 0]                                   # [slices, column, query in slice]
        return np.ascontiguousarray(t.transpose(0, 2, 1)).reshape(-1, COLS)[:B]


def check_lists(st: Launch):
    """P1: keys name valid rows of their chunk, once each; counts <= kp and the first `count` slots hold keys; padding queries
    hold nothing.  -> number of keys."""
    L = st.L
    B, kp, rows = L["B"], L["kp"], L["rows"]
    assert st.counts.min() >= 0 and st.counts.max() <= kp, ("P1 count outside [0, kp]", int(st.counts.min()), int(st.counts.max()))
    assert not st.counts[:, B:].any(), "P1 a padding query holds keys"
    if st.table is not None:
        t = st.table.transpose(0, 3, 1, 2).reshape(L["b_pad"], -1)
        assert not t[B:].any(), "P1 a padding query published a bound"
    c, q, sc, row, o = st.live()
    raw = st.lists[:, :B, :kp][np.arange(kp)[None, None, :] < st.counts[:, :B, None]]
    assert (raw != 0).all(), "P1 an empty slot below the count"
    assert (row < rows).all(), ("P1 key names a row past the end", int(row.max()), rows)
    lo, hi = st.starts[c], st.starts[c + 1]
    bad = (row < lo) | (row >= hi)
    assert not bad.any(), ("P1 key outside its chunk's tiles", int(c[bad][0]), int(q[bad][0]), int(row[bad][0]))
    ident = (c.astype(np.int64) * B + q) * (1 << 32) + row
    assert np.unique(ident).size == ident.size, "P1 a row twice in one list"
    return ident.size


def check_scores(st: Launch):
    """P2: every key's score within delta of S[row, q].  -> (max |s - S| / delta, keys)."""
    c, q, sc, row, o = st.live()
    if sc.size == 0:
        return 0.0, 0
    ratio = np.abs(sc.astype(np.float64) - st.S[row, q]) / st.delta[row, q]
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1.0, ("P2 key score off", float(ratio[i]), "chunk", int(c[i]), "query", int(q[i]), "row", int(row[i]),
                             float(sc[i]), float(st.S[row[i], q[i]]))
    return float(ratio[i]), sc.size


def _chunk_reduce(a: np.ndarray, starts: np.ndarray, rows: int) -> np.ndarray:
    """max over the (valid) rows of each chunk: [n_chunks, B]"""
    return np.maximum.reduceat(a[:rows], np.minimum(starts[:-1], rows - 1), axis=0)


def check_table(st: Launch):
    """P3: every column at most the best S + delta of the chunks that share it, at least every key of their final lists
    (as orderable integers) and at least the best S - delta of their FIRST tiles.  -> max (column - max S) / (max (S + delta) - max S)."""
    L = st.L
    if not st.bounds_on:
        return None
    B, rows, nc = L["B"], L["rows"], L["n_chunks"]
    assert st.starts[-2] < rows, "every chunk holds a valid row"
    cols = st.table_cols()                                     # [B, 64]
    tab = np.where(cols != 0, f32_from_orderable(cols).astype(np.float64), -np.inf)
    col_of = np.arange(nc) % COLS

    def fold(per_chunk, init):
        out = np.full((COLS, B), init, per_chunk.dtype)
        np.maximum.at(out, col_of, per_chunk)
        return out.T                                           # [B, 64]
    hi = fold(_chunk_reduce(st.S + st.delta, st.starts, rows), -np.inf)
    mx = fold(_chunk_reduce(st.S, st.starts, rows), -np.inf)
    over = tab > hi
    assert not over.any(), ("P3 column above every row it covers", np.argwhere(over)[0].tolist(), float(tab[over][0]), float(hi[over][0]))
    c, q, sc, row, o = st.live()
    best = np.zeros((nc, B), np.uint32)
    np.maximum.at(best, (c, q), o)
    keymax = fold(best, np.uint32(0))
    under = cols < keymax
    assert not under.any(), ("P3 column below a key of its chunks", np.argwhere(under)[0].tolist())
    first_lo = np.full((nc, B), -np.inf)
    low = st.S - st.delta
    for ch in range(nc):
        r0 = int(st.starts[ch])
        first_lo[ch] = low[r0:min(r0 + TILE, rows)].max(axis=0)
    boot = fold(first_lo, -np.inf)
    missed = tab < boot
    assert not missed.any(), ("P3 column below the first tile of a chunk (BOOT fold)", np.argwhere(missed)[0].tolist())
    return float(((tab - mx) / (hi - mx)).max())


def thresholds(st: Launch) -> np.ndarray:
    """T(c, q) of P4: float64 [n_chunks, B], the largest of (a) the list's lowest score when it is full, (b) the kp-row bound,
    (c) the k-row bound minus slack, the last two from the final table."""
    L = st.L
    B, kp, nc = L["B"], L["kp"], L["n_chunks"]
    c, q, sc, row, o = st.live()
    lowest = np.full((nc, B), np.inf)
    np.minimum.at(lowest, (c, q), sc.astype(np.float64))
    T = np.where(st.counts[:, :B] == kp, lowest, -np.inf)
    if st.bounds_on:
        b_kp, b_k = table_bounds(st.table_cols(), L["gshift"], L["gshift_k"], L["k_rows"], st.slack)
        T = np.maximum(T, np.maximum(b_kp, b_k)[None, :])
    return T


def table_share(st: Launch) -> float:
    """share of (chunk, query) whose T is a table term (b) or (c), not the list's own lowest score"""
    if not st.bounds_on:
        return 0.0
    L = st.L
    c, q, sc, row, o = st.live()
    lowest = np.full((L["n_chunks"], L["B"]), np.inf)
    np.minimum.at(lowest, (c, q), sc.astype(np.float64))
    own = np.where(st.counts[:, :L["B"]] == L["kp"], lowest, -np.inf)
    return float((thresholds(st) > own).mean())


def check_drops(st: Launch):
    """P4: a valid row that is not in its chunk's list has S <= T + delta.  -> (undecided share, pairs checked)."""
    L = st.L
    B, rows = L["B"], L["rows"]
    T = thresholds(st)
    c, q, sc, row, o = st.live()
    kept = np.zeros((rows, B), bool)
    kept[row, q] = True
    chunk_of = np.searchsorted(st.starts, np.arange(rows), side="right") - 1
    undecided, worst = 0, None
    for r0 in range(0, rows, 16384):
        sl = slice(r0, min(r0 + 16384, rows))
        Tr = T[chunk_of[sl]]
        lost = ~kept[sl] & (st.S[sl] > Tr + st.delta[sl])
        if lost.any() and worst is None:
            r, qq = np.argwhere(lost)[0]
            worst = ("P4 row lost without a reason", "row", int(r0 + r), "chunk", int(chunk_of[r0 + r]), "query", int(qq),
                     "S", float(st.S[r0 + r, qq]), "T", float(Tr[r, qq]), "lost pairs in block", int(lost.sum()))
        undecided += int((np.abs(st.S[sl] - Tr) < st.delta[sl]).sum())
    assert worst is None, worst
    share = undecided / float(rows * B)
    assert share <= UNDECIDED_CAP, ("P4 too many undecided pairs", share)
    return share, rows * B


def check_collect(L, thr, unc_ids, counts, keys, S, delta, key_ref=None):
    """P5.  thr float32 [B] (collect_thr), unc_ids int32 [u], counts int32 [>= u] and keys uint64 [u, exact_cap] by compact index.
    key_ref = (Sk, dk): what the key scores are compared with (the scan's S, delta by default; after a search the library has
    replaced them by fp32 cosines -- sqe.h -- and the caller passes that reference).
    -> (undecided share, max |s - Sk| / dk, queries over the cap)"""
    B, rows, cap = L["B"], L["rows"], L["exact_cap"]
    Sk, dk = key_ref if key_ref is not None else (S, delta)
    unc = np.nonzero(thr[:B] != np.inf)[0]
    assert np.array_equal(unc_ids, unc), ("P5 unc_ids is not the ascending list of the uncertified queries", unc_ids[:8], unc[:8])
    undecided, worst, over = 0, 0.0, 0
    for i, q in enumerate(unc.tolist()):
        n = int(counts[i])
        assert n >= 0
        if n > cap:
            over += 1
            continue
        sc, row, o = unpack_key(keys[i, :n])
        assert (keys[i, :n] != 0).all() and (row < rows).all(), ("P5 key outside the index", q)
        assert np.unique(row).size == n, ("P5 a row twice among the keys", q)
        got = np.zeros(rows, bool)
        got[row] = True
        t = float(thr[q])
        must = S[:, q] >= t + delta[:, q]
        assert got[must].all(), ("P5 row at or above the threshold missing", "query", q, "rows", np.nonzero(must & ~got)[0][:8].tolist())
        assert not (S[row, q] < t - delta[row, q]).any(), ("P5 key below the threshold", q)
        if n:
            worst = max(worst, float((np.abs(sc.astype(np.float64) - Sk[row, q]) / dk[row, q]).max()))
        undecided += int((np.abs(S[:, q] - t) < delta[:, q]).sum())
    assert worst <= 1.0, ("P5 key score off", worst)
    share = undecided / float(max(1, unc.size) * rows)
    assert share <= UNDECIDED_CAP, ("P5 too many undecided pairs", share)
    return share, worst, over


def check_first_pass(st: Launch) -> dict:
    """P1 .. P4 on one launch -> the recorded figures"""
    keys = check_lists(st)
    p2, _ = check_scores(st)
    p3 = check_table(st)
    und, pairs = check_drops(st)
    return {"keys": keys, "p2": p2, "p3": p3, "undecided": und, "pairs": pairs, "table_decides": table_share(st)}
