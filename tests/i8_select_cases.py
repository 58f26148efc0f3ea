"""Cases for the stage tests of the int8 search (oracle/i8_select.py is the checker; tests/test_i8_select_cpu.py and
tests/test_i8_select_gpu.py use what is here).

FakeLaunch is a NumPy stand-in for the three kernels around the collect scan -- i8_sample_select_kernel (or, in the bf16 sample
form, i8_thresholds_kernel), the collect predicate, select_i8_kernel -- and the bf16 fallback, on small clustered operands.  It
answers i8_last / i8_read / state_read / ids / get_rows like a VectorIndex after a search with "i8_keep_select", so the checker runs
on it unchanged; `fault` makes ONE stage wrong the way a wrong kernel would be.  The data builders below are the GPU cases."""
import numpy as np

from oracle import i8_select as S
from oracle import rounding as R

# ---------------------------------------------------------------------------------------------------------------- the stand-in
DIM, TILE_ROWS = 256, 256
ROWS = 8 * TILE_ROWS - 77                              # eight tiles, the last one partial (and never sampled)
B, B_PAD, SAMPLE_B_PAD = 8, 64, 256
N_CHUNKS, LIST_CAP, POOL_CAP = 3, 32, 256
SAMPLE_CHUNKS, STEP, M = 2, 1, 8
CLUSTERS = (800, 150, 150, 20, 20)                     # rows per centre; the rest is background
NOISE = (0.3, 0.05, 0.05, 0.15, 0.05)                  # spread of each crowd: wider than the int8 error (0), far inside it (1, 2, 4), about a bf16 eps (3)
STAGE1 = 64

FAULTS = {
    # fault: (configuration it is seeded in, property the checker must name)
    "m_plus_1": ("budget", "threshold"),
    "no_anchor": ("anchored", "threshold"),
    "budget_inverted": ("budget", "threshold"),
    "thr_eff_parent": ("anchored", "thr_eff"),
    "sample_unsorted": ("anchored", "sample"),
    "tie_higher_row": ("anchored", "select"),
    "one_eps_cut": ("anchored", "select"),
    "certified_pool_overflow": ("anchored", "certificate"),
    "certified_on_equality": ("equality", "certificate"),
    "thr_ignores_sample": ("anchored", "certificate"),
    "trace_counts_past_cap": ("anchored", "trace"),
    "snapshot_after_fallback": ("budget", "select"),
}
# configuration: k, sample depth m, anchor margin, key budget, int8 sample form
CONFIGS = {"anchored": (4, M, 0.25, 0, 1), "budget": (4, M, 0.25, 1, 1), "equality": (1, 1, 0.0, 0, 1), "bf16_sample": (4, M, 0.25, 0, 0)}


def _key(score, row):
    return (np.uint64((int(score) & 0xFFFFFFFF) ^ 0x80000000) << np.uint64(32)) | np.uint64(0xFFFFFFFF - int(row))


def _chunk_range(n_tiles, n_chunks, c):
    base, rem = divmod(n_tiles, n_chunks)
    begin = c * base + min(c, rem)
    return begin, begin + base + (1 if c < rem else 0)


def _ranked(cos, rows, higher_row_first=False):
    """order by (cosine descending, row ascending)"""
    return np.lexsort((-rows if higher_row_first else rows, -cos.astype(np.float64)))


class FakeLaunch:
    def __init__(self, config="anchored", fault=None):
        self.k, m, self.margin, self.key_budget, self.sample_int8 = CONFIGS[config]
        k = self.k
        f32 = np.float32
        rng = np.random.default_rng(11)
        # ---- operands: every row shares the direction u (so that a query along -u sees only negative cosines), clusters of
        # near-identical rows on top of it, background rows, one bit-identical pair; queries 0-3 aim at a centre, 4 at the pair, 5 at a
        # background row (a lone best row), 6 and 7 the other way
        u = rng.standard_normal(DIM)
        cen = rng.standard_normal((len(CLUSTERS), DIM))
        label = np.concatenate([np.full(n, c) for c, n in enumerate(CLUSTERS)] + [np.full(ROWS - sum(CLUSTERS), -1)])
        rng.shuffle(label)
        x = 2.0 * u + np.where(label[:, None] >= 0, cen[np.maximum(label, 0)] + np.asarray(NOISE)[np.maximum(label, 0), None] * rng.standard_normal((ROWS, DIM)),
                               rng.standard_normal((ROWS, DIM)))
        # the four rows nearest to query 0 are the last of its crowd in tile 6: sampled, but behind what fills the last chunk's list and
        # the pool, so select_i8 never sees them and the sample's k-th cosine is the better lower bound
        late = np.nonzero((label == 0) & (np.arange(ROWS) < 7 * TILE_ROWS))[0][-4:]
        x[late] = 2.0 * u + cen[0] + 0.05 * rng.standard_normal((4, DIM))
        pair = np.nonzero(label == 4)[0][:2]
        x[pair[1]] = x[pair[0]]
        q = np.stack([2.0 * u + cen[0], 2.0 * u + cen[1], 2.0 * u + cen[2], 2.0 * u + cen[3], x[pair[0]], x[np.nonzero(label == -1)[0][0]],
                      -2.0 * u - cen[0], -2.0 * u + rng.standard_normal(DIM)]) + 0.02 * rng.standard_normal((B, DIM))
        x, q = x.astype(f32), q.astype(f32)
        tiles = (ROWS + TILE_ROWS - 1) // TILE_ROWS
        xn = np.zeros((tiles * TILE_ROWS, DIM), f32)
        xn[:ROWS] = x / np.linalg.norm(x, axis=1, keepdims=True)
        qn = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
        self.master, self.qn = xn[:ROWS].copy(), qn
        scales = np.repeat(R.i8_tile_scales(xn, ROWS)[::TILE_ROWS], TILE_ROWS).astype(np.uint32)
        x8 = R.i8_quantize(xn, scales)
        sqi = R.i8_row_scales(qn)
        q8 = R.i8_quantize(qn, sqi)
        score = (x8.astype(np.int64) @ q8.astype(np.int64).T) * scales[:, None].astype(np.int64)        # [rows, B]
        cos64 = S.true_cosines(self.master, qn)
        cos32 = cos64.astype(f32)                                                    # an "fp32 re-score": within 6e-8 of float64
        q8_resid = (R.i8_residual(qn, q8, sqi) * 1.0001 + 1e-7).astype(f32)
        i8_resid_max = f32(R.i8_residual(xn[:ROWS], x8[:ROWS], scales[:ROWS]).max() * 1.0001 + 1e-7)
        q_resid = (R.bf16_residual(qn) * 1.0001 + 1e-7).astype(f32)
        resid_max = f32(R.bf16_residual(xn[:ROWS]).max() * 1.0001 + 1e-7)
        s0 = R.i8_scale_unit(DIM)
        unit = (s0 * s0) * sqi.astype(np.float64)
        eps8 = R.scan_eps(q8_resid, i8_resid_max, DIM).astype(f32)
        eps16 = R.scan_eps(q_resid, resid_max, DIM).astype(f32)
        eps16r = f32(R.scan_eps(f32(0), resid_max, DIM))
        # ---- threshold pass
        full_tiles = ROWS // TILE_ROWS
        sample_best = np.zeros((SAMPLE_CHUNKS, SAMPLE_B_PAD, 16, 2), np.int32)
        sample_best[..., 1] = -1
        sample_cos = np.full((B, m), -np.inf, f32)
        sample_ids = np.full((B, m), -1, np.int64)
        thr_int = np.full(B_PAD, 0x7FFFFFFF, np.int32)
        thr_eff = np.full(B_PAD, np.inf, f32)
        rr = np.arange(TILE_ROWS)
        lane_of, order_in_tile = (rr >> 7) * 4 + ((rr >> 2) & 3), ((rr >> 4) & 7) * 4 + (rr & 3)
        if self.sample_int8:
            for c in range(SAMPLE_CHUNKS):
                tb, te = _chunk_range(full_tiles // STEP, SAMPLE_CHUNKS, c)
                for lane in range(8):
                    rows_l = rr[lane_of == lane]
                    rows_l = rows_l[np.argsort(order_in_tile[rows_l], kind="stable")]
                    srow = (np.arange(tb, te)[:, None] * STEP * TILE_ROWS + rows_l[None, :]).reshape(-1)
                    o = np.argsort(-score[srow], axis=0, kind="stable")[:2]           # [2, B]
                    sample_best[c, :B, 2 * lane:2 * lane + 2, 0] = np.take_along_axis(score[srow], o, 0).T
                    sample_best[c, :B, 2 * lane:2 * lane + 2, 1] = srow[o].T
        for qi in range(B):
            if self.sample_int8:
                v = sample_best[:, qi].reshape(-1, 2).astype(np.int64)
                o = np.lexsort((v[:, 1], -v[:, 0]))
                sc, row = v[o, 0], v[o, 1]
                t = int(sc[min(m + (1 if fault == "m_plus_1" else 0), sc.size) - 1])
                top = row[:k]
                o = _ranked(cos32[top, qi], top)
                sample_cos[qi, :k], sample_ids[qi, :k] = cos32[top[o], qi], top[o]
                v = np.floor((float(sample_cos[qi, 0]) - float(eps8[qi]) * (1.0 + float(f32(self.margin)))) / unit[qi]) - 1.0
                ta = t if fault == "no_anchor" else min(t, S._clamp_int(v))
                too_many = self.key_budget > 0 and ta < t and int((sc >= ta).sum()) * STEP > self.key_budget
                if fault == "budget_inverted":
                    too_many = self.key_budget > 0 and ta < t and not too_many
                thr = t if too_many else ta
            else:
                srows = (np.arange(0, tiles, STEP)[:, None] * TILE_ROWS + rr[None, :]).reshape(-1)
                srows = srows[srows < ROWS]
                o = _ranked(cos32[srows, qi], srows)[:m]
                sample_cos[qi, :o.size], sample_ids[qi, :o.size] = cos32[srows[o], qi], srows[o]
                thr = S.threshold_rule_bf16(sample_cos[qi, m - 1], unit[qi])
            thr_int[qi] = thr
            tu = float(thr) * unit[qi]
            thr_eff[qi] = f32(tu * (1.0 + 1e-6) + 1e-7) if fault == "thr_eff_parent" else f32(tu + abs(tu) * 1e-6 + 1e-7)
        if fault == "sample_unsorted":
            sample_cos[0, [1, 2]], sample_ids[0, [1, 2]] = sample_cos[0, [2, 1]], sample_ids[0, [2, 1]]
        # ---- collect scan
        cnt = np.zeros((N_CHUNKS, B_PAD), np.int32)
        lists = np.zeros((N_CHUNKS, B_PAD, LIST_CAP), np.uint64)
        pcnt = np.zeros(B_PAD, np.int32)
        pools = np.zeros((B_PAD, POOL_CAP), np.uint64)
        for c in range(N_CHUNKS):
            t0, t1 = _chunk_range(tiles, N_CHUNKS, c)
            for r in range(t0 * TILE_ROWS, min(t1 * TILE_ROWS, ROWS)):
                for qi in np.nonzero(score[r] >= thr_int[:B])[0]:
                    if cnt[c, qi] < LIST_CAP:
                        lists[c, qi, cnt[c, qi]] = _key(score[r, qi], r)
                    else:
                        if pcnt[qi] < POOL_CAP:
                            pools[qi, pcnt[qi]] = _key(score[r, qi], r)
                        pcnt[qi] += 1
                    cnt[c, qi] += 1
        # ---- select
        sel_cos = np.full((B, k), -np.inf, f32)
        sel_ids = np.full((B, k), -1, np.int64)
        sel_thr = np.zeros(B_PAD, f32)
        trace = np.zeros((B, 4), np.int32)
        self.planted = {}
        for qi in range(B):
            keys = [lists[c, qi, :min(cnt[c, qi], LIST_CAP)] for c in range(N_CHUNKS)] + [pools[qi, :min(pcnt[qi], POOL_CAP)]]
            sc, row = S.key_fields(np.concatenate(keys))
            total = int(np.minimum(cnt[:, qi], LIST_CAP).sum() + min(pcnt[qi], POOL_CAP))
            overflow = pcnt[qi] > POOL_CAP or total > S.KEY_CAP
            N = min(total, S.KEY_CAP)
            # bf16 estimates: within eps16r of the cosine.  Query 3: the worst case the two-eps cut of stage 3 exists for -- the best row
            # estimated 0.9 eps low, every other row 0.9 eps high
            est = cos32[row, qi].astype(np.float64)
            if qi == 3 and N > k:
                best = np.argmax(cos64[row, qi])
                err = np.full(row.size, 0.9 * float(eps16r))
                err[best] = -0.9 * float(eps16r)
                est = est + err
            s1 = np.argsort(-sc, kind="stable")[:STAGE1]
            thr2 = -0x7FFFFFFF
            if s1.size >= k:
                t1 = np.sort(est[s1])[-k] - float(eps16r)
                thr2 = S._clamp_int(np.floor((t1 - float(eps8[qi])) / unit[qi]) - 1.0)
            in2 = sc >= thr2
            in2[s1] = True
            R2 = int(in2.sum())
            in3 = in2.copy()
            if R2 > k:
                cut = np.sort(est[in2])[-k] - (1.0 if fault == "one_eps_cut" else 2.0) * float(eps16r)
                in3 &= est >= cut
                if qi == 3:
                    self.planted["one_eps"] = bool(in3[best]) if N > k else None
            R3 = int(in3.sum())
            from_sample = R3 < k
            if from_sample:
                sel_cos[qi], sel_ids[qi] = sample_cos[qi, :k], sample_ids[qi, :k]
                kth = f32(-np.inf)
            else:
                r3 = row[in3]
                o = _ranked(cos32[r3, qi], r3, higher_row_first=(fault == "tie_higher_row"))[:k]
                sel_cos[qi], sel_ids[qi] = cos32[r3[o], qi], r3[o]
                kth = sel_cos[qi, k - 1]
            certified = (not overflow) and (not from_sample) and f32(thr_eff[qi] + eps8[qi]) < kth
            if qi == 0:
                self.planted["sample_above_found"] = bool(sample_cos[qi, k - 1] > kth) and not certified
            if config == "equality" and qi == 5:
                # the fp32 cosine of the best row lands exactly ON thr_eff + eps8 (a value within 2e-6 of its float64 product): not certified
                # (taken at the low end of the eps bracket, so that the checker's verdict does not hang on a rounding of the sum)
                edge = f32(thr_eff[qi] + f32(float(eps8[qi]) * (1.0 - S.BRACKET)))
                self.planted["equality"] = abs(float(edge) - cos64[sel_ids[qi, 0], qi]) < 1.5e-6 and not overflow and not from_sample
                sel_cos[qi, 0] = kth = edge
                certified = fault == "certified_on_equality"
            if fault == "certified_pool_overflow" and overflow and not from_sample:
                certified = True
            if certified:
                sel_thr[qi] = np.inf
            else:
                lb = kth if fault == "thr_ignores_sample" else max(kth, sample_cos[qi, k - 1])
                sel_thr[qi] = f32((lb if lb > -np.inf else f32(-1.0)) - eps16[qi])
            trace[qi] = (int(cnt[:, qi].sum()) if fault == "trace_counts_past_cap" else N, R2, R3,
                         (1 if overflow else 0) | (2 if from_sample else 0) | (4 if certified else 0))
        # ---- the bf16 collect pass answers the uncertified queries exactly
        fin_cos, fin_ids = sel_cos.copy(), sel_ids.copy()
        allrows = np.arange(ROWS)
        for qi in np.nonzero((trace[:, 3] & 4) == 0)[0]:
            o = _ranked(cos32[:, qi], allrows)[:k]
            fin_cos[qi], fin_ids[qi] = cos32[o, qi], o
        self.final = (fin_cos, fin_ids)
        if fault == "snapshot_after_fallback":
            sel_cos, sel_ids = fin_cos.copy(), fin_ids.copy()
        unc = int(((trace[:, 3] & 4) == 0).sum())
        self.stats = dict(i8_collected=int(trace[:, 0].sum()), i8_rescored=int(trace[:, 2].sum()), uncertified=unc)
        self.opts = dict(margin=self.margin, key_budget=self.key_budget, id_base=0)
        self.L = dict(rows=ROWS, tile_stride=TILE_ROWS * DIM, dim=DIM, B=B, b_pad=B_PAD, k=k, tile_rows=TILE_ROWS, q_pitch=DIM + 128,
                      query_block=64, n_chunks=N_CHUNKS, list_cap=LIST_CAP, sample_int8=self.sample_int8, sample_step=STEP,
                      sample_tiles=full_tiles // STEP, sample_chunks=SAMPLE_CHUNKS if self.sample_int8 else 0, sample_b_pad=SAMPLE_B_PAD,
                      sample_m=m, uncertified=unc, pool_cap=POOL_CAP, kernel=6)
        self.buf = {S.I8_THRESHOLDS: thr_int, S.I8_THR_EFF: thr_eff, S.I8_SAMPLE_COS: sample_cos, S.I8_SAMPLE_IDS: sample_ids,
                    S.I8_SELECT_COS: sel_cos, S.I8_SELECT_IDS: sel_ids, S.I8_SELECT_THR: sel_thr, S.I8_SELECT_TRACE: trace,
                    S.I8_LIST_COUNTS: cnt, S.I8_LISTS: lists, S.I8_POOL_COUNTS: pcnt, S.I8_POOLS: pools, S.I8_SAMPLE_BEST: sample_best}
        self.state_buf = {S.STATE_QN: qn, S.STATE_Q8_SCALES: sqi.astype(np.uint32), S.STATE_Q8_RESID: q8_resid, S.STATE_Q_RESID: q_resid,
                          S.STATE_I8_RESID_MAX: np.array([i8_resid_max], f32), S.STATE_RESID_MAX: np.array([resid_max], f32)}
        self.thr_int, self.unit, self.trace, self.pcnt = thr_int, unit, trace, pcnt

    def i8_last(self):
        return dict(self.L)

    @staticmethod
    def _read(src, dtype, count, offset_bytes):
        raw = np.ascontiguousarray(src).reshape(-1).view(np.uint8)
        nbytes = count * np.dtype(dtype).itemsize
        if offset_bytes < 0 or offset_bytes + nbytes > raw.size:
            raise ValueError("read past the buffer")
        return raw[offset_bytes:offset_bytes + nbytes].copy().view(dtype)

    def i8_read(self, what, dtype, count, offset_bytes=0):
        return self._read(self.buf[what], dtype, count, offset_bytes)

    def state_read(self, what, dtype, count, offset_bytes=0):
        return self._read(self.state_buf[what], dtype, count, offset_bytes)

    def ids(self):
        return np.arange(ROWS, dtype=np.int64)

    def get_rows(self, ids):
        return self.master[np.asarray(ids)]


# ---------------------------------------------------------------------------------------------------------------- GPU case data
def gaussian_case(n, dim, b, seed):
    """Gaussian rows, half of the queries planted on rows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((b, dim), dtype=np.float32)
    planted = rng.integers(0, n, (b + 1) // 2)
    q[:planted.size] = x[planted] + 0.1 * q[:planted.size]
    return x, q


def clustered_case(n=80000, dim=256, b=300, centres=40, noise=0.05, seed=23):
    """the data of tests/test_i8_gpu.py: test_clustered_rows_stay_exact"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((centres, dim)).astype(np.float32)
    x = (cen[rng.integers(0, centres, n)] + noise * rng.standard_normal((n, dim))).astype(np.float32)
    q = (cen[rng.integers(0, centres, b)] + noise * rng.standard_normal((b, dim))).astype(np.float32)
    return x, q


def opposite_case(n=60000, dim=256, b=100, seed=31):
    """rows u + g, queries -u + g: every cosine is negative, so is every threshold"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(dim).astype(np.float32)
    x = u + rng.standard_normal((n, dim), dtype=np.float32)
    q = -u + rng.standard_normal((b, dim), dtype=np.float32)
    return x, q


def crowd_case(n=120000, dim=512, crowd=4500, b=8, seed=37, shuffled=True):
    """`crowd` rows within 3e-3 of one centre among Gaussian rows (shuffled through them, or appended behind them as one block),
    b queries aimed at the centre -> (x, q, crowd row positions)"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal(dim).astype(np.float32)
    cen /= np.linalg.norm(cen)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    pos = np.sort(rng.choice(n, crowd, replace=False)) if shuffled else np.arange(n - crowd, n)
    x[pos] = cen + (3e-3 / np.sqrt(dim)) * rng.standard_normal((crowd, dim), dtype=np.float32)
    q = cen + (3e-3 / np.sqrt(dim)) * rng.standard_normal((b, dim), dtype=np.float32)
    return x, q.astype(np.float32), pos


def ties_case(n=40000, dim=256, copies=600, b=4, seed=41):
    """`copies` bit-identical rows spread over the index, one query on them.  The copied row carries one element large enough to set
    the scale of every tile it sits in, so all copies quantise alike and every int8 score of (copy, query) is the same number."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    row = rng.standard_normal(dim).astype(np.float32)
    row[7] = 6.5
    pos = np.sort(rng.choice(n, copies, replace=False))
    x[pos] = row
    q = rng.standard_normal((b, dim), dtype=np.float32)
    q[0] = row
    return x, q, pos
