"""NumPy restatement of the stages around the int8 collect scan (csrc/select_i8.hip: i8_sample_select_kernel, select_i8_kernel;
csrc/quant.hip: i8_thresholds_kernel), as a CHECKER of one launch.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  The checker reads the launch's OWN buffers back (sqe_index_i8_read with the
option "i8_keep_select", sqe_index_state_read, the stored fp32 rows) and states, property by property, what each stage must have
made of them: integers where the kernels use integers, float64 elsewhere.  Nothing is recomputed from the caller's inputs, so a
property that fails names the stage that broke:

    threshold     thr_int from the sample (int8 form: m-th largest sample score, anchored on the sample's best true cosine unless
                  the key budget says otherwise; bf16 form: ceil(m-th true cosine / unit))
    thr_eff       thr_int * unit rounded UP, by no more than twice the formula's own slack
    sample        the k best sample rows, their fp32 cosines, order, padding
    select        what select_i8_kernel answered before the bf16 collect pass: from the sample, or a valid top-k of the gathered rows
    trace         keys gathered, rows estimated, rows re-scored, flags, against the lists and the counters
    certificate   certified exactly when thr_eff + eps8 < k-th cosine and nothing overflowed; else collect_thr, which is sound

unit = S0^2 * sqi with S0 = rounding.i8_scale_unit(dim) squared in float64.  eps8 / eps16 = rounding.scan_eps of the int8 / bf16
residuals.  The device contracts scan_eps's multiply-adds and NumPy does not, so every rule that depends on an eps is evaluated at
eps * (1 -+ 2^-22) -- two float32 ulps, derived from the three roundings of the expression, not measured -- and any value between
the two results is accepted.  An fp32 cosine is a 64-lane fmaf chain over unit vectors: within COS_TOL = 2e-6 of the float64 product
(include/sqe.h).

A failed property raises PropertyError (an AssertionError) whose message starts with the property's name.
"""
from __future__ import annotations

import numpy as np

from . import rounding as R

KEY_CAP = 12288          # select_i8.hip: keys a query holds in LDS
RS_CAP = 4096            # rows of a query that get a bf16 estimate
SS_TOP = 256             # i8_sample_select_kernel: sample values kept above the histogram cut
SS_CAP = 4096
BRACKET = 2.0 ** -22
COS_TOL = 2.0e-6
INT_MIN_THR, INT_MAX_THR = -0x7FFFFFFF, 0x7FFFFFFF
F_OVERFLOW, F_SAMPLE, F_CERTIFIED = 1, 2, 4

# what the checker reads (the values of semantic_query_engine_amd.engine's I8_* / STATE_*: include/sqe.h)
(I8_THRESHOLDS, I8_LIST_COUNTS, I8_LISTS, I8_SAMPLE_BEST, I8_POOL_COUNTS, I8_POOLS) = (3, 4, 5, 6, 7, 8)
(I8_THR_EFF, I8_SAMPLE_COS, I8_SAMPLE_IDS, I8_SELECT_COS, I8_SELECT_IDS, I8_SELECT_THR, I8_SELECT_TRACE) = range(10, 17)
(STATE_RESID_MAX, STATE_I8_RESID_MAX, STATE_QN, STATE_Q_RESID, STATE_Q8_RESID, STATE_Q8_SCALES) = range(1, 7)


class PropertyError(AssertionError):
    def __init__(self, prop, msg):
        super().__init__(f"{prop}: {msg}")
        self.prop = prop


def _need(cond, prop, msg):
    if not cond:
        raise PropertyError(prop, msg() if callable(msg) else msg)


# ------------------------------------------------------------------------------------------------ reading a launch
def read_launch(idx, L=None):
    """Every buffer the checker needs, read from `idx` (a VectorIndex after a search with "i8_keep_select", or a stand-in with the
    same i8_last / i8_read / state_read / ids / get_rows) -> dict."""
    L = dict(idx.i8_last()) if L is None else dict(L)
    B, bp, k, m, nc, dim = L["B"], L["b_pad"], L["k"], L["sample_m"], L["n_chunks"], L["dim"]
    cap, pcap = L["list_cap"], L["pool_cap"]
    d = dict(L=L)
    d["thr_int"] = idx.i8_read(I8_THRESHOLDS, np.int32, bp)
    d["thr_eff"] = idx.i8_read(I8_THR_EFF, np.float32, bp)
    d["sample_cos"] = idx.i8_read(I8_SAMPLE_COS, np.float32, B * m).reshape(B, m)
    d["sample_ids"] = idx.i8_read(I8_SAMPLE_IDS, np.int64, B * m).reshape(B, m)
    d["sel_cos"] = idx.i8_read(I8_SELECT_COS, np.float32, B * k).reshape(B, k)
    d["sel_ids"] = idx.i8_read(I8_SELECT_IDS, np.int64, B * k).reshape(B, k)
    d["sel_thr"] = idx.i8_read(I8_SELECT_THR, np.float32, bp)
    d["trace"] = idx.i8_read(I8_SELECT_TRACE, np.int32, B * 4).reshape(B, 4)
    d["cnt"] = idx.i8_read(I8_LIST_COUNTS, np.int32, nc * bp).reshape(nc, bp)
    d["lists"] = idx.i8_read(I8_LISTS, np.uint64, nc * bp * cap).reshape(nc, bp, cap)
    d["pcnt"] = idx.i8_read(I8_POOL_COUNTS, np.int32, bp)
    d["pools"] = idx.i8_read(I8_POOLS, np.uint64, bp * pcap).reshape(bp, pcap)
    if L["sample_int8"]:
        ncs, bps = L["sample_chunks"], L["sample_b_pad"]
        d["sample_best"] = idx.i8_read(I8_SAMPLE_BEST, np.int32, ncs * bps * 32).reshape(ncs, bps, 16, 2)
    d["qn"] = idx.state_read(STATE_QN, np.float32, B * dim).reshape(B, dim)
    d["sqi"] = idx.state_read(STATE_Q8_SCALES, np.uint32, B)
    d["q8_resid"] = idx.state_read(STATE_Q8_RESID, np.float32, B)
    d["q_resid"] = idx.state_read(STATE_Q_RESID, np.float32, B)
    d["i8_resid_max"] = idx.state_read(STATE_I8_RESID_MAX, np.float32, 1)[0]
    d["resid_max"] = idx.state_read(STATE_RESID_MAX, np.float32, 1)[0]
    d["master"] = idx.get_rows(idx.ids())                  # the stored fp32 rows by POSITION
    return d


def true_cosines(master, qn, block=32768):
    """float64 [rows, B]: the exact product of the stored fp32 rows and the normalised fp32 queries."""
    q64 = np.ascontiguousarray(qn.astype(np.float64).T)
    out = np.empty((master.shape[0], qn.shape[0]), np.float64)
    for r0 in range(0, master.shape[0], block):
        out[r0:r0 + block] = master[r0:r0 + block].astype(np.float64) @ q64
    return out


def key_fields(keys):
    """uint64 keys -> (int64 score, int64 row): include/sqe.h SQE_I8_LISTS"""
    keys = np.asarray(keys, dtype=np.uint64)
    hi = (keys >> np.uint64(32)).astype(np.int64) ^ 0x80000000
    score = np.where(hi >= (1 << 31), hi - (1 << 32), hi)
    return score, (0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF)).astype(np.int64))


def gathered_rows(d, q):
    """Rows select_i8_kernel can gather for query q -- the first list_cap keys of each (chunk, query) list, the first pool_cap of
    the pool -- and the total it counts -> (rows int64, scores int64, total)."""
    L = d["L"]
    cap, pcap = L["list_cap"], L["pool_cap"]
    n = np.minimum(d["cnt"][:, q], cap)
    keys = [d["lists"][c, q, :n[c]] for c in np.nonzero(n > 0)[0]]
    pn = min(int(d["pcnt"][q]), pcap)
    if pn > 0:
        keys.append(d["pools"][q, :pn])
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    score, row = key_fields(keys)
    return row, score, int(n.sum()) + pn


def units(d):
    s0 = R.i8_scale_unit(d["L"]["dim"])
    return (s0 * s0) * d["sqi"].astype(np.float64)


def eps_brackets(d):
    """-> (eps8 [B], eps16 [B]) float32 as NumPy evaluates kernels.h's scan_eps; a rule takes them at eps * (1 -+ BRACKET)"""
    K = d["L"]["dim"]
    return (R.scan_eps(d["q8_resid"], d["i8_resid_max"], K).astype(np.float32),
            R.scan_eps(d["q_resid"], d["resid_max"], K).astype(np.float32))


def _clamp_int(v):
    return INT_MIN_THR if v < -2.0e9 else INT_MAX_THR if v > 2.0e9 else int(v)


# ------------------------------------------------------------------------------------------------ the threshold
def sample_keys(d, q):
    """Valid entries of the int8 sample of query q, ordered by score descending then row ascending -> (score, row) int64"""
    v = d["sample_best"][:, q].reshape(-1, 2).astype(np.int64)
    v = v[v[:, 1] >= 0][:SS_CAP]
    o = np.lexsort((v[:, 1], -v[:, 0]))
    return v[o, 0], v[o, 1]


def sample_cut_crowded(score, m):
    """i8_sample_select_kernel keeps at most SS_TOP values at or above its histogram cut (1,024 linear bins over the scores present,
    the cut where min(m + 8, SS_TOP) values lie at or above).  True when more than SS_TOP qualify: it then kept an arbitrary SS_TOP
    of them, and only `thr_int <= rule` can be asked."""
    if score.size == 0:
        return False
    smin, rng = int(score.min()), int(score.max()) - int(score.min()) + 1
    bins = ((score - smin) * 1024) // rng
    want = min(m + 8, SS_TOP)
    if score.size < want:
        return False                                         # no bin reaches `want`: the cut stays at bin 0, everything is kept
    cut = np.sort(bins)[::-1][want - 1]
    return int((bins >= cut).sum()) > SS_TOP


def threshold_rule_int8(score, m, k, c0, eps8, unit, margin, step, key_budget):
    """-> (set of accepted thr_int, t, anchored values) for one query.  score: the ordered sample scores."""
    count = score.size
    if count == 0:
        return {INT_MIN_THR}, INT_MIN_THR, (INT_MIN_THR, INT_MIN_THR)
    t = int(score[min(m, count) - 1])
    ends = []
    for e in (float(eps8) * (1.0 + BRACKET), float(eps8) * (1.0 - BRACKET)):          # the larger eps gives the lower anchor
        v = np.floor((float(c0) - e * (1.0 + float(np.float32(margin)))) / unit) - 1.0
        ends.append(min(t, _clamp_int(v)))
    accepted = set()
    for ta in range(ends[0], ends[1] + 1):
        too_many = key_budget > 0 and ta < t and int((score >= ta).sum()) * step > key_budget
        accepted.add(t if too_many else ta)
    return accepted, t, (ends[0], ends[1])


def threshold_rule_bf16(tau, unit):
    if not tau > -np.inf:
        return INT_MIN_THR
    v = np.ceil(float(tau) / unit)
    return 0x7FFFFFFE if v > 2.0e9 else INT_MIN_THR if v < -2.0e9 else int(v)


def check_thresholds(d, opts, report):
    L = d["L"]
    B, bp, k, m, step = L["B"], L["b_pad"], L["k"], L["sample_m"], L["sample_step"]
    unit, (eps8, _) = units(d), eps_brackets(d)
    _need(np.all(d["thr_int"][B:] == INT_MAX_THR) and np.all(np.isposinf(d["thr_eff"][B:])), "threshold",
          "a padding query has a threshold other than 0x7fffffff / +inf")
    anchored = crowded = 0
    widest = 0
    for q in range(B):
        got = int(d["thr_int"][q])
        if L["sample_int8"]:
            score, _ = sample_keys(d, q)
            ok, t, (lo, hi) = threshold_rule_int8(score, m, k, d["sample_cos"][q, 0], eps8[q], unit[q], opts["margin"], step,
                                                  opts["key_budget"])
            widest = max(widest, hi - lo)
            if sample_cut_crowded(score, m):
                crowded += 1
                _need(got <= max(ok), "threshold", lambda: f"query {q}: thr_int {got} above the rule's {sorted(ok)} (more than {SS_TOP} "
                      "sample values at the cut: only <= is asked)")
            else:
                _need(got in ok, "threshold", lambda: f"query {q}: thr_int {got}, the rule gives {sorted(ok)} (m-th sample score {t}, "
                      f"anchor {lo}..{hi})")
                anchored += got < t                          # (counted where the m-th sample score is known: not behind a crowded cut)
        else:
            want = threshold_rule_bf16(d["sample_cos"][q, m - 1], unit[q])
            _need(got == want, "threshold", lambda: f"query {q}: thr_int {got}, ceil(tau / unit) = {want}")
    report.update(anchored=anchored, crowded_cuts=crowded, widest_bracket=max(widest, report.get("widest_bracket", 0)))


def check_thr_eff(d, report):
    B = d["L"]["B"]
    t = d["thr_int"][:B].astype(np.int64)
    live = np.abs(t) < 0x7FFFFFFE                                                    # saturated thresholds are left out
    exact = t.astype(np.float64) * units(d)                                          # (a 31-bit integer times a double: 1e-16 relative)
    got = d["thr_eff"][:B].astype(np.float64)
    bad = live & ~(got >= exact)
    _need(not bad.any(), "thr_eff", lambda: f"query {np.nonzero(bad)[0][0]}: thr_eff {float(got[bad][0])!r} lies BELOW thr_int * unit = "
          f"{float(exact[bad][0])!r} (by {(exact - got)[bad].max():.3e}; {int(bad.sum())} queries): an uncollected row may have an estimate above it")
    hi = exact + np.abs(exact) * 2.0e-6 + 2.0e-7
    bad = live & ~(got <= hi)
    _need(not bad.any(), "thr_eff", lambda: f"query {np.nonzero(bad)[0][0]}: thr_eff {float(got[bad][0])!r} is more than twice the formula's slack above "
          f"thr_int * unit = {float(exact[bad][0])!r}")
    report["thr_eff_checked"] = int(live.sum())


# ------------------------------------------------------------------------------------------------ sample cosines, select output
def _check_ranked(prop, q, cos, rows, cos64_q, what):
    """cosines non-increasing with ties to the lower row, each within COS_TOL of float64 -> worst |cos - float64|"""
    for i in range(len(rows) - 1):
        _need(cos[i] > cos[i + 1] or (cos[i] == cos[i + 1] and rows[i] < rows[i + 1]), prop,
              lambda: f"query {q}: {what} {i} and {i + 1} are out of order: ({cos[i]!r}, {rows[i]}) before ({cos[i + 1]!r}, {rows[i + 1]})")
    if len(rows) == 0:
        return 0.0
    err = np.abs(cos.astype(np.float64) - cos64_q[rows])
    _need(err.max() <= COS_TOL, prop, lambda: f"query {q}: {what} of row {rows[err.argmax()]} is {err.max():.3e} from the float64 product")
    return float(err.max())


def _check_topk_replay(prop, q, rows, cos64_q, pool_rows, want, what):
    """rows: a valid top-`want` of pool_rows by float64 cosine, to within COS_TOL"""
    _need(len(set(rows.tolist())) == len(rows), prop, lambda: f"query {q}: {what} repeat a row: {rows.tolist()}")
    _need(np.isin(rows, pool_rows).all(), prop, lambda: f"query {q}: {what} name rows outside the rows they were chosen from: "
          f"{rows[~np.isin(rows, pool_rows)].tolist()}")
    _need(len(rows) == want, prop, lambda: f"query {q}: {len(rows)} {what}, {want} expected")
    if want:
        kth = np.partition(cos64_q[pool_rows], -want)[-want]
        low = cos64_q[rows] < kth - COS_TOL
        _need(not low.any(), prop, lambda: f"query {q}: row {rows[low][0]} is among the {what} with cosine {cos64_q[rows][low][0]!r}, but the "
              f"{want}-th best of its candidates has {kth!r}: a better row was dropped")


def check_sample(d, cos64, report):
    L = d["L"]
    B, k, m, step, tr = L["B"], L["k"], L["sample_m"], L["sample_step"], L["tile_rows"]
    worst = 0.0
    if not L["sample_int8"]:
        tiles = (L["rows"] + tr - 1) // tr
        srows = (np.arange(0, tiles, step)[:, None] * tr + np.arange(tr)[None, :]).reshape(-1)
        srows = srows[srows < L["rows"]]
    for q in range(B):
        ids, cos = d["sample_ids"][q], d["sample_cos"][q]
        if L["sample_int8"]:
            score, row = sample_keys(d, q)
            kk = min(k, score.size)
            if not sample_cut_crowded(score, m):
                _need(set(ids[:kk].tolist()) == set(row[:kk].tolist()), "sample", lambda: f"query {q}: sample ids {sorted(ids[:kk].tolist())} "
                      f"are not the {kk} best sample keys {sorted(row[:kk].tolist())}")
            else:
                _need(np.isin(ids[:kk], row).all() and len(set(ids[:kk].tolist())) == kk, "sample", f"query {q}: sample ids outside the sample")
        else:
            kk = min(m, srows.size)
            _check_topk_replay("sample", q, ids[:kk], cos64[:, q], srows, kk, "sample rows")
        worst = max(worst, _check_ranked("sample", q, cos[:kk], ids[:kk], cos64[:, q], "sample cosine"))
        _need(np.all(np.isneginf(cos[kk:])) and np.all(ids[kk:] == -1), "sample", f"query {q}: the row past its {kk} entries is not (-inf, -1)")
    report["worst_cos_err"] = max(worst, report.get("worst_cos_err", 0.0))


def check_trace(d, report, stats=None):
    L = d["L"]
    B, k = L["B"], L["k"]
    tr = d["trace"]
    _need(not (tr[:, 3] & ~7).any(), "trace", "unknown flag bits")
    for q in range(B):
        N, R2, R3, fl = (int(v) for v in tr[q])
        _, _, total = gathered_rows(d, q)
        _need(N == min(total, KEY_CAP), "trace", lambda: f"query {q}: N = {N}, the lists and the pool hold {total} keys (cap {KEY_CAP})")
        if N >= k:
            _need(k <= R3 <= R2 <= min(N, RS_CAP), "trace", lambda: f"query {q}: k <= R3 <= R2 <= min(N, {RS_CAP}) fails: k {k}, R3 {R3}, R2 {R2}, N {N}")
        else:
            _need(R2 == N and R3 == N, "trace", lambda: f"query {q}: {N} keys, fewer than k, but R2 {R2}, R3 {R3}")
        hard = total > KEY_CAP or int(d["pcnt"][q]) > L["pool_cap"]
        over = bool(fl & F_OVERFLOW)
        _need(over or not hard, "trace", lambda: f"query {q}: {total} keys gathered, pool count {int(d['pcnt'][q])}: the overflow flag is missing")
        _need(hard or not over or R2 == RS_CAP, "trace", lambda: f"query {q}: overflow flag without an overflow (total {total}, pool "
              f"{int(d['pcnt'][q])}, R2 {R2})")
        _need(bool(fl & F_SAMPLE) == (R3 < k), "trace", lambda: f"query {q}: flag 2 (answered from the sample) is {bool(fl & F_SAMPLE)} with R3 = {R3}, k = {k}")
    unc = int(((tr[:, 3] & F_CERTIFIED) == 0).sum())
    if stats is not None:
        _need(int(tr[:, 0].sum()) == stats["i8_collected"], "trace", lambda: f"sum of N {int(tr[:, 0].sum())} != i8_collected {stats['i8_collected']}")
        _need(int(tr[:, 2].sum()) == stats["i8_rescored"], "trace", lambda: f"sum of R3 {int(tr[:, 2].sum())} != i8_rescored {stats['i8_rescored']}")
        _need(unc == stats["uncertified"], "trace", lambda: f"{unc} queries without flag 4, stats say {stats['uncertified']} uncertified")
    _need(unc == L["uncertified"], "trace", lambda: f"{unc} queries without flag 4, the launch record says {L['uncertified']} uncertified")
    report.update(uncertified=unc, from_sample=int(((tr[:, 3] & F_SAMPLE) != 0).sum()), overflow=int(((tr[:, 3] & F_OVERFLOW) != 0).sum()),
                  certified=B - unc, max_keys=int(tr[:, 0].max()) if B else 0, max_estimated=int(tr[:, 1].max()) if B else 0)


def check_select(d, cos64, opts, report, final=None):
    L = d["L"]
    B, k = L["B"], L["k"]
    base = int(opts.get("id_base", 0))
    worst = 0.0
    for q in range(B):
        fl = int(d["trace"][q, 3])
        cos, ids = d["sel_cos"][q], d["sel_ids"][q]
        if fl & F_SAMPLE:
            want_ids = np.where(d["sample_ids"][q, :k] >= 0, d["sample_ids"][q, :k] + base, -1)
            _need(np.array_equal(cos.view(np.uint32), d["sample_cos"][q, :k].view(np.uint32)) and np.array_equal(ids, want_ids), "select",
                  lambda: f"query {q}: answered from the sample, but the output is not the sample's first k entries: {ids.tolist()} / {want_ids.tolist()}")
        elif not fl & F_OVERFLOW:
            rows = ids - base
            crow, _, _ = gathered_rows(d, q)
            _need(rows.min() >= 0 and rows.max() < L["rows"], "select", lambda: f"query {q}: output ids {ids.tolist()} outside the index")
            _check_topk_replay("select", q, rows, cos64[:, q], crow, k, "returned rows")
            worst = max(worst, _check_ranked("select", q, cos, rows, cos64[:, q], "returned cosine"))
        if final is not None and fl & F_CERTIFIED:
            fcos, fids = final
            _need(np.array_equal(fcos[q].view(np.uint32), cos.view(np.uint32)) and np.array_equal(fids[q], ids if opts.get("final_ids") is None
                  else opts["final_ids"](ids)), "select", lambda: f"query {q} is certified, but the search returned something else than select_i8 wrote")
    report["worst_cos_err"] = max(worst, report.get("worst_cos_err", 0.0))


def check_certificate(d, cos64, report):
    L = d["L"]
    B, k = L["B"], L["k"]
    eps8, eps16 = eps_brackets(d)
    f32 = np.float32
    lo8, hi8 = (eps8.astype(np.float64) * (1.0 - BRACKET)).astype(f32), (eps8.astype(np.float64) * (1.0 + BRACKET)).astype(f32)
    lo16, hi16 = (eps16.astype(np.float64) * (1.0 - BRACKET)).astype(f32), (eps16.astype(np.float64) * (1.0 + BRACKET)).astype(f32)
    n_live = cos64.shape[0]
    for q in range(B):
        fl = int(d["trace"][q, 3])
        thr = d["sel_thr"][q]
        kth = d["sel_cos"][q, k - 1]
        cert = bool(fl & F_CERTIFIED)
        _need(cert == bool(np.isposinf(thr)), "certificate", lambda: f"query {q}: flag 4 is {cert}, collect_thr is {thr!r}")
        if cert:
            _need(not fl & (F_OVERFLOW | F_SAMPLE), "certificate", lambda: f"query {q}: certified with flags {fl} (an overflow or an answer from the sample)")
            _need(f32(d["thr_eff"][q] + lo8[q]) < kth, "certificate", lambda: f"query {q}: certified, but thr_eff + eps8 = {d['thr_eff'][q]!r} + {lo8[q]!r} "
                  f"is not below the k-th cosine {kth!r}")
            continue
        if not fl & (F_OVERFLOW | F_SAMPLE):
            _need(not f32(d["thr_eff"][q] + hi8[q]) < kth, "certificate", lambda: f"query {q}: thr_eff + eps8 = {d['thr_eff'][q]!r} + {hi8[q]!r} < "
                  f"k-th cosine {kth!r} and nothing overflowed, but the query is not certified")
        lb = max(kth if not fl & F_SAMPLE else f32(-np.inf), d["sample_cos"][q, k - 1])
        lb = lb if lb > -np.inf else f32(-1.0)
        _need(f32(lb - hi16[q]) <= thr <= f32(lb - lo16[q]), "certificate", lambda: f"query {q}: collect_thr {thr!r}, expected max(k-th found, k-th of "
              f"the sample) - eps16 = {lb!r} - {eps16[q]!r}")
        if n_live >= k:
            true_kth = np.partition(cos64[:, q], -k)[-k]
            _need(float(thr) + float(eps16[q]) * (1.0 - BRACKET) <= true_kth + COS_TOL, "certificate", lambda: f"query {q}: collect_thr + eps16 = "
                  f"{float(thr) + float(eps16[q])!r} is above the true k-th cosine {true_kth!r}: the bf16 pass could miss a top-k row")


def check_launch(idx, opts, final=None, stats=None, L=None):
    """The full checker on the last int8 search of `idx`.  opts: margin, key_budget (the index options the rule needs), id_base,
    final_ids (optional: maps select_i8's ids to what the search returns, for an index with deletes).  final: (cos, ids) the search
    returned.  stats: Context.stats() after that search.  -> report dict (shares and worst errors for the notes)."""
    d = read_launch(idx, L)
    report = dict(B=d["L"]["B"])
    cos64 = true_cosines(d["master"], d["qn"])
    check_thresholds(d, opts, report)
    check_thr_eff(d, report)
    check_sample(d, cos64, report)
    check_trace(d, report, stats)
    check_select(d, cos64, opts, report, final)
    check_certificate(d, cos64, report)
    report["data"], report["cos64"] = d, cos64
    return report


def check_final(report, final, to_position=None):
    """The search's final answer is a valid exact top-k of ALL live rows (replay form: 47 % of the clustered queries have their k-th
    and (k+1)-th cosines within 4e-6 of each other).  to_position: maps returned ids to row positions."""
    d, cos64 = report["data"], report["cos64"]
    k = d["L"]["k"]
    allrows = np.arange(cos64.shape[0])
    worst = 0.0
    for q in range(d["L"]["B"]):
        rows = final[1][q] if to_position is None else to_position(final[1][q])
        _check_topk_replay("final", q, rows, cos64[:, q], allrows, min(k, allrows.size), "final rows")
        worst = max(worst, _check_ranked("final", q, final[0][q], rows, cos64[:, q], "final cosine"))
    return worst


def summary(report):
    """the figures of a report (no buffers), for a log line"""
    return {key: (float(f"{v:.3e}") if isinstance(v, float) else int(v)) for key, v in report.items() if key not in ("data", "cos64")}
