"""oracle/select.py can fail, stage by stage: a NumPy emulation of the stages behind the bf16 scan (lists from a float64 product of
the bf16 copies, a bound table built to the scan's P3, the exact fp32 chain, the fp32 certificate, the tail) passes check_launch in
every configuration of tests/test_select_stages_gpu.py that fits a CPU, with its undecided share under the cap, and each seeded
fault fails at the stage that owns it.  Also the cross-check of the chain: oracle.c's fmaf chain against the NumPy round-to-odd form
and against a plain scalar loop.  No GPU."""
import numpy as np
import pytest

from oracle import rounding as RD
from oracle import scan as SC
from oracle import select as SL

CU = 256
f32 = np.float32


def _normalise(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _topk_keys(keys, k, id_base):
    keys = np.sort(keys)[::-1][:k]
    sc, row, _ = SC.unpack_key(keys)
    cos, ids = np.full(k, -np.inf, np.float32), np.full(k, -1, np.int64)
    cos[:keys.size], ids[:keys.size] = sc, row + id_base
    return cos, ids


def emulate(x, q, k, rescore_k=0, certify=True, fault=None, id_base=0, exact_cap=SC.EXACT_CAP, tweak=None):
    """One search on normalised float32 rows x and queries q -> (d, final, first): the dict oracle.select.read_launch would
    return, the final answer and select's own answer.  tweak(lists, counts, table): edits the first pass's buffers in place."""
    n, K = x.shape
    B = q.shape[0]
    L = SC.expected_plan(n, B, k, CU, rescore_k)
    kp, nc, bp = L["kp"], L["n_chunks"], L["b_pad"]
    L.update(dim=K, certified=int(certify), uncertified=0, list_cap=kp, exact_cap=exact_cap)
    xb, qb = RD.bf16_round(x), RD.bf16_round(q)
    s32 = (SC.scores(xb, qb)[0].astype(np.float32) + f32(0.0)) if n else np.zeros((0, B), np.float32)
    starts = SC.chunk_row_starts(L["n_tiles"], nc)
    lists = np.zeros((nc, bp, kp), np.uint64)
    counts = np.zeros((nc, bp), np.int32)
    table = np.zeros((bp // 64, 1, 64, 64), np.uint32)
    qs = np.arange(B)
    for c in range(nc):
        r0, r1 = int(starts[c]), int(min(starts[c + 1], n))
        if r1 <= r0:
            continue
        keys = -np.sort(-SC.pack_key(s32[r0:r1].T, np.arange(r0, r1)[None, :]).view(np.int64) ^ np.int64(-2 ** 63), axis=1)
        keys = (keys ^ np.int64(-2 ** 63)).view(np.uint64)[:, :kp]                         # unsigned descending sort
        lists[c, :B, :keys.shape[1]] = keys
        counts[c, :B] = keys.shape[1]
        top = (keys[:, 0] >> np.uint64(32)).astype(np.uint32)
        table[qs // 64, 0, c % 64, qs % 64] = np.maximum(table[qs // 64, 0, c % 64, qs % 64], top)
    if L["gshift"] >= 0:                                           # the filter: keys below the final kp-row bound were dropped
        cols = np.ascontiguousarray(table[:, 0].transpose(0, 2, 1)).reshape(-1, 64)[:B]
        b_kp, _ = SC.table_bounds(cols, L["gshift"], -1, 0, np.zeros(B, np.float32))
        sc = SC.unpack_key(lists[:, :B])[0].astype(np.float64)
        keep = (sc >= b_kp[None, :, None]) & (lists[:, :B] != 0)
        counts[:, :B] = keep.sum(axis=2)                           # lists are sorted: the kept keys are a prefix
    if tweak is not None:
        tweak(lists, counts, table)
    q_resid = RD.bf16_residual(q).astype(np.float32)
    resid_max = f32(RD.bf16_residual(x).max()) if n else f32(0)
    d = dict(L=L, lists=lists, counts=counts, table=table, qn=q, q_resid=q_resid, resid_max=resid_max, master=x)
    cos = np.full((B, k), -np.inf, np.float32)
    ids = np.full((B, k), -1, np.int64)
    thr = np.full(bp, np.inf, np.float32)
    cols = np.ascontiguousarray(table[:, 0].transpose(0, 2, 1)).reshape(-1, 64)
    for b in range(B):
        keys = np.sort(np.concatenate([lists[c, b, :min(counts[c, b], kp)] for c in range(nc)]))[::-1]
        place = kp - 1 if fault == "T_off" else kp
        T = keys[place - 1] if keys.size >= place else np.uint64(0)
        sel = keys[keys >= T]
        if fault == "below_T" and keys.size > kp:
            sel = np.concatenate([keys[:kp - 1], keys[kp:kp + 1]])
        _, rows, _ = SC.unpack_key(sel)
        m = rows.size
        sc = SL.chain_scores(x, rows, q[b], skip_last_vec=(fault == "skip_vec"))
        o = np.lexsort((-rows if fault == "ties_reversed" else rows, -sc.astype(np.float64)))[:k]
        cos[b, :o.size], ids[b, :o.size] = sc[o], rows[o] + id_base
        if not certify:
            continue
        kth = cos[b, k - 1] if m >= k else f32(-np.inf)
        gfin = f32(-np.inf)
        if L["gshift"] >= 0 and fault != "no_gfin":
            g = 0 if fault == "no_fold" else L["gshift"]
            v = cols[b].reshape(64 >> g, 1 << g).max(axis=1).min()
            if v != 0:
                gfin = SC.f32_from_orderable(np.array([v], np.uint32))[0]
        unseen = max(SC.unpack_key(np.array([T]))[0][0] if T else f32(-np.inf), gfin)
        if unseen > -np.inf:
            eps = f32(RD.scan_eps(q_resid[b], resid_max, K))
            if fault == "eps_half":
                eps = f32(eps * f32(0.5))
            if not (m >= k and kth > f32(unseen + eps)):
                thr[b] = f32(kth if m >= k else f32(-1.0)) if fault == "thr_no_eps" else f32((kth if m >= k else f32(-1.0)) - eps)
    first = (cos.copy(), ids.copy())
    if certify:
        unc = np.nonzero(thr[:B] != np.inf)[0].astype(np.int32)
        ccounts = np.zeros(B, np.int32)
        ckeys = np.zeros((unc.size, exact_cap), np.uint64)
        for i, b in enumerate(unc.tolist()):
            rows = np.nonzero(s32[:, b] >= thr[b])[0][::-1]        # (the collect scan appends in no particular order)
            ccounts[i] = rows.size
            rows = rows[:exact_cap]
            keys = SC.pack_key(SL.chain_scores(x, rows, q[b]), rows)
            ckeys[i, :rows.size] = keys
            over = ccounts[i] > exact_cap
            if (not over and fault != "keep_first") or (over and fault == "replace_over"):
                cos[b], ids[b] = _topk_keys(keys, k, id_base)
        L["uncertified"] = int(unc.size)
        d.update(thr=thr, unc_count=int(unc.size), unc_ids=unc[::-1].copy() if fault == "unsorted" else unc, ccounts=ccounts, ckeys=ckeys)
    return d, (cos, ids), first


def gauss(n, dim, B, seed=0, near=True):
    rng = np.random.default_rng(seed)
    x = _normalise(rng.standard_normal((n, dim)))
    q = rng.standard_normal((B, dim))
    if near and n:
        q[::3] = x[rng.integers(0, n, q[::3].shape[0])] + 0.3 * q[::3]
    return x, _normalise(q)


def passes(x, q, k, show="", **kw):
    d, final, _ = emulate(x, q, k, **kw)
    rep = SL.check_launch(d, final, kw.get("id_base", 0))
    print("SELECT_STAGES_CPU", show, SL.summary(rep))
    assert rep["first_failure"] is None and rep.get("undecided_share", 0.0) <= SL.UNDECIDED_CAP
    return rep


def fails(stage, x, q, k, **kw):
    with pytest.raises(SL.StageError) as e:
        d, final, _ = emulate(x, q, k, **kw)
        SL.check_launch(d, final, kw.get("id_base", 0))
    assert e.value.stage == stage, str(e.value)
    return str(e.value)


# ------------------------------------------------------------------------------ the chain
def _scalar_chain(x, q):
    """plain scalar loop: Python floats are doubles, so fmaf(a, b, c) is taken as round32(exact) with fractions"""
    from fractions import Fraction
    out = np.empty(x.shape[0], np.float32)
    for i, r in enumerate(x):
        lane = []
        for l in range(64):
            s = f32(0)
            for v in range(l, x.shape[1] // 4, 64):
                for c in range(4):
                    exact = Fraction(float(r[4 * v + c])) * Fraction(float(q[4 * v + c])) + Fraction(float(s))
                    s = _round_f32(exact)
            lane.append(s)
        for off in (32, 16, 8, 4, 2, 1):
            lane = [f32(lane[l] + lane[l ^ off]) for l in range(64)]
        out[i] = lane[0] + f32(0.0)
    return out


def _round_f32(fr):
    """a Fraction -> the nearest float32, ties to even (through the two neighbouring float32 values of its double)"""
    a = f32(float(fr))                                             # double rounding may be off by one float32 ulp: repair
    from fractions import Fraction
    cand = [a, np.nextafter(a, f32(np.inf)), np.nextafter(a, f32(-np.inf))]
    best = min(cand, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.array(c, np.float32).view(np.uint32)) & 1))
    return f32(best)


@pytest.mark.parametrize("dim", [64, 128, 192, 256, 320, 1024])
def test_chain_c_against_numpy(dim):
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((300, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    x[100:200, dim // 2:] = x[100:200, :dim // 2]                  # cancelling: the second half undoes the first
    qc = q.copy()
    qc[dim // 2:] = -qc[:dim // 2]
    x[200:] *= (10.0 ** rng.uniform(-6, 6, (100, dim))).astype(np.float32)     # wide exponent range: sums that lose bits
    for qq in (q, qc):
        a, b = SL.chain_scores(x, None, qq), SL.chain_scores_numpy(x, qq)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        rows = np.array([5, 299, 0, 150])
        assert np.array_equal(SL.chain_scores(x, rows, qq).view(np.uint32), a[rows].view(np.uint32))
    assert np.abs(SL.chain_scores(x[100:200], None, qc)).max() < 1e-3 * np.abs(SL.chain_scores(x[100:200], None, q)).max() + 1e-3


@pytest.mark.parametrize("dim", [64, 320])
def test_chain_against_a_scalar_loop(dim):
    rng = np.random.default_rng(7 + dim)
    x = rng.standard_normal((6, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    x[3:, dim // 2:] = x[3:, :dim // 2]
    q2 = q.copy()
    q2[dim // 2:] = -q2[:dim // 2]
    for qq in (q, q2):
        assert np.array_equal(SL.chain_scores(x, None, qq).view(np.uint32), _scalar_chain(x, qq).view(np.uint32))
    assert not np.array_equal(SL.chain_scores(x, None, q).view(np.uint32), SL.chain_scores(x, None, q, skip_last_vec=True).view(np.uint32))


def test_fmaf_round_to_odd_on_double_rounding_cases():
    """a * b + c whose float64 sum lands exactly half way between two float32 values: plain float64 arithmetic rounds twice"""
    a = np.array([1 + 2.0 ** -12], np.float32)
    b = np.array([1 + 2.0 ** -12], np.float32)                     # a * b = 1 + 2^-11 + 2^-24
    c = np.array([2.0 ** -60], np.float32)
    got = SL._fmaf(a, b, c)[0]
    assert got == f32(1 + 2.0 ** -11 + 2.0 ** -23)                 # above the tie: up; (float32)(a * b + c in double) gives 1 + 2^-11
    assert f32(np.float64(a[0]) * np.float64(b[0]) + np.float64(c[0])) == f32(1 + 2.0 ** -11)
    assert SL._fmaf(a, b, -c)[0] == f32(1 + 2.0 ** -11)


# ------------------------------------------------------------------------------ the certificate by hand
def test_certificate_reference_by_hand():
    cols = SC.f32_orderable(np.linspace(0.10, 0.73, 64, dtype=np.float32))
    lin = np.linspace(0.10, 0.73, 64, dtype=np.float32)
    assert SL.gfin_of(cols, 0) == lin[0] and SL.gfin_of(cols, 1) == lin[1] and SL.gfin_of(cols, 2) == lin[3] and SL.gfin_of(cols, -1) == -np.inf
    holed = cols.copy()
    holed[8:12] = 0                                                # one whole quad unpublished: no bound
    assert SL.gfin_of(holed, 2) == -np.inf and SL.gfin_of(holed[::-1].copy(), 0) == -np.inf
    eps = SL.eps64(f32(1e-3), f32(1.5e-3), 64)
    assert abs(eps - ((1 + 1e-3) * 1.5e-3 + 1e-3 + 2e-4)) < 1e-8   # the accumulation term is floored at 2e-4 below dim 1598
    assert SL.eps64(f32(0), f32(0), 8192) == pytest.approx(8192 * 1.1920929e-7 * 1.05, rel=1e-6)
    T = SC.pack_key(np.array([0.5], np.float32), np.array([7]))[0]
    args = dict(cols=cols, q_resid=f32(1e-3), resid_max=f32(1.5e-3), K=64, k=10)
    c = SL.certificate_reference(T, 0.5 + 2 * eps, 64, gshift=-1, **args)
    assert c["certified"] is True and c["by"] == "T" and c["unseen"] == 0.5
    c = SL.certificate_reference(T, 0.5 + 0.5 * eps, 64, gshift=-1, **args)
    assert c["certified"] is False and c["thr"] == pytest.approx(0.5 - 0.5 * eps, abs=1e-12)
    c = SL.certificate_reference(T, 0.5 + eps + 2.0 ** -23, 64, gshift=-1, **args)
    assert c["certified"] is None                                  # inside the band
    c = SL.certificate_reference(T, 0.9, 64, gshift=2, **args)     # gfin = 0.13 < score(T)
    assert c["by"] == "T" and c["gfin"] == lin[3]
    c = SL.certificate_reference(np.uint64(0), 0.12, 12, gshift=2, **args)
    assert c["by"] == "gfin" and c["certified"] is False           # 0.12 < 0.13 + eps
    c = SL.certificate_reference(np.uint64(0), -np.inf, 5, gshift=2, **args)
    assert c["certified"] is False and c["thr"] == -1.0 - eps      # m < k under a bound
    c = SL.certificate_reference(np.uint64(0), -np.inf, 5, gshift=-1, **args)
    assert c["certified"] is True and c["by"] == "none"            # nothing cut, no bound: certified whatever m is


# ------------------------------------------------------------------------------ the emulation passes
def test_forms_and_key_routes():
    x, q = gauss(16385, 64, 5)
    rep = passes(x[:16384], q, 10, "small 64x64")
    assert (rep["form"], rep["n_chunks"], rep["kp"], rep["gshift"]) == ("small", 64, 64, 0)
    rep = passes(x[:4096], q, 100, "small 16x256", rescore_k=256)
    assert (rep["form"], rep["n_chunks"], rep["kp"], rep["n_keys_max"]) == ("small", 16, 256, 4096)
    rep = passes(x, q, 10, "large 65x64")
    assert (rep["form"], rep["n_chunks"], rep["route_lds"]) == ("large", 65, 5)
    xg, qg = gauss(70001, 128, 3, seed=1)
    rep = passes(xg, qg, 100, "large global", rescore_k=256)
    assert (rep["form"], rep["route_global"]) == ("large", 3)
    assert rep["n_keys_min"] == rep["n_keys_max"] == 255 * 256 + (70001 - 273 * 256)    # bounds off: every list is full, the last chunk has 113 rows
    rep = passes(xg[:10000], qg, 100, "large lds", rescore_k=256)
    assert (rep["form"], rep["route_lds"], rep["n_keys_max"]) == ("large", 3, 10000)


@pytest.mark.parametrize("B", [1, 64, 65, 300, 600, 1024])
def test_batch_sizes(B):
    x, q = gauss(16385, 64, B, seed=B)
    rep = passes(x, q, 10, f"B={B}")
    assert rep["n_chunks"] == (65 if B <= 768 else 64) and rep["certified"] + rep["uncertified"] == B


@pytest.mark.parametrize("dim", [64, 192, 256, 320, 1024])
def test_rescore_dims(dim):
    x, q = gauss(2000 + dim % 7, dim, 9, seed=dim)
    rep = passes(x, q, 10, f"dim={dim}", rescore_k=50)             # m = 50: no multiple of 4 or 64
    assert rep["kp"] == 50 and rep["m_lt_kp"] == 0


@pytest.mark.parametrize("n", [1, 3, 37, 9])
def test_tiny_indexes(n):
    x, q = gauss(n, 64, 5, seed=n, near=False)
    rep = passes(x, q, 10, f"n={n}")
    assert rep["m_lt_kp"] == 5 and rep["m_lt_k"] == (5 if n < 10 else 0)
    assert rep["no_unseen"] == 5 and rep["certified"] == 5        # nothing was cut and no bound was used: certified, all rows returned


@pytest.mark.parametrize("rescore_k,k,gshift", [(0, 10, 0), (32, 10, 1), (16, 10, 2), (128, 10, -1), (0, 1, 0)])
def test_gshift_plans(rescore_k, k, gshift):
    x, q = gauss(16385, 64, 40, seed=3)
    rep = passes(x, q, k, f"gshift={gshift}", rescore_k=rescore_k)
    assert rep["gshift"] == gshift and rep["by_gfin"] == 0         # the emulation has no k-row bound: gfin can only tie (oracle/select.py)


def ties_case(n_same, B=6):
    x, q = gauss(16384, 64, B, seed=11)
    same = np.arange(7, 16384, 16384 // n_same)[:n_same]           # spread over all 64 chunks
    x[same] = x[same[0]]
    q[0] = x[same[0]]
    q[3] = x[same[0]]
    return x, q, same


def test_ties_and_the_cap():
    x, q, same = ties_case(300)
    d, final, first = emulate(x, q, 10)
    rep = SL.check_launch(d, final)
    assert rep["uncertified"] >= 2 and rep["over_cap"] == 0 and np.array_equal(final[1][0], same[:10])
    ref = SL.select_reference(d, 0)
    assert np.array_equal(ref["rows"], same[:64]), "the lowest 64 of the identical rows are selected"
    x, q, same = ties_case(5000)
    d, final, first = emulate(x, q, 10)
    rep = SL.check_launch(d, final)
    assert rep["over_cap"] == 2 and np.array_equal(final[1][0], same[:10]) and SL._same(*final, *first)
    print("SELECT_STAGES_CPU ties", SL.summary(rep))


def ladder_case(k=10, kp=64, frac=0.75, n=16385, dim=64, B=8):
    """Query 0 = u; rows with cosines 0.9 - j * step to u, the gap between the k-th and the kp-th being frac * eps."""
    rng = np.random.default_rng(5)
    x, q = gauss(n, dim, B, seed=5)
    u = q[0].astype(np.float64)
    eps = SL.eps64(RD.bf16_residual(q[:1])[0], RD.bf16_residual(x).max(), dim)
    step = frac * eps / (kp - k)
    put = rng.choice(n, kp + 40, replace=False)
    for j, r in enumerate(put):
        w = rng.standard_normal(dim)
        w -= (w @ u) * u
        c = 0.9 - j * step
        x[r] = (c * u + np.sqrt(1 - c * c) * w / np.linalg.norm(w)).astype(np.float32)
    return x, q


def test_partial_failures_and_id_base():
    x, q = ladder_case()
    rep = passes(x, q, 10, "ladder", id_base=1_000_000_007)
    assert 1 <= rep["uncertified"] < rep["B"] and rep["by_T"] == rep["B"]
    rep = passes(x, q, 10, "every query fails", rescore_k=10)
    assert rep["uncertified"] == rep["B"]


def test_without_the_certificate():
    x, q = gauss(16385, 64, 7, seed=9)
    rep = passes(x, q, 10, "certify=0", certify=False, rescore_k=64)
    assert rep["visible"] == 7


def _hand_table(value_of_col):
    def tweak(lists, counts, table):
        table[0, 0, :, 0] = SC.f32_orderable(np.array([value_of_col(c) for c in range(64)], np.float32))
    return tweak


def test_gfin_decides_on_a_hand_written_table():
    """gfin > score(T) needs lists the k-row bound emptied (oracle/select.py); here the table of query 0 is written by hand:
    every column 0.5 eps below the k-th cosine, the kp-th key far below."""
    x, q = gauss(16385, 64, 4, seed=13)
    d, final, _ = emulate(x, q, 10, rescore_k=32)
    ref = SL.select_reference(d, 0)
    eps = SL.eps64(d["q_resid"][0], d["resid_max"], 64)
    assert ref["kth_score"] - ref["score_T"] > 2 * eps
    high = ref["kth_score"] - 0.5 * eps
    both = _hand_table(lambda c: high)
    rep = passes(x, q, 10, "hand table", rescore_k=32, tweak=both)
    assert rep["by_gfin"] == 1 and rep["uncertified"] >= 1
    assert "certified = True" in fails("certificate", x, q, 10, rescore_k=32, tweak=both, fault="no_gfin")
    pairs = _hand_table(lambda c: high if c % 2 == 0 else 0.05)     # gshift = 1: the maximum of each PAIR of columns counts
    rep = passes(x, q, 10, "hand table, pairs", rescore_k=32, tweak=pairs)
    assert rep["gshift"] == 1 and rep["by_gfin"] == 1
    fails("certificate", x, q, 10, rescore_k=32, tweak=pairs, fault="no_fold")


def test_m_below_k_under_a_bound():
    """m < k with a bound in force (lists emptied by hand): thr = -1 - eps, every row is collected, more than exact_cap, and the
    first-pass answer -- five rows and padding -- stands."""
    def tweak(lists, counts, table):
        counts[:, 0] = 0
        counts[3, 0] = 5
    x, q = gauss(16385, 64, 3, seed=17)
    d, final, _ = emulate(x, q, 10, tweak=tweak)
    rep = SL.check_launch(d, final)
    assert rep["m_lt_k"] == 1 and rep["over_cap"] == 1 and (final[1][0] >= 0).sum() == 5
    eps = SL.eps64(d["q_resid"][0], d["resid_max"], 64)
    assert abs(float(d["thr"][0]) - (-1.0 - eps)) <= SL.THR_TOL


# ------------------------------------------------------------------------------ each seeded fault fails at its stage
@pytest.fixture(scope="module")
def visible():
    """k = kp = 16 without the certificate: select's answer is the final answer and every selected row is in it; rows 100 .. 119
    are bit-identical and query 0 aims at them."""
    x, q = gauss(3000, 128, 6, seed=21)
    x[100:120] = x[100]
    q[0] = x[100]
    return x, q


@pytest.mark.parametrize("fault,stage", [("T_off", "select"), ("below_T", "select"), ("skip_vec", "rescore"), ("ties_reversed", "order")])
def test_select_faults(visible, fault, stage):
    x, q = visible
    passes(x, q, 16, "visible", certify=False, rescore_k=16)
    fails(stage, x, q, 16, certify=False, rescore_k=16, fault=fault)


def test_certificate_and_threshold_faults():
    x, q = ladder_case()
    d, final, _ = emulate(x, q, 10)
    ref = SL.select_reference(d, 0)
    eps = SL.eps64(d["q_resid"][0], d["resid_max"], 64)
    assert 0.55 * eps < ref["kth_score"] - ref["score_T"] < 0.95 * eps, "the ladder puts query 0 between eps / 2 and eps"
    assert "query 0" in fails("certificate", x, q, 10, fault="eps_half")
    fails("threshold", x, q, 10, fault="thr_no_eps")
    fails("compact", x, q, 10, rescore_k=10, fault="unsorted")


def test_tail_faults():
    x, q = ladder_case()
    d, final, first = emulate(x, q, 10, rescore_k=10)
    assert not np.array_equal(final[1][0], first[1][0]), "select's answer for the ladder query is not the exact one"
    fails("tail", x, q, 10, rescore_k=10, fault="keep_first")
    x, q, same = ties_case(300)
    d, final, first = emulate(x, q, 10, exact_cap=256)
    assert SL.check_launch(d, final)["over_cap"] == 2
    fails("tail", x, q, 10, exact_cap=256, fault="replace_over")
