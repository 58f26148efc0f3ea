"""Seeded inputs and the read-back harness of tests/test_scan_stages_gpu.py, shared with the child processes that repeat two
of its cases on the knobs build (`python -m tests.scan_stage_cases <form>`), in the style of encoder_stage_cases.py.

Every case searches once, reads what that one launch of the bf16 scan left (VectorIndex.scan_last / scan_read), asserts the
plan and kernel family it meant to test and applies P1 .. P5 of oracle/scan.py over every (row, query)."""
import functools
import json
import sys

import numpy as np

from oracle import rounding as RD
from oracle import scan as SC

N_A = 64 * 256                  # section A: one tile per chunk on a part with >= 128 CUs
N_B = 70_001                    # section B: 274 tiles
TIE_ROWS = np.arange(9216 - 200, 9216 + 200)      # tile 36 starts a chunk with 256 chunks (18 + 18) and with 128 (12 x 3)
PLANS_B = [(0, 10), (0, 1), (0, 16), (0, 20), (0, 40), (16, 10), (32, 10), (0, 64)]


def expected_family(bn, form="default"):
    """-> (family, nst, nstb) of scan.hip launch_scan_bf16; form: default | v0 | ring2 (the knobs SQE_SCAN=v0, SQE_SCAN128=2)"""
    from semantic_query_engine_amd import engine as E
    if bn == 256:
        return (E.SCAN_FAMILY_STAGED, 2, 2) if form == "v0" else (E.SCAN_FAMILY_PINGPONG, 0, 0)
    if bn == 128:
        return (E.SCAN_FAMILY_STAGED, 2, 2) if form == "ring2" else (E.SCAN_FAMILY_STAGED, 3, 2)
    return (E.SCAN_FAMILY_STAGED, 3, 3)


def assert_plan(ctx, L, rows, B, k, rescore_k, form="default"):
    want = SC.expected_plan(rows, B, k, ctx.device_info()["cu_count"], rescore_k)
    if form == "v0" and want["bn"] == 256:
        want["k_rows"] = 0                                    # that kernel takes the minimum of the quad maxima
    got = {key: L[key] for key in want}
    assert got == want, (got, want)
    assert (L["family"], L["nst"], L["nstb"]) == expected_family(L["bn"], form), L
    assert L["certified"] == 1
    return want


# ------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def rows_a(dim):
    return np.random.default_rng(100 + dim).standard_normal((N_A, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def queries_a(dim):
    rng = np.random.default_rng(200 + dim)
    q = rng.standard_normal((300, dim)).astype(np.float32)
    x = rows_a(dim)
    q[::7] = x[rng.integers(0, N_A, q[::7].shape[0])] + 0.1 * q[::7]
    return q


@functools.lru_cache(maxsize=None)
def rows_b(kind, n=N_B, dim=128):
    """gauss | rising | falling | ties | negative.  rising / falling: Gaussian rows sorted by their cosine with one direction u
    (the queries of block `hard` are u plus a little noise, so for them every row beats all rows before it / none does).  The
    two-coordinate circle of test_search_gpu.py::test_adversarial_orderings is not used: its bf16 copies hold thousands of
    bit-identical scores, which sit in the undecided band by construction; ties have their own case."""
    rng = np.random.default_rng({"gauss": 1, "rising": 2, "falling": 3, "ties": 4, "negative": 5}[kind] * 1000 + n % 1000)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    u = rng.standard_normal(dim).astype(np.float32)
    if kind in ("rising", "falling"):
        s = (x / np.linalg.norm(x, axis=1, keepdims=True)) @ u
        order = np.argsort(s, kind="stable")
        x = np.ascontiguousarray(x[order] if kind == "rising" else x[order[::-1]])
    elif kind == "ties":
        x[TIE_ROWS] = x[TIE_ROWS[0]]
    elif kind == "negative":
        x[:, 0] = np.abs(x[:, 0]) + 4.0
        u = -(x / np.linalg.norm(x, axis=1, keepdims=True)).mean(axis=0)
    x.setflags(write=False)
    return x, u


@functools.lru_cache(maxsize=None)
def queries_b(kind, B, n=N_B, dim=128):
    """B queries: 50 near stored rows (from query 8 on), a `hard` block of 8 in front, Gaussian queries behind."""
    x, u = rows_b(kind, n, dim)
    rng = np.random.default_rng(B * 31 + len(kind))
    q = rng.standard_normal((B, dim)).astype(np.float32)
    near = rng.integers(0, n, 50)
    q[8:58] = x[near] + 0.1 * q[8:58]
    if kind in ("rising", "falling", "negative"):
        q[:8] = u + 0.02 * np.linalg.norm(u) / np.sqrt(dim) * q[:8]
    elif kind == "ties":
        q[0] = x[TIE_ROWS[0]]
    q.setflags(write=False)
    return q


# ------------------------------------------------------------------------------ read-back
def reference(idx, L):
    """-> (S, delta, slack) of the launch, from the library's own copies"""
    from semantic_query_engine_amd import engine as E
    B, dim = L["B"], L["dim"]
    xb = idx.scan_bf16()
    assert not xb[L["rows"]:].any(), "rows past the end of the scanned copy are zero"
    qn = idx.state_read(E.STATE_QN, np.float32, B * dim).reshape(B, dim)
    S, delta = SC.scores(xb[:L["rows"]], RD.bf16_round(qn))
    slack = SC.slack_of(idx.state_read(E.STATE_Q_RESID, np.float32, B), idx.state_read(E.STATE_RESID_MAX, np.float32, 1)[0], dim)
    return S, delta, slack


def read_launch(idx, L, ref=None):
    from semantic_query_engine_amd import engine as E
    nc, bp, cap = L["n_chunks"], L["b_pad"], L["list_cap"]
    counts = idx.scan_read(E.SCAN_LIST_COUNTS, np.int32, nc * bp).reshape(nc, bp)
    lists = idx.scan_read(E.SCAN_LISTS, np.uint64, nc * bp * cap).reshape(nc, bp, cap)
    table = idx.scan_read(E.SCAN_BOUNDS, np.uint32, bp * L["ngroups"] * 64).reshape(bp // 64, L["ngroups"], 64, 64)
    S, delta, slack = ref if ref is not None else reference(idx, L)
    return SC.Launch(L, lists, counts, table, S, delta, slack)


def report(name, L, out):
    fam = "pingpong" if (L["family"] == 0) else "staged%d%d" % (L["nst"], L["nstb"])
    print("SCAN_STAGES " + json.dumps({"case": name, "bn": L["bn"], "family": fam, "kp": L["kp"], "k": L["k"], "chunks": L["n_chunks"],
                                        **{k: (round(v, 6) if isinstance(v, float) else v) for k, v in out.items()}}), flush=True)


def run_every_score(ctx, idx, n, dim, B, form="default", name="A"):
    """Section A: kp = 256, one tile per chunk, bounds off -- every list holds every row of its tile, P2 sees all rows x B scores."""
    q = queries_a(dim)[:B]
    k = 100
    idx.search(q, k)
    L = idx.scan_last()
    assert_plan(ctx, L, n, B, k, 256, form)
    assert L["n_chunks"] == L["n_tiles"] and L["gshift"] < 0 and L["gshift_k"] < 0 and L["kp"] == L["trig"] == 256
    st = read_launch(idx, L)
    out = SC.check_first_pass(st)
    assert out["keys"] == n * B, (out["keys"], n * B)
    assert np.array_equal(st.counts[:, :B], np.minimum(256, n - 256 * np.arange(L["n_chunks"]))[:, None].repeat(B, 1))
    report("%s n=%d dim=%d B=%d" % (name, n, dim, B), L, out)
    return out


def run_bounds(ctx, idx, kind, n, B, rescore_k, k, ref_cache, form="default", name="B"):
    """Section B: one search under the bounds, P1 .. P4.  ref_cache: dict that keeps (S, delta, slack) of (index, queries)."""
    q = queries_b(kind, B, n)
    idx.set_option("rescore_k", rescore_k)
    cos, ids = idx.search(q, k)
    L = idx.scan_last()
    want = assert_plan(ctx, L, n, B, k, rescore_k, form)
    if (kind, n, B) not in ref_cache:
        ref_cache.clear()                                      # one reference at a time: 2 x 168 MB at B = 300
        ref_cache[(kind, n, B)] = reference(idx, L)
    st = read_launch(idx, L, ref_cache[(kind, n, B)])
    assert st.bounds_on == (want["gshift"] >= 0 or want["gshift_k"] >= 0)
    out = SC.check_first_pass(st)
    if kind == "ties" and n == N_B:
        check_ties(st, cos, ids, k)
    report("%s %s n=%d B=%d rescore_k=%d" % (name, kind, n, B, rescore_k), L, out)
    return st, out


def check_ties(st, cos, ids, k):
    """400 bit-identical rows across a chunk boundary, query 0 on them: equal scores are ordered by the key, so a list that had
    to choose kept the LOWEST rows, and the answer is the first k of them."""
    c, q, sc, row, o = st.live()
    mine = (q == 0) & np.isin(row, TIE_ROWS)
    assert np.unique(o[mine]).size == 1, "identical operands, identical scores"
    for ch in np.unique(c[mine]):
        lo, hi = st.starts[ch], st.starts[ch + 1]
        there = TIE_ROWS[(TIE_ROWS >= lo) & (TIE_ROWS < hi)]
        kept = np.sort(row[mine & (c == ch)])
        assert np.array_equal(kept, there[:kept.size]), ("a higher row kept over a lower one", int(ch))
    assert kept.size and np.array_equal(ids[0], TIE_ROWS[:k])


def run_collect(ctx, idx, L, x_master=None):
    """Section C: P5 on the buffers of the collect pass.  The key scores are compared with the fp32 cosines the re-score left in
    them (include/sqe.h), computed in float64 from the fp32 rows and queries the library holds."""
    from semantic_query_engine_amd import engine as E
    B, dim, rows = L["B"], L["dim"], L["rows"]
    S, delta, _ = reference(idx, L)
    thr = idx.scan_read(E.SCAN_COLLECT_THR, np.float32, L["b_pad"])
    u = int(idx.scan_read(E.SCAN_UNC_COUNT, np.int32, 1)[0])
    assert u == L["uncertified"]
    unc_ids = idx.scan_read(E.SCAN_UNC_IDS, np.int32, u)
    counts = idx.scan_read(E.SCAN_COLLECT_COUNTS, np.int32, B)
    keys = idx.scan_read(E.SCAN_COLLECT_KEYS, np.uint64, u * L["exact_cap"]).reshape(u, L["exact_cap"])
    assert not counts[u:].any(), "a compact index past the count collected rows"
    qn = idx.state_read(E.STATE_QN, np.float32, B * dim).reshape(B, dim).astype(np.float64)
    xm = idx.get_rows(np.arange(rows)).astype(np.float64)
    Sk = xm @ qn.T
    dk = 1.05 * dim * 2.0 ** -24 * (np.abs(xm) @ np.abs(qn).T)
    need = (S >= thr[None, :B].astype(np.float64) - delta).sum(axis=0)
    assert need.max() <= L["exact_cap"], "the reference says a query overflows the collect buffer: pick other data"
    share, worst, over = SC.check_collect(L, thr, unc_ids, counts, keys, S, delta, key_ref=(Sk, dk))
    assert over == 0
    return {"uncertified": u, "undecided": share, "p2_fp32": worst}


# ------------------------------------------------------------------------------ child process: one A case and one B case on another form
def main(form):
    from semantic_query_engine_amd import Context, VectorIndex
    ctx = Context(0)
    B = {"v0": 300, "ring2": 100, "krot": 300}[form]
    fam = "default" if form == "krot" else form
    idx = VectorIndex(ctx, 192)
    idx.set_option("rescore_k", 256)
    idx.add(rows_a(192))
    run_every_score(ctx, idx, N_A, 192, B, fam, name="D/" + form + " A")
    idx.close()
    idx = VectorIndex(ctx, 128)
    idx.add(rows_b("gauss")[0])
    run_bounds(ctx, idx, "gauss", N_B, B, 0, 10, {}, fam, name="D/" + form + " B")
    idx.close()
    print(json.dumps({"ok": True}))


if __name__ == "__main__":
    main(sys.argv[1])
