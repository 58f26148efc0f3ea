"""What ONE launch of the bf16 scan leaves behind -- every candidate key, every column of the bound table, every dropped row,
every key of the collect pass -- against a float64 product of the library's own bf16 copies (oracle/scan.py, P1 .. P5), through
the test-only read-back sqe_index_scan_last / sqe_index_scan_read.  The final top-k would not show a lost row, a stale operand
tile or a table column that is too high: the fp32 re-score, the certificate and the collect pass mask them, and the certificate
trusts the same table.  tests/test_scan_stages_cpu.py shows on a NumPy emulation that each property can fail.

Every case asserts from scan_last() the plan and the kernel family it means to test, computed from the device's CU count
(tests/scan_stage_cases.py: assert_plan).  Notes on the shapes:
  * Section A searches with k = 100: with rescore_k = 256 the kp-row bound is off, and the k-row bound is off only for k > 64.
  * (rescore_k, k) = (0, 40) and (0, 64) give kp = 128: the kp-row bound is off, the k-row bound (group size 1) stays on; that is
    what the plan says and what is asserted.
  * The collect launches never store to the lists, their counts or the table (scan.hip: COLLECT mode returns before the final
    compaction and filter_group appends to the collect buffers only), so sections A and B read them whether or not a
    certificate failed.  The fp32 re-score (exact.hip) overwrites the SCORE half of the collect keys with the fp32 cosine, so
    section C checks the key scores against a float64 product of the fp32 rows and queries instead of the bf16 copies; the
    row sets are checked against the bf16 reference as P5 states.
Measured ratios: profiles/scan_stages/NOTES.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import scan as SC
from tests import scan_stage_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS_LIB = os.path.join(ROOT, "semantic_query_engine_amd", "libsqe_knobs.so")


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _index(ctx, x, rescore_k=0):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, x.shape[1])
    idx.set_option("rescore_k", rescore_k)
    idx.add(x)
    return idx


# ------------------------------------------------------------------------------ A. every score of the launch
@pytest.fixture(scope="module")
def index_a(ctx):
    """dim -> the 64 x 256-row index of section A (built once, searched by every batch size)"""
    made = {}

    def get(dim):
        if dim not in made:
            made[dim] = _index(ctx, C.rows_a(dim), 256)
        return made[dim]
    yield get
    for idx in made.values():
        idx.close()


CASES_A = ([(b, d) for b in (1, 64) for d in (64, 192, 1024)] + [(b, d) for b in (65, 128) for d in (64, 192)] +
           [(b, d) for b in (129, 300) for d in (64, 192, 1024)])


@pytest.mark.parametrize("B,dim", CASES_A)
def test_every_score_of_the_launch(ctx, index_a, B, dim):
    """KS = 1 (shorter than every ring), 3 (neither even nor longer than 3) and 16 K steps; the 64- and 128-query rings, the
    ping-pong kernel with one and two query blocks.  rows x B scores, each within its delta."""
    out = C.run_every_score(ctx, index_a(dim), C.N_A, dim, B)
    assert out["p2"] <= 1.0


@pytest.mark.parametrize("n,B", [(C.N_A - 255, 64), (C.N_A - 255, 300), (1, 7), (255, 7), (256, 7), (257, 7)])
def test_every_score_partial_tiles(ctx, n, B):
    """A last tile of one row, and indexes of one row / one row short of a tile / one tile / one tile and a row: rows past the
    end are masked in the BOOT fold and in the filter, and a list of exactly kp = trig = 256 keys is compacted with n == kp."""
    idx = _index(ctx, C.rows_a(192)[:n], 256)
    C.run_every_score(ctx, idx, n, 192, B)
    idx.close()


# ------------------------------------------------------------------------------ B. the bounds
@pytest.fixture(scope="module")
def index_b(ctx):
    made, refs = {}, {}

    def get(kind, n):
        if (kind, n) not in made:
            for idx in made.values():                          # one index at a time
                idx.close()
            made.clear()
            made[(kind, n)] = _index(ctx, C.rows_b(kind, n)[0])
        return made[(kind, n)], refs
    yield get
    for idx in made.values():
        idx.close()


N_LONG = 200_001               # 782 tiles: three or four per chunk at 256 chunks
CASES_B = ([("gauss", C.N_B, b, p) for b in (64, 100, 300) for p in C.PLANS_B] +
           [(kind, C.N_B, b, p) for kind in ("rising", "falling", "ties", "negative") for b in (64, 100, 300)
            for p in ((0, 10), (16, 10), (0, 64))] +
           [("gauss", 16_385, b, p) for b in (64, 100, 300) for p in ((0, 10), (16, 10))] + [("negative", 16_385, 100, (0, 10))] +
           # the bound table is first fetched during a chunk's second entry and applied two K steps later,
           # so with one or two tiles per chunk and two K steps per tile the staged kernels hardly filter a tile against it;
           # three or four tiles per chunk for them as well
           [("gauss", N_LONG, 64, (0, 10)), ("gauss", N_LONG, 100, (0, 10)), ("gauss", N_LONG, 100, (0, 1))])


@pytest.mark.parametrize("kind,n,B,plan", CASES_B, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bounds(ctx, index_b, kind, n, B, plan):
    """70,001 rows at dim 128: 274 tiles dealt unevenly to 256 chunks (128 at B = 300), every table column shared by four (two)
    chunks; 16,385 rows: 65 chunks, column 0 shared, the other 63 not, the last chunk one row.  P1 .. P4 under every plan."""
    idx, refs = index_b(kind, n)
    st, out = C.run_bounds(ctx, idx, kind, n, B, plan[0], plan[1], refs)
    if plan[1] <= 32:
        assert st.L["kp"] <= 64 and st.L["gshift"] >= 0
    else:                                                       # k = 40, 64: kp = 128 turns the kp-row bound off, the k-row bound stays
        assert st.L["kp"] == 128 and st.L["gshift"] < 0 and st.L["gshift_k"] == 0 and st.L["k_rows"] == 0
    if kind == "negative":
        assert st.S[:, :8].max() < 0, "every real score of the hard block is negative: a pad row's 0 would be the maximum"
    assert out["p3"] is not None and out["p3"] <= 1.0
    if n == N_LONG:
        # the kp-row bound is a score ~3,000 rows' best reach in each of 64 columns, a list's own lowest the 64th of < 1,100 rows
        assert out["table_decides"] > 0.5, "the table terms were meant to be the deciding ones of P4 here"


# ------------------------------------------------------------------------------ C. the collect pass
@pytest.mark.parametrize("n,dim", [(20_001, 128), (3_000, 1024)])
@pytest.mark.parametrize("b", [8, 100, 200, 300, 600])
def test_collect_pass(ctx, n, dim, b):
    """rescore_k = k = 10 leaves the first pass no margin: every query goes through the collect pass, the four count ranges of
    run_collect_fallback (<= 64, <= 256, <= 512, above) and each collect kernel with them."""
    rng = np.random.default_rng(n + b)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((b, dim)).astype(np.float32)
    idx = _index(ctx, x, 10)
    idx.search(q, 10)
    L = idx.scan_last()
    C.assert_plan(ctx, L, n, b, 10, 10)
    assert L["uncertified"] == b
    out = C.run_collect(ctx, idx, L)
    C.report("C n=%d dim=%d B=%d" % (n, dim, b), L, out)
    idx.close()


def test_collect_pass_partial_failures(ctx):
    """test_search_gpu.py::test_partial_certificate_failures, n_hard = 5 of 64: only the queries aimed at a cluster of
    near-identical rows fail their certificate; unc_ids is their ascending list and the others have no keys."""
    n_hard, b, d, n = 5, 64, 256, 30000
    rng = np.random.default_rng(77 + n_hard)
    x = rng.standard_normal((n, d)).astype(np.float32)
    centre = rng.standard_normal(d).astype(np.float32)
    x[rng.choice(n, 3000, replace=False)] = centre + 3e-3 * rng.standard_normal((3000, d)).astype(np.float32)
    q = rng.standard_normal((b, d)).astype(np.float32)
    hard = rng.choice(b, n_hard, replace=False)
    q[hard] = centre + 3e-3 * rng.standard_normal((n_hard, d)).astype(np.float32)
    idx = _index(ctx, x)
    idx.search(q, 10)
    L = idx.scan_last()
    C.assert_plan(ctx, L, n, b, 10, 0)
    assert n_hard <= L["uncertified"] <= n_hard + 3
    out = C.run_collect(ctx, idx, L)
    from semantic_query_engine_amd import engine as E
    assert set(hard.tolist()) <= set(idx.scan_read(E.SCAN_UNC_IDS, np.int32, L["uncertified"]).tolist())
    st = C.read_launch(idx, L)                                  # the first pass's buffers outlive the collect launches
    SC.check_first_pass(st)
    C.report("C partial n=%d dim=%d B=%d" % (n, d, b), L, out)
    idx.close()


def test_read_back_errors(ctx):
    """SQE_ERR_STATE before a search and after a search the int8 first pass answered; range checks as sqe_index_i8_read."""
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    from semantic_query_engine_amd import engine as E
    idx = VectorIndex(ctx, 256)
    with pytest.raises(RuntimeError):
        idx.scan_last()
    x = C.rows_b("gauss")[0][:20000].reshape(10000, 256)
    idx.add(x)
    idx.search(x[:3], 5)
    L = idx.scan_last()
    assert (L["rows"], L["B"], L["k"], L["dim"]) == (10000, 3, 5, 256)
    with pytest.raises(RuntimeError):
        idx.scan_read(E.SCAN_LIST_COUNTS, np.int32, L["n_chunks"] * L["b_pad"] + 1)
    with pytest.raises(RuntimeError):
        idx.scan_read(99, np.int32, 1)
    for key, val in (("scan_mode", SCAN_INT8_RESCORE), ("i8_min_rows", 0), ("i8_sample_step", 4), ("i8_sample_m", 64)):
        idx.set_option(key, val)
    idx.search(x[:3], 5)
    idx.i8_last()
    with pytest.raises(RuntimeError):
        idx.scan_last()
    idx.close()


# ------------------------------------------------------------------------------ D. the A/B forms of the knobs build
@pytest.fixture(scope="module")
def knobs_env():
    # always through make: a knobs library left over from an older tree must not be the one that is tested
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "semantic_query_engine_amd", "csrc"), "KNOBS=1", "-j8"],
                          stdout=subprocess.DEVNULL)
    return dict(os.environ, SQE_LIB=KNOBS_LIB)


@pytest.mark.parametrize("form,var,val", [("v0", "SQE_SCAN", "v0"), ("ring2", "SQE_SCAN128", "2"), ("krot", "SQE_KROT", "1")])
def test_ab_forms(form, var, val, knobs_env):
    """The two-stage 256-query kernel (B = 300), the older ring of the 128-query tile (B = 100) and the rotated K walk (B = 300):
    one case of A (dim 192) and one of B each, in a child process of its own that asserts the family from scan_last()."""
    env = dict(knobs_env, **{var: val})
    out = subprocess.run([sys.executable, "-m", "tests.scan_stage_cases", form], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=300)
    sys.stdout.write("".join(line + "\n" for line in out.stdout.splitlines() if line.startswith("SCAN_STAGES")))
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["ok"] is True
