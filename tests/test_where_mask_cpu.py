"""The host side of the mask route of sqe_index_search_where (csrc/fieldpred.cpp): the depth rule sqe_where_depth against exact
integer binomial sums, the cost rule's shape, the ABI of the read-back, and both under ASan + UBSan as a stand-alone program.
No GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_query_engine_amd", "csrc")

KS = (1, 3, 10, 20, 64, 100, 256)
LIVES = (1000, 70_001, 10_000_000, (1 << 31) + 7)
FRACTIONS = (0.001, 0.01, 0.06, 0.1, 0.21, 0.3, 0.5, 0.75, 0.9, 0.99, 0.999)
ISSUE_TABLE = {          # k -> d at f = 0.1 / 0.21 / 0.3 / 0.5 / 0.75 / 1.0 (0: none)
    1: (66, 30, 20, 10, 5, 1),
    3: (108, 49, 33, 18, 10, 3),
    10: (220, 101, 69, 38, 22, 10),
    20: (0, 166, 113, 64, 38, 20),
    100: (0, 0, 0, 248, 156, 100),
}
TABLE_F = (0.1, 0.21, 0.3, 0.5, 0.75, 1.0)
ONE = 10 ** 9


@pytest.fixture(scope="module")
def where_depth():
    so = os.path.join(ROOT, "semantic_query_engine_amd", "libsqe.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from semantic_query_engine_amd import engine
    return engine.where_depth


def _tail_scaled(d, k, s, live):
    """(numerator, denominator) of P[Binomial(d, s / live) < k] as exact integers"""
    num, c = 0, 1
    for i in range(min(k, d + 1)):
        num += c * s ** i * (live - s) ** (d - i)
        c = c * (d - i) // (i + 1)
    return num, live ** d


def _within(d, k, s, live):
    """the exact tail at d is <= 2^-10 (1 + 1e-9)"""
    num, den = _tail_scaled(d, k, s, live)
    return num * 1024 * ONE <= den * (ONE + 1)


def _beyond(d, k, s, live):
    """the exact tail at d is > 2^-10 (1 - 1e-9)"""
    num, den = _tail_scaled(d, k, s, live)
    return num * 1024 * ONE > den * (ONE - 1)


def _cases():
    for k in KS:
        for live in LIVES:
            sel = {k - 1, k, k + 1, live, live - 1, live // 2}
            sel.update(int(f * live) for f in FRACTIONS)
            for s in sorted(x for x in sel if 0 <= x <= live):
                yield k, s, live


def test_depth_rule_against_exact_binomial_sums(where_depth):
    checked = none = 0
    for k, s, live in _cases():
        d = where_depth(k, s, live)
        if s < k:
            assert d == 0, (k, s, live, d)
            continue
        if d == 0:                                   # no depth up to 256 may do (the tail falls with d)
            assert _beyond(256, k, s, live), (k, s, live)
            none += 1
            continue
        assert k <= d <= 256, (k, s, live, d)
        assert _within(d, k, s, live), (k, s, live, d)
        assert _beyond(d - 1, k, s, live), (k, s, live, d)
        checked += 1
    print(f"{checked} depths and {none} refusals agree with the exact sums")
    assert checked > 200 and none > 50


def test_depth_rule_gives_the_documented_table(where_depth):
    live = 1_000_000
    for k, row in ISSUE_TABLE.items():
        got = tuple(where_depth(k, int(round(f * live)), live) for f in TABLE_F)
        assert got == row, (k, got)
    assert where_depth(10, 60_000, live) == 0 and where_depth(3, 60_000, live) == 183
    # selected = live: exactly k; arguments outside the domain answer 0
    for k in KS:
        assert where_depth(k, live, live) == k
        assert where_depth(k, k - 1, live) == 0
    assert where_depth(0, 10, 10) == 0 and where_depth(257, 1000, 1000) == 0 and where_depth(3, 10, 0) == 0
    assert where_depth(3, 20, 10) == 3               # more selected than live reads as every row


def test_header_and_bindings_agree():
    from semantic_query_engine_amd import _native, engine
    text = open(os.path.join(ROOT, "include", "sqe.h")).read()
    assert re.search(r"typedef struct \{ int32_t route, depth, first_pass_i8, pad; int64_t selected, live, swept; \} sqe_where_last_t;", text)
    assert re.search(r"enum \{ SQE_WHERE_ROUTE_NONE = 0, SQE_WHERE_ROUTE_GATHER = 1, SQE_WHERE_ROUTE_MASK = 2 \};", text)
    assert ctypes.sizeof(_native.WhereLast) == 40
    assert (engine.WHERE_ROUTE_NONE, engine.WHERE_ROUTE_GATHER, engine.WHERE_ROUTE_MASK) == (0, 1, 2)
    for name in ("sqe_index_where_last", "sqe_where_depth"):
        assert name in _native.SIGNATURES
    for option in ("where_route", "where_mask_depth", "where_mask_min_rows"):
        assert f'"{option}"' in text and f'k == "{option}"' in open(os.path.join(CSRC, "api.hip")).read()


def _driver(lines):
    subprocess.check_call(["make", "-C", CSRC, "wheredepth_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build_san", "wheredepth_asan")
    text = "".join(" ".join(str(v) for v in line) + "\n" for line in lines)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def test_rules_under_asan_ubsan(where_depth):
    lines = [(k, s, live, 1, k, 0) for k, s, live in _cases()]
    lines += [(0, 5, 5, 1, 1, 0), (257, 500, 500, 1, 256, 0), (-3, 5, 5, 1, 1, 0), (3, -1, 10, 1, 3, 0), (3, 5, -10, 1, 3, 0),
              (256, (1 << 62), (1 << 62) + 5, 1 << 30, 256, 1), (1, 1, 1, 0, 1, 1)]
    rows = _driver(lines)
    for line, (depth, _) in zip(lines, rows):
        assert depth == where_depth(*line[:3]), line


def test_cost_rule_shape():
    """The rule is a pure function of (live, M, B, k, d, first pass): it never prefers the mask route for a narrower predicate
    where it refuses it for a broader one, nor for a bf16 first pass where it refuses it for int8, and it refuses an empty one."""
    live = 10_000_000
    lines = []
    for i8 in (0, 1):
        for b in (1, 64, 1024, 5000):
            for d in (3, 18, 38, 248):
                for pct in (0, 1, 3, 6, 10, 15, 21, 30, 50, 75, 100):
                    lines.append((min(d, 10), live * pct // 100, live, b, d, i8))
    rows = _driver(lines)
    got = {line: cheaper for line, (_, cheaper) in zip(lines, rows)}
    for (k, s, lv, b, d, i8), cheaper in got.items():
        if s == 0:
            assert cheaper == 0
        if cheaper:
            assert all(got[(k, s2, lv, b, d, i8)] for (k2, s2, lv2, b2, d2, i82) in got if (k2, lv2, b2, d2, i82) == (k, lv, b, d, i8) and s2 > s)
            if i8 == 0:
                assert got[(k, s, lv, b, d, 1)]
    assert any(got.values()) and not all(got.values())
    # the same fractions of an index a tenth the size decide alike: size and dimension cancel
    small = _driver([(k, s // 10, lv // 10, b, d, i8) for (k, s, lv, b, d, i8) in lines])
    assert [c for _, c in small] == [c for _, c in rows]
