"""Seeded inputs and the harness of tests/test_select_stages_gpu.py: every case searches once on a fresh single-device flat index
without deletes, asserts from scan_last() the plan it meant to launch (computed from the device's CU count, as
scan_stage_cases.assert_plan does) and hands the read-back buffers and the final answer to oracle/select.py: check_launch."""
import functools
import json

import numpy as np

from oracle import scan as SC
from oracle import select as SL


@functools.lru_cache(maxsize=None)
def gauss_rows(n, dim, seed=0):
    x = np.random.default_rng(1000 * seed + dim + n % 997).standard_normal((n, dim)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def gauss_queries(B, dim, n, seed=0):
    """B Gaussian queries, every third one near a stored row"""
    rng = np.random.default_rng(7000 * seed + 31 * B + dim)
    q = rng.standard_normal((B, dim)).astype(np.float32)
    x = gauss_rows(n, dim, seed)
    q[::3] = x[rng.integers(0, n, q[::3].shape[0])] + 0.3 * q[::3]
    q.setflags(write=False)
    return q


def tie_rows(n_same, n=16384, dim=128):
    """-> (rows, queries, the identical rows): n_same bit-identical rows spread over all 64 chunks, queries 0 and 3 aimed at them"""
    x = gauss_rows(n, dim, 3).copy()
    q = gauss_queries(6, dim, n, 3).copy()
    same = np.arange(7, n, n // n_same)[:n_same]
    x[same] = x[same[0]]
    q[0] = x[same[0]]
    q[3] = x[same[0]]
    return x, q, same


def partial_failures(n_hard=5, b=64, d=256, n=30000):
    """the data of test_scan_stages_gpu.py::test_collect_pass_partial_failures"""
    rng = np.random.default_rng(77 + n_hard)
    x = rng.standard_normal((n, d)).astype(np.float32)
    centre = rng.standard_normal(d).astype(np.float32)
    x[rng.choice(n, 3000, replace=False)] = centre + 3e-3 * rng.standard_normal((3000, d)).astype(np.float32)
    q = rng.standard_normal((b, d)).astype(np.float32)
    hard = rng.choice(b, n_hard, replace=False)
    q[hard] = centre + 3e-3 * rng.standard_normal((n_hard, d)).astype(np.float32)
    return x, q, np.sort(hard)


def make_index(ctx, x, **options):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, x.shape[1])
    for key, val in options.items():
        idx.set_option(key, val)
    idx.add(x)
    return idx


def assert_plan(ctx, L, rows, B, k, rescore_k, certify=True):
    """the plan of the launch, from the device's CU count; without the certificate the k-row bound's fields are not compared"""
    want = SC.expected_plan(rows, B, k, ctx.device_info()["cu_count"], rescore_k)
    skip = () if certify else ("gshift_k", "k_rows")
    got = {key: L[key] for key in want if key not in skip}
    assert got == {key: v for key, v in want.items() if key not in skip}, (got, want)
    assert L["certified"] == int(certify)
    return want


def expected_form(want):
    return "large" if want["n_chunks"] * want["kp"] > SL.SMALL_SLOTS else "small"


def search_and_check(ctx, idx, q, k, rescore_k, name, id_base=0, certify=True):
    """-> (report, L, (cos, ids)); asserts the plan and the launch form before it compares"""
    idx.set_option("rescore_k", rescore_k)
    cos, ids = idx.search(q, k)
    L = idx.scan_last()
    want = assert_plan(ctx, L, len(idx), q.shape[0], k, rescore_k, certify)
    rep = SL.check_launch(idx, (cos, ids), id_base, L)
    assert rep["form"] == expected_form(want) and rep["route_lds"] + rep["route_global"] == q.shape[0]
    out = SL.summary(rep)
    out.pop("first_failure")
    print("SELECT_STAGES " + json.dumps({"case": name, "rows": L["rows"], "dim": L["dim"], **out}), flush=True)
    return rep, L, (cos, ids)
