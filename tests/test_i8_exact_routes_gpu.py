"""Bit-exact collect sets of EVERY kernel the int8 launcher can pick (scan_i8.hip: launch_scan_i8; search.hip: i8_scan_select).

The launcher chooses among seven kernel instantiations by (dim, batch); sqe_i8_launch_t.kernel says which one ran, and every case
here asserts it against expected_kernel -- the route table restated in plain Python -- BEFORE it compares keys, so a change of the
dispatch cannot move a route off its test unnoticed.  The comparison is tests/test_i8_exact_gpu.py's: the launch's own operands
read back, {(acc * s, row) : acc * s >= thr} recomputed exactly, equality with the keys the launch wrote.

  A  Gaussian rows, every route.  76,877 rows = 301 tiles with a partial last one: on 256 CUs 45 chunks of two tiles and 211 of
     one, so at dim 256 a staged kernel's chunk is 2 K-steps, fewer than its 3-deep ring; dims with one, two and three slice
     groups per tile for the streaming rings; dims that are staged only because the queries do not fit the LDS budget.
  B  Edge data, one case per instantiation.  153,677 rows = 601 tiles (chunks of 2-3 tiles up to batch 256) that hold two blocks
     of whole, unsampled tiles:
       crowd       three consecutive tiles of one chunk, rows a c + sqrt(1 - a^2) u around a fixed unit vector c, and eight queries
                   near c: each collects all 768 rows, more than a (chunk, query) list holds (the pool branch slot >= list_cap) and
                   more per 32-row wave than the 192-slot wave buffer of the streaming kernels (the mid-chunk flush);
       saturation  two tiles of sign rows +-1 / sqrt(dim), four queries that are such rows and four that are their negatives:
                   |acc| = 0.90-0.95 x min(2^23, dim 127^2), both signs, where __mul24(acc, scale) relies on quant.hip's norm cap.
     Each precondition is asserted from the NumPy side of the comparison: a case cannot pass without reaching its edge.
  C  Two identical searches collect the same key set, for both staged kernels and stream<64,32>."""
import numpy as np
import pytest

from tests.test_i8_exact_gpu import _check_collect, _check_sample, _chunk_range, _i8_index, _launch_lists, expected_kernel

pytestmark = pytest.mark.gpu

STEP, M, K_TOP = 8, 64, 10
N_A = 76_800 + 77          # 301 tiles, the last one partial
N_B = 153_600 + 77         # 601 tiles
WAVE_BUF = 192             # scan_i8.hip: key slots of one wave of a streaming kernel (it flushes when fewer than 64 are free)
PLANT = 12                 # rows summed into a query of section A where Gaussian queries cannot certify (dim >= 2048)
CROWD_Q, SAT_Q = 8, 4      # queries near the crowd's centre; copies of sign rows, and as many negated copies


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def device():
    import torch
    return torch.device("cuda", 0)


def _names():
    from semantic_query_engine_amd import engine as E
    return {getattr(E, n): n[len("I8_KERNEL_"):] for n in dir(E) if n.startswith("I8_KERNEL_")}


def _search_once(ctx, x, q, dim):
    idx = _i8_index(ctx, dim, STEP, M)
    idx.add(x)
    ctx.stats_reset()
    idx.search(q, K_TOP)
    return idx, idx.i8_last()


# ------------------------------------------------------------------------------------------------------------------ A
ROUTES_A = [("STREAM_64_32", 1024, 1), ("STREAM_64_32", 1024, 64), ("STREAM_64_32", 2048, 33),
            ("STREAM_64_16", 1536, 40), ("STREAM_64_16", 512, 64),
            ("STREAM_128_16", 512, 65), ("STREAM_128_16", 1024, 128),
            ("STAGED_64", 256, 7), ("STAGED_64", 768, 64), ("STAGED_64", 2560, 20),          # 2560: staged because of the LDS budget
            ("STAGED_128", 384, 100), ("STAGED_128", 768, 128), ("STAGED_128", 1536, 128)]   # 1536: staged because of the LDS budget


@pytest.mark.parametrize("kernel,dim,b", ROUTES_A)
def test_gaussian_rows_every_route(ctx, device, kernel, dim, b):
    from semantic_query_engine_amd import engine as E
    rng = np.random.default_rng(100_000 * dim + b)
    x = rng.standard_normal((N_A, dim), dtype=np.float32)
    q = rng.standard_normal((b, dim), dtype=np.float32)
    if dim >= 2048:
        # Gaussian queries cannot certify here: the int8 bound eps ~ 0.024 does not depend on dim, while the gap between the 10th
        # and the ~512th best cosine of 76,877 Gaussian rows is ~1 sigma = 1 / sqrt(dim) -- 0.022 at dim 2048, 0.020 at 2560 (measured:
        # 1 of 33 and 4 of 20 queries took the bf16 pass, which reuses the list buffers).  Each query gets the sum of PLANT rows
        # added: cosine ~ 1 / sqrt(PLANT + 1) = 0.28 with each of them, so its 10th cosine stands far above the threshold, which
        # still is the 64th best of a sample of Gaussian scores: the collect scan sees the same crowd of borderline rows.
        for i in range(b):
            q[i] += x[rng.choice(N_A, PLANT, replace=False)].sum(axis=0)
    idx, L = _search_once(ctx, x, q, dim)
    del x
    assert (L["rows"], L["dim"], L["B"]) == (N_A, dim, b)
    assert L["kernel"] == expected_kernel(dim, b) == getattr(E, "I8_KERNEL_" + kernel), _names().get(L["kernel"], L["kernel"])
    keys = _check_collect(idx, L, device=device)
    assert keys == ctx.stats()["i8_collected"]
    _check_sample(idx, L, device=device)
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ B
def _unsampled_run(t0, t1, length, taken=()):
    """first run of `length` consecutive tiles in [t0, t1) that the threshold pass does not sample and nobody has taken"""
    for t in range(t0, t1 - length + 1):
        run = range(t, t + length)
        if all(u % STEP != 0 and u not in taken for u in run):
            return list(run)
    return None


def _edge_data(dim, b, n_chunks, seed, a_lo=0.3, a_hi=0.9):
    """-> rows, queries, crowd tiles, saturation tiles (module docstring, B)"""
    assert b >= CROWD_Q + 2 * SAT_Q
    rng = np.random.default_rng(seed)
    tiles = (N_B + 255) // 256
    x = rng.standard_normal((N_B, dim), dtype=np.float32)
    q = rng.standard_normal((b, dim), dtype=np.float32)
    crowd = None
    for c in range(n_chunks // 3, n_chunks):                   # a chunk of three tiles or more, away from the ends
        crowd = _unsampled_run(*_chunk_range(tiles, n_chunks, c), 3)
        if crowd:
            break
    assert crowd, "no chunk holds three consecutive unsampled tiles"
    sat = _unsampled_run(1, tiles - 1, 2, taken=crowd)
    # crowd: unit rows at cosine a of the centre
    centre = rng.standard_normal(dim)
    centre /= np.linalg.norm(centre)
    u = rng.standard_normal((3 * 256, dim))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    a = rng.uniform(a_lo, a_hi, 3 * 256)[:, None]
    x[crowd[0] * 256:(crowd[-1] + 1) * 256] = (a * centre + np.sqrt(1.0 - a * a) * u).astype(np.float32)
    q[:CROWD_Q] = (centre + 0.3 / np.sqrt(dim) * rng.standard_normal((CROWD_Q, dim))).astype(np.float32)
    # saturation: sign rows, queries that are copies and negated copies of some of them
    signs = (rng.integers(0, 2, (2 * 256, dim)) * 2 - 1).astype(np.float32) / np.float32(np.sqrt(dim))
    x[sat[0] * 256:(sat[-1] + 1) * 256] = signs
    pick = rng.choice(2 * 256, 2 * SAT_Q, replace=False)
    q[CROWD_Q:CROWD_Q + SAT_Q] = signs[pick[:SAT_Q]]
    q[CROWD_Q + SAT_Q:CROWD_Q + 2 * SAT_Q] = -signs[pick[SAT_Q:]]
    return x, q, crowd, sat


ROUTES_B = [("STREAM_64_32", 1024, 40), ("STREAM_64_16", 512, 40), ("STREAM_128_16", 1024, 100), ("STAGED_64", 768, 40),
            ("STAGED_128", 384, 100), ("DEEP", 512, 200), ("PP", 256, 300)]


@pytest.mark.parametrize("kernel,dim,b", ROUTES_B)
def test_edge_data_every_instantiation(ctx, device, kernel, dim, b):
    from semantic_query_engine_amd import engine as E
    tiles = (N_B + 255) // 256
    qblocks = (b + 255) // 256 if b > 128 else 1
    n_chunks = min(ctx.device_info()["cu_count"] // qblocks, tiles)          # scan.hip: make_scan_plan
    x, q, crowd, sat = _edge_data(dim, b, n_chunks, seed=7_000 * dim + b)
    idx, L = _search_once(ctx, x, q, dim)
    del x
    assert (L["rows"], L["dim"], L["B"], L["n_chunks"]) == (N_B, dim, b, n_chunks)
    assert L["kernel"] == expected_kernel(dim, b) == getattr(E, "I8_KERNEL_" + kernel), _names().get(L["kernel"], L["kernel"])
    assert L["uncertified"] == 0
    probe = {}
    keys = _check_collect(idx, L, device=device, probe=probe)
    assert keys == ctx.stats()["i8_collected"]
    _check_sample(idx, L, device=device)
    # ---- the preconditions: the launch reached every edge this case is about
    bound = min(1 << 23, dim * 127 * 127)
    per_list, per_wave = probe["per_list"], probe["per_wave"]
    pcnt = idx.i8_read(E.I8_POOL_COUNTS, np.int32, L["b_pad"])
    print(f"\n{kernel} ({dim}, {b}): chunks {n_chunks}, crowd tiles {crowd}, saturation tiles {sat}, keys {keys}, "
          f"acc max {probe['acc_max']} ({probe['acc_max'] / bound:.3f}) min {probe['acc_min']} ({probe['acc_min'] / bound:.3f}) of {bound}, "
          f"largest list {per_list.max()} (cap {L['list_cap']}), largest pool {pcnt.max()} (cap {L['pool_cap']}), "
          f"largest wave group {per_wave.max()} (buffer {WAVE_BUF})")
    assert probe["acc_max"] >= 0.88 * bound and probe["acc_min"] <= -0.88 * bound
    assert max(probe["acc_max"], -probe["acc_min"]) < (1 << 23), "quant.hip's norm cap: __mul24 takes 24-bit operands"
    c_full, q_full = np.unravel_index(per_list.argmax(), per_list.shape)
    assert per_list[c_full, q_full] > L["list_cap"] and pcnt[q_full] > 0
    assert _chunk_range(tiles, n_chunks, c_full)[0] <= crowd[0] and crowd[-1] < _chunk_range(tiles, n_chunks, c_full)[1]
    assert pcnt.max() <= L["pool_cap"] and not probe["over"]                   # no pool overflowed: every query was compared
    if kernel.startswith("STREAM"):
        assert per_wave.max() > WAVE_BUF                                       # at least one mid-chunk flush
    idx.close()


# ------------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("kernel,dim,b", [("STAGED_64", 768, 64), ("STAGED_128", 384, 100), ("STREAM_64_32", 1024, 33)])
def test_identical_calls_collect_the_same_keys(ctx, kernel, dim, b):
    from semantic_query_engine_amd import engine as E
    n = 20_000 + 77
    rng = np.random.default_rng(dim + b)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    q = rng.standard_normal((b, dim), dtype=np.float32)
    idx = _i8_index(ctx, dim, 4, M)
    idx.add(x)
    got = []
    for _ in range(2):
        cos, ids = idx.search(q, K_TOP)
        L = idx.i8_last()
        assert L["kernel"] == expected_kernel(dim, b) == getattr(E, "I8_KERNEL_" + kernel)
        assert L["uncertified"] == 0
        kq, key, _, over = _launch_lists(idx, L)
        assert not over
        o = np.lexsort((key, kq))
        got.append((kq[o], key[o], cos, ids))
    assert got[0][0].size > 0
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][2], got[1][2]) and np.array_equal(got[0][3], got[1][3])
    idx.close()
