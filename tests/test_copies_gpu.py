"""The scanned copies and the measured residuals against a float64 restatement (oracle/rounding.py).

Every certificate, collect threshold and radial cut-off in the library trusts four measured numbers -- the bf16 and int8
rounding residuals of the query and of the worst stored row -- and the copies they were measured on.  The end-to-end tests
cannot see them: the fp32 re-score, the certificate and the fallback mask a wrong copy or an under-measured residual on
benign data.  Here they are read back (sqe_index_state_read, sqe_index_i8_read) and checked directly:

  fp32 rows   against float64 x / (||x|| + 1e-9): relative error <= (dim / 128 + 6) * 2^-24 -- the worst case of dim / 64
              sequential fp32 adds per lane, the product rounding and six tree levels, halved by the square root, plus one
              rounding each for the + 1e-9 and the division.  A dropped element shows as ~1 / dim.
  bf16 copy   bit-equal to bf16_round of the library's own fp32 rows; rows past the end are zero.
  residuals   measured >= float64 always; on a fresh index also <= 1.0002 * float64 + 2e-7 (the kernel's own factor 1.0001 and
              its fp32 sum's rounding, <= 5e-6 at dim 8192, are well inside).  The index maxima only grow, so after updates
              and deletes only the lower bound holds.
  int8 copy   as properties (equality with a float32 restatement would hinge on ties at half-integers): see _check_i8.

after each write path: add, update (scatter form), delete + add (compaction), save + load (restore form)."""
import os

import numpy as np
import pytest

from oracle import retrieval as R
from oracle import rounding as RD

from . import rounding_cases as RC
from .gpu_util import assert_topk_matches

pytestmark = pytest.mark.gpu

DIMS = [64, 256, 320, 512, 576, 1024, 1088, 2048, 2112, 8192]      # NV = 1, 1, 2, 2, 4, 4, 8, 8, 0, 0 of normalize_rows_kernel
I8_DIMS = [256, 512, 1024, 2048, 8192]
ROWS = 1553            # 6 tiles + 17: a partial last tile, more rows than one wave per row in a 4-wave block
REGULAR = slice(0, 6)  # EDGE_NAMES whose int8 residual is ordinary (one_hot and one_large quantise badly: test 9)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _rows_for(dim):
    return 300 if dim == 8192 else ROWS


def _f64_normalize(x):
    x64 = x.astype(np.float64)
    return x64 / (np.sqrt((x64 * x64).sum(axis=1, keepdims=True)) + 1e-9)


def _resid_max(idx, what):
    from semantic_query_engine_amd import engine as E
    return float(idx.state_read(what, np.float32, 1)[0])


def _check_fp32(got, raw, edge_pos):
    """got: the library's rows (get_rows); raw: what was added at the same positions; edge_pos: positions of edge rows"""
    dim = raw.shape[1]
    bound = (dim / 128 + 6) * 2.0 ** -24
    regular = np.ones(raw.shape[0], bool)
    regular[edge_pos] = False
    ref = _f64_normalize(raw[regular])
    err = np.abs(got[regular].astype(np.float64) - ref)
    worst = (err / np.maximum(np.abs(ref), 1e-300)).max()
    print(f"dim {dim}: fp32 rows, worst relative error {worst / 2.0 ** -24:.2f} x 2^-24 (bound {dim / 128 + 6:.1f})")
    assert np.all(err <= bound * np.abs(ref))
    if len(edge_pos):
        with np.errstate(all="ignore"):
            ref32 = R.normalize_rows(raw[edge_pos])
        g = got[edge_pos]
        assert np.array_equal(np.isnan(g), np.isnan(ref32)) and np.array_equal(np.isinf(g), np.isinf(ref32))
        assert np.array_equal(g == 0, ref32 == 0)
        fin = np.isfinite(ref32)
        assert np.all(np.abs(g[fin].astype(np.float64) - ref32[fin]) <= bound * np.abs(ref32[fin].astype(np.float64)) + 1e-37)


def _check_bf16(idx, got, fresh):
    """bf16 copy bit-equal to bf16_round(library fp32 rows), zero past the end, resid_max against float64"""
    from semantic_query_engine_amd import engine as E
    n = got.shape[0]
    copy = idx.scan_bf16()
    assert copy.shape == ((n + 255) // 256 * 256, got.shape[1])
    assert np.array_equal(copy[:n], RD.bf16_round(got))
    assert not copy[n:].any()
    resid = RD.bf16_residual(got)
    true_max = float(np.nanmax(resid))                       # NaN rows are left out, as the kernel leaves them out
    measured = _resid_max(idx, E.STATE_RESID_MAX)
    print(f"dim {got.shape[1]}: bf16 resid_max {measured:.6e}, float64 {true_max:.6e}, ratio {measured / true_max:.6f}")
    assert measured >= true_max
    if fresh:
        assert measured <= 1.0002 * true_max + 2e-7
    return measured


def _check_query_residuals(idx, q, i8=False):
    from semantic_query_engine_amd import engine as E
    dim, B = q.shape[1], q.shape[0]
    st = idx.state()
    assert st["last_B"] == B and st["last_i8"] == int(i8)
    qn = idx.state_read(E.STATE_QN, np.float32, B * dim).reshape(B, dim)
    bound = (dim / 128 + 6) * 2.0 ** -24
    ref = _f64_normalize(q)
    assert np.all(np.abs(qn.astype(np.float64) - ref) <= bound * np.abs(ref))
    measured = idx.state_read(E.STATE_Q_RESID, np.float32, B).astype(np.float64)
    true = RD.bf16_residual(qn)
    assert np.all(measured >= true) and np.all(measured <= 1.0002 * true + 2e-7)
    return qn


def _untiled_i8(idx, n):
    from semantic_query_engine_amd import engine as E
    st = idx.state()
    assert st["i8_rows"] == n and st["i8_tile_stride"] > 0, st
    tiles, stride, hs = (n + 255) // 256, st["i8_tile_stride"], st["dim"] // 64
    raw = idx.i8_read(E.I8_ROWS, np.int8, tiles * stride).reshape(tiles, stride)[:, :hs * 256 * 64].reshape(tiles, hs, 256, 64)
    x8 = np.ascontiguousarray(raw.transpose(0, 2, 1, 3)).reshape(tiles * 256, st["dim"])
    sxi = idx.i8_read(E.I8_ROW_SCALES, np.uint32, tiles * 256)
    return x8, sxi


def _check_scaled_rows(xn, x8, sxi, per_tile):
    """properties 2 - 6 for rows xn (library fp32), their int8 copy x8 and integer scales sxi (per row); per_tile: the scale
    is shared by 256-row tiles (stored rows) or per row (queries).  -> float64 residual per row (NaN for non-finite rows)"""
    n, dim = xn.shape
    s0 = RD.i8_scale_unit(dim)
    assert sxi.min() >= 1 and sxi.max() <= 65535                                            # 1
    s = sxi.astype(np.float64) * s0
    fin = RD.i8_finite_rows(xn)
    x64 = xn.astype(np.float64)
    with np.errstate(all="ignore"):
        assert np.all(127.0 * s[fin] >= np.abs(x64[fin]).max(axis=1))                       # 2: the scale covers the row
        assert np.all(np.sqrt((x64[fin] ** 2).sum(axis=1)) / s[fin] <= 2800.0 * (1 + 2e-6))
        need = RD.i8_need(xn)
        if per_tile:
            tiles = (n + 255) // 256
            padded = np.zeros(tiles * 256)
            padded[:n] = need
            need = np.repeat(padded.reshape(tiles, 256).max(axis=1), 256)[:n]               # 5: non-finite rows count as 0
        above_one = sxi > 1
        assert np.all((sxi[above_one] - 1.0) * s0 < need[above_one] * (1 + 3e-6))           # 3: the scale is minimal
        assert x8.min() >= -127                                                             # 4: rounded to nearest, clamped
        assert np.all(np.abs(x64[fin] / s[fin, None] - x8[fin]) <= 0.5 + 1e-4)
        assert not x8[~fin].any()                                                           # 5: NaN / inf rows are zero vectors
        assert np.all(np.sqrt((x8.astype(np.float64) ** 2).sum(axis=1)) <= 2800.0 + 0.5 * np.sqrt(dim) + 1.0)   # 6
        resid = RD.i8_residual(xn, x8, sxi)
    resid[~fin] = np.nan
    return resid


def _check_i8(idx, got, fresh):
    """The int8 copy of the stored rows, stated as properties:
    1 one scale per tile, 1 <= sxi <= 65535; 2 the scale covers every finite row of the tile (127 s >= max|x|, ||x|| / s <= 2800);
    3 it is minimal; 4 elements are rounded to nearest and clamped to +-127; 5 NaN / inf rows are zero and do not raise the scale;
    6 ||x8|| <= 2800 + 0.5 sqrt(dim) + 1 (every dot product stays below 2^23); rows past the end are zero;
    8 i8resid_max >= float64 max residual, and <= 1.0002 * that + 2.1e-7 on a fresh index."""
    from semantic_query_engine_amd import engine as E
    n = got.shape[0]
    x8, sxi = _untiled_i8(idx, n)
    assert np.array_equal(sxi.reshape(-1, 256), np.repeat(sxi[::256, None], 256, 1))        # 1
    assert not x8[n:].any()
    resid = _check_scaled_rows(got, x8[:n], sxi[:n], per_tile=True)
    true_max = float(np.nanmax(resid))
    measured = _resid_max(idx, E.STATE_I8_RESID_MAX)
    print(f"dim {got.shape[1]}: int8 i8resid_max {measured:.6e}, float64 {true_max:.6e}, ratio {measured / true_max:.6f}")
    assert measured >= true_max                                                             # 8
    if fresh:
        assert measured <= 1.0002 * true_max + 2.1e-7
    return measured


def _check_i8_queries(idx, qn):
    """7: the quantised queries and their scales satisfy properties 2 - 4 per row; q8resid against float64"""
    from semantic_query_engine_amd import engine as E
    B, dim = qn.shape
    L = idx.i8_last()
    assert (L["B"], L["dim"]) == (B, dim)
    q8 = idx.i8_read(E.I8_QUERIES, np.int8, L["b_pad"] * L["q_pitch"]).reshape(L["b_pad"], L["q_pitch"])
    assert not q8[B:].any()
    sqi = idx.state_read(E.STATE_Q8_SCALES, np.uint32, B)
    resid = _check_scaled_rows(qn, q8[:B, :dim], sqi, per_tile=False)
    measured = idx.state_read(E.STATE_Q8_RESID, np.float32, B).astype(np.float64)
    assert np.all(measured >= resid) and np.all(measured <= 1.0002 * resid + 2.1e-7)


def _queries(dim, B, one_hot=True):
    q, _ = RC.copies_case(dim, B, seed=B, edges=False)
    if B >= 5:
        if one_hot:
            q[1] = 0.0; q[1, dim // 2] = 3.0        # one-hot: bf16-exact, residual 0
        q[B - 1] *= np.float32(1e-12)
    return q


def _write_paths(idx, x, edge_pos, rng, one_hot=True):
    """The other write paths, one after the other; after each yields (label, {live id: the raw row it holds}, ids that hold
    an edge row)."""
    n, dim = x.shape
    raw = {i: x[i] for i in range(n)}
    edges = set(int(i) for i in edge_pos)
    # update of 40 rows (the scatter form): two ids in one tile, one id twice (same data both times: the scatter has no order)
    a = 256 + 17
    others = rng.choice(np.setdiff1d(np.arange(n), [a, a + 1]), 37, replace=False)
    upd = np.concatenate([[a, a + 1], others, [a]])
    new = (rng.standard_normal((40, dim)) * rng.uniform(0.01, 50.0, (40, 1))).astype(np.float32)
    if one_hot:
        new[1] = 0.0; new[1, 3] = 7.0                # a one-hot row arrives by update
    new[39] = new[0]
    idx.update(upd, new)
    for i, r in zip(upd, new):
        raw[int(i)] = r
        edges.discard(int(i))
    yield "update", raw, edges
    # delete of 200 scattered ids plus the first and the last row (compaction), then add of 300 rows
    gone = np.unique(np.concatenate([rng.choice(np.arange(1, n - 1), min(200, n - 60), replace=False), [0, n - 1]]))
    idx.delete(gone)
    for i in gone:
        del raw[int(i)]
        edges.discard(int(i))
    more = (rng.standard_normal((300, dim)) * rng.uniform(0.01, 50.0, (300, 1))).astype(np.float32)
    idx.add(more)
    for j in range(300):
        raw[n + j] = more[j]
    yield "delete+add", raw, edges


def _by_position(idx, raw):
    ids = idx.ids()
    assert sorted(raw) == ids.tolist()
    return ids, np.stack([raw[int(i)] for i in ids])


@pytest.mark.parametrize("dim", DIMS)
def test_fp32_rows_bf16_copy_and_residual_after_every_write_path(ctx, dim, tmp_path):
    from semantic_query_engine_amd import SCAN_BF16_RESCORE, VectorIndex
    from semantic_query_engine_amd import engine as E
    n = _rows_for(dim)
    x, edge_pos = RC.copies_case(dim, n)
    rng = np.random.default_rng(dim)
    idx = VectorIndex(ctx, dim)
    idx.set_option("scan_mode", SCAN_BF16_RESCORE)
    idx.add(x)
    got = idx.get_rows(np.arange(n))
    _check_fp32(got, x, edge_pos)
    fresh_max = _check_bf16(idx, got, fresh=True)
    # save + load of an index without updates or deletes: same rows, same copy, the same residual bit for bit
    path = os.path.join(tmp_path, "fresh.sqe")
    idx.save(path)
    loaded = VectorIndex.load(ctx, path)
    got_l = loaded.get_rows(np.arange(n))
    assert np.array_equal(got_l.view(np.uint32), got.view(np.uint32))
    assert _check_bf16(loaded, got_l, fresh=True) == fresh_max
    loaded.close()
    # per-query residuals (the query form of the same kernel: resid_rows instead of resid_max)
    for B in (1, 5, 64, 130):
        q = _queries(dim, B)
        idx.search(q, 10)
        _check_query_residuals(idx, q)
    for label, raw, edges in _write_paths(idx, x, edge_pos, rng):
        ids, rows = _by_position(idx, raw)
        got = idx.get_rows(ids)
        print(label)
        _check_fp32(got, rows, np.nonzero(np.isin(ids, sorted(edges)))[0])
        _check_bf16(idx, got, fresh=False)
    path = os.path.join(tmp_path, "holes.sqe")
    idx.save(path)
    loaded = VectorIndex.load(ctx, path)
    assert np.array_equal(loaded.ids(), ids)
    got_l = loaded.get_rows(ids)
    assert np.array_equal(got_l.view(np.uint32), got.view(np.uint32))
    _check_bf16(loaded, got_l, fresh=True)               # the restore form measures the live rows anew
    loaded.close()
    idx.close()


def _i8_index(ctx, dim):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    idx = VectorIndex(ctx, dim)
    idx.set_option("scan_mode", SCAN_INT8_RESCORE)
    idx.set_option("i8_min_rows", 0)
    idx.set_option("i8_sample_step", 1)
    return idx


@pytest.mark.parametrize("dim", I8_DIMS)
def test_int8_copy_scales_and_residuals_after_every_write_path(ctx, dim):
    """The int8 first pass answers an index of >= 1024 rows (four whole tiles for its threshold pass), so dim 8192 runs 1100
    rows here where the bf16 test runs 300: four tiles and a partial fifth."""
    n = 1100 if dim == 8192 else ROWS
    x, edge_pos = RC.copies_case(dim, n, seed=1, edges=False)
    edge_pos = np.array([0, 5, n // 2, n // 2 + 1, n - 2, n - 1])
    x[edge_pos] = RC.edge_rows(dim)[REGULAR]
    rng = np.random.default_rng(dim + 1)
    idx = _i8_index(ctx, dim)
    idx.add(x)
    fresh = True
    for B in (1, 5, 64, 130):
        q = _queries(dim, B, one_hot=False)
        idx.search(q, 10)
        qn = _check_query_residuals(idx, q, i8=True)
        _check_i8_queries(idx, qn)
        if fresh:
            _check_i8(idx, idx.get_rows(np.arange(n)), fresh=True)
            fresh = False
    for label, raw, _ in _write_paths(idx, x, edge_pos, rng, one_hot=False):   # (a one-hot row would send the index to bf16: test 9)
        ids, _ = _by_position(idx, raw)
        idx.search(_queries(dim, 5, one_hot=False), 10)   # re-quantises what the write path left stale
        assert idx.state()["last_i8"] == 1, label
        print(label)
        _check_i8(idx, idx.get_rows(ids), fresh=False)
    idx.close()


def test_rows_that_quantise_badly_answer_in_bf16_and_stay_readable(ctx):
    """9: one one-hot-like row inside a Gaussian tile (residual above "i8_max_resid" = 0.02): the index builds its int8 copy,
    answers with the bf16 scan, and the copy and its scales can still be read and hold properties 1 - 6 and 8."""
    from semantic_query_engine_amd import engine as E
    dim, n = 256, 1100
    x, _ = RC.copies_case(dim, n, seed=9, edges=False)
    x[700] = 0.01 * x[700]
    x[700, 11] = 100.0
    idx = _i8_index(ctx, dim)
    idx.add(x)
    q = _queries(dim, 5)
    ctx.stats_reset()
    cos, ids = idx.search(q, 10)
    ref_cos, ref_ids = R.knn_search(x, q, 10)
    assert_topk_matches(cos, ids, ref_cos, ref_ids, R.normalize_rows(x), R.normalize_rows(q))
    st = idx.state()
    assert st["last_i8"] == 0 and st["i8_rows"] == n
    with pytest.raises(Exception):
        idx.i8_last()                                     # no search was answered by the int8 first pass
    measured = _check_i8(idx, idx.get_rows(np.arange(n)), fresh=True)
    assert measured > 0.02
    idx.close()
