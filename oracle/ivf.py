"""Float64 and bit-level restatements of the IVF search stages (csrc/ivf.hip, csrc/ivf_scan.hip, csrc/ivf_select.hip, csrc/quant.hip).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  tests/test_ivf_stages_gpu.py reads the state of the last IVF search back
(sqe_index_ivf_state[_read]) and compares it, stage by stage, with what this module computes from the same operands:

    i8_strip            the int8 list scans' estimate, bit for bit (integer dot product, then three float32 products)
    i8_rows_of_lists    the list-ordered int8 copy in its tiled layout, byte for byte
    bf16_strip          the float64 dot product of the bf16 copies (the MFMA scan lies within rounding.acc_term(K) of it)
    collect_reference   the key set of the collect mode for a given threshold, and the rank rule of that threshold
    kmeans_reference    Lloyd on the sphere in float64 from the picks of ivf_train's seeded partial Fisher-Yates
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np

from . import rounding as RD

TILE = 256                    # rows of a tile of the int8 copy
SLICE = 64                    # bytes of a K slice
SLICE_STRIDE = TILE * SLICE   # 16 KiB between the K slices of a tile
IVF_LIST_CAP = 8192           # keys of a query's collect list (ivf_kernels.h)


def tile_stride(dim: int) -> int:
    """Bytes between tiles of the list-ordered int8 copy: dim / 64 slices of 16 KiB and 2 KiB of padding (ivf.hip: ensure_i8_operands)."""
    return (dim // SLICE) * SLICE_STRIDE + 2048


# ------------------------------------------------------------------------------ int8 estimate
def i8_strip(x8_rows: np.ndarray, row_scales: np.ndarray, q8: np.ndarray, q_scale, dim: int) -> np.ndarray:
    """Estimated cosines of int8 rows [n, dim] (integer scales row_scales [n]) against one int8 query [dim] (integer scale
    q_scale) -> float32 [n], or against m queries [m, dim] (scales [m]) -> float32 [n, m], as both int8 list-scan kernels
    compute them.

    acc = <x8, q8> exactly (|acc| <= 127^2 dim; int64 here).  (float)acc is the round-to-nearest-even conversion: int64 -> float64
    is exact below 2^53 and float64 -> float32 rounds to nearest even, which is the single rounding the device's int32 -> float32
    conversion performs.  Then float32(acc) * float32(sxi) * (unit^2 * float32(sqi)), left to right, every product in float32;
    unit^2 is the float32 square of the float32 scale unit."""
    x8 = np.atleast_2d(np.asarray(x8_rows)).astype(np.int64)
    q = np.asarray(q8).astype(np.int64)
    acc = x8 @ (q if q.ndim == 1 else q.T)
    accf = acc.astype(np.float64).astype(np.float32)
    unit = np.float32(RD.i8_scale_unit(dim))
    unit2 = np.float32(unit * unit)
    qs = (unit2 * np.asarray(q_scale).astype(np.uint32).astype(np.float32)).astype(np.float32)
    rs = np.asarray(row_scales).astype(np.uint32).astype(np.float32)
    if q.ndim == 2:
        rs = rs[:, None]
    return ((accf * rs).astype(np.float32) * qs).astype(np.float32)


# ------------------------------------------------------------------------------ list-ordered int8 copy
def tile_offsets(offsets: np.ndarray) -> np.ndarray:
    """Tiles in front of each list: every list starts on a tile -> int64 [nlist + 1]."""
    lens = np.diff(np.asarray(offsets, dtype=np.int64))
    return np.concatenate([[0], np.cumsum((lens + TILE - 1) // TILE)]).astype(np.int64)


def copy_positions(offsets: np.ndarray) -> np.ndarray:
    """Row of the copy (tile * 256 + row in tile) that holds position p of the list-ordered sequence -> int64 [n]."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    toff = tile_offsets(offsets)
    lists = np.repeat(np.arange(lens.size), lens)
    return toff[lists] * TILE + (np.arange(offsets[-1]) - offsets[lists])


def tile_layout(x8: np.ndarray, pos: np.ndarray, total_tiles: int) -> np.ndarray:
    """int8 rows [n, dim] written at copy rows pos [n] in the tiled layout -> int8 [total_tiles, tile_stride]: the 64-byte K slice
    h of tile row r sits at h * 16 KiB + r * 64.  Bytes no row is written to are zero."""
    n, dim = x8.shape
    hs = dim // SLICE
    out = np.zeros((total_tiles, tile_stride(dim)), np.int8)
    body = out[:, :hs * SLICE_STRIDE].reshape(total_tiles, hs, TILE, SLICE)
    body[pos // TILE, :, pos % TILE, :] = x8.reshape(n, hs, SLICE)
    return out


def untile(raw: np.ndarray, pos: np.ndarray, dim: int) -> np.ndarray:
    """The inverse over the rows that exist: int8 [n, dim] read at copy rows pos from a tiled buffer [total_tiles, tile_stride]."""
    hs = dim // SLICE
    tiles = raw.shape[0]
    body = np.ascontiguousarray(raw[:, :hs * SLICE_STRIDE]).reshape(tiles, hs, TILE, SLICE)
    return body[pos // TILE, :, pos % TILE, :].reshape(pos.size, dim)


def i8_rows_of_lists(xn: np.ndarray, order: np.ndarray, offsets: np.ndarray, scales: np.ndarray | None = None
                     ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The list-ordered int8 copy of normalised rows xn: position p of the list-ordered sequence is row order[p], quantised with
    its OWN scale (rounding.i8_row_scales / i8_quantize), laid out in tiles where every list starts on a tile.
    -> (tiled int8 [total_tiles, tile_stride], scales uint32 [total_tiles * 256] (0 where no row sits), copy rows pos [n]).
    `scales` (optional, [n] by position) replaces the computed scales: see scale_boundary."""
    xn = np.atleast_2d(np.asarray(xn, dtype=np.float32))
    rows = xn[np.asarray(order, dtype=np.int64)]
    sx = RD.i8_row_scales(rows) if scales is None else np.asarray(scales, dtype=np.uint32)
    x8 = RD.i8_quantize(rows, sx)
    pos = copy_positions(offsets)
    total = int(tile_offsets(offsets)[-1])
    tiled = tile_layout(x8, pos, total)
    sc = np.zeros(total * TILE, np.uint32)
    sc[pos] = sx
    return tiled, sc, pos


def scale_boundary(xn_rows: np.ndarray) -> np.ndarray:
    """Rows whose integer scale float32 arithmetic cannot pin down: the scale is ceil(t), t = need / S0 * 1.000001, and the kernel
    evaluates t in float32 -- one rounding each for max|x| / 127 (or two and a 256-term sum for ||x|| / 2800), the division by S0
    and the product, at most 4 * 2^-24 relative together for rows whose largest element sets the scale, 2^-24 (dim / 2 + 4) for
    the others.  Where the float64 t lies within that of an integer the device may round to either side, and only there."""
    xn_rows = np.atleast_2d(np.asarray(xn_rows, dtype=np.float32))
    dim = xn_rows.shape[1]
    need = RD.i8_need(xn_rows)
    t = need / RD.i8_scale_unit(dim) * 1.000001
    by_norm = np.sqrt((xn_rows.astype(np.float64) ** 2).sum(axis=1)) / RD.I8_NORM_CAP >= np.abs(xn_rows).max(axis=1) / 127.0 * (1 - 1e-6)
    rel = np.where(by_norm, (dim / 2 + 4) * 2.0 ** -24, 4 * 2.0 ** -24)
    return np.abs(t - np.rint(t)) <= t * rel


# ------------------------------------------------------------------------------ bf16 estimate
def bf16_strip(rows_bf16: np.ndarray, q_bf16: np.ndarray) -> np.ndarray:
    """Float64 dot products of bf16 rows [n, dim] (bit patterns, as read back) with one bf16 query [dim] -> float64 [n], or with
    m queries [m, dim] -> float64 [n, m]."""
    r = RD.bf16_to_f32(np.atleast_2d(rows_bf16)).astype(np.float64)
    q = RD.bf16_to_f32(q_bf16).astype(np.float64)
    return r @ (q if q.ndim == 1 else q.T)


# ------------------------------------------------------------------------------ collect mode
def f32_orderable(v: np.ndarray) -> np.ndarray:
    """float32 -> uint32 whose unsigned order is the float order (common.h)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def make_keys(scores: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """(orderable(score) << 32) | (0xFFFFFFFF - row) (common.h: make_key)."""
    return (f32_orderable(scores).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(rows).astype(np.uint64))


def collect_reference(estimates: List[np.ndarray], row_ids: List[np.ndarray], threshold: float) -> np.ndarray:
    """Keys of one query's collect list for the threshold the device reports: every (estimate bits, row id) over ALL rows of the
    probed lists -- sample tile and other tiles alike -- with estimate >= threshold; NaN estimates never enter.
    estimates / row_ids: one float32 / integer array per probed list.  -> sorted uint64 keys."""
    est = np.concatenate([np.asarray(e, dtype=np.float32) for e in estimates]) if estimates else np.zeros(0, np.float32)
    ids = np.concatenate([np.asarray(r, dtype=np.int64) for r in row_ids]) if row_ids else np.zeros(0, np.int64)
    est = (est + np.float32(0.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        keep = ~np.isnan(est) & (est >= np.float32(threshold))
    return np.sort(make_keys(est[keep], ids[keep]))


def collect_want(S: int, total: int, kp: int) -> int:
    """Rank (1 = largest) of the sample score that ivf_threshold_kernel takes as threshold; 0: the probed set is at most
    IVF_LIST_CAP / 4 rows (or the sample is empty) and the threshold is -inf."""
    if total <= IVF_LIST_CAP // 4 or S <= 0:
        return 0
    t = 8.0 * kp * S / total
    return min(S, int(t + 3.0 * math.sqrt(t) + 2.0))


def threshold_rank_ok(sample: np.ndarray, threshold: float, want: int) -> bool:
    """The threshold is one of the sample scores and its rank is within +-1 of `want` (the device evaluates `want` in float32,
    possibly fused: at a truncation boundary it may land one off, nothing more).  With ties the threshold holds the ranks
    (scores above it) + 1 .. (scores at or above it)."""
    s = np.asarray(sample, dtype=np.float32)
    s = s[~np.isnan(s)]
    thr = np.float32(threshold)
    gt, ge = int((s > thr).sum()), int((s >= thr).sum())
    if ge == gt:
        return False                                   # not a sample score
    return any(gt < w <= ge for w in (want - 1, want, want + 1))


# ------------------------------------------------------------------------------ k-means
_M64 = (1 << 64) - 1


def splitmix(state: int) -> Tuple[int, int]:
    """One step of splitmix64 -> (new state, output)."""
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def train_picks(n: int, nlist: int, seed: int) -> np.ndarray:
    """Rows ivf_train starts its centroids from: a partial Fisher-Yates of 0 .. n-1 driven by splitmix64(seed ^ 0x5eed5eed)."""
    perm = list(range(n))
    state = (seed ^ 0x5EED5EED) & _M64
    for i in range(nlist):
        state, r = splitmix(state)
        j = i + r % (n - i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.asarray(perm[:nlist], dtype=np.int64)


def assign_best(x64: np.ndarray, cent64: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """arg-max cosine with ties to the lowest list id -> (list, runner-up list, gap between the two best cosines)."""
    s = x64 @ cent64.T
    best = np.argmax(s, axis=1)                        # first maximum: lowest id
    top = s[np.arange(s.shape[0]), best]
    s2 = s.copy()
    s2[np.arange(s.shape[0]), best] = -np.inf
    second = np.argmax(s2, axis=1)
    gap = top - s2[np.arange(s.shape[0]), second] if cent64.shape[0] > 1 else np.full(s.shape[0], np.inf)
    return best, second, gap


def kmeans_reference(xn: np.ndarray, picks: np.ndarray, iters: int) -> List[Dict[str, np.ndarray]]:
    """Lloyd on the sphere in float64 from centroids xn[picks]: assign every row to its arg-max cosine (ties to the lowest list
    id), centroid = sum / (||sum|| + 1e-9), a list nobody is assigned to keeps its centroid.  One record per iteration:
    assign, second, gap (assign_best against the centroids the iteration started from), counts, sums, abs_sums (sum of |x| per
    component: the scale of the fp32 summation bound) and the centroids it produced."""
    x64 = np.asarray(xn).astype(np.float64)
    cent = x64[np.asarray(picks, dtype=np.int64)].copy()
    nlist = cent.shape[0]
    out = []
    for _ in range(max(1, iters)):
        best, second, gap = assign_best(x64, cent)
        counts = np.bincount(best, minlength=nlist)
        sums = np.zeros_like(cent)
        abs_sums = np.zeros_like(cent)
        np.add.at(sums, best, x64)
        np.add.at(abs_sums, best, np.abs(x64))
        new = cent.copy()
        live = counts > 0
        new[live] = sums[live] / (np.sqrt((sums[live] ** 2).sum(axis=1, keepdims=True)) + 1e-9)
        cent = new
        out.append({"assign": best, "second": second, "gap": gap, "counts": counts, "sums": sums, "abs_sums": abs_sums,
                    "centroids": cent.copy()})
    return out
