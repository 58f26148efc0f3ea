"""NumPy restatement of the roundings behind the exactness certificate.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Every search proves "no row outside the re-scored set can reach the
k-th cosine" from one inequality,

    |scan score - fp32 cosine| <= scan_eps(dq, dx, K)                      (csrc/kernels.h)

whose inputs are measured by the library: dq / dx = || v - copy(v) ||_2 of the query / the worst stored row, for the bf16
copies (csrc/normalize.hip) and the int8 copies (csrc/quant.hip).  This module restates the two roundings and the bound so
that tests can check the measured inputs against float64: the copies element by element, the residuals as norms, the
bound row by row.  Residuals and dot products are float64 throughout.
"""
from __future__ import annotations

import numpy as np

# ------------------------------------------------------------------------------ bf16
def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns (uint16), round to nearest even, NaN -> quiet NaN keeping sign and high payload:
    csrc/common.h f32_to_bf16, bit for bit."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    r = np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), r)
    return r.astype(np.uint16)


def bf16_to_f32(b: np.ndarray) -> np.ndarray:
    """bf16 bit patterns -> the float32 values they stand for (exact)."""
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_residual(x: np.ndarray) -> np.ndarray:
    """|| x_r - bf16(x_r) ||_2 per row in float64 (NaN for a row that holds a NaN or an inf)."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        e = x.astype(np.float64) - bf16_to_f32(bf16_round(x)).astype(np.float64)
        return np.sqrt((e * e).sum(axis=1))


# ------------------------------------------------------------------------------ int8
I8_TILE_ROWS = 256
I8_NORM_CAP = 2800.0


def i8_scale_unit(dim: int) -> float:
    """S0 = 4 / (127 * 160 * sqrt(dim)), evaluated in float32 as csrc/quant.hip does; a row scale is sxi * S0."""
    return float(np.float32(4.0) / (np.float32(127.0) * np.float32(160.0) * np.sqrt(np.float32(dim))))


def i8_finite_rows(xn: np.ndarray) -> np.ndarray:
    """Rows the quantiser treats as finite: no NaN, largest magnitude below 3e38 (the others become zero vectors)."""
    xn = np.atleast_2d(np.asarray(xn, dtype=np.float32))
    with np.errstate(invalid="ignore"):
        return ~np.isnan(xn).any(axis=1) & (np.abs(xn).max(axis=1) < np.float32(3.0e38))


def i8_need(row: np.ndarray) -> np.ndarray:
    """Smallest scale a row admits: max(max|x| / 127, ||x|| / 2800) in float64; 0 for a non-finite row.  Rows of a 2-d input."""
    x = np.atleast_2d(np.asarray(row, dtype=np.float32)).astype(np.float64)
    fin = i8_finite_rows(row)
    with np.errstate(invalid="ignore", over="ignore"):
        need = np.maximum(np.abs(x).max(axis=1) / 127.0, np.sqrt((x * x).sum(axis=1)) / I8_NORM_CAP)
    return np.where(fin, need, 0.0)


def i8_scale_of(need: np.ndarray, dim: int) -> np.ndarray:
    """need -> integer scale: ceil(need / S0 * 1.000001) clamped to [1, 65535]."""
    s = np.ceil(np.asarray(need, dtype=np.float64) / i8_scale_unit(dim) * 1.000001)
    return np.clip(s, 1, 65535).astype(np.uint32)


def i8_tile_scales(xn: np.ndarray, n_rows: int | None = None) -> np.ndarray:
    """One integer scale per 256-row tile, the largest its first n_rows rows need -> uint32 [rows], repeated over each tile."""
    xn = np.atleast_2d(np.asarray(xn, dtype=np.float32))
    n_rows = xn.shape[0] if n_rows is None else n_rows
    need = i8_need(xn[:n_rows])
    tiles = (n_rows + I8_TILE_ROWS - 1) // I8_TILE_ROWS
    padded = np.zeros(tiles * I8_TILE_ROWS)
    padded[:n_rows] = need
    per_tile = i8_scale_of(padded.reshape(tiles, I8_TILE_ROWS).max(axis=1), xn.shape[1])
    return np.repeat(per_tile, I8_TILE_ROWS)[:n_rows]


def i8_row_scales(qn: np.ndarray) -> np.ndarray:
    """One integer scale per row (the query form)."""
    qn = np.atleast_2d(np.asarray(qn, dtype=np.float32))
    return i8_scale_of(i8_need(qn), qn.shape[1])


def i8_quantize(xn: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """x8 = clamp(rint(x / (sxi * S0)), -127, 127) with the division in float32 and ties to even, as the kernel computes it;
    non-finite rows are zero vectors."""
    xn = np.atleast_2d(np.asarray(xn, dtype=np.float32))
    s = (np.asarray(scales).astype(np.float32) * np.float32(i8_scale_unit(xn.shape[1])))[:, None]
    fin = i8_finite_rows(xn)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.rint(np.where(fin[:, None], xn, np.float32(0)) / s), -127, 127)
    return q.astype(np.int8)


def i8_residual(xn: np.ndarray, x8: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """|| x_r - sxi S0 x8_r ||_2 per row in float64."""
    xn = np.atleast_2d(np.asarray(xn, dtype=np.float32))
    s = np.asarray(scales).astype(np.float64)[:, None] * i8_scale_unit(xn.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        e = xn.astype(np.float64) - s * np.asarray(x8).astype(np.float64)
        return np.sqrt((e * e).sum(axis=1))


# ------------------------------------------------------------------------------ the bound
def acc_term(K: int) -> float:
    """The share of scan_eps that covers the two fp32 accumulation chains the bound compares (kernels.h)."""
    return float(max(np.float32(2.0e-4), np.float32(K) * np.float32(1.1920929e-7) * np.float32(1.05)))


def scan_eps(dq, dx, K: int):
    """kernels.h scan_eps in float32 arithmetic: (1 + dq) dx 1.000001 + dq 1.000001 + acc_term(K)."""
    dq, dx = np.asarray(dq, dtype=np.float32), np.asarray(dx, dtype=np.float32)
    one = np.float32(1.000001)
    return (np.float32(1.0) + dq) * dx * one + dq * one + np.float32(acc_term(K))
