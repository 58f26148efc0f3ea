"""The checker of the bit-exact int8 tests catches what it claims to catch (tests/test_i8_exact_gpu.py: _check_collect).

A NumPy stand-in for an index answers i8_last / i8_read the way the library does -- the tiled int8 copy and its tile scales from
oracle/rounding.py's quantiser, the row-major quantised queries, thresholds, (chunk, query) lists with the documented key packing
(include/sqe.h: SQE_I8_LISTS) and the overflow pools -- after a "launch" computed in plain integer arithmetic.  _check_collect
passes on it, and fails on each single seeded fault of the kind a wrong kernel would produce.  No GPU."""
import numpy as np
import pytest

from oracle import rounding as R
from tests.test_i8_exact_gpu import _check_collect, _chunk_range

ROWS, DIM, B, B_PAD = 1024 - 77, 256, 16, 64           # four tiles, the last one partial
TILE_ROWS, N_CHUNKS, LIST_CAP, POOL_CAP, M = 256, 3, 4, 256, 24
TILE_STRIDE = TILE_ROWS * DIM + 256                     # (the library pads a tile too: the checker must go by tile_stride)
Q_PITCH = DIM + 128


def _key(score, row):
    return (np.uint64((int(score) & 0xFFFFFFFF) ^ 0x80000000) << np.uint64(32)) | np.uint64(0xFFFFFFFF - int(row))


class FakeIndex:
    """fault: None or one of FAULTS -- what the stand-in's launch gets wrong"""

    def __init__(self, fault=None):
        from semantic_query_engine_amd import engine as E
        rng = np.random.default_rng(5)
        tiles = (ROWS + TILE_ROWS - 1) // TILE_ROWS
        x = rng.standard_normal((ROWS, DIM)).astype(np.float32)
        q = rng.standard_normal((B, DIM)).astype(np.float32)
        # tile 1: sign rows, whose tile scale is small (41 against ~180).  An unsigned 24-bit multiply adds (scale & 255) << 24 to the
        # product of a negative accumulator: only where that lands above the threshold -- (scale & 255) < 128 -- does a key appear
        x[TILE_ROWS:2 * TILE_ROWS] = (rng.integers(0, 2, (TILE_ROWS, DIM)) * 2 - 1).astype(np.float32)
        xn = np.zeros((tiles * TILE_ROWS, DIM), np.float32)            # rows past ROWS are zero vectors (quant.hip)
        xn[:ROWS] = x / np.linalg.norm(x, axis=1, keepdims=True)
        qn = q / np.linalg.norm(q, axis=1, keepdims=True)
        scales = np.repeat(R.i8_tile_scales(xn, ROWS)[::TILE_ROWS], TILE_ROWS).astype(np.uint32)       # one per tile, on each of its rows
        x8 = R.i8_quantize(xn, scales)
        q8 = np.zeros((B_PAD, Q_PITCH), np.int8)
        q8[:B, :DIM] = R.i8_quantize(qn, R.i8_row_scales(qn))
        tiled = np.zeros((tiles, TILE_STRIDE), np.int8)
        tiled[:, : TILE_ROWS * DIM] = x8.reshape(tiles, TILE_ROWS, DIM // 64, 64).transpose(0, 2, 1, 3).reshape(tiles, -1)
        # ---- the launch
        xs = x8.astype(np.int64)
        acc = xs @ q8[:B, :DIM].astype(np.int64).T
        score = acc * scales[:, None].astype(np.int64)
        thr = np.full(B_PAD, 0x7FFFFFFF, np.int32)                      # padding queries collect nothing
        thr[:B] = -np.sort(-score[:ROWS], axis=0)[M - 1]                # ~M keys per query
        if fault == "stale_slice":                                     # one collected row: its last 64-byte K slice zeroed before the product
            stale_row = int(np.nonzero(score[:ROWS, 0] >= thr[0])[0][0])
            xs[stale_row, DIM - 64:] = 0
            score = (xs @ q8[:B, :DIM].astype(np.int64).T) * scales[:, None].astype(np.int64)
        if fault == "unsigned_mul24":                                  # the low 24 bits of acc taken as unsigned, the low 32 of the product kept
            prod = ((acc & 0xFFFFFF) * scales[:, None].astype(np.int64)) & 0xFFFFFFFF
            score = np.where(prod >= (1 << 31), prod - (1 << 32), prod)
            assert np.array_equal(score[acc >= 0], (acc * scales[:, None].astype(np.int64))[acc >= 0]) and 0 < (scales[TILE_ROWS] & 255) < 128
        cnt = np.zeros((N_CHUNKS, B_PAD), np.int32)
        lists = np.zeros((N_CHUNKS, B_PAD, LIST_CAP), np.uint64)
        pcnt = np.zeros(B_PAD, np.int32)
        pools = np.zeros((B_PAD, POOL_CAP), np.uint64)

        def append(c, qi, key):
            if cnt[c, qi] < LIST_CAP:
                lists[c, qi, cnt[c, qi]] = key
            else:
                if pcnt[qi] < POOL_CAP:
                    pools[qi, pcnt[qi]] = key
                pcnt[qi] += 1
            cnt[c, qi] += 1

        dropped = moved = shifted = False
        for c in range(N_CHUNKS):
            t0, t1 = _chunk_range(tiles, N_CHUNKS, c)
            for r in range(t0 * TILE_ROWS, min(t1 * TILE_ROWS, ROWS)):
                for qi in np.nonzero(score[r] >= thr[:B])[0]:
                    if fault == "dropped_key" and not dropped:
                        dropped = True
                        continue
                    if fault == "wrong_chunk" and not moved:
                        moved = True
                        append(c + 1, qi, _key(score[r, qi], r))
                        continue
                    if fault == "row_off_by_one" and not shifted:
                        shifted = True
                        append(c, qi, _key(score[r, qi], r + 1))
                        continue
                    append(c, qi, _key(score[r, qi], r))
        if fault == "padding_query":
            append(0, B, _key(thr[0], 3))
        assert pcnt.max() > 0, "the stand-in's lists are sized so that some key goes to a pool"
        self.L = dict(rows=ROWS, tile_stride=TILE_STRIDE, dim=DIM, B=B, b_pad=B_PAD, k=10, tile_rows=TILE_ROWS, q_pitch=Q_PITCH,
                      query_block=64, n_chunks=N_CHUNKS, list_cap=LIST_CAP, sample_int8=0, sample_step=1, sample_tiles=0, sample_chunks=0,
                      sample_b_pad=256, sample_m=M, uncertified=0, pool_cap=POOL_CAP, kernel=E.I8_KERNEL_STAGED_64)
        self.buf = {E.I8_ROWS: tiled, E.I8_ROW_SCALES: scales, E.I8_QUERIES: q8, E.I8_THRESHOLDS: thr, E.I8_LIST_COUNTS: cnt,
                    E.I8_LISTS: lists, E.I8_POOL_COUNTS: pcnt, E.I8_POOLS: pools}
        self.keys = int(np.minimum(cnt, LIST_CAP).sum() + pcnt.sum())

    def i8_last(self):
        return dict(self.L)

    def i8_read(self, what, dtype, count, offset_bytes=0):
        raw = np.ascontiguousarray(self.buf[what]).reshape(-1).view(np.uint8)
        nbytes = count * np.dtype(dtype).itemsize
        if offset_bytes < 0 or offset_bytes + nbytes > raw.size:
            raise ValueError("read past the buffer")
        return raw[offset_bytes:offset_bytes + nbytes].copy().view(dtype)


FAULTS = ["dropped_key", "wrong_chunk", "stale_slice", "row_off_by_one", "unsigned_mul24", "padding_query"]


def test_checker_passes_on_a_correct_launch():
    idx = FakeIndex()
    probe = {}
    assert _check_collect(idx, idx.i8_last(), probe=probe) == idx.keys
    assert probe["per_list"].sum() == idx.keys and probe["per_list"].max() > LIST_CAP and not probe["over"]
    assert _check_collect(idx, idx.i8_last(), block_tiles=1) == idx.keys           # the blocked form reads by tile_stride too


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_fails_on_a_seeded_fault(fault):
    idx = FakeIndex(fault)
    with pytest.raises(AssertionError):
        _check_collect(idx, idx.i8_last())


def test_checker_refuses_a_launch_that_did_not_certify():
    idx = FakeIndex()
    with pytest.raises(AssertionError):
        _check_collect(idx, dict(idx.i8_last(), uncertified=1))
