"""The TILED copy of the quantised queries (quant.hip) that the 256-query int8 kernels read (scan_i8.hip: scan_i8_pp_kernel, its
five-stage build, sample_i8_pp_kernel): block qb of 256 queries at qb * (dim / 64) * 16 KiB, the 64-byte K slice h of query r at
h * 16 KiB + r * 64, queries past B zero.

Three properties, all integer work, so the bar is equality:
  * the tiled copy is the row-major copy (SQE_I8_QUERIES, which every older test reads) re-tiled, byte for byte, padding included;
  * what a launch collects is the set {(acc * s, row) : acc * s >= thr} recomputed from the launch's ROW-MAJOR operands, and the
    threshold pass's best-two lists are the ones recomputed from them -- a wrong lane offset or a stale K slice of the tiled operand
    shows here (the final top-k would hide it behind the fp32 re-score and the bf16 fallback);
  * two identical searches collect the same keys.
n = 20,077 rows: a partial last tile, and more than the 4 * step * 256 rows the int8 pass needs.  The shapes cover the smallest dim
the launcher admits, one and several query blocks, a full last block, and a batch whose collect scan does not read the tiled copy
at all (the threshold pass pads every batch to 256-query blocks and always does)."""
import numpy as np
import pytest

from tests.test_i8_exact_gpu import _check_collect, _check_sample, _launch_lists, expected_kernel

pytestmark = pytest.mark.gpu

N_ROWS = 20_000 + 77
STEP = 4
M = 64          # (tests/test_i8_exact_gpu.py's: the threshold is the 64th best of the sample, so every query certifies on Gaussian rows)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _i8_index(ctx, dim, step, m):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    idx = VectorIndex(ctx, dim)
    idx.set_option("scan_mode", SCAN_INT8_RESCORE)
    idx.set_option("i8_min_rows", 0)
    idx.set_option("i8_sample_step", step)
    idx.set_option("i8_sample_m", m)
    return idx


@pytest.fixture(scope="module")
def searched(ctx):
    """(dim, B) -> (index, queries, what sqe_index_i8_last says of its one search); built once per shape, never searched again"""
    made = {}

    def get(dim, b):
        if (dim, b) not in made:
            rng = np.random.default_rng(1000 * dim + b)
            x = rng.standard_normal((N_ROWS, dim), dtype=np.float32)
            q = rng.standard_normal((b, dim), dtype=np.float32)
            idx = _i8_index(ctx, dim, STEP, M)
            idx.add(x)
            idx.search(q, 10)
            L = idx.i8_last()
            assert (L["rows"], L["dim"], L["B"]) == (N_ROWS, dim, b)
            assert L["sample_int8"] == 1 and L["sample_step"] == STEP and L["sample_b_pad"] == (b + 255) // 256 * 256
            made[(dim, b)] = (idx, q, L)
        return made[(dim, b)]

    yield get
    for idx, _, _ in made.values():
        idx.close()


def _retile(q8_rows, dim):
    """int8 [rows, dim] row-major -> the bytes of the tiled copy: [blocks][dim / 64][256][64], rows padded with zeros"""
    blocks = (q8_rows.shape[0] + 255) // 256
    full = np.zeros((blocks * 256, dim), np.int8)
    full[: q8_rows.shape[0]] = q8_rows
    return np.ascontiguousarray(full.reshape(blocks, 256, dim // 64, 64).transpose(0, 2, 1, 3)).reshape(-1)


@pytest.mark.parametrize("dim,b", [(256, 129), (512, 257), (1024, 256), (1024, 700), (1024, 33)])
def test_tiled_copy_is_the_row_major_copy(searched, dim, b):
    from semantic_query_engine_amd import engine as E
    idx, _, L = searched(dim, b)
    assert L["query_block"] == (256 if b > 128 else 64)
    assert L["kernel"] == expected_kernel(dim, b)
    rows = idx.i8_read(E.I8_QUERIES, np.int8, L["b_pad"] * L["q_pitch"]).reshape(L["b_pad"], L["q_pitch"])[:, :dim]
    assert rows[:b].any() and not rows[b:].any()
    blocks = (L["b_pad"] + 255) // 256
    tiled = idx.i8_read(E.I8_QUERIES_TILED, np.int8, blocks * 256 * dim)
    want = _retile(rows, dim)
    assert tiled.shape == want.shape
    assert np.array_equal(tiled, want), f"{np.count_nonzero(tiled != want)} bytes differ"
    # the buffer ends there: one byte more is outside it
    with pytest.raises(Exception):
        idx.i8_read(E.I8_QUERIES_TILED, np.int8, blocks * 256 * dim + 1)


@pytest.mark.parametrize("dim,b", [(256, 129), (512, 257), (1024, 700)])
def test_collected_keys_and_sample_lists_are_bit_exact(ctx, searched, dim, b):
    idx, _, L = searched(dim, b)
    assert L["query_block"] == 256
    assert L["kernel"] == expected_kernel(dim, b)
    keys = _check_collect(idx, L)
    assert keys > 0
    _check_sample(idx, L)


def test_identical_calls_collect_the_same_keys(ctx):
    dim, b = 1024, 700
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N_ROWS, dim), dtype=np.float32)
    q = rng.standard_normal((b, dim), dtype=np.float32)
    idx = _i8_index(ctx, dim, STEP, M)
    idx.add(x)
    got = []
    for _ in range(2):
        cos, ids = idx.search(q, 10)
        L = idx.i8_last()
        assert L["uncertified"] == 0
        kq, key, _, over = _launch_lists(idx, L)
        assert not over
        o = np.lexsort((key, kq))
        got.append((kq[o], key[o], cos, ids))
    assert got[0][0].size > 0
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    assert np.array_equal(got[0][2], got[1][2]) and np.array_equal(got[0][3], got[1][3])
    idx.close()
