"""The sub-batch loops of the lexical index (lexical.hip: lex_topk_run, lex_match_run).  GPU only.

A grid holds at most 65,535 queries, so a batch of 65,537 takes two launches, the second with every per-query pointer moved
on: the query offsets, min_should, the partial keys, the two outputs and count_out.  The index is one chunk of 40 ordered
documents, so the match sets step by 65,535 queries as well (their bit maps would allow far more).  Query i is pattern i mod 7
of seven distinct patterns; 7 is coprime to 65,535 = 3 * 5 * 17 * 257, so a pointer left behind at the second launch reads
another pattern than the one its row belongs to.  Every row has to equal the row of its pattern in a batch of 7, and that
batch the NumPy references, bit for bit."""
import numpy as np
import pytest

from . import lexphrase_reference as PR
from .lexbool_reference import FILTER, MUST, MUST_NOT, SHOULD, LexBoolRef

pytestmark = pytest.mark.gpu

T = 12
N_DOCS = 40
B, K, CAP = 65_537, 3, 2
# plain queries of different lengths: a pointer that is not moved on lands in another pattern's terms
PLAIN = [[0], [1, 2], [], [3, 0, 1], [5, 11], [2, 2, 4, 5], [6, 7, 0, 1, 2]]
# boolean queries that differ in length, in roles and in min_should
BOOL = [
    ([0, 9], [SHOULD, SHOULD], 0),
    ([0, 9], [SHOULD, SHOULD], 2),                      # only min_should tells it from the one before; term 9 is in no document: count 0
    ([2], [MUST], 0),
    ([11, 0], [MUST, SHOULD], 0),                       # nor is term 11
    ([0, 1, 2], [FILTER, MUST_NOT, SHOULD], 0),
    ([3, 4, 5, 0], [SHOULD, SHOULD, SHOULD, SHOULD], 3),
    ([1], [FILTER], 0),
]
# clause queries: phrases and terms
PHRASE = [
    ([[0, 1]], [MUST], 0),
    ([[0], [1]], [SHOULD, SHOULD], 2),
    ([[1, 0], [2]], [SHOULD, SHOULD], 0),
    ([[11, 0]], [MUST], 0),                             # count 0
    ([[0], [1, 2], [3]], [FILTER, MUST_NOT, SHOULD], 0),
    ([[2, 3], [0, 1], [4]], [SHOULD, SHOULD, SHOULD], 2),
    ([[1]], [FILTER], 0),
]


def same_bits(a, b):
    return all(u.shape == w.shape and u.dtype == w.dtype and np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
               for u, w in zip(a, b))


def tiled(lists, dtype, n=B):
    """(offsets, values) of lists[i mod 7] for i < n, built from one tiled array rather than n Python lists."""
    lens = np.array([len(x) for x in lists], np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.resize(lens, n), out=off[1:])
    flat = np.concatenate([np.asarray(x, dtype).reshape(-1) for x in lists])
    reps, rest = divmod(n, len(lists))
    return off, np.concatenate([np.tile(flat, reps), flat[:int(lens[:rest].sum())]]).astype(dtype)


def rows_repeat(big, small):
    """row i of every array of big is row i mod 7 of the same array of small"""
    return same_bits(big, tuple(np.resize(x, (B,) + x.shape[1:]) for x in small))


@pytest.fixture(scope="module")
def world():
    from semantic_query_engine_amd import Context, LexicalIndex
    rng = np.random.default_rng(17)
    ids = 3 + 2 * np.arange(N_DOCS, dtype=np.int64)
    docs = [rng.integers(0, 8, int(rng.integers(2, 12))).astype(np.int32) for _ in range(N_DOCS)]      # terms 8 .. 11 in no document
    docs[5] = np.array([0, 1, 0, 1, 2], np.int32)
    lex = LexicalIndex(Context(0), T)
    lex.put(ids, docs, ordered=True)
    assert lex.info()["chunk_rows"] >= N_DOCS
    ref = PR.LexPhraseRef(ids, docs, np.ones(N_DOCS, bool), T)
    return lex, ref


def test_search_across_the_grid_limit(world):
    lex, ref = world
    small = lex.search(PLAIN, K)
    assert same_bits(small, ref.ref.search(PLAIN, K)[:2])
    assert len({small[1][j].tobytes() + small[0][j].tobytes() for j in range(7)}) == 7          # a wrong pattern shows
    assert rows_repeat(lex.search(tiled(PLAIN, np.int32), K), small)


def test_search_bool_and_match_across_the_grid_limit(world):
    lex, ref = world
    Q, R, M = [p[0] for p in BOOL], [p[1] for p in BOOL], [p[2] for p in BOOL]
    bref = LexBoolRef(ref.ref)
    small = lex.search_bool(Q, R, K, M)
    assert same_bits(small, bref.search(Q, R, K, M)[:2])
    small_m = lex.match(Q, R, M, cap=CAP)
    assert same_bits(small_m, bref.match(Q, R, M, cap=CAP)[:2])
    assert small_m[0].min() == 0 and small_m[0].max() > CAP and len(set(small_m[0].tolist())) >= 5
    stale = M[-1:] + M[:-1]                 # what the second launch reads through a min_should pointer left behind: 65,535 mod 7 = 1
    assert not same_bits(bref.search(Q, R, K, stale)[:2], small) and not np.array_equal(bref.match(Q, R, stale, cap=CAP)[0], small_m[0])
    q, r, m = tiled(Q, np.int32), tiled(R, np.uint8), np.resize(np.array(M, np.int32), B)
    assert rows_repeat(lex.search_bool(q, r, K, m), small)
    assert rows_repeat(lex.match(q, r, m, cap=CAP), small_m)


def test_search_phrase_and_match_across_the_grid_limit(world):
    lex, ref = world
    Q, R, M = [p[0] for p in PHRASE], [p[1] for p in PHRASE], [p[2] for p in PHRASE]
    small = lex.search_phrase(Q, R, K, M)
    assert same_bits(small, ref.search(Q, R, K, M)[:2])
    small_m = lex.match_phrase(Q, R, M, cap=CAP)
    assert same_bits(small_m, ref.match(Q, R, M, cap=CAP)[:2])
    assert small_m[0].min() == 0 and small_m[0].max() > CAP and len(set(small_m[0].tolist())) >= 5
    stale = M[-1:] + M[:-1]
    assert not same_bits(ref.search(Q, R, K, stale)[:2], small) and not np.array_equal(ref.match(Q, R, stale, cap=CAP)[0], small_m[0])
    reps = B // 7 + 1
    q, r, m = (Q * reps)[:B], tiled(R, np.uint8), np.resize(np.array(M, np.int32), B)
    assert rows_repeat(lex.search_phrase(q, r, K, m), small)
    assert rows_repeat(lex.match_phrase(q, r, m, cap=CAP), small_m)
