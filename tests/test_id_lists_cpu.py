"""How per-query id lists reach the C ABI (no GPU, no library): the arrays ``VectorIndex.search_filtered_each`` and
``VectorIndex.search_excluding`` hand to sqe_index_search_filtered_each / sqe_index_search_excluding, read back from the
pointers by a stand-in ``lib``, and ``engine._pack_id_lists``, the one place that builds them."""
import ctypes as C

import numpy as np
import pytest

from semantic_query_engine_amd import engine as E

DIM = 8

# (lists, list_of_query, B, none_is_no_list) -> (ids, offsets, list_of_query, n_lists)
CASES = {
    "default list_of_query": (([[3, 1], [], [7]], None, 3, False), ([3, 1, 7], [0, 2, 2, 3], [0, 1, 2], 3)),
    "explicit list_of_query": (([[5], np.array([2, 2, 9])], [1, 0, 1, 1], 4, False), ([5, 2, 2, 9], [0, 1, 4], [1, 0, 1, 1], 2)),
    "explicit, deny": (([[5], [2, 2, 9]], [1, -1, 0], 3, True), ([5, 2, 2, 9], [0, 1, 4], [1, -1, 0], 2)),
    "None list": (([[4], None, [6, 6]], [0, 1, 2, 1, -1], 5, True), ([4, 6, 6], [0, 1, 1, 3], [0, -1, 2, -1, -1], 3)),
    "None list, default": (([None, [1]], None, 2, True), ([1], [0, 0, 1], [-1, 1], 2)),
    "empty lists": (([], [-1, -1], 2, True), ([], [0], [-1, -1], 0)),
}


def _same(got, want):
    ids, offsets, loq, n_lists = got
    assert (ids.dtype, offsets.dtype, loq.dtype) == (np.int64, np.int64, np.int32)
    assert (ids.tolist(), offsets.tolist(), loq.tolist(), n_lists) == tuple(want)
    assert all(a.flags.c_contiguous and a.ndim == 1 for a in (ids, offsets, loq))


def _read(ptr, n, ctype, dtype):
    return np.ctypeslib.as_array((ctype * n).from_address(ptr)).astype(dtype) if n else np.empty(0, dtype)


class _Lib:
    """Both entry points: keeps what the three id-list pointers hold."""

    def _take(self, handle, q, b, k, ids, offsets, n_lists, loq, cos, out_ids):
        off = _read(offsets, n_lists + 1, C.c_int64, np.int64)
        self.got = (_read(ids, int(off[-1]), C.c_int64, np.int64), off, _read(loq, b, C.c_int32, np.int32), n_lists)
        return 0

    sqe_index_search_filtered_each = sqe_index_search_excluding = _take


def _index():
    idx = E.VectorIndex.__new__(E.VectorIndex)
    idx.lib, idx.handle, idx.dim = _Lib(), None, DIM
    return idx


def _search(idx, deny):
    return idx.search_excluding if deny else idx.search_filtered_each


@pytest.mark.parametrize("name", CASES)
def test_methods_pass_these_arrays(name):
    (lists, loq, b, deny), want = CASES[name]
    idx = _index()
    given = None if loq is None else np.array(loq, np.int32)
    cos, ids = _search(idx, deny)(np.ones((b, DIM), np.float32), 3, lists, given)
    assert cos.shape == ids.shape == (b, 3)
    _same(idx.lib.got, want)
    assert given is None or given.tolist() == list(loq)          # the caller's array is not written to


@pytest.mark.parametrize("deny", [False, True])
def test_methods_raise(deny):
    idx = _index()
    q = np.ones((3, DIM), np.float32)
    with pytest.raises(ValueError) as e:
        _search(idx, deny)(q, 3, [[1], [2]])
    assert str(e.value) == "2 lists for 3 queries: pass list_of_query"
    with pytest.raises(ValueError) as e:
        _search(idx, deny)(q, 3, [[1], [2]], [0, 1])
    assert str(e.value) == "list_of_query has 2 entries for 3 queries"
    with pytest.raises(ValueError) as e:
        _search(idx, deny)(np.ones((3, DIM + 1), np.float32), 3, [[1]] * 3)
    assert str(e.value) == f"expected [B, {DIM}] queries, got (3, {DIM + 1})"
    assert not hasattr(idx.lib, "got")


@pytest.mark.parametrize("name", CASES)
def test_pack_id_lists(name):
    args, want = CASES[name]
    _same(E._pack_id_lists(*args), want)


def test_pack_id_lists_edges():
    _same(E._pack_id_lists([], None, 0, False), ([], [0], [], 0))
    _same(E._pack_id_lists(iter([[1], (2, 3)]), None, 2, False), ([1, 2, 3], [0, 1, 3], [0, 1], 2))
    # a query that names no entry of `lists` keeps its value: the library turns it away
    _same(E._pack_id_lists([None], [5, 0], 2, True), ([], [0, 0], [5, -1], 1))
    for none_is_no_list in (False, True):
        with pytest.raises(ValueError) as e:
            E._pack_id_lists([[1], [2]], None, 3, none_is_no_list)
        assert str(e.value) == "2 lists for 3 queries: pass list_of_query"
        with pytest.raises(ValueError) as e:
            E._pack_id_lists([[1], [2]], [0, 1], 3, none_is_no_list)
        assert str(e.value) == "list_of_query has 2 entries for 3 queries"


def test_queries():
    q = E._queries(np.arange(DIM), DIM)
    assert q.shape == (1, DIM) and q.dtype == np.float32 and q.flags.c_contiguous
    assert E._queries(np.ones((3, 2 * DIM))[:, ::2], DIM).flags.c_contiguous
    with pytest.raises(ValueError) as e:
        E._queries(np.ones((2, 5)), DIM)
    assert str(e.value) == f"expected [B, {DIM}] queries, got (2, 5)"
    with pytest.raises(ValueError) as e:
        E._queries(np.ones((2, 5)), DIM, "sub-queries")
    assert str(e.value) == f"expected [Bs, {DIM}] sub-queries, got (2, 5)"
