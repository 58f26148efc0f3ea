"""Exclusion search on the host side (no GPU): the clause test ``exclusion_rows``, the routing of such clauses through
``search_excluding`` and the three entries of the C ABI.  The device index is the oracle-backed stand-in of
tests/test_filter_cpu.py with ``search_excluding`` added."""
import os

import numpy as np
import pytest

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from tests.test_filter_cpu import DIM, FilterVectors, _fill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ExcludeVectors(FilterVectors):
    """FilterVectors + search_excluding: row b is the exact top-k over the live rows outside lists[list_of_query[b]]."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        super().__init__(ctx, dim, kind, nlist)
        self.excl_calls = []                             # (batch size, lists, list_of_query) of every exclusion call

    def search_excluding(self, q, k, lists, list_of_query=None):
        q = np.asarray(q, np.float32)
        loq = np.arange(q.shape[0]) if list_of_query is None else np.asarray(list_of_query)
        assert loq.shape[0] == q.shape[0] and (list_of_query is not None or len(lists) == q.shape[0])
        self.excl_calls.append((q.shape[0], [None if a is None else np.asarray(a).copy() for a in lists], loq.copy()))
        cos = np.full((q.shape[0], k), -np.inf, np.float32)
        ids = np.full((q.shape[0], k), -1, np.int64)
        for b in range(q.shape[0]):
            deny = [] if loq[b] < 0 or lists[loq[b]] is None else lists[loq[b]]
            sel = np.nonzero(~np.isin(self.live, deny))[0]
            if sel.size:
                c, pos = R.exact_topk(self.xn[sel], R.normalize_rows(q[b:b + 1]), k)
                cos[b], ids[b] = c[0], np.where(pos[0] >= 0, self.live[sel][np.maximum(pos[0], 0)], -1)
        return cos, ids


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", ExcludeVectors)
    return RT.GpuSearchClient(ctx=object(), dim=DIM)


def _doc(d):
    return {"term": {"doc_id": f"PMC{d}.txt"}}


def _deny(client, clause):
    idx = client.index("idx")
    with idx.lock:
        rows = RT.exclusion_rows(idx, clause)
    return None if rows is None else rows.tolist()


def test_exclusion_rows(client):
    _fill(client)                                        # 6 documents of 4 chunks: document d owns rows 4 d .. 4 d + 3
    # only must_not: the union of its sub-clauses, a single clause or a list of them
    assert _deny(client, {"bool": {"must_not": _doc(1)}}) == [4, 5, 6, 7]
    assert _deny(client, {"bool": {"must_not": [_doc(1)]}}) == [4, 5, 6, 7]
    assert _deny(client, {"bool": {"must_not": [_doc(4), {"ids": {"values": ["PMC0.txt_2", "PMC4.txt_17", "nope"]}}, _doc(1)]}}) == \
        [2, 4, 5, 6, 7, 16, 17, 18, 19]
    assert _deny(client, {"bool": {"must_not": [{"bool": {"filter": [_doc(2)], "must_not": {"ids": {"values": ["PMC2.txt_9"]}}}}]}}) == [8, 10, 11]
    assert _deny(client, {"bool": {"must_not": []}}) == []
    assert _deny(client, {"bool": {"must_not": _doc(77)}}) == []
    # the deny-list is the complement of what filter_rows selects
    idx = client.index("idx")
    for clause in ({"bool": {"must_not": [_doc(0), _doc(5)]}}, {"bool": {"must_not": {"terms": {"doc_id": ["PMC3.txt"]}}}}):
        with idx.lock:
            assert np.array_equal(np.setdiff1d(idx.vectors.ids(), RT.exclusion_rows(idx, clause)), RT.filter_rows(idx, clause))
    # anything with a positive part, or that is no bool at all: None (the allow-list route)
    for clause in ({"bool": {"filter": [_doc(1)], "must_not": _doc(2)}}, {"bool": {"must": _doc(1), "must_not": _doc(2)}},
                   {"bool": {"should": [_doc(1)], "must_not": _doc(2)}}, {"bool": {"must_not": _doc(2), "minimum_should_match": 1}},
                   {"bool": {"filter": [_doc(1)]}}, {"bool": {}}, _doc(1), {"ids": {"values": ["PMC0.txt_2"]}}, None, [1, 2]):
        assert _deny(client, clause) is None
    # an unserved sub-clause raises
    for clause in ({"bool": {"must_not": {"match": {"text": "x"}}}}, {"bool": {"must_not": [_doc(1), {"term": {"text": "x"}}]}}):
        with pytest.raises(ValueError):
            _deny(client, clause)


def test_indexer_search_routes_must_not_and_exclude_ids(client):
    x, docs = _fill(client)
    ix = RT.OpenSearchIndexer(client, "idx")
    vec = client.index("idx").vectors
    q = x[5:6] + 0.01
    assert ix.search(q, k=3)[0][0]["text"] == docs[5]["text"]
    vec.calls.clear()
    hits = ix.search(q, k=3, filter={"bool": {"must_not": [_doc(1)]}})
    assert len(vec.excl_calls) == 1 and not vec.calls                # one exclusion call, no allow-list
    n, lists, loq = vec.excl_calls[0]
    assert n == 1 and [a.tolist() for a in lists] == [[4, 5, 6, 7]] and loq.tolist() == [0]
    assert len(hits) == 3 and all(s["doc_id"] != "PMC1.txt" for s, _ in hits)
    with client.index("idx").lock:
        allow = RT.filter_rows(client.index("idx"), {"bool": {"must_not": [_doc(1)]}})
    c1, i1 = vec.search(q, 3, filter_ids=allow)                      # the route of before: the same hits
    assert [s["text"] for s, _ in hits] == [docs[int(r)]["text"] for r in i1[0]]
    assert [sc for _, sc in hits] == [float(1.0 / (2.0 - float(c))) for c in c1[0]]
    # a clause with a positive part keeps the allow-list route
    vec.calls.clear()
    ix.search(q, k=3, filter={"bool": {"filter": [_doc(1)], "must_not": {"ids": {"values": ["PMC1.txt_5"]}}}})
    assert len(vec.excl_calls) == 1 and [c[1].tolist() for c in vec.calls] == [[4, 6, 7]]
    # exclude_ids: _id strings, unknown ones skipped
    hits = ix.search(q, k=3, exclude_ids=["PMC1.txt_5", "PMC1.txt_6", "PMC9.txt_99"])
    assert vec.excl_calls[-1][1][0].tolist() == [5, 6] and docs[5]["text"] not in [s["text"] for s, _ in hits] and len(hits) == 3
    for kw in (dict(filter=_doc(1)), dict(min_score=0.5), dict(collapse={"field": "doc_id"}), dict(mmr={"lambda": 0.5})):
        with pytest.raises(ValueError):
            ix.search(q, k=3, exclude_ids=["PMC1.txt_5"], **kw)


def test_search_batch_three_routes(client):
    from tests.test_filter_each_cpu import EachVectors

    class Both(ExcludeVectors, EachVectors):
        pass

    idx = client.index("idx")
    idx.vectors = Both(dim=DIM)
    x, docs = _fill(client)
    ix = RT.OpenSearchIndexer(client, "idx")
    vec = idx.vectors
    q = np.random.default_rng(2).standard_normal((6, DIM)).astype(np.float32)
    not1 = {"bool": {"must_not": [_doc(1)]}}
    not1_again = {"bool": {"must_not": [{"term": {"doc_id": "PMC1.txt"}}]}}
    not23 = {"bool": {"must_not": [_doc(2), _doc(3)]}}
    filters = [not1, None, _doc(3), not23, not1_again, None]
    vec.calls.clear()
    cos, ids = ix.search_batch(q, k=3, filters=filters)
    # one exclusion call beside the one per-query filtered call and the one plain call
    assert len(vec.excl_calls) == 1 and len(vec.each_calls) == 1 and [c[0] for c in vec.calls] == [2]
    n, lists, loq = vec.excl_calls[0]
    assert n == 3 and [a.tolist() for a in lists] == [[4, 5, 6, 7], list(range(8, 16))] and loq.tolist() == [0, 1, 0]
    n, lists, loq = vec.each_calls[0]
    assert n == 1 and [a.tolist() for a in lists] == [[12, 13, 14, 15]] and loq.tolist() == [0]
    for b, flt in enumerate(filters):                                # request order, each row the single search of before
        allow = None
        if flt is not None:
            with idx.lock:
                allow = RT.filter_rows(idx, flt)
        c1, i1 = vec.search(q[b:b + 1], 3, filter_ids=allow)
        assert np.array_equal(ids[b], i1[0]) and np.array_equal(cos[b], c1[0])
    # an index whose vectors have no search_excluding keeps the allow-list route
    idx.vectors = EachVectors(dim=DIM)
    idx.vectors.add(x)
    c2, i2 = ix.search_batch(q, k=3, filters=filters)
    assert np.array_equal(i2, ids) and np.array_equal(c2, cos) and len(idx.vectors.each_calls) == 1


@pytest.mark.parametrize("flag", [False, True])
def test_shim_knn_filter_must_not(monkeypatch, flag):
    """a knn.filter that only excludes goes through search_excluding, with and without --per-query-filters: same hits as the
    allow-list route gave (the stand-in of tests/test_filter_cpu.py has no search_excluding and keeps that route)"""
    from fastapi.testclient import TestClient
    from semantic_query_engine_amd import shim
    from tests.test_filter_cpu import _app, _knn
    flt = {"bool": {"must_not": [{"term": {"doc_id": "d0"}}, {"ids": {"values": ["d2_7"]}}]}}
    hits = {}
    for vectors in (ExcludeVectors, FilterVectors):
        monkeypatch.setattr(RT, "VectorIndex", vectors)
        client = RT.GpuSearchClient(ctx=object(), dim=DIM)
        with TestClient(shim.create_app(client, None, DIM, per_query_filters=flag and vectors is ExcludeVectors)) as c:
            c, client, x = next(_app(c, client))
            r = c.post("/idx/_search", json=_knn(x[1] + 0.01, 4, flt))
            assert r.status_code == 200, r.text
            hits[vectors] = [(h["_id"], h["_score"]) for h in r.json()["hits"]["hits"]]
            vec = client.index("idx").vectors
            if vectors is ExcludeVectors:
                assert len(vec.excl_calls) == 1 and [a.tolist() for a in vec.excl_calls[0][1]] == [[0, 1, 2, 7]]
                assert all(c[1] is None for c in vec.calls)              # no allow-list was built or searched
            r = c.post("/idx/_search", json=_knn(x[1], 4, {"bool": {"must_not": {"match": {"text": "t1"}}}}))
            assert r.status_code == 400 and r.json()["error"]["type"] == "parsing_exception"
    assert len(hits[ExcludeVectors]) == 4 and hits[ExcludeVectors] == hits[FilterVectors]
    assert not {i for i, _ in hits[ExcludeVectors]} & {"d0_0", "d0_1", "d0_2", "d2_7"}


def test_symbols_exported_and_bound():
    so = os.path.join(ROOT, "semantic_query_engine_amd", "libsqe.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    from semantic_query_engine_amd import VectorIndex, Context, _native
    lib = _native.load()
    for name in ("sqe_index_search_excluding", "sqe_index_search_excluding_device", "sqe_exclude_swept"):
        assert name in _native.SIGNATURES and hasattr(lib, name), name
        assert name in open(os.path.join(ROOT, "include", "sqe.h")).read()
    assert len(_native.SIGNATURES["sqe_index_search_excluding"][1]) == 10
    assert callable(VectorIndex.search_excluding) and callable(VectorIndex.search_excluding_device) and callable(Context.exclude_swept)
    # argument checks need no device: null index, null output of the counter
    assert lib.sqe_index_search_excluding(None, None, 1, 1, None, None, 0, None, None, None) == -1
    assert lib.sqe_exclude_swept(None, None) == -1
