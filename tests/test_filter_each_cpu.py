"""Per-query filters on the host side (no GPU): OpenSearchIndexer.search_batch(filters=), the shim's search batcher with
``per_query_filters`` and two concurrent filtered ``_search`` requests.  The device index is the oracle-backed stand-in of
tests/test_filter_cpu.py with ``search_filtered_each`` added."""
import asyncio
import threading

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from semantic_query_engine_amd import shim
from tests.test_filter_cpu import DIM, FilterVectors, _app, _fill, _knn


class EachVectors(FilterVectors):
    """FilterVectors + search_filtered_each: row b is the exact top-k over the live rows among lists[list_of_query[b]]."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        super().__init__(ctx, dim, kind, nlist)
        self.each_calls = []                             # (batch size, lists, list_of_query) of every per-query call

    def search_filtered_each(self, q, k, lists, list_of_query=None):
        q = np.asarray(q, np.float32)
        loq = np.arange(q.shape[0]) if list_of_query is None else np.asarray(list_of_query)
        assert loq.shape[0] == q.shape[0] and (list_of_query is not None or len(lists) == q.shape[0])
        self.each_calls.append((q.shape[0], [np.asarray(a).copy() for a in lists], loq.copy()))
        cos = np.full((q.shape[0], k), -np.inf, np.float32)
        ids = np.full((q.shape[0], k), -1, np.int64)
        for b in range(q.shape[0]):
            sel = np.nonzero(np.isin(self.live, lists[loq[b]]))[0]
            if sel.size:
                c, pos = R.exact_topk(self.xn[sel], R.normalize_rows(q[b:b + 1]), k)
                cos[b], ids[b] = c[0], np.where(pos[0] >= 0, self.live[sel][np.maximum(pos[0], 0)], -1)
        return cos, ids


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", EachVectors)
    return RT.GpuSearchClient(ctx=object(), dim=DIM)


def _doc(d):
    return {"term": {"doc_id": f"PMC{d}.txt"}}


def test_search_batch_filters(client):
    x, docs = _fill(client)                              # 6 documents of 4 chunks: document d owns rows 4 d .. 4 d + 3
    ix = RT.OpenSearchIndexer(client, "idx")
    vec = client.index("idx").vectors
    rng = np.random.default_rng(1)
    q = rng.standard_normal((7, DIM)).astype(np.float32)
    # equal clauses (whatever their key order) share a list; None entries go to the plain search
    both = {"bool": {"filter": [_doc(1)], "must_not": {"ids": {"values": ["PMC1.txt_4"]}}}}
    both_reordered = {"bool": {"must_not": {"ids": {"values": ["PMC1.txt_4"]}}, "filter": [_doc(1)]}}
    filters = [_doc(3), None, both, _doc(3), None, both_reordered, _doc(5)]
    cos, ids = ix.search_batch(q, k=3, filters=filters)
    assert cos.shape == (7, 3) and ids.shape == (7, 3)
    assert len(vec.each_calls) == 1 and [c[0] for c in vec.calls] == [2]
    n, lists, loq = vec.each_calls[0]
    assert n == 5 and [a.tolist() for a in lists] == [[12, 13, 14, 15], [5, 6, 7], [20, 21, 22, 23]]
    assert loq.tolist() == [0, 1, 0, 1, 2]
    # rows come back in request order: every row is what the single search of that request gives
    for b, flt in enumerate(filters):
        allow = None
        if flt is not None:
            with client.index("idx").lock:
                allow = RT.filter_rows(client.index("idx"), flt)
        c1, i1 = vec.search(q[b:b + 1], 3, filter_ids=allow)
        assert np.array_equal(ids[b], i1[0]) and np.array_equal(cos[b], c1[0])
    # all None: plain rows through the per-query path's plain search; filters=None: the call of before, nothing else
    vec.calls.clear()
    vec.each_calls.clear()
    c0, i0 = ix.search_batch(q, k=3)
    assert [(c[0], c[1]) for c in vec.calls] == [(7, None)] and not vec.each_calls
    c1, i1 = ix.search_batch(q, k=3, filters=[None] * 7)
    assert np.array_equal(i0, i1) and np.array_equal(c0, c1) and not vec.each_calls
    # an unserved clause raises before any device call; so does a wrong number of filters
    vec.calls.clear()
    with pytest.raises(ValueError):
        ix.search_batch(q, k=3, filters=[_doc(1)] * 6 + [{"term": {"text": "x"}}])
    with pytest.raises(ValueError):
        ix.search_batch(q, k=3, filters=[_doc(1)] * 6)
    assert not vec.calls and not vec.each_calls


def _six(client, **kw):
    _fill(client, n_docs=4, chunks=3)
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=50.0, **kw)
    rng = np.random.default_rng(5)
    qs = rng.standard_normal((6, DIM)).astype(np.float32)
    flts = [None, _doc(1), _doc(2), None, _doc(1), _doc(2)]

    async def run():
        return await asyncio.gather(*[b.search("idx", qs[i:i + 1], 3, "embedding", flts[i]) for i in range(6)])

    return b, flts, asyncio.run(run())


def test_batcher_per_query_filters(client):
    b, flts, res = _six(client, per_query_filters=True)
    vec = client.index("idx").vectors
    assert b.batches == 2                                # one plain call and one per-query filtered call
    assert [(c[0], c[1]) for c in vec.calls] == [(2, None)]
    assert len(vec.each_calls) == 1
    n, lists, loq = vec.each_calls[0]
    assert n == 4 and sorted(a.tolist() for a in lists) == [[3, 4, 5], [6, 7, 8]]
    assert sorted(loq.tolist()) == [0, 0, 1, 1]
    for i, hits in enumerate(res):
        assert len(hits) == 3
        if flts[i] is not None:
            assert {h["_source"]["doc_id"] for h in hits} == {flts[i]["term"]["doc_id"]}


def test_batcher_default_is_unchanged(client):
    b, flts, res = _six(client)
    vec = client.index("idx").vectors
    assert b.batches == 3 and len(vec.calls) == 3 and not vec.each_calls
    on = _six_hits(res)
    assert all(len(h) == 3 for h in on)


def _six_hits(res):
    return [[(h["_id"], h["_score"]) for h in hits] for hits in res]


def test_batcher_same_hits_with_and_without(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", EachVectors)
    off = _six(RT.GpuSearchClient(ctx=object(), dim=DIM))[2]
    on = _six(RT.GpuSearchClient(ctx=object(), dim=DIM), per_query_filters=True)[2]
    assert _six_hits(on) == _six_hits(off)


def test_batcher_falls_back_one_by_one(client, monkeypatch):
    """a failing per-query batch is retried request by request, each still over its own clause"""
    _fill(client, n_docs=4, chunks=3)
    vec = client.index("idx").vectors
    real = vec.search_filtered_each

    def flaky(q, k, lists, list_of_query=None):
        if np.asarray(q).shape[0] > 1:
            raise RuntimeError("device error")
        return real(q, k, lists, list_of_query)

    monkeypatch.setattr(vec, "search_filtered_each", flaky)
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=50.0, per_query_filters=True)
    qs = np.random.default_rng(6).standard_normal((2, DIM)).astype(np.float32)

    async def run():
        return await asyncio.gather(b.search("idx", qs[0:1], 3, "embedding", _doc(1)), b.search("idx", qs[1:2], 3, "embedding", _doc(2)))

    res = asyncio.run(run())
    assert {h["_source"]["doc_id"] for h in res[0]} == {"PMC1.txt"} and {h["_source"]["doc_id"] for h in res[1]} == {"PMC2.txt"}
    assert b.batches == 2


def _concurrent(c, bodies):
    out = [None] * len(bodies)
    gate = threading.Barrier(len(bodies))

    def post(i):
        gate.wait()
        out[i] = c.post("/idx/_search", json=bodies[i])

    ts = [threading.Thread(target=post, args=(i,)) for i in range(len(bodies))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return out


def test_http_two_concurrent_filters(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", EachVectors)
    hits = {}
    for flag in (False, True):
        client = RT.GpuSearchClient(ctx=object(), dim=DIM)
        with TestClient(shim.create_app(client, None, DIM, per_query_filters=flag)) as c:
            c, client, x = next(_app(c, client))
            bodies = [_knn(x[1] + 0.01, 3, {"term": {"doc_id": "d2"}}), _knn(x[7] + 0.01, 3, {"terms": {"doc_id": ["d0", "d3"]}})]
            rs = _concurrent(c, bodies)
            assert all(r.status_code == 200 for r in rs), [r.text for r in rs]
            hits[flag] = [r.json()["hits"]["hits"] for r in rs]
            vec = client.index("idx").vectors
            assert bool(vec.each_calls) == flag
            assert {h["_source"]["doc_id"] for h in hits[flag][0]} == {"d2"}
            assert {h["_source"]["doc_id"] for h in hits[flag][1]} <= {"d0", "d3"}
    assert hits[True] == hits[False]


def test_main_has_the_flag():
    import inspect
    assert "--per-query-filters" in inspect.getsource(shim.main)
    assert inspect.signature(shim.create_app).parameters["per_query_filters"].default is False
    assert inspect.signature(shim._SearchBatcher.__init__).parameters["per_query_filters"].default is False
