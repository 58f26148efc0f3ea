"""Filtered k-NN on the host side (no GPU): the shim's ``knn.filter``, OpenSearchIndexer.search(filter=), the filter
clause parser and the doc_id -> vector ids map that serves it, through overwrite, delete and save / load.  The device
index is an oracle-backed stand-in whose ``search`` takes ``filter_ids``."""
import json
import os
import threading

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from semantic_query_engine_amd import shim

DIM = 16


class FilterVectors:
    """VectorIndex stand-in: rows keyed by id, exact top-k over the live rows (or the live rows among filter_ids)."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        self.dim, self.xn, self.live, self.next_id = dim, np.zeros((0, dim), np.float32), np.zeros(0, np.int64), 0
        self.calls = []                                  # (batch size, filter_ids or None) of every search

    def __len__(self):
        return int(self.live.size)

    def ids(self):
        return self.live.copy()

    def add(self, x):
        x = R.normalize_rows(np.asarray(x, np.float32))
        self.xn = np.concatenate([self.xn, x], 0)
        self.live = np.concatenate([self.live, np.arange(self.next_id, self.next_id + x.shape[0])])
        self.next_id += x.shape[0]

    def _pos(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        pos = np.searchsorted(self.live, ids)
        assert np.all(pos < self.live.size) and np.all(self.live[np.minimum(pos, self.live.size - 1)] == ids)
        return pos

    def delete(self, ids):
        keep = np.ones(self.live.size, bool)
        keep[self._pos(ids)] = False
        self.live, self.xn = self.live[keep], self.xn[keep]

    def update(self, ids, x):
        self.xn[self._pos(ids)] = R.normalize_rows(np.asarray(x, np.float32))

    def get_rows(self, ids):
        return self.xn[self._pos(ids)]

    def search(self, q, k, nprobe=0, filter_ids=None):
        q = np.asarray(q, np.float32)
        self.calls.append((q.shape[0], None if filter_ids is None else np.asarray(filter_ids).copy()))
        sel = np.arange(self.live.size) if filter_ids is None else np.nonzero(np.isin(self.live, filter_ids))[0]
        if sel.size == 0:
            return np.full((q.shape[0], k), -np.inf, np.float32), np.full((q.shape[0], k), -1, np.int64)
        cos, pos = R.exact_topk(self.xn[sel], R.normalize_rows(q), k)
        return cos.astype(np.float32), np.where(pos >= 0, self.live[sel][np.maximum(pos, 0)], -1)

    def save(self, path):
        np.savez(path + ".npz", xn=self.xn, live=self.live, next_id=self.next_id)
        os.replace(path + ".npz", path)

    @classmethod
    def load(cls, ctx, path):
        d = np.load(path)
        v = cls(ctx, d["xn"].shape[1])
        v.xn, v.live, v.next_id = d["xn"], d["live"], int(d["next_id"])
        return v


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", FilterVectors)
    return RT.GpuSearchClient(ctx=object(), dim=DIM)


def _fill(client, name="idx", n_docs=6, chunks=4, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_docs * chunks, DIM)).astype(np.float32)
    docs = [{"doc_id": f"PMC{d}.txt", "text": f"chunk {c} of {d}"} for d in range(n_docs) for c in range(chunks)]
    RT.OpenSearchIndexer(client, name).add_embeddings(x, docs)
    return x, docs


def _rows(client, clause, name="idx"):
    idx = client.index(name)
    with idx.lock:
        return RT.filter_rows(idx, clause).tolist()


def test_filter_clauses(client):
    _fill(client)
    # the _id rule of the reference: f"{doc_id}_{i}" with i the position in the add call
    assert _rows(client, {"term": {"doc_id": "PMC1.txt"}}) == [4, 5, 6, 7]
    assert _rows(client, {"term": {"doc_id": {"value": "PMC2.txt"}}}) == [8, 9, 10, 11]
    assert _rows(client, {"terms": {"doc_id": ["PMC0.txt", "PMC5.txt", "nope"]}}) == [0, 1, 2, 3, 20, 21, 22, 23]
    assert _rows(client, {"ids": {"values": ["PMC1.txt_5", "PMC3.txt_12", "missing"]}}) == [5, 12]
    assert _rows(client, {"bool": {"filter": [{"terms": {"doc_id": ["PMC0.txt", "PMC1.txt"]}}],
                                   "must_not": {"ids": {"values": ["PMC0.txt_1"]}}}}) == [0, 2, 3, 4, 5, 6, 7]
    assert _rows(client, {"bool": {"should": [{"term": {"doc_id": "PMC0.txt"}}, {"term": {"doc_id": "PMC4.txt"}}]}}) == \
        [0, 1, 2, 3, 16, 17, 18, 19]
    assert _rows(client, {"bool": {"must_not": [{"terms": {"doc_id": ["PMC0.txt", "PMC1.txt", "PMC2.txt"]}}]}}) == \
        list(range(12, 24))
    assert _rows(client, {"bool": {"must": {"term": {"doc_id": "PMC0.txt"}}, "filter": {"term": {"doc_id": "PMC1.txt"}}}}) == []
    for bad in ({"match_all": {}}, {"term": {"text": "x"}}, {"range": {"doc_id": {"gte": 1}}}, {"bool": {"boost": 2}},
                {"term": {"doc_id": "a"}, "ids": {"values": []}}, {"terms": {"doc_id": "PMC1.txt"}},
                {"bool": {"should": [{"term": {"doc_id": "a"}}], "minimum_should_match": 2}}, "PMC1.txt"):
        with pytest.raises(ValueError):
            _rows(client, bad)


def test_indexer_search_filter(client):
    x, docs = _fill(client)
    ix = RT.OpenSearchIndexer(client, "idx")
    q = x[5:6] + 0.01
    hits = ix.search(q, k=3, filter={"term": {"doc_id": "PMC3.txt"}})
    assert len(hits) == 3 and all(h[0]["doc_id"] == "PMC3.txt" for h in hits)
    assert [round(h[1], 6) for h in hits] == sorted((round(h[1], 6) for h in hits), reverse=True)
    assert ix.search(q, k=3)[0][0]["text"] == docs[5]["text"]          # unfiltered: unchanged
    assert ix.search(q, k=3, filter={"term": {"doc_id": "unknown"}}) == []
    calls = client.index("idx").vectors.calls
    assert calls[-2][1] is None and calls[-1][1].size == 0


def test_doc_map_through_overwrite_delete_and_reload(client, tmp_path):
    x, docs = _fill(client)
    idx = client.index("idx")
    ix = RT.OpenSearchIndexer(client, "idx")
    # overwrite _id PMC1.txt_4 (row 4) with a document of another doc_id: the map follows
    RT._commit_documents(idx, x[4:5] * 2, [{"doc_id": "PMC9.txt", "text": "moved"}], lambda i, d: "PMC1.txt_4")
    assert _rows(client, {"term": {"doc_id": "PMC1.txt"}}) == [5, 6, 7]
    assert _rows(client, {"term": {"doc_id": "PMC9.txt"}}) == [4]
    hits = ix.search(x[4:5], k=5, filter={"term": {"doc_id": "PMC9.txt"}})
    assert [h[0]["text"] for h in hits] == ["moved"]
    # deletes drop rows from the map
    assert RT.delete_documents(idx, ["PMC1.txt_5", "PMC2.txt_8"]) == [True, True]
    assert _rows(client, {"terms": {"doc_id": ["PMC1.txt", "PMC2.txt"]}}) == [6, 7, 9, 10, 11]
    assert RT.delete_by_query(idx, {"query": {"term": {"doc_id": "PMC0.txt"}}}) == 4
    assert "PMC0.txt" not in idx.rows_of_doc
    before = {d: sorted(r) for d, r in idx.rows_of_doc.items()}
    # save / load rebuilds the same map
    client.save_index("idx", str(tmp_path))
    client2 = RT.GpuSearchClient(ctx=object(), dim=DIM)
    assert client2.load_index("idx", str(tmp_path))
    assert {d: sorted(r) for d, r in client2.index("idx").rows_of_doc.items()} == before
    with client2.index("idx").lock:
        assert RT.filter_rows(client2.index("idx"), {"term": {"doc_id": "PMC9.txt"}}).tolist() == [4]


# ---------------------------------------------------------------- the shim


def _bulk(lines):
    return ("\n".join(json.dumps(x) for x in lines) + "\n").encode()


@pytest.fixture()
def app(client):
    # one event loop for the whole test (the search batcher's task lives on it), as under uvicorn
    with TestClient(shim.create_app(client, None, DIM)) as c:
        yield from _app(c, client)


def _app(c, client):
    c.put("/idx", json={"mappings": {"properties": {"embedding": {"type": "knn_vector", "dimension": DIM}}}})
    rng = np.random.default_rng(3)
    x = rng.standard_normal((12, DIM)).astype(np.float32)
    lines = []
    for i in range(12):
        lines += [{"index": {"_index": "idx", "_id": f"d{i // 3}_{i}"}},
                  {"doc_id": f"d{i // 3}", "text": f"t{i}", "embedding": [float(v) for v in x[i]]}]
    r = c.post("/_bulk", content=_bulk(lines), headers={"content-type": "application/x-ndjson"})
    assert r.status_code == 200 and not r.json()["errors"]
    yield c, client, x


def _knn(vec, k, flt=None):
    spec = {"vector": [float(v) for v in vec], "k": k}
    if flt is not None:
        spec["filter"] = flt
    return {"size": k, "query": {"knn": {"embedding": spec}}}


def test_shim_knn_filter(app):
    c, client, x = app
    q = x[1] + 0.01
    plain = c.post("/idx/_search", json=_knn(q, 5)).json()["hits"]["hits"]
    assert plain[0]["_id"] == "d0_1"
    for flt, docs in (({"term": {"doc_id": "d2"}}, {"d2"}),
                      ({"terms": {"doc_id": ["d1", "d3"]}}, {"d1", "d3"}),
                      ({"ids": {"values": ["d0_0", "d3_11"]}}, {"d0", "d3"}),
                      ({"bool": {"must_not": {"term": {"doc_id": "d0"}}}}, {"d1", "d2", "d3"}),
                      ({"bool": {"filter": {"terms": {"doc_id": ["d0", "d1"]}}, "must_not": {"ids": {"values": ["d0_1"]}}}}, {"d0", "d1"})):
        r = c.post("/idx/_search", json=_knn(q, 5, flt))
        assert r.status_code == 200, r.text
        hits = r.json()["hits"]["hits"]
        assert hits and {h["_source"]["doc_id"] for h in hits} <= docs
        scores = [h["_score"] for h in hits]
        assert scores == sorted(scores, reverse=True)
    ids = [h["_id"] for h in c.post("/idx/_search", json=_knn(q, 5, {"ids": {"values": ["d0_0", "d3_11"]}})).json()["hits"]["hits"]]
    assert sorted(ids) == ["d0_0", "d3_11"]
    # same query without the filter: exactly as before
    assert c.post("/idx/_search", json=_knn(q, 5)).json()["hits"]["hits"] == plain


def test_shim_filter_unknown_doc_is_empty(app):
    c, _client, x = app
    r = c.post("/idx/_search", json=_knn(x[0], 3, {"term": {"doc_id": "nope"}}))
    assert r.status_code == 200
    assert r.json()["hits"]["hits"] == [] and r.json()["hits"]["max_score"] is None


def test_shim_unserved_filter_is_400_before_the_batcher(app, monkeypatch):
    c, client, x = app
    n_calls = len(client.index("idx").vectors.calls)
    for flt in ({"match": {"text": "t1"}}, {"term": {"text": "t1"}}, {"range": {"doc_id": {"gte": "a"}}}, [1, 2]):
        r = c.post("/idx/_search", json=_knn(x[0], 3, flt))
        assert r.status_code == 400, (flt, r.text)
        assert r.json()["error"]["type"] == "parsing_exception"
    assert len(client.index("idx").vectors.calls) == n_calls


def test_batcher_never_mixes_filters(client):
    import asyncio
    _fill(client, n_docs=4, chunks=3)
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=50.0)
    rng = np.random.default_rng(5)
    qs = rng.standard_normal((6, DIM)).astype(np.float32)
    flts = [None, {"term": {"doc_id": "PMC1.txt"}}, {"term": {"doc_id": "PMC2.txt"}},
            None, {"term": {"doc_id": "PMC1.txt"}}, {"term": {"doc_id": "PMC2.txt"}}]

    async def run():
        return await asyncio.gather(*[b.search("idx", qs[i:i + 1], 3, "embedding", flts[i]) for i in range(6)])

    res = asyncio.run(run())
    calls = client.index("idx").vectors.calls
    assert sorted(c[0] for c in calls) == [2, 2, 2]                       # three device calls, one per filter
    assert sum(c[1] is None for c in calls) == 1
    assert sorted(c[1].tolist() for c in calls if c[1] is not None) == [[3, 4, 5], [6, 7, 8]]
    for i, hits in enumerate(res):
        if flts[i] is not None:
            assert {h["_source"]["doc_id"] for h in hits} == {flts[i]["term"]["doc_id"]}


def test_delete_by_query_uses_the_map(client):
    _fill(client)
    idx = client.index("idx")
    assert RT.delete_by_query(idx, {"query": {"terms": {"doc_id": ["PMC1.txt", "PMC4.txt"]}}}) == 8
    assert sorted(idx.row_of_id.values()) == [r for r in range(24) if r // 4 not in (1, 4)]
    with pytest.raises(ValueError):
        RT.delete_by_query(idx, {"query": {"bool": {"must": []}}})


def test_threads_share_the_map(client):
    _fill(client, n_docs=2, chunks=2)
    ix = RT.OpenSearchIndexer(client, "idx")
    rng = np.random.default_rng(9)
    errors = []

    def adder(t):
        try:
            for j in range(20):
                ix.add_embeddings(rng.standard_normal((1, DIM)).astype(np.float32), [{"doc_id": f"T{t}", "text": f"{j}"}])
        except Exception as e:            # pragma: no cover
            errors.append(e)

    ts = [threading.Thread(target=adder, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors
    # every add call names its chunk "T{t}_0": the second and later calls overwrite row of the first
    assert len(_rows(client, {"terms": {"doc_id": ["T0", "T1"]}})) == 2
