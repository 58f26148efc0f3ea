"""Radial k-NN on the host side (no GPU): the shim's ``knn.min_score`` / ``knn.max_distance``, the conversions to a cosine
floor, exact ``hits.total``, the 400s, batching of radial requests, and OpenSearchIndexer.search(min_score=).  The device
index is an oracle-backed stand-in whose ``range_search`` answers from an fp32 NumPy product."""
import asyncio
import json

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from semantic_query_engine_amd import shim

DIM = 16


class RangeVectors:
    """VectorIndex stand-in: top-k and radial search over the rows added so far (ids = positions)."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        self.dim, self.xn = dim, np.zeros((0, dim), np.float32)
        self.calls = []                                  # ("knn", B, k) / ("range", B, max_hits, thresholds)

    def __len__(self):
        return int(self.xn.shape[0])

    def ids(self):
        return np.arange(len(self), dtype=np.int64)

    @property
    def next_id(self):
        return len(self)

    def add(self, x):
        self.xn = np.concatenate([self.xn, R.normalize_rows(np.asarray(x, np.float32))], 0)

    def update(self, ids, x):
        self.xn[np.asarray(ids, np.int64)] = R.normalize_rows(np.asarray(x, np.float32))

    def get_rows(self, ids):
        return self.xn[np.asarray(ids, np.int64)]

    def search(self, q, k, nprobe=0, filter_ids=None):
        q = np.asarray(q, np.float32)
        self.calls.append(("knn", q.shape[0], k))
        cos, pos = R.exact_topk(self.xn, R.normalize_rows(q), k)
        return cos.astype(np.float32), pos.astype(np.int64)

    def range_search(self, q, min_cos, max_hits=10):
        q = np.asarray(q, np.float32)
        b = q.shape[0]
        t = np.broadcast_to(np.asarray(min_cos, np.float32), (b,)).copy()
        self.calls.append(("range", b, max_hits, t))
        c = R.normalize_rows(q) @ self.xn.T
        counts = np.zeros(b, np.int64)
        cos = np.full((b, max_hits), -np.inf, np.float32)
        ids = np.full((b, max_hits), -1, np.int64)
        for i in range(b):
            hit = np.nonzero(c[i] >= t[i])[0]
            order = hit[np.lexsort((hit, -c[i][hit]))]
            counts[i] = hit.size
            m = min(hit.size, max_hits)
            cos[i, :m], ids[i, :m] = c[i][order[:m]], order[:m]
        return counts, cos, ids


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", RangeVectors)
    return RT.GpuSearchClient(ctx=object(), dim=DIM)


def _cluster(n, seed=0):
    """n rows around one direction (cosines to it spread over ~[0.5, 1]), then the direction itself."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(DIM).astype(np.float32)
    x = d + rng.uniform(0.1, 1.0, (n, 1)).astype(np.float32) * rng.standard_normal((n, DIM)).astype(np.float32)
    return x.astype(np.float32), d


def test_conversions():
    assert RT.radial_min_cos(min_score=0.9) == np.float32(2.0 - 1.0 / 0.9)
    assert RT.radial_min_cos(min_score=1.0) == np.float32(1.0)
    assert RT.radial_min_cos(min_score=0.5) == np.float32(0.0)
    assert RT.radial_min_cos(min_score=0.0) == -np.inf and RT.radial_min_cos(min_score=-2) == -np.inf
    assert RT.radial_min_cos(max_distance=0.25) == np.float32(0.75)
    assert RT.radial_min_cos(max_distance=2.0) == np.float32(-1.0)
    assert RT.radial_min_cos(min_score=0.9).dtype == np.float32
    for bad in ({}, {"min_score": 0.5, "max_distance": 0.5}, {"min_score": float("nan")}, {"max_distance": float("nan")}):
        with pytest.raises(ValueError):
            RT.radial_min_cos(**bad)


def test_indexer_search_min_score(client):
    x, d = _cluster(40)
    docs = [{"doc_id": f"D{i}", "text": f"t{i}"} for i in range(40)]
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x, docs)
    q = d[None]
    c = (R.normalize_rows(q) @ R.normalize_rows(x).T)[0]
    s = np.sort(c)[::-1]
    floor = float(1.0 / (2.0 - (s[4] + s[5]) / 2))           # between the 5th and 6th best: 5 hits pass
    hits = ix.search(q, k=3, min_score=floor)
    assert len(hits) == 3 and all(h[1] >= floor for h in hits)
    hits = ix.search(q, k=10, min_score=floor)
    assert len(hits) == 5 and all(h[1] >= floor for h in hits)          # the floor cuts below k
    assert [h[0]["text"] for h in hits] == [docs[i]["text"] for i in np.argsort(-c)[:5]]
    assert ix.search(q, k=3, min_score=1.01) == []                       # cos >= 1.0099: nothing
    dist = float(1.0 - (s[1] + s[2]) / 2)                                 # 2 rows within that cosine distance
    assert len(ix.search(q, k=10, max_distance=dist)) == 2
    assert len(ix.search(q, k=3)) == 3                                    # plain top-k: unchanged
    with pytest.raises(ValueError):
        ix.search(q, k=3, min_score=0.9, max_distance=0.1)
    with pytest.raises(ValueError):
        ix.search(q, k=3, min_score=0.9, filter={"term": {"doc_id": "D1"}})
    kinds = [c[0] for c in client.index("idx").vectors.calls]
    assert kinds == ["range", "range", "range", "range", "knn"]


# ---------------------------------------------------------------- the shim


def _bulk(lines):
    return ("\n".join(json.dumps(x) for x in lines) + "\n").encode()


@pytest.fixture()
def app(client):
    with TestClient(shim.create_app(client, None, DIM)) as c:
        c.put("/idx", json={"mappings": {"properties": {"embedding": {"type": "knn_vector", "dimension": DIM}}}})
        x, d = _cluster(60, seed=3)
        lines = []
        for i in range(60):
            lines += [{"index": {"_index": "idx", "_id": f"r{i}"}},
                      {"doc_id": f"d{i}", "text": f"t{i}", "embedding": [float(v) for v in x[i]]}]
        r = c.post("/_bulk", content=_bulk(lines), headers={"content-type": "application/x-ndjson"})
        assert r.status_code == 200 and not r.json()["errors"]
        yield c, client, x, d


def _radial(vec, size=None, **spec):
    body = {"query": {"knn": {"embedding": {"vector": [float(v) for v in vec], **spec}}}}
    if size is not None:
        body["size"] = size
    return body


def _cos(x, d):
    return (R.normalize_rows(d[None]) @ R.normalize_rows(x).T)[0]


def test_shim_min_score(app):
    c, client, x, d = app
    cos = _cos(x, d)
    floor = 0.8
    want = int(np.sum(cos >= np.float32(2.0 - 1.0 / floor)))
    assert 5 < want < 60
    r = c.post("/idx/_search", json=_radial(d, size=5, min_score=floor))
    assert r.status_code == 200, r.text
    h = r.json()["hits"]
    assert h["total"] == {"value": want, "relation": "eq"}                # exact, beyond size
    assert len(h["hits"]) == 5 and all(x["_score"] >= floor - 1e-6 for x in h["hits"])
    assert h["max_score"] == h["hits"][0]["_score"]
    assert [x["_id"] for x in h["hits"]] == [f"r{i}" for i in np.argsort(-cos, kind="stable")[:5]]
    # no size: 10 hits by default
    r = c.post("/idx/_search", json=_radial(d, min_score=floor)).json()["hits"]
    assert len(r["hits"]) == min(10, want) and r["total"]["value"] == want
    # the unthresholded answer would hold rows below the floor
    r = c.post("/idx/_search", json=_radial(d, size=60, min_score=floor)).json()["hits"]
    assert len(r["hits"]) == want and min(x["_score"] for x in r["hits"]) >= floor - 1e-6
    # nothing above the floor: empty, total 0
    r = c.post("/idx/_search", json=_radial(d, size=5, min_score=1.5)).json()["hits"]
    assert r == {"total": {"value": 0, "relation": "eq"}, "max_score": None, "hits": []}


def test_shim_max_distance(app):
    c, client, x, d = app
    cos = _cos(x, d)
    dist = 0.3
    want = int(np.sum(cos >= np.float32(1.0 - dist)))
    r = c.post("/idx/_search", json=_radial(d, size=3, max_distance=dist)).json()["hits"]
    assert r["total"]["value"] == want and len(r["hits"]) == min(3, want)
    t = client.index("idx").vectors.calls[-1]
    assert t[0] == "range" and t[3][0] == np.float32(1.0 - dist)


def test_shim_radial_400s(app):
    c, client, x, d = app
    n = len(client.index("idx").vectors.calls)
    for spec in ({"k": 3, "min_score": 0.5}, {"k": 3, "max_distance": 0.5}, {"min_score": 0.5, "max_distance": 0.5}):
        r = c.post("/idx/_search", json=_radial(d, size=3, **spec))
        assert r.status_code == 400 and r.json()["error"]["type"] == "parsing_exception", (spec, r.text)
    r = c.post("/idx/_search", json=_radial(d, size=3, min_score=0.5, filter={"term": {"doc_id": "d1"}}))
    assert r.status_code == 400 and r.json()["error"]["type"] == "parsing_exception"
    r = c.post("/idx/_search", json=_radial(d, size=10001, min_score=0.5))
    assert r.status_code == 400
    assert len(client.index("idx").vectors.calls) == n                    # nothing reached the device


def test_shim_knn_without_k_unchanged(app):
    c, client, x, d = app
    r = c.post("/idx/_search", json=_radial(d, size=4)).json()["hits"]     # no k, no floor: size top hits
    assert len(r["hits"]) == 4 and r["total"]["value"] == 4
    assert client.index("idx").vectors.calls[-1][:3] == ("knn", 1, 4)
    r = c.post("/idx/_search", json=_radial(d)).json()["hits"]
    assert len(r["hits"]) == 10


def test_batcher_radial_calls(client):
    x, d = _cluster(30, seed=7)
    RT.OpenSearchIndexer(client, "idx").add_embeddings(x, [{"doc_id": f"D{i}", "text": f"t{i}"} for i in range(30)])
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=50.0)
    q = np.stack([d, d, d, d]).astype(np.float32)
    floors = [0.6, None, 0.9, None]
    sizes = [4, 3, 7, 5]

    async def run():
        return await asyncio.gather(*[b.search("idx", q[i:i + 1], sizes[i], "embedding", min_cos=floors[i]) for i in range(4)])

    res = asyncio.run(run())
    calls = client.index("idx").vectors.calls
    assert len(calls) == 2                                               # one radial call, one top-k call
    radial = [c for c in calls if c[0] == "range"][0]
    knn = [c for c in calls if c[0] == "knn"][0]
    assert radial[1] == 2 and radial[2] == 7 and radial[3].tolist() == [np.float32(0.6), np.float32(0.9)]
    assert knn[1:] == (2, 5)
    cos = _cos(x, d)
    for i in (0, 2):
        hits, total = res[i]
        assert total == int(np.sum(cos >= np.float32(floors[i])))
        assert len(hits) == min(sizes[i], total)
    assert len(res[1]) == 3 and len(res[3]) == 5
