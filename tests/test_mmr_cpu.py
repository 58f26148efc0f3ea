"""MMR search on the host side (no GPU): the float64 reference of tests/mmr_reference.py on a hand-worked case and on its
two structural properties, OpenSearchIndexer.search(mmr=), the shim's ``ext.mmr`` body, its 400s and the batching of MMR
requests.  The device index is a stand-in whose ``search_mmr`` answers with the reference over an fp32 NumPy product."""
import asyncio
import json

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from semantic_query_engine_amd import shim

from . import mmr_reference as M

DIM = 16


# ---------------------------------------------------------------- the reference itself
def test_reference_hand_worked_case():
    c = [0.9, 0.85, 0.8, 0.5, 0.3]
    S = np.eye(5)
    for (i, j), v in {(0, 1): 0.95, (0, 2): 0.2, (0, 3): 0.1, (0, 4): 0.0, (1, 2): 0.3, (1, 3): 0.1, (1, 4): 0.0,
                      (2, 3): 0.9, (2, 4): 0.1, (3, 4): 0.2}.items():
        S[i, j] = S[j, i] = v
    # t0: 0.5 c -> row 0 (0.45).  t1: pen = S[:, 0]: -0.05, 0.3, 0.2, 0.15 -> row 2.  t2: pen(1) = 0.95, pen(3) = 0.9,
    # pen(4) = 0.1: -0.05, -0.2, 0.1 -> row 4.  t3: row 1 (-0.05), then row 3 (0.25 - 0.45 = -0.2)
    order, objs, margins = M.greedy(c, S, 0.5, 5)
    assert order.tolist() == [0, 2, 4, 1, 3]
    assert np.allclose(objs, [0.45, 0.3, 0.1, -0.05, -0.2], atol=1e-12)
    assert np.allclose(margins[:4], [0.025, 0.1, 0.15, 0.15], atol=1e-12) and np.isinf(margins[4])
    # a tie goes to the lower rank: two identical candidates at lam = 1
    assert M.greedy([0.5, 0.5, 0.4], np.eye(3), 1.0, 2)[0].tolist() == [0, 1]
    # lam = 0: the first pick is the best hit (every objective is 0), then the least similar row
    assert M.greedy(c, S, 0.0, 2)[0].tolist() == [0, 4]


def _random_case(seed, n=40, dim=24):
    rng = np.random.default_rng(seed)
    rows = M.norm64(rng.standard_normal((n, dim)) + 2.0 * rng.standard_normal(dim))
    q = M.norm64(rng.standard_normal(dim))
    c = rows @ q
    order = np.lexsort((np.arange(n), -c))
    return c[order], rows[order] @ rows[order].T


def test_reference_lambda_one_is_topk_and_prefix_stable():
    for seed in range(5):
        c, S = _random_case(seed)
        assert M.greedy(c, S, 1.0, 12)[0].tolist() == list(range(12))
        for lam in (0.0, 0.3, 0.7):
            full = M.greedy(c, S, lam, 40)[0]
            assert full[0] == 0 and sorted(full.tolist()) == list(range(40))
            for k in (1, 5, 17):
                assert M.greedy(c, S, lam, k)[0].tolist() == full[:k].tolist()
        assert M.greedy(c, S, 0.3, 12)[0].tolist() != list(range(12))          # the penalty changes something


# ---------------------------------------------------------------- the retrieval client and the shim
class MmrVectors:
    """VectorIndex stand-in: top-k and MMR search over the rows added so far (ids = positions)."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        self.dim, self.xn = dim, np.zeros((0, dim), np.float32)
        self.calls = []                                  # ("knn", B, k) / ("mmr", B, k, n_cand, [lam])

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

    def search_mmr(self, q, k, lam=0.5, n_cand=0, nprobe=0):
        q = np.asarray(q, np.float32)
        b = q.shape[0]
        lam = np.broadcast_to(np.asarray(lam, np.float32), (b,))
        self.calls.append(("mmr", b, k, n_cand, [round(float(v), 6) for v in lam]))
        n = n_cand if n_cand else min(256, max(32, 4 * k))
        assert k <= n <= 256 and np.all((lam >= 0) & (lam <= 1))
        c = R.normalize_rows(q) @ self.xn.T
        cos = np.full((b, k), -np.inf, np.float32)
        ids = np.full((b, k), -1, np.int64)
        obj = np.full((b, k), -np.inf, np.float32)
        for i in range(b):
            top = np.lexsort((np.arange(len(self)), -c[i]))[:n]
            order, objs, _ = M.greedy(c[i, top], self.xn[top].astype(np.float64) @ self.xn[top].astype(np.float64).T, lam[i], k)
            m = order.shape[0]
            cos[i, :m], ids[i, :m], obj[i, :m] = c[i, top[order]], top[order], objs
        return cos, ids, obj


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", MmrVectors)
    return RT.GpuSearchClient(ctx=object(), dim=DIM)


def _docs(n_docs=12, per=5, seed=0):
    """n_docs documents of `per` near-identical chunks around their own direction; the query is close to document 0, then 1, ..."""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((n_docs, DIM)).astype(np.float32)
    q = (centre * np.r_[2.0, np.linspace(0.6, 0.2, n_docs - 1)][:, None].astype(np.float32)).sum(axis=0)
    x = np.repeat(centre, per, axis=0) + 0.05 * rng.standard_normal((n_docs * per, DIM)).astype(np.float32)
    docs = [{"doc_id": f"D{i // per}", "text": f"t{i}"} for i in range(n_docs * per)]
    return x.astype(np.float32), docs, q.astype(np.float32)


def _want(x, q, k, lam, n):
    """The reference over the raw data -> row numbers in selection order."""
    xn = R.normalize_rows(x)
    c = (R.normalize_rows(q[None]) @ xn.T)[0]
    top = np.lexsort((np.arange(x.shape[0]), -c))[:n]
    order, _, _ = M.greedy(c[top], xn[top].astype(np.float64) @ xn[top].astype(np.float64).T, lam, k)
    return top[order].tolist()


def test_indexer_mmr_keyword(client):
    x, docs, q = _docs()
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x, docs)
    plain = ix.search(q[None], k=3)
    assert len({h[0]["doc_id"] for h in plain}) == 1                      # the three best chunks are one document
    hits = ix.search(q[None], k=3, mmr={"lambda": 0.5, "candidates": 32})
    assert [int(h[0]["text"][1:]) for h in hits] == _want(x, q, 3, 0.5, 32)
    assert hits[0][0]["text"] == plain[0][0]["text"]                      # the first pick is the best hit
    assert len({h[0]["doc_id"] for h in hits}) == 3                       # near-duplicates of the first pick are passed over
    c = (R.normalize_rows(q[None]) @ R.normalize_rows(x).T)[0]
    for h in hits:                                                        # same tuple shape and _score rule as the plain search
        row = int(h[0]["text"][1:])
        assert set(h[0]) == {"doc_id", "text", "embedding"} and abs(h[1] - 1.0 / (2.0 - float(c[row]))) < 1e-6
    vec = client.index("idx").vectors
    assert vec.calls[-1] == ("mmr", 1, 3, 32, [0.5])
    assert [h[0]["text"] for h in ix.search(q[None], k=3, mmr={"lambda": 1.0})] == [h[0]["text"] for h in plain]
    assert vec.calls[-1] == ("mmr", 1, 3, 0, [1.0])                       # candidates absent: automatic
    ix.search(q[None], k=3, mmr={})
    assert vec.calls[-1] == ("mmr", 1, 3, 0, [0.5])
    ix.search(q[None], k=3, mmr={"lambda": np.float32(0.25), "candidates": np.int64(40)})      # NumPy numbers are numbers
    assert vec.calls[-1] == ("mmr", 1, 3, 40, [0.25])
    n = len(vec.calls)
    for bad in ({"filter": {"term": {"doc_id": "D1"}}}, {"min_score": 0.5}, {"max_distance": 0.5}, {"collapse": {"field": "doc_id"}}):
        with pytest.raises(ValueError):
            ix.search(q[None], k=3, mmr={"lambda": 0.5}, **bad)
    for bad in ({"lambda": 1.5}, {"lambda": -0.1}, {"lambda": float("nan")}, {"lambda": "0.5"}, {"candidates": 2}, {"candidates": 257},
                {"candidates": 6.5}, {"diversity": 0.5}, "0.5"):
        with pytest.raises(ValueError):
            ix.search(q[None], k=3, mmr=bad)
    assert len(vec.calls) == n                                            # nothing reached the device


def _bulk(lines):
    return ("\n".join(json.dumps(x) for x in lines) + "\n").encode()


@pytest.fixture()
def app(client):
    with TestClient(shim.create_app(client, None, DIM)) as c:
        c.put("/idx", json={"mappings": {"properties": {"embedding": {"type": "knn_vector", "dimension": DIM}}}})
        x, docs, q = _docs()
        lines = []
        for i, d in enumerate(docs):
            lines += [{"index": {"_index": "idx", "_id": f"r{i}"}},
                      {"doc_id": d["doc_id"], "text": d["text"], "embedding": [float(v) for v in x[i]]}]
        r = c.post("/_bulk", content=_bulk(lines), headers={"content-type": "application/x-ndjson"})
        assert r.status_code == 200 and not r.json()["errors"]
        yield c, client, x, docs, q


def _knn(vec, size=None, ext=None, collapse=None, **spec):
    body = {"query": {"knn": {"embedding": {"vector": [float(v) for v in vec], **spec}}}}
    if size is not None:
        body["size"] = size
    if ext is not None:
        body["ext"] = ext
    if collapse is not None:
        body["collapse"] = collapse
    return body


def test_shim_ext_mmr(app):
    c, client, x, docs, q = app
    r = c.post("/idx/_search", json=_knn(q, size=4, k=4, ext={"mmr": {"candidates": 40, "diversity": 0.25}}))
    assert r.status_code == 200, r.text
    h = r.json()["hits"]
    want = _want(x, q, 4, 0.75, 40)                                        # lambda = 1 - diversity
    assert [x_["_id"] for x_ in h["hits"]] == [f"r{row}" for row in want]
    assert h["total"] == {"value": 4, "relation": "eq"} and h["max_score"] == h["hits"][0]["_score"]
    assert set(h["hits"][0]["_source"]) == {"doc_id", "text", "embedding"}
    assert client.index("idx").vectors.calls[-1] == ("mmr", 1, 4, 40, [0.75])
    # defaults: diversity 0.5, automatic depth
    r = c.post("/idx/_search", json=_knn(q, size=3, ext={"mmr": {}}))
    assert [x_["_id"] for x_ in r.json()["hits"]["hits"]] == [f"r{row}" for row in _want(x, q, 3, 0.5, 32)]
    assert client.index("idx").vectors.calls[-1] == ("mmr", 1, 3, 32, [0.5])      # the depth is resolved per request
    # an ext without mmr is ignored, as before the feature
    r = c.post("/idx/_search", json=_knn(q, size=3, k=3, ext={"rerank": {"model": "x"}}))
    assert r.status_code == 200 and client.index("idx").vectors.calls[-1] == ("knn", 1, 3)
    r = c.post("/idx/_search", json=_knn(q, size=3, ext={"rerank": {}, "mmr": {"candidates": 40}}))
    assert r.status_code == 200 and client.index("idx").vectors.calls[-1] == ("mmr", 1, 3, 40, [0.5])
    # diversity 0 is the plain search, and the plain search is unchanged
    plain = c.post("/idx/_search", json=_knn(q, size=3, k=3)).json()["hits"]["hits"]
    same = c.post("/idx/_search", json=_knn(q, size=3, k=3, ext={"mmr": {"diversity": 0}})).json()["hits"]["hits"]
    assert [x_["_id"] for x_ in same] == [x_["_id"] for x_ in plain] and len({x_["_source"]["doc_id"] for x_ in plain}) == 1


def test_shim_ext_mmr_400s(app):
    c, client, x, docs, q = app
    n = len(client.index("idx").vectors.calls)
    ok = {"mmr": {"candidates": 32, "diversity": 0.5}}
    bodies = [_knn(q, size=3, ext={"mmr": {"diversity": 1.5}}),
              _knn(q, size=3, ext={"mmr": {"diversity": -0.1}}),
              _knn(q, size=3, ext={"mmr": {"diversity": "0.5"}}),
              _knn(q, size=3, ext={"mmr": {"candidates": 2}}),
              _knn(q, size=3, ext={"mmr": {"candidates": 257}}),
              _knn(q, size=3, ext={"mmr": {"lambda": 0.5}}),
              _knn(q, size=3, ext={"mmr": 0.5}),
              _knn(q, size=3, ext=ok, filter={"term": {"doc_id": "D1"}}),
              _knn(q, size=3, ext=ok, min_score=0.5),
              _knn(q, size=3, ext=ok, max_distance=0.5),
              _knn(q, size=3, ext=ok, collapse={"field": "doc_id"}),
              _knn(q, size=257, ext={"mmr": {}})]
    for body in bodies:
        r = c.post("/idx/_search", json=body)
        assert r.status_code == 400, (body.get("ext"), r.text)
        err = r.json()
        assert err["status"] == 400 and err["error"]["type"] in ("parsing_exception", "illegal_argument_exception")
        assert err["error"]["root_cause"][0]["type"] == err["error"]["type"]
    assert len(client.index("idx").vectors.calls) == n                    # nothing reached the device


def test_batcher_one_device_call_per_depth(client):
    x, docs, q = _docs()
    RT.OpenSearchIndexer(client, "idx").add_embeddings(x, docs)
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=100.0)
    rng = np.random.default_rng(5)
    qs = (q[None] + 0.3 * rng.standard_normal((40, DIM))).astype(np.float32)
    sizes = [1 + i % 5 for i in range(40)]
    lams = [round(0.1 * (i % 11), 1) for i in range(40)]

    async def run():
        deep = [b.search("idx", qs[i:i + 1], sizes[i], "embedding", mmr=(lams[i], 48)) for i in range(24)]
        auto = [b.search("idx", qs[i:i + 1], sizes[i], "embedding", mmr=(lams[i], 0)) for i in range(24, 32)]   # 4 k <= 32
        plain = [b.search("idx", qs[i:i + 1], sizes[i], "embedding") for i in range(32, 40)]
        return await asyncio.gather(*deep, *auto, *plain)

    res = asyncio.run(run())
    calls = [c[:4] for c in client.index("idx").vectors.calls if c[0] in ("knn", "mmr")]
    # ONE device call per depth at the largest k, never mixed with plain requests
    assert sorted(calls, key=str) == sorted([("mmr", 24, 5, 48), ("mmr", 8, 5, 32), ("knn", 8, 5)], key=str)
    assert b.batches == 3 and sorted(b.batch_sizes) == [8, 8, 24]
    sent = {c[3]: c[4] for c in client.index("idx").vectors.calls if c[0] == "mmr"}
    assert sent[48] == [round(v, 6) for v in np.asarray(lams[:24], np.float32).tolist()]      # per-request weights, in order
    for i in range(32):                                                   # each request: its own k (prefix) and its own lambda
        n = 48 if i < 24 else 32
        assert [int(h["_source"]["text"][1:]) for h in res[i]] == _want(x, qs[i], sizes[i], np.float32(lams[i]), n), i
    for i in range(32, 40):
        assert len(res[i]) == sizes[i]


def test_batcher_automatic_depth_belongs_to_the_request(client):
    """Automatic depth is min(256, max(32, 4 k)) of the request's OWN k: requests of size 3 (depth 32), 16 (64) and 64 (256)
    that arrive together are answered as each would be alone, in one device call per depth."""
    x, docs, q = _docs(n_docs=80, per=5)
    RT.OpenSearchIndexer(client, "idx").add_embeddings(x, docs)
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=100.0)
    rng = np.random.default_rng(7)
    qs = (q[None] + 0.3 * rng.standard_normal((12, DIM))).astype(np.float32)
    sizes = [3, 16, 64] * 4
    assert [RT.mmr_depth(k, 0) for k in (3, 8, 9, 16, 64, 200)] == [32, 32, 36, 64, 256, 256] and RT.mmr_depth(3, 50) == 50

    async def run():
        return await asyncio.gather(*[b.search("idx", qs[i:i + 1], sizes[i], "embedding", mmr=(0.5, 0)) for i in range(12)])

    res = asyncio.run(run())
    calls = sorted(c[:4] for c in client.index("idx").vectors.calls if c[0] == "mmr")
    assert calls == [("mmr", 4, 3, 32), ("mmr", 4, 16, 64), ("mmr", 4, 64, 256)]
    alone = shim._SearchBatcher(client, max_batch=1, max_wait_ms=0.0)
    differ = 0
    for i in range(12):
        n = {3: 32, 16: 64, 64: 256}[sizes[i]]
        got = [int(h["_source"]["text"][1:]) for h in res[i]]
        assert got == _want(x, qs[i], sizes[i], 0.5, n), i
        assert got == [int(h["_source"]["text"][1:]) for h in asyncio.run(alone.search("idx", qs[i:i + 1], sizes[i], "embedding", mmr=(0.5, 0)))]
        differ += got[:3] != _want(x, qs[i], 3, 0.5, 256)[:3] if sizes[i] == 3 else 0
    print(f"[mmr] {differ} of 4 size-3 requests would have changed at the depth of the largest request")
