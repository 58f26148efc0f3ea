"""Collapse on ``doc_id`` on the host side (no GPU): OpenSearchIndexer.search(collapse=), the lazy push of group keys, the
shim's ``collapse`` body, its 400s, ``hits.total`` and the batching of collapsed requests.  The device index is a stand-in
whose ``search_collapsed`` answers from an fp32 NumPy product over the keys it was given."""
import asyncio
import json

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from semantic_query_engine_amd import shim

DIM = 16
NONE = -(1 << 63)


class CollapseVectors:
    """VectorIndex stand-in: top-k and collapsed search over the rows added so far (ids = positions)."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        self.dim, self.xn = dim, np.zeros((0, dim), np.float32)
        self.keys = np.zeros(0, np.int64)
        self.calls = []                                  # ("knn", B, k) / ("collapsed", B, k) / ("set_keys", [ids])

    def __len__(self):
        return int(self.xn.shape[0])

    def ids(self):
        return np.arange(len(self), dtype=np.int64)

    @property
    def next_id(self):
        return len(self)

    def add(self, x):
        x = np.asarray(x, np.float32)
        self.xn = np.concatenate([self.xn, R.normalize_rows(x)], 0)
        self.keys = np.concatenate([self.keys, np.full(x.shape[0], NONE, np.int64)])

    def update(self, ids, x):
        self.xn[np.asarray(ids, np.int64)] = R.normalize_rows(np.asarray(x, np.float32))

    def get_rows(self, ids):
        return self.xn[np.asarray(ids, np.int64)]

    def set_keys(self, ids, keys):
        ids = np.asarray(ids, np.int64)
        assert ids.size == 0 or (ids.min() >= 0 and ids.max() < len(self))
        self.calls.append(("set_keys", ids.tolist()))
        self.keys[ids] = np.asarray(keys, np.int64)

    def search(self, q, k, nprobe=0, filter_ids=None):
        q = np.asarray(q, np.float32)
        self.calls.append(("knn", q.shape[0], k))
        cos, pos = R.exact_topk(self.xn, R.normalize_rows(q), k)
        return cos.astype(np.float32), pos.astype(np.int64)

    def search_collapsed(self, q, k):
        q = np.asarray(q, np.float32)
        b = q.shape[0]
        self.calls.append(("collapsed", b, k))
        c = R.normalize_rows(q) @ self.xn.T
        cos = np.full((b, k), -np.inf, np.float32)
        ids = np.full((b, k), -1, np.int64)
        keys = np.full((b, k), NONE, np.int64)
        for i in range(b):
            seen, j = set(), 0
            for r in np.lexsort((np.arange(len(self)), -c[i])):
                key = int(self.keys[r])
                if key != NONE and key in seen:
                    continue
                seen.add(key)
                cos[i, j], ids[i, j], keys[i, j] = c[i, r], r, key
                j += 1
                if j == k:
                    break
        return cos, ids, keys

    def save(self, path):
        np.save(path + ".npy", self.xn)                  # the rows only: keys are not part of a saved index
        open(path, "wb").close()

    @classmethod
    def load(cls, ctx, path):
        self = cls()
        self.xn = np.load(path + ".npy")
        self.keys = np.full(self.xn.shape[0], NONE, np.int64)
        return self


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", CollapseVectors)
    return RT.GpuSearchClient(ctx=object(), dim=DIM)


def _docs(n_docs=12, per=5, seed=0):
    """n_docs documents of `per` chunks around their own direction, and a query close to document 0, then 1, 2, ..."""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((n_docs, DIM)).astype(np.float32)
    q = (centre * np.r_[2.0, np.linspace(0.6, 0.2, n_docs - 1)][:, None].astype(np.float32)).sum(axis=0)
    x = np.repeat(centre, per, axis=0) + 0.2 * rng.standard_normal((n_docs * per, DIM)).astype(np.float32)
    docs = [{"doc_id": f"D{i // per}", "text": f"t{i}"} for i in range(n_docs * per)]
    return x.astype(np.float32), docs, q.astype(np.float32)


def _want(x, docs, q, k):
    """Brute force: the best chunk of every doc_id, best documents first -> [(doc_id, text)]."""
    c = (R.normalize_rows(q[None]) @ R.normalize_rows(x).T)[0]
    best = {}
    for r in np.lexsort((np.arange(len(docs)), -c)):
        best.setdefault(docs[r]["doc_id"], docs[r]["text"])
    return list(best.items())[:k]


def _set_key_rows(calls):
    return [c[1] for c in calls if c[0] == "set_keys"]


def test_indexer_collapse_one_hit_per_document(client):
    x, docs, q = _docs()
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x, docs)
    plain = ix.search(q[None], k=3)
    assert len({h[0]["doc_id"] for h in plain}) == 1                      # the three best chunks are one document
    hits = ix.search(q[None], k=3, collapse={"field": "doc_id"})
    assert [(h[0]["doc_id"], h[0]["text"]) for h in hits] == _want(x, docs, q, 3)
    assert len({h[0]["doc_id"] for h in hits}) == 3
    c = (R.normalize_rows(q[None]) @ R.normalize_rows(x).T)[0]
    for h in hits:                                                        # same tuple shape and _score rule as the plain search
        row = int(h[0]["text"][1:])
        assert set(h[0]) == {"doc_id", "text", "embedding"} and abs(h[1] - 1.0 / (2.0 - float(c[row]))) < 1e-6
    assert len(ix.search(q[None], k=50, collapse={"field": "doc_id"})) == 12   # fewer documents than k
    for bad in ({"filter": {"term": {"doc_id": "D1"}}}, {"min_score": 0.5}, {"max_distance": 0.5}):
        with pytest.raises(ValueError):
            ix.search(q[None], k=3, collapse={"field": "doc_id"}, **bad)
    for bad in ({"field": "text"}, {"field": "doc_id", "inner_hits": {"name": "x"}}, "doc_id"):
        with pytest.raises(ValueError):
            ix.search(q[None], k=3, collapse=bad)


def test_keys_are_pushed_lazily_and_once(client):
    x, docs, q = _docs()
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x[:40], docs[:40])
    vec = client.index("idx").vectors
    ix.search(q[None], k=3)
    assert _set_key_rows(vec.calls) == []                                 # a plain search sends no keys
    ix.search(q[None], k=3, collapse={"field": "doc_id"})
    assert _set_key_rows(vec.calls) == [list(range(40))]                  # the first collapsed search: every row
    ix.search(q[None], k=3, collapse={"field": "doc_id"})
    assert _set_key_rows(vec.calls) == [list(range(40))]                  # nothing new: nothing sent
    ix.add_embeddings(x[40:], docs[40:])
    hits = ix.search(q[None], k=12, collapse={"field": "doc_id"})
    assert _set_key_rows(vec.calls) == [list(range(40)), list(range(40, 60))]   # only the rows added since
    assert [(h[0]["doc_id"], h[0]["text"]) for h in hits] == _want(x, docs, q, 12)
    keys = vec.keys
    assert all(len({int(keys[r]) for r in range(60) if docs[r]["doc_id"] == d}) == 1 for d in {d["doc_id"] for d in docs})
    assert len(set(keys.tolist())) == 12


def test_overwrite_that_changes_doc_id_resends_the_key(client):
    x, docs, q = _docs()
    idx = client.index("idx")
    by_id = lambda i, d: d["_id"]
    RT._commit_documents(idx, x, [{**d, "_id": f"r{i}"} for i, d in enumerate(docs)], by_id)
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.search(q[None], k=3, collapse={"field": "doc_id"})
    n_calls = len(_set_key_rows(idx.vectors.calls))
    # row 7 (document D1) is overwritten as a chunk of a NEW document close to the query; row 8 keeps its document
    moved = dict(docs[7], doc_id="NEW", _id="r7")
    same = dict(docs[8], _id="r8")
    RT._commit_documents(idx, np.stack([q, x[8]]), [moved, same], by_id)
    hits = ix.search(q[None], k=3, collapse={"field": "doc_id"})
    assert _set_key_rows(idx.vectors.calls)[n_calls:] == [[7]]            # only the row whose doc_id changed
    x2, docs2 = x.copy(), [dict(d) for d in docs]
    x2[7], docs2[7]["doc_id"] = q, "NEW"
    assert [(h[0]["doc_id"], h[0]["text"]) for h in hits] == _want(x2, docs2, q, 3)
    assert hits[0][0]["doc_id"] == "NEW"


def test_load_index_then_collapse(client, monkeypatch, tmp_path):
    x, docs, q = _docs()
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x, docs)
    ix.search(q[None], k=3, collapse={"field": "doc_id"})
    client.save_index("idx", str(tmp_path))
    client2 = RT.GpuSearchClient(ctx=object(), dim=DIM)
    assert client2.load_index("idx", str(tmp_path))
    vec = client2.index("idx").vectors
    assert np.all(vec.keys == NONE)                                       # a loaded index has no keys ...
    hits = RT.OpenSearchIndexer(client2, "idx").search(q[None], k=4, collapse={"field": "doc_id"})
    assert _set_key_rows(vec.calls) == [list(range(60))]                  # ... the docstore supplies them, nothing extra to call
    assert [(h[0]["doc_id"], h[0]["text"]) for h in hits] == _want(x, docs, q, 4)


# ---------------------------------------------------------------- the shim
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


def _knn(vec, size=None, collapse=None, **spec):
    body = {"query": {"knn": {"embedding": {"vector": [float(v) for v in vec], **spec}}}}
    if size is not None:
        body["size"] = size
    if collapse is not None:
        body["collapse"] = collapse
    return body


def test_shim_collapse(app):
    c, client, x, docs, q = app
    r = c.post("/idx/_search", json=_knn(q, size=4, k=4, collapse={"field": "doc_id"}))
    assert r.status_code == 200, r.text
    h = r.json()["hits"]
    assert [(x_["_source"]["doc_id"], x_["_source"]["text"]) for x_ in h["hits"]] == _want(x, docs, q, 4)
    assert h["total"] == {"value": 4, "relation": "eq"} and h["max_score"] == h["hits"][0]["_score"]
    assert [x_["_id"] for x_ in h["hits"]] == [f"r{t[1:]}" for _, t in _want(x, docs, q, 4)]
    assert set(h["hits"][0]["_source"]) == {"doc_id", "text", "embedding"}
    # more documents asked for than there are: total as the plain k-NN search reports it (the hits returned)
    h = c.post("/idx/_search", json=_knn(q, size=50, collapse={"field": "doc_id"})).json()["hits"]
    assert len(h["hits"]) == 12 and h["total"]["value"] == 12
    # the plain search is unchanged
    h = c.post("/idx/_search", json=_knn(q, size=3, k=3)).json()["hits"]
    assert len({x_["_source"]["doc_id"] for x_ in h["hits"]}) == 1
    # an overwrite through the bulk call that moves a chunk to another document
    line = [{"index": {"_index": "idx", "_id": "r7"}}, {"doc_id": "NEW", "text": "moved", "embedding": [float(v) for v in q]}]
    assert not c.post("/_bulk", content=_bulk(line), headers={"content-type": "application/x-ndjson"}).json()["errors"]
    n_calls = len(_set_key_rows(client.index("idx").vectors.calls))
    h = c.post("/idx/_search", json=_knn(q, size=2, collapse={"field": "doc_id"})).json()["hits"]
    assert h["hits"][0]["_source"]["doc_id"] == "NEW" and h["hits"][0]["_id"] == "r7"
    assert _set_key_rows(client.index("idx").vectors.calls)[n_calls:] == [[7]]


def test_shim_collapse_400s(app):
    c, client, x, docs, q = app
    n = len(client.index("idx").vectors.calls)
    bodies = [_knn(q, size=3, collapse={"field": "text"}),
              _knn(q, size=3, collapse={"field": "doc_id", "inner_hits": {"name": "chunks"}}),
              _knn(q, size=3, collapse="doc_id"),
              _knn(q, size=3, collapse={"field": "doc_id"}, filter={"term": {"doc_id": "D1"}}),
              _knn(q, size=3, collapse={"field": "doc_id"}, min_score=0.5),
              _knn(q, size=3, collapse={"field": "doc_id"}, max_distance=0.5),
              _knn(q, size=257, collapse={"field": "doc_id"})]
    for body in bodies:
        r = c.post("/idx/_search", json=body)
        assert r.status_code == 400, (body.get("collapse"), r.text)
        err = r.json()
        assert err["status"] == 400 and err["error"]["type"] in ("parsing_exception", "illegal_argument_exception")
        assert err["error"]["root_cause"][0]["type"] == err["error"]["type"]
    assert len(client.index("idx").vectors.calls) == n                    # nothing reached the device


def test_batcher_one_device_call_for_concurrent_collapsed_requests(client):
    x, docs, q = _docs()
    RT.OpenSearchIndexer(client, "idx").add_embeddings(x, docs)
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=100.0)
    rng = np.random.default_rng(5)
    qs = (q[None] + 0.3 * rng.standard_normal((40, DIM))).astype(np.float32)
    sizes = [1 + i % 5 for i in range(40)]

    async def run():
        collapsed = [b.search("idx", qs[i:i + 1], sizes[i], "embedding", collapse=True) for i in range(32)]
        plain = [b.search("idx", qs[i:i + 1], sizes[i], "embedding") for i in range(32, 40)]
        return await asyncio.gather(*collapsed, *plain)

    res = asyncio.run(run())
    calls = [c for c in client.index("idx").vectors.calls if c[0] in ("knn", "collapsed")]
    assert sorted(calls) == [("collapsed", 32, 5), ("knn", 8, 5)]          # ONE device call for the 32, never mixed with plain ones
    assert b.batches == 2 and sorted(b.batch_sizes) == [8, 32]
    for i in range(32):
        assert [(h["_source"]["doc_id"], h["_source"]["text"]) for h in res[i]] == _want(x, docs, qs[i], sizes[i])
    for i in range(32, 40):
        assert len(res[i]) == sizes[i]
