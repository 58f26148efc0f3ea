"""Fused multi-query search on the host side (no GPU): the NumPy reference of tests/fuse_reference.py on hand-worked cases and
on its structural properties, OpenSearchIndexer.search_multi, the shim's ``hybrid`` body, its 400s, the batching of hybrid
requests and the two new symbols of the ABI.  The device index is a stand-in whose ``search_fused`` answers with the reference
over an fp32 NumPy top-n."""
import asyncio
import json
import os

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from semantic_query_engine_amd import shim

from . import fuse_reference as F

DIM = 16
NINF = -np.inf
# T(1, r) = rint(2^40 / (60 + r)), worked by hand: 2^40 = 1099511627776 = 61 x 18024780783 + 13 = 62 x 17734058512 + 32
# (.516: up) = 63 x 17452565520 + 16 = 64 x 17179869184
T1, T2, T3, T4 = 18024780783, 17734058513, 17452565520, 17179869184

COS = [[0.9, 0.8, 0.7, 0.6], [0.95, 0.85, 0.6, 0.4], [0.99, 0.3, 0.2, NINF]]
IDS = [[10, 20, 30, 40], [20, 10, 50, 30], [10, 45, 35, -1]]          # 10 in all three lists; the third list is padded


# ---------------------------------------------------------------- the reference itself
def test_reference_terms():
    assert [int(F.rrf_term(1.0, 60, r)) for r in (1, 2, 3, 4)] == [T1, T2, T3, T4]
    assert int(F.rrf_term(64.0, 1, 1)) == 2 ** 45 and int(F.rrf_term(0.5, 60, 4)) == 2 ** 33
    assert int(F.rrf_term(1e-38, 60, 1)) == 0                                # a tiny weight adds nothing, the row is still listed
    assert int(F.rrf_term(1.0, 1, 2)) == 366503875925                        # 2^40 / 3 = ...925.33
    assert int(F.rrf_term(3.0, 6, 2)) == 412316860416                        # 3 x 2^40 / 8, exact


def test_reference_hand_worked_rrf():
    fused, ids, cos = F.fuse(COS, IDS, 8, "rrf", None, 60)
    # 10: ranks 1, 2, 1; 20: ranks 2, 1; 30: ranks 3, 4; 45: rank 2; 35 and 50: rank 3 each, the tie goes to the lower id; 40: rank 4
    want_int = [2 * T1 + T2, T1 + T2, T3 + T4, T2, T3, T3, T4]
    assert want_int == [53783620079, 35758839296, 34632434704, 17734058513, 17452565520, 17452565520, 17179869184]
    assert ids.tolist() == [10, 20, 30, 45, 35, 50, 40, -1]
    assert fused[:7].tolist() == [np.float32(v * 2.0 ** -40) for v in want_int] and np.isneginf(fused[7])
    assert cos[:7].tolist() == [np.float32(v) for v in (0.99, 0.95, 0.7, 0.3, 0.2, 0.6, 0.6)] and np.isneginf(cos[7])
    assert fused.dtype == np.float32 and ids.dtype == np.int64 and cos.dtype == np.float32
    # k below the number of distinct rows cuts the same ranking; the tie at the cut is resolved by id
    assert F.fuse(COS, IDS, 5, "rrf")[1].tolist() == [10, 20, 30, 45, 35]
    # weights: with the second list at 4 and the others at 0.01, its first row passes the row that is in all three lists
    w = [0.01, 4.0, 0.01]
    fused, ids, _ = F.fuse(COS, IDS, 2, "rrf", w, 60)
    assert ids.tolist() == [20, 10]
    assert fused.tolist() == [np.float32((int(F.rrf_term(0.01, 60, 2)) + int(F.rrf_term(4.0, 60, 1))) * 2.0 ** -40),
                              np.float32((2 * int(F.rrf_term(0.01, 60, 1)) + int(F.rrf_term(4.0, 60, 2))) * 2.0 ** -40)]
    assert int(F.rrf_term(4.0, 60, 1)) == 72099123133 and int(F.rrf_term(4.0, 60, 2)) == 70936234050      # 2^42 / 61, 2^42 / 62
    # another rank constant: c = 1 makes the first places count much more
    assert F.fuse(COS, IDS, 3, "rrf", None, 1)[1].tolist() == [10, 20, 30]


def test_reference_hand_worked_max():
    fused, ids, cos = F.fuse(COS, IDS, 8, "max")
    # best cosines: 10: 0.99, 20: 0.95, 30: 0.7, 40 and 50: 0.6 each (lower id first), 45: 0.3, 35: 0.2
    assert ids.tolist() == [10, 20, 30, 40, 50, 45, 35, -1]
    assert fused[:7].tolist() == [np.float32(v) for v in (0.99, 0.95, 0.7, 0.6, 0.6, 0.3, 0.2)]
    assert np.array_equal(fused.view(np.uint32), cos.view(np.uint32)) and np.isneginf(fused[7])
    with pytest.raises(ValueError):
        F.fuse(COS, IDS, 3, "max", [1.0, 1.0, 1.0])
    # no list, and lists of padding only: all padding
    for lists in (([], []), ([[NINF] * 3], [[-1] * 3])):
        fused, ids, cos = F.fuse(*lists, 2, "rrf")
        assert ids.tolist() == [-1, -1] and np.all(np.isneginf(fused)) and np.all(np.isneginf(cos))


def _random_lists(seed, m=6, n=12, universe=30):
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(universe)[:n] for _ in range(m)]).astype(np.int64) + 2 ** 40
    cos = -np.sort(-rng.uniform(-1, 1, (m, n)).astype(np.float32), axis=1)
    short = rng.integers(0, m)
    ids[short, n - 3:], cos[short, n - 3:] = -1, NINF                      # one padded list
    return cos, ids, rng.uniform(0.1, 8.0, m).astype(np.float32)


def test_reference_permutation_invariance():
    for seed in range(5):
        cos, ids, w = _random_lists(seed)
        p = np.random.default_rng(100 + seed).permutation(cos.shape[0])
        for mode, wt in (("rrf", w), ("rrf", None), ("max", None)):
            a = F.fuse(cos, ids, 10, mode, wt)
            b = F.fuse(cos[p], ids[p], 10, mode, None if wt is None else wt[p])
            assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a, b)), (seed, mode)


def test_reference_one_list():
    for seed in range(5):
        cos, ids, _ = _random_lists(seed, m=1)
        fused, out, best = F.fuse(cos, ids, 12, "max")                       # m = 1 with MAX: the list itself
        assert np.array_equal(out, ids[0]) and np.array_equal(fused.view(np.uint32), cos[0].view(np.uint32))
        assert np.array_equal(best.view(np.uint32), cos[0].view(np.uint32))
        assert np.array_equal(F.fuse(cos, ids, 12, "rrf")[1], ids[0])       # m = 1 with RRF: the list's order
        twice = F.fuse(np.repeat(cos, 2, 0), np.repeat(ids, 2, 0), 12, "max")   # a list repeated in MAX changes nothing
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(twice, (fused, out, best)))


# ---------------------------------------------------------------- the retrieval client and the shim
class FuseVectors:
    """VectorIndex stand-in: top-k and fused search over the rows added so far (ids = positions)."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        self.dim, self.xn = dim, np.zeros((0, dim), np.float32)
        self.calls = []                                  # ("knn", B, k) / ("fused", Bs, offsets, k, mode, depth, c, weights)

    def __len__(self):
        return int(self.xn.shape[0])

    def ids(self):
        return np.arange(len(self), dtype=np.int64)

    @property
    def next_id(self):
        return len(self)

    def add(self, x):
        self.xn = np.concatenate([self.xn, R.normalize_rows(np.asarray(x, np.float32))], 0)

    def get_rows(self, ids):
        return self.xn[np.asarray(ids, np.int64)]

    def _topk(self, q, k):
        cos, pos = R.exact_topk(self.xn, R.normalize_rows(np.asarray(q, np.float32)), k)
        return cos.astype(np.float32), pos.astype(np.int64)

    def search(self, q, k, nprobe=0, filter_ids=None):
        self.calls.append(("knn", np.asarray(q).shape[0], k))
        return self._topk(q, k)

    def search_fused(self, q, k, offsets=None, mode="rrf", weights=None, depth=0, rank_constant=60, nprobe=0):
        q = np.asarray(q, np.float32)
        offsets = [0, q.shape[0]] if offsets is None else [int(v) for v in offsets]
        self.calls.append(("fused", q.shape[0], offsets, k, mode, depth, rank_constant,
                           None if weights is None else [round(float(v), 6) for v in weights]))
        n = depth if depth else (k if mode == "max" else min(256, max(32, 4 * k)))
        assert 1 <= k <= n <= 256 and all(0 <= b - a <= 32 and (b - a) * n <= 2048 for a, b in zip(offsets, offsets[1:]))
        cos, ids = self._topk(q, min(n, len(self)))
        return F.fuse_groups(cos, ids, offsets, k, mode, weights, rank_constant)


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", FuseVectors)
    return RT.GpuSearchClient(ctx=object(), dim=DIM)


def _docs(n_docs=12, per=5, seed=0):
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal((n_docs, DIM)).astype(np.float32)
    x = np.repeat(centre, per, axis=0) + 0.3 * rng.standard_normal((n_docs * per, DIM)).astype(np.float32)
    docs = [{"doc_id": f"D{i // per}", "text": f"t{i}"} for i in range(n_docs * per)]
    qs = (centre[[0, 0, 1, 2]] + 0.5 * rng.standard_normal((4, DIM))).astype(np.float32)      # rephrasings around documents 0, 1, 2
    return x.astype(np.float32), docs, qs


def _want(x, qs, k, mode="rrf", weights=None, depth=0, c=60):
    """The reference over the raw data -> (row numbers in fused order, fused scores, best cosines)."""
    n = depth if depth else (k if mode == "max" else min(256, max(32, 4 * k)))
    cos, pos = R.exact_topk(R.normalize_rows(x), R.normalize_rows(qs), min(n, x.shape[0]))
    fused, ids, best = F.fuse(cos.astype(np.float32), pos.astype(np.int64), k, mode, weights, c)
    return ids.tolist(), fused, best


def test_indexer_search_multi(client):
    x, docs, qs = _docs()
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x, docs)
    vec = client.index("idx").vectors
    hits = ix.search_multi(qs, k=5)
    rows, _, best = _want(x, qs, 5)
    assert [int(h[0]["text"][1:]) for h in hits] == rows
    for h, c in zip(hits, best):                                             # same tuple shape and _score rule as search
        assert set(h[0]) == {"doc_id", "text", "embedding"} and abs(h[1] - 1.0 / (2.0 - float(c))) < 1e-6
    assert vec.calls[-1] == ("fused", 4, [0, 4], 5, "rrf", 32, 60, None)     # defaults: rrf, constant 60, automatic depth
    hits = ix.search_multi(qs, k=5, fusion={"method": "max"})
    assert [int(h[0]["text"][1:]) for h in hits] == _want(x, qs, 5, "max")[0]
    assert vec.calls[-1] == ("fused", 4, [0, 4], 5, "max", 5, 60, None)
    hits = ix.search_multi(qs, k=3, fusion={"method": "rrf", "rank_constant": 10, "window": 40, "weights": [1, 1, 8, np.float32(0.5)]})
    assert [int(h[0]["text"][1:]) for h in hits] == _want(x, qs, 3, "rrf", [1, 1, 8, 0.5], 40, 10)[0]
    assert vec.calls[-1] == ("fused", 4, [0, 4], 3, "rrf", 40, 10, [1.0, 1.0, 8.0, 0.5])
    assert [h[0]["text"] for h in ix.search_multi(qs[0], k=3, fusion={"method": "max"})] == [h[0]["text"] for h in ix.search(qs[0:1], k=3)]
    n = len(vec.calls)
    for bad in ({"method": "mean"}, {"rank_constant": 0}, {"rank_constant": 10001}, {"rank_constant": 1.5}, {"window": 2}, {"window": 257},
                {"weights": [1, 1, 1]}, {"weights": [1, 1, 1, 0]}, {"weights": [1, 1, 1, 65]}, {"weights": [1, 1, 1, float("nan")]},
                {"weights": [1, 1, 1, "1"]}, {"method": "max", "weights": [1, 1, 1, 1]}, {"normalization": "min_max"}, "rrf"):
        with pytest.raises(ValueError):
            ix.search_multi(qs, k=3, fusion=bad)
    with pytest.raises(ValueError):
        ix.search_multi(np.zeros((33, DIM), np.float32), k=3)                 # more than 32 sub-queries
    with pytest.raises(ValueError):
        ix.search_multi(np.zeros((9, DIM), np.float32), k=3, fusion={"window": 256})      # 9 x 256 > 2048
    assert len(vec.calls) == n                                               # nothing reached the device


def _bulk(lines):
    return ("\n".join(json.dumps(x) for x in lines) + "\n").encode()


@pytest.fixture()
def app(client):
    with TestClient(shim.create_app(client, None, DIM)) as c:
        c.put("/idx", json={"mappings": {"properties": {"embedding": {"type": "knn_vector", "dimension": DIM}}}})
        x, docs, qs = _docs()
        lines = []
        for i, d in enumerate(docs):
            lines += [{"index": {"_index": "idx", "_id": f"r{i}"}},
                      {"doc_id": d["doc_id"], "text": d["text"], "embedding": [float(v) for v in x[i]]}]
        r = c.post("/_bulk", content=_bulk(lines), headers={"content-type": "application/x-ndjson"})
        assert r.status_code == 200 and not r.json()["errors"]
        yield c, client, x, docs, qs


def _sub(vec, **spec):
    return {"knn": {"embedding": {"vector": [float(v) for v in vec], **spec}}}


def _hybrid(qs, size=None, fusion=None, k=None, **top):
    body = {"query": {"hybrid": {"queries": [_sub(v, **({} if k is None else {"k": k})) for v in qs]}}, **top}
    if size is not None:
        body["size"] = size
    if fusion is not None:
        body["ext"] = {"fusion": fusion}
    return body


def test_shim_hybrid(app):
    c, client, x, docs, qs = app
    vec = client.index("idx").vectors
    r = c.post("/idx/_search", json=_hybrid(qs, size=5))
    assert r.status_code == 200, r.text
    h = r.json()["hits"]
    rows, fused, best = _want(x, qs, 5)
    assert [x_["_id"] for x_ in h["hits"]] == [f"r{row}" for row in rows]
    assert [x_["fields"]["_fused"] for x_ in h["hits"]] == [[float(v)] for v in fused]
    for x_, cb in zip(h["hits"], best):                                      # _score comes from the best cosine, as for knn
        assert abs(x_["_score"] - 1.0 / (2.0 - float(cb))) < 1e-6 and set(x_["_source"]) == {"doc_id", "text", "embedding"}
    assert h["total"] == {"value": 5, "relation": "eq"} and h["max_score"] == max(x_["_score"] for x_ in h["hits"])
    assert vec.calls[-1] == ("fused", 4, [0, 4], 5, "rrf", 32, 60, None)     # default: rrf with constant 60
    # without size the smallest k of the sub-queries is the k
    body = _hybrid(qs, fusion={"method": "max"})
    for sub, k in zip(body["query"]["hybrid"]["queries"], (7, 4, 9, 6)):
        sub["knn"]["embedding"]["k"] = k
    r = c.post("/idx/_search", json=body)
    assert [x_["_id"] for x_ in r.json()["hits"]["hits"]] == [f"r{row}" for row in _want(x, qs, 4, "max")[0]]
    assert vec.calls[-1] == ("fused", 4, [0, 4], 4, "max", 4, 60, None)
    # every option
    r = c.post("/idx/_search", json=_hybrid(qs, size=3, fusion={"method": "rrf", "rank_constant": 10, "window": 40, "weights": [1, 1, 8, 0.5]}))
    rows, fused, _ = _want(x, qs, 3, "rrf", [1, 1, 8, 0.5], 40, 10)
    assert [x_["_id"] for x_ in r.json()["hits"]["hits"]] == [f"r{row}" for row in rows]
    assert [x_["fields"]["_fused"][0] for x_ in r.json()["hits"]["hits"]] == [float(v) for v in fused]
    assert vec.calls[-1] == ("fused", 4, [0, 4], 3, "rrf", 40, 10, [1.0, 1.0, 8.0, 0.5])
    # one sub-query is served too, and the plain knn body is unchanged
    r = c.post("/idx/_search", json=_hybrid(qs[:1], size=3, fusion={"method": "max"}))
    plain = c.post("/idx/_search", json={"size": 3, "query": _sub(qs[0], k=3)})
    assert [x_["_id"] for x_ in r.json()["hits"]["hits"]] == [x_["_id"] for x_ in plain.json()["hits"]["hits"]]
    assert vec.calls[-1] == ("knn", 1, 3) and "fields" not in plain.json()["hits"]["hits"][0]


def test_shim_body_that_is_no_object_is_still_a_400(app):
    """The hybrid dispatch looks at the body before the knn parser does: a JSON body that is not an object stays the 400
    parsing_exception it was."""
    c, client, x, docs, qs = app
    n = len(client.index("idx").vectors.calls)
    for raw in ("[]", "[1]", '"x"', "3", "null", '{"query": []}', '{"query": "hybrid"}', '{"query": {"hybrid": []}}'):
        r = c.post("/idx/_search", content=raw, headers={"content-type": "application/json"})
        assert r.status_code == 400 and r.json()["error"]["type"] == "parsing_exception", (raw, r.text)
    assert len(client.index("idx").vectors.calls) == n


def test_shim_hybrid_400s(app):
    c, client, x, docs, qs = app
    n = len(client.index("idx").vectors.calls)
    nan = [float(v) for v in qs[0]]
    nan[3] = "NaN"
    bodies = [{"query": {"hybrid": {"queries": [_sub(qs[0]), {"match": {"text": "x"}}]}}},                # a non-knn sub-query
              {"query": {"hybrid": {"queries": [_sub(qs[0]), {"term": {"doc_id": "D1"}}]}}},
              {"query": {"hybrid": {"queries": [_sub(qs[0]), _sub(qs[1], filter={"term": {"doc_id": "D1"}})]}}},
              {"query": {"hybrid": {"queries": [_sub(qs[0]), _sub(qs[1], min_score=0.5)]}}},
              {"query": {"hybrid": {"queries": [_sub(qs[0]), _sub(qs[1], max_distance=0.5)]}}},
              _hybrid(qs, size=3, collapse={"field": "doc_id"}),
              {**_hybrid(qs, size=3), "ext": {"mmr": {"candidates": 32}}},
              {"query": {"hybrid": {"queries": []}}},
              {"query": {"hybrid": {}}},
              {"query": {"hybrid": {"queries": [_sub(qs[0])] * 33}}},                                     # more than 32 sub-queries
              {"query": {"hybrid": {"queries": [_sub(qs[0]), {"knn": {"other": {"vector": [0.0] * DIM}}}]}}},   # two fields
              {"query": {"hybrid": {"queries": [_sub(qs[0]), _sub(qs[1][:5])]}}},                         # a short vector
              {"query": {"hybrid": {"queries": [_sub(qs[0]), {"knn": {"embedding": {"vector": [[0.0] * DIM]}}}]}}},
              {"query": {"hybrid": {"queries": [_sub(qs[0]), {"knn": {"embedding": {"vector": nan}}}]}}},
              _hybrid(qs, size=0), _hybrid(qs, size=257),
              _hybrid(qs, size=3, fusion={"method": "mean"}),
              _hybrid(qs, size=3, fusion={"rank_constant": 0}),
              _hybrid(qs, size=3, fusion={"window": 2}),
              _hybrid(qs, size=3, fusion={"window": 257}),
              _hybrid(qs, size=3, fusion={"weights": [1, 1]}),
              _hybrid(qs, size=3, fusion={"weights": [1, 1, 1, -1]}),
              _hybrid(qs, size=3, fusion={"method": "max", "weights": [1, 1, 1, 1]}),
              _hybrid(qs, size=3, fusion={"normalization": "min_max"}),
              _hybrid(np.repeat(qs, 3, 0), size=3, fusion={"window": 256})]                               # 12 x 256 > 2048
    for body in bodies:
        r = c.post("/idx/_search", json=body)
        assert r.status_code == 400, (str(body)[:200], r.text)
        err = r.json()
        assert err["status"] == 400 and err["error"]["type"] in ("parsing_exception", "illegal_argument_exception")
        assert err["error"]["root_cause"][0]["type"] == err["error"]["type"]
    for body in bodies[:7]:                                                  # the combinations the issue names: parsing_exception
        assert c.post("/idx/_search", json=body).json()["error"]["type"] == "parsing_exception"
    assert len(client.index("idx").vectors.calls) == n                       # nothing reached the device


def test_batcher_concurrent_hybrid_requests_share_one_call(client):
    x, docs, qs = _docs()
    RT.OpenSearchIndexer(client, "idx").add_embeddings(x, docs)
    b = shim._SearchBatcher(client, max_batch=64, max_wait_ms=100.0)
    rng = np.random.default_rng(5)
    groups = [(qs[: 1 + i % 4] + 0.3 * rng.standard_normal((1 + i % 4, DIM))).astype(np.float32) for i in range(12)]
    weights = [None if i % 2 else [float(1 + j) for j in range(1 + i % 4)] for i in range(12)]

    async def run():
        two = [b.search("idx", groups[i], 5, "embedding", fusion=("rrf", 60, 32, weights[i])) for i in range(2)]
        more = [b.search("idx", groups[i], 5, "embedding", fusion=("rrf", 60, 32, weights[i])) for i in range(2, 8)]
        other_c = [b.search("idx", groups[i], 5, "embedding", fusion=("rrf", 10, 32, None)) for i in range(8, 10)]
        other_m = [b.search("idx", groups[10], 5, "embedding", fusion=("max", 60, 5, None))]
        other_k = [b.search("idx", groups[11], 4, "embedding", fusion=("rrf", 60, 32, None))]
        plain = [b.search("idx", groups[0][:1], 5, "embedding")]
        return await asyncio.gather(*two, *more, *other_c, *other_m, *other_k, *plain)

    res = asyncio.run(run())
    calls = [c for c in client.index("idx").vectors.calls if c[0] in ("knn", "fused")]
    fused = sorted((c for c in calls if c[0] == "fused"), key=lambda c: -c[1])
    ms = [g.shape[0] for g in groups]
    # ONE device call for the eight requests of equal (k, method, window, rank_constant), each a logical query of its own
    assert fused[0][:7] == ("fused", sum(ms[:8]), np.concatenate([[0], np.cumsum(ms[:8])]).tolist(), 5, "rrf", 32, 60)
    assert fused[0][7] == [v for i in range(8) for v in (weights[i] or [1.0] * ms[i])]
    assert sorted(c[1:2] + c[3:7] for c in fused[1:]) == sorted([(ms[8] + ms[9], 5, "rrf", 32, 10), (ms[10], 5, "max", 5, 60),
                                                                  (ms[11], 4, "rrf", 32, 60)])
    assert len(calls) == 5 and b.batches == 5 and sorted(b.batch_sizes) == [1, 1, 1, 2, 8]
    for i in range(12):                                                      # every request is answered as it would be alone
        mode, c, k = ("max", 60, 5) if i == 10 else ("rrf", 10 if i in (8, 9) else 60, 4 if i == 11 else 5)
        rows, fs, _ = _want(x, groups[i], k, mode, weights[i] if i < 8 else None, 5 if mode == "max" else 32, c)
        assert [int(h["_source"]["text"][1:]) for h in res[i]] == rows, i
        assert [h["fields"]["_fused"][0] for h in res[i]] == [float(v) for v in fs], i
    assert len(res[12]) == 5 and "fields" not in res[12][0]


def test_native_binds_the_new_symbols():
    from semantic_query_engine_amd import _native
    for name in ("sqe_index_search_fused", "sqe_index_search_fused_device"):
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 13
    lib = _native.load()
    assert lib.sqe_index_search_fused.argtypes is not None and lib.sqe_index_search_fused_device.argtypes is not None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sqe.h")).read()
    assert "SQE_FUSE_MAX = 0, SQE_FUSE_RRF = 1" in text
    from semantic_query_engine_amd.engine import FUSE_MODES
    assert FUSE_MODES == {"max": 0, "rrf": 1}
