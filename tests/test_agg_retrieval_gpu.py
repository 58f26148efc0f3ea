"""Field aggregations end to end on the GPU: OpenSearchIndexer.aggregate and the shim's "size": 0 request over a few hundred
documents, with a field filter (the device predicate), a text `match` filter (the allow-list route) and none, against counting
the documents in Python; terms keys in their fields' own types; a request without aggs answers as before.  GPU only."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N_DOCS = 64, 300
WORDS = ["aspirin", "fever", "pain", "gene", "cancer", "risk", "trial", "dose"]
SCHEMA = {"year": "long", "user_id": "keyword", "published": "date", "open": "boolean", "impact": "double"}


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def corpus():
    from oracle import wordpiece as WP
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    rng = np.random.default_rng(89)
    docs = []
    for i in range(N_DOCS):
        d = {"doc_id": f"d{i // 3}", "text": " ".join(rng.choice(WORDS, int(rng.integers(2, 6)))), "user_id": f"user{(i * i) % 7}",
             "open": bool(i % 3), "impact": float((i % 11) - 5) / 4, "published": f"20{10 + i % 12}-03-0{1 + i % 5}T00:00:00Z"}
        if i % 9:
            d["year"] = int(2000 + (i * 7) % 24)
        docs.append(d)
    toks = WP.synthetic_vocab([" ".join(WORDS)], size=200)
    x = rng.standard_normal((N_DOCS, DIM)).astype(np.float32)
    return docs, x, WordPieceTokenizer(vocab_text="\n".join(toks) + "\n")


def _count(docs, name, keep):
    out = {}
    for d in docs:
        if keep(d) and d.get(name) is not None:
            out[d[name]] = out.get(d[name], 0) + 1
    return out


def _ranked(counts, first_seen):
    """count descending; ties to the lower value -- for a keyword the value seen first"""
    return sorted(counts.items(), key=lambda kv: (-kv[1], first_seen(kv[0])))


AGGS = {"years": {"terms": {"field": "year", "size": 5}}, "users": {"terms": {"field": "user_id", "size": 10}},
        "open": {"terms": {"field": "open"}}, "impact": {"terms": {"field": "impact", "size": 20}},
        "months": {"terms": {"field": "published", "size": 3}}, "year_stats": {"stats": {"field": "year"}},
        "decades": {"histogram": {"field": "year", "interval": 10}}, "top_impact": {"max": {"field": "impact"}}}


def _check(docs, keep, selected, got):
    from semantic_query_engine_amd.fields import _date_ms
    kept = [d for d in docs if keep(d)]
    assert selected == len(kept)
    users_seen = {}
    for d in docs:
        users_seen.setdefault(d["user_id"], len(users_seen))
    years = _ranked(_count(docs, "year", keep), lambda v: v)
    assert [(b["key"], b["doc_count"]) for b in got["years"]["buckets"]] == years[:5]
    assert got["years"]["sum_other_doc_count"] == sum(c for _, c in years[5:])
    assert [(b["key"], b["doc_count"]) for b in got["users"]["buckets"]] == _ranked(_count(docs, "user_id", keep), users_seen.get)
    assert all(isinstance(b["key"], str) for b in got["users"]["buckets"])
    assert [(b["key"], b["key_as_string"], b["doc_count"]) for b in got["open"]["buckets"]] == \
        [(int(v), "true" if v else "false", c) for v, c in _ranked(_count(docs, "open", keep), lambda v: v)]
    assert [(b["key"], b["doc_count"]) for b in got["impact"]["buckets"]] == _ranked(_count(docs, "impact", keep), lambda v: v)
    assert all(isinstance(b["key"], float) for b in got["impact"]["buckets"])
    months = _ranked({_date_ms(k): c for k, c in _count(docs, "published", keep).items()}, lambda v: v)[:3]
    assert [(b["key"], b["doc_count"]) for b in got["months"]["buckets"]] == months
    assert all(b["key_as_string"].endswith("T00:00:00.000Z") for b in got["months"]["buckets"])
    ys = [d["year"] for d in kept if d.get("year") is not None]
    assert got["year_stats"] == ({"count": len(ys), "min": min(ys), "max": max(ys), "avg": sum(ys) / len(ys), "sum": sum(ys)} if ys else
                                 {"count": 0, "min": None, "max": None, "avg": None, "sum": 0})
    decades = {}
    for y in ys:
        decades[y // 10 * 10] = decades.get(y // 10 * 10, 0) + 1
    want = [(k, decades.get(k, 0)) for k in range(min(decades), max(decades) + 1, 10)] if decades else []
    assert [(b["key"], b["doc_count"]) for b in got["decades"]["buckets"]] == want
    assert got["top_impact"] == {"value": max(d["impact"] for d in kept) if kept else None}


def _cases(an):
    has = lambda d, w: set(an.query(w).tolist()) <= set(an.analyze([d["text"]])[0].tolist())      # noqa: E731
    return [
        (None, lambda d: True),
        ({"bool": {"filter": [{"range": {"year": {"gte": 2008}}}, {"term": {"open": True}}]}},
         lambda d: d.get("year") is not None and d["year"] >= 2008 and d["open"]),                 # the device predicate
        ({"match": {"text": {"query": "gene", "operator": "and"}}}, lambda d: has(d, "gene")),     # the allow-list
        ({"bool": {"filter": [{"match": {"text": {"query": "pain", "operator": "and"}}}, {"range": {"year": {"lt": 2015}}}]}},
         lambda d: has(d, "pain") and d.get("year") is not None and d["year"] < 2015),
        ({"term": {"user_id": "nobody"}}, lambda d: False),
    ]


def test_indexer_aggregate_equals_counting_the_documents(ctx, corpus):
    from semantic_query_engine_amd import retrieval as RT
    docs, x, tok = corpus
    client = RT.GpuSearchClient(ctx, dim=DIM)
    client.configure_fields("agg", SCHEMA)
    ix = RT.OpenSearchIndexer(client, "agg")
    ix.add_embeddings(x[:200], docs[:200])
    RT.configure_analyzer(tok, max_len=64)
    try:
        for n_docs in (200, N_DOCS):                              # the second round after an add: the new rows' values follow
            for flt, keep in _cases(RT._analyzer):
                r = ix.aggregate(AGGS, filter=flt)
                print(flt, r["selected"])
                _check(docs[:n_docs], keep, r["selected"], r["aggregations"])
            if n_docs == 200:
                ix.add_embeddings(x[200:], docs[200:])
        routes = client.index("agg").vectors.aggregate_last()
        assert len(routes) == 8 and all(r["route"] == 0 for r in routes)          # the last filter selected nothing
        with pytest.raises(ValueError):
            ix.aggregate({"s": {"sum": {"field": "impact"}}})
    finally:
        RT.configure_analyzer(None)


def test_shim_size_zero_aggs_equal_counting_the_documents(ctx, corpus):
    from fastapi.testclient import TestClient
    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim
    docs, x, tok = corpus
    RT.configure_analyzer(tok, max_len=64)
    try:
        client = RT.GpuSearchClient(ctx, dim=DIM)
        with TestClient(shim.create_app(client, None, DIM)) as c:
            props = {name: {"type": t} for name, t in SCHEMA.items()}
            props["embedding"] = {"type": "knn_vector", "dimension": DIM}
            assert c.put("/agg", json={"mappings": {"properties": props}}).status_code == 200
            lines = []
            for i, d in enumerate(docs):
                lines += [{"index": {"_index": "agg", "_id": f"id{i}"}}, {**d, "embedding": x[i].tolist()}]
            r = c.post("/_bulk", content="\n".join(json.dumps(line) for line in lines) + "\n", headers={"content-type": "application/x-ndjson"})
            assert r.status_code == 200 and not r.json()["errors"]
            knn = {"size": 5, "query": {"knn": {"embedding": {"vector": x[7].tolist(), "k": 5}}}}
            before = c.post("/agg/_search", json=knn).json()
            for flt, keep in _cases(RT._analyzer):
                body = {"size": 0, "aggs": AGGS}
                if flt is not None:
                    body["query"] = flt
                r = c.post("/agg/_search", json=body)
                assert r.status_code == 200, r.text
                out = r.json()
                assert out["hits"]["hits"] == [] and out["hits"]["max_score"] is None
                _check(docs, keep, out["hits"]["total"]["value"], out["aggregations"])
            assert c.post("/agg/_search", json={"size": 0, "aggs": AGGS, "query": {"match_all": {}}}).json()["hits"]["total"]["value"] == N_DOCS
            assert c.post("/agg/_search", json={**knn, "aggs": AGGS}).status_code == 400
            assert c.post("/agg/_search", json={"size": 2, "aggs": AGGS}).status_code == 400
            after = c.post("/agg/_search", json=knn).json()               # a request without aggs answers exactly as before
            before.pop("took"), after.pop("took")
            assert after == before and [h["_id"] for h in after["hits"]["hits"]][0] == "id7"
    finally:
        RT.configure_analyzer(None)
