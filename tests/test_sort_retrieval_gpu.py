"""Sorted search through the Python layers on the GPU: OpenSearchIndexer.search_sorted on a small named index with declared long /
date / double fields against sorting the docstore in Python, `from_` and `search_after` round trips through the returned
sort_values, and the shim's `_search` with `sort`: hits, sort arrays, hits.total, the 400s, and a knn request with a `sort` key
that answers exactly as without it.  GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N_DOCS = 64, 400
SCHEMA = {"year": "long", "published": "date", "impact": "double", "open": "boolean", "user_id": "keyword"}
DAY = 86_400_000


def _docs():
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N_DOCS, DIM)).astype(np.float32)
    docs = []
    for i in range(N_DOCS):
        d = {"doc_id": f"PMC{i // 4}.txt", "text": f"chunk {i}", "user_id": f"u{i % 5}", "open": bool(i % 3 == 0)}
        if i % 7:
            d["year"] = int(rng.integers(2000, 2012))
        if i % 5:
            d["published"] = int(1_400_000_000_000 + int(rng.integers(0, 40)) * DAY)
        if i % 4:
            d["impact"] = float(rng.integers(-6, 7)) / 4.0          # many ties, both signs and zero
        docs.append(d)
    return x, docs


@pytest.fixture(scope="module")
def setup():
    from semantic_query_engine_amd import Context
    from semantic_query_engine_amd import retrieval as RT
    client = RT.GpuSearchClient(ctx=Context(0), dim=DIM)
    client.configure_fields("papers", SCHEMA)
    x, docs = _docs()
    ix = RT.OpenSearchIndexer(client, "papers")
    ix.add_embeddings(x, docs)
    return client, ix, x, docs


def _want(docs, sort, keep=lambda d: True):
    """the docstore sorted in Python: sort = [(name, desc, missing_first)] -> [(row, sort_values)] in order"""
    def key(item):
        i, d = item
        out = []
        for name, desc, first in sort:
            v = d.get(name)
            out.append(((-1 if first else 1), 0) if v is None else (0, -v if desc else v))
        return tuple(out) + (i,)
    rows = sorted(((i, d) for i, d in enumerate(docs) if keep(d)), key=key)
    return [(i, [d.get(name) for name, _, _ in sort] + [i]) for i, d in rows]


CASES = [
    ("year", [("year", False, False)]),
    ({"year": "desc"}, [("year", True, False)]),
    ({"published": {"order": "asc", "missing": "_first"}}, [("published", False, True)]),
    ([{"impact": "desc"}, "year"], [("impact", True, False), ("year", False, False)]),
    ([{"open": {"order": "desc", "missing": "_first"}}, {"impact": "asc"}, {"published": "desc"}, {"year": {"missing": "_first"}}],
     [("open", True, True), ("impact", False, False), ("published", True, False), ("year", False, True)]),
]


@pytest.mark.parametrize("body, sort", CASES)
def test_search_sorted_equals_sorting_the_docstore(setup, body, sort):
    _, ix, _, docs = setup
    want = _want(docs, sort)
    total, hits = ix.search_sorted(body, 256)
    assert total == N_DOCS and len(hits) == 256
    assert [sv for _, sv in hits] == [sv for _, sv in want[:256]]
    assert [(src["doc_id"], src["text"]) for src, _ in hits] == [(docs[i]["doc_id"], docs[i]["text"]) for i, _ in want[:256]]
    for (src, sv), (i, _) in zip(hits[:20], want):
        assert type(sv[-1]) is int and all(v is None or type(v) is type(docs[i][name]) for v, (name, _, _) in zip(sv, sort))
    # from_ drops rows on the host; search_after takes a hit's sort_values back, through a JSON round trip too
    import json
    total, page = ix.search_sorted(body, 10, from_=35)
    assert total == N_DOCS and [sv for _, sv in page] == [sv for _, sv in want[35:45]]
    seen, after = [], None
    while True:
        total, page = ix.search_sorted(body, 64, search_after=after)
        assert total == N_DOCS
        if not page:
            break
        seen += [sv[-1] for _, sv in page]
        after = json.loads(json.dumps(page[-1][1]))
    assert seen == [i for i, _ in want]
    # filters: a conjunction of field leaves (the device predicate) and one that needs an allow-list
    flt = {"bool": {"filter": [{"range": {"year": {"gte": 2005}}}, {"term": {"user_id": "u2"}}]}}
    keep = lambda d: d.get("year") is not None and d["year"] >= 2005 and d["user_id"] == "u2"      # noqa: E731
    total, hits = ix.search_sorted(body, 50, filter=flt)
    assert total == sum(keep(d) for d in docs) and [sv for _, sv in hits] == [sv for _, sv in _want(docs, sort, keep)[:50]]
    flt = {"bool": {"should": [{"term": {"doc_id": "PMC3.txt"}}, {"range": {"year": {"lt": 2002}}}]}}
    keep = lambda d: d["doc_id"] == "PMC3.txt" or (d.get("year") is not None and d["year"] < 2002)      # noqa: E731
    total, hits = ix.search_sorted(body, 50, filter=flt, from_=3)
    assert total == sum(keep(d) for d in docs) and [sv for _, sv in hits] == [sv for _, sv in _want(docs, sort, keep)[3:53]]


def test_search_sorted_refusals(setup):
    _, ix, _, _ = setup
    for kw in (dict(sort={"user_id": "asc"}, k=5), dict(sort="_score", k=5), dict(sort="nope", k=5), dict(sort="year", k=0),
               dict(sort="year", k=200, from_=57), dict(sort="year", k=5, from_=-1), dict(sort="year", k=5, search_after=[2001]),
               dict(sort="year", k=5, filter={"range": {"nope": {"gte": 1}}}), dict(sort={"year": {"missing": 3}}, k=5)):
        with pytest.raises(ValueError):
            ix.search_sorted(**kw)


def test_shim_search_with_sort(setup):
    from fastapi.testclient import TestClient
    from semantic_query_engine_amd import shim
    client, _, x, docs = setup
    rev = {row: os_id for os_id, row in client.index("papers").row_of_id.items()}
    with TestClient(shim.create_app(client, None, DIM)) as c:
        sort = [("impact", True, False), ("year", False, False)]
        body = {"sort": [{"impact": "desc"}, "year"]}
        want = _want(docs, sort)
        r = c.post("/papers/_search", json=body)
        assert r.status_code == 200
        out = r.json()["hits"]
        assert out["total"] == {"value": N_DOCS, "relation": "eq"} and out["max_score"] is None and len(out["hits"]) == 10
        for hit, (i, sv) in zip(out["hits"], want):
            assert hit["_score"] is None and hit["sort"] == sv and hit["_id"] == rev[i] and hit["_index"] == "papers"
            assert hit["_source"]["text"] == docs[i]["text"] and hit["_source"]["doc_id"] == docs[i]["doc_id"]
        # size, from and search_after; match_all; every query kind of the route
        r = c.post("/papers/_search", json={**body, "size": 7, "from": 5, "query": {"match_all": {}}})
        assert [h["sort"] for h in r.json()["hits"]["hits"]] == [sv for _, sv in want[5:12]]
        r = c.post("/papers/_search", json={**body, "size": 256, "search_after": out["hits"][-1]["sort"]})
        assert [h["sort"] for h in r.json()["hits"]["hits"]] == [sv for _, sv in want[10:266]] and r.json()["hits"]["total"]["value"] == N_DOCS
        queries = [
            ({"term": {"user_id": "u1"}}, lambda d: d["user_id"] == "u1"),
            ({"terms": {"year": [2001, 2003]}}, lambda d: d.get("year") in (2001, 2003)),
            ({"range": {"published": {"gte": 1_400_000_000_000 + 20 * DAY}}}, lambda d: d.get("published", 0) >= 1_400_000_000_000 + 20 * DAY),
            ({"exists": {"field": "impact"}}, lambda d: "impact" in d),
            ({"ids": {"values": [rev[3], rev[9], rev[200]]}}, None),
            ({"bool": {"must_not": [{"term": {"doc_id": "PMC0.txt"}}], "filter": [{"term": {"open": True}}]}},
             lambda d: d["doc_id"] != "PMC0.txt" and d["open"]),
        ]
        for query, keep in queries:
            rows = _want(docs, sort, keep) if keep else [w for w in want if w[0] in (3, 9, 200)]
            r = c.post("/papers/_search", json={**body, "size": 256, "query": query})
            assert r.status_code == 200, (query, r.json())
            assert r.json()["hits"]["total"]["value"] == len(rows) and [h["sort"] for h in r.json()["hits"]["hits"]] == [sv for _, sv in rows[:256]]
        # what sort_spec and the window refuse answers 400
        for bad, kind in (({"sort": {"user_id": "asc"}}, "parsing_exception"), ({"sort": "_score"}, "parsing_exception"),
                          ({"sort": ["_doc"]}, "parsing_exception"), ({"sort": {"year": {"mode": "min"}}}, "parsing_exception"),
                          ({"sort": {"year": {"unmapped_type": "long"}}}, "parsing_exception"), ({"sort": {"year": {"missing": 0}}}, "parsing_exception"),
                          ({"sort": "nope"}, "parsing_exception"), ({"sort": ["year"] * 2}, "parsing_exception"),
                          ({"sort": "year", "search_after": [1]}, "parsing_exception"),
                          ({"sort": "year", "query": {"range": {"nope": {"gte": 1}}}}, "parsing_exception"),
                          ({"sort": "year", "size": 0}, "illegal_argument_exception"), ({"sort": "year", "size": 257}, "illegal_argument_exception"),
                          ({"sort": "year", "size": 200, "from": 57}, "illegal_argument_exception")):
            r = c.post("/papers/_search", json=bad)
            assert r.status_code == 400 and r.json()["error"]["type"] == kind, (bad, r.json())
        # a knn request keeps its route: with a sort key it answers exactly as without it
        knn = {"size": 5, "query": {"knn": {"embedding": {"vector": x[17].tolist(), "k": 5}}}}
        plain, sorted_ = c.post("/papers/_search", json=knn), c.post("/papers/_search", json={**knn, "sort": [{"year": "desc"}]})
        assert plain.status_code == sorted_.status_code == 200 and plain.json()["hits"] == sorted_.json()["hits"]
        assert "sort" not in plain.json()["hits"]["hits"][0]
        flt = {"size": 5, "query": {"knn": {"embedding": {"vector": x[17].tolist(), "k": 5, "filter": {"term": {"user_id": "u2"}}}}}}
        assert c.post("/papers/_search", json=flt).json()["hits"] == c.post("/papers/_search", json={**flt, "sort": "year"}).json()["hits"]
