"""Field aggregations without a GPU: the model of tests/agg_reference.py checked by hand on a dozen rows, the layout pack_aggs
produces against the C structs, pack_aggs' refusals, f64_from_image as the inverse of f64_image, FieldSchema.aggregation for every
served form and every refusal, and OpenSearchIndexer.aggregate and the shim's "size": 0 request over a stand-in index backed by
the model."""
import ctypes as C

import numpy as np
import pytest

from tests import agg_reference as A
from tests.fields_reference import I64_MAX, NONE, FieldModel


def _model():
    m = FieldModel(12)
    ids = np.arange(12)
    #              0   1   2   3   4   5   6     7   8   9   10  11
    m.set_field(0, ids, [5, 3, 5, 3, 9, 9, NONE, 7, 1, 1, 2, 2])                 # five values tie at count 2
    m.set_field(1, ids, [-7, -6, -2, -1, 0, 2, 3, 4, 8, NONE, 13, 14])
    m.set_field(2, ids, [I64_MAX, I64_MAX, I64_MAX, NONE + 1, 1 << 62, -(1 << 62), NONE, NONE, NONE, NONE, NONE, NONE])
    return m


def test_stats_by_hand():
    m = _model()
    r = A.aggregate(m, [], [(0, "stats"), (2, "stats"), (5, "stats")])
    assert r["selected"] == 12
    a, big, unset = r["aggs"]
    assert (a["count"], a["min"], a["max"], a["sum"]) == (11, 1, 9, 47) and a["n_buckets"] == a["other"] == 0 and a["keys"].size == 0
    assert big["sum"] == 3 * I64_MAX + NONE + 1 and big["sum"] > I64_MAX         # 2^64 - 2: the exact sum has left int64
    assert (unset["count"], unset["min"], unset["max"], unset["sum"]) == (0, I64_MAX, NONE, 0)     # a count of zero
    # the two partial sums the library carries compose to the exact sum, negative values included
    s = A.stats_of(np.array([-1, NONE + 1, I64_MAX, -(1 << 32), 1 << 32], np.int64))
    assert s["sum_lo"] == 0xFFFFFFFF + 1 + 0xFFFFFFFF and s["sum_hi"] == -1 - (1 << 31) + ((1 << 31) - 1) - 1 + 1
    assert (s["sum_hi"] << 32) + s["sum_lo"] == s["sum"] == -1
    # under a predicate and an allow-list: rows 0..5 with a value in field 1 below 0
    r = A.aggregate(m, [(1, "range", None, -1)], [(0, "stats")], filter_ids=[0, 1, 2, 3, 4, 5, 99])
    assert r["selected"] == 4 and r["aggs"][0]["sum"] == 16 and r["aggs"][0]["count"] == 4


def test_terms_ties_at_the_size_boundary_by_hand():
    m = _model()
    r = A.aggregate(m, [], [(0, "terms", 3), (0, "terms", 1), (0, "terms", 256)])
    t3, t1, t_all = r["aggs"]
    # 1, 2, 3, 5, 9 hold two rows each and 7 one: the lower values win the tie
    assert t3["keys"].tolist() == [1, 2, 3] and t3["counts"].tolist() == [2, 2, 2] and t3["n_buckets"] == 6 and t3["other"] == 5
    assert t1["keys"].tolist() == [1] and t1["other"] == 9
    assert t_all["keys"].tolist() == [1, 2, 3, 5, 9, 7] and t_all["counts"].tolist() == [2, 2, 2, 2, 2, 1] and t_all["other"] == 0
    assert t3["count"] == 11 and t3["min"] == 1 and t3["max"] == 9 and t3["sum"] == 47      # the stats members are filled too


def test_histogram_negative_keys_and_offset_by_hand():
    m = _model()
    r = A.aggregate(m, [], [(1, "histogram", 5, 3)])
    h = r["aggs"][0]
    # buckets floor((v - 3) / 5): -7 -6 -> -2 (key -7); -2 -1 0 2 -> -1 (key -2); 3 4 -> 0 (key 3); 8 -> 1 (key 8); 13 14 -> 2 (key 13)
    assert h["keys"].tolist() == [-7, -2, 3, 8, 13] and h["counts"].tolist() == [2, 4, 2, 1, 2] and h["n_buckets"] == 5 and h["other"] == 0
    r = A.aggregate(m, [(1, "in", [-7, 14])], [(1, "histogram", 5, 3)])
    assert r["aggs"][0]["keys"].tolist() == [-7, -2, 3, 8, 13] and r["aggs"][0]["counts"].tolist() == [1, 0, 0, 0, 1]      # the empty ones appear
    with pytest.raises(A.TooManyBuckets) as e:
        A.aggregate(m, [], [(1, "histogram", 5, 3), (0, "stats")], bucket_cap=4)
    assert e.value.n_buckets == 5 and e.value.result["aggs"][1]["sum"] == 47 and e.value.result["aggs"][0]["n_buckets"] == 5
    with pytest.raises(A.TooManyBuckets) as e:
        A.aggregate(m, [], [(2, "histogram", 1, 0)])
    assert e.value.n_buckets == (1 << 64) - 1
    h = A.aggregate(m, [], [(2, "histogram", 1 << 62, (1 << 62) - 1)])["aggs"][0]
    assert h["n_buckets"] == 5 and h["counts"].tolist() == [1, 1, 0, 1, 3] and h["keys"][0] == I64_MAX      # -2^63 - 1, wrapped


def test_pack_aggs_layout_matches_the_structs():
    from semantic_query_engine_amd import _native as N
    from semantic_query_engine_amd.engine import AGG_DTYPE, AGG_RESULT_DTYPE, pack_aggs
    assert AGG_DTYPE.itemsize == C.sizeof(N.FieldAgg) == 32 and AGG_RESULT_DTYPE.itemsize == C.sizeof(N.FieldAggResult) == 56
    assert C.sizeof(N.AggRoute) == 32 and C.sizeof(N.AggLast) == 8 + 8 * 32
    for name, _ in N.FieldAgg._fields_:
        assert AGG_DTYPE.fields[name][1] == getattr(N.FieldAgg, name).offset
    for name, _ in N.FieldAggResult._fields_:
        assert AGG_RESULT_DTYPE.fields[name][1] == getattr(N.FieldAggResult, name).offset
    p = pack_aggs([(3, "stats"), (0, "terms", 25), {"field": 7, "kind": "histogram", "interval": 1000, "offset": 7}, (1, "histogram", 5),
                   (2, "terms")])
    assert p.tolist() == [(0, 3, 0, 0, 0, 0), (1, 0, 25, 0, 0, 0), (2, 7, 0, 0, 1000, 7), (2, 1, 0, 0, 5, 0), (1, 2, 10, 0, 0, 0)]
    raw = (N.FieldAgg * 5).from_buffer_copy(p.tobytes())
    assert (raw[2].kind, raw[2].field, raw[2].interval, raw[2].offset, raw[1].size) == (2, 7, 1000, 7, 25)


@pytest.mark.parametrize("aggs", [
    [], [(0, "stats")] * 9, [(8, "stats")], [(-1, "terms", 3)], [(0, "cardinality")], [(0, "terms", 0)], [(0, "terms", 257)],
    [(0, "histogram", 0)], [(0, "histogram", 5, 5)], [(0, "histogram", 5, -1)],
])
def test_pack_aggs_refusals(aggs):
    from semantic_query_engine_amd.engine import pack_aggs
    with pytest.raises(ValueError):
        pack_aggs(aggs)


def test_f64_from_image_inverts_f64_image():
    from semantic_query_engine_amd.engine import f64_from_image, f64_image
    tiny = np.nextafter(0.0, 1.0)
    edge = np.array([0.0, tiny, -tiny, 1.0, -1.0, 1.5, -2.75, np.finfo(np.float64).max, np.finfo(np.float64).min,
                     np.finfo(np.float64).tiny, -np.finfo(np.float64).tiny, np.inf, -np.inf, 1e300, -1e-300, 2015.0, -273.15])
    back = f64_from_image(f64_image(edge))
    assert back.dtype == np.float64 and np.array_equal(back.view(np.int64), edge.view(np.int64))      # bit for bit
    for x in edge.tolist():
        assert f64_from_image(f64_image(x)) == x and isinstance(f64_from_image(f64_image(x)), float)
    z = f64_from_image(f64_image(-0.0))
    assert z == 0.0 and np.signbit(z) == False                 # noqa: E712  both zeros are one value, +0.0
    assert np.isnan(f64_from_image(f64_image(np.nan))) and np.isnan(f64_from_image(f64_image(-np.nan)))
    rng = np.random.default_rng(3)
    bits = rng.integers(-(1 << 63), (1 << 63) - 1, 10_000, dtype=np.int64)
    vals = bits.view(np.float64)
    vals = vals[np.isfinite(vals) & (vals != 0)]
    assert np.array_equal(f64_from_image(f64_image(vals)).view(np.int64), vals.view(np.int64))
    order = np.sort(vals)
    assert np.all(np.diff(f64_image(order)) > 0)               # and the image keeps the order it inverts


# ---------------------------------------------------------------- the schema's translation
def _schema():
    from semantic_query_engine_amd.fields import FieldSchema
    s = FieldSchema()
    s.declare({"year": "long", "user_id": "keyword", "published": "date", "impact": "double", "open": "boolean", "pages": "integer"})
    for u in ("zoe", "adam"):
        s.device_value("user_id", u, learn=True)               # codes in the order seen: zoe 0, adam 1
    return s


def _r(**kw):
    base = {"count": 0, "min": I64_MAX, "max": NONE, "sum": 0, "n_buckets": 0, "other": 0, "keys": np.empty(0, np.int64),
            "counts": np.empty(0, np.int64)}
    base.update({k: (np.asarray(v, np.int64) if k in ("keys", "counts") else v) for k, v in kw.items()})
    return base


def test_schema_aggregation_every_served_form():
    from semantic_query_engine_amd.engine import f64_image
    s = _schema()
    agg, shape = s.aggregation({"terms": {"field": "year", "size": 3}})
    assert agg == (0, "terms", 3)
    assert shape(_r(count=9, other=2, keys=[2015, 2001], counts=[4, 3])) == {
        "doc_count_error_upper_bound": 0, "sum_other_doc_count": 2, "buckets": [{"key": 2015, "doc_count": 4}, {"key": 2001, "doc_count": 3}]}
    assert s.aggregation({"terms": {"field": "pages"}})[0] == (5, "terms", 10)                     # the default size
    agg, shape = s.aggregation({"terms": {"field": "user_id", "size": 5}})
    assert agg == (1, "terms", 5) and [b["key"] for b in shape(_r(keys=[1, 0], counts=[2, 2]))["buckets"]] == ["adam", "zoe"]
    _, shape = s.aggregation({"terms": {"field": "open"}})
    assert shape(_r(keys=[1, 0], counts=[5, 1]))["buckets"] == [{"key": 1, "key_as_string": "true", "doc_count": 5},
                                                                {"key": 0, "key_as_string": "false", "doc_count": 1}]
    _, shape = s.aggregation({"terms": {"field": "impact"}})
    assert [b["key"] for b in shape(_r(keys=[f64_image(-2.5), f64_image(0.1)], counts=[1, 1]))["buckets"]] == [-2.5, 0.1]
    _, shape = s.aggregation({"terms": {"field": "published"}})
    assert shape(_r(keys=[86_400_000], counts=[1]))["buckets"] == [{"key": 86_400_000, "key_as_string": "1970-01-02T00:00:00.000Z", "doc_count": 1}]
    agg, shape = s.aggregation({"histogram": {"field": "year", "interval": 5, "offset": 2}})
    assert agg == (0, "histogram", 5, 2) and shape(_r(keys=[1997, 2002], counts=[0, 7])) == {
        "buckets": [{"key": 1997, "doc_count": 0}, {"key": 2002, "doc_count": 7}]}
    assert s.aggregation({"histogram": {"field": "published", "interval": 1000.0}})[0] == (2, "histogram", 1000, 0)
    for text, ms in (("250ms", 250), ("30s", 30_000), ("5m", 300_000), ("2h", 7_200_000), ("1d", 86_400_000)):
        agg, shape = s.aggregation({"date_histogram": {"field": "published", "fixed_interval": text}})
        assert agg == (2, "histogram", ms, 0)
    assert shape(_r(keys=[-86_400_000], counts=[2]))["buckets"] == [{"key": -86_400_000, "key_as_string": "1969-12-31T00:00:00.000Z", "doc_count": 2}]
    for kind in ("min", "max", "value_count", "stats", "sum", "avg"):
        for name in ("year", "pages", "open", "published"):
            assert s.aggregation({kind: {"field": name}})[0] == (s.slot[name], "stats")
    r = _r(count=4, min=-3, max=9, sum=10)
    got = {kind: s.aggregation({kind: {"field": "year"}})[1](r) for kind in ("min", "max", "value_count", "stats", "sum", "avg")}
    assert got == {"min": {"value": -3}, "max": {"value": 9}, "value_count": {"value": 4}, "sum": {"value": 10}, "avg": {"value": 2.5},
                   "stats": {"count": 4, "min": -3, "max": 9, "avg": 2.5, "sum": 10}}
    none = {kind: s.aggregation({kind: {"field": "year"}})[1](_r()) for kind in ("min", "max", "value_count", "stats", "sum", "avg")}
    assert none == {"min": {"value": None}, "max": {"value": None}, "value_count": {"value": 0}, "sum": {"value": 0}, "avg": {"value": None},
                    "stats": {"count": 0, "min": None, "max": None, "avg": None, "sum": 0}}
    assert s.aggregation({"max": {"field": "impact"}})[1](_r(count=1, max=f64_image(7.25))) == {"value": 7.25}
    assert s.aggregation({"min": {"field": "published"}})[1](_r(count=1, min=0)) == {"value": 0, "value_as_string": "1970-01-01T00:00:00.000Z"}
    big = s.aggregation({"sum": {"field": "year"}})[1](_r(count=3, sum=3 * I64_MAX))
    assert big == {"value": 3 * I64_MAX}                                           # a Python int: the sum does not wrap


@pytest.mark.parametrize("spec, says", [
    ({"sum": {"field": "impact"}}, "accumulation order"), ({"avg": {"field": "impact"}}, "accumulation order"),
    ({"stats": {"field": "impact"}}, "accumulation order"), ({"histogram": {"field": "impact", "interval": 1}}, "long / integer / date"),
    ({"histogram": {"field": "user_id", "interval": 1}}, "long / integer / date"), ({"date_histogram": {"field": "year", "fixed_interval": "1d"}}, "date fields"),
    ({"min": {"field": "user_id"}}, "keyword"), ({"value_count": {"field": "user_id"}}, "keyword"), ({"stats": {"field": "user_id"}}, "keyword"),
    ({"terms": {"field": "year"}, "aggs": {"x": {"max": {"field": "pages"}}}}, "sub-aggregations"),
    ({"terms": {"field": "year"}, "aggregations": {}}, "sub-aggregations"),
    ({"terms": {"field": "year", "order": {"_key": "asc"}}}, "order"), ({"terms": {"field": "year", "min_doc_count": 2}}, "min_doc_count"),
    ({"terms": {"field": "year", "missing": 0}}, "missing"), ({"max": {"field": "year", "missing": 0}}, "missing"),
    ({"terms": {"field": "year", "size": 0}}, "size"), ({"terms": {"field": "year", "size": 257}}, "size"), ({"terms": {"field": "year", "size": "3"}}, "size"),
    ({"histogram": {"field": "year", "interval": 0}}, "interval"), ({"histogram": {"field": "year", "interval": 2.5}}, "interval"),
    ({"histogram": {"field": "year"}}, "interval"), ({"histogram": {"field": "year", "interval": 5, "offset": 5}}, "offset"),
    ({"histogram": {"field": "year", "interval": 5, "offset": -1}}, "offset"),
    ({"date_histogram": {"field": "published", "calendar_interval": "month"}}, "calendar_interval"),
    ({"date_histogram": {"field": "published", "fixed_interval": "1w"}}, "fixed_interval"),
    ({"date_histogram": {"field": "published", "fixed_interval": "0s"}}, "fixed_interval"),
    ({"date_histogram": {"field": "published"}}, "fixed_interval"),
    ({"cardinality": {"field": "year"}}, "cardinality"), ({"percentiles": {"field": "year"}}, "percentiles"),
    ({"terms": {"field": "nope"}}, "no configured field"), ({"terms": {"size": 3}}, "needs a field"), ({"terms": "year"}, "needs a field"),
    ({"min": {"field": "year"}, "max": {"field": "year"}}, "one kind"), ("terms", "object"), ({}, "one kind"),
])
def test_schema_aggregation_refusals_say_what_is_served(spec, says):
    with pytest.raises(ValueError) as e:
        _schema().aggregation(spec)
    assert says in str(e.value), str(e.value)
    assert "served" in str(e.value) or "configured field" in str(e.value)


# ---------------------------------------------------------------- the indexer and the shim over a stand-in index
def _agg_client(monkeypatch):
    from semantic_query_engine_amd import retrieval as RT
    from tests.test_fields_cpu import DIM, SCHEMA, FieldVectors, _docs

    class AggVectors(FieldVectors):
        def aggregate_fields(self, pred, aggs, filter_ids=None, bucket_cap=None):
            self.calls.append(("aggregate_fields", pred, None if filter_ids is None else np.asarray(filter_ids).tolist()))
            try:
                return A.aggregate(self.model, pred, aggs, filter_ids=filter_ids, bucket_cap=bucket_cap)
            except A.TooManyBuckets as e:
                from semantic_query_engine_amd._native import SqeError
                raise SqeError(-1, f"too_many_buckets: {e.n_buckets}") from None

    monkeypatch.setattr(RT, "VectorIndex", AggVectors)
    client = RT.GpuSearchClient(ctx=object(), dim=DIM)
    client.configure_fields("idx", SCHEMA)
    x, docs = _docs()
    RT.OpenSearchIndexer(client, "idx").add_embeddings(x, docs)
    return client, x, docs


def _count(docs, name, keep=lambda d: True):
    out = {}
    for d in docs:
        if keep(d) and d.get(name) is not None:
            out[d[name]] = out.get(d[name], 0) + 1
    return out


def test_indexer_aggregate_routes_the_filter(monkeypatch):
    from semantic_query_engine_amd import retrieval as RT
    client, x, docs = _agg_client(monkeypatch)
    ix = RT.OpenSearchIndexer(client, "idx")
    calls = client.index("idx").vectors.calls
    aggs = {"users": {"terms": {"field": "user_id", "size": 10}}, "years": {"stats": {"field": "year"}},
            "open": {"terms": {"field": "open"}}, "n_impact": {"value_count": {"field": "impact"}}}
    r = ix.aggregate(aggs)
    assert r["selected"] == len(docs) and calls[-1] == ("aggregate_fields", [], None)
    assert {b["key"]: b["doc_count"] for b in r["aggregations"]["users"]["buckets"]} == _count(docs, "user_id")
    years = [d["year"] for d in docs if d.get("year") is not None]
    assert r["aggregations"]["years"] == {"count": len(years), "min": min(years), "max": max(years), "avg": sum(years) / len(years), "sum": sum(years)}
    assert {b["key_as_string"]: b["doc_count"] for b in r["aggregations"]["open"]["buckets"]} == {"true": 20, "false": 20}
    assert r["aggregations"]["n_impact"] == {"value": sum("impact" in d for d in docs)}
    # a conjunction of field leaves is the device predicate; anything else an allow-list beside the empty predicate
    r = ix.aggregate(aggs, filter={"range": {"year": {"gte": 2010}}})
    assert calls[-1][1] and calls[-1][2] is None
    keep = lambda d: d.get("year") is not None and d["year"] >= 2010      # noqa: E731
    assert r["selected"] == sum(keep(d) for d in docs)
    assert {b["key"]: b["doc_count"] for b in r["aggregations"]["users"]["buckets"]} == _count(docs, "user_id", keep)
    flt = {"bool": {"should": [{"term": {"doc_id": "PMC1.txt"}}, {"range": {"year": {"lt": 2003}}}]}}
    r = ix.aggregate(aggs, filter=flt)
    keep = lambda d: d["doc_id"] == "PMC1.txt" or (d.get("year") is not None and d["year"] < 2003)      # noqa: E731
    assert calls[-1][1] == [] and calls[-1][2] == [i for i, d in enumerate(docs) if keep(d)]
    assert r["selected"] == sum(keep(d) for d in docs)
    assert {b["key"]: b["doc_count"] for b in r["aggregations"]["users"]["buckets"]} == _count(docs, "user_id", keep)
    r = ix.aggregate({"y": {"terms": {"field": "year"}}}, filter={"bool": {"must_not": [{"term": {"doc_id": "PMC0.txt"}}]}})      # the exclusion route elsewhere
    assert r["selected"] == len(docs) - 4 and calls[-1][2] == list(range(4, len(docs)))
    nine = {f"a{j}": {"max": {"field": "pages"}} for j in range(9)}                                # more than one call's eight
    r = ix.aggregate(nine)
    assert len(r["aggregations"]) == 9 and len({one["value"] for one in r["aggregations"].values()}) == 1
    for bad in ({"s": {"sum": {"field": "impact"}}}, {}, {"h": {"histogram": {"field": "published", "interval": 1}}}):
        with pytest.raises(ValueError):
            ix.aggregate(bad)
    with pytest.raises(ValueError):
        RT.OpenSearchIndexer(RT.GpuSearchClient(ctx=object(), dim=8), "plain").aggregate({"y": {"terms": {"field": "year"}}})


def test_shim_size_zero_aggs(monkeypatch):
    from fastapi.testclient import TestClient
    from semantic_query_engine_amd import shim
    from tests.test_fields_cpu import DIM
    client, x, docs = _agg_client(monkeypatch)
    with TestClient(shim.create_app(client, None, DIM)) as c:
        body = {"size": 0, "aggs": {"users": {"terms": {"field": "user_id", "size": 3}}, "latest": {"max": {"field": "published"}}}}
        r = c.post("/idx/_search", json=body)
        assert r.status_code == 200
        out = r.json()
        assert out["hits"] == {"total": {"value": len(docs), "relation": "eq"}, "max_score": None, "hits": []}
        assert [b["doc_count"] for b in out["aggregations"]["users"]["buckets"]] == [8, 8, 8]
        assert [b["key"] for b in out["aggregations"]["users"]["buckets"]] == ["u0", "u1", "u2"]      # ties: the value seen first
        assert out["aggregations"]["users"]["sum_other_doc_count"] == 16
        assert out["aggregations"]["latest"]["value_as_string"] == "2024-07-15T12:00:00.000Z"
        for query in ({"match_all": {}}, None):
            r2 = c.post("/idx/_search", json={"size": 0, "aggregations": body["aggs"], **({"query": query} if query else {})})
            assert r2.status_code == 200 and r2.json()["aggregations"] == out["aggregations"]
        r = c.post("/idx/_search", json={**body, "query": {"bool": {"filter": [{"term": {"user_id": "u1"}}, {"range": {"year": {"gte": 2010}}}]}}})
        want = sum(d["user_id"] == "u1" and d.get("year") is not None and d["year"] >= 2010 for d in docs)
        assert r.status_code == 200 and r.json()["hits"]["total"]["value"] == want
        assert r.json()["aggregations"]["users"]["buckets"] == [{"key": "u1", "doc_count": want}]
        knn = {"knn": {"embedding": {"vector": x[0].tolist(), "k": 3}}}
        for bad in ({**body, "size": 3}, {"aggs": body["aggs"]}, {**body, "query": knn}, {**body, "aggregations": body["aggs"]},
                    {"size": 0, "aggs": {"s": {"sum": {"field": "impact"}}}}, {"size": 0, "aggs": {}},
                    {"size": 0, "aggs": {"y": {"terms": {"field": "year"}, "aggs": {"m": {"max": {"field": "pages"}}}}}},
                    {**body, "query": {"range": {"nope": {"gte": 1}}}}):
            r = c.post("/idx/_search", json=bad)
            assert r.status_code == 400, bad
        assert "size" in c.post("/idx/_search", json={**body, "size": 3}).json()["error"]["reason"]
        assert "knn" in c.post("/idx/_search", json={**body, "query": knn}).json()["error"]["reason"]
        # a request without aggs takes the route it always took
        r = c.post("/idx/_search", json={"size": 3, "query": knn})
        assert r.status_code == 200 and len(r.json()["hits"]["hits"]) == 3 and "aggregations" not in r.json()
