"""Numeric fields on the host side (no GPU): the NumPy model the GPU tests compare with, ``f64_image``, ``pack_predicates``,
the schema and the translation of ``range`` / ``term`` / ``terms`` / ``exists`` (``filter_rows``, ``OpenSearchIndexer.search``,
``search_batch``, the shim), the keyword dictionary, the refusals, save / load, and the host-only argument checks of the C ABI
(csrc/fieldpred.cpp) under AddressSanitizer and UBSan.  The device index is a stand-in backed by the model."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import retrieval as R
from semantic_query_engine_amd import fields as F
from semantic_query_engine_amd import retrieval as RT
from semantic_query_engine_amd import shim
from semantic_query_engine_amd.engine import FIELD_DTYPE, FIELD_NONE, FOP_IN, FOP_NOT, FOP_RANGE, f64_image, pack_predicates
from tests.fields_reference import NONE, FieldModel, clause_holds

DIM = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_query_engine_amd", "csrc")
I64_MAX = (1 << 63) - 1


# ---------------------------------------------------------------- the model, by hand
def test_model_on_hand_made_cases():
    assert NONE == FIELD_NONE == -(1 << 63)
    col = np.array([5, NONE, 7, -3, 7], np.int64)
    assert clause_holds(col, "range", (5, 7)).tolist() == [True, False, True, False, True]
    assert clause_holds(col, "range", (None, None)).tolist() == [True, False, True, True, True]            # exists
    assert clause_holds(col, "range", (8, 7)).tolist() == [False] * 5
    assert clause_holds(col, "range", (5, 7), not_=True).tolist() == [False, True, False, True, False]      # the row without a value passes
    assert clause_holds(col, "in", ([7, -3],)).tolist() == [False, False, True, True, True]
    assert clause_holds(col, "in", ([NONE],)).tolist() == [False] * 5
    assert clause_holds(col, "in", ([7],), not_=True).tolist() == [True, True, False, True, False]
    m = FieldModel(5)
    m.set_field(0, [0, 1, 2, 3, 4], [10, 20, 30, 40, 50])
    m.set_field(1, [1, 3, 1], [7, 8, 9])                       # a repeated id: the last value
    assert m.get_field(1, [0, 1, 3]).tolist() == [NONE, 9, 8]
    assert m.select([]).tolist() == [0, 1, 2, 3, 4]            # the empty predicate: every live row
    assert m.select([(0, "range", 20, 40), (1, "range", None, None)]).tolist() == [1, 3]
    assert m.select([(0, "range", 20, 40), (1, "in", [9], {"not_": True})]).tolist() == [2, 3]
    assert m.select([(5, "range", None, None)]).tolist() == [] and m.select([(5, "in", [1], {"not_": True})]).size == 5
    m.delete([1])
    m.add(2)                                                   # ids 5, 6 start without values
    assert m.ids.tolist() == [0, 2, 3, 4, 5, 6] and m.get_field(0, [4, 5]).tolist() == [50, NONE]
    counts, ids = m.match([[(0, "range", 30, None)], [], [(0, "range", 99, None)]], 2)
    assert counts.tolist() == [3, 6, 0] and ids.tolist() == [[2, 3], [0, 2], [-1, -1]]
    with pytest.raises(KeyError):
        m.set_field(0, [1], [5])                               # a dead id


def test_f64_image_preserves_order():
    tiny = 5e-324
    xs = [-np.inf, -1.7976931348623157e308, -1.5, -2.2250738585072014e-308, -2 * tiny, -tiny, 0.0, tiny, 2 * tiny,
          2.2250738585072014e-308, 1.0, 1.0000000000000002, 1.7976931348623157e308, np.inf]
    img = f64_image(np.array(xs))
    assert img.dtype == np.int64 and np.all(np.diff(img) > 0)
    assert f64_image(-0.0) == f64_image(0.0) == 0 and isinstance(f64_image(1.5), int)
    assert f64_image(-tiny) == -1 and f64_image(tiny) == 1
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-300, 300, 2000), [0.0, -0.0, np.inf, -np.inf]])
    b = rng.permutation(a)
    ia, ib = f64_image(a), f64_image(b)
    assert np.array_equal(a < b, ia < ib) and np.array_equal(a == b, ia == ib)
    nan_img = f64_image(np.array([np.nan, struct.unpack("<d", b"\xff" * 8)[0]]))
    assert nan_img[0] > f64_image(np.inf) and nan_img[1] == FIELD_NONE + 1       # total, and never FIELD_NONE
    assert f64_image(np.array([[1.0, -2.0]])).shape == (1, 2)


def test_pack_predicates():
    clauses, offsets, sets = pack_predicates([[(0, "range", 1, 5), (1, "in", [3, 1, 3], {"not_": True})], [],
                                              [{"field": 2, "op": "range", "lo": None, "hi": 9, "not_": True}]])
    assert clauses.dtype == FIELD_DTYPE and clauses.itemsize == 24
    assert clauses.tolist() == [(0, FOP_RANGE, 1, 5), (1, FOP_IN | FOP_NOT, 0, 2), (2, FOP_RANGE | FOP_NOT, FIELD_NONE + 1, 9)]
    assert offsets.tolist() == [0, 2, 2, 3] and sets.tolist() == [1, 3]
    assert pack_predicates([[(0, "range", None, None)]])[0].tolist() == [(0, 0, FIELD_NONE + 1, I64_MAX)]
    for bad in ([[(8, "range", 0, 1)]], [[(0, "like", 0, 1)]], [[(0, "range", 0, 1)] * 9], [[]] * 65,
                [[(0, "in", list(range(4097)))]], [[(0, "in", list(range(3000)))], [(1, "in", list(range(3000)))]]):
        with pytest.raises(ValueError):
            pack_predicates(bad)
    assert pack_predicates([[(0, "in", list(range(4096)))]])[2].shape == (4096,)


# ---------------------------------------------------------------- the device stand-in
class FieldVectors:
    """VectorIndex stand-in: exact top-k over the live rows, the fields in the model of tests/fields_reference.py."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        self.dim, self.xn, self.model = dim, np.zeros((0, dim), np.float32), FieldModel(0)
        self.calls = []

    def __len__(self):
        return int(self.model.ids.size)

    @property
    def next_id(self):
        return self.model.next_id

    def ids(self):
        return self.model.ids.copy()

    def add(self, x):
        x = R.normalize_rows(np.asarray(x, np.float32))
        self.xn = np.concatenate([self.xn, x], 0)
        self.model.add(x.shape[0])

    def delete(self, ids):
        keep = np.ones(len(self), bool)
        keep[self.model._pos(ids)] = False
        self.xn = self.xn[keep]
        self.model.delete(ids)

    def update(self, ids, x):
        self.xn[self.model._pos(ids)] = R.normalize_rows(np.asarray(x, np.float32))

    def get_rows(self, ids):
        return self.xn[self.model._pos(ids)]

    def set_field(self, field, ids, values):
        self.calls.append(("set_field", field, np.asarray(ids).tolist()))
        self.model.set_field(field, ids, values)

    def count_fields(self, preds):
        return self.model.match(preds, 0)[0]

    def match_fields(self, preds, cap):
        self.calls.append(("match_fields", preds))
        return self.model.match(preds, cap)

    def _topk(self, q, k, sel):
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        if sel.size == 0:
            return np.full((q.shape[0], k), -np.inf, np.float32), np.full((q.shape[0], k), -1, np.int64)
        cos, pos = R.exact_topk(self.xn[sel], R.normalize_rows(q), k)
        return cos.astype(np.float32), np.where(pos >= 0, self.model.ids[sel][np.maximum(pos, 0)], -1)

    def search(self, q, k, nprobe=0, filter_ids=None):
        self.calls.append(("search", None if filter_ids is None else np.asarray(filter_ids).tolist()))
        sel = np.arange(len(self)) if filter_ids is None else np.nonzero(np.isin(self.model.ids, filter_ids))[0]
        return self._topk(q, k, sel)

    def search_where(self, q, k, pred, filter_ids=None):
        self.calls.append(("search_where", pred))
        return self._topk(q, k, np.nonzero(self.model.mask(pred))[0])

    def search_where_each(self, q, k, preds, pred_of_query=None):
        self.calls.append(("search_where_each", preds, np.asarray(pred_of_query).tolist()))
        out = [self._topk(q[b], k, np.nonzero(self.model.mask(preds[p]))[0]) for b, p in enumerate(pred_of_query)]
        return np.concatenate([c for c, _ in out]), np.concatenate([i for _, i in out])

    def search_filtered_each(self, q, k, lists, list_of_query=None):
        self.calls.append(("search_filtered_each",))
        loq = range(len(lists)) if list_of_query is None else list_of_query
        out = [self._topk(q[b], k, np.nonzero(np.isin(self.model.ids, lists[f]))[0]) for b, f in enumerate(loq)]
        return np.concatenate([c for c, _ in out]), np.concatenate([i for _, i in out])

    def save(self, path):
        np.savez(path + ".npz", xn=self.xn, live=self.model.ids, next_id=self.model.next_id)
        os.replace(path + ".npz", path)

    @classmethod
    def load(cls, ctx, path):
        d = np.load(path)
        v = cls(ctx, d["xn"].shape[1])
        v.xn, v.model.ids, v.model.next_id = d["xn"], d["live"], int(d["next_id"])
        return v


SCHEMA = {"year": "long", "user_id": "keyword", "published": "date", "impact": "double", "open": "boolean", "pages": "integer",
          "weight": "float"}


@pytest.fixture()
def client(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", FieldVectors)
    c = RT.GpuSearchClient(ctx=object(), dim=DIM)
    c.configure_fields("idx", SCHEMA)
    return c


def _docs(n=40, seed=1):
    rng = np.random.default_rng(seed)
    docs = []
    for i in range(n):
        d = {"doc_id": f"PMC{i // 4}.txt", "text": f"chunk {i}", "year": 2000 + i % 25, "user_id": f"u{i % 5}",
             "published": f"{2000 + i % 25}-0{1 + i % 9}-15T12:00:00Z", "impact": float(rng.standard_normal()) * 3, "open": bool(i % 2),
             "pages": int(rng.integers(1, 500)), "weight": i / 8.0}
        if i % 7 == 3:
            del d["impact"]                                   # a document without a value
        if i % 11 == 5:
            d["year"] = None
        docs.append(d)
    return rng.standard_normal((n, DIM)).astype(np.float32), docs


def _fill(client, name="idx"):
    x, docs = _docs()
    RT.OpenSearchIndexer(client, name).add_embeddings(x, docs)
    return x, docs


def _rows(client, clause, name="idx"):
    idx = client.index(name)
    with idx.lock:
        return RT.filter_rows(idx, clause).tolist()


def _brute(docs, test):
    return [i for i, d in enumerate(docs) if test(d)]


def _ms(s):
    return F._date_ms(s)


# ---------------------------------------------------------------- translation of every served form
def test_filter_rows_serves_every_leaf(client):
    x, docs = _fill(client)
    year = lambda d: d.get("year")                            # noqa: E731
    assert _rows(client, {"range": {"year": {"gte": 2015}}}) == _brute(docs, lambda d: year(d) is not None and year(d) >= 2015)
    assert _rows(client, {"range": {"year": {"gt": 2015, "lte": 2020}}}) == _brute(docs, lambda d: year(d) is not None and 2015 < year(d) <= 2020)
    assert _rows(client, {"range": {"year": {"lt": 2003}}}) == _brute(docs, lambda d: year(d) is not None and year(d) < 2003)
    assert _rows(client, {"range": {"year": {"gt": 2015.5, "lt": 2018.5}}}) == _brute(docs, lambda d: year(d) in (2016, 2017, 2018))
    assert _rows(client, {"range": {"year": {"gte": 2021, "lte": 2020}}}) == []
    assert _rows(client, {"term": {"year": 2007}}) == _brute(docs, lambda d: year(d) == 2007)
    assert _rows(client, {"term": {"year": {"value": "2007"}}}) == _brute(docs, lambda d: year(d) == 2007)
    assert _rows(client, {"terms": {"year": [2001, 2002, 1900]}}) == _brute(docs, lambda d: year(d) in (2001, 2002))
    assert _rows(client, {"exists": {"field": "year"}}) == _brute(docs, lambda d: year(d) is not None)
    assert _rows(client, {"exists": {"field": "impact"}}) == _brute(docs, lambda d: "impact" in d)
    assert _rows(client, {"term": {"user_id": "u3"}}) == _brute(docs, lambda d: d["user_id"] == "u3")
    assert _rows(client, {"terms": {"user_id": ["u0", "u4", "nobody"]}}) == _brute(docs, lambda d: d["user_id"] in ("u0", "u4"))
    assert _rows(client, {"term": {"user_id": "nobody"}}) == []                   # an unknown keyword selects nothing
    assert _rows(client, {"terms": {"user_id": []}}) == []
    assert _rows(client, {"term": {"open": True}}) == _brute(docs, lambda d: d["open"])
    assert _rows(client, {"term": {"open": "false"}}) == _brute(docs, lambda d: not d["open"])
    assert _rows(client, {"range": {"impact": {"gt": 0.0}}}) == _brute(docs, lambda d: d.get("impact", -1.0) > 0.0)
    assert _rows(client, {"range": {"impact": {"lte": -0.0}}}) == _brute(docs, lambda d: d.get("impact", 1.0) <= 0.0)
    assert _rows(client, {"range": {"weight": {"gte": 0.125, "lt": 1.0}}}) == _brute(docs, lambda d: 0.125 <= d["weight"] < 1.0)
    assert _rows(client, {"term": {"weight": 0.25}}) == _brute(docs, lambda d: d["weight"] == 0.25)
    assert _rows(client, {"range": {"pages": {"gte": 100, "lte": 300}}}) == _brute(docs, lambda d: 100 <= d["pages"] <= 300)
    cut = "2010-06-01"
    assert _rows(client, {"range": {"published": {"gte": cut}}}) == _brute(docs, lambda d: _ms(d["published"]) >= _ms(cut))
    assert _rows(client, {"range": {"published": {"lt": _ms(cut)}}}) == _brute(docs, lambda d: _ms(d["published"]) < _ms(cut))
    # inside bool, beside the routes that were there: composed on the host
    got = _rows(client, {"bool": {"filter": [{"range": {"year": {"gte": 2010}}}, {"term": {"doc_id": "PMC3.txt"}}]}})
    assert got == _brute(docs, lambda d: year(d) is not None and year(d) >= 2010 and d["doc_id"] == "PMC3.txt") and got
    got = _rows(client, {"bool": {"should": [{"term": {"user_id": "u1"}}, {"range": {"year": {"lt": 2002}}}], "must_not": {"term": {"open": True}}}})
    assert got == _brute(docs, lambda d: (d["user_id"] == "u1" or (year(d) is not None and year(d) < 2002)) and not d["open"])
    assert _rows(client, {"term": {"doc_id": "PMC1.txt"}}) == [4, 5, 6, 7]         # doc_id keeps its route
    assert F._date_ms("1970-01-01") == 0 and F._date_ms("1970-01-01T00:00:01+01:00") == -3_599_000 and F._date_ms("86400000") == 86_400_000


def test_conjunctions_take_search_where(client):
    x, docs = _fill(client)
    ix = RT.OpenSearchIndexer(client, "idx")
    v = client.index("idx").vectors
    q = x[7:8] + 0.01

    def ids_of(hits):
        return [(h[0]["doc_id"], h[0]["text"]) for h in hits]

    def brute(test, k=5):
        sel = np.array(_brute(docs, test), np.int64)
        _, ids = v._topk(q, k, sel)
        return [(docs[i]["doc_id"], docs[i]["text"]) for i in ids[0] if i >= 0]

    v.calls.clear()
    flt = {"range": {"year": {"gte": 2010}}}
    assert ids_of(ix.search(q, 5, filter=flt)) == brute(lambda d: d.get("year") is not None and d["year"] >= 2010)
    assert [c[0] for c in v.calls if c[0].startswith("search")] == ["search_where"]
    assert v.calls[-1][1] == [(0, "range", 2010, I64_MAX)]
    v.calls.clear()
    flt = {"bool": {"filter": [{"range": {"year": {"gte": 2005}}}, {"terms": {"user_id": ["u1", "u2"]}}], "must_not": [{"term": {"open": True}}]}}
    assert ids_of(ix.search(q, 5, filter=flt)) == brute(lambda d: d.get("year") is not None and d["year"] >= 2005 and d["user_id"] in ("u1", "u2") and not d["open"])
    assert v.calls[-1][0] == "search_where" and v.calls[-1][1][2] == (4, "range", 1, 1, {"not_": True})
    # a bool that only excludes field leaves is such a conjunction too
    v.calls.clear()
    assert ids_of(ix.search(q, 5, filter={"bool": {"must_not": {"term": {"user_id": "u2"}}}})) == brute(lambda d: d["user_id"] != "u2")
    assert v.calls[-1][0] == "search_where"
    # mixed with another route: the host composes, the filtered search answers
    v.calls.clear()
    flt = {"bool": {"filter": [{"range": {"year": {"gte": 2005}}}, {"term": {"doc_id": "PMC4.txt"}}]}}
    assert ids_of(ix.search(q, 5, filter=flt)) == brute(lambda d: d.get("year") is not None and d["year"] >= 2005 and d["doc_id"] == "PMC4.txt")
    assert [c[0] for c in v.calls if c[0].startswith("search")] == ["search"] and any(c[0] == "match_fields" for c in v.calls)
    # search_batch: one term on user_id per query -> one search_where_each; equal clauses share a predicate
    v.calls.clear()
    users = ["u0", "u3", "u0", "nobody"]
    cos, ids = ix.search_batch(x[:4], 3, filters=[{"term": {"user_id": u}} for u in users])
    assert [c[0] for c in v.calls if c[0].startswith("search")] == ["search_where_each"]
    assert len(v.calls[-1][1]) == 3 and v.calls[-1][2] == [0, 1, 0, 2]
    for b, u in enumerate(users):
        want = v._topk(x[b], 3, np.array(_brute(docs, lambda d: d["user_id"] == u), np.int64))
        assert np.array_equal(ids[b], want[1][0]) and np.array_equal(cos[b], want[0][0])
    assert np.all(ids[3] == -1)
    # one filter that is no such conjunction: the per-query list route, as before
    v.calls.clear()
    ix.search_batch(x[:2], 3, filters=[{"term": {"user_id": "u1"}}, {"term": {"doc_id": "PMC1.txt"}}])
    assert [c[0] for c in v.calls if c[0].startswith("search")] == ["search_filtered_each"]


def test_values_are_pushed_lazily_and_follow_overwrites(client, tmp_path):
    x, docs = _fill(client)
    idx = client.index("idx")
    v = idx.vectors
    assert not any(c[0] == "set_field" for c in v.calls)                           # nothing goes out before a filter needs it
    assert _rows(client, {"term": {"year": 2001}}) == [1, 26]
    sent = [c for c in v.calls if c[0] == "set_field"]
    assert len(sent) == len(SCHEMA) and all(c[2] == list(range(40)) for c in sent)
    v.calls.clear()
    assert _rows(client, {"term": {"year": 2001}}) == [1, 26]
    assert not any(c[0] == "set_field" for c in v.calls)                           # nothing new, nothing sent
    # an overwrite changes row 1, an add appends row 40: exactly those rows go out
    new = [{"doc_id": "PMC0.txt", "text": "again", "year": 1999, "user_id": "fresh"}, {"doc_id": "PMCX.txt", "text": "new", "year": 2001}]
    RT._commit_documents(idx, x[:2], new, lambda i, d: ["PMC0.txt_1", "brand_new"][i])
    assert _rows(client, {"term": {"year": 2001}}) == [26, 40]
    assert all(c[2] == [1, 40] for c in v.calls if c[0] == "set_field")
    assert _rows(client, {"term": {"user_id": "fresh"}}) == [1] and _rows(client, {"exists": {"field": "impact"}}).count(1) == 0
    assert v.model.get_field(3, [1]).tolist() == [NONE]                            # the overwritten document has no impact any more
    # save / load: the documents keep their values, the schema is declared again, everything is pushed again
    client.save_index("idx", str(tmp_path))
    other = RT.GpuSearchClient(ctx=object(), dim=DIM)
    assert other.load_index("idx", str(tmp_path))
    with pytest.raises(ValueError):
        _rows(other, {"term": {"year": 2001}})                                      # not configured yet
    other.configure_fields("idx", SCHEMA)
    assert _rows(other, {"term": {"year": 2001}}) == [26, 40]
    assert _rows(other, {"term": {"user_id": "fresh"}}) == [1]
    sent = [c for c in other.index("idx").vectors.calls if c[0] == "set_field"]
    assert len(sent) == len(SCHEMA) and all(c[2] == list(range(41)) for c in sent)


def test_keyword_dictionary():
    s = F.FieldSchema()
    s.declare({"user_id": "keyword", "journal": "keyword"})
    assert [s.device_value("user_id", u, learn=True) for u in ("a", "b", "a", "c", 7)] == [0, 1, 0, 2, 3]
    assert s.device_value("journal", "a", learn=True) == 0                          # a dictionary per field
    assert s.device_value("user_id", "zzz", learn=False) is None and s.device_value("user_id", "7", learn=False) == 3
    assert s.device_value("user_id", None, learn=True) == FIELD_NONE
    assert s.codes["user_id"] == {"a": 0, "b": 1, "c": 2, "7": 3}
    assert s.leaf({"term": {"user_id": "b"}}) == (0, "range", 1, 1) and s.leaf({"term": {"user_id": "zzz"}}) == (0, "range", 1, 0)
    assert s.leaf({"terms": {"user_id": ["c", "a", "zzz", "a"]}}) == (0, "in", [0, 2])
    assert s.leaf({"term": {"other": "b"}}) is None and s.leaf({"match": {"text": "x"}}) is None
    with pytest.raises(ValueError):
        s.leaf({"range": {"user_id": {"gte": "a"}}})


def test_refusals(client, monkeypatch):
    x, docs = _fill(client)
    ix = RT.OpenSearchIndexer(client, "idx")
    with pytest.raises(ValueError, match="is not served"):
        _rows(client, {"range": {"nope": {"gte": 1}}})                              # an unknown field
    with pytest.raises(ValueError, match="at most 8"):
        client.configure_fields("idx", {"eighth": "long", "ninth": "long"})         # 7 declared: the ninth does not fit
    assert "eighth" not in client.index("idx").fields.slot                          # and nothing of the call stays
    client.configure_fields("idx", {"eighth": "long", "year": "long"})
    with pytest.raises(ValueError, match="already"):
        client.configure_fields("idx", {"year": "keyword"})
    for mapping in ({"a": "text"}, {"doc_id": "keyword"}):
        with pytest.raises(ValueError):
            client.configure_fields("other", mapping)
    n = len(client.index("idx").sources)
    for bad in ({"year": "nineteen"}, {"year": 2015.5}, {"year": True}, {"pages": 1 << 40}, {"impact": "x"}, {"impact": float("nan")},
                {"open": "yes"}, {"published": "last tuesday"}, {"user_id": ["a", "b"]}, {"year": 1 << 70}):
        with pytest.raises(F.FieldValueError, match="failed to parse field"):
            ix.add_embeddings(x[:2], [{"doc_id": "ok", "text": "fine", "year": 2000}, {"doc_id": "d", "text": "t", **bad}])
    assert len(client.index("idx").sources) == n and len(client.index("idx").vectors) == n      # nothing of a refused call stays
    with pytest.raises(ValueError, match="at most 4096"):
        _rows(client, {"terms": {"year": list(range(5000))}})                       # set too large
    for clause in ({"range": {"year": {"from": 1}}}, {"terms": {"year": 2000}}, {"term": {"year": [1, 2]}}, {"term": {"year": "x"}}):
        with pytest.raises(ValueError):
            _rows(client, clause)
    # fields not configured: what was there before
    plain = RT.GpuSearchClient(ctx=object(), dim=DIM)
    RT.OpenSearchIndexer(plain, "p").add_embeddings(x, docs)
    assert set(plain.index("p").sources[0]) == {"doc_id", "text"}
    for clause in ({"range": {"year": {"gte": 2015}}}, {"term": {"year": 2015}}, {"exists": {"field": "year"}}):
        with pytest.raises(ValueError, match="is not served"):
            _rows(plain, clause, "p")
    assert ix.search(x[:1], 3, filter={"range": {"nope": {"gte": 1}}}) == []        # the reference's search reports and returns nothing


# ---------------------------------------------------------------- the shim
def _bulk(lines):
    return "\n".join(json.dumps(line) for line in lines) + "\n"


def _knn(vec, k, flt=None):
    spec = {"vector": [float(v) for v in vec], "k": k}
    if flt is not None:
        spec["filter"] = flt
    return {"size": k, "query": {"knn": {"embedding": spec}}}


@pytest.mark.parametrize("per_query", [False, True])
def test_shim_mappings_and_knn_filter(monkeypatch, per_query):
    monkeypatch.setattr(RT, "VectorIndex", FieldVectors)
    client = RT.GpuSearchClient(ctx=object(), dim=DIM)
    x, docs = _docs()
    with TestClient(shim.create_app(client, None, DIM, per_query_filters=per_query)) as c:
        props = {name: {"type": t} for name, t in SCHEMA.items()}
        props.update({"embedding": {"type": "knn_vector", "dimension": DIM}, "text": {"type": "text"}, "doc_id": {"type": "keyword"}})
        assert c.put("/idx", json={"mappings": {"properties": props}}).status_code == 200
        assert client.index("idx").fields.type == SCHEMA
        nine = {f"f{i}": {"type": "long"} for i in range(9)}
        r = c.put("/big", json={"mappings": {"properties": nine}})
        assert r.status_code == 400 and r.json()["error"]["type"] == "mapper_parsing_exception" and not client.exists("big")
        lines = []
        for i, d in enumerate(docs):
            lines += [{"index": {"_index": "idx", "_id": f"id{i}"}}, {**{k: v for k, v in d.items() if v is not None}, "embedding": x[i].tolist()}]
        lines += [{"index": {"_index": "idx", "_id": "bad"}}, {"doc_id": "d", "text": "t", "year": "nineteen", "embedding": x[0].tolist()}]
        r = c.post("/_bulk", content=_bulk(lines), headers={"content-type": "application/x-ndjson"}).json()
        assert r["errors"] and [it["index"]["status"] for it in r["items"]] == [201] * 40 + [400]
        assert r["items"][-1]["index"]["error"]["type"] == "mapper_parsing_exception"
        assert len(client.index("idx").vectors) == 40
        v = client.index("idx").vectors
        year = lambda d: d.get("year")                        # noqa: E731
        cases = [({"range": {"year": {"gte": 2015}}}, lambda d: year(d) is not None and year(d) >= 2015, "search_where"),
                 ({"bool": {"filter": [{"term": {"user_id": "u2"}}], "must_not": [{"range": {"year": {"lt": 2005}}}]}},
                  lambda d: d["user_id"] == "u2" and not (year(d) is not None and year(d) < 2005), "search_where"),
                 ({"bool": {"filter": [{"range": {"year": {"gte": 2005}}}, {"term": {"doc_id": "PMC4.txt"}}]}},
                  lambda d: year(d) is not None and year(d) >= 2005 and d["doc_id"] == "PMC4.txt", "search")]
        for flt, test, route in cases:
            v.calls.clear()
            r = c.post("/idx/_search", json=_knn(x[3], 4, flt))
            assert r.status_code == 200
            _, want = v._topk(x[3], 4, np.array(_brute(docs, test), np.int64))
            hits = r.json()["hits"]["hits"]
            assert [h["_id"] for h in hits] == [f"id{i}" for i in want[0] if i >= 0]
            searches = [call[0] for call in v.calls if call[0].startswith("search")]
            assert searches == [{"search_where": "search_where_each", "search": "search_filtered_each"}[route] if per_query else route]
        assert hits[0]["_source"]["doc_id"] == "PMC4.txt" and "year" in hits[0]["_source"]
        r = c.post("/idx/_search", json=_knn(x[3], 4, {"range": {"nope": {"gte": 1}}}))
        assert r.status_code == 400
        r = c.post("/idx/_search", json=_knn(x[3], 4, {"range": {"user_id": {"gte": "a"}}}))
        assert r.status_code == 400
        # an index made without mappings keeps the 400 for range
        c.put("/plain")
        r = c.post("/plain/_search", json=_knn(x[3], 4, {"range": {"year": {"gte": 2015}}}))
        assert r.status_code == 400


# ---------------------------------------------------------------- the host-only argument checks under ASan + UBSan
def _np_check(n_preds, offsets, clauses, n_set, sets):
    """NumPy restatement of fieldpred_check: True = refused"""
    if not 0 <= n_preds <= 64 or not 0 <= n_set <= 4096:
        return True
    if n_preds == 0:
        return False
    if offsets[0] != 0:
        return True
    for j in range(n_preds):
        if offsets[j + 1] < offsets[j] or offsets[j + 1] - offsets[j] > 8:
            return True
    for field, op, lo, hi in clauses[:offsets[n_preds]]:
        if not 0 <= field < 8 or (op & ~0x100) not in (0, 1):
            return True
        if op & 1:
            if lo < 0 or hi < lo or hi > n_set:
                return True
            if any(sets[i] <= sets[i - 1] for i in range(lo + 1, hi)):
                return True
    return False


def _np_plan(n_preds, offsets, clauses):
    first, plan = [], []
    for f in range(8):
        first.append(len(plan))
        for j in range(n_preds):
            for c in range(offsets[j], offsets[j + 1]):
                if clauses[c][0] == f:
                    plan.append((f, clauses[c][1], j, clauses[c][2], clauses[c][3]))
    return first + [len(plan)], plan


def test_fieldpred_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "fieldpred_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build_san", "fieldpred_asan")
    rng = np.random.default_rng(11)
    r = (0, 0, -5, 5)
    cases = [                                                  # (n_preds, offsets, clauses, n_set, sets)
        (0, [], [], 0, []),
        (1, [0, 0], [], 0, []),
        (1, [0, 1], [r], 0, []),
        (64, list(range(65)), [r] * 64, 0, []),
        (65, list(range(66)), [r] * 65, 0, []),                # too many predicates: the offsets are not read
        (65, [], [], 0, []),
        (-1, [0], [], 0, []),
        (1, [0, 8], [r] * 8, 0, []),
        (1, [0, 9], [r] * 9, 0, []),                           # too many clauses: the clauses are not read
        (1, [0, 9], [], 0, []),
        (2, [1, 1, 2], [r, r], 0, []),                         # does not start at 0
        (2, [0, 2, 1], [r, r], 0, []),                         # decreases
        (2, [0, -1, 1], [r], 0, []),
        (1, [0, 1], [(8, 0, 0, 1)], 0, []),
        (1, [0, 1], [(-1, 0, 0, 1)], 0, []),
        (1, [0, 1], [(0, 2, 0, 1)], 0, []),
        (1, [0, 1], [(0, 0x200, 0, 1)], 0, []),
        (1, [0, 1], [(7, 0x101, 0, 3)], 3, [1, 2, 3]),
        (1, [0, 1], [(7, 1, 0, 4)], 3, [1, 2, 3]),             # past the set: the values are not read
        (1, [0, 1], [(7, 1, -1, 2)], 3, [1, 2, 3]),
        (1, [0, 1], [(7, 1, 2, 1)], 3, [1, 2, 3]),
        (1, [0, 1], [(7, 1, 1 << 40, (1 << 40) + 2)], 3, [1, 2, 3]),
        (1, [0, 1], [(7, 1, 0, 3)], 3, [1, 2, 2]),             # not strictly ascending
        (1, [0, 1], [(7, 1, 0, 3)], 3, [3, 2, 1]),
        (2, [0, 1, 2], [(7, 1, 0, 2), (0, 1, 2, 3)], 3, [1, 2, 0]),     # slices are ordered one by one
        (1, [0, 1], [(0, 1, 0, 0)], 0, []),                    # an empty slice
        (1, [0, 1], [(0, 1, 0, 4096)], 4096, list(range(4096))),
        (1, [0, 1], [r], 4097, list(range(4097))),
        (1, [0, 1], [r], 4097, []),                            # too many set values: they are not read
        (1, [0, 1], [r], -1, []),
        (1, [0, 1], [(0, 0, -(1 << 63), (1 << 63) - 1)], 0, []),
    ]
    for _ in range(40):                                        # random well-formed tables: the plan
        n_preds = int(rng.integers(1, 65))
        lens = rng.integers(0, 9, n_preds)
        offsets = [0] + np.cumsum(lens).tolist()
        n_set = int(rng.integers(0, 50))
        sets = np.sort(rng.choice(1000, n_set, replace=False)).tolist()
        clauses = []
        for _c in range(offsets[-1]):
            if n_set and rng.random() < 0.4:
                lo = int(rng.integers(0, n_set + 1))
                clauses.append((int(rng.integers(0, 8)), 1 | (0x100 if rng.random() < 0.5 else 0), lo, int(rng.integers(lo, n_set + 1))))
            else:
                clauses.append((int(rng.integers(0, 8)), 0x100 if rng.random() < 0.5 else 0, int(rng.integers(-99, 99)), int(rng.integers(-99, 99))))
        cases.append((n_preds, offsets, clauses, n_set, sets))
    blob = b""
    for n_preds, offsets, clauses, n_set, sets in cases:
        blob += struct.pack("<qq", n_preds, len(offsets)) + np.array(offsets, "<i8").tobytes()
        blob += struct.pack("<q", len(clauses)) + np.array(clauses, dtype=FIELD_DTYPE).tobytes()
        blob += struct.pack("<qq", n_set, len(sets)) + np.array(sets, "<i8").tobytes()
    (tmp_path / "cases.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == f"ok {len(cases)} cases" and "ERROR" not in p.stderr and "runtime error" not in p.stderr
    out = (tmp_path / "out.bin").read_bytes()
    at = 0
    refused = 0
    for n_preds, offsets, clauses, n_set, sets in cases:
        status, = struct.unpack_from("<i", out, at)
        at += 4
        assert status == int(_np_check(n_preds, offsets, clauses, n_set, sets)), (n_preds, offsets, clauses[:3], n_set)
        refused += status
        if status:
            continue
        first = list(struct.unpack_from("<9i", out, at))
        n, = struct.unpack_from("<i", out, at + 36)
        at += 40
        plan = [struct.unpack_from("<iiiqq", out, at + 28 * i) for i in range(n)]
        at += 28 * n
        want_first, want_plan = _np_plan(n_preds, offsets, clauses)
        assert first == want_first and plan == want_plan
    assert at == len(out) and refused == 21
