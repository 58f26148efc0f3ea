"""A filter together with radial, collapsed or MMR search on the host side (no GPU): OpenSearchIndexer.search_within, which
method of the index it calls and with which predicate or allow-list, the shape of what it returns, the combinations ``search``
still refuses, and the ctypes signatures of the new calls against include/sqe.h.  The device index is a NumPy stand-in."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import retrieval as R
from semantic_query_engine_amd import retrieval as RT
from tests.test_fields_cpu import FieldVectors

DIM = 16
NONE = -(1 << 63)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class WithinVectors(FieldVectors):
    """VectorIndex stand-in: FieldVectors plus group keys and the three searches that take ``pred`` / ``filter_ids``, each
    answered from an fp32 NumPy product over the selected rows."""

    def __init__(self, ctx=None, dim=DIM, kind=0, nlist=0):
        super().__init__(ctx, dim, kind, nlist)
        self.keys = {}

    def set_keys(self, ids, keys):
        self.keys.update(zip(np.asarray(ids).tolist(), np.asarray(keys).tolist()))

    def _rows(self, pred, filter_ids):
        """positions of the rows the predicate selects, intersected with the list when there is one"""
        sel = self.model.mask([] if pred is None else pred)
        if filter_ids is not None:
            sel &= np.isin(self.model.ids, filter_ids)
        return np.nonzero(sel)[0]

    def _ranked(self, q, pos):
        c = (R.normalize_rows(np.asarray(q, np.float32).reshape(1, -1)) @ self.xn[pos].T)[0].astype(np.float32)
        order = np.lexsort((pos, -c))
        return c[order], self.model.ids[pos[order]]

    @staticmethod
    def _pad(rows, k):
        cos = np.full((1, k), -np.inf, np.float32)
        ids = np.full((1, k), -1, np.int64)
        for j, (c, i) in enumerate(rows[:k]):
            cos[0, j], ids[0, j] = c, i
        return cos, ids

    def _note(self, what, pred, filter_ids):
        self.calls.append((what, pred, None if filter_ids is None else sorted(np.asarray(filter_ids).tolist())))

    def range_search(self, q, min_cos, max_hits=10, pred=None, filter_ids=None):
        self._note("range_search", pred, filter_ids)
        c, ids = self._ranked(q, self._rows(pred, filter_ids))
        keep = c >= np.float32(min_cos)
        cos, out = self._pad(list(zip(c[keep], ids[keep])), max_hits)
        return np.array([int(keep.sum())], np.int64), cos, out

    def search_collapsed(self, q, k, pred=None, filter_ids=None):
        self._note("search_collapsed", pred, filter_ids)
        c, ids = self._ranked(q, self._rows(pred, filter_ids))
        seen, rows = set(), []
        for ci, i in zip(c, ids):
            key = self.keys.get(int(i), NONE)
            if key != NONE and key in seen:
                continue
            seen.add(key)
            rows.append((ci, i))
        cos, out = self._pad(rows, k)
        return cos, out, np.array([[self.keys.get(int(i), NONE) if i >= 0 else NONE for i in out[0]]], np.int64)

    def search_mmr(self, q, k, lam=0.5, n_cand=0, nprobe=0, pred=None, filter_ids=None):
        self._note("search_mmr", pred, filter_ids)
        self.calls.append(("mmr_args", float(lam), int(n_cand)))
        c, ids = self._ranked(q, self._rows(pred, filter_ids))
        cos, out = self._pad(list(zip(c, ids)), k)                    # the stand-in keeps the ranking: lambda 1
        return cos, out, cos.copy()


SCHEMA = {"year": "long", "user_id": "keyword"}


@pytest.fixture()
def indexer(monkeypatch):
    monkeypatch.setattr(RT, "VectorIndex", WithinVectors)
    client = RT.GpuSearchClient(ctx=object(), dim=DIM)
    client.configure_fields("idx", SCHEMA)
    rng = np.random.default_rng(4)
    n = 48
    centre = rng.standard_normal((n // 4, DIM)).astype(np.float32)
    x = (np.repeat(centre, 4, axis=0) + 0.2 * rng.standard_normal((n, DIM))).astype(np.float32)
    docs = [{"doc_id": f"D{i // 4}", "text": f"t{i}", "year": 2000 + i % 20, "user_id": f"u{i % 3}"} for i in range(n)]
    ix = RT.OpenSearchIndexer(client, "idx")
    ix.add_embeddings(x, docs)
    q = (centre[0] + 0.5 * centre[1] + 0.3 * centre[2]).astype(np.float32)[None]
    return ix, client.index("idx").vectors, x, docs, q


def _cos(x, q):
    return (R.normalize_rows(q) @ R.normalize_rows(x).T)[0]


def _named(vec, what):
    return [c for c in vec.calls if c[0] == what]


FIELDS = {"bool": {"filter": [{"range": {"year": {"gte": 2005}}}, {"term": {"user_id": "u1"}}]}}
DOC = {"terms": {"doc_id": ["D0", "D2", "D5"]}}
MIXED = {"bool": {"filter": [{"range": {"year": {"gte": 2005}}}, {"terms": {"doc_id": ["D0", "D1", "D2", "D5"]}}]}}


def _selected(docs, clause):
    if clause is FIELDS:
        return [i for i, d in enumerate(docs) if d["year"] >= 2005 and d["user_id"] == "u1"]
    if clause is DOC:
        return [i for i, d in enumerate(docs) if d["doc_id"] in ("D0", "D2", "D5")]
    return [i for i, d in enumerate(docs) if d["year"] >= 2005 and d["doc_id"] in ("D0", "D1", "D2", "D5")]


@pytest.mark.parametrize("clause", [FIELDS, DOC, MIXED], ids=["field_conjunction", "doc_id_terms", "bool_of_both"])
def test_which_method_is_called_with_which_row_set(indexer, clause):
    ix, vec, x, docs, q = indexer
    sel = _selected(docs, clause)
    assert 3 <= len(sel) < len(docs)
    c = _cos(x, q)
    ranked = sorted(sel, key=lambda r: (-c[r], r))
    for what, kwargs in (("search_collapsed", {"collapse": {"field": "doc_id"}}), ("range_search", {"min_score": 0.55}),
                         ("range_search", {"max_distance": 0.9}), ("search_mmr", {"mmr": {"lambda": 1.0, "candidates": 8}})):
        vec.calls.clear()
        hits = ix.search_within(q, 3, clause, **kwargs)
        (_, pred, allow), = _named(vec, what)
        if clause is FIELDS:          # a conjunction of field leaves: the predicate goes down, no id list is made
            assert allow is None and len(pred) == 2 and not _named(vec, "match_fields")
        else:                         # anything else: its rows as the allow-list, zero clauses
            assert pred is None and allow == sel
        assert not [c_ for c_ in vec.calls if c_[0] in ("search", "search_where")]
        # the return shape and the _score rule of search
        assert all(set(h[0]) == {"doc_id", "text", "year", "user_id", "embedding"} for h in hits)
        rows = [int(h[0]["text"][1:]) for h in hits]
        assert set(rows) <= set(sel)
        for h, r in zip(hits, rows):
            assert abs(h[1] - 1.0 / (2.0 - float(c[r]))) < 1e-6 and len(h[0]["embedding"]) == DIM
        if what == "search_collapsed":
            want, seen = [], set()
            for r in ranked:
                if docs[r]["doc_id"] not in seen:
                    seen.add(docs[r]["doc_id"])
                    want.append(r)
            assert rows == want[:3]
        elif what == "search_mmr":
            assert rows == ranked[:3] and _named(vec, "mmr_args") == [("mmr_args", 1.0, 8)]
        else:
            floor = RT.radial_min_cos(kwargs.get("min_score"), kwargs.get("max_distance"))
            assert rows == [r for r in ranked if np.float32(c[r]) >= floor][:3]


def test_without_a_kind_it_is_the_filtered_search(indexer):
    ix, vec, x, docs, q = indexer
    vec.calls.clear()
    hits = ix.search_within(q, 4, FIELDS)
    assert [c[0] for c in vec.calls if c[0].startswith(("search", "range"))] == ["search_where"]
    assert [h[0]["text"] for h in hits] == [h[0]["text"] for h in ix.search(q, 4, filter=FIELDS)]


def test_at_most_one_kind_and_a_filter(indexer):
    ix, vec, x, docs, q = indexer
    col, mmr = {"field": "doc_id"}, {"lambda": 0.5}
    for bad in ({"collapse": col, "mmr": mmr}, {"collapse": col, "min_score": 0.5}, {"mmr": mmr, "max_distance": 0.5},
                {"min_score": 0.5, "max_distance": 0.5}, {"collapse": col, "mmr": mmr, "min_score": 0.5}):
        with pytest.raises(ValueError):
            ix.search_within(q, 3, FIELDS, **bad)
    with pytest.raises(ValueError):
        ix.search_within(q, 3, None, collapse=col)
    for bad in ({"collapse": {"field": "text"}}, {"mmr": {"lambda": 2.0}}, {"mmr": {"lambda": 0.5, "candidates": 2}}):
        with pytest.raises(ValueError):
            ix.search_within(q, 3, FIELDS, **bad)


def test_search_still_refuses_the_combinations(indexer):
    ix, vec, x, docs, q = indexer
    for bad in ({"collapse": {"field": "doc_id"}}, {"min_score": 0.5}, {"max_distance": 0.5}, {"mmr": {"lambda": 0.5}}):
        for clause in (FIELDS, DOC):
            with pytest.raises(ValueError):
                ix.search(q, 3, filter=clause, **bad)


def test_positional_calls_of_older_stand_ins_keep_working(monkeypatch):
    """with neither a predicate nor a list the methods make the call they made before: a stand-in without the new arguments"""
    from tests.test_collapse_cpu import CollapseVectors
    monkeypatch.setattr(RT, "VectorIndex", CollapseVectors)
    client = RT.GpuSearchClient(ctx=object(), dim=DIM)
    ix = RT.OpenSearchIndexer(client, "idx")
    rng = np.random.default_rng(0)
    ix.add_embeddings(rng.standard_normal((8, DIM)).astype(np.float32), [{"doc_id": f"D{i // 2}", "text": f"t{i}"} for i in range(8)])
    hits = ix.search(rng.standard_normal((1, DIM)).astype(np.float32), 3, collapse={"field": "doc_id"})
    assert len({h[0]["doc_id"] for h in hits}) == 3


# ---------------------------------------------------------------- the ctypes table against the header
NEW = ["sqe_index_range_search_where", "sqe_index_range_search_where_device", "sqe_index_search_collapsed_where",
       "sqe_index_search_collapsed_where_device", "sqe_index_search_mmr_where", "sqe_index_search_mmr_where_device",
       "sqe_index_within_last"]


def test_ctypes_signatures_pack_as_the_header_declares():
    from semantic_query_engine_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sqe.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, name
        want = []
        for param in m.group(1).split(","):
            param = " ".join(param.split())
            if "sqe_within_last_t*" in param:
                want.append(C.POINTER(N.WithinLast))
            elif "*" in param:
                want.append(C.c_void_p)
            elif param.startswith("int64_t "):
                want.append(C.c_int64)
            else:
                assert param.startswith("int "), (name, param)
                want.append(C.c_int)
        res, args = N.SIGNATURES[name]
        assert res is C.c_int and args == want, name
    # the row-set arguments are those of sqe_index_search_where, in its order, after the arguments of the unrestricted call
    row_set = N.SIGNATURES["sqe_index_search_where"][1][4:10]
    for name, plain in (("sqe_index_range_search_where", "sqe_index_range_search"), ("sqe_index_search_collapsed_where", "sqe_index_search_collapsed"),
                        ("sqe_index_search_mmr_where", "sqe_index_search_mmr")):
        for suffix in ("", "_device"):
            args, base = N.SIGNATURES[name + suffix][1], N.SIGNATURES[plain + suffix][1]
            head = {"sqe_index_range_search": 5, "sqe_index_search_collapsed": 4, "sqe_index_search_mmr": 7}[plain]
            assert args == base[:head] + row_set + base[head:], name + suffix
    assert C.sizeof(N.WithinLast) == 40 and [f[0] for f in N.WithinLast._fields_] == ["kind", "route", "depth", "pad", "selected", "live", "swept"]
    body = re.search(r"typedef struct \{([^}]*)\} sqe_within_last_t;", text).group(1)
    assert " ".join(body.split()) == "int32_t kind, route, depth, pad; int64_t selected, live, swept;"
