"""The CPU side of the boolean lexical queries: the NumPy reference (tests/lexbool_reference.py) against cases worked out by
hand on the five-document corpus of tests/test_lexical_cpu.py, the translator from OpenSearch text clauses to (terms, roles,
min_should), the composition of a text clause with the other filter clauses against a fake lexical object, and the ctypes
table against the header's declarations.  No GPU."""
import os
import re
import threading

import numpy as np
import pytest

from oracle import wordpiece as WP
from tests import lex_reference as LR
from tests import lexbool_reference as BR
from tests.lexbool_reference import FILTER, MUST, MUST_NOT, SHOULD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ the reference, by hand
@pytest.fixture(scope="module")
def hand():
    """ids 10..14 with bags 10: [0, 0, 1], 11: [1, 2], 12: [0, 2, 2, 2, 3], 13: [], 14: [1]; term 4 is in no document.
    Impacts (tests/test_lexical_cpu.py works them out): 10: {0: 32532, 1: 13977}, 11: {1: 16676, 2: 27087},
    12: {0: 17150, 2: 32200, 3: 27157}, 14: {1: 20668}."""
    ids = [12, 10, 14, 11, 13]
    bags = {10: [0, 0, 1], 11: [1, 2], 12: [0, 2, 2, 2, 3], 13: [], 14: [1]}
    return BR.LexBoolRef(LR.LexRef(ids, [bags[i] for i in ids], 5))


def ask(ref, terms, roles, ms=0, k=5):
    """-> ([(id, score_int), ...] of the hits in rank order, the match set)"""
    score, ids, sint = ref.search([terms], [roles], k, [ms])
    n = int((ids[0] >= 0).sum())
    counts, mids, _ = ref.match([terms], [roles], [ms])
    assert counts[0] == n and np.all(np.isneginf(score[0, n:])) and np.all(ids[0, n:] == -1)
    assert [float(s) for s in score[0, :n]] == [float(np.float32(int(v) / 65536)) for v in sint[0, :n]]
    return list(zip(ids[0, :n].tolist(), sint[0, :n].tolist())), mids[0].tolist()


def test_all_should_is_the_plain_search(hand):
    for q in ([0, 1], [1, 1], [4], [], [2, 3, 2]):
        want = hand.ref.search([q], 4)
        got = hand.search([q], [[SHOULD] * len(q)], 4)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_m_is_one_without_a_required_occurrence(hand):
    # SHOULD 0, SHOULD 3, min_should 0: m = max(1, 0) = 1 -- documents 10 and 12, not every document
    assert ask(hand, [0, 3], [SHOULD, SHOULD], 0) == ([(12, 17150 + 27157), (10, 32532)], [10, 12])
    assert ask(hand, [0, 3], [SHOULD, SHOULD], 1) == ask(hand, [0, 3], [SHOULD, SHOULD], 0)
    assert ask(hand, [0, 3], [SHOULD, SHOULD], 2) == ([(12, 44307)], [12])


def test_m_is_min_should_with_a_required_occurrence(hand):
    # MUST 1, SHOULD 0, min_should 0: the SHOULD term only scores -- 10, 11 and 14 match; 10 adds I(0)
    assert ask(hand, [1, 0], [MUST, SHOULD], 0) == ([(10, 13977 + 32532), (14, 20668), (11, 16676)], [10, 11, 14])
    assert ask(hand, [1, 0], [MUST, SHOULD], 1) == ([(10, 46509)], [10])
    assert ask(hand, [1, 0], [MUST, SHOULD], 2) == ([], [])            # above the number of SHOULD occurrences


def test_must_not_only_and_empty_match_nothing(hand):
    assert ask(hand, [3], [MUST_NOT]) == ([], [])                      # not "everything but document 12"
    assert ask(hand, [], []) == ([], [])
    assert ask(hand, [1, 2], [SHOULD, MUST_NOT]) == ([(14, 20668), (10, 13977)], [10, 14])


def test_a_term_no_document_holds(hand):
    assert ask(hand, [4, 1], [MUST, SHOULD]) == ([], [])               # df = 0 as MUST: holds nowhere
    assert ask(hand, [1, 4], [MUST, MUST_NOT]) == ask(hand, [1], [MUST])      # df = 0 as MUST_NOT: denies nothing
    assert ask(hand, [1], [MUST])[1] == [10, 11, 14]


def test_a_repeated_should_occurrence_counts_each_time(hand):
    # SHOULD 0 twice, min_should 2: one term reaches the count, and scores twice
    assert ask(hand, [0, 0], [SHOULD, SHOULD], 2) == ([(10, 2 * 32532), (12, 2 * 17150)], [10, 12])
    assert ask(hand, [0, 0, 3], [SHOULD] * 3, 3) == ([(12, 2 * 17150 + 27157)], [12])
    assert ask(hand, [0, 0], [MUST, MUST])[0] == [(10, 65064), (12, 34300)]


def test_filter_only_matches_score_zero_and_rank_last(hand):
    assert ask(hand, [1], [FILTER]) == ([(10, 0), (11, 0), (14, 0)], [10, 11, 14])      # ties to the lowest id
    # FILTER 1, SHOULD 2, min_should 0: document 11 scores, 10 and 14 are hits with score 0.0 after it
    hits, ids = ask(hand, [1, 2], [FILTER, SHOULD])
    assert hits == [(11, 27087), (10, 0), (14, 0)] and ids == [10, 11, 14]
    score, got, _ = hand.search([[1, 2]], [[FILTER, SHOULD]], 2)
    assert got.tolist() == [[11, 10]] and score.tolist() == [[float(np.float32(27087 / 65536)), 0.0]]
    assert ask(hand, [1, 0], [MUST, MUST_NOT]) == ([(14, 20668), (11, 16676)], [11, 14])


# ------------------------------------------------------------------------------ the translator
WORDS = ["aspirin reduces fever and pain in adult patients", "the brca1 gene and breast cancer risk",
         "metformin is a first line treatment of type 2 diabetes", "fever pain aspirin aspirin"]


@pytest.fixture()
def analyzer():
    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    toks = WP.synthetic_vocab(WORDS, size=400)
    RT.configure_analyzer(WordPieceTokenizer(vocab_text="\n".join(toks) + "\n"), max_len=64)
    yield RT._analyzer
    RT.configure_analyzer(None)


def m(text, **opts):
    return {"match": {"text": dict(query=text, **opts) if opts else text}}


def test_translator_accepts(analyzer):
    from semantic_query_engine_amd import retrieval as RT

    def t(text):
        terms = analyzer.query(text).tolist()
        assert len(terms) == len(text.split())                   # these words are whole word pieces
        return terms

    def tr(clause):
        terms, roles, ms = RT.text_query(clause)
        assert terms.dtype == np.int32 and roles.dtype == np.uint8
        return terms.tolist(), roles.tolist(), ms

    a, f, p, g = t("aspirin")[0], t("fever")[0], t("pain")[0], t("gene")[0]
    assert tr(m("aspirin fever")) == ([a, f], [SHOULD, SHOULD], 0)
    assert tr({"match": {"text": {"query": "aspirin fever"}}}) == ([a, f], [SHOULD, SHOULD], 0)
    assert tr(m("aspirin fever", operator="or")) == ([a, f], [SHOULD, SHOULD], 0)
    assert tr(m("aspirin fever", operator="and")) == ([a, f], [MUST, MUST], 0)
    assert tr(m("aspirin fever", operator="AND")) == ([a, f], [MUST, MUST], 0)
    assert tr(m("aspirin fever pain", minimum_should_match=2)) == ([a, f, p], [SHOULD] * 3, 2)
    assert tr(m("aspirin fever pain", minimum_should_match="2")) == ([a, f, p], [SHOULD] * 3, 2)
    assert tr(m("aspirin fever pain", minimum_should_match=0))[2] == 0
    # percentages are floored: 3 terms at 67 % -> 2.01 -> 2, at 66 % -> 1.98 -> 1, at 34 % -> 1.02 -> 1, at 33 % -> 0
    assert [tr(m("aspirin fever pain", minimum_should_match=f"{pc}%"))[2] for pc in (100, 67, 66, 34, 33)] == [3, 2, 1, 1, 0]
    assert tr(m("aspirin fever pain gene", minimum_should_match="75%"))[2] == 3
    assert tr(m("aspirin aspirin")) == ([a, a], [SHOULD, SHOULD], 0)            # occurrences, not distinct terms
    bool_ = {"bool": {"must": [m("aspirin"), m("fever pain", operator="and")], "should": [m("gene"), m("pain aspirin")],
                      "filter": m("fever"), "must_not": [m("gene pain"), m("aspirin fever", operator="and")]}}
    assert tr(bool_) == ([a, f, p, f, g, p, a, g, p, a, f], [MUST] * 3 + [FILTER] + [SHOULD] * 3 + [MUST_NOT] * 4, 0)
    assert tr({"bool": {"should": [m("gene"), m("pain"), m("fever")], "minimum_should_match": 2}}) == ([g, p, f], [SHOULD] * 3, 2)
    assert tr({"bool": {"should": [m("gene"), m("pain"), m("fever")], "minimum_should_match": "67%"}})[2] == 2
    assert tr({"bool": {"should": [m("gene pain")], "minimum_should_match": 1}}) == ([g, p], [SHOULD] * 2, 1)
    assert tr({"bool": {"filter": [m("gene")]}}) == ([g], [FILTER], 0)
    # a bool that is one must clause is that clause
    assert tr({"bool": {"must": [m("aspirin fever pain", minimum_should_match=2)]}}) == ([a, f, p], [SHOULD] * 3, 2)
    assert tr({"bool": {"must": m("aspirin fever", operator="and")}}) == ([a, f], [MUST, MUST], 0)
    assert tr(m("")) == ([], [], 0)


@pytest.mark.parametrize("clause", [
    {"match": {"title": "aspirin"}}, {"match": {"text": "a", "doc_id": "b"}}, {"match": {"text": 5}}, {"match": "aspirin"},
    m("aspirin", fuzziness="AUTO"), m("aspirin", operator="xor"), {"match": {"text": {"operator": "and"}}},
    m("aspirin fever", minimum_should_match=-1), m("aspirin fever", minimum_should_match="-50%"), m("aspirin fever", minimum_should_match=1.5),
    m("aspirin fever", minimum_should_match=True), m("aspirin fever", operator="and", minimum_should_match=1),
    {"bool": {"must": [m("aspirin fever"), m("pain")]}},                            # must of a multi-term OR match
    {"bool": {"filter": [m("aspirin fever")], "should": [m("pain")]}},
    {"bool": {"should": [m("aspirin fever", operator="and"), m("pain")]}},
    {"bool": {"should": [m("aspirin fever"), m("pain")], "minimum_should_match": 2}},      # clauses there, occurrences here
    {"bool": {"should": [m("aspirin"), m("pain")], "minimum_should_match": -1}},
    {"bool": {"must": [{"bool": {"must": [m("aspirin")]}}, m("pain")]}},            # nested
    {"bool": {"must": [{"term": {"doc_id": "x"}}, m("pain")]}},
    {"bool": {"must": [m("aspirin"), m("pain", minimum_should_match=1)]}},
    {"bool": {"must_not": [m("aspirin")]}}, {"bool": {}}, {"bool": {"boost": 2, "must": [m("aspirin"), m("pain")]}},
    {"match_phrase": {"text": "aspirin fever"}}, {"term": {"text": "aspirin"}},
    {"bool": {"must": [m(" ".join(["aspirin"] * 40), operator="and")], "should": [m(" ".join(["fever"] * 30))]}},      # 70 occurrences
    "aspirin", [m("aspirin")], {"match": {"text": "a"}, "bool": {}}])
def test_translator_refuses(analyzer, clause):
    from semantic_query_engine_amd import retrieval as RT
    with pytest.raises(ValueError):
        RT.text_query(clause)


def test_translator_needs_an_analyzer():
    from semantic_query_engine_amd import retrieval as RT
    assert RT._analyzer is None
    with pytest.raises(ValueError):
        RT.text_query(m("aspirin"))


# ------------------------------------------------------------------------------ filter composition
class FakeLex:
    """LexicalIndex stand-in: ``match`` answered by the dense reference over the analysed texts."""

    def __init__(self, n_terms, bags):
        self.ref = BR.LexBoolRef(LR.LexRef(np.arange(len(bags)), bags, n_terms))
        self.calls = []

    def match(self, queries, roles, min_should=None, cap=None):
        self.calls.append(([np.asarray(q).tolist() for q in queries], [np.asarray(r).tolist() for r in roles], list(min_should), cap))
        return self.ref.match(queries, roles, min_should, cap)[:2]

    def count(self, queries, roles, min_should=None):
        return self.match(queries, roles, min_should, cap=0)[0]


class FakeVectors:
    def __init__(self, n):
        self.n = n

    def ids(self):
        return np.arange(self.n, dtype=np.int64)


class FakeNamed:
    def __init__(self, texts, doc_ids):
        self.vectors, self.lock = FakeVectors(len(texts)), threading.Lock()
        self.sources = [{"doc_id": d, "text": t} for d, t in zip(doc_ids, texts)]
        self.row_of_id = {f"{d}_{r}": r for r, d in enumerate(doc_ids)}


@pytest.fixture()
def named(analyzer, monkeypatch):
    from semantic_query_engine_amd import retrieval as RT
    texts = WORDS + ["aspirin and the gene", "pain"]
    idx = FakeNamed(texts, ["d0", "d1", "d0", "d1", "d2", "d2"])
    lex = FakeLex(analyzer.n_terms, analyzer.analyze(texts))
    monkeypatch.setattr(RT, "push_text", lambda named: lex)
    return idx, lex


def test_text_clauses_compose_with_the_other_filter_clauses(named):
    from semantic_query_engine_amd import retrieval as RT
    idx, lex = named

    def rows(clause):
        out = RT.filter_rows(idx, clause)
        assert out.dtype == np.int64
        return out.tolist()

    assert rows(m("aspirin")) == [0, 3, 4] and rows(m("aspirin fever", operator="and")) == [0, 3]
    assert lex.calls[-1][1:] == ([[MUST, MUST]], [0], None)
    d0 = {"terms": {"doc_id": ["d0", "d2"]}}                       # rows 0, 2, 4, 5
    assert rows({"bool": {"filter": [d0, m("aspirin")]}}) == [0, 4]                        # intersection with terms on doc_id
    assert rows({"bool": {"must": [m("aspirin")], "filter": {"term": {"doc_id": "d1"}}}}) == [3]
    assert rows({"bool": {"filter": [d0], "must_not": [m("aspirin")]}}) == [2, 5]          # must_not
    assert rows({"bool": {"must_not": m("aspirin")}}) == [1, 2, 5]
    assert rows({"bool": {"should": [m("gene"), {"ids": {"values": ["d2_5"]}}]}}) == [1, 4, 5]
    assert rows({"bool": {"filter": [m("pain fever gene", minimum_should_match=2)]}}) == [0, 3]
    assert RT.exclusion_rows(idx, {"bool": {"must_not": [m("aspirin"), {"term": {"doc_id": "d1"}}]}}).tolist() == [0, 1, 3, 4]
    lists, loq = RT.resolve_each(idx, [m("aspirin"), None, {"bool": {"filter": [d0, m("aspirin")]}}, m("aspirin")])
    assert [x.tolist() for x in lists] == [[0, 3, 4], [0, 4]] and loq.tolist() == [0, -1, 1, 0]
    for bad in (m("aspirin", fuzziness=1), {"bool": {"filter": [d0, {"match": {"title": "x"}}]}}, {"match_phrase": {"text": "a b"}}):
        with pytest.raises(ValueError):
            RT.filter_rows(idx, bad)


def test_indexer_count_text_and_search_text(named):
    from semantic_query_engine_amd import retrieval as RT

    class Client:
        def index(self, name):
            return named[0]

    ix = RT.OpenSearchIndexer(Client(), "docs")
    assert ix.count_text("aspirin") == 3 and ix.count_text(m("aspirin fever", operator="and")) == 2
    assert ix.count_text({"bool": {"must": [m("aspirin")], "must_not": [m("gene")]}}) == 2
    with pytest.raises(ValueError):
        ix.count_text({"bool": {"must_not": [m("gene")]}})


# ------------------------------------------------------------------------------ the ctypes table
def test_native_table_carries_the_headers_signatures():
    """Both entry points, host and _device forms, with the header's parameter lists: a pointer is c_void_p, B and k are int,
    cap is int64."""
    import ctypes as C

    from semantic_query_engine_amd import _native as N
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sqe.h")).read(), flags=re.S)
    for name in ("sqe_lex_search_bool", "sqe_lex_search_bool_device", "sqe_lex_match", "sqe_lex_match_device"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        want = [C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int for p in params]
        res, args = N.SIGNATURES[name]
        assert res is C.c_int and args == want, (name, params)
    assert [p.split()[-1] for p in params[:6]] == ["lex", "qoffsets_host", "qterms_host", "qroles_host", "min_should_host", "B"]
    from semantic_query_engine_amd import engine as E
    from semantic_query_engine_amd import retrieval as RT
    roles = re.search(r"enum\s*\{\s*SQE_LEX_SHOULD = 0, SQE_LEX_MUST = 1, SQE_LEX_FILTER = 2, SQE_LEX_MUST_NOT = 3\s*\}", text)
    assert roles and (E.LEX_SHOULD, E.LEX_MUST, E.LEX_FILTER, E.LEX_MUST_NOT) == (0, 1, 2, 3) == (SHOULD, MUST, FILTER, MUST_NOT)
    assert (RT.LEX_SHOULD, RT.LEX_MUST, RT.LEX_FILTER, RT.LEX_MUST_NOT) == (0, 1, 2, 3)
    for method in ("search_bool", "match", "count"):
        assert callable(getattr(E.LexicalIndex, method))


# ------------------------------------------------------------------------------ the shim's parsing (stand-ins, no GPU)
class FakeBoolLex(FakeLex):
    def search_bool(self, queries, roles, k, min_should=None):
        return self.ref.search(queries, roles, k, min_should)[:2]


class ShimVectors:
    def __init__(self, dim, n):
        self.dim, self.n, self.x = dim, n, np.random.default_rng(4).standard_normal((n, dim)).astype(np.float32)

    def __len__(self):
        return self.n

    def ids(self):
        return np.arange(self.n, dtype=np.int64)

    def get_rows(self, rows):
        return self.x[np.asarray(rows, dtype=np.int64)]

    def search(self, q, k, nprobe=0, filter_ids=None):
        rows = np.arange(self.n) if filter_ids is None else np.asarray(filter_ids, np.int64)
        cos = np.full((len(q), k), -np.inf, np.float32)
        ids = np.full((len(q), k), -1, np.int64)
        take = rows[:k]                                           # any fixed order will do: the test reads which rows were allowed
        cos[:, :take.size], ids[:, :take.size] = 0.5, take
        return cos, ids


@pytest.fixture()
def app(analyzer, monkeypatch):
    from fastapi.testclient import TestClient

    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim
    texts = WORDS + ["aspirin and the gene", "pain"]

    class Client:
        dim = 8

        def __init__(self):
            self.named = FakeNamed(texts, ["d0", "d1", "d0", "d1", "d2", "d2"])
            self.named.vectors = ShimVectors(8, len(texts))

        def index(self, name):
            return self.named

        def exists(self, name):
            return name == "docs"

        def count(self, index):
            return {"count": len(texts)}

    lex = FakeBoolLex(analyzer.n_terms, analyzer.analyze(texts))
    monkeypatch.setattr(shim, "push_text", lambda named: lex)
    monkeypatch.setattr(RT, "push_text", lambda named: lex)
    with TestClient(shim.create_app(Client(), None, 8)) as http:
        yield http, lex


def test_shim_bool_search_count_and_knn_filter(app):
    http, lex = app
    both = m("aspirin fever", operator="and")
    r = http.post("/docs/_search", json={"size": 5, "query": {"bool": {"must": [both]}}})
    assert r.status_code == 200, r.text
    assert [h["_id"] for h in r.json()["hits"]["hits"]] == ["d1_3", "d0_0"] and lex.calls == []      # search_bool, not match
    clause = {"bool": {"filter": [m("aspirin")], "should": [m("gene")], "must_not": [m("fever")]}}
    hits = http.post("/docs/_search", json={"query": clause}).json()["hits"]["hits"]
    assert [h["_id"] for h in hits] == ["d2_4"] and hits[0]["_score"] > 0
    hits = http.post("/docs/_search", json={"query": {"bool": {"filter": [m("aspirin")]}}}).json()["hits"]["hits"]
    assert [(h["_id"], h["_score"]) for h in hits] == [("d0_0", 0.0), ("d1_3", 0.0), ("d2_4", 0.0)]
    assert http.post("/docs/_count", json={"query": both}).json()["count"] == 2
    assert http.post("/docs/_count", json={"query": m("aspirin")}).json()["count"] == 3
    assert http.post("/docs/_count", json={"query": clause}).json()["count"] == 1
    assert http.get("/docs/_count").json()["count"] == 6 and http.post("/docs/_count", json={}).json()["count"] == 6
    knn = {"size": 6, "query": {"knn": {"embedding": {"vector": [0.0] * 7 + [1.0], "k": 6, "filter": both}}}}
    assert sorted(h["_id"] for h in http.post("/docs/_search", json=knn).json()["hits"]["hits"]) == ["d0_0", "d1_3"]
    knn["query"]["knn"]["embedding"]["filter"] = {"bool": {"filter": [m("aspirin"), {"term": {"doc_id": "d2"}}]}}
    assert [h["_id"] for h in http.post("/docs/_search", json=knn).json()["hits"]["hits"]] == ["d2_4"]
    for query in ({"bool": {"must": [m("aspirin fever"), m("pain")]}}, {"bool": {"must_not": [m("pain")]}}, {"bool": {"must": [m("a", fuzziness=1)]}},
                  {"bool": {"must": [m("aspirin")]}, "match": {"text": "x"}}):
        assert http.post("/docs/_search", json={"query": query}).status_code == 400, query
    assert http.post("/docs/_search", json={"size": 0, "query": {"bool": {"must": [both]}}}).status_code == 400
    assert http.post("/docs/_count", json={"query": {"bool": {"must_not": [m("pain")]}}}).status_code == 400
    assert http.post("/docs/_search", json={"query": {"match": {"text": {"query": "aspirin", "operator": "and"}}}}).status_code == 400
    knn["query"]["knn"]["embedding"]["filter"] = m("aspirin", fuzziness=1)
    assert http.post("/docs/_search", json=knn).status_code == 400
