"""The CPU side of the phrase queries: the NumPy reference (tests/lexphrase_reference.py) against cases worked out by hand, the
translator from OpenSearch clauses to (clauses, roles, min_should) (``retrieval.text_clauses``), the unchanged ``text_query``
and the refusal that stays without ``positions``, the filter and shim routes against a fake lexical object, the ctypes table
against the header, and the new host-only code of csrc/lexbag.cpp under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import lexbool_reference as BR
from tests import lexphrase_reference as PR
from tests.lexbool_reference import FILTER, MUST, MUST_NOT, SHOULD
from tests.test_lexbool_cpu import WORDS, FakeNamed, ShimVectors, m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_query_engine_amd", "csrc")


# ------------------------------------------------------------------------------ the reference, by hand
DOCS = {10: [0, 0, 1], 11: [1, 2], 12: [0, 2, 2, 2, 3], 13: [], 14: [1], 15: [0, 1]}      # 15 is put as a bag; term 4 is nowhere


@pytest.fixture(scope="module")
def hand():
    ids = [12, 10, 15, 14, 11, 13]
    return PR.LexPhraseRef(ids, [DOCS[i] for i in ids], [i != 15 for i in ids], 5)


def impact_by_hand(clause, pf, dl):
    """I(c, d) in plain Python floats from the definition: N = 6, the df of the corpus above, avgdl = 13 / 6."""
    df = {0: 3, 1: 4, 2: 2, 3: 1}
    idf = 0.0
    for t in clause:
        idf = idf + math.log(1.0 + ((6 - df[t]) + 0.5) / (df[t] + 0.5))
    norm = 1.2 * ((1.0 - 0.75) + 0.75 * (dl / (13.0 / 6.0)))
    return max(1, round(idf * (pf / (pf + norm)) * 65536.0))      # round(): half to even, as rint


def ask(ref, clauses, roles, ms=0, k=6):
    score, ids, sint = ref.search([clauses], [roles], k, [ms])
    n = int((ids[0] >= 0).sum())
    counts, mids, _ = ref.match([clauses], [roles], [ms])
    assert counts[0] == n and np.all(np.isneginf(score[0, n:])) and np.all(ids[0, n:] == -1)
    assert [float(s) for s in score[0, :n]] == [float(np.float32(int(v) / 65536)) for v in sint[0, :n]]
    return list(zip(ids[0, :n].tolist(), sint[0, :n].tolist())), mids[0].tolist()


def by_id(ref, v):
    return {int(i): int(x) for i, x in zip(ref.ref.ids, v)}


def test_phrase_frequency_by_hand(hand):
    assert by_id(hand, hand.pf([0, 0])) == {10: 1, 11: 0, 12: 0, 13: 0, 14: 0, 15: 0}
    assert by_id(hand, hand.pf([2, 2])) == {10: 0, 11: 0, 12: 2, 13: 0, 14: 0, 15: 0}        # overlap: `2 2` in `2 2 2`
    assert by_id(hand, hand.pf([2, 2, 2]))[12] == 1 and hand.pf([2, 2, 2, 2]).sum() == 0
    assert by_id(hand, hand.pf([0, 1])) == {10: 1, 11: 0, 12: 0, 13: 0, 14: 0, 15: 0}        # 15 holds 0 and 1, as a bag
    assert by_id(hand, hand.pf([1, 2])) == {10: 0, 11: 1, 12: 0, 13: 0, 14: 0, 15: 0}
    # longer than the document: rows are in id order, so 10's `0 0 1` is followed by 11's `1 2` -- `1 1` and `0 1 1` hold nowhere
    assert hand.pf([1, 1]).sum() == 0 and hand.pf([0, 1, 1]).sum() == 0 and hand.pf([0, 0, 1, 1]).sum() == 0
    assert hand.pf([1, 2, 0]).sum() == 0 and hand.pf([0, 2, 2, 2, 3, 1]).sum() == 0
    assert by_id(hand, hand.pf([0, 2, 2, 2, 3]))[12] == 1                                    # L = dl
    assert hand.pf([0, 4]).sum() == 0                                                        # a term of df = 0
    assert by_id(hand, hand.pf([1])) == {10: 1, 11: 1, 12: 0, 13: 0, 14: 1, 15: 1}           # L = 1: tf, bags included
    rng = np.random.default_rng(0)
    for _ in range(200):                                                                     # the window walk, position by position
        c = [int(t) for t in rng.integers(0, 4, int(rng.integers(2, 5)))]
        assert hand.pf(c).tolist() == [PR.pf_one(s, c) for s in hand.seqs], c


def test_phrase_scores_and_roles_by_hand(hand):
    assert hand.ref.avgdl == 13.0 / 6.0 and hand.ref.df.tolist() == [3, 4, 2, 1, 0]
    i01, i22 = impact_by_hand([0, 1], 1, 3), impact_by_hand([2, 2], 2, 5)
    assert ask(hand, [[0, 1]], [MUST]) == ([(10, i01)], [10])
    assert ask(hand, [[0, 1]], [SHOULD]) == ask(hand, [[0, 1]], [MUST])
    assert ask(hand, [[2, 2]], [MUST]) == ([(12, i22)], [12]) and i22 != impact_by_hand([2, 2], 1, 5)
    assert ask(hand, [[0, 1]], [FILTER]) == ([(10, 0)], [10])                                # a FILTER phrase scores 0
    # the terms hold in the bag, the phrase does not
    assert ask(hand, [[0], [1], [0, 1]], [FILTER, FILTER, MUST_NOT]) == ([(15, 0)], [15])
    hits, ids = ask(hand, [[0, 1], [1]], [SHOULD, SHOULD])
    assert ids == [10, 11, 14, 15] and hits[0] == (10, i01 + int(hand.ref.impact[0, 1]))     # row 0 is id 10
    # MUST phrase with SHOULD terms; min_should over two phrases and a term
    assert ask(hand, [[2, 2], [3], [1]], [MUST, SHOULD, SHOULD])[1] == [12]
    assert ask(hand, [[0, 0], [0, 1], [2]], [SHOULD] * 3, 2)[1] == [10] and ask(hand, [[0, 0], [0, 1], [2]], [SHOULD] * 3, 3)[1] == []
    assert ask(hand, [[0, 0], [1, 2], [2]], [SHOULD] * 3, 2)[1] == [11]
    assert ask(hand, [[0, 1], [0, 1]], [SHOULD, SHOULD], 2) == ([(10, 2 * i01)], [10])       # a repeated clause counts each time
    assert ask(hand, [[0, 1]], [MUST_NOT]) == ([], []) and ask(hand, [], []) == ([], [])
    assert ask(hand, [[0, 4], [1]], [MUST, SHOULD]) == ([], [])


def test_clauses_of_one_term_are_the_boolean_reference(hand):
    plain = BR.LexBoolRef(hand.ref)
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(0, 5))
        q = [int(t) for t in rng.integers(0, 5, n)]
        r = [int(x) for x in rng.integers(0, 4, n)]
        ms = int(rng.integers(0, 3))
        a, b = hand.search([[[t] for t in q]], [r], 6, [ms]), plain.search([q], [r], 6, [ms])
        assert all(np.array_equal(u, w) for u, w in zip(a, b))
        assert np.array_equal(hand.match([[[t] for t in q]], [r], [ms])[1], plain.match([q], [r], [ms])[1])


# ------------------------------------------------------------------------------ the translator
@pytest.fixture()
def analyzer():
    from oracle import wordpiece as WP
    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    toks = WP.synthetic_vocab(WORDS, size=400)
    tok = WordPieceTokenizer(vocab_text="\n".join(toks) + "\n")
    RT.configure_analyzer(tok, max_len=128, positions=True)
    yield RT._analyzer
    RT.configure_analyzer(None)


def ph(text, **opts):
    return {"match_phrase": {"text": dict(query=text, **opts) if opts else text}}


def test_text_clauses_accepts(analyzer):
    from semantic_query_engine_amd import retrieval as RT

    def t(text):
        terms = analyzer.query(text).tolist()
        assert len(terms) == len(text.split())
        return terms

    def tc(clause):
        clauses, roles, ms = RT.text_clauses(clause)
        assert roles.dtype == np.uint8 and all(isinstance(c, list) for c in clauses)
        return clauses, roles.tolist(), ms

    a, f, p, g = t("aspirin")[0], t("fever")[0], t("pain")[0], t("gene")[0]
    assert tc(ph("aspirin fever")) == ([[a, f]], [MUST], 0)
    assert tc(ph("aspirin fever", slop=0)) == ([[a, f]], [MUST], 0)
    assert tc({"match_phrase": {"text": {"query": "fever aspirin aspirin"}}}) == ([[f, a, a]], [MUST], 0)
    assert tc(ph("aspirin")) == ([[a]], [MUST], 0) and tc(ph("")) == ([], [], 0)
    assert tc({"bool": {"must": [ph("aspirin fever")]}}) == ([[a, f]], [MUST], 0)
    bool_ = {"bool": {"must": [m("gene"), ph("fever pain")], "should": [ph("aspirin aspirin"), m("pain gene")], "filter": ph("pain in"),
                      "must_not": [ph("gene and"), m("aspirin fever")]}}
    i, an = t("in")[0], t("and")[0]
    assert tc(bool_) == ([[g], [f, p], [p, i], [a, a], [p], [g], [g, an], [a], [f]],
                         [MUST, MUST, FILTER, SHOULD, SHOULD, SHOULD, MUST_NOT, MUST_NOT, MUST_NOT], 0)
    # minimum_should_match counts members: phrases are one clause each
    assert tc({"bool": {"should": [ph("aspirin fever"), ph("fever pain"), m("gene")], "minimum_should_match": 2}}) == \
        ([[a, f], [f, p], [g]], [SHOULD] * 3, 2)
    assert tc({"bool": {"should": [ph("aspirin fever"), ph("fever pain"), m("gene")], "minimum_should_match": "67%"}})[2] == 2
    assert tc({"bool": {"must_not": [ph("aspirin fever")], "filter": [m("pain")]}}) == ([[p], [a, f]], [FILTER, MUST_NOT], 0)
    # everything text_query serves, every occurrence a clause of its own
    for clause in (m("aspirin fever"), m("aspirin fever pain", minimum_should_match=2), m("aspirin fever", operator="and"), m(""),
                   {"bool": {"must": [m("aspirin")], "should": [m("gene"), m("pain aspirin")], "must_not": [m("gene pain")]}}):
        terms, roles, ms = RT.text_query(clause)
        assert tc(clause) == ([[int(x)] for x in terms], roles.tolist(), ms)


@pytest.mark.parametrize("clause", [
    ph("aspirin fever", slop=1), ph("aspirin fever", slop="0"), ph("aspirin fever", slop=True), ph("aspirin fever", analyzer="standard"),
    {"match_phrase": {"title": "aspirin fever"}}, {"match_phrase": {"text": "a", "title": "b"}}, {"match_phrase": {"text": 5}},
    {"match_phrase": "aspirin fever"}, {"match_phrase": {"text": {"slop": 0}}}, ph(" ".join(["aspirin"] * 65)),
    {"bool": {"must": [ph("aspirin fever"), m("pain gene")]}},                      # must of a multi-term OR match, as before
    {"bool": {"should": [ph("aspirin fever"), m("pain gene")], "minimum_should_match": 2}},      # a wide match member still is not a clause
    {"bool": {"must_not": [ph("aspirin fever")]}},                                  # no positive clause
    {"bool": {"must": [{"bool": {"must": [ph("aspirin fever")]}}, m("pain")]}},     # nested
    {"bool": {"must": [{"bool": {"must": [ph("aspirin fever")]}}]}},                # ... also as the only member
    {"bool": {"must": [ph(" ".join(["aspirin"] * 40))], "should": [ph(" ".join(["fever"] * 30))]}},      # 70 occurrences
    {"bool": {"must": [ph("aspirin fever")], "boost": 2}}, {"match_phrase_prefix": {"text": "aspirin fev"}},
    {"span_near": {"clauses": [ph("a b")]}}])
def test_text_clauses_refuses(analyzer, clause):
    from semantic_query_engine_amd import retrieval as RT
    with pytest.raises(ValueError):
        RT.text_clauses(clause)


def test_text_query_is_unchanged(analyzer):
    """With positions on, ``text_query`` still refuses phrases and still answers what it answered."""
    from semantic_query_engine_amd import retrieval as RT
    for clause in (ph("aspirin fever"), {"bool": {"must": [ph("aspirin fever")]}}, {"bool": {"filter": [m("pain"), ph("aspirin fever")]}}):
        with pytest.raises(ValueError):
            RT.text_query(clause)
    a, f = analyzer.query("aspirin fever").tolist()
    terms, roles, ms = RT.text_query(m("aspirin fever", operator="and"))
    assert terms.dtype == np.int32 and (terms.tolist(), roles.tolist(), ms) == ([a, f], [MUST, MUST], 0)
    import inspect
    assert list(inspect.signature(RT.text_query).parameters) == ["clause"]
    assert list(inspect.signature(RT.configure_analyzer).parameters) == ["tokenizer", "max_len", "positions"]
    assert inspect.signature(RT.configure_analyzer).parameters["positions"].default is False


# ------------------------------------------------------------------------------ routes, against a fake lexical object
class FakePhraseLex:
    """LexicalIndex stand-in over the dense reference; ``ordered`` says how ``push_text`` would have put the documents."""

    def __init__(self, n_terms, docs, ordered=True):
        self.ref = PR.LexPhraseRef(np.arange(len(docs)), docs, [ordered] * len(docs), n_terms)
        self.plain = BR.LexBoolRef(self.ref.ref)
        self.calls = []

    def match_phrase(self, queries, roles, min_should=None, cap=None):
        self.calls.append(("match_phrase", [[list(c) for c in q] for q in queries], [np.asarray(r).tolist() for r in roles], list(min_should), cap))
        return self.ref.match(queries, roles, min_should, cap)[:2]

    def count_phrase(self, queries, roles, min_should=None):
        return self.match_phrase(queries, roles, min_should, cap=0)[0]

    def search_phrase(self, queries, roles, k, min_should=None):
        self.calls.append(("search_phrase", len(queries)))
        return self.ref.search(queries, roles, k, min_should)[:2]

    def match(self, queries, roles, min_should=None, cap=None):
        self.calls.append(("match",))
        return self.plain.match(queries, roles, min_should, cap)[:2]

    def count(self, queries, roles, min_should=None):
        return self.match(queries, roles, min_should, cap=0)[0]

    def search_bool(self, queries, roles, k, min_should=None):
        self.calls.append(("search_bool",))
        return self.plain.search(queries, roles, k, min_should)[:2]


TEXTS = WORDS + ["aspirin and the gene", "pain", "pain fever"]       # row 3 is "fever pain aspirin aspirin", row 0 has "fever and pain"
DOC_IDS = ["d0", "d1", "d0", "d1", "d2", "d2", "d0"]


@pytest.fixture()
def named(analyzer, monkeypatch):
    from semantic_query_engine_amd import retrieval as RT
    idx = FakeNamed(TEXTS, DOC_IDS)
    idx.vectors = ShimVectors(8, len(TEXTS))                       # (search_text reads the hits' embeddings back)
    lex = FakePhraseLex(analyzer.n_terms, analyzer.analyze(TEXTS))
    monkeypatch.setattr(RT, "push_text", lambda named: lex)
    return idx, lex


def test_phrases_compose_with_the_other_filter_clauses(named):
    from semantic_query_engine_amd import retrieval as RT
    idx, lex = named

    def rows(clause):
        out = RT.filter_rows(idx, clause)
        assert out.dtype == np.int64
        return out.tolist()

    assert rows(ph("fever pain")) == [3] and lex.calls[-1][0] == "match_phrase" and lex.calls[-1][2:] == ([[MUST]], [0], None)
    assert rows(ph("pain fever")) == [6] and rows(ph("aspirin aspirin")) == [3] and rows(ph("pain aspirin")) == [3]
    assert rows(m("fever pain", operator="and")) == [0, 3, 6] and lex.calls[-1] == ("match",)          # no phrase: the old route
    assert rows({"bool": {"filter": [{"terms": {"doc_id": ["d0", "d2"]}}, ph("and the")]}}) == [4]
    assert rows({"bool": {"filter": [m("pain")], "must_not": [ph("fever pain")]}}) == [0, 5, 6]
    assert rows({"bool": {"must_not": ph("and the")}}) == [0, 1, 2, 3, 5, 6]                           # row 1 has `and breast`
    assert RT.exclusion_rows(idx, {"bool": {"must_not": [ph("and the"), {"term": {"doc_id": "d1"}}]}}).tolist() == [1, 3, 4]
    assert rows({"bool": {"should": [ph("fever pain"), ph("pain fever"), m("gene")], "minimum_should_match": 1}}) == [1, 3, 4, 6]
    lists, loq = RT.resolve_each(idx, [ph("and the"), None, m("gene"), ph("and the")])
    assert [x.tolist() for x in lists] == [[4], [1, 4]] and loq.tolist() == [0, -1, 1, 0]
    for bad in (ph("fever pain", slop=2), {"bool": {"filter": [{"match_phrase": {"title": "x y"}}]}}):
        with pytest.raises(ValueError):
            RT.filter_rows(idx, bad)


def test_indexer_count_text_and_search_text_with_phrases(named):
    from semantic_query_engine_amd import retrieval as RT
    idx, lex = named

    class Client:
        def index(self, name):
            return idx

    ix = RT.OpenSearchIndexer(Client(), "docs")
    assert ix.count_text(ph("and the")) == 1 and ix.count_text({"bool": {"must": [m("pain")], "must_not": [ph("fever pain")]}}) == 3
    assert ix.count_text("aspirin") == 3 and lex.calls[-1] == ("match",)
    hits = ix.search_text({"bool": {"must": [ph("fever pain")], "should": [m("aspirin")]}}, 5)
    assert [h["text"] for h, _ in hits] == [TEXTS[3]] and hits[0][1] > 0 and lex.calls[-1] == ("search_phrase", 1)
    assert [h["text"] for h, _ in ix.search_text(ph("pain fever"), 5)] == [TEXTS[6]]
    with pytest.raises(ValueError):
        ix.count_text({"bool": {"must_not": [ph("fever pain")]}})


def test_without_positions_the_refusal_stays(monkeypatch):
    """configure_analyzer(..., positions=False), the default: documents go up as bags and match_phrase is refused everywhere."""
    from oracle import wordpiece as WP
    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    tok = WordPieceTokenizer(vocab_text="\n".join(WP.synthetic_vocab(WORDS, size=400)) + "\n")
    for kw in ({}, {"positions": False}):
        RT.configure_analyzer(tok, max_len=64, **kw)
        try:
            assert RT._analyzer.positions is False
            for clause in (ph("aspirin fever"), {"bool": {"must": [ph("aspirin fever")]}}):
                with pytest.raises(ValueError):
                    RT.text_clauses(clause)
                with pytest.raises(ValueError):
                    RT.text_query(clause)
                with pytest.raises(ValueError):
                    RT.filter_rows(FakeNamed(TEXTS, DOC_IDS), clause)
            assert RT.text_clauses(m("aspirin"))[0] == [[int(RT._analyzer.query("aspirin")[0])]]      # the rest is served
        finally:
            RT.configure_analyzer(None)


def test_push_text_sends_sequences_only_with_positions(monkeypatch):
    from oracle import wordpiece as WP
    from semantic_query_engine_amd import engine as E
    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    tok = WordPieceTokenizer(vocab_text="\n".join(WP.synthetic_vocab(WORDS, size=400)) + "\n")
    puts = []

    class Lex:
        def __init__(self, ctx, n_terms):
            pass

        def put(self, ids, bags, **kw):
            puts.append((np.asarray(ids).tolist(), [np.asarray(b).tolist() for b in bags], kw))

        def delete(self, ids):
            pass

    monkeypatch.setattr(E, "LexicalIndex", Lex)
    for positions, want in ((False, {}), (True, {"ordered": True})):
        RT.configure_analyzer(tok, max_len=64, positions=positions)
        try:
            idx = FakeNamed(TEXTS, DOC_IDS)
            idx.vectors.ctx = None
            RT.push_text(idx)
            assert puts[-1][0] == list(range(len(TEXTS))) and puts[-1][2] == want
            assert puts[-1][1] == [b.tolist() for b in RT._analyzer.analyze(TEXTS)]             # in order: the sequence
        finally:
            RT.configure_analyzer(None)


# ------------------------------------------------------------------------------ the shim's parsing (stand-ins, no GPU)
@pytest.fixture()
def app(analyzer, monkeypatch):
    from fastapi.testclient import TestClient

    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim

    class Client:
        dim = 8

        def __init__(self):
            self.named = FakeNamed(TEXTS, DOC_IDS)
            self.named.vectors = ShimVectors(8, len(TEXTS))

        def index(self, name):
            return self.named

        def exists(self, name):
            return name == "docs"

        def count(self, index):
            return {"count": len(TEXTS)}

    lex = FakePhraseLex(analyzer.n_terms, analyzer.analyze(TEXTS))
    monkeypatch.setattr(shim, "push_text", lambda named: lex)
    monkeypatch.setattr(RT, "push_text", lambda named: lex)
    with TestClient(shim.create_app(Client(), None, 8)) as http:
        yield http, lex


def test_shim_phrase_search_count_and_knn_filter(app):
    http, lex = app
    r = http.post("/docs/_search", json={"size": 5, "query": ph("and the")})
    assert r.status_code == 200, r.text
    hits = r.json()["hits"]["hits"]
    assert [h["_id"] for h in hits] == ["d2_4"] and hits[0]["_score"] > 0 and lex.calls[-1] == ("search_phrase", 1)
    clause = {"bool": {"must": [ph("fever pain")], "should": [m("aspirin")], "must_not": [m("gene")]}}
    hits = http.post("/docs/_search", json={"query": clause}).json()["hits"]["hits"]
    assert [h["_id"] for h in hits] == ["d1_3"]
    hits = http.post("/docs/_search", json={"query": {"bool": {"filter": [ph("pain fever")]}}}).json()["hits"]["hits"]
    assert [(h["_id"], h["_score"]) for h in hits] == [("d0_6", 0.0)]
    assert http.post("/docs/_count", json={"query": ph("and the")}).json()["count"] == 1
    assert http.post("/docs/_count", json={"query": clause}).json()["count"] == 1
    assert http.post("/docs/_count", json={"query": m("aspirin")}).json()["count"] == 3 and lex.calls[-1] == ("match",)
    knn = {"size": 7, "query": {"knn": {"embedding": {"vector": [0.0] * 7 + [1.0], "k": 7, "filter": ph("and the")}}}}
    assert [h["_id"] for h in http.post("/docs/_search", json=knn).json()["hits"]["hits"]] == ["d2_4"]
    knn["query"]["knn"]["embedding"]["filter"] = ph("pain")
    assert sorted(h["_id"] for h in http.post("/docs/_search", json=knn).json()["hits"]["hits"]) == ["d0_0", "d0_6", "d1_3", "d2_5"]
    knn["query"]["knn"]["embedding"]["filter"] = {"bool": {"filter": [ph("and the"), {"term": {"doc_id": "d2"}}]}}
    assert [h["_id"] for h in http.post("/docs/_search", json=knn).json()["hits"]["hits"]] == ["d2_4"]
    for query in (ph("and the", slop=1), {"bool": {"must_not": [ph("and the")]}}, {"match_phrase": {"title": "and the"}},
                  {"bool": {"must": [ph("and the")]}, "match_phrase": {"text": "x"}}):
        assert http.post("/docs/_search", json={"query": query}).status_code == 400, query
    assert http.post("/docs/_count", json={"query": ph("and the", slop=1)}).status_code == 400
    assert http.post("/docs/_search", json={"size": 0, "query": ph("and the")}).status_code == 400
    knn["query"]["knn"]["embedding"]["filter"] = ph("and the", analyzer="x")
    assert http.post("/docs/_search", json=knn).status_code == 400


# ------------------------------------------------------------------------------ the ctypes table
def test_native_table_carries_the_headers_signatures():
    import ctypes as C

    from semantic_query_engine_amd import _native as N
    from semantic_query_engine_amd import engine as E
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sqe.h")).read(), flags=re.S)
    for name in ("sqe_lex_put_ordered", "sqe_lex_search_phrase", "sqe_lex_search_phrase_device", "sqe_lex_match_phrase",
                 "sqe_lex_match_phrase_device"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert decl, name
        params = [p.strip() for p in decl.group(1).split(",")]
        want = [C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int for p in params]
        res, args = N.SIGNATURES[name]
        assert res is C.c_int and args == want, (name, params)
    assert [p.split()[-1] for p in params[:7]] == ["lex", "qoffsets_host", "coffsets_host", "qterms_host", "croles_host", "min_should_host", "B"]
    assert N.SIGNATURES["sqe_lex_put_ordered"] == N.SIGNATURES["sqe_lex_put"]
    assert re.search(r"SQE_LEX_SEQ_OFF = 6,\s*SQE_LEX_SEQ = 7", text) and (E.LEX_SEQ_OFF, E.LEX_SEQ) == (6, 7)
    for method in ("search_phrase", "match_phrase", "count_phrase", "search_phrase_device", "match_phrase_device"):
        assert callable(getattr(E.LexicalIndex, method))
    import inspect
    assert inspect.signature(E.LexicalIndex.put).parameters["ordered"].default is False


# ------------------------------------------------------------------------------ lexbag.cpp's sequence code under the sanitizers
def _query_case(n_terms, qoff, coff, terms):
    qoff, coff, terms = np.asarray(qoff, np.int64), np.asarray(coff, np.int64), np.asarray(terms, np.int32)
    return struct.pack("<iiq", 0, n_terms, qoff.shape[0] - 1) + qoff.tobytes() + struct.pack("<q", coff.shape[0]) + coff.tobytes() + \
        struct.pack("<q", terms.shape[0]) + terms.tobytes()


def _doc_case(n_terms, terms):
    terms = np.asarray(terms, np.int32)
    return struct.pack("<iiq", 1, n_terms, terms.shape[0]) + terms.tobytes()


def test_lexseq_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "lexseq_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build_san", "lexseq_asan")
    rng = np.random.default_rng(6)
    good, bad = [], []
    for B in (0, 1, 7, 200):                                      # random well-formed batches
        nc = rng.integers(0, 5, B)
        qoff = np.concatenate([[0], np.cumsum(nc)])
        lens = rng.integers(1, 9, int(qoff[-1]))
        coff = np.concatenate([[0], np.cumsum(lens)])
        good.append((97, qoff, coff, rng.integers(0, 97, int(coff[-1]))))
    good.append((131072, [0, 2, 3], [0, 32, 64, 128], [131071] * 128))                    # 64 occurrences per query: the limit itself
    good.append((5, [0, 64], list(range(65)), [4] * 64))                                  # 64 clauses of one term
    bad += [(97, [1, 2], [0, 1, 2], [0, 0]),                                              # clause ranges do not start at 0
            (97, [0, 2, 1], [0, 1, 2], [0, 0]),                                           # ... decrease
            (97, [0, -1], [0], []),                                                       # ... below zero
            (97, [0, 2 ** 62, 2 ** 61], [0], []),                                         # huge, then decreasing: coffsets never read
            (97, [0, 2], [1, 2, 3], [0, 0, 0]),                                           # occurrence ranges do not start at 0
            (97, [0, 2], [0, 2, 1], [0, 0]),                                              # ... decrease
            (97, [0, 2], [0, 1, 1], [0]),                                                 # an empty clause
            (97, [0, 1], [0, 0], []),                                                     # ... the only one
            (97, [0, 2], [0, 2 ** 62, 2 ** 61], []),                                      # huge, then decreasing: terms never read
            (97, [0, 2], [0, 33, 65], [1] * 65),                                          # 65 occurrences in a query
            (97, [0, 1, 3], [0, 1, 40, 66], [1] * 66),                                    # ... in the second one
            (97, [0, 1], [0, 2], [3, 97]), (97, [0, 1], [0, 2], [-1, 3]),                 # terms out of range
            (1, [0, 1], [0, 1], [1])]
    docs = [[], [5], [3, 3, 3], rng.integers(0, 97, 300).tolist(), [2] * 70000 + [0], [], [96, 0, 96]]
    blob = b"".join(_query_case(*c) for c in good + bad) + b"".join(_doc_case(97, d) for d in docs)
    cases, out = tmp_path / "cases.bin", tmp_path / "out.bin"
    cases.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(cases), str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip() == f"ok {len(good) + len(bad) + len(docs)} cases"
    data = out.read_bytes()
    n = len(good) + len(bad)
    assert list(struct.unpack(f"<{n}i", data[:4 * n])) == [0] * len(good) + [1] * len(bad)
    pos, log = 4 * n, []
    for d in docs:
        at, dl, distinct = struct.unpack_from("<qqi", data, pos)
        pos += 20
        terms = np.frombuffer(data, np.int32, distinct, pos)
        tf = np.frombuffer(data, np.int32, distinct, pos + 4 * distinct)
        pos += 8 * distinct
        (log_len,) = struct.unpack_from("<q", data, pos)
        got_log = np.frombuffer(data, np.int32, log_len, pos + 8)
        pos += 8 + 4 * log_len
        u, c = np.unique(np.asarray(d, np.int32), return_counts=True)
        assert at == len(log) and dl == len(d) and np.array_equal(terms, u) and np.array_equal(tf, np.minimum(c, 65535))
        log += d
        assert np.array_equal(got_log, np.asarray(log, np.int32))
    assert pos == len(data)
