"""The CPU side of the lexical index: the NumPy reference of the integer BM25 (tests/lex_reference.py) against a corpus worked
out by hand and against a plain float64 BM25, the analyzer, the shim's parsing of ``match`` and of ``hybrid`` with a ``match``
(served by stand-ins backed by the reference, as tests/test_shim_cpu.py does), and the host-only bag code (csrc/lexbag.cpp)
under AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU."""
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

from oracle import retrieval as R
from oracle import wordpiece as WP
from tests import lex_reference as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_query_engine_amd", "csrc")


# ------------------------------------------------------------------------------ the reference
def test_reference_on_a_hand_computed_corpus():
    """Five documents, k1 = 1.2, b = 0.75.  N = 5, L = 11, avgdl = 2.2; df = (2, 3, 2, 1);
    idf(0) = idf(2) = ln(1 + 3.5 / 2.5) = ln 2.4 = 0.875469, idf(1) = ln(1 + 2.5 / 3.5) = 0.538997, idf(3) = ln(1 + 4.5 / 1.5)
    = ln 4 = 1.386294.  norm = 1.2 (0.25 + 0.75 dl / 2.2): 1.527273 (dl 3), 1.118182 (dl 2), 2.345455 (dl 5), 0.709091 (dl 1).
    I = rint(65536 idf tf / (tf + norm)), e.g. document 10, term 0: 65536 x 0.875469 x 2 / 3.527273 = 32532.06."""
    ids = [12, 10, 14, 11, 13]                                    # out of order: rows are the ids ascending
    bags = {10: [0, 0, 1], 11: [1, 2], 12: [0, 2, 2, 2, 3], 13: [], 14: [1]}
    ref = LR.LexRef(ids, [bags[i] for i in ids], 5)
    assert ref.ids.tolist() == [10, 11, 12, 13, 14] and ref.dl.tolist() == [3, 2, 5, 0, 1]
    assert ref.df.tolist() == [2, 3, 2, 1, 0] and float(ref.avgdl) == 2.2
    want = np.zeros((5, 5), np.uint64)
    want[0, [0, 1]] = [32532, 13977]
    want[1, [1, 2]] = [16676, 27087]
    want[2, [0, 2, 3]] = [17150, 32200, 27157]
    want[4, 1] = 20668
    assert np.array_equal(ref.impact, want)
    score, got, sint = ref.search([[0, 1], [1, 1], [4], [], [2, 3, 2]], 4)
    assert got.tolist() == [[10, 14, 12, 11], [14, 11, 10, -1], [-1] * 4, [-1] * 4, [12, 11, -1, -1]]
    assert sint.tolist() == [[46509, 20668, 17150, 16676], [41336, 33352, 27954, 0], [0] * 4, [0] * 4, [91557, 54174, 0, 0]]
    assert score[0, 0] == np.float32(46509 / 65536) and np.isneginf(score[1, 3]) and np.isneginf(score[2]).all()


def test_reference_ties_go_to_the_lowest_id():
    ref = LR.LexRef([9, 3, 6], [[1, 2], [1, 2], [1, 2]], 4)
    assert ref.search([[1]], 3)[1].tolist() == [[3, 6, 9]]


def test_tf_cap_and_dl():
    ref = LR.LexRef([0, 1], [[2] * 70000, [2]], 3)
    assert ref.tf[0, 2] == 65535 and ref.dl[0] == 70000


def test_reference_ranking_against_plain_float64_bm25():
    """The integer score is the float64 BM25 with every term rounded to 2^-16 (or raised to it): over a query of at most 64
    occurrences the two differ by at most 64 x 2^-16, so the integer ranking is the float ranking up to ties that close."""
    rng = np.random.default_rng(5)
    p = 1.0 / np.arange(1, 61)
    p /= p.sum()
    bags = [rng.choice(60, int(rng.integers(0, 41)), p=p) for _ in range(700)]
    ref = LR.LexRef(np.arange(700) * 2 + 1, bags, 64)
    tol = 64 * 2.0 ** -16
    for q in ([0], [3, 3, 7], list(range(64)), [59, 58, 1], rng.integers(0, 60, 64).tolist()):
        f = ref.search_float(q)
        score, ids, sint = ref.search([q], 50)
        rows = np.searchsorted(ref.ids, ids[0][ids[0] >= 0])
        assert np.all(np.abs(sint[0][:rows.size].astype(np.float64) * 2.0 ** -16 - f[rows]) <= tol)
        assert np.all(f[rows][:-1] >= f[rows][1:] - tol)                        # float order, up to ties within tol
        rest = np.setdiff1d(np.nonzero(f > 0)[0], rows)
        if rows.size == 50 and rest.size:
            assert f[rest].max() <= f[rows].min() + tol                         # nothing better was left out


# ------------------------------------------------------------------------------ analyzer
WORDS = ["aspirin reduces fever and pain in adult patients", "the brca1 gene and breast cancer risk",
         "metformin is a first line treatment of type 2 diabetes", "fever pain aspirin aspirin"]


@pytest.fixture(scope="module")
def tokenizer():
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    toks = WP.synthetic_vocab(WORDS, size=400)
    tok = WordPieceTokenizer(vocab_text="\n".join(toks) + "\n")
    assert tok.vocab_size == len(toks)
    return tok, toks


def test_analyzer_round_trips(tokenizer):
    from semantic_query_engine_amd import retrieval as RT
    tok, toks = tokenizer
    an = RT.Analyzer(tok, max_len=64)
    assert an.n_terms == len(toks)
    special = {toks.index(t) for t in ("[CLS]", "[SEP]", "[PAD]")}
    for text, terms in zip(WORDS, an.analyze(WORDS)):
        full = tok.encode(text, 66)
        assert terms.tolist() == full[1:-1] and not special & set(terms.tolist())
        assert np.all((terms >= 0) & (terms < an.n_terms))
        back = " ".join(toks[t] for t in terms).replace(" ##", "")
        assert back == text                                                      # the word pieces spell the text
    assert an.analyze([""])[0].size == 0
    assert an.query(" ".join(["aspirin"] * 100)).size == RT.LEX_MAX_QUERY     # a query is cut to 64 occurrences
    # queries and documents go through one function: a document's own text scores it
    bags = an.analyze(WORDS)
    ref = LR.LexRef(np.arange(4), bags, an.n_terms)
    assert ref.search([an.query("aspirin fever")], 4)[1][0].tolist()[:2] == [3, 0]


def test_configure_analyzer(tokenizer):
    from semantic_query_engine_amd import retrieval as RT
    assert RT._analyzer is None
    RT.configure_analyzer(tokenizer[0], max_len=128)
    try:
        assert RT._analyzer.max_len == 128 and RT._analyzer.n_terms == tokenizer[0].vocab_size
    finally:
        RT.configure_analyzer(None)
    assert RT._analyzer is None
    with pytest.raises(RuntimeError):
        RT.push_text(object())


# ------------------------------------------------------------------------------ shim
DIM = 16


class RefLex:
    """LexicalIndex stand-in answered by the reference."""

    def __init__(self, n_terms):
        self.n_terms, self.docs = n_terms, {}

    def put(self, ids, bags):
        self.docs.update({int(i): np.asarray(b) for i, b in zip(ids, bags)})

    def search(self, queries, k):
        keys = sorted(self.docs)
        return LR.LexRef(keys, [self.docs[i] for i in keys], self.n_terms).search(queries, k)[:2]


class RefVectors:
    def __init__(self, dim):
        self.dim, self.xn, self.calls = dim, np.zeros((0, dim), np.float32), []

    def __len__(self):
        return self.xn.shape[0]

    def add(self, x):
        self.xn = np.concatenate([self.xn, R.normalize_rows(np.asarray(x, np.float32))], 0)

    def get_rows(self, rows):
        return self.xn[np.asarray(rows, dtype=np.int64)]

    def search(self, q, k, nprobe=0):
        cos, ids = R.exact_topk(self.xn, R.normalize_rows(np.asarray(q, np.float32)), k)
        return cos.astype(np.float32), ids

    def search_hybrid(self, lex, q, q_terms, k, offsets=None, weights=None, depth=0, rank_constant=60, nprobe=0):
        self.calls.append((len(q_terms), None if weights is None else np.asarray(weights).tolist(), depth, rank_constant))
        n = depth or min(256, max(32, 4 * k))
        cos, ids = self.search(q, n) if len(q) else (np.empty((0, n), np.float32), np.empty((0, n), np.int64))
        ls, li = lex.search(q_terms, n)
        return LR.hybrid(cos, ids, offsets, ls, li, k, weights, rank_constant)


class RefNamed:
    def __init__(self, dim):
        self.vectors, self.sources, self.row_of_id, self.lock = RefVectors(dim), [], {}, threading.Lock()


class RefClient:
    def __init__(self, dim):
        self.dim, self._ix = dim, {}

    def index(self, name):
        return self._ix.setdefault(name, RefNamed(self.dim))

    def exists(self, name):
        return name in self._ix

    def count(self, index):
        return {"count": len(self.index(index).vectors)}


@pytest.fixture()
def app(tokenizer, monkeypatch):
    from fastapi.testclient import TestClient

    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim
    RT.configure_analyzer(tokenizer[0], max_len=64)
    client = RefClient(DIM)
    idx = client.index("docs")
    rng = np.random.default_rng(2)
    x = rng.standard_normal((len(WORDS), DIM)).astype(np.float32)
    idx.vectors.add(x)
    lex = RefLex(RT._analyzer.n_terms)
    for row, text in enumerate(WORDS):
        idx.sources.append({"doc_id": f"d{row}", "text": text})
        idx.row_of_id[f"d{row}_0"] = row
    lex.put(range(len(WORDS)), RT._analyzer.analyze(WORDS))
    monkeypatch.setattr(shim, "push_text", lambda named: lex)
    with TestClient(shim.create_app(client, None, DIM)) as http:
        yield http, idx, x, lex
    RT.configure_analyzer(None)


def test_shim_match(app):
    from semantic_query_engine_amd import retrieval as RT
    http, idx, x, lex = app
    for body in ({"query": {"match": {"text": "aspirin fever"}}, "size": 3}, {"query": {"match": {"text": {"query": "aspirin fever"}}}, "size": 3}):
        r = http.post("/docs/_search", json=body)
        assert r.status_code == 200, r.text
        hits = r.json()["hits"]["hits"]
        score, ids = lex.search([RT._analyzer.query("aspirin fever")], 3)
        assert [h["_id"] for h in hits] == [f"d{i}_0" for i in ids[0] if i >= 0] == ["d3_0", "d0_0"]
        assert [h["_score"] for h in hits] == [float(s) for s in score[0][:2]]
        assert r.json()["hits"]["max_score"] == float(score[0][0]) and hits[0]["_source"]["text"] == WORDS[3]
    assert http.post("/docs/_search", json={"query": {"match": {"text": "zzzz"}}}).json()["hits"]["hits"] == []


@pytest.mark.parametrize("match", [{"text": {"query": "aspirin", "operator": "and"}}, {"text": {"query": "aspirin", "fuzziness": "AUTO"}},
                                   {"title": "aspirin"}, {"text": "a", "doc_id": "b"}, {"text": 5}, {"text": {"operator": "and"}}, "aspirin"])
def test_shim_match_refuses_what_it_does_not_serve(app, match):
    http = app[0]
    r = http.post("/docs/_search", json={"query": {"match": match}})
    assert r.status_code == 400 and r.json()["error"]["type"] == "parsing_exception"
    r = http.post("/docs/_search", json={"query": {"hybrid": {"queries": [{"knn": {"embedding": {"vector": [0.0] * DIM, "k": 2}}},
                                                                          {"match": match}]}}})
    assert r.status_code == 400 and r.json()["error"]["type"] == "parsing_exception"


def test_shim_match_size_and_analyzer(app):
    from semantic_query_engine_amd import retrieval as RT
    http = app[0]
    assert http.post("/docs/_search", json={"query": {"match": {"text": "aspirin"}}, "size": 0}).status_code == 400
    assert http.post("/docs/_search", json={"query": {"match": {"text": "aspirin"}}, "size": 257}).status_code == 400
    RT.configure_analyzer(None)                                   # no analyzer: the existing 400
    assert http.post("/docs/_search", json={"query": {"match": {"text": "aspirin"}}}).status_code == 400


def test_shim_hybrid_with_match(app):
    from semantic_query_engine_amd import retrieval as RT
    http, idx, x, lex = app
    knn = {"knn": {"embedding": {"vector": x[1].tolist(), "k": 3}}}
    match = {"match": {"text": "aspirin fever"}}
    body = {"size": 3, "query": {"hybrid": {"queries": [match, knn]}}, "ext": {"fusion": {"weights": [2.0, 0.5], "window": 4, "rank_constant": 7}}}
    r = http.post("/docs/_search", json=body)
    assert r.status_code == 200, r.text
    assert idx.vectors.calls[-1] == (1, [0.5, 2.0], 4, 7)        # weights in sub-query order: the match's goes last
    cos, ids = idx.vectors.search(x[1:2], 4)
    ls, li = lex.search([RT._analyzer.query("aspirin fever")], 4)
    fused, want, wcos, bm = LR.hybrid(cos, ids, [0, 1], ls, li, 3, [0.5, 2.0], 7)
    hits = r.json()["hits"]["hits"]
    assert [h["_id"] for h in hits] == [f"d{i}_0" for i in want[0]]
    for j, h in enumerate(hits):
        assert h["fields"]["_fused"] == [float(fused[0, j])]
        assert h["fields"].get("_bm25") == ([float(bm[0, j])] if np.isfinite(bm[0, j]) else None)
        assert h["_score"] == (float(1.0 / (2.0 - float(wcos[0, j]))) if np.isfinite(wcos[0, j]) else 0.0)
    assert any("_bm25" in h["fields"] for h in hits) and any("_bm25" not in h["fields"] for h in hits)
    # a match alone among the sub-queries, and what is refused
    r = http.post("/docs/_search", json={"size": 2, "query": {"hybrid": {"queries": [match]}}})
    assert r.status_code == 200 and [h["_id"] for h in r.json()["hits"]["hits"]] == ["d3_0", "d0_0"]
    assert http.post("/docs/_search", json={"query": {"hybrid": {"queries": [match, knn, match]}}}).status_code == 400
    assert http.post("/docs/_search", json={"query": {"hybrid": {"queries": [match, knn]}}, "ext": {"fusion": {"method": "max"}}}).status_code == 400
    assert http.post("/docs/_search", json={"query": {"hybrid": {"queries": [match] + [knn] * 32}}}).status_code == 400


# ------------------------------------------------------------------------------ lexbag.cpp under the sanitizers
def _case(n_terms, max_len, offsets, ids, terms):
    offsets, ids, terms = np.asarray(offsets, np.int64), np.asarray(ids, np.int64), np.asarray(terms, np.int32)
    assert offsets.shape[0] == ids.shape[0] + 1
    return struct.pack("<iiq", n_terms, max_len, ids.shape[0]) + offsets.tobytes() + ids.tobytes() + struct.pack("<q", terms.shape[0]) + terms.tobytes()


def test_lexbag_under_asan_ubsan(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "lexbag_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build_san", "lexbag_asan")
    rng = np.random.default_rng(4)
    good = []
    for n in (0, 1, 5, 300):
        lens = rng.integers(0, 50, n)
        off = np.concatenate([[0], np.cumsum(lens)])
        good.append((97, 0, off, rng.permutation(10 * n + 1)[:n], rng.integers(0, 97, int(off[-1]))))
    good.append((3, 0, [0, 70000, 70001], [4, 2], [2] * 70000 + [0]))                     # tf above the cap
    good.append((131072, 64, [0, 64, 64], [0, 2 ** 62], [131071] * 64))                  # the limits themselves
    bad = [(97, 0, [1, 2], [1], [0, 0]),                                                  # offsets do not start at 0
           (97, 0, [0, 3, 1], [1, 2], [0]),                                               # offsets decrease
           (97, 0, [0, -1], [1], []),                                                     # ... below zero
           (97, 0, [0, 2 ** 62, 2 ** 61], [1, 2], []),                                    # huge, then decreasing: terms never read
           (97, 0, [0, 1, 2], [1, 2], [5, 97]),                                           # a term out of range
           (97, 0, [0, 1, 2], [1, 2], [-1, 5]),
           (97, 0, [0, 1, 2], [1, 2], [2 ** 31 - 1, -2 ** 31]),
           (97, 0, [0, 1, 2], [1, -2], [5, 6]),                                           # a negative id
           (97, 0, [0, 1, 2, 3], [8, 9, 8], [5, 6, 7]),                                   # a duplicate id
           (97, 64, [0, 65], [1], [3] * 65)]                                              # a query of 65 occurrences
    cases = [(c, 0) for c in good] + [(c, 1) for c in bad]
    (tmp_path / "cases.bin").write_bytes(b"".join(_case(*c) for c, _ in cases))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.stdout.strip() == f"ok {len(cases)} cases"
    out = (tmp_path / "out.bin").read_bytes()
    pos = 0
    for (n_terms, _max_len, off, ids, terms), status in cases:
        assert struct.unpack_from("<i", out, pos)[0] == status
        pos += 4
        if status:
            continue
        terms = np.asarray(terms, np.int64)
        for i in range(len(ids)):                                 # the canonical bag: distinct terms ascending, capped tf, dl
            bag = terms[off[i]:off[i + 1]]
            uniq, cnt = np.unique(bag, return_counts=True)
            dl, d = struct.unpack_from("<qi", out, pos)
            pos += 12
            assert dl == bag.shape[0] and d == uniq.shape[0]
            got = np.frombuffer(out, np.int32, 2 * d, pos)
            pos += 8 * d
            assert np.array_equal(got[:d], uniq) and np.array_equal(got[d:], np.minimum(cnt, 65535))
    assert pos == len(out)
