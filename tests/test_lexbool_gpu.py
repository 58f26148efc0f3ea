"""Boolean lexical queries and match sets (sqe_lex_search_bool, sqe_lex_match; lexical.hip) and match sets as k-NN filters.  GPU only.

Everything is bit for bit against tests/lexbool_reference.py: ids equal, scores equal as bytes and as the uint32 score_int
recovered from the float (the reference's score_int is checked to lie below 2^24 first), counts and id lists equal.  The corpus
has three chunks, the last partial; before the device is looked at the reference itself has to show that the queries reach a
count of 0, a count above cap, matches in all three chunks, matches at the two rows either side of a chunk boundary and a
zero-score hit inside the top k."""
import numpy as np
import pytest

from . import lex_reference as LR
from . import lexbool_reference as BR
from .lexbool_reference import FILTER, MUST, MUST_NOT, SHOULD

pytestmark = pytest.mark.gpu

T = 600                                 # terms; term 599 is in no document
N_DOCS = 40_000
RARE = [590, 591, 592]                  # only in the planted bag


def same_bits(a, b):
    return all(u.shape == w.shape and u.dtype == w.dtype and np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
               for u, w in zip(a, b))


def flat(bags, dtype=np.int32):
    lens = np.array([len(b) for b in bags], np.int64)
    off = np.zeros(lens.shape[0] + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    terms = np.concatenate([np.asarray(b, dtype) for b in bags]) if off[-1] else np.zeros(0, dtype)
    return off, terms.astype(dtype)


def make_corpus(n=N_DOCS, seed=11):
    """n bags of 4..20 occurrences over terms 0..589, term t with probability ~ 1 / (t + 1); ids 7 + 3 i."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 591)
    p /= p.sum()
    lens = rng.integers(4, 21, n)
    draws = rng.choice(590, int(lens.sum()), p=p).astype(np.int32)
    bags = [a for a in np.split(draws, np.cumsum(lens)[:-1])]
    return 7 + 3 * np.arange(n, dtype=np.int64), bags


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def world(ctx):
    """(index, LexRef, LexBoolRef, bags, chunk_rows): the planted bag stands at the last row of chunk 0, the first of chunk 1 and
    in chunk 2, so one AND query matches on both sides of a chunk boundary and in every chunk."""
    from semantic_query_engine_amd import LexicalIndex
    ids, bags = make_corpus()
    lex = LexicalIndex(ctx, T)
    c = lex.info()["chunk_rows"]
    assert 2 * c < N_DOCS < 3 * c                             # three chunks, the last partial
    for row in (c - 1, c, 2 * c + 5):
        bags[row] = np.array(RARE + [3, 3, 0] + ([1] if row == c else []), np.int32)      # term 1 in one of them only
    order = np.random.default_rng(1).permutation(N_DOCS)
    for lo in range(0, N_DOCS, 10_000):
        part = order[lo:lo + 10_000]
        lex.put(ids[part], flat([bags[j] for j in part]))
    ref = LR.LexRef(ids, bags, T)
    assert ref.df[599] == 0 and all(ref.df[t] == 3 for t in RARE)
    return lex, ref, BR.LexBoolRef(ref), bags, c


def cases(bags):
    """name -> (terms, roles, min_should); query terms come from the bags of actual documents, so AND queries have matches."""
    rng = np.random.default_rng(5)

    def distinct(row, n):
        u = np.unique(bags[row])
        return [int(t) for t in rng.permutation(u)[:n]]

    d = [int(r) for r in rng.integers(0, N_DOCS, 12)]
    a5 = distinct(d[3], 5)
    mixed = distinct(d[5], 4)
    out = {
        "and2": (distinct(d[0], 2), [MUST] * 2, 0),
        "and3": (distinct(d[1], 3), [MUST] * 3, 0),
        "and64": ((distinct(d[2], 20) * 64)[:64], [MUST] * 64, 0),
        "and_planted": (RARE[:2], [MUST] * 2, 0),
        "ms1": (a5, [SHOULD] * len(a5), 1),
        "ms2": (a5, [SHOULD] * len(a5), 2),
        "ms_all_plus_one": (a5, [SHOULD] * len(a5), len(a5) + 1),
        "ms64": ((a5 * 64)[:64], [SHOULD] * 64, 64),
        "mixed": (mixed + [0], [MUST, SHOULD, FILTER, SHOULD][:len(mixed)] + [MUST_NOT], 0),
        "mixed_ms1": (mixed + [1], [MUST, SHOULD, FILTER, SHOULD][:len(mixed)] + [MUST_NOT], 1),
        "must_and_must_not": ([mixed[0], mixed[0]], [MUST, MUST_NOT], 0),
        "repeated_should": ([a5[0], a5[0], a5[1]], [SHOULD] * 3, 2),
        "repeated_must": ([mixed[0], mixed[0], mixed[1]], [MUST, MUST, SHOULD], 0),
        "filter_only": ([RARE[0]], [FILTER], 0),
        "filter_then_should": ([2, RARE[1], 5], [FILTER, SHOULD, SHOULD], 0),
        "filter_rare_should_common": ([RARE[2], 1], [FILTER, SHOULD], 0),
        "df0_must": ([599, 0], [MUST, SHOULD], 0),
        "df0_must_not": ([0, 599], [SHOULD, MUST_NOT], 0),
        "df0_should": ([599], [SHOULD], 0),
        "must_not_only": ([0, 1], [MUST_NOT, MUST_NOT], 0),
        "empty": ([], [], 0),
        "common_or": ([0, 1], [SHOULD, SHOULD], 0),
        "common_minus": ([0, 1, 2], [SHOULD, SHOULD, MUST_NOT], 0),
        "filter_ms2": ([4, 7, 9], [FILTER, SHOULD, SHOULD], 2),
    }
    return out


@pytest.fixture(scope="module")
def batch(world):
    """The cases as one batch, the reference's dense answer to each and the coverage the corpus has to give."""
    lex, ref, bref, bags, c = world
    cs = cases(bags)
    names = list(cs)
    Q, R, M = [cs[n][0] for n in names], [cs[n][1] for n in names], [cs[n][2] for n in names]
    counts, _ids, rows = bref.match(Q, R, M, cap=0)
    by = dict(zip(names, range(len(names))))
    # ---- coverage, from the reference alone
    for n in ("ms_all_plus_one", "must_and_must_not", "df0_must", "must_not_only", "empty", "df0_should"):
        assert counts[by[n]] == 0, n
    assert counts[by["common_or"]] > 1000                                       # above every cap used below
    planted = rows[by["and_planted"]]
    assert planted.tolist() == [c - 1, c, 2 * c + 5]                            # both sides of a chunk boundary, every chunk
    assert {int(r) // c for r in rows[by["and2"]]} == {0, 1, 2}
    _s, _i, sint = bref.search(Q, R, 256, M)
    zero_hit = by["filter_rare_should_common"]
    assert 0 < counts[zero_hit] <= 256 and (sint[zero_hit, :counts[zero_hit]] == 0).any() and (sint[zero_hit, :counts[zero_hit]] > 0).any()
    assert counts[by["filter_only"]] == 3
    assert counts[by["ms64"]] > 0 and counts[by["and64"]] > 0 and counts[by["ms2"]] > 0 and counts[by["mixed_ms1"]] > 0
    assert counts[by["common_minus"]] < counts[by["common_or"]] and counts[by["df0_must_not"]] == int((ref.tf[:, 0] > 0).sum())
    return names, Q, R, M, counts


def score_int_of(score):
    """The uint32 score_int behind a float score (exact below 2^24); padding -> 0."""
    s = np.where(np.isfinite(score), score, 0.0).astype(np.float64) * 65536.0
    assert np.array_equal(s, np.rint(s))
    return s.astype(np.uint32)


def check_search(lex, bref, Q, R, M, k):
    want_s, want_i, sint = bref.search(Q, R, k, M)
    assert int(sint.max(initial=0)) < 1 << 24
    got = lex.search_bool(Q, R, k, M)
    assert np.array_equal(got[1], want_i), [(b, got[1][b, :6], want_i[b, :6]) for b in range(len(Q)) if not np.array_equal(got[1][b], want_i[b])][:3]
    assert same_bits(got, (want_s, want_i))
    assert np.array_equal(score_int_of(got[0]), sint.astype(np.uint32))
    return got


@pytest.mark.parametrize("k", [1, 10, 256])
def test_search_bool_matches_reference(world, batch, k):
    lex, ref, bref, bags, c = world
    names, Q, R, M, counts = batch
    got = check_search(lex, bref, Q, R, M, k)
    at = names.index("filter_rare_should_common")
    if k == 256:                                                  # zero-score hits rank after every positive score
        n = int(counts[at])
        assert got[0][at, n - 1] == 0.0 and got[1][at, n - 1] >= 0 and np.isneginf(got[0][at, n])
        at = names.index("filter_only")
        assert got[0][at, :3].tolist() == [0.0] * 3 and got[1][at, :3].tolist() == [int(ref.ids[r]) for r in (c - 1, c, 2 * c + 5)]


def test_search_bool_batch_invariance(world, batch):
    lex, ref, bref, bags, c = world
    names, Q, R, M, counts = batch
    whole = lex.search_bool(Q, R, 10, M)
    mc, mi = lex.match(Q, R, M, cap=50)
    for b in range(len(Q)):
        one = lex.search_bool([Q[b]], [R[b]], 10, [M[b]])
        assert same_bits((one[0][0], one[1][0]), (whole[0][b], whole[1][b])), names[b]
        oc, oi = lex.match([Q[b]], [R[b]], [M[b]], cap=50)
        assert oc[0] == mc[b] and np.array_equal(oi[0], mi[b]), names[b]


@pytest.mark.parametrize("B", [1, 64, 257])
@pytest.mark.parametrize("k", [1, 10, 256])
def test_all_should_is_plain_search(world, B, k):
    """Every role SHOULD, min_should NULL or zeros: bit for bit sqe_lex_search."""
    lex, ref, bref, bags, c = world
    rng = np.random.default_rng(100 + B)
    Q = []
    for b in range(B):
        bag = bags[int(rng.integers(0, N_DOCS))]
        Q.append([int(t) for t in rng.choice(bag, int(rng.integers(0, 7)))] + ([599] if b % 9 == 0 else []))
    R = [[SHOULD] * len(q) for q in Q]
    plain = lex.search(Q, k)
    assert same_bits(lex.search_bool(Q, R, k), plain)
    assert same_bits(lex.search_bool(Q, R, k, [0] * B), plain)
    assert same_bits(lex.search_bool(Q, R, k, [1] * B), plain)    # m = max(1, min_should)


def test_match_sets(world, batch):
    lex, ref, bref, bags, c = world
    names, Q, R, M, counts = batch
    got_c, got_i = lex.match(Q, R, M, cap=0)
    assert np.array_equal(got_c, counts) and got_i.shape == (len(Q), 0)
    assert np.array_equal(lex.count(Q, R, M), counts)
    for cap in (1, 37, 1000):                                     # counts do not depend on cap; common_or has more than any of these
        want_c, want_i, _ = bref.match(Q, R, M, cap=cap)
        got_c, got_i = lex.match(Q, R, M, cap=cap)
        assert np.array_equal(got_c, counts) and np.array_equal(got_i, want_i), cap
        for b in range(len(Q)):                                   # ascending, then padding only
            n = min(cap, int(counts[b]))
            assert np.all(np.diff(got_i[b, :n]) > 0) and np.all(got_i[b, n:] == -1)
    for name in ("and2", "and_planted", "common_or", "mixed", "ms2", "empty"):       # cap = count and count + 7, one query each
        b = names.index(name)
        for cap in (int(counts[b]), int(counts[b]) + 7):
            want_c, want_i, _ = bref.match([Q[b]], [R[b]], [M[b]], cap=cap)
            got_c, got_i = lex.match([Q[b]], [R[b]], [M[b]], cap=cap)
            assert got_c[0] == counts[b] and np.array_equal(got_i, want_i), (name, cap)
    got_c, got_i = lex.match(Q, R, M)                             # cap = None: the largest count
    assert got_i.shape[1] == counts.max() and np.array_equal(got_i, bref.match(Q, R, M)[1])
    assert lex.info()["rebuilds"] == 1                            # nothing here touched the index


def test_delete_and_replacing_put_equal_a_fresh_index(ctx, world, batch):
    from semantic_query_engine_amd import LexicalIndex
    _lex, ref, bref, bags, c = world
    names, Q, R, M, counts = batch
    ids, _ = make_corpus()
    rng = np.random.default_rng(77)
    lex = LexicalIndex(ctx, T)
    lex.put(ids, flat(bags))
    assert np.array_equal(lex.count(Q, R, M), counts)             # built, searched once
    gone = rng.choice(N_DOCS, 9000, replace=False)                # the live documents now end in chunk 1
    changed = rng.choice(np.setdiff1d(np.arange(N_DOCS), gone), 300, replace=False)
    new_bags = list(bags)
    for j in changed:
        new_bags[j] = bags[(j * 7 + 1) % N_DOCS][::-1].copy()
    lex.delete(ids[gone])
    lex.put(ids[changed], flat([new_bags[j] for j in changed]))
    live = np.setdiff1d(np.arange(N_DOCS), gone)
    fresh = LexicalIndex(ctx, T)
    fresh.put(ids[live], flat([new_bags[j] for j in live]))
    assert same_bits(lex.search_bool(Q, R, 10, M), fresh.search_bool(Q, R, 10, M))
    a, b = lex.match(Q, R, M, cap=300), fresh.match(Q, R, M, cap=300)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], counts)
    assert lex.info()["rebuilds"] == 2 and lex.info()["chunks"] == 2
    # and the fresh index agrees with the reference of the live documents
    small = BR.LexBoolRef(LR.LexRef(ids[live], [new_bags[j] for j in live], T))
    check_search(fresh, small, Q, R, M, 10)
    assert np.array_equal(b[1], small.match(Q, R, M, cap=300)[1])
    lex.close()
    fresh.close()


def test_invalid_arguments_write_nothing(world):
    from semantic_query_engine_amd import _native as N
    lex = world[0]
    lib = N.load()
    score, ids = np.full((2, 4), 77.0, np.float32), np.full((2, 4), 77, np.int64)
    cnt, mid = np.full(2, 77, np.int64), np.full((2, 4), 77, np.int64)

    def call(Q, R, M, k=4, cap=4, null_ids=False):
        qoff, qterms = flat(Q)
        _, roles = flat(R, np.uint8)
        ms = None if M is None else np.asarray(M, np.int32)
        common = (lex.handle, qoff.ctypes.data, qterms.ctypes.data, roles.ctypes.data, None if ms is None else ms.ctypes.data, len(Q))
        return (lib.sqe_lex_search_bool(*common, k, score.ctypes.data, ids.ctypes.data),
                lib.sqe_lex_match(*common, cap, cnt.ctypes.data, None if null_ids else mid.ctypes.data))

    ok = ([[1, 2], [3]], [[MUST, SHOULD], [FILTER]], [0, 0])
    bad = [dict(Q=[[1, 2], [3]], R=[[MUST, 4], [FILTER]], M=[0, 0]),              # a role above 3
           dict(Q=ok[0], R=ok[1], M=[0, -1]), dict(Q=ok[0], R=ok[1], M=[65, 0]),  # min_should outside [0, 64]
           dict(Q=[[1, T], [3]], R=ok[1], M=None),                                # what sqe_lex_search refuses: a term out of range,
           dict(Q=[[1] * 65, [3]], R=[[MUST] * 65, [FILTER]], M=None)]            # more than 64 occurrences
    for kw in bad:
        assert call(**kw) == (-1, -1), kw
    assert call(*ok, k=0, cap=-1) == (-1, -1)                     # k outside [1, 256]; cap < 0
    assert call(*ok, k=257, null_ids=True) == (-1, -1)            # ids are needed for cap > 0
    assert np.all(score == 77) and np.all(ids == 77) and np.all(cnt == 77) and np.all(mid == 77)
    assert call(*ok) == (0, 0) and not np.any(cnt == 77) and not np.any(ids == 77)


def test_no_queries_and_empty_index(ctx):
    from semantic_query_engine_amd import LexicalIndex
    lex = LexicalIndex(ctx, T)
    for _ in range(2):                                            # empty, then B = 0 and searches on three documents
        score, ids = lex.search_bool([], [], 5)
        assert score.shape == (0, 5) and ids.shape == (0, 5)
        counts, mids = lex.match([], [], cap=3)
        assert counts.shape == (0,) and mids.shape == (0, 3)
        score, ids = lex.search_bool([[1, 2]], [[MUST, SHOULD]], 5)
        counts, mids = lex.match([[1], [2]], [[FILTER], [SHOULD]], cap=3)
        if len(lex) == 0:
            assert np.all(np.isneginf(score)) and np.all(ids == -1) and counts.tolist() == [0, 0] and np.all(mids == -1)
            assert lex.count([[1]], [[MUST]]).tolist() == [0]
        else:
            assert ids[0].tolist() == [4, 9, -1, -1, -1] and counts.tolist() == [2, 2] and mids.tolist() == [[4, 9, -1], [4, 6, -1]]
        lex.put([4, 6, 9], [[1, 2], [2], [1, 1]])
    lex.close()


def test_device_form_writes_device_memory(world, batch):
    import torch
    lex, ref, bref, bags, c = world
    names, Q, R, M, counts = batch
    k, cap = 10, 20
    score = torch.empty((len(Q), k), dtype=torch.float32, device="cuda")
    ids = torch.empty((len(Q), k), dtype=torch.int64, device="cuda")
    cnt = torch.empty(len(Q), dtype=torch.int64, device="cuda")
    mid = torch.empty((len(Q), cap), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lex.search_bool_device(Q, R, k, score.data_ptr(), ids.data_ptr(), M)
    lex.match_device(Q, R, M, cap, cnt.data_ptr(), mid.data_ptr())
    lex.ctx.synchronize()
    want = lex.search_bool(Q, R, k, M)
    assert same_bits((score.cpu().numpy(), ids.cpu().numpy()), want)
    wc, wi = lex.match(Q, R, M, cap=cap)
    assert np.array_equal(cnt.cpu().numpy(), wc) and np.array_equal(mid.cpu().numpy(), wi)


# ------------------------------------------------------------------------------ retrieval layer and shim
PD = 64
VOCAB = ["aspirin", "fever", "pain", "brca1", "gene", "olaparib", "cancer", "risk", "metformin", "diabetes", "trial", "dose",
         "adult", "patients", "therapy", "tumor", "marker", "insulin", "placebo", "cohort"]


@pytest.fixture(scope="module")
def toy():
    """300 chunks of 3..9 words over a toy vocabulary (word w with probability ~ 1 / (w + 1)), ten doc_ids, random vectors."""
    from oracle import wordpiece as WP
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    rng = np.random.default_rng(23)
    p = 1.0 / np.arange(1, len(VOCAB) + 1)
    p /= p.sum()
    texts = [" ".join(rng.choice(VOCAB, int(rng.integers(3, 10)), p=p)) for _ in range(300)]
    docs = [{"doc_id": f"d{i % 10}", "text": t} for i, t in enumerate(texts)]
    toks = WP.synthetic_vocab([" ".join(VOCAB)], size=200)
    x = rng.standard_normal((len(docs), PD)).astype(np.float32)
    return docs, WordPieceTokenizer(vocab_text="\n".join(toks) + "\n"), x


def m(text, **opts):
    return {"match": {"text": dict(query=text, **opts) if opts else text}}


def live_reference(idx, analyzer):
    rows = [r for r, s in enumerate(idx.sources) if s is not None]
    return BR.LexBoolRef(LR.LexRef(rows, analyzer.analyze([idx.sources[r]["text"] for r in rows]), analyzer.n_terms))


def test_indexer_text_clauses_as_knn_filters(ctx, toy):
    """search(query_emb, k, filter=...) is VectorIndex.search over the reference's match ids, bit for bit."""
    from semantic_query_engine_amd import retrieval as RT
    docs, tok, x = toy
    client = RT.GpuSearchClient(ctx, dim=PD)
    ix = RT.OpenSearchIndexer(client, "toy")
    ix.add_embeddings(x, docs)
    RT.configure_analyzer(tok, max_len=256)
    try:
        an, idx = RT._analyzer, client.index("toy")
        bref = live_reference(idx, an)
        q = x[17:18] + 0.05
        k = 12

        def ref_ids(clause):
            terms, roles, ms = RT.text_query(clause)
            return bref.match([terms], [roles], [ms])[1][0]

        def check(flt, allow):
            assert 0 < allow.shape[0] < len(docs)
            cos, ids = idx.vectors.search(q, k, filter_ids=allow)
            hits = ix.search(q, k, filter=flt)
            assert [h["text"] for h, _ in hits] == [idx.sources[r]["text"] for r in ids[0] if r >= 0] and len(hits) == min(k, allow.shape[0])
            assert [s for _, s in hits] == [float(1.0 / (2.0 - float(c))) for c, r in zip(cos[0], ids[0]) if r >= 0]
            bc, bi = ix.search_batch(np.concatenate([q, x[3:4]]), k, filters=[flt, None])
            assert same_bits((bc[0:1], bi[0:1]), (cos, ids)) and same_bits((bc[1:2], bi[1:2]), idx.vectors.search(x[3:4], k))

        both = m("gene cancer", operator="and")
        a = ref_ids(both)
        check(both, a)
        in_docs = np.array([r for r, d in enumerate(docs) if d["doc_id"] in ("d1", "d4", "d7")], np.int64)
        check({"bool": {"filter": [both, {"terms": {"doc_id": ["d1", "d4", "d7"]}}]}}, np.intersect1d(a, in_docs))
        check({"bool": {"must_not": [m("aspirin")]}}, np.setdiff1d(np.arange(len(docs)), ref_ids(m("aspirin"))))
        # the text routes of the indexer against the reference
        assert ix.count_text(both) == a.shape[0] and ix.count_text("aspirin fever") == ref_ids(m("aspirin fever")).shape[0]
        clause = {"bool": {"must": [m("gene")], "should": [m("cancer"), m("risk")], "filter": [m("aspirin")], "must_not": [m("dose")]}}
        terms, roles, ms = RT.text_query(clause)
        score, ids, _ = bref.search([terms], [roles], 20, [ms])
        hits = ix.search_text(clause, 20)
        assert [h["text"] for h, _ in hits] == [idx.sources[r]["text"] for r in ids[0] if r >= 0] and len(hits) > 1
        assert [s for _, s in hits] == [float(s) for s in score[0] if np.isfinite(s)]
        terms, roles, ms = RT.text_query(m("gene cancer risk", minimum_should_match=2))
        score, ids, _ = bref.search([terms], [roles], 20, [ms])
        hits = ix.search_text("gene cancer risk", 20, minimum_should_match=2)
        assert [s for _, s in hits] == [float(s) for s in score[0] if np.isfinite(s)] and len(hits) > 0
        assert [h["text"] for h, _ in ix.search_text("gene cancer", 256, operator="and")] == \
            [idx.sources[r]["text"] for r in bref.search(*[[v] for v in RT.text_query(both)[:2]], 256)[1][0] if r >= 0]
    finally:
        RT.configure_analyzer(None)


def test_shim_text_clauses_end_to_end(ctx, toy):
    import json

    from fastapi.testclient import TestClient

    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim
    docs, tok, x = toy
    RT.configure_analyzer(tok, max_len=256)
    try:
        an = RT._analyzer
        client = RT.GpuSearchClient(ctx, dim=PD)
        with TestClient(shim.create_app(client, None, PD)) as c:
            assert c.put("/toy", json={}).status_code == 200
            lines = []
            for i, d in enumerate(docs):
                lines.append(json.dumps({"index": {"_index": "toy", "_id": f"c{i}"}}))
                lines.append(json.dumps({"doc_id": d["doc_id"], "text": d["text"], "embedding": x[i].tolist()}))
            assert c.post("/_bulk", content=("\n".join(lines) + "\n").encode()).json()["errors"] is False
            idx = client.index("toy")
            bref = live_reference(idx, an)
            # _search with operator: a bool of one must clause
            both = m("gene cancer", operator="and")
            r = c.post("/toy/_search", json={"size": 50, "query": {"bool": {"must": [both]}}})
            assert r.status_code == 200, r.text
            terms, roles, ms = RT.text_query(both)
            score, ids, _ = bref.search([terms], [roles], 50, [ms])
            hits = r.json()["hits"]["hits"]
            assert [h["_id"] for h in hits] == [f"c{i}" for i in ids[0] if i >= 0] and len(hits) > 1
            assert [h["_score"] for h in hits] == [float(s) for s in score[0] if np.isfinite(s)]
            assert all(t in h["_source"]["text"].split() for h in hits for t in ("gene", "cancer"))
            # a bool with every role; the filter-only matches come last with _score 0
            clause = {"bool": {"filter": [m("aspirin")], "should": [m("risk")], "must_not": [m("dose")]}}
            r = c.post("/toy/_search", json={"size": 256, "query": clause})
            terms, roles, ms = RT.text_query(clause)
            score, ids, sint = bref.search([terms], [roles], 256, [ms])
            hits = r.json()["hits"]["hits"]
            assert [h["_id"] for h in hits] == [f"c{i}" for i in ids[0] if i >= 0]
            assert [h["_score"] for h in hits] == [float(s) for s in score[0] if np.isfinite(s)] and hits[-1]["_score"] == 0.0 < hits[0]["_score"]
            # _count with a query
            n = int(bref.match([terms], [roles], [ms], cap=0)[0][0])
            assert c.post("/toy/_count", json={"query": clause}).json()["count"] == n == len(hits)
            assert c.post("/toy/_count", json={"query": both}).json()["count"] == int(bref.match(*[[v] for v in RT.text_query(both)], cap=0)[0][0])
            assert c.get("/toy/_count").json()["count"] == len(docs)
            # knn.filter with a match
            allow = bref.match(*[[v] for v in RT.text_query(both)])[1][0]
            body = {"size": 8, "query": {"knn": {"embedding": {"vector": x[5].tolist(), "k": 8, "filter": {"bool": {"filter": [both]}}}}}}
            r = c.post("/toy/_search", json=body)
            assert r.status_code == 200, r.text
            cos, vid = idx.vectors.search(x[5:6], 8, filter_ids=allow)
            assert [h["_id"] for h in r.json()["hits"]["hits"]] == [f"c{i}" for i in vid[0] if i >= 0]
            body["query"]["knn"]["embedding"]["filter"] = both
            assert [h["_id"] for h in c.post("/toy/_search", json=body).json()["hits"]["hits"]] == [f"c{i}" for i in vid[0] if i >= 0]
            # what still gets the 400
            for query in ({"bool": {"must": [m("gene cancer"), m("risk")]}}, {"bool": {"must": [{"bool": {"must": [m("gene")]}}, m("risk")]}},
                          {"match": {"text": {"query": "gene", "fuzziness": "AUTO"}}}, {"bool": {"must_not": [m("gene")]}}):
                assert c.post("/toy/_search", json={"query": query}).status_code == 400, query
            assert c.post("/toy/_count", json={"query": {"bool": {"must": [m("gene cancer"), m("risk")]}}}).status_code == 400
            body["query"]["knn"]["embedding"]["filter"] = m("gene", fuzziness="AUTO")
            assert c.post("/toy/_search", json=body).status_code == 400
    finally:
        RT.configure_analyzer(None)
