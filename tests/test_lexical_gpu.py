"""BM25 lexical index (sqe_lex_*, lexical.hip) and hybrid BM25 + k-NN rank fusion (sqe_index_search_hybrid, fuse.hip).  GPU only.

The score is defined in integers (include/sqe.h), so every comparison here is bit for bit: LexicalIndex.search against
tests/lex_reference.py on the same documents -- ids equal, scores equal as bytes --, the device state against the reference's
df / idf / dl / impacts, and search_hybrid against tests/fuse_reference.py fed the library's OWN vector and lexical lists.  No
tolerance, no case left out.  Before a score is compared the reference's score_int is checked to lie below 2^24, so the float
output hides no low bit."""
import ctypes as C

import numpy as np
import pytest

from . import lex_reference as LR

pytestmark = pytest.mark.gpu

T = 97                                  # terms; term 96 is in no document
QUERIES = [[3, 3, 7, 1, 0],             # a repeated term (the bag of the tied documents)
           [96],                        # df = 0: no hit
           [0],                         # the commonest term
           [],                          # the empty query
           [95, 90],                    # rare terms: k above the number of hits
           [5, 96, 12, 5],
           list(range(64))]             # the longest query allowed


def same_bits(a, b):
    return all(u.shape == w.shape and u.dtype == w.dtype and np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
               for u, w in zip(a, b))


def flat(bags):
    lens = np.array([len(b) for b in bags], np.int64)
    off = np.zeros(lens.shape[0] + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    terms = np.concatenate([np.asarray(b, np.int32) for b in bags]) if off[-1] else np.zeros(0, np.int32)
    return off, terms.astype(np.int32)


def zipf_bags(rng, n, terms=96, max_len=40):
    """n bags of 0..max_len occurrences, term t with probability ~ 1 / (t + 1)."""
    p = 1.0 / np.arange(1, terms + 1)
    p /= p.sum()
    lens = rng.integers(0, max_len + 1, n)
    draws = rng.choice(terms, int(lens.sum()), p=p).astype(np.int32)
    return [a for a in np.split(draws, np.cumsum(lens)[:-1])] if n else []


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def chunk_rows(ctx):
    from semantic_query_engine_amd import LexicalIndex
    lex = LexicalIndex(ctx, T)
    c = lex.info()["chunk_rows"]
    lex.close()
    return c


@pytest.fixture(scope="module")
def corpus(chunk_rows):
    """2 C + 17 documents; ids 5 + 3 i.  Document 0 is empty, document 1 has tf > 1, and the bag of document 5 stands again
    in the two other chunks."""
    c = chunk_rows
    n = 2 * c + 17
    bags = zipf_bags(np.random.default_rng(3), n)
    bags[0] = np.zeros(0, np.int32)
    bags[1] = np.array([2, 2, 2, 4], np.int32)
    bags[5] = np.array([3, 3, 7, 1, 0], np.int32)
    bags[c + 5] = bags[5].copy()
    bags[2 * c + 5] = bags[5].copy()
    ids = 5 + 3 * np.arange(n, dtype=np.int64)
    return ids, bags


_BUILT = {}


def built(ctx, corpus, n):
    """(index, reference) over the first n documents, put in a shuffled order; made once per size."""
    if n not in _BUILT:
        from semantic_query_engine_amd import LexicalIndex
        ids, bags = corpus
        order = np.random.default_rng(n).permutation(n)
        lex = LexicalIndex(ctx, T)
        lex.put(ids[order], flat([bags[j] for j in order]))
        _BUILT[n] = (lex, LR.LexRef(ids[:n], bags[:n], T))
    return _BUILT[n]


def sizes(c):
    return {"1": 1, "C-1": c - 1, "C": c, "C+1": c + 1, "2C+17": 2 * c + 17}


def check_search(lex, ref, queries, k):
    want_s, want_i, sint = ref.search(queries, k)
    assert int(sint.max(initial=0)) < 1 << 24                # the float output holds every bit of score_int
    got = lex.search(queries, k)
    assert np.array_equal(got[1], want_i), (got[1][:, :8], want_i[:, :8])
    assert same_bits(got, (want_s, want_i))
    return got


@pytest.mark.parametrize("k", [1, 10, 256])
@pytest.mark.parametrize("size", ["1", "C-1", "C", "C+1", "2C+17"])
def test_search_matches_reference(ctx, corpus, chunk_rows, size, k):
    lex, ref = built(ctx, corpus, sizes(chunk_rows)[size])
    all7 = check_search(lex, ref, QUERIES, k)                 # B = 7
    for b, q in enumerate(QUERIES):                           # B = 1: row b of the batch is the single call
        one = check_search(lex, ref, [q], k)
        assert same_bits((one[0][0], one[1][0]), (all7[0][b], all7[1][b]))
    assert np.all(all7[1][1] == -1) and np.all(np.isneginf(all7[0][1]))      # df = 0
    assert np.all(all7[1][3] == -1)                                          # empty query


def test_ties_come_in_id_order(ctx, corpus, chunk_rows):
    c = chunk_rows
    lex, ref = built(ctx, corpus, 2 * c + 17)
    ids, _ = corpus
    twins = [int(ids[5]), int(ids[c + 5]), int(ids[2 * c + 5])]             # one bag, one row in each chunk
    score, got = check_search(lex, ref, [QUERIES[0]], 256)
    at = [int(np.nonzero(got[0] == t)[0][0]) for t in twins]
    assert at[1] == at[0] + 1 and at[2] == at[0] + 2
    assert score[0][at[0]] == score[0][at[1]] == score[0][at[2]]


def test_impact_clamps_to_one(ctx, chunk_rows):
    """A term in every document: idf * 2^16 is about 1 at 2 C + 17 documents, so with k1 = 3, b = 1 most impacts round to 0 and
    are raised to 1 -- a document that holds a query term is always a hit."""
    from semantic_query_engine_amd import LexicalIndex
    n = 2 * chunk_rows + 17
    bags = [np.concatenate([[0], b]).astype(np.int32) for b in zipf_bags(np.random.default_rng(9), n)]
    ids = np.arange(n, dtype=np.int64)
    ref = LR.LexRef(ids, bags, T, k1=3.0, b=1.0)
    assert ref.df[0] == n and np.rint(ref.bm25[:, 0] * 65536.0).min() == 0.0 and ref.impact[:, 0].min() == 1
    lex = LexicalIndex(ctx, T, k1=3.0, b=1.0)
    lex.put(ids, flat(bags))
    got = check_search(lex, ref, [[0], [0, 0, 0]], 256)
    assert np.all(got[1] >= 0)
    lex.close()


def test_mutations_equal_a_fresh_index(ctx, chunk_rows):
    from semantic_query_engine_amd import LexicalIndex
    c = chunk_rows
    rng = np.random.default_rng(21)
    n = c + 40
    bags = zipf_bags(rng, n)
    ids = rng.permutation(4 * n)[:n].astype(np.int64)          # out of order, with gaps
    live = {}
    lex = LexicalIndex(ctx, T)

    def step(rebuilds):
        keys = sorted(live)
        ref = LR.LexRef(keys, [live[i] for i in keys], T)
        fresh = LexicalIndex(ctx, T)
        if keys:
            fresh.put(keys, flat([live[i] for i in keys]))
        for k in (10, 256):
            got = check_search(lex, ref, QUERIES, k)
            assert same_bits(got, fresh.search(QUERIES, k))
        fresh.close()
        assert len(lex) == len(keys)
        assert lex.info()["rebuilds"] == rebuilds and lex.info()["documents"] == len(keys)

    assert lex.info()["rebuilds"] == 0
    lex.put(ids, flat(bags))
    live.update({int(i): b for i, b in zip(ids, bags)})
    step(1)
    step(1)                                                    # nothing changed: no rebuild
    again = ids[rng.permutation(n)[:10]]                       # replace live ids, one by an empty bag
    new = zipf_bags(rng, 10)
    new[0] = np.zeros(0, np.int32)
    lex.put(again, flat(new))
    live.update({int(i): b for i, b in zip(again, new)})
    step(2)
    gone = ids[rng.permutation(n)[:c]]                         # a whole chunk's worth
    lex.delete(np.concatenate([gone, [10 ** 12, -3]]))         # unknown ids are skipped
    for i in gone:
        del live[int(i)]
    step(3)
    lex.delete(np.array([10 ** 12], np.int64))                 # nothing deleted: nothing to rebuild
    step(3)
    lex.delete(np.array(sorted(live), np.int64))               # everything
    live.clear()
    step(4)
    back = zipf_bags(rng, 20)
    lex.put(ids[:20], flat(back))
    live.update({int(i): b for i, b in zip(ids[:20], back)})
    step(5)
    lex.close()


def test_state_read_back(ctx, corpus, chunk_rows):
    from semantic_query_engine_amd import engine as E
    c = chunk_rows
    n = c + 1
    lex, ref = built(ctx, corpus, n)
    lex.search([[0]], 1)
    info = lex.info()
    assert info["documents"] == n and info["n_terms"] == T and info["chunks"] == 2 and info["chunk_rows"] == c
    assert np.float64(info["avgdl"]).tobytes() == np.float64(ref.avgdl).tobytes()
    assert np.array_equal(lex.state_read(E.LEX_DF, np.int32, T), ref.df)
    assert lex.state_read(E.LEX_IDF, np.float64, T).tobytes() == ref.idf.tobytes()
    assert np.array_equal(lex.state_read(E.LEX_IDS, np.int64, n), ref.ids)
    assert np.array_equal(lex.state_read(E.LEX_DL, np.int64, n), ref.dl)
    table = lex.state_read(E.LEX_TABLE, np.uint32, 2 * (T + 1)).reshape(2, T + 1)
    assert info["postings"] == int((ref.tf > 0).sum()) == int(table[:, T].sum())
    post = lex.state_read(E.LEX_POSTINGS, np.uint32, 2 * info["postings"]).reshape(-1, 2)
    base = 0
    for ch in range(2):
        rows = np.arange(ch * c, min(n, (ch + 1) * c))
        for t in range(T):
            run = post[base + table[ch, t]:base + table[ch, t + 1]]
            hold = rows[ref.tf[rows, t] > 0]
            want = set(zip(hold.tolist(), ref.impact[hold, t].tolist()))
            assert len(run) == len(want) and set(map(tuple, run.tolist())) == want, (ch, t)
        base += int(table[ch, T])


def test_invalid_arguments_leave_everything_untouched(ctx):
    from semantic_query_engine_amd import LexicalIndex, _native as N
    lib = N.load()
    for k1, b in ((-0.1, 0.75), (3.1, 0.75), (float("nan"), 0.75), (1.2, -0.01), (1.2, 1.5), (1.2, float("nan"))):
        h = C.c_void_p(7)
        assert lib.sqe_lex_create(ctx.handle, T, k1, b, C.byref(h)) == -1 and not h.value
    for n_terms in (0, 131073):
        h = C.c_void_p()
        assert lib.sqe_lex_create(ctx.handle, n_terms, 1.2, 0.75, C.byref(h)) == -1
    lex = LexicalIndex(ctx, T)
    lex.put([1, 2, 3], [[1, 2], [2, 3, 3], [4]])
    before = lex.search(QUERIES[:3] + [[2, 3]], 4)

    def put(ids, bags):
        off, terms = flat(bags)
        ids = np.asarray(ids, np.int64)
        return lib.sqe_lex_put(lex.handle, ids.ctypes.data, off.ctypes.data, terms.ctypes.data, ids.shape[0])

    assert put([7, 8], [[1], [T]]) == -1                       # a term out of range
    assert put([7, 8], [[1], [-1]]) == -1
    assert put([7, -8], [[1], [2]]) == -1                      # a negative id
    assert put([7, 9, 7], [[1], [2], [3]]) == -1               # a duplicate id
    bad_off = np.array([0, 2, 1], np.int64)
    two = np.array([7, 8], np.int64)
    terms = np.array([1, 2], np.int32)
    assert lib.sqe_lex_put(lex.handle, two.ctypes.data, bad_off.ctypes.data, terms.ctypes.data, 2) == -1
    assert len(lex) == 3 and lex.info()["rebuilds"] == 1
    assert same_bits(lex.search(QUERIES[:3] + [[2, 3]], 4), before)

    def search(queries, k, alloc_k=None):
        off, terms = flat(queries)
        score = np.full((len(queries), alloc_k or max(k, 1)), 77.0, np.float32)
        ids = np.full(score.shape, 77, np.int64)
        rc = lib.sqe_lex_search(lex.handle, off.ctypes.data, terms.ctypes.data, len(queries), k, score.ctypes.data, ids.ctypes.data)
        return rc, score, ids

    for queries, k in (([[1], [T]], 4), ([[-1]], 4), ([[1] * 65], 4), ([[1]], 0), ([[1]], 257), ([[1]], -1)):
        rc, score, ids = search(queries, k, alloc_k=4)
        assert rc == -1 and np.all(score == 77.0) and np.all(ids == 77), (queries, k)
    rc, score, ids = search([[1] * 64], 4)
    assert rc == 0 and ids[0, 0] == 1
    lex.close()


# ------------------------------------------------------------------------------ hybrid
D = 64
ROWS = 4096
ONLY_LEX = 5000                         # an id the vector index does not hold
ONLY_VEC = 7                            # a row without a document in the lexical index


@pytest.fixture(scope="module")
def hdata():
    rng = np.random.default_rng(31)
    centre = rng.standard_normal((300, D)).astype(np.float32)
    x = centre[rng.integers(0, 300, ROWS)] + rng.standard_normal((ROWS, D)).astype(np.float32)
    bags = zipf_bags(rng, ROWS + 1)
    bags[ROWS] = np.array([95, 95, 94, 93], np.int32)          # the document of ONLY_LEX: rare terms
    ids = np.concatenate([np.arange(ROWS), [ONLY_LEX]]).astype(np.int64)
    keep = ids != ONLY_VEC
    return x, centre, ids[keep], [b for b, kp in zip(bags, keep) if kp]


@pytest.fixture(scope="module")
def hlex(ctx, hdata):
    from semantic_query_engine_amd import LexicalIndex
    lex = LexicalIndex(ctx, T)
    lex.put(hdata[2], flat(hdata[3]))
    return lex


@pytest.fixture(scope="module")
def hvec(ctx, hdata):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, D)
    idx.add(hdata[0])
    return idx


def depth_of(k, depth):
    return depth if depth else min(256, max(32, 4 * k))


def check_hybrid(idx, lex, q, q_terms, offsets, k, weights=None, depth=0, c=60, nprobe=0):
    got = idx.search_hybrid(lex, q, q_terms, k, offsets=offsets, weights=weights, depth=depth, rank_constant=c, nprobe=nprobe)
    n = depth_of(k, depth)
    if q.shape[0]:
        cos, ids = idx.search(q, n, nprobe=nprobe)
    else:
        cos, ids = np.empty((0, n), np.float32), np.empty((0, n), np.int64)
    ls, li = lex.search(q_terms, n)
    want = LR.hybrid(cos, ids, offsets, ls, li, k, weights, c)
    assert np.array_equal(got[1], want[1]), (got[1][:, :8], want[1][:, :8])
    assert same_bits(got, want)
    return got, (ls, li)


def near(hdata, rows, seed):
    rng = np.random.default_rng(seed)
    return (hdata[0][rows] + 0.3 * rng.standard_normal((len(rows), D)).astype(np.float32)).astype(np.float32)


def test_hybrid_ragged_groups_and_weights(hdata, hvec, hlex):
    q = near(hdata, [ONLY_VEC, 100, 200, 300, 400], 1)
    offsets = np.array([0, 2, 2, 5], np.int64)                 # G = 3: two sub-queries, none, three
    terms = [[95, 94, 3], [5, 12, 5], [0, 1]]
    for weights, k, depth in ((None, 10, 0), (np.array([0.5, 2.0, 1.0, 64.0, 1e-3, 3.0, 0.25, 8.0], np.float32), 10, 40), (None, 256, 256)):
        (fused, ids, cos, bm), _ = check_hybrid(hvec, hlex, q, terms, offsets, k, weights, depth)
    # an id only the lexical index holds and a row only the vector index holds are both returned
    (fused, ids, cos, bm), _ = check_hybrid(hvec, hlex, q, terms, offsets, 64, depth=64)
    a = int(np.nonzero(ids[0] == ONLY_LEX)[0][0])
    b = int(np.nonzero(ids[0] == ONLY_VEC)[0][0])
    assert np.isneginf(cos[0, a]) and bm[0, a] > 0 and np.isneginf(bm[0, b]) and cos[0, b] > 0.5


def test_hybrid_without_vectors_is_the_lexical_order(hdata, hvec, hlex):
    q = np.zeros((0, D), np.float32)
    (fused, ids, cos, bm), (ls, li) = check_hybrid(hvec, hlex, q, [[3, 3, 7], []], np.array([0, 0, 0], np.int64), 20, depth=32)
    assert np.array_equal(ids[0], li[0][:20]) and same_bits((bm[0],), (ls[0][:20],)) and np.all(np.isneginf(cos))
    assert np.all(ids[1] == -1) and np.all(np.isneginf(bm[1])) and np.all(np.isneginf(fused[1]))


def test_hybrid_with_empty_lexical_queries_is_the_fused_search(hdata, hvec, hlex):
    q = near(hdata, [10, 20, 30, 40, 50, 60], 2)
    offsets = np.array([0, 1, 4, 6], np.int64)
    w = np.array([1.0, 0.5, 2.0, 3.0, 1.0, 7.0], np.float32)
    for weights in (None, w):
        wh = None if weights is None else np.concatenate([weights, np.ones(3, np.float32)])
        (fused, ids, cos, bm), _ = check_hybrid(hvec, hlex, q, [[], [], []], offsets, 10, wh, depth=32)
        assert same_bits((fused, ids, cos), hvec.search_fused(q, 10, offsets=offsets, mode="rrf", weights=weights, depth=32))
        assert np.all(np.isneginf(bm))


def test_hybrid_ivf(ctx, hdata, hlex):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    ivf = VectorIndex(ctx, D, INDEX_IVF_FLAT, 16)
    ivf.add(hdata[0])
    ivf.train(hdata[0], iters=5, seed=1)
    q = near(hdata, [11, 22, 33, 44], 3)
    check_hybrid(ivf, hlex, q, [[5, 9], [2]], np.array([0, 2, 4], np.int64), 10, depth=32, nprobe=4)
    ivf.close()


def test_hybrid_device_group_equals_single_device(hdata, hvec, hlex):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, LexicalIndex, VectorIndex
    gctx = Context(devices=[0, 0], exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    g.add(hdata[0])
    glex = LexicalIndex(gctx, T)                               # lives on the leader
    glex.put(hdata[2], flat(hdata[3]))
    q = near(hdata, [ONLY_VEC, 100, 200, 300, 400], 4)
    offsets = np.array([0, 2, 2, 5], np.int64)
    terms = [[95, 94, 3], [5, 12, 5], []]
    w = np.array([0.5, 2.0, 1.0, 4.0, 1e-2, 3.0, 0.25, 8.0], np.float32)
    for weights, k, depth in ((None, 10, 0), (w, 20, 64)):
        a = g.search_hybrid(glex, q, terms, k, offsets=offsets, weights=weights, depth=depth)
        assert same_bits(a, hvec.search_hybrid(hlex, q, terms, k, offsets=offsets, weights=weights, depth=depth))
    e = np.zeros((0, D), np.float32)
    assert same_bits(g.search_hybrid(glex, e, [[3, 7]], 5, offsets=[0, 0]), hvec.search_hybrid(hlex, e, [[3, 7]], 5, offsets=[0, 0]))
    glex.close()
    g.close()
    gctx.close()


def test_hybrid_invalid_arguments(hdata, hvec, hlex):
    from semantic_query_engine_amd import _native as N
    q = near(hdata, list(range(32)), 5)
    with pytest.raises(N.SqeError):
        hvec.search_hybrid(hlex, q, [[1]], 10, offsets=[0, 32])            # 32 vector sub-queries: one too many
    with pytest.raises(N.SqeError):
        hvec.search_hybrid(hlex, q[:8], [[1]], 10, depth=256)              # (8 + 1) x 256 > 2048
    with pytest.raises(N.SqeError):
        hvec.search_hybrid(hlex, q[:2], [[T]], 10)                         # a term out of range
    with pytest.raises(N.SqeError):
        hvec.search_hybrid(hlex, q[:2], [[1] * 65], 10)
    with pytest.raises(N.SqeError):
        hvec.search_hybrid(hlex, q[:2], [[1]], 10, weights=[1.0, 1.0, 0.0])   # the lexical weight out of range


# ------------------------------------------------------------------------------ retrieval layer and shim
PD = 64


@pytest.fixture(scope="module")
def pmc(pmc_dir):
    """60 chunks of the bundled PMC files, a synthetic vocab over them, random vectors."""
    import os

    from oracle import retrieval as R
    from oracle import wordpiece as WP
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    docs = R.corpus_docs(pmc_dir, files=sorted(os.listdir(pmc_dir))[:6])[:60]
    toks = WP.synthetic_vocab([d["text"] for d in docs], size=1500)
    x = np.random.default_rng(41).standard_normal((len(docs), PD)).astype(np.float32)
    return docs, WordPieceTokenizer(vocab_text="\n".join(toks) + "\n"), x


def live_reference(idx, analyzer):
    rows = [r for r, s in enumerate(idx.sources) if s is not None]
    return LR.LexRef(rows, analyzer.analyze([idx.sources[r]["text"] for r in rows]), analyzer.n_terms)


def test_indexer_search_text_and_hybrid(ctx, pmc, tmp_path):
    from semantic_query_engine_amd import retrieval as RT
    docs, tok, x = pmc
    client = RT.GpuSearchClient(ctx, dim=PD)
    ix = RT.OpenSearchIndexer(client, "pmc")
    ix.add_embeddings(x[:50], docs[:50])
    assert ix.search_text("patients", 5) == []                    # no analyzer: the error path of every search here
    RT.configure_analyzer(tok, max_len=2048)
    try:
        an, idx = RT._analyzer, client.index("pmc")
        words = docs[7]["text"].split()
        query = " ".join(words[3:9])

        def check_text(k=64):                                    # every hit: the index holds fewer documents
            score, ids, _ = live_reference(idx, an).search([an.query(query)], k)
            hits = ix.search_text(query, k)
            assert [(h["doc_id"], h["text"]) for h, _ in hits] == [(idx.sources[r]["doc_id"], idx.sources[r]["text"]) for r in ids[0] if r >= 0]
            assert [s for _, s in hits] == [float(s) for s in score[0] if np.isfinite(s)] and len(hits) > 0
            return ids[0]

        first = check_text()
        assert 7 in first.tolist() and idx.lex.info()["rebuilds"] == 1
        ix.add_embeddings(x[50:], docs[50:])                      # added rows are pushed by the next query
        check_text()
        assert len(idx.lex) == 60 and idx.lex.info()["rebuilds"] == 2
        # an overwrite changes a text, a delete removes one: both reach the lexical index
        RT._commit_documents(idx, x[7:8], [{"doc_id": docs[7]["doc_id"], "text": "nothing of the kind"}], lambda i, d: f"{docs[7]['doc_id']}_7")
        client.delete(index="pmc", id=f"{docs[9]['doc_id']}_9")
        after = check_text()
        assert 9 not in after.tolist() and len(idx.lex) == 59 and idx.lex.info()["rebuilds"] == 3
        # hybrid: the library's own two lists through the reference
        q = x[20:21] + 0.1
        fusion = {"rank_constant": 10, "window": 16, "weights": [1.0, 2.0]}
        hits = ix.search_hybrid(q, query, 8, fusion=fusion)
        cos, ids = idx.vectors.search(q, 16)
        ls, li = idx.lex.search([an.query(query)], 16)
        fused, want, _c, _b = LR.hybrid(cos, ids, [0, 1], ls, li, 8, [1.0, 2.0], 10)
        assert [h["text"] for h, _ in hits] == [idx.sources[r]["text"] for r in want[0]]
        assert [s for _, s in hits] == [float(v) for v in fused[0]]
        # the lexical index is not saved: a loaded index rebuilds it from the docstore
        client.save_index("pmc", str(tmp_path))
        other = RT.GpuSearchClient(ctx, dim=PD)
        assert other.load_index("pmc", str(tmp_path))
        assert RT.OpenSearchIndexer(other, "pmc").search_text(query, 10) == ix.search_text(query, 10)
    finally:
        RT.configure_analyzer(None)


def test_shim_match_and_hybrid_end_to_end(ctx, pmc):
    import json

    from fastapi.testclient import TestClient

    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim
    docs, tok, x = pmc
    RT.configure_analyzer(tok, max_len=2048)
    try:
        an = RT._analyzer
        client = RT.GpuSearchClient(ctx, dim=PD)
        query = " ".join(docs[12]["text"].split()[2:8])
        with TestClient(shim.create_app(client, None, PD)) as c:
            assert c.put("/pmc", json={}).status_code == 200
            lines = []
            for i, d in enumerate(docs):
                lines.append(json.dumps({"index": {"_index": "pmc", "_id": f"c{i}"}}))
                lines.append(json.dumps({"doc_id": d["doc_id"], "text": d["text"], "embedding": x[i].tolist()}))
            assert c.post("/_bulk", content=("\n".join(lines) + "\n").encode()).json()["errors"] is False
            idx = client.index("pmc")
            r = c.post("/pmc/_search", json={"size": 64, "query": {"match": {"text": {"query": query}}}})
            assert r.status_code == 200, r.text
            score, ids, _ = live_reference(idx, an).search([an.query(query)], 64)
            hits = r.json()["hits"]["hits"]
            assert [h["_id"] for h in hits] == [f"c{i}" for i in ids[0] if i >= 0] and "c12" in [h["_id"] for h in hits]
            assert [h["_score"] for h in hits] == [float(s) for s in score[0] if np.isfinite(s)]
            # an overwrite through _bulk reaches the lexical index
            line = [json.dumps({"index": {"_index": "pmc", "_id": "c12"}}), json.dumps({"doc_id": "x", "text": "other words", "embedding": x[12].tolist()})]
            assert c.post("/_bulk", content=("\n".join(line) + "\n").encode()).json()["errors"] is False
            r = c.post("/pmc/_search", json={"size": 64, "query": {"match": {"text": query}}})
            score, ids, _ = live_reference(idx, an).search([an.query(query)], 64)
            assert [h["_id"] for h in r.json()["hits"]["hits"]] == [f"c{i}" for i in ids[0] if i >= 0]
            # hybrid with a match beside two knn sub-queries
            subs = [{"knn": {"embedding": {"vector": x[3].tolist(), "k": 6}}}, {"match": {"text": query}},
                    {"knn": {"embedding": {"vector": x[30].tolist(), "k": 6}}}]
            body = {"size": 6, "query": {"hybrid": {"queries": subs}}, "ext": {"fusion": {"window": 12, "weights": [1.0, 3.0, 0.5]}}}
            r = c.post("/pmc/_search", json=body)
            assert r.status_code == 200, r.text
            cos, vid = idx.vectors.search(x[[3, 30]], 12)
            ls, li = idx.lex.search([an.query(query)], 12)
            fused, want, wcos, bm = LR.hybrid(cos, vid, [0, 2], ls, li, 6, [1.0, 0.5, 3.0], 60)
            hits = r.json()["hits"]["hits"]
            assert [h["_id"] for h in hits] == [f"c{i}" for i in want[0]]
            assert [h["fields"]["_fused"][0] for h in hits] == [float(v) for v in fused[0]]
            assert [h["fields"].get("_bm25", [None])[0] for h in hits] == [float(v) if np.isfinite(v) else None for v in bm[0]]
            assert c.post("/pmc/_search", json={"query": {"match": {"text": {"query": query, "operator": "and"}}}}).status_code == 400
    finally:
        RT.configure_analyzer(None)


def test_hybrid_invalid_arguments_write_nothing(hdata, hvec, hlex):
    from semantic_query_engine_amd import _native as N
    lib = N.load()
    q = near(hdata, [1, 2], 6)
    off = np.array([0, 2], np.int64)
    outs = [np.full((1, 4), 77.0, np.float32), np.full((1, 4), 77, np.int64), np.full((1, 4), 77.0, np.float32), np.full((1, 4), 77.0, np.float32)]

    def call(terms, k, n, c, weights):
        qoff, qterms = flat([terms])
        w = None if weights is None else np.asarray(weights, np.float32)
        return lib.sqe_index_search_hybrid(hvec.handle, hlex.handle, q.ctypes.data, 1, off.ctypes.data, qoff.ctypes.data, qterms.ctypes.data,
                                           k, n, c, None if w is None else w.ctypes.data, 0, outs[0].ctypes.data, outs[1].ctypes.data,
                                           outs[2].ctypes.data, outs[3].ctypes.data)

    for args in (([T], 4, 0, 60, None), ([1] * 65, 4, 0, 60, None), ([1], 0, 0, 60, None), ([1], 257, 0, 60, None), ([1], 4, 3, 60, None),
                 ([1], 4, 0, 0, None), ([1], 4, 0, 60, [1.0, 1.0, float("nan")]), ([1], 4, 0, 60, [1.0, 65.0, 1.0])):
        assert call(*args) == -1, args
        assert all(np.all(o == 77) for o in outs), args
    assert call([1], 4, 0, 60, None) == 0 and outs[1][0, 0] >= 0
