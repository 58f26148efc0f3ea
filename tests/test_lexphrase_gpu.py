"""Phrase queries (sqe_lex_put_ordered, sqe_lex_search_phrase, sqe_lex_match_phrase; lexical.hip) and phrase match sets as k-NN
filters.  GPU only.

Everything is bit for bit against tests/lexphrase_reference.py: ids, float scores, counts and match ids.  One corpus serves all
tests: 44 terms (so phrases repeat by chance), 16,384 + 37 documents (two chunks, the second nearly empty), lengths 0..40 with a
few of 65..300 (the lanes of a wave stride more than once), one document in eight put as a bag.  The hand-placed documents aim
at the start positions whose tail would run into the NEXT document's sequence; each such document holds every term of its
phrase, so the candidate map cannot hide a verification that reads past the end."""
import numpy as np
import pytest

from . import lexphrase_reference as PR
from .lexbool_reference import FILTER, MUST, MUST_NOT, SHOULD

pytestmark = pytest.mark.gpu

T = 44                                  # terms 0..39 random; A, B, X only where planted; Z in no document
A, B, X, Z = 40, 41, 42, 43
N_DOCS = 16_384 + 37
C = 16_384                              # rows of a chunk (checked against sqe_lex_info)
PLANTED = {
    100: [B, 1, 2, A], 101: [B, 3],                       # `A B`: 100 ends with A, 101 begins with B; 100 holds both terms
    C - 1: [B, 7, A], C: [B, 4, 4],                       # the same pair across the chunk boundary
    200: [1, 2, 3, A, B],                                 # `A B` at the last two positions
    300: [A, X, B], 301: [B, 0, 1],                       # L = dl: `A X B`; L = dl + 1: `A X B B` would need 301's first word
    400: [X, X, X], 401: [X, 5],                          # `X X` in `X X X`: pf = 2 (3 if the window left the document)
    500: [A, B, A, B, A],                                 # `A B A`: a repeated term, overlapping: pf = 2
    600: [A, B, 6, X],                                    # put as a BAG: holds A, B and X, but no phrase
    700: [6, A, B, 9, A, B],                              # pf = 2 apart
}
BAG_ROWS = {600}


def same_bits(a, b):
    return all(u.shape == w.shape and u.dtype == w.dtype and np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8))
               for u, w in zip(a, b))


def flat(bags, dtype=np.int32):
    lens = np.array([len(b) for b in bags], np.int64)
    off = np.zeros(lens.shape[0] + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    terms = np.concatenate([np.asarray(b, dtype) for b in bags]) if off[-1] else np.zeros(0, dtype)
    return off, terms.astype(dtype)


def make_corpus(n=N_DOCS, seed=3):
    """ids 5 + 2 i (row = i), documents over terms 0..39 with probability ~ 1 / (t + 3), ordered flags."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(3, 43)
    p /= p.sum()
    lens = rng.integers(0, 41, n)
    lens[rng.choice(n, 24, replace=False)] = rng.integers(65, 301, 24)
    lens[n - 1] = 70                                           # a long one in the small second chunk
    draws = rng.choice(40, int(lens.sum()), p=p).astype(np.int32)
    docs = [a for a in np.split(draws, np.cumsum(lens)[:-1])]
    ordered = rng.integers(0, 8, n) != 0
    for row, seq in PLANTED.items():
        docs[row] = np.array(seq, np.int32)
        ordered[row] = row not in BAG_ROWS
    return 5 + 2 * np.arange(n, dtype=np.int64), docs, ordered


def put_all(lex, ids, docs, ordered, rows, step=5000):
    """The rows in the given order, the ordered ones through the ordered put."""
    rows = np.asarray(rows)
    for lo in range(0, rows.shape[0], step):
        part = rows[lo:lo + step]
        for flag in (True, False):
            sel = [int(j) for j in part if bool(ordered[j]) == flag]
            if sel:
                lex.put(ids[sel], flat([docs[j] for j in sel]), ordered=flag)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def world(ctx):
    from semantic_query_engine_amd import LexicalIndex
    ids, docs, ordered = make_corpus()
    lex = LexicalIndex(ctx, T)
    assert lex.info()["chunk_rows"] == C
    put_all(lex, ids, docs, ordered, np.random.default_rng(1).permutation(N_DOCS))
    ref = PR.LexPhraseRef(ids, docs, ordered, T)
    assert ref.ref.df[Z] == 0 and 0.1 < 1.0 - ordered.mean() < 0.15
    return lex, ref, ids, docs, ordered


def window(docs, ordered, rng, L):
    """L consecutive terms of a random ordered document that is long enough."""
    rows = [r for r in range(N_DOCS) if ordered[r] and len(docs[r]) >= L and r not in PLANTED]
    r = int(rng.choice(rows))
    p = int(rng.integers(0, len(docs[r]) - L + 1))
    return [int(t) for t in docs[r][p:p + L]]


def cases(docs, ordered):
    """name -> (clauses, roles, min_should)"""
    rng = np.random.default_rng(9)
    w = lambda L: window(docs, ordered, rng, L)                  # noqa: E731
    common2 = [0, 0]                                             # the two most common terms next to each other
    out = {
        "next_document": ([[A, B]], [MUST], 0),                  # 1, 2, 9: 200, 500, 700 -- not 100, C - 1, 600
        "ends_document": ([[3, A, B]], [MUST], 0),               # 2: 200
        "whole_document": ([[A, X, B]], [MUST], 0),              # 3: 300
        "longer_than_document": ([[A, X, B, B]], [MUST], 0),     # 4: nothing
        "overlap": ([[X, X]], [MUST], 0),                        # 5: 400 with pf = 2
        "repeated_term": ([[A, B, A]], [SHOULD], 0),             # 6: 500 with pf = 2
        "df0": ([[A, Z]], [SHOULD], 0),                          # 8
        "df0_must_not": ([[A], [A, Z]], [SHOULD, MUST_NOT], 0),
        "bag_only": ([[A, B], [X]], [SHOULD, SHOULD], 0),        # 9: 600 through the term, 200 .. through the phrase
        "bag_only_terms": ([[A], [B], [A, B]], [MUST, MUST, MUST_NOT], 0),   # the terms hold in 100, 300, 600 and C - 1; the phrase does not
        "L2": ([w(2)], [MUST], 0), "L3": ([w(3)], [MUST], 0), "L16": ([w(16)], [MUST], 0), "L64": ([w(64)], [MUST], 0),
        "L64_should": ([w(64)], [SHOULD], 0),
        "common": ([common2], [MUST], 0),
        "should": ([w(2), w(2)], [SHOULD, SHOULD], 0),
        "filter_only": ([w(2)], [FILTER], 0),                    # scores 0.0
        "filter_then_should": ([common2, [1]], [FILTER, SHOULD], 0),     # zero-score hits rank last
        "must_not": ([[0], common2], [SHOULD, MUST_NOT], 0),
        "must_not_only": ([common2], [MUST_NOT], 0),
        "ms2": ([[0, 1], [1, 0], [2]], [SHOULD, SHOULD, SHOULD], 2),     # two phrases and a term
        "ms2_filter": ([[5], [0, 1], [1, 0], [2]], [FILTER, SHOULD, SHOULD, SHOULD], 2),
        "ms3": ([[0, 1], [1, 0], [2]], [SHOULD, SHOULD, SHOULD], 3),
        "ms4": ([[0, 1], [1, 0], [2]], [SHOULD, SHOULD, SHOULD], 4),     # more than there are
        "must_with_should": ([[0, 1], [2], [5]], [MUST, SHOULD, SHOULD], 0),
        "must_with_should_ms1": ([[0, 1], [2], [1, 2]], [MUST, SHOULD, SHOULD], 1),
        "repeated_clause": ([[0, 1], [0, 1], [3]], [SHOULD, SHOULD, SHOULD], 2),
        "two_must": ([[0, 1], [2, 0]], [MUST, MUST], 0),
        "term_then_phrase": ([[A], [1, 2]], [MUST, MUST], 0),    # the required term first: 100 and 200
        "mixed": ([[0, 1], [4], [2, 3], [0, 0, 0]], [MUST, FILTER, SHOULD, MUST_NOT], 0),
        "empty": ([], [], 0),
    }
    for i in range(12):                                          # random windows in random roles
        n = int(rng.integers(1, 4))
        roles = [int(x) for x in rng.choice([SHOULD, SHOULD, MUST, FILTER, MUST_NOT], n)]
        out[f"random{i}"] = ([w(int(rng.integers(1, 5))) for _ in range(n)], roles, int(rng.integers(0, 2)))
    return out


@pytest.fixture(scope="module")
def batch(world):
    """The cases as one batch, the reference's dense answer and the coverage the corpus has to give (reference only)."""
    lex, ref, ids, docs, ordered = world
    cs = cases(docs, ordered)
    names = list(cs)
    Q, R, M = [cs[n][0] for n in names], [cs[n][1] for n in names], [cs[n][2] for n in names]
    counts, _ids, rows = ref.match(Q, R, M, cap=0)
    by = dict(zip(names, range(len(names))))
    hit = lambda n: rows[by[n]].tolist()                        # noqa: E731
    assert hit("next_document") == [200, 500, 700] and ref.pf([A, B])[[100, C - 1, 600]].tolist() == [0, 0, 0]
    assert ref.pf([A, B])[[200, 500, 700]].tolist() == [1, 2, 2]
    assert hit("ends_document") == [200] and hit("whole_document") == [300] and hit("longer_than_document") == []
    assert hit("overlap") == [400] and ref.pf([X, X])[400] == 2 and hit("repeated_term") == [500] and ref.pf([A, B, A])[500] == 2
    assert hit("df0") == [] and hit("bag_only") == [200, 300, 400, 401, 500, 600, 700] and hit("bag_only_terms") == [100, 300, 600, C - 1]
    assert hit("term_then_phrase") == [100, 200]
    for n in ("L2", "L3", "L16", "L64", "ms2", "ms2_filter", "ms3", "must_with_should", "must_with_should_ms1", "two_must", "mixed",
              "repeated_clause", "filter_only", "should"):
        assert counts[by[n]] > 0, n
    for n in ("ms4", "must_not_only", "empty"):
        assert counts[by[n]] == 0, n
    assert counts[by["common"]] > 1000 and {int(r) // C for r in rows[by["common"]]} == {0, 1}
    assert 0 < counts[by["must_not"]] < int((ref.ref.tf[:, 0] > 0).sum())
    assert counts[by["ms3"]] < counts[by["ms2"]] and counts[by["ms2_filter"]] < counts[by["ms2"]]
    assert max(ref.pf([0, 0]).max(), ref.pf([0, 1]).max()) >= 3                # phrase frequencies above 1 are scored
    assert max(len(d) for d in docs) > 128                                     # more than two strides of a wave
    return names, Q, R, M, counts


def check_search(lex, ref, Q, R, M, k):
    want_s, want_i, sint = ref.search(Q, R, k, M)
    assert int(sint.max(initial=0)) < 1 << 27
    got = lex.search_phrase(Q, R, k, M)
    assert np.array_equal(got[1], want_i), [(b, got[1][b, :6], want_i[b, :6]) for b in range(len(Q)) if not np.array_equal(got[1][b], want_i[b])][:3]
    assert same_bits(got, (want_s, want_i)), [(b, got[0][b, :4], want_s[b, :4]) for b in range(len(Q)) if not np.array_equal(got[0][b], want_s[b])][:3]
    return got


@pytest.mark.parametrize("k", [1, 10, 256])
def test_search_phrase_matches_reference(world, batch, k):
    lex, ref, ids, docs, ordered = world
    names, Q, R, M, counts = batch
    got = check_search(lex, ref, Q, R, M, k)
    if k == 256:
        at = names.index("filter_only")                            # a FILTER-only phrase scores 0.0
        n = int(counts[at])
        fin = np.isfinite(got[0][at])
        assert fin.sum() == min(n, 256) > 0 and np.all(got[0][at][fin] == 0.0) and np.all(got[1][at][fin] >= 0)
        at = names.index("overlap")                                # pf = 2 is what the score holds
        want = ref.impact([X, X])[400]
        assert got[1][at, 0] == ids[400] and got[0][at, 0] == np.float32(np.float64(want) * 2.0 ** -16)
        f = np.float64(1.0)
        one = max(1.0, np.rint(np.float64(ref.idf_of([X, X])) * (f / (f + ref.ref.norm[400])) * 65536.0))
        assert int(want) != int(one)                               # a pf of 1 would have scored differently
    if k == 10:
        at = names.index("filter_then_should")                     # zero-score hits rank after every positive score
        s, i = lex.search_phrase([Q[at]], [R[at]], 256, [M[at]])
        fin = s[0][np.isfinite(s[0])]
        assert fin[0] > 0.0 and np.all(np.diff(fin) <= 0)


def test_match_phrase_sets(world, batch):
    lex, ref, ids, docs, ordered = world
    names, Q, R, M, counts = batch
    got_c, got_i = lex.match_phrase(Q, R, M, cap=0)
    assert np.array_equal(got_c, counts) and got_i.shape == (len(Q), 0)
    assert np.array_equal(lex.count_phrase(Q, R, M), counts)
    for cap in (1, 37, 1000):
        want_c, want_i, _ = ref.match(Q, R, M, cap=cap)
        got_c, got_i = lex.match_phrase(Q, R, M, cap=cap)
        assert np.array_equal(got_c, counts) and np.array_equal(got_i, want_i), cap
    got_c, got_i = lex.match_phrase(Q, R, M)                       # cap = None: the largest count
    assert got_i.shape[1] == counts.max() and np.array_equal(got_i, ref.match(Q, R, M)[1])


def test_clauses_of_one_term_are_search_bool(world):
    """Every clause of length 1: bit for bit sqe_lex_search_bool and sqe_lex_match."""
    lex, ref, ids, docs, ordered = world
    rng = np.random.default_rng(41)
    Q, R, M = [], [], []
    for b in range(64):
        n = int(rng.integers(0, 7))
        Q.append([int(t) for t in rng.integers(0, T, n)])
        R.append([int(x) for x in rng.choice([SHOULD, SHOULD, MUST, FILTER, MUST_NOT], n)])
        M.append(int(rng.integers(0, 3)))
    QC = [[[t] for t in q] for q in Q]
    for k in (1, 10, 256):
        assert same_bits(lex.search_phrase(QC, R, k, M), lex.search_bool(Q, R, k, M))
    assert same_bits(lex.search_phrase(QC, R, 10), lex.search_bool(Q, R, 10))
    for cap in (0, 50):
        assert same_bits(lex.match_phrase(QC, R, M, cap=cap), lex.match(Q, R, M, cap=cap))


def test_batch_independence(world, batch):
    lex, ref, ids, docs, ordered = world
    names, Q, R, M, counts = batch
    pick = [j % len(names) for j in range(64)]
    Q64, R64, M64 = [Q[b] for b in pick], [R[b] for b in pick], [M[b] for b in pick]
    whole = lex.search_phrase(Q64, R64, 10, M64)
    mc, mi = lex.match_phrase(Q64, R64, M64, cap=50)
    for j in range(0, 64, 3):
        one = lex.search_phrase([Q64[j]], [R64[j]], 10, [M64[j]])
        assert same_bits((one[0][0], one[1][0]), (whole[0][j], whole[1][j])), names[pick[j]]
        oc, oi = lex.match_phrase([Q64[j]], [R64[j]], [M64[j]], cap=50)
        assert oc[0] == mc[j] and np.array_equal(oi[0], mi[j]), names[pick[j]]


def live_sequences(lex):
    """(seq_off, seq, dl) of the device index."""
    from semantic_query_engine_amd import engine as E
    n = lex.info()["documents"]
    off = lex.state_read(E.LEX_SEQ_OFF, np.int64, n + 1)
    return off, lex.state_read(E.LEX_SEQ, np.int32, int(off[-1])), lex.state_read(E.LEX_DL, np.int64, n)


def test_churn_equals_a_fresh_index(ctx, world, batch):
    """Ordered replaced by bag, bag by ordered, deletions and enough re-puts to compact the logs: the index answers like a
    fresh one of the live documents, and the device sequences are the live ones in id order."""
    from semantic_query_engine_amd import LexicalIndex
    _lex, _ref, ids, docs, ordered = world
    names, Q, R, M, _counts = batch
    n = 3000
    rng = np.random.default_rng(8)
    lex = LexicalIndex(ctx, T)
    put_all(lex, ids, docs, ordered, np.arange(n))
    lex.count_phrase(Q, R, M)                                      # built once
    new_docs, new_ordered = list(docs[:n]), ordered[:n].copy()
    to_bag = rng.choice(np.nonzero(new_ordered)[0], 200, replace=False)
    to_seq = np.nonzero(~new_ordered)[0][:150]
    new_ordered[to_bag] = False
    new_ordered[to_seq] = True
    changed = rng.choice(n, 300, replace=False)
    for j in changed:
        new_docs[j] = docs[(int(j) * 7 + 1) % n][::-1].copy()
    gone = rng.choice(n, 700, replace=False)
    lex.delete(ids[gone])
    touched = np.setdiff1d(np.union1d(np.union1d(to_bag, to_seq), changed), gone)
    put_all(lex, ids, new_docs, new_ordered, touched)
    live = np.setdiff1d(np.arange(n), gone)
    # lex_rebuild compacts the logs when log_term holds more than 2 P + 1024 entries or log_seq more than 2 S + 1024 words, P
    # and S being the live postings and sequence words.  No rebuild ran since the first one, so at the rebuild after the first
    # round below the logs hold the 3000 first documents, the touched ones and the live ones once more: the compaction runs
    # there (the deleted and replaced entries alone exceed 1024) and rewrites every seq_off; the second round doubles the
    # compacted logs (not above the bound), the third crosses it again.  The bound is restated here so that a corpus or a
    # threshold that no longer reaches the compaction fails this test instead of passing without it.
    posts = lambda dd, rows: sum(len(np.unique(dd[j])) for j in rows)                                   # noqa: E731
    words = lambda dd, oo, rows: sum(len(dd[j]) for j in rows if oo[j])                                 # noqa: E731
    P, S = posts(new_docs, live), words(new_docs, new_ordered, live)
    assert posts(docs, range(n)) + posts(new_docs, touched) + P > 2 * P + 1024
    assert words(docs, ordered, range(n)) + words(new_docs, new_ordered, touched) + S > 2 * S + 1024
    assert 3 * P > 2 * P + 1024 and 3 * S > 2 * S + 1024
    for _ in range(3):                                             # the dead entries now outweigh the live ones: the logs compact
        put_all(lex, ids, new_docs, new_ordered, live)
        lex.count_phrase(Q[:1], R[:1], M[:1])
    put_all(lex, ids, new_docs, new_ordered, live[:50])            # and the compacted log takes puts again
    fresh = LexicalIndex(ctx, T)
    put_all(fresh, ids, new_docs, new_ordered, live)
    assert same_bits(lex.search_phrase(Q, R, 10, M), fresh.search_phrase(Q, R, 10, M))
    assert same_bits(lex.match_phrase(Q, R, M, cap=300), fresh.match_phrase(Q, R, M, cap=300))
    small = PR.LexPhraseRef(ids[live], [new_docs[j] for j in live], new_ordered[live], T)
    check_search(fresh, small, Q, R, M, 10)
    assert np.array_equal(fresh.match_phrase(Q, R, M, cap=300)[1], small.match(Q, R, M, cap=300)[1])
    for ix in (lex, fresh):
        off, seq, dl = live_sequences(ix)
        want = [new_docs[j] if new_ordered[j] else None for j in live]         # ids ascend with j
        assert off[-1] == sum(len(s) for s in want if s is not None) == seq.shape[0]
        at = 0
        for r, s in enumerate(want):
            if s is None:
                assert off[r] == -1
            else:
                assert off[r] == at and dl[r] == len(s) and np.array_equal(seq[at:at + len(s)], s)
                at += len(s)
    lex.close()
    fresh.close()


def test_an_index_without_ordered_puts_is_unchanged(ctx, world, batch):
    """The same terms put as bags only: the same info, the same answers of the existing calls, no sequences on the device."""
    from semantic_query_engine_amd import LexicalIndex
    from semantic_query_engine_amd import _native as N
    from semantic_query_engine_amd import engine as E
    _lex, _ref, ids, docs, ordered = world
    names, Q, R, M, _counts = batch
    n = 2500
    bags = LexicalIndex(ctx, T)
    bags.put(ids[:n], flat(docs[:n]))
    seqs = LexicalIndex(ctx, T)
    seqs.put(ids[:n], flat(docs[:n]), ordered=True)
    rng = np.random.default_rng(2)
    plain = [[int(t) for t in rng.integers(0, T, int(rng.integers(0, 6)))] for _ in range(40)]
    roles = [[int(x) for x in rng.choice([SHOULD, MUST, FILTER, MUST_NOT], len(q))] for q in plain]
    assert same_bits(bags.search(plain, 10), seqs.search(plain, 10))
    assert same_bits(bags.search_bool(plain, roles, 10), seqs.search_bool(plain, roles, 10))
    assert same_bits(bags.match(plain, roles, cap=40), seqs.match(plain, roles, cap=40))
    a, b = bags.info(), seqs.info()
    for key in ("documents", "postings", "n_terms", "chunk_rows", "chunks", "rebuilds", "avgdl"):
        assert a[key] == b[key], key
    assert bags.state_read(E.LEX_SEQ_OFF, np.int64, 0).shape == (0,) and bags.state_read(E.LEX_SEQ, np.int32, 0).shape == (0,)
    out = np.zeros(1, np.int64)
    assert N.load().sqe_lex_state_read(bags.handle, E.LEX_SEQ_OFF, 0, out.ctypes.data, 8) == -1      # it holds nothing
    assert seqs.state_read(E.LEX_SEQ_OFF, np.int64, n + 1)[-1] == sum(len(d) for d in docs[:n])
    # phrases on the bags: none holds; one-term clauses answer as search_bool
    ref = PR.LexPhraseRef(ids[:n], docs[:n], np.zeros(n, bool), T)
    check_search(bags, ref, Q, R, M, 10)
    assert bags.count_phrase([[[0, 0]], [[0], [0, 1]]], [[MUST], [SHOULD, SHOULD]]).tolist() == [0, int((ref.ref.tf[:, 0] > 0).sum())]
    check_search(seqs, PR.LexPhraseRef(ids[:n], docs[:n], np.ones(n, bool), T), Q, R, M, 10)
    bags.close()
    seqs.close()


def test_invalid_arguments_write_nothing(world):
    from semantic_query_engine_amd import _native as N
    lex = world[0]
    lib = N.load()
    score, ids = np.full((2, 4), 77.0, np.float32), np.full((2, 4), 77, np.int64)
    cnt, mid = np.full(2, 77, np.int64), np.full((2, 4), 77, np.int64)

    def call(qoff, coff, terms, roles, M, k=4, cap=4, null_ids=False):
        qoff, coff = np.asarray(qoff, np.int64), np.asarray(coff, np.int64)
        terms, roles = np.asarray(terms, np.int32), np.asarray(roles, np.uint8)
        ms = None if M is None else np.asarray(M, np.int32)
        common = (lex.handle, qoff.ctypes.data, coff.ctypes.data, terms.ctypes.data, roles.ctypes.data, None if ms is None else ms.ctypes.data,
                  qoff.shape[0] - 1)
        return (lib.sqe_lex_search_phrase(*common, k, score.ctypes.data, ids.ctypes.data),
                lib.sqe_lex_match_phrase(*common, cap, cnt.ctypes.data, None if null_ids else mid.ctypes.data))

    ok = dict(qoff=[0, 2, 3], coff=[0, 2, 3, 5], terms=[1, 2, 3, 0, 1], roles=[MUST, SHOULD, FILTER], M=[0, 0])
    bad = [dict(ok, roles=[MUST, 4, FILTER]),                                     # what the boolean calls refuse: a role above 3,
           dict(ok, M=[0, -1]), dict(ok, M=[65, 0]),                              # min_should outside [0, 64],
           dict(ok, terms=[1, T, 3, 0, 1]), dict(ok, terms=[1, -1, 3, 0, 1]),     # a term out of range
           dict(ok, coff=[0, 2, 2, 5]),                                           # an empty clause
           dict(ok, coff=[1, 2, 3, 5]), dict(ok, qoff=[1, 2, 3]),                 # tables that do not start at 0
           dict(ok, coff=[0, 3, 2, 5]), dict(ok, qoff=[0, 3, 2]),                 # ... or decrease
           dict(qoff=[0, 2, 3], coff=[0, 33, 65, 66], terms=[1] * 66, roles=[MUST, SHOULD, FILTER], M=None)]      # 65 occurrences in a query
    for kw in bad:
        assert call(**kw) == (-1, -1), kw
    assert call(**ok, k=0, cap=-1) == (-1, -1)
    assert call(**ok, k=257, null_ids=True) == (-1, -1)
    assert np.all(score == 77) and np.all(ids == 77) and np.all(cnt == 77) and np.all(mid == 77)
    assert call(**ok) == (0, 0) and not np.any(cnt == 77) and not np.any(ids == 77)
    assert call(qoff=[0, 2], coff=[0, 32, 64], terms=[1] * 64, roles=[MUST, SHOULD], M=None) == (0, 0)      # 64 occurrences are served


def test_no_queries_and_empty_index(ctx):
    from semantic_query_engine_amd import LexicalIndex
    lex = LexicalIndex(ctx, T)
    for _ in range(2):
        score, ids = lex.search_phrase([], [], 5)
        assert score.shape == (0, 5) and ids.shape == (0, 5)
        counts, mids = lex.match_phrase([], [], cap=3)
        assert counts.shape == (0,) and mids.shape == (0, 3)
        score, ids = lex.search_phrase([[[1, 2]]], [[MUST]], 5)
        counts, mids = lex.match_phrase([[[1, 2]], [[2, 1]], [[2]]], [[FILTER], [SHOULD], [SHOULD]], cap=3)
        if len(lex) == 0:
            assert np.all(np.isneginf(score)) and np.all(ids == -1) and counts.tolist() == [0, 0, 0] and np.all(mids == -1)
        else:
            assert ids[0].tolist() == [4, -1, -1, -1, -1] and counts.tolist() == [1, 1, 3] and mids.tolist() == [[4, -1, -1], [9, -1, -1], [4, 6, 9]]
        lex.put([4, 9], [[1, 2], [2, 1, 1]], ordered=True)
        lex.put([6], [[2, 1, 2]])                                  # a bag: `1 2` and `2 1` do not hold
    lex.close()


def test_device_form_writes_device_memory(world, batch):
    import torch
    lex, ref, ids_, docs, ordered = world
    names, Q, R, M, counts = batch
    k, cap = 10, 20
    score = torch.empty((len(Q), k), dtype=torch.float32, device="cuda")
    ids = torch.empty((len(Q), k), dtype=torch.int64, device="cuda")
    cnt = torch.empty(len(Q), dtype=torch.int64, device="cuda")
    mid = torch.empty((len(Q), cap), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lex.search_phrase_device(Q, R, k, score.data_ptr(), ids.data_ptr(), M)
    lex.match_phrase_device(Q, R, M, cap, cnt.data_ptr(), mid.data_ptr())
    lex.ctx.synchronize()
    assert same_bits((score.cpu().numpy(), ids.cpu().numpy()), lex.search_phrase(Q, R, k, M))
    wc, wi = lex.match_phrase(Q, R, M, cap=cap)
    assert np.array_equal(cnt.cpu().numpy(), wc) and np.array_equal(mid.cpu().numpy(), wi)


# ------------------------------------------------------------------------------ retrieval layer and shim
PD = 64
VOCAB = ["aspirin", "fever", "pain", "brca1", "gene", "olaparib", "cancer", "risk", "metformin", "diabetes", "trial", "dose"]


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


def ph(text):
    return {"match_phrase": {"text": text}}


def m(text, **opts):
    return {"match": {"text": dict(query=text, **opts) if opts else text}}


def live_reference(idx, analyzer):
    rows = [r for r, s in enumerate(idx.sources) if s is not None]
    return PR.LexPhraseRef(rows, analyzer.analyze([idx.sources[r]["text"] for r in rows]), [True] * len(rows), analyzer.n_terms)


def test_indexer_phrases_as_knn_filters(ctx, toy):
    """search(query_emb, k, filter={"match_phrase": ...}) is VectorIndex.search over the reference's match ids, bit for bit."""
    from semantic_query_engine_amd import retrieval as RT
    docs, tok, x = toy
    client = RT.GpuSearchClient(ctx, dim=PD)
    ix = RT.OpenSearchIndexer(client, "toy")
    ix.add_embeddings(x, docs)
    RT.configure_analyzer(tok, max_len=256, positions=True)
    try:
        an, idx = RT._analyzer, client.index("toy")
        ref = live_reference(idx, an)
        q = x[17:18] + 0.05
        k = 12

        def ref_ids(clause):
            clauses, roles, ms = RT.text_clauses(clause)
            return ref.match([clauses], [roles], [ms])[1][0]

        def check(flt, allow):
            assert 0 < allow.shape[0] < len(docs)
            cos, ids = idx.vectors.search(q, k, filter_ids=allow)
            hits = ix.search(q, k, filter=flt)
            assert [h["text"] for h, _ in hits] == [idx.sources[r]["text"] for r in ids[0] if r >= 0] and len(hits) == min(k, allow.shape[0])
            bc, bi = ix.search_batch(np.concatenate([q, x[3:4]]), k, filters=[flt, None])
            assert same_bits((bc[0:1], bi[0:1]), (cos, ids)) and same_bits((bc[1:2], bi[1:2]), idx.vectors.search(x[3:4], k))

        phrase = ph("aspirin fever")
        a = ref_ids(phrase)
        words = [d["text"].split() for d in docs]
        assert a.tolist() == [r for r, w in enumerate(words) if any(w[i:i + 2] == ["aspirin", "fever"] for i in range(len(w)))]
        assert a.shape[0] < ref_ids(m("aspirin fever", operator="and")).shape[0]       # the order is what the phrase adds
        check(phrase, a)
        in_docs = np.array([r for r, d in enumerate(docs) if d["doc_id"] in ("d1", "d4", "d7")], np.int64)
        check({"bool": {"filter": [phrase, {"terms": {"doc_id": ["d1", "d4", "d7"]}}]}}, np.intersect1d(a, in_docs))
        check({"bool": {"must_not": [phrase]}}, np.setdiff1d(np.arange(len(docs)), a))          # the exclusion route
        assert ix.count_text(phrase) == a.shape[0]
        clause = {"bool": {"must": [ph("aspirin fever")], "should": [m("pain"), ph("fever aspirin")], "must_not": [m("dose")]}}
        clauses, roles, ms = RT.text_clauses(clause)
        score, ids, _ = ref.search([clauses], [roles], 20, [ms])
        hits = ix.search_text(clause, 20)
        assert [h["text"] for h, _ in hits] == [idx.sources[r]["text"] for r in ids[0] if r >= 0] and len(hits) > 1
        assert [s for _, s in hits] == [float(s) for s in score[0] if np.isfinite(s)]
    finally:
        RT.configure_analyzer(None)


def test_shim_phrases_end_to_end(ctx, toy):
    import json

    from fastapi.testclient import TestClient

    from semantic_query_engine_amd import retrieval as RT
    from semantic_query_engine_amd import shim
    docs, tok, x = toy
    RT.configure_analyzer(tok, max_len=256, positions=True)
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
            ref = live_reference(idx, an)
            clause = {"bool": {"must": [ph("aspirin fever")], "should": [m("pain")], "must_not": [ph("fever pain")]}}
            clauses, roles, ms = RT.text_clauses(clause)
            for query in (ph("aspirin fever"), clause):                   # _search: bare and inside a bool
                r = c.post("/toy/_search", json={"size": 50, "query": query})
                assert r.status_code == 200, r.text
                cl, ro, mm = RT.text_clauses(query)
                score, ids, _ = ref.search([cl], [ro], 50, [mm])
                hits = r.json()["hits"]["hits"]
                assert [h["_id"] for h in hits] == [f"c{i}" for i in ids[0] if i >= 0] and len(hits) > 1
                assert [h["_score"] for h in hits] == [float(s) for s in score[0] if np.isfinite(s)]
            n = int(ref.match([clauses], [roles], [ms], cap=0)[0][0])
            assert c.post("/toy/_count", json={"query": clause}).json()["count"] == n and len(hits) == min(n, 50)
            allow = ref.match([[an.analyze(["aspirin fever"])[0].tolist()]], [[MUST]], [0])[1][0]
            body = {"size": 8, "query": {"knn": {"embedding": {"vector": x[5].tolist(), "k": 8, "filter": ph("aspirin fever")}}}}
            r = c.post("/toy/_search", json=body)
            assert r.status_code == 200, r.text
            cos, vid = idx.vectors.search(x[5:6], 8, filter_ids=allow)
            assert [h["_id"] for h in r.json()["hits"]["hits"]] == [f"c{i}" for i in vid[0] if i >= 0]
            assert c.post("/toy/_search", json={"query": {"match_phrase": {"text": {"query": "aspirin fever", "slop": 2}}}}).status_code == 400
    finally:
        RT.configure_analyzer(None)
