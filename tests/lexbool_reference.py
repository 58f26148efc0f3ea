"""NumPy reference of the boolean lexical queries (include/sqe.h: sqe_lex_search_bool, sqe_lex_match), written from the
definition on top of tests/lex_reference.py's impacts.  Dense: every query is evaluated against every document.

  occurrence j holds in d  iff  tf(t_j, d) >= 1
  d matches q  iff  every MUST / FILTER occurrence holds, no MUST_NOT occurrence holds and at least m SHOULD occurrences hold
                    (counted per occurrence), m = min_should with a MUST / FILTER occurrence in the query, else max(1, min_should)
  a query without a SHOULD, MUST or FILTER occurrence matches nothing
  score_int = the uint64 sum of I(t_j, d) over the SHOULD and MUST occurrences (I is 0 where the occurrence does not hold)
Ranking: lexsort on (id, -score_int) over the matches -- a match with score_int 0 is a hit --, padding (-inf, -1).
The match set: the matching ids ascending."""
import numpy as np

SHOULD, MUST, FILTER, MUST_NOT = 0, 1, 2, 3


class LexBoolRef:
    def __init__(self, ref):
        self.ref = ref                                            # a lex_reference.LexRef

    def evaluate(self, query, roles, min_should: int = 0):
        """-> (matches [N] bool, score_int [N] uint64) of one query."""
        r = self.ref
        assert len(query) == len(roles) <= 64 and 0 <= int(min_should) <= 64
        required = np.ones(r.N, bool)
        denied = np.zeros(r.N, bool)
        should = np.zeros(r.N, np.int64)
        score = np.zeros(r.N, np.uint64)
        n_required = n_should = 0
        for t, role in zip(query, roles):
            holds = r.tf[:, int(t)] >= 1
            assert role in (SHOULD, MUST, FILTER, MUST_NOT)
            if role in (MUST, FILTER):
                required &= holds
                n_required += 1
            if role == MUST_NOT:
                denied |= holds
            if role == SHOULD:
                should += holds
                n_should += 1
            if role in (SHOULD, MUST):
                score += r.impact[:, int(t)]
        m = int(min_should) if n_required else max(1, int(min_should))
        matches = required & ~denied & (should >= m)
        if n_required + n_should == 0:
            matches[:] = False
        return matches, score

    def search(self, queries, roles, k: int, min_should=None):
        """-> (scores [B, k] float32, ids [B, k] int64, score_int [B, k] uint64, hit [B, k] bool)"""
        r = self.ref
        B = len(queries)
        score = np.full((B, k), -np.inf, np.float32)
        ids = np.full((B, k), -1, np.int64)
        sint = np.zeros((B, k), np.uint64)
        for i in range(B):
            matches, s = self.evaluate(queries[i], roles[i], 0 if min_should is None else min_should[i])
            hit = np.nonzero(matches)[0]
            order = hit[np.lexsort((r.ids[hit], -s[hit].astype(np.int64)))][:k]
            t = order.shape[0]
            sint[i, :t] = s[order]
            score[i, :t] = (s[order].astype(np.float64) * 2.0 ** -16).astype(np.float32)
            ids[i, :t] = r.ids[order]
        return score, ids, sint

    def match(self, queries, roles, min_should=None, cap=None):
        """-> (counts [B] int64, ids [B, cap] int64 ascending, -1 padded, rows: the list of each query's matching rows)"""
        r = self.ref
        B = len(queries)
        rows = [np.nonzero(self.evaluate(queries[i], roles[i], 0 if min_should is None else min_should[i])[0])[0] for i in range(B)]
        counts = np.array([x.shape[0] for x in rows], np.int64).reshape(B)
        if cap is None:
            cap = int(counts.max(initial=0))
        ids = np.full((B, cap), -1, np.int64)
        for i, x in enumerate(rows):
            n = min(cap, x.shape[0])
            ids[i, :n] = np.sort(r.ids[x])[:n]
        return counts, ids, rows
