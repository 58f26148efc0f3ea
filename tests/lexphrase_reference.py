"""NumPy reference of the phrase queries (include/sqe.h: sqe_lex_put_ordered, sqe_lex_search_phrase, sqe_lex_match_phrase),
written from the definition on top of tests/lex_reference.py's impacts and tests/lexbool_reference.py's rules.

A document is a bag, or a sequence whose bag is its multiset.  A query is a list of clauses, a clause a list of terms, one role
per clause.

  pf(c, d)  L >= 2: the start positions p, 0 <= p <= dl - L, with seq_d[p + j] == t_j for every j -- a sliding window over the
            document's own sequence, overlaps counted --, capped at 65535; 0 for a document without a sequence.  L = 1: tf.
  clause c holds in d  iff  pf(c, d) >= 1; the match rules are LexBoolRef's with "occurrence" read as "clause"
  idf(c)  = idf(t_0) + idf(t_1) + ...                         Python floats, left to right
  I(c, d) = max(1, rint(idf(c) * (pf / (pf + norm)) * 2^16))   float64, every operation rounded on its own; L = 1: LexRef's I(t, d)
  score_int = the uint64 sum of I(c, d) over the SHOULD and MUST clauses that hold
``search`` and ``match`` are LexBoolRef's, over this ``evaluate``."""
import numpy as np

from tests import lex_reference as LR
from tests.lexbool_reference import FILTER, MUST, MUST_NOT, SHOULD, LexBoolRef

PF_CAP = 65535


def pf_one(seq, clause) -> int:
    """pf of one clause in one sequence (None: a bag), position by position: the plain statement of the definition."""
    if seq is None:
        return 0
    seq, L = [int(t) for t in seq], len(clause)
    return min(PF_CAP, sum(1 for p in range(0, len(seq) - L + 1) if all(seq[p + j] == int(clause[j]) for j in range(L))))


class LexPhraseRef(LexBoolRef):
    def __init__(self, ids, docs, ordered, n_terms: int, k1: float = 1.2, b: float = 0.75):
        """``docs[i]``: the terms of document ``ids[i]``; ``ordered[i]``: put with its sequence (else as a bag)."""
        ids = np.asarray(ids, np.int64).reshape(-1)
        super().__init__(LR.LexRef(ids, docs, n_terms, k1, b))
        order = np.argsort(ids, kind="stable")
        self.seqs = [np.asarray(docs[j], np.int32).reshape(-1) if ordered[j] else None for j in order]      # by row
        # every sequence one after the other: the row of each word and how many words of its row follow it (itself included)
        rows = [r for r, s in enumerate(self.seqs) if s is not None and s.size]
        self.cat = np.concatenate([self.seqs[r] for r in rows]) if rows else np.zeros(0, np.int32)
        self.row_of = np.concatenate([np.full(self.seqs[r].size, r, np.int64) for r in rows]) if rows else np.zeros(0, np.int64)
        self.left = np.concatenate([np.arange(self.seqs[r].size, 0, -1) for r in rows]) if rows else np.zeros(0, np.int64)

    def pf(self, clause) -> np.ndarray:
        """[N] int64: the sliding-window comparison of every document at once; a window never leaves its document."""
        r, L = self.ref, len(clause)
        assert L >= 1
        if L == 1:
            return r.tf[:, int(clause[0])].astype(np.int64)
        n = self.cat.shape[0]
        ok = self.left >= L                                      # the window p .. p + L - 1 lies inside the row of p
        for j, t in enumerate(clause):
            shifted = np.zeros(n, bool)
            if j < n:
                shifted[:n - j] = self.cat[j:] == int(t)
            ok &= shifted
        return np.minimum(np.bincount(self.row_of[ok], minlength=r.N).astype(np.int64), PF_CAP)

    def idf_of(self, clause) -> float:
        idf = float(self.ref.idf[int(clause[0])])
        for t in clause[1:]:
            idf = idf + float(self.ref.idf[int(t)])
        return idf

    def impact(self, clause, pf=None) -> np.ndarray:
        """[N] uint64: I(c, d), 0 where the clause does not hold."""
        r = self.ref
        if len(clause) == 1:
            return r.impact[:, int(clause[0])]
        pf = self.pf(clause) if pf is None else pf
        f = pf.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            imp = np.rint(np.float64(self.idf_of(clause)) * (f / (f + r.norm)) * 65536.0)
        return np.where(pf > 0, np.maximum(1.0, imp), 0.0).astype(np.uint64)

    def evaluate(self, query, roles, min_should: int = 0):
        """-> (matches [N] bool, score_int [N] uint64) of one query: ``query`` a list of clauses, ``roles`` one per clause."""
        r = self.ref
        assert len(query) == len(roles) and sum(len(c) for c in query) <= 64 and 0 <= int(min_should) <= 64
        required = np.ones(r.N, bool)
        denied = np.zeros(r.N, bool)
        should = np.zeros(r.N, np.int64)
        score = np.zeros(r.N, np.uint64)
        n_required = n_should = 0
        for clause, role in zip(query, roles):
            assert role in (SHOULD, MUST, FILTER, MUST_NOT) and len(clause) >= 1
            pf = self.pf(clause)
            holds = pf >= 1
            if role in (MUST, FILTER):
                required &= holds
                n_required += 1
            if role == MUST_NOT:
                denied |= holds
            if role == SHOULD:
                should += holds
                n_should += 1
            if role in (SHOULD, MUST):
                score += self.impact(clause, pf)
        m = int(min_should) if n_required else max(1, int(min_should))
        matches = required & ~denied & (should >= m)
        if n_required + n_should == 0:
            matches[:] = False
        return matches, score
