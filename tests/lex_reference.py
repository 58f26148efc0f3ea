"""NumPy reference of the lexical index (include/sqe.h: sqe_lex_*), written from the definition.

``LexRef(ids, bags, n_terms, k1, b)`` holds the live documents; ``search(queries, k)`` returns (scores [B, k] float32,
ids [B, k] int64, score_int [B, k] uint64).

  tf = min(occurrences, 65535), dl = occurrences, N = documents, avgdl = float64(sum dl) / float64(N)
  idf(t) = math.log(1.0 + ((N - df) + 0.5) / (df + 0.5))        one math.log per distinct df
  norm(d) = k1 * ((1.0 - b) + b * (dl / avgdl))                 NumPy float64, every operation rounded on its own
  I(t, d) = max(1, rint(idf * (tf / (tf + norm)) * 2^16))       np.rint: round half to even
  score_int = the uint64 sum of I over the query's term occurrences; score = float32(float64(score_int) * 2^-16)
Ranking: lexsort on (id, -score_int); documents with score_int == 0 are no hits; padding (-inf, -1).

``hybrid(...)`` is the reference of sqe_index_search_hybrid: it feeds tests/fuse_reference.fuse the library's own vector lists
and its own lexical list (which carries cos = -inf) and reads each hit's BM25 score off that list."""
import math

import numpy as np

from tests import fuse_reference as FR

TF_CAP = 65535


class LexRef:
    def __init__(self, ids, bags, n_terms: int, k1: float = 1.2, b: float = 0.75):
        ids = np.asarray(ids, np.int64).reshape(-1)
        assert len(set(ids.tolist())) == ids.shape[0] and len(bags) == ids.shape[0]
        order = np.argsort(ids, kind="stable")
        self.ids = ids[order]                                     # row = rank of the id
        self.n_terms, self.k1, self.b = n_terms, float(k1), float(b)
        N = self.ids.shape[0]
        count = np.zeros((N, n_terms), np.int64)
        for row, j in enumerate(order):
            bag = np.asarray(bags[j], np.int64).reshape(-1)
            if bag.size:
                np.add.at(count[row], bag, 1)
        self.dl = count.sum(axis=1)
        self.tf = np.minimum(count, TF_CAP)
        self.df = (count > 0).sum(axis=0).astype(np.int32)
        self.N = N
        self.avgdl = np.float64(self.dl.sum()) / np.float64(N) if N else np.float64(0.0)
        by_df = {int(f): math.log(1.0 + ((N - int(f)) + 0.5) / (int(f) + 0.5)) for f in set(self.df.tolist()) if f > 0}
        self.idf = np.array([by_df.get(int(f), 0.0) for f in self.df], np.float64)
        tf = self.tf.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.norm = self.k1 * ((1.0 - self.b) + self.b * (self.dl.astype(np.float64) / self.avgdl)) if N else np.zeros(0)
            frac = tf / (tf + self.norm[:, None])
            self.bm25 = np.where(self.tf > 0, self.idf[None, :] * frac, 0.0)           # float64 idf * tf / (tf + norm)
            imp = np.rint(self.bm25 * 65536.0)
        self.impact = np.where(self.tf > 0, np.maximum(1.0, imp), 0.0).astype(np.uint64)      # [N, n_terms]

    def score_int(self, query) -> np.ndarray:
        s = np.zeros(self.N, np.uint64)
        for t in query:
            s += self.impact[:, int(t)]
        return s

    def search(self, queries, k: int):
        B = len(queries)
        score = np.full((B, k), -np.inf, np.float32)
        ids = np.full((B, k), -1, np.int64)
        sint = np.zeros((B, k), np.uint64)
        for i, q in enumerate(queries):
            s = self.score_int(q)
            hit = np.nonzero(s)[0]
            order = hit[np.lexsort((self.ids[hit], -s[hit].astype(np.int64)))][:k]
            t = order.shape[0]
            sint[i, :t] = s[order]
            score[i, :t] = (s[order].astype(np.float64) * 2.0 ** -16).astype(np.float32)
            ids[i, :t] = self.ids[order]
        return score, ids, sint

    def search_float(self, query):
        """Plain float64 BM25 of every row (no integers): the cross-check of the integer definition."""
        s = np.zeros(self.N, np.float64)
        for t in query:
            s += self.bm25[:, int(t)]
        return s


def hybrid(vec_cos, vec_ids, offsets, lex_score, lex_ids, k: int, weights=None, c: int = 60):
    """vec_cos / vec_ids [Bs, n] as ``search(q, n)`` returned them, lex_score / lex_ids [G, n] as ``LexicalIndex.search``
    returned them, ``weights`` [Bs + G] or None -> (fused, ids, cos, bm25) [G, k]."""
    offsets = np.asarray(offsets, np.int64)
    G = offsets.shape[0] - 1
    Bs = int(offsets[-1])
    w = None if weights is None else np.asarray(weights, np.float32)
    out = (np.empty((G, k), np.float32), np.empty((G, k), np.int64), np.empty((G, k), np.float32), np.empty((G, k), np.float32))
    for g in range(G):
        a, b = int(offsets[g]), int(offsets[g + 1])
        n = lex_ids.shape[1]
        cl = [np.asarray(vec_cos[j], np.float32) for j in range(a, b)] + [np.full(n, -np.inf, np.float32)]
        il = [np.asarray(vec_ids[j], np.int64) for j in range(a, b)] + [np.asarray(lex_ids[g], np.int64)]
        wg = None if w is None else np.concatenate([w[a:b], w[Bs + g:Bs + g + 1]])
        fused, ids, cos = FR.fuse(cl, il, k, "rrf", wg, c)
        of = {int(i): s for s, i in zip(lex_score[g], lex_ids[g]) if i >= 0}
        bm = np.array([of.get(int(i), -np.inf) for i in ids], np.float32)
        for o, v in zip(out, (fused, ids, cos, bm)):
            o[g] = v
    return out
