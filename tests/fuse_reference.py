"""NumPy reference of the fused multi-query search (include/sqe.h: sqe_index_search_fused), written from the definition.

``fuse(cos_lists, id_lists, k, mode, weights, c)`` takes the lists of ONE logical query as ``search(q_sub, n)`` returned
them (cos [m, n] float32, ids [m, n] int64, (-inf, -1) padded) and returns (fused [k] float32, ids [k] int64, cos [k] float32).

RRF: fused_int(x) = sum over the lists j that hold x of rint(2^40 w_j / (c + rank)) -- a float64 division, round half to
even, summed as np.uint64 --, fused = float32(float64(fused_int) * 2^-40).  MAX: the largest cosine over the lists that hold
x, compared as a float.  Ranking: the score descending, ties to the lowest id (lexsort on (id, -score)); padding
(-inf, -1, -inf)."""
import numpy as np

TWO40 = float(2 ** 40)


def rrf_term(w, c: int, rank: int) -> np.uint64:
    """T(w, r) = llrint(ldexp((double)w / (double)(c + r), 40)) for an fp32 weight."""
    return np.uint64(np.rint(np.float64(np.float32(w)) / np.float64(c + rank) * TWO40))


def _best_cos(a: np.float32, b: np.float32) -> np.float32:
    """The larger of two cosines; +0 above -0 (the one case where 'compared as a float' leaves the bits open)."""
    if b > a or (b == a and np.signbit(a) and not np.signbit(b)):
        return b
    return a


def fuse(cos_lists, id_lists, k: int, mode: str = "rrf", weights=None, c: int = 60):
    m = len(cos_lists)
    cos_lists = np.asarray(cos_lists, np.float32).reshape(m, -1) if m else np.empty((0, 0), np.float32)
    id_lists = np.asarray(id_lists, np.int64).reshape(m, -1) if m else np.empty((0, 0), np.int64)
    if mode not in ("rrf", "max"):
        raise ValueError(mode)
    if mode == "max" and weights is not None:
        raise ValueError("weights must be None with max")
    w = np.ones(m, np.float32) if weights is None else np.asarray(weights, np.float32)
    score, best = {}, {}
    for j in range(m):
        rank = 0
        for cj, ij in zip(cos_lists[j], id_lists[j]):
            if ij < 0:
                continue                      # padding: skipped
            rank += 1
            x = int(ij)
            best[x] = np.float32(cj) if x not in best else _best_cos(best[x], np.float32(cj))
            if mode == "rrf":
                score[x] = score.get(x, np.uint64(0)) + rrf_term(w[j], c, rank)
    ids = np.array(sorted(best), np.int64)
    fused = np.full(k, -np.inf, np.float32)
    id_out = np.full(k, -1, np.int64)
    cos_out = np.full(k, -np.inf, np.float32)
    if ids.size == 0:
        return fused, id_out, cos_out
    bc = np.array([best[int(x)] for x in ids], np.float32)
    if mode == "rrf":
        si = np.array([score[int(x)] for x in ids], np.uint64)
        key = -si.astype(np.float64)          # exact: fused_int < 2^50
        val = (si.astype(np.float64) * 2.0 ** -40).astype(np.float32)
    else:
        key = -(bc.astype(np.float64) + 0.0)  # -0 and +0 compare equal
        val = bc
    order = np.lexsort((ids, key))[:k]
    t = order.shape[0]
    fused[:t], id_out[:t], cos_out[:t] = val[order], ids[order], bc[order]
    return fused, id_out, cos_out


def fuse_groups(cos, ids, offsets, k: int, mode: str = "rrf", weights=None, c: int = 60):
    """``fuse`` over every group of a batch: cos / ids [Bs, n] as ``search(q, n)`` returned them -> ([G, k]) x 3."""
    offsets = np.asarray(offsets, np.int64)
    G = offsets.shape[0] - 1
    out = (np.empty((G, k), np.float32), np.empty((G, k), np.int64), np.empty((G, k), np.float32))
    for g in range(G):
        a, b = int(offsets[g]), int(offsets[g + 1])
        r = fuse(cos[a:b], ids[a:b], k, mode, None if weights is None else np.asarray(weights, np.float32)[a:b], c)
        for o, v in zip(out, r):
            o[g] = v
    return out
