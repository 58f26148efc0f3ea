"""Float64 reference of MMR search (sqe_index_search_mmr, include/sqe.h), shared by test_mmr_cpu.py and test_mmr_gpu.py.

For candidates with cosines c (rank order: descending, ties to the lowest id), row similarities S and a weight lam, step t
picks the not yet chosen candidate with the largest obj(i) = lam c_i - (1 - lam) pen(i), ties to the lower rank, where pen
is 0 before the first pick and afterwards the largest similarity to a chosen candidate.

``greedy`` is that definition in float64.  ``replay`` is the main oracle of the GPU tests: it does not run a second greedy
choice that could part from the library's at a near tie and then differ everywhere after it; it walks the library's OWN
selection order and checks at every step, in float64, that the pick was (within the tolerance) the best one available and
that the reported objective is the float64 one.  It skips nothing.

Tolerance.  The project treats cosines within 2e-6 as tied and the ABI promises s(i, j) within 2e-6
of the float64 dot product.  An objective lam c - (1 - lam) pen therefore carries at most lam 2e-6 + (1 - lam) 2e-6 = 2e-6,
and a comparison of two of them 4e-6: OBJ_TOL."""
import numpy as np

COS_TOL = 2e-6
OBJ_TOL = 4e-6


def norm64(a):
    a = np.asarray(a, np.float64)
    return a / (np.sqrt((a * a).sum(axis=-1, keepdims=True)) + 1e-9)


def greedy(c, S, lam, k):
    """Float64 greedy MMR over candidates in rank order -> (order [m], objective [m], margin [m]) with m = min(k, len(c));
    margin[t] = the chosen objective minus the best objective among the others still available (inf when none is left)."""
    c = np.asarray(c, np.float64)
    S = np.asarray(S, np.float64)
    n = c.shape[0]
    lam = float(lam)
    pen = np.zeros(n)
    free = np.ones(n, bool)
    order, objs, margins = [], [], []
    for t in range(min(k, n)):
        obj = np.where(free, lam * c - (1.0 - lam) * pen, -np.inf)
        i = int(np.argmax(obj))                               # the first maximum: ties to the lower rank
        rest = obj.copy()
        rest[i] = -np.inf
        order.append(i)
        objs.append(obj[i])
        margins.append(obj[i] - rest.max() if free.sum() > 1 else np.inf)
        free[i] = False
        pen = S[:, i].copy() if t == 0 else np.maximum(pen, S[:, i])
    return np.asarray(order, np.int64), np.asarray(objs), np.asarray(margins)


def replay(q, lam, got, cand, rows_of, what=""):
    """The replay check of one batch.
    q [B, dim] raw fp32 queries; lam scalar or [B]; got = (cos, ids, mmr) [B, k] of the library; cand = (cos, ids) [B, n] of
    search(q, n) on the same index; rows_of(ids) -> the stored fp32 rows of those ids (get_rows).
    Asserts, per query: the picks are distinct candidates of search(q, n), cos_out is bit for bit that search's cosine of the
    id, min(k, candidates) picks are made and the rest is (-inf, -1, -inf) padding; at every step the chosen candidate's
    float64 objective is >= the best float64 objective among the candidates not yet chosen - OBJ_TOL, and mmr_out is within
    OBJ_TOL of it.  -> (largest shortfall against the best available objective, largest |mmr_out - float64 objective|)."""
    cos, ids, mmr = got
    ccos, cids = cand
    b, k = ids.shape
    n = cids.shape[1]
    assert cos.shape == mmr.shape == (b, k) and ccos.shape == (b, n) and q.shape[0] == b
    lam = np.broadcast_to(np.asarray(lam, np.float32), (b,)).astype(np.float64)
    live = np.unique(cids[cids >= 0])
    stored = np.asarray(rows_of(live), np.float64) if live.size else np.zeros((0, q.shape[1]))
    qn = norm64(q)
    worst_gap = worst_obj = 0.0
    for i in range(b):
        m = int((cids[i] >= 0).sum())
        assert np.all(cids[i, m:] == -1), (what, i)
        picks = min(k, m)
        assert np.all(ids[i, :picks] >= 0) and np.all(ids[i, picks:] == -1), (what, i, ids[i], m)
        assert np.all(np.isneginf(cos[i, picks:])) and np.all(np.isneginf(mmr[i, picks:])), (what, i)
        rank_of = {int(r): j for j, r in enumerate(cids[i, :m])}
        assert len(set(ids[i, :picks].tolist())) == picks, (what, i, "a pick repeats")
        assert all(int(r) in rank_of for r in ids[i, :picks]), (what, i, "a pick is not a candidate of search(q, n)")
        ranks = np.array([rank_of[int(r)] for r in ids[i, :picks]], np.int64)
        assert np.array_equal(cos[i, :picks].view(np.uint32), ccos[i, ranks].view(np.uint32)), (what, i, "cos_out is not search's cosine")
        R = stored[np.searchsorted(live, cids[i, :m])]
        c64 = R @ qn[i]
        S = R @ R.T
        pen = np.zeros(m)
        free = np.ones(m, bool)
        for t, j in enumerate(ranks):
            obj = lam[i] * c64 - (1.0 - lam[i]) * pen
            best = obj[free].max()
            gap = best - obj[j]
            worst_gap = max(worst_gap, gap)
            assert gap <= OBJ_TOL, (what, i, t, "not the best available pick", gap)
            d = abs(float(mmr[i, t]) - obj[j])
            worst_obj = max(worst_obj, d)
            assert d <= OBJ_TOL, (what, i, t, "mmr_out", float(mmr[i, t]), obj[j])
            free[j] = False
            pen = S[:, j].copy() if t == 0 else np.maximum(pen, S[:, j])
    return worst_gap, worst_obj


def full_reference(x, q, n, k, lam, block=128, per_step=False):
    """Float64 from the raw data: per query the top n + 1 rows of x (normalised in float64; cosine descending, ties to the
    lowest row), the greedy choice over the first n of them.
    -> (ids [B, k] picks as row numbers, margin [B] smallest step margin -- with per_step the margins [B, k] of every
    step --, edge [B] gap between the n-th and n + 1-th cosine)."""
    xn, qn = norm64(x), norm64(q)
    rows = np.arange(xn.shape[0])
    b = q.shape[0]
    out = np.full((b, k), -1, np.int64)
    margin = np.full((b, k) if per_step else b, np.inf)
    edge = np.full(b, np.inf)
    for b0 in range(0, b, block):
        c = qn[b0:b0 + block] @ xn.T
        for i in range(c.shape[0]):
            top = np.argpartition(-c[i], min(n + 8, c.shape[1] - 1))[:n + 8]
            top = top[np.lexsort((rows[top], -c[i, top]))][:n + 1]
            if top.shape[0] > n:
                edge[b0 + i] = c[i, top[n - 1]] - c[i, top[n]]
            top = top[:n]
            R = xn[top]
            order, _, marg = greedy(c[i, top], R @ R.T, lam, k)
            out[b0 + i, :order.shape[0]] = top[order]
            if per_step:
                margin[b0 + i, :marg.shape[0]] = marg
            else:
                margin[b0 + i] = marg.min() if marg.size else np.inf
    return out, margin, edge
