"""MMR k-NN search (sqe_index_search_mmr, mmr.hip): a greedy, diversified choice of k rows among the exact top-n.  GPU only.

The oracle is tests/mmr_reference.py.  Its replay check walks the library's own selection order in float64 (queries
normalised in float64, the stored rows read back with get_rows) and asserts at every step that the pick was the best one
available within 4e-6 and that mmr_out is the float64 objective within 4e-6; picks have to be candidates of search(q, n) on
the same index and carry that search's cosine bit for bit.  4e-6 is twice the project's 2e-6 cosine tie tolerance: each of
the two objectives compared carries at most lam 2e-6 + (1 - lam) 2e-6.  The sequence test compares whole selections with
the float64 greedy choice computed from the raw data and skips a query only where one of its float64 steps was decided by
a margin <= 4e-6 or its n-th and n + 1-th float64 cosines lie within 2e-6; the skipped share is capped at 3 %.
Everything that compares two runs of the library (batch sizes, prefixes, entry points, device groups, budgets, IVF, the
int8 first pass) is bit for bit."""
import json
import os

import numpy as np
import pytest

from . import mmr_reference as M

pytestmark = pytest.mark.gpu

D = 256
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(64, 10, 0.5), (256, 64, 0.3), (50, 7, 0.7), (32, 32, 0.0), (1, 1, 0.5)]


def same_bits(a, b):
    return all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8)) for u, w in zip(a, b))


def _corpus(rng):
    """Rows centre[doc] + g with the corpus' document sizes (tests/golden/chunker.json), shuffled."""
    counts = np.array(list(json.load(open(os.path.join(HERE, "golden", "chunker.json")))["counts"].values()), np.int64)
    owner = np.repeat(np.arange(counts.shape[0]), counts)
    rng.shuffle(owner)
    centre = rng.standard_normal((counts.shape[0], D)).astype(np.float32)
    x = centre[owner]
    x += rng.standard_normal(x.shape, dtype=np.float32)
    return x, centre


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(41)
    x, centre = _corpus(rng)
    assert x.shape[0] == 32_717
    q = centre[rng.integers(0, centre.shape[0], 1500)] + rng.standard_normal((1500, D)).astype(np.float32)
    return x, q.astype(np.float32)


@pytest.fixture(scope="module")
def index(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    idx = VectorIndex(ctx, D)
    idx.add(data[0])
    return idx


@pytest.fixture(scope="module")
def stored(index, data):
    """The stored rows, read back once (get_rows): what the replay check takes its float64 dot products from."""
    rows = index.get_rows(np.arange(data[0].shape[0]))
    return lambda ids: rows[np.asarray(ids, np.int64)]


def _replay(idx, q, n, k, lam, rows_of, what):
    got = idx.search_mmr(q, k, lam=lam, n_cand=n)
    cand = idx.search(q, n)
    gap, err = M.replay(q, lam, got, cand, rows_of, what)
    print(f"[mmr] {what}: B {q.shape[0]}, worst shortfall {gap:.2e}, worst |mmr_out - f64| {err:.2e}")
    return got


# ---------------------------------------------------------------- 1. the replay check
@pytest.mark.parametrize("n,k,lam", CASES)
def test_replay(data, index, stored, n, k, lam):
    _, q = data
    for b in (1, 3, 130):
        _replay(index, q[:b], n, k, lam, stored, f"n={n} k={k} lam={lam} B={b}")


def test_replay_per_query_lambda_and_two_passes(data, index, stored):
    _, q = data
    lam = np.linspace(0.0, 1.0, 1500).astype(np.float32)
    _replay(index, q, 64, 10, 0.5, stored, "two passes")                     # 1500 x 64 rows > the default budget of 65536
    got = _replay(index, q, 64, 10, lam, stored, "per-query lambda")
    for i in (0, 700, 1499):                                               # a query's answer depends on its own weight only
        assert same_bits(index.search_mmr(q[i:i + 1], 10, lam=float(lam[i]), n_cand=64), [a[i:i + 1] for a in got])


@pytest.mark.parametrize("dim", [64, 1024])
def test_replay_other_dims(ctx, dim):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(42 + dim)
    centre = rng.standard_normal((300, dim)).astype(np.float32)
    owner = rng.integers(0, 300, 4096)
    x = centre[owner] + rng.standard_normal((4096, dim)).astype(np.float32)
    q = centre[rng.integers(0, 300, 33)] + rng.standard_normal((33, dim)).astype(np.float32)
    idx = VectorIndex(ctx, dim)
    idx.add(x)
    rows = idx.get_rows(np.arange(4096))
    for n, k, lam in ((50, 7, 0.7), (256, 64, 0.3)):
        _replay(idx, q, n, k, lam, lambda ids: rows[ids], f"dim={dim} n={n} k={k}")
    idx.close()


# ---------------------------------------------------------------- 2. whole selections against the float64 greedy choice
@pytest.mark.parametrize("n,k,lam", [(64, 10, 0.5), (32, 3, 0.7)])
def test_sequence_equals_float64(data, index, n, k, lam):
    x, q = data
    q = q[:512]
    want, margin, edge = M.full_reference(x, q, n, k, lam)
    skip = (margin <= M.OBJ_TOL) | (edge <= M.COS_TOL)
    cos, ids, _ = index.search_mmr(q, k, lam=lam, n_cand=n)
    bad = np.flatnonzero(~skip & (ids != want).any(axis=1))
    plain = index.search(q, k)[1]
    changed = int((ids != plain).any(axis=1).sum())
    print(f"[mmr] sequence n={n} k={k} lam={lam}: skipped {int(skip.sum())} of 512, mismatches {bad.size}, "
          f"{changed} of 512 differ from the plain top-{k}")
    assert skip.mean() <= 0.03, skip.sum()
    assert bad.size == 0, (bad[:5], ids[bad[:2]], want[bad[:2]])
    assert np.array_equal(ids[:, 0], plain[:, 0])                          # the first pick is the best hit
    assert changed > 0                                                     # MMR changes something on this data


# ---------------------------------------------------------------- 3. two runs of the library, bit for bit
def test_lambda_one_is_plain_topk(data, index):
    _, q = data
    for n, k in ((64, 10), (0, 3), (256, 256)):
        cos, ids, mmr = index.search_mmr(q[:130], k, lam=1.0, n_cand=n)
        assert same_bits((cos, ids), index.search(q[:130], k))
        assert np.array_equal(mmr, cos)


def test_batch_position_prefix_and_automatic_depth(data, index):
    _, q = data
    for n, k, lam in ((64, 10, 0.5), (256, 64, 0.3)):
        full = index.search_mmr(q[:130], k, lam=lam, n_cand=n)
        for i in (0, 77, 129):                                             # alone vs inside a batch
            assert same_bits(index.search_mmr(q[i:i + 1], k, lam=lam, n_cand=n), [a[i:i + 1] for a in full])
        for k1 in (1, 3, k - 1):                                           # the k'-run is the prefix of the k-run
            assert same_bits(index.search_mmr(q[:130], k1, lam=lam, n_cand=n), [a[:, :k1] for a in full])
    for k, n in ((3, 32), (10, 40), (100, 256)):                           # n_cand = 0: min(256, max(32, 4 k))
        assert same_bits(index.search_mmr(q[:9], k), index.search_mmr(q[:9], k, n_cand=n))


def test_device_entry(ctx, data, index):
    import torch
    _, q = data
    b = 130
    lam = np.linspace(0.2, 0.9, b).astype(np.float32)
    for n, k in ((64, 10), (256, 64)):
        host = index.search_mmr(q[:b], k, lam=lam, n_cand=n)
        qd = torch.from_numpy(q[:b]).cuda()
        cd = torch.empty((b, k), dtype=torch.float32, device="cuda")
        idd = torch.empty((b, k), dtype=torch.int64, device="cuda")
        md = torch.empty((b, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        index.search_mmr_device(qd.data_ptr(), b, k, cd.data_ptr(), idd.data_ptr(), md.data_ptr(), lam=lam, n_cand=n)
        ctx.synchronize()
        assert same_bits(host, (cd.cpu().numpy(), idd.cpu().numpy(), md.cpu().numpy()))


def test_budget_passes(data, index):
    _, q = data
    want = index.search_mmr(q[:130], 10, lam=0.5, n_cand=64)
    want2 = index.search_mmr(q[:9], 64, lam=0.3, n_cand=256)
    index.set_option("mmr_row_budget", 256)                                # 4 queries per pass at n = 64, one at n = 256
    try:
        assert same_bits(index.search_mmr(q[:130], 10, lam=0.5, n_cand=64), want)
        assert same_bits(index.search_mmr(q[:9], 64, lam=0.3, n_cand=256), want2)
    finally:
        index.set_option("mmr_row_budget", 1 << 16)
    from semantic_query_engine_amd import _native
    with pytest.raises(_native.SqeError):
        index.set_option("mmr_row_budget", 255)


@pytest.mark.parametrize("P", [2, 3, 8])
def test_group_equals_single_device(data, index, P):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, q = data
    gctx = Context(devices=[0] * P, exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    g.add(x)
    lam = np.linspace(0.0, 1.0, 130).astype(np.float32)
    for n, k, lm in ((64, 10, lam), (256, 64, 0.3), (1, 1, 0.5)):
        assert same_bits(g.search_mmr(q[:130], k, lam=lm, n_cand=n), index.search_mmr(q[:130], k, lam=lm, n_cand=n)), (P, n, k)
    g.set_option("mmr_row_budget", 4096)                                   # several passes of the group
    assert same_bits(g.search_mmr(q[:130], 10, lam=0.5, n_cand=64), index.search_mmr(q[:130], 10, lam=0.5, n_cand=64))
    g.close()
    gctx.close()


def test_group_device_entry(data, index):
    """The _device form on a group: queries and outputs in the leader's memory, the weights on the host, several passes
    enqueued with no synchronisation between them; against the group's host form and the single device, bit for bit."""
    import torch
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, q = data
    gctx = Context(devices=[0, 0], exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    g.add(x)
    g.set_option("mmr_row_budget", 4096)                                   # 32 queries per pass at n = 64, 8 at n = 256
    b = 130
    lam = np.linspace(0.1, 1.0, b).astype(np.float32)
    for n, k in ((64, 10), (256, 64)):
        host = g.search_mmr(q[:b], k, lam=lam, n_cand=n)
        assert same_bits(host, index.search_mmr(q[:b], k, lam=lam, n_cand=n))
        qd = torch.from_numpy(q[:b]).cuda()
        cd = torch.empty((b, k), dtype=torch.float32, device="cuda")
        idd = torch.empty((b, k), dtype=torch.int64, device="cuda")
        md = torch.empty((b, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        g.search_mmr_device(qd.data_ptr(), b, k, cd.data_ptr(), idd.data_ptr(), md.data_ptr(), lam=lam, n_cand=n)
        gctx.synchronize()
        assert same_bits(host, (cd.cpu().numpy(), idd.cpu().numpy(), md.cpu().numpy())), (n, k)
    g.close()
    gctx.close()


def test_group_deletes_and_short_index(data, index):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    x, q = data
    gctx = Context(devices=[0] * 3, exchange=EXCHANGE_COPY)
    g, s = VectorIndex(gctx, D), VectorIndex(index.ctx, D)
    for idx in (g, s):
        idx.add(x[:5000])
        idx.delete(np.arange(0, 5000, 7))
        idx.set_option("id_base", 1_000_000)
    assert same_bits(g.search_mmr(q[:40], 10, lam=0.5, n_cand=64), s.search_mmr(q[:40], 10, lam=0.5, n_cand=64))
    for idx in (g, s):
        idx.delete(idx.ids()[20:])                                         # 20 live rows: fewer than n, shards of 6 or 7
    a, b = g.search_mmr(q[:5], 32, lam=0.4, n_cand=64), s.search_mmr(q[:5], 32, lam=0.4, n_cand=64)
    assert same_bits(a, b) and np.all(a[1][:, :20] >= 1_000_000) and np.all(a[1][:, 20:] == -1)
    g.close()
    s.close()
    gctx.close()


def test_ivf_all_lists_equals_flat(ctx, data, index):
    """An IVF search is approximate by construction (ivf.hip, ivf_scan.hip): int8 estimates pick the kp = min(256, max(32, 4 n)) rows that are
    re-scored in fp32, with no certificate.  With every list probed it returns the FLAT index's answer where kp leaves room
    for the estimates' error -- depths 64 (kp = 256 = 4 n) and 32 (8 n) here -- and there MMR on the two indexes is compared
    bit for bit.  At depth 256 kp = n: a row near the 256th place may be another one than FLAT's, so there the definition is
    checked as it reads -- the candidates are what search(q, n, nprobe) of THIS index returns -- by the replay check."""
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    x, q = data
    ivf = VectorIndex(ctx, D, INDEX_IVF_FLAT, 64)
    ivf.add(x)
    ivf.train(x[:10_000], iters=5, seed=1)
    for n, k, lam in ((64, 10, 0.5), (32, 3, 0.7)):
        assert same_bits(ivf.search_mmr(q[:40], k, lam=lam, n_cand=n, nprobe=64), index.search_mmr(q[:40], k, lam=lam, n_cand=n))
    rows = ivf.get_rows(np.arange(x.shape[0]))
    got = ivf.search_mmr(q[:40], 64, lam=0.3, n_cand=256, nprobe=64)
    M.replay(q[:40], 0.3, got, ivf.search(q[:40], 256, nprobe=64), lambda ids: rows[ids], "IVF n=256 k=64")
    ivf.close()


def test_int8_first_pass_candidates(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    idx = VectorIndex(ctx, D)
    idx.add(x)
    idx.set_option("scan_mode", 0)                                         # SQE_SCAN_BF16_RESCORE
    want = idx.search_mmr(q[:200], 5, lam=0.5, n_cand=16)
    # SQE_SCAN_INT8_RESCORE on an index this small: sample every 4th tile, threshold at the 64th place of the sample
    for key, val in (("scan_mode", 2), ("i8_min_rows", 0), ("i8_sample_step", 4), ("i8_sample_m", 64)):
        idx.set_option(key, val)
    got = idx.search_mmr(q[:200], 5, lam=0.5, n_cand=16)
    last = idx.i8_last()                                                   # the candidates came through the int8 first pass
    assert last["k"] == 16 and last["B"] == 200
    assert same_bits(got, want)
    idx.close()


# ---------------------------------------------------------------- 4. duplicates
def test_duplicates_are_passed_over(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, _ = data
    rng = np.random.default_rng(43)
    xs = x[:8000].copy()
    at = np.sort(rng.choice(8000, 8, replace=False))
    xs[at] = xs[at[0]]                                                     # 8 bit-identical copies of one row
    q = (xs[at[0]] + 0.5 * rng.standard_normal(D).astype(np.float32))[None]
    want, margin, _ = M.full_reference(xs, q, 32, 3, 0.5, per_step=True)
    # the float64 choice keeps one copy: step 0 is an exact tie among the copies (the rank rule decides it), the later
    # steps are decided clearly
    assert margin[0, 0] == 0.0 and margin[0, 1:].min() > 1e-4 and np.isin(want[0], at).sum() == 1
    idx = VectorIndex(ctx, D)
    idx.add(xs)
    assert np.array_equal(idx.search(q, 3)[1][0], at[:3])                  # the plain search returns three copies
    cos, ids, mmr = idx.search_mmr(q, 3, lam=0.5, n_cand=32)
    assert ids[0, 0] == at[0] and np.isin(ids[0], at).sum() == 1           # exactly one copy, the lowest id, in first place
    assert np.array_equal(ids, want)
    idx.close()


# ---------------------------------------------------------------- 5. edges
def test_fewer_rows_than_n_and_k_empty_index_and_no_queries(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    idx = VectorIndex(ctx, D)
    for arr in idx.search_mmr(q[:3], 4, lam=0.5):                          # an empty index: all padding
        assert arr.shape == (3, 4) and np.all(arr == (-1 if arr.dtype == np.int64 else -np.inf))
    idx.add(x[:5])
    rows = idx.get_rows(np.arange(5))
    got = _replay(idx, q[:3], 32, 8, 0.5, lambda ids: rows[ids], "5 rows, n=32, k=8")
    assert np.all(got[1][:, :5] >= 0) and np.all(got[1][:, 5:] == -1)
    assert np.all(np.isneginf(got[0][:, 5:])) and np.all(np.isneginf(got[2][:, 5:]))
    assert [a.shape for a in idx.search_mmr(q[:0], 4)] == [(0, 4)] * 3     # B = 0
    idx.close()


def test_after_deletes_and_update(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, q = data
    idx = VectorIndex(ctx, D)
    idx.add(x[:6000])
    before = idx.search_mmr(q[:20], 10, lam=0.5, n_cand=64)
    gone = np.unique(np.concatenate([before[1][:, 0], np.arange(0, 6000, 3)]))      # every first pick and a third of the rows
    idx.delete(gone)
    live = idx.ids()
    rows = idx.get_rows(live)
    rows_of = lambda ids: rows[np.searchsorted(live, ids)]
    got = _replay(idx, q[:20], 64, 10, 0.5, rows_of, "after deletes")
    assert not np.isin(got[1], gone).any() and got[1].max() > live.shape[0]          # ids, not positions
    # a candidate row is rewritten: the Gram product reads the new row
    target = int(got[1][0, 1])
    idx.update(np.array([target]), x[6001][None])
    rows = idx.get_rows(live)
    after = _replay(idx, q[:20], 64, 10, 0.5, rows_of, "after update")
    assert not same_bits(after, got)
    idx.close()


def test_invalid_arguments_leave_outputs_untouched(data, index):
    from semantic_query_engine_amd import _native
    lib = _native.load()
    _, q = data
    qq = np.ascontiguousarray(q[:3])
    c = np.full((3, 4), 7.0, np.float32)
    i = np.full((3, 4), 7, np.int64)
    m = np.full((3, 4), 7.0, np.float32)
    out = (c.ctypes.data, i.ctypes.data, m.ctypes.data)

    keep = []                                                              # the weight arrays outlive the calls that read them

    def lam(*v):
        keep.append(np.asarray(v, np.float32))
        return keep[-1]

    ok = lam(0.5, 0.5, 0.5)
    h, qp = index.handle, qq.ctypes.data
    bad = [(h, qp, 3, 4, 3, ok.ctypes.data, 0, *out),                                 # k > n
           (h, qp, 3, 4, 257, ok.ctypes.data, 0, *out),                               # n > 256
           (h, qp, 3, 0, 0, ok.ctypes.data, 0, *out),
           (h, qp, 3, 257, 0, ok.ctypes.data, 0, *out),
           (h, qp, -1, 4, 0, ok.ctypes.data, 0, *out),
           (h, qp, 3, 4, 0, lam(0.5, np.nan, 0.5).ctypes.data, 0, *out),
           (h, qp, 3, 4, 0, lam(0.5, 0.5, -0.1).ctypes.data, 0, *out),
           (h, qp, 3, 4, 0, lam(1.1, 0.5, 0.5).ctypes.data, 0, *out),
           (h, None, 3, 4, 0, ok.ctypes.data, 0, *out),
           (h, qp, 3, 4, 0, None, 0, *out),
           (h, qp, 3, 4, 0, ok.ctypes.data, 0, None, out[1], out[2]),
           (h, qp, 3, 4, 0, ok.ctypes.data, 0, out[0], None, out[2]),
           (h, qp, 3, 4, 0, ok.ctypes.data, 0, out[0], out[1], None),
           (None, qp, 3, 4, 0, ok.ctypes.data, 0, *out)]
    for args in bad:
        assert lib.sqe_index_search_mmr(*args) == -1, args[2:5]
        assert lib.sqe_index_search_mmr_device(*args) == -1, args[2:5]
    assert np.all(c == 7.0) and np.all(i == 7) and np.all(m == 7.0)
    assert lib.sqe_index_search_mmr(h, qp, 0, 4, 0, ok.ctypes.data, 0, *out) == 0                      # B = 0 writes nothing
    assert np.all(c == 7.0) and np.all(i == 7) and np.all(m == 7.0)
    assert lib.sqe_index_search_mmr(h, qp, 3, 4, 0, ok.ctypes.data, 0, *out) == 0
    assert same_bits((c, i, m), index.search_mmr(qq, 4, lam=0.5))
    with pytest.raises(ValueError):
        index.search_mmr(qq, 4, lam=1.5)
