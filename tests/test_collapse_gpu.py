"""Collapsed k-NN search (sqe_index_search_collapsed, collapse.hip): per query the k best groups of the exact ranking and
each group's best row.  GPU only.

The reference is NumPy in float64, written here: rows and queries normalised as x / (||x|| + 1e-9), c = q x^T, a stable
sort by (-c, id), the first row of every key (a row without a key is its own group), the first k.  Tolerances are the
project's: cosines within 1e-3 of float64; ids and keys equal to the reference at every output
position except where the reference's own neighbouring group cosines (j against j - 1 or j + 1, the k-th against the
k + 1-th included) lie within 2e-6 (a near pair skips both of its positions); at most 3 % of a case's positions may be
skipped that way, and every case asserts it.  A case is one test: case 1 runs its four batch sizes per k and caps the
skipped share over all their positions together (at B = 1 and k = 64 a single near pair is 2 of 64 positions).  Inside the crowd of near-identical rows (case 4) the float64 and the fp32 ranking cannot agree on WHICH of the
3,000 rows is best (their cosines differ by less than fp32 resolves), so at the crowd's position the key and the cosine
are compared and the id has to name a crowd row whose float64 cosine is within 2e-6 of the crowd's best.
Everything that compares two runs of the library (depths, budgets, IVF, device groups, entry points) is bit for bit."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 256
TOL = 2e-6
NONE = -(1 << 63)
HERE = os.path.dirname(os.path.abspath(__file__))


def _norm64(a):
    a = np.asarray(a, np.float64)
    return a / (np.sqrt((a * a).sum(axis=1)) + 1e-9)[:, None]


def _groups(keys):
    """Group index per row: rows that share a key share an index, a row without a key gets one of its own."""
    keys = np.asarray(keys, np.int64)
    gid = np.empty(keys.shape[0], np.int64)
    has = keys != NONE
    _, inv = np.unique(keys[has], return_inverse=True)
    gid[has] = inv
    gid[~has] = (inv.max() + 1 if inv.size else 0) + np.arange(int((~has).sum()))
    return gid


def reference(x, q, keys, ids, k, block=128):
    """-> (cos [B, k + 1] float64, ids [B, k + 1], keys [B, k + 1]): the first k + 1 groups,
    padded with (-inf, -1, NONE).  `ids` are the (ascending) ids of the rows of x."""
    xn = _norm64(x)
    qn = _norm64(q)
    gid = _groups(keys)
    ids = np.asarray(ids, np.int64)
    keys = np.asarray(keys, np.int64)
    b = q.shape[0]
    rc = np.full((b, k + 1), -np.inf)
    ri = np.full((b, k + 1), -1, np.int64)
    rk = np.full((b, k + 1), NONE, np.int64)
    for b0 in range(0, b, block):
        c = qn[b0:b0 + block] @ xn.T
        for i in range(c.shape[0]):
            order = np.lexsort((ids, -c[i]))
            _, first = np.unique(gid[order], return_index=True)
            first = np.sort(first)[:k + 1]
            rows = order[first]
            m = rows.shape[0]
            rc[b0 + i, :m] = c[i, rows]
            ri[b0 + i, :m] = ids[rows]
            rk[b0 + i, :m] = keys[rows]
    return rc, ri, rk


def compare(got, ref, k, what, crowd_key=None, cap=True):
    """One result (cos, ids, keys) [B, k] against the reference's first k + 1 groups (columns beyond k + 1 are ignored).
    -> (positions skipped, positions); with cap the 3 % cap on the skipped share is asserted here, else by the caller over
    the runs of its case."""
    cos, ids, keys = got
    rc, ri, rk = (a[:cos.shape[0]] for a in ref)
    assert cos.shape == ids.shape == keys.shape == (rc.shape[0], k)
    c0 = rc[:, :k]
    valid = ri[:, :k] >= 0
    err = np.abs(np.where(valid, cos.astype(np.float64) - c0, 0.0))
    near = np.zeros(c0.shape, bool)
    with np.errstate(invalid="ignore"):
        gap = np.abs(rc[:, :k] - rc[:, 1:k + 1]) <= TOL          # position j against j + 1
    near |= gap
    near[:, 1:] |= gap[:, :-1]
    near &= valid
    share = near.mean() if near.size else 0.0
    exact = ~near
    id_ok = ids == ri[:, :k]
    if crowd_key is not None:
        at_crowd = (rk[:, :k] == crowd_key) & (keys == crowd_key)
        id_ok |= at_crowd
    bad = int((exact & ~(id_ok & (keys == rk[:, :k]))).sum())
    print(f"[collapse] {what}: positions {c0.size}, skipped {int(near.sum())} ({100 * share:.3f} %), max|dcos| {err.max() if err.size else 0:.2e}, "
          f"mismatches {bad}")
    if cap:
        assert share <= 0.03, (what, share)
    assert (err < 1e-3).all(), (what, err.max())
    assert np.all(np.isneginf(cos[~valid])) and np.all(ids[~valid] == -1) and np.all(keys[~valid] == NONE), what
    assert bad == 0, (what, bad, np.argwhere(exact & ~(id_ok & (keys == rk[:, :k])))[:5])
    return int(near.sum()), int(c0.size)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(w).view(np.uint8)) for u, w in zip(a, b))


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _corpus(rng, copies=1):
    """Rows a * centre[key] + g with the corpus' group sizes (tests/golden/chunker.json), shuffled; keys are arbitrary int64."""
    counts = np.array(list(json.load(open(os.path.join(HERE, "golden", "chunker.json")))["counts"].values()), np.int64)
    counts = np.tile(counts, copies)
    ng = counts.shape[0]
    key_vals = rng.choice(1 << 62, size=ng, replace=False).astype(np.int64) - (1 << 61)
    owner = np.repeat(np.arange(ng), counts)
    rng.shuffle(owner)
    centre = rng.standard_normal((ng, D)).astype(np.float32)
    x = centre[owner]
    x += rng.standard_normal(x.shape, dtype=np.float32)
    return x, key_vals[owner], centre


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(31)
    x, keys, centre = _corpus(rng)
    assert x.shape[0] == 32_717 and np.unique(keys).size == 3_027
    q = centre[rng.integers(0, centre.shape[0], 1500)] + rng.standard_normal((1500, D)).astype(np.float32)
    return x, keys, q.astype(np.float32)


@pytest.fixture(scope="module")
def index(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, keys, _ = data
    idx = VectorIndex(ctx, D)
    idx.add(x)
    idx.set_keys(np.arange(x.shape[0]), keys)
    return idx


@pytest.fixture(scope="module")
def ref257(data):
    x, keys, q = data
    return reference(x, q, keys, np.arange(x.shape[0]), 256)


# ---------------------------------------------------------------- 1. FLAT against the reference
@pytest.mark.parametrize("k", [1, 3, 10, 64, 256])
def test_flat_against_reference(ctx, data, index, ref257, k):
    _, _, q = data
    skipped = positions = 0
    for b in (1, 64, 1024, 1500):
        got = index.search_collapsed(q[:b], k)
        swept = ctx.stats()["collapse_swept"]
        print(f"[collapse] k={k} B={b}: swept {swept} of {b}")
        s, p = compare(got, ref257, k, f"flat k={k} B={b}", cap=False)
        skipped, positions = skipped + s, positions + p
        if k <= 10:
            assert swept == 0            # the automatic depth sees k documents for every query of this data
        if k == 256:
            assert swept == b            # 256 rows of the ranking never hold 256 documents here
    print(f"[collapse] flat k={k}: skipped {skipped} of {positions} positions ({100 * skipped / positions:.3f} %)")
    assert skipped <= 0.03 * positions, (k, skipped, positions)


# ---------------------------------------------------------------- 2. self-consistency, no tolerance
def test_self_consistency(data, index):
    _, keys, q = data
    for k in (10, 256):
        cos, ids, gk = index.search_collapsed(q[:6], k)
        for i in range(6):
            assert np.unique(gk[i]).size == k                      # a key never appears twice in one output row
            for j in range(0, k, 1 if k == 10 else 37):
                rows = np.flatnonzero(keys == gk[i, j])
                c1, i1 = index.search(q[i:i + 1], 1, filter_ids=rows)
                assert i1[0, 0] == ids[i, j] and c1.view(np.uint32)[0, 0] == cos.view(np.uint32)[i, j]
                assert keys[ids[i, j]] == gk[i, j]


# ---------------------------------------------------------------- 3. rows without keys
def test_rows_without_keys(ctx, data):
    from semantic_query_engine_amd import VectorIndex
    x, keys, q = data
    n = 12_000
    idx = VectorIndex(ctx, D)
    idx.add(x[:n])
    for k in (1, 10, 64, 256):
        c0, i0 = idx.search(q[:200], k)
        c1, i1, k1 = idx.search_collapsed(q[:200], k)
        assert same_bits((c0, i0), (c1, i1)) and np.all(k1 == NONE)
    half = keys[:n].copy()
    half[1::2] = NONE
    idx.set_keys(np.arange(n), half)
    assert np.array_equal(idx.get_keys(np.arange(n)), half)
    for k in (10, 64):
        compare(idx.search_collapsed(q[:200], k), reference(x[:n], q[:200], half, np.arange(n), k), k, f"half keyed k={k}")
    idx.set_keys(np.arange(n), np.full(n, NONE))                   # keys removed again: a plain search
    c0, i0 = idx.search(q[:50], 10)
    c1, i1, k1 = idx.search_collapsed(q[:50], 10)
    assert same_bits((c0, i0), (c1, i1)) and np.all(k1 == NONE)
    idx.close()


# ---------------------------------------------------------------- 4. the crowd: stage B on a FLAT index
CROWD_KEY = 7_777_777_777


@pytest.fixture(scope="module")
def crowd_data(data):
    x, keys, q = data
    rng = np.random.default_rng(32)
    c0 = rng.standard_normal(D).astype(np.float32)
    crowd = c0 + 1e-3 * rng.standard_normal((3000, D)).astype(np.float32)
    xs = np.concatenate([x[:20_000], crowd, x[20_000:]])
    ks = np.concatenate([keys[:20_000], np.full(3000, CROWD_KEY, np.int64), keys[20_000:]])
    qq = q[:64].copy()
    qq[:16] = c0 + 0.5 * rng.standard_normal((16, D)).astype(np.float32) + 0.5 * q[:16]
    return xs, ks, qq


@pytest.fixture(scope="module")
def crowd_index(ctx, crowd_data):
    from semantic_query_engine_amd import VectorIndex
    xs, ks, _ = crowd_data
    idx = VectorIndex(ctx, D)
    idx.add(xs)
    idx.set_keys(np.arange(xs.shape[0]), ks)
    return idx


def test_crowd(ctx, crowd_data, crowd_index):
    xs, ks, qq = crowd_data
    ref = reference(xs, qq, ks, np.arange(xs.shape[0]), 10)
    assert np.all(ref[2][:16, 0] == CROWD_KEY)                     # the crowd is the best document of the queries aimed at it
    got = crowd_index.search_collapsed(qq, 10)
    swept = ctx.stats()["collapse_swept"]
    print(f"[collapse] crowd: swept {swept} of 64")
    assert swept >= 16
    compare(got, ref, 10, "crowd k=10", crowd_key=CROWD_KEY)
    cos, ids, gk = got
    assert np.all((gk == CROWD_KEY).sum(axis=1) <= 1)              # once
    xn, qn = _norm64(xs), _norm64(qq)
    for i in range(16):
        assert gk[i, 0] == CROWD_KEY and 20_000 <= ids[i, 0] < 23_000
        c = xn[20_000:23_000] @ qn[i]
        assert c.max() - c[ids[i, 0] - 20_000] <= TOL
    crowd_index.set_option("range_key_budget", 4096)
    small = crowd_index.search_collapsed(qq, 10)
    crowd_index.set_option("range_key_budget", 1 << 25)
    assert same_bits(got, small)


# ---------------------------------------------------------------- 5. the depth does not change the answer
def test_depth_gives_same_bits(data, index, crowd_data, crowd_index):
    _, _, q = data
    for idx, qq, shapes in ((index, q, ((1, 3), (64, 10), (300, 64), (1100, 10))), (crowd_index, crowd_data[2], ((64, 10), (20, 3)))):
        for b, k in shapes:
            auto = idx.search_collapsed(qq[:b], k)
            for depth in (k, 256):
                idx.set_option("collapse_depth", depth)
                got = idx.search_collapsed(qq[:b], k)
                idx.set_option("collapse_depth", 0)
                assert same_bits(auto, got), (b, k, depth)


# ---------------------------------------------------------------- 6. fewer than k groups, empty index, B == 0
def test_padding_and_empty(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(33)
    x = rng.standard_normal((40, D)).astype(np.float32)
    q = rng.standard_normal((5, D)).astype(np.float32)
    keys = np.arange(40, dtype=np.int64) // 8 + 100                # 5 groups
    keys[39] = NONE                                                # ... and one row by itself
    idx = VectorIndex(ctx, D)
    c, i, g = idx.search_collapsed(q, 4)                           # empty index
    assert np.all(np.isneginf(c)) and np.all(i == -1) and np.all(g == NONE)
    idx.add(x)
    idx.set_keys(np.arange(40), keys)
    ref = reference(x, q, keys, np.arange(40), 10)
    assert np.all(ref[1][:, 6:] == -1)
    got = idx.search_collapsed(q, 10)
    compare(got, ref, 10, "six groups, k=10")
    assert np.all(got[1][:, :6] >= 0) and np.all(got[1][:, 6:] == -1) and np.all(np.isneginf(got[0][:, 6:])) and np.all(got[2][:, 6:] == NONE)
    c, i, g = idx.search_collapsed(np.zeros((0, D), np.float32), 3)
    assert c.shape == (0, 3) and i.shape == (0, 3) and g.shape == (0, 3)
    idx.close()


# ---------------------------------------------------------------- 7. keys move with their rows
def test_keys_follow_rows(ctx, tmp_path):
    from semantic_query_engine_amd import VectorIndex, _native
    rng = np.random.default_rng(34)
    n, base = 6000, 1000
    centre = rng.standard_normal((1000, D)).astype(np.float32)
    owner = rng.permutation(np.repeat(np.arange(1000), 6))
    x = centre[owner] + rng.standard_normal((n, D)).astype(np.float32)
    keys = (owner.astype(np.int64) * 1_000_003 - 5_000_000)
    q = centre[rng.integers(0, 1000, 96)] + rng.standard_normal((96, D)).astype(np.float32)
    idx = VectorIndex(ctx, D)
    idx.reserve(n)
    idx.set_option("id_base", base)
    idx.add(x)
    idx.set_keys(np.arange(n), keys)
    # a third of the rows leave: whole documents (owner % 5 == 0) and single chunks
    dead = (owner % 5 == 0) | (rng.random(n) < 0.16)
    idx.delete(np.flatnonzero(dead))
    live = np.flatnonzero(~dead)
    assert np.array_equal(idx.get_keys(live), keys[live])
    # rows past the reserved capacity: they start without a key; some get one of an existing document, some a new one
    extra_owner = rng.integers(0, 1000, 3000)
    xe = centre[extra_owner] + rng.standard_normal((3000, D)).astype(np.float32)
    idx.add(xe)
    new_ids = np.arange(n, n + 3000)
    assert np.all(idx.get_keys(new_ids) == NONE) and np.array_equal(idx.get_keys(live), keys[live])
    ke = np.where(np.arange(3000) % 3 == 0, NONE, extra_owner.astype(np.int64) * 1_000_003 - 5_000_000)
    idx.set_keys(new_ids, ke)
    # overwrite some rows: the key stays with the row
    upd = live[::50]
    xu = centre[(owner[upd] + 1) % 1000] + rng.standard_normal((upd.shape[0], D)).astype(np.float32)
    idx.update(upd, xu)
    x_all = np.concatenate([x, xe])
    x_all[upd] = xu
    k_all = np.concatenate([keys, ke])
    ids_live = np.concatenate([live, new_ids])
    assert np.array_equal(idx.ids(), ids_live) and np.array_equal(idx.get_keys(ids_live), k_all[ids_live])
    ref = reference(x_all[ids_live], q, k_all[ids_live], ids_live + base, 10)
    got = idx.search_collapsed(q, 10)
    compare(got, ref, 10, "after delete / add / update")
    gone = set((owner[dead & (owner % 5 == 0)].astype(np.int64) * 1_000_003 - 5_000_000).tolist()) - set(ke.tolist())
    assert not (set(got[2].ravel().tolist()) & gone)               # a deleted document never appears
    big = idx.search_collapsed(q[:8], 256)                         # the sweep reads the moved keys too
    compare(big, reference(x_all[ids_live], q[:8], k_all[ids_live], ids_live + base, 256), 256, "after delete / add / update k=256")
    # a dead id: SQE_ERR_INVALID and nothing written
    before = idx.get_keys(ids_live)
    with pytest.raises(_native.SqeError) as e:
        idx.set_keys(np.array([ids_live[0], int(np.flatnonzero(dead)[0])]), np.array([1, 2]))
    assert e.value.code == -1
    with pytest.raises(_native.SqeError):
        idx.get_keys(np.array([int(np.flatnonzero(dead)[0])]))
    assert np.array_equal(idx.get_keys(ids_live), before)
    # a repeated id: the last key wins
    idx.set_keys(np.array([ids_live[3], ids_live[3]]), np.array([11, 12]))
    assert idx.get_keys(ids_live[3:4])[0] == 12
    # save / load: keys are not in the file
    path = str(tmp_path / "keys.sqe")
    idx.save(path)
    loaded = VectorIndex.load(ctx, path)
    assert np.all(loaded.get_keys(ids_live) == NONE)
    c0, i0 = loaded.search(q, 10)
    c1, i1, k1 = loaded.search_collapsed(q, 10)
    assert same_bits((c0, i0), (c1, i1)) and np.all(k1 == NONE)
    loaded.close()
    idx.close()


def test_never_keyed_index_saves_the_same_file(ctx, tmp_path):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(35)
    x = rng.standard_normal((3000, D)).astype(np.float32)
    a, b = VectorIndex(ctx, D), VectorIndex(ctx, D)
    a.add(x)
    b.add(x)
    b.set_keys(np.arange(3000), np.arange(3000) // 7)
    b.search_collapsed(x[:4], 5)
    a.save(str(tmp_path / "a.sqe"))
    b.save(str(tmp_path / "b.sqe"))
    assert open(str(tmp_path / "a.sqe"), "rb").read() == open(str(tmp_path / "b.sqe"), "rb").read()
    a.close()
    b.close()


# ---------------------------------------------------------------- 8. IVF equals FLAT
def test_ivf_equals_flat(ctx, data, index):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    x, keys, q = data
    ivf = VectorIndex(ctx, D, INDEX_IVF_FLAT, 64)
    ivf.add(x)
    ivf.train(x[:10_000], iters=5, seed=1)
    ivf.set_keys(np.arange(x.shape[0]), keys)
    for b, k in ((64, 10), (33, 64), (5, 256)):
        got = ivf.search_collapsed(q[:b], k)
        assert ctx.stats()["collapse_swept"] == b                  # an IVF index answers every query with the sweep
        assert same_bits(got, index.search_collapsed(q[:b], k)), (b, k)
    ivf.close()


# ---------------------------------------------------------------- 9. device groups
@pytest.mark.parametrize("P", [2, 3])
def test_group_equals_single_device(ctx, crowd_data, crowd_index, P):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    xs, ks, qq = crowd_data
    rng = np.random.default_rng(36)
    # one query whose ten best documents all sit on rows of shard 0 (ids that are multiples of 6, for P = 2 and 3 alike)
    qs = rng.standard_normal(D).astype(np.float32)
    xs, ks = xs.copy(), ks.copy()
    spots = np.arange(0, 6 * 30, 6)
    xs[spots] = qs * np.linspace(3.0, 2.0, 30)[:, None].astype(np.float32) + rng.standard_normal((30, D)).astype(np.float32)
    ks[spots] = 9_000_000_000 + np.arange(30) // 3
    qq = np.concatenate([qq, qs[None]])
    single = VectorIndex(ctx, D)
    single.add(xs)
    single.set_keys(np.arange(xs.shape[0]), ks)
    want = single.search_collapsed(qq, 10)
    assert np.all(want[1][-1] % 6 == 0) and np.all(want[2][-1] >= 9_000_000_000)
    gctx = Context(devices=[0] * P, exchange=EXCHANGE_COPY)
    g = VectorIndex(gctx, D)
    g.add(xs)
    g.set_keys(np.arange(xs.shape[0]), ks)
    assert np.array_equal(g.get_keys(np.arange(0, xs.shape[0], 7)), ks[::7])
    assert same_bits(g.search_collapsed(qq, 10), want)
    assert gctx.stats()["collapse_swept"] > 0                      # the crowd queries were swept on the shards
    assert same_bits(g.search_collapsed(qq[:9], 64), single.search_collapsed(qq[:9], 64))
    g.close()
    gctx.close()
    single.close()


# ---------------------------------------------------------------- 10. above i8_min_rows: the int8 first pass in stage A
def test_int8_first_pass_and_large_sweep(ctx):
    from semantic_query_engine_amd import VectorIndex
    rng = np.random.default_rng(37)
    x, keys, centre = _corpus(rng, copies=32)
    n = x.shape[0]
    assert n == 1_046_944 and centre.shape[0] == 96_864
    b, k = 256, 10
    q = (centre[rng.integers(0, centre.shape[0], b)] + rng.standard_normal((b, D)).astype(np.float32)).astype(np.float32)
    idx = VectorIndex(ctx, D)
    idx.reserve(n)
    idx.add(x)
    idx.set_keys(np.arange(n), keys)
    idx.set_option("collapse_depth", 20)
    ctx.stats_reset()
    got = idx.search_collapsed(q, k)
    st = ctx.stats()
    last = idx.i8_last()                                           # raises unless the int8 first pass answered
    print(f"[collapse] 1M rows: swept {st['collapse_swept']} of {b}, i8_collected {st['i8_collected']}, int8 depth {last['k']}")
    assert last["rows"] == n and last["k"] == 20 and st["i8_collected"] > 0
    assert st["collapse_swept"] > 0
    # blocked float64 reference on the host: per block of rows the best row of every group, merged across blocks
    qn = _norm64(q)
    gid = _groups(keys)
    ng = int(gid.max()) + 1
    best_c = np.full((b, ng), -np.inf)
    best_r = np.full((b, ng), n, np.int64)
    order = np.argsort(gid, kind="stable")                         # rows of a group together, ascending id inside
    starts = np.flatnonzero(np.r_[True, np.diff(gid[order]) != 0])
    for r0 in range(0, ng, 8192):
        g1 = min(ng, r0 + 8192)
        rows = order[starts[r0]:(starts[g1] if g1 < ng else n)]
        c = qn @ _norm64(x[rows]).T                                # [b, rows of these groups]
        seg = starts[r0:g1] - starts[r0]
        mx = np.maximum.reduceat(c, seg, axis=1)
        best_c[:, r0:g1] = mx
        grp = np.repeat(np.arange(g1 - r0), np.diff(np.r_[seg, rows.shape[0]]))
        hit = c == mx[:, grp]
        pos = np.where(hit, rows[None, :], n)
        best_r[:, r0:g1] = np.minimum.reduceat(pos, seg, axis=1)
    rc = np.full((b, k + 1), -np.inf)
    ri = np.full((b, k + 1), -1, np.int64)
    for i in range(b):
        top = np.lexsort((best_r[i], -best_c[i]))[:k + 1]
        rc[i], ri[i] = best_c[i, top], best_r[i, top]
    compare(got, (rc, ri, keys[ri]), k, "1M rows, depth 20, k=10")
    idx.close()


# ---------------------------------------------------------------- 11. entry points, plain search untouched, invalid arguments
def test_device_entry_plain_search_and_invalid(ctx, data, index):
    import torch
    from semantic_query_engine_amd import _native
    _, _, q = data
    b = 80
    p0 = index.search(q[:b], 10)
    for k in (10, 256):
        host = index.search_collapsed(q[:b], k)
        qd = torch.from_numpy(q[:b]).cuda()
        cd = torch.empty((b, k), dtype=torch.float32, device="cuda")
        idd = torch.empty((b, k), dtype=torch.int64, device="cuda")
        kd = torch.empty((b, k), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        index.search_collapsed_device(qd.data_ptr(), b, k, cd.data_ptr(), idd.data_ptr(), kd.data_ptr())
        ctx.synchronize()
        assert same_bits(host, (cd.cpu().numpy(), idd.cpu().numpy(), kd.cpu().numpy()))
    assert same_bits(p0, index.search(q[:b], 10))
    lib = _native.load()
    qq = np.ascontiguousarray(q[:3])
    c = np.empty((3, 4), np.float32)
    i = np.empty((3, 4), np.int64)
    g = np.empty((3, 4), np.int64)
    args = (c.ctypes.data, i.ctypes.data, g.ctypes.data)
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, 3, 4, *args) == 0
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, 3, 0, *args) == -1
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, 3, 257, *args) == -1
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, -1, 4, *args) == -1
    assert lib.sqe_index_search_collapsed(index.handle, None, 3, 4, *args) == -1
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, 3, 4, None, i.ctypes.data, g.ctypes.data) == -1
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, 3, 4, c.ctypes.data, None, g.ctypes.data) == -1
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, 3, 4, c.ctypes.data, i.ctypes.data, None) == -1
    assert lib.sqe_index_search_collapsed(None, qq.ctypes.data, 3, 4, *args) == -1
    assert lib.sqe_index_search_collapsed(index.handle, qq.ctypes.data, 0, 4, *args) == 0
    assert lib.sqe_index_set_keys(index.handle, None, None, 3) == -1 and lib.sqe_index_get_keys(index.handle, None, 3, None) == -1
    with pytest.raises(_native.SqeError):
        index.set_option("collapse_depth", 257)
