"""The stages of an IVF search, read back (sqe_index_ivf_state[_read]) and compared with oracle/ivf.py: every list-scan route, every
score strip, the list-ordered int8 copy, the collect mode's thresholds and key lists, and the k-means training.  GPU only.

The structure is fixed, not hoped for: centres are orthonormal (nlist <= dim) or random unit vectors; the index is trained on
exactly those nlist rows with iters = 1, so every row is a pick and its own list; rows are centre + small noise with a chosen
count per list, queries the normalised sum of the centres they are meant to probe + small noise.  Every case asserts the list
lengths on the exported assignment, the probing counts on the probes it reads back and its route on ivf_state() before it
compares anything.  Strips are compared at EVERY position below the probed list's length, for EVERY (query, probe) pair.

Lengths (ivf_scan.hip, and the unit tables of ivf.hip): 0 (empty list), 1, 255 / 256 / 257 (around a 256-row tile), 1281 (6 tiles: units 3 + 3), 2304 (9 tiles: units
5 + 4, a whole last tile), 2305 (10 tiles: 5 + 5, one row in the last), 4097 (17 tiles: 5 + 4 + 4 + 4, just past LS_SEG = 4096).
"""
import numpy as np
import pytest

from oracle import ivf as IV
from oracle import retrieval as R
from oracle import rounding as RD
from tests.gpu_util import assert_topk_matches

pytestmark = pytest.mark.gpu

LENS = [0, 1, 255, 256, 257, 1281, 2305, 4097, 300, 2304]      # list 8 is probed by nobody
NOBODY = 8
# (queries, lists they probe): list 7 (4097 rows) is probed by 65 queries (LS_Q = 64: two query groups, ST_Q = 32: three), list 0
# (empty) and list 1 by 33 (ST_Q = 32: two), the last group probes 769 rows (<= IVF_LIST_CAP / 4: the collect mode lists them all)
GROUPS5 = [(33, (0, 1, 2, 7, 9)), (32, (1, 2, 3, 7, 9)), (40, (3, 4, 5, 6, 9)), (5, (0, 1, 2, 3, 4))]
ALL8 = (0, 1, 2, 3, 4, 5, 6, 7)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _E():
    from semantic_query_engine_amd import engine as E
    return E


def _kp(k):
    return min(256, max(32, 4 * k))


def _centres(nlist, dim, seed):
    rng = np.random.default_rng(seed)
    if nlist <= dim:
        qm, _ = np.linalg.qr(rng.standard_normal((dim, nlist)))
        return np.ascontiguousarray(qm.T).astype(np.float32)
    return R.normalize_rows(rng.standard_normal((nlist, dim)).astype(np.float32))


class Built:
    pass


def _build(ctx, dim, lens, seed, sigma=0.3, check_copy=True):
    """-> index with list i holding exactly lens[i] rows (asserted), its centroids, the raw rows and their lists"""
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    nlist = len(lens)
    cen = _centres(nlist, dim, seed)
    idx = VectorIndex(ctx, dim, INDEX_IVF_FLAT, nlist)
    idx.train(cen, iters=1, seed=seed)
    centroids, _ = idx.ivf_export(nlist)
    picks = IV.train_picks(nlist, nlist, seed)                   # every row is a pick: list i starts from (and stays) centre picks[i]
    assert np.allclose(centroids, cen[picks], atol=2e-6)
    rng = np.random.default_rng(seed + 1)
    lab = rng.permutation(np.repeat(np.arange(nlist), lens))
    x = centroids[lab] + np.float32(sigma / np.sqrt(dim)) * rng.standard_normal((lab.size, dim), dtype=np.float32)
    idx.add(x)
    _, assign = idx.ivf_export(nlist)
    assert np.array_equal(assign, lab) and np.array_equal(np.bincount(assign, minlength=nlist), lens)
    b = Built()
    b.idx, b.dim, b.nlist, b.lens, b.centroids, b.x, b.assign = idx, dim, nlist, list(lens), centroids, x, assign.copy()
    b.copy_checked, b.check_copy = False, check_copy
    return b


def _queries(centroids, groups, seed, sigma=0.2):
    """groups: (count, lists to probe) -> raw queries, and the target tuple of each"""
    rng = np.random.default_rng(seed)
    dim = centroids.shape[1]
    qs, targets = [], []
    for count, lists in groups:
        base = centroids[list(lists)].sum(0)
        noise = sigma * np.sqrt(len(lists)) / np.sqrt(dim) * rng.standard_normal((count, dim))
        qs.append((base[None, :] + noise) * rng.uniform(0.5, 2.0, (count, 1)))       # (queries are not unit vectors)
        targets += [tuple(lists)] * count
    return np.concatenate(qs).astype(np.float32), targets


def _read_structure(idx, st):
    E = _E()
    order = idx.ivf_state_read(E.IVF_ORDER, np.int32, st["n_assigned"]) if st["n_assigned"] else np.zeros(0, np.int32)
    offsets = idx.ivf_state_read(E.IVF_OFFSETS, np.int64, st["nlist"] + 1)
    return order, offsets


def _check_int8_copy(idx, st, x_live, order, offsets, compare=True):
    """bytes and scales of the list-ordered int8 copy against oracle.ivf.i8_rows_of_lists on the normalised rows the index holds
    -> (int8 rows, integer scales) by list position, as the device holds them (compare = False: only read)"""
    E = _E()
    n, dim = st["n_assigned"], st["dim"]
    assert st["i8_tile_stride"] == IV.tile_stride(dim)
    tiles = st["total_tiles"]
    if not compare:
        raw = idx.ivf_state_read(E.IVF_I8_ROWS, np.int8, tiles * st["i8_tile_stride"]).reshape(tiles, st["i8_tile_stride"])
        pos = IV.copy_positions(offsets)
        return IV.untile(raw, pos, dim), idx.ivf_state_read(E.IVF_I8_ROW_SCALES, np.uint32, tiles * 256)[pos]
    xn = idx.ivf_state_read(E.IVF_ROWS_F32, np.float32, n * dim).reshape(n, dim)
    assert np.allclose(xn, R.normalize_rows(x_live), atol=1e-6)
    assert np.array_equal(np.sort(order), np.arange(n))
    tile_off = idx.ivf_state_read(E.IVF_TILE_OFF, np.int64, st["nlist"] + 1)
    assert np.array_equal(tile_off, IV.tile_offsets(offsets)) and tile_off[-1] == tiles
    raw = idx.ivf_state_read(E.IVF_I8_ROWS, np.int8, tiles * st["i8_tile_stride"]).reshape(tiles, st["i8_tile_stride"])
    sxi = idx.ivf_state_read(E.IVF_I8_ROW_SCALES, np.uint32, tiles * 256)
    ref_tiled, ref_scales, pos = IV.i8_rows_of_lists(xn, order, offsets)
    dev_sx, ref_sx = sxi[pos], ref_scales[pos]
    diff = dev_sx != ref_sx
    if diff.any():
        # the integer scale is a ceil() the kernel evaluates in float32: it may differ from the float64 one by one step where, and
        # only where, that float64 value lies within float32 rounding of an integer (oracle.ivf.scale_boundary); the bytes are
        # then held to the scale the device took
        assert np.all(IV.scale_boundary(xn[order])[diff]), np.flatnonzero(diff)
        assert np.all(np.abs(dev_sx[diff].astype(np.int64) - ref_sx[diff].astype(np.int64)) == 1)
        assert diff.sum() <= max(1, n // 1000), diff.sum()
        ref_tiled, _, _ = IV.i8_rows_of_lists(xn, order, offsets, scales=dev_sx)
    x8_dev, x8_ref = IV.untile(raw, pos, dim), IV.untile(ref_tiled, pos, dim)
    bad = np.flatnonzero((x8_dev != x8_ref).any(axis=1))
    assert bad.size == 0, (bad[:10], order[bad[:10]])
    return x8_dev, dev_sx


def _check_strips(b, st, order, offsets, sample_only=False):
    """every (query, probe) strip at every position of its list against the restatement; -> (probes, estimates per (list, query))"""
    E = _E()
    idx, dim = b.idx, st["dim"]
    B, nprobe, max_len, n = st["B"], st["nprobe"], st["max_len"], st["n_assigned"]
    probes = idx.ivf_state_read(E.IVF_PROBES, np.int64, B * nprobe).reshape(B, nprobe)
    strips = idx.ivf_state_read(E.IVF_STRIPS, np.float32, B * nprobe * max_len).reshape(B * nprobe, max_len)
    lens = np.diff(offsets)
    assert max_len == (max(int(lens.max()), 1) + 3) // 4 * 4
    i8 = st["list_kernel"] in (E.IVF_KERNEL_I8_STAGED, E.IVF_KERNEL_I8_STREAM)
    if i8:
        x8, sx = b.x8, b.sx
        q8 = idx.ivf_state_read(E.IVF_Q8, np.int8, B * st["q8_pitch"]).reshape(B, st["q8_pitch"])[:, :dim]
        sqi = idx.ivf_state_read(E.IVF_Q8_SCALES, np.uint32, B)
        assert st["q8_pitch"] == dim + 128
    else:
        pitch = st["scan_pitch"] // 2
        scan = idx.ivf_state_read(E.IVF_SCAN_BF16, np.uint16, n * pitch).reshape(n, pitch)[:, :dim]
        qb = idx.ivf_state_read(E.IVF_QB, np.uint16, B * pitch).reshape(B, pitch)[:, :dim]
        tol = RD.acc_term(dim)
    flat = probes.reshape(-1)
    worst, est = 0.0, {}
    for L in np.unique(flat):
        assert 0 <= L < st["nlist"]
        pairs = np.flatnonzero(flat == L)
        qs = pairs // nprobe
        ln, off = int(lens[L]), int(offsets[L])
        if ln == 0:
            continue
        lim = min(ln, 256) if sample_only else ln
        got = strips[pairs, :lim].T                                   # [positions, queries]
        if i8:
            ref = IV.i8_strip(x8[off:off + ln], sx[off:off + ln], q8[qs], sqi[qs], dim)
            est[int(L)] = (qs, ref)
            same = got.view(np.uint32) == ref[:lim].view(np.uint32)
            assert same.all(), (int(L), ln, np.argwhere(~same)[:8].tolist(), got[~same][:4], ref[:lim][~same][:4])
        else:
            ref = IV.bf16_strip(scan[order[off:off + ln]], qb[qs])
            dev = np.abs(got.astype(np.float64) - ref[:lim])
            assert np.all(dev <= tol), (int(L), ln, np.argwhere(dev > tol)[:8].tolist(), float(dev.max()), tol)
            worst = max(worst, float(dev.max()))
    if not i8:
        print(f"dim {dim} B {B} nprobe {nprobe}: largest bf16 strip deviation {worst:.3e} = {worst / tol:.4f} of acc_term({dim}) = {tol:.3e}")
    return probes, est


def _check_collect(b, st, order, offsets, probes, est):
    """the collect mode: thresholds by the rank rule, key lists as sets, totals; est: full estimates per probed list"""
    E = _E()
    idx = b.idx
    B, nprobe, kp, cap = st["B"], st["nprobe"], st["kp"], st["list_cap"]
    assert cap == IV.IVF_LIST_CAP and st["fallback"] == 0
    thr = idx.ivf_state_read(E.IVF_THRESHOLDS, np.float32, B)
    cnt = idx.ivf_state_read(E.IVF_COUNTS, np.int32, 2 * B)
    lists = idx.ivf_state_read(E.IVF_KEY_LISTS, np.uint64, B * cap).reshape(B, cap)
    lens = np.diff(offsets)
    col = {L: {int(q): j for j, q in enumerate(qs)} for L, (qs, _) in est.items()}
    n_inf = n_thr = 0
    for q in range(B):
        e_all, ids_all, sample = [], [], []
        for L in probes[q]:
            ln, off = int(lens[L]), int(offsets[L])
            if ln == 0:
                continue
            e = est[int(L)][1][:, col[int(L)][q]]
            e_all.append(e)
            ids_all.append(order[off:off + ln])
            sample.append(e[:256])
        total = int(lens[probes[q]].sum())
        assert cnt[B + q] == total
        sample = np.concatenate(sample) if sample else np.zeros(0, np.float32)
        want = IV.collect_want(sample.size, total, kp)
        if want == 0:
            assert np.isneginf(thr[q]), (q, thr[q], total)
            n_inf += 1
        else:
            assert IV.threshold_rank_ok(sample, thr[q], want), (q, float(thr[q]), want, int((sample > thr[q]).sum()), int((sample >= thr[q]).sum()))
            n_thr += 1
        ref = IV.collect_reference(e_all, ids_all, thr[q])
        assert cnt[q] == ref.size, (q, int(cnt[q]), ref.size)
        if want == 0:
            assert ref.size == total
        assert ref.size <= cap
        assert np.array_equal(np.sort(lists[q, :cnt[q]]), ref), q
    return n_inf, n_thr


def _search_and_check(b, q, targets, k, nprobe, kernel, grid, split=0):
    """one search: route, probing counts, int8 copy (first time), strips, collect state, then the top-k against the oracle"""
    E = _E()
    idx = b.idx
    cos, ids = idx.search(q, k, nprobe=nprobe)
    st = idx.ivf_state()
    assert (st["list_kernel"], st["grid"], st["split"]) == (kernel, grid, split), st
    assert st["sub_batches"] == 1 and st["B"] == q.shape[0] and st["nprobe"] == nprobe and st["k"] == k and st["kp"] == _kp(k)
    assert st["dim"] == b.dim and st["nlist"] == b.nlist and st["n_assigned"] == b.x.shape[0]
    assert st["coarse"] == (E.IVF_COARSE_DENSE if b.nlist % 128 == 0 else E.IVF_COARSE_FLAT)
    order, offsets = _read_structure(idx, st)
    assert np.array_equal(np.diff(offsets), np.bincount(b.assign, minlength=b.nlist))
    assert np.array_equal(b.assign[order], np.repeat(np.arange(b.nlist), np.diff(offsets)))
    i8 = kernel in (E.IVF_KERNEL_I8_STAGED, E.IVF_KERNEL_I8_STREAM)
    if i8 and not b.copy_checked:
        b.x8, b.sx = _check_int8_copy(idx, st, b.x, order, offsets, compare=b.check_copy)
        b.copy_checked = True
    collect = grid == E.IVF_GRID_COLLECT
    probes, est = _check_strips(b, st, order, offsets, sample_only=collect)
    if targets is not None:
        for i, t in enumerate(targets):
            assert set(probes[i].tolist()) == set(t), (i, probes[i], t)
    if collect:
        n_inf, n_thr = _check_collect(b, st, order, offsets, probes, est)
        print(f"dim {b.dim}: collect mode, {n_thr} thresholds by rank, {n_inf} at -inf, queued {st['queued']}")
    xn, qn = R.normalize_rows(b.x), R.normalize_rows(q)
    ref_cos, ref_ids = R.ivf_search(xn, qn, b.centroids, b.assign, k, nprobe)
    assert_topk_matches(cos, ids, ref_cos, ref_ids, xn, qn)
    return st, probes


# ---------------------------------------------------------------- the dim routes x the length and group edges
_built = {}


def _case(ctx, dim):
    if dim not in _built:
        _built[dim] = _build(ctx, dim, LENS, seed=1000 + dim)
    return _built[dim]


def _route(dim, name):
    """(list kernel, grid, split) ivf.hip takes for this dim and search (ivf_route_plan; its gates restated in the comments of SEARCHES)"""
    E = _E()
    if dim < 256 or dim % 128:
        return E.IVF_KERNEL_BF16_MFMA, E.IVF_GRID_LIST, 0
    st_lds = 32 * (dim + 128) + 5 * 256 * 4 + 32 * 8 + 4 * 36 * 68 * 4
    if dim % 256 == 0 and st_lds <= 80 * 1024:
        return E.IVF_KERNEL_I8_STREAM, {"list": E.IVF_GRID_COLLECT, "b64": E.IVF_GRID_UNITS1}.get(name, E.IVF_GRID_PAIR_GRID), 0
    if name == "list":
        return E.IVF_KERNEL_I8_STAGED, E.IVF_GRID_LIST, 0
    return E.IVF_KERNEL_I8_STAGED, E.IVF_GRID_PAIR, {"long": 16, "mid": 16, "b3": 16, "b16": 4, "b64": 1}[name]


# name -> (groups, nprobe).  Pairs = B * nprobe.  Staged pair mode: split = min(16, 512 / pairs) workgroups share a list's tiles.
# Streaming: up to 512 pairs take the pair grid unless pairs * tiles of the longest list (17) exceeds max(8192, 2 * tiles): 512
# pairs do (8704) and take the single-tile unit table; more than 512 pairs with nprobe <= 32 take the collect mode.
SEARCHES = {
    "long": ([(1, (7,))], 1),             # split 16 over 17 tiles: two tiles per segment, segments 9 .. 15 get none
    "mid": ([(1, (6,))], 1),              # split 16 over 10 tiles: segments 10 .. 15 get none
    "b3": ([(3, ALL8)], 8),               # 24 pairs, split 16, empty list included
    "b16": ([(16, ALL8)], 8),             # 128 pairs, split 4
    "b64": ([(64, ALL8)], 8),             # 512 pairs, split 1: a whole 4097-row list per workgroup (two segments)
    "list": (GROUPS5, 5),                 # 550 pairs: one workgroup per list / the collect mode
}
# 1024 (the streaming kernel at its LDS limit) and 1280 (the staged kernel by the LDS gate) keep the 4097-row list
CASES = [(64, "long"), (64, "list"), (320, "b3"), (320, "list"),
         (384, "long"), (384, "mid"), (384, "b3"), (384, "b16"), (384, "b64"), (384, "list"),
         (1280, "long"), (1280, "b64"), (1280, "list"),
         (256, "long"), (256, "mid"), (256, "b3"), (256, "b16"), (256, "b64"), (256, "list"),
         (1024, "long"), (1024, "b64"), (1024, "list")]


@pytest.mark.parametrize("dim,name", CASES)
def test_list_scan_routes_and_strips(ctx, dim, name):
    E = _E()
    b = _case(ctx, dim)
    groups, nprobe = SEARCHES[name]
    q, targets = _queries(b.centroids, groups, seed=dim * 7 + len(name))
    kernel, grid, split = _route(dim, name)
    st, probes = _search_and_check(b, q, targets, 10, nprobe, kernel, grid, split)
    if name == "list":
        per_list = np.bincount(probes.reshape(-1), minlength=b.nlist)
        assert per_list[7] == 65 and per_list[0] == 38 and per_list[NOBODY] == 0 and per_list[9] == 105
        assert q.shape[0] * nprobe > 512
    if grid == E.IVF_GRID_UNITS1:
        tiles = (np.asarray(b.lens) + 255) // 256
        assert st["n_units1"] == tiles.sum() and q.shape[0] * nprobe * tiles.max() > max(8192, 2 * st["n_units1"])
    if grid == E.IVF_GRID_COLLECT:
        # the sample is the first tile of every non-empty list, the rest are runs of <= 5 tiles
        assert st["n_unitsS"] == np.count_nonzero(b.lens) and st["n_unitsR"] > 0 and st["queued"] == 0


# ---------------------------------------------------------------- streaming kernel, unit table of <= 5 tiles (strip mode)
def test_stream_units4_more_probes_than_the_collect_mode_takes(ctx):
    """nprobe = 33 > 32 keeps a batch of more than 512 pairs out of the collect mode: ivf_list_stream_i8_kernel over the unit table
    of runs of <= 5 tiles, every list probed by all 33 queries (two query passes per unit)."""
    E = _E()
    lens = LENS[:8] + [2304] + [1 + i % 3 for i in range(31)]
    b = _build(ctx, 256, lens, seed=77)
    groups = [(1, tuple(range(9)) + tuple(9 + (i + j) % 31 for j in range(24))) for i in range(33)]
    q, targets = _queries(b.centroids, groups, seed=78)
    st, probes = _search_and_check(b, q, targets, 10, 33, E.IVF_KERNEL_I8_STREAM, E.IVF_GRID_UNITS4)
    assert st["B"] * st["nprobe"] > 512 and np.bincount(probes.reshape(-1), minlength=40)[7] == 33
    # units: near-equal runs of <= 5 tiles per list
    tiles = (np.asarray(lens) + 255) // 256
    assert st["n_units4"] == sum((t + 4) // 5 for t in tiles) and st["queued"] == 0


# ---------------------------------------------------------------- the persistent unit queue, dense and flat coarse routes
@pytest.mark.parametrize("nlist", [640, 648])
def test_unit_queue_and_coarse_routes(ctx, nlist):
    """More lists than 2 x CUs: the collect mode's launches run persistent workgroups that take units from a queue.  520 lists of
    257 rows (a sample tile and a one-row tile each) and 120 of 1 - 3 rows: the sample pass (640 units), the collect pass (520
    units) and the gated fallback launch (640 units) are all queued.  nlist = 640 is a multiple of 128 and takes the dense coarse
    GEMM + ivf_probe_select_kernel; 648 the flat index over the centroids (there with short lists only: one list of 257 rows,
    so the collect pass has a single unit and only the sample and fallback launches are queued)."""
    E = _E()
    if nlist == 640:
        lens = [257] * 520 + [1 + i % 3 for i in range(120)]
    else:
        lens = [257] + [1 + i % 3 for i in range(647)]
    # (134 k rows at nlist 640: the int8 copy is read for the strip restatement but not compared with the rows again -- every
    # other int8 case here compares it)
    b = _build(ctx, 256, lens, seed=nlist, sigma=0.5, check_copy=nlist != 640)
    # queries sit next to a stored row each: the rows of its list then spread over cosines far wider apart than the int8 estimate
    # errs, so the kp = 40 best estimates hold the true top 10 (rows of one list around a query at their centre would not)
    rng = np.random.default_rng(nlist + 1)
    home = rng.integers(0, nlist, 33)
    home[:4] = [0, 1, nlist - 1, nlist - 2]
    near = np.array([rng.choice(np.flatnonzero(b.assign == h)) for h in home])
    q = (b.x[near] + 0.2 / 16 * rng.standard_normal((33, 256))).astype(np.float32)
    st, probes = _search_and_check(b, q, None, 10, 16, E.IVF_KERNEL_I8_STREAM, E.IVF_GRID_COLLECT)
    assert np.array_equal(probes[:, 0], home)
    assert st["n_unitsS"] == nlist > st["persistent"] and st["n_units4"] == nlist
    if nlist == 640:
        assert st["n_unitsR"] == 520 > st["persistent"]
        assert st["queued"] == E.IVF_QUEUED_SAMPLE | E.IVF_QUEUED_COLLECT | E.IVF_QUEUED_FALLBACK
    else:
        assert st["n_unitsR"] == 1
        assert st["queued"] == E.IVF_QUEUED_SAMPLE | E.IVF_QUEUED_FALLBACK


# ---------------------------------------------------------------- the int8 copy after update and delete
def test_int8_copy_follows_update_and_delete(ctx):
    """update of rows that change their list and delete both reset the list-ordered int8 copy: bytes, scales and strips are checked
    again after each."""
    E = _E()
    lens = [0, 1, 255, 256, 257, 600]
    b = _build(ctx, 256, lens, seed=55)
    q, targets = _queries(b.centroids, [(3, (0, 1, 2, 3, 4, 5))], seed=56)
    route = (E.IVF_KERNEL_I8_STREAM, E.IVF_GRID_PAIR_GRID)
    _search_and_check(b, q, targets, 10, 6, *route)
    # five rows of list 5 move to list 2 (255 -> 260 rows: one more tile), two of list 4 to the empty list 0
    rng = np.random.default_rng(57)
    rows5 = np.flatnonzero(b.assign == 5)[:5]
    rows4 = np.flatnonzero(b.assign == 4)[:2]
    moved = np.concatenate([rows5, rows4])
    to = np.array([2] * 5 + [0] * 2)
    new = (b.centroids[to] + 0.3 / 16 * rng.standard_normal((7, 256))).astype(np.float32)
    b.idx.update(moved, new)
    b.x[moved] = new
    b.assign[moved] = to
    _, assign = b.idx.ivf_export(b.nlist)
    assert np.array_equal(assign, b.assign) and np.bincount(assign, minlength=6).tolist() == [2, 1, 260, 256, 255, 595]
    b.copy_checked = False
    _search_and_check(b, q, targets, 10, 6, *route)
    assert b.copy_checked
    # delete: list 3 drops to 255 rows (one whole tile no more), list 1 becomes empty
    gone = np.concatenate([np.flatnonzero(b.assign == 3)[:1], np.flatnonzero(b.assign == 1), np.flatnonzero(b.assign == 5)[:20]])
    b.idx.delete(b.idx.ids()[gone])
    keep = np.ones(b.x.shape[0], bool)
    keep[gone] = False
    b.x, b.assign = b.x[keep], b.assign[keep]
    _, assign = b.idx.ivf_export(b.nlist)
    assert np.array_equal(assign, b.assign) and np.bincount(assign, minlength=6).tolist() == [2, 0, 260, 255, 255, 575]
    b.copy_checked = False
    cos, ids = b.idx.search(q, 10, nprobe=6)
    st = b.idx.ivf_state()
    assert (st["list_kernel"], st["grid"]) == route and st["n_assigned"] == b.x.shape[0]
    order, offsets = _read_structure(b.idx, st)
    b.x8, b.sx = _check_int8_copy(b.idx, st, b.x, order, offsets)
    _check_strips(b, st, order, offsets)
    xn, qn = R.normalize_rows(b.x), R.normalize_rows(q)
    ref_cos, ref_ids = R.ivf_search(xn, qn, b.centroids, b.assign, 10, 6)
    live = b.idx.ids()
    assert_topk_matches(cos, np.where(ids >= 0, np.searchsorted(live, ids), -1), ref_cos, ref_ids, xn, qn)


# ---------------------------------------------------------------- collect mode: a crowd of identical rows
def test_collect_mode_crowd_takes_the_direct_append_path(ctx):
    """1,500 bit-identical rows in the 2305-row list, probed by exactly 64 queries aimed at them (two passes of ST_Q = 32 queries per
    unit): every pass over a unit finds 32 x (copies in the unit) keys at or above the thresholds, far more than the ST_CBUF = 1024
    a workgroup buffers, so the rest goes straight to the lists.  The lists still equal the reference sets, nothing falls back."""
    E = _E()
    b = _build(ctx, 256, LENS, seed=91)
    rng = np.random.default_rng(92)
    crowd = rng.permutation(np.flatnonzero(b.assign == 6))[:1500]
    v = (b.centroids[6] + 0.3 / 16 * rng.standard_normal(256)).astype(np.float32)
    b.idx.update(crowd, np.repeat(v[None, :], 1500, 0))
    b.x[crowd] = v
    _, assign = b.idx.ivf_export(b.nlist)
    assert np.array_equal(assign, b.assign)
    q, targets = _queries(b.centroids, [(64, (6, 3, 4, 5, 9)), (41, (0, 1, 2, 7, 9))], seed=93)
    q[:64] = (v[None, :] + 0.3 * b.centroids[[3, 4, 5, 9]].sum(0)[None, :] + 0.01 / 16 * rng.standard_normal((64, 256))).astype(np.float32)
    st, probes = _search_and_check(b, q, targets, 10, 5, E.IVF_KERNEL_I8_STREAM, E.IVF_GRID_COLLECT)
    assert np.array_equal(np.flatnonzero((probes == 6).any(axis=1)), np.arange(64))
    # copies in the first four non-sample tiles of the list (inside its first unit of the collect pass), times the 32 queries
    # of a pass: all at or above their query's threshold (asserted: the copies are in the query's list)
    order, offsets = _read_structure(b.idx, st)
    in_unit = np.isin(order[offsets[6] + 256: offsets[6] + 1280], crowd).sum()
    assert 32 * in_unit > 1024, in_unit
    cnt = b.idx.ivf_state_read(E.IVF_COUNTS, np.int32, 2 * st["B"])
    lists = b.idx.ivf_state_read(E.IVF_KEY_LISTS, np.uint64, st["B"] * st["list_cap"]).reshape(st["B"], -1)
    for i in range(64):
        rows = 0xFFFFFFFF - (lists[i, :cnt[i]] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert np.isin(crowd, rows).all()


# ---------------------------------------------------------------- state rules
def test_state_rules(ctx):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    from semantic_query_engine_amd._native import SqeError
    E = _E()
    flat = VectorIndex(ctx, 64)
    with pytest.raises(SqeError, match="IVF indexes only"):
        flat.ivf_state()
    idx = VectorIndex(ctx, 64, INDEX_IVF_FLAT, 4)
    with pytest.raises(SqeError, match="no IVF search yet"):
        idx.ivf_state()
    with pytest.raises(SqeError, match="no IVF search yet"):
        idx.ivf_state_read(E.IVF_PROBES, np.int64, 1)
    b = _case(ctx, 64)
    q, _ = _queries(b.centroids, [(2, (7,))], seed=5)
    b.idx.search(q, 3, nprobe=1)
    st = b.idx.ivf_state()
    assert st["B"] == 2 and st["kp"] == 32 and st["list_kernel"] == E.IVF_KERNEL_BF16_MFMA
    with pytest.raises(SqeError, match="range outside"):
        b.idx.ivf_state_read(E.IVF_PROBES, np.int64, 3)
    with pytest.raises(SqeError, match="did not use"):
        b.idx.ivf_state_read(E.IVF_I8_ROWS, np.int8, 1)                      # a bf16 search has no int8 copy
    with pytest.raises(SqeError, match="did not use"):
        b.idx.ivf_state_read(E.IVF_THRESHOLDS, np.float32, 1)
    with pytest.raises(SqeError, match="unknown buffer"):
        b.idx.ivf_state_read(99, np.int8, 1)
    cosr = b.idx.ivf_state_read(E.IVF_PROBES_COS, np.float32, 2)
    qn = b.idx.ivf_state_read(E.IVF_QN, np.float32, 2 * 64).reshape(2, 64)
    assert np.allclose(qn, R.normalize_rows(q), atol=1e-6)
    assert np.allclose(cosr, (qn.astype(np.float64) @ b.centroids[7].astype(np.float64)), atol=2e-6)


# ---------------------------------------------------------------- k-means
KM_N, KM_D, KM_NLIST = 4000, 64, 16
KM_DATA_SEED, KM_TRAIN_SEED = 3, 11          # chosen on the CPU: the reference alone excludes no row (cap: 0.5 %)
GAP = 2e-6                                   # cosines closer than this the fp32 assignment cannot tell apart (tests/test_ivf_gpu.py)


def _km_data():
    rng = np.random.default_rng(KM_DATA_SEED)
    cen = rng.standard_normal((KM_NLIST, KM_D)).astype(np.float32)
    return (cen[rng.integers(0, KM_NLIST, KM_N)] + 0.3 * rng.standard_normal((KM_N, KM_D))).astype(np.float32)


def km_reference(x, iters, seed):
    """-> (iterations of oracle.ivf.kmeans_reference, tolerance [nlist, dim], excluded rows, excluded lists, final assignment).

    Tolerance, per component j of the centroid of a list of m rows, with u = 2^-24:
      the device's normalised sample differs from the float64 one by d_in = (dim / 2 + 3) u relative per element (a dim-term sum of
      squares, a square root, the + 1e-9 and the division);
      the fp32 atomic sum of m terms in any order is within gamma_m sum |x_ij| of the exact sum, gamma_m = m u / (1 - m u):
          e_j = (gamma_m + d_in (1 + gamma_m)) A_j,   A_j = sum_i |x_ij|;
      c = S / ||S|| moves by at most e_j / ||S|| + |c_j| ||e|| / ||S|| to first order, divided by (1 - ||e|| / ||S||) for the rest;
      the normalisation itself, and the one the coarse index applies to the centroid it stores and the one before it that an
      unchanged sum would see, are three evaluations of d_in |c_j|.
    Summed over the iterations (an earlier centroid error can move a later sum only through an assignment, and rows whose two
    best centroids are within GAP are excluded with their lists)."""
    u = 2.0 ** -24
    x64 = x.astype(np.float64)
    xn64 = x64 / (np.sqrt((x64 * x64).sum(1, keepdims=True)) + 1e-9)
    picks = IV.train_picks(x.shape[0], KM_NLIST, seed)
    its = IV.kmeans_reference(xn64, picks, iters)
    d_in = (KM_D / 2 + 3) * u
    tol = np.zeros((KM_NLIST, KM_D))
    bad_rows = np.zeros(x.shape[0], bool)
    bad_lists = np.zeros(KM_NLIST, bool)
    for it in its:
        amb = it["gap"] < GAP
        # a row next to a list that is already in doubt is in doubt too
        amb |= bad_lists[it["assign"]] | (bad_lists[it["second"]] & (it["gap"] < 1e-2))
        bad_rows |= amb
        bad_lists[it["assign"][amb]] = True
        bad_lists[it["second"][amb]] = True
        m = it["counts"].astype(np.float64)[:, None]
        gamma = m * u / (1 - m * u)
        e = (gamma + d_in * (1 + gamma)) * it["abs_sums"]
        sn = np.sqrt((it["sums"] ** 2).sum(1, keepdims=True))
        en = np.sqrt((e ** 2).sum(1, keepdims=True))
        live = it["counts"] > 0
        c = np.abs(it["centroids"])
        step = np.zeros_like(tol)
        step[live] = ((e[live] / sn[live] + c[live] * en[live] / sn[live]) / (1 - en[live] / sn[live]))
        tol += step + 3 * d_in * c
    best, second, gap = IV.assign_best(xn64, its[-1]["centroids"])
    final_amb = (gap < GAP) | bad_lists[best] | (bad_lists[second] & (gap < 1e-2))
    return its, tol, bad_rows | final_amb, bad_lists, best


@pytest.mark.parametrize("iters", [1, 4])
def test_kmeans_against_float64_lloyd(ctx, iters):
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    x = _km_data()
    its, tol, bad_rows, bad_lists, best = km_reference(x, iters, KM_TRAIN_SEED)
    assert bad_rows.mean() <= 0.005, bad_rows.sum()
    idx = VectorIndex(ctx, KM_D, INDEX_IVF_FLAT, KM_NLIST)
    idx.train(x, iters=iters, seed=KM_TRAIN_SEED)
    idx.add(x)
    centroids, assign = idx.ivf_export(KM_NLIST)
    ok = ~bad_rows
    assert np.array_equal(assign[ok], best[ok])
    ref = its[-1]["centroids"]
    dev = np.abs(centroids.astype(np.float64) - ref)
    good = ~bad_lists
    assert good.sum() >= KM_NLIST - 2
    ratio = (dev[good] / tol[good]).max()
    print(f"k-means iters {iters}: largest centroid deviation {dev[good].max():.3e}, derived tolerance there "
          f"{tol[good].reshape(-1)[np.argmax((dev[good] / tol[good]).reshape(-1))]:.3e} (ratio {ratio:.4f}), smallest tolerance {tol[good].min():.3e}, "
          f"rows excluded by the tie rule {bad_rows.sum()} of {x.shape[0]} ({100 * bad_rows.mean():.3f} %), lists excluded {bad_lists.sum()}")
    assert np.all(dev[good] <= tol[good]), (np.argwhere(dev > tol)[:8].tolist(), float(ratio))
    assert np.allclose(np.linalg.norm(centroids.astype(np.float64), axis=1), 1.0, atol=(KM_D / 2 + 3) * 2.0 ** -23)
    # the tolerance can see one row: leaving the first row out of its list moves that centroid by more than the tolerance
    c0 = its[-1]["assign"][0]
    rows = np.flatnonzero(its[-1]["assign"] == c0)[1:]
    x64 = x.astype(np.float64)
    xn64 = x64 / (np.sqrt((x64 * x64).sum(1, keepdims=True)) + 1e-9)
    s = xn64[rows].sum(0)
    assert np.any(np.abs(s / np.linalg.norm(s) - ref[c0]) > tol[c0])


def test_kmeans_duplicate_picks_leave_empty_lists_their_centroid(ctx):
    """Training rows = nlist rows of which half are copies of the other half: every row is a pick, each pair's copies all go to the
    pair's lower list id (ties to the lowest id), the higher one ends empty and must keep its centroid -- the normalised row."""
    from semantic_query_engine_amd import INDEX_IVF_FLAT, VectorIndex
    nlist, dim, seed = 16, 64, 21
    rng = np.random.default_rng(seed)
    half = rng.standard_normal((nlist // 2, dim)).astype(np.float32) * 3.0
    x = np.concatenate([half, half])
    picks = IV.train_picks(nlist, nlist, seed)
    its = IV.kmeans_reference(R.normalize_rows(x), picks, 1)
    pair = picks % (nlist // 2)                                  # list i starts from row picks[i], a copy of half[pair[i]]
    low = np.array([np.flatnonzero(pair == p).min() for p in range(nlist // 2)])
    high = np.array([np.flatnonzero(pair == p).max() for p in range(nlist // 2)])
    assert np.all(its[0]["counts"][low] == 2) and np.all(its[0]["counts"][high] == 0)      # the reference: empty lists exist
    idx = VectorIndex(ctx, dim, INDEX_IVF_FLAT, nlist)
    idx.train(x, iters=1, seed=seed)
    idx.add(x)
    centroids, assign = idx.ivf_export(nlist)
    x64 = x.astype(np.float64)
    want = (x64 / (np.sqrt((x64 * x64).sum(1, keepdims=True)) + 1e-9))[picks]
    tol = 3 * (dim / 2 + 3) * 2.0 ** -24 * np.abs(want) + 2.0 ** -149      # three fp32 normalisations of a unit vector (km_reference)
    assert np.all(np.abs(centroids - want) <= tol), np.abs(centroids - want).max()
    assert np.allclose(np.linalg.norm(centroids.astype(np.float64), axis=1), 1.0, atol=1e-6)       # an emptied list is not zeroed
    # every stored row sits in a list of its pair; in the lower one wherever the two stored centroids are the same bits (their
    # fp32 scores are then equal and ties go to the lowest id)
    assert np.array_equal(pair[assign], np.arange(nlist) % (nlist // 2))
    same = np.array([np.array_equal(centroids[low[p]], centroids[high[p]]) for p in range(nlist // 2)])
    print(f"duplicate picks: {same.sum()} of {nlist // 2} pairs store bit-identical centroids")
    for r in range(nlist):
        p = r % (nlist // 2)
        if same[p]:
            assert assign[r] == low[p]
