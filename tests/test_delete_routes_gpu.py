"""Every block route of the delete's in-place compaction (csrc/compact.hip), and every byte it moved.

Each case reads the whole index back (ids, master rows, the bf16 copy over its whole padded extent, keys, field columns,
IVF assignments), deletes, asserts that sqe_index_delete_last reports exactly the blocks tests/delete_reference.py plans for
those positions -- so the route a case is there for is asserted, not assumed -- reads everything back again and hands both
to delete_reference.check_delete: ids, rows, bf16 rows and their zeroed tail, keys, fields and lists bit for bit against the
state before; the search after the delete bit for bit against a fresh index built from the same raw rows; and, where the
int8 first pass runs, the int8 copy that search re-quantised against the fresh index's, whole tiles.

The cases and their deleted positions are delete_reference.CASES (the CPU tests replay their plans and seed the faults the
checker must catch).  Each prints one line of figures: the route as the library reported it, and wall times.  GPU only."""
import json
import time

import numpy as np
import pytest

from tests import delete_reference as D

pytestmark = pytest.mark.gpu

K, B = 10, 32


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _queries(rng, x):
    q = rng.standard_normal((B, x.shape[1])).astype(np.float32)
    near = rng.integers(0, x.shape[0], B // 2)
    q[:B // 2] = x[near] + 0.05 * q[:B // 2]
    return q


def _new_index(ctx, dim, i8=False, nlist=0):
    from semantic_query_engine_amd import INDEX_FLAT, INDEX_IVF_FLAT, SCAN_INT8_RESCORE, VectorIndex
    idx = VectorIndex(ctx, dim, INDEX_IVF_FLAT if nlist else INDEX_FLAT, nlist)
    if i8:
        idx.set_option("scan_mode", SCAN_INT8_RESCORE)
        idx.set_option("i8_min_rows", 0)
        idx.set_option("i8_sample_step", 1)                 # the int8 pass then answers from 1024 rows on
    return idx


def _read_back(idx, keys=False, fields=(), nlist=0):
    ids = idx.ids()
    s = {"ids": ids, "len": len(idx), "next_id": idx.next_id, "rows": idx.get_rows(ids)}
    if not nlist:
        from semantic_query_engine_amd import engine as E
        st = idx.state()                                    # positions 0 .. round_up(n, 256) - 1 at the whole pitch, the pad included
        rows, cols = D.round_up(st["rows"], 256), st["scan_pitch"] // 2
        s["bf16"] = idx.state_read(E.STATE_SCAN_BF16, np.uint16, rows * cols).reshape(rows, cols)
    if keys:
        s["keys"] = idx.get_keys(ids)
    if fields:
        s["fields"] = {slot: idx.get_field(slot, ids) for slot in fields}
    if nlist:
        s["assign"] = idx.ivf_export(nlist)[1]
    return s


def _read_i8(idx, n, into):
    """the int8 copy as the last search left it: whole tiles, the rows of the last tile past n included"""
    from semantic_query_engine_amd import engine as E
    st = idx.state()
    assert st["i8_rows"] == n and st["last_i8"] == 1, st
    tiles, stride, payload = (n + 255) // 256, st["i8_tile_stride"], st["dim"] // 64 * 256 * 64
    into["i8_rows"] = idx.i8_read(E.I8_ROWS, np.int8, tiles * stride).reshape(tiles, stride)[:, :payload]
    into["i8_scales"] = idx.i8_read(E.I8_ROW_SCALES, np.uint32, tiles * 256)
    into["i8_last_rows"] = idx.i8_last()["rows"]


def _searched(idx, q, n, i8, nprobe=0):
    out = {"search": idx.search(q, K, nprobe=nprobe)}
    if i8 and n >= 1024:
        _read_i8(idx, n, out)
    return out


def _delete_and_check(ctx, idx, raw, q, pos, i8=False, keys=False, fields=(), nlist=0, train=None):
    """delete the row POSITIONS pos of idx (whose rows were added as `raw`, in position order); -> figures"""
    dim, n_old = raw.shape[1], raw.shape[0]
    before = _read_back(idx, keys, fields, nlist)
    assert before["len"] == n_old
    t0 = time.perf_counter()
    idx.delete(before["ids"][pos])
    t_delete = time.perf_counter() - t0
    last = idx.delete_last()
    w = D.block_rows(dim, keys)
    assert last == D.expected_last(D.plan(n_old, pos, w), n_old, pos, dim, keys), last
    after = _read_back(idx, keys, fields, nlist)
    live = np.setdiff1d(np.arange(n_old), pos)
    fresh_idx = _new_index(ctx, dim, i8, nlist)
    fresh_idx.add(raw[live])
    if nlist:
        fresh_idx.train(train, iters=4, seed=1)
    after.update(_searched(idx, q, live.size, i8, nprobe=nlist))
    fresh = _searched(fresh_idx, q, live.size, i8, nprobe=nlist)
    cos_equal = bool(np.array_equal(after["search"][0].view(np.uint32), fresh["search"][0].view(np.uint32)))
    if nlist:                                               # IVF: the ids of a search over all lists; the cosines are only reported
        fresh["search"] = (after["search"][0], fresh["search"][1])
    fresh_idx.close()
    D.check_delete(before, after, pos, fresh)
    return dict(last, delete_s=round(t_delete, 4), cosines_bit_equal=cos_equal, int8_checked="i8_rows" in fresh)


def _report(name, figures, t0):
    print("\ndelete_routes " + json.dumps(dict(figures, case=name, wall_s=round(time.perf_counter() - t0, 2))))


@pytest.mark.parametrize("name", list(D.CASES))
def test_case(ctx, name):
    t0 = time.perf_counter()
    c = D.CASES[name]
    dim, has_keys, w, n_old, pos = D.case_delete(name)
    i8, fields, nlist = bool(c.get("i8")), tuple(c.get("fields", ())), int(c.get("nlist", 0))
    rng = np.random.default_rng(sum(name.encode()))
    x = rng.standard_normal((n_old, dim), dtype=np.float32)
    q = _queries(rng, x[np.setdiff1d(np.arange(n_old), pos)[:4096]])
    idx = _new_index(ctx, dim, i8, nlist)
    train = None
    if nlist:                                               # trained on all but the last 500 rows, which are added afterwards
        train = x[:n_old - 500]
        idx.add(train)
        idx.train(train, iters=4, seed=1)
        idx.add(x[n_old - 500:])
    else:
        idx.add(x)
    ids = np.arange(n_old)
    if has_keys:
        from semantic_query_engine_amd import KEY_NONE
        keys = rng.integers(0, 1 << 40, n_old)
        keys[rng.choice(n_old, n_old // 10, replace=False)] = KEY_NONE
        idx.set_keys(ids, keys)
    for slot in fields:
        some = np.sort(rng.choice(n_old, n_old * 3 // 4, replace=False))      # a quarter of the rows holds no value
        idx.set_field(slot, some, rng.integers(-(1 << 40), 1 << 40, some.size))
    if i8:
        idx.search(q[:4], K)                                # the int8 copy exists before the delete
        assert idx.state()["i8_rows"] == n_old
    figures = _delete_and_check(ctx, idx, x, q, pos, i8, has_keys, fields, nlist, train)
    assert figures["int8_checked"] == i8
    idx.close()
    _report(name, figures, t0)


def test_case_h_second_delete_after_add_and_update(ctx):
    """B2's delete, an add that outgrows the allocation, an update, then a second delete on the index that has a map by now;
    the int8 copy is compared with a fresh index's after every step"""
    t0 = time.perf_counter()
    dim, w = 8192, D.block_rows(8192, False)
    rng = np.random.default_rng(8)
    raw = rng.standard_normal((D.H_ROWS, dim), dtype=np.float32)
    q = _queries(rng, raw[w:])
    idx = _new_index(ctx, dim, True)
    idx.add(raw)
    idx.search(q[:4], K)

    def same_as_fresh(raw_now):
        fresh_idx = _new_index(ctx, dim, True)
        fresh_idx.add(raw_now)
        got, want = _searched(idx, q, raw_now.shape[0], True), _searched(fresh_idx, q, raw_now.shape[0], True)
        fresh_idx.close()
        ids = idx.ids()
        assert np.array_equal(got["search"][1], np.where(want["search"][1] >= 0, ids[np.maximum(want["search"][1], 0)], -1))
        assert np.array_equal(got["search"][0].view(np.uint32), want["search"][0].view(np.uint32))
        assert got["i8_last_rows"] == raw_now.shape[0]
        assert np.array_equal(got["i8_scales"], want["i8_scales"]) and np.array_equal(got["i8_rows"], want["i8_rows"])

    first = _delete_and_check(ctx, idx, raw, q, np.arange(w), i8=True)
    assert first["direct_blocks"] == 3 and first["staged_blocks"] == 1
    raw = raw[w:]
    more = rng.standard_normal((D.H_ADDED, dim), dtype=np.float32)
    idx.add(more)                                           # 9271 rows in an allocation made for 9000
    raw = np.concatenate([raw, more])
    live_ids = np.concatenate([np.arange(w, D.H_ROWS), np.arange(D.H_ROWS, D.H_ROWS + D.H_ADDED)])      # new rows: ids from next_id on
    assert np.array_equal(idx.ids(), live_ids) and idx.next_id == D.H_ROWS + D.H_ADDED
    same_as_fresh(raw)
    upd = np.sort(rng.choice(raw.shape[0], D.H_UPDATED, replace=False))
    new = rng.standard_normal((D.H_UPDATED, dim), dtype=np.float32)
    idx.update(live_ids[upd], new)
    raw[upd] = new
    same_as_fresh(raw)
    pos = D.case_h_second(w, raw.shape[0])
    second = _delete_and_check(ctx, idx, raw, q, pos, i8=True)
    assert second["staged_blocks"] == 1 and second["direct_blocks"] >= 2 and second["first_pos"] == 100
    assert np.array_equal(idx.ids(), np.delete(live_ids, pos)) and idx.next_id == D.H_ROWS + D.H_ADDED
    idx.close()
    _report("H/1", first, t0)
    _report("H/2", second, t0)


def test_delete_last_states(ctx):
    from semantic_query_engine_amd import EXCHANGE_COPY, Context, VectorIndex
    from semantic_query_engine_amd._native import SqeError
    x = np.random.default_rng(0).standard_normal((600, 64)).astype(np.float32)
    idx = VectorIndex(ctx, 64)
    idx.add(x)
    with pytest.raises(SqeError) as e:
        idx.delete_last()
    assert e.value.code == -4                               # SQE_ERR_STATE: nothing was deleted yet
    idx.delete([7, 300])
    assert idx.delete_last() == {"n_old": 600, "n_new": 598, "first_pos": 7, "block_rows": D.block_rows(64, False), "staged_blocks": 1,
                                 "direct_blocks": 0, "staged_rows": 593, "direct_rows": 0, "stage_bytes": 593 * D.stage_pitch(64, False)}
    idx.delete([599])                                       # the last row alone: one block of one row
    assert idx.delete_last()["staged_rows"] == 1 and idx.delete_last()["first_pos"] == 597
    grp = VectorIndex(Context(devices=[0, 0], exchange=EXCHANGE_COPY), 64)
    grp.add(x)
    grp.delete([5])
    with pytest.raises(SqeError) as e:
        grp.delete_last()
    assert e.value.code == -5                               # SQE_ERR_UNSUPPORTED on a device group
