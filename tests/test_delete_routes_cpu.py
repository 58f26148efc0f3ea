"""The delete's block rule and the checker of tests/test_delete_routes_gpu.py, without a GPU (tests/delete_reference.py).

The plan of every delete the GPU tests run is replayed on row tags in three orders of the rows within a launch, the routes the
GPU cases are there for are asserted on the plans, and seeded faults -- two in the plan, three in a NumPy stand-in of an index
-- must each fail the property they belong to."""
import numpy as np
import pytest

from tests import delete_reference as D

DELETES = {d[0]: d[1:] for d in D.all_deletes()}


def test_block_rows_table():
    """the w of the dims the block rule is documented with"""
    assert [D.block_rows(d, False) for d in (64, 256, 1024, 8192)] == [335544, 86480, 21788, 2729]
    assert D.block_rows(2048, True) == (128 << 20) // 12320 and D.block_rows(2048, False) == (128 << 20) // 12304
    assert D.block_rows(1 << 20, False) == 256


@pytest.mark.parametrize("label", sorted(DELETES))
@pytest.mark.parametrize("order", D.ORDERS)
def test_every_gpu_plan_replays(label, order):
    dim, has_keys, w, n_old, pos = DELETES[label]
    blocks = D.plan(n_old, pos, w)
    assert blocks[0][0] == pos[0] and blocks[-1][1] == n_old
    assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
    mem, read = D.replay(blocks, pos, n_old, order, w=w)
    live = np.setdiff1d(np.arange(n_old), pos)
    assert np.array_equal(mem[:live.size], live)
    assert read[live[live > pos[0]]].all() and not read[:pos[0]].any() and not read[pos].any()


def _modes(label):
    dim, has_keys, w, n_old, pos = DELETES[label]
    blocks = D.plan(n_old, pos, w)
    return w, n_old, pos, blocks, [m for _, _, m in blocks], [b1 - b0 for b0, b1, _ in blocks]


def test_the_cases_take_the_routes_they_are_there_for():
    S, X = D.STAGED, D.DIRECT
    w, n, pos, blocks, modes, lens = _modes("A")
    assert modes == [S, S, S] and 40 <= pos[0] <= 60
    w, n, pos, blocks, modes, lens = _modes("B1")
    assert modes == [S, S, S, S] and pos.size == w - 1                      # one deleted row short of the switch
    w, n, pos, blocks, modes, lens = _modes("B2")
    assert modes == [S, X, X, X] and lens == [w, w, w, n - 3 * w] and 0 < lens[-1] < w      # the switch at exactly w; ragged end
    live = np.setdiff1d(np.arange(n), pos)
    for b0, b1, m in blocks[1:3]:
        assert np.searchsorted(live, b1 - 1) == b0 - 1                       # tight: dest(b1 - 1) = b0 - 1
    w, n, pos, blocks, modes, lens = _modes("C")
    assert modes == [S, S, X, X] and lens[2] < lens[3] and np.isin(pos, np.arange(blocks[2][0], n)).any()
    for label in ("D0", "D1"):
        w, n, pos, blocks, modes, lens = _modes(label)
        assert modes == [S, S, X, X] and lens[2] != lens[3] and pos[-1] == n - 1
        assert (n - pos.size) % 256 == (0 if label == "D0" else 1)
    for label in ("E64", "E192", "E2112", "F", "G", "H/1", "H/2"):
        w, n, pos, blocks, modes, lens = _modes(label)
        assert modes[0] == S and modes.count(X) >= 2 and set(modes[1:]) == {X}, (label, modes)
    assert _modes("H/2")[2][-1] == _modes("H/2")[1] - 1 and _modes("H/2")[2][0] == 100


def test_expected_last_counts_blocks_and_rows():
    dim, has_keys, w, n_old, pos = DELETES["C"]
    L = D.expected_last(D.plan(n_old, pos, w), n_old, pos, dim, has_keys)
    assert L == {"n_old": 12000, "n_new": 6000, "first_pos": 0, "block_rows": 2729, "staged_blocks": 2, "direct_blocks": 2,
                 "staged_rows": 5458, "direct_rows": 12000 - 5458, "stage_bytes": 2729 * 49168}
    dim, has_keys, w, n_old, pos = DELETES["A"]
    L = D.expected_last(D.plan(n_old, pos, w), n_old, pos, dim, has_keys)
    assert L["direct_blocks"] == 0 and L["staged_rows"] == 7000 - 50 and L["stage_bytes"] == 2729 * 49168


# ---------------------------------------------------------------------------------------------------------------- seeded faults
def test_fault_direct_block_one_row_too_long():
    """b1 = b0 + shift + 1: on B2 the last row of the block lands on the block's own first row"""
    dim, has_keys, w, n_old, pos = DELETES["B2"]
    blocks = D.plan(n_old, pos, w)
    b0, b1, mode = blocks[1]
    assert mode == D.DIRECT and b1 - b0 == w
    bad = blocks[:1] + [(b0, b1 + 1, mode), (b1 + 1, blocks[2][1], D.DIRECT)] + blocks[3:]
    with pytest.raises(D.ReplayError, match=f"row {b1} is written onto the live row {b0} that has not been read"):
        D.replay(bad, pos, n_old, "descending", w=w)
    failed = 0
    for seed in range(8):                                                    # a shuffle reads row b0 first half of the time
        try:
            D.replay(bad, pos, n_old, "shuffled", w=w, seed=seed)
        except D.ReplayError:
            failed += 1
    assert failed >= 1
    D.replay(bad, pos, n_old, "ascending", w=w)                              # the order that hides it: why replay runs three


def test_fault_staged_block_moved_in_place():
    for label in ("A", "B1"):                                                # (C's rows halve their position: in place would be safe)
        dim, has_keys, w, n_old, pos = DELETES[label]
        blocks = D.plan(n_old, pos, w)
        at = 1                                                               # a full staged block: longer than the shift below it
        assert blocks[at][2] == D.STAGED and blocks[at][1] - blocks[at][0] == w > np.searchsorted(pos, blocks[at][0])
        bad = list(blocks)
        bad[at] = (blocks[at][0], blocks[at][1], D.DIRECT)
        with pytest.raises(D.ReplayError, match="that has not been read"):
            D.replay(bad, pos, n_old, "descending", w=w)


def test_fault_staged_block_longer_than_the_buffer():
    dim, has_keys, w, n_old, pos = DELETES["A"]
    blocks = D.plan(n_old, pos, w + 1)
    with pytest.raises(D.ReplayError, match="more rows than the staging buffer"):
        D.replay(blocks, pos, n_old, "ascending", w=w)


def test_fault_a_block_skipped():
    dim, has_keys, w, n_old, pos = DELETES["C"]
    blocks = D.plan(n_old, pos, w)
    with pytest.raises(D.ReplayError, match="not tags\\[live\\]"):
        D.replay(blocks[:-1], pos, n_old, "ascending", w=w)


def _stand_in(n=3000, dim=64, seed=5):
    """read-backs of a NumPy index before and after a correct delete, with keys, two fields and IVF lists"""
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.choice(n, 700, replace=False))
    live = np.setdiff1d(np.arange(n), pos)
    ids = np.sort(rng.choice(2 * n, n, replace=False)).astype(np.int64)
    bf = np.zeros((D.round_up(n, 256), dim + 64), np.uint16)                 # 64 pad columns per row, zero as the library keeps them
    bf[:n, :dim] = rng.integers(1, 1 << 16, (n, dim))
    before = {"ids": ids, "len": n, "next_id": 2 * n, "rows": rng.standard_normal((n, dim)).astype(np.float32), "bf16": bf,
              "keys": rng.integers(0, 50, n), "fields": {0: rng.integers(0, 9, n), 3: rng.integers(-5, 5, n)},
              "assign": rng.integers(0, 16, n).astype(np.int32)}
    abf = np.zeros((D.round_up(live.size, 256), dim + 64), np.uint16)
    abf[:live.size] = bf[live]
    after = {"ids": ids[live], "len": live.size, "next_id": 2 * n, "rows": before["rows"][live], "bf16": abf,
             "keys": before["keys"][live], "fields": {s: c[live] for s, c in before["fields"].items()},
             "assign": before["assign"][live]}
    return before, after, pos, live


def test_checker_accepts_a_correct_delete():
    before, after, pos, live = _stand_in()
    D.check_delete(before, after, pos)
    q = np.arange(12, dtype=np.float32).reshape(3, 4)
    fresh = {"search": (q, np.arange(12).reshape(3, 4))}
    after["search"] = (q.copy(), after["ids"][np.arange(12).reshape(3, 4)])
    D.check_delete(before, after, pos, fresh)


def test_fault_id_written_at_source_position():
    """map[i] = id instead of map[dest(i)] = id"""
    before, after, pos, live = _stand_in()
    m = before["ids"].copy()
    m[live] = before["ids"][live]                                            # every id stays where it was
    after["ids"] = m[:live.size]
    with pytest.raises(AssertionError, match=r"property 1 \(ids\)"):
        D.check_delete(before, after, pos)


@pytest.mark.parametrize("what, name", [("keys", r"property 4 \(keys\)"), ("assign", r"property 4 \(IVF lists\)"),
                                        ("field", r"property 4 \(field 3\)")])
def test_fault_column_left_behind(what, name):
    before, after, pos, live = _stand_in()
    if what == "field":
        after["fields"][3] = before["fields"][3][:live.size]
    else:
        after[what] = before[what][:live.size]
    with pytest.raises(AssertionError, match=name):
        D.check_delete(before, after, pos)


def test_fault_tail_not_zeroed():
    before, after, pos, live = _stand_in()
    n_new, pad = live.size, D.round_up(live.size, 256)
    after["bf16"][n_new:pad] = before["bf16"][n_new:pad]                     # the rows the compaction left where they were
    with pytest.raises(AssertionError, match=r"property 3 \(bf16 tail\): row %d " % n_new):
        D.check_delete(before, after, pos)


@pytest.mark.parametrize("where", ["live", "tail"])
def test_fault_copy_runs_past_the_payload(where):
    """one 16-byte vector too many per row: it lands in the pad behind the payload, which nothing else ever writes"""
    before, after, pos, live = _stand_in()
    dim, n_new = before["rows"].shape[1], live.size
    row = 777 if where == "live" else n_new + 2                              # a moved row / a row of the zeroed tail
    after["bf16"][row, dim:dim + 8] = 0x3F80
    with pytest.raises(AssertionError, match=r"property 3 \(bf16 pad\): the pad columns of row %d " % row):
        D.check_delete(before, after, pos)
    before, after, pos, live = _stand_in()
    before["bf16"][5, dim + 3] = 1                                           # a pad that was dirty before is a finding of its own
    with pytest.raises(AssertionError, match=r"property 3 \(bf16 pad\): the pad columns were not zero before"):
        D.check_delete(before, after, pos)


def test_fault_one_row_overwritten_and_search_and_int8():
    before, after, pos, live = _stand_in()
    rows = after["rows"].copy()
    rows[1234] = rows[1235]
    with pytest.raises(AssertionError, match=r"property 2 \(master rows\)"):
        D.check_delete(before, dict(after, rows=rows), pos)
    bf = after["bf16"].copy()
    bf[17, 5] ^= 1
    with pytest.raises(AssertionError, match=r"property 3 \(bf16 copy\)"):
        D.check_delete(before, dict(after, bf16=bf), pos)
    cos = np.linspace(1, 0, 8, dtype=np.float32).reshape(2, 4)
    p = np.arange(8).reshape(2, 4)
    fresh = {"search": (cos, p), "i8_rows": np.ones((4, 8), np.int8), "i8_scales": np.ones(4, np.uint32)}
    good = dict(after, search=(cos.copy(), after["ids"][p]), i8_rows=np.ones((4, 8), np.int8), i8_scales=np.ones(4, np.uint32),
                i8_last_rows=live.size)
    D.check_delete(before, good, pos, fresh)
    with pytest.raises(AssertionError, match=r"property 5 \(search ids\)"):
        D.check_delete(before, dict(good, search=(cos, p)), pos, fresh)
    with pytest.raises(AssertionError, match=r"property 5 \(search cosines\)"):
        D.check_delete(before, dict(good, search=(np.nextafter(cos, 2, dtype=np.float32), after["ids"][p])), pos, fresh)
    with pytest.raises(AssertionError, match=r"property 6 \(int8 rows\)"):
        D.check_delete(before, dict(good, i8_rows=np.zeros((4, 8), np.int8)), pos, fresh)
    with pytest.raises(AssertionError, match=r"property 6 \(int8 row scales\)"):
        D.check_delete(before, dict(good, i8_scales=np.zeros(4, np.uint32)), pos, fresh)
    with pytest.raises(AssertionError, match=r"property 6 \(int8 rows scanned\)"):
        D.check_delete(before, dict(good, i8_last_rows=live.size + 1), pos, fresh)
