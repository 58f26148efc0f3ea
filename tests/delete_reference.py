"""The delete's block walk and its moves, restated in NumPy (no GPU, nothing imported from the library).

sqe_index_delete (csrc/compact.hip) slides the live rows down over the deleted ones in place.  The host walks the rows from
the first deleted position in blocks [b0, b1):

  staged   fewer than w rows are deleted below b0: the block is [b0, min(n, b0 + w)); one launch copies its live rows into a
           staging buffer, a second writes them to their destinations
  direct   at least w rows are deleted below b0 (`shift` of them): the block is [b0, min(n, b0 + shift)); one launch moves the
           rows in place, which is safe only because every destination then lies below b0

with w = max(256, 128 MiB / stage_pitch) and stage_pitch = round_up(6 dim + (keys ? 24 : 12), 16).

block_rows / plan restate that rule, replay carries a plan out on an array of row tags launch by launch and fails where a
write would land on a live row nobody has read yet, expected_last is what sqe_index_delete_last must report, and check_delete
compares two read-backs of an index, before and after a delete, bit for bit.  CASES are the deletes of
tests/test_delete_routes_gpu.py; tests/test_delete_routes_cpu.py replays every one of them and seeds the faults."""
import numpy as np

STAGE_BYTES = 128 << 20
STAGED, DIRECT = "staged", "direct"
ORDERS = ("ascending", "descending", "shuffled")


def round_up(v, m):
    return (v + m - 1) // m * m


def stage_pitch(dim, has_keys):
    return round_up(6 * dim + (24 if has_keys else 12), 16)


def block_rows(dim, has_keys):
    return max(256, STAGE_BYTES // stage_pitch(dim, has_keys))


def _sorted_positions(positions, n_old):
    pos = np.asarray(positions, np.int64).reshape(-1)
    srt = np.sort(pos)
    assert srt.size == 0 or (srt[0] >= 0 and srt[-1] < n_old and np.all(np.diff(srt) > 0)), "positions must be distinct rows of the index"
    return srt


def plan(n_old, positions, w):
    """-> [(b0, b1, STAGED | DIRECT), ...]: the blocks the host loop walks for these deleted positions."""
    pos = _sorted_positions(positions, n_old)
    blocks = []
    if pos.size == 0:
        return blocks
    b0 = int(pos[0])
    while b0 < n_old:
        shift = int(np.searchsorted(pos, b0, side="left"))       # deleted rows below b0
        if shift >= w:
            b1, mode = min(n_old, b0 + shift), DIRECT
        else:
            b1, mode = min(n_old, b0 + w), STAGED
        blocks.append((b0, b1, mode))
        b0 = b1
    return blocks


def expected_last(blocks, n_old, positions, dim, has_keys):
    """What sqe_index_delete_last reports after a delete that walked `blocks`."""
    pos = _sorted_positions(positions, n_old)
    w = block_rows(dim, has_keys)
    staged = [(b0, b1) for b0, b1, mode in blocks if mode == STAGED]
    direct = [(b0, b1) for b0, b1, mode in blocks if mode == DIRECT]
    return {"n_old": n_old, "n_new": n_old - int(pos.size), "first_pos": int(pos[0]), "block_rows": w,
            "staged_blocks": len(staged), "direct_blocks": len(direct),
            "staged_rows": sum(b1 - b0 for b0, b1 in staged), "direct_rows": sum(b1 - b0 for b0, b1 in direct),
            "stage_bytes": min(w, n_old - int(pos[0])) * stage_pitch(dim, has_keys) if staged else 0}


class ReplayError(AssertionError):
    pass


def replay(blocks, positions, n_old, order, w=None, seed=0):
    """Carry the moves of `blocks` out on the row tags 0 .. n_old - 1, launch by launch; -> (memory after, rows that were read).

    A launch handles the live rows of its block one after the other in `order` (ascending, descending, or a seeded shuffle):
    a row is read whole, then written, as one wave of compact_move_kernel does it.  A staged block is two launches (every
    live row into its staging slot, then every slot to its destination), a direct block is one.  ReplayError where a write
    lands on a live row that no launch has read yet, where a staged block has more rows than the staging buffer has slots
    (`w`, when given), or where the first n_new tags are not tags[live] in the end."""
    assert order in ORDERS
    pos = _sorted_positions(positions, n_old)
    live = np.ones(n_old, bool)
    live[pos] = False
    below = np.cumsum(~live) - (~live)                         # deleted rows below each position
    dest = np.arange(n_old, dtype=np.int64) - below
    mem = np.arange(n_old, dtype=np.int64)                     # the tags: mem[p] = the row whose bytes position p holds
    read = np.zeros(n_old, bool)
    rng = np.random.default_rng(seed)
    for b0, b1, mode in blocks:
        rows = np.arange(b0, b1, dtype=np.int64)
        rows = rows[live[b0:b1]]
        if order == "descending":
            rows = rows[::-1]
        elif order == "shuffled":
            rows = rng.permutation(rows)
        if mode == STAGED:
            if w is not None and b1 - b0 > w:
                raise ReplayError(f"replay: the staged block [{b0}, {b1}) has more rows than the staging buffer has slots ({w})")
            stage = mem[rows].copy()                           # launch 1: reads only, into slots of the row's own
            read[rows] = True
            _check_writes(rows, dest, live, read, None, (b0, b1, mode))
            mem[dest[rows]] = stage                            # launch 2: writes only
        else:
            rank = np.full(n_old, -1, np.int64)                # when each row of this launch is read
            rank[rows] = np.arange(rows.size)
            _check_writes(rows, dest, live, read, rank, (b0, b1, mode))
            vals = mem[rows].copy()
            read[rows] = True
            mem[dest[rows]] = vals
    n_new = n_old - pos.size
    want = np.nonzero(live)[0]
    if not np.array_equal(mem[:n_new], want):
        bad = int(np.nonzero(mem[:n_new] != want)[0][0])
        raise ReplayError(f"replay: the result is not tags[live]: position {bad} holds row {int(mem[bad])}, not row {int(want[bad])}")
    return mem, read


def _check_writes(rows, dest, live, read, rank, block):
    """the writes of one launch: unsafe where the destination is a live row that was not read before the launch and is not
    read earlier in it (rank: the read order of a direct launch; None for the write launch of a staged block)"""
    d = dest[rows]
    unread = live[d] & ~read[d]
    if rank is not None:
        unread &= ~((rank[d] >= 0) & (rank[d] < rank[rows]))
    if unread.any():
        j = int(np.nonzero(unread)[0][0])
        raise ReplayError(f"replay: block {block}: row {int(rows[j])} is written onto the live row {int(d[j])} that has not been read")


# ---------------------------------------------------------------------------------------------------------------- checker
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def check_delete(before, after, positions, fresh=None):
    """Two read-backs of an index, `before` and `after` the delete of the row POSITIONS `positions` (of the before state).

    A read-back is a dict: "ids" int64 [n], "len", "next_id", "rows" float32 [n, dim] (get_rows of all ids), and where the
    index has them "bf16" uint16 [round_up(n, 256), pitch / 2] (the whole scanned copy at its whole pitch: dim values, then the pad), "keys" int64 [n], "fields" {slot: int64
    [n]}, "assign" int32 [n].  `after` may also carry "search" = (cos, ids) and, after an int8 search, "i8_rows", "i8_scales",
    "i8_last_rows"; `fresh` then carries the same of an index built from the live raw rows (its ids are positions).  Every
    comparison is bit for bit; each property fails with a message that names it."""
    n_old = int(before["len"])
    pos = _sorted_positions(positions, n_old)
    live = np.setdiff1d(np.arange(n_old, dtype=np.int64), pos)
    n_new = live.size
    # 1: ids, len, next_id
    assert after["len"] == n_new, f"property 1 (len): {after['len']} live rows, expected {n_new}"
    assert after["next_id"] == before["next_id"], f"property 1 (next_id): {after['next_id']}, was {before['next_id']}"
    assert np.array_equal(after["ids"], before["ids"][live]), "property 1 (ids): ids() is not the live ids" + _first_diff(after["ids"], before["ids"][live])
    # 2: master rows
    assert after["rows"].shape == (n_new, before["rows"].shape[1]), "property 2 (master rows): shape"
    assert np.array_equal(_bits(after["rows"]), _bits(before["rows"])[live]), \
        "property 2 (master rows): get_rows(live) changed" + _first_diff(_bits(after["rows"]), _bits(before["rows"])[live])
    # 3: the bf16 copy and its zeroed tail
    if "bf16" in before:
        dim, end = before["rows"].shape[1], round_up(n_new, 256)
        assert after["bf16"].shape == (end, before["bf16"].shape[1]), f"property 3 (bf16 copy): read as {after['bf16'].shape}, expected {end} rows"
        assert not before["bf16"][:, dim:].any(), "property 3 (bf16 pad): the pad columns were not zero before the delete"
        got, was = after["bf16"][:n_new, :dim], before["bf16"][live, :dim]
        assert np.array_equal(got, was), "property 3 (bf16 copy): a live row's bf16 copy changed" + _first_diff(got, was)
        tail = np.nonzero(after["bf16"][n_new:, :dim].any(axis=1))[0]
        assert tail.size == 0, f"property 3 (bf16 tail): row {n_new + int(tail[0]) if tail.size else -1} past the new end is not zero ({tail.size} rows)"
        # the pad between rows is never moved and is zero from the allocation on: a copy that runs past a row's payload lands here
        pads = np.nonzero(after["bf16"][:, dim:].any(axis=1))[0]
        assert pads.size == 0, f"property 3 (bf16 pad): the pad columns of row {int(pads[0]) if pads.size else -1} are not zero ({pads.size} rows)"
    # 4: what moves with the rows
    if "keys" in before:
        assert np.array_equal(after["keys"], before["keys"][live]), "property 4 (keys): a key did not move with its row" + _first_diff(after["keys"], before["keys"][live])
    for slot, col in before.get("fields", {}).items():
        assert np.array_equal(after["fields"][slot], col[live]), \
            f"property 4 (field {slot}): a value did not move with its row" + _first_diff(after["fields"][slot], col[live])
    if "assign" in before:
        assert np.array_equal(after["assign"], before["assign"][live]), \
            "property 4 (IVF lists): an assignment did not move with its row" + _first_diff(after["assign"], before["assign"][live])
    if fresh is None:
        return
    # 5: searches like a fresh index of the live rows
    cos, ids = after["search"]
    fcos, fpos = fresh["search"]
    fids = np.where(fpos >= 0, after["ids"][np.maximum(fpos, 0)], -1)
    assert np.array_equal(ids, fids), "property 5 (search ids): not the fresh index's" + _first_diff(ids, fids)
    assert np.array_equal(_bits(cos), _bits(fcos)), "property 5 (search cosines): not bit-equal to the fresh index's" + _first_diff(_bits(cos), _bits(fcos))
    # 6: the int8 copy the search after the delete re-quantised
    if "i8_rows" in fresh:
        assert after["i8_last_rows"] == n_new, f"property 6 (int8 rows scanned): {after['i8_last_rows']}, expected {n_new}"
        assert np.array_equal(after["i8_scales"], fresh["i8_scales"]), "property 6 (int8 row scales): not the fresh index's" + _first_diff(after["i8_scales"], fresh["i8_scales"])
        assert np.array_equal(after["i8_rows"], fresh["i8_rows"]), "property 6 (int8 rows): not the fresh index's" + _first_diff(after["i8_rows"], fresh["i8_rows"])


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f" (shapes {a.shape} and {b.shape})"
    ne = np.argwhere(a != b)
    if ne.size == 0:
        return ""
    at = tuple(int(v) for v in ne[0])
    return f" ({ne.shape[0]} elements differ, the first at {at}: {a[at]} and {b[at]})"


# ---------------------------------------------------------------------------------------------------------------- the cases
def _scattered(rng, lo, hi, count):
    return lo + rng.choice(hi - lo, count, replace=False)


def case_a(w, rng):
    return np.concatenate([[50], _scattered(rng, 51, 7000, 99)])


def case_c(w, rng):
    return np.arange(0, 12000, 2)


def _case_d(tail_count):
    def positions(w, rng):
        # n_new = 9000 - 3000 - tail_count: 5120 = 20 x 256 with 880 rows of the last third, 5121 with 879
        return np.concatenate([_scattered(rng, 0, 4000, 3000), _scattered(rng, 6000, 8999, tail_count - 1), [8999]])
    return positions


def _case_e(w, rng):
    n = case_rows("E", w)
    return np.concatenate([np.arange(w), _scattered(rng, w, n, n // 100)])


def _case_f(w, rng):
    return np.concatenate([np.arange(w), _scattered(rng, w, 36000, 300)])


# name -> dim, rows before the delete (a number, or a function of w), keys, field slots, IVF lists, int8 property, positions(w, rng)
CASES = {
    "A": dict(dim=8192, n_old=7000, i8=True, positions=case_a),
    "B1": dict(dim=8192, n_old=9000, positions=lambda w, rng: np.arange(w - 1)),
    "B2": dict(dim=8192, n_old=9000, positions=lambda w, rng: np.arange(w)),
    "C": dict(dim=8192, n_old=12000, positions=case_c),
    "D0": dict(dim=8192, n_old=9000, i8=True, positions=_case_d(880)),
    "D1": dict(dim=8192, n_old=9000, i8=True, positions=_case_d(879)),
    "E64": dict(dim=64, n_old="E", positions=_case_e),
    "E192": dict(dim=192, n_old="E", positions=_case_e),
    "E2112": dict(dim=2112, n_old="E", positions=_case_e),
    "F": dict(dim=2048, n_old=36000, keys=True, fields=(0, 3), positions=_case_f),
    "G": dict(dim=2048, n_old=36000, nlist=16, positions=_case_f),
}
H_ROWS, H_ADDED, H_UPDATED = 9000, 3000, 10      # case H (dim 8192, int8): B2's delete, an add, an update, a second delete


def case_rows(n_old, w):
    return w * 12 // 5 if n_old == "E" else n_old                # the E cases: about 2.4 w rows


def case_delete(name):
    """-> (dim, has_keys, w, n_old, positions) of the one delete of a case of CASES; the positions are seeded by the name."""
    c = CASES[name]
    has_keys = bool(c.get("keys"))
    w = block_rows(c["dim"], has_keys)
    n_old = case_rows(c["n_old"], w)
    rng = np.random.default_rng(sum(name.encode()) + 1000)
    return c["dim"], has_keys, w, n_old, np.sort(np.asarray(c["positions"](w, rng), np.int64))


def case_h_second(w, n_rows):
    """positions of case H's second delete on its n_rows rows: w contiguous rows from 100 on and 50 scattered above them, the
    last row (an added one) among them"""
    rng = np.random.default_rng(77)
    return np.sort(np.concatenate([np.arange(100, 100 + w), _scattered(rng, 100 + w, n_rows - 1, 49), [n_rows - 1]]))


def all_deletes():
    """every delete the GPU tests run: (label, dim, has_keys, w, n_old, positions)"""
    for name in CASES:
        yield (name,) + case_delete(name)
    w = block_rows(8192, False)
    yield "H/1", 8192, False, w, H_ROWS, np.arange(w, dtype=np.int64)
    n2 = H_ROWS - w + H_ADDED
    yield "H/2", 8192, False, w, n2, case_h_second(w, n2)
