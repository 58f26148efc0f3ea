"""One index through a long life, every query kind after every change (tests/session_cases.py): four sessions on the real
index -- FLAT with the bf16 first pass, FLAT with the int8 first pass across a bitmap block border, IVF (against a FLAT twin, at
nprobe = nlist) and a device group of three logical shards (against a single-device twin).  Every step asserts from the
library's read-backs that the transition it is named after happened; every checkpoint runs every probe against a fresh twin
index and against the NumPy model.  The CPU side of the same checker is tests/test_session_cpu.py.  GPU only."""
import time

import numpy as np
import pytest

from tests import session_cases as SC
from tests.session_fakes import fill_twin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


class IvfDriver:
    """the IVF index behind the driver interface: every call that takes nprobe probes every list"""

    def __init__(self, idx, nlist):
        self.idx, self.nlist = idx, nlist

    def __getattr__(self, name):
        return getattr(self.idx, name)

    def __len__(self):
        return len(self.idx)

    def session_train(self, x):
        self.idx.train(x, iters=4, seed=1)

    def search(self, q, k, filter_ids=None):
        return self.idx.search(q, k, nprobe=self.nlist, filter_ids=filter_ids)

    def search_mmr(self, q, k, **kw):
        return self.idx.search_mmr(q, k, nprobe=self.nlist, **kw)

    def search_fused(self, q, k, **kw):
        return self.idx.search_fused(q, k, nprobe=self.nlist, **kw)


def _flat(ctx, cfg):
    from semantic_query_engine_amd import SCAN_INT8_RESCORE, VectorIndex
    idx = VectorIndex(ctx, cfg.dim)
    if cfg.int8:
        for key, val in (("scan_mode", SCAN_INT8_RESCORE), ("i8_min_rows", 0), ("i8_sample_step", 4), ("i8_sample_m", 64)):
            idx.set_option(key, val)
    return idx


def _session_index(ctx, cfg):
    from semantic_query_engine_amd import EXCHANGE_COPY, INDEX_IVF_FLAT, Context, VectorIndex
    if cfg.kind == "ivf":
        return IvfDriver(VectorIndex(ctx, cfg.dim, INDEX_IVF_FLAT, cfg.nlist), cfg.nlist)
    if cfg.devices > 1:
        return VectorIndex(Context(devices=[0] * cfg.devices, exchange=EXCHANGE_COPY), cfg.dim)
    return _flat(ctx, cfg)


class Transitions:
    """What the read-backs show before and after every step.  `seen` collects one line per step for the notes."""

    def __init__(self, cfg, idx):
        self.cfg, self.idx = cfg, idx
        self.single = cfg.devices == 1
        self.flat = self.single and cfg.kind == "flat"
        self.was = {}
        self.seen = []

    def _snapshot(self):
        idx = self.idx
        s = {"len": len(idx), "next_id": idx.next_id, "ids": idx.ids(), "fields": idx.field_info()}
        if self.flat:
            s["state"] = idx.state()
        if 0 < s["len"] <= 4096:
            s["rows"] = idx.get_rows(s["ids"])
        return s

    def before(self, run, step):
        self.was = self._snapshot()

    def after(self, run, step, info):
        was, now = self.was, self._snapshot()
        note = getattr(self, step)(was, now, info)
        self.seen.append(f"{step}: {note}")

    def _deleted(self, was, now, info):
        gone = info["deleted"]
        assert now["len"] == was["len"] - gone.size and now["next_id"] == was["next_id"]
        assert np.array_equal(now["ids"], np.setdiff1d(was["ids"], gone))
        if not self.single:
            return f"len {was['len']} -> {now['len']}"
        last = self.idx.delete_last()
        first = int(np.searchsorted(was["ids"], gone.min()))
        assert (last["n_old"], last["n_new"], last["first_pos"]) == (was["len"], now["len"], first), last
        if self.flat and was["state"]["i8_rows"]:
            # compact.hip: the int8 copy is kept up to the tile of the first deleted position
            # (or whole again, where the step itself searched after the delete)
            assert now["state"]["i8_rows"] in (min(was["state"]["i8_rows"], first // 256 * 256), now["len"]), (was["state"], now["state"])
        return f"delete_last n_old {last['n_old']} n_new {last['n_new']} first_pos {last['first_pos']}"

    def _added(self, was, now, info):
        assert now["len"] == was["len"] + info["added"] and now["next_id"] == was["next_id"] + info["added"]
        assert np.array_equal(now["ids"][was["len"]:], np.arange(was["next_id"], now["next_id"]))
        if self.flat:
            assert now["state"]["rows"] == now["len"]

    # ---- one method per step
    def add_first(self, was, now, info):
        assert was["len"] == 0 and now["fields"] == {"fields": 0, "device_bytes": 0}
        self._added(was, now, info)
        assert np.array_equal(now["ids"], np.arange(now["len"]))
        return f"len {now['len']}, ids are positions, no field column"

    def late_columns(self, was, now, info):
        assert was["fields"]["fields"] == 0 and now["fields"]["fields"] == 3
        assert now["fields"]["device_bytes"] >= 3 * 8 * now["len"] and now["len"] == was["len"]
        return f"field_info {was['fields']} -> {now['fields']}"

    def first_delete(self, was, now, info):
        assert np.array_equal(was["ids"], np.arange(was["len"]))
        note = self._deleted(was, now, info)
        assert now["ids"][0] != 0 and not np.array_equal(now["ids"], np.arange(now["len"]))
        return note + f"; ids()[0] = {now['ids'][0]}: ids are no longer positions"

    def add_into_tail(self, was, now, info):
        self._added(was, now, info)
        assert now["fields"] == was["fields"]                      # nothing was reallocated
        return f"len {was['len']} -> {now['len']}, field_info unchanged at {now['fields']['device_bytes']} bytes"

    def grow_with_columns(self, was, now, info):
        self._added(was, now, info)
        assert now["fields"]["fields"] == 3 and now["fields"]["device_bytes"] > was["fields"]["device_bytes"]
        assert now["fields"]["device_bytes"] >= 3 * 8 * now["len"] > was["fields"]["device_bytes"]
        return f"len {was['len']} -> {now['len']}, field columns {was['fields']['device_bytes']} -> {now['fields']['device_bytes']} bytes"

    def gather_sizes(self, was, now, info):
        g, d = info["gathered"], info["per_device"]
        assert now["len"] == was["len"] and d["small"] <= SC.GATHER_ROWS < d["large"] <= SC.SUB_FIRST_CAP < d["above"]
        if not self.single:
            return f"gathered {g['large']}, {g['small']}, {g['above']} rows, at most {d['large']}, {d['small']}, {d['above']} on a shard"
        last = self.idx.within_last()                                # the radial search after the collapsed ones, on the small set
        assert (last["kind"], last["route"], last["selected"]) == (SC.RADIAL, SC.ROUTE_GATHER, g["small"]), last
        return (f"gathered {g['large']}, {g['small']}, {g['above']} rows (the sub-index first holds {SC.SUB_FIRST_CAP}), every call "
                "read back by within_last / where_last as the gather route over that many rows")

    def _updated(self, was, now, info):
        ids = info["updated"]
        assert now["len"] == was["len"] and np.array_equal(now["ids"], was["ids"])
        note = f"{ids.size} rows overwritten, id {info['entered']} into a top-k"
        if "rows" in was:
            changed = np.any(was["rows"] != now["rows"], axis=1)
            assert np.array_equal(now["ids"][changed], ids)
            note += ", get_rows changed for exactly them"
        if self.flat and self.cfg.int8:
            # api.hip: the int8 copy is re-quantised in place where it matches the capacity, dropped otherwise
            assert now["state"]["i8_rows"] in (0, was["state"]["i8_rows"]), (was["state"], now["state"])
            note += f", i8_rows {was['state']['i8_rows']} -> {now['state']['i8_rows']}"
        return note

    def update_topk(self, was, now, info):
        return self._updated(was, now, info)

    def update_again(self, was, now, info):
        return self._updated(was, now, info) + f", columns set for {info['columns']} late rows"

    def delete_after_update(self, was, now, info):
        return self._deleted(was, now, info)

    def shrink_word_border(self, was, now, info):
        assert (was["len"] - 1) // 32 > (now["len"] - 1) // 32 and now["len"] % 32
        return self._deleted(was, now, info) + ": across a bitmap word border"

    def shrink_block_border(self, was, now, info):
        assert (was["len"] - 1) // 32768 > (now["len"] - 1) // 32768 and now["len"] % 256
        return self._deleted(was, now, info) + ": across the border of 1,024 bitmap words, into a 256-row tile"

    def delete_all(self, was, now, info):
        note = self._deleted(was, now, info)
        assert now["len"] == 0 and now["ids"].size == 0 and now["fields"]["fields"] == 3
        return note + ": empty"

    def refill(self, was, now, info):
        assert was["len"] == 0
        self._added(was, now, info)
        assert now["ids"][0] == was["next_id"] and now["fields"] == was["fields"]
        return f"len 0 -> {now['len']}, ids from {now['ids'][0]}"

    def delete_then_add(self, was, now, info):
        assert now["len"] == was["len"] - 1 + info["added"] and now["next_id"] == was["next_id"] + info["added"]
        assert not np.isin(info["deleted"], now["ids"]).any() and now["ids"][-1] == now["next_id"] - 1
        return f"id {int(info['deleted'][0])} gone, ids {was['next_id']}..{now['next_id'] - 1} given"


@pytest.mark.parametrize("name", list(SC.SESSIONS))
def test_session(ctx, name):
    cfg = SC.SESSIONS[name]
    driver = _session_index(ctx, cfg)
    idx = driver.idx if isinstance(driver, IvfDriver) else driver
    twins = []

    def make_twin(model):
        while twins:
            twins.pop().close()                               # one twin at a time
        twins.append(fill_twin(_flat(ctx, cfg), model, SC.GATHER_ROWS))
        return twins[-1]

    i8_searches = []

    def after_probe(p):
        """after the plain search of every checkpoint: the pass that answered it saw exactly the live rows"""
        if p.name != "search" or len(idx) == 0:
            return
        if cfg.int8:
            last, st = idx.i8_last(), idx.state()
            assert st["last_i8"] == 1 and (last["rows"], last["B"]) == (len(idx), SC.B), (last, st)
            assert st["i8_rows"] == len(idx), st
            i8_searches.append(last["rows"])
        if cfg.kind == "ivf":
            st = idx.ivf_state()
            assert (st["n_assigned"], st["nprobe"], st["nlist"], st["B"]) == (len(idx), cfg.nlist, cfg.nlist, SC.B), st

    tr = Transitions(cfg, idx)
    run = SC.Run(cfg, driver, make_twin, routes=cfg.devices == 1)
    t0 = time.perf_counter()
    try:
        SC.run_session(run, tr.before, tr.after, after_probe)
    finally:
        wall = time.perf_counter() - t0
        while twins:
            twins.pop().close()
        idx.close()
        if cfg.devices > 1:
            idx.ctx.close()                                   # the group's own context; the module's is the fixture's
    assert [e["step"] for e in run.log] == list(cfg.steps) and len(tr.seen) == len(cfg.steps)
    assert run.near_ties == []
    if cfg.int8:
        assert i8_searches == [e["live"] for e in run.log]
    print(f"\nsession {name}: {len(cfg.steps)} steps, {run.probes_run} probes, largest |cosine - twin| {run.max_twin_diff:.3g} "
          f"(bound {SC.TWIN_TOL}), wall {wall:.2f} s")
    for line in tr.seen:
        print("  " + line)
    for e in run.log:
        print(f"  checkpoint {e['step']}: {e['live']} live, sets {e['sets']}, {e['seconds']:.2f} s")
