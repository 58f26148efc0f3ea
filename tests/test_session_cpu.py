"""The session checker of tests/session_cases.py, without a GPU (tests/test_session_gpu.py runs it on the real index):
(a) a faithful NumPy stand-in of the index (tests/session_fakes.py: FakeIndex) passes every checkpoint of all four schedules --
    the checker asks nothing a correct index cannot give;
(b) the near-tie condition holds for the committed seeds, the schedules force the transitions their steps are named after, and
    every checkpoint that can has a row set for the mask route, one for the gather route and an empty one;
(c) eight stand-ins with one seeded stale-state fault each FAIL, each at the step that first exposes it -- the checker is
    tight enough to see the bugs the state behind an index handle invites.  The pattern of tests/test_encoder_stages_cpu.py."""
import copy

import numpy as np
import pytest

from tests import session_cases as SC
from tests.session_fakes import FAULTS, FakeIndex, fake_twin
from tests.session_model import NONE, SessionModel


def _run(name, fault=None, **changed):
    cfg = copy.copy(SC.SESSIONS[name])
    for key, value in changed.items():
        setattr(cfg, key, value)
    run = SC.Run(cfg, FakeIndex(cfg.dim, fault), fake_twin)
    infos = {}
    SC.run_session(run, after=lambda r, step, info: infos.__setitem__(step, dict(info, live=len(r.model))))
    return run, infos


@pytest.fixture(scope="module")
def faithful():
    return {name: _run(name) for name in SC.SESSIONS}


def test_model_mutations():
    m = SessionModel(4)
    x = np.arange(24, dtype=np.float32).reshape(6, 4) + 1
    assert m.add(x).tolist() == [0, 1, 2, 3, 4, 5] and m.next_id == 6
    m.set_keys([1, 2], [7, 8])
    m.set_field(2, [0, 5], [10, 50])
    m.delete([0, 2])
    assert m.live.tolist() == [1, 3, 4, 5] and m.keys().tolist() == [7, NONE, NONE, NONE] and m.field(2).tolist() == [NONE, NONE, NONE, 50]
    assert m.add(x[:1]).tolist() == [6] and m.field(2, [6]).tolist() == [NONE] and m.keys([6]).tolist() == [NONE]
    m.update([6, 1], x[4:6])
    assert np.array_equal(m.raw([1, 6]), x[[5, 4]]) and m.select([(2, "range", 40, None)]).tolist() == [5]
    assert m.select([], [5, 0, 99, 3]).tolist() == [3, 5] and m.by_id().shape == (7, 4) and not m.by_id()[0].any()
    for bad in (lambda: m.delete([0]), lambda: m.update([2], x[:1]), lambda: m.set_keys([9], [1]), lambda: m.delete([1, 1])):
        with pytest.raises(KeyError):
            bad()
    assert len(m) == 5


@pytest.mark.parametrize("name", list(SC.SESSIONS))
def test_faithful_stand_in_passes_every_checkpoint(faithful, name):
    run, _ = faithful[name]
    cfg = SC.SESSIONS[name]
    assert [e["step"] for e in run.log] == list(cfg.steps)
    assert run.max_twin_diff == 0.0 and run.probes_run > 50 * len(cfg.steps)
    for m in SC.DRIVER_METHODS:
        assert hasattr(FakeIndex, m), m


@pytest.mark.parametrize("name", list(SC.SESSIONS))
def test_near_tie_condition_holds_for_the_committed_seeds(faithful, name):
    run, _ = faithful[name]
    assert run.near_ties == [], run.near_ties[:5]


@pytest.mark.parametrize("name", list(SC.SESSIONS))
def test_schedules_force_their_transitions(faithful, name):
    run, infos = faithful[name]
    live = {e["step"]: e["live"] for e in run.log}
    cap0 = max(1024, -(-SC.SESSIONS[name].n0 // 256) * 256) * SC.SESSIONS[name].devices      # api.hip: index_grow, per shard
    assert live["first_delete"] < live["late_columns"] and 0 in infos["first_delete"]["deleted"]
    assert infos["first_delete"]["deleted"][-1] == SC.SESSIONS[name].n0 - 1 and 101 in infos["first_delete"]["deleted"]
    assert live["first_delete"] < live["add_into_tail"] <= cap0 < live["grow_with_columns"]
    assert live["delete_after_update"] < live["update_topk"] == live["grow_with_columns"]
    if "gather_sizes" in live:
        g = infos["gather_sizes"]["per_device"]
        assert g["small"] <= SC.GATHER_ROWS < g["large"] <= SC.SUB_FIRST_CAP < g["above"] <= SC.WIDE_GATHER_ROWS
    if "shrink_word_border" in live:
        i = infos["shrink_word_border"]
        assert (i["n_old"] - 1) // 32 > (i["n_new"] - 1) // 32 and i["n_new"] % 32 != 0
        # no delete before it crosses a word border: the step is the first to leave whole stale words behind
        for step in ("first_delete", "delete_after_update"):
            before = live[list(live)[list(live).index(step) - 1]]
            assert (before + 31) // 32 == (live[step] + 31) // 32, step
    if "shrink_block_border" in live:
        i = infos["shrink_block_border"]
        assert (i["n_old"] - 1) // 32768 > (i["n_new"] - 1) // 32768 and i["n_new"] % 256 not in (0, 255)
    # step 5: in both updates one row enters the top-k of the step's query on its (moved) position, next to the one that leaves
    for step in ("update_topk", "update_again"):
        assert infos[step]["entered"] in infos[step]["updated"] and infos[step]["updated"].size >= 4
    # the lists of every checkpoint name one id never given and, once rows were deleted, the lowest deleted id, the one deleted
    # last and one from the middle of every delete; step 8's own deleted id is among them, between two live ids
    seen = []
    for e in run.log:
        if "deleted" in infos[e["step"]]:
            seen.append(infos[e["step"]]["deleted"])
        named = e["not_live"]
        assert sum(not any(i in d for d in seen) for i in named) == 1 and named[-1] > max([int(d.max()) for d in seen] + [e["live"]]), e
        for d in seen:
            assert int(d[d.size // 2]) in named
        if seen:
            assert min(int(d.min()) for d in seen) in named and int(seen[-1][-1]) in named
    if "delete_then_add" in live:
        gone = int(infos["delete_then_add"]["deleted"][0])
        last = run.log[-1]
        assert gone in last["not_live"] and run.model.live[0] < gone < run.model.live[-1] and last["step"] == "delete_then_add"
    if "delete_all" in live:
        assert live["delete_all"] == 0 and live["refill"] > 2 * SC.GATHER_ROWS
    # the row sets: wherever the index holds enough rows with field values, one set for each route and an empty one
    for e in run.log:
        sizes = e["sets"]
        if e["step"] == "add_first" or e["live"] == 0:
            continue
        assert sizes["pred_big"] > SC.GATHER_ROWS and sizes["list_big"] > SC.GATHER_ROWS and sizes["both"] > 0, e
        assert 0 < sizes["pred_small"] <= SC.GATHER_ROWS and 0 < sizes["list_small"] <= SC.GATHER_ROWS, e
        assert sizes["pred_empty"] == 0 and sizes["list_empty"] == 0


# the step whose checkpoint (or whose own probes) first sees each fault
FAILS_AT = {
    "keys_stay": "first_delete",
    "field_tail": "add_into_tail",
    "bits_beyond_n": "shrink_word_border",
    "gather_leftover": "add_first",            # the first checkpoint already gathers a small set after a larger one
    "update_one_route": "update_topk",         # the row that enters a top-k there; see the test below
    "deleted_resolves": "first_delete",
    "no_id_after_map": "add_into_tail",
    "collapsed_inherits_keys": "late_columns",  # the first two collapsed searches over gathered keys
}


@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_fault_fails_at_its_step(fault):
    assert set(FAILS_AT) == set(FAULTS)
    with pytest.raises(SC.CheckpointFailure) as e:
        _run("flat_bf16", fault)
    print(fault, "->", e.value)
    assert e.value.step == FAILS_AT[fault], str(e.value)


def test_group_and_ivf_schedules_see_the_faults_their_steps_cover():
    """the shorter schedules still hold the steps that expose these"""
    for name, faults in (("group", ("keys_stay", "no_id_after_map", "update_one_route", "gather_leftover")),
                         ("ivf", ("field_tail", "deleted_resolves", "collapsed_inherits_keys"))):
        for fault in faults:
            with pytest.raises(SC.CheckpointFailure) as e:
                _run(name, fault)
            assert e.value.step == FAILS_AT[fault], (name, str(e.value))


def test_a_stale_first_pass_copy_shows_only_where_an_updated_row_enters_a_top_k():
    """The stand-in takes the plain search's candidates from a copy of the rows and scores them from the master, as the library
    does.  With updates that only move rows OUT of every top-k, a copy the update never refreshes costs a wasted candidate and
    the whole schedule passes; with the schedule's updates, which also move a row IN, it fails at the first of them -- and
    again, with a copy that is stale only from the second update on, on the positions the delete moved the rows to."""
    run, _ = _run("flat_bf16", "update_one_route", entering_updates=False)
    assert [e["step"] for e in run.log] == list(SC.SESSIONS["flat_bf16"].steps)
    with pytest.raises(SC.CheckpointFailure) as e:
        _run("flat_bf16", "update_one_route")
    assert e.value.step == "update_topk" and e.value.probe == "search", str(e.value)

    class StaleFromTheSecondUpdate(FakeIndex):
        updates = 0

        def update(self, ids, x):
            self.updates += 1
            self.fault = "update_one_route" if self.updates == 2 else None
            super().update(ids, x)
            self.fault = None
    for name in ("flat_bf16", "flat_int8"):
        cfg = SC.SESSIONS[name]
        run = SC.Run(cfg, StaleFromTheSecondUpdate(cfg.dim), fake_twin)
        with pytest.raises(SC.CheckpointFailure) as e:
            SC.run_session(run)
        assert e.value.step == "update_again" and e.value.probe == "search", (name, str(e.value))


def test_a_dead_id_between_live_ones_is_named_on_the_lists():
    """the deleted_resolves stand-in leaves an id below every live id alone (as id 0 is after first_delete) and resolves only a
    dead id between two live ones: it is seen at first_delete because the lists name such an id, and with the lowest deleted
    id alone on them it would pass that step"""
    with pytest.raises(SC.CheckpointFailure) as e:
        _run("flat_bf16", "deleted_resolves")
    assert e.value.step == "first_delete"
    cfg = SC.SESSIONS["flat_bf16"]
    run = SC.Run(cfg, FakeIndex(cfg.dim, "deleted_resolves"), fake_twin)
    run.not_live = lambda: np.asarray(([min(run.deleted)] if run.deleted else []) + [run.model.next_id + 50], np.int64)
    SC.run_session(run)
