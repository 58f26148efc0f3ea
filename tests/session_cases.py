"""Model-based session tests: one seeded schedule of mutations on one index, every query kind after every mutation.

The pieces, all without a GPU:
* ``Config`` / ``SESSIONS``: the four sessions (shapes, seeds, which steps).
* ``Run``: applies every mutation to a tests.session_model.SessionModel and to a DRIVER, the subset of VectorIndex methods the
  session calls (see ``DRIVER_METHODS``).  The driver is the real index on the GPU (tests/test_session_gpu.py) and a NumPy
  stand-in, faithful or with one seeded fault, on the CPU (tests/session_fakes.py, tests/test_session_cpu.py).
* ``Run.checkpoint``: every probe on one batch of B = 9 queries, answered by the driver, compared with two oracles:
    - the TWIN, a fresh index built from the model's live rows in ascending id order with the model's keys and fields
      (positions map back through the live ids; an IVF session's twin is FLAT): every integer equal, cosines and MMR / fused
      scores within 1e-6 (the bound tests/test_delete_gpu.py::_fresh_equivalence holds an index and its rebuild to), and the
      restricted radial / collapsed / MMR calls bit for bit (tests/test_within_gpu.py::_same);
    - the MODEL, independent of the library: plain, filtered and search_where top-k by gpu_util.assert_topk_matches at its
      default tolerances, the integer calls against agg_reference / sort_reference / FieldModel exactly, the read-backs exactly
      (get_rows against the float64 normalisation within the bound of tests/test_copies_gpu.py::_check_fp32).
* ``STEPS``: the schedule, each step named after the transition it forces; a checkpoint follows every step.

A condition on the inputs: in the float64 model no two adjacent scores among the ranked rows a probe can look at (its top
k + 1, the candidates of MMR and fusion, the prefix a collapsed search walks) lie closer than NEAR_TIE = 1e-5, five times the
2e-6 assert_topk_matches takes for a tie, unless the two rows are bit-identical (planted duplicates, which must resolve to the
lowest live id).  Every checkpoint records the violations in ``Run.near_ties``; the seeds in SESSIONS leave it empty."""
import time

import numpy as np

from oracle import retrieval as R
from tests import agg_reference, sort_reference
from tests.fields_reference import NONE
from tests.gpu_util import assert_topk_matches
from tests.session_model import SessionModel

B = 9
K = 10                                   # plain, filtered, excluding, where
K_COLLAPSED = 4
K_MMR, N_CAND = 4, 8
K_FUSED, FUSE_DEPTH = 5, 8
FUSE_OFFSETS = np.array([0, 3, 6, 9], np.int64)
N_DENY = 3
RADIAL_HITS = 10
GATHER_ROWS = 256                        # "filter_gather_rows" of the session index and of every twin
WIDE_GATHER_ROWS = 2048                  # ... during the step gather_sizes
SUB_FIRST_CAP = 1024                     # rows the scratch sub-index holds once allocated (api.hip: index_grow's minimum)
CAT, YEAR, SHARD, UNSET = 0, 1, 5, 3     # field slots; UNSET never gets a value
NEAR_TIE = 1e-5
TWIN_TOL = 1e-6
ROUTE_NONE, ROUTE_GATHER, ROUTE_MASK = 0, 1, 2
RADIAL, COLLAPSED, MMR = 1, 2, 3         # the kinds within_last reports

DRIVER_METHODS = ("add", "update", "delete", "set_keys", "set_field", "set_option", "search", "search_filtered_each",
                  "search_excluding", "range_search", "search_collapsed", "search_mmr", "search_fused", "search_where",
                  "search_where_each", "aggregate_fields", "sort_fields", "count_fields", "match_fields", "ids", "get_rows",
                  "get_keys", "get_field", "__len__")

PRED_BIG = [(YEAR, "range", 2004, None)]
PRED_EMPTY = [(YEAR, "range", 3000, None)]
AGGS = [(YEAR, "stats"), (CAT, "terms", 5)]
SORT = [(YEAR, "desc", {"missing": "first"}), (CAT, "asc")]


class Config:
    def __init__(self, name, dim, seed, n0, steps, small_shard, small_list, kind="flat", int8=False, nlist=0, devices=1):
        self.name, self.dim, self.seed, self.n0, self.steps = name, dim, seed, n0, tuple(steps)
        self.small_shard = small_shard          # SHARD <= small_shard selects about 150 rows
        self.small_list = small_list            # per mille of the live ids on the small list
        self.kind, self.int8, self.nlist, self.devices = kind, int8, nlist, devices
        self.planted = int8                     # see _plant
        # rows that take the index past its first capacity (api.hip: index_grow; every shard of a group has its own)
        self.grow_add = 600 if int8 else (500 if devices == 1 else 2600)
        self.entering_updates = True            # see _update; False only where tests/test_session_cpu.py shows what that misses

    @property
    def pred_small(self):
        return [(SHARD, "range", 0, self.small_shard), (CAT, "in", [11], {"not_": True})]


ALL_STEPS = ("add_first", "late_columns", "first_delete", "add_into_tail", "grow_with_columns", "gather_sizes", "update_topk",
             "delete_after_update", "update_again", "shrink_word_border", "shrink_block_border", "delete_all", "refill",
             "delete_then_add")

SESSIONS = {
    # steps 1-8; 700 rows fill 22 bitmap words and no multiple of 32
    "flat_bf16": Config("flat_bf16", 64, 0, 700, [s for s in ALL_STEPS if s != "shrink_block_border"], 180, 130),
    # steps 2, 3, 5, 6 (after the two of step 1 that give it rows and columns): 33,000 rows cross one bitmap block
    "flat_int8": Config("flat_int8", 256, 3, 33000, ALL_STEPS[:5] + ALL_STEPS[6:11], 5, 5, int8=True),
    # steps 1-3, 5, 7
    "ivf": Config("ivf", 64, 2, 700, ALL_STEPS[:5] + ALL_STEPS[6:9] + ALL_STEPS[11:13], 180, 130, kind="ivf", nlist=8),
    # steps 1-5 and 8 on three logical shards
    "group": Config("group", 64, 4, 700, ALL_STEPS[:9] + ALL_STEPS[13:], 70, 55, devices=3),
}


def mix(ids, salt):
    """a 64-bit hash of every id (splitmix64's finaliser): what decides keys, field values and list membership"""
    with np.errstate(over="ignore"):
        z = np.asarray(ids, np.int64).astype(np.uint64) + np.uint64(salt) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def keys_of(ids, seed):
    ids = np.asarray(ids, np.int64)
    keys = (ids // 3) * 7 + 5                                # at most 3 rows a key
    return np.where(mix(ids, seed + 11) % np.uint64(20) == 0, NONE, keys)


def field_of(slot, ids, seed):
    ids = np.asarray(ids, np.int64)
    if slot == CAT:
        return (mix(ids, seed + 21) % np.uint64(12)).astype(np.int64)
    if slot == YEAR:
        year = 2000 + (mix(ids, seed + 31) % np.uint64(21)).astype(np.int64)
        return np.where(mix(ids, seed + 41) % np.uint64(10) == 0, NONE, year)
    if slot == SHARD:
        return (mix(ids, seed + 51) % np.uint64(1000)).astype(np.int64)
    raise ValueError(slot)


class CheckpointFailure(AssertionError):
    def __init__(self, step, probe, detail):
        super().__init__(f"step {step}: {probe}: {detail}")
        self.step, self.probe, self.detail = step, probe, detail


class RowSet:
    def __init__(self, pred, allow, S):
        self.pred, self.allow, self.S = pred, allow, S

    @property
    def route(self):
        return ROUTE_NONE if self.S.size == 0 else (ROUTE_GATHER if self.S.size <= GATHER_ROWS else ROUTE_MASK)


class Probe:
    """One call: fn(driver, tr) -> tuple of arrays, tr translating id lists (the identity for the session index, ids ->
    positions for the twin).  out: one letter per output, c = cosines / scores, i = ids, n = integers.  bits: the floats are
    compared with the twin's on their bits.  expect: what the route read-backs must show after the call on the session index,
    ("within", kind, route, selected) or ("where", route, selected)."""

    def __init__(self, name, out, fn, bits=False, expect=None):
        self.name, self.out, self.fn, self.bits, self.expect = name, out, fn, bits, expect


def _agg_flat(res):
    out = [np.int64(res["selected"])]
    for a in res["aggs"]:
        out += [a["count"], a["min"], a["max"], a["sum"], a["n_buckets"], a["other"], np.asarray(a["keys"]), np.asarray(a["counts"])]
    return tuple(out)


def _sort_flat(res):
    return np.int64(res["total"]), np.asarray(res["ids"]), np.asarray(res["values"])


class Run:
    """One session.  driver: the index under test; make_twin(model) -> a driver over a fresh index of the model's live rows;
    routes: the driver has where_last / within_last (a single-device index)."""

    def __init__(self, cfg, driver, make_twin, routes=False, log=None):
        self.cfg, self.driver, self.make_twin, self.routes = cfg, driver, make_twin, routes
        self.model = SessionModel(cfg.dim)
        self.rng = np.random.default_rng(cfg.seed)
        self.deleted = []                      # every id deleted so far, in order
        self.deleted_inside = []               # one id from the middle of every delete
        self.near_ties = []
        self.max_twin_diff = 0.0
        self.probes_run = 0
        self.q = None
        self.step = None
        self.radial = {}                       # probe name -> (row set, thresholds) of the radial probes since the last check
        self.log = log if log is not None else []

    # ------------------------------------------------------------ mutations: model and driver alike
    def rows(self, m):
        return self.rng.standard_normal((m, self.cfg.dim)).astype(np.float32)

    def add(self, x):
        self.driver.add(x)
        return self.model.add(x)

    def update(self, ids, x):
        self.driver.update(np.asarray(ids, np.int64), x)
        self.model.update(ids, x)

    def delete(self, ids):
        ids = np.asarray(ids, np.int64)
        self.driver.delete(ids)
        self.model.delete(ids)
        self.deleted += ids.tolist()
        self.deleted_inside.append(int(ids[ids.size // 2]))

    def set_columns(self, ids, keys=True):
        """keys and the three field columns of these live rows, from the hash of their ids"""
        ids = np.asarray(ids, np.int64)
        if keys:
            self.driver.set_keys(ids, keys_of(ids, self.cfg.seed))
            self.model.set_keys(ids, keys_of(ids, self.cfg.seed))
        for slot in (CAT, YEAR, SHARD):
            self.driver.set_field(slot, ids, field_of(slot, ids, self.cfg.seed))
            self.model.set_field(slot, ids, field_of(slot, ids, self.cfg.seed))

    # ------------------------------------------------------------ the float64 model of the scores
    def _scores(self):
        """float64 [n_live, B]: normalised fp32 rows x normalised fp32 queries"""
        xn = self.model.normalized().astype(np.float64)
        return xn @ R.normalize_rows(self.q).astype(np.float64).T

    def ranked(self, scores, S, b, depth=None):
        """-> (ids, scores) of the rows S (ascending live ids) for query b: best first, ties to the lowest id"""
        pos = np.searchsorted(self.model.live, S)
        s = scores[pos, b]
        if depth is not None and 0 < depth < S.size:
            near = np.flatnonzero(s >= np.partition(s, S.size - depth)[S.size - depth])
            S, s = S[near], s[near]
        order = np.lexsort((S, -s))
        if depth is not None:
            order = order[:depth]
        return S[order], s[order]

    def _collapsed_prefix(self, ids, k):
        """rows of a ranking a collapsed search of k walks to see k + 1 groups"""
        if ids.size == 0:
            return 0
        key = self.model.keys(ids)
        key = np.where(key == NONE, -ids - 1, key)
        _, first = np.unique(key, return_index=True)
        first = np.sort(first)
        return int(first[k]) + 1 if first.size > k else ids.size

    def _near_tie_check(self, name, scores, S, depth_of):
        for b in range(B):
            ids, s = self.ranked(scores, S, b, 64)
            d = min(ids.size, depth_of(ids))
            gaps = s[:d - 1] - s[1:d]
            for j in np.flatnonzero(gaps < NEAR_TIE):
                a, c = int(ids[j]), int(ids[j + 1])
                if gaps[j] == 0 and np.array_equal(self.model.rows[a].view(np.uint32), self.model.rows[c].view(np.uint32)) and a < c:
                    continue                                  # a planted duplicate: the lower id ranks first
                self.near_ties.append((self.step, name, b, a, c, float(gaps[j])))

    # ------------------------------------------------------------ the row sets of a checkpoint
    def listed(self, S, rng):
        """an allow-list for the ids S: shuffled, with repeats, one deleted id and one id that was never given"""
        return rng.permutation(np.concatenate([S, S[:5], self.not_live()])).astype(np.int64)

    def not_live(self):
        """ids that name no row: one never given; of the deleted ones the lowest, the one deleted last and one from the middle
        of every delete so far (ids between live ones, whose place in the id order a live row took)"""
        return np.unique(np.asarray([self.model.next_id + 50] + ([min(self.deleted), self.deleted[-1]] if self.deleted else [])
                                    + self.deleted_inside, np.int64))

    def draw_sets(self, rng):
        m, cfg = self.model, self.cfg
        live = m.live
        h = mix(live, cfg.seed + 61) % np.uint64(1000)
        sets = {}

        def put(name, pred, of):
            allow = None if of is None else self.listed(of, rng)
            sets[name] = RowSet(pred, allow, m.select(pred, allow))

        put("pred_big", PRED_BIG, None)
        put("pred_small", cfg.pred_small, None)
        put("pred_empty", PRED_EMPTY, None)
        put("list_big", [], live[h < 550])
        put("list_small", [], live[h < cfg.small_list])
        put("list_empty", [], live[:0])
        put("both", PRED_BIG, live[h < 700])
        assert sets["list_empty"].S.size == 0 and sets["pred_empty"].S.size == 0
        return sets

    # ------------------------------------------------------------ probes
    def _thresholds(self, scores, S):
        """float32 [B]: between the third and the fourth best score of S, so a radial search counts three rows (more where
        rows are duplicates); -1 where S holds fewer than four rows"""
        t = np.full(B, -1.0, np.float32)
        for b in range(B):
            _, s = self.ranked(scores, S, b, 4)
            if s.size == 4 and s[2] - s[3] >= NEAR_TIE:
                t[b] = np.float32(0.5 * (s[2] + s[3]))
            elif s.size == 4 and s[2] != s[3]:                  # too close for a threshold between them: a near tie, on record
                self.near_ties.append((self.step, "threshold", b, -1, -1, float(s[2] - s[3])))
        return t

    def restricted_probes(self, name, rs, t, route=None):
        """the three restricted kinds on one row set; route None: do not look at within_last"""
        q = self.q
        self.radial[f"range_search[{name}]"] = (rs.S, t)

        def exp(kind):
            return None if route is None else ("within", kind, route, rs.S.size)
        return [
            Probe(f"range_search[{name}]", "nci",
                  lambda d, tr: d.range_search(q, t, RADIAL_HITS, pred=rs.pred, filter_ids=tr(rs.allow)), True, exp(RADIAL)),
            Probe(f"range_search[{name}, all]", "nci",
                  lambda d, tr: d.range_search(q, -1.0, 3, pred=rs.pred, filter_ids=tr(rs.allow)), True, exp(RADIAL)),
            Probe(f"search_collapsed[{name}]", "cin",
                  lambda d, tr: d.search_collapsed(q, K_COLLAPSED, pred=rs.pred, filter_ids=tr(rs.allow)), True, exp(COLLAPSED)),
            Probe(f"search_mmr[{name}]", "cic",
                  lambda d, tr: d.search_mmr(q, K_MMR, lam=0.5, n_cand=N_CAND, pred=rs.pred, filter_ids=tr(rs.allow)), True,
                  None if route is None else ("within", MMR, None, rs.S.size)),      # its route is search_where's own choice
        ]

    def where_probe(self, name, rs, where_route):
        """search_where with "where_route" forced (1 gather, 2 mask) and put back"""
        q = self.q

        def fn(d, tr):
            d.set_option("where_route", where_route)
            try:
                return d.search_where(q, K, rs.pred, filter_ids=tr(rs.allow))
            finally:
                d.set_option("where_route", 0)
        route = ROUTE_NONE if rs.S.size == 0 else (ROUTE_GATHER if where_route == 1 or self.cfg.kind == "ivf" else ROUTE_MASK)
        return Probe(f"search_where[{name}]", "ci", fn, False, ("where", route, rs.S.size))

    def standard_probes(self, sets, scores):
        q, m = self.q, self.model
        live = m.live
        loq = (np.arange(B) % 3).astype(np.int32)
        lists = ("list_big", "list_small", "list_empty")
        preds = ("pred_big", "pred_small", "pred_empty")
        deny = []
        for b in range(B):
            top = self.ranked(scores, live, b, N_DENY)[0]
            deny.append(np.concatenate([top, self.not_live()]) if b % 2 == 0 else None)
        P = [Probe("search", "ci", lambda d, tr: d.search(q, K))]
        for s in lists:
            P.append(Probe(f"search[filter_ids={s}]", "ci", lambda d, tr, a=sets[s].allow: d.search(q, K, filter_ids=tr(a))))
        P.append(Probe("search_filtered_each", "ci",
                       lambda d, tr: d.search_filtered_each(q, K, [tr(sets[s].allow) for s in lists], loq)))
        P.append(Probe("search_excluding", "ci",
                       lambda d, tr: d.search_excluding(q, K, [None if x is None else tr(x) for x in deny])))
        t_all = self._thresholds(scores, live)
        self.radial["range_search"] = (live, t_all)
        P.append(Probe("range_search", "nci", lambda d, tr: d.range_search(q, t_all, RADIAL_HITS)))
        P.append(Probe("range_search[all]", "nci", lambda d, tr: d.range_search(q, -1.0, 4)))
        P.append(Probe("search_collapsed", "cin", lambda d, tr: d.search_collapsed(q, K_COLLAPSED)))
        P.append(Probe("search_mmr", "cic", lambda d, tr: d.search_mmr(q, K_MMR, lam=0.5, n_cand=N_CAND)))
        P.append(Probe("search_fused", "cic", lambda d, tr: d.search_fused(q, K_FUSED, offsets=FUSE_OFFSETS, depth=FUSE_DEPTH)))
        P.append(self.where_probe("pred_big", sets["pred_big"], 2))
        P.append(self.where_probe("pred_small", sets["pred_small"], 1))
        P.append(self.where_probe("pred_empty", sets["pred_empty"], 1))
        P.append(self.where_probe("both", sets["both"], 2))
        each = [sets[s].pred for s in preds]
        P.append(Probe("search_where_each", "ci", lambda d, tr: d.search_where_each(q, K, each, loq)))
        # a predicate alone first (its kernel writes every word of the map, the padding included), then a list alone, then both
        for s in ("pred_big", "pred_small", "list_big", "list_small", "list_empty", "both"):
            rs = sets[s]
            P += self.restricted_probes(s, rs, self._thresholds(scores, rs.S), rs.route if self.routes else None)
        big, lst = sets["pred_big"], sets["list_big"]
        P.append(Probe("aggregate_fields", "n" * 17, lambda d, tr: _agg_flat(d.aggregate_fields(big.pred, AGGS))))
        P.append(Probe("aggregate_fields[list]", "n" * 17,
                       lambda d, tr: _agg_flat(d.aggregate_fields(big.pred, AGGS, filter_ids=tr(lst.allow)))))
        P.append(Probe("sort_fields", "nin", lambda d, tr: _sort_flat(d.sort_fields(big.pred, SORT, 20))))
        P.append(Probe("sort_fields[list]", "nin", lambda d, tr: _sort_flat(d.sort_fields([], SORT, 20, filter_ids=tr(lst.allow)))))
        P.append(Probe("count_fields", "n", lambda d, tr: (d.count_fields(each),)))
        P.append(Probe("match_fields", "ni", lambda d, tr: d.match_fields(each, 7)))
        return P

    # ------------------------------------------------------------ comparing
    def _fail(self, probe, detail):
        raise CheckpointFailure(self.step, probe, detail)

    def _compare_twin(self, p, got, want, live):
        if len(got) != len(want) or len(got) != len(p.out):
            self._fail(p.name, f"{len(got)} outputs, the twin {len(want)}")
        for j, (g, w, what) in enumerate(zip(got, want, p.out)):
            if isinstance(g, (int, np.integer)) or isinstance(w, (int, np.integer)):
                if int(g) != int(w):
                    self._fail(p.name, f"output {j}: {g} but the twin {w}")
                continue
            g, w = np.asarray(g), np.asarray(w)
            if what == "i":
                w = np.where(w >= 0, live[np.clip(w, 0, max(live.size - 1, 0))] if live.size else -1, -1)
            if g.shape != w.shape or g.dtype != w.dtype:
                self._fail(p.name, f"output {j}: {g.dtype}{g.shape} but the twin {w.dtype}{w.shape}")
            if what in "in":
                if not np.array_equal(g, w):
                    at = np.argwhere(g != w)[0].tolist()
                    self._fail(p.name, f"output {j} differs from the twin at {at}: {g[tuple(at)]} vs {w[tuple(at)]}")
                continue
            fin = np.isfinite(w)
            if not np.array_equal(np.isfinite(g), fin) or not np.array_equal(g[~fin], w[~fin]):
                self._fail(p.name, f"output {j}: the padding differs from the twin's")
            diff = float(np.abs(g[fin].astype(np.float64) - w[fin].astype(np.float64)).max()) if fin.any() else 0.0
            self.max_twin_diff = max(self.max_twin_diff, diff)
            if p.bits and not np.array_equal(g.view(np.uint32), w.view(np.uint32)):
                self._fail(p.name, f"output {j}: bits differ from the twin's (largest difference {diff:.3g})")
            if diff > TWIN_TOL:
                self._fail(p.name, f"output {j}: {diff:.3g} from the twin, above {TWIN_TOL}")

    def _check_routes(self, p):
        if not self.routes or p.expect is None:
            return
        expect = p.expect
        if p.expect[0] == "within":
            last = self.driver.within_last()
            got = ("within", last["kind"], last["route"], last["selected"])
            if p.expect[2] is None:                              # MMR: whichever route the search_where inside it took
                where = self.driver.where_last()
                if where["selected"] != p.expect[3]:
                    self._fail(p.name, f"read-back {where} of the search_where inside it, expected {p.expect[3]} selected rows")
                expect = p.expect[:2] + (where["route"],) + p.expect[3:]
        else:
            last = self.driver.where_last()
            got = ("where", last["route"], last["selected"])
        if got != expect or last["live"] != len(self.model):
            self._fail(p.name, f"read-back {last}, expected {expect} over {len(self.model)} live rows")

    def to_twin(self):
        """the translation of an id list for the twin: a live id becomes its position, every other id one the twin never gave"""
        live = self.model.live

        def tr(ids):
            if ids is None:
                return None
            ids = np.asarray(ids, np.int64).reshape(-1)
            pos = np.searchsorted(live, ids)
            hit = (pos < live.size) & (live[np.minimum(pos, max(live.size - 1, 0))] == ids) if live.size else np.zeros(ids.size, bool)
            return np.where(hit, pos, live.size + 50).astype(np.int64)
        return tr

    def run_probes(self, probes, twin, after=None):
        """every probe on the driver and on the twin -> {name: the driver's outputs}"""
        live = self.model.live.copy()
        tr = self.to_twin()
        results = {}
        for p in probes:
            got = p.fn(self.driver, lambda ids: ids)
            self._check_routes(p)
            if after is not None:
                after(p)
            want = p.fn(twin, tr)
            self._compare_twin(p, tuple(got), tuple(want), live)
            results[p.name] = got
            self.probes_run += 1
        return results

    # ------------------------------------------------------------ the model's own checks
    def _topk_ref(self, scores, S, k):
        cos = np.full((B, k), -np.inf)
        ids = np.full((B, k), -1, np.int64)
        for b in range(B):
            i, s = self.ranked(scores, S, b, k)
            cos[b, :i.size], ids[b, :i.size] = s, i
        return cos, ids

    def model_checks(self, sets, scores, results):
        m = self.model
        xn, qn = m.by_id(), R.normalize_rows(self.q)
        topk = [("search", m.live)] + [(f"search[filter_ids={s}]", sets[s].S) for s in ("list_big", "list_small", "list_empty")]
        topk += [(f"search_where[{s}]", sets[s].S) for s in ("pred_big", "pred_small", "pred_empty", "both")]
        for name, S in topk:
            cos, ids = results[name]
            ref_cos, ref_ids = self._topk_ref(scores, S, K)
            try:
                if np.any((ids < -1) | (ids >= xn.shape[0])):
                    raise AssertionError("an id that was never given")
                assert_topk_matches(cos, ids, ref_cos, ref_ids, xn, qn)
                # bit-identical rows score alike: the lower id must come first, which the helper's tolerance would not insist on
                tie = (ref_cos[:, 1:] == ref_cos[:, :-1]) & (ref_ids[:, 1:] >= 0)
                assert np.array_equal(ids[:, 1:][tie], ref_ids[:, 1:][tie]) and np.array_equal(ids[:, :-1][tie], ref_ids[:, :-1][tie]), \
                    "duplicate rows do not resolve to the lowest live id"
            except AssertionError as e:
                self._fail(name, f"against the float64 model: {e}")
        self.radial_checks(scores, results)
        big, lst = sets["pred_big"], sets["list_big"]
        each = [sets[s].pred for s in ("pred_big", "pred_small", "pred_empty")]
        want = agg_reference.aggregate(m.fm, big.pred, AGGS)
        if tuple(map(_plain, results["aggregate_fields"])) != tuple(map(_plain, _agg_flat(want))):
            self._fail("aggregate_fields", "differs from agg_reference")
        want = agg_reference.aggregate(m.fm, big.pred, AGGS, filter_ids=lst.allow)
        if tuple(map(_plain, results["aggregate_fields[list]"])) != tuple(map(_plain, _agg_flat(want))):
            self._fail("aggregate_fields[list]", "differs from agg_reference")
        for name, pred, allow in (("sort_fields", big.pred, None), ("sort_fields[list]", [], lst.allow)):
            total, ids, values = results[name]
            got = {"total": int(total), "ids": ids, "values": values}
            if not sort_reference.same(got, sort_reference.sort_fields(m.fm, pred, SORT, 20, filter_ids=allow)):
                self._fail(name, "differs from sort_reference")
        counts, ids = m.fm.match(each, 7)
        if not np.array_equal(results["count_fields"][0], counts):
            self._fail("count_fields", f"{results['count_fields'][0]} but FieldModel {counts}")
        if not (np.array_equal(results["match_fields"][0], counts) and np.array_equal(results["match_fields"][1], ids)):
            self._fail("match_fields", "differs from FieldModel")
        for name in ("range_search[all]",) + tuple(f"range_search[{s}, all]" for s in sets if s != "pred_empty"):
            size = len(m) if name == "range_search[all]" else sets[name[13:-6]].S.size
            if not np.all(results[name][0] == size):
                self._fail(name, f"counts {results[name][0]} at threshold -1, the set holds {size} rows")

    def radial_checks(self, scores, results):
        """the counts of every radial probe since the last call: the rows of the set at or above the threshold, which lies
        5e-6 or more from every score"""
        for name, (S, t) in self.radial.items():
            if name not in results:                          # a step that ran only some of a set's restricted probes
                continue
            pos =np.searchsorted(self.model.live, S)
            want = (scores[pos] >= t.astype(np.float64)[None, :]).sum(axis=0)
            if not np.array_equal(results[name][0], want):
                self._fail(name, f"counts {results[name][0]} but the float64 model counts {want}")
        self.radial = {}

    def readback_checks(self):
        m, d = self.model, self.driver
        live = m.live
        if len(d) != len(m):
            self._fail("len", f"{len(d)} but the model holds {len(m)}")
        ids = d.ids()
        if ids.dtype != np.int64 or not np.array_equal(ids, live):
            self._fail("ids", "differ from the model's live ids")
        self.probes_run += 2
        if live.size == 0:
            return
        if not np.array_equal(d.get_keys(live), m.keys()):
            self._fail("get_keys", f"differ from the model's at ids {live[d.get_keys(live) != m.keys()][:5]}")
        for slot in (CAT, YEAR, SHARD, UNSET):
            got = d.get_field(slot, live)
            if not np.array_equal(got, m.field(slot)):
                self._fail(f"get_field[{slot}]", f"differ from the model's at ids {live[got != m.field(slot)][:5]}")
        sample = live if live.size <= 4096 else np.unique(np.concatenate([live[:300], live[-600:], live[::61]]))
        got = d.get_rows(sample)
        x64 = m.raw(sample).astype(np.float64)
        ref = x64 / (np.sqrt((x64 * x64).sum(axis=1, keepdims=True)) + 1e-9)
        bound = (self.cfg.dim / 128 + 6) * 2.0 ** -24              # tests/test_copies_gpu.py::_check_fp32
        bad = np.abs(got.astype(np.float64) - ref) > bound * np.abs(ref)
        if got.dtype != np.float32 or bad.any():
            self._fail("get_rows", f"rows of ids {sample[bad.any(axis=1)][:5]} are not the model's rows, normalised")
        self.probes_run += 6

    # ------------------------------------------------------------ a checkpoint
    def checkpoint(self, after=None):
        t0 = time.perf_counter()
        rng = np.random.default_rng([self.cfg.seed, len(self.log)])
        scores = self._scores()
        sets = self.draw_sets(rng)
        deep = lambda ids: max(K + N_DENY + 1, self._collapsed_prefix(ids, K_COLLAPSED), N_CAND + 1, FUSE_DEPTH + 1)
        self._near_tie_check("all", scores, self.model.live, deep)
        for name, rs in sets.items():
            self._near_tie_check(name, scores, rs.S, lambda ids: max(K + 1, self._collapsed_prefix(ids, K_COLLAPSED), N_CAND + 1))
        twin = self.make_twin(self.model)
        results = self.run_probes(self.standard_probes(sets, scores), twin, after)
        self.model_checks(sets, scores, results)
        self.readback_checks()
        self.log.append({"step": self.step, "live": len(self.model), "sets": {k: int(v.S.size) for k, v in sets.items()},
                         "not_live": self.not_live().tolist(),
                         "seconds": time.perf_counter() - t0})
        return sets, scores, twin


def _plain(v):
    return v.tolist() if isinstance(v, np.ndarray) else int(v)


# ---------------------------------------------------------------------------------------------- the schedule
# Every step changes the model and the driver through the Run and returns what it did, for the read-back assertions of
# tests/test_session_gpu.py.  Step numbers are those of the issue this schedule was written for.
PLANTED, PLANT_TOP, PLANT_STEP = 60, 0.9, 0.008


def _plant(run, x):
    """Tens of thousands of random rows in dim 256 lie too densely under a random query for the near-tie condition to hold at
    any seed.  So every query gets PLANTED rows, at random positions, built as c q + sqrt(1 - c^2) u with u orthogonal to q:
    their cosines are c = 0.9, 0.892, ... to fp32 rounding, 0.008 apart and far above what a random row scores (about 0.27
    at most), so the top of every ranking over a large part of the index is made of them.  Position 101 (duplicated by
    add_first) holds the second best row of query 5."""
    rng, n0 = run.rng, x.shape[0]
    free = np.setdiff1d(np.arange(n0), [101, 200, 450])
    spots = rng.choice(free, (B, PLANTED), replace=False)
    spots[5, 1] = 101
    qh = run.q.astype(np.float64)
    qh /= np.sqrt((qh * qh).sum(axis=1, keepdims=True))
    for b in range(B):
        for j in range(PLANTED):
            c = PLANT_TOP - PLANT_STEP * j
            u = rng.standard_normal(x.shape[1])
            u -= (u @ qh[b]) * qh[b]
            u /= np.sqrt(u @ u)
            x[spots[b, j]] = ((c * qh[b] + np.sqrt(1 - c * c) * u) * rng.uniform(0.5, 2.0)).astype(np.float32)


def add_first(run):
    """1. the first rows (three bit-identical ones among them), the query batch near some of them; an IVF driver trains"""
    cfg = run.cfg
    x = run.rows(cfg.n0)
    run.q = run.rows(B)
    if cfg.planted:
        _plant(run, x)
    else:
        near = run.rng.integers(0, cfg.n0, 5)
        run.q[:5] = x[near] + 0.3 * run.q[:5]
        run.q[5] = x[101] + 0.3 * run.q[5]
    x[200] = x[450] = x[101]
    run.add(x)
    if hasattr(run.driver, "session_train"):
        run.driver.session_train(x)
    return {"added": cfg.n0}


def late_columns(run):
    """1. keys and fields for the first time, on rows that already exist: the columns are allocated late"""
    run.set_columns(run.model.live)
    return {}


def first_delete(run):
    """2. the id map appears: position 0, the last position, the best row of query 0, the lowest duplicate and a few more"""
    live = run.model.live
    scores = run._scores()
    top = run.ranked(scores, live, 0, 1)[0]
    ids = np.unique(np.concatenate([live[[0, -1, 31, 32, 333]], top, [101]]))
    run.delete(ids)
    return {"deleted": ids}


def add_into_tail(run):
    """3. rows that still fit the capacity land on the positions the delete freed: they have no key and no field value"""
    return {"added": run.add(run.rows(20)).size}


def grow_with_columns(run):
    """3. past the capacity while map, keys and fields are live: every buffer is reallocated and swapped"""
    return {"added": run.add(run.rows(run.cfg.grow_add)).size}


def gather_sizes(run):
    """4. on the gather route: a large set, a small one (the tail of the sub-index is zeroed), one above the sub-index's
    capacity (it is reallocated); then a collapsed search that gathers keys, a radial and a plain filtered search"""
    m = run.model
    live = m.live
    rng = np.random.default_rng([run.cfg.seed, 99])
    scores = run._scores()
    twin = run.make_twin(m)
    sets = {"large": live[mix(live, 71) % np.uint64(1000) < 600], "small": live[mix(live, 72) % np.uint64(1000) < 80],
            "above": live[mix(live, 73) % np.uint64(1000) < 975]}
    # what one device gathers: on a group every shard gathers its own rows (id modulo the shards) into its own sub-index
    per_device = {k: int(np.bincount(v % run.cfg.devices, minlength=run.cfg.devices).max()) for k, v in sets.items()}
    assert GATHER_ROWS < per_device["large"] <= SUB_FIRST_CAP and 0 < per_device["small"] <= GATHER_ROWS
    assert SUB_FIRST_CAP < per_device["above"] <= WIDE_GATHER_ROWS
    q = run.q
    P = []
    for d in (run.driver, twin):
        d.set_option("filter_gather_rows", WIDE_GATHER_ROWS)
    try:
        for name in ("large", "small", "above"):
            allow = run.listed(sets[name], rng)
            rs = RowSet([], allow, m.select([], allow))
            run._near_tie_check(f"gather_{name}", scores, rs.S, lambda ids: max(K + 1, run._collapsed_prefix(ids, K_COLLAPSED), N_CAND + 1))
            t = run._thresholds(scores, rs.S)
            P += run.restricted_probes(f"gather_{name}", rs, t, ROUTE_GATHER if run.routes else None)
            P.append(run.where_probe(f"gather_{name}", rs, 1))
            P.append(Probe(f"search[filter_ids=gather_{name}]", "ci", lambda d, tr, a=allow: d.search(q, K, filter_ids=tr(a))))
        # keys gathered for one set must not answer for the next
        small = RowSet([], run.listed(sets["small"], rng), sets["small"])
        pred = RowSet(run.cfg.pred_small, None, m.select(run.cfg.pred_small))
        for name, rs in (("keys_small", small), ("keys_pred", pred), ("keys_small_again", small)):
            P.append(run.restricted_probes(name, rs, run._thresholds(scores, rs.S), ROUTE_GATHER if run.routes and rs.S.size else None)[2])
        P += run.restricted_probes("after_keys", small, run._thresholds(scores, small.S), ROUTE_GATHER if run.routes else None)[:2]
        P.append(Probe("search[filter_ids=after_keys]", "ci", lambda d, tr: d.search(q, K, filter_ids=tr(small.allow))))
        results = run.run_probes(P, twin)
        run.radial_checks(scores, results)
        for name in ("large", "small", "above"):
            if not np.all(results[f"range_search[gather_{name}, all]"][0] == sets[name].size):
                run._fail(f"range_search[gather_{name}, all]", f"counts at threshold -1, the set holds {sets[name].size} rows")
    finally:
        for d in (run.driver, twin):
            d.set_option("filter_gather_rows", GATHER_ROWS)
    return {"gathered": {k: int(v.size) for k, v in sets.items()}, "per_device": per_device}


def row_at_cosine(run, b, c):
    """a raw row whose cosine with query b is c to fp32 rounding: c q + sqrt(1 - c^2) u, u orthogonal to q, at some length"""
    qh = run.q[b].astype(np.float64)
    qh /= np.sqrt(qh @ qh)
    u = run.rng.standard_normal(run.cfg.dim)
    u -= (u @ qh) * qh
    u /= np.sqrt(u @ u)
    return ((c * qh + np.sqrt(1 - c * c) * u) * run.rng.uniform(0.5, 2.0)).astype(np.float32)


def _update(run, b, extra, enter_at, cosine):
    """Overwrites the second best row of query b and the rows at the positions `extra` with random vectors, which leave every
    top-k.  The row at position `enter_at` instead gets a vector that ENTERS the top-k of query b (at `cosine`, between two
    planted steps of flat_int8 and below the best row elsewhere): a search whose first pass reads a copy of the rows (bf16
    scan copy, int8 tiles) takes its candidates from that copy and re-scores them from the master, so a copy left stale by
    the update only costs a candidate when a row leaves, but misses the row when it enters."""
    live = run.model.live
    top = run.ranked(run._scores(), live, b, 2)[0][1:]                 # the second best row of query b
    ids = np.unique(np.concatenate([top, live[extra], live[[enter_at]]]))
    x = run.rows(ids.size)
    if run.cfg.entering_updates:
        x[np.searchsorted(ids, live[enter_at])] = row_at_cosine(run, b, cosine)
    run.update(ids, x)
    if run.cfg.entering_updates:
        assert live[enter_at] in run.ranked(run._scores(), live, b, K)[0] and top[0] not in run.ranked(run._scores(), live, b, K)[0]
    return {"updated": ids, "entered": int(live[enter_at])}


def update_topk(run):
    """5. rows overwritten: one of them leaves the current top-k, one enters it"""
    return _update(run, 1, [0, 256, -1], 255, PLANT_TOP - 2.5 * PLANT_STEP)


def delete_after_update(run):
    """5. ... then a delete: the compaction moves the overwritten rows"""
    live = run.model.live
    ids = live[[1, 2, 257, 600, -2, -3]]
    run.delete(ids)
    return {"deleted": ids}


def update_again(run):
    """5. ... then overwritten again, on the positions the delete moved them to (one row leaves a top-k, one enters it); half of
    the rows added since get keys and field values"""
    out = _update(run, 2, [0, 255, -1], 254, PLANT_TOP - 4.5 * PLANT_STEP)
    late = run.model.live[run.model.keys() == NONE]
    late = late[late >= run.cfg.n0][::2]
    run.set_columns(late)
    out["columns"] = late.size
    return out


def _delete_tail(run, new_n, inner):
    live = run.model.live
    ids = np.unique(np.concatenate([live[new_n + len(inner):], live[inner]]))
    run.delete(ids)
    assert len(run.model) == new_n
    # the first row sets after the shrink: a predicate alone (its kernel writes every word of the map, the padding included),
    # then a list alone (the map is cleared and marked); the checkpoint that follows starts with lists
    scores = run._scores()
    sets = run.draw_sets(np.random.default_rng([run.cfg.seed, 98]))
    P = []
    for s in ("pred_big", "list_big"):
        rs = sets[s]
        run._near_tie_check(f"shrunk, {s}", scores, rs.S, lambda ids: max(K + 1, run._collapsed_prefix(ids, K_COLLAPSED), N_CAND + 1))
        P += run.restricted_probes(f"shrunk, {s}", rs, run._thresholds(scores, rs.S), rs.route if run.routes else None)[:3]
        P.append(run.where_probe(f"shrunk, {s}", rs, 1))
    results = run.run_probes(P, run.make_twin(run.model))
    run.radial_checks(scores, results)
    for s in ("pred_big", "list_big"):
        if not np.all(results[f"range_search[shrunk, {s}, all]"][0] == sets[s].S.size):
            run._fail(f"range_search[shrunk, {s}, all]", f"counts at threshold -1, the set holds {sets[s].S.size} rows")
    return {"deleted": ids, "n_old": live.size, "n_new": new_n}


def shrink_word_border(run):
    """6. down across a 32-position word border of the allow bitmap, to the middle of a word"""
    n = len(run.model)
    new_n = (n - 1) // 32 * 32 - 32 - 14
    return _delete_tail(run, new_n, [5, 40, 41])


def shrink_block_border(run):
    """6. down across a border of 1,024 words (32,768 positions), to the middle of a 256-row tile"""
    n = len(run.model)
    assert n > 32768
    return _delete_tail(run, 32768 - 102, [7, 300, 20000])


def delete_all(run):
    """7. everything goes: every probe on the empty index"""
    ids = run.model.live.copy()
    run.delete(ids)
    return {"deleted": ids}


def refill(run):
    """7. rows again, on the positions of the old ones; keys and field values for three in four of them"""
    ids = run.add(run.rows(640))
    run.set_columns(ids[ids % 4 != 3])
    return {"added": ids.size}


def delete_then_add(run):
    """8. an id goes and rows come: the lists of the checkpoint name the deleted id and an id never given"""
    live = run.model.live
    gone = live[[live.size // 2]]
    run.delete(gone)
    ids = run.add(run.rows(9))
    run.set_columns(ids[:4])
    return {"deleted": gone, "added": ids.size}


STEPS = {f.__name__: f for f in (add_first, late_columns, first_delete, add_into_tail, grow_with_columns, gather_sizes, update_topk,
                                 delete_after_update, update_again, shrink_word_border, shrink_block_border, delete_all, refill,
                                 delete_then_add)}


def run_session(run, before=None, after=None, after_probe=None):
    """the whole schedule: before(run, name) and after(run, name, info) surround every step, a checkpoint follows it"""
    run.driver.set_option("filter_gather_rows", GATHER_ROWS)
    for name in run.cfg.steps:
        run.step = name
        if before is not None:
            before(run, name)
        info = STEPS[name](run)
        if after is not None:
            after(run, name, info)
        run.checkpoint(after_probe)
    return run

