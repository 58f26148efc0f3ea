"""Numeric fields of a named index: the schema ``GpuSearchClient.configure_fields`` declares, what a document's value becomes on
the device (an int64 per row and field slot, ``VectorIndex.set_field``), and the translation of OpenSearch ``range`` / ``term`` /
``terms`` / ``exists`` clauses into device predicates (``VectorIndex.match_fields`` / ``search_where``).

The device compares int64 only:
  long / integer   the value itself
  boolean          0 / 1
  date             epoch milliseconds (an int is taken as such; a string is ISO 8601, without an offset UTC)
  double / float   ``engine.f64_image``, the order-preserving image of the double
  keyword          a dense code from a per-field host dictionary (exact, no hashing); a value the dictionary has never seen
                   selects nothing
"""
from __future__ import annotations

import datetime as _dt
import math
from typing import Dict, List, Optional, Set

import numpy as np

from .engine import AGG_MAX, FIELD_MAX_CLAUSES, FIELD_MAX_PREDS, FIELD_MAX_SET, FIELD_NONE, MAX_FIELDS, f64_from_image, f64_image  # noqa: F401

FIELD_TYPES = ("long", "integer", "boolean", "date", "double", "float", "keyword")
RESERVED = ("doc_id", "text", "embedding")      # what the docstore and the other routes already own
I64_MAX = (1 << 63) - 1
NOTHING = ("range", 1, 0)                        # lo > hi: holds for no row
_EPOCH = _dt.datetime(1970, 1, 1, tzinfo=_dt.timezone.utc)


class FieldValueError(ValueError):
    """A document's value does not parse as its field's type (OpenSearch: mapper_parsing_exception)."""


def _date_ms(v) -> int:
    if isinstance(v, bool):
        raise ValueError("a boolean is no date")
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, str):
        s = v.strip()
        if s.lstrip("-").isdigit():
            return int(s)
        d = _dt.datetime.fromisoformat(s[:-1] + "+00:00" if s.endswith(("Z", "z")) else s)
        if d.tzinfo is None:
            d = d.replace(tzinfo=_dt.timezone.utc)
        delta = d - _EPOCH
        return (delta.days * 86_400 + delta.seconds) * 1000 + delta.microseconds // 1000
    raise ValueError(f"{type(v).__name__} is no date")


def _integral(v) -> int:
    if isinstance(v, bool):
        raise ValueError("a boolean is no integer")
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        if not math.isfinite(v) or v != math.floor(v):
            raise ValueError(f"{v} is no integer")
        return int(v)
    if isinstance(v, str):
        return int(v.strip())
    raise ValueError(f"{type(v).__name__} is no integer")


def _boolean(v) -> int:
    if isinstance(v, (bool, np.bool_)):
        return int(v)
    if isinstance(v, str) and v in ("true", "false"):
        return int(v == "true")
    raise ValueError(f"{v!r} is no boolean (true / false)")


def _double(v) -> float:
    if isinstance(v, bool):
        raise ValueError("a boolean is no number")
    f = float(v)
    if f != f:
        raise ValueError("NaN is no field value")
    return f


class FieldSchema:
    """The fields of one index: name -> (slot, type), and the keyword dictionaries."""

    def __init__(self):
        self.slot: Dict[str, int] = {}
        self.type: Dict[str, str] = {}
        self.codes: Dict[str, Dict[str, int]] = {}       # keyword field -> value -> dense code
        self.inverse: Dict[str, List[str]] = {}          # keyword field -> code -> value, rebuilt when the dictionary has grown

    def declare(self, mapping: Dict[str, str]) -> None:
        """Add fields (a name declared before keeps its slot and must keep its type).  ValueError, with nothing changed: an
        unknown type, a reserved name, a ninth field."""
        fresh = []
        for name, ftype in mapping.items():
            if ftype not in FIELD_TYPES:
                raise ValueError(f"field [{name}]: type [{ftype}] is not served ({' / '.join(FIELD_TYPES)})")
            if name in RESERVED:
                raise ValueError(f"field [{name}] is not configurable: the docstore owns it")
            if name in self.type:
                if self.type[name] != ftype:
                    raise ValueError(f"field [{name}] is a {self.type[name]} already")
            elif name not in fresh:
                fresh.append(name)
        if len(self.slot) + len(fresh) > MAX_FIELDS:
            raise ValueError(f"an index holds at most {MAX_FIELDS} fields ({len(self.slot)} declared, {len(fresh)} more asked for)")
        for name in fresh:
            self.slot[name] = len(self.slot)
            self.type[name] = mapping[name]
            if mapping[name] == "keyword":
                self.codes[name] = {}

    # ---- values
    def parse(self, name: str, v):
        """The canonical host value of a document's field (what ``sources`` keeps), or FieldValueError."""
        t = self.type[name]
        try:
            if t in ("long", "integer"):
                out = _integral(v)
                if not (FIELD_NONE < out <= I64_MAX) or (t == "integer" and not -(1 << 31) <= out < (1 << 31)):
                    raise ValueError(f"{out} is out of range")
                return out
            if t == "boolean":
                return bool(_boolean(v))
            if t == "date":
                out = _date_ms(v)
                if not (FIELD_NONE < out <= I64_MAX):
                    raise ValueError(f"{out} is out of range")
                return int(v) if isinstance(v, np.integer) else v
            if t in ("double", "float"):
                return _double(v)
            if isinstance(v, (dict, list, tuple)):
                raise ValueError("a keyword is one scalar value")
            return v if isinstance(v, str) else str(v)
        except (ValueError, TypeError, OverflowError) as e:
            raise FieldValueError(f"failed to parse field [{name}] of type [{t}]: {e}") from None

    def device_value(self, name: str, v, learn: bool) -> Optional[int]:
        """The int64 the device holds for host value ``v`` (FIELD_NONE for None).  ``learn``: an unseen keyword gets the next
        code; otherwise it gives None -- it equals no stored value."""
        if v is None:
            return FIELD_NONE
        t = self.type[name]
        if t in ("long", "integer"):
            return _integral(v)
        if t == "boolean":
            return _boolean(v)
        if t == "date":
            return _date_ms(v)
        if t in ("double", "float"):
            return f64_image(_double(v))
        table = self.codes[name]
        key = v if isinstance(v, str) else str(v)
        if learn:
            return table.setdefault(key, len(table))
        return table.get(key)

    def document_fields(self, doc: Dict) -> Dict:
        """The configured fields a document carries, parsed (None and absent: no value)."""
        out = {}
        for name in self.slot:
            v = doc.get(name) if isinstance(doc, dict) else None
            if v is not None:
                out[name] = self.parse(name, v)
        return out

    # ---- clauses
    def _bound(self, name: str, v, key: str):
        """The inclusive int64 bound of ``{key: v}`` (gt / gte / lt / lte), or None for a bound no value meets."""
        t = self.type[name]
        lower = key in ("gt", "gte")
        if t in ("double", "float"):
            f = float(v)
            if f != f:
                return None
            b = f64_image(f)
        elif t == "boolean":
            b = _boolean(v)
        else:
            if isinstance(v, (float, np.floating)) and not isinstance(v, bool) and t != "date":
                if v != v:
                    return None
                if v == math.inf or v == -math.inf:
                    if (v > 0) == lower:
                        return None
                    return FIELD_NONE + 1 if lower else I64_MAX
                if v != math.floor(v):                    # 2015.5: gte / gt -> 2016, lte / lt -> 2015, both inclusive already
                    key = "gte" if lower else "lte"
                    b = math.floor(v) + 1 if lower else math.floor(v)
                else:
                    b = int(v)
            else:
                b = _date_ms(v) if t == "date" else _integral(v)
        if key == "gt":
            b += 1
        elif key == "lt":
            b -= 1
        if lower:
            return None if b > I64_MAX else max(b, FIELD_NONE + 1)
        return None if b <= FIELD_NONE else min(b, I64_MAX)

    def leaf(self, clause) -> Optional[tuple]:
        """The device clause ``(slot, "range", lo, hi)`` / ``(slot, "in", values)`` of a ``range`` / ``term`` / ``terms`` /
        ``exists`` clause on a configured field; None for any other clause (another route may serve it).  ValueError for a
        malformed clause on a configured field."""
        if not isinstance(clause, dict) or len(clause) != 1:
            return None
        (kind, spec), = clause.items()
        if kind not in ("range", "term", "terms", "exists") or not isinstance(spec, dict):
            return None
        if kind == "exists":
            name = spec.get("field")
            if set(spec) != {"field"} or name not in self.slot:
                return None
            return (self.slot[name], "range", None, None)
        names = [n for n in spec if n != "boost"]
        if len(names) != 1 or names[0] not in self.slot:
            return None
        name, v = names[0], spec[names[0]]
        slot, t = self.slot[name], self.type[name]
        try:
            if kind == "range":
                if t == "keyword":
                    raise ValueError("a keyword field has no order")
                if not isinstance(v, dict) or not set(v) <= {"gt", "gte", "lt", "lte", "boost", "format", "relation"}:
                    raise ValueError("takes gt / gte / lt / lte")
                lo, hi = FIELD_NONE + 1, I64_MAX
                for key in ("gt", "gte", "lt", "lte"):
                    if v.get(key) is None:
                        continue
                    b = self._bound(name, v[key], key)
                    if b is None:
                        return (slot,) + NOTHING
                    lo, hi = (max(lo, b), hi) if key in ("gt", "gte") else (lo, min(hi, b))
                return (slot, "range", lo, hi) if lo <= hi else (slot,) + NOTHING
            if kind == "term":
                if isinstance(v, dict):
                    v = v["value"]
                if isinstance(v, (dict, list)):
                    raise ValueError("takes one value")
                if t in ("double", "float") and float(v) != float(v):
                    return (slot,) + NOTHING
                d = self.device_value(name, v, learn=False)
                return (slot,) + NOTHING if d is None or d == FIELD_NONE else (slot, "range", d, d)
            if not isinstance(v, list):
                raise ValueError("takes a list of values")
            vals = set()
            for w in v:
                if t in ("double", "float") and float(w) != float(w):
                    continue
                d = self.device_value(name, w, learn=False)
                if d is not None and d != FIELD_NONE:
                    vals.add(d)
            if len(vals) > FIELD_MAX_SET:
                raise ValueError(f"{len(vals)} values (at most {FIELD_MAX_SET})")
            return (slot, "in", sorted(vals)) if vals else (slot,) + NOTHING
        except (KeyError, TypeError, ValueError, OverflowError) as e:
            raise ValueError(f"{kind} on field [{name}] of type [{t}]: {e}") from None

    def conjunction(self, clause) -> Optional[List[tuple]]:
        """The device predicate of a filter that is a pure conjunction of field leaves -- one leaf, or a ``bool`` with only
        ``filter`` / ``must`` / ``must_not`` whose members are all leaves -- or None.  At most 8 clauses and 4,096 set values;
        a longer one is composed on the host (``retrieval.filter_rows``)."""
        one = self.leaf(clause)
        if one is not None:
            return [one]
        if not isinstance(clause, dict) or set(clause) != {"bool"}:
            return None
        spec = clause["bool"]
        if not isinstance(spec, dict) or not spec or not set(spec) <= {"filter", "must", "must_not"}:
            return None
        pred = []
        for key in ("filter", "must", "must_not"):
            members = spec.get(key, [])
            for c in members if isinstance(members, list) else [members]:
                cl = self.leaf(c)
                if cl is None:
                    return None
                pred.append(cl + ({"not_": True},) if key == "must_not" else cl)
        n_set = sum(len(cl[2]) for cl in pred if cl[1] == "in")
        if len(pred) > FIELD_MAX_CLAUSES or n_set > FIELD_MAX_SET:
            return None
        return pred

    # ---- aggregations
    def _key(self, name: str, v: int):
        """A device value of field ``name`` in the field's own type -> (key, key_as_string or None)"""
        t = self.type[name]
        if t == "keyword":
            inverse = self.inverse.get(name)
            if inverse is None or len(inverse) != len(self.codes[name]):         # the dictionary only grows, densely
                inverse = self.inverse[name] = sorted(self.codes[name], key=self.codes[name].get)
            return inverse[v], None
        if t == "boolean":
            return v, "true" if v else "false"
        if t in ("double", "float"):
            return f64_from_image(v), None
        if t == "date":
            return v, _date_string(v)
        return v, None

    def aggregation(self, spec):
        """One OpenSearch aggregation body on a configured field -> (the device aggregation ``pack_aggs`` takes, shape), where
        ``shape(r)`` turns that aggregation's entry of ``VectorIndex.aggregate_fields`` into the OpenSearch answer.  Served (AGG_SERVED):
        ``terms`` on every type (keys come back in the field's own type; ties in count go to the lower value, for a keyword
        the value seen first), ``histogram`` on long / integer / date, ``date_histogram`` with a ``fixed_interval`` in ms / s /
        m / h / d, ``min`` / ``max`` / ``value_count`` on every type but keyword, ``stats`` / ``sum`` / ``avg`` on long / integer /
        boolean / date.  Everything else is a ValueError that says so."""
        if not isinstance(spec, dict):
            raise ValueError(f"an aggregation is an object; served: {AGG_SERVED}")
        if "aggs" in spec or "aggregations" in spec:
            raise ValueError(f"sub-aggregations are not served; served: {AGG_SERVED}")
        if len(spec) != 1:
            raise ValueError(f"an aggregation names one kind; served: {AGG_SERVED}")
        (kind, body), = spec.items()
        options = {"terms": {"field", "size"}, "histogram": {"field", "interval", "offset"}, "date_histogram": {"field", "fixed_interval"},
                   "min": {"field"}, "max": {"field"}, "value_count": {"field"}, "stats": {"field"}, "sum": {"field"}, "avg": {"field"}}
        if kind not in options:
            raise ValueError(f"aggregation [{kind}] is not served; served: {AGG_SERVED}")
        if not isinstance(body, dict) or "field" not in body:
            raise ValueError(f"aggregation [{kind}] needs a field; served: {AGG_SERVED}")
        if kind == "date_histogram" and "calendar_interval" in body:
            raise ValueError("date_histogram: calendar_interval is not served (a month has no fixed length); use fixed_interval in ms / s / m / h / d")
        extra = sorted(set(body) - options[kind])
        if extra:
            raise ValueError(f"aggregation [{kind}]: option {extra} is not served; served: {AGG_SERVED}")
        name = body["field"]
        if name not in self.slot:
            raise ValueError(f"aggregation [{kind}]: [{name}] is no configured field ({sorted(self.slot)})")
        slot, t = self.slot[name], self.type[name]

        def buckets(r, stringed):
            out = []
            for v, c in zip(r["keys"].tolist(), r["counts"].tolist()):
                key, text = self._key(name, v)
                out.append({"key": key, "key_as_string": text, "doc_count": c} if stringed and text is not None else {"key": key, "doc_count": c})
            return out

        if kind == "terms":
            size = body.get("size", 10)
            if isinstance(size, bool) or not isinstance(size, int) or not 1 <= size <= 256:
                raise ValueError(f"terms: size [{size}] is not served (1..256)")
            return (slot, "terms", size), lambda r: {"doc_count_error_upper_bound": 0, "sum_other_doc_count": r["other"],
                                                     "buckets": buckets(r, True)}
        if kind in ("histogram", "date_histogram"):
            if t not in (("date",) if kind == "date_histogram" else ("long", "integer", "date")):
                raise ValueError(f"{kind} on field [{name}] of type [{t}] is not served (histogram: long / integer / date fields; "
                                 "date_histogram: date fields; a float histogram would round)")
            if kind == "date_histogram":
                interval, offset = _fixed_interval_ms(body.get("fixed_interval")), 0
            else:
                interval, offset = body.get("interval"), body.get("offset", 0)
                for what, v in (("interval", interval), ("offset", offset)):
                    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != math.floor(v):
                        raise ValueError(f"histogram: {what} [{v}] is not served (an integer; interval >= 1 and 0 <= offset < interval)")
                interval, offset = int(interval), int(offset)
                if interval < 1 or not 0 <= offset < interval:
                    raise ValueError(f"histogram: interval [{interval}] / offset [{offset}] are not served (interval >= 1, 0 <= offset < interval)")
            return (slot, "histogram", interval, offset), lambda r: {"buckets": buckets(r, t == "date")}
        if t == "keyword":
            raise ValueError(f"{kind} on the keyword field [{name}] is not served (a keyword has no order; terms is)")
        if kind in ("stats", "sum", "avg") and t in ("double", "float"):
            raise ValueError(f"{kind} on field [{name}] of type [{t}] is not served: a floating-point sum has an accumulation order "
                             "(min / max / value_count / terms are)")

        def value(v):
            key, text = self._key(name, v)
            return {"value": key, "value_as_string": text} if t == "date" else {"value": key}

        def shape(r):
            n = r["count"]
            if kind == "value_count":
                return {"value": n}
            if kind in ("min", "max"):
                return value(r[kind]) if n else {"value": None}
            if kind == "sum":
                return {"value": r["sum"]}
            if kind == "avg":
                return {"value": r["sum"] / n if n else None}
            return {"count": n, "min": r["min"] if n else None, "max": r["max"] if n else None, "avg": r["sum"] / n if n else None,
                    "sum": r["sum"]}
        return (slot, "stats"), shape


    # ---- sorting
    def sort_spec(self, body):
        """An OpenSearch ``sort`` on configured fields -> (keys, names): the sort keys ``engine.pack_sort`` takes and the fields
        they name.  Served (SORT_SERVED): ``"year"``, ``{"year": "desc"}``, ``{"published": {"order": "asc", "missing": "_first" |
        "_last"}}`` and a list of at most 4 of these, on long / integer / boolean / date / double / float fields (``f64_image``
        keeps the order of doubles).  Missing values go last by default, whatever the order.  ValueError for everything else: a
        keyword field (its dictionary codes are in order of first appearance, not of the strings), ``_score`` / ``_doc``,
        ``mode`` / ``unmapped_type`` or any other option, a literal ``missing`` value, an undeclared field, a field named twice."""
        entries = body if isinstance(body, list) else [body]
        if not 1 <= len(entries) <= 4:
            raise ValueError(f"sort takes 1 to 4 keys, got {len(entries)}; served: {SORT_SERVED}")
        keys, names = [], []
        for e in entries:
            order, missing = "asc", "_last"
            if isinstance(e, str):
                name = e
            elif isinstance(e, dict) and len(e) == 1:
                (name, spec), = e.items()
                if isinstance(spec, str):
                    order = spec
                elif isinstance(spec, dict):
                    extra = sorted(set(spec) - {"order", "missing"})
                    if extra:
                        raise ValueError(f"sort on [{name}]: option {extra} is not served; served: {SORT_SERVED}")
                    order, missing = spec.get("order", "asc"), spec.get("missing", "_last")
                else:
                    raise ValueError(f"sort on [{name}]: an order or an object of options; served: {SORT_SERVED}")
            else:
                raise ValueError(f"a sort key is a field name or an object with one field; served: {SORT_SERVED}")
            if name in ("_score", "_doc"):
                raise ValueError(f"sort on [{name}] is not served; served: {SORT_SERVED}")
            if name not in self.slot:
                raise ValueError(f"sort: [{name}] is no configured field ({sorted(self.slot)})")
            if self.type[name] == "keyword":
                raise ValueError(f"sort on the keyword field [{name}] is not served: its device codes are in order of first appearance, "
                                 "not of the strings")
            if order not in ("asc", "desc"):
                raise ValueError(f"sort on [{name}]: order [{order}] is not served (asc / desc)")
            if isinstance(missing, bool) or missing not in ("_first", "_last"):
                raise ValueError(f"sort on [{name}]: missing [{missing}] is not served (_first / _last; a literal value is not)")
            if name in names:
                raise ValueError(f"sort names [{name}] twice")
            keys.append((self.slot[name], order, {"missing": missing[1:]}))
            names.append(name)
        return keys, names

    def sort_values(self, names: List[str], row) -> list:
        """A row of device values in the sort slots -> the values in the fields' own types: a date as epoch milliseconds, a
        double through ``f64_from_image``, a boolean as such, missing as None."""
        out = []
        for name, v in zip(names, row):
            t = self.type[name]
            v = int(v)
            out.append(None if v == FIELD_NONE else bool(v) if t == "boolean" else f64_from_image(v) if t in ("double", "float") else v)
        return out

    def sort_cursor(self, names: List[str], search_after):
        """OpenSearch ``search_after`` -- a hit's ``sort`` array ``[v_0, ..., id]`` -> the cursor ``VectorIndex.sort_fields``
        takes: (device values, None for missing; the id)."""
        if not isinstance(search_after, (list, tuple)) or len(search_after) != len(names) + 1:
            raise ValueError(f"search_after takes the {len(names) + 1} values of a hit's sort array (one per sort key, then the row id)")
        rid = search_after[-1]
        if isinstance(rid, bool) or not isinstance(rid, (int, np.integer)):
            raise ValueError(f"search_after: the last value [{rid}] is no row id")
        try:
            values = [None if v is None else int(self.device_value(name, v, learn=False)) for name, v in zip(names, search_after)]
        except (ValueError, TypeError, OverflowError) as e:
            raise ValueError(f"search_after: {e}") from None
        return values, int(rid)


SORT_SERVED = ("a field name, {field: 'asc' | 'desc'} or {field: {'order', 'missing': '_first' | '_last'}} on long / integer / "
               "boolean / date / double / float fields, at most 4 keys")

AGG_SERVED = ("terms {field, size}, histogram {field, interval, offset} on long / integer / date fields, date_histogram {field, "
              "fixed_interval}, min / max / value_count {field} on every type but keyword, stats / sum / avg {field} on long / "
              "integer / boolean / date fields")


def _fixed_interval_ms(v) -> int:
    units = {"ms": 1, "s": 1000, "m": 60_000, "h": 3_600_000, "d": 86_400_000}
    if isinstance(v, str):
        for unit in ("ms", "s", "m", "h", "d"):                # "ms" before "s"
            digits = v[:-len(unit)]
            if v.endswith(unit) and digits.isdigit() and int(digits) >= 1:
                return int(digits) * units[unit]
    raise ValueError(f"date_histogram: fixed_interval [{v}] is not served (a positive integer and ms / s / m / h / d, as in '1d')")


def _date_string(ms: int) -> str:
    """epoch milliseconds as OpenSearch prints a date (strict_date_optional_time, UTC)"""
    try:
        d = _EPOCH + _dt.timedelta(milliseconds=ms)
    except OverflowError:
        return str(ms)
    return d.strftime("%Y-%m-%dT%H:%M:%S.") + f"{d.microsecond // 1000:03d}Z"


# ------------------------------------------------------------------------------ the named index's side
def schema_of(idx) -> Optional[FieldSchema]:
    return getattr(idx, "fields", None)


def configure(idx, mapping: Dict[str, str]) -> FieldSchema:
    """Declare fields on a named index (caller holds ``idx.lock``).  Rows the index already holds are sent by the next push,
    with the values their documents carry."""
    schema = schema_of(idx) or FieldSchema()
    known = set(schema.slot)
    schema.declare(dict(mapping))
    idx.fields = schema
    if set(schema.slot) != known:
        idx.fields_sent_upto = 0                  # a new slot: every row's value goes out again
        idx.fields_stale = set()
    return schema


def field_changed(idx, row: int) -> None:
    """An overwrite replaced the document of stored row ``row`` (caller holds ``idx.lock``): its values are sent again."""
    if schema_of(idx) is not None:
        stale: Optional[Set[int]] = getattr(idx, "fields_stale", None)
        if stale is None:
            stale = idx.fields_stale = set()
        stale.add(row)


def push_fields(idx) -> int:
    """Send the field values of the rows the device does not have them for yet: every live row on the first call (also after
    ``load_index``: fields are not part of a saved index), afterwards the rows added since and the rows an overwrite changed.
    Caller holds ``idx.lock``.  -> rows sent."""
    schema = schema_of(idx)
    if schema is None:
        return 0
    upto = getattr(idx, "fields_sent_upto", 0)
    stale = getattr(idx, "fields_stale", None) or set()
    rows = sorted({r for r in stale if r < upto} | set(range(upto, len(idx.sources))))
    rows = [r for r in rows if idx.sources[r] is not None]
    if rows:
        ids = np.asarray(rows, np.int64)
        for name, slot in schema.slot.items():
            vals = [schema.device_value(name, idx.sources[r].get(name), learn=True) for r in rows]
            idx.vectors.set_field(slot, ids, np.asarray(vals, np.int64))
    idx.fields_sent_upto = len(idx.sources)
    idx.fields_stale = set()
    return len(rows)


def match_rows(idx, pred: List[tuple]) -> np.ndarray:
    """Vector ids (int64, ascending) of the live rows a device predicate selects.  Caller holds ``idx.lock``."""
    push_fields(idx)
    count = int(idx.vectors.count_fields([pred])[0])
    if count == 0:
        return np.empty(0, np.int64)
    return idx.vectors.match_fields([pred], count)[1][0]


def aggregate_rows(idx, aggs: Dict[str, Dict], pred: List[tuple], allow: Optional[np.ndarray]):
    """Named OpenSearch aggregations (``FieldSchema.aggregation``) over the live rows device predicate ``pred`` selects, also
    restricted to the vector ids ``allow`` when given -> (rows selected, {name: the OpenSearch answer}).  Eight aggregations go
    in one call (``VectorIndex.aggregate_fields``); more take one call per eight.  ValueError for what is not served, a histogram
    of more than 16,384 buckets included.  Caller holds ``idx.lock``."""
    from ._native import SqeError
    schema = schema_of(idx)
    if schema is None:
        raise ValueError("aggregations run on configured fields (configure_fields): this index has none")
    if not isinstance(aggs, dict) or not aggs:
        raise ValueError("aggs is an object of named aggregations")
    plans = [(name,) + schema.aggregation(spec) for name, spec in aggs.items()]
    push_fields(idx)
    selected, out = 0, {}
    for first in range(0, len(plans), AGG_MAX):
        chunk = plans[first:first + AGG_MAX]
        try:
            r = idx.vectors.aggregate_fields(pred, [agg for _, agg, _ in chunk], filter_ids=allow)
        except SqeError as e:
            if e.code == -1:
                raise ValueError(str(e)) from None
            raise
        selected = r["selected"]
        for (name, _, shape), one in zip(chunk, r["aggs"]):
            out[name] = shape(one)
    return selected, out


def sort_rows(idx, sort, k: int, pred: List[tuple], allow: Optional[np.ndarray], search_after=None):
    """The first ``k`` live rows, in the order of the OpenSearch ``sort`` (``FieldSchema.sort_spec``), of the rows device predicate
    ``pred`` selects, also restricted to the vector ids ``allow`` when given, after the cursor ``search_after`` when given ->
    (rows selected whatever the cursor, vector ids [m], their sort arrays ``[v_0, ..., id]``), one device call
    (``VectorIndex.sort_fields``).  ValueError for what is not served.  Caller holds ``idx.lock``."""
    from ._native import SqeError
    schema = schema_of(idx)
    if schema is None:
        raise ValueError("sort runs on configured fields (configure_fields): this index has none")
    keys, names = schema.sort_spec(sort)
    after = None if search_after is None else schema.sort_cursor(names, search_after)
    push_fields(idx)
    try:
        r = idx.vectors.sort_fields(pred, keys, k, filter_ids=allow, after=after)
    except SqeError as e:
        if e.code == -1:
            raise ValueError(str(e)) from None
        raise
    ids = r["ids"]
    return r["total"], ids, [schema.sort_values(names, r["values"][i]) + [int(ids[i])] for i in range(ids.shape[0])]
