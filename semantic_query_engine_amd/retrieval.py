"""Host-side mirror of the reference's retrieval interface, backed by libsqe (MI355X).

Same names, argument meaning, return shapes and error behaviour as the reference's
``app/main.py`` so ``RAGModel`` / the routes can call them unchanged:

    OpenSearchIndexer(client, index_name)        main.py:291-298
        .has_any_data() -> bool                  main.py:300-307
        .add_embeddings(embeddings, docs)        main.py:309-338
        .search(query_emb, k=3)                  main.py:347-373
    cosine_similarity(a, b) -> float             main.py:59-64
    lfu_cache_get(query_emb) -> Optional[str]    main.py:67-98
    lfu_cache_put(query_emb, response)           main.py:121-128

The OpenSearch ``client`` argument becomes a :class:`GpuSearchClient` (named indexes, each a
libsqe vector index in HBM plus a host docstore of ``_source`` dicts); Redis becomes a
:class:`SemanticLfuCache` (cache matrix resident in HBM, LFU bookkeeping on the host).
Everything numeric runs in the HIP library; nothing here falls back to NumPy.
"""
from __future__ import annotations

import numbers
import threading
import time
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

from .engine import INDEX_FLAT, CacheMatrix, Context, VectorIndex
from . import fields as F
from .fields import FieldValueError, push_fields

# Constants of the reference (main.py:35-44), names kept.
BATCH_SIZE = 64
CHUNK_SIZE = 512
EMBED_DIM = 1024
REDIS_MAX_ITEMS = 1000
CACHE_SIM_THRESHOLD = 0.96

_default_ctx: Optional[Context] = None
_ctx_lock = threading.Lock()


def default_context(device: Optional[int] = None, devices=None) -> Context:
    """Process-wide context.  ``devices=[0, 1, ...]``: this one process drives all of them (what the
    reference's single uvicorn process needs); otherwise one device -- ``device``, or LOCAL_RANK in the
    one-process-per-GPU form."""
    global _default_ctx
    with _ctx_lock:
        if _default_ctx is None:
            import os
            if devices is not None:
                _default_ctx = Context(devices=devices)
            else:
                dev = device if device is not None else int(os.environ.get("LOCAL_RANK", "0"))
                _default_ctx = Context(dev)
        return _default_ctx


# ------------------------------------------------------------------------------ index
class _GpuNamedIndex:
    """One OpenSearch index: vectors in HBM, ``_source`` documents on the host."""

    def __init__(self, ctx: Context, dim: int, kind: int, nlist: int):
        self.vectors = VectorIndex(ctx, dim, kind, nlist)
        self.sources: List[Optional[Dict[str, str]]] = []   # vector id -> {"doc_id", "text"}; None once deleted
        self.row_of_id: Dict[str, int] = {}           # OpenSearch _id -> vector id
        self.rows_of_doc: Dict[str, Set[int]] = {}    # doc_id -> vector ids of its live chunks (filters, delete_by_query)
        self.lock = threading.Lock()
        # collapsed search (push_keys): doc_id -> the int64 group key of its rows; rows below keys_sent_upto have had their key
        # sent to the device, except the ones in keys_stale (an overwrite changed their doc_id since)
        self.key_of_doc: Dict[str, int] = {}
        self.keys_sent_upto = 0
        self.keys_stale: Set[int] = set()
        # numeric fields (configure_fields / push_fields): the schema, and which rows' values the device holds -- as for the keys
        self.fields: Optional[F.FieldSchema] = None
        self.fields_sent_upto = 0
        self.fields_stale: Set[int] = set()


def _rows_of_doc(idx) -> Dict[str, Set[int]]:
    """The doc_id -> vector ids map of an index (built once from ``sources`` for an index object that has none)."""
    m = getattr(idx, "rows_of_doc", None)
    if m is None:
        m = {}
        for row, src in enumerate(idx.sources):
            if src is not None:
                m.setdefault(str(src["doc_id"]), set()).add(row)
        idx.rows_of_doc = m
    return m


def _doc_add(m: Dict[str, Set[int]], doc_id, row: int) -> None:
    m.setdefault(str(doc_id), set()).add(row)


def _doc_remove(m: Dict[str, Set[int]], doc_id, row: int) -> None:
    rows = m.get(str(doc_id))
    if rows is not None:
        rows.discard(row)
        if not rows:
            del m[str(doc_id)]


class GpuSearchClient:
    """Stands where the ``OpenSearch`` client object stood (main.py:250-259): a registry of
    named cosine indexes (the per-user ``<base>-<user_id>`` indexes of
    embedding_gen.py:211 are just more names)."""

    def __init__(self, ctx: Optional[Context] = None, dim: int = EMBED_DIM, kind: int = INDEX_FLAT,
                 nlist: int = 0, devices=None):
        """``devices=[0, ..., 7]``: every index of this client is sharded over those GPUs of the node, driven
        from this one process (ignored when a context is passed)."""
        self.ctx = ctx or default_context(devices=devices)
        self.dim, self.kind, self.nlist = dim, kind, nlist
        self._indexes: Dict[str, _GpuNamedIndex] = {}
        self._lock = threading.Lock()

    def index(self, name: str) -> _GpuNamedIndex:
        with self._lock:
            if name not in self._indexes:
                self._indexes[name] = _GpuNamedIndex(self.ctx, self.dim, self.kind, self.nlist)
            return self._indexes[name]

    def exists(self, name: str) -> bool:
        with self._lock:
            return name in self._indexes

    def count(self, index: str) -> Dict[str, int]:
        """Shape of ``client.count(index=...)`` (main.py:304-305): live documents."""
        return {"count": len(self.index(index).vectors)}

    def configure_fields(self, index: str, mapping: Dict[str, str]) -> None:
        """Declare the filterable fields of an index: ``{"year": "long", "user_id": "keyword", "published": "date", "impact":
        "double"}`` (types: long / integer / boolean / date / double / float / keyword; at most 8 fields per index).  From then
        on documents may carry these fields, a value that does not parse refuses the document (``FieldValueError``), and
        ``range`` / ``term`` / ``terms`` / ``exists`` on them are served as filters, evaluated on the device.  Declare them
        again after ``load_index``: a saved index keeps the documents' values, not the schema."""
        idx = self.index(index)
        with idx.lock:
            F.configure(idx, mapping)

    def aggregate(self, index: str, aggs: Dict[str, Dict], filter: Optional[Dict] = None) -> Dict:
        """OpenSearch ``aggs`` with ``"size": 0`` over the documents ``filter`` selects (None: every live one) ->
        {"selected": their number, "aggregations": {name: answer}} (``aggregate_filtered``)."""
        selected, out = aggregate_filtered(self.index(index), aggs, filter)
        return {"selected": selected, "aggregations": out}

    def search_sorted(self, index: str, sort, k: int = 10, filter: Optional[Dict] = None, search_after=None, from_: int = 0) -> Dict:
        """OpenSearch ``sort`` without a scoring query: the ``k`` first documents ``filter`` selects in field order ->
        {"total": documents selected, "hits": [(vector id, _source, sort array)]} (``sorted_filtered``)."""
        total, hits = sorted_filtered(self.index(index), sort, k, filter, search_after, from_)
        return {"total": total, "hits": hits}

    def delete(self, index: str, id: str, **_ignored) -> Dict:
        """Shape of opensearch-py's ``client.delete(index=, id=)``: ``result`` is ``deleted`` or ``not_found``."""
        found = delete_documents(self.index(index), [id])[0]
        return {"_index": index, "_id": id, "_version": 1, "result": "deleted" if found else "not_found",
                "_shards": {"total": 1, "successful": 1 if found else 0, "failed": 0}}

    def delete_by_query(self, index: str, body: Dict, **_ignored) -> Dict:
        """Shape of ``client.delete_by_query(index=, body=)`` for ``term`` / ``terms`` on ``doc_id`` and ``ids`` queries
        (withdrawing every chunk of a document: ``{"query": {"term": {"doc_id": "..."}}}``)."""
        t0 = time.perf_counter()
        n = delete_by_query(self.index(index), body)
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "total": n, "deleted": n, "batches": 1,
                "version_conflicts": 0, "noops": 0, "retries": {"bulk": 0, "search": 0}, "failures": []}

    # ---- persistence: OpenSearch kept the index across restarts, so ``has_any_data()`` could skip the
    # rebuild (main.py:422-424).  Here one named index = <dir>/<name>.sqeidx (vectors, sqe_index_save) +
    # <dir>/<name>.docs.jsonl ({"_id", "doc_id", "text"} of every live row, in ascending vector id -- the order in
    # which sqe_index_save writes the rows; after deletes VectorIndex.ids() pairs the two again on load).
    def save_index(self, name: str, directory: str) -> None:
        import json
        import os
        idx = self.index(name)
        os.makedirs(directory, exist_ok=True)
        with idx.lock:
            idx.vectors.save(os.path.join(directory, name + ".sqeidx"))
            id_of_row = {row: os_id for os_id, row in idx.row_of_id.items()}
            with open(os.path.join(directory, name + ".docs.jsonl"), "w", encoding="utf-8") as f:
                for row, src in enumerate(idx.sources):
                    if src is None:
                        continue
                    extra = {key: v for key, v in src.items() if key not in ("doc_id", "text")}      # configured field values
                    f.write(json.dumps({"_id": id_of_row[row], "doc_id": src["doc_id"], "text": src["text"], **extra}) + "\n")

    def load_index(self, name: str, directory: str) -> bool:
        """Load a saved index under ``name``; False when there is nothing to load."""
        import json
        import os
        vp, dp = os.path.join(directory, name + ".sqeidx"), os.path.join(directory, name + ".docs.jsonl")
        if not (os.path.exists(vp) and os.path.exists(dp)):
            return False
        named = _GpuNamedIndex.__new__(_GpuNamedIndex)
        named.vectors = VectorIndex.load(self.ctx, vp)
        ids = named.vectors.ids()
        named.sources, named.row_of_id, named.lock = [None] * named.vectors.next_id, {}, threading.Lock()
        named.rows_of_doc = {}
        lines = 0
        with open(dp, "r", encoding="utf-8") as f:
            for j, line in enumerate(f):
                lines += 1
                if j >= ids.shape[0]:
                    continue
                d = json.loads(line)
                row = int(ids[j])
                named.sources[row] = {key: v for key, v in d.items() if key != "_id"}
                named.row_of_id[d["_id"]] = row
                _doc_add(named.rows_of_doc, d["doc_id"], row)
        if lines != ids.shape[0]:
            raise ValueError(f"{name}: {lines} documents for {ids.shape[0]} vectors")
        with self._lock:
            self._indexes[name] = named
        return True


def delete_documents(idx: "_GpuNamedIndex", os_ids: List[str]) -> List[bool]:
    """OpenSearch "delete" of the given ``_id`` s of one index, in one device call: True where the ``_id`` existed
    (a repeat within the call is not found the second time).  The vectors go first; the docstore follows only once
    the device delete succeeded, so docstore and vector ids stay in step."""
    with idx.lock:
        found, rows, gone = [], [], set()
        for os_id in os_ids:
            row = idx.row_of_id.get(os_id)
            ok = row is not None and os_id not in gone
            found.append(ok)
            if ok:
                gone.add(os_id)
                rows.append(row)
        if rows:
            docs = _rows_of_doc(idx)
            idx.vectors.delete(np.asarray(rows, np.int64))
            for os_id in gone:
                row = idx.row_of_id.pop(os_id)
                _text_changed(idx, row, gone=True)
                _doc_remove(docs, idx.sources[row]["doc_id"], row)
                idx.sources[row] = None
            idx._id_of_row = None                     # (the shim's reverse map)
    return found


# ------------------------------------------------------------------------------ lexical side (BM25 over the `text` field)
LEX_MAX_QUERY = 64                                       # term occurrences of a lexical query (include/sqe.h: sqe_lex_search)


class Analyzer:
    """Text -> term ids for the lexical index: the WordPiece tokenizer without [CLS], [SEP] or [PAD].  Queries and documents
    go through this one function.  ``max_len`` bounds the word pieces of one text and has to hold a whole chunk."""

    def __init__(self, tokenizer, max_len: int = 4096, positions: bool = False):
        self.tokenizer, self.max_len, self.positions = tokenizer, int(max_len), bool(positions)
        self.n_terms = int(tokenizer.vocab_size)

    def analyze(self, texts: List[str]) -> List[np.ndarray]:
        ids, lens = self.tokenizer.encode_batch(list(texts), self.max_len + 2)
        return [ids[i, 1:int(lens[i]) - 1].copy() for i in range(len(texts))]      # between [CLS] and [SEP]; past lens: [PAD]

    def query(self, text: str) -> np.ndarray:
        """The term occurrences of a query: the first 64 word pieces of the text (sqe_lex_search takes no more)."""
        return self.analyze([text])[0][:LEX_MAX_QUERY]


_analyzer: Optional[Analyzer] = None


def configure_analyzer(tokenizer, max_len: int = 4096, positions: bool = False) -> None:
    """Install the process-wide analyzer of the ``text`` field (None: remove it).  Once one is configured, a named index
    grows a ``LexicalIndex`` the first time a text or hybrid query needs it (``push_text``); with none, nothing changes.
    ``positions``: documents are sent with their word-piece order (``LexicalIndex.put(..., ordered=True)``, four bytes per
    word piece on the device) and ``match_phrase`` is served (``text_clauses``); without it ``match_phrase`` stays refused."""
    global _analyzer
    _analyzer = None if tokenizer is None else Analyzer(tokenizer, max_len, positions)


# roles of a term occurrence and the translation of OpenSearch text clauses to them (include/sqe.h: sqe_lex_search_bool)
LEX_SHOULD, LEX_MUST, LEX_FILTER, LEX_MUST_NOT = 0, 1, 2, 3


def _min_should(v, n: int) -> int:
    """``minimum_should_match`` over ``n`` optional occurrences: a non-negative integer (also as a string), or a positive
    percentage ``"p%"``, floored as Lucene floors it."""
    if isinstance(v, str) and v.endswith("%") and v[:-1].isdigit():
        return n * int(v[:-1]) // 100
    if isinstance(v, str) and v.isdigit():
        v = int(v)
    if isinstance(v, bool) or not isinstance(v, int) or v < 0:
        raise ValueError(f"minimum_should_match [{v}] is not served (a non-negative integer or a positive percentage)")
    return v


def _match_parts(match) -> Tuple[np.ndarray, str, object]:
    """``{"text": "..." | {"query", "operator", "minimum_should_match"}}`` -> (term occurrences, operator, minimum_should_match
    or None); anything else in ``match`` (another field, fuzziness, ...) raises ValueError."""
    if _analyzer is None:
        raise ValueError("match needs an analyzer: retrieval.configure_analyzer(tokenizer)")
    if not isinstance(match, dict) or set(match) != {"text"}:
        raise ValueError("match is served on the [text] field only")
    spec = match["text"]
    operator, msm = "or", None
    if isinstance(spec, dict):
        if "query" not in spec or not set(spec) <= {"query", "operator", "minimum_should_match"}:
            raise ValueError(f"match.text takes [query], [operator] and [minimum_should_match], got {sorted(spec)}")
        operator, msm, spec = spec.get("operator", "or"), spec.get("minimum_should_match"), spec["query"]
        operator = operator.lower() if isinstance(operator, str) else operator
        if operator not in ("or", "and"):
            raise ValueError(f"match.text operator [{operator}] is not served (or, and)")
    if not isinstance(spec, str):
        raise ValueError("match.text query must be a string")
    return _analyzer.query(spec), operator, msm


def text_query(clause) -> Tuple[np.ndarray, np.ndarray, int]:
    """An OpenSearch clause on the analysed ``text`` field -> (terms int32, roles uint8, min_should) of ONE flat boolean query
    (``LexicalIndex.search_bool`` / ``match``).  Served, because they map onto the flat model exactly:
      ``{"match": {"text": "..." | {"query": "...", "operator": "or" | "and", "minimum_should_match": n | "p%"}}}``: ``or``
        makes every term SHOULD, ``and`` every term MUST (and takes no ``minimum_should_match``);
      ``{"bool": {"must": [...], "should": [...], "filter": [...], "must_not": [...], "minimum_should_match": n | "p%"}}`` whose
        members are such ``match`` clauses without a ``minimum_should_match`` of their own: a ``must`` / ``filter`` member must be
        single-term or ``operator: and``, a ``should`` member single-term or ``or`` (with ``minimum_should_match`` above 1 every
        ``should`` member must be single-term: OpenSearch counts clauses, the flat model occurrences), a ``must_not`` member of
        any operator makes all its terms MUST_NOT.  A bool that holds one ``must`` member and nothing else is that member, with
        every option a ``match`` takes.
    Anything else raises ValueError: nested bools, ``must`` of a multi-term ``or`` match, a bool without a positive clause,
    negative ``minimum_should_match``, other fields, fuzziness, more than 64 term occurrences."""
    if not isinstance(clause, dict) or len(clause) != 1:
        raise ValueError("a text clause is {'match': {'text': ...}} or a {'bool': {...}} of such clauses")
    (kind, spec), = clause.items()
    terms: List[int] = []
    roles: List[int] = []
    if kind == "match":
        t, operator, msm = _match_parts(spec)
        if operator == "and" and msm is not None:
            raise ValueError("match.text: minimum_should_match together with operator [and] is not served")
        terms, roles = t.tolist(), [LEX_MUST if operator == "and" else LEX_SHOULD] * len(t)
        ms = 0 if msm is None else _min_should(msm, len(terms))
    elif kind == "bool" and isinstance(spec, dict) and set(spec) == {"must"} and len(_as_list(spec["must"])) == 1:
        return text_query(_as_list(spec["must"])[0])      # a bool that is one must clause is that clause, options and all
    elif kind == "bool" and isinstance(spec, dict) and set(spec) <= {"must", "should", "filter", "must_not", "minimum_should_match"}:
        n_should = wide_should = 0
        for key, role in (("must", LEX_MUST), ("filter", LEX_FILTER), ("should", LEX_SHOULD), ("must_not", LEX_MUST_NOT)):
            for member in _as_list(spec.get(key, [])):
                if not isinstance(member, dict) or set(member) != {"match"}:
                    raise ValueError(f"bool.{key}: every member must be a match clause on [text]")
                t, operator, msm = _match_parts(member["match"])
                if msm is not None:
                    raise ValueError(f"bool.{key}: a member match with minimum_should_match is not served")
                if role in (LEX_MUST, LEX_FILTER) and len(t) > 1 and operator != "and":
                    raise ValueError(f"bool.{key}: a multi-term match needs operator [and]")
                if role == LEX_SHOULD and len(t) > 1 and operator != "or":
                    raise ValueError("bool.should: a multi-term match with operator [and] is not served")
                if role == LEX_SHOULD:
                    n_should += 1
                    wide_should += len(t) > 1
                terms += t.tolist()
                roles += [role] * len(t)
        ms = _min_should(spec["minimum_should_match"], n_should) if "minimum_should_match" in spec else 0
        if ms > 1 and wide_should:
            raise ValueError("bool: minimum_should_match above 1 needs single-term should members")
        if not any(r != LEX_MUST_NOT for r in roles):
            raise ValueError("bool: at least one must, filter or should term is needed")
    else:
        raise ValueError(f"text clause [{kind}] is not served (match on [text], bool of such matches)")
    if len(terms) > LEX_MAX_QUERY:
        raise ValueError(f"a text query holds at most {LEX_MAX_QUERY} term occurrences, got {len(terms)}")
    return np.asarray(terms, np.int32), np.asarray(roles, np.uint8), min(int(ms), LEX_MAX_QUERY + 1)


def has_phrase(clause) -> bool:
    """Whether ``match_phrase`` occurs anywhere in a clause: such a clause goes through ``text_clauses`` and the phrase calls
    of the lexical index, every other one keeps ``text_query`` and the boolean calls."""
    if isinstance(clause, dict):
        return "match_phrase" in clause or any(has_phrase(v) for v in clause.values())
    return isinstance(clause, list) and any(has_phrase(v) for v in clause)


def _phrase_parts(spec) -> List[int]:
    """``{"text": "..." | {"query": "...", "slop": 0}}`` -> the word pieces of the phrase, in order; a non-zero ``slop``,
    another field or any other option (``analyzer``, ...) raises ValueError, as does a phrase of more than 64 word pieces."""
    if _analyzer is None or not _analyzer.positions:
        raise ValueError("match_phrase needs an analyzer with positions: retrieval.configure_analyzer(tokenizer, positions=True)")
    if not isinstance(spec, dict) or set(spec) != {"text"}:
        raise ValueError("match_phrase is served on the [text] field only")
    spec = spec["text"]
    if isinstance(spec, dict):
        if "query" not in spec or not set(spec) <= {"query", "slop"}:
            raise ValueError(f"match_phrase.text takes [query] and [slop], got {sorted(spec)}")
        slop = spec.get("slop", 0)
        if isinstance(slop, bool) or not isinstance(slop, int) or slop != 0:
            raise ValueError(f"match_phrase.text slop [{slop}] is not served (0)")
        spec = spec["query"]
    if not isinstance(spec, str):
        raise ValueError("match_phrase.text query must be a string")
    terms = _analyzer.analyze([spec])[0].tolist()
    if len(terms) > LEX_MAX_QUERY:
        raise ValueError(f"a phrase holds at most {LEX_MAX_QUERY} word pieces, got {len(terms)}")
    return terms


def text_clauses(clause) -> Tuple[List[List[int]], np.ndarray, int]:
    """An OpenSearch clause on the analysed ``text`` field -> (clauses, roles uint8, min_should) of ONE clause query
    (``LexicalIndex.search_phrase`` / ``match_phrase``): a list of clauses, each a list of term ids, one role per clause.
    Served: everything ``text_query`` serves (every term occurrence a clause of its own, its role kept), and
      ``{"match_phrase": {"text": "..." | {"query": "...", "slop": 0}}}``: one MUST clause of the word pieces in order, as a
        leaf and as a member of ``bool.must`` / ``should`` / ``filter`` / ``must_not`` beside ``match`` members.  A phrase
        member is ONE clause, so ``minimum_should_match`` above 1 accepts phrase members under ``should``.  A phrase that
        analyses to nothing matches nothing.
    Needs ``configure_analyzer(..., positions=True)``.  Anything else raises ValueError: a non-zero ``slop``, another field,
    an ``analyzer`` option, more than 64 word pieces in all."""
    if not has_phrase(clause):
        terms, roles, ms = text_query(clause)
        return [[int(t)] for t in terms], roles, ms
    if not isinstance(clause, dict) or len(clause) != 1:
        raise ValueError("a text clause is {'match': ...}, {'match_phrase': ...} or a {'bool': {...}} of such clauses")
    (kind, spec), = clause.items()
    clauses: List[List[int]] = []
    roles: List[int] = []
    ms = 0
    if kind == "match_phrase":
        t = _phrase_parts(spec)
        clauses, roles = ([t], [LEX_MUST]) if t else ([], [])
    elif kind == "bool" and isinstance(spec, dict) and set(spec) == {"must"} and len(_as_list(spec["must"])) == 1 and \
            isinstance(_as_list(spec["must"])[0], dict) and "bool" not in _as_list(spec["must"])[0]:
        return text_clauses(_as_list(spec["must"])[0])      # a bool that is one must LEAF is that leaf; a nested bool stays refused
    elif kind == "bool" and isinstance(spec, dict) and set(spec) <= {"must", "should", "filter", "must_not", "minimum_should_match"}:
        n_should = wide_should = 0
        nothing = False
        for key, role in (("must", LEX_MUST), ("filter", LEX_FILTER), ("should", LEX_SHOULD), ("must_not", LEX_MUST_NOT)):
            for member in _as_list(spec.get(key, [])):
                if isinstance(member, dict) and set(member) == {"match_phrase"}:
                    t = _phrase_parts(member["match_phrase"])
                    n_should += role == LEX_SHOULD
                    if t:
                        clauses.append(t)
                        roles.append(role)
                    elif role in (LEX_MUST, LEX_FILTER):          # a required phrase without a word piece holds nowhere
                        nothing = True
                    continue
                if not isinstance(member, dict) or set(member) != {"match"}:
                    raise ValueError(f"bool.{key}: every member must be a match or match_phrase clause on [text]")
                t, operator, msm = _match_parts(member["match"])
                if msm is not None:
                    raise ValueError(f"bool.{key}: a member match with minimum_should_match is not served")
                if role in (LEX_MUST, LEX_FILTER) and len(t) > 1 and operator != "and":
                    raise ValueError(f"bool.{key}: a multi-term match needs operator [and]")
                if role == LEX_SHOULD and len(t) > 1 and operator != "or":
                    raise ValueError("bool.should: a multi-term match with operator [and] is not served")
                if role == LEX_SHOULD:
                    n_should += 1
                    wide_should += len(t) > 1
                clauses += [[int(x)] for x in t]
                roles += [role] * len(t)
        ms = _min_should(spec["minimum_should_match"], n_should) if "minimum_should_match" in spec else 0
        if ms > 1 and wide_should:
            raise ValueError("bool: minimum_should_match above 1 needs single-term or phrase should members")
        if not any(r != LEX_MUST_NOT for r in roles) and not nothing:
            raise ValueError("bool: at least one must, filter or should clause is needed")
        if nothing:
            clauses, roles, ms = [], [], 0
    else:
        raise ValueError(f"text clause [{kind}] is not served (match or match_phrase on [text], bool of such clauses)")
    n = sum(len(c) for c in clauses)
    if n > LEX_MAX_QUERY:
        raise ValueError(f"a text query holds at most {LEX_MAX_QUERY} term occurrences, got {n}")
    return clauses, np.asarray(roles, np.uint8), min(int(ms), LEX_MAX_QUERY + 1)


def text_match_rows(idx: "_GpuNamedIndex", clause) -> np.ndarray:
    """Vector ids (int64, ascending) of the live documents whose text matches ``clause`` (``text_query``; with a
    ``match_phrase`` in it ``text_clauses``): the match set of the index's ``LexicalIndex``, whose ids are the vector ids.
    Caller holds ``idx.lock``."""
    if has_phrase(clause):
        clauses, roles, ms = text_clauses(clause)
        if ms > LEX_MAX_QUERY:
            return np.empty(0, np.int64)
        counts, ids = push_text(idx).match_phrase([clauses], [roles], [ms])
        return np.ascontiguousarray(ids[0, :int(counts[0])], dtype=np.int64)
    terms, roles, ms = text_query(clause)
    if ms > LEX_MAX_QUERY:                                # above every count of SHOULD occurrences: nothing matches
        return np.empty(0, np.int64)
    counts, ids = push_text(idx).match([terms], [roles], [ms])
    return np.ascontiguousarray(ids[0, :int(counts[0])], dtype=np.int64)


def _text_changed(idx, row: int, gone: bool = False) -> None:
    """Row ``row`` got another text or left the index (caller holds ``idx.lock``): the next ``push_text`` sends or deletes
    it.  An index without a lexical side records nothing: its first push sends every live row."""
    if getattr(idx, "lex", None) is not None:
        (idx.lex_gone if gone else idx.lex_stale).add(row)


def push_text(idx: "_GpuNamedIndex"):
    """Bring the index's ``LexicalIndex`` (ids = vector ids) in step with the docstore and return it: every live row on the
    first call (also after ``load_index``: the lexical index is not saved, it is rebuilt from the docstore), afterwards the
    rows added since, the rows an overwrite rewrote and the rows deleted.  Caller holds ``idx.lock``."""
    if _analyzer is None:
        raise RuntimeError("no analyzer configured: call configure_analyzer(WordPieceTokenizer(vocab))")
    if getattr(idx, "lex", None) is None or getattr(idx, "lex_analyzer", None) is not _analyzer:
        from .engine import LexicalIndex
        idx.lex = LexicalIndex(idx.vectors.ctx, _analyzer.n_terms)
        idx.lex_analyzer, idx.lex_sent_upto, idx.lex_stale, idx.lex_gone = _analyzer, 0, set(), set()
    if idx.lex_gone:
        idx.lex.delete(np.asarray(sorted(idx.lex_gone), np.int64))
    upto = idx.lex_sent_upto
    rows = sorted({r for r in idx.lex_stale if r < upto} | set(range(upto, len(idx.sources))))
    rows = [r for r in rows if idx.sources[r] is not None]
    for lo in range(0, len(rows), 256):
        part = rows[lo:lo + 256]
        bags = _analyzer.analyze([str(idx.sources[r].get("text") or "") for r in part])
        if _analyzer.positions:
            idx.lex.put(np.asarray(part, np.int64), bags, ordered=True)
        else:
            idx.lex.put(np.asarray(part, np.int64), bags)
    idx.lex_sent_upto, idx.lex_stale, idx.lex_gone = len(idx.sources), set(), set()
    return idx.lex


def _check_hybrid_fusion(fusion, k: int) -> Tuple[int, int, Optional[List[float]]]:
    """``fusion={"rank_constant": 60, "window": n, "weights": [w_knn, w_text]}`` of a hybrid text + vector request ->
    (rank_constant, depth, weights or None), by the rules of ``_check_fusion`` for two lists (rrf only)."""
    if fusion is not None and isinstance(fusion, dict) and fusion.get("method", "rrf") != "rrf":
        raise ValueError("hybrid text + vector fusion is rank fusion (rrf) only")
    _method, c, depth, w = _check_fusion(fusion, k, 2)
    return c, depth, w


def _key_changed(idx, row: int, doc_id) -> None:
    """An overwrite gave stored row ``row`` the document ``doc_id`` (caller holds ``idx.lock``, before ``sources`` is
    rewritten): if that is another document, the row's group key is sent again by the next collapsed search."""
    old = idx.sources[row]
    if old is None or str(old["doc_id"]) != str(doc_id):
        if getattr(idx, "keys_stale", None) is None:
            idx.keys_stale = set()
        idx.keys_stale.add(row)


def push_keys(idx: "_GpuNamedIndex") -> int:
    """Send the group keys (one int per ``doc_id``) of the rows the device does not have them for yet: every live row on
    the first call (also after ``load_index``: keys are not part of a saved index), afterwards the rows added since and
    the rows whose ``doc_id`` an overwrite changed.  Caller holds ``idx.lock``.  -> rows sent."""
    table = getattr(idx, "key_of_doc", None)
    if table is None:
        table = idx.key_of_doc = {}
    upto = getattr(idx, "keys_sent_upto", 0)
    stale = getattr(idx, "keys_stale", None) or set()
    rows = sorted({r for r in stale if r < upto} | set(range(upto, len(idx.sources))))
    rows = [r for r in rows if idx.sources[r] is not None]
    if rows:
        keys = [table.setdefault(str(idx.sources[r]["doc_id"]), len(table)) for r in rows]
        idx.vectors.set_keys(np.asarray(rows, np.int64), np.asarray(keys, np.int64))
    idx.keys_sent_upto = len(idx.sources)
    idx.keys_stale = set()
    return len(rows)


def collapsed_search(idx: "_GpuNamedIndex", q: np.ndarray, k: int):
    """``collapse`` on ``doc_id``: the k best documents and each document's best chunk -> (cos, ids) as ``search``."""
    with idx.lock:
        push_keys(idx)
        cos, ids, _keys = idx.vectors.search_collapsed(q, k)
    return cos, ids


def _check_collapse(collapse) -> None:
    if not isinstance(collapse, dict) or set(collapse) != {"field"} or collapse["field"] != "doc_id":
        raise ValueError("collapse is served as {'field': 'doc_id'} only (no inner_hits, no other field)")


MMR_MAX_CANDIDATES = 256                                 # sqe_index_search_mmr: k <= n_cand <= 256 (include/sqe.h)


def _check_mmr(mmr, k: int) -> Tuple[float, int]:
    """``mmr={"lambda": 0.5, "candidates": 64}`` -> (lambda, candidates); both keys are optional (0.5; 0 = automatic)."""
    if not isinstance(mmr, dict) or not set(mmr) <= {"lambda", "candidates"}:
        raise ValueError("mmr is served as {'lambda': weight in [0, 1], 'candidates': depth} only")
    lam, n = mmr.get("lambda", 0.5), mmr.get("candidates", 0)
    if isinstance(lam, bool) or not isinstance(lam, numbers.Real) or not 0.0 <= float(lam) <= 1.0:      # a NaN fails too
        raise ValueError(f"mmr lambda must be a number in [0, 1], got {lam!r}")
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or (n != 0 and not k <= n <= MMR_MAX_CANDIDATES):
        raise ValueError(f"mmr candidates must be 0 (automatic) or in [k, {MMR_MAX_CANDIDATES}], got {n!r} at k = {k}")
    if not 1 <= k <= MMR_MAX_CANDIDATES:
        raise ValueError(f"mmr: k must be in [1, {MMR_MAX_CANDIDATES}], got {k}")
    return float(lam), int(n)


RERANK_MAX = 256


def rerank_depth(k: int, candidates: Optional[int] = None) -> int:
    """Hits a reranked search retrieves: ``candidates``, by default min(256, max(32, 4 k)); k <= n <= 256."""
    n = min(RERANK_MAX, max(32, 4 * k)) if candidates is None else candidates
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not k <= n <= RERANK_MAX:
        raise ValueError(f"rerank: candidates must be an integer with k <= candidates <= {RERANK_MAX}")
    return int(n)


def _check_rerank(rerank, k: int) -> Tuple[str, int]:
    if not isinstance(rerank, dict) or not isinstance(rerank.get("query_text"), str) or set(rerank) - {"query_text", "candidates"}:
        raise ValueError('rerank takes {"query_text": str, "candidates": n}')
    if _reranker is None:
        raise ValueError("rerank: no reranker configured: call configure_reranker(Reranker(encoder, tokenizer))")
    return rerank["query_text"], rerank_depth(k, rerank.get("candidates"))


def rerank_order(scores, k: int) -> List[int]:
    """Positions of the k best scores, best first; equal scores keep their retrieval order."""
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")[:k].tolist()


def mmr_depth(k: int, candidates: int) -> int:
    """The depth an MMR request of k hits searches: ``candidates``, or the automatic min(256, max(32, 4 k)) for 0
    (sqe_index_search_mmr's rule).  It belongs to the request: a batch never changes it."""
    return int(candidates) if candidates else min(MMR_MAX_CANDIDATES, max(32, 4 * k))


FUSE_MAX_DEPTH = 256                                     # sqe_index_search_fused: k <= n <= 256, at most 32 sub-queries of a
FUSE_MAX_QUERIES = 32                                    # logical query, sub-queries x depth <= 2048 (include/sqe.h)
FUSE_MAX_ENTRIES = 2048


def fuse_depth(k: int, window: int, method: str) -> int:
    """The depth a fused request of k hits searches every sub-query at: ``window``, or for 0 the automatic k ("max") /
    min(256, max(32, 4 k)) ("rrf") of sqe_index_search_fused."""
    return int(window) if window else (k if method == "max" else min(FUSE_MAX_DEPTH, max(32, 4 * k)))


def _check_fusion(fusion, k: int, m: int) -> Tuple[str, int, int, Optional[List[float]]]:
    """``fusion={"method": "rrf" | "max", "rank_constant": 60, "window": n, "weights": [...]}`` for m sub-queries and k hits
    -> (method, rank_constant, depth, weights or None); every key is optional (rrf, 60, automatic depth, all 1)."""
    fusion = {} if fusion is None else fusion
    if not isinstance(fusion, dict) or not set(fusion) <= {"method", "rank_constant", "window", "weights"}:
        raise ValueError("fusion is served as {'method': 'rrf' | 'max', 'rank_constant': c, 'window': depth, 'weights': [...]} only")
    method, c, n, w = fusion.get("method", "rrf"), fusion.get("rank_constant", 60), fusion.get("window", 0), fusion.get("weights")
    if method not in ("rrf", "max"):
        raise ValueError(f"fusion method must be 'rrf' or 'max', got {method!r}")
    if not 1 <= m <= FUSE_MAX_QUERIES:
        raise ValueError(f"fusion takes 1 to {FUSE_MAX_QUERIES} sub-queries, got {m}")
    if not 1 <= k <= FUSE_MAX_DEPTH:
        raise ValueError(f"fusion: k must be in [1, {FUSE_MAX_DEPTH}], got {k}")
    if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 1 <= c <= 10000:
        raise ValueError(f"fusion rank_constant must be an integer in [1, 10000], got {c!r}")
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or (n != 0 and not k <= n <= FUSE_MAX_DEPTH):
        raise ValueError(f"fusion window must be 0 (automatic) or in [k, {FUSE_MAX_DEPTH}], got {n!r} at k = {k}")
    depth = fuse_depth(k, int(n), method)
    if m * depth > FUSE_MAX_ENTRIES:
        raise ValueError(f"fusion: sub-queries x window must not exceed {FUSE_MAX_ENTRIES}, got {m} x {depth}")
    if w is not None:
        if method == "max":
            raise ValueError("fusion weights are not served with method 'max'")
        if not isinstance(w, (list, tuple)) or len(w) != m:
            raise ValueError(f"fusion weights must be a list of {m} numbers, one per sub-query")
        for v in w:
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 < float(np.float32(v)) <= 64.0:      # a NaN fails too
                raise ValueError(f"fusion weights must be numbers in (0, 64], got {v!r}")
        w = [float(v) for v in w]
    return method, int(c), depth, w


def _as_list(v) -> list:
    return v if isinstance(v, list) else [v]


def filter_rows(idx: "_GpuNamedIndex", clause: Dict) -> np.ndarray:
    """Vector ids (int64, ascending) of the live documents an OpenSearch filter clause selects.  Served: ``range`` (``gt`` /
    ``gte`` / ``lt`` / ``lte``), ``term``, ``terms`` and ``exists`` on a field declared with ``configure_fields`` (matched on the
    device, ``fields.match_rows``), ``term`` /
    ``terms`` on ``doc_id``, ``ids``, ``match`` on ``text`` (``text_query``: the match set of the lexical index, made on the
    device), ``match_phrase`` on ``text`` (``text_clauses``; needs ``configure_analyzer(..., positions=True)``) and ``bool``
    over those (``filter`` / ``must`` = AND, ``should`` = OR, ``must_not`` = NOT; as in OpenSearch,
    ``should`` only restricts when there is no ``filter`` / ``must`` or when ``minimum_should_match`` is 1).  Anything else
    raises ValueError.  Caller holds ``idx.lock``."""
    if not isinstance(clause, dict) or len(clause) != 1:
        raise ValueError("a filter clause is one of {'term': {'doc_id': ...}}, {'terms': {'doc_id': [...]}}, "
                         "{'ids': {'values': [...]}}, {'match': {'text': ...}}, {'match_phrase': {'text': ...}}, {'bool': {...}}")
    (kind, spec), = clause.items()
    if kind in ("match", "match_phrase"):
        return text_match_rows(idx, clause)
    schema = F.schema_of(idx)
    if schema is not None:
        push_fields(idx)                              # first: the keyword dictionaries learn from the documents they send
    leaf = schema.leaf(clause) if schema is not None else None
    if leaf is not None:                              # range / term / terms / exists on a configured field: matched on the device
        return F.match_rows(idx, [leaf])
    if kind in ("term", "terms") and isinstance(spec, dict) and set(spec) == {"doc_id"}:
        v = spec["doc_id"]
        if kind == "term":
            wanted = [v["value"] if isinstance(v, dict) else v]
        elif isinstance(v, list):
            wanted = v
        else:
            raise ValueError("terms: doc_id takes a list of values")
        docs = _rows_of_doc(idx)
        rows = set()
        for w in wanted:
            rows |= docs.get(str(w), set())
        return np.array(sorted(rows), np.int64)
    if kind == "ids" and isinstance(spec, dict) and set(spec) <= {"values"}:
        rows = {idx.row_of_id[str(v)] for v in spec.get("values", []) if str(v) in idx.row_of_id}
        return np.array(sorted(rows), np.int64)
    if kind == "bool" and isinstance(spec, dict) and set(spec) <= {"filter", "must", "should", "must_not", "minimum_should_match"}:
        msm = spec.get("minimum_should_match", None)
        if msm not in (None, 0, 1, "0", "1"):
            raise ValueError(f"bool: minimum_should_match [{msm}] is not served (0 or 1)")
        required = [filter_rows(idx, c) for key in ("filter", "must") for c in _as_list(spec.get(key, []))]
        should = [filter_rows(idx, c) for c in _as_list(spec.get("should", []))]
        if should and (not required or str(msm) == "1"):
            union = should[0]
            for r in should[1:]:
                union = np.union1d(union, r)
            required.append(union)
        if required:
            rows = required[0]
            for r in required[1:]:
                rows = np.intersect1d(rows, r, assume_unique=True)
        else:
            rows = idx.vectors.ids()                  # only must_not: everything live
        for c in _as_list(spec.get("must_not", [])):
            rows = np.setdiff1d(rows, filter_rows(idx, c), assume_unique=True)
        return rows.astype(np.int64)
    raise ValueError(f"filter clause [{kind}] is not served (term / terms on doc_id, ids, match / match_phrase on text, bool"
                     + (")" if schema is None else f"; range / term / terms / exists on the configured fields {sorted(schema.slot)})"))


def field_predicate(idx: "_GpuNamedIndex", clause) -> Optional[List[tuple]]:
    """The device predicate of a filter that is a pure conjunction of leaves on configured fields (``FieldSchema.conjunction``:
    one leaf, or a ``bool`` of ``filter`` / ``must`` / ``must_not`` leaves), else None.  Such a filter is answered by
    ``VectorIndex.search_where``: no id list is made on the host.  The values not yet on the device are sent first
    (``push_fields``).  Caller holds ``idx.lock``."""
    schema = F.schema_of(idx)
    if schema is None or clause is None or not hasattr(idx.vectors, "search_where"):
        return None
    push_fields(idx)                                  # first: the keyword dictionaries learn from the documents they send
    return schema.conjunction(clause)


def field_predicates(idx: "_GpuNamedIndex", filters) -> Optional[Tuple[List[List[tuple]], np.ndarray]]:
    """-> (preds, pred_of_query) when EVERY filter of a batch is such a conjunction (equal clauses share a predicate), else
    None.  More distinct predicates than one call takes (64): None.  Caller holds ``idx.lock``."""
    import json
    if F.schema_of(idx) is None:
        return None
    preds: List[List[tuple]] = []
    pred_of: Dict[str, int] = {}
    poq = np.zeros(len(filters), np.int32)
    n_set = 0
    for b, clause in enumerate(filters):
        if clause is None:
            return None
        key = json.dumps(clause, sort_keys=True)
        if key not in pred_of:
            pred = field_predicate(idx, clause)
            if pred is None:
                return None
            pred_of[key] = len(preds)
            preds.append(pred)
            n_set += sum(len(cl[2]) for cl in pred if cl[1] == "in")
        poq[b] = pred_of[key]
    if not preds or len(preds) > F.FIELD_MAX_PREDS or n_set > F.FIELD_MAX_SET:
        return None
    return preds, poq


def row_set_of(idx: "_GpuNamedIndex", filter: Optional[Dict]) -> Tuple[List[tuple], Optional[np.ndarray]]:
    """-> (pred, allow): the row set of the documents ``filter`` selects, as the ``VectorIndex`` calls that take ``pred`` and
    ``filter_ids`` want it.  None: the empty predicate and no list (every live document).  A filter that is a pure conjunction
    of field leaves becomes the device predicate (``field_predicate``), with no list; anything else ``filter_rows`` serves --
    text ``match`` / ``match_phrase`` clauses and a ``bool`` with only ``must_not`` included -- becomes the empty predicate AND
    the allow-list of its rows.  ValueError for what is not served.  Caller holds ``idx.lock``."""
    pred = [] if filter is None else field_predicate(idx, filter)
    if pred is not None:
        return pred, None
    return [], filter_rows(idx, filter)


def aggregate_filtered(idx: "_GpuNamedIndex", aggs: Dict[str, Dict], filter: Optional[Dict] = None) -> Tuple[int, Dict[str, Dict]]:
    """Named OpenSearch aggregations on configured fields (``FieldSchema.aggregation``) over the live documents ``filter``
    selects (None: all of them; ``row_set_of``) -> (documents selected, {name: answer}), computed on the device from the field
    columns (``VectorIndex.aggregate_fields``).  ValueError for what is not served."""
    with idx.lock:
        pred, allow = row_set_of(idx, filter)
        return F.aggregate_rows(idx, aggs, pred, allow)


SORT_MAX_WINDOW = 256      # from_ + k of a sorted search (sqe_index_sort_fields: k <= 256); deeper pages take search_after


def sorted_filtered(idx: "_GpuNamedIndex", sort, k: int, filter: Optional[Dict] = None, search_after=None,
                    from_: int = 0) -> Tuple[int, List[Tuple[int, Dict, list]]]:
    """The ``k`` first live documents ``filter`` selects (None: all of them) in the order of the OpenSearch ``sort`` on
    configured fields (``FieldSchema.sort_spec``), after skipping ``from_`` and after the cursor ``search_after`` (a hit's sort
    array) when given -> (documents selected, whatever the cursor and the window; [(vector id, _source, sort array ``[v_0, ...,
    id]``)]), ranked on the device from the field columns (``VectorIndex.sort_fields``) over the row set of the filter
    (``row_set_of``).  ``from_ + k <= 256``: the first ``from_`` rows are dropped here.  The stored vector
    is not fetched.  ValueError for what is not served."""
    for what, v, lo in (("k", k, 1), ("from", from_, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"sorted search: {what} [{v}] is not served (an integer >= {lo})")
    if from_ + k > SORT_MAX_WINDOW:
        raise ValueError(f"sorted search: from + size = {from_ + k} is beyond the window of {SORT_MAX_WINDOW} rows: page with search_after")
    with idx.lock:
        pred, allow = row_set_of(idx, filter)
        total, ids, sorts = F.sort_rows(idx, sort, int(from_ + k), pred, allow, search_after)
        return total, [(int(row), dict(idx.sources[int(row)]), sv) for row, sv in zip(ids[from_:].tolist(), sorts[from_:])]


def exclusion_rows(idx: "_GpuNamedIndex", clause) -> Optional[np.ndarray]:
    """Vector ids (int64, ascending) a clause DENIES, when it is a ``bool`` whose only key is ``must_not``: the union of its
    ``must_not`` sub-clauses, each resolved by ``filter_rows`` (an unserved one raises ValueError).  Such a clause selects
    everything else, which ``VectorIndex.search_excluding`` answers at the cost of a plain search instead of an allow-list
    of nearly the whole index.  Any other clause: None.  Caller holds ``idx.lock``."""
    if not isinstance(clause, dict) or set(clause) != {"bool"}:
        return None
    spec = clause["bool"]
    if not isinstance(spec, dict) or set(spec) != {"must_not"}:
        return None
    rows = np.empty(0, np.int64)
    for c in _as_list(spec["must_not"]):
        rows = np.union1d(rows, filter_rows(idx, c))
    return rows.astype(np.int64)


def _can_exclude(idx: "_GpuNamedIndex") -> bool:
    """A vectors object without ``search_excluding`` (a stand-in index) keeps such clauses on the allow-list route: with
    ``certify`` = 1 both routes return the same bits."""
    return hasattr(idx.vectors, "search_excluding")


def resolve_each(idx: "_GpuNamedIndex", filters) -> Tuple[List[np.ndarray], np.ndarray]:
    """-> (lists, list_of_query) of one filter clause or None per query: the allow-list of every distinct clause (equal
    ``json.dumps(..., sort_keys=True)`` share one) and, per query, its list (-1 for None).  An unserved clause raises
    ValueError.  Caller holds ``idx.lock``."""
    import json
    lists: List[np.ndarray] = []
    list_of: Dict[str, int] = {}
    loq = np.full(len(filters), -1, np.int32)
    for b, clause in enumerate(filters):
        if clause is None:
            continue
        key = json.dumps(clause, sort_keys=True)
        if key not in list_of:
            list_of[key] = len(lists)
            lists.append(filter_rows(idx, clause))
        loq[b] = list_of[key]
    return lists, loq


def resolve_routes(idx: "_GpuNamedIndex", filters) -> Tuple[List[np.ndarray], np.ndarray, List[np.ndarray], np.ndarray]:
    """-> (lists, list_of_query, deny, deny_of_query) of one filter clause or None per query.  A clause ``exclusion_rows``
    serves goes to the deny-lists (equal clauses share one; -1 in ``deny_of_query`` for every other query), the rest is
    what ``resolve_each`` returns.  An unserved clause raises ValueError.  Caller holds ``idx.lock``."""
    import json
    rest = list(filters)
    deny: List[np.ndarray] = []
    deny_of: Dict[str, int] = {}
    doq = np.full(len(rest), -1, np.int32)
    if _can_exclude(idx):
        for b, clause in enumerate(rest):
            rows = None if clause is None else exclusion_rows(idx, clause)
            if rows is None:
                continue
            key = json.dumps(clause, sort_keys=True)
            if key not in deny_of:
                deny_of[key] = len(deny)
                deny.append(rows)
            doq[b] = deny_of[key]
            rest[b] = None
    lists, loq = resolve_each(idx, rest)
    return lists, loq, deny, doq


def search_resolved(idx: "_GpuNamedIndex", q: np.ndarray, k: int, lists, loq: np.ndarray, deny=None,
                    doq: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """-> (cos, ids) [B, k] of queries ``q`` for what ``resolve_each`` (or, with ``deny`` / ``doq``, ``resolve_routes``)
    returned: the queries with an allow-list in ONE per-query filtered call, those with a deny-list in ONE exclusion call,
    the others in one plain search, rows in request order."""
    if q.ndim == 1:
        q = q[None]
    if loq.shape[0] != q.shape[0]:
        raise ValueError(f"{loq.shape[0]} filters for {q.shape[0]} queries")
    cos = np.full((loq.shape[0], k), -np.inf, np.float32)
    ids = np.full((loq.shape[0], k), -1, np.int64)
    if doq is None:
        doq = np.full(loq.shape[0], -1, np.int32)
    plain, each, excl = np.nonzero((loq < 0) & (doq < 0))[0], np.nonzero(loq >= 0)[0], np.nonzero(doq >= 0)[0]
    if excl.size:
        cos[excl], ids[excl] = idx.vectors.search_excluding(np.ascontiguousarray(q[excl]), k, deny, doq[excl])
    if plain.size:
        cos[plain], ids[plain] = idx.vectors.search(np.ascontiguousarray(q[plain]), k)
    if each.size:
        cos[each], ids[each] = idx.vectors.search_filtered_each(np.ascontiguousarray(q[each]), k, lists, loq[each])
    return cos, ids


def _query_ids(idx: "_GpuNamedIndex", body: Dict) -> List[str]:
    """``_id`` s a delete_by_query body selects: ``term`` / ``terms`` on ``doc_id``, or ``ids``; anything else raises."""
    q = (body or {}).get("query")
    if not isinstance(q, dict) or len(q) != 1:
        raise ValueError("delete_by_query needs one of {'term': {'doc_id': ...}}, {'terms': {'doc_id': [...]}}, {'ids': {'values': [...]}}")
    (kind, spec), = q.items()
    if kind == "ids":
        return [str(v) for v in spec.get("values", [])]
    if kind in ("term", "terms"):
        rows = filter_rows(idx, q)
        id_of_row = {row: os_id for os_id, row in idx.row_of_id.items()}
        return [id_of_row[int(row)] for row in rows if int(row) in id_of_row]
    raise ValueError(f"delete_by_query: query [{kind}] is not served (term / terms on doc_id, ids)")


def delete_by_query(idx: "_GpuNamedIndex", body: Dict) -> int:
    """Delete what ``_query_ids`` selects; -> number of documents deleted."""
    with idx.lock:
        os_ids = _query_ids(idx, body)
    return sum(delete_documents(idx, os_ids))


def _commit_documents(idx: "_GpuNamedIndex", embeddings: np.ndarray, docs: List[Dict[str, str]], id_of) -> int:
    """The "index" op of the bulk call (main.py:318-338): insert, or overwrite an existing ``_id``.

    Order matters: (1) validate and convert the vectors, (2) plan against the docstore WITHOUT touching it,
    (3) run the device add / update, (4) only then commit ``sources`` / ``row_of_id``.  A failing device call
    (wrong dimension, allocation failure) therefore leaves host docstore and vector rows in step: every later
    add still lands at vector row == sources row."""
    vecs = np.ascontiguousarray(embeddings, dtype=np.float32)
    if vecs.ndim != 2 or vecs.shape[1] != idx.vectors.dim:
        raise ValueError(f"embeddings must be [n, {idx.vectors.dim}], got {vecs.shape}")
    n = min(len(docs), vecs.shape[0])                 # zip() semantics of main.py:318
    with idx.lock:
        schema = F.schema_of(idx)
        # configured fields: every value parses before anything is touched (FieldValueError refuses the call)
        extras = [schema.document_fields(docs[i]) for i in range(n)] if schema is not None else None
        doc_rows = _rows_of_doc(idx)
        base = len(idx.sources)
        new_src: List[Dict[str, str]] = []
        new_ids: Dict[str, int] = {}                  # _id -> position in this call's insert list
        new_from: List[int] = []                      # embedding row of each insert (the LAST writer of its _id)
        upd: Dict[int, tuple] = {}                    # stored row -> (source, embedding row); last writer wins
        for i in range(n):
            os_id = id_of(i, docs[i])
            src = {"doc_id": docs[i]["doc_id"], "text": docs[i]["text"]}
            if extras is not None:
                src.update(extras[i])
            row = idx.row_of_id.get(os_id)
            if row is not None:
                upd[row] = (src, i)
            elif os_id in new_ids:                    # same _id twice in one call: the later document replaces the earlier
                new_src[new_ids[os_id]], new_from[new_ids[os_id]] = src, i
            else:
                new_ids[os_id] = len(new_src)
                new_src.append(src)
                new_from.append(i)
        # normalisation x / (||x|| + 1e-9) (main.py:315-316) happens on the GPU
        if new_from:
            contiguous = new_from == list(range(new_from[0], new_from[0] + len(new_from)))
            idx.vectors.add(vecs[new_from[0]:new_from[0] + len(new_from)] if contiguous else vecs[new_from])
        try:
            if upd:
                rows = sorted(upd)
                idx.vectors.update(np.array(rows, np.int64), vecs[[upd[r][1] for r in rows]])
        finally:
            # the appended vector rows exist whatever the update did: their documents must exist too
            for os_id, pos in new_ids.items():
                idx.row_of_id[os_id] = base + pos
            idx.sources.extend(new_src)
            for pos, src in enumerate(new_src):
                _doc_add(doc_rows, src["doc_id"], base + pos)
        for row, (src, _i) in upd.items():
            _key_changed(idx, row, src["doc_id"])
            _text_changed(idx, row)
            F.field_changed(idx, row)
            if idx.sources[row] is not None:
                _doc_remove(doc_rows, idx.sources[row]["doc_id"], row)
            idx.sources[row] = src
            _doc_add(doc_rows, src["doc_id"], row)
    return n


def radial_min_cos(min_score: Optional[float] = None, max_distance: Optional[float] = None) -> np.float32:
    """The cosine floor of a radial k-NN query.  Hits score ``1 / (2 - cos)``, so ``min_score = s`` is
    ``cos >= 2 - 1/s`` (``s <= 0``: every row); ``max_distance = d`` bounds the cosine distance ``1 - cos <= d``, i.e.
    ``cos >= 1 - d``.  Rounded to fp32 once: a row whose score lies within an fp32 ulp of the floor may fall either side."""
    if (min_score is None) == (max_distance is None):
        raise ValueError("exactly one of min_score and max_distance")
    if min_score is not None:
        s = float(min_score)
        if s != s:
            raise ValueError("min_score is NaN")
        return np.float32(-np.inf) if s <= 0.0 else np.float32(2.0 - 1.0 / s)
    d = float(max_distance)
    if d != d:
        raise ValueError("max_distance is NaN")
    return np.float32(1.0 - d)


class OpenSearchIndexer:
    """Drop-in for the reference class of the same name (main.py:291-373)."""

    def __init__(self, client: GpuSearchClient, index_name: str):
        self.client = client
        self.index_name = index_name

    def has_any_data(self) -> bool:
        if not self.client:
            return False
        try:
            resp = self.client.count(index=self.index_name)
            return resp["count"] > 0
        except Exception:
            return False

    def add_embeddings(self, embeddings: np.ndarray, docs: List[Dict[str, str]]):
        if not self.client or embeddings.size == 0:
            print("[OpenSearchIndexer] No embeddings or no OpenSearch client.")
            return
        try:
            idx = self.client.index(self.index_name)
            n = _commit_documents(idx, embeddings, docs, lambda i, d: f"{d['doc_id']}_{i}")   # _id rule of main.py:325
            print(f"[OpenSearchIndexer] Inserted {n} docs, errors=[]")
        except FieldValueError:
            raise                                     # a configured field's value does not parse: nothing was committed
        except Exception as e:
            print(f"[OpenSearchIndexer] Bulk indexing error: {e}")

    def search(self, query_emb: np.ndarray, k: int = 3, filter: Optional[Dict] = None, min_score: Optional[float] = None,
               max_distance: Optional[float] = None, collapse: Optional[Dict] = None,
               mmr: Optional[Dict] = None, exclude_ids: Optional[List[str]] = None,
               rerank: Optional[Dict] = None) -> List[Tuple[Dict[str, str], float]]:
        """``filter``: an OpenSearch filter clause (``filter_rows``); the k best among the documents it selects.  A ``bool``
        with only ``must_not`` is answered by the exclusion search (``exclusion_rows``): same hits, the cost of a plain search.
        ``exclude_ids``: OpenSearch ``_id`` s to leave out (hits already shown, the document being read), the direct form of
        the same search; unknown ids are skipped.
        ``min_score`` / ``max_distance``: radial search, the at most k best hits at or above the floor (``radial_min_cos``).
        ``collapse={"field": "doc_id"}``: one hit per document, each the document's best chunk (``collapsed_search``).
        ``mmr={"lambda": 0.5, "candidates": 64}``: maximal marginal relevance, the greedy choice of k hits among the best
        ``candidates`` (0 or absent: automatic) that weighs a hit's cosine (``lambda``) against its similarity to the hits
        already chosen (1 - ``lambda``); hits come in selection order, ``_score`` is the hit's own (``VectorIndex.search_mmr``).
        ``rerank={"query_text": str, "candidates": n}``: the n best hits of whichever search the other arguments select
        (``rerank_depth``) are scored against ``query_text`` by the configured cross-encoder (``Reranker``) on their ``text``
        field; the k best by that score come back, score descending, ties in retrieval order, the score the model's."""
        want = k
        if rerank is not None:
            query_text, k = _check_rerank(rerank, k)          # every route below retrieves the n candidates
        radial = min_score is not None or max_distance is not None
        if exclude_ids is not None and (radial or filter is not None or collapse is not None or mmr is not None):
            raise ValueError("exclude_ids is not served together with filter, min_score, max_distance, collapse or mmr")
        if mmr is not None:
            lam, n_cand = _check_mmr(mmr, k)
            if radial or filter is not None or collapse is not None:
                raise ValueError("mmr is not served together with filter, min_score, max_distance or collapse")
        if collapse is not None:
            _check_collapse(collapse)
            if radial or filter is not None:
                raise ValueError("collapse is not served together with filter, min_score or max_distance")
        if min_score is not None and max_distance is not None:
            raise ValueError("min_score and max_distance are exclusive")
        if radial and filter is not None:
            raise ValueError("radial search (min_score / max_distance) does not take a filter")
        if not self.client or query_emb.size == 0:
            return []
        try:
            idx = self.client.index(self.index_name)
            q = np.ascontiguousarray(query_emb, dtype=np.float32)
            if mmr is not None:
                cos, ids, _obj = idx.vectors.search_mmr(q[0:1], k, lam=lam, n_cand=n_cand)
            elif collapse is not None:
                cos, ids = collapsed_search(idx, q[0:1], k)
            elif radial:
                _, cos, ids = idx.vectors.range_search(q[0:1], radial_min_cos(min_score, max_distance), k)
            elif exclude_ids is not None:
                with idx.lock:
                    deny = np.array(sorted({idx.row_of_id[str(v)] for v in exclude_ids if str(v) in idx.row_of_id}), np.int64)
                cos, ids = idx.vectors.search_excluding(q[0:1], k, [deny])
            elif filter is None:
                cos, ids = idx.vectors.search(q[0:1], k)      # row 0 only (main.py:355)
            else:
                with idx.lock:
                    pred = field_predicate(idx, filter)
                    deny = exclusion_rows(idx, filter) if pred is None and _can_exclude(idx) else None
                    allow = filter_rows(idx, filter) if pred is None and deny is None else None
                if pred is not None:                  # a conjunction of field leaves: evaluated where the rows are
                    cos, ids = idx.vectors.search_where(q[0:1], k, pred)
                elif deny is not None:
                    cos, ids = idx.vectors.search_excluding(q[0:1], k, [deny])
                else:
                    cos, ids = idx.vectors.search(q[0:1], k, filter_ids=allow)
            results = self._vector_hits(idx, cos, ids)
            if rerank is not None and results:
                scores = _reranker.score(query_text, [str(src.get("text", "")) for src, _ in results])
                results = [(results[j][0], float(scores[j])) for j in rerank_order(scores, want)]
            print(f"[OpenSearchIndexer] Found {len(results)} relevant results.")
            return results
        except Exception as e:
            print(f"[OpenSearchIndexer] Search error: {e}")
            return []

    def _vector_hits(self, idx, cos, ids) -> List[Tuple[Dict[str, str], float]]:
        """Row 0 of a k-NN answer as ``search`` returns it: (_source with the stored vector, _score) per hit."""
        rows = [int(r) for r in ids[0] if r >= 0]
        embs = idx.vectors.get_rows(rows) if rows else np.zeros((0, idx.vectors.dim), np.float32)
        results = []
        for j, row in enumerate(rows):
            src = dict(idx.sources[row])
            src["embedding"] = embs[j].tolist()           # _source carries the stored vector
            # nmslib cosinesimil _score = 1 / (1 + (1 - cos))
            results.append((src, float(1.0 / (2.0 - float(cos[0, j])))))
        return results

    def search_within(self, query_emb: np.ndarray, k: int, filter: Dict, min_score: Optional[float] = None,
                      max_distance: Optional[float] = None, collapse: Optional[Dict] = None, mmr: Optional[Dict] = None,
                      rerank: Optional[Dict] = None) -> List[Tuple[Dict[str, str], float]]:
        """``filter`` together with ONE of radial search (``min_score`` / ``max_distance``), ``collapse`` or ``mmr``, each as
        ``search`` takes it: the documents the filter selects are the only ones that count, are walked or are candidates
        ("this user's chunks, one hit per document").  The filter is translated as ``search(filter=)`` translates it: a
        conjunction of leaves on configured fields is evaluated on the device (``field_predicate``), anything else becomes
        the allow-list of its rows (``filter_rows``).  With none of the three it is ``search(filter=)``.  Hits, ``_score`` and
        ``rerank`` as ``search``; exact, like the unrestricted searches (``VectorIndex.range_search`` / ``search_collapsed`` /
        ``search_mmr`` with ``pred`` / ``filter_ids``)."""
        if filter is None:
            raise ValueError("search_within needs a filter; without one it is search")
        radial = min_score is not None or max_distance is not None
        if min_score is not None and max_distance is not None:
            raise ValueError("min_score and max_distance are exclusive")
        if int(radial) + int(collapse is not None) + int(mmr is not None) > 1:
            raise ValueError("search_within takes at most one of min_score / max_distance, collapse and mmr")
        if not radial and collapse is None and mmr is None:
            return self.search(query_emb, k, filter=filter, rerank=rerank)
        want = k
        if rerank is not None:
            query_text, k = _check_rerank(rerank, k)
        if mmr is not None:
            lam, n_cand = _check_mmr(mmr, k)
        if collapse is not None:
            _check_collapse(collapse)
        if not self.client or query_emb.size == 0:
            return []
        try:
            idx = self.client.index(self.index_name)
            q = np.ascontiguousarray(query_emb, dtype=np.float32)
            with idx.lock:
                pred = field_predicate(idx, filter)
                allow = filter_rows(idx, filter) if pred is None else None
                if collapse is not None:
                    push_keys(idx)
                    cos, ids, _keys = idx.vectors.search_collapsed(q[0:1], k, pred=pred, filter_ids=allow)
            if mmr is not None:
                cos, ids, _obj = idx.vectors.search_mmr(q[0:1], k, lam=lam, n_cand=n_cand, pred=pred, filter_ids=allow)
            elif radial:
                _, cos, ids = idx.vectors.range_search(q[0:1], radial_min_cos(min_score, max_distance), k, pred=pred, filter_ids=allow)
            results = self._vector_hits(idx, cos, ids)
            if rerank is not None and results:
                scores = _reranker.score(query_text, [str(src.get("text", "")) for src, _ in results])
                results = [(results[j][0], float(scores[j])) for j in rerank_order(scores, want)]
            print(f"[OpenSearchIndexer] Found {len(results)} relevant results.")
            return results
        except Exception as e:
            print(f"[OpenSearchIndexer] Search error: {e}")
            return []

    def aggregate(self, aggs: Dict[str, Dict], filter: Optional[Dict] = None) -> Dict:
        """Facets of this index: ``aggs={"per_year": {"terms": {"field": "year", "size": 10}}, ...}`` over the documents
        ``filter`` selects -> {"selected", "aggregations"} (``GpuSearchClient.aggregate``).  What is not served raises ValueError."""
        return self.client.aggregate(self.index_name, aggs, filter)

    def search_sorted(self, sort, k: int = 10, filter: Optional[Dict] = None, search_after=None,
                      from_: int = 0) -> Tuple[int, List[Tuple[Dict, list]]]:
        """The ``k`` first documents of this index ``filter`` selects, in the order of the fields ``sort`` names
        (``sort=[{"published": "desc"}, "year"]``, ``FieldSchema.sort_spec``) -> (documents selected, [(_source, sort_values)]).
        A hit's ``sort_values`` is ``[v_0, ..., id]``: pass it back as ``search_after`` for the next page; ``from_ + k <= 256``
        (``GpuSearchClient.search_sorted``).  What is not served raises ValueError."""
        r = self.client.search_sorted(self.index_name, sort, k, filter, search_after, from_)
        return r["total"], [(src, sv) for _row, src, sv in r["hits"]]

    def search_multi(self, query_embs: np.ndarray, k: int = 3, fusion: Optional[Dict] = None) -> List[Tuple[Dict[str, str], float]]:
        """Several vectors for ONE question (the query and its rephrasings, the sentences of a long question), one ranked list
        back, shaped as ``search`` returns it.  ``fusion={"method": "rrf" | "max", "rank_constant": 60, "window": n,
        "weights": [...]}``: reciprocal rank fusion over every sub-query's best ``window`` hits (0 or absent: automatic), or
        the hit's best cosine over the sub-queries; one device call (``VectorIndex.search_fused``).  Hits come in fused order;
        the score is the ``_score`` of the hit's best cosine, as ``search`` maps it."""
        q = np.ascontiguousarray(query_embs, dtype=np.float32)
        if q.ndim == 1:
            q = q[None]
        method, c, depth, weights = _check_fusion(fusion, k, q.shape[0] if q.size else 1)
        if not self.client or q.size == 0:
            return []
        try:
            idx = self.client.index(self.index_name)
            with idx.lock:
                _fused, ids, cos = idx.vectors.search_fused(q, k, mode=method, weights=weights, depth=depth, rank_constant=c)
                rows = [int(r) for r in ids[0] if r >= 0]
                embs = idx.vectors.get_rows(rows) if rows else np.zeros((0, idx.vectors.dim), np.float32)
                results = []
                for j, row in enumerate(rows):
                    src = dict(idx.sources[row])
                    src["embedding"] = embs[j].tolist()
                    results.append((src, float(1.0 / (2.0 - float(cos[0, j])))))
            print(f"[OpenSearchIndexer] Found {len(results)} relevant results.")
            return results
        except Exception as e:
            print(f"[OpenSearchIndexer] Search error: {e}")
            return []

    def _text_hits(self, idx, rows: List[int], scores) -> List[Tuple[Dict[str, str], float]]:
        embs = idx.vectors.get_rows(rows) if rows else np.zeros((0, idx.vectors.dim), np.float32)
        out = []
        for j, row in enumerate(rows):
            src = dict(idx.sources[row])
            src["embedding"] = embs[j].tolist()
            out.append((src, float(scores[j])))
        return out

    def search_text(self, query_text, k: int = 3, operator: Optional[str] = None,
                    minimum_should_match=None) -> List[Tuple[Dict[str, str], float]]:
        """OpenSearch ``match`` on the ``text`` field: the k best documents by BM25 (``LexicalIndex``; the configured
        analyzer makes the terms of the query as it made those of the documents), shaped as ``search`` returns them; the
        score is the BM25 score.  ``operator="and"``: every term must be there; ``minimum_should_match``: that many of them
        (an integer or ``"p%"``).  ``query_text`` may also be a whole clause dict (``text_query``: ``match`` with its options,
        or a ``bool`` of ``match`` clauses); a document that only ``filter`` terms matched scores 0.0 and comes last."""
        boolean = isinstance(query_text, dict) or operator is not None or minimum_should_match is not None
        if not self.client or (not boolean and not str(query_text).strip()):
            return []
        try:
            idx = self.client.index(self.index_name)
            with idx.lock:
                if boolean:
                    clause = query_text
                    if not isinstance(clause, dict):
                        spec = {"query": str(query_text), "operator": operator or "or"}
                        if minimum_should_match is not None:
                            spec["minimum_should_match"] = minimum_should_match
                        clause = {"match": {"text": spec}}
                    phrase = has_phrase(clause)
                    terms, roles, ms = text_clauses(clause) if phrase else text_query(clause)
                    if ms > LEX_MAX_QUERY:                # above every count of SHOULD occurrences: nothing matches
                        return []
                    lex = push_text(idx)
                    score, ids = (lex.search_phrase if phrase else lex.search_bool)([terms], [roles], k, [ms])
                else:
                    lex = push_text(idx)
                    score, ids = lex.search([_analyzer.query(str(query_text))], k)
                rows = [int(r) for r in ids[0] if r >= 0]
                results = self._text_hits(idx, rows, score[0])
            print(f"[OpenSearchIndexer] Found {len(results)} relevant results.")
            return results
        except Exception as e:
            print(f"[OpenSearchIndexer] Search error: {e}")
            return []

    def count_text(self, clause) -> int:
        """OpenSearch ``_count`` with a text clause (``text_query``; a plain string stands for its ``match``): the exact
        number of live documents that match, counted on the device (``LexicalIndex.match`` with ``cap`` 0).  An unserved
        clause raises ValueError."""
        if not isinstance(clause, dict):
            clause = {"match": {"text": str(clause)}}
        phrase = has_phrase(clause)
        terms, roles, ms = text_clauses(clause) if phrase else text_query(clause)
        if ms > LEX_MAX_QUERY:
            return 0
        idx = self.client.index(self.index_name)
        with idx.lock:
            lex = push_text(idx)
            return int((lex.count_phrase if phrase else lex.count)([terms], [roles], [ms])[0])

    def search_hybrid(self, query_emb: np.ndarray, query_text: str, k: int = 3,
                      fusion: Optional[Dict] = None) -> List[Tuple[Dict[str, str], float]]:
        """Lexical plus vector: reciprocal rank fusion of the k-NN list of ``query_emb`` (row 0) and the BM25 list of
        ``query_text``, in one device call (``VectorIndex.search_hybrid``).  ``fusion={"rank_constant": 60, "window": n,
        "weights": [w_knn, w_text]}``, every key optional.  Hits come in fused order, shaped as ``search`` returns them; the
        score is the fused score."""
        c, depth, weights = _check_hybrid_fusion(fusion, k)
        if not self.client or query_emb.size == 0:
            return []
        try:
            idx = self.client.index(self.index_name)
            q = np.ascontiguousarray(query_emb, dtype=np.float32).reshape(-1, idx.vectors.dim)[0:1]
            with idx.lock:
                lex = push_text(idx)
                fused, ids, _cos, _bm25 = idx.vectors.search_hybrid(lex, q, [_analyzer.query(str(query_text))], k, weights=weights,
                                                                    depth=depth, rank_constant=c)
                rows = [int(r) for r in ids[0] if r >= 0]
                results = self._text_hits(idx, rows, fused[0])
            print(f"[OpenSearchIndexer] Found {len(results)} relevant results.")
            return results
        except Exception as e:
            print(f"[OpenSearchIndexer] Search error: {e}")
            return []

    # batched form of the same call (the GPU path's throughput is in B > 1)
    def search_batch(self, query_embs: np.ndarray, k: int = 3, filters=None) -> Tuple[np.ndarray, np.ndarray]:
        """``filters``: one OpenSearch filter clause (``filter_rows``) or None per query.  Every filtered query is answered
        over the documents its own clause selects, all of them in ONE device call (``VectorIndex.search_filtered_each``;
        equal clauses share a list); the queries whose clause only excludes (``exclusion_rows``) go in ONE exclusion call
        (``VectorIndex.search_excluding``); queries with None get the plain search.  Rows come back in request order."""
        idx = self.client.index(self.index_name)
        q = np.ascontiguousarray(query_embs, dtype=np.float32)
        if filters is None:
            return idx.vectors.search(q, k)
        filters = list(filters)
        if len(filters) != (1 if q.ndim == 1 else q.shape[0]):
            raise ValueError(f"{len(filters)} filters for {1 if q.ndim == 1 else q.shape[0]} queries")
        with idx.lock:                                    # every clause is resolved before any device call
            where = field_predicates(idx, filters)        # conjunctions of field leaves throughout: one search_where_each
            if where is None:
                lists, loq, deny, doq = resolve_routes(idx, filters)
        if where is not None:
            return idx.vectors.search_where_each(q, k, where[0], where[1])
        return search_resolved(idx, q, k, lists, loq, deny, doq)


# ------------------------------------------------------------------------------ cache
class SemanticLfuCache:
    """The Redis LIST ``query_cache_lfu`` of main.py:56-128 with the scan on the GPU.

    List position 0 is the newest entry (``lpush``, main.py:128).  The embeddings live in
    slots of a resident cache matrix; ``_order[i]`` is the slot of list position ``i``."""

    def __init__(self, ctx: Optional[Context] = None, max_items: int = REDIS_MAX_ITEMS,
                 threshold: float = CACHE_SIM_THRESHOLD, dim: int = EMBED_DIM):
        self.ctx = ctx or default_context()
        self.max_items, self.threshold, self.dim = max_items, threshold, dim
        self.matrix = CacheMatrix(self.ctx, max_items, dim)
        self._order: List[int] = []                    # list position -> slot
        self._entries: Dict[int, Dict] = {}            # slot -> {"response", "freq"}
        self._free = list(range(max_items - 1, -1, -1))
        self._lock = threading.Lock()
        self.last_index, self.last_sim = -1, -1.0

    def __len__(self) -> int:
        return len(self._order)

    def get(self, query_emb: np.ndarray) -> Optional[str]:
        """lfu_cache_get (main.py:67-98)."""
        with self._lock:
            self.last_index, self.last_sim = -1, -1.0
            if not self._order:
                return None
            best_sim, best_index = self.matrix.best(self._order, query_emb[0])
            self.last_index, self.last_sim = best_index, best_sim
            if best_sim < self.threshold or best_index < 0:
                return None
            entry = self._entries[self._order[best_index]]
            entry["freq"] = entry.get("freq", 1) + 1
            return entry["response"]

    def _remove_least_frequent_item(self) -> None:
        """main.py:101-118: first strict minimum of freq in list order."""
        if not self._order:
            return
        min_freq, min_index = float("inf"), -1
        for i, slot in enumerate(self._order):
            freq = self._entries[slot].get("freq", 1)
            if freq < min_freq:
                min_freq, min_index = freq, i
        if min_index >= 0:
            slot = self._order.pop(min_index)
            del self._entries[slot]
            self._free.append(slot)

    def put(self, query_emb: np.ndarray, response: str) -> None:
        """lfu_cache_put (main.py:121-128)."""
        with self._lock:
            if len(self._order) >= self.max_items:
                self._remove_least_frequent_item()
            slot = self._free.pop()
            self.matrix.set_slot(slot, np.asarray(query_emb, dtype=np.float32)[0])
            self._entries[slot] = {"response": response, "freq": 1}
            self._order.insert(0, slot)

    def freqs(self) -> List[int]:
        return [self._entries[s].get("freq", 1) for s in self._order]

    def responses(self) -> List[str]:
        return [self._entries[s]["response"] for s in self._order]


_default_cache: Optional[SemanticLfuCache] = None


def _cache() -> SemanticLfuCache:
    global _default_cache
    if _default_cache is None:
        _default_cache = SemanticLfuCache()
    return _default_cache


def cosine_similarity(a: np.ndarray, b: np.ndarray) -> float:
    """main.py:59-64 on the GPU (fp32, zero-norm rule); returns a Python float."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(1, -1)
    return float(default_context().cosine_all(a, np.asarray(b, dtype=np.float32))[0])


def lfu_cache_get(query_emb: np.ndarray) -> Optional[str]:
    return _cache().get(query_emb)


def lfu_cache_put(query_emb: np.ndarray, response: str) -> None:
    _cache().put(query_emb, response)


# ------------------------------------------------------------------------------ embeddings
class Embedder:
    """Tokenizer + encoder pair standing where Ollama stood (main.py:134-145): text -> 1024 floats.
    No prefix or instruction is added to queries or passages (the reference adds none, main.py:139)."""

    def __init__(self, encoder, tokenizer, max_len: int = 512):
        self.encoder, self.tokenizer, self.max_len = encoder, tokenizer, max_len
        self._lock = threading.Lock()

    def _tokenize(self, texts: List[str]):
        ids, lens = self.tokenizer.encode_batch(texts, self.max_len)
        s = int(min(self.max_len, max(16, (int(lens.max()) + 15) // 16 * 16)))
        return ids[:, :s], lens

    def embed(self, texts: List[str]) -> np.ndarray:
        if not texts:
            return np.zeros((0, self.encoder.cfg["hidden"]), np.float32)
        ids, lens = self._tokenize(texts)
        with self._lock:
            return self.encoder.encode_ids(ids, lens)

    def embed_batches(self, texts: List[str], batch_size: int = 64) -> np.ndarray:
        """Order-preserving bulk form: the WordPiece tokenisation of batch i + 1 (host, GIL released inside
        the C++ tokenizer) runs on a worker thread while the GPU encodes batch i."""
        if not texts:
            return np.zeros((0, self.encoder.cfg["hidden"]), np.float32)
        from concurrent.futures import ThreadPoolExecutor
        chunks = [texts[i:i + batch_size] for i in range(0, len(texts), batch_size)]
        out = []
        with ThreadPoolExecutor(max_workers=1) as pool:
            nxt = pool.submit(self._tokenize, chunks[0])
            for i in range(len(chunks)):
                ids, lens = nxt.result()
                if i + 1 < len(chunks):
                    nxt = pool.submit(self._tokenize, chunks[i + 1])
                with self._lock:
                    out.append(self.encoder.encode_ids(ids, lens))
        return np.concatenate(out, axis=0)


class Reranker:
    """Tokenizer + cross-encoder pair (a BERT with a classification head): scores (query, passage) pairs, where OpenSearch's
    ``rerank`` search-pipeline processor calls a model.  ``label``: the logit that is the score (default: the last)."""

    BATCH = 64

    def __init__(self, encoder, tokenizer, max_len: int = 512, max_query: int = 64, label: Optional[int] = None):
        n = encoder.labels
        if n < 1:
            raise ValueError("Reranker: the encoder has no classification head (load_weights(..., head=True))")
        self.label = n - 1 if label is None else label
        if not 0 <= self.label < n:
            raise ValueError(f"Reranker: label must be in [0, {n})")
        self.encoder, self.tokenizer, self.max_len = encoder, tokenizer, max_len
        self.max_query = min(max_query, max_len - 3)
        self._lock = threading.Lock()

    def score(self, query: str, texts: List[str]) -> np.ndarray:
        """-> float32 [n]: the model's score of (query, text) for every text, in batches of 64 pairs."""
        out = np.zeros(len(texts), np.float32)
        for lo in range(0, len(texts), self.BATCH):
            part = texts[lo:lo + self.BATCH]
            ids, types, lens = self.tokenizer.encode_pairs([query] * len(part), part, self.max_len, self.max_query)
            s = int(min(self.max_len, max(16, (int(lens.max()) + 15) // 16 * 16)))
            with self._lock:
                out[lo:lo + len(part)] = self.encoder.score_ids(ids[:, :s], types[:, :s], lens)[:, self.label]
        return out


_embedder: Optional[Embedder] = None
_reranker: Optional[Reranker] = None


def configure_embedder(embedder: Embedder) -> None:
    """Install the process-wide embedder used by the reference-named functions below."""
    global _embedder
    _embedder = embedder


def configure_reranker(reranker: Optional[Reranker]) -> None:
    """Install the process-wide reranker behind ``OpenSearchIndexer.search(rerank=...)`` (None: remove it)."""
    global _reranker
    _reranker = reranker


def _require_embedder() -> Embedder:
    if _embedder is None:
        raise RuntimeError("no embedder configured: call configure_embedder(Embedder(encoder, tokenizer))")
    return _embedder


async def ollama_embed_text(text: str, model: str = "mxbai-embed-large:latest") -> List[float]:
    """main.py:134-145: one text -> its embedding as a list of floats (``model`` kept for call compatibility)."""
    return _require_embedder().embed([text])[0].tolist()


async def embed_texts_in_batches(texts: List[str], batch_size: int = 64) -> np.ndarray:
    """main.py:148-169: order-preserving embedding of ``texts`` -> float32 [n, 1024]; [] -> np.array([])."""
    if not texts:
        return np.array([])
    return _require_embedder().embed_batches(texts, batch_size).astype(np.float32)


async def embed_query(query: str) -> np.ndarray:
    """main.py:172-180: one query -> float32 [1, 1024]; blank -> size-0 array."""
    if not query.strip():
        return np.array([])
    return _require_embedder().embed([query]).astype(np.float32)
