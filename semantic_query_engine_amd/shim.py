"""Wire-compatible HTTP front for the GPU path: the subset of the Ollama and
OpenSearch REST APIs that the reference uses, so the UNMODIFIED ``app/main.py`` can be pointed at it
with environment variables only (``OLLAMA_API_URL=http://HOST:PORT/api``, ``OPENSEARCH_HOST=HOST``,
``OPENSEARCH_PORT=PORT``).

    reference call (app/main.py)                       endpoint here
    ------------------------------------------------   ------------------------------------------
    :141  POST {OLLAMA_API_URL}/embeddings              POST /api/embeddings      {"embedding": [...]}
    :258  os_client.info()                              GET  /
    :261  os_client.indices.exists(name)                HEAD /{index}
    :282  os_client.indices.create(index, body)         PUT  /{index}
    :304  client.count(index=...)                       GET|POST /{index}/_count  {"count": n}; with {"query": {"match": ...}
                                                        | {"bool": ...}} on the text field the documents that match
    :342  helpers.bulk(client, actions)                 POST /_bulk (NDJSON, gzip accepted; index, create, update,
                                                        delete -- applied in body order)
          client.delete(index, id)                      DELETE /{index}/_doc/{id}
          client.delete_by_query(index, body)           POST /{index}/_delete_by_query (term / terms on doc_id, ids)
    :361  client.search(index, body={"size","query":{"knn":{"embedding":{"vector","k"}}}})
                                                        GET|POST /{index}/_search
                                                        (also knn.filter, knn.min_score / max_distance and
                                                        "collapse": {"field": "doc_id"}: one hit per document, and
                                                        "ext": {"mmr": {"candidates": n, "diversity": d}}: maximal
                                                        marginal relevance with lambda = 1 - d;
                                                        {"query": {"hybrid": {"queries": [{"knn": ...}, ...]}}} with
                                                        "ext": {"fusion": {"method", "rank_constant", "window",
                                                        "weights"}}: several vectors, one fused list;
                                                        {"query": {"match": {"text": "..." | {"query": "..."}}}}: BM25
                                                        over the text field (needs an analyzer:
                                                        retrieval.configure_analyzer), _score = the BM25 score;
                                                        {"query": {"bool": {"must", "should", "filter", "must_not",
                                                        "minimum_should_match"}}} over match clauses, which there take
                                                        "operator" and "minimum_should_match" (retrieval.text_query);
                                                        with configure_analyzer(..., positions=True) also
                                                        {"match_phrase": {"text": "..." | {"query", "slop": 0}}}, bare or
                                                        as a member of such a bool (retrieval.text_clauses);
                                                        knn.filter takes such match clauses beside term / terms / ids; one
                                                        {"match": ...} may also stand among the hybrid sub-queries:
                                                        lexical + vector rank fusion, fields._bm25 beside
                                                        fields._fused;
                                                        started with --reranker: "ext": {"rerank": {"query_context":
                                                        {"query_text": ...}}} reorders the hits by a cross-encoder's
                                                        score, which becomes _score)

Scores are the k-NN plugin's nmslib ``cosinesimil`` score ``1 / (2 - cos)``; ``_source`` carries
``doc_id``, ``text`` and the stored vector, as it did in OpenSearch.  Concurrent requests are
micro-batched because that is where the GPU path's throughput is: embedding requests into one encoder
call per <= 64 texts or 2 ms, ``_search`` requests into one batched scan per index per <= 64 queries or
1 ms (the reference issues every query as B = 1, main.py:499, :684; a B = 64 scan of 10 M rows costs what
a B = 1 scan costs -- both read the index once).

The app is built around two duck-typed objects so that the wire layer can be tested without a GPU:
``client`` (retrieval.GpuSearchClient: ``index(name)``, ``exists(name)``, ``count(index=)``; deletes go through
retrieval.delete_documents / delete_by_query on ``index(name)``, whose ``vectors`` need ``delete(ids)``) and
``embedder`` (retrieval.Embedder: ``embed(texts) -> float32 [n, dim]``).

    python -m semantic_query_engine_amd.shim --model /models/mxbai-embed-large-v1 --port 9200
"""
from __future__ import annotations

import asyncio
import gzip
import json
import numbers
import time
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
from fastapi import FastAPI, Request, Response
from fastapi.responses import JSONResponse

from .retrieval import (_check_collapse, _check_fusion, _check_mmr, mmr_depth, _doc_add, _doc_remove, _key_changed, _query_ids, _rows_of_doc, delete_documents, filter_rows, exclusion_rows, _can_exclude, resolve_routes, search_resolved,
                        push_keys, radial_min_cos, rerank_order, _text_changed, push_text, text_query, text_clauses, has_phrase, LEX_MAX_QUERY)
from . import retrieval as _retrieval
from . import fields as _fields
from .retrieval import field_predicate, field_predicates

_SHARDS = {"total": 1, "successful": 1, "skipped": 0, "failed": 0}
MAX_SEARCH_K = 256                                       # sqe_index_search: 1 <= k <= 256 (include/sqe.h)
MAX_RADIAL_SIZE = 10000                                  # sqe_index_range_search: max_hits <= 10000 (OpenSearch's window)
_EACH = "\x00each"                                       # batch key of filtered requests under per_query_filters
_RADIAL = "\x00radial"                                   # batch key of radial requests (no filter serialises to it)
_COLLAPSE = "\x00collapse"                               # ... and of collapsed requests
_MMR = "\x00mmr"                                         # ... and, followed by the depth, of MMR requests
_FUSE = "\x00fuse"                                       # ... and, followed by (k, method, depth, rank constant), of hybrid requests
_TEXT = "\x00text"                                       # ... of match requests on the text field
_BOOL = "\x00bool"                                       # ... of boolean text requests (bool over match clauses)
_COUNT = "\x00count"                                     # ... and of _count requests with a text query
_PHRASE = "\x00phrase"                                   # ... of clause requests (a match_phrase in them; retrieval.text_clauses)
_PCOUNT = "\x00pcount"                                   # ... and of their _count requests
_HYBRID = "\x00hybrid"                                   # ... and, followed by (k, depth, rank constant), of hybrid requests with a match


def _parse_match(match) -> str:
    """``{"text": "..."}`` or ``{"text": {"query": "..."}}`` -> the query text; anything else in ``match`` (another field,
    operator, fuzziness, ...) is not served."""
    if not isinstance(match, dict) or set(match) != {"text"}:
        raise ValueError("match is served on the [text] field only")
    spec = match["text"]
    if isinstance(spec, dict):
        if set(spec) != {"query"}:
            raise ValueError(f"match.text is served as a string or {{'query': string}} only, got {sorted(spec)}")
        spec = spec["query"]
    if not isinstance(spec, str):
        raise ValueError("match.text query must be a string")
    return spec


def _match_terms(text: str) -> np.ndarray:
    """The term occurrences of a match query by the configured analyzer."""
    analyzer = _retrieval._analyzer
    if analyzer is None:
        raise ValueError("match needs an analyzer: retrieval.configure_analyzer(tokenizer)")
    return analyzer.query(text)


class _EmbedBatcher:
    """Collects concurrent single-text requests into one ``embedder.embed`` call."""

    def __init__(self, embedder, max_batch: int = 64, max_wait_ms: float = 2.0):
        self.embedder, self.max_batch, self.max_wait = embedder, max_batch, max_wait_ms / 1e3
        self.queue: "asyncio.Queue" = asyncio.Queue()
        self.task: Optional[asyncio.Task] = None
        self.batches = 0

    async def embed(self, text: str) -> np.ndarray:
        if self.task is None or self.task.done():
            self.task = asyncio.get_running_loop().create_task(self._run())
        fut = asyncio.get_running_loop().create_future()
        await self.queue.put((text, fut))
        return await fut

    async def _run(self):
        loop = asyncio.get_running_loop()
        while True:
            items = [await self.queue.get()]
            deadline = loop.time() + self.max_wait
            while len(items) < self.max_batch:
                left = deadline - loop.time()
                if left <= 0:
                    break
                try:
                    items.append(await asyncio.wait_for(self.queue.get(), left))
                except asyncio.TimeoutError:
                    break
            texts = [t for t, _ in items]
            try:
                out = await loop.run_in_executor(None, self.embedder.embed, texts)
                self.batches += 1
                for (_, fut), row in zip(items, out):
                    if not fut.done():
                        fut.set_result(row)
            except Exception as e:                       # every waiter sees the failure
                for _, fut in items:
                    if not fut.done():
                        fut.set_exception(e)


class _SearchBatcher:
    """Collects concurrent k-NN requests into one batched scan per index."""

    def __init__(self, client, max_batch: int = 64, max_wait_ms: float = 1.0, per_query_filters: bool = False):
        self.client, self.max_batch, self.max_wait = client, max_batch, max_wait_ms / 1e3
        self.per_query_filters = per_query_filters        # filtered requests share one call whatever their filters
        self.queue: "asyncio.Queue" = asyncio.Queue()
        self.task: Optional[asyncio.Task] = None
        self.batches = 0                                  # device calls made
        self.batch_sizes: List[int] = []

    async def search(self, index: str, vector: np.ndarray, k: int, field: str, flt: Optional[Dict] = None,
                     min_cos: Optional[float] = None, collapse: bool = False, mmr: Optional[Tuple[float, int]] = None,
                     fusion: Optional[Tuple[str, int, int, Optional[List[float]]]] = None, terms: Optional[np.ndarray] = None):
        """``flt``: an OpenSearch filter clause; only requests with identical filters share a device call, unless the
        batcher was made with ``per_query_filters``: then the filtered requests of an index share ONE call whatever their
        filters, each answered over its own clause (``VectorIndex.search_filtered_each``).  ``min_cos``:
        a radial request (k = its size), answered as (hits, exact total); radial requests share calls only with each
        other (thresholds are per query, max_hits is the largest size).  ``collapse``: one hit per ``doc_id``; collapsed
        requests share calls only with each other.  ``mmr``: (lambda, candidates); the depth is resolved HERE, per request
        (``mmr_depth``: an automatic depth follows the request's own k, never the largest k of a batch), and MMR requests
        of equal depth share calls (lambda is per query, k is the largest: at one depth the greedy choice is prefix-stable).
        ``fusion``: (method, rank_constant, depth, weights) of a hybrid request (``_check_fusion``; the depth is the request's
        own); ``vector`` holds its m sub-queries, and hybrid requests of equal (k, method, depth, rank_constant) share ONE
        fused call, each as a logical query of its own with its own weights.  ``terms``: the term occurrences of a ``match``
        on the text field: alone (``vector`` is a placeholder row) it is a BM25 request, and BM25 requests of an index share
        one lexical search; with ``fusion`` it is the lexical list of a hybrid request (weights: the sub-queries' first, the
        lexical list's last), and such requests of equal (k, depth, rank_constant) share ONE hybrid call.  A tuple
        (terms, roles, min_should) as ``terms`` is a boolean text request (``retrieval.text_query``): those of an index
        share one ``search_bool`` call, or, with k == 0 (a _count), one counting call."""
        if self.task is None or self.task.done():
            self.task = asyncio.get_running_loop().create_task(self._run())
        fut = asyncio.get_running_loop().create_future()
        if terms is not None and fusion is None:
            # a boolean request carries (terms, roles, min_should); k == 0 asks for its count alone
            # (a list of clauses in place of the terms: a clause request, retrieval.text_clauses)
            phrase = isinstance(terms, tuple) and isinstance(terms[0], list)
            key = _TEXT if not isinstance(terms, tuple) else (_PCOUNT if phrase else _COUNT) if k == 0 else _PHRASE if phrase else _BOOL
            await self.queue.put((index, vector, k, field, fut, key, None, None, terms))
            return await fut
        if terms is not None:
            _method, c, depth, weights = fusion
            await self.queue.put((index, vector, k, field, fut, f"{_HYBRID}{k}:{depth}:{c}", None, None,
                                  (vector.shape[0], weights, terms, depth, c)))
            return await fut
        if fusion is not None:
            method, c, depth, weights = fusion
            await self.queue.put((index, vector, k, field, fut, f"{_FUSE}{k}:{method}:{depth}:{c}", None, None,
                                  (vector.shape[0], weights, method, depth, c)))
            return await fut
        if mmr is not None:
            mmr = (mmr[0], mmr_depth(k, mmr[1]))
            await self.queue.put((index, vector, k, field, fut, f"{_MMR}{mmr[1]}", None, None, mmr))
            return await fut
        key = _COLLAPSE if collapse else _RADIAL if min_cos is not None else None if flt is None else json.dumps(flt, sort_keys=True)
        if self.per_query_filters and key is not None and key not in (_COLLAPSE, _RADIAL):
            key = _EACH
        await self.queue.put((index, vector, k, field, fut, key, flt, min_cos))
        return await fut

    async def _run(self):
        loop = asyncio.get_running_loop()
        while True:
            items = [await self.queue.get()]
            deadline = loop.time() + self.max_wait
            while len(items) < self.max_batch:
                left = deadline - loop.time()
                if left <= 0:
                    break
                try:
                    items.append(await asyncio.wait_for(self.queue.get(), left))
                except asyncio.TimeoutError:
                    break
            groups: Dict[tuple, List] = {}
            for it in items:
                groups.setdefault((it[0], it[5]), []).append(it)
            for (name, key), group in groups.items():
                fn, extra = _route(key, group)
                try:
                    vectors = np.concatenate([g[1] for g in group], axis=0)
                    hits = await loop.run_in_executor(None, fn, self.client, name, vectors,
                                                      [g[2] for g in group], [g[3] for g in group], *extra)
                    self.batches += 1
                    self.batch_sizes.append(len(group))
                    for g, h in zip(group, hits):
                        if not g[4].done():
                            g[4].set_result(h)
                except Exception as e:
                    # A failing batch must not turn every co-batched client's search into a 500 (requests are
                    # validated before they are queued, so this is a device error or a request the validation
                    # missed): run the group's requests one by one, only the offending ones fail.
                    if len(group) == 1:
                        if not group[0][4].done():
                            group[0][4].set_exception(e)
                        continue
                    for g in group:
                        if g[4].done():
                            continue
                        try:
                            one = _route(key, [g])[1]
                            h = await loop.run_in_executor(None, fn, self.client, name, g[1], [g[2]], [g[3]], *one)
                            self.batches += 1
                            self.batch_sizes.append(1)
                            g[4].set_result(h[0])
                        except Exception as e1:
                            g[4].set_exception(e1)


def _route(key: Optional[str], group: List[tuple]):
    """(batch function, its arguments after the common five) for the queued requests ``group`` that share the batch key
    ``key``; the one-by-one retry of a failed batch calls it with a group of one."""
    if key == _RADIAL:
        return _range_hits_batch, ([g[7] for g in group],)
    if key == _COLLAPSE:
        return _collapse_hits_batch, ()
    if key == _EACH:
        return _each_hits_batch, ([g[6] for g in group],)
    if key is not None and key.startswith(_MMR):         # g[8] = (lambda, depth)
        return _mmr_hits_batch, ([g[8][0] for g in group], group[0][8][1])
    if key == _TEXT:                                     # g[8] = the query's terms
        return _text_hits_batch, ([g[8] for g in group],)
    if key == _BOOL:                                     # g[8] = (terms, roles, min_should)
        return _bool_hits_batch, ([g[8] for g in group],)
    if key == _COUNT:
        return _count_batch, ([g[8] for g in group],)
    if key == _PHRASE:                                   # g[8] = (clauses, roles, min_should)
        return _bool_hits_batch, ([g[8] for g in group], True)
    if key == _PCOUNT:
        return _count_batch, ([g[8] for g in group], True)
    if key is not None and key.startswith(_HYBRID):      # g[8] = (m, weights, terms, depth, rank constant)
        return _hybrid_hits_batch, ([g[8][0] for g in group], [g[8][1] for g in group], [g[8][2] for g in group], *group[0][8][3:])
    if key is not None and key.startswith(_FUSE):        # g[8] = (m, weights, method, depth, rank constant)
        return _fused_hits_batch, ([g[8][0] for g in group], [g[8][1] for g in group], *group[0][8][2:])
    return _search_hits_batch, (() if group[0][6] is None else (group[0][6],))      # plain, or the filter the group shares


def _os_error(status: int, etype: str, reason: str, **extra) -> JSONResponse:
    err = {"type": etype, "reason": reason}
    err.update(extra)
    return JSONResponse({"error": {"root_cause": [err], **err}, "status": status}, status_code=status)


async def _body(request: Request) -> bytes:
    raw = await request.body()
    if request.headers.get("content-encoding", "").lower() == "gzip" and raw:
        raw = gzip.decompress(raw)                       # opensearch-py with http_compress=True (main.py:254)
    return raw


def create_app(client, embedder=None, embed_dim: int = 1024, per_query_filters: bool = False, reranker=None) -> FastAPI:
    app = FastAPI(title="semantic-query-engine GPU shim")
    batcher = _EmbedBatcher(embedder) if embedder is not None else None
    searcher = _SearchBatcher(client, per_query_filters=per_query_filters)
    mappings: Dict[str, Any] = {}
    app.state.batcher = batcher
    app.state.search_batcher = searcher

    # ------------------------------------------------------------------ Ollama
    @app.post("/api/embeddings")
    async def ollama_embeddings(request: Request):
        if batcher is None:
            return JSONResponse({"error": "no embedding model loaded"}, status_code=500)
        try:
            payload = json.loads(await _body(request) or b"{}")
        except ValueError:
            return JSONResponse({"error": "invalid JSON"}, status_code=400)
        if "model" not in payload:
            return JSONResponse({"error": "model is required"}, status_code=400)
        prompt = payload.get("prompt", "")
        if not isinstance(prompt, str) or prompt == "":
            return JSONResponse({"embedding": []})       # Ollama answers an empty prompt with an empty list
        vec = await batcher.embed(prompt)
        return JSONResponse({"embedding": [float(x) for x in vec]})

    # ------------------------------------------------------------------ OpenSearch
    @app.get("/")
    async def info():
        return {"name": "sqe-gpu", "cluster_name": "sqe", "cluster_uuid": "sqe",
                "version": {"distribution": "opensearch", "number": "2.11.0", "build_type": "sqe-shim",
                            "lucene_version": "n/a", "minimum_wire_compatibility_version": "7.10.0",
                            "minimum_index_compatibility_version": "7.0.0"},
                "tagline": "The OpenSearch Project: https://opensearch.org/"}

    @app.post("/_bulk")
    @app.put("/_bulk")
    async def bulk_root(request: Request):
        return await _bulk(request, None)

    @app.post("/{index}/_bulk")
    @app.put("/{index}/_bulk")
    async def bulk_index(index: str, request: Request):
        return await _bulk(request, index)

    async def _bulk(request: Request, default_index: Optional[str]):
        t0 = time.perf_counter()
        lines = [ln for ln in (await _body(request)).split(b"\n") if ln.strip()]
        # group the documents of one index into one add_embeddings-style device call, and the deletes likewise; body
        # order holds per index: the pending documents of an index are written before a delete on that index runs, and
        # the pending deletes before a document that follows them
        items: List[Dict[str, Any]] = []
        steps: List[tuple] = []                           # ("docs" | "delete", index, [(slot, op, _id, _source)])
        open_step: Dict[str, int] = {}                    # index -> position of its last step in `steps`
        i = 0
        try:
            while i < len(lines):
                action = json.loads(lines[i])
                (op, meta), = action.items()
                i += 1
                if op == "delete":
                    name = meta.get("_index", default_index)
                    slot = len(items)
                    items.append(None)
                    at = open_step.get(name)
                    if at is None or steps[at][0] != "delete":
                        steps.append(("delete", name, []))
                        at = open_step[name] = len(steps) - 1
                    steps[at][2].append((slot, op, meta.get("_id"), None))
                    continue
                if op not in ("index", "create", "update"):
                    return _os_error(400, "illegal_argument_exception", f"Malformed action/metadata line, unknown action [{op}]")
                if i >= len(lines):
                    return _os_error(400, "illegal_argument_exception", "The bulk request must be terminated by a newline [\\n]")
                src = json.loads(lines[i])
                i += 1
                name = meta.get("_index", default_index)
                slot = len(items)
                items.append(None)
                at = open_step.get(name)
                if at is None or steps[at][0] != "docs":
                    steps.append(("docs", name, []))
                    at = open_step[name] = len(steps) - 1
                steps[at][2].append((slot, op, meta.get("_id"), src))
        except ValueError as e:
            return _os_error(400, "parse_exception", f"malformed bulk body: {e}")
        errors = False
        loop = asyncio.get_running_loop()
        for kind, name, docs in steps:
            fn = _index_docs if kind == "docs" else _delete_docs
            res = await loop.run_in_executor(None, fn, client, name, docs, embed_dim)
            for (slot, op, _id, _src), r in zip(docs, res):
                items[slot] = {op: r}
                errors = errors or "error" in r
        return {"took": int((time.perf_counter() - t0) * 1e3), "errors": errors, "items": items}

    @app.delete("/{index}/_doc/{doc_id}")
    async def delete_doc(index: str, doc_id: str):
        if not client.exists(index):
            return _os_error(404, "index_not_found_exception", f"no such index [{index}]", index=index)
        try:
            r, = await asyncio.get_running_loop().run_in_executor(None, _delete_docs, client, index, [(0, "delete", doc_id, None)], embed_dim)
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        status = r.pop("status")
        return JSONResponse(r, status_code=status)

    @app.post("/{index}/_delete_by_query")
    async def delete_by_query(index: str, request: Request):
        t0 = time.perf_counter()
        if not client.exists(index):
            return _os_error(404, "index_not_found_exception", f"no such index [{index}]", index=index)
        raw = await _body(request)
        try:
            body = json.loads(raw) if raw.strip() else {}
            idx = client.index(index)
            with idx.lock:
                os_ids = _query_ids(idx, body)
        except ValueError as e:
            return _os_error(400, "parsing_exception", str(e))
        try:
            res = await asyncio.get_running_loop().run_in_executor(
                None, _delete_docs, client, index, [(j, "delete", _id, None) for j, _id in enumerate(os_ids)], embed_dim)
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        n = sum(1 for r in res if r["status"] == 200)
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "total": n, "deleted": n, "batches": 1,
                "version_conflicts": 0, "noops": 0, "retries": {"bulk": 0, "search": 0}, "throttled_millis": 0,
                "requests_per_second": -1.0, "throttled_until_millis": 0, "failures": []}

    @app.head("/{index}")
    async def index_exists(index: str):
        return Response(status_code=200 if client.exists(index) else 404)

    @app.put("/{index}")
    async def index_create(index: str, request: Request):
        if client.exists(index):
            return _os_error(400, "resource_already_exists_exception", f"index [{index}] already exists", index=index)
        raw = await _body(request)
        body = json.loads(raw) if raw.strip() else {}
        for field, spec in body.get("mappings", {}).get("properties", {}).items():
            if spec.get("type") == "knn_vector":
                dim = int(spec.get("dimension", embed_dim))
                space = spec.get("method", {}).get("space_type", "cosinesimil")
                if dim != client.dim:
                    return _os_error(400, "mapper_parsing_exception", f"knn_vector dimension {dim} != {client.dim} of this server")
                if space != "cosinesimil":
                    return _os_error(400, "mapper_parsing_exception", f"space_type [{space}] is not served; only cosinesimil")
        declared = {field: spec.get("type") for field, spec in body.get("mappings", {}).get("properties", {}).items()
                    if isinstance(spec, dict) and spec.get("type") in _fields.FIELD_TYPES and field not in _fields.RESERVED}
        if len(declared) > _fields.MAX_FIELDS:
            return _os_error(400, "mapper_parsing_exception", f"an index holds at most {_fields.MAX_FIELDS} filterable fields, "
                             f"the mapping declares {len(declared)}: {sorted(declared)}")
        mappings[index] = body
        client.index(index)
        if declared:                                  # long / integer / boolean / date / double / float / keyword: filterable on the device
            client.configure_fields(index, declared)
        return {"acknowledged": True, "shards_acknowledged": True, "index": index}

    @app.get("/{index}/_count")
    @app.post("/{index}/_count")
    async def count(index: str, request: Request):
        """Every live document, or, with ``{"query": {"match": ...} | {"bool": ...}}`` (``text_query``), those whose text
        matches: counted on the device, the concurrent requests of an index in one call."""
        if not client.exists(index):
            return _os_error(404, "index_not_found_exception", f"no such index [{index}]", index=index)
        raw = await _body(request)
        try:
            body = json.loads(raw) if raw.strip() else {}
            query = body.get("query") if isinstance(body, dict) else None
            if isinstance(query, dict) and has_phrase(query):
                text = text_clauses(query)
            else:
                text = text_query(query) if isinstance(query, dict) and ("match" in query or "bool" in query) else None
        except (ValueError, TypeError, AttributeError) as e:
            return _os_error(400, "parsing_exception", f"_count serves a match on [text] or a bool of such matches: {e}")
        if text is None:
            return {"count": client.count(index=index)["count"], "_shards": _SHARDS}
        try:
            n = 0 if text[2] > LEX_MAX_QUERY else await searcher.search(index, np.zeros((1, client.dim), np.float32), 0, "embedding", terms=text)
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        return {"count": n, "_shards": _SHARDS}

    @app.get("/{index}/_search")
    @app.post("/{index}/_search")
    async def search(index: str, request: Request):
        t0 = time.perf_counter()
        if not client.exists(index):
            return _os_error(404, "index_not_found_exception", f"no such index [{index}]", index=index)
        raw = await _body(request)
        try:
            body = json.loads(raw) if raw.strip() else {}
            if isinstance(body, dict) and ("aggs" in body or "aggregations" in body):
                return await search_aggs(index, body, t0)
            if isinstance(body, dict) and "sort" in body and _sort_route(body.get("query")):
                return await search_sorted(index, body, t0)
            if isinstance(body, dict) and isinstance(body.get("query"), dict) and "hybrid" in body["query"]:
                return await search_hybrid(index, body, t0)
            if isinstance(body, dict) and isinstance(body.get("query"), dict) and "match" in body["query"]:
                return await search_match(index, body, t0)
            if isinstance(body, dict) and isinstance(body.get("query"), dict) and ("bool" in body["query"] or "match_phrase" in body["query"]):
                return await search_bool(index, body, t0)
            knn = body["query"]["knn"]
            (field, spec), = knn.items()
            vector = np.asarray(spec["vector"], dtype=np.float32)
            given = [key for key in ("k", "min_score", "max_distance") if key in spec]
            if len(given) > 1:
                return _os_error(400, "parsing_exception", f"knn takes one of [k], [min_score], [max_distance], got {given}")
            min_cos = None
            if given and given[0] != "k":
                # radial search: the best `size` hits at or above the floor, hits.total the exact count
                min_cos = float(radial_min_cos(**{given[0]: float(spec[given[0]])}))
                k = int(body.get("size", 10))
            else:
                k = int(body.get("size", spec.get("k", 10)))
                k = max(1, min(k, int(spec.get("k", k)))) if "k" in spec else k
            flt = spec.get("filter")
            collapse = body.get("collapse")
            if collapse is not None:
                _check_collapse(collapse)
            mmr = None
            if isinstance(body.get("ext"), dict) and "mmr" in body["ext"]:      # any other ext is ignored, as it always was
                mmr = _parse_ext_mmr(body["ext"]["mmr"], k)
            rerank_text = None
            if reranker is not None and isinstance(body.get("ext"), dict) and "rerank" in body["ext"]:
                rerank_text = _parse_ext_rerank(body["ext"]["rerank"])
        except (KeyError, ValueError, TypeError) as e:
            return _os_error(400, "parsing_exception", f"only {{'query': {{'knn': {{field: {{'vector', 'k', 'filter'}}}}}}}} is served: {e}")
        if min_cos is not None and flt is not None:
            return _os_error(400, "parsing_exception", "knn: radial search (min_score / max_distance) with a filter is not served")
        if collapse is not None and (min_cos is not None or flt is not None):
            return _os_error(400, "parsing_exception", "collapse together with knn.filter, min_score or max_distance is not served")
        if mmr is not None and (min_cos is not None or flt is not None or collapse is not None):
            return _os_error(400, "parsing_exception", "ext.mmr together with knn.filter, min_score, max_distance or collapse is not served")
        if flt is not None:
            named = client.index(index)
            try:
                with named.lock:
                    if field_predicate(named, flt) is not None:
                        pass                              # a conjunction of field leaves: translated, nothing to resolve
                    elif not _can_exclude(named) or exclusion_rows(named, flt) is None:    # (a must_not is checked without its complement)
                        filter_rows(named, flt)           # validated here: an unserved clause never joins a batch
            except (ValueError, TypeError, AttributeError) as e:
                return _os_error(400, "parsing_exception", f"knn filter: {e}")
        # every request is validated BEFORE it joins a batch: one malformed request must fail alone
        if vector.ndim != 1 or vector.shape[0] != client.dim:
            got = "x".join(str(d) for d in vector.shape) or "a scalar"
            return _os_error(400, "illegal_argument_exception", f"query vector must be a flat list of {client.dim} numbers, got {got}")
        if not np.all(np.isfinite(vector)):
            return _os_error(400, "illegal_argument_exception", "query vector holds a NaN or an infinity")
        if min_cos is not None and not 0 <= k <= MAX_RADIAL_SIZE:
            return _os_error(400, "illegal_argument_exception", f"size must be in [0, {MAX_RADIAL_SIZE}] (radial search), got {k}")
        if min_cos is None and not 1 <= k <= MAX_SEARCH_K:
            return _os_error(400, "illegal_argument_exception", f"size / k must be in [1, {MAX_SEARCH_K}] (sqe_index_search), got {k}")
        vector = vector[None, :]
        try:
            if min_cos is not None:
                hits, total = await searcher.search(index, vector, k, field, min_cos=min_cos)
            elif mmr is not None:
                hits = await searcher.search(index, vector, k, field, mmr=mmr)
                total = min(client.count(index=index)["count"], len(hits))
            elif collapse is not None:
                hits = await searcher.search(index, vector, k, field, collapse=True)
                total = min(client.count(index=index)["count"], len(hits))
            else:
                hits = await searcher.search(index, vector, k, field) if flt is None else \
                    await searcher.search(index, vector, k, field, flt)
                total = min(client.count(index=index)["count"], len(hits))
            if rerank_text is not None and hits:
                texts = [str(h["_source"].get("text") or "") for h in hits]
                scores = await asyncio.get_running_loop().run_in_executor(None, reranker.score, rerank_text, texts)
                hits = [dict(hits[j], _score=float(scores[j])) for j in rerank_order(scores, len(hits))]
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "_shards": _SHARDS,
                "hits": {"total": {"value": int(total), "relation": "eq"},
                         "max_score": hits[0]["_score"] if hits else None, "hits": hits}}

    async def search_aggs(index: str, body: Dict, t0: float):
        """``{"size": 0, "aggs": {name: {...}}, "query": ...}``: aggregations on the configured fields over the documents the
        query selects (absent or ``match_all``: all of them; else anything ``filter_rows`` takes), no hits
        (``GpuSearchClient.aggregate``)."""
        query = body.get("query")
        if "aggs" in body and "aggregations" in body:
            return _os_error(400, "parsing_exception", "aggs and aggregations are one option under two names: give one")
        if isinstance(query, dict) and "knn" in query:
            return _os_error(400, "parsing_exception", "aggs beside a knn query are not served: aggregations take \"size\": 0 and a filter query")
        size = body.get("size", 10)
        if isinstance(size, bool) or size != 0:
            return _os_error(400, "parsing_exception", f"aggs are served with \"size\": 0 only (hits and aggregations in one request are not), got size {size}")
        if query is not None and not isinstance(query, dict):
            return _os_error(400, "parsing_exception", "aggs: query must be an object")
        flt = None if query is None or set(query) == {"match_all"} else query
        try:
            # a malformed body is a ValueError of the translation; anything else is a fault of this server, answered 500
            r = await asyncio.get_running_loop().run_in_executor(None, client.aggregate, index, body.get("aggs", body.get("aggregations")), flt)
        except ValueError as e:
            return _os_error(400, "parsing_exception", f"aggs: {e}")
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "_shards": _SHARDS,
                "hits": {"total": {"value": int(r["selected"]), "relation": "eq"}, "max_score": None, "hits": []},
                "aggregations": r["aggregations"]}

    async def search_sorted(index: str, body: Dict, t0: float):
        """``{"sort": [...], "query": <a filter or none>, "size", "from", "search_after"}``: the documents the query selects
        (absent or ``match_all``: all of them; else what ``_sort_route`` admits and ``filter_rows`` takes) in the order of the
        configured fields ``sort`` names, no scoring (``GpuSearchClient.search_sorted``).  Such requests are not batched: each
        is one device call, serialised under the index lock."""
        query = body.get("query")
        size, from_ = body.get("size", 10), body.get("from", 0)
        if isinstance(size, bool) or not isinstance(size, int) or not 1 <= size <= MAX_SEARCH_K:
            return _os_error(400, "illegal_argument_exception", f"size must be in [1, {MAX_SEARCH_K}] (sqe_index_sort_fields), got {size}")
        if isinstance(from_, bool) or not isinstance(from_, int) or from_ < 0 or from_ + size > MAX_SEARCH_K:
            return _os_error(400, "illegal_argument_exception",
                             f"from + size must be in [1, {MAX_SEARCH_K}] (page further with search_after), got from {from_} and size {size}")
        flt = None if query is None or set(query) == {"match_all"} else query
        try:
            # a malformed body is a ValueError of the translation; anything else is a fault of this server, answered 500
            r = await asyncio.get_running_loop().run_in_executor(None, client.search_sorted, index, body["sort"], size, flt,
                                                                 body.get("search_after"), from_)
        except ValueError as e:
            return _os_error(400, "parsing_exception", f"sort: {e}")
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        named = client.index(index)
        with named.lock:
            rev = {row: os_id for os_id, row in named.row_of_id.items()}
        hits = [{"_index": index, "_id": rev.get(row), "_score": None, "_source": src, "sort": sv} for row, src, sv in r["hits"]]
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "_shards": _SHARDS,
                "hits": {"total": {"value": int(r["total"]), "relation": "eq"}, "max_score": None, "hits": hits}}

    async def search_match(index: str, body: Dict, t0: float):
        """``{"query": {"match": {"text": "..." | {"query": "..."}}}}``: the ``size`` best documents by BM25."""
        try:
            if set(body["query"]) != {"match"}:
                raise ValueError(f"match is served alone, got {sorted(body['query'])}")
            text = _parse_match(body["query"]["match"])
            unserved = [key for key in ("collapse",) if body.get(key) is not None]
            if unserved:
                raise ValueError(f"match together with {unserved} is not served")
            k = int(body.get("size", 10))
            terms = _match_terms(text)
        except (KeyError, ValueError, TypeError, AttributeError) as e:
            return _os_error(400, "parsing_exception", f"match is served as {{'match': {{'text': string | {{'query': string}}}}}} only: {e}")
        if not 1 <= k <= MAX_SEARCH_K:
            return _os_error(400, "illegal_argument_exception", f"size must be in [1, {MAX_SEARCH_K}] (sqe_lex_search), got {k}")
        try:
            hits = await searcher.search(index, np.zeros((1, client.dim), np.float32), k, "embedding", terms=terms)
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "_shards": _SHARDS,
                "hits": {"total": {"value": len(hits), "relation": "eq"},
                         "max_score": hits[0]["_score"] if hits else None, "hits": hits}}

    async def search_bool(index: str, body: Dict, t0: float):
        """``{"query": {"bool": {...}}}`` over ``match`` clauses on the text field (``text_query``): the ``size`` best matching
        documents by BM25; a document that only ``filter`` terms matched scores 0 and comes last.  ``operator`` and
        ``minimum_should_match`` of a single ``match`` are served as ``{"bool": {"must": [{"match": ...}]}}``.  With an analyzer
        that keeps positions, ``match_phrase`` clauses stand among the members of the ``bool``, and a bare
        ``{"query": {"match_phrase": ...}}`` comes through here too (``text_clauses``)."""
        try:
            if set(body["query"]) not in ({"bool"}, {"match_phrase"}):
                raise ValueError(f"bool or match_phrase is served alone, got {sorted(body['query'])}")
            if body.get("collapse") is not None:
                raise ValueError("bool together with collapse is not served")
            k = int(body.get("size", 10))
            text = text_clauses(body["query"]) if has_phrase(body["query"]) else text_query(body["query"])
        except (KeyError, ValueError, TypeError, AttributeError) as e:
            return _os_error(400, "parsing_exception", f"bool is served over match and match_phrase clauses on [text] only, match_phrase with slop 0 and an analyzer "
                                                        f"that keeps positions: {e}")
        if not 1 <= k <= MAX_SEARCH_K:
            return _os_error(400, "illegal_argument_exception", f"size must be in [1, {MAX_SEARCH_K}] (sqe_lex_search_bool), got {k}")
        try:
            hits = [] if text[2] > LEX_MAX_QUERY else \
                await searcher.search(index, np.zeros((1, client.dim), np.float32), k, "embedding", terms=text)
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "_shards": _SHARDS,
                "hits": {"total": {"value": len(hits), "relation": "eq"},
                         "max_score": hits[0]["_score"] if hits else None, "hits": hits}}

    async def search_hybrid(index: str, body: Dict, t0: float):
        """``{"query": {"hybrid": {"queries": [{"knn": {field: {"vector", "k"}}}, ...]}}}``: 1..32 knn sub-queries on one
        field, fused into one list (``"ext": {"fusion": {...}}``: ``_check_fusion``; default rrf with constant 60).  At most
        one sub-query may be ``{"match": {"text": ...}}``: its BM25 list joins the rank fusion (rrf only; at most 31 knn
        sub-queries beside it; fusion weights in the order of the sub-queries)."""
        try:
            subs = body["query"]["hybrid"]["queries"]
            if not isinstance(subs, list) or not subs:
                raise ValueError("hybrid.queries must be a non-empty list")
            field, vectors, ks = None, [], []
            terms, match_at = None, None
            for at, sub in enumerate(subs):
                if isinstance(sub, dict) and set(sub) == {"match"}:
                    if terms is not None:
                        raise ValueError("at most one match sub-query is served")
                    terms, match_at = _match_terms(_parse_match(sub["match"])), at
                    continue
                if not isinstance(sub, dict) or set(sub) != {"knn"}:
                    raise ValueError("every hybrid sub-query must be a knn query or one match on [text]")
                (f, spec), = sub["knn"].items()
                if field is not None and f != field:
                    raise ValueError(f"hybrid sub-queries must name one field, got [{field}] and [{f}]")
                field = f
                unserved = [key for key in ("filter", "min_score", "max_distance") if key in spec]
                if unserved:
                    raise ValueError(f"hybrid sub-queries with {unserved} are not served")
                vectors.append(np.asarray(spec["vector"], dtype=np.float32))
                if "k" in spec:
                    ks.append(int(spec["k"]))
            k = int(body["size"]) if "size" in body else min(ks) if ks else 10
            if body.get("collapse") is not None:
                raise ValueError("hybrid together with collapse is not served")
            ext = body.get("ext") if isinstance(body.get("ext"), dict) else {}
            if "mmr" in ext:
                raise ValueError("hybrid together with ext.mmr is not served")
            if not 1 <= k <= MAX_SEARCH_K:
                return _os_error(400, "illegal_argument_exception", f"size / k must be in [1, {MAX_SEARCH_K}] (sqe_index_search_fused), got {k}")
            fusion = _check_fusion(ext.get("fusion"), k, len(subs))
            if terms is not None:
                if fusion[0] != "rrf":
                    raise ValueError("hybrid with a match sub-query is rank fusion (rrf) only")
                if fusion[3] is not None:                  # weights come in sub-query order; the lexical list's goes last
                    w = list(fusion[3])
                    fusion = (*fusion[:3], w[:match_at] + w[match_at + 1:] + [w[match_at]])
        except (KeyError, ValueError, TypeError, AttributeError) as e:
            return _os_error(400, "parsing_exception", f"hybrid is served as {{'queries': [{{'knn': {{field: {{'vector', 'k'}}}}}}, ...]}} only: {e}")
        # every request is validated BEFORE it joins a batch: one malformed request must fail alone
        for vector in vectors:
            if vector.ndim != 1 or vector.shape[0] != client.dim:
                got = "x".join(str(d) for d in vector.shape) or "a scalar"
                return _os_error(400, "illegal_argument_exception", f"query vector must be a flat list of {client.dim} numbers, got {got}")
            if not np.all(np.isfinite(vector)):
                return _os_error(400, "illegal_argument_exception", "query vector holds a NaN or an infinity")
        try:
            stacked = np.stack(vectors) if vectors else np.zeros((0, client.dim), np.float32)
            hits = await searcher.search(index, stacked, k, field or "embedding", fusion=fusion, terms=terms)
            total = min(client.count(index=index)["count"], len(hits))
        except Exception as e:
            return _os_error(500, "sqe_device_exception", str(e))
        return {"took": int((time.perf_counter() - t0) * 1e3), "timed_out": False, "_shards": _SHARDS,
                "hits": {"total": {"value": int(total), "relation": "eq"},
                         "max_score": max(h["_score"] for h in hits) if hits else None, "hits": hits}}

    return app


def _index_docs(client, name: str, docs, embed_dim: int):
    """docs: [(slot, op, _id, _source)] of one index -> per-document bulk item bodies, in order.

    Vectors are validated and converted first, the device add / update runs next, and the host docstore
    (``sources`` / ``row_of_id``) is committed only after it succeeded: a failing device call reports every
    planned document as failed (500) and leaves docstore and vector rows in step."""
    idx = client.index(name)
    out: List[Optional[Dict[str, Any]]] = [None] * len(docs)
    shards = {"total": 1, "successful": 1, "failed": 0}
    with idx.lock:
        schema = _fields.schema_of(idx)
        doc_rows = _rows_of_doc(idx)
        base_rows = len(idx.sources)
        new_vecs: List[np.ndarray] = []
        new_recs: List[Dict[str, Any]] = []
        new_ids: Dict[str, int] = {}                          # _id -> position among this call's inserts
        upd: Dict[int, tuple] = {}                            # stored row -> (record, vector): last writer wins
        planned: List[tuple] = []                             # (position in docs, item body on success)
        for pos, (_slot, op, _id, src) in enumerate(docs):
            base = {"_index": name, "_id": _id, "_shards": shards, "_primary_term": 1}
            emb = src.get("embedding") if isinstance(src, dict) else None
            vec = None
            if _id is not None and isinstance(emb, list) and len(emb) == client.dim:
                try:
                    vec = np.asarray(emb, dtype=np.float32)  # None / strings inside the list fail here, per document
                except (TypeError, ValueError):
                    vec = None
            if vec is None or vec.shape != (client.dim,):
                out[pos] = {**base, "status": 400, "error": {"type": "mapper_parsing_exception",
                                                             "reason": f"_id and an 'embedding' of {client.dim} floats are required"}}
                continue
            rec = {"doc_id": src.get("doc_id"), "text": src.get("text")}
            if schema is not None:
                try:
                    rec.update(schema.document_fields(src))      # the configured fields, parsed: a value that does not parse refuses the document
                except _fields.FieldValueError as e:
                    out[pos] = {**base, "status": 400, "error": {"type": "mapper_parsing_exception", "reason": str(e)}}
                    continue
            row = idx.row_of_id.get(_id)
            if row is None and _id not in new_ids:
                new_ids[_id] = len(new_vecs)
                new_vecs.append(vec)
                new_recs.append(rec)
                planned.append((pos, {**base, "_version": 1, "result": "created", "_seq_no": base_rows + len(new_vecs) - 1, "status": 201}))
            elif op == "create":
                out[pos] = {**base, "status": 409, "error": {"type": "version_conflict_engine_exception",
                                                             "reason": f"[{_id}]: version conflict, document already exists"}}
            elif row is None:                                 # second write to an _id inserted earlier in this request
                p0 = new_ids[_id]
                new_vecs[p0], new_recs[p0] = vec, rec
                planned.append((pos, {**base, "_version": 2, "result": "updated", "_seq_no": base_rows + p0, "status": 200}))
            else:
                upd[row] = (rec, vec)
                planned.append((pos, {**base, "_version": 2, "result": "updated", "_seq_no": row, "status": 200}))
        try:
            if new_vecs:
                idx.vectors.add(np.stack(new_vecs))
        except Exception as e:                                # nothing was appended: docstore untouched
            for pos, body in planned:
                out[pos] = {k: v for k, v in body.items() if k in ("_index", "_id")}
                out[pos].update({"status": 500, "error": {"type": "sqe_device_exception", "reason": str(e)}})
            return out
        for _id, p0 in new_ids.items():                       # the vector rows exist: so do their documents
            idx.row_of_id[_id] = base_rows + p0
        idx.sources.extend(new_recs)
        for p0, rec in enumerate(new_recs):
            _doc_add(doc_rows, rec["doc_id"], base_rows + p0)
        upd_failed = None
        try:
            if upd:
                rows = sorted(upd)
                idx.vectors.update(np.asarray(rows, np.int64), np.stack([upd[r][1] for r in rows]))
                for r in rows:
                    _key_changed(idx, r, upd[r][0]["doc_id"])
                    _text_changed(idx, r)
                    _fields.field_changed(idx, r)
                    if idx.sources[r] is not None:
                        _doc_remove(doc_rows, idx.sources[r]["doc_id"], r)
                    idx.sources[r] = upd[r][0]
                    _doc_add(doc_rows, upd[r][0]["doc_id"], r)
        except Exception as e:
            upd_failed = str(e)
        for pos, body in planned:
            if upd_failed is not None and body["result"] == "updated" and body["_seq_no"] < base_rows:
                out[pos] = {"_index": name, "_id": body["_id"], "status": 500,
                            "error": {"type": "sqe_device_exception", "reason": upd_failed}}
            else:
                out[pos] = body
    return out


def _delete_docs(client, name: str, docs, embed_dim: int = 0):
    """docs: [(slot, "delete", _id, None)] of one index -> per-document delete item bodies, in order (one device delete):
    200 "deleted", or 404 "not_found" as OpenSearch reports a missing document (not an error of the bulk call)."""
    idx = client.index(name)
    shards = {"total": 1, "successful": 1, "failed": 0}
    try:
        found = delete_documents(idx, [d[2] for d in docs])
    except Exception as e:
        return [{"_index": name, "_id": d[2], "status": 500, "error": {"type": "sqe_device_exception", "reason": str(e)}} for d in docs]
    return [{"_index": name, "_id": d[2], "_version": 1, "result": "deleted" if ok else "not_found",
             "_shards": shards if ok else {**shards, "successful": 0}, "_primary_term": 1, "status": 200 if ok else 404}
            for d, ok in zip(docs, found)]


def _names_text(clause) -> bool:
    """a ``match`` / ``match_phrase`` clause anywhere inside"""
    if isinstance(clause, dict):
        return any(key in ("match", "match_phrase") or _names_text(v) for key, v in clause.items())
    return isinstance(clause, list) and any(_names_text(v) for v in clause)


def _sort_route(query) -> bool:
    """A ``_search`` body with a ``sort`` key is a sorted search (no scoring, ``search_sorted``) when its query is absent,
    ``match_all``, one ``term`` / ``terms`` / ``range`` / ``exists`` / ``ids`` clause, or a ``bool`` that holds no ``match`` /
    ``match_phrase`` clause anywhere.  Every other query keeps its route and its treatment of ``sort``."""
    if query is None:
        return True
    if not isinstance(query, dict) or len(query) != 1:
        return False
    (kind, spec), = query.items()
    return kind in ("match_all", "term", "terms", "range", "exists", "ids") or (kind == "bool" and not _names_text(spec))


def _search_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], flt: Optional[Dict] = None):
    """One batched scan for the concurrent requests of one index: row b of ``vectors`` is request b's query
    (the reference sends row 0 only, main.py:355).  Exact cosine order, ``_score = 1 / (2 - cos)`` (what
    OpenSearchIndexer.search returns, with _id); request b gets its own first ``ks[b]`` hits.  ``flt``: the
    filter clause every request of the batch shares (the filtered search over the documents it selects)."""
    idx = client.index(name)
    kmax = max(ks)
    with idx.lock:
        if flt is None:
            cos, ids = idx.vectors.search(np.ascontiguousarray(vectors, dtype=np.float32), kmax)
        else:
            pred = field_predicate(idx, flt)          # a conjunction of field leaves: evaluated on the device, no id list
            deny = exclusion_rows(idx, flt) if pred is None and _can_exclude(idx) else None      # a clause that only excludes: the exclusion search
            if pred is not None:
                cos, ids = idx.vectors.search_where(np.ascontiguousarray(vectors, dtype=np.float32), kmax, pred)
            elif deny is not None:
                q = np.ascontiguousarray(vectors, dtype=np.float32)
                cos, ids = idx.vectors.search_excluding(q, kmax, [deny], np.zeros(q.shape[0], np.int32))
            else:
                cos, ids = idx.vectors.search(np.ascontiguousarray(vectors, dtype=np.float32), kmax,
                                              filter_ids=filter_rows(idx, flt))
        return _hits_of(idx, name, cos, ids, ks, fields, client.dim)


def _each_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], flts: List[Dict]):
    """One per-query filtered search for the concurrent filtered requests of one index: request b is answered over the
    documents its own clause ``flts[b]`` selects (resolved here, under ``idx.lock``; equal clauses share a list; the
    clauses that only exclude are answered together by the exclusion search)."""
    idx = client.index(name)
    with idx.lock:
        where = field_predicates(idx, flts)           # conjunctions of field leaves throughout: one search_where_each
        if where is not None:
            cos, ids = idx.vectors.search_where_each(np.ascontiguousarray(vectors, dtype=np.float32), max(ks), where[0], where[1])
        else:
            lists, loq, deny, doq = resolve_routes(idx, flts)
            cos, ids = search_resolved(idx, np.ascontiguousarray(vectors, dtype=np.float32), max(ks), lists, loq, deny, doq)
        return _hits_of(idx, name, cos, ids, ks, fields, client.dim)


def _hits_of(idx, name: str, cos: np.ndarray, ids: np.ndarray, ks: List[int], fields: List[str], dim: int):
    """Hit lists of a batched result (caller holds idx.lock): request b takes its first ks[b] valid rows."""
    rows_of = [[int(r) for r in ids[b][:ks[b]] if r >= 0] for b in range(len(ks))]
    flat = [r for rows in rows_of for r in rows]
    embs = idx.vectors.get_rows(flat) if flat else np.zeros((0, dim), np.float32)
    rev = getattr(idx, "_id_of_row", None)
    if rev is None or len(rev) != len(idx.row_of_id):
        rev = {row: os_id for os_id, row in idx.row_of_id.items()}
        idx._id_of_row = rev
    out, at = [], 0
    for b, rows in enumerate(rows_of):
        hits = []
        for j, row in enumerate(rows):
            src = idx.sources[row]
            hits.append({"_index": name, "_id": rev.get(row), "_score": float(1.0 / (2.0 - float(cos[b, j]))),
                         "_source": {**src, fields[b]: [float(x) for x in embs[at + j]]}})
        at += len(rows)
        out.append(hits)
    return out


def _range_hits_batch(client, name: str, vectors: np.ndarray, sizes: List[int], fields: List[str], min_cos: List[float]):
    """One radial search for the concurrent radial requests of one index: per-request floors, max_hits = the largest
    size.  Request b gets (its first ``sizes[b]`` hits, the exact number of rows at or above its floor)."""
    idx = client.index(name)
    with idx.lock:
        counts, cos, ids = idx.vectors.range_search(np.ascontiguousarray(vectors, dtype=np.float32),
                                                    np.asarray(min_cos, np.float32), max(sizes))
        hits = _hits_of(idx, name, cos, ids, sizes, fields, client.dim)
    return [(h, int(counts[b])) for b, h in enumerate(hits)]


def _collapse_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str]):
    """One collapsed search for the concurrent collapsed requests of one index (``collapse`` on ``doc_id``): request b gets
    its first ``ks[b]`` documents, each with its best chunk.  The keys of rows the device has none for yet go first."""
    idx = client.index(name)
    with idx.lock:
        push_keys(idx)
        cos, ids, _keys = idx.vectors.search_collapsed(np.ascontiguousarray(vectors, dtype=np.float32), max(ks))
        return _hits_of(idx, name, cos, ids, ks, fields, client.dim)


def _parse_ext_rerank(spec) -> str:
    """``"ext": {"rerank": {"query_context": {"query_text": "..."}}}`` -> the text every hit is scored against."""
    try:
        text = spec["query_context"]["query_text"]
    except (KeyError, TypeError):
        text = None
    if not isinstance(text, str):
        raise ValueError("ext.rerank is served as {'query_context': {'query_text': str}} only")
    return text


def _parse_ext_mmr(spec, k: int) -> Tuple[float, int]:
    """The ``mmr`` object of ``"ext": {"mmr": {"candidates": n, "diversity": d}}`` -> (lambda = 1 - d, candidates); both
    keys are optional (diversity 0.5, candidates 0 = automatic).  The Python keyword of ``OpenSearchIndexer.search`` is the
    contract; this body is the form OpenSearch is believed to take."""
    if not isinstance(spec, dict) or not set(spec) <= {"candidates", "diversity"}:
        raise ValueError("ext.mmr is served as {'candidates': depth, 'diversity': weight in [0, 1]} only")
    d = spec.get("diversity", 0.5)
    if isinstance(d, bool) or not isinstance(d, numbers.Real) or not 0.0 <= float(d) <= 1.0:
        raise ValueError(f"ext.mmr diversity must be a number in [0, 1], got {d!r}")
    return _check_mmr({"lambda": 1.0 - float(d), "candidates": spec.get("candidates", 0)}, k)


def _mmr_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], lams: List[float], n_cand: int):
    """One MMR search for the concurrent MMR requests of one index with equal depth ``n_cand`` (explicit: resolved per
    request by ``_SearchBatcher.search``, so no request's depth depends on its batch): per-request lambda, k = the
    largest k; request b gets its first ``ks[b]`` picks (the greedy choice is prefix-stable), in selection order."""
    idx = client.index(name)
    with idx.lock:
        cos, ids, _obj = idx.vectors.search_mmr(np.ascontiguousarray(vectors, dtype=np.float32), max(ks),
                                                lam=np.asarray(lams, np.float32), n_cand=n_cand)
        return _hits_of(idx, name, cos, ids, ks, fields, client.dim)


def _fused_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], ms: List[int], weights: List,
                      method: str, depth: int, c: int):
    """One fused search for the concurrent hybrid requests of one index with equal (k, method, depth, rank constant):
    request b is the logical query of its own ``ms[b]`` rows of ``vectors`` with its own ``weights[b]`` (None = all 1), so
    no request's answer depends on its batch.  Hits come in fused order; ``_score`` is the hit's best cosine mapped as for
    knn, ``fields._fused`` the fused score."""
    idx = client.index(name)
    offsets = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    w = None
    if any(v is not None for v in weights):
        w = np.concatenate([np.ones(m, np.float32) if v is None else np.asarray(v, np.float32) for m, v in zip(ms, weights)])
    with idx.lock:
        fused, ids, cos = idx.vectors.search_fused(np.ascontiguousarray(vectors, dtype=np.float32), ks[0], offsets=offsets, mode=method,
                                                   weights=w, depth=depth, rank_constant=c)
        out = _hits_of(idx, name, cos, ids, ks, fields, client.dim)
    for b, hits in enumerate(out):
        for j, hit in enumerate(hits):                    # the valid rows of a fused list are its first ones
            hit["fields"] = {"_fused": [float(fused[b, j])]}
    return out


def _text_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], terms: List[np.ndarray]):
    """One lexical search for the concurrent match requests of one index (``vectors`` holds placeholder rows): request b
    gets its first ``ks[b]`` hits, ``_score`` the BM25 score."""
    idx = client.index(name)
    with idx.lock:
        lex = push_text(idx)
        score, ids = lex.search(terms, max(ks))
        out = _hits_of(idx, name, np.zeros_like(score), ids, ks, fields, client.dim)      # (the cosine mapping does not apply)
    for b, hits in enumerate(out):
        for j, hit in enumerate(hits):                    # the valid rows of a list are its first ones
            hit["_score"] = float(score[b, j])
    return out


def _bool_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], queries: List[tuple], phrase: bool = False):
    """One boolean lexical search (``LexicalIndex.search_bool``) for the concurrent boolean text requests of one index:
    ``queries[b]`` = (terms, roles, min_should); hits and ``_score`` as ``_text_hits_batch`` gives them.  ``phrase``: the
    requests are clause requests, (clauses, roles, min_should), answered by one ``search_phrase``."""
    idx = client.index(name)
    with idx.lock:
        lex = push_text(idx)
        search = lex.search_phrase if phrase else lex.search_bool
        score, ids = search([q[0] for q in queries], [q[1] for q in queries], max(ks), [q[2] for q in queries])
        out = _hits_of(idx, name, np.zeros_like(score), ids, ks, fields, client.dim)
    for b, hits in enumerate(out):
        for j, hit in enumerate(hits):
            hit["_score"] = float(score[b, j])
    return out


def _count_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], queries: List[tuple], phrase: bool = False):
    """One counting call (``LexicalIndex.count``; ``count_phrase`` for clause requests) for the concurrent _count requests
    with a text query of one index."""
    idx = client.index(name)
    with idx.lock:
        lex = push_text(idx)
        counts = (lex.count_phrase if phrase else lex.count)([q[0] for q in queries], [q[1] for q in queries], [q[2] for q in queries])
    return [int(c) for c in counts]


def _hybrid_hits_batch(client, name: str, vectors: np.ndarray, ks: List[int], fields: List[str], ms: List[int], weights: List,
                       terms: List[np.ndarray], depth: int, c: int):
    """One hybrid search for the concurrent hybrid requests with a match of one index with equal (k, depth, rank constant):
    request b is the group of its own ``ms[b]`` rows of ``vectors`` and its own lexical query ``terms[b]``; ``weights[b]``
    (None = all 1) holds its sub-queries' weights, then its lexical list's.  Hits come in fused order; ``_score`` is the hit's
    best cosine mapped as for knn (0 for a hit only the lexical list holds), ``fields._fused`` the fused score and
    ``fields._bm25`` the BM25 score (absent for a hit the lexical list does not hold)."""
    idx = client.index(name)
    offsets = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    w = None
    if any(v is not None for v in weights):
        w = np.concatenate([np.ones(m, np.float32) if v is None else np.asarray(v[:m], np.float32) for m, v in zip(ms, weights)] +
                           [np.array([1.0 if v is None else v[m] for m, v in zip(ms, weights)], np.float32)])
    with idx.lock:
        lex = push_text(idx)
        q = np.ascontiguousarray(vectors, dtype=np.float32).reshape(-1, client.dim)
        fused, ids, cos, bm25 = idx.vectors.search_hybrid(lex, q, terms, ks[0], offsets=offsets, weights=w, depth=depth, rank_constant=c)
        out = _hits_of(idx, name, cos, ids, ks, fields, client.dim)
    for b, hits in enumerate(out):
        for j, hit in enumerate(hits):
            hit["fields"] = {"_fused": [float(fused[b, j])]}
            if np.isfinite(bm25[b, j]):
                hit["fields"]["_bm25"] = [float(bm25[b, j])]
    return out


def _search_hits(client, name: str, vector: np.ndarray, k: int, field: str):
    """The un-batched form (one request): row 0 only."""
    return _search_hits_batch(client, name, vector[0:1], [k], [field])[0]


def main(argv=None) -> None:
    import argparse

    import uvicorn

    from .retrieval import GpuSearchClient, default_context
    from .weights import embedder_from_local, reranker_from_local

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", help="local Hugging Face directory or GGUF file of the embedding model (never a model name)")
    ap.add_argument("--reranker", help="local Hugging Face directory of a BERT cross-encoder (BertForSequenceClassification): "
                                       "_search then honours ext.rerank")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=9200)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--load", help="directory with indexes written by GpuSearchClient.save_index")
    ap.add_argument("--per-query-filters", action="store_true",
                    help="concurrent filtered _search requests of an index share one device call whatever their filters")
    args = ap.parse_args(argv)
    ctx = default_context()
    client = GpuSearchClient(ctx, dim=args.dim)
    if args.load:
        import glob
        import os
        for p in glob.glob(os.path.join(args.load, "*.sqeidx")):
            client.load_index(os.path.basename(p)[:-len(".sqeidx")], args.load)
    embedder = embedder_from_local(ctx, args.model) if args.model else None
    if embedder is not None:                              # the model's own WordPiece vocabulary analyses the text field
        _retrieval.configure_analyzer(embedder.tokenizer)
    reranker = reranker_from_local(ctx, args.reranker) if args.reranker else None
    uvicorn.run(create_app(client, embedder, args.dim, per_query_filters=args.per_query_filters, reranker=reranker),
                host=args.host, port=args.port, log_level="warning")


if __name__ == "__main__":
    main()
