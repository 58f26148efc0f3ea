"""``ext.rerank`` of the HTTP shim over the real GPU index and a real cross-encoder: a shim started with a reranker reorders the
hits of a ``_search`` response by the model's score (``_score`` and ``max_score`` follow); a shim started without one answers
the same body as it always did.  GPU only."""
import json

import numpy as np
import pytest
from fastapi.testclient import TestClient

from oracle import wordpiece as WP
from tests import encoder_stage_cases as SC
from tests import rerank_reference as RR
from tests.test_oracle_wordpiece import SAMPLES

pytestmark = pytest.mark.gpu

INDEX, DIM = "medical-search-index", 1024


def _fill(c, xn, texts):
    assert c.put(f"/{INDEX}", json={"mappings": {"properties": {"embedding": {
        "type": "knn_vector", "dimension": DIM, "method": {"space_type": "cosinesimil"}}}}}).status_code == 200
    lines = []
    for i, t in enumerate(texts):
        lines.append(json.dumps({"index": {"_index": INDEX, "_id": f"doc_{i}"}}))
        lines.append(json.dumps({"doc_id": f"doc{i}", "text": t, "embedding": xn[i].tolist()}))
    assert c.post("/_bulk", content=("\n".join(lines) + "\n").encode()).json()["errors"] is False


def test_ext_rerank_reorders_only_when_a_reranker_is_loaded():
    from semantic_query_engine_amd import Context, shim
    from semantic_query_engine_amd.retrieval import GpuSearchClient, Reranker
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    ctx = Context(0)
    vocab = WP.synthetic_vocab(SAMPLES, size=1500)
    cfg = SC.config(hidden=256, inter=1024, heads=4, layers=2, vocab_size=len(vocab), max_pos=64)
    rr = Reranker(RR.make_encoder(ctx, cfg, RR.weights(cfg, 1, seed=13)), WordPieceTokenizer(vocab_text="\n".join(vocab) + "\n"),
                  max_len=64, max_query=12)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((30, DIM)).astype(np.float32)
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    texts = [SAMPLES[i % len(SAMPLES)] + f" {i}" for i in range(30)]
    q = xn[4] + 0.5 * xn[9]
    body = {"size": 6, "query": {"knn": {"embedding": {"vector": (q / np.linalg.norm(q)).tolist(), "k": 6}}}}
    ext = dict(body, ext={"rerank": {"query_context": {"query_text": "which treatment helps"}}})

    # (one event loop per client, kept for all its requests: the shim's search batcher lives on it)
    with TestClient(shim.create_app(GpuSearchClient(ctx, dim=DIM), None, DIM)) as plain:
        _fill(plain, xn, texts)
        base = plain.post(f"/{INDEX}/_search", json=body).json()["hits"]
        ignored = plain.post(f"/{INDEX}/_search", json=ext).json()["hits"]
    assert ignored == base and base["hits"][0]["_id"] == "doc_4"          # without a reranker ext.rerank is ignored, as any ext

    with TestClient(shim.create_app(GpuSearchClient(ctx, dim=DIM), None, DIM, reranker=rr)) as c:
        _fill(c, xn, texts)
        assert c.post(f"/{INDEX}/_search", json=body).json()["hits"] == base      # no ext: the same response
        got = c.post(f"/{INDEX}/_search", json=ext).json()["hits"]
        bad = c.post(f"/{INDEX}/_search", json=dict(body, ext={"rerank": {"query_context": {}}}))
    scores = rr.score("which treatment helps", [h["_source"]["text"] for h in base["hits"]])
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    assert len(set(scores.tolist())) == 6 and order.tolist() != list(range(6)), "the model was to disagree with the cosine order"
    assert [h["_id"] for h in got["hits"]] == [base["hits"][j]["_id"] for j in order]
    assert [h["_score"] for h in got["hits"]] == [float(scores[j]) for j in order]
    assert got["max_score"] == float(scores.max()) == got["hits"][0]["_score"] and got["total"] == base["total"]
    assert [h["_source"] for h in got["hits"]] == [base["hits"][j]["_source"] for j in order]
    assert bad.status_code == 400 and bad.json()["error"]["type"] == "parsing_exception"
