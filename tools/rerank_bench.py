#!/usr/bin/env python3
"""Cost of cross-encoder scoring (sqe_encode_pairs_device) on the MI355X against the embedding forward pass it extends
(sqe_encode_device, unchanged by the head): BERT-large, random weights, one label.

Per shape B x S, in ONE process, after a warm-up of each call at that shape, the two calls take turns inside every repeat;
each is timed with device events on the stream both run on (median and range of `--repeats` rounds of `--iters` calls):

  score_ms    sqe_encode_pairs_device: embedding with segment ids, the 24 layers, pooling LayerNorm, pooler, classifier
  encode_ms   sqe_encode_device at the same B and S
  ratio       score_ms / encode_ms

and, once, `Reranker.score` of 64 passages of about 512 words against one query, wall clock, tokenisation included
(request_ms: what a reranked request pays on top of its search).  The head kernels' own time comes from a separate
    rocprofv3 --kernel-trace --stats -- python tools/rerank_bench.py --shapes 64x512 --repeats 2 --no-request
usage (GPU box): python tools/rerank_bench.py [--shapes 16x128,...] [--out profiles/rerank/rerank_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bench_configs import BERT_LARGE, random_bert_weights
from semantic_query_engine_amd import Context
from semantic_query_engine_amd.encoder import BertEncoder
from semantic_query_engine_amd.retrieval import Reranker
from semantic_query_engine_amd.tokenizer import WordPieceTokenizer

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="16x128,64x128,256x128,16x512,64x512,256x512")
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-request", action="store_true")
ap.add_argument("--out", default="")
ARGS = ap.parse_args()

dev = torch.device("cuda", 0)
ctx = Context(0)
stream = torch.cuda.Stream()                  # both calls and the events that time them go on this stream
torch.cuda.set_stream(stream)
ctx.set_stream(stream.cuda_stream)
H = BERT_LARGE["hidden"]
w = random_bert_weights()
rng = np.random.default_rng(1)
w["pooler.dense.weight"] = (rng.standard_normal((H, H)) * 2.0 / np.sqrt(H)).astype(np.float32)
w["pooler.dense.bias"] = np.zeros(H, np.float32)
w["classifier.weight"] = rng.standard_normal((1, H)).astype(np.float32)
w["classifier.bias"] = np.zeros(1, np.float32)
enc = BertEncoder(ctx)
enc.load_weights(w, head=True)
out = open(ARGS.out, "a") if ARGS.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def device_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


for shape in ARGS.shapes.split(","):
    B, S = (int(v) for v in shape.split("x"))
    g = torch.Generator(device=dev).manual_seed(S + B)
    ids = torch.randint(1000, 30000, (B, S), generator=g, device=dev, dtype=torch.int32)
    types = (torch.arange(S, device=dev)[None, :] >= 24).to(torch.int32).repeat(B, 1).contiguous()
    lens = torch.full((B,), S, device=dev, dtype=torch.int32)
    emb = torch.empty((B, H), device=dev)
    logits = torch.empty((B, 1), device=dev)
    score = lambda: enc.score_ids_device(ids.data_ptr(), types.data_ptr(), lens.data_ptr(), B, S, logits.data_ptr())
    encode = lambda: enc.encode_ids_device(ids.data_ptr(), lens.data_ptr(), B, S, emb.data_ptr())
    for fn in (score, encode, score, encode, score, encode):     # warm-up: the third call of a shape replays its graph
        fn()
    torch.cuda.synchronize()
    ts, te = [], []
    for _ in range(ARGS.repeats):
        ts.append(device_ms(score, ARGS.iters))
        te.append(device_ms(encode, ARGS.iters))
    ms, me = statistics.median(ts), statistics.median(te)
    emit({"B": B, "S": S, "score_ms": round(ms, 4), "score_range": [round(min(ts), 4), round(max(ts), 4)],
          "encode_ms": round(me, 4), "encode_range": [round(min(te), 4), round(max(te), 4)], "ratio": round(ms / me, 4),
          "iters": ARGS.iters, "repeats": ARGS.repeats, "finite": bool(torch.isfinite(logits).all())})

if not ARGS.no_request:
    # a vocabulary of BERT's size whose words are t0 .. tN: one word piece per word
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += [f"t{i}" for i in range(BERT_LARGE["vocab_size"] - len(vocab))]
    rr = Reranker(enc, WordPieceTokenizer(vocab_text="\n".join(vocab) + "\n"))
    words = rng.integers(0, 30000, (64, 512))
    passages = [" ".join(f"t{v}" for v in row) for row in words]
    query = " ".join(f"t{v}" for v in rng.integers(0, 30000, 12))
    rr.score(query, passages)
    times = []
    for _ in range(ARGS.repeats):
        t0 = time.perf_counter()
        s = rr.score(query, passages)
        times.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    rr.tokenizer.encode_pairs([query] * 64, passages, 512, 64)
    tok_ms = (time.perf_counter() - t0) * 1e3
    emit({"request": "Reranker.score, 64 passages x 512 words", "request_ms": round(statistics.median(times), 3),
          "request_range": [round(min(times), 3), round(max(times), 3)], "tokenize_ms": round(tok_ms, 3),
          "finite": bool(np.isfinite(s).all())})
