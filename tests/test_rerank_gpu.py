"""Cross-encoder scoring end to end against the float64 forward of tests/rerank_reference.py.  GPU only.

CLS rows: cosine >= 0.999 per row, the bar tests/test_encoder_gpu.py sets for the same quantity.  Logits: inside
RR.logit_bound_e2e, which is derived (tanh is 1-Lipschitz): ||w_c,l|| sigma_max(W_p) ||cls_gpu - cls_ref|| plus the fp32 bounds
of the two head stages.  Ordering: any two pairs whose reference logits differ by more than twice that bound come out in the
reference order.  The bound needs the CLS rows the GPU computed, so before the GPU call the test checks on the CPU that the
seed separates at least 10 of the 15 pair comparisons at the drift a CLS cosine of 0.99999 gives (PREDICTED_COS: what the bf16
encoder reaches on these models, far inside the 0.999 bar); after the call it asserts the same count under the real bound, so
the ordering check can never pass for want of pairs to compare."""
import numpy as np
import pytest

from oracle import wordpiece as WP
from tests import encoder_stage_cases as SC
from tests import rerank_reference as RR
from tests.test_oracle_wordpiece import SAMPLES

pytestmark = pytest.mark.gpu

PREDICTED_COS = 0.99999
SMALL = dict(hidden=256, inter=1024, heads=4, layers=4, max_pos=128)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


def _cos(a, b):
    return float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))


def _separated(logits, bound):
    """pairs (i, j), i < j, of column-0 logits further apart than twice the larger of their bounds"""
    n = logits.shape[0]
    return [(i, j) for i in range(n) for j in range(i + 1, n)
            if abs(logits[i, 0] - logits[j, 0]) > 2.0 * max(bound[i, 0], bound[j, 0])]


def _predicted_bound(w, ref):
    """RR.logit_bound_e2e at the CLS drift PREDICTED_COS gives, from CPU-side quantities only"""
    drift = np.linalg.norm(ref["cls"], axis=1) * np.sqrt(2.0 * (1.0 - PREDICTED_COS))
    cls_like = ref["cls"] + drift[:, None] * np.eye(ref["cls"].shape[1])[0][None]     # any rows at that distance
    return RR.logit_bound_e2e(w, cls_like, ref["cls"], ref["pooled"])


def _pairs(cfg, B, S, seed):
    """B pairs of full length, the segment boundary at a different place in each; every pair draws its tokens from its own
    three ids (texts about different things), so the CLS rows -- and with them the scores -- differ from pair to pair"""
    ids, types, lens = RR.pair_batch(cfg, B, S, 3 + 4 * np.arange(B), seed=seed)
    rng = np.random.default_rng(seed)
    for b in range(B):
        ids[b] = rng.choice(rng.integers(0, cfg.vocab_size, 3), S)
    return ids, types, lens


def _measure(enc, w, cfg, ids, types, lens, ref):
    """one scoring call -> (logits, per-row CLS cosine, logit bound, separated pairs), printed before anything is asserted"""
    B, S = ids.shape
    logits = enc.score_ids(ids, types, lens)
    cls, pooled, _ = RR.read_head(enc, B, cfg.hidden, 1)
    cs = [_cos(cls[b], ref["cls"][b]) for b in range(B)]
    bound = RR.logit_bound_e2e(w, cls, ref["cls"], pooled)
    err = np.abs(logits - ref["logits"])
    pairs = _separated(ref["logits"], bound)
    print(f"E2E hidden {cfg.hidden} layers {cfg.layers} B {B} S {S}: min CLS cosine {min(cs):.7f}, worst |logit error| / bound "
          f"{float((err / bound).max()):.4f} (error {err.max():.4f}, bound {bound.max():.3f}, logits {np.round(ref['logits'][:, 0], 2)}), "
          f"separated pairs {len(pairs)}", flush=True)
    return logits, cs, bound, pairs


# seeds: the first whose batches separate at least 10 of the 15 pairs at both S (searched on the CPU with _predicted_bound)
@pytest.mark.parametrize("c,B,S,seed", [(SMALL, 6, 32, 233), (SMALL, 6, 64, 233),
                                        (dict(hidden=1024, inter=4096, heads=16, layers=2, max_pos=128), 4, 128, 12)],
                         ids=["H256-S32", "H256-S64", "H1024-S128"])
def test_cls_logits_and_order(ctx, c, B, S, seed):
    cfg = SC.config(**c)
    w = RR.weights(cfg, 1, seed)
    ids, types, lens = _pairs(cfg, B, S, seed)
    ref = RR.forward(w, cfg, ids, types, lens)
    predicted = _separated(ref["logits"], _predicted_bound(w, ref))
    if B == 6:
        assert len(predicted) >= 10, f"seed {seed} separates only {len(predicted)} of 15 pairs"
    logits, cs, bound, pairs = _measure(RR.make_encoder(ctx, cfg, w), w, cfg, ids, types, lens, ref)
    assert min(cs) >= 0.999, cs
    assert (np.abs(logits - ref["logits"]) <= bound).all(), (logits, ref["logits"], bound)
    if B == 6:
        assert len(pairs) >= 10, (len(pairs), bound)
    for i, j in pairs:
        assert (logits[i, 0] > logits[j, 0]) == (ref["logits"][i, 0] > ref["logits"][j, 0]), (i, j)


def test_embedding_and_scoring_share_an_encoder_without_bleed(ctx):
    from semantic_query_engine_amd._native import SqeError
    from semantic_query_engine_amd.encoder import BertEncoder
    cfg = SC.config(**SMALL)
    w = RR.weights(cfg, 1, seed=11)
    enc = RR.make_encoder(ctx, cfg, w)
    ids, types, lens = RR.pair_batch(cfg, 6, 32, 3 + 4 * np.arange(6), seed=11)
    e1 = enc.encode_ids(ids, lens)
    e2 = enc.encode_ids(ids, lens)
    assert enc.state()["mode"] == "captured"
    s1 = enc.score_ids(ids, types, lens)
    assert enc.state()["mode"] == "eager", "a scoring call replayed the embedding call's graph"
    s2 = enc.score_ids(ids, types, lens)
    assert enc.state()["mode"] == "captured"
    e3 = enc.encode_ids(ids, lens)
    assert enc.state()["mode"] == "replayed", "the scoring calls took the embedding call's place in the graph cache"
    assert np.array_equal(e1.view(np.uint32), e2.view(np.uint32)) and np.array_equal(e1.view(np.uint32), e3.view(np.uint32))
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    assert np.array_equal(enc.score_ids(ids, types, lens).view(np.uint32), s1.view(np.uint32)) and enc.state()["mode"] == "replayed"
    # the embedding is the one an encoder without a head computes
    plain = SC.make_encoder(ctx, cfg, {n: v for n, v in w.items() if n not in RR.HEAD_TENSORS})
    assert plain.labels == 0
    assert np.array_equal(plain.encode_ids(ids, lens).view(np.uint32), e1.view(np.uint32))
    with pytest.raises(SqeError) as e:
        plain.score_ids(ids, types, lens)
    assert e.value.code == -4                                     # SQE_ERR_STATE
    # a partial head fails finalize
    part = BertEncoder(ctx, vocab_size=cfg.vocab_size, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads, inter=cfg.inter,
                       max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps)
    for n, v in w.items():
        if n != "classifier.bias":
            part.load_tensor(n, v)
    with pytest.raises(SqeError) as e:
        part.finalize()
    assert e.value.code == -4 and "head" in str(e.value)
    with pytest.raises(ValueError):
        part.load_weights({n: v for n, v in w.items() if n != "classifier.bias"}, head=True)
    # without head=True a classification checkpoint loads as an embedder: pooler.* and classifier.* are passed over
    trunk = BertEncoder(ctx, vocab_size=cfg.vocab_size, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads, inter=cfg.inter,
                        max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps)
    trunk.load_weights(w)
    assert trunk.labels == 0
    assert np.array_equal(trunk.encode_ids(ids, lens).view(np.uint32), e1.view(np.uint32))


# ------------------------------------------------------------------------------------------------ Reranker and search
class Recorder:
    """An encoder that keeps, for every scoring call, its inputs and the CLS rows, pooled rows and logits the GPU held."""

    def __init__(self, enc):
        self.enc, self.cfg, self.calls = enc, enc.cfg, []

    @property
    def labels(self):
        return self.enc.labels

    def score_ids(self, ids, types, lens):
        out = self.enc.score_ids(ids, types, lens)
        cls, pooled, _ = RR.read_head(self.enc, ids.shape[0], self.cfg["hidden"], out.shape[1])
        self.calls.append((ids.copy(), types.copy(), lens.copy(), cls, pooled, out.copy()))
        return out


def _bounds(rec, w, cfg):
    """per recorded pair, in call order: (reference logit, bound, GPU logit)"""
    rows = []
    for ids, types, lens, cls, pooled, out in rec.calls:
        ref = RR.forward(w, cfg, ids, types, lens)
        bound = RR.logit_bound_e2e(w, cls, ref["cls"], pooled)
        rows += [(ref["logits"][b, 0], bound[b, 0], float(out[b, 0])) for b in range(ids.shape[0])]
    return np.array(rows)


@pytest.fixture(scope="module")
def reranker(ctx):
    from semantic_query_engine_amd.retrieval import Reranker
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    vocab = WP.synthetic_vocab(SAMPLES, size=1500)
    cfg = SC.config(vocab_size=len(vocab), **SMALL)
    w = RR.weights(cfg, 1, seed=13, mixing=True)           # the scores are to depend on the text
    rec = Recorder(RR.make_encoder(ctx, cfg, w))
    return Reranker(rec, WordPieceTokenizer(vocab_text="\n".join(vocab) + "\n"), max_len=64, max_query=12), rec, w, cfg


def _texts(n, seed):
    words = sorted({x for s in SAMPLES for x in s.split()})
    rng = np.random.default_rng(seed)
    return [" ".join(rng.choice(words, int(rng.integers(1, 14)))) for _ in range(n)]


def test_reranker_batches_equal_single_calls(reranker):
    rr, rec, w, cfg = reranker
    texts = _texts(70, 1)
    texts[3] = ""
    rec.calls.clear()
    batched = rr.score("which treatment helps patients", texts)
    assert [c[0].shape[0] for c in rec.calls] == [64, 6] and batched.shape == (70,) and batched.dtype == np.float32
    assert all(c[0].shape[1] % 16 == 0 and c[0].shape[1] <= 64 for c in rec.calls)
    rows = _bounds(rec, w, cfg)
    assert np.array_equal(rows[:, 2].astype(np.float32), batched)
    assert (np.abs(rows[:, 2] - rows[:, 0]) <= rows[:, 1]).all()
    rec.calls.clear()
    # one call per text, all 70: rows 64 .. 69 went through the short second batch
    single = np.array([rr.score("which treatment helps patients", [t])[0] for t in texts])
    assert [c[0].shape[0] for c in rec.calls] == [1] * 70
    one = _bounds(rec, w, cfg)
    assert (np.abs(one[:, 2] - one[:, 0]) <= one[:, 1]).all()
    assert np.abs(one[:, 0] - rows[:, 0]).max() <= 1e-9             # the same pairs: padding changes nothing in float64
    # ... which proves which text each row held only where the texts score apart (a few thousandths at the least here)
    refs = np.round(one[:, 0], 6)
    assert len(set(refs[64:])) == 6 and not set(refs[64:]) & set(refs[:64]), \
        "the texts of the second batch were to score unlike each other and unlike every text of the first"
    gap = np.abs(single - batched)
    print(f"RERANKER batch against single calls: worst gap {gap.max():.4f} (second batch {gap[64:].max():.4f}), "
          f"allowed {(one[:, 1] + rows[:, 1]).min():.3f} and up")
    assert (gap <= one[:, 1] + rows[:, 1]).all()


def test_search_rerank_returns_the_reference_order(ctx, reranker):
    """The separation condition is met by the choice of documents below and asserted under the bound the call itself gives
    (measured on an MI355X: steps of 11 to 12 between the first four reference scores, bounds of 3 to 5 per document)."""
    from semantic_query_engine_amd import retrieval as RT
    rr, rec, w, cfg = reranker
    query_text, dim, k, n = "does the treatment reduce pain", 1024, 3, 8
    # 8 documents near the query vector (cosine falling with their number), 32 far from it
    rng = np.random.default_rng(2)
    q = rng.standard_normal(dim).astype(np.float32)
    q /= np.linalg.norm(q)
    noise = rng.standard_normal((40, dim)).astype(np.float32)
    noise -= (noise @ q)[:, None] * q
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    c = np.r_[np.linspace(0.9, 0.6, n), np.full(40 - n, 0.1)].astype(np.float32)[:, None]
    x = c * q + np.sqrt(1 - c * c) * noise
    # their texts, from 300 candidates: the four that score lowest, and four whose reference scores step down evenly from the
    # best to just above those (steps of about 11.6; twice the logit bound is 6 to 10); retrieval order and score order are unrelated
    pool = _texts(300, 3)
    ids, types, lens = rr.tokenizer.encode_pairs([query_text] * len(pool), pool, 64, 12)
    ref = RR.forward(w, cfg, ids, types, lens)["logits"][:, 0]
    low = [int(i) for i in np.argsort(ref)[:n - 4]]
    steps = [int(np.abs(ref - t).argmin()) for t in np.linspace(ref.max(), ref[low].max() + 1.0, 4)]
    assert len(set(steps + low)) == n
    chosen = steps + low
    texts = [pool[i] for i in np.random.default_rng(4).permutation(chosen)] + _texts(40 - n, 5)
    want = sorted(range(n), key=lambda i: -ref[pool.index(texts[i])])[:k]
    ix = RT.OpenSearchIndexer(RT.GpuSearchClient(ctx, dim=dim), "rerank-idx")
    ix.add_embeddings(x, [{"doc_id": f"D{i}", "text": t} for i, t in enumerate(texts)])
    RT.configure_reranker(rr)
    try:
        rec.calls.clear()
        hits = ix.search(q[None], k=k, rerank={"query_text": query_text, "candidates": n})
    finally:
        RT.configure_reranker(None)
    assert len(rec.calls) == 1 and rec.calls[0][0].shape[0] == n
    rows = _bounds(rec, w, cfg)                                    # the 8 retrieved, in retrieval order = document number
    assert (np.abs(rows[:, 2] - rows[:, 0]) <= rows[:, 1]).all()
    order = np.argsort(-rows[:, 0])
    gaps = rows[order[:k], 0] - rows[order[1:k + 1], 0]
    assert (gaps > 2.0 * rows[:, 1].max()).all(), "the documents were to be separated by more than twice the bound"
    assert order[:k].tolist() == want
    assert [h[0]["doc_id"] for h in hits] == [f"D{i}" for i in want]
    assert [h[1] for h in hits] == [float(np.float32(rows[i, 2])) for i in want]       # the model's scores
    assert [h[0]["text"] for h in hits] == [texts[i] for i in want]
