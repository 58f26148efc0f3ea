"""Shared by the rerank tests (helper, not a test): a float64 BERT cross-encoder forward pass -- per-token type rows in the
embedding sum, the encoder layers, then the classification head (pooler, tanh, classifier) -- plus the weights, batches and
bounds those tests use.  oracle/bert.py: bert_encode adds type row 0 only, so the forward is restated here from that
module's stage_* functions; tests/test_rerank_reference_cpu.py holds it against transformers.BertForSequenceClassification.

Head weights are drawn so that the logits spread (pooler std 2 / sqrt(H), classifier std 1: default initialisation gives
logits near 0.02, which ranks nothing) and stay fp32; the encoder matrices are bf16 numbers as oracle.bert.random_weights
makes them, so the GPU encoder and this reference hold the same parameters.

BOUNDS (the head is fp32 on fp32: tests/encoder_stage_cases.py has the rounding model).
  pooled   |got - tanh(ref)| <= bound_linear_f32(mag, H) + 2^-20   tanh is 1-Lipschitz, so the fp32 error of the sum passes
           through at most unchanged; the result is at most 1 in magnitude, where 2^-20 is 8 fp32 ulps
  logits   |got - ref| <= bound_linear_f32(mag, H)                 on the pooled rows the GPU itself holds
  end to end, logits against the float64 forward: head(cls_gpu) differs from head(cls_ref) by at most
           ||w_c,l||_2 sigma_max(W_p) ||cls_gpu - cls_ref||_2 (tanh 1-Lipschitz), and the GPU's head differs from the float64
           head on ITS cls rows by at most sum_j |w_c,l,j| pooled_bound_j + logit_bound: logit_bound_e2e is the sum."""
import numpy as np

from oracle import bert as OB
from semantic_query_engine_amd.encoder import HEAD_TENSORS
from tests import encoder_stage_cases as SC

TANH_TOL = 2.0 ** -20


def weights(cfg: OB.BertCfg, labels: int, seed: int, mixing: bool = False):
    """name -> fp32 NumPy array: SC.weights(cfg, seed) plus the four head tensors.
    mixing: value and attention-output weights x 8, query and key x 4 (powers of two: still bf16 numbers).  With plain
    N(0, 0.02) weights the CLS row is little more than the residual of its own token, [CLS], and every tokenised text scores
    alike (a range of 3 over 200 texts against a logit bound of 4 to 6); with these the row depends on what the text says
    (a range of 38 over the same texts) while the encoder's drift, and so the bound, stays where it was (3 to 5).  Sharper
    attention (query x 16, key x 8) spreads the scores further but multiplies the drift: bounds of 40 to 210."""
    w = SC.weights(cfg, seed)
    if mixing:
        for l in range(cfg.layers):
            p = f"encoder.layer.{l}.attention."
            for n, f in (("self.value", 8.0), ("output.dense", 8.0), ("self.query", 4.0), ("self.key", 4.0)):
                w[p + n + ".weight"] *= np.float32(f)
    rng = np.random.default_rng(seed * 31 + labels)
    H = cfg.hidden
    w["pooler.dense.weight"] = (rng.standard_normal((H, H)) * 2.0 / np.sqrt(H)).astype(np.float32)
    w["pooler.dense.bias"] = (rng.standard_normal(H) * 0.1).astype(np.float32)
    w["classifier.weight"] = rng.standard_normal((labels, H)).astype(np.float32)
    w["classifier.bias"] = rng.standard_normal(labels).astype(np.float32)
    return w


def pair_batch(cfg: OB.BertCfg, B: int, S: int, boundaries, lens=None, seed: int = 0):
    """ids, types, lens: row b is type 0 before position boundaries[b] and 1 from there to lens[b] - 1 (0 in the padding, as
    the tokenizer leaves it); a boundary >= lens[b] gives a row of type 0 only."""
    ids, lens = SC.batch(cfg, B, S, lens, seed)
    pos = np.arange(S)[None, :]
    types = ((pos >= np.asarray(boundaries)[:, None]) & (pos < lens[:, None])).astype(np.int32)
    return ids, types, lens


def embed(w, cfg: OB.BertCfg, ids, types):
    """float64 [B, S, H]: LayerNorm(word[id] + pos[s] + type[types[b][s]]); types None: row 0 everywhere."""
    f = lambda n: np.asarray(w[n], np.float64)
    ids = np.clip(np.asarray(ids), 0, cfg.vocab_size - 1)
    types = np.zeros_like(ids) if types is None else np.clip(np.asarray(types), 0, cfg.type_vocab - 1)
    x = (f("embeddings.word_embeddings.weight")[ids] + f("embeddings.position_embeddings.weight")[:ids.shape[1]][None]
         + f("embeddings.token_type_embeddings.weight")[types])
    return OB.stage_ln(x, f("embeddings.LayerNorm.weight"), f("embeddings.LayerNorm.bias"), cfg.ln_eps)


def head(w, cls):
    """cls [B, H] -> (pooled, pooled_mag, logits, logits_mag), float64; the mags are those of OB.stage_linear."""
    z, mag_p = OB.stage_linear(cls, w["pooler.dense.weight"], w["pooler.dense.bias"])
    pooled = np.tanh(z)
    return (pooled, mag_p) + classify(w, pooled)


def classify(w, pooled):
    return OB.stage_linear(pooled, w["classifier.weight"], w["classifier.bias"])


def forward(w, cfg: OB.BertCfg, ids, types, lens):
    """The whole cross-encoder in float64 -> dict(cls [B, H], pooled [B, H], logits [B, L])."""
    B, S = np.asarray(ids).shape
    H = cfg.hidden
    x = embed(w, cfg, ids, types).reshape(B * S, H)
    for l in range(cfg.layers):
        L = SC.layer_weights(w, l)
        qkv, _ = OB.stage_linear(x, L.Wqkv, L.bqkv)
        att, _ = OB.stage_attention(qkv.reshape(B, S, 3 * H), lens, cfg.heads)
        pre, _ = OB.stage_linear(att.reshape(B * S, H), L.Wo, L.bo, resid=x)
        x1 = OB.stage_ln(pre, L.g1, L.b1n, cfg.ln_eps)
        z, _ = OB.stage_linear(x1, L.W1, L.b1)
        pre, _ = OB.stage_linear(OB.stage_gelu(z), L.W2, L.b2, resid=x1)
        x = OB.stage_ln(pre, L.g2, L.b2n, cfg.ln_eps)
    cls = x.reshape(B, S, H)[:, 0]
    pooled, _, logits, _ = head(w, cls)
    return dict(cls=cls, pooled=pooled, logits=logits)


def head_ratios(w, cls_gpu, pooled_gpu, logits_gpu):
    """Worst |got - ref| / bound of the two head stages, each on the input the GPU itself held."""
    H = cls_gpu.shape[1]
    pooled, mag_p, _, _ = head(w, cls_gpu)
    logits, mag_c = classify(w, pooled_gpu)
    return dict(pooled=SC.worst_ratio(pooled_gpu, pooled, SC.bound_linear_f32(mag_p, H) + TANH_TOL),
                logits=SC.worst_ratio(logits_gpu, logits, SC.bound_linear_f32(mag_c, H)))


def logit_bound_e2e(w, cls_gpu, cls_ref, pooled_gpu):
    """[B, L]: how far the GPU's logits may lie from forward()'s (module docstring)."""
    H = cls_gpu.shape[1]
    Wc = np.asarray(w["classifier.weight"], np.float64)
    sigma = np.linalg.norm(np.asarray(w["pooler.dense.weight"], np.float64), 2)
    drift = np.linalg.norm(Wc, axis=1)[None, :] * sigma * np.linalg.norm(cls_gpu - cls_ref, axis=1)[:, None]
    _, mag_p, _, _ = head(w, cls_gpu)
    _, mag_c = classify(w, pooled_gpu)
    return drift + (SC.bound_linear_f32(mag_p, H) + TANH_TOL) @ np.abs(Wc).T + SC.bound_linear_f32(mag_c, H)


def make_encoder(ctx, cfg: OB.BertCfg, w):
    from semantic_query_engine_amd.encoder import BertEncoder
    enc = BertEncoder(ctx, vocab_size=cfg.vocab_size, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                      inter=cfg.inter, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps)
    enc.load_weights(w, head=True)
    return enc


def read_head(enc, B: int, H: int, L: int):
    """cls, pooled, logits of the scoring call that just returned, float64."""
    rd = lambda what, n: enc.state_read(what, np.float32, B * n).astype(np.float64).reshape(B, n)
    return rd("cls", H), rd("pooled", H), rd("logits", L)
