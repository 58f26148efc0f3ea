"""tests/rerank_reference.py (the float64 cross-encoder forward the GPU rerank tests compare with) against
transformers.BertForSequenceClassification in float64: per-token type rows, the encoder, pooler, tanh, classifier.  Both sides
are float64 restatements of the same formula, so they agree to 1e-9.  CPU only."""
import numpy as np
import pytest
import torch

from tests import encoder_stage_cases as SC
from tests import rerank_reference as RR


def _hf_model(cfg, w, labels):
    from transformers import BertConfig, BertForSequenceClassification
    hf = BertForSequenceClassification(BertConfig(
        vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
        intermediate_size=cfg.inter, max_position_embeddings=cfg.max_pos, type_vocab_size=cfg.type_vocab, hidden_act="gelu",
        layer_norm_eps=cfg.ln_eps, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, classifier_dropout=0.0,
        num_labels=labels))
    sd = {(n if n.startswith("classifier.") else "bert." + n): torch.as_tensor(v) for n, v in w.items()}
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing)
    return hf.double().eval()


@pytest.mark.parametrize("labels", [1, 3])
def test_reference_matches_transformers(labels):
    cfg = SC.config(hidden=128, inter=512, heads=2, layers=2, vocab_size=512, max_pos=64)
    w = RR.weights(cfg, labels, seed=5)
    B, S = 3, 32
    ids, types, lens = RR.pair_batch(cfg, B, S, boundaries=[2, 17, 9], lens=[32, 25, 11], seed=1)
    assert types[0, 2:].all() and not types[0, :2].any() and types[1, 17:25].all() and not types[1, 25:].any()
    got = RR.forward(w, cfg, ids, types, lens)["logits"]
    mask = (np.arange(S)[None, :] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        ref = _hf_model(cfg, w, labels)(input_ids=torch.as_tensor(ids, dtype=torch.long), attention_mask=torch.as_tensor(mask),
                                        token_type_ids=torch.as_tensor(types, dtype=torch.long)).logits.numpy()
    assert ref.dtype == np.float64 and got.shape == ref.shape == (B, labels)
    delta = float(np.abs(got - ref).max())
    print(f"labels {labels}: max |delta| {delta:.3e}, logits {np.round(ref.ravel(), 3)}")
    assert delta <= 1e-9
    # the type rows matter: the same batch with type 0 everywhere scores differently
    assert np.abs(RR.forward(w, cfg, ids, None, lens)["logits"] - ref).max() > 1e-3
    assert np.ptp(ref[:, -1]) > 0.1                      # the head weights spread the logits
