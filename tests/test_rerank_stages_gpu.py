"""The stages a scoring call (sqe_encode_pairs) adds to the encoder, each against float64 on the stage's own input.  GPU only.

  embedding with segment ids   one-layer models, so SQE_ENC_X still holds the embedding LayerNorm output: every token row
                               against LayerNorm(word + position + the token's OWN type row) within bound_ln_bf16 -- and the
                               same comparison against type row 0 everywhere must fail, so a kernel that ignores the ids
                               cannot pass
  head                         SQE_ENC_CLS / POOLED / LOGITS: pooled within bound_linear_f32 + 2^-20 of tanh(float64) on the
                               CLS rows read back, logits within bound_linear_f32 on the pooled rows read back
  routes                       the same call eager, captured and replayed gives the same bits; so does the first shape
                               again after a larger batch grew the workspace and dropped the recorded graphs
Bounds and helpers: tests/encoder_stage_cases.py, tests/rerank_reference.py.  Measured ratios: profiles/rerank/NOTES.md."""
import functools

import numpy as np
import pytest

from tests import encoder_stage_cases as SC
from tests import rerank_reference as RR

pytestmark = pytest.mark.gpu

HIDDEN = (128, 384, 1024)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@functools.lru_cache(maxsize=None)
def _model(hidden, labels):
    """one-layer model with a small FFN (the layers are not under test here)"""
    cfg = SC.config(hidden, inter=128, max_pos=64)
    return cfg, RR.weights(cfg, labels, seed=7)


@pytest.fixture(scope="module")
def encoder(ctx):
    made = {}

    def get(hidden, labels):
        if (hidden, labels) not in made:
            cfg, w = _model(hidden, labels)
            made[hidden, labels] = RR.make_encoder(ctx, cfg, w)
        return made[hidden, labels]
    return get


def _read_x(enc, T, H):
    return SC.bf16_bits_to_f64(enc.state_read("x", np.uint16, T * H)).reshape(T, H)


# ------------------------------------------------------------------------------------------------ embedding
@pytest.mark.parametrize("hidden", HIDDEN)
def test_embedding_adds_each_tokens_own_type_row(encoder, hidden):
    cfg, w = _model(hidden, 2)
    enc = encoder(hidden, 2)
    B, S = 3, 32
    for boundaries, lens in (([2, 17, 31], [32, 32, 32]),            # type 1 from positions 2, 17 and 31
                             ([31, 32, 2], [32, 20, 9])):            # ragged; the middle row is type 0 throughout
        ids, types, lens = RR.pair_batch(cfg, B, S, boundaries, lens, seed=2)
        assert types.any() and (boundaries[1] < 32 or not types[1].any())
        enc.score_ids(ids, types, lens)
        got = _read_x(enc, B * S, hidden)
        ref = RR.embed(w, cfg, ids, types).reshape(B * S, hidden)
        ratio = SC.worst_ratio(got, ref, SC.bound_ln_bf16(ref))
        ref0 = RR.embed(w, cfg, ids, None).reshape(B * S, hidden)
        ratio0 = SC.worst_ratio(got, ref0, SC.bound_ln_bf16(ref0))
        print(f"EMBED hidden {hidden} boundaries {boundaries}: ratio {ratio:.4f}, against type row 0 everywhere {ratio0:.1f}")
        assert ratio <= 1.0, (hidden, boundaries, ratio)
        assert ratio0 > 1.0, "the check cannot tell a kernel that ignores the type ids"
        rows0 = (types.reshape(-1) == 0)
        assert SC.worst_ratio(got[rows0], ref0[rows0], SC.bound_ln_bf16(ref0[rows0])) <= 1.0      # type-0 tokens: row 0


@pytest.mark.parametrize("hidden", HIDDEN)
def test_null_types_are_all_zero_types(encoder, hidden):
    cfg, w = _model(hidden, 2)
    enc = encoder(hidden, 2)
    ids, _, lens = RR.pair_batch(cfg, 3, 32, [32, 32, 32], seed=3)
    a = enc.score_ids(ids, np.zeros_like(ids), lens)
    xa = enc.state_read("x", np.uint16, ids.size * hidden)
    b = enc.score_ids(ids, None, lens)
    xb = enc.state_read("x", np.uint16, ids.size * hidden)
    assert np.array_equal(xa, xb) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # out-of-range type ids are clamped into [0, type_vocab)
    wild = np.where(np.arange(32)[None, :] >= 5, 7, -3).astype(np.int32).repeat(3, 0)
    enc.score_ids(ids, wild, lens)
    xc = enc.state_read("x", np.uint16, ids.size * hidden)
    enc.score_ids(ids, np.clip(wild, 0, 1), lens)
    assert np.array_equal(xc, enc.state_read("x", np.uint16, ids.size * hidden)) and not np.array_equal(xc, xa)


# ------------------------------------------------------------------------------------------------ head
# H = 128 leaves half the lanes of the float4 pass idle, 384 ends in a half pass, 1024 fills the four register passes and
# 1152 is past them (the pooler then streams its weight row); B = 257 is past any batch tile of the head
HEAD_CASES = [(h, l, b, 8) for h in HIDDEN for l in (1, 2, 3) for b in (1, 5)] + \
             [(128, l, 257, 16) for l in (1, 2, 3)] + [(1152, 2, 5, 8)]


@pytest.mark.parametrize("hidden,labels,B,S", HEAD_CASES, ids=lambda v: str(v))
def test_head_against_float64_on_its_own_input(encoder, hidden, labels, B, S):
    cfg, w = _model(hidden, labels)
    enc = encoder(hidden, labels)
    assert enc.labels == labels
    ids, types, lens = RR.pair_batch(cfg, B, S, np.arange(B) % S + 1, seed=4)
    logits = enc.score_ids(ids, types, lens)
    assert logits.shape == (B, labels) and logits.dtype == np.float32
    cls, pooled, read = RR.read_head(enc, B, hidden, labels)
    assert np.array_equal(read, logits.astype(np.float64)), "the `logits` read-back is not what sqe_encode_pairs returned"
    assert np.isfinite(cls).all() and np.abs(pooled).max() <= 1.0
    ratios = RR.head_ratios(w, cls, pooled, read)
    print(f"HEAD hidden {hidden} labels {labels} B {B}: pooled {ratios['pooled']:.4f} logits {ratios['logits']:.4f} "
          f"(logit spread {np.ptp(read):.2f})")
    assert max(ratios.values()) <= 1.0, ratios
    # the CLS rows the head read are the pooling LayerNorm of the encoder's own sums (the `out` stage of an embedding call)
    L = SC.layer_weights(w, 0)
    st = enc.state()
    pre = np.stack([enc.state_read("pre", np.float32, B * S * hidden, s * st["pre_stride"] * 4).astype(np.float64)
                    for s in range(st["pre_slices"])]).sum(0).reshape(B * S, hidden) if st["pre_slices"] else \
        SC.bf16_bits_to_f64(enc.state_read("pre", np.uint16, B * S * hidden)).reshape(B * S, hidden)
    from oracle import bert as OB
    ref = OB.stage_ln(pre[::S], L.g2, L.b2n, cfg.ln_eps)
    assert SC.worst_ratio(cls, ref, SC.bound_ln_f32(ref)) <= 1.0


def test_state_read_of_the_head_needs_a_scoring_call(encoder):
    from semantic_query_engine_amd._native import SqeError
    cfg, w = _model(128, 2)
    enc = encoder(128, 2)
    ids, types, lens = RR.pair_batch(cfg, 2, 8, [3, 4], seed=5)
    enc.score_ids(ids, types, lens)
    enc.state_read("cls", np.float32, 2 * 128)
    with pytest.raises(SqeError) as e:
        enc.state_read("out", np.float32, 2 * 128)                # the embedding result buffer is not this call's
    assert e.value.code == -4
    enc.encode_ids(ids, lens)
    for what in ("cls", "pooled", "logits"):
        with pytest.raises(SqeError) as e:
            enc.state_read(what, np.float32, 2)
        assert e.value.code == -4                                 # SQE_ERR_STATE
    assert enc.score_ids(ids[:0], types[:0], lens[:0]).shape == (0, 2)      # B == 0 is valid


# ------------------------------------------------------------------------------------------------ routes
def test_eager_captured_replayed_and_after_the_workspace_grew(ctx):
    cfg, w = _model(384, 3)
    enc = RR.make_encoder(ctx, cfg, w)                            # its own encoder: the graph cache starts empty
    ids, types, lens = RR.pair_batch(cfg, 3, 32, [2, 17, 31], seed=6)
    outs = []
    for want in ("eager", "captured", "replayed"):
        outs.append(enc.score_ids(ids, types, lens))
        assert enc.state()["mode"] == want
    assert all(np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)) for o in outs)
    ref = RR.forward(w, cfg, ids, types, lens)
    cls, pooled, _ = RR.read_head(enc, 3, 384, 3)
    assert (np.abs(outs[0] - ref["logits"]) <= RR.logit_bound_e2e(w, cls, ref["cls"], pooled)).all()
    big = RR.pair_batch(cfg, 9, 32, np.arange(9) + 2, seed=7)     # T = 288: t_pad 256 -> 512, and more CLS rows
    enc.score_ids(*big)
    st = enc.state()
    assert st["t_pad"] == 512 and st["mode"] == "eager"
    again = enc.score_ids(ids, types, lens)
    assert enc.state()["mode"] == "eager", "the graphs recorded against the old workspace must be gone"
    assert np.array_equal(again.view(np.uint32), outs[0].view(np.uint32))
    assert np.array_equal(enc.score_ids(ids, types, lens).view(np.uint32), outs[0].view(np.uint32))
    assert enc.state()["mode"] == "captured"
