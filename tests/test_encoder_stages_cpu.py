"""The float64 stage references of the encoder (oracle/bert.py: stage_*) and the bounds the GPU stage tests hold the
kernels to (tests/encoder_stage_cases.py), checked without a GPU:
(a) the stage functions chained without rounding are bert_encode, every layer, every valid row;
(b) a NumPy emulation of the encoder's rounding model passes every bound on every GPU case small enough for a CPU -- the
    bounds are not too tight for a correct kernel;
(c) seven seeded faults, each as small as such a defect can be, FAIL their bound -- the bounds are tight enough to see a
    subtly wrong kernel, which the end-to-end bars of tests/test_encoder_gpu.py (cos >= 0.999, 6e-2) cannot."""
import numpy as np
import pytest

from oracle import bert as OB
from tests import encoder_stage_cases as SC


def test_chained_stages_are_bert_encode():
    cfg = OB.BertCfg.toy()
    w = SC.weights(cfg, seed=3)
    ids, lens = SC.batch(cfg, 4, 40, seed=1)
    import torch
    cls, hidden = OB.bert_encode({k: torch.from_numpy(v) for k, v in w.items()}, cfg, ids, lens, return_hidden=True)
    B, S = ids.shape
    H = cfg.hidden
    valid = np.arange(S)[None, :] < lens[:, None]
    x = OB.stage_embed_ln(ids, w["embeddings.word_embeddings.weight"], w["embeddings.position_embeddings.weight"],
                          w["embeddings.token_type_embeddings.weight"][0], w["embeddings.LayerNorm.weight"],
                          w["embeddings.LayerNorm.bias"], cfg.ln_eps)
    assert np.abs(x - hidden[0])[valid].max() < 1e-5
    x = x.reshape(B * S, H)
    for l in range(cfg.layers):
        L = SC.layer_weights(w, l)
        qkv, _ = OB.stage_linear(x, L.Wqkv, L.bqkv)
        att, mag = OB.stage_attention(qkv.reshape(B, S, 3 * H), lens, cfg.heads)
        assert (mag >= np.abs(att) - 1e-12).all()
        pre, _ = OB.stage_linear(att.reshape(B * S, H), L.Wo, L.bo, resid=x)
        x1 = OB.stage_ln(pre, L.g1, L.b1n, cfg.ln_eps)
        h = OB.stage_gelu(OB.stage_linear(x1, L.W1, L.b1)[0])
        pre, mag = OB.stage_linear(h, L.W2, L.b2, resid=x1)
        assert (mag >= np.abs(pre) - 1e-12).all()
        x = OB.stage_ln(pre, L.g2, L.b2n, cfg.ln_eps)
        assert np.abs(x.reshape(B, S, H) - hidden[l + 1])[valid].max() < 1e-5, l
    assert np.abs(x.reshape(B, S, H)[:, 0] - cls).max() < 1e-5


def _emulated_ratios(cfg, w, ids, lens, **kw):
    return SC.check_stages(SC.emulate(w, cfg, ids, lens, **kw), w, cfg, ids, lens)


def _assert_inside(ratios, what):
    print(what, {k: round(v, 3) for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (what, ratios)


def _slices(cfg, B, S):
    """K slices of (out-proj, FFN-down) as a 256-CU part would run them; two where the ring kernel's cost model decides"""
    r = SC.expected_routes(cfg, B, S, 256)
    return tuple(r[k][1] or 2 for k in ("out_proj", "ffn_down"))


@pytest.mark.parametrize("c", SC.FEW_TOKEN_CONFIGS, ids=lambda c: f"H{c['hidden']}")
def test_emulation_inside_bounds_few_token_shapes(c):
    cfg = SC.config(**c)
    w = SC.weights(cfg, seed=3)
    for B, S in SC.FEW_TOKEN_SHAPES:
        ids, lens = SC.batch(cfg, B, S)
        _assert_inside(_emulated_ratios(cfg, w, ids, lens, slices=_slices(cfg, B, S), gelu="erf"), (c["hidden"], B, S))


@pytest.mark.parametrize("c", SC.RING_CONFIGS, ids=lambda c: f"H{c['hidden']}")
def test_emulation_inside_bounds_ring_shapes(c):
    cfg = SC.config(**c)
    w = SC.weights(cfg, seed=4)
    for B, S in SC.RING_SHAPES:
        ids, lens = SC.batch(cfg, B, S)
        for sl in ((1, 1), (1, 2), (1, 4)):
            _assert_inside(_emulated_ratios(cfg, w, ids, lens, slices=sl, gelu="erf"), (c["hidden"], B, S, sl))


@pytest.mark.parametrize("variant", ["base", "sharp"])
def test_emulation_inside_bounds_attention_shapes(variant):
    cfg = SC.config(128, max_pos=512)
    w = SC.weights(cfg, seed=5, variant=variant)
    for S in SC.ATTENTION_S:
        for short_first in (True, False):
            lens = SC.attention_lens(S, short_first)
            ids, lens = SC.batch(cfg, len(lens), S, lens)
            _assert_inside(_emulated_ratios(cfg, w, ids, lens), (variant, S, short_first))


@pytest.mark.parametrize("hidden", SC.LN_HIDDEN)
def test_emulation_inside_bounds_layernorm_shapes(hidden):
    cfg = SC.config(hidden)
    for variant in ("base", "offset", "flat"):
        w = SC.weights(cfg, seed=6, variant=variant)
        for B, S in SC.LN_SHAPES:
            ids, lens = SC.batch(cfg, B, S)
            _assert_inside(_emulated_ratios(cfg, w, ids, lens, slices=_slices(cfg, B, S)), (hidden, variant, B, S))


def test_emulation_inside_bounds_depth_and_bf16_pre():
    B, S = SC.DEPTH_SHAPE
    for depth in (1, 2, 3, 4):
        cfg = SC.config(layers=depth, **SC.DEPTH_CONFIG)
        w = SC.weights(cfg, seed=7)
        ids, lens = SC.batch(cfg, B, S)
        _assert_inside(_emulated_ratios(cfg, w, ids, lens, slices=(1, 2)), ("depth", depth))
    # the large-batch form at a small shape: bf16 `pre` rows and the polynomial GELU
    cfg = SC.config(**SC.DEPTH_CONFIG)
    w = SC.weights(cfg, seed=7)
    ids, lens = SC.batch(cfg, B, S)
    _assert_inside(_emulated_ratios(cfg, w, ids, lens, pre_bf16=True, gelu="poly"), "bf16 pre")


# fault -> (weight set, the stages whose bound must fail, emulate() arguments)
FAULTS = {
    "ulp2": ("base", ("qkv",), {}),
    "drop_slice": ("base", ("pre",), dict(slices=(1, 2))),
    "mask_admit": ("base", ("att",), {}),
    "mask_drop": ("base", ("att",), {}),
    "skip_rescale": ("sharp", ("att",), {}),
    "bias_block": ("base", ("qkv",), {}),
    "ln_mean": ("base", ("embed", "x1", "out"), {}),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_fails_its_bound(fault):
    """One layer at hidden 128, sequences of 130 tokens (three key tiles), the batch of the attention cases: its first sequence is
    20 tokens long and is the one whose key mask is off by one.  Without the fault every stage is inside its bound; with it
    the stage that holds the fault is outside, and no other stage is (each stage is judged on its own input)."""
    variant, broken, kw = FAULTS[fault]
    cfg = SC.config(128, max_pos=512)
    w = SC.weights(cfg, seed=5, variant=variant)
    lens = SC.attention_lens(130, True)
    ids, lens = SC.batch(cfg, len(lens), 130, lens)
    clean = _emulated_ratios(cfg, w, ids, lens, **kw)
    assert max(clean.values()) <= 1.0, clean
    bad = _emulated_ratios(cfg, w, ids, lens, fault=fault, fault_seq=0, **kw)
    print(fault, {k: round(v, 3) for k, v in bad.items()})
    for stage in SC.STAGES:
        if stage in broken:
            assert bad[stage] > 1.0, (fault, stage, bad)
        else:
            assert bad[stage] <= 1.0, (fault, stage, bad)


def test_bf16_helpers():
    import torch
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 3
    assert np.array_equal(SC.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy())
    bits = (SC.bf16_round(x).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(SC.bf16_bits_to_f64(bits), SC.bf16_round(x))
    assert SC.bf16_step(np.array([1.0]), 2)[0] == 1.0 + 2.0 ** -6
    assert len(SC.ring_forced_settings()) == 21
