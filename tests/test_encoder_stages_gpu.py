"""Every stage of the encoder, every row, against float64 -- on the stage's own input.  GPU only.

After an encode the encoder's workspace still holds what the last layer computed (sqe_encoder_state[_read],
BertEncoder.state / state_read).  Each stage's output is recomputed in float64 (oracle/bert.py: stage_*) from the input the
GPU itself held and the bf16 weights, and every element of every valid row must be inside the bound that the rounding model
gives for that stage (tests/encoder_stage_cases.py; tests/test_encoder_stages_cpu.py shows that a correct emulation passes
those bounds and that seven small seeded faults do not).  Before it compares, every case asserts from state() WHICH kernel ran:
GEMM family, ring tile, K slices, attention tiling.  The variants that only the knobs library can select (every ring tile and
slice count, the A/B forms README.md lists) run in child processes on libsqe_knobs.so, one at a time.
profiles/encoder_stages/NOTES.md has the measured |got - ref| / bound of every stage and route."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import encoder_stage_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS_LIB = os.path.join(ROOT, "semantic_query_engine_amd", "libsqe_knobs.so")
LARGE_CFG = dict(hidden=1024, inter=4096, heads=16, max_pos=512)


@pytest.fixture(scope="module")
def ctx():
    from semantic_query_engine_amd import Context
    return Context(0)


@pytest.fixture(scope="module")
def cus(ctx):
    return ctx.device_info()["cu_count"]


def _valid_rows(lens, S):
    return (np.arange(S)[None, :] < np.asarray(lens)[:, None]).reshape(-1)


# ------------------------------------------------------------------------------------------------ few-token GEMM
@pytest.mark.parametrize("shape", SC.FEW_TOKEN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("c", SC.FEW_TOKEN_CONFIGS, ids=lambda c: f"H{c['hidden']}")
def test_few_token_gemm(ctx, cus, c, shape):
    """T <= 64 and K % 512 == 0: the few-token kernel at all four sites, the two residual sites in 1, 2 or 4 K slices as the CU
    count allows (hidden 512: out-proj 1, FFN-down 4; hidden 1024: 2 and 4 on a 256-CU part); T = 65: the ring kernel."""
    cfg = SC.config(**c)
    w = SC.weights(cfg, seed=3)
    B, S = shape
    ids, lens = SC.batch(cfg, B, S)
    ratios, st, _, _ = SC.run_case(SC.make_encoder(ctx, cfg, w), cfg, w, ids, lens, "few-token")
    SC.assert_routes(st, cfg, B, S, cus)
    family = "ring" if B * S > 64 else "few-token"
    assert {g["family"] for g in st["gemm"].values()} == {family}, st
    SC.assert_inside(ratios, (c, shape))


# ------------------------------------------------------------------------------------------------ ring GEMM, shipped library
@pytest.mark.parametrize("shape", SC.RING_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("c", SC.RING_CONFIGS, ids=lambda c: f"H{c['hidden']}")
def test_ring_gemm_as_shipped(ctx, cus, c, shape):
    """t_pad = 256, 512, 1024, 2048 with T no multiple of 4, 64 or 256: the ring kernel at all four sites, tile and slices from
    the cost model; from 1,024 padded tokens on the measured rule of launch_gemm_ring decides the two residual sites."""
    cfg = SC.config(**c)
    w = SC.weights(cfg, seed=4)
    B, S = shape
    ids, lens = SC.batch(cfg, B, S)
    ratios, st, _, _ = SC.run_case(SC.make_encoder(ctx, cfg, w), cfg, w, ids, lens, "ring")
    SC.assert_routes(st, cfg, B, S, cus)
    assert {g["family"] for g in st["gemm"].values()} == {"ring"}, st
    assert st["gemm"]["qkv"]["slices"] == 1 and st["gemm"]["ffn_up"]["slices"] == 1
    if st["t_pad"] >= 1024:
        assert (st["gemm"]["out_proj"]["menu"], st["gemm"]["out_proj"]["slices"]) == (0, 1), st
        assert (st["gemm"]["ffn_down"]["menu"], st["gemm"]["ffn_down"]["slices"]) == (4 if st["t_pad"] >= 2048 else 1, 2), st
    SC.assert_inside(ratios, (c, shape))


# ------------------------------------------------------------------------------------------------ children on the knobs library
@pytest.fixture(scope="module")
def knobs_env():
    # always through make: a knobs library left over from an older tree must not be the one that is tested
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "semantic_query_engine_amd", "csrc"), "KNOBS=1", "-j8"],
                          stdout=subprocess.DEVNULL)
    return dict(os.environ, SQE_LIB=KNOBS_LIB)


CHILD = "import sys; sys.path.insert(0, %r); from tests import encoder_stage_cases as SC; SC.child_main(sys.argv[1])" % ROOT


def _child(env, spec, timeout=600):
    out = subprocess.run([sys.executable, "-c", CHILD, json.dumps(spec)], env=env, capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["ok"] is True


@pytest.mark.parametrize("m,s,c", SC.ring_forced_settings(), ids=lambda v: f"H{v['hidden']}" if isinstance(v, dict) else str(v))
def test_ring_gemm_every_tile_and_slice_count(knobs_env, m, s, c):
    """SQE_RING_FORCE_<epilogue>_K<K> = menu:slices pins the ring kernel's choice per epilogue and depth: tile m at all four
    sites, the FFN-down GEMM in s K slices, at t_pad = 256 and 512.  The child asserts that state() shows the forced entry."""
    H, I = c["hidden"], c["inter"]
    env = dict(knobs_env, **{f"SQE_RING_FORCE_0_K{H}": f"{m}:1", f"SQE_RING_FORCE_1_K{H}": f"{m}:1",
                             f"SQE_RING_FORCE_2_K{H}": f"{m}:1", f"SQE_RING_FORCE_2_K{I}": f"{m}:{s}"})
    _child(env, dict(cfg=c, shapes=SC.RING_FORCED_SHAPES, label=f"ring forced {m}:{s}",
                     expect=dict(family="ring", menu=m, slices=dict(qkv=1, out_proj=1, ffn_up=1, ffn_down=s), pre_slices=s)))


KNOB_FORMS = {
    # knob -> (environment, child spec): each at the one shape where it differs from the default
    "enc_gemm_0": (dict(SQE_ENC_GEMM="0"), dict(cfg=LARGE_CFG, shapes=[(32, 512)], batch="large", seed=11,
                                                expect=dict(family="persistent", pre_slices=0))),
    "enc_gemm_v0": (dict(SQE_ENC_GEMM_V0="1"), dict(cfg=LARGE_CFG, shapes=[(32, 512)], batch="large", seed=11,
                                                    expect=dict(family="one-tile", pre_slices=1))),
    "enc_skinny_0": (dict(SQE_ENC_SKINNY="0"), dict(cfg=SC.FEW_TOKEN_CONFIGS[0], shapes=[(4, 16)], seed=3,
                                                    expect=dict(family="ring"))),
    "att_form_1": (dict(SQE_ATT_FORM="1"), dict(cfg=dict(hidden=128, max_pos=512), shapes=[(0, 320)], batch="attention", seed=5,
                                                variant="sharp", expect=dict(att=[8, 2]))),
    "att_form_2": (dict(SQE_ATT_FORM="2"), dict(cfg=dict(hidden=128, max_pos=512), shapes=[(0, 320)], batch="attention", seed=5,
                                                variant="sharp", expect=dict(att=[8, 1]))),
    "att_form_3": (dict(SQE_ATT_FORM="3"), dict(cfg=dict(hidden=128, max_pos=512), shapes=[(0, 320)], batch="attention", seed=5,
                                                variant="sharp", expect=dict(att=[4, 1]))),
    "enc_graph_0": (dict(SQE_ENC_GRAPH="0"), dict(cfg=dict(hidden=128), shapes=[(2, 24)], calls=3, seed=5,
                                                  expect=dict(modes=["eager", "eager", "eager"]))),
}


@pytest.mark.parametrize("knob", sorted(KNOB_FORMS))
def test_knob_forms(knobs_env, knob):
    """The A/B forms README.md lists for the encoder pass the same stage bounds as the default and report themselves in
    state(): the two-stage persistent GEMM, the one-tile-per-workgroup GEMM, the ring kernel in place of the few-token one, the
    three other attention tilings, and kernel-by-kernel launches without graph replay."""
    env, spec = KNOB_FORMS[knob]
    _child(dict(knobs_env, **env), dict(spec, label=knob))


# ------------------------------------------------------------------------------------------------ ping-pong GEMM
@pytest.mark.parametrize("shape", [(32, 512), (33, 500)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ping_pong_gemm(ctx, cus, shape):
    """16k tokens at hidden 1024: all four sites on the ping-pong kernel (polynomial GELU, bf16 `pre` rows); 33 x 500 = 16,500
    tokens leaves the last token tile ragged (t_pad = 16,640).  Every row, float64 matmuls."""
    cfg = SC.config(**LARGE_CFG)
    w = SC.weights(cfg, seed=11)
    B, S = shape
    ids, lens = SC.large_batch(cfg, B, S)
    ratios, st, _, _ = SC.run_case(SC.make_encoder(ctx, cfg, w), cfg, w, ids, lens, "ping-pong")
    SC.assert_routes(st, cfg, B, S, cus)
    assert {g["family"] for g in st["gemm"].values()} == {"ping-pong"} and st["pre_slices"] == 0, st
    SC.assert_inside(ratios, shape)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("S", SC.ATTENTION_S)
def test_attention_tilings(ctx, cus, S):
    """64-row (S < 128), 128-row (S < 256) and 4 x 2 (S >= 256) tilings at hidden 128 / 2 heads; lengths 1, 63, 64, 65, S - 1, S
    and one shorter than a query block, first in one batch and last in the other; base weights (flat softmax) and sharp ones
    (|q k| / 8 ~ 30: rows whose maximum sits in the first key tile and rows whose maximum comes in the last)."""
    cfg = SC.config(128, max_pos=512)
    for variant in ("base", "sharp"):
        w = SC.weights(cfg, seed=5, variant=variant)
        enc = SC.make_encoder(ctx, cfg, w)
        for short_first in (True, False):
            lens = SC.attention_lens(S, short_first)
            ids, lens = SC.batch(cfg, len(lens), S, lens)
            if variant == "sharp" and S > 64:
                ids = SC.steer_last_key(cfg, w, ids, lens)
            ratios, st, buf, _ = SC.run_case(enc, cfg, w, ids, lens, f"attention {variant}")
            SC.assert_routes(st, cfg, len(lens), S, cus)
            if variant == "sharp":
                b = int(np.argmax(lens == S))                                  # a full-length sequence, head 0
                q, k = buf["qkv"][b * S:(b + 1) * S, :64], buf["qkv"][b * S:(b + 1) * S, 128:192]
                sc = q @ k.T / 8.0
                assert 15.0 <= np.abs(sc).max() <= 80.0, np.abs(sc).max()
                if S > 64:
                    top = sc.argmax(-1)
                    assert (top < 64).any() and (top >= (S - 1) // 64 * 64).any()
            SC.assert_inside(ratios, (S, variant, short_first))


# ------------------------------------------------------------------------------------------------ LayerNorm family, embedding
@pytest.mark.parametrize("hidden", SC.LN_HIDDEN)
def test_layernorm_family(ctx, cus, hidden):
    """hidden 128 / 384 / 1280: the strided loop (1, 2, 5 trips); 256 / 512 / 768 / 1024: rows in registers (1..4 loads); T % 4 and
    B % 4 = 1, 2, 3 (the tails of layernorm_kernel and pool_ln_kernel); 1, 2 or 4 partial sums from whichever GEMM route the
    shape takes.  offset: embedding sums of 8 + small.  flat: zero-variance embedding rows, whose LayerNorm is its bias exactly."""
    cfg = SC.config(hidden)
    for variant in ("base", "offset", "flat"):
        w = SC.weights(cfg, seed=6, variant=variant)
        enc = SC.make_encoder(ctx, cfg, w)
        for B, S in SC.LN_SHAPES:
            ids, lens = SC.batch(cfg, B, S)
            ratios, st, buf, _ = SC.run_case(enc, cfg, w, ids, lens, f"layernorm {variant}")
            SC.assert_routes(st, cfg, B, S, cus)
            if variant == "flat":
                assert np.array_equal(buf["x"], np.broadcast_to(w["embeddings.LayerNorm.bias"].astype(np.float64), buf["x"].shape))
            SC.assert_inside(ratios, (hidden, variant, B, S))


def test_embedding_edges(ctx, cus):
    """ids 0 and vocab - 1 at valid positions, position S - 1 = max_pos - 1; ids outside [0, vocab) at padded positions (the
    kernel clamps them) change no valid row of any stage, bit for bit."""
    cfg = SC.config(128, max_pos=40)
    w = SC.weights(cfg, seed=8)
    enc = SC.make_encoder(ctx, cfg, w)
    B, S = 3, cfg.max_pos
    ids, lens = SC.batch(cfg, B, S, np.array([S, 7, 1]))
    valid = _valid_rows(lens, S)
    assert (ids.reshape(-1)[valid] == 0).any() and (ids.reshape(-1)[valid] == cfg.vocab_size - 1).any() and lens[0] == cfg.max_pos
    ratios, st, buf, out = SC.run_case(enc, cfg, w, ids, lens, "embedding")
    SC.assert_routes(st, cfg, B, S, cus)
    SC.assert_inside(ratios, "embedding")
    wild = ids.copy()
    wild.reshape(-1)[~valid] = np.resize(np.array([-1, -2 ** 31, cfg.vocab_size, cfg.vocab_size + 7, 2 ** 31 - 1], np.int64),
                                         int((~valid).sum())).astype(np.int32)
    ratios2, _, buf2, out2 = SC.run_case(enc, cfg, w, wild, lens, "embedding, wild padding ids")
    SC.assert_inside(ratios2, "embedding, wild padding ids")
    assert np.array_equal(out2, out)
    for k in ("x", "qkv", "att", "x1", "hbuf"):
        assert np.array_equal(buf2[k][valid], buf[k][valid]), k
    assert np.array_equal(buf2["pre"][:, valid], buf["pre"][:, valid])


# ------------------------------------------------------------------------------------------------ depth
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_depth(ctx, cus, depth):
    """Models of depth 1..4 over the same weights (tensors are seeded one by one, so a deeper model extends a shallower one):
    the last layer of each, i.e. every layer of the deepest and both directions of the x / x1 ping-pong of the layer loop."""
    cfg = SC.config(layers=depth, **SC.DEPTH_CONFIG)
    w = SC.weights(cfg, seed=7)
    w4 = SC.weights(SC.config(layers=4, **SC.DEPTH_CONFIG), seed=7)
    assert all(np.array_equal(v, w4[k]) for k, v in w.items())
    B, S = SC.DEPTH_SHAPE
    ids, lens = SC.batch(cfg, B, S)
    ratios, st, _, _ = SC.run_case(SC.make_encoder(ctx, cfg, w), cfg, w, ids, lens, f"depth {depth}")
    SC.assert_routes(st, cfg, B, S, cus)
    SC.assert_inside(ratios, depth)


# ------------------------------------------------------------------------------------------------ workspace and graph cache
def test_workspace_growth_and_graph_cache(ctx, cus):
    """The host logic around the kernels: a shape is launched kernel by kernel, then recorded, then replayed; a larger shape
    grows the workspace and drops the recorded graphs; ten more shapes push entries out of the cache of eight.  Every call gives
    the bits of the first call of its shape and of a fresh encoder, and state() describes the call that just returned."""
    cfg = SC.config(128, layers=2, max_pos=256)
    w = SC.weights(cfg, seed=9)
    enc = SC.make_encoder(ctx, cfg, w)
    with pytest.raises(Exception):
        enc.state()                                                      # SQE_ERR_STATE before the first encode
    with pytest.raises(Exception):
        enc.state_read("x", np.uint16, 1)

    def call(B, S, mode, first=None):
        ids, lens = SC.batch(cfg, B, S)
        ratios, st, _, out = SC.run_case(enc, cfg, w, ids, lens, f"graph cache {mode}")
        SC.assert_routes(st, cfg, B, S, cus)
        assert st["mode"] == mode, (B, S, st)
        SC.assert_inside(ratios, (B, S, mode))
        assert first is None or np.array_equal(out, first), (B, S, mode)
        return out

    first = call(2, 24, "eager")
    call(2, 24, "captured", first)
    call(2, 24, "replayed", first)
    call(8, 200, "eager")                                                # t_pad 256 -> 1792: new workspace, graphs destroyed
    call(2, 24, "eager", first)
    ids, lens = SC.batch(cfg, 2, 24)
    assert np.array_equal(SC.make_encoder(ctx, cfg, w).encode_ids(ids, lens), first)
    firsts = {}
    for s in range(10, 20):                                              # ten more keys: (8, 200), (2, 24) and two of these leave
        firsts[s] = call(1, s, "eager")
        call(1, s, "captured", firsts[s])
    call(2, 24, "eager", first)                                          # evicted: seen for the first time again
    call(2, 24, "captured", first)
    call(2, 24, "replayed", first)
    call(1, 19, "replayed", firsts[19])                                  # still cached
    call(1, 10, "eager", firsts[10])                                     # evicted
    with pytest.raises(Exception):
        enc.state_read("qkv", np.uint16, 1, offset=(256 + 64) * 3 * cfg.hidden * 2)      # one element past the end
