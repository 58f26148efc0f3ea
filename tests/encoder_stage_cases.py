"""Shared by tests/test_encoder_stages_cpu.py and tests/test_encoder_stages_gpu.py: the per-stage error bounds of the
encoder, the comparison of one set of stage buffers with the float64 stage references (oracle/bert.py: stage_*), a NumPy
emulation of the encoder's rounding model (with the seeded faults the bounds must catch), and the weight sets and batches
the cases use.

THE ROUNDING MODEL.  Every stage reads bf16 activations and bf16 weights, multiplies exactly (bf16 x bf16 fits fp32),
accumulates in fp32 and rounds its output once to bf16 -- except the two residual GEMMs, whose fp32 sums (`pre`) go to the
LayerNorm kernels unrounded (as up to four K-slice partial sums), or as bf16 rows on the large-batch kernels.  A stage is
compared with the float64 result computed FROM THE INPUT THE ENCODER ITSELF HELD, so one stage's error never reaches the
next stage's check.  bf16 keeps 8 significant bits, so rounding to it moves a value by at most half an ulp <= 2^-8 relative
(2^-9 at the top of a binade); e = 2^-24 is the same figure for fp32:

  linear, bf16 out    |got - ref| <= 2^-8 |ref| + 4 K e mag        mag = sum_k |w x| + |b| + |resid|
                      K e mag is the textbook bound of an fp32 dot product of length K and the factor 4 covers any summation
                      order (MFMA blocks, waves, K slices); the first term is the one bf16 rounding.  A sum that sits on a
                      rounding boundary may fall either way: either neighbour is within half an ulp plus the fp32 error.
  linear, fp32 out    |sum of the slices - ref| <= 4 K e mag
  GELU                1.13 (4 K e mag) + 2e-4 + 2^-8 |ref|         1.13 >= max |GELU'|; 2e-4 = the pinned tolerance of the
                      polynomial GELU (tests/test_gelu_fit_cpu.py; the erf form is far inside it); then one bf16 rounding
  LayerNorm, bf16 out 2^-8 |ref| + 1e-5 (1 + |ref|)                of the encoder's OWN fp32 input sums
  LayerNorm, fp32 out 1e-5 (1 + |ref|)
  embedding LN        the LayerNorm input here is not the encoder's own stored sum but word + position + type added in fp32
                      (the scratch row is overwritten later), while the reference adds the three tables exactly: the sum
                      carries up to 2 e (|w| + |p| + |t|) per element, which the LayerNorm multiplies by r = 1 / sigma.  With the
                      `offset` weights (sums of 8 + small, sigma 0.03) that is 1e-6 x 35 = 3e-5 on outputs near zero, above
                      the 1e-5 of the plain LayerNorm bound (measured: 1.006 x that bound at hidden 384, the finding in
                      profiles/encoder_stages/NOTES.md); no fp32 kernel can do better, so the embedding stage adds the
                      perturbation term of the next entry with a = 2 e (|w| + |p| + |t|) to the LayerNorm bound.
  attention           2^-7 sum_j p_j |v_j| + 2^-8 |ref|            every probability is rounded to bf16 before P V (2^-9
                      relative on average, 2^-8 at worst) while the denominator sums the unrounded ones; 2^-7 leaves the
                      same again for the exp2, the scale and the fp32 score and P V sums
  out-proj + LN1      the out-projection's fp32 sums are overwritten by FFN-down, so x1 is checked as the composite
                      LN1(x + att Wo^T + bo).  A perturbation d of the LayerNorm input, |d_i| <= a_i = 4 K e mag_i, moves
                      output i by at most r |g_i| (a_i + mean(a) + |n_i| rms(a)) to first order (r = 1 / sqrt(var + eps),
                      n = the normalised row: the three terms are d_i itself, the shift of the mean and the change of r);
                      the LayerNorm bf16 bound is added to that.  On the large-batch kernels the out-projection writes bf16 rows
                      like FFN-down does, and a is the bf16 linear bound.
No bound depends on a case; K, mag, ref come from the stage at hand."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np

from oracle import bert as OB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gelu_fit  # noqa: E402

U2 = 2.0 ** -8            # one bf16 rounding: half an ulp, relative, at worst
ACC = 4.0 * 2.0 ** -24    # x K x mag: fp32 accumulation
GELU_SLOPE, GELU_TOL = 1.13, 2e-4
LN_TOL = 1e-5
ATT_P = 2.0 ** -7

STAGES = ("embed", "qkv", "att", "x1", "hbuf", "pre", "out")


# ---------------------------------------------------------------------------------------------------- bf16
def bf16_round(a) -> np.ndarray:
    """float -> nearest bf16 (ties to even), returned as float64 (finite values only)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def bf16_bits_to_f64(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_step(a, ulps: int) -> np.ndarray:
    """bf16 values (as float64) moved `ulps` units in the last place away from zero."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) + np.uint32(ulps << 16)
    return u.view(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- bounds
def bound_linear_bf16(ref, mag, K):
    return U2 * np.abs(ref) + ACC * K * mag


def bound_linear_f32(mag, K):
    return ACC * K * mag


def bound_gelu(ref_out, mag, K):
    return GELU_SLOPE * ACC * K * mag + GELU_TOL + U2 * np.abs(ref_out)


def bound_ln_bf16(ref):
    return U2 * np.abs(ref) + LN_TOL * (1.0 + np.abs(ref))


def bound_ln_f32(ref):
    return LN_TOL * (1.0 + np.abs(ref))


def bound_attention(ref, mag):
    return ATT_P * mag + U2 * np.abs(ref)


def bound_ln_of_perturbed(pre_ref, a, g, eps):
    """LayerNorm output bound when its fp32 input is within `a` (elementwise) of pre_ref: see the module docstring."""
    mu = pre_ref.mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(((pre_ref - mu) ** 2).mean(-1, keepdims=True) + eps)
    n = (pre_ref - mu) * r
    return r * np.abs(g) * (a + a.mean(-1, keepdims=True) + np.abs(n) * np.sqrt((a * a).mean(-1, keepdims=True)))


def worst_ratio(got, ref, bound) -> float:
    """max |got - ref| / bound; a zero bound admits only equality."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(ratio.max())


# ---------------------------------------------------------------------------------------------------- weights and batches
def config(hidden, inter=None, heads=None, layers=1, vocab_size=300, max_pos=128) -> OB.BertCfg:
    return OB.BertCfg(vocab_size=vocab_size, hidden=hidden, layers=layers, heads=heads or hidden // 64,
                      inter=inter or 4 * hidden, max_pos=max_pos)


def weights(cfg: OB.BertCfg, seed: int, variant: str = "base"):
    """name -> fp32 NumPy array, every value a bf16 number (the encoder and the references hold the same parameters).
    base    oracle.bert.random_weights
    sharp   query weights and bias x 16, key weights and bias x 8 (powers of two: still bf16): |q k| / 8 reaches ~30, the
            softmax has one or two heavy keys per row and the running maximum moves between key tiles
    offset  type embedding + 8: every embedding sum is 8 + small, the cancellation case of the two-pass variance
    flat    word and position tables zero, the type row constant: every embedding row has zero variance"""
    w = {k: v.numpy().copy() for k, v in OB.random_weights(cfg, seed=seed).items()}
    if variant == "sharp":
        for l in range(cfg.layers):
            p = f"encoder.layer.{l}.attention.self."
            for t in ("weight", "bias"):
                w[p + "query." + t] *= 16.0
                w[p + "key." + t] *= 8.0
    elif variant == "offset":
        n = "embeddings.token_type_embeddings.weight"
        w[n] = bf16_round(w[n] + 8.0).astype(np.float32)
    elif variant == "flat":
        w["embeddings.word_embeddings.weight"][:] = 0.0
        w["embeddings.position_embeddings.weight"][:] = 0.0
        w["embeddings.token_type_embeddings.weight"][:] = 0.40625
    elif variant != "base":
        raise ValueError(variant)
    return w


def batch(cfg: OB.BertCfg, B: int, S: int, lens=None, seed: int = 0):
    """ids [B, S] over the whole vocabulary, ids 0 and vocab - 1 at valid positions; lens [B] (default: ragged, lens[0] = S)."""
    rng = np.random.default_rng(seed * 7919 + B * 1000 + S)
    ids = rng.integers(0, cfg.vocab_size, (B, S)).astype(np.int32)
    if lens is None:
        lens = rng.integers(1, S + 1, B)
        lens[0] = S
    lens = np.asarray(lens, dtype=np.int32)
    ids[0, 0] = 0
    if B > 1:
        ids[B - 1, 0] = cfg.vocab_size - 1
    elif lens[0] > 1:
        ids[0, lens[0] - 1] = cfg.vocab_size - 1
    return ids, lens


def steer_last_key(cfg: OB.BertCfg, w, ids, lens):
    """One-layer model, sharp weights: picks the id at the LAST position of the first full-length sequence so that for some query
    rows of head 0 that key beats every earlier one by a clear margin (a score step of 1 = a factor e) -- the running maximum of
    those rows then rises in the last key tile, however few keys that tile holds.  Predicted in float64 from the weights."""
    B, S = ids.shape
    b = int(np.argmax(lens == S))
    f = lambda n: np.asarray(w[n], np.float64)
    L, H = layer_weights(w, 0), cfg.hidden
    ln = lambda rows: OB.stage_ln(rows, f("embeddings.LayerNorm.weight"), f("embeddings.LayerNorm.bias"), cfg.ln_eps)
    pos, typ = f("embeddings.position_embeddings.weight"), f("embeddings.token_type_embeddings.weight")[0]
    x = ln(f("embeddings.word_embeddings.weight")[ids[b]] + pos[:S] + typ)
    q = x[:S - 1] @ L.Wqkv[:64].T + L.bqkv[:64]
    k = x[:S - 1] @ L.Wqkv[H:H + 64].T + L.bqkv[H:H + 64]
    best = (q @ k.T / 8.0).max(-1)
    cand = ln(f("embeddings.word_embeddings.weight") + pos[S - 1] + typ) @ L.Wqkv[H:H + 64].T + L.bqkv[H:H + 64]   # [vocab, 64]
    wins = ((q @ cand.T / 8.0) > best[:, None] + 1.0).sum(0)
    ids = ids.copy()
    ids[b, S - 1] = int(wins.argmax())
    assert wins.max() >= 1
    return ids


def attention_lens(S: int, short_first: bool):
    """len = 1, 63, 64, 65, S - 1, S (those that fit) and a length shorter than one query block, which comes first in one batch
    and last in the other: K/V staging of the last tile of a sequence runs into the next sequence or into the tail rows."""
    body = sorted({v for v in (1, 63, 64, 65, S - 1, S) if 1 <= v <= S})
    short = min(20, S)                      # < 64 query rows: the other query blocks of that sequence return at once
    return np.array(([short] + body) if short_first else (body + [short]), dtype=np.int32)


def layer_weights(w, l: int):
    p = f"encoder.layer.{l}."
    f = lambda n: np.asarray(w[n], np.float64)
    return SimpleNamespace(
        Wqkv=np.concatenate([f(p + f"attention.self.{n}.weight") for n in ("query", "key", "value")]),
        bqkv=np.concatenate([f(p + f"attention.self.{n}.bias") for n in ("query", "key", "value")]),
        Wo=f(p + "attention.output.dense.weight"), bo=f(p + "attention.output.dense.bias"),
        g1=f(p + "attention.output.LayerNorm.weight"), b1n=f(p + "attention.output.LayerNorm.bias"),
        W1=f(p + "intermediate.dense.weight"), b1=f(p + "intermediate.dense.bias"),
        W2=f(p + "output.dense.weight"), b2=f(p + "output.dense.bias"),
        g2=f(p + "output.LayerNorm.weight"), b2n=f(p + "output.LayerNorm.bias"))


# ---------------------------------------------------------------------------------------------------- the comparison
def check_stages(buf, w, cfg: OB.BertCfg, ids, lens):
    """buf: the last layer's stage buffers as float64 -- x [T, H], qkv [T, 3H], att [T, H], x1 [T, H], hbuf [T, I],
    pre [ns, T, H] fp32 partial sums (or [1, T, H] bf16 rows with pre_bf16 = True: the large-batch kernels, which write both
    residual sums that way), out [B, H] -- from an encoder's read-back or from emulate().  Every stage is recomputed in float64 from its input IN buf and compared on every row < T (attention: the rows
    at positions < lens[b]).  Returns stage -> worst |got - ref| / bound."""
    ids, lens = np.asarray(ids), np.asarray(lens)
    B, S = ids.shape
    T, H = B * S, cfg.hidden
    L = layer_weights(w, cfg.layers - 1)
    f = lambda n: np.asarray(w[n], np.float64)
    ratios = {}
    if cfg.layers == 1:                       # x is the embedding LayerNorm output
        idc = np.clip(ids, 0, cfg.vocab_size - 1)
        tables = (f("embeddings.word_embeddings.weight")[idc], f("embeddings.position_embeddings.weight")[:S][None],
                  f("embeddings.token_type_embeddings.weight")[0][None, None])
        g = f("embeddings.LayerNorm.weight")
        ref = OB.stage_embed_ln(idc, f("embeddings.word_embeddings.weight"), f("embeddings.position_embeddings.weight"),
                                f("embeddings.token_type_embeddings.weight")[0], g, f("embeddings.LayerNorm.bias"),
                                cfg.ln_eps).reshape(T, H)
        total = (tables[0] + tables[1] + tables[2]).reshape(T, H)
        summed = 2.0 * 2.0 ** -24 * (np.abs(tables[0]) + np.abs(tables[1]) + np.abs(tables[2])).reshape(T, H)
        ratios["embed"] = worst_ratio(buf["x"], ref, bound_ln_bf16(ref) + bound_ln_of_perturbed(total, summed, g, cfg.ln_eps))
    ref, mag = OB.stage_linear(buf["x"], L.Wqkv, L.bqkv)
    ratios["qkv"] = worst_ratio(buf["qkv"], ref, bound_linear_bf16(ref, mag, H))
    ref, mag = OB.stage_attention(buf["qkv"].reshape(B, S, 3 * H), lens, cfg.heads)
    valid = (np.arange(S)[None, :] < lens[:, None]).reshape(T)
    ref, mag = ref.reshape(T, H)[valid], mag.reshape(T, H)[valid]
    ratios["att"] = worst_ratio(buf["att"][valid], ref, bound_attention(ref, mag))
    pre_ref, mag = OB.stage_linear(buf["att"], L.Wo, L.bo, resid=buf["x"])
    ref = OB.stage_ln(pre_ref, L.g1, L.b1n, cfg.ln_eps)
    a = bound_linear_bf16(pre_ref, mag, H) if buf["pre_bf16"] else bound_linear_f32(mag, H)
    ratios["x1"] = worst_ratio(buf["x1"], ref, bound_ln_of_perturbed(pre_ref, a, L.g1, cfg.ln_eps) + bound_ln_bf16(ref))
    z, mag = OB.stage_linear(buf["x1"], L.W1, L.b1)
    ref = OB.stage_gelu(z)
    ratios["hbuf"] = worst_ratio(buf["hbuf"], ref, bound_gelu(ref, mag, H))
    del z
    ref, mag = OB.stage_linear(buf["hbuf"], L.W2, L.b2, resid=buf["x1"])
    pre_sum = buf["pre"].sum(0)
    bound = bound_linear_bf16(ref, mag, cfg.inter) if buf["pre_bf16"] else bound_linear_f32(mag, cfg.inter)
    ratios["pre"] = worst_ratio(pre_sum, ref, bound)
    ref = OB.stage_ln(pre_sum[::S], L.g2, L.b2n, cfg.ln_eps)          # the CLS row of every sequence
    ratios["out"] = worst_ratio(buf["out"], ref, bound_ln_f32(ref))
    return ratios


def read_back(enc, cfg: OB.BertCfg):
    """The stage buffers of the encode that just returned (BertEncoder.state / state_read), rows < T, widened to float64."""
    st = enc.state()
    T, H, I = st["T"], cfg.hidden, cfg.inter
    rd = lambda what, width: bf16_bits_to_f64(enc.state_read(what, np.uint16, T * width)).reshape(T, width)
    buf = {"x": rd("x", H), "x1": rd("x1", H), "qkv": rd("qkv", 3 * H), "att": rd("att", H), "hbuf": rd("hbuf", I)}
    ns = st["pre_slices"]
    buf["pre_bf16"] = ns == 0
    assert (st["gemm"]["out_proj"]["family"] in ("ping-pong", "persistent")) == (ns == 0), st      # both residual sites alike
    if ns == 0:
        buf["pre"] = rd("pre", H)[None]
    else:
        assert st["pre_stride"] == st["t_pad"] * H
        buf["pre"] = np.stack([enc.state_read("pre", np.float32, T * H, s * st["pre_stride"] * 4).astype(np.float64).reshape(T, H)
                               for s in range(ns)])
    buf["out"] = enc.state_read("out", np.float32, st["B"] * H).astype(np.float64).reshape(st["B"], H)
    return buf, st


# ---------------------------------------------------------------------------------------------------- routing, restated
def expected_gemm(T, t_pad, N, K, cu_count, resid):
    """(family, K slices or None where the ring kernel's cost model decides) of one GEMM site in the shipped library."""
    if T <= 64 and K % 512 == 0:
        s = 1
        if resid:
            while s < 4 and K % (512 * s * 2) == 0 and (N // 16) * s * 2 <= cu_count:
                s *= 2
        return "few-token", s
    if N % 256 == 0 and t_pad % 256 == 0 and (N // 256) * (t_pad // 256) >= cu_count:
        return "ping-pong", 1
    return "ring", None


def expected_routes(cfg: OB.BertCfg, B, S, cu_count):
    T, H, I = B * S, cfg.hidden, cfg.inter
    t_pad = (T + 255) // 256 * 256
    sites = {"qkv": (3 * H, H, False), "out_proj": (H, H, True), "ffn_up": (I, H, False), "ffn_down": (H, I, True)}
    return {k: expected_gemm(T, t_pad, n, kk, cu_count, r) for k, (n, kk, r) in sites.items()}


def expected_attention(S):
    return (4, 2) if S >= 256 else (8, 1) if S >= 128 else (4, 1)


def assert_routes(st, cfg, B, S, cu_count):
    """state() against the routing rules above; returns the ring menu entries seen, for the notes."""
    assert (st["B"], st["S"], st["T"], st["t_pad"]) == (B, S, B * S, (B * S + 255) // 256 * 256), st
    assert (st["att_nw"], st["att_nq"]) == expected_attention(S), st
    want = expected_routes(cfg, B, S, cu_count)
    for site, (family, slices) in want.items():
        g = st["gemm"][site]
        assert g["family"] == family, (site, g, want)
        if slices is not None:
            assert g["slices"] == slices, (site, g, want)
        assert (g["menu"] >= 0) == (family == "ring"), (site, g)
    down = st["gemm"]["ffn_down"]
    assert st["pre_slices"] == (0 if down["family"] in ("ping-pong", "persistent") else down["slices"]), st
    return {site: (g["menu"], g["slices"]) for site, g in st["gemm"].items() if g["family"] == "ring"}


# ---------------------------------------------------------------------------------------------------- emulation
def kernel_gelu_coefficients():
    src = open(os.path.join(ROOT, "semantic_query_engine_amd", "csrc", "enc_device.h")).read()
    body = src[src.index("f32x2 gelu_poly2(f32x2 v)"):]
    body = body[:body.index("return __builtin_elementwise_fma(v, h")]
    vals = [float(m) for m in re.findall(r"f32x2\{(-?[0-9.e+-]+)f,", body)]
    assert len(vals) == 7, vals
    return vals[::-1]


def _emu_linear(x, W, b, resid=None, slices=1, no_bias_block=None):
    """fp32 accumulation (BLAS sgemm) of bf16 operands; `slices` K slices, bias and residual added by slice 0."""
    x32, W32 = x.astype(np.float32), W.astype(np.float32)
    K = x.shape[1]
    b32 = b.astype(np.float32).copy()
    if no_bias_block is not None:
        b32[16 * no_bias_block:16 * no_bias_block + 16] = 0.0
    out = []
    for s in range(slices):
        k0, k1 = s * K // slices, (s + 1) * K // slices
        y = x32[:, k0:k1] @ W32[:, k0:k1].T
        if s == 0:
            y = y + b32
            if resid is not None:
                y = y + resid.astype(np.float32)
        out.append(y)
    return np.stack(out)


def _emu_ln(x, g, b, eps, short_mean=False):
    x = np.asarray(x, np.float64)
    mu = (x[..., :-4] if short_mean else x).mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return ((x - mu) / np.sqrt(var + eps) * g + b).astype(np.float32)


def _emu_attention(qkv, B, S, H, heads, lens, fault=None, fault_seq=0):
    """The kernel's online softmax over 64-key tiles: fp32 scores, running maximum and rescale, probabilities rounded to bf16
    for P V and summed unrounded for the denominator; rows >= len are not written (zero here)."""
    out = np.zeros((B, S, H))
    t = qkv.reshape(B, S, 3, heads, 64)
    for b in range(B):
        n = int(lens[b])
        keys = n
        if b == fault_seq and fault == "mask_admit":
            keys = n + 1
        if b == fault_seq and fault == "mask_drop":
            keys = n - 1
        assert 1 <= keys <= S
        q, k, v = (t[b, :, i].transpose(1, 0, 2) for i in range(3))                     # [heads, S, 64]
        sc = (q[:, :n].astype(np.float32) @ k[:, :keys].astype(np.float32).transpose(0, 2, 1)).astype(np.float64) / 8.0
        m = np.full((heads, n), -np.inf)
        l = np.zeros((heads, n))
        o = np.zeros((heads, n, 64))
        for k0 in range(0, keys, 64):
            s = sc[:, :, k0:k0 + 64]
            m_new = np.maximum(m, s.max(-1))
            alpha = np.exp(m - m_new)
            if fault == "skip_rescale" and k0 > 0:
                alpha = np.ones_like(alpha)
            p = np.exp(s - m_new[..., None]).astype(np.float32)
            l = l * alpha + p.sum(-1)
            o = o * alpha[..., None] + bf16_round(p) @ v[:, k0:min(k0 + 64, keys)]
            m = m_new
        out[b, :n] = bf16_round((o / l[..., None]).transpose(1, 0, 2).reshape(n, H))
    return out.reshape(B * S, H)


def emulate(w, cfg: OB.BertCfg, ids, lens, slices=(1, 1), pre_bf16=False, gelu="poly", fault=None, fault_seq=0):
    """The encoder's arithmetic in NumPy under the rounding model of the module docstring; returns the last layer's stage
    buffers in the form check_stages takes.  slices = K slices of (out-proj, FFN-down).  fault: None, or one seeded defect --
    ulp2 (one qkv element 2 bf16 ulps off), drop_slice (the last FFN-down K slice missing), mask_admit / mask_drop (sequence
    fault_seq attends to key len / not to key len - 1), skip_rescale (running sums not rescaled when the maximum rises in a later
    tile), bias_block (QKV bias missing in columns 16..31), ln_mean (LayerNorm means over the first H - 4 elements)."""
    ids, lens = np.asarray(ids), np.asarray(lens)
    B, S = ids.shape
    T, H = B * S, cfg.hidden
    f = lambda n: np.asarray(w[n], np.float64)
    short = fault == "ln_mean"
    idc = np.clip(ids, 0, cfg.vocab_size - 1)
    emb = (f("embeddings.word_embeddings.weight")[idc] + f("embeddings.position_embeddings.weight")[:S][None]
           + f("embeddings.token_type_embeddings.weight")[0]).astype(np.float32).reshape(T, H)
    x = bf16_round(_emu_ln(emb, f("embeddings.LayerNorm.weight"), f("embeddings.LayerNorm.bias"), cfg.ln_eps, short))
    coeff = kernel_gelu_coefficients()
    for l in range(cfg.layers):
        L = layer_weights(w, l)
        buf = {"x": x, "pre_bf16": pre_bf16}
        buf["qkv"] = bf16_round(_emu_linear(x, L.Wqkv, L.bqkv, no_bias_block=1 if fault == "bias_block" else None)[0])
        if fault == "ulp2":
            i = np.unravel_index(np.abs(buf["qkv"]).argmax(), buf["qkv"].shape)
            buf["qkv"][i] = bf16_step(buf["qkv"][i], 2)[0]
        buf["att"] = _emu_attention(buf["qkv"], B, S, H, cfg.heads, lens, fault, fault_seq)
        pre = _emu_linear(buf["att"], L.Wo, L.bo, resid=x, slices=1 if pre_bf16 else slices[0])
        pre = bf16_round(pre) if pre_bf16 else pre
        buf["x1"] = bf16_round(_emu_ln(pre.sum(0, dtype=np.float32), L.g1, L.b1n, cfg.ln_eps, short))
        z = _emu_linear(buf["x1"], L.W1, L.b1)[0]
        act = gelu_fit.gelu_poly_f32(z, coeff) if gelu == "poly" else OB.stage_gelu(z).astype(np.float32)
        buf["hbuf"] = bf16_round(act)
        pre = _emu_linear(buf["hbuf"], L.W2, L.b2, resid=buf["x1"], slices=1 if pre_bf16 else slices[1])
        if fault == "drop_slice":
            pre[-1] = 0.0
        buf["pre"] = bf16_round(pre)[:1] if pre_bf16 else pre.astype(np.float64)
        pre_sum = buf["pre"].sum(0).astype(np.float32)
        if l + 1 < cfg.layers:
            x = bf16_round(_emu_ln(pre_sum, L.g2, L.b2n, cfg.ln_eps, short))
    buf["out"] = _emu_ln(pre_sum[::S], L.g2, L.b2n, cfg.ln_eps, short).astype(np.float64)
    return buf


# ---------------------------------------------------------------------------------------------------- the cases
FEW_TOKEN_CONFIGS = (dict(hidden=512, inter=2048, heads=8), dict(hidden=1024, inter=4096, heads=16))
FEW_TOKEN_SHAPES = ((1, 1), (1, 9), (3, 21), (4, 16), (5, 13))                 # (4, 16): T = 64; (5, 13): T = 65, ring kernel
RING_CONFIGS = (dict(hidden=256, inter=1024, heads=4), dict(hidden=384, inter=1536, heads=6))
RING_SHAPES = ((3, 85), (7, 73), (9, 113), (17, 120))                          # t_pad = 256, 512, 1024, 2048
RING_FORCED_SHAPES = ((3, 85), (7, 73))                                        # t_pad = 256, 512
ATTENTION_S = (48, 64, 65, 127, 128, 130, 200, 255, 256, 257, 320, 512)
LN_HIDDEN = (128, 384, 1280, 256, 512, 768, 1024)                              # loop path: 1, 2, 5 trips; register path: nit 1..4
LN_SHAPES = ((1, 5), (2, 9), (3, 5))                                           # T % 4 = 1, 2, 3 and B % 4 = 1, 2, 3
DEPTH_CONFIG, DEPTH_SHAPE = dict(hidden=256, inter=1024, heads=4), (3, 64)
RING_MENU = ((2, 1), (4, 1), (6, 1), (8, 1), (4, 2), (6, 2), (8, 2))           # (fm, fn): 32 fm features x 64 fn tokens per tile


def ring_forced_settings():
    """(menu index, FFN-down K slices, config) for every ring tile and slice count that fits: N % (32 fm) == 0 at the four
    sites, t_pad % (64 fn) == 0 at 256 and 512, K / 64 % s == 0 and K / 64 / s >= 4 (out-proj, K = hidden of 256 or 384, never
    splits under that rule: it is forced to one slice).  fm = 6 needs hidden 384; fm = 8 needs hidden 256."""
    out = []
    for m, (fm, fn) in enumerate(RING_MENU):
        c = RING_CONFIGS[1] if fm == 6 else RING_CONFIGS[0]
        assert all(n % (32 * fm) == 0 for n in (3 * c["hidden"], c["hidden"], c["inter"])) and 256 % (64 * fn) == 0
        for s in (1, 2, 4):
            ks = c["inter"] // 64
            assert ks % s == 0 and ks // s >= 4
            out.append((m, s, c))
    return out


# ---------------------------------------------------------------------------------------------------- on the GPU
def make_encoder(ctx, cfg: OB.BertCfg, w):
    from semantic_query_engine_amd.encoder import BertEncoder
    enc = BertEncoder(ctx, vocab_size=cfg.vocab_size, hidden=cfg.hidden, layers=cfg.layers, heads=cfg.heads,
                      inter=cfg.inter, max_pos=cfg.max_pos, type_vocab=cfg.type_vocab, ln_eps=cfg.ln_eps)
    enc.load_weights(w)
    return enc


def run_case(enc, cfg, w, ids, lens, label):
    """One encode, its read-back and the stage comparison.  Prints one `STAGES {json}` line (label, what ran, the worst
    |got - ref| / bound per stage) BEFORE anything is asserted on the ratios; returns (ratios, state, buffers, result)."""
    import json
    out = enc.encode_ids(ids, lens)
    buf, st = read_back(enc, cfg)
    assert np.array_equal(buf["out"], out.astype(np.float64)), "the `out` read-back is not what sqe_encode returned"
    ratios = check_stages(buf, w, cfg, ids, lens)
    print("STAGES " + json.dumps({"case": label, "hidden": cfg.hidden, "B": int(ids.shape[0]), "S": int(ids.shape[1]),
                                  "mode": st["mode"], "att": [st["att_nw"], st["att_nq"]], "pre_slices": st["pre_slices"],
                                  "gemm": {k: [g["family"], g["menu"], g["slices"]] for k, g in st["gemm"].items()},
                                  "ratios": {k: round(v, 4) for k, v in ratios.items()}}), flush=True)
    return ratios, st, buf, out


def assert_inside(ratios, label):
    assert max(ratios.values()) <= 1.0, (label, ratios)


def large_batch(cfg, B, S):
    """the batch of tests/test_encoder_gpu.py::test_large_batch_persistent_gemms at (B, S): ragged long sequences, one full, one
    of a single token"""
    rng = np.random.default_rng(5)
    ids = rng.integers(0, cfg.vocab_size, (B, S)).astype(np.int32)
    lens = rng.integers(300, S + 1, B).astype(np.int32)
    lens[0], lens[1] = S, 1
    return ids, lens


def child_main(spec_json: str):
    """Body of the child processes of tests/test_encoder_stages_gpu.py that run on the knobs library (SQE_LIB; the knob itself
    is in the environment).  spec: cfg (config() arguments), seed, variant, shapes [[B, S], ...], batch ("ragged" | "large" |
    "attention"), calls (identical calls per shape, default 1), expect {family, menu, slices {site: n}, att [nw, nq],
    pre_slices, modes [...]} -- every key optional.  Prints one JSON line; any failed expectation or bound is an assertion."""
    import json
    from semantic_query_engine_amd import Context
    spec = json.loads(spec_json)
    cfg = config(**spec["cfg"])
    w = weights(cfg, spec.get("seed", 4), spec.get("variant", "base"))
    ex = spec.get("expect", {})
    ctx = Context(0)
    enc = make_encoder(ctx, cfg, w)
    worst = {}
    for B, S in spec["shapes"]:
        if spec.get("batch") == "large":
            ids, lens = large_batch(cfg, B, S)
        elif spec.get("batch") == "attention":
            lens = attention_lens(S, True)
            ids, lens = batch(cfg, len(lens), S, lens)
        else:
            ids, lens = batch(cfg, B, S)
        first = None
        for call in range(spec.get("calls", 1)):
            ratios, st, _, out = run_case(enc, cfg, w, ids, lens, spec.get("label", "child"))
            for site, g in st["gemm"].items():
                if "family" in ex:
                    assert g["family"] == ex["family"], (site, g, ex)
                if "menu" in ex:
                    assert g["menu"] == ex["menu"], (site, g, ex)          # a rejected force shows here
                if site in ex.get("slices", {}):
                    assert g["slices"] == ex["slices"][site], (site, g, ex)
            if "att" in ex:
                assert [st["att_nw"], st["att_nq"]] == ex["att"], (st, ex)
            if "pre_slices" in ex:
                assert st["pre_slices"] == ex["pre_slices"], (st, ex)
            if "modes" in ex:
                assert st["mode"] == ex["modes"][call], (call, st, ex)
            assert_inside(ratios, (B, S, call))
            first = out if first is None else first
            assert np.array_equal(out, first), "identical calls gave different bits"
            for k, v in ratios.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(json.dumps({"ok": True, "worst": worst}))
