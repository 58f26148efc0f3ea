"""BERT encoder object over the C ABI (sqe_encoder_*): the model that ran inside Ollama for
``ollama_embed_text`` (main.py:134-145).  Weights are named as in the HF ``BertModel`` state dict."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping

import numpy as np

from . import _native as N
from .engine import Context

BERT_LARGE = dict(vocab_size=30522, hidden=1024, layers=24, heads=16, inter=4096, max_pos=512, type_vocab=2,
                  ln_eps=1e-12)

# sqe_encoder_state_read: what (SQE_ENC_*); sqe_encoder_state: mode, GEMM family and site names
STATE_BUFFERS = dict(x=0, x1=1, qkv=2, att=3, hbuf=4, pre=5, out=6, cls=7, pooled=8, logits=9)
HEAD_TENSORS = ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias")
MODES = ("eager", "captured", "replayed")
GEMM_FAMILIES = ("few-token", "ring", "ping-pong", "persistent", "one-tile")
GEMM_SITES = ("qkv", "out_proj", "ffn_up", "ffn_down")


class BertEncoder:
    def __init__(self, ctx: Context, **cfg):
        self.ctx, self.lib = ctx, ctx.lib
        full = dict(BERT_LARGE)
        full.update(cfg)
        self.cfg = full
        c = N.BertCfg(full["vocab_size"], full["hidden"], full["layers"], full["heads"], full["inter"],
                      full["max_pos"], full["type_vocab"], full["ln_eps"])
        h = C.c_void_p()
        N.check(self.lib.sqe_encoder_create(ctx.handle, C.byref(c), C.byref(h)))
        self.handle = h
        ctx._children.add(self)

    def close(self) -> None:
        if getattr(self, "handle", None):
            if self.ctx.handle:
                self.lib.sqe_encoder_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weights(self, weights: Mapping[str, "np.ndarray"], head: bool = False) -> None:
        """weights: name -> fp32 array (NumPy or anything with ``.numpy()``); pooler and classifier entries are ignored
        unless ``head`` (so the trunk of a reranker checkpoint loads as an embedder): then the classification head
        (HEAD_TENSORS, a ``BertForSequenceClassification`` export) is loaded too."""
        if head and any(n not in weights for n in HEAD_TENSORS):
            raise ValueError("load_weights(head=True): the checkpoint lacks " +
                             ", ".join(n for n in HEAD_TENSORS if n not in weights))
        for name, w in weights.items():
            if name.endswith("position_ids") or (not head and name.startswith(("pooler.", "classifier."))):
                continue
            self.load_tensor(name, w)
        self.finalize()

    def load_tensor(self, name: str, w) -> None:
        """One named tensor (sqe_encoder_load_tensor); load_weights does this for a whole checkpoint and finalizes."""
        a = np.ascontiguousarray(w.numpy() if hasattr(w, "numpy") else w, dtype=np.float32)
        shape = (C.c_int64 * a.ndim)(*a.shape)
        N.check(self.lib.sqe_encoder_load_tensor(self.handle, name.encode(), a.ctypes.data, shape, a.ndim))

    def finalize(self) -> None:
        """Accepts the encoder tensors alone or with the whole head (sqe_encoder_finalize); load_weights ends with it."""
        N.check(self.lib.sqe_encoder_finalize(self.handle))

    def encode_ids(self, ids: np.ndarray, lens: np.ndarray) -> np.ndarray:
        """ids int32 [B,S] (anything past lens[b] is ignored), lens [B] -> CLS embeddings fp32 [B, hidden]."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        b, s = ids.shape
        out = np.empty((b, self.cfg["hidden"]), np.float32)
        if b:
            N.check(self.lib.sqe_encode(self.handle, ids.ctypes.data, lens.ctypes.data, b, s, out.ctypes.data))
        return out

    def encode_ids_device(self, ids_ptr: int, lens_ptr: int, b: int, s: int, out_ptr: int) -> None:
        N.check(self.lib.sqe_encode_device(self.handle, ids_ptr, lens_ptr, b, s, out_ptr))

    @property
    def labels(self) -> int:
        """Outputs of the classification head; 0 without one."""
        n = C.c_int()
        N.check(self.lib.sqe_encoder_labels(self.handle, C.byref(n)))
        return n.value

    def score_ids(self, ids: np.ndarray, types, lens: np.ndarray) -> np.ndarray:
        """ids, types int32 [B,S] (types None: all 0), lens [B] -> classifier logits fp32 [B, labels] (sqe_encode_pairs)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        b, s = ids.shape
        if types is not None:
            types = np.ascontiguousarray(types, dtype=np.int32)
            if types.shape != ids.shape:
                raise ValueError("score_ids: types must have the shape of ids")
        out = np.empty((b, self.labels), np.float32)
        N.check(self.lib.sqe_encode_pairs(self.handle, ids.ctypes.data, types.ctypes.data if types is not None else None,
                                          lens.ctypes.data, b, s, out.ctypes.data))
        return out

    def score_ids_device(self, ids_ptr: int, types_ptr: int, lens_ptr: int, b: int, s: int, logits_ptr: int) -> None:
        N.check(self.lib.sqe_encode_pairs_device(self.handle, ids_ptr, types_ptr or None, lens_ptr, b, s, logits_ptr))

    def state(self) -> dict:
        """What the encode that just returned ran, and the extents of what state_read can copy out (sqe_encoder_state;
        test infrastructure): shape, eager / captured / replayed, attention form, and per GEMM site the kernel family,
        ring menu index (-1 off the ring kernel) and number of K slices."""
        st = N.EncoderState()
        N.check(self.lib.sqe_encoder_state(self.handle, st))
        out = {f: int(getattr(st, f)) for f in ("B", "S", "T", "t_pad", "att_nw", "att_nq", "pre_slices", "pre_stride")}
        out["mode"] = MODES[st.mode]
        out["gemm"] = {site: dict(family=GEMM_FAMILIES[g.family], menu=int(g.menu), slices=int(g.slices))
                       for site, g in zip(GEMM_SITES, st.gemm)}
        return out

    def state_read(self, what: str, dtype, count: int, offset: int = 0) -> np.ndarray:
        """`count` elements of `dtype` from byte `offset` of one workspace buffer as the last layer left it
        (sqe_encoder_state_read; what = one of STATE_BUFFERS; bf16 buffers read as uint16)."""
        out = np.empty(count, dtype)
        N.check(self.lib.sqe_encoder_state_read(self.handle, STATE_BUFFERS[what], offset, out.ctypes.data, out.nbytes))
        return out
