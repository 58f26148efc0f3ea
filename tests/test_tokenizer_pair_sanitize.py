"""The pair form of csrc/tokenizer.cpp (sqe_tokenize_pair_batch) under AddressSanitizer + UndefinedBehaviorSanitizer.

`make -C semantic_query_engine_amd/csrc tokenizer_pair_asan` builds the host-only tokenizer with
g++ -fsanitize=address,undefined beside tests/native/tokenizer_pair_sanitize_driver.cpp, a stand-alone program.  The inputs are
the malformed-UTF-8 families of tests/test_tokenizer_sanitize.py, placed on both sides of the pair at several (max_len, max_a);
the driver must exit cleanly (any sanitizer report aborts with a non-zero code) and its ids and type ids must equal what the
shipped libsqe.so returns for the same bytes.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from oracle import wordpiece as WP
from tests.test_oracle_wordpiece import SAMPLES
from tests.test_tokenizer_sanitize import _cases as _single_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "semantic_query_engine_amd", "csrc")
SHAPES = ((48, 12), (4, 1), (16, 13), (64, 61), (512, 64))       # (max_len, max_a): the smallest, max_a = max_len - 3, the default


def _pair_cases():
    texts = [b for _, b in _single_cases()]
    plain = SAMPLES[3].encode("utf-8")
    cases = []
    for i, t in enumerate(texts):
        max_len, max_a = SHAPES[i % len(SHAPES)]
        cases.append((max_len, max_a, t, plain))                 # malformed bytes as A ...
        cases.append((max_len, max_a, plain, t))                 # ... as B ...
        cases.append((max_len, max_a, t, texts[(i + 7) % len(texts)]))   # ... and on both sides
    cases.append((4, 1, b"", b""))
    return cases


def test_pair_tokenizer_under_asan_ubsan_matches_the_library(tmp_path):
    subprocess.check_call(["make", "-C", CSRC, "tokenizer_pair_asan"], stdout=subprocess.DEVNULL)
    exe = os.path.join(CSRC, "build_san", "tokenizer_pair_asan")
    toks = WP.synthetic_vocab(SAMPLES + ["background methods results conclusions patients treatment study data analysis " * 3], size=1500)
    vocab = "\n".join(toks).encode("utf-8")
    (tmp_path / "vocab.txt").write_bytes(vocab)
    cases = _pair_cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        for max_len, max_a, a, b in cases:
            f.write(struct.pack("<iiqq", max_len, max_a, len(a), len(b)))
            f.write(a)
            f.write(b)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path / "vocab.txt"), str(tmp_path / "cases.bin"), str(tmp_path / "ids.bin")],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.stdout.strip() == f"ok {len(cases)} cases"

    # the same bytes through the shipped library (ctypes, raw bytes: no Python-side decoding in between)
    from semantic_query_engine_amd import _native as N
    lib = N.load()
    h = C.c_void_p()
    N.check(lib.sqe_tokenizer_create(vocab, len(vocab), C.byref(h)))
    got = np.fromfile(tmp_path / "ids.bin", dtype=np.int32)
    pos = 0
    try:
        for max_len, max_a, a, b in cases:
            ids, types, n = np.full(max_len, -7, np.int32), np.full(max_len, -7, np.int32), np.zeros(1, np.int32)
            na, nb = np.array([len(a)], np.int64), np.array([len(b)], np.int64)
            N.check(lib.sqe_tokenize_pair_batch(h, (C.c_char_p * 1)(a), na.ctypes.data_as(N.c_i64_p), (C.c_char_p * 1)(b),
                                                nb.ctypes.data_as(N.c_i64_p), 1, max_len, max_a, ids.ctypes.data,
                                                types.ctypes.data, n.ctypes.data))
            assert n[0] == got[pos]
            assert np.array_equal(ids, got[pos + 1:pos + 1 + max_len]) and np.array_equal(types, got[pos + 1 + max_len:pos + 1 + 2 * max_len])
            pos += 1 + 2 * max_len
    finally:
        lib.sqe_tokenizer_destroy(h)
    assert pos == got.size
