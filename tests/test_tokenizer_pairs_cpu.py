"""sqe_tokenize_pair_batch / WordPieceTokenizer.encode_pairs: [CLS] A [SEP] B [SEP] with type ids and the two-step truncation
(A to max_a pieces, B to what is left).  Where A fits in max_a the ids and type ids are those of
tokenizers.BertWordPieceTokenizer under enable_truncation(max_len, strategy="only_second").  CPU only."""
import ctypes as C

import numpy as np
import pytest

from oracle import wordpiece as WP
from tests.test_oracle_wordpiece import SAMPLES

MAX_LEN, MAX_A = 40, 16


@pytest.fixture(scope="module")
def vocab():
    return WP.synthetic_vocab(SAMPLES, size=1500)


@pytest.fixture(scope="module")
def tok(vocab):
    from semantic_query_engine_amd.tokenizer import WordPieceTokenizer
    return WordPieceTokenizer(vocab_text="\n".join(vocab) + "\n")


@pytest.fixture(scope="module")
def hf(vocab, tmp_path_factory):
    from tokenizers import BertWordPieceTokenizer
    p = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    p.write_text("\n".join(vocab) + "\n", encoding="utf-8")
    return BertWordPieceTokenizer(str(p), lowercase=True)


def _body(tok, text, limit=4096):
    return tok.encode(text, limit + 2)[1:-1]


def _check_row(tok, vocab, a, b, ids, types, n, max_len, max_a):
    """the contract, restated from the single-text encoding"""
    cls, sep = vocab.index("[CLS]"), vocab.index("[SEP]")
    pa = _body(tok, a)[:max_a]
    pb = _body(tok, b)[:max_len - 3 - len(pa)]
    want = [cls] + pa + [sep] + pb + [sep]
    assert n == len(want) <= max_len
    assert ids[:n].tolist() == want and not ids[n:].any()
    assert types[:n].tolist() == [0] * (len(pa) + 2) + [1] * (len(pb) + 1) and not types[n:].any()
    return pa, pb


def test_pairs_match_the_hf_tokenizer_where_a_fits(tok, hf, vocab):
    a_texts = [s for s in SAMPLES if 0 < len(_body(tok, s)) <= MAX_A][:12]
    assert len(a_texts) >= 6
    b_texts = [SAMPLES[(3 * i + 1) % len(SAMPLES)] * (1 + i % 3) for i in range(len(a_texts))]
    b_texts[0] = ""                                                     # B empty: [CLS] A [SEP] [SEP]
    ids, types, lens = tok.encode_pairs(a_texts, b_texts, MAX_LEN, MAX_A)
    hf.enable_truncation(MAX_LEN, strategy="only_second")
    cut = 0
    for i, (a, b) in enumerate(zip(a_texts, b_texts)):
        e = hf.encode(a, b)
        assert ids[i, :lens[i]].tolist() == e.ids and types[i, :lens[i]].tolist() == e.type_ids, (a, b)
        _, pb = _check_row(tok, vocab, a, b, ids[i], types[i], int(lens[i]), MAX_LEN, MAX_A)
        cut += len(pb) < len(_body(tok, b))
    assert lens[0] == len(_body(tok, a_texts[0])) + 3 and types[0, lens[0] - 1] == 1
    assert cut >= 3                                                     # several rows had B truncated


def test_b_cut_in_the_middle_of_a_word(tok, hf, vocab):
    word = next(w for s in SAMPLES for w in s.split() if len(_body(tok, w)) >= 3 and vocab.index("[UNK]") not in _body(tok, w))
    pieces = _body(tok, word)
    a = next(s for s in SAMPLES if 0 < len(_body(tok, s)) <= 6)
    na = len(_body(tok, a))
    max_len = na + 3 + len(pieces) + 1                                  # room for "word" and ONE piece of the second
    ids, types, lens = tok.encode_pairs([a], [word + " " + word], max_len, 6)
    pa, pb = _check_row(tok, vocab, a, word + " " + word, ids[0], types[0], int(lens[0]), max_len, 6)
    assert pb == pieces + pieces[:1] and lens[0] == max_len
    hf.enable_truncation(max_len, strategy="only_second")
    e = hf.encode(a, word + " " + word)
    assert ids[0].tolist() == e.ids and types[0].tolist() == e.type_ids


def test_b_cut_to_nothing_and_max_len_4(tok, vocab):
    cls, sep = vocab.index("[CLS]"), vocab.index("[SEP]")
    long_a = " ".join(SAMPLES[:4])
    assert len(_body(tok, long_a)) > 13
    ids, types, lens = tok.encode_pairs([long_a], [SAMPLES[5]], 16, 13)            # max_a = max_len - 3: nothing left for B
    assert lens[0] == 16 and ids[0, 14] == sep and ids[0, 15] == sep and types[0].tolist() == [0] * 15 + [1]
    ids, types, lens = tok.encode_pairs([long_a, "", ""], [SAMPLES[5], SAMPLES[5], ""], 4, 1)
    pa, pb = _body(tok, long_a)[:1], _body(tok, SAMPLES[5])
    assert ids.tolist() == [[cls, pa[0], sep, sep], [cls, sep, pb[0], sep], [cls, sep, sep, 0]]
    assert types.tolist() == [[0, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 0]] and lens.tolist() == [4, 4, 3]


def test_a_longer_than_max_a_is_the_single_text_encoding(tok, vocab):
    long_a = " ".join(SAMPLES[:6])
    for max_a in (1, 5, MAX_A):
        ids, types, lens = tok.encode_pairs([long_a], [SAMPLES[7]], MAX_LEN, max_a)
        single = tok.encode(long_a, max_a + 2)
        assert len(single) == max_a + 2 and ids[0, :max_a + 2].tolist() == single
        _check_row(tok, vocab, long_a, SAMPLES[7], ids[0], types[0], int(lens[0]), MAX_LEN, max_a)


def test_threaded_batch_equals_row_by_row(tok):
    ids, types, lens = tok.encode_pairs([], [], MAX_LEN, MAX_A)
    assert ids.shape == (0, MAX_LEN) and types.shape == (0, MAX_LEN) and lens.shape == (0,)
    a = [SAMPLES[i % len(SAMPLES)] for i in range(65)]
    b = [SAMPLES[(7 * i + 2) % len(SAMPLES)] * (i % 4) for i in range(65)]
    ids, types, lens = tok.encode_pairs(a, b, MAX_LEN, MAX_A)               # n >= 64: the threaded path
    for i in range(65):
        i1, t1, l1 = tok.encode_pairs(a[i:i + 1], b[i:i + 1], MAX_LEN, MAX_A)
        assert np.array_equal(ids[i], i1[0]) and np.array_equal(types[i], t1[0]) and lens[i] == l1[0]


def test_invalid_arguments(tok):
    from semantic_query_engine_amd import _native as N
    for max_len, max_a in ((3, 1), (4, 0), (4, 2), (16, 14), (16, -1), (0, 0)):
        with pytest.raises(N.SqeError) as e:
            tok.encode_pairs(["a"], ["b"], max_len, max_a)
        assert e.value.code == -1                                           # SQE_ERR_INVALID
    with pytest.raises(ValueError):
        tok.encode_pairs(["a"], [], 16, 4)
    lib = N.load()
    out = np.zeros(16, np.int32)
    one = (C.c_char_p * 1)(b"a")
    size = np.array([1], np.int64).ctypes.data_as(N.c_i64_p)
    args = lambda **kw: [kw.get("tok", tok.handle), kw.get("a", one), size, one, kw.get("bs", size), kw.get("n", 1), 16, 4,
                         out.ctypes.data, kw.get("types", out.ctypes.data), out.ctypes.data]
    assert lib.sqe_tokenize_pair_batch(*args()) == 0
    assert lib.sqe_tokenize_pair_batch(*args(tok=None)) == -1
    assert lib.sqe_tokenize_pair_batch(*args(n=-1)) == -1
    assert lib.sqe_tokenize_pair_batch(*args(types=None)) == -1
    assert lib.sqe_tokenize_pair_batch(*args(a=None)) == -1
    assert lib.sqe_tokenize_pair_batch(*args(bs=np.array([-1], np.int64).ctypes.data_as(N.c_i64_p))) == -1
