"""Word-bounded merge-rank encode, the parts that need no GPU: the reference helper's
identities, the two inputs on which words change the tokens (so that the GPU tests
cannot pass on inputs where they do not), and the Python mask checker.  The
header / binding / export coverage of the new entry points is test_abi.py's.
"""
import numpy as np
import pytest

import bpe_oracle as O
from bpe_words_ref import XY_MERGES, XY_TEXT, XY_WHOLE, XY_WORDS, encode_words_ref, model, text, word_bounds


def test_reference_identities():
    merges, data = model("code", 53), text("code", 53)
    n = len(data)
    assert encode_words_ref(data, merges, np.zeros(n, np.uint8)) == O.encode_merge_order(data, merges)
    assert encode_words_ref(data, merges, np.ones(n, np.uint8)) == list(data)
    z = np.ones(n, np.uint8)
    z[0] = 0   # byte 0 starts a word whatever the mask says
    assert encode_words_ref(data, merges, z) == list(data)
    assert word_bounds(0, np.zeros(0, np.uint8)) == [0]
    assert encode_words_ref(b"", merges, np.zeros(0, np.uint8)) == []


def test_words_change_the_hand_case():
    data = np.frombuffer(XY_TEXT, np.uint8)
    assert O.encode_merge_order(XY_TEXT, XY_MERGES) == XY_WHOLE
    for ws in (O.heuristic_word_starts(data), O.gpt4_word_starts(XY_TEXT)):
        assert encode_words_ref(XY_TEXT, XY_MERGES, ws) == XY_WORDS


def test_words_change_synth_code():
    merges, data = model("code", 53), text("code", 53)
    got = encode_words_ref(data, merges, O.gpt4_word_starts(data))
    whole = O.encode_merge_order(data, merges)
    assert (len(got), len(whole)) == (8036, 7973)
    voc = O.vocab_from_merges(merges).entries
    assert O.decode(got, voc) == data


def test_mask_checker():
    from gpubpe import _lib
    from gpubpe.merge_encoder import checked_word_starts
    assert checked_word_starts(5) == (_lib.GBPE_WORDS_NONE, None)
    assert checked_word_starts(5, words="heuristic") == (_lib.GBPE_WORDS_HEURISTIC, None)
    assert checked_word_starts(5, words="gpt4") == (_lib.GBPE_WORDS_GPT4, None)
    mode, mask = checked_word_starts(4, word_starts=[True, False, 7, 0])
    assert mode == _lib.GBPE_WORDS_MASK and mask.dtype == np.uint8 and mask.tolist() == [1, 0, 1, 0]
    mode, mask = checked_word_starts(3, word_starts=b"\x00\x02\x00")
    assert mode == _lib.GBPE_WORDS_MASK and mask.tolist() == [0, 1, 0]
    assert checked_word_starts(0, word_starts=np.zeros(0, np.uint8))[0] == _lib.GBPE_WORDS_MASK
    bad = [
        dict(n=4, word_starts=np.zeros(4, np.uint8), words="gpt4"),   # both
        dict(n=4, word_starts=np.zeros(3, np.uint8)),                 # short
        dict(n=4, word_starts=np.zeros(5, np.uint8)),                 # long
        dict(n=4, word_starts=np.zeros((2, 2), np.uint8)),            # not one-dimensional
        dict(n=4, word_starts=np.zeros(4, np.float32)),               # not a mask
        dict(n=4, words="words"),                                     # unknown name
    ]
    for kw in bad:
        with pytest.raises(_lib.GpuBpeError) as e:
            checked_word_starts(**kw)
        assert e.value.code == _lib.GBPE_E_INVALID, kw
