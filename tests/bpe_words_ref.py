"""Reference of the word-bounded merge-rank encode — TEST INFRASTRUCTURE ONLY.

Word i of a mask is bytes[starts[i]:starts[i + 1]] (byte 0 always starts a word);
the result is the concatenation of O.encode_merge_order(word, merges) over the
words, cached by word.  Shared by test_bpe_words_host.py, test_gpu_bpe_words.py
and test_js_bpe_words.py.
"""
import functools

import numpy as np

import bpe_oracle as O


def word_bounds(n, ws):
    """Offsets of the words of an n-byte input under the mask ws, with n at the end."""
    ws = np.asarray(ws).astype(bool).copy()
    assert ws.shape == (n,)
    if n:
        ws[0] = True
    return np.flatnonzero(ws).tolist() + [n]


def encode_words_ref(data, merges, ws):
    data = bytes(data)
    merges = [list(m[:3]) for m in merges]
    cache = {}
    out = []
    b = word_bounds(len(data), ws)
    for s, e in zip(b[:-1], b[1:]):
        w = data[s:e]
        if w not in cache:
            cache[w] = O.encode_merge_order(w, merges)
        out += cache[w]
    return out


@functools.lru_cache(maxsize=None)
def model(kind, seed):
    """The 600-merge models of test_gpu_merge_encode.py."""
    from gpubpe import synth
    return [m[:3] for m in O.train(getattr(synth, kind)(60_000, seed=seed), 600)["merges"]]


@functools.lru_cache(maxsize=None)
def text(kind, seed):
    from gpubpe import synth
    return getattr(synth, kind)(12_000, seed=seed + 100)


XY_MERGES = [[120, 32, 256], [256, 121, 257]]
XY_TEXT = b"x yx y x"
XY_WORDS = [120, 32, 121, 120, 32, 121, 32, 120]
XY_WHOLE = [257, 257, 32, 120]
