"""Reference of the batch word starts and the batch word-bounded merge-rank encode —
TEST INFRASTRUCTURE ONLY.

The expected value everywhere is the per-document oracle: each document alone
through O.gpt4_word_starts / O.heuristic_word_starts and encode_words_ref, offsets by
cumulative length.  Shared by test_bpe_words_batch_host.py,
test_gpu_bpe_words_batch.py and test_js_bpe_words_batch.py.
"""
import numpy as np

import bpe_oracle as O
from bpe_words_ref import encode_words_ref

NONE, MASK, HEUR, GPT4 = 0, 1, 2, 3   # GBPE_WORDS_*

# documents → the whole-buffer GPT-4 mask with the document starts forced / the per-document mask
HAND_PAIRS = [
    ([b"12", b"345 6789"], "1011010001", "1010010001"),   # the digit run restarts
    ([b"a1", b"2345"], "111010", "111001"),
    ([b"don'", b"t x"], "1000110", "1001110"),            # the look-ahead stops at the document end
    ([b"don", b"'t x"], "1001010", "1001110"),
    ([b"we'", b"ll x"], "1001010", "1011010"),
    ([b"we'l", b"l x"], "1000110", "1011110"),
    ([b"it's", b"x"], "10111", "10001"),                  # the after-letter test must not see the next document
    ([b"a\xc2", b"7a"], "1111", "1011"),                  # a cut sequence reads 0, not the next document's byte
    ([b"12", b"", b"", b"345"], "10110", "10100"),
]


def bits(ws):
    return "".join("1" if v else "0" for v in np.asarray(ws).tolist())


def doc_offsets(docs):
    offs = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        offs[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return offs


def split(data, offs):
    return [bytes(data[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])]


def doc_mask(doc, mode, mask=None):
    """The mask of one document alone in a GBPE_WORDS_* mode (mask: the caller's, for MASK)."""
    if mode == GPT4:
        return np.asarray(O.gpt4_word_starts(doc)).astype(np.uint8) if doc else np.zeros(0, np.uint8)
    if mode == HEUR:
        return np.asarray(O.heuristic_word_starts(np.frombuffer(doc, np.uint8))).astype(np.uint8)
    if mode == MASK:
        return (np.asarray(mask) != 0).astype(np.uint8)
    return np.zeros(len(doc), np.uint8)


def gpt4_batch_ref(docs):
    """Per-document GPT-4 word starts over the concatenation."""
    parts = [doc_mask(bytes(d), GPT4) for d in docs]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def gpt4_forced_ref(docs):
    """What a caller without the batch form gets: the whole-buffer mask, document starts set."""
    data = b"".join(docs)
    ws = np.asarray(O.gpt4_word_starts(data)).astype(np.uint8) if data else np.zeros(0, np.uint8)
    for o in doc_offsets(docs)[:-1]:
        if int(o) < len(data):
            ws[int(o)] = 1
    return ws


def encode_words_batch_ref(docs, merges, mode, mask=None):
    """(tokens, offsets): each document alone through encode_words_ref in `mode`;
    `mask` (mode MASK) is one mask over the concatenation."""
    offs = doc_offsets(docs)
    tokens, tok_off = [], [0]
    for d, doc in enumerate(docs):
        doc = bytes(doc)
        own = None if mask is None else np.asarray(mask)[int(offs[d]):int(offs[d + 1])]
        tokens += encode_words_ref(doc, merges, doc_mask(doc, mode, own))
        tok_off.append(len(tokens))
    return tokens, tok_off


def random_cuts(data, k, seed):
    """Document offsets of `data` cut at k random offsets in [1, n), each snapped forward
    to a codepoint start (duplicates fall together): np.uint64[D + 1]."""
    n = len(data)
    cuts = set()
    for c in np.random.default_rng(seed).integers(1, n, k).tolist():
        while c < n and (data[c] & 0xC0) == 0x80:
            c += 1
        cuts.add(c)
    return np.asarray([0] + sorted(cuts - {0, n}) + [n], np.uint64)
