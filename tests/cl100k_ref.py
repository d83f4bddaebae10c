"""Sequential reference for the cl100k_base word starts.

Written from the split pattern itself,

    '(?i:[sdmt]|ll|ve|re)|[^\\r\\n\\p{L}\\p{N}]?+\\p{L}+|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]++[\\r\\n]*|\\s*[\\r\\n]|\\s+(?!\\S)|\\s+

as a matcher that tries the seven alternatives in order at each match start and
moves to the match's end — not from the local rules the kernels use, so that the
two derivations check each other.  The classes are read from the generated header
csrc/unicode_classes_cl100k.h as text: the device and this file share one table
whatever Unicode version the running Python has.

Bytes decode as the kernels decode them: the lead byte picks the length, and the
bytes a sequence lacks at the end of the text read as 0.
"""
import os
import re

import numpy as np

L, N, W, R, O = range(5)

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpu-bpe_amd", "csrc",
                      "unicode_classes_cl100k.h")

_tables = None


def tables():
    """(unicode version stamp, index list, class bytes) of the generated header."""
    global _tables
    if _tables is None:
        text = open(HEADER, encoding="utf-8").read()
        stamp = re.search(r"\(Unicode ([0-9.]+) via", text).group(1)
        arrays = {}
        for name, body in re.findall(r"kCl100k(Index|Class)\[\d+\] = \{([^}]*)\}", text):
            arrays[name] = [int(x) for x in body.replace("\n", " ").split(",") if x.strip()]
        assert len(arrays["Index"]) == 0x110000 >> 8 and len(arrays["Class"]) % 256 == 0
        _tables = (stamp, arrays["Index"], bytes(arrays["Class"]))
    return _tables


def klass(cp: int) -> int:
    if cp >= 0x110000:
        return O
    _, idx, cls = tables()
    return cls[(idx[cp >> 8] << 8) | (cp & 0xFF)]


def decode(data: bytes):
    """The codepoints of `data` and the byte offset of each one's lead byte."""
    cps, offs = [], []
    n = len(data)
    i = 0
    while i < n:
        b = data[i]
        if b < 0x80:
            size, cp = 1, b
        elif b & 0xE0 == 0xC0:
            size, cp = 2, b & 0x1F
        elif b & 0xF0 == 0xE0:
            size, cp = 3, b & 0x0F
        else:
            size, cp = 4, b & 0x07
        for j in range(1, size):
            cp = (cp << 6) | ((data[i + j] & 0x3F) if i + j < n else 0)
        cps.append(cp)
        offs.append(i)
        i += size
    return cps, offs


_S = {ord("s"), ord("S"), 0x17F}   # simple case folding: the long s folds to s


def _fold(cp):
    if cp in _S:
        return "s"
    return chr(cp).lower() if cp < 0x80 else ""


def match_end(cps, k, i):
    """End (exclusive) of the match that starts at codepoint i."""
    n = len(cps)
    # '(?i:[sdmt]|ll|ve|re)
    if cps[i] == 0x27:
        if i + 1 < n and _fold(cps[i + 1]) in ("s", "d", "m", "t"):
            return i + 2
        if i + 2 < n and _fold(cps[i + 1]) + _fold(cps[i + 2]) in ("ll", "ve", "re"):
            return i + 3
    # [^\r\n\p{L}\p{N}]?+\p{L}+
    j = i + 1 if k[i] in (W, O) else i
    if j < n and k[j] == L:
        while j < n and k[j] == L:
            j += 1
        return j
    # \p{N}{1,3}
    if k[i] == N:
        j = i
        while j < n and j < i + 3 and k[j] == N:
            j += 1
        return j
    #  ?[^\s\p{L}\p{N}]++[\r\n]*
    j = i + 1 if cps[i] == 0x20 else i
    if j < n and k[j] == O:
        while j < n and k[j] == O:
            j += 1
        while j < n and k[j] == R:
            j += 1
        return j
    # the rest begin with whitespace: [i, e) is the maximal run
    e = i
    while e < n and k[e] in (W, R):
        e += 1
    assert e > i, "no alternative matches"
    # \s*[\r\n]: greedy, so it backs off to the run's last CR / LF
    for j in range(e - 1, i - 1, -1):
        if k[j] == R:
            return j + 1
    # \s+(?!\S): the whole run at the end of the text, else all but its last blank
    if e == n:
        return e
    if e - 1 > i:
        return e - 1
    # \s+
    return e


def starts(cps):
    """1 per codepoint at which a match starts."""
    k = [klass(c) for c in cps]
    out = [0] * len(cps)
    i = 0
    while i < len(cps):
        out[i] = 1
        i = match_end(cps, k, i)
    return out


def mask(data: bytes) -> np.ndarray:
    """The word-start byte mask of one text."""
    cps, offs = decode(data)
    ws = np.zeros(len(data), dtype=np.uint8)
    for o, s in zip(offs, starts(cps)):
        ws[o] = s
    return ws


def mask_docs(data: bytes, doc_off) -> np.ndarray:
    """The mask of documents laid end to end: each one's own."""
    ws = np.zeros(len(data), dtype=np.uint8)
    for a, b in zip(doc_off[:-1], doc_off[1:]):
        ws[a:b] = mask(data[a:b])
    return ws


def pieces(text: str):
    """The matches of a str, as tiktoken would hand them to the merges."""
    cps = [ord(c) for c in text]
    s = starts(cps) + [1]
    cut = [i for i, v in enumerate(s) if v]
    return [text[a:b] for a, b in zip(cut[:-1], cut[1:])]
