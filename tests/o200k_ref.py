"""Sequential reference for the o200k_base word starts.

Written from the split pattern itself,

    [^\\r\\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]*[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?
    |[^\\r\\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]+[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?
    |\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n/]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+

as a small backtracking engine: each alternative is a list of greedy repetitions of a
codepoint set, the optional contraction and the look-ahead, tried in order at each
match start, every repetition giving back one codepoint at a time until the rest
matches — not the local rules or the automaton the kernels use, so that the two
derivations check each other.  The classes are read from the generated header
csrc/unicode_classes_o200k.h as text: the device and this file share one table
whatever Unicode version the running Python has.

Bytes decode as the kernels decode them: the lead byte picks the length, and the
bytes a sequence lacks at the end of the text read as 0.
"""
import os
import re

import numpy as np

from cl100k_ref import decode  # noqa: F401  (the same decoding)

U, L, B, M, N, W, R, O = range(8)

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpu-bpe_amd", "csrc",
                      "unicode_classes_o200k.h")

_tables = None


def tables():
    """(unicode version stamp, index list, class bytes) of the generated header."""
    global _tables
    if _tables is None:
        text = open(HEADER, encoding="utf-8").read()
        stamp = re.search(r"\(Unicode ([0-9.]+) via", text).group(1)
        arrays = {}
        for name, body in re.findall(r"kO200k(Index|Class)\[\d+\] = \{([^}]*)\}", text):
            arrays[name] = [int(x) for x in body.replace("\n", " ").split(",") if x.strip()]
        assert len(arrays["Index"]) == 0x110000 >> 8 and len(arrays["Class"]) % 256 == 0
        _tables = (stamp, arrays["Index"], bytes(arrays["Class"]))
    return _tables


def klass(cp: int) -> int:
    if cp >= 0x110000:
        return O
    _, idx, cls = tables()
    return cls[(idx[cp >> 8] << 8) | (cp & 0xFF)]


# ── the pattern's pieces: a set is a predicate on (codepoint, class) ─────────

def _in(*classes):
    return lambda cp, k: k in classes


PREFIX = _in(M, W, O)                    # [^\r\n\p{L}\p{N}]
UPPER = _in(U, B, M)                     # [\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]
LOWER = _in(L, B, M)                     # [\p{Ll}\p{Lm}\p{Lo}\p{M}]
NUMBER = _in(N)                          # \p{N}
SPACE = lambda cp, k: cp == 0x20
PUNCT = _in(M, O)                        # [^\s\p{L}\p{N}]
TAIL = lambda cp, k: k == R or cp == 0x2F   # [\r\n/]
BLANK = _in(W, R)                        # \s
NEWLINE = _in(R)                         # [\r\n]

_S = {ord("s"), ord("S"), 0x17F}   # simple case folding: the long s folds to s


def _fold(cp):
    if cp in _S:
        return "s"
    return chr(cp).lower() if cp < 0x80 else ""


CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")

# an item: ("rep", set, least, most), ("contraction",) = (?i:'s|...)?, ("not_nonblank",) = (?!\S)
INF = 1 << 60
ALTERNATIVES = (
    (("rep", PREFIX, 0, 1), ("rep", UPPER, 0, INF), ("rep", LOWER, 1, INF), ("contraction",)),
    (("rep", PREFIX, 0, 1), ("rep", UPPER, 1, INF), ("rep", LOWER, 0, INF), ("contraction",)),
    (("rep", NUMBER, 1, 3),),
    (("rep", SPACE, 0, 1), ("rep", PUNCT, 1, INF), ("rep", TAIL, 0, INF)),
    (("rep", BLANK, 0, INF), ("rep", NEWLINE, 1, INF)),
    (("rep", BLANK, 1, INF), ("not_nonblank",)),
    (("rep", BLANK, 1, INF),),
)


def _match(items, at, cps, k, pos):
    """End of the first way, in a backtracking engine's order, in which items[at:] match at pos; None if none."""
    n = len(cps)
    while at < len(items):          # (the items that cannot give anything back run in this loop)
        it = items[at]
        if it[0] == "contraction":
            # the group is optional and greedy: the first alternative that matches, else nothing;
            # only the end of the alternative follows it, so nothing is ever given back
            for c in CONTRACTIONS:
                if pos + len(c) <= n and cps[pos] == 0x27 and \
                        all(_fold(cps[pos + 1 + j]) == ch for j, ch in enumerate(c[1:])):
                    pos += len(c)
                    break
            at += 1
        elif it[0] == "not_nonblank":
            if pos < n and k[pos] not in (W, R):
                return None
            at += 1
        else:
            _, inset, least, most = it
            hi = pos
            while hi < n and hi - pos < most and inset(cps[hi], k[hi]):
                hi += 1
            for stop in range(hi, pos + least - 1, -1):     # greedy: the longest first
                end = _match(items, at + 1, cps, k, stop)
                if end is not None:
                    return end
            return None
    return pos


def match_end(cps, k, i):
    """End (exclusive) of the match that starts at codepoint i."""
    for alt in ALTERNATIVES:
        end = _match(alt, 0, cps, k, i)
        if end is not None and end > i:
            return end
    raise AssertionError("no alternative matches")


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
        ws[int(a):int(b)] = mask(data[int(a):int(b)])
    return ws


def pieces(text: str):
    """The matches of a str, as tiktoken would hand them to the merges."""
    cps = [ord(c) for c in text]
    s = starts(cps) + [1]
    cut = [i for i, v in enumerate(s) if v]
    return [text[a:b] for a, b in zip(cut[:-1], cut[1:])]
