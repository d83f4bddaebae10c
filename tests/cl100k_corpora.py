"""Corpora of the cl100k_base word-start tests — TEST INFRASTRUCTURE ONLY.

The kernels (csrc/pretok_cl100k.h) mark 16 bytes per thread and 4096 per block with a
16-byte halo, look back over four codepoints and ahead over one, and carry three scans
over the blocks: the digit position, the newlines a run of "other" takes with it
(forward), and whether a newline follows in the same whitespace run (backward).
pretok_corpora.py's ``periodic`` puts a pattern on every in-block offset; the
generators here supply the patterns and the texts whose masks have a closed form.
Everything stays in the kernels' domain (pretok_corpora.in_domain).
"""
from __future__ import annotations

import numpy as np

import pretok_corpora as P

BLK = P.BLK

# the host fuzz against `regex`: every class in every UTF-8 width, both apostrophes, the
# long s, the Kelvin sign, a combining mark, nine kinds of whitespace, CR and LF
PALETTE_STR = ("abstdmlvreSTDMLVREx" "\u017f\u212a\u00e9\u4f60\U00010437"
               "07\u0663\u00b2\u0969\U0001d7d8"
               "'\u2019.,!\u0301\u20ac\U0001f600\x01\x1c\x1f\u200b"
               " \t\x0b\x0c\x85\u00a0\u2003\u2028\u3000" "\n\r")
HOST_FUZZ_SEED = 201
HOST_FUZZ_STRINGS = 40_000

e = lambda s: s.encode("utf-8")
LETTERS = [bytes([c]) for c in b"stmdrevlSTMDREVLaxzQ"] + [e(c) for c in "\u017f\u212a\u00e9\u4f60\U00010437"]
NUMBERS = [bytes([c]) for c in b"0123456789"] + [e(c) for c in "\u0663\u00b2\u0969\U0001d7d8"]
BLANKS = [b" ", b" ", b" ", b"\t"] + [e(c) for c in "\x85\u00a0\u2003\u2028\u3000"]
NEWLINES = [b"\n", b"\n", b"\r"]
OTHERS = [b"'", b"'", b".", b",", b"\x01", b"\x1c"] + [e(c) for c in "\u2019\u0301\u20ac\U0001f600\u200b"] + P.BEYOND
CLASSES = [LETTERS, NUMBERS, BLANKS, NEWLINES, OTHERS]
SUFFIXES = [e(s) for s in "s S t T m M d D re RE rE ve Ve ll LL lL se r l v \u017f l\u017f".split()]

FUZZ_SEEDS = (211, 212, 213, 214, 215, 216)
FUZZ_CODEPOINTS = 30_000
FUZZ_CUTS = (0, 1, 2, 3)


def fuzz(n_codepoints: int, seed: int) -> bytes:
    """About n_codepoints codepoints: iid draws (a class, then one of its pieces); with
    probability 0.15 a contraction template (an optional blank or "other", an apostrophe, one
    of SUFFIXES, half the time a letter), with 0.1 a run of 1-8 numbers of mixed width,
    with 0.15 a whitespace run of 1-6 with newlines in it, with 0.1 "other"s and then newlines."""
    rng = np.random.default_rng(seed)
    out, cps = [], 0
    pick = lambda pieces: pieces[int(rng.integers(0, len(pieces)))]
    while cps < n_codepoints:
        r = rng.random()
        if r < 0.15:
            head = [[], [pick(BLANKS)], [pick(OTHERS)], [pick(LETTERS)]][int(rng.integers(0, 4))]
            suf = pick(SUFFIXES)
            part = head + [pick([b"'", b"'", e("\u2019")]), suf] + ([pick(LETTERS)] if rng.integers(0, 2) else [])
        elif r < 0.25:
            part = [pick(NUMBERS) for _ in range(int(rng.integers(1, 9)))]
        elif r < 0.4:
            part = [pick(NEWLINES) if rng.random() < 0.35 else pick(BLANKS) for _ in range(int(rng.integers(1, 7)))]
        elif r < 0.5:
            part = [pick(OTHERS) for _ in range(int(rng.integers(1, 4)))] + [pick(NEWLINES) for _ in range(int(rng.integers(0, 4)))]
        else:
            part = [pick(CLASSES[int(rng.integers(0, 5))])]
        out += part
        cps += len(part)
    return b"".join(out)


def _probe_list() -> list:
    probes = [
        ("contraction", e("don't we'LL I'Ve x're")),
        ("contraction_long_s", e("it'\u017f a'\u212a b\u2019s \u00e9'd\u4f60")),
        ("contraction_at_start", e("'tis ''s .'t 1'm 'llama")),
        ("contraction_after_blank", e("a 'll\t's \u3000're  'd")),
        ("contraction_then", e("a's1 b'll. c'd\u0301 e't\n'm")),
        ("other_then_letters", e("a.b a..b ,x \u0301y !\u00e9 \u20ac\u4f60")),
        ("blank_then_other", e("a . b  . c\t. d \u20ace\u3000!")),
        ("blank_then_letters", e("a b  c\td\u3000e \u00a0f\x85g")),
        ("three_digits", e("x1234567 \u0663\u0663\u0663\u0663 12\u00b2")),
        ("digits_mixed_width", b"x" + P._digits(7, 1) + b" " + P._digits(5, 2)),
        ("blank_then_newline", e("a  \n b \t\n\n  c \r\n  d")),
        ("eaten_newlines", e("a.\n\n\nb !\r\n x ..\n \ny")),
        ("eaten_then_blank", e(".\n . ,\r\r\t\n'\n's")),
        ("wide_blanks", e("a\u3000\u3000b \u2003\n\u2003 c\u00a0\u00a0.d")),
        ("line_separators", e("a\u2028b\u0085\nc\u2029 \u2028d")),
        ("not_whitespace", e("a\x1cb \x1f\x1f c\u200b\n\x1c1")),
        ("beyond_unicode", b"a" + P.BEYOND[0] + b"b " + P.BEYOND[1] + b"\n7" + P.BEYOND[0] + b"'s"),
        ("surrogate", b"a\xed\xa0\x80b \xed\xbf\xbf\n.\xed\xa0\x80 "),
        ("trailing_blanks", e("a   b    \u30001   .")),
    ]
    out = []
    for name, pat in probes:
        period = len(pat) + 3 - len(pat) % 2      # odd, at least two newlines of padding
        out.append((name, pat, period))
    return out


PROBES = _probe_list()


def periodic(pattern: bytes, period: int) -> bytes:
    return P.periodic(pattern, period)


# ── closed forms (the scans across blocks) ───────────────────────────────────

RUN_LENGTHS = (4095, 4096, 4097, 3 * 4096 + 5)
CHAIN_N = P.CHAIN_N          # 1026 blocks: two per thread in k_ptc_scan2


def blank_run(k: int, j):
    """(bytes, mask): `a`, k blanks with one newline at run offset j (None: none), `x`.
    The blank after `a` starts a match; with a newline, \\s*[\\r\\n] takes the run up to it
    and what follows starts another; the run's last blank goes with the letter; the
    letter starts a match only right after the newline."""
    run = bytearray(b" " * k)
    if j is not None:
        run[j] = 0x0A
    data = b"a" + bytes(run) + b"x"
    m = np.zeros(len(data), np.uint8)
    m[0] = m[1] = 1
    if j is not None and j + 1 < k:
        m[1 + j + 1] = 1
    if j != k - 1:
        m[k] = 1                     # the last blank (when a blank it is)
    else:
        m[k + 1] = 1                 # the letter after the newline
    return data, m


def eaten_run(k: int):
    """(bytes, mask): `.`, k newlines, ` a`: the newlines all go with the full stop."""
    data = b"." + b"\n" * k + b" a"
    m = np.zeros(len(data), np.uint8)
    m[0] = m[k + 1] = 1
    return data, m


def digit_run(n: int):
    data = (np.arange(n, dtype=np.int64) % 10 + 0x30).astype(np.uint8).tobytes()
    return data, (np.arange(n) % 3 == 0).astype(np.uint8)


def blanks_then_newline(n: int):
    data = b" " * (n - 1) + b"\n"
    m = np.zeros(n, np.uint8)
    m[0] = 1
    return data, m


# ── the class table ──────────────────────────────────────────────────────────

def sweep_documents(lo: int, hi: int):
    """(bytes, offsets): `a` c `b` as a document of its own for every codepoint c in [lo, hi)
    (surrogates as the 3-byte sequences they would be)."""
    cp = np.arange(lo, hi, dtype=np.uint32)
    size = np.where(cp < 0x80, 1, np.where(cp < 0x800, 2, np.where(cp < 0x10000, 3, 4)))
    offs = np.zeros(cp.shape[0] + 1, np.uint64)
    offs[1:] = np.cumsum(size + 2)
    buf = np.zeros(int(offs[-1]), np.uint8)
    at = offs[:-1].astype(np.int64)
    buf[at] = ord("a")
    for s in (1, 2, 3, 4):
        sel = size == s
        c, p = cp[sel], at[sel] + 1
        if s == 1:
            buf[p] = c
        else:
            buf[p] = (0xF00 >> s & 0xFF) | (c >> (6 * (s - 1)))
            for j in range(1, s):
                buf[p + j] = 0x80 | ((c >> (6 * (s - 1 - j))) & 0x3F)
        buf[p + s] = ord("b")
    return buf.tobytes(), offs


# ── many documents ───────────────────────────────────────────────────────────

BATCH_TEXT = b"we'll 1234567  \n\n  x.\n\n'tis don't   9.\r\n\n a \t\n b'S 77 ..!\n\n z 1\n"
assert len(BATCH_TEXT) == 64
CUT_TAILS = [b"", e("\u4f60")[:1], e("\u4f60")[:2], e("\U00010437")[:3], e("\u00e9")[:1]]


def batch_documents():
    """(bytes, offsets): for every cut c of BATCH_TEXT the documents text[:c] + tail and text[c:],
    the tail in turn nothing or a UTF-8 sequence cut short, with an empty document after
    every seventh pair."""
    docs = []
    for c in range(len(BATCH_TEXT) + 1):
        docs += [BATCH_TEXT[:c] + CUT_TAILS[c % len(CUT_TAILS)], BATCH_TEXT[c:]]
        if c % 7 == 0:
            docs.append(b"")
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return b"".join(docs), offs
