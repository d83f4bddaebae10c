"""Corpora of the GPT-4 word-start tests — TEST INFRASTRUCTURE ONLY.

pretok.hip marks 16 bytes per thread and 4096 per block (plus a 16-byte halo each
side), looks back over three codepoints and ahead over the codepoint itself and
three more, and scans the digit-run position over the blocks.  These generators put
every rule of k_pt_mark at every one of those edges:

``PALETTE``: one-codepoint pieces per class, in every UTF-8 width the class has.
``fuzz``: iid palette draws, contraction templates and mixed-width digit runs.
``end_cases``: short inputs that end in every contraction suffix.
``periodic`` / ``PROBES``: a short pattern at every in-block offset 0..4095.
``digit_chain``: long ASCII digit runs with a closed-form mask (the block scans).
``sweep_bmp`` / ``sweep_astral``: every codepoint (the device class table).

Domain: the kernel is written for well-formed UTF-8 that may be cut short at its
end — every byte 0x80-0xBF is owned by the lead byte before it, by that lead's
size.  ``in_domain`` checks it; every generator stays inside it (the surrogates and
the 4-byte sequences of codepoints >= 0x110000 decode like any other sequence).
"""
from __future__ import annotations

import numpy as np

BLK = 4096    # pretok.hip PT_BLK: bytes per workgroup
ITEMS = 16    # pretok.hip PT_ITEMS: bytes per thread

# class ids of unicode_classes.h and of the oracle's PT_* constants
LETTER, DIGIT, WS, PUNCT, SYMBOL, NL, OTHER = range(7)


def _u(*cps: int) -> list:
    return [chr(c).encode("utf-8") for c in cps]


BEYOND = [b"\xf5\x80\x80\x80", b"\xf7\xbf\xbf\xbf"]   # decode to 0x140000 and 0x1FFFFF: class Other

PALETTE = {
    LETTER: [bytes([c]) for c in b"stmdrevlSTMDREVLaxzQ"] + _u(0xE9, 0x11F, 0x4F60, 0x10437, 0x301),
    DIGIT: [bytes([c]) for c in b"0123456789"] + _u(0x663, 0xB2, 0x969, 0x1D7D8),
    WS: [b" ", b"\t"] + _u(0xA0, 0x2003, 0x3000),
    NL: [b"\n", b"\r"] + _u(0x85, 0x2028),
    PUNCT: [b"'", b"."] + _u(0x2019, 0x201C, 0x10100, 0xA1),
    SYMBOL: [b"+"] + _u(0x20AC, 0x1F600, 0xA9),
    OTHER: [b"\x01"] + _u(0x200B, 0xE000, 0x378, 0xE0001) + BEYOND,
}
APOS = [b"'", "\u2019".encode()]
SUFFIXES = [s.encode() for s in "s S t T m M d D re RE rE ve Ve ll LL lL se r l v".split()]


def fuzz(n_codepoints: int, seed: int) -> bytes:
    """About n_codepoints codepoints: iid draws (a class, then one of its pieces); with
    probability 0.2 a contraction template instead (a letter, either apostrophe, one of
    SUFFIXES, and half the time a letter), with 0.15 a run of 1-8 digits of mixed width."""
    rng = np.random.default_rng(seed)
    out, cps = [], 0
    pick = lambda pieces: pieces[int(rng.integers(0, len(pieces)))]
    while cps < n_codepoints:
        r = rng.random()
        if r < 0.2:
            suf = pick(SUFFIXES)
            out += [pick(PALETTE[LETTER]), pick(APOS), suf]
            cps += 2 + len(suf)
            if rng.integers(0, 2):
                out.append(pick(PALETTE[LETTER]))
                cps += 1
        elif r < 0.35:
            k = int(rng.integers(1, 9))
            out += [pick(PALETTE[DIGIT]) for _ in range(k)]
            cps += k
        else:
            out.append(pick(PALETTE[int(rng.integers(0, 7))]))
            cps += 1
    return b"".join(out)


# what the GPU tests run: the CPU tests assert their coverage for exactly these
FUZZ_SEEDS = (101, 102, 103, 104, 105, 106)
FUZZ_CODEPOINTS = 30_000
FUZZ_CUTS = (0, 1, 2, 3)          # bytes cut off the end
END_SEED = 107
DEVICE_SEED = 108
SYMBOLS_SEED = 109
TRAIN_SEED = 110
CHAIN_SEED = 111
CHAIN_N = 1025 * BLK + 7          # 1026 blocks: two per thread in k_pt_scan2


def end_cases(seed: int = END_SEED) -> list:
    """Short inputs that end in a contraction: for every suffix and both apostrophes, fuzz
    text of a varying length, a letter, the apostrophe, the suffix and nothing after it.
    The first ones have no text in front, so the contraction starts at byte 0."""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    for suf in SUFFIXES:
        for ap in APOS:
            letter = PALETTE[LETTER][int(rng.integers(0, len(PALETTE[LETTER])))]
            head = b"" if k < 6 else fuzz(40 + 7 * k, seed * 1000 + k)
            out.append(head + letter + ap + suf)
            k += 1
    return out


def device_corpus(seed: int = DEVICE_SEED) -> bytes:
    """a little over three blocks, behind a 3-byte ASCII prefix (so a slice that starts at
    offset 0-3 starts on a codepoint boundary)"""
    return b"abc" + fuzz(8000, seed)


def symbols_corpus(seed: int = SYMBOLS_SEED) -> bytes:
    """about 20 000 bytes behind a 1-byte ASCII prefix (a slice from offset 1 starts on a
    codepoint boundary)"""
    return b"z" + fuzz(12_300, seed)


def train_corpus(seed: int = TRAIN_SEED) -> bytes:
    """about 60 KB"""
    return fuzz(37_000, seed)


def contraction_ends(data: bytes) -> dict:
    """{"apos", "one", "two"}: offsets e such that data[:e] ends right after the apostrophe
    of a contraction, after one suffix letter, after both letters of a two-letter suffix,
    each with an ASCII letter before the apostrophe and one following at data[e] (the first
    such places after the first block)."""
    found = {}
    for ap in APOS:
        i = data.find(ap, BLK)
        while i >= 0 and len(found) < 3:
            e = i + len(ap)
            nxt = data[e:e + 3]
            after_letter = data[i - 1:i].isalpha()
            if "apos" not in found and after_letter and nxt[:1].isalpha():
                found["apos"] = e
            if after_letter and nxt[:2].lower() in (b"re", b"ve", b"ll") and nxt[2:3].isalpha():
                found.setdefault("one", e + 1)
                found.setdefault("two", e + 2)
            i = data.find(ap, e)
    assert len(found) == 3, found
    return found


def periodic(pattern: bytes, period: int) -> bytes:
    """The pattern, padded with newlines to an odd period, 4096 times, plus the first 5
    bytes of one more unit.  An odd period is coprime to 4096, so each byte of the pattern
    lands on every in-block offset 0..4095 exactly once: on offset 0, on 4095 and on every
    16-byte thread edge."""
    assert period % 2 == 1 and period > len(pattern) and period <= 41
    unit = pattern + b"\n" * (period - len(pattern))
    return unit * BLK + unit[:5]


def _digits(length: int, first: int) -> bytes:
    """a digit run of mixed width: widths first, first + 1, ... (mod 4) + 1"""
    by_width = {1: [b"7", b"0"], 2: _u(0x663, 0xB2), 3: _u(0x969), 4: _u(0x1D7D8)}
    out = []
    for k in range(length):
        w = (first + k) % 4 + 1
        out.append(by_width[w][k % len(by_width[w])])
    return b"".join(out)


def _probe_list() -> list:
    e = lambda s: s.encode("utf-8")
    probes = [
        ("contraction_2byte_letter", e("\u00e9\u2019ll x'S y\u2019Ve.")),
        ("contraction_rejected_3byte", e("\u4f60's'll a\u2019tz b'rex")),
        ("contraction_4byte_mark", e("\U00010437'd\u0301 x'm")),
        ("contraction_then_multibyte", e("a's\u00e9 b's\u20ac c\u2019ll\u4f60 d\u2019ll\u3002")),
        ("contraction_not_after_letter", e("1's 2\u2019ll e\u0301\u2019s .'t")),
        ("contraction_lookalikes", e("a'\u017f b'\u212a c\u2019\u0131l d'Ll")),   # long s, Kelvin sign, dotless i
        ("two_apostrophes", e("a''s b\u2019\u2019t c'\u2019ll d\u2019're")),
        ("contraction_chain", e("a's't\u2019re've\u2019ll'd")),
        ("ws_runs", e(" \t\u00a0\u2003\u3000a  \u30007")),
        ("ws_single", e("\u00e9\u00a0x\u20031\u3000\t. '")),
        ("newlines", e("a\u2028b\u0085c\r\nd\u2028\u20281")),
        ("symbols_punct", e("\u20ac1+\u00e9\u201cx\u201d\U0001f6007")),
        ("other_neighbours", e("\x01a\u200b1\ue000 \u0378.\U000e0001+\x01\n\u200b")),
        ("beyond_unicode", b"a" + BEYOND[0] + b"1" + BEYOND[1] + b"b7" + BEYOND[0] + b"'s"),
        ("surrogate", b"a\xed\xa0\x801\xed\xbf\xbf.\xed\xa0\x80 "),
        ("digits_then_contraction", e("12a's345\u2019ll6789")),
    ]
    for length in range(1, 8):
        probes.append((f"digits_{length}", b"x" + _digits(length, length)))
    probes.append(("digits_9_alternating", e("1\u06632\u09693\U0001d7d8456") + b"x" + _digits(3, 3)))
    out = []
    for name, pat in probes:
        period = len(pat) + 3 - len(pat) % 2      # odd, at least two newlines of padding
        out.append((name, pat, period))
    return out


PROBES = _probe_list()


def digit_chain(n: int, seed: int):
    """(bytes, mask): n bytes of ASCII digit runs separated by a single ``x``, run lengths
    drawn from 1..7, 4095, 4096, 4097, 9001 and 20000.  The mask in closed form: ``x`` is a
    start, a digit at run offset k is a start iff k % 3 == 0."""
    rng = np.random.default_rng(seed)
    lengths = np.array(list(range(1, 8)) + [4095, 4096, 4097, 9001, 20000])
    runs = lengths[rng.integers(0, len(lengths), size=n // 8 + 16)]
    ends = np.cumsum(runs + 1)                       # each run and the x after it
    xs = ends[ends <= n] - 1
    data = rng.integers(0x30, 0x3A, size=n, dtype=np.uint8)
    data[xs] = ord("x")
    idx = np.arange(n, dtype=np.int64)
    last_x = np.full(n, -1, np.int64)
    last_x[xs] = xs
    last_x = np.maximum.accumulate(last_x)
    k = idx - last_x - 1                             # offset in the digit run (-1 at an x)
    mask = ((k < 0) | (k % 3 == 0)).astype(np.uint8)
    return data.tobytes(), mask


def sweep_bmp() -> bytes:
    """every codepoint 0..0xFFFF after a letter, a digit, a full stop and a space (the
    surrogates too: they decode like any 3-byte sequence, class Other)"""
    s = "".join(c + chr(cp) for cp in range(0x10000) for c in "a1. ")
    return s.encode("utf-8", "surrogatepass")


def sweep_astral() -> bytes:
    """``a`` + every codepoint 0x10000..0x10FFFF, then ``a`` + 4-byte sequences that decode
    to 0x110000 and above (leads F4 with a second byte from 0x90, F5, F6, F7)"""
    cp = np.arange(0x10000, 0x110000, dtype=np.uint32)
    b = np.empty((cp.shape[0], 5), np.uint8)
    b[:, 0] = ord("a")
    b[:, 1] = 0xF0 | (cp >> 18)
    b[:, 2] = 0x80 | ((cp >> 12) & 0x3F)
    b[:, 3] = 0x80 | ((cp >> 6) & 0x3F)
    b[:, 4] = 0x80 | (cp & 0x3F)
    tail = []
    for lead in (0xF4, 0xF5, 0xF6, 0xF7):
        for second in range(0x90 if lead == 0xF4 else 0x80, 0xC0):
            for rest in (0x80, 0xBF):
                tail.append(bytes([ord("a"), lead, second, rest, rest]))
    return b.tobytes() + b"".join(tail)


def lead_offsets(data: bytes):
    """(offsets, sizes) of the lead bytes: every byte that is not 0x80-0xBF, with the
    sequence length its value announces"""
    a = np.frombuffer(data, np.uint8)
    pos = np.flatnonzero((a & 0xC0) != 0x80)
    lead = a[pos]
    size = np.where(lead < 0x80, 1, np.where(lead < 0xE0, 2, np.where(lead < 0xF0, 3, 4)))
    return pos, size


def in_domain(data: bytes) -> bool:
    """well-formed UTF-8 in the kernel's sense, possibly cut short at the end: the first byte
    is a lead, each lead is followed by exactly the continuation bytes its size announces
    (fewer only at the very end), no lead is 0x80-0xBF, 0xC0, 0xC1 or above 0xF7, and no
    3- or 4-byte sequence is an overlong form (the oracle maps codepoints back to bytes by
    the codepoint's own length)"""
    if not data:
        return True
    a = np.frombuffer(data, np.uint8)
    pos, size = lead_offsets(data)
    if pos.size == 0 or pos[0] != 0:
        return False
    nxt = np.append(pos[1:], len(data))
    if not np.array_equal(pos[:-1] + size[:-1], nxt[:-1]) or pos[-1] + size[-1] < len(data):
        return False
    lead = a[pos]
    if np.any((lead == 0xC0) | (lead == 0xC1) | (lead > 0xF7)):
        return False
    second = np.where(pos + 1 < len(data), a[np.minimum(pos + 1, len(data) - 1)], 0xBF)
    if np.any((lead == 0xE0) & (second < 0xA0)) or np.any((lead == 0xF0) & (second < 0x90)):
        return False
    return True
