"""Corpora of the o200k_base word-start tests — TEST INFRASTRUCTURE ONLY.

The kernels (csrc/pretok_o200k.h) mark 16 bytes per thread and 4096 per block with a
16-byte halo, look back over one codepoint and ahead over two, and carry over the blocks
the state of an 11-state automaton (forward) and two flags (backward): a newline follows
in the whitespace run, and every letter from here to the end of the letter run is
upper-only.  pretok_corpora.py's ``periodic`` puts a pattern on every in-block offset;
the generators here supply the patterns, the fuzz and the texts whose masks have a
closed form.  Everything stays in the kernels' domain (pretok_corpora.in_domain).
"""
from __future__ import annotations

import numpy as np

import cl100k_corpora as K
import pretok_corpora as P

BLK = P.BLK
e = lambda s: s.encode("utf-8")

X = "\u4e2d"      # Lo: in both letter sets
MK = "\u0301"     # Mn

# every class in every UTF-8 width it exists in
UPPER_STR = "ASTDMLVRE\u00c9\u01c5\u1e00\u212a\U0001040f"          # Lu, Lt (U+01C5), the Kelvin sign
LOWER_STR = "astdmlvrex\u00e9\u017f\u1e01\U00010437"
BOTH_STR = "\u00aa\u02b0\u4f60\u4e2d\U00020000"                     # Lo, Lm
MARK_STR = "\u0301\u0903\U000e0100"                                 # Mn, Mc
NUMBER_STR = "07\u0663\u00b2\u0969\U0001d7d8"
OTHER_STR = "/''\u2019.,!\u20ac\U0001f600\x01\x1c\x1f\u200b"
BLANK_STR = " \t\x0b\x0c\x85\u00a0\u2003\u2028\u3000"
NEWLINE_STR = "\n\r"
PALETTE_STR = UPPER_STR + LOWER_STR + BOTH_STR + MARK_STR + NUMBER_STR + OTHER_STR + BLANK_STR + NEWLINE_STR
HOST_FUZZ_SEED = 301
HOST_FUZZ_STRINGS = 40_000

_pieces = lambda s: [e(c) for c in s]
UPPERS, LOWERS, BOTHS, MARKS = _pieces(UPPER_STR), _pieces(LOWER_STR), _pieces(BOTH_STR), _pieces(MARK_STR)
NUMBERS = [bytes([c]) for c in b"0123456789"] + _pieces(NUMBER_STR[2:])
OTHERS = _pieces(OTHER_STR) + P.BEYOND
BLANKS = [b" ", b" ", b" "] + _pieces(BLANK_STR)
NEWLINES = [b"\n", b"\n", b"\r"]
CLASSES = [UPPERS, LOWERS, BOTHS, MARKS, NUMBERS, BLANKS, NEWLINES, OTHERS]
LETTERISH = [UPPERS, UPPERS, LOWERS, LOWERS, BOTHS, MARKS]
SUFFIXES = K.SUFFIXES

FUZZ_SEEDS = (311, 312, 313, 314)
FUZZ_CODEPOINTS = 30_000
FUZZ_CUTS = (0, 1, 2, 3)


def fuzz(n_codepoints: int, seed: int) -> bytes:
    """About n_codepoints codepoints.  With probability 0.2 a letter run of 1-8 drawn from the
    upper-only, lower-only and both-sided letters and the marks (case splits, the backtrack);
    0.1 one or two "other"s, a run of 1-3 marks and half the time a letter; 0.12 a chain of 1-4
    contractions after nothing, a blank, an "other" or a letter; 0.08 "other"s and then 0-5 of
    newline and `/`; 0.08 a run of 1-8 numbers; 0.12 a whitespace run of 1-6 with newlines in
    it; else one iid draw (a class, then one of its pieces)."""
    rng = np.random.default_rng(seed)
    out, cps = [], 0
    pick = lambda pieces: pieces[int(rng.integers(0, len(pieces)))]
    while cps < n_codepoints:
        r = rng.random()
        if r < 0.2:
            part = [pick(pick(LETTERISH)) for _ in range(int(rng.integers(1, 9)))]
        elif r < 0.3:
            part = [pick(OTHERS) for _ in range(int(rng.integers(1, 3)))] + \
                   [pick(MARKS) for _ in range(int(rng.integers(1, 4)))] + ([pick(LOWERS + UPPERS)] if rng.integers(0, 2) else [])
        elif r < 0.42:
            part = [[], [pick(BLANKS)], [pick(OTHERS)], [pick(LOWERS)], [pick(UPPERS)], [pick(MARKS)]][int(rng.integers(0, 6))]
            for _ in range(int(rng.integers(1, 5))):
                part = part + [pick([b"'", b"'", b"'", e("\u2019")]), pick(SUFFIXES)]
            part = part + ([pick(LOWERS + UPPERS)] if rng.integers(0, 2) else [])
        elif r < 0.5:
            part = [pick(OTHERS) for _ in range(int(rng.integers(1, 3)))] + \
                   [pick([b"\n", b"\r", b"/", b"/"]) for _ in range(int(rng.integers(0, 6)))]
        elif r < 0.58:
            part = [pick(NUMBERS) for _ in range(int(rng.integers(1, 9)))]
        elif r < 0.7:
            part = [pick(NEWLINES) if rng.random() < 0.35 else pick(BLANKS) for _ in range(int(rng.integers(1, 7)))]
        else:
            part = [pick(CLASSES[int(rng.integers(0, 8))])]
        out += part
        cps += sum(len(P.lead_offsets(p)[0]) for p in part)
    return b"".join(out)


# ── known answers: the pattern against the `regex` module, `|` between the matches ─────────
KNOWN = [
    ("abCd", "ab|Cd"), ("ABc", "ABc"), ("ABC", "ABC"),
    ("camelCaseHTTPServer XMLHttp", "camel|Case|HTTPServer| XMLHttp"),
    (f"A{X}B", f"A{X}|B"), (f"A{X}Bc", f"A{X}Bc"), (f"A{X}BCD", f"A{X}|BCD"), (f"a{X}B", f"a{X}|B"),
    (f"{MK}AB", f"{MK}|AB"), (f" {MK}AB", f" {MK}|AB"), (f"1{MK}a", f"1|{MK}a"), (f"A{MK}B", f"A{MK}|B"),
    (f"a{MK}'s", f"a{MK}'s"),
    (f"!{MK}a", f"!{MK}a"), (f"!!{MK}a", f"!!{MK}|a"), (f" !{MK}a", f" !{MK}|a"),
    ("don't stop", "don't| stop"), ("DON'T", "DON'T"), ("HTTPServer's x", "HTTPServer's| x"),
    (f"it's{X}", f"it's|{X}"), ("A'sb", "A's|b"), ("aB'sC", "a|B's|C"), ("x'\u017fy", "x'\u017f|y"),
    ("a'LLama", "a'LL|ama"),
    ("a'l", "a|'l"), ("a''s", "a|''|s"), (".'s", ".'|s"), ("a 's", "a| '|s"), ("!!'s", "!!'|s"),
    ("a's's", "a's|'s"), ("a's's's's's", "a's|'s's|'s's"), ("'s's's", "'s's|'s"),
    ("a'll'll'll", "a'll|'ll'll"), ("a'sb's", "a's|b's"), ("a'll'd", "a'll|'d"),
    ("a/\n/b", "a|/\n/|b"), ("!\n/\n a", "!\n/\n| a"), ("!\n/!/", "!\n/|!/"), ("a\n/b", "a|\n|/b"),
    ("  \n\n  x", "  \n\n| | x"), ("1234567", "123|456|7"), ("a.b a..b", "a|.b| a|..|b"),
    ("\u01c5a \u01c5A a\u01c5", "\u01c5a| \u01c5A| a|\u01c5"), ("a\u02b0B A\u02b0", "a\u02b0|B| A\u02b0"),
]


def _probe_list() -> list:
    probes = [
        ("case_split", e("abCd ABc camelCaseHTTPServer XMLHttp")),
        ("backtrack", e(f"A{X}B A{X}Bc A{X}BCD a{X}B")),
        ("marks_as_letters", e(f"{MK}AB  {MK}AB 1{MK}a A{MK}B a{MK}'s")),
        ("marks_after_punct", e(f"!{MK}a !!{MK}a  !{MK}a ..{MK}{MK}B")),
        ("contraction", e("don't stop DON'T HTTPServer's x")),
        ("contraction_then", e(f"it's{X} A'sb aB'sC x'\u017fy a'LLama")),
        ("not_contraction", e("a'l a''s .'s a 's !!'s a\u2019s")),
        ("chains", e("a's's 's's's a'll'll'll a'sb's a'll'd")),
        ("chain_long", e("a's's's's's \u00c9've'RE'll'D've")),
        ("slash_tail", e("a/\n/b !\n/\n a !\n/!/ a\n/b //a/ /")),
        ("blanks_digits", e("  \n\n  x 1234567 a.b a..b \r\n 9")),
        ("titlecase_modifier", e("\u01c5a \u01c5A a\u01c5 a\u02b0B A\u02b0 \u02b0\u02b0A")),
        ("wide_letters", e("\U0001040f\U00010437\U0001040f \U00020000\U0001040f \U000e0100A")),
        ("upper_then_end", e(f"AB{X}CD. AB{X}CD's AB{X}CD1 {X}A")),
    ]
    keep = ("blank_then_other", "blank_then_letters", "digits_mixed_width", "blank_then_newline", "eaten_newlines",
            "eaten_then_blank", "wide_blanks", "line_separators", "not_whitespace", "beyond_unicode", "surrogate",
            "trailing_blanks")
    out = []
    for name, pat in probes:
        period = len(pat) + 3 - len(pat) % 2      # odd, at least two newlines of padding
        out.append((name, pat, period))
    return out + [p for p in K.PROBES if p[0] in keep]


PROBES = _probe_list()
periodic = P.periodic


# ── closed forms (the states across blocks) ──────────────────────────────────
# k counts codepoints; the masks are byte masks

RUN_LENGTHS = K.RUN_LENGTHS
CHAIN_N = P.CHAIN_N          # 1026 blocks: two per thread in k_pto_scan2


def _mask(n, at):
    m = np.zeros(n, np.uint8)
    m[list(at)] = 1
    return m


def upper_run(k: int, j, tail: bytes):
    """(bytes, mask): `A` k times, the one at offset j (None: none) replaced by a both-sided letter,
    then `tail` (nothing or `c`).  With the `c` the run and it are one match.  Without it the
    run is one match when all of it is upper-only; else [..Ll..]+ needs the both-sided letter, so
    the match ends on it and the upper-only letters behind it are the next."""
    cps = ["A"] * k
    if j is not None:
        cps[j] = X
    data = e("".join(cps)) + tail
    at = [0]
    if j is not None and not tail and j + 1 < k:
        at.append(j + 3)
    return data, _mask(len(data), at)


def case_phase(k: int):
    """(bytes, mask): `a`, k both-sided letters, `B`: the B starts a match however far the a lies"""
    data = b"a" + e(X) * k + b"B"
    return data, _mask(len(data), [0, len(data) - 1])


def contraction_chain(k: int, lead: bytes):
    """(bytes, mask): `lead` (`a` or nothing) and `'s` k times.  After a letter the first 's is its
    suffix, the next is a word ('s) that takes the one after it as its suffix, and so on:
    the apostrophes alternate, from the second one after `a`, from the first one alone."""
    data = lead + b"'s" * k
    first = 1 if lead else 0
    return data, _mask(len(data), [0] + [len(lead) + 2 * i for i in range(first, k, 2)])


def marks_run(k: int, bangs: int):
    """(bytes, mask): `!` or `!!`, k marks, `a`.  One `!` is the prefix of a word made of the marks
    and the a; after two the marks are punctuation and the a stands alone."""
    data = b"!" * bangs + e(MK) * k + b"a"
    return data, _mask(len(data), [0] + ([len(data) - 1] if bangs == 2 else []))


def slash_tail(k: int):
    """(bytes, mask): `.`, then newline and `/` k times, then `!`: the tail goes with the full stop"""
    data = b"." + b"\n/" * k + b"!"
    return data, _mask(len(data), [0, len(data) - 1])


def closed_forms(k: int) -> list:
    """[(name, bytes, mask)] of every chain at run length k"""
    out = []
    for tail in (b"", b"c"):
        for j in (None, 0, k // 2, k - 1):
            out.append((f"upper_run tail {tail!r} Lo at {j}",) + upper_run(k, j, tail))
    out.append(("case_phase",) + case_phase(k))
    out.append(("contraction_chain after a",) + contraction_chain(k, b"a"))
    out.append(("contraction_chain alone",) + contraction_chain(k, b""))
    out.append(("marks after !!",) + marks_run(k, 2))
    out.append(("marks after !",) + marks_run(k, 1))
    out.append(("slash_tail",) + slash_tail(k))
    for j in (None, 0, k // 2, k - 1):
        out.append((f"blank_run newline at {j}",) + K.blank_run(k, j))
    return out


def chain_forms() -> list:
    """one of each kind over more than 1024 blocks"""
    n = CHAIN_N
    return [("upper_run Lo in the middle",) + upper_run(n, n // 2, b""),
            ("upper_run then c",) + upper_run(n, None, b"c"),
            ("case_phase",) + case_phase(n // 3 + 1),
            ("contraction_chain after a",) + contraction_chain(n // 2 + 1, b"a"),
            ("contraction_chain alone",) + contraction_chain(n // 2 + 1, b""),
            ("marks after !!",) + marks_run(n // 2 + 1, 2),
            ("marks after !",) + marks_run(n // 2 + 1, 1),
            ("slash_tail",) + slash_tail(n // 2 + 1),
            ("digits",) + K.digit_run(n),
            ("blanks",) + K.blanks_then_newline(n),
            ("eaten",) + K.eaten_run(n)]


# ── the class table ──────────────────────────────────────────────────────────
sweep_documents = K.sweep_documents

# ── many documents ───────────────────────────────────────────────────────────
# a case split, a chained contraction, a mark after punctuation, a `/` tail, a backtrack
BATCH_TEXT = e(f"camelCase a's's!{MK}a  x.\n/\n 123456  \n\n HTTPServer's A{X}B !!{MK}b\r\n")
assert len(BATCH_TEXT) == 64, len(BATCH_TEXT)
CUT_TAILS = K.CUT_TAILS


def batch_documents():
    """(bytes, offsets): for every cut c of BATCH_TEXT the documents text[:c] + tail and text[c:],
    the tail in turn nothing or a UTF-8 sequence cut short, with an empty document after
    every seventh pair.  (A cut inside a sequence leaves a document that begins with
    continuation bytes: it is cut at codepoint boundaries only.)"""
    leads = set(P.lead_offsets(BATCH_TEXT)[0].tolist()) | {len(BATCH_TEXT)}
    docs = []
    for c in sorted(leads):
        docs += [BATCH_TEXT[:c] + CUT_TAILS[c % len(CUT_TAILS)], BATCH_TEXT[c:]]
        if c % 7 == 0:
            docs.append(b"")
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return b"".join(docs), offs
