"""The o200k_base word starts without a GPU: the backtracking reference
(o200k_ref.py, written from the pattern) against the `regex` module and against known
answers, the generated class table against unicodedata, the corpora's closed forms against
the reference, and the header, the library and the bindings for the new entry points."""
from __future__ import annotations

import os
import re
import sys
import unicodedata

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import o200k_corpora as K  # noqa: E402
import o200k_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

# \s and \S written out as the White_Space property: `regex` counts U+001C-U+001F as
# whitespace, Rust's regex (tiktoken) does not
WS = "\\t-\\r \\x85\\xa0\\u1680\\u2000-\\u200a\\u2028\\u2029\\u202f\\u205f\\u3000"
PATTERN = (r"[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
           r"|[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
           r"|\p{N}{1,3}| ?[^WS\p{L}\p{N}]+[\r\n/]*|[WS]*[\r\n]+|[WS]+(?![^WS])|[WS]+").replace("WS", WS)

NON_SURROGATE = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]


@pytest.fixture(scope="module")
def rx():
    return pytest.importorskip("regex")


@pytest.fixture(scope="module")
def agreeing(rx):
    """The codepoints whose table class agrees with regex's own properties, over the eight classes."""
    every = "".join(map(chr, NON_SURROGATE))
    sets = {name: {ord(c) for c in rx.findall(pat, every)}
            for name, pat in (("U", r"[\p{Lu}\p{Lt}]"), ("L", r"\p{Ll}"), ("B", r"[\p{Lm}\p{Lo}]"), ("M", r"\p{M}"),
                              ("N", r"\p{N}"))}
    by_class = {R.U: "U", R.L: "L", R.B: "B", R.M: "M", R.N: "N"}
    ok = set()
    for cp in NON_SURROGATE:
        k = by_class.get(R.klass(cp))
        if all((name == k) == (cp in s) for name, s in sets.items()):
            ok.add(cp)
    left_out = len(NON_SURROGATE) - len(ok)
    print(f"table (Unicode {R.tables()[0]}) and regex {rx.__version__} disagree on {left_out} of "
          f"{len(NON_SURROGATE)} codepoints ({100 * left_out / len(NON_SURROGATE):.2f} %)")
    assert left_out <= 0.02 * len(NON_SURROGATE)
    return ok


def regex_starts(rx_compiled, s: str):
    out = [0] * len(s)
    pos = 0
    for m in rx_compiled.finditer(s):
        assert m.start() == pos and m.end() > pos, "the matches must cover the text"
        out[pos] = 1
        pos = m.end()
    assert pos == len(s)
    return out


def test_matcher_against_regex_fuzz(rx, agreeing):
    pat = rx.compile(PATTERN)
    palette = [ord(c) for c in K.PALETTE_STR]
    assert all(cp in agreeing for cp in palette), [hex(cp) for cp in palette if cp not in agreeing]
    assert {R.klass(cp) for cp in palette} == set(range(8))
    rng = np.random.default_rng(K.HOST_FUZZ_SEED)
    assert K.HOST_FUZZ_STRINGS >= 40_000
    for _ in range(K.HOST_FUZZ_STRINGS):
        cps = [palette[i] for i in rng.integers(0, len(palette), size=int(rng.integers(1, 15)))]
        s = "".join(map(chr, cps))
        assert R.starts(cps) == regex_starts(pat, s), repr(s)


def test_matcher_against_regex_templates(rx, agreeing):
    """the GPU fuzz's templates (case-mixed runs, marks after punctuation, contraction chains,
    `/` tails) as short strings: what iid draws reach rarely"""
    pat = rx.compile(PATTERN)
    data = K.fuzz(12_000, 302)
    cps, _ = R.decode(data)
    cps = [cp for cp in cps if cp in agreeing]
    for a in range(0, len(cps) - 24, 11):
        piece = cps[a:a + 24]
        assert R.starts(piece) == regex_starts(pat, "".join(map(chr, piece))), repr("".join(map(chr, piece)))


def test_matcher_against_regex_every_codepoint(rx, agreeing):
    """`a` c `b`, `A` c `B`, `!` c `a` and ` ` c `1` for every codepoint c: every class in four neighbourhoods"""
    pat = rx.compile(PATTERN)
    seen = {}   # the answer depends on c through its class and the few codepoints the pattern names
    for cp in sorted(agreeing):
        for a, b in (("a", "b"), ("A", "B"), ("!", "a"), (" ", "1")):
            s = a + chr(cp) + b
            got = R.starts([ord(a), cp, ord(b)])
            assert got == regex_starts(pat, s), repr(s)
            seen.setdefault((a, R.klass(cp)), set()).add(tuple(got))
    assert len(seen) == 32


def test_table_against_unicodedata():
    stamp, _, _ = R.tables()
    if stamp != unicodedata.unidata_version:
        pytest.skip(f"the table is Unicode {stamp}, this Python has {unicodedata.unidata_version}")
    white = set(range(0x09, 0x0E)) | {0x20, 0x85, 0xA0, 0x1680} | set(range(0x2000, 0x200B)) | \
        {0x2028, 0x2029, 0x202F, 0x205F, 0x3000}
    assert len(white) == 25
    for cp in range(0x110000):
        cat = unicodedata.category(chr(cp))
        want = R.R if cp in (0x0A, 0x0D) else R.W if cp in white else R.U if cat in ("Lu", "Lt") else \
            R.L if cat == "Ll" else R.B if cat in ("Lm", "Lo") else R.M if cat[0] == "M" else R.N if cat[0] == "N" else R.O
        assert R.klass(cp) == want, hex(cp)
    assert R.klass(0x110000) == R.O and R.klass(0x301) == R.M and R.klass(0x1C) == R.O and R.klass(0x85) == R.W
    assert R.klass(0x1C5) == R.U and R.klass(0x2B0) == R.B and R.klass(0x17F) == R.L and R.klass(0x212A) == R.U


def test_generator_reproduces_all_three_headers(tmp_path):
    """tools/gen_unicode_classes.py writes the three committed headers byte for byte (on the
    Unicode version they are stamped with)."""
    if R.tables()[0] != unicodedata.unidata_version:
        pytest.skip("another Unicode version")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_unicode_classes", os.path.join(ROOT, "tools", "gen_unicode_classes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    csrc = os.path.join(ROOT, "gpu-bpe_amd", "csrc")
    for name, classify, prefix in (("unicode_classes.h", gen.classify, "kUni"),
                                   ("unicode_classes_cl100k.h", gen.classify_cl100k, "kCl100k"),
                                   ("unicode_classes_o200k.h", gen.classify_o200k, "kO200k")):
        text = open(os.path.join(csrc, name), encoding="utf-8").read()
        legend = "".join(line + "\n" for line in text.split("\n")[1:3])
        out = tmp_path / name
        gen.write_table(name, classify, legend, prefix, str(out))
        assert out.read_text(encoding="utf-8") == text, name


@pytest.mark.parametrize("text,want", K.KNOWN, ids=[repr(t)[:24] for t, _ in K.KNOWN])
def test_known_answers(text, want):
    assert R.pieces(text) == want.split("|")
    data = text.encode()
    cuts = np.flatnonzero(R.mask(data)).tolist() + [len(data)]
    assert [data[a:b].decode() for a, b in zip(cuts[:-1], cuts[1:])] == want.split("|")


def test_known_answers_against_regex(rx):
    pat = rx.compile(PATTERN)
    for text, want in K.KNOWN:
        assert [m.group() for m in pat.finditer(text)] == want.split("|"), text


def test_corpora_hold_what_the_gpu_tests_need():
    """every generator stays in the kernels' domain, and the closed forms are the reference's"""
    import pretok_corpora as P
    for seed in K.FUZZ_SEEDS:
        data = K.fuzz(K.FUZZ_CODEPOINTS, seed)
        assert P.in_domain(data) and len(data) > 10 * P.BLK
    data = K.fuzz(K.FUZZ_CODEPOINTS, K.FUZZ_SEEDS[0])
    pieces = [data[a:b] for a, b in zip(*(lambda c: (c[:-1], c[1:]))(np.flatnonzero(R.mask(data)).tolist() + [len(data)]))]
    text = [p.decode("utf-8", "replace") for p in pieces]
    # case splits, marks inside punctuation, chained contractions and `/` tails all occur
    assert sum(1 for a, b in zip(pieces[:-1], pieces[1:]) if a[-1:].islower() and b[:1].isupper()) > 50
    assert sum(1 for t in text if len(t) > 2 and t[0] in ".,!/" and t[1] in ".,!/'" and K.MK in t) > 5
    assert sum(1 for a, b in zip(text[:-1], text[1:]) if a[-2:-1] == "'" and b[:1] == "'" and b.count("'") == 2) > 20
    assert sum(1 for t in text if "\n/" in t or "//" in t) > 20
    for name, pat, period in K.PROBES:
        assert P.in_domain(K.periodic(pat, period)), name
    for t, _ in K.KNOWN:                                   # every known-answer family is in a probe
        assert any(t.encode() in pat for _, pat, _ in K.PROBES) or t in ("ABC",), t
    for k in (5, 16, 300) + K.RUN_LENGTHS[:1]:
        for name, data, m in K.closed_forms(k):
            assert P.in_domain(data), name
            assert np.array_equal(R.mask(data), m), (k, name)
    for name, data, m in ((n,) + f for n, f in (("eaten", K.K.eaten_run(2 * P.BLK + 3)), ("digits", K.K.digit_run(10_001)),
                                               ("blanks", K.K.blanks_then_newline(10_001)))):
        assert np.array_equal(R.mask(data), m), name
    assert -(-K.CHAIN_N // P.BLK) > 1024               # two blocks per scan thread
    data, offs = K.batch_documents()
    assert offs[0] == 0 and offs[-1] == len(data) and any(a == b for a, b in zip(offs[:-1], offs[1:]))
    assert all(P.in_domain(data[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:]))
    got = R.pieces(K.BATCH_TEXT.decode())
    assert {"camel", "Case", " a's", "'s", f"!{K.MK}a", f" !!{K.MK}", ".\n/\n", f" A{K.X}", "B", " HTTPServer's"} <= set(got), got


NEW = ("gbpe_pretokenize_o200k", "gbpe_pretokenize_o200k_device", "gbpe_pretokenize_o200k_batch",
       "gbpe_pretokenize_o200k_batch_device")


def test_header_library_and_bindings_cover_the_new_entry_points():
    from gpubpe import _lib, merge_encoder, pretokenizer
    header = open(os.path.join(ROOT, "include", "gpubpe.h")).read()
    assert re.search(r"#define GBPE_WORDS_O200K\s+6u", header)
    assert re.search(r"#define GBPE_WORDS_CL100K\s+4u", header)
    assert re.search(r"#define GBPE_ABI_VERSION 10\b", header)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in _lib.EXPORTED, name
    assert _lib.GBPE_WORDS_O200K == 6 and merge_encoder.WORDS_MODES["o200k_base"] == 6
    assert sorted(merge_encoder.WORDS_MODES.values()) == [2, 3, 4, 6]
    assert "o200k_base" in pretokenizer.RULES and "o200k" not in pretokenizer.RULES
    mode, mask = merge_encoder.checked_word_starts(3, None, "o200k_base")
    assert mode == 6 and mask is None
    with pytest.raises(_lib.GpuBpeError, match="o200k_base"):
        merge_encoder.checked_word_starts(3, None, "o200k")
    with pytest.raises(ValueError, match="o200k_base"):
        pretokenizer.GpuPreTokenizer(None).pre_tokenize_bytes(b"a", rules="o200k")
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in NEW:
            assert hasattr(lib, name), name
        names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
        assert "k_pretok_o200k" in names and "k_pretok_o200k_docs" in names and len(names) == len(set(names))
