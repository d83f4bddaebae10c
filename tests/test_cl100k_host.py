"""The cl100k_base word starts without a GPU: the sequential reference
(cl100k_ref.py, written from the pattern) against the `regex` module and against
known answers, the generated class table against unicodedata, and the header, the
library and the bindings for the new entry points."""
from __future__ import annotations

import os
import re
import sys
import unicodedata

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cl100k_corpora as K  # noqa: E402
import cl100k_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

# \s and \S written out as the White_Space property: `regex` counts U+001C-U+001F as
# whitespace, Rust's regex (tiktoken) does not
WS = "\\t-\\r \\x85\\xa0\\u1680\\u2000-\\u200a\\u2028\\u2029\\u202f\\u205f\\u3000"
PATTERN = (r"'(?i:[sdmt]|ll|ve|re)|[^\r\n\p{L}\p{N}]?+\p{L}+|\p{N}{1,3}| ?[^WS\p{L}\p{N}]++[\r\n]*"
           r"|[WS]*[\r\n]|[WS]+(?![^WS])|[WS]+").replace("WS", WS)

NON_SURROGATE = [cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000]


@pytest.fixture(scope="module")
def rx():
    return pytest.importorskip("regex")


@pytest.fixture(scope="module")
def agreeing(rx):
    """The codepoints whose table class agrees with regex's own \\p{L} and \\p{N}."""
    every = "".join(map(chr, NON_SURROGATE))
    letters = {ord(c) for c in rx.findall(r"\p{L}", every)}
    numbers = {ord(c) for c in rx.findall(r"\p{N}", every)}
    ok = {cp for cp in NON_SURROGATE
          if (R.klass(cp) == R.L) == (cp in letters) and (R.klass(cp) == R.N) == (cp in numbers)}
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
    rng = np.random.default_rng(K.HOST_FUZZ_SEED)
    for _ in range(K.HOST_FUZZ_STRINGS):
        cps = [palette[i] for i in rng.integers(0, len(palette), size=int(rng.integers(1, 15)))]
        s = "".join(map(chr, cps))
        assert R.starts(cps) == regex_starts(pat, s), repr(s)


def test_matcher_against_regex_every_codepoint(rx, agreeing):
    """`a` c `b` and ` ` c `1` for every codepoint c: every class in both neighbourhoods"""
    pat = rx.compile(PATTERN)
    seen = {}   # the answer depends on c through its class and the few codepoints the pattern names
    for cp in sorted(agreeing):
        for a, b in (("a", "b"), (" ", "1")):
            s = a + chr(cp) + b
            got = R.starts([ord(a), cp, ord(b)])
            assert got == regex_starts(pat, s), repr(s)
            seen.setdefault((a, R.klass(cp)), set()).add(tuple(got))
    assert len(seen) == 10


def test_table_against_unicodedata():
    stamp, _, _ = R.tables()
    if stamp != unicodedata.unidata_version:
        pytest.skip(f"the table is Unicode {stamp}, this Python has {unicodedata.unidata_version}")
    white = set(range(0x09, 0x0E)) | {0x20, 0x85, 0xA0, 0x1680} | set(range(0x2000, 0x200B)) | \
        {0x2028, 0x2029, 0x202F, 0x205F, 0x3000}
    assert len(white) == 25
    for cp in range(0x110000):
        cat = unicodedata.category(chr(cp))[0]
        want = R.R if cp in (0x0A, 0x0D) else R.W if cp in white else R.L if cat == "L" else R.N if cat == "N" else R.O
        assert R.klass(cp) == want, hex(cp)
    assert R.klass(0x110000) == R.O and R.klass(0x301) == R.O and R.klass(0x1C) == R.O and R.klass(0x85) == R.W


def test_generator_reproduces_both_headers(tmp_path):
    """tools/gen_unicode_classes.py writes the two committed headers byte for byte (on the
    Unicode version they are stamped with)."""
    if R.tables()[0] != unicodedata.unidata_version:
        pytest.skip("another Unicode version")
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_unicode_classes", os.path.join(ROOT, "tools", "gen_unicode_classes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    csrc = os.path.join(ROOT, "gpu-bpe_amd", "csrc")
    for name, classify, prefix in (("unicode_classes.h", gen.classify, "kUni"),
                                   ("unicode_classes_cl100k.h", gen.classify_cl100k, "kCl100k")):
        text = open(os.path.join(csrc, name), encoding="utf-8").read()
        legend = "".join(line + "\n" for line in text.split("\n")[1:3])
        out = tmp_path / name
        gen.write_table(name, classify, legend, prefix, str(out))
        assert out.read_text(encoding="utf-8") == text, name


KNOWN = [
    ("don't  stop\n\n  x 'tis 1234567 a.b a..b",
     "don|'t| | stop|\n\n| | x| '|tis| |123|456|7| a|.b| a|..|b"),
    ("it'\u017f", "it|'\u017f"),                 # the long s folds to s
    ("it\u2019s", "it|\u2019s"),                 # U+2019 opens no contraction: it is the letters' prefix
    ("'there", "'t|here"),
    ("''s", "''|s"),
    (".\n\n x", ".\n\n| x"),
    ("a\u0301b", "a|\u0301b"),                   # a mark is not a letter
    ("x \t\ny", "x| \t\n|y"),
    ("a   ", "a|   "),
    ("   ", "   "),
    ("a\x1cb", "a|\x1cb"),                       # U+001C is not whitespace
    ("A'LL'Ve'rE", "A|'LL|'Ve|'rE"),
    ("a \u2028\u0085\nb", "a| \u2028\u0085\n|b"),   # U+2028 and U+0085 are plain whitespace
    ("a\u2028\u2028b", "a|\u2028|\u2028b"),
]


@pytest.mark.parametrize("text,want", KNOWN, ids=[repr(t)[:24] for t, _ in KNOWN])
def test_known_answers(text, want):
    assert R.pieces(text) == want.split("|")
    data = text.encode()
    cuts = np.flatnonzero(R.mask(data)).tolist() + [len(data)]
    assert [data[a:b].decode() for a, b in zip(cuts[:-1], cuts[1:])] == want.split("|")


def test_corpora_hold_what_the_gpu_tests_need():
    """every generator stays in the kernels' domain, and the closed forms are the reference's"""
    import pretok_corpora as P
    for seed in K.FUZZ_SEEDS:
        data = K.fuzz(K.FUZZ_CODEPOINTS, seed)
        assert P.in_domain(data) and len(data) > 10 * P.BLK
    for name, pat, period in K.PROBES:
        assert P.in_domain(K.periodic(pat, period)), name
    for k in K.RUN_LENGTHS:
        for j in (None, 0, k // 2, k - 1):
            data, m = K.blank_run(k, j)
            assert np.array_equal(R.mask(data), m), (k, j)
    for j in (None, 0):
        data, m = K.blank_run(1, j)
        assert np.array_equal(R.mask(data), m), j
    for data, m in (K.eaten_run(2 * P.BLK + 3), K.digit_run(10_001), K.blanks_then_newline(10_001)):
        assert np.array_equal(R.mask(data), m)
    assert -(-K.CHAIN_N // P.BLK) > 1024               # two blocks per scan thread
    data, offs = K.batch_documents()
    assert offs[0] == 0 and offs[-1] == len(data) and any(a == b for a, b in zip(offs[:-1], offs[1:]))
    for lo, hi in ((0x7E, 0x82), (0x7FE, 0x802), (0xD7FE, 0xD802), (0xFFFE, 0x10002)):
        data, offs = K.sweep_documents(lo, hi)
        docs = [data[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
        assert docs == [b"a" + chr(cp).encode("utf-8", "surrogatepass") + b"b" for cp in range(lo, hi)]


NEW = ("gbpe_pretokenize_cl100k", "gbpe_pretokenize_cl100k_device", "gbpe_pretokenize_cl100k_batch",
       "gbpe_pretokenize_cl100k_batch_device")


def test_header_library_and_bindings_cover_the_new_entry_points():
    from gpubpe import _lib, merge_encoder, pretokenizer
    header = open(os.path.join(ROOT, "include", "gpubpe.h")).read()
    assert re.search(r"#define GBPE_WORDS_CL100K\s+4u", header)
    assert re.search(r"#define GBPE_ABI_VERSION 10\b", header)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in _lib.EXPORTED, name
    assert _lib.GBPE_WORDS_CL100K == 4 and merge_encoder.WORDS_MODES["cl100k"] == 4
    assert "cl100k" in pretokenizer.RULES
    mode, mask = merge_encoder.checked_word_starts(3, None, "cl100k")
    assert mode == 4 and mask is None
    with pytest.raises(_lib.GpuBpeError):
        merge_encoder.checked_word_starts(3, None, "o200k")
    with pytest.raises(ValueError):
        pretokenizer.GpuPreTokenizer(None).pre_tokenize_bytes(b"a", rules="o200k")
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in NEW:
            assert hasattr(lib, name), name
        names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
        assert "k_pretok_cl100k" in names and "k_pretok_cl100k_docs" in names and len(names) == len(set(names))
