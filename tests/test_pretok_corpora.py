"""The corpora of test_gpu_pretok_rules.py can fail a wrong kernel: what they hold, and
where it lands relative to the 4096-byte blocks and 16-byte threads of pretok.hip, is
asserted here from the bytes and the oracle's classes (no GPU).  Plus the device class
table (unicode_classes.h) against the oracle's classifier."""
from __future__ import annotations

import os
import re
import sys
import unicodedata

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import bpe_oracle as O  # noqa: E402
import pretok_corpora as P  # noqa: E402

CLASSES = (O.PT_LETTER, O.PT_DIGIT, O.PT_WHITESPACE, O.PT_PUNCT, O.PT_SYMBOL, O.PT_NEWLINE, O.PT_OTHER)
UNI_HEADER = os.path.join(os.path.dirname(HERE), "gpu-bpe_amd", "csrc", "unicode_classes.h")


def test_class_ids_are_the_oracles():
    assert (P.LETTER, P.DIGIT, P.WS, P.PUNCT, P.SYMBOL, P.NL, P.OTHER) == CLASSES


@pytest.fixture(scope="module")
def all_classes():
    """the oracle's class of every codepoint below 0x110000"""
    return np.array([O.pt_classify(cp) for cp in range(0x110000)], np.uint8)


@pytest.fixture(scope="module")
def fuzz_decoded():
    """[(data, cps, sizes, classes)] of the fuzz corpora the GPU tests run"""
    out = []
    for seed in P.FUZZ_SEEDS:
        data = P.fuzz(P.FUZZ_CODEPOINTS, seed)
        cps, sizes = O.utf8_to_codepoints(data)
        out.append((data, cps, sizes, [O.pt_classify(c) for c in cps]))
    return out


def test_palette_pieces_have_their_class(all_classes):
    assert sorted(P.PALETTE) == sorted(CLASSES)
    width_of = np.array([O._utf8_len(cp) for cp in range(0x110000)], np.uint8)
    for cls, pieces in P.PALETTE.items():
        assert len(set(pieces)) == len(pieces)
        widths = set()
        for piece in pieces:
            cps, sizes = O.utf8_to_codepoints(piece)
            assert len(cps) == 1 and sizes[0] == len(piece), piece
            assert O.pt_classify(cps[0]) == cls, (piece, cls)
            widths.add(len(piece))
        # every UTF-8 width in which the class exists at all
        assert widths == set(np.unique(width_of[all_classes == cls]).tolist()), (cls, widths)
    for piece in P.BEYOND:
        assert O.utf8_to_codepoints(piece)[0][0] >= 0x110000 and piece in P.PALETTE[P.OTHER]
    for ch in "stmdrevl":
        assert ch.encode() in P.PALETTE[P.LETTER] and ch.upper().encode() in P.PALETTE[P.LETTER]


def test_in_domain_rejects_what_the_kernel_is_not_written_for():
    for bad in (b"\x80a", b"a\xc3\xa9\x80", b"\xe4\xbda", b"\xc0\x80", b"\xe0\x80\x80", b"\xf0\x80\x80\x80",
                b"a\xf8\x80\x80\x80"):
        assert not P.in_domain(bad), bad
    for good in (b"", b"a", b"a\xc3", "é你\U00010437".encode(), "a你".encode()[:-1], "\U00010437".encode()[:1],
                 b"\xed\xa0\x80", P.BEYOND[0] + P.BEYOND[1]):
        assert P.in_domain(good), good


def test_every_generator_stays_in_the_domain():
    for seed in P.FUZZ_SEEDS:
        data = P.fuzz(P.FUZZ_CODEPOINTS, seed)
        for cut in P.FUZZ_CUTS:
            assert P.in_domain(data[:len(data) - cut]), (seed, cut)
    for case in P.end_cases():
        assert P.in_domain(case)
    for name, pat, period in P.PROBES:
        assert P.in_domain(P.periodic(pat, period)), name
    assert P.in_domain(P.digit_chain(60_000, P.CHAIN_SEED)[0])
    assert P.in_domain(P.sweep_bmp()) and P.in_domain(P.sweep_astral())
    assert P.in_domain(P.train_corpus())
    for data, offsets in ((P.device_corpus(), (0, 1, 2, 3)), (P.symbols_corpus(), (0, 1))):
        leads = set(P.lead_offsets(data)[0].tolist())
        assert P.in_domain(data) and all(a in leads for a in offsets)   # a cut at any end stays inside


def test_fuzz_holds_every_class_pair(fuzz_decoded):
    pairs = set()
    for _, _, _, cls in fuzz_decoded:
        pairs |= set(zip(cls[:-1], cls[1:]))
    assert len(pairs) == 49


def _contractions(cps, cls):
    """(suffix, apostrophe, what follows) of every letter + apostrophe + suffix in the text;
    what follows is "letter", "other" or "end" """
    suffixes = [(s, [c for c in s]) for s in P.SUFFIXES]
    for i in range(1, len(cps)):
        if cps[i] not in (0x27, 0x2019) or cls[i - 1] != O.PT_LETTER:
            continue
        for s, want in suffixes:
            j = i + 1 + len(want)
            if cps[i + 1:j] == want:
                follow = "end" if j >= len(cps) else "letter" if cls[j] == O.PT_LETTER else "other"
                yield s, cps[i], follow


def test_fuzz_holds_every_contraction_form(fuzz_decoded):
    seen = set()
    for _, cps, _, cls in fuzz_decoded:
        seen |= set(_contractions(cps, cls))
    at_zero = 0
    for case in P.end_cases():
        cps, _ = O.utf8_to_codepoints(case)
        cls = [O.pt_classify(c) for c in cps]
        ends = [c for c in _contractions(cps, cls) if c[2] == "end"]
        assert ends, case
        seen |= set(ends)
        at_zero += len(cps) == 2 + len(ends[-1][0])
    assert at_zero >= 4                       # a contraction whose letter is the input's first byte
    for s in P.SUFFIXES:
        for ap in (0x27, 0x2019):
            assert any((s, ap, f) in seen for f in ("letter", "other", "end")), (s, ap)
            assert (s, ap, "end") in seen, (s, ap)
        for follow in ("letter", "other", "end"):
            assert any((s, ap, follow) in seen for ap in (0x27, 0x2019)), (s, follow)


def test_fuzz_holds_digit_runs_of_every_length_and_first_width(fuzz_decoded):
    seen = set()
    for _, _, sizes, cls in fuzz_decoded:
        i = 0
        while i < len(cls):
            if cls[i] != O.PT_DIGIT:
                i += 1
                continue
            j = i
            while j < len(cls) and cls[j] == O.PT_DIGIT:
                j += 1
            seen.add((j - i, sizes[i]))
            i = j
    for length in range(1, 9):
        for width in (1, 2, 3, 4):
            assert (length, width) in seen, (length, width)


def test_fuzz_cuts_land_inside_a_codepoint(fuzz_decoded):
    for cut in (1, 2, 3):
        inside = 0
        for data, _, _, _ in fuzz_decoded:
            pos, size = P.lead_offsets(data[:len(data) - cut])
            inside += int(pos[-1] + size[-1] > len(data) - cut)
        assert inside >= 1, cut


def test_device_and_symbol_corpora_fit_their_cases():
    data = P.device_corpus()
    assert 3 * P.BLK + 3 < len(data) - 3 and 8195 + 3 <= len(data) < 4 * P.BLK
    ends = P.contraction_ends(data)
    e = ends["apos"]
    assert data[:e].endswith(tuple(P.APOS)) and data[e:e + 1].isalpha() and e > P.BLK + 3
    e = ends["one"]
    assert data[e - 1:e + 1].lower() in (b"re", b"ve", b"ll") and data[e + 1:e + 2].isalpha()
    assert ends["two"] == e + 1
    sym = P.symbols_corpus()
    assert 19_000 < len(sym) < 21_000 and len(sym) - 1 > 4111
    assert 55_000 < len(P.train_corpus()) < 65_000


@pytest.mark.parametrize("name,pat,period", P.PROBES, ids=[p[0] for p in P.PROBES])
def test_periodic_probe_reaches_every_edge(name, pat, period):
    data = P.periodic(pat, period)
    assert len(data) == P.BLK * period + 5 and len(data) <= 41 * P.BLK + 5
    pos, size = P.lead_offsets(data)
    unit = pos % period
    for j, sz in sorted({(int(u), int(s)) for u, s in zip(unit[:200], size[:200]) if u < len(pat)}):
        at = set((pos[unit == j] % P.BLK).tolist())
        assert {0, P.BLK - 1} <= at, (name, j)
        assert set(range(0, P.BLK, P.ITEMS)) <= at               # the first byte of every thread
        assert set(range(P.ITEMS - 1, P.BLK, P.ITEMS)) <= at     # and the last
        for k in range(1, sz):                # the block edge falls before its k-th byte
            assert 0 in set(((pos[unit == j] + k) % P.BLK).tolist()), (name, j, k)
    assert set(np.unique(unit[unit < len(pat)]).tolist()) == set(P.lead_offsets(pat)[0].tolist())


def test_probes_cover_the_listed_rules():
    names = {p[0] for p in P.PROBES}
    assert len(names) == len(P.PROBES)
    assert {f"digits_{k}" for k in range(1, 8)} <= names
    for _, pat, _ in P.PROBES:
        assert b"\n" not in pat[:1] and len(pat) <= 38


def test_digit_chain_closed_form_is_the_oracle():
    data, mask = P.digit_chain(60_000, P.CHAIN_SEED)
    assert len(data) == 60_000 and data.count(b"x") >= 5
    np.testing.assert_array_equal(O.gpt4_word_starts(data), mask)
    big, _ = P.digit_chain(P.CHAIN_N, P.CHAIN_SEED)
    assert len(big) == P.CHAIN_N and -(-P.CHAIN_N // P.BLK) > 1024    # two blocks per k_pt_scan2 thread
    runs = {len(r) for r in big.split(b"x")[:-1]}
    assert set(range(1, 8)) | {4095, 4096, 4097, 9001, 20000} == runs


def _parse_table(text: str, name: str) -> np.ndarray:
    m = re.search(name + r"\[(\d+)\]\s*=\s*\{([^}]*)\}", text)
    vals = np.array([int(v) for v in m.group(2).replace("\n", " ").split(",") if v.strip()], np.int64)
    assert vals.shape[0] == int(m.group(1))
    return vals


def test_device_class_table_is_the_oracles_classifier(all_classes):
    text = open(UNI_HEADER, encoding="utf-8").read()
    version = re.search(r"Unicode (\d+\.\d+\.\d+)", text.split("\n", 1)[0]).group(1)
    if version != unicodedata.unidata_version:
        pytest.skip(f"unicode_classes.h is Unicode {version}, this Python's unicodedata is {unicodedata.unidata_version}")
    shift = int(re.search(r"kUniBlockShift = (\d+)", text).group(1))
    blocks = int(re.search(r"kUniBlocks = (\d+)", text).group(1))
    idx, cls = _parse_table(text, "kUniIndex"), _parse_table(text, "kUniClass")
    assert shift == 8 and idx.shape[0] == 0x110000 >> shift and cls.shape[0] == blocks << shift
    assert idx.min() >= 0 and idx.max() == blocks - 1
    cp = np.arange(0x110000)
    got = cls[(idx[cp >> shift] << shift) | (cp & 0xFF)]      # pt_class in pretok.hip
    bad = np.flatnonzero(got != all_classes)
    assert bad.size == 0, [(hex(int(c)), int(got[c]), int(all_classes[c])) for c in bad[:8]]
