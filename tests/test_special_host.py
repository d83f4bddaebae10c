"""Special tokens of the merge-rank encode, the parts that need no GPU: the nine entry
points are declared, exported and bound, the host check of a table, the reference
helper's identities, and the inputs on which "each piece alone" differs from "whole
buffer, the specials' edges forced" (so that the GPU tests cannot pass with the
shortcut).
"""
import os
import re

import numpy as np
import pytest

import bpe_oracle as O
from bpe_words_ref import XY_MERGES, encode_words_ref
from conftest import ROOT
from special_ref import (GPT4, HEUR, IDS, MASK, NONE, TABLE, chain_model, encode_special_ref, find_specials,
                         forced_mask_ref, mark_ref, piece_mask_ref, pieces, recipe)

NEW = {"gbpe_specials_upload": 6, "gbpe_specials_free": 1, "gbpe_specials_mark": 7, "gbpe_specials_mark_device": 7,
       "gbpe_bpe_encode_special": 10, "gbpe_bpe_encode_special_device": 10, "gbpe_bpe_encode_special_batch": 13,
       "gbpe_bpe_encode_special_batch_device": 13}


@pytest.fixture(scope="module")
def lib():
    from gpubpe import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_symbols_declared_exported_bound(lib):
    from gpubpe import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gpubpe.h")).read(), flags=re.S)
    for name, argc in NEW.items():
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
        assert len(getattr(lib, name).argtypes) == argc, name
    assert re.search(r"#define GBPE_SPECIALS_MAX\s+254u", src) and re.search(r"#define GBPE_SPECIAL_MAX_BYTES\s+128u", src)
    assert (_lib.GBPE_SPECIALS_MAX, _lib.GBPE_SPECIAL_MAX_BYTES) == (254, 128)
    # the timing call reports the special calls too: it is the ninth symbol of the feature's surface
    assert len(lib.gbpe_bpe_encode_last_timing.argtypes) == 4


def test_abi_version_is_still_10(lib):
    src = open(os.path.join(ROOT, "include", "gpubpe.h")).read()
    assert re.search(r"#define GBPE_ABI_VERSION 10\b", src)
    assert lib.gbpe_abi_version() == 10


def test_kernels_listed(lib):
    names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
    for k in ("k_sp_cand", "k_sp_accept", "k_me_sp_mask", "k_me_walk_special"):
        assert k in names, k


def test_python_layer_has_the_calls():
    import inspect
    from gpubpe import MergeEncoder
    assert "special_tokens" in inspect.signature(MergeEncoder.__init__).parameters
    for fn in (MergeEncoder.encode_bytes, MergeEncoder.encode_batch, MergeEncoder.encode):
        assert inspect.signature(fn).parameters["special"].default is None
    assert callable(MergeEncoder.find_special)


def test_checked_special_tokens():
    from gpubpe import _lib
    from gpubpe.merge_encoder import checked_special_tokens
    assert checked_special_tokens({"<|e|>": 7, b"\xff\x00": 0xFFFFFFFF}) == [(b"<|e|>", 7), (b"\xff\x00", 0xFFFFFFFF)]
    assert len(checked_special_tokens({bytes([1, k]): k for k in range(254)})) == 254
    assert checked_special_tokens({b"a" * 128: 1}) == [(b"a" * 128, 1)]
    bad = [{}, {bytes([1, k]): k for k in range(255)}, {b"": 1}, {b"a" * 129: 1}, {"a": 1, b"a": 2}, {3: 1},
           {b"a": -1}, {b"a": 1 << 32}, {b"a": 1.5}, [b"a"], "a"]
    for table in bad:
        with pytest.raises(_lib.GpuBpeError) as e:
            checked_special_tokens(table)
        assert e.value.code == _lib.GBPE_E_INVALID, table


def test_scan_identities():
    assert find_specials(b"aaaaa", [b"aa"]) == [(0, 0), (2, 0)]
    assert find_specials(b"<|<|a|>|>", [b"<|a|>"]) == [(2, 0)]
    assert find_specials(b"abcbcd", [b"abc", b"bcd", b"cb"]) == [(0, 0), (3, 1)]
    assert find_specials(b"<s><s>>x<s", [b"<s>", b"<s>>"]) == [(0, 0), (3, 1)]
    assert mark_ref(b"xaaaaa", [b"b", b"aa"]).tolist() == [0, 2, 255, 2, 255, 0]
    # a special lies inside one document
    assert mark_ref([b"xa", b"ay"], [b"aa"]).tolist() == [0, 0, 0, 0]
    assert mark_ref([b"x<s>", b">"], [b"<s>", b"<s>>"]).tolist() == [0, 1, 255, 255, 0]
    assert pieces(b"abEOTcd", [b"EOT"]) == [(0, 2, None), (2, 5, 0), (5, 7, None)]


@pytest.mark.parametrize("seed", range(6))
def test_anchor_chains_are_the_scan(seed):
    """The device's decomposition (special.hip): chains from uncovered candidates are disjoint and
    together are the sequential scan — on overlapping tables over a two-letter alphabet."""
    rng = np.random.default_rng(seed)
    tables = [[b"aa"], [b"ab", b"ba", b"aba"], [b"a", b"aab", b"ba"], [b"abab", b"ba", b"bb"], [b"a" * 128, b"ab"],
              [b"b" + b"a" * 127, b"aab", b"aaaa"]]
    table = tables[seed]
    for n in (1, 2, 7, 300, 700):
        data = bytes(rng.choice(np.frombuffer(b"aaab", np.uint8), n).tolist())
        got, writes = chain_model(data, table)
        assert got == find_specials(data, table)
        assert max(writes) <= 1
    got, writes = chain_model(b"a" * 600, table)
    assert got == find_specials(b"a" * 600, table) and max(writes) <= 1


def test_piece_alone_is_not_edges_forced():
    # a contraction after a letter / a digit run: the whole-buffer rules look across the special
    assert piece_mask_ref(b"itEOT's", [b"EOT"], GPT4).tolist() == [1, 0, 0, 0, 0, 1, 1]
    assert forced_mask_ref(b"itEOT's", [b"EOT"], GPT4).tolist() == [1, 0, 0, 0, 0, 1, 0]
    assert piece_mask_ref(b"1200734", [b"007"], GPT4).tolist() == [1, 0, 0, 0, 0, 1, 0]
    assert forced_mask_ref(b"1200734", [b"007"], GPT4).tolist() == [1, 0, 0, 0, 0, 1, 1]


def test_xy_cases():
    assert encode_special_ref([b"x y<|e|>x y"], XY_MERGES, [b"<|e|>"], [999], NONE) == ([257, 999, 257], [0, 3])
    assert encode_special_ref([b"x <|e|>y"], XY_MERGES, [b"<|e|>"], [999], NONE) == ([256, 999, 121], [0, 3])
    assert O.encode_merge_order(b"x y", XY_MERGES) == [257]


def test_corpus_recipe():
    data, merges = recipe()
    assert len(data) == 13554
    hits = find_specials(data, TABLE)
    assert len(hits) == 317 and [sum(1 for _, k in hits if k == j) for j in range(4)] == [74, 74, 74, 95]
    want, tok_off = encode_special_ref([data], merges, TABLE, IDS, GPT4)
    assert len(want) == 8497 and tok_off == [0, 8497]
    assert sum(1 for t in want if t >= 50000) == 317
    per, forced = piece_mask_ref(data, TABLE, GPT4), forced_mask_ref(data, TABLE, GPT4)
    assert int((per != forced).sum()) == 3
    outside = mark_ref(data, TABLE) == 0
    assert int((per != forced)[outside].sum()) == 3
    # the shortcut's token stream: the buffer's words under the forced mask, specials replaced by their ids
    short = []
    for a, b, k in pieces(data, TABLE):
        short += [IDS[k]] if k is not None else encode_words_ref(data[a:b], merges, forced[a:b])
    assert short != want
    # without specials in the text the reference is the plain one
    plain = b"int main() { return 0; }"
    assert encode_special_ref([plain], merges, [b"<|endoftext|>"], [50000], GPT4)[0] == \
        encode_words_ref(plain, merges, O.gpt4_word_starts(plain))
    # mode MASK: the entries under a special's bytes are ignored, a piece's first byte is forced
    ws = (np.random.default_rng(3).random(len(data)) < 0.1).astype(np.uint8)
    flipped = ws.copy()
    flipped[~outside] ^= 1
    for a, b, k in pieces(data, TABLE):
        flipped[a] = 0
    assert int((flipped != ws).sum()) > 317
    assert encode_special_ref([data], merges, TABLE, IDS, MASK, flipped) == \
        encode_special_ref([data], merges, TABLE, IDS, MASK, ws)
    assert len({len(encode_special_ref([data], merges, TABLE, IDS, m, ws)[0]) for m in (NONE, MASK, HEUR)}) >= 2
