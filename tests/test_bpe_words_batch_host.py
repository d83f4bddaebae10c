"""Batch word starts and batch word-bounded merge-rank encode, the parts that need no
GPU: the four entry points are declared, exported and bound, the reference helper's
identities, and the inputs on which the per-document rules differ from "whole buffer,
document starts forced" (so that the GPU tests cannot pass on inputs where the two
agree).
"""
import os
import re

import numpy as np
import pytest

import bpe_oracle as O
from bpe_words_batch_ref import (GPT4, HAND_PAIRS, HEUR, MASK, NONE, bits, doc_offsets, encode_words_batch_ref,
                                 gpt4_batch_ref, gpt4_forced_ref, random_cuts, split)
from bpe_words_ref import XY_MERGES, encode_words_ref, model, text
from conftest import ROOT

NEW = ("gbpe_pretokenize_gpt4_batch", "gbpe_pretokenize_gpt4_batch_device", "gbpe_bpe_encode_words_batch",
       "gbpe_bpe_encode_words_batch_device")


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
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.gbpe_pretokenize_gpt4_batch.argtypes) == 6
    assert len(lib.gbpe_bpe_encode_words_batch.argtypes) == 12
    assert len(lib.gbpe_bpe_encode_words_batch_device.argtypes) == 12


def test_abi_version_is_10(lib):
    src = open(os.path.join(ROOT, "include", "gpubpe.h")).read()
    assert re.search(r"#define GBPE_ABI_VERSION 10\b", src)
    assert lib.gbpe_abi_version() == 10 and b"abi 10" in lib.gbpe_version()


def test_python_layers_have_the_batch_calls():
    from gpubpe import GpuPreTokenizer, MergeEncoder
    assert callable(MergeEncoder.encode_batch) and callable(GpuPreTokenizer.pre_tokenize_batch)


def test_reference_identities():
    merges, data = model("code", 53), text("code", 53)
    arr = np.frombuffer(data, np.uint8)
    ws = (np.random.default_rng(3).random(len(data)) < 0.1).astype(np.uint8)
    singles = {NONE: O.encode_merge_order(data, merges),
               MASK: encode_words_ref(data, merges, ws),
               HEUR: encode_words_ref(data, merges, O.heuristic_word_starts(arr)),
               GPT4: encode_words_ref(data, merges, O.gpt4_word_starts(data))}
    for mode, want in singles.items():
        mask = ws if mode == MASK else None
        assert encode_words_batch_ref([data], merges, mode, mask) == (want, [0, len(want)]), mode
        # empty documents contribute nothing
        got, off = encode_words_batch_ref([b"", b"", data, b"", b""], merges, mode, mask)
        assert got == want and off == [0, 0, 0, len(want), len(want), len(want)], mode
    assert encode_words_batch_ref([], merges, GPT4) == ([], [0])
    assert gpt4_batch_ref([data]).tolist() == np.asarray(O.gpt4_word_starts(data)).tolist()
    assert gpt4_batch_ref([b"", data, b""]).tolist() == gpt4_batch_ref([data]).tolist()
    assert doc_offsets([b"ab", b"", b"c"]).tolist() == [0, 2, 2, 3]
    # mode NONE cuts at a document start and nowhere else
    assert encode_words_batch_ref([b"x", b" y"], XY_MERGES, NONE) == ([120, 32, 121], [0, 1, 3])
    assert O.encode_merge_order(b"x y", XY_MERGES) == [257]


@pytest.mark.parametrize("docs,forced,per", HAND_PAIRS, ids=[repr(b"|".join(p[0])) for p in HAND_PAIRS])
def test_hand_pairs_separate_the_rules(docs, forced, per):
    assert forced != per
    assert bits(gpt4_forced_ref(docs)) == forced
    assert bits(gpt4_batch_ref(docs)) == per


def test_heuristic_is_local():
    """The byte-class rule reads one byte back: per-document = whole buffer with the document starts set."""
    data = text("code", 53)
    offs = random_cuts(data, 300, seed=7)
    whole = np.asarray(O.heuristic_word_starts(np.frombuffer(data, np.uint8))).astype(np.uint8)
    whole[offs[:-1].astype(np.int64)] = 1
    per = np.concatenate([np.asarray(O.heuristic_word_starts(np.frombuffer(d, np.uint8))).astype(np.uint8)
                          for d in split(data, offs)])
    assert whole.tolist() == per.tolist()


def test_cuts_change_synth_code():
    merges, data = model("code", 53), text("code", 53)
    offs = random_cuts(data, 300, seed=7)
    docs = split(data, offs)
    assert len(docs) == 296 and all(docs)
    forced, per = gpt4_forced_ref(docs), gpt4_batch_ref(docs)
    assert int((forced != per).sum()) == 27
    want, tok_off = encode_words_batch_ref(docs, merges, GPT4)
    assert len(encode_words_ref(data, merges, forced)) == 8149 and len(want) == 8144
    assert want == encode_words_ref(data, merges, per) and tok_off[-1] == 8144
    voc = O.vocab_from_merges(merges).entries
    for d, doc in enumerate(docs):
        assert O.decode(want[tok_off[d]:tok_off[d + 1]], voc) == doc
