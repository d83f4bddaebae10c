"""Byte spans of the merge-rank encode's tokens, the parts that need no GPU: the
position-carrying oracle (bpe_spans_ref.py) against the references the encoder's other
tests use, the properties of its starts, the two entry points declared, exported and
bound, and the Python layer's argument checks.
"""
import inspect
import os
import re

import numpy as np
import pytest

import bpe_oracle as O
import merge_models as M
import merge_wide as MW
from bpe_spans_ref import CL100K, GPT4, HEUR, MASK, NONE, doc_tok_off, merge_order_spans, spans_ref
from bpe_words_batch_ref import doc_offsets, encode_words_batch_ref, random_cuts, split
from bpe_words_ref import XY_MERGES, XY_TEXT, XY_WHOLE, XY_WORDS, encode_words_ref, model, text
from conftest import ROOT
from special_ref import IDS, TABLE, encode_special_ref, recipe

NEW = {"gbpe_bpe_encode_spans": 14, "gbpe_bpe_encode_spans_device": 14}
A = ord("a")
A_MERGES = [[A, A, 256], [256, A, 257], [256, 256, 258]]


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
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
        assert len(getattr(lib, name).argtypes) == argc, name
    names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
    assert "k_me_walk_spans" in names and "k_me_compact_spans" in names and len(names) == len(set(names))


def test_abi_version_is_still_10(lib):
    src = open(os.path.join(ROOT, "include", "gpubpe.h")).read()
    assert re.search(r"#define GBPE_ABI_VERSION 10\b", src)
    assert lib.gbpe_abi_version() == 10


def test_python_argument_checks_need_no_device():
    from gpubpe import MergeEncoder, _lib
    for fn in (MergeEncoder.encode_bytes_spans, MergeEncoder.encode_batch_spans):
        params = inspect.signature(fn).parameters
        assert [params[k].default for k in ("word_starts", "words", "special")] == [None, None, None]
    enc = MergeEncoder.__new__(MergeEncoder)   # no engine, no library: the checks come first
    enc._sp = enc._h = None
    bad = [dict(word_starts=[1, 0], words="gpt4"), dict(words="gpt2"), dict(word_starts=[1, 0, 0]),
           dict(word_starts=[[1, 0]]), dict(word_starts=[0.5, 1.0]), dict(special=True)]
    for kw in bad:
        for call in (lambda: enc.encode_bytes_spans(b"ab", **kw), lambda: enc.encode_batch_spans([b"a", b"b"], **kw)):
            with pytest.raises(_lib.GpuBpeError) as e:
                call()
            assert e.value.code == _lib.GBPE_E_INVALID, kw


def test_cascade_by_hand():
    # aa→256, 256 a→257, 256 256→258: a position survives several passes
    want = {1: ([A], [0]), 2: ([256], [0]), 3: ([257], [0]), 4: ([258], [0]), 5: ([256, 257], [0, 2]),
            6: ([258, 256], [0, 4]), 7: ([258, 257], [0, 4]), 8: ([258, 258], [0, 4]),
            9: ([258, 256, 257], [0, 4, 6])}
    for k, (tok, pos) in want.items():
        assert merge_order_spans(b"a" * k, A_MERGES) == (tok, pos), k
        assert O.encode_merge_order(b"a" * k, A_MERGES) == tok, k
    assert spans_ref([XY_TEXT], XY_MERGES) == (XY_WHOLE, [0, 3, 6, 7])
    assert spans_ref([XY_TEXT], XY_MERGES, mode=MASK, mask=np.ones(len(XY_TEXT), np.uint8)) == (XY_WORDS, list(range(8)))


def check_starts(docs, tokens, starts):
    """Strictly increasing, from each non-empty document's offset, tiling [0, n)."""
    offs = doc_offsets(docs).tolist()
    n = offs[-1]
    assert len(tokens) == len(starts)
    s = np.asarray(starts + [n], np.int64)
    assert (np.diff(s) > 0).all()
    assert n == 0 or s[0] == 0
    tok_off = doc_tok_off(docs, starts)
    for d, doc in enumerate(docs):
        if doc:
            assert s[tok_off[d]] == offs[d], d   # no token crosses a document start
    return tok_off


def test_tokens_are_the_references():
    data, merges = recipe()
    docs = split(data, random_cuts(data, 300, seed=11))
    ws = (np.random.default_rng(3).random(len(data)) < 0.1).astype(np.uint8)
    for mode in (NONE, MASK, HEUR, GPT4):
        m = ws if mode == MASK else None
        for dd in ([data], docs):
            tokens, starts = spans_ref(dd, merges, TABLE, IDS, mode, m)
            want, tok_off = encode_special_ref(dd, merges, TABLE, IDS, mode, m)
            assert tokens == want, mode
            assert check_starts(dd, tokens, starts) == tok_off, mode
        tokens, starts = spans_ref(docs, merges, mode=mode, mask=m)
        want, tok_off = encode_words_batch_ref(docs, merges, mode, m)
        assert tokens == want and check_starts(docs, tokens, starts) == tok_off, mode
    code = text("code", 53)[:4000]
    tokens, starts = spans_ref([code], model("code", 53), mode=GPT4)
    assert tokens == encode_words_ref(code, model("code", 53), O.gpt4_word_starts(code))
    check_starts([code], tokens, starts)
    # the specials' tokens sit at the specials' bytes
    tokens, starts = spans_ref([data], merges, TABLE, IDS, GPT4)
    at = [s for t, s in zip(tokens, starts) if t >= 50000]
    assert len(at) == 317 and all(any(data.startswith(sp, s) for sp in TABLE) for s in at)


@pytest.mark.parametrize("seed", [0, 2, 3, 9, 12, 27])
def test_adversarial_models(seed):
    case = M.model_case(seed)
    for t in case["texts"]:
        tokens, starts = spans_ref([t], case["merges"])
        assert tokens == M.reference(t, case["merges"]), (seed, len(t))
        check_starts([t], tokens, starts)
    docs, mask = M.batch_docs(case)
    tokens, starts = spans_ref(docs, case["merges"], mode=MASK, mask=mask)
    want, tok_off = encode_words_batch_ref(docs, case["merges"], MASK, mask)
    assert tokens == want and check_starts(docs, tokens, starts) == tok_off


def test_lengths_are_the_vocabulary_s():
    """With no special, a token's span is its vocabulary entry's length."""
    for merges, data, mode in ((model("code", 53), text("code", 53)[:6000], GPT4), (model("english", 41), text("english", 41)[:3000], NONE),
                               (A_MERGES, b"a" * 9 + b" " + b"a" * 1025, NONE)):
        _, voff = MW.dense_vocab(np.asarray(merges, np.int64))
        lens = np.diff(voff.astype(np.int64))
        tokens, starts = spans_ref([data], merges, mode=mode)
        assert np.array_equal(np.diff(np.asarray(starts + [len(data)], np.int64)), lens[np.asarray(tokens)])


def test_a_special_s_span_is_not_its_id_s_length():
    """A length table read by id gives the special the model token's length: the oracle does not."""
    tokens, starts = spans_ref([b"aaaa<|e|>aa"], A_MERGES, [b"<|e|>"], [256])   # 256 is "aa" in the model
    assert tokens == [258, 256, 256] and starts == [0, 4, 9]
    _, voff = MW.dense_vocab(np.asarray(A_MERGES, np.int64))
    by_table = np.cumsum([0] + [int(voff[t + 1] - voff[t]) for t in tokens]).tolist()
    assert by_table[:-1] != starts


def test_cl100k_mode_is_its_own_mask():
    merges = [[ord("."), ord("b"), 256]]
    assert spans_ref([b"a.b"], merges, mode=CL100K) == ([97, 256], [0, 1])
    assert spans_ref([b"a.b"], merges, mode=GPT4)[0] != [97, 256]
