"""The merge-rank encoder on the adversarial merge lists of merge_models.py: every kernel
text that holds the walk (k_me_walk<false, 4096>, k_me_walk<true, cs>, k_me_walk_docs<cs>
and its special form, each with its heap branch) against the oracle, a table at the highest
load the sizing rule allows, and the statuses of gbpe_bpe_upload.  test_merge_models.py
shows on the CPU that these cases tell a right encoder from a wrong one."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import merge_models as M
from bpe_words_batch_ref import MASK, NONE, encode_words_batch_ref
from bpe_words_ref import encode_words_ref
from encode_dev import DevBuffers
from gpubpe import BPEEngine, MergeEncoder, _lib
from special_ref import encode_special_ref

pytestmark = pytest.mark.gpu

CHUNK_SIZES = [4096, 1024, 256]


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


@pytest.fixture(scope="module")
def encoders(engine):
    """seed → the model's encoder (with the special table: special=False gives the plain calls),
    uploaded once for all the tests of the module."""
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = MergeEncoder(engine, M.model_case(seed)["merges"], special_tokens={M.SPECIAL: M.SPECIAL_ID})
        return made[seed]

    yield get
    for e in made.values():
        e.destroy()


def _what(seed, text=None):
    c = M.model_case(seed)
    return f"seed {seed} merges {c['merges']} text {text!r}"


# the references, computed once and shared by the chunk sizes

@functools.lru_cache(maxsize=None)
def _masked_refs(seed):
    """[(text, mask, tokens)]: a 0.1 mask on mask_text, and starts [0, 1025] on a closed model's 2,051 bytes."""
    c = M.model_case(seed)
    t = c["mask_text"]
    ws = M.random_mask(len(t), 3000 + seed)
    out = [(t, ws, encode_words_ref(t, c["merges"], ws))]
    if c["closed"]:
        t = c["texts"][-1]
        ws = np.zeros(len(t), np.uint8)
        ws[[0, 1025]] = 1
        out.append((t, ws, M.np_merge_order_words(t, c["merges"], ws).tolist()))
    return out


@functools.lru_cache(maxsize=None)
def _batch_ref(seed, mode):
    c = M.model_case(seed)
    docs, mask = M.batch_docs(c)
    mask = mask if mode == MASK else None
    return docs, mask, encode_words_batch_ref(docs, c["merges"], mode, mask)


@functools.lru_cache(maxsize=None)
def _special_ref(seed):
    c = M.model_case(seed)
    docs = M.special_docs(c, seed)
    return docs, encode_special_ref(docs, c["merges"], [M.SPECIAL], [M.SPECIAL_ID], NONE)


# ── the small models through every walk ────────────────────────────────────

@pytest.mark.parametrize("group", list(M.GROUPS))
def test_whole_string(engine, encoders, group):
    for seed in M.GROUPS[group]:
        c = M.model_case(seed)
        for t in c["texts"]:
            got = encoders(seed).encode_bytes(t, special=False).tolist()
            assert got == M.reference(t, c["merges"]), _what(seed, t)


@pytest.mark.parametrize("cs", CHUNK_SIZES)
@pytest.mark.parametrize("group", list(M.GROUPS))
def test_callers_mask(engine, encoders, monkeypatch, group, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for seed in M.GROUPS[group]:
        for t, ws, want in _masked_refs(seed):
            got = encoders(seed).encode_bytes(t, word_starts=ws, special=False).tolist()
            assert got == want, _what(seed, t) + f" starts {np.flatnonzero(ws).tolist()}"


@pytest.mark.parametrize("cs", CHUNK_SIZES)
@pytest.mark.parametrize("mode", [NONE, MASK])
@pytest.mark.parametrize("group", list(M.GROUPS))
def test_batch(engine, encoders, monkeypatch, group, mode, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for seed in M.GROUPS[group]:
        docs, mask, (want, want_off) = _batch_ref(seed, mode)
        got, off = encoders(seed).encode_batch(docs, word_starts=mask, special=False)
        assert off.tolist() == want_off, _what(seed, docs)
        assert got.tolist() == want, _what(seed, docs)


@pytest.mark.parametrize("cs", CHUNK_SIZES)
@pytest.mark.parametrize("group", list(M.GROUPS))
def test_special_batch(engine, encoders, monkeypatch, group, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for seed in M.GROUPS[group]:
        docs, (want, want_off) = _special_ref(seed)
        got, off = encoders(seed).encode_batch(docs)
        assert off.tolist() == want_off, _what(seed, docs)
        assert got.tolist() == want, _what(seed, docs)


def test_issue_table(engine):
    merges, text, want = M.NUL_NUL
    enc = MergeEncoder(engine, merges)
    assert enc.encode_bytes(text).tolist() == want
    enc.destroy()
    for merges, _, _ in M.REJECTED + [M.FEEDS_BACK]:
        with pytest.raises(_lib.GpuBpeError) as err:
            MergeEncoder(engine, merges)
        assert err.value.code == _lib.GBPE_E_INVALID


# ── the large model: 131,072 slots at load 0.498 ───────────────────────────

@pytest.fixture(scope="module")
def big(engine):
    merges, text = M.big_model()
    enc = MergeEncoder(engine, merges.tolist())
    yield enc, text
    enc.destroy()


def test_big_model_heap_path(big):
    enc, text = big
    whole, _, _ = M.big_reference()
    assert np.array_equal(enc.encode_bytes(text).astype(np.int64), whole)


def test_big_model_short_words(big):
    enc, text = big
    _, words, ws = M.big_reference()
    assert np.array_equal(enc.encode_bytes(text, word_starts=ws).astype(np.int64), words)


def test_big_model_device_form(engine, big):
    enc, text = big
    whole, words, ws = M.big_reference()
    dev = DevBuffers(engine)
    try:
        n = len(text)
        d_in = dev.alloc(n, np.frombuffer(text, np.uint8))
        d_ws = dev.alloc(n, ws)
        d_out = dev.alloc(4 * n)
        for mask, mode, want in ((None, NONE, whole), (d_ws, MASK, words)):
            n_out = C.c_uint64()
            rc = dev.lib.gbpe_bpe_encode_words_device(engine.device, enc._h, d_in, n, mask, mode, d_out, n, C.byref(n_out))
            assert rc == _lib.GBPE_OK and n_out.value == want.size
            assert np.array_equal(dev.fetch(d_out, want.size, np.uint32).astype(np.int64), want)
    finally:
        dev.free()


# ── upload statuses ────────────────────────────────────────────────────────

A, B = ord("a"), ord("b")
BAD_UPLOADS = [
    ("id_0x10000", [[A, B, 256], [A, A, 0x10000]], 1),
    ("a_0x10000", [[0x10000, B, 256]], 0),
    ("b_0x10000", [[A, B, 256], [B, B, 257], [A, 0x10000, 258]], 2),
    ("new_id_255", [[A, B, 256], [256, A, 255]], 1),
    ("new_id_0", [[A, B, 0]], 0),
    ("repeated_after_live", [[A, B, 256], [B, A, 257], [A, A, 256]], 2),
    ("repeated_after_dead", [[A, B, 256], [A, B, 300], [B, B, 257], [B, A, 300]], 3),        # 300: a repeated pair's
    ("repeated_after_missing_operand", [[9000, A, 300], [A, B, 256], [B, B, 300]], 2),      # 300: never created
]


@pytest.mark.parametrize("name,merges,index", BAD_UPLOADS, ids=[b[0] for b in BAD_UPLOADS])
def test_upload_rejects(engine, name, merges, index):
    lib = _lib.load()
    arr = np.ascontiguousarray(np.asarray(merges, np.uint32).reshape(-1, 3))
    h = C.c_void_p(0xDEAD0)
    rc = lib.gbpe_bpe_upload(engine.device, arr.ctypes.data_as(_lib.u32p), arr.shape[0], C.byref(h))
    assert rc == _lib.GBPE_E_INVALID
    assert h.value is None   # *out == NULL
    msg = lib.gbpe_last_error(engine.device).decode()
    assert f"merge {index} " in msg, msg


def test_upload_of_no_merges(engine):
    lib = _lib.load()
    h = C.c_void_p(0xDEAD0)
    assert lib.gbpe_bpe_upload(engine.device, None, 0, C.byref(h)) == _lib.GBPE_OK
    assert h.value not in (None, 0xDEAD0)
    out = np.zeros(8, np.uint32)
    n = C.c_uint64()
    assert lib.gbpe_bpe_encode(engine.device, h, b"ab\0\0", 4, out.ctypes.data_as(_lib.u32p), 8, C.byref(n)) == _lib.GBPE_OK
    assert out[: n.value].tolist() == [A, B, 0, 0]
    lib.gbpe_bpe_free(h)
