"""The merge-rank encoder on models with ids above 0xFFFF (gbpe_bpe_upload_wide):
merge_models.py's adversarial lists relabelled by merge_wide.f through every walk (whole
string, caller's mask at each chunk size, batch, special batch, the heap path of the closed
models), the collision lists, a table at the highest load the sizing rule allows, a model
with more entries than 16-bit ids allow, the upload's statuses and a decode round trip.
The expected tokens are f of what the narrow model's references give (those of
test_gpu_merge_models.py, computed once for both modules); test_merge_wide.py shows on the
CPU that these cases tell a 32-bit packed key from a right one."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import merge_models as M
import merge_wide as W
import test_gpu_merge_models as G
from bpe_words_batch_ref import MASK, NONE
from encode_dev import DevBuffers
from gpubpe import BPEEngine, MergeEncoder, _lib

pytestmark = pytest.mark.gpu

CHUNK_SIZES = [4096, 1024, 256]


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


@pytest.fixture(scope="module")
def encoders(engine):
    """seed → the relabelled model's encoder, with the special table (its id relabelled too)."""
    made = {}

    def get(seed):
        if seed not in made:
            made[seed] = MergeEncoder(engine, W.relabel(M.model_case(seed)["merges"]),
                                      special_tokens={M.SPECIAL: W.f(M.SPECIAL_ID)})
        return made[seed]

    yield get
    for e in made.values():
        e.destroy()


def _what(seed, text=None):
    return f"seed {seed} merges {W.relabel(M.model_case(seed)['merges'])} text {text!r}"


# ── 5. the relabelled small models through every walk ──────────────────────

def test_relabelled_models_take_the_wide_upload(encoders):
    wide = [s for s in M.SEEDS if encoders(s).wide]
    assert len(wide) >= 100
    assert all(encoders(s).wide == any(v > 0xFFFF for m in W.relabel(M.model_case(s)["merges"]) for v in m) for s in M.SEEDS)
    closed = [s for s in wide if M.model_case(s)["closed"]]
    assert len(closed) >= 30 and [len(t) for t in M.model_case(closed[0])["texts"][-4:]] == M.LONG_LENGTHS


@pytest.mark.parametrize("group", list(M.GROUPS))
def test_whole_string(engine, encoders, group):
    for seed in M.GROUPS[group]:
        c = M.model_case(seed)
        for t in c["texts"]:   # (a closed model's LONG_LENGTHS texts are one segment: me_heap)
            got = encoders(seed).encode_bytes(t, special=False).tolist()
            assert got == W.relabel_tokens(M.reference(t, c["merges"])), _what(seed, t)


@pytest.mark.parametrize("cs", CHUNK_SIZES)
@pytest.mark.parametrize("group", list(M.GROUPS))
def test_callers_mask(engine, encoders, monkeypatch, group, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for seed in M.GROUPS[group]:
        for t, ws, want in G._masked_refs(seed):
            got = encoders(seed).encode_bytes(t, word_starts=ws, special=False).tolist()
            assert got == W.relabel_tokens(want), _what(seed, t) + f" starts {np.flatnonzero(ws).tolist()}"


@pytest.mark.parametrize("cs", CHUNK_SIZES)
@pytest.mark.parametrize("mode", [NONE, MASK])
@pytest.mark.parametrize("group", list(M.GROUPS))
def test_batch(engine, encoders, monkeypatch, group, mode, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for seed in M.GROUPS[group]:
        docs, mask, (want, want_off) = G._batch_ref(seed, mode)
        got, off = encoders(seed).encode_batch(docs, word_starts=mask, special=False)
        assert off.tolist() == want_off, _what(seed, docs)
        assert got.tolist() == W.relabel_tokens(want), _what(seed, docs)


@pytest.mark.parametrize("cs", CHUNK_SIZES)
@pytest.mark.parametrize("group", list(M.GROUPS))
def test_special_batch(engine, encoders, monkeypatch, group, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for seed in M.GROUPS[group]:
        docs, (want, want_off) = G._special_ref(seed)
        got, off = encoders(seed).encode_batch(docs)
        assert off.tolist() == want_off, _what(seed, docs)
        assert got.tolist() == W.relabel_tokens(want), _what(seed, docs)   # (the special's id is f(SPECIAL_ID))


# ── 6. the collision lists ─────────────────────────────────────────────────

def _device_encode(engine, dev, enc, text, ws):
    n = len(text)
    d_in = dev.alloc(n, np.frombuffer(text, np.uint8))
    d_ws = dev.alloc(n, ws) if ws is not None else None
    d_out = dev.alloc(4 * n)
    n_out = C.c_uint64()
    rc = dev.lib.gbpe_bpe_encode_words_device(engine.device, enc._h, d_in, n, d_ws, MASK if ws is not None else NONE, d_out, n,
                                              C.byref(n_out))
    assert rc == _lib.GBPE_OK
    return dev.fetch(d_out, n_out.value, np.uint32).tolist()


@pytest.mark.parametrize("name,merges,text,want", W.COLLISIONS, ids=[c[0] for c in W.COLLISIONS])
def test_collision_lists(engine, name, merges, text, want):
    enc = MergeEncoder(engine, merges)
    dev = DevBuffers(engine)
    try:
        assert enc.wide
        assert enc.encode_bytes(text).tolist() == want                                # gbpe_bpe_encode
        one_word = np.zeros(len(text), np.uint8)
        assert enc.encode_bytes(text, word_starts=one_word).tolist() == want          # gbpe_bpe_encode_words
        cut = one_word.copy()
        cut[1] = 1
        want_cut = M.np_merge_order_words(text, merges, cut).tolist()
        assert want_cut != want
        assert enc.encode_bytes(text, word_starts=cut).tolist() == want_cut
        assert _device_encode(engine, dev, enc, text, None) == want                   # gbpe_bpe_encode_words_device
        assert _device_encode(engine, dev, enc, text, one_word) == want
        assert _device_encode(engine, dev, enc, text, cut) == want_cut
    finally:
        dev.free()
        enc.destroy()


# ── 7. the large model relabelled: 131,072 slots at load 0.498 ─────────────

@pytest.fixture(scope="module")
def big(engine):
    merges, text = M.big_model()
    wide = W.f_array(merges)
    assert wide.shape == (65_280, 3) and int(wide.max()) > 0xFFFF
    enc = MergeEncoder(engine, wide.tolist())
    assert enc.wide
    yield enc, text
    enc.destroy()


def test_big_model_heap_path(big):
    enc, text = big
    whole, _, _ = M.big_reference()
    assert np.array_equal(enc.encode_bytes(text).astype(np.int64), W.f_array(whole))


def test_big_model_short_words(big):
    enc, text = big
    _, words, ws = M.big_reference()
    assert np.array_equal(enc.encode_bytes(text, word_starts=ws).astype(np.int64), W.f_array(words))


def test_big_model_device_form(engine, big):
    enc, text = big
    whole, words, ws = M.big_reference()
    dev = DevBuffers(engine)
    try:
        assert _device_encode(engine, dev, enc, text, None) == W.f_array(whole).tolist()
        assert _device_encode(engine, dev, enc, text, ws) == W.f_array(words).tolist()
    finally:
        dev.free()


# ── 8, 10. more entries than the narrow form can hold; decode round trip ───

@pytest.fixture(scope="module")
def many(engine):
    merges, text, tokens = W.many_pairs_model()
    assert merges.shape[0] == 69_536 > 0x10000 - 256 and int(merges[:, 2].max()) == 256 + 69_536 - 1 > 0xFFFF
    enc = MergeEncoder(engine, merges.tolist())
    assert enc.wide
    yield enc, merges, text, tokens
    enc.destroy()


def test_many_pairs_model(many):
    enc, merges, text, tokens = many
    assert len(text) == W.MANY_TEXT_LEN and M.segments(text[:300], merges[:W.MANY_LEVEL1].tolist()) == [300]
    level2 = int((tokens >= 256 + W.MANY_LEVEL1).sum())
    assert level2 >= 500 and int((tokens > 0xFFFF).sum()) >= level2   # second-level merges fire, wide ids come out
    assert np.array_equal(enc.encode_bytes(text).astype(np.int64), tokens)


def test_many_pairs_round_trip(engine, many):
    enc, merges, text, tokens = many
    lib = _lib.load()
    raw, offs = W.dense_vocab(merges)
    vocab = C.c_void_p()
    _lib.check(lib.gbpe_vocab_upload(engine.device, raw.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(_lib.u64p),
                                     offs.shape[0] - 1, C.byref(vocab)), engine.device, "vocab upload")
    try:
        got = np.ascontiguousarray(enc.encode_bytes(text), np.uint32)
        out = np.zeros(len(text) + 16, np.uint8)
        n = C.c_uint64()
        _lib.check(lib.gbpe_decode(engine.device, vocab, got.ctypes.data_as(_lib.u32p), got.shape[0],
                                   out.ctypes.data_as(C.c_void_p), out.shape[0], C.byref(n)), engine.device, "decode")
        assert bytes(out[: n.value]) == text
    finally:
        lib.gbpe_vocab_free(vocab)


# ── 9. upload statuses ─────────────────────────────────────────────────────

A, B = G.A, G.B
OVER = W.MAX_ID + 1
BAD_WIDE_UPLOADS = [
    ("a_over", [[A, B, 256], [OVER, B, 257]], 1),
    ("b_over", [[A, B, 256], [B, B, 257], [A, OVER, 258]], 2),
    ("id_over", [[A, B, OVER]], 0),
    ("id_0xFFFFFFFF", [[A, B, 256], [A, A, 0xFFFFFFFF]], 1),
] + G.BAD_UPLOADS[-5:]


def _upload_wide(engine, merges):
    lib = _lib.load()
    arr = np.ascontiguousarray(np.asarray(merges, np.uint32).reshape(-1, 3))
    h = C.c_void_p(0xDEAD0)
    rc = lib.gbpe_bpe_upload_wide(engine.device, arr.ctypes.data_as(_lib.u32p) if arr.size else None, arr.shape[0], C.byref(h))
    return rc, h


@pytest.mark.parametrize("name,merges,index", BAD_WIDE_UPLOADS, ids=[b[0] for b in BAD_WIDE_UPLOADS])
def test_wide_upload_rejects(engine, name, merges, index):
    rc, h = _upload_wide(engine, merges)
    assert rc == _lib.GBPE_E_INVALID
    assert h.value is None   # *out == NULL
    msg = _lib.load().gbpe_last_error(engine.device).decode()
    assert f"merge {index} " in msg, msg


def test_wide_upload_takes_what_the_narrow_one_rejects(engine):
    assert [b[0] for b in BAD_WIDE_UPLOADS[-5:]] == ["new_id_255", "new_id_0", "repeated_after_live", "repeated_after_dead",
                                                     "repeated_after_missing_operand"]
    lib = _lib.load()
    for name, merges, _ in G.BAD_UPLOADS[:3]:   # an id of 0x10000: the wide call's to take
        rc, h = _upload_wide(engine, merges)
        assert rc == _lib.GBPE_OK and h.value not in (None, 0xDEAD0), name
        lib.gbpe_bpe_free(h)
    rc, h = _upload_wide(engine, [[A, B, W.MAX_ID], [W.MAX_ID, W.MAX_ID, 256]])   # the bound itself
    assert rc == _lib.GBPE_OK
    out = np.zeros(8, np.uint32)
    n = C.c_uint64()
    assert lib.gbpe_bpe_encode(engine.device, h, b"ababab", 6, out.ctypes.data_as(_lib.u32p), 8, C.byref(n)) == _lib.GBPE_OK
    assert out[: n.value].tolist() == [256, W.MAX_ID]
    lib.gbpe_bpe_free(h)


def test_wide_upload_of_no_merges(engine):
    lib = _lib.load()
    rc, h = _upload_wide(engine, [])
    assert rc == _lib.GBPE_OK and h.value not in (None, 0xDEAD0)
    out = np.zeros(8, np.uint32)
    n = C.c_uint64()
    assert lib.gbpe_bpe_encode(engine.device, h, b"ab\0\0", 4, out.ctypes.data_as(_lib.u32p), 8, C.byref(n)) == _lib.GBPE_OK
    assert out[: n.value].tolist() == [A, B, 0, 0]
    lib.gbpe_bpe_free(h)


def test_merge_encoder_picks_the_upload(engine, monkeypatch):
    lib = _lib.load()
    calls = []
    real = {name: getattr(lib, name) for name in ("gbpe_bpe_upload", "gbpe_bpe_upload_wide")}
    for name, fn in real.items():
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=fn: (calls.append(_n), _f(*a))[1])
    _, merges, text, want = W.COLLISIONS[0]
    enc = MergeEncoder(engine, merges)
    assert calls == ["gbpe_bpe_upload_wide"] and enc.wide and enc.encode_bytes(text).tolist() == want
    enc.destroy()
    merges, text, want = M.NUL_NUL
    enc = MergeEncoder(engine, merges)   # a narrow list: the upload it always took
    assert calls[1:] == ["gbpe_bpe_upload"] and not enc.wide and enc.encode_bytes(text).tolist() == want
    enc.destroy()
    enc = MergeEncoder(engine, [[A, B, 0xFFFF], [0xFFFF, A, 256]])   # 0xFFFF is still narrow
    assert calls[2:] == ["gbpe_bpe_upload"] and enc.encode_bytes(b"aba").tolist() == [256]
    enc.destroy()
    for merges, index in (([[A, B, 256], [A, A, OVER]], 1), ([[A, B, 2 ** 32]], 0), ([[A, -1, 256]], 0)):
        with pytest.raises(_lib.GpuBpeError) as err:
            MergeEncoder(engine, merges)
        assert err.value.code == _lib.GBPE_E_INVALID and f"merge {index} " in str(err.value)
