"""Word-bounded merge-rank encode on the GPU (gbpe_bpe_encode_words /
gbpe_bpe_encode_words_device) against the per-word oracle of bpe_words_ref.py:
identities, oracle parity in every mode, chunk and long-segment edges at every
chunk size the word kernels are built for (GBPE_DEBUG me_cs), statuses, and the
device form's alignment and bounds.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
from bpe_words_ref import XY_MERGES, XY_TEXT, XY_WHOLE, XY_WORDS, encode_words_ref, model, text
from encode_dev import DevBuffers
from gpubpe import BPEEngine, MergeEncoder, _lib

pytestmark = pytest.mark.gpu

A = ord("a")
A_MERGES = [[A, A, 256], [256, A, 257], [256, 256, 258]]
CHUNK_SIZES = [4096, 1024, 256]
NONE, MASK, HEUR, GPT4 = _lib.GBPE_WORDS_NONE, _lib.GBPE_WORDS_MASK, _lib.GBPE_WORDS_HEURISTIC, _lib.GBPE_WORDS_GPT4
CANARY = 0xA5A5A5A5
GUARD = 8


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc_a(engine):
    e = MergeEncoder(engine, A_MERGES)
    yield e
    e.destroy()


def _mask(n, starts):
    ws = np.zeros(n, np.uint8)
    ws[list(starts)] = 1
    return ws


def host_call(engine, enc, data, ws, mode, out_cap=None):
    """gbpe_bpe_encode_words into a guarded host array: (status, n_out, out[out_cap + GUARD])."""
    data = bytes(data)
    cap = len(data) if out_cap is None else out_cap
    out = np.full(cap + GUARD, CANARY, np.uint32)
    buf = C.create_string_buffer(data, len(data)) if data else None
    n = C.c_uint64(12345)
    wsp = None if ws is None else np.ascontiguousarray(ws, np.uint8).ctypes.data_as(C.c_void_p)
    rc = _lib.load().gbpe_bpe_encode_words(engine.device, enc._h, buf, len(data), wsp, mode,
                                           out.ctypes.data_as(_lib.u32p), cap, C.byref(n))
    return rc, int(n.value), out


def dev_call(engine, enc, data, ws, mode, out_cap=None, off=0, tail=b"", ws_tail=b""):
    """gbpe_bpe_encode_words_device with d_bytes / d_ws `off` bytes into their
    allocations, `tail` / `ws_tail` lying right behind the n bytes, and 0xA5
    words around the output: (status, n_out, out[out_cap + GUARD])."""
    data = bytes(data)
    n = len(data)
    cap = n if out_cap is None else out_cap
    dev = DevBuffers(engine)
    try:
        lead = b"a" * off   # (a byte in front of the input that would merge with byte 0, if read)
        d_in = dev.alloc(off + n + len(tail) + 1, np.frombuffer(lead + data + tail + b"\0", np.uint8))
        d_ws = None
        if ws is not None:
            host_ws = np.concatenate([np.zeros(off, np.uint8), np.asarray(ws, np.uint8),
                                      np.frombuffer(ws_tail + b"\0", np.uint8)])
            d_ws = C.c_void_p(dev.alloc(host_ws.shape[0], host_ws).value + off)
        d_out = dev.alloc(4 * (cap + GUARD), np.full(cap + GUARD, CANARY, np.uint32))
        n_out = C.c_uint64(12345)
        rc = dev.lib.gbpe_bpe_encode_words_device(engine.device, enc._h, C.c_void_p(d_in.value + off), n, d_ws, mode,
                                                  d_out, cap, C.byref(n_out))
        return rc, int(n_out.value), dev.fetch(d_out, cap + GUARD, np.uint32)
    finally:
        dev.free()


def check_both(engine, enc, data, ws, want, what):
    """The host and the device form give `want` and leave the words behind it alone."""
    for name, call in (("host", host_call), ("device", dev_call)):
        rc, n, out = call(engine, enc, data, ws, MASK)
        assert rc == _lib.GBPE_OK and n == len(want), (what, name, rc, n, len(want))
        assert out[:n].tolist() == want, (what, name)
        assert (out[n:] == CANARY).all(), (what, name)


# ── identities and hand cases ──────────────────────────────────────────────

def test_identities(engine):
    merges, data = model("code", 53), text("code", 53)
    enc = MergeEncoder(engine, merges)
    n = len(data)
    whole = enc.encode_bytes(data).tolist()
    assert whole == O.encode_merge_order(data, merges)
    assert enc.encode_bytes(data, word_starts=np.zeros(n, np.uint8)).tolist() == whole
    assert enc.encode_bytes(data, word_starts=np.ones(n, np.uint8)).tolist() == list(data)
    ones = np.ones(n, np.uint8)
    ones[0] = 0   # byte 0 starts a word whatever the mask says
    assert enc.encode_bytes(data, word_starts=ones).tolist() == list(data)
    ws = (np.random.default_rng(7).random(n) < 0.1).astype(np.uint8)
    ws[0] = 0
    assert enc.encode_bytes(data, word_starts=ws).tolist() == encode_words_ref(data, merges, ws)
    enc.destroy()


def test_hand_case(engine):
    enc = MergeEncoder(engine, XY_MERGES)
    assert enc.encode_bytes(XY_TEXT).tolist() == XY_WHOLE
    assert enc.encode_bytes(XY_TEXT, words="heuristic").tolist() == XY_WORDS
    assert enc.encode_bytes(XY_TEXT, words="gpt4").tolist() == XY_WORDS
    assert enc.encode(XY_TEXT.decode(), words="gpt4")["tokens"] == XY_WORDS
    # words "x ", "yx ", "y x": the first merge fires inside a word, the second never does
    assert enc.encode_bytes(XY_TEXT, word_starts=[1, 0, 1, 0, 0, 1, 0, 0]).tolist() == [256, 121, 256, 121, 32, 120]
    assert enc.encode_bytes(b"", words="gpt4").tolist() == []
    assert enc.encode_bytes(b"", word_starts=[]).tolist() == []
    with pytest.raises(_lib.GpuBpeError) as e:
        enc.encode_bytes(XY_TEXT, word_starts=[1, 0], words=None)
    assert e.value.code == _lib.GBPE_E_INVALID
    enc.destroy()


# ── oracle parity ──────────────────────────────────────────────────────────

def _lib_mask(engine, fn, data):
    ws = np.full(len(data), 0xEE, np.uint8)
    buf = C.create_string_buffer(data, len(data))
    _lib.check(getattr(_lib.load(), fn)(engine.device, buf, len(data), ws.ctypes.data_as(C.c_void_p)), engine.device, fn)
    return ws


@pytest.mark.parametrize("kind,seed", [("english", 51), ("multilingual", 52), ("code", 53)])
def test_oracle_parity(engine, kind, seed):
    merges, data = model(kind, seed), text(kind, seed)
    voc = O.vocab_from_merges(merges).entries
    enc = MergeEncoder(engine, merges)
    n = len(data)
    arr = np.frombuffer(data, np.uint8)
    rng = np.random.default_rng(seed)
    for density in (0.5, 0.1, 0.01):
        ws = (rng.random(n) < density).astype(np.uint8)
        got = enc.encode_bytes(data, word_starts=ws).tolist()
        assert got == encode_words_ref(data, merges, ws), (kind, density)
        assert O.decode(got, voc) == data
    for words, oracle_ws, fn in (("heuristic", O.heuristic_word_starts(arr), "gbpe_word_boundary"),
                                 ("gpt4", O.gpt4_word_starts(data), "gbpe_pretokenize_gpt4")):
        got = enc.encode_bytes(data, words=words).tolist()
        assert got == encode_words_ref(data, merges, oracle_ws), (kind, words)
        assert got == enc.encode_bytes(data, word_starts=_lib_mask(engine, fn, data)).tolist(), (kind, words)
        assert O.decode(got, voc) == data
    if kind == "code":   # (the input on which words change the tokens: test_bpe_words_host.py)
        assert len(enc.encode_bytes(data, words="gpt4")) == 8036 and len(enc.encode_bytes(data)) == 7973
    enc.destroy()


# ── chunk edges and the long path, at every chunk size of the word kernels ──

def _edge_cases():
    cases = []
    for n in (4095, 4096, 4097, 8193):
        spaced = (b"aaaaaaa " * (n // 8 + 1))[:n]   # short segments: no merge joins a space
        cases.append((f"spaced {n}, no word start", spaced, [0]))
        cases.append((f"run {n}, one word", b"a" * n, [0]))
        cases.append((f"run {n}, words of 12 with one over [4090, 4102)", b"a" * n, range(4090 % 12, n, 12)))
        cases.append((f"run {n}, words of 7", b"a" * n, range(0, n, 7)))
    n = 8193
    cases.append(("word start at 4096", b"a" * n, list(range(0, 4000, 5)) + [4096] + list(range(4200, n, 9))))
    cases.append(("word start at 4097", b"a" * n, list(range(0, 4000, 5)) + [4097] + list(range(4200, n, 9))))
    cases.append(("a word over [4090, 4102)", b"a" * n, list(range(0, 4090, 10)) + [4090, 4102] + list(range(4110, n, 10))))
    cases.append(("a chunk with no word start", b"a" * n, [0, 100]))
    cases.append(("spaced, a chunk with no word start", (b"aaaaaaa " * 1025)[:n], [0, 3, 100, 8190]))
    return cases


def _long_cases():
    return [
        ("two long segments", b"a" * 10_000, [0, 5000]),
        ("one long, one short", b"a" * 10_000, [0, 9500]),
        ("segments of 1024 and 1025", b"a" * 2049, [0, 1024]),
        ("segments of 1025 and 1024", b"a" * 2049, [0, 1025]),
        ("four segments of 1025 in one chunk", b"a" * 4100, [0, 1025, 2050, 3075]),
        ("four segments of 1025, then short words", b"a" * 5000, [0, 1025, 2050, 3075, 4100, 4103, 4500]),
    ]


@pytest.fixture(scope="module")
def edge_refs():
    return [(what, data, _mask(len(data), starts), encode_words_ref(data, A_MERGES, _mask(len(data), starts)))
            for what, data, starts in _edge_cases() + _long_cases()]


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_chunk_and_long_edges(engine, enc_a, edge_refs, monkeypatch, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for what, data, ws, want in edge_refs:
        check_both(engine, enc_a, data, ws, want, (cs, what))


def test_bad_chunk_size_knob(engine, enc_a, monkeypatch):
    monkeypatch.setenv("GBPE_DEBUG", "me_cs=512")
    rc, n, out = host_call(engine, enc_a, b"aaaa", np.zeros(4, np.uint8), MASK)
    assert rc == _lib.GBPE_E_INVALID and n == 0 and (out == CANARY).all()


# ── status ─────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("call", [host_call, dev_call])
def test_status(engine, enc_a, call):
    data = b"aaaa aaaaa"
    ws = _mask(len(data), [0, 2, 5])
    want = encode_words_ref(data, A_MERGES, ws)
    total = len(want)
    for bad_ws, bad_mode in ((ws, 4), (ws, 0xFFFFFFFF), (None, MASK), (ws, NONE), (ws, HEUR), (ws, GPT4)):
        rc, n, out = call(engine, enc_a, data, bad_ws, bad_mode)
        assert rc == _lib.GBPE_E_INVALID and n == 0 and (out == CANARY).all(), (bad_mode, bad_ws is None)
    rc, n, out = call(engine, enc_a, b"", ws[:0], MASK)
    assert rc == _lib.GBPE_OK and n == 0 and (out == CANARY).all()
    rc, n, out = call(engine, enc_a, b"", None, GPT4)
    assert rc == _lib.GBPE_OK and n == 0 and (out == CANARY).all()
    rc, n, out = call(engine, enc_a, data, ws, MASK, out_cap=total - 1)
    assert rc == _lib.GBPE_E_CAPACITY and n == total
    assert out[: total - 1].tolist() == want[: total - 1] and (out[total - 1:] == CANARY).all()
    rc, n, out = call(engine, enc_a, data, ws, MASK, out_cap=total)
    assert rc == _lib.GBPE_OK and n == total and out[:total].tolist() == want and (out[total:] == CANARY).all()


def test_size_query(engine, enc_a):
    data = b"aaaa aaaaa"
    ws = _mask(len(data), [0, 2, 5])
    total = len(encode_words_ref(data, A_MERGES, ws))
    lib = _lib.load()
    n = C.c_uint64()
    buf = C.create_string_buffer(data, len(data))
    rc = lib.gbpe_bpe_encode_words(engine.device, enc_a._h, buf, len(data), ws.ctypes.data_as(C.c_void_p), MASK, None, 0,
                                   C.byref(n))
    assert rc == _lib.GBPE_E_CAPACITY and n.value == total
    dev = DevBuffers(engine)
    try:
        d_in, d_ws = dev.alloc(len(data), np.frombuffer(data, np.uint8)), dev.alloc(len(data), ws)
        rc = lib.gbpe_bpe_encode_words_device(engine.device, enc_a._h, d_in, len(data), d_ws, MASK, None, 0, C.byref(n))
        assert rc == _lib.GBPE_E_CAPACITY and n.value == total
        d_out = dev.alloc(64)
        rc = lib.gbpe_bpe_encode_words_device(engine.device, enc_a._h, d_in, len(data), d_ws, MASK,
                                              C.c_void_p(d_out.value + 2), 16, C.byref(n))
        assert rc == _lib.GBPE_E_INVALID and n.value == 0   # d_out is not 4-byte aligned
    finally:
        dev.free()


# ── device form ────────────────────────────────────────────────────────────

@pytest.mark.parametrize("off", [1, 2, 3])
def test_device_alignment_and_bounds(engine, off):
    merges, data = model("code", 53), text("code", 53)[:5000] + b"\na"
    merges = merges + [[A, A, 900]]   # the byte behind the input would merge with the last one
    enc = MergeEncoder(engine, merges)
    n = len(data)
    ws = (np.random.default_rng(off).random(n) < 0.1).astype(np.uint8)
    ws[n - 1] = 0
    want = encode_words_ref(data, merges, ws)
    assert want[-1] == A and encode_words_ref(data + b"a", merges, np.append(ws, 0).astype(np.uint8))[-1] == 900
    for ws_tail in (b"\0\0\0\0", b"\1\1\1\1"):
        rc, m, out = dev_call(engine, enc, data, ws, MASK, off=off, tail=b"aaaa", ws_tail=ws_tail)
        assert rc == _lib.GBPE_OK and out[:m].tolist() == want and (out[m:] == CANARY).all(), (off, ws_tail)
    cap = len(want) - 100
    rc, m, out = dev_call(engine, enc, data, ws, MASK, out_cap=cap, off=off, tail=b"aaaa")
    assert rc == _lib.GBPE_E_CAPACITY and m == len(want)
    assert out[:cap].tolist() == want[:cap] and (out[cap:] == CANARY).all()
    arr = np.frombuffer(data, np.uint8)
    for mode, oracle_ws in ((HEUR, O.heuristic_word_starts(arr)), (GPT4, O.gpt4_word_starts(data))):
        rc, m, out = dev_call(engine, enc, data, None, mode, off=off, tail=b"aaaa")
        assert rc == _lib.GBPE_OK and out[:m].tolist() == encode_words_ref(data, merges, oracle_ws), (off, mode)
        assert (out[m:] == CANARY).all()
    rc, m, out = dev_call(engine, enc, data, None, NONE, off=off, tail=b"aaaa")
    assert rc == _lib.GBPE_OK and out[:m].tolist() == enc.encode_bytes(data).tolist() and (out[m:] == CANARY).all()
    enc.destroy()


# ── the existing entry point ───────────────────────────────────────────────

def test_whole_string_encode_unchanged(engine):
    b = ord("b")
    cases = [
        ([[A, A, 256]], b"a" * 9),
        (A_MERGES, b"a" * 10_001 + b" aa"),
        ([[256, A, 300], [A, A, 256]], b"aaaa"),
        ([[A, b, 256], [A, b, 257], [256, ord("c"), 258]], b"abcabab c"),
        ([], b"hello"),
        ([[A, b, 256]], b""),
        (XY_MERGES, XY_TEXT),
    ]
    for merges, data in cases:
        enc = MergeEncoder(engine, merges)
        want = O.encode_merge_order(data, merges)
        assert enc.encode_bytes(data).tolist() == want, (merges, data[:20])
        rc, n, out = host_call(engine, enc, data, None, NONE)
        assert rc == _lib.GBPE_OK and out[:n].tolist() == want, (merges, data[:20])
        enc.destroy()


def plain_call(engine, enc, data, out_cap, null_out=False):
    """gbpe_bpe_encode into a guarded host array (or out = NULL): (status, n_out, out[out_cap + GUARD])."""
    out = np.full(out_cap + GUARD, CANARY, np.uint32)
    buf = C.create_string_buffer(data, len(data)) if data else None
    n = C.c_uint64(12345)
    outp = None if null_out else out.ctypes.data_as(_lib.u32p)
    rc = _lib.load().gbpe_bpe_encode(engine.device, enc._h, buf, len(data), outp, out_cap, C.byref(n))
    return rc, int(n.value), out


@pytest.mark.parametrize("data", [b"aaaa aaaaa", b"a" * 1025 + b" aa"], ids=["short", "long-segment"])
def test_whole_string_encode_statuses(engine, enc_a, data):
    # gbpe_bpe_encode is gbpe_bpe_encode_words with GBPE_WORDS_NONE: its statuses and its tokens
    # (the second input has one segment just past 1024 bytes: the heap arena path)
    want = O.encode_merge_order(data, A_MERGES)
    total = len(want)
    rc, n, out = plain_call(engine, enc_a, data, total)
    assert rc == _lib.GBPE_OK and n == total and out[:total].tolist() == want and (out[total:] == CANARY).all()
    wrc, wn, wout = host_call(engine, enc_a, data, None, NONE, out_cap=total)
    assert (wrc, wn) == (rc, n) and (wout == out).all()
    rc, n, out = plain_call(engine, enc_a, data, total - 1)
    assert rc == _lib.GBPE_E_CAPACITY and n == total
    assert out[: total - 1].tolist() == want[: total - 1] and (out[total - 1:] == CANARY).all()
    wrc, wn, wout = host_call(engine, enc_a, data, None, NONE, out_cap=total - 1)
    assert (wrc, wn) == (rc, n) and (wout == out).all()
    rc, n, out = plain_call(engine, enc_a, data, 0, null_out=True)
    assert rc == _lib.GBPE_E_CAPACITY and n == total and (out == CANARY).all()
    rc, n, out = plain_call(engine, enc_a, b"", 4)
    assert rc == _lib.GBPE_OK and n == 0 and (out == CANARY).all()
    wrc, wn, wout = host_call(engine, enc_a, b"", None, NONE, out_cap=4)
    assert (wrc, wn) == (rc, n) and (wout == out).all()


# ── inventory and timing ───────────────────────────────────────────────────

def test_inventory_and_timing(engine, enc_a):
    lib = _lib.load()
    names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
    assert "k_me_long" in names and "k_me_walk_words" in names and len(names) == len(set(names))
    rc, n, _ = host_call(engine, enc_a, b"aaaa aaaaa" * 50, None, GPT4)
    assert rc == _lib.GBPE_OK and n > 0
    a, b, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    assert lib.gbpe_bpe_encode_last_timing(engine.device, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert a.value >= 0 and b.value >= 0 and c.value >= 0
    assert b.value > 0   # (the walk ran)
