"""Special tokens of the merge-rank encode on the GPU: the matcher alone
(gbpe_specials_mark*) against mark_ref, and the encoder (gbpe_bpe_encode_special*)
against encode_special_ref — each piece between accepted specials alone, each special
one token.  Host and device forms, single buffer and batch, every chunk size of the
word kernels (GBPE_DEBUG me_cs), canary words around every output.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
from bpe_words_ref import XY_MERGES, model
from encode_dev import DevBuffers
from gpubpe import BPEEngine, MergeEncoder, _lib
from gpubpe.merge_encoder import checked_special_tokens
from special_ref import (GPT4, HEUR, IDS, MASK, NONE, TABLE, doc_offsets, encode_special_ref, mark_ref, random_cuts,
                         recipe, split)

pytestmark = pytest.mark.gpu

A = ord("a")
A_MERGES = [[A, A, 256], [256, A, 257], [256, 256, 258]]
CHUNK_SIZES = [4096, 1024, 256]
MODES = [NONE, MASK, HEUR, GPT4]
CANARY = 0xA5A5A5A5
CANARY64 = 0xA5A5A5A5A5A5A5A5
GUARD = 8
EOT = b"<|endoftext|>"


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


def make(engine, merges, specials, ids=None):
    ids = list(range(1000, 1000 + len(specials))) if ids is None else ids
    return MergeEncoder(engine, merges, special_tokens=dict(zip(specials, ids)))


# ── part 1: the matcher ────────────────────────────────────────────────────

def mark_host(engine, enc, data, offs=None):
    data = bytes(data)
    n = len(data)
    mark = np.full(n + 2 * GUARD, 0xA5, np.uint8)
    buf = C.create_string_buffer(data, n) if data else None
    rc = _lib.load().gbpe_specials_mark(engine.device, enc._sp, buf, n,
                                        offs.ctypes.data_as(_lib.u64p) if offs is not None else None,
                                        offs.shape[0] - 1 if offs is not None else 0, C.c_void_p(mark.ctypes.data + GUARD))
    return rc, mark


def mark_dev(engine, enc, data, offs=None, off=0, tail=None):
    """The device form with d_bytes and d_mark `off` bytes into their allocations, more of the
    input's last bytes right behind it, 0xA5 around d_mark."""
    data = bytes(data)
    n = len(data)
    dev = DevBuffers(engine)
    try:
        tail = (data[-200:] * 2)[:200] if tail is None else tail
        d_in = dev.alloc(off + n + len(tail), np.frombuffer(b"<" * off + data + tail, np.uint8))
        d_off = dev.alloc(8 * offs.shape[0], offs) if offs is not None else None
        d_mark = dev.alloc(off + n + 2 * GUARD, np.full(off + n + 2 * GUARD, 0xA5, np.uint8))
        rc = dev.lib.gbpe_specials_mark_device(engine.device, enc._sp, C.c_void_p(d_in.value + off), n, d_off,
                                               offs.shape[0] - 1 if offs is not None else 0,
                                               C.c_void_p(d_mark.value + off + GUARD))
        return rc, dev.fetch(d_mark, off + n + 2 * GUARD, np.uint8)[off:]
    finally:
        dev.free()


def check_mark(engine, enc, specials, docs, what, off=0):
    one = isinstance(docs, bytes)
    data = docs if one else b"".join(docs)
    offs = None if one else doc_offsets(docs)
    want = mark_ref(docs, specials)
    n = len(data)
    for name, call in (("host", mark_host), ("device", lambda *a: mark_dev(*a, off=off))):
        rc, mark = call(engine, enc, data, offs)
        assert rc == _lib.GBPE_OK, (what, name, rc)
        bad = np.flatnonzero(mark[GUARD:GUARD + n] != want)
        assert bad.size == 0, (what, name, bad[:10].tolist())
        assert (mark[:GUARD] == 0xA5).all() and (mark[GUARD + n:] == 0xA5).all(), (what, name)
    return want


def test_mark_identities(engine):
    for specials, data, starts in (([b"aa"], b"aaaaa", [0, 2]), ([b"<|a|>"], b"<|<|a|>|>", [2]),
                                   ([b"abc", b"bcd", b"cb"], b"abcbcd", [0, 3]),
                                   ([b"<s>", b"<s>>"], b"<s><s>>x<s", [0, 3])):
        enc = make(engine, A_MERGES, specials)
        want = check_mark(engine, enc, specials, data, (specials, data))
        assert np.flatnonzero((want != 0) & (want != 255)).tolist() == starts
        assert enc.find_special(data).tolist() == want.tolist()
        enc.destroy()


def test_mark_block_edges_and_ends(engine):
    specials = [EOT, b"EOT", b"007", b"re", b"X" * 128]
    enc = make(engine, A_MERGES, specials)
    filler = (b"int x = 12; ab cd " * 600)
    for sp in (EOT, b"X" * 128):
        for at in (4095, 4096, 4096 - 127, 4096 - 1, 4096 - len(sp), 4096 - len(sp) + 1, 8192 - 3):
            data = filler[:at] + sp + filler[: 9000 - at - len(sp)]
            want = check_mark(engine, enc, specials, data, (sp[:4], at))
            assert want[at] == 1 + specials.index(sp) and (want[at + 1:at + len(sp)] == 255).all()
    for data, what in ((filler[:5000] + EOT, "ends at n"), (EOT + filler[:5000], "at byte 0"), (EOT, "the whole input"),
                       (b"X" * 128, "the whole input, 128 bytes"), (filler[:4090] + EOT[:-1], "near miss at the end"),
                       (filler[:4096] + b"X" * 127, "near miss of 127 bytes"), (b"r", "one byte"),
                       (EOT * 700, "specials only")):
        check_mark(engine, enc, specials, data, what)
    # the bytes behind the input complete a special: it must not match (the device form's tail does that)
    rc, mark = mark_dev(engine, enc, filler[:100] + EOT[:5], tail=EOT[5:] + b"abc")
    assert rc == _lib.GBPE_OK and (mark[GUARD:GUARD + 105] == mark_ref(filler[:100] + EOT[:5], specials)).all()
    enc.destroy()


def test_mark_chains_cross_blocks(engine):
    for specials in ([b"aa"], [b"aaa", b"aaaaaaa"], [b"a" * 128, b"aa"], [b"ab", b"ba", b"aba"]):
        enc = make(engine, A_MERGES, specials)
        check_mark(engine, enc, specials, b"a" * 9000, (specials[0][:4], "run"))
        check_mark(engine, enc, specials, b"b" + b"a" * 8999, (specials[0][:4], "shifted run"))
        rng = np.random.default_rng(len(specials[0]))
        check_mark(engine, enc, specials, bytes(rng.choice(np.frombuffer(b"aaab", np.uint8), 9000).tolist()), "random ab")
        enc.destroy()


def test_mark_big_table_and_alignment(engine):
    specials = [b"<" + bytes([48 + k // 64, 48 + k % 64]) + b"|" * (1 + k % 5) for k in range(254)]
    assert len(set(specials)) == 254
    enc = make(engine, A_MERGES, specials)
    rng = np.random.default_rng(9)
    data = b"".join(specials[int(k)] + b"ab<cd"[: int(k) % 6] for k in rng.integers(0, 254, 900))
    want = check_mark(engine, enc, specials, data, "254 entries, one first byte")
    assert len(set(want.tolist()) - {0, 255}) > 200
    for off in (1, 2, 3):
        check_mark(engine, enc, specials, data[:6000], ("odd alignment", off), off=off)
    enc.destroy()


def test_mark_documents(engine):
    specials = [b"<s>", b"<s>>", EOT]
    enc = make(engine, A_MERGES, specials)
    check_mark(engine, enc, specials, [b"x<s>", b">"], "the longer one is cut, the shorter fits")
    check_mark(engine, enc, specials, [b"ab<|endof", b"text|>cd", EOT, b"", b"", EOT + b"<s"], "cut special, empty documents")
    check_mark(engine, enc, specials, [b"", b"", EOT * 3, b""], "empty first and last")
    data, _ = recipe()
    docs = split(data, random_cuts(data, 300, seed=11))
    table = TABLE
    enc2 = make(engine, A_MERGES, table)
    want = check_mark(engine, enc2, table, docs, "recipe cut again")
    assert int(((want != 0) & (want != 255)).sum()) < 317   # (some cuts fell inside specials)
    assert enc2.find_special(docs).tolist() == want.tolist()
    n = len(data)
    for offs in (np.asarray([1, 4, n], np.uint64), np.asarray([0, 6, 4, n], np.uint64), np.asarray([0, 4, n - 1], np.uint64),
                 np.asarray([0, 4, n + 5], np.uint64)):
        for call in (mark_host, mark_dev):
            rc, mark = call(engine, enc2, data, offs)
            assert rc == _lib.GBPE_E_INVALID and (mark == 0xA5).all(), (offs.tolist(), call.__name__)
    rc, mark = mark_host(engine, enc2, b"", None)
    assert rc == _lib.GBPE_OK and (mark == 0xA5).all()
    rc, mark = mark_host(engine, enc2, b"re", np.zeros(1, np.uint64))   # n_docs == 0: nothing written
    assert rc == _lib.GBPE_OK and (mark == 0xA5).all()
    enc.destroy()
    enc2.destroy()


def test_upload_rejections(engine):
    lib = _lib.load()

    def upload(strings, ids=None):
        raw = np.frombuffer(b"".join(strings) + b"\0", np.uint8)
        offs = np.zeros(len(strings) + 1, np.uint64)
        offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
        ids = np.asarray(ids if ids is not None else list(range(len(strings))) + [0], np.uint32)
        h = C.c_void_p(0xDEAD)
        rc = lib.gbpe_specials_upload(engine.device, raw.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(_lib.u64p),
                                      ids.ctypes.data_as(_lib.u32p), len(strings), C.byref(h))
        return rc, h

    for strings in ([], [bytes([1, k]) for k in range(255)], [b"a", b""], [b"a" * 129], [b"ab", b"c", b"ab"]):
        rc, h = upload(strings)
        assert rc == _lib.GBPE_E_INVALID and not h.value, len(strings)
    rc, h = upload([bytes([1, k]) for k in range(254)])
    assert rc == _lib.GBPE_OK and h.value
    lib.gbpe_specials_free(h)
    rc, h = upload([b"a" * 128, b"a"], [0xFFFFFFFF, 0])
    assert rc == _lib.GBPE_OK and h.value
    lib.gbpe_specials_free(h)
    for table in ({}, {b"": 1}, {b"a" * 129: 1}, {"a": 1, b"a": 2}):
        with pytest.raises(_lib.GpuBpeError):
            MergeEncoder(engine, A_MERGES, special_tokens=table)
    assert checked_special_tokens({"<s>": 3}) == [(b"<s>", 3)]


# ── part 2: the encoder ────────────────────────────────────────────────────

def enc_host(engine, enc, data, offs, ws, mode, out_cap=None, sp=True):
    """gbpe_bpe_encode_special (offs None) or _batch into guarded host arrays: (status, n_out, out, tok_off)."""
    data = bytes(data)
    n = len(data)
    n_docs = 0 if offs is None else offs.shape[0] - 1
    cap = n if out_cap is None else out_cap
    out = np.full(cap + GUARD, CANARY, np.uint32)
    tok_off = np.full(n_docs + 1 + GUARD, CANARY64, np.uint64)
    buf = C.create_string_buffer(data, n) if data else None
    cnt = C.c_uint64(12345)
    wsp = None if ws is None else np.ascontiguousarray(ws, np.uint8).ctypes.data_as(C.c_void_p)
    lib, h = _lib.load(), (enc._sp if sp else None)
    if offs is None:
        rc = lib.gbpe_bpe_encode_special(engine.device, enc._h, h, buf, n, wsp, mode, out.ctypes.data_as(_lib.u32p), cap,
                                         C.byref(cnt))
    else:
        rc = lib.gbpe_bpe_encode_special_batch(engine.device, enc._h, h, buf, n, offs.ctypes.data_as(_lib.u64p), n_docs, wsp,
                                               mode, out.ctypes.data_as(_lib.u32p), cap, tok_off.ctypes.data_as(_lib.u64p),
                                               C.byref(cnt))
    return rc, int(cnt.value), out, tok_off


def enc_dev(engine, enc, data, offs, ws, mode, out_cap=None, sp=True, off=0):
    """The device forms with d_bytes / d_word_starts `off` bytes into their allocations, bytes that
    would merge or match in front of and behind the input, canaries behind d_out and d_tok_off."""
    data = bytes(data)
    n = len(data)
    n_docs = 0 if offs is None else offs.shape[0] - 1
    cap = n if out_cap is None else out_cap
    dev = DevBuffers(engine)
    try:
        d_in = dev.alloc(off + n + 5, np.frombuffer(b"a" * off + data + b"aaaa\0", np.uint8))
        d_ws = None
        if ws is not None:
            host_ws = np.concatenate([np.zeros(off, np.uint8), np.asarray(ws, np.uint8), np.zeros(5, np.uint8)])
            d_ws = C.c_void_p(dev.alloc(host_ws.shape[0], host_ws).value + off)
        d_out = dev.alloc(4 * (cap + GUARD), np.full(cap + GUARD, CANARY, np.uint32))
        d_tok = dev.alloc(8 * (n_docs + 1 + GUARD), np.full(n_docs + 1 + GUARD, CANARY64, np.uint64))
        cnt = C.c_uint64(12345)
        h = enc._sp if sp else None
        if offs is None:
            rc = dev.lib.gbpe_bpe_encode_special_device(engine.device, enc._h, h, C.c_void_p(d_in.value + off), n, d_ws, mode,
                                                        d_out, cap, C.byref(cnt))
        else:
            d_off = dev.alloc(8 * (n_docs + 1), offs)
            rc = dev.lib.gbpe_bpe_encode_special_batch_device(engine.device, enc._h, h, C.c_void_p(d_in.value + off), n,
                                                              d_off, n_docs, d_ws, mode, d_out, cap, d_tok, C.byref(cnt))
        return rc, int(cnt.value), dev.fetch(d_out, cap + GUARD, np.uint32), dev.fetch(d_tok, n_docs + 1 + GUARD, np.uint64)
    finally:
        dev.free()


def check_enc(engine, enc, docs, mode, what, want, ws=None):
    """Both forms give the reference's tokens (docs a list: and offsets) and leave the canaries alone."""
    one = isinstance(docs, bytes)
    data = docs if one else b"".join(docs)
    offs = None if one else doc_offsets(docs)
    tokens, tok_off = want
    nd = 0 if one else len(docs)
    for name, call in (("host", enc_host), ("device", enc_dev)):
        rc, n, out, toff = call(engine, enc, data, offs, ws, mode)
        assert rc == _lib.GBPE_OK and n == len(tokens), (what, name, rc, n, len(tokens))
        bad = np.flatnonzero(out[:n] != np.asarray(tokens, np.uint32))
        assert bad.size == 0, (what, name, bad[:5].tolist())
        assert (out[n:] == CANARY).all(), (what, name)
        if one:
            assert (toff == CANARY64).all(), (what, name)
        else:
            assert toff[: nd + 1].tolist() == tok_off and (toff[nd + 1:] == CANARY64).all(), (what, name)


def _rand_mask(n, seed, density=0.1):
    return (np.random.default_rng(seed).random(n) < density).astype(np.uint8)


@pytest.fixture(scope="module")
def recipe_refs():
    data, merges = recipe()
    docs = split(data, random_cuts(data, 300, seed=11))
    ws = _rand_mask(len(data), 3)
    single = {m: encode_special_ref([data], merges, TABLE, IDS, m, ws if m == MASK else None) for m in MODES}
    batch = {m: encode_special_ref(docs, merges, TABLE, IDS, m, ws if m == MASK else None) for m in MODES}
    return data, merges, docs, ws, single, batch


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_recipe_all_modes(engine, recipe_refs, monkeypatch, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    data, merges, docs, ws, single, batch = recipe_refs
    assert len(data) == 13554 and len(single[GPT4][0]) == 8497
    enc = make(engine, merges, TABLE, IDS)
    for mode in MODES:
        m = ws if mode == MASK else None
        check_enc(engine, enc, data, mode, (cs, mode, "single"), single[mode], m)
        check_enc(engine, enc, docs, mode, (cs, mode, "batch"), batch[mode], m)
    assert enc.encode_bytes(data, words="gpt4").tolist() == single[GPT4][0]
    got, off = enc.encode_batch(docs, words="gpt4")
    assert got.tolist() == batch[GPT4][0] and off.tolist() == batch[GPT4][1]
    # special=False: today's result
    plain = MergeEncoder(engine, merges)
    assert enc.encode_bytes(data, words="gpt4", special=False).tolist() == plain.encode_bytes(data, words="gpt4").tolist()
    got, off = enc.encode_batch(docs, words="gpt4", special=False)
    want, woff = plain.encode_batch(docs, words="gpt4")
    assert got.tolist() == want.tolist() and off.tolist() == woff.tolist()
    plain.destroy()
    enc.destroy()


def test_hand_cases(engine):
    enc = make(engine, XY_MERGES, [b"<|e|>"], [999])
    for mode in (NONE, HEUR, GPT4):
        check_enc(engine, enc, b"x y<|e|>x y", mode, "xy", encode_special_ref([b"x y<|e|>x y"], XY_MERGES, [b"<|e|>"], [999], mode))
    assert enc.encode_bytes(b"x y<|e|>x y").tolist() == [257, 999, 257]
    assert enc.encode_bytes(b"x <|e|>y").tolist() == [256, 999, 121]
    assert enc.encode("x <|e|>y")["tokens"] == [256, 999, 121]
    assert enc.encode_bytes(b"").tolist() == []
    enc.destroy()
    # the piece alone, not the buffer with the edges forced
    merges = model("code", 53)
    enc = make(engine, merges, [b"EOT", b"007"], [70000, 70001])
    for data in (b"itEOT's", b"1200734", b"it's EOTit's007's 12345"):
        for mode in MODES:
            ws = _rand_mask(len(data), 1, 0.4) if mode == MASK else None
            check_enc(engine, enc, data, mode, (data, mode),
                      encode_special_ref([data], merges, [b"EOT", b"007"], [70000, 70001], mode, ws), ws)
    enc.destroy()


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_chunk_edges_long_pieces_adjacent(engine, monkeypatch, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    specials, ids = [EOT, b"aaa<"], [999, 998]
    enc = make(engine, A_MERGES, specials, ids)
    spaced = (b"aaaaaaa " * (3 * cs // 8 + 40))
    cases = []
    for k in (1, 2, 3):   # a special that starts in the last byte of lane k's chunk and runs into the next
        cases.append((("last byte of chunk", k), spaced[: k * cs - 1] + EOT + spaced[:50]))
        cases.append((("first byte of chunk", k), spaced[: k * cs] + EOT + spaced[:50]))
        cases.append((("over the chunk edge", k), b"a" * (k * cs - 6) + EOT + b"a" * 50))
    cases.append(("after a 1,500-byte piece", b"a" * 1500 + EOT + b"aa"))
    cases.append(("before a 1,500-byte piece", b"aa" + EOT + b"a" * 1500))
    cases.append(("between two long pieces", b"a" * 1100 + EOT + b"a" * 1025 + EOT))
    cases.append(("two adjacent", b"aaaa" + EOT + EOT + b"aaaa"))
    cases.append(("adjacent, different", b"aaaa<" + EOT + b"aaa<" + EOT))
    cases.append(("specials only", EOT * (cs // 13 + 3)))
    cases.append(("one special", EOT))
    for what, data in cases:
        for mode in (NONE, GPT4):
            check_enc(engine, enc, data, mode, (cs, what, mode), encode_special_ref([data], A_MERGES, specials, ids, mode))
    uncut = enc.encode_bytes(b"a" * 1500, special=False).tolist()
    assert enc.encode_bytes(EOT + b"a" * 1500).tolist() == [999] + uncut
    # ("aaa<" takes the < of an EOT that follows a run: the piece before it is 1,497 bytes, the heap path still)
    assert enc.encode_bytes(b"a" * 1500 + EOT).tolist() == enc.encode_bytes(b"a" * 1497, special=False).tolist() + [998] + \
        enc.encode_bytes(EOT[1:], special=False).tolist()
    # as documents: a special at a document's first byte, empty documents, a cut special
    docs = [b"", EOT + b"aaaa", b"", EOT, b"aa" + EOT[:5], EOT[5:] + b"aaa", b"a" * 1500, EOT + b"a" * (cs + 3) + EOT, b""]
    for mode in (NONE, GPT4):
        check_enc(engine, enc, docs, mode, (cs, "documents", mode), encode_special_ref(docs, A_MERGES, specials, ids, mode))
    enc.destroy()


def test_no_match_is_the_plain_call(engine):
    data, merges = recipe()
    enc = make(engine, merges, [b"<|never|>", b"<|fim_prefix|>", b"\xff\xfe"])
    plain = MergeEncoder(engine, merges)
    docs = split(data, random_cuts(data, 300, seed=11))
    ws = _rand_mask(len(data), 3)
    for mode, kw in ((NONE, {}), (MASK, {"word_starts": ws}), (HEUR, {"words": "heuristic"}), (GPT4, {"words": "gpt4"})):
        assert enc.encode_bytes(data, **kw).tolist() == plain.encode_bytes(data, **kw).tolist(), mode
        got, off = enc.encode_batch(docs, **kw)
        want, woff = plain.encode_batch(docs, **kw)
        assert got.tolist() == want.tolist() and off.tolist() == woff.tolist(), mode
    assert not enc.find_special(data).any()
    plain.destroy()
    enc.destroy()


@pytest.mark.parametrize("call", [enc_host, enc_dev])
def test_capacity_invalid_and_empty(engine, call):
    specials, ids = [EOT], [999]
    enc = make(engine, A_MERGES, specials, ids)
    docs = [b"aaaa aaaaa", b"", EOT + b"aaa", b"aa" + EOT + b"aaaa", b""]
    data, offs, nd = b"".join(docs), doc_offsets(docs), len(docs)
    for o, d in ((offs, docs), (None, [data])):
        want, tok_off = encode_special_ref(d, A_MERGES, specials, ids, GPT4)
        total = len(want)
        for cap in (0, 1, total - 1):
            rc, n, out, toff = call(engine, enc, data, o, None, GPT4, out_cap=cap)
            assert rc == _lib.GBPE_E_CAPACITY and n == total, cap
            assert out[:cap].tolist() == want[:cap] and (out[cap:] == CANARY).all(), cap
            if o is not None:
                assert toff[: nd + 1].tolist() == tok_off and (toff[nd + 1:] == CANARY64).all(), cap
        rc, n, out, toff = call(engine, enc, data, o, None, GPT4, out_cap=total)
        assert rc == _lib.GBPE_OK and n == total and out[:total].tolist() == want and (out[total:] == CANARY).all()
    n = len(data)
    ws = np.zeros(n, np.uint8)

    def untouched(out, toff):
        return (out == CANARY).all() and (toff == CANARY64).all()

    for bad in (np.asarray([1, 4, n], np.uint64), np.asarray([0, 6, 4, n], np.uint64), np.asarray([0, 4, n - 1], np.uint64)):
        for mode in MODES:
            rc, cnt, out, toff = call(engine, enc, data, bad, ws if mode == MASK else None, mode)
            assert rc == _lib.GBPE_E_INVALID and cnt == 0 and untouched(out, toff), (bad.tolist(), mode)
    for o in (offs, None):
        for bad_ws, bad_mode in ((ws, 4), (None, MASK), (ws, NONE), (ws, GPT4)):
            rc, cnt, out, toff = call(engine, enc, data, o, bad_ws, bad_mode)
            assert rc == _lib.GBPE_E_INVALID and cnt == 0 and untouched(out, toff), (bad_mode, bad_ws is None)
        rc, cnt, out, toff = call(engine, enc, data, o, None, GPT4, sp=False)   # specials == NULL
        assert rc == _lib.GBPE_E_INVALID and cnt == 0 and untouched(out, toff)
    rc, cnt, out, toff = call(engine, enc, b"", None, None, GPT4)
    assert rc == _lib.GBPE_OK and cnt == 0 and untouched(out, toff)
    rc, cnt, out, toff = call(engine, enc, b"", np.zeros(4, np.uint64), None, GPT4)
    assert rc == _lib.GBPE_OK and cnt == 0 and (out == CANARY).all()
    assert toff[:4].tolist() == [0] * 4 and (toff[4:] == CANARY64).all()
    enc.destroy()


def test_size_query_and_alignment(engine):
    enc = make(engine, A_MERGES, [EOT], [999])
    data = b"aaaa" + EOT + b"aaa"
    want, _ = encode_special_ref([data], A_MERGES, [EOT], [999], GPT4)
    lib = _lib.load()
    n = C.c_uint64()
    buf = C.create_string_buffer(data, len(data))
    rc = lib.gbpe_bpe_encode_special(engine.device, enc._h, enc._sp, buf, len(data), None, GPT4, None, 0, C.byref(n))
    assert rc == _lib.GBPE_E_CAPACITY and n.value == len(want)
    dev = DevBuffers(engine)
    try:
        d_in = dev.alloc(len(data), np.frombuffer(data, np.uint8))
        d_out = dev.alloc(256, np.full(64, CANARY, np.uint32))
        rc = lib.gbpe_bpe_encode_special_device(engine.device, enc._h, enc._sp, d_in, len(data), None, GPT4, None, 0, C.byref(n))
        assert rc == _lib.GBPE_E_CAPACITY and n.value == len(want)
        rc = lib.gbpe_bpe_encode_special_device(engine.device, enc._h, enc._sp, d_in, len(data), None, GPT4,
                                                C.c_void_p(d_out.value + 2), 32, C.byref(n))
        assert rc == _lib.GBPE_E_INVALID and n.value == 0 and (dev.fetch(d_out, 64, np.uint32) == CANARY).all()
    finally:
        dev.free()
    enc.destroy()


@pytest.mark.parametrize("off", [1, 3])
def test_device_odd_offsets(engine, off):
    data, merges = recipe()
    data = data[:5000] + b"\na"
    merges = merges + [[A, A, 900]]   # the bytes around the input would merge with its ends
    enc = make(engine, merges, TABLE, IDS)
    offs = random_cuts(data, 40, seed=off)
    docs = split(data, offs)
    ws = _rand_mask(len(data), off)
    for mode in MODES:
        m = ws if mode == MASK else None
        want, tok_off = encode_special_ref(docs, merges, TABLE, IDS, mode, m)
        rc, n, out, toff = enc_dev(engine, enc, data, offs, m, mode, off=off)
        assert rc == _lib.GBPE_OK and out[:n].tolist() == want and (out[n:] == CANARY).all(), (off, mode)
        assert toff[: len(docs) + 1].tolist() == tok_off, (off, mode)
        want, _ = encode_special_ref([data], merges, TABLE, IDS, mode, m)
        rc, n, out, toff = enc_dev(engine, enc, data, None, m, mode, off=off)
        assert rc == _lib.GBPE_OK and out[:n].tolist() == want and (out[n:] == CANARY).all(), (off, mode, "single")
    enc.destroy()


def test_round_trip_through_device_decode(engine):
    from gpubpe import flatten_vocab
    data, merges = recipe()
    voc = list(O.vocab_from_merges(merges).entries)
    first = len(voc)
    ids = [first + k for k in range(4)]   # directly after the model's
    enc = make(engine, merges, TABLE, ids)
    tokens = enc.encode_bytes(data, words="gpt4")
    assert int((tokens >= first).sum()) == 317
    flat, offs = flatten_vocab(voc + TABLE)   # the specials' strings at their ids
    lib, ctx = _lib.load(), engine.device
    dv = C.c_void_p()
    _lib.check(lib.gbpe_vocab_upload(ctx, flat.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(_lib.u64p), offs.shape[0] - 1,
                                     C.byref(dv)), ctx, "vocab upload")
    out = np.zeros(len(data) + 8, np.uint8)
    n = C.c_uint64()
    _lib.check(lib.gbpe_decode(ctx, dv, tokens.ctypes.data_as(_lib.u32p), tokens.shape[0], out.ctypes.data_as(C.c_void_p),
                               out.shape[0], C.byref(n)), ctx, "decode")
    assert n.value == len(data) and out[: n.value].tobytes() == data
    lib.gbpe_vocab_free(dv)
    enc.destroy()


def test_back_to_back_calls_and_timing(engine, recipe_refs):
    data, merges, docs, ws, single, batch = recipe_refs
    enc = make(engine, merges, TABLE, IDS)
    for _ in range(2):   # (the pooled blocks of the first call are the second's)
        assert enc.encode_bytes(data, words="gpt4").tolist() == single[GPT4][0]
        assert enc.encode_batch(docs, words="gpt4")[0].tolist() == batch[GPT4][0]
        assert enc.encode_bytes(data[:3000], words="gpt4").tolist() == \
            encode_special_ref([data[:3000]], merges, TABLE, IDS, GPT4)[0]
    lib = _lib.load()
    a, b, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    assert lib.gbpe_bpe_encode_last_timing(engine.device, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert a.value > 0 and b.value > 0 and c.value >= 0   # (the matcher counts under the word starts)
    names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
    for name in ("k_sp_cand", "k_sp_accept", "k_me_sp_mask", "k_me_walk_special"):
        assert name in names, name
    assert len(names) == len(set(names))
    enc.destroy()
