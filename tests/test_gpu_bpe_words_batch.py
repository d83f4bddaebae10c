"""Many documents in one call on the GPU: the document-aware GPT-4 word starts
(gbpe_pretokenize_gpt4_batch*) and the batch word-bounded merge-rank encode
(gbpe_bpe_encode_words_batch*) against the per-document oracle of
bpe_words_batch_ref.py — each document alone, offsets by cumulative length.  Host
and device forms, every chunk size of the word kernels (GBPE_DEBUG me_cs), canary
words around every output.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
from bpe_words_batch_ref import (GPT4, HAND_PAIRS, HEUR, MASK, NONE, doc_offsets, encode_words_batch_ref, gpt4_batch_ref,
                                 gpt4_forced_ref, random_cuts, split)
from bpe_words_ref import XY_MERGES, model, text
from encode_dev import DevBuffers
from gpubpe import BPEEngine, GpuPreTokenizer, MergeEncoder, _lib

pytestmark = pytest.mark.gpu

A = ord("a")
A_MERGES = [[A, A, 256], [256, A, 257], [256, 256, 258]]
CHUNK_SIZES = [4096, 1024, 256]
MODES = [NONE, MASK, HEUR, GPT4]
CANARY = 0xA5A5A5A5
CANARY64 = 0xA5A5A5A5A5A5A5A5
GUARD = 8
KINDS = [("english", 51), ("multilingual", 52), ("code", 53)]


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


# ── part 1: the GPT-4 batch mask ───────────────────────────────────────────

def pt_host(engine, data, offs):
    """gbpe_pretokenize_gpt4_batch into a guarded host array: (status, ws[GUARD + n + GUARD])."""
    data = bytes(data)
    n = len(data)
    ws = np.full(n + 2 * GUARD, 0xA5, np.uint8)
    buf = C.create_string_buffer(data, n) if data else None
    rc = _lib.load().gbpe_pretokenize_gpt4_batch(engine.device, buf, n, offs.ctypes.data_as(_lib.u64p), offs.shape[0] - 1,
                                                 C.c_void_p(ws.ctypes.data + GUARD))
    return rc, ws


def pt_dev(engine, data, offs, off=0):
    """The device form with d_bytes and d_ws `off` bytes into their allocations, the next
    document's kind of bytes right behind the input, 0xA5 around d_ws."""
    data = bytes(data)
    n = len(data)
    dev = DevBuffers(engine)
    try:
        d_in = dev.alloc(off + n + 8, np.frombuffer(b"9" * off + data + b"9t 9t 9t", np.uint8))
        d_off = dev.alloc(8 * offs.shape[0], offs)
        d_ws = dev.alloc(off + n + 2 * GUARD, np.full(off + n + 2 * GUARD, 0xA5, np.uint8))
        rc = dev.lib.gbpe_pretokenize_gpt4_batch_device(engine.device, C.c_void_p(d_in.value + off), n, d_off,
                                                        offs.shape[0] - 1, C.c_void_p(d_ws.value + off + GUARD))
        return rc, dev.fetch(d_ws, off + n + 2 * GUARD, np.uint8)[off:]
    finally:
        dev.free()


def check_mask(engine, docs, what, want=None):
    data = b"".join(docs)
    offs = doc_offsets(docs)
    want = gpt4_batch_ref(docs) if want is None else want
    n = len(data)
    for name, call in (("host", pt_host), ("device", pt_dev)):
        rc, ws = call(engine, data, offs)
        assert rc == _lib.GBPE_OK, (what, name, rc)
        got = ws[GUARD:GUARD + n]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, name, bad[:10].tolist())
        assert (ws[:GUARD] == 0xA5).all() and (ws[GUARD + n:] == 0xA5).all(), (what, name)


def test_mask_hand_pairs(engine):
    for docs, forced, per in HAND_PAIRS:
        want = np.asarray([int(c) for c in per], np.uint8)
        check_mask(engine, docs, docs, want)


@pytest.mark.parametrize("kind,seed", KINDS)
def test_mask_synth_cuts(engine, kind, seed):
    data = text(kind, seed)
    docs = split(data, random_cuts(data, 300, seed=7))
    want = gpt4_batch_ref(docs)
    if kind == "code":   # (the cuts on which the per-document rules matter: test_bpe_words_batch_host.py)
        assert int((want != gpt4_forced_ref(docs)).sum()) == 27
    check_mask(engine, docs, kind, want)


def _cut(data, starts):
    offs = [0] + sorted(set(starts)) + [len(data)]
    return [data[a:b] for a, b in zip(offs[:-1], offs[1:])]


def test_mask_block_and_halo_edges(engine):
    digits = (b"1234567890" * 500)[:5000]
    for starts in ([4095], [4096], [4097], [4095, 4096, 4097]):
        check_mask(engine, _cut(digits, starts), ("digits", starts))
    for word in (b"we'll", b"don't"):
        for lead in range(len(word) + 1):   # the word's byte `lead` is byte 4096
            head = (b"ab cd " * 700)[: 4096 - lead - 1] + b" "
            data = head + word + b" x" + b" it's 12345 we've" * 20
            w0 = len(head)
            check_mask(engine, [data], (word, lead, "one document"))
            for k in range(len(word) + 1):
                check_mask(engine, _cut(data, [w0 + k]), (word, lead, k))
    mixed = (b"it's 1234567 we'll don't x9 \xc3\xa9t\xc3\xa9 " * 400)[:9000]
    arr = np.frombuffer(mixed, np.uint8)
    for p in list(range(4096 - 17, 4096 + 18)) + [8192 - 1, 8192, 8192 + 1]:
        if (arr[p] & 0xC0) != 0x80:
            check_mask(engine, _cut(mixed, [p]), ("mixed", p))
    # two starts inside one halo, and a sequence cut by a document end on the block edge
    check_mask(engine, _cut(mixed, [4090, 4094, 4099, 4103]), "four starts around 4096")
    cutseq = b"a" * 4095 + b"\xc3" + b"9a" * 50
    check_mask(engine, _cut(cutseq, [4096]), "cut sequence at 4096")
    cutseq = b"a" * 4094 + b"\xe2\x82" + b"9a" * 50
    check_mask(engine, _cut(cutseq, [4096]), "cut 3-byte sequence at 4096")


def test_mask_empty_and_tiny_documents(engine):
    body = [b"12", b"345 don't", b"we'll 6789"]
    check_mask(engine, [b"", b""] + body, "empty first")
    check_mask(engine, body + [b"", b""], "empty last")
    check_mask(engine, body[:1] + [b""] * 70 + body[1:], "a run of 70 empty")
    check_mask(engine, [b""] * 70 + body + [b""] * 70, "runs at both ends")
    rng = np.random.default_rng(11)
    pool = np.frombuffer(b"0123456789ab' tsl", np.uint8)
    tiny = [bytes(rng.choice(pool, 2)) for _ in range(3000)]
    check_mask(engine, tiny, "3,000 two-byte documents")
    rc, ws = pt_host(engine, b"", np.zeros(4, np.uint64))
    assert rc == _lib.GBPE_OK and (ws == 0xA5).all()
    rc, ws = pt_host(engine, b"abc", np.zeros(1, np.uint64))   # n_docs == 0: nothing launched
    assert rc == _lib.GBPE_OK and (ws == 0xA5).all()


@pytest.mark.parametrize("off", [1, 2, 3])
def test_mask_device_alignment(engine, off):
    data = text("multilingual", 52)[:9000]
    data = data[: len(data) - 1] if (data[-1] & 0xC0) == 0x80 else data
    offs = random_cuts(data, 60, seed=off)
    docs = split(data, offs)
    want = gpt4_batch_ref(docs)
    rc, ws = pt_dev(engine, data, offs, off=off)
    assert rc == _lib.GBPE_OK
    assert (ws[GUARD:GUARD + len(data)] == want).all()
    assert (ws[:GUARD] == 0xA5).all() and (ws[GUARD + len(data):] == 0xA5).all()


def _bad_offsets(n):
    return [np.asarray([1, 4, n], np.uint64), np.asarray([0, 6, 4, n], np.uint64), np.asarray([0, 4, n - 1], np.uint64),
            np.asarray([0, 4, n + 5], np.uint64)]


def test_mask_bad_offsets(engine):
    data = b"12345 don't 6789"
    for offs in _bad_offsets(len(data)):
        for call in (pt_host, pt_dev):
            rc, ws = call(engine, data, offs)
            assert rc == _lib.GBPE_E_INVALID and (ws == 0xA5).all(), (offs.tolist(), call.__name__)
    dev = DevBuffers(engine)
    try:
        d = dev.alloc(64)
        rc = dev.lib.gbpe_pretokenize_gpt4_batch_device(engine.device, d, 4, C.c_void_p(d.value + 4), 1, d)
        assert rc == _lib.GBPE_E_INVALID   # d_doc_off is not 8-byte aligned
    finally:
        dev.free()


def test_pre_tokenize_batch(engine):
    pt = GpuPreTokenizer(engine)
    for docs, forced, per in HAND_PAIRS:
        ws, offs = pt.pre_tokenize_batch(docs)
        assert "".join(map(str, ws.tolist())) == per and offs.tolist() == doc_offsets(docs).tolist()
    data = b"".join(HAND_PAIRS[0][0])
    ws, offs = pt.pre_tokenize_batch(data, offsets=[0, 2, len(data)])
    assert "".join(map(str, ws.tolist())) == HAND_PAIRS[0][2]
    ws, offs = pt.pre_tokenize_batch([])
    assert ws.shape == (0,) and offs.tolist() == [0]
    one = pt.pre_tokenize_bytes(data)["wordStarts"]
    assert pt.pre_tokenize_batch([data])[0].tolist() == one.tolist()


# ── part 2: the tokens and their offsets ───────────────────────────────────

def enc_host(engine, enc, data, offs, ws, mode, out_cap=None):
    """gbpe_bpe_encode_words_batch into guarded host arrays: (status, n_out, out, tok_off)."""
    data = bytes(data)
    n, n_docs = len(data), offs.shape[0] - 1
    cap = n if out_cap is None else out_cap
    out = np.full(cap + GUARD, CANARY, np.uint32)
    tok_off = np.full(n_docs + 1 + GUARD, CANARY64, np.uint64)
    buf = C.create_string_buffer(data, n) if data else None
    cnt = C.c_uint64(12345)
    wsp = None if ws is None else np.ascontiguousarray(ws, np.uint8).ctypes.data_as(C.c_void_p)
    rc = _lib.load().gbpe_bpe_encode_words_batch(engine.device, enc._h, buf, n, offs.ctypes.data_as(_lib.u64p), n_docs, wsp,
                                                 mode, out.ctypes.data_as(_lib.u32p), cap,
                                                 tok_off.ctypes.data_as(_lib.u64p), C.byref(cnt))
    return rc, int(cnt.value), out, tok_off


def enc_dev(engine, enc, data, offs, ws, mode, out_cap=None, off=0):
    """The device form with d_bytes / d_word_starts `off` bytes into their allocations, a byte
    that would merge in front of and behind the input, and canaries behind d_out and d_tok_off."""
    data = bytes(data)
    n, n_docs = len(data), offs.shape[0] - 1
    cap = n if out_cap is None else out_cap
    dev = DevBuffers(engine)
    try:
        d_in = dev.alloc(off + n + 5, np.frombuffer(b"a" * off + data + b"aaaa\0", np.uint8))
        d_ws = None
        if ws is not None:
            host_ws = np.concatenate([np.zeros(off, np.uint8), np.asarray(ws, np.uint8), np.zeros(5, np.uint8)])
            d_ws = C.c_void_p(dev.alloc(host_ws.shape[0], host_ws).value + off)
        d_off = dev.alloc(8 * (n_docs + 1), offs)
        d_out = dev.alloc(4 * (cap + GUARD), np.full(cap + GUARD, CANARY, np.uint32))
        d_tok = dev.alloc(8 * (n_docs + 1 + GUARD), np.full(n_docs + 1 + GUARD, CANARY64, np.uint64))
        cnt = C.c_uint64(12345)
        rc = dev.lib.gbpe_bpe_encode_words_batch_device(engine.device, enc._h, C.c_void_p(d_in.value + off), n, d_off,
                                                        n_docs, d_ws, mode, d_out, cap, d_tok, C.byref(cnt))
        return rc, int(cnt.value), dev.fetch(d_out, cap + GUARD, np.uint32), dev.fetch(d_tok, n_docs + 1 + GUARD, np.uint64)
    finally:
        dev.free()


def check_enc(engine, enc, merges, docs, mode, what, ws=None, want=None):
    """Both forms give the per-document oracle's tokens and offsets and leave the canaries alone."""
    data = b"".join(docs)
    offs = doc_offsets(docs)
    tokens, tok_off = encode_words_batch_ref(docs, merges, mode, ws) if want is None else want
    nd = len(docs)
    for name, call in (("host", enc_host), ("device", enc_dev)):
        rc, n, out, toff = call(engine, enc, data, offs, ws, mode)
        assert rc == _lib.GBPE_OK and n == len(tokens), (what, name, rc, n, len(tokens))
        assert toff[: nd + 1].tolist() == tok_off, (what, name)
        assert out[:n].tolist() == tokens, (what, name)
        assert (out[n:] == CANARY).all() and (toff[nd + 1:] == CANARY64).all(), (what, name)
    return tokens, tok_off


def _rand_mask(n, seed, density=0.1):
    return (np.random.default_rng(seed).random(n) < density).astype(np.uint8)


def test_one_document_is_the_single_buffer_call(engine):
    merges, data = model("code", 53), text("code", 53)
    enc = MergeEncoder(engine, merges)
    ws = _rand_mask(len(data), 5)
    for mode, kw in ((NONE, {}), (MASK, {"word_starts": ws}), (HEUR, {"words": "heuristic"}), (GPT4, {"words": "gpt4"})):
        single = enc.encode_bytes(data, **kw).tolist()
        check_enc(engine, enc, merges, [data], mode, ("single", mode), ws if mode == MASK else None,
                  want=(single, [0, len(single)]))
        got, off = enc.encode_batch([data], **kw)
        assert got.tolist() == single and off.tolist() == [0, len(single)]
    enc.destroy()


def test_hand_cases(engine):
    enc = MergeEncoder(engine, XY_MERGES)
    assert enc.encode_bytes(b"x y").tolist() == [257]
    for mode in (NONE, HEUR, GPT4):
        check_enc(engine, enc, XY_MERGES, [b"x", b" y"], mode, ("xy", mode), want=([120, 32, 121], [0, 1, 3]))
    # a mask that is 0 at a document start still cuts there
    check_enc(engine, enc, XY_MERGES, [b"x", b" y"], MASK, "xy mask 0", ws=np.zeros(3, np.uint8),
              want=([120, 32, 121], [0, 1, 3]))
    check_enc(engine, enc, XY_MERGES, [b"x ", b"y"], MASK, "xy mask 0", ws=np.zeros(3, np.uint8),
              want=([256, 121], [0, 1, 2]))
    got, off = enc.encode_batch([b"x", b" y"])
    assert got.tolist() == [120, 32, 121] and off.tolist() == [0, 1, 3]
    got, off = enc.encode_batch(b"x y", offsets=[0, 1, 3], word_starts=[0, 0, 0])
    assert got.tolist() == [120, 32, 121] and off.tolist() == [0, 1, 3]
    got, off = enc.encode_batch([])
    assert got.tolist() == [] and off.tolist() == [0]
    enc.destroy()


def _chunk_edge_cases(cs):
    spaced = (b"aaaaaaa " * (3 * cs // 8 + 2))[: 2 * cs + 9]
    run = b"a" * (2 * cs + 9)
    cases = []
    for name, data in (("spaced", spaced), ("run", run)):
        for starts in ([cs - 1], [cs], [cs + 1], [cs - 1, cs, cs + 1], [2 * cs - 1, 2 * cs, 2 * cs + 1]):
            cases.append(((name, starts), _cut(data, starts)))
    cases.append(("600 one-byte documents", [b"a"] * 600))
    cases.append(("600 one-byte documents in a text", [b"aaaa aa"] + [b"a"] * 600 + [b" aaaaa aaa"]))
    body = [b"aaaa aaaaa", b"aaa", b"aa aaaa"]
    cases.append(("empty first", [b""] * 3 + body))
    cases.append(("empty middle", body[:1] + [b""] * 70 + body[1:]))
    cases.append(("empty last", body + [b""] * 3))   # doc_off[n_docs - 1] == n
    cases.append(("empty everywhere", [b""] * 70 + body[:2] + [b""] * 5 + body[2:] + [b""] * 70))
    cases.append(("3,000 documents", [(b"aaaa aaa a aaaaaa" * 2)[: 1 + (i * 7) % 23] for i in range(3000)]))
    # long segments (above 1024 bytes: the heap path)
    cases.append(("1,025 a, one document", [b"a" * 1025]))
    # (the short path twice; under A_MERGES the oracle gives a cut at 512 the uncut tokens, a cut at 513 others)
    cases.append(("1,025 a cut at 512", [b"a" * 512, b"a" * 513]))
    cases.append(("1,025 a cut at 513", [b"a" * 513, b"a" * 512]))
    cases.append(("a 3,000-byte run from cs - 5, then a document", [b"b" * (cs - 5), b"a" * 3000, b"aaaa b"]))
    cases.append(("a start right after a long segment", [b"aa " + b"a" * 1500, b"a" * 7, b"a" * 1100, b"", b"aa"]))
    return cases


@pytest.fixture(scope="module")
def edge_refs():
    return {cs: [(what, docs, mode, encode_words_batch_ref(docs, A_MERGES, mode))
                 for what, docs in _chunk_edge_cases(cs) for mode in (NONE, GPT4)] for cs in CHUNK_SIZES}


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_chunk_empty_and_long_edges(engine, enc_a, edge_refs, monkeypatch, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    uncut = enc_a.encode_bytes(b"a" * 1025).tolist()
    for what, docs, mode, want in edge_refs[cs]:
        check_enc(engine, enc_a, A_MERGES, docs, mode, (cs, what, mode), want=want)
        if what == "1,025 a cut at 513":
            assert want[0] != uncut   # (the cut changes the tokens)
    # the same under a caller's mask that is 0 at every document start
    for what, docs in _chunk_edge_cases(cs)[:10]:
        n = sum(map(len, docs))
        ws = _rand_mask(n, cs, 0.05)
        ws[doc_offsets(docs)[:-1].astype(np.int64)] = 0
        check_enc(engine, enc_a, A_MERGES, docs, MASK, (cs, what, "mask"), ws=ws)


@pytest.fixture(scope="module")
def synth_refs():
    refs = {}
    for kind, seed in KINDS:
        merges, data = model(kind, seed), text(kind, seed)
        docs = split(data, random_cuts(data, 300, seed=7))
        ws = _rand_mask(len(data), seed)
        refs[kind] = (merges, docs, ws, {mode: encode_words_batch_ref(docs, merges, mode, ws if mode == MASK else None)
                                         for mode in MODES})
    return refs


@pytest.mark.parametrize("cs", CHUNK_SIZES)
@pytest.mark.parametrize("kind,seed", KINDS)
def test_synth_cuts_all_modes(engine, synth_refs, monkeypatch, kind, seed, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    merges, docs, ws, want = synth_refs[kind]
    voc = O.vocab_from_merges(merges).entries
    enc = MergeEncoder(engine, merges)
    for mode in MODES:
        tokens, tok_off = check_enc(engine, enc, merges, docs, mode, (kind, cs, mode), ws if mode == MASK else None,
                                    want=want[mode])
        for d in range(0, len(docs), 7):   # every document's tokens decode to the document
            assert O.decode(tokens[tok_off[d]:tok_off[d + 1]], voc) == docs[d], (kind, mode, d)
        assert O.decode(tokens, voc) == b"".join(docs)
    if kind == "code":
        assert len(want[GPT4][0]) == 8144
        got, off = enc.encode_batch(docs, words="gpt4")
        assert got.tolist() == want[GPT4][0] and off.tolist() == want[GPT4][1]
    enc.destroy()


@pytest.mark.parametrize("call", [enc_host, enc_dev])
def test_capacity_and_size_query(engine, enc_a, call):
    docs = [b"aaaa aaaaa", b"", b"aaa", b"aa aaaa", b""]
    data, offs, nd = b"".join(docs), doc_offsets(docs), len(docs)
    ws = np.zeros(len(data), np.uint8)
    ws[[2, 5, 11]] = 1
    want, tok_off = encode_words_batch_ref(docs, A_MERGES, MASK, ws)
    total = len(want)
    for cap in (0, 1, total - 1):
        rc, n, out, toff = call(engine, enc_a, data, offs, ws, MASK, out_cap=cap)
        assert rc == _lib.GBPE_E_CAPACITY and n == total, cap
        assert toff[: nd + 1].tolist() == tok_off and (toff[nd + 1:] == CANARY64).all(), cap
        assert out[:cap].tolist() == want[:cap] and (out[cap:] == CANARY).all(), cap
    rc, n, out, toff = call(engine, enc_a, data, offs, ws, MASK, out_cap=total)
    assert rc == _lib.GBPE_OK and n == total and out[:total].tolist() == want and (out[total:] == CANARY).all()


def test_size_query_null_out(engine, enc_a):
    docs = [b"aaaa aaaaa", b"aaa"]
    data, offs = b"".join(docs), doc_offsets(docs)
    want, tok_off = encode_words_batch_ref(docs, A_MERGES, GPT4)
    lib = _lib.load()
    n = C.c_uint64()
    toff = np.zeros(3, np.uint64)
    buf = C.create_string_buffer(data, len(data))
    rc = lib.gbpe_bpe_encode_words_batch(engine.device, enc_a._h, buf, len(data), offs.ctypes.data_as(_lib.u64p), 2, None,
                                         GPT4, None, 0, toff.ctypes.data_as(_lib.u64p), C.byref(n))
    assert rc == _lib.GBPE_E_CAPACITY and n.value == len(want) and toff.tolist() == tok_off
    dev = DevBuffers(engine)
    try:
        d_in, d_off = dev.alloc(len(data), np.frombuffer(data, np.uint8)), dev.alloc(24, offs)
        d_tok = dev.alloc(64, np.full(8, CANARY64, np.uint64))
        rc = lib.gbpe_bpe_encode_words_batch_device(engine.device, enc_a._h, d_in, len(data), d_off, 2, None, GPT4, None, 0,
                                                    d_tok, C.byref(n))
        assert rc == _lib.GBPE_E_CAPACITY and n.value == len(want)
        assert dev.fetch(d_tok, 8, np.uint64).tolist() == tok_off + [CANARY64] * 5
        # a misaligned d_out, d_tok_off or d_doc_off is refused with nothing written
        d_out = dev.alloc(256, np.full(64, CANARY, np.uint32))
        dev.put(d_tok, np.full(8, CANARY64, np.uint64))
        for out_p, tok_p, off_p in ((C.c_void_p(d_out.value + 2), d_tok, d_off),
                                    (d_out, C.c_void_p(d_tok.value + 4), d_off),
                                    (d_out, d_tok, C.c_void_p(d_off.value + 4))):
            n = C.c_uint64(12345)
            rc = lib.gbpe_bpe_encode_words_batch_device(engine.device, enc_a._h, d_in, len(data), off_p, 2, None, GPT4,
                                                        out_p, 32, tok_p, C.byref(n))
            assert rc == _lib.GBPE_E_INVALID and n.value == 0
        assert (dev.fetch(d_out, 64, np.uint32) == CANARY).all() and (dev.fetch(d_tok, 8, np.uint64) == CANARY64).all()
    finally:
        dev.free()


@pytest.mark.parametrize("call", [enc_host, enc_dev])
def test_invalid_and_empty(engine, enc_a, call):
    data = b"aaaa aaaaa aaaaaa"
    n = len(data)
    ws = np.zeros(n, np.uint8)
    good = np.asarray([0, 4, n], np.uint64)

    def untouched(out, toff):
        return (out == CANARY).all() and (toff == CANARY64).all()

    for offs in _bad_offsets(n):
        for mode in MODES:
            rc, cnt, out, toff = call(engine, enc_a, data, offs, ws if mode == MASK else None, mode)
            assert rc == _lib.GBPE_E_INVALID and cnt == 0 and untouched(out, toff), (offs.tolist(), mode)
    for bad_ws, bad_mode in ((ws, 4), (ws, 0xFFFFFFFF), (None, MASK), (ws, NONE), (ws, HEUR), (ws, GPT4)):
        rc, cnt, out, toff = call(engine, enc_a, data, good, bad_ws, bad_mode)
        assert rc == _lib.GBPE_E_INVALID and cnt == 0 and untouched(out, toff), (bad_mode, bad_ws is None)
    # n == 0 or n_docs == 0: every tok_off entry 0, nothing else written
    rc, cnt, out, toff = call(engine, enc_a, b"", np.zeros(4, np.uint64), None, GPT4)
    assert rc == _lib.GBPE_OK and cnt == 0 and (out == CANARY).all()
    assert toff[:4].tolist() == [0] * 4 and (toff[4:] == CANARY64).all()
    rc, cnt, out, toff = call(engine, enc_a, data, np.zeros(1, np.uint64), None, NONE)
    assert rc == _lib.GBPE_OK and cnt == 0 and (out == CANARY).all()
    assert toff[:1].tolist() == [0] and (toff[1:] == CANARY64).all()


def test_bad_chunk_size_knob(engine, enc_a, monkeypatch):
    monkeypatch.setenv("GBPE_DEBUG", "me_cs=512")
    rc, n, out, toff = enc_host(engine, enc_a, b"aaaa", np.asarray([0, 2, 4], np.uint64), None, NONE)
    assert rc == _lib.GBPE_E_INVALID and n == 0 and (out == CANARY).all() and (toff == CANARY64).all()


@pytest.mark.parametrize("off", [1, 2, 3])
def test_device_odd_offsets(engine, off):
    merges, data = model("code", 53), text("code", 53)[:5000] + b"\na"
    merges = merges + [[A, A, 900]]   # the bytes around the input would merge with its ends
    enc = MergeEncoder(engine, merges)
    offs = random_cuts(data, 40, seed=off)
    docs = split(data, offs)
    ws = _rand_mask(len(data), off)
    ws[len(data) - 1] = 0
    for mode in MODES:
        want, tok_off = encode_words_batch_ref(docs, merges, mode, ws if mode == MASK else None)
        assert want[-1] == A
        rc, n, out, toff = enc_dev(engine, enc, data, offs, ws if mode == MASK else None, mode, off=off)
        assert rc == _lib.GBPE_OK and out[:n].tolist() == want and (out[n:] == CANARY).all(), (off, mode)
        assert toff[: len(docs) + 1].tolist() == tok_off and (toff[len(docs) + 1:] == CANARY64).all(), (off, mode)
    enc.destroy()


def test_inventory_and_timing(engine, enc_a):
    lib = _lib.load()
    names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
    for name in ("k_doc_flags", "k_pretok_docs", "k_me_mask01", "k_me_walk_docs", "k_me_tok_off"):
        assert name in names, name
    assert len(names) == len(set(names))
    docs = [b"aaaa aaaaa" * 50, b"aaa" * 40]
    rc, n, _, _ = enc_host(engine, enc_a, b"".join(docs), doc_offsets(docs), None, GPT4)
    assert rc == _lib.GBPE_OK and n > 0
    a, b, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    assert lib.gbpe_bpe_encode_last_timing(engine.device, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert a.value >= 0 and b.value >= 0 and c.value >= 0
    assert b.value > 0   # (the walk ran)
