"""Byte spans of the merge-rank encode's tokens on the GPU (gbpe_bpe_encode_spans*).

Every case runs the host and the device form and asks three things: the tokens are, bit for
bit, those of the existing entry point of the same shape (gbpe_bpe_encode_words, _words_batch,
_special, _special_batch); the starts are those of the position-carrying oracle
(bpe_spans_ref.spans_ref); and the canary words before and after out, tok_start and tok_off
stand.  The shapes are the smallest at which the walk, the heap path and the compaction can
go wrong, at every chunk size of the word kernels (GBPE_DEBUG me_cs).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
import merge_models as M
import merge_wide as MW
from bpe_spans_ref import CL100K, GPT4, HEUR, MASK, NONE, doc_tok_off, spans_ref
from bpe_words_batch_ref import doc_offsets, random_cuts, split
from bpe_words_ref import model, text
from encode_dev import DevBuffers
from gpubpe import BPEEngine, MergeEncoder, _lib

pytestmark = pytest.mark.gpu

A = ord("a")
A_MERGES = [[A, A, 256], [256, A, 257], [256, 256, 258]]
CHUNK_SIZES = [4096, 1024, 256]
CANARY = 0xA5A5A5A5
CANARY64 = 0xA5A5A5A5A5A5A5A5
GUARD = 8
EOT = b"<|endoftext|>"


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


@pytest.fixture(scope="module")
def a_enc(engine):
    """The `a` model; the special's id is the model's token "aa": its span must still be the special's."""
    enc = MergeEncoder(engine, A_MERGES, special_tokens={EOT: 256, b"<s>": 998})
    yield enc
    enc.destroy()


A_SPECIALS, A_IDS = [EOT, b"<s>"], [256, 998]


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def run(engine, enc, data, offs, ws, mode, device, sp, out_cap=None, off=0, nulls=False):
    """gbpe_bpe_encode_spans (device: _device) into arrays with GUARD canary words on both sides:
    (status, n_out, out, tok_start, tok_off), the three with their guards.  `off`: d_bytes and
    d_word_starts that many bytes into their allocations.  `nulls`: out and tok_start NULL."""
    data = bytes(data)
    n = len(data)
    n_docs = 0 if offs is None else offs.shape[0] - 1
    cap = n if out_cap is None else out_cap
    h = enc._sp if sp else None
    cnt = C.c_uint64(12345)
    out = np.full(cap + 2 * GUARD, CANARY, np.uint32)
    ts = np.full(cap + 2 * GUARD, CANARY64, np.uint64)
    tok = np.full(n_docs + 1 + 2 * GUARD, CANARY64, np.uint64)
    lib = _lib.load()
    if not device:
        src = np.frombuffer(data, np.uint8)
        wsa = None if ws is None else np.ascontiguousarray(ws, np.uint8)
        rc = lib.gbpe_bpe_encode_spans(engine.device, enc._h, h, vp(src) if n else None, n,
                                       offs.ctypes.data_as(_lib.u64p) if offs is not None else None, n_docs,
                                       None if wsa is None else vp(wsa), mode,
                                       None if nulls else C.cast(out.ctypes.data + 4 * GUARD, _lib.u32p),
                                       None if nulls else C.cast(ts.ctypes.data + 8 * GUARD, _lib.u64p), cap,
                                       C.cast(tok.ctypes.data + 8 * GUARD, _lib.u64p) if offs is not None else None,
                                       C.byref(cnt))
        return rc, int(cnt.value), out, ts, tok
    dev = DevBuffers(engine)
    try:
        # bytes that would merge or match in front of and behind the input
        d_in = dev.alloc(off + n + 5, np.frombuffer(b"a" * off + data + b"aaaa\0", np.uint8))
        d_ws = None
        if ws is not None:
            host_ws = np.concatenate([np.zeros(off, np.uint8), np.asarray(ws, np.uint8), np.zeros(5, np.uint8)])
            d_ws = C.c_void_p(dev.alloc(host_ws.shape[0], host_ws).value + off)
        d_out = dev.alloc(out.nbytes, out)
        d_ts = dev.alloc(ts.nbytes, ts)
        d_tok = dev.alloc(tok.nbytes, tok)
        d_off = dev.alloc(8 * (n_docs + 1), offs) if offs is not None else None
        rc = lib.gbpe_bpe_encode_spans_device(engine.device, enc._h, h, C.c_void_p(d_in.value + off), n, d_off, n_docs, d_ws,
                                              mode, None if nulls else C.c_void_p(d_out.value + 4 * GUARD),
                                              None if nulls else C.c_void_p(d_ts.value + 8 * GUARD), cap,
                                              C.c_void_p(d_tok.value + 8 * GUARD) if offs is not None else None, C.byref(cnt))
        return (rc, int(cnt.value), dev.fetch(d_out, out.shape[0], np.uint32), dev.fetch(d_ts, ts.shape[0], np.uint64),
                dev.fetch(d_tok, tok.shape[0], np.uint64))
    finally:
        dev.free()


def existing(engine, enc, data, offs, ws, mode, sp):
    """(tokens, tok_off) of the existing entry point of the same shape (host form)."""
    data = bytes(data)
    n = len(data)
    n_docs = 0 if offs is None else offs.shape[0] - 1
    out = np.zeros(max(n, 1), np.uint32)
    tok = np.zeros(n_docs + 1, np.uint64)
    cnt = C.c_uint64()
    src = np.frombuffer(data, np.uint8)
    wsa = None if ws is None else np.ascontiguousarray(ws, np.uint8)
    lib = _lib.load()
    name = "gbpe_bpe_encode_" + ("special" if sp else "words") + ("_batch" if offs is not None else "")
    args = [engine.device, enc._h] + ([enc._sp] if sp else []) + [vp(src) if n else None, n]
    if offs is not None:
        args += [offs.ctypes.data_as(_lib.u64p), n_docs]
    args += [None if wsa is None else vp(wsa), mode, out.ctypes.data_as(_lib.u32p), out.shape[0]]
    if offs is not None:
        args += [tok.ctypes.data_as(_lib.u64p)]
    _lib.check(getattr(lib, name)(*args, C.byref(cnt)), engine.device, name)
    return out[: cnt.value].copy(), tok if offs is not None else None


def guards_stand(arr, used, canary):
    """Nothing before the array, nothing at or beyond index `used`."""
    return (arr[:GUARD] == canary).all() and (arr[GUARD + used:] == canary).all()


_REFS = {}


def ref(key, *args, **kw):
    """spans_ref, computed once per case: the chunk sizes share it."""
    if key not in _REFS:
        _REFS[key] = spans_ref(*args, **kw)
    return _REFS[key]


def check(engine, enc, docs, mode, want, what, ws=None, sp=False, off=0):
    """Host and device form: the existing call's tokens, the oracle's tokens and starts, the canaries."""
    one = isinstance(docs, bytes)
    data = docs if one else b"".join(docs)
    offs = None if one else doc_offsets(docs)
    nd = 0 if one else len(docs)
    tokens, starts = want
    old, old_off = existing(engine, enc, data, offs, ws, mode, sp)
    assert old.tolist() == tokens, (what, "the oracle's tokens are not the existing call's")
    for device in (False, True):
        rc, n, out, ts, tok = run(engine, enc, data, offs, ws, mode, device, sp, off=off if device else 0)
        assert rc == _lib.GBPE_OK and n == len(tokens), (what, device, rc, n, len(tokens))
        assert np.array_equal(out[GUARD:GUARD + n], old), (what, device)
        bad = np.flatnonzero(ts[GUARD:GUARD + n] != np.asarray(starts, np.uint64))
        assert bad.size == 0, (what, device, bad[:5].tolist(), ts[GUARD:GUARD + n][bad[:5]].tolist(),
                               [starts[i] for i in bad[:5]])
        assert guards_stand(out, n, CANARY) and guards_stand(ts, n, CANARY64), (what, device)
        if one:
            assert (tok == CANARY64).all(), (what, device)
        else:
            assert np.array_equal(tok[GUARD:GUARD + nd + 1], old_off) and guards_stand(tok, nd + 1, CANARY64), (what, device)
            assert tok[GUARD:GUARD + nd + 1].tolist() == doc_tok_off(docs, starts), (what, device)
            for d, doc in enumerate(docs):   # a non-empty document's first token starts at its first byte
                if doc:
                    assert int(ts[GUARD + int(tok[GUARD + d])]) == int(offs[d]), (what, device, d)


def a_want(docs, mode=NONE, sp=False, mask=None):
    docs = [docs] if isinstance(docs, bytes) else docs
    return spans_ref(docs, A_MERGES, A_SPECIALS if sp else (), A_IDS, mode, mask)


# ── the walk ───────────────────────────────────────────────────────────────

@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_cascading_merges(engine, a_enc, monkeypatch, cs):
    """aa→256, 256 a→257, 256 256→258 on runs of 1 to 9: a position survives several passes."""
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for k in range(1, 10):
        check(engine, a_enc, b"a" * k, NONE, a_want(b"a" * k), (cs, "run", k))
    data = b" ".join(b"a" * k for k in range(1, 10)) + b" "
    data = data * (2 * cs // len(data) + 2)   # runs across two chunk edges, at every phase
    for mode in (NONE, GPT4):
        check(engine, a_enc, data, mode, a_want(data, mode), (cs, "runs", mode))


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_chunk_edges(engine, a_enc, monkeypatch, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    spaced = b"aaaaaaa aaa aaaaa " * (3 * cs // 18 + 10)
    cases = [("a segment from the chunk's last byte", b" " * (cs - 1) + b"a" * 40 + b" aaa"),
             ("a segment from the chunk's first byte", b" " * cs + b"a" * 40 + b" aaa"),
             # the run covers chunk 1 (and at 256 chunk 2) whole: base[c] == hi there, then chunks with starts
             ("a chunk without a segment start", b"aa " * 33 + b"a" * (2 * cs + 50) + b" " + spaced[: cs + 9])]
    cases += [(("length", n), spaced[:n]) for n in (cs - 1, cs, cs + 1, 2 * cs + 1)]
    for what, data in cases:
        check(engine, a_enc, data, NONE, a_want(data), (cs, what))
    ws = (np.random.default_rng(cs).random(2 * cs + 1) < 0.2).astype(np.uint8)
    data = b"a" * (2 * cs + 1)   # every cut is the mask's
    check(engine, a_enc, data, MASK, a_want(data, MASK, mask=ws), (cs, "masked run"), ws=ws)


def uncut_byte(merges):
    """A byte u whose run is one segment: some live merge joins a token ending in u to one starting with u."""
    cross = M.cross_pairs(merges)
    us = [u for u in range(32, 127) if (u, u) in cross]
    assert us
    return us[0]


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_heap_path(engine, a_enc, monkeypatch, cs):
    """Uncut runs of exactly ME_LONG = 1024 bytes (the short path's longest) and 1025 (the heap's shortest),
    and one of about 3000 that starts mid-chunk with short words behind it."""
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for n in (1024, 1025):
        check(engine, a_enc, b"a" * n, NONE, a_want(b"a" * n), (cs, "a", n))
        data = b"aa aaa " + b"a" * n + b" aaaa"
        check(engine, a_enc, data, NONE, a_want(data), (cs, "a, inside", n))
    data = b"aaaaa a " * 12 + b"a" * 3001 + b" aaa aaaaa aa" * 9
    check(engine, a_enc, data, NONE, a_want(data), (cs, "a", 3001))
    merges = model("code", 53)
    u = bytes([uncut_byte(merges)])
    enc = MergeEncoder(engine, merges)
    code = text("code", 53)
    for n in (1024, 1025, 2999):
        data = code[:101] + b"\n" + u * n + b"\n" + code[200:420]
        assert max(M.segments(data, merges)) >= n
        check(engine, enc, data, NONE, ref(("heap, code", n), [data], merges), (cs, "code", n))
    enc.destroy()


# ── special tokens ─────────────────────────────────────────────────────────

@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_specials(engine, a_enc, monkeypatch, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    spaced = b"aaaaaaa " * (2 * cs // 8 + 40)
    cases = [("over the chunk edge", spaced[: cs - 5] + EOT + spaced[:50]),
             ("from the chunk's last byte", spaced[: 2 * cs - 1] + EOT + spaced[:50]),
             ("inside a run over the edge", b"a" * (cs - 6) + EOT + b"a" * 50),
             ("first and last bytes", EOT + spaced[:30] + EOT),
             ("back to back", b"aaaa" + EOT + EOT + b"aaaa"),
             ("back to back, different", b"aaaa<" + EOT + b"<s>" + EOT),
             ("behind a long piece", b"a" * 1500 + EOT + b"aa"),
             ("one special", EOT)]
    for what, data in cases:
        for mode in (NONE, GPT4):
            check(engine, a_enc, data, mode, a_want(data, mode, sp=True), (cs, what, mode), sp=True)
    docs = [EOT + b"aaaa", b"", b"aa" + EOT, EOT, b"aa" + EOT[:5], EOT[5:] + b"aaa", EOT + b"a" * (cs + 3) + EOT]
    for mode in (NONE, GPT4):
        check(engine, a_enc, docs, mode, a_want(docs, mode, sp=True), (cs, "documents", mode), sp=True)


def test_a_special_s_span_is_its_own_length(engine, a_enc):
    """The special's id, 256, is the model's "aa": a length table read by id would give it two bytes."""
    data = b"aaaa" + EOT + b"aa"
    want = a_want(data, sp=True)
    assert want == ([258, 256, 256], [0, 4, 17])
    check(engine, a_enc, data, NONE, want, "id of a model token", sp=True)
    tokens, starts = a_enc.encode_bytes_spans(data)
    assert tokens.tolist() == [258, 256, 256] and starts.tolist() == [0, 4, 17, 19]
    assert [data[int(s):int(e)] for s, e in zip(starts[:-1], starts[1:])] == [b"aaaa", EOT, b"aa"]


def test_a_table_that_never_matches(engine):
    merges, data = model("code", 53), text("code", 53)[:5000]
    enc = MergeEncoder(engine, merges, special_tokens={b"<|never|>": 7, b"\xff\xfe": 8})
    docs = split(data, random_cuts(data, 12, seed=5))
    for mode in (NONE, GPT4):
        want = spans_ref([data], merges, mode=mode)
        check(engine, enc, data, mode, want, ("no match", mode), sp=True)
        check(engine, enc, data, mode, want, ("no table", mode), sp=False)
        want = spans_ref(docs, merges, mode=mode)
        check(engine, enc, docs, mode, want, ("no match, batch", mode), sp=True)
    enc.destroy()


# ── many documents ─────────────────────────────────────────────────────────

@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_batch(engine, a_enc, monkeypatch, cs):
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    spaced = b"aaaaaaa aaa " * (cs // 12 + 20)
    docs = [b"", b"", spaced[:cs - 7], b"aaaaaaa", b"", b"", b"aaa aa", b"a" * (cs - 6), b"a", spaced[:cs + 5], b"", b""]
    assert len(b"".join(docs[:4])) == cs and len(b"".join(docs[:8])) == 2 * cs   # documents that end on a chunk edge
    for mode in (NONE, HEUR, GPT4):
        check(engine, a_enc, docs, mode, a_want(docs, mode), (cs, "documents", mode))
    check(engine, a_enc, [b"", b""], NONE, ([], []), (cs, "empty documents only"))
    check(engine, a_enc, [b"aaaaa"], NONE, a_want([b"aaaaa"]), (cs, "one document"))


# ── every mode, adversarial models, wide ids ──────────────────────────────

ASCII_SEEDS = [8, 16, 33]   # model_case's alphabets of two or more printable ASCII bytes (asserted below)


@pytest.mark.parametrize("cs", CHUNK_SIZES)
def test_every_mode(engine, monkeypatch, cs):
    """merge_models.model_case: NONE, MASK and HEURISTIC on every kind of model (a closed one's long texts take
    the heap path), GPT4 and CL100K on the models over printable ASCII, the rules' domain."""
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    for seed in ASCII_SEEDS:
        alpha = M.model_case(seed)["alphabet"]
        assert len(alpha) >= 2 and all(32 <= b < 128 for b in alpha), seed
    for seed in [0, 2, 3] + ASCII_SEEDS:
        case = M.model_case(seed)
        enc = MergeEncoder(engine, case["merges"], special_tokens={M.SPECIAL: M.SPECIAL_ID})
        docs, mask = M.batch_docs(case)
        sdocs = M.special_docs(case, seed)
        data = b"".join(docs)
        modes = [NONE, MASK, HEUR] + ([GPT4, CL100K] if seed in ASCII_SEEDS else [])
        for mode in modes:
            m = mask if mode == MASK else None
            check(engine, enc, docs, mode, ref((seed, mode, "batch"), docs, case["merges"], mode=mode, mask=m),
                  (cs, seed, mode, "batch"), ws=m)
            if mode != MASK:
                check(engine, enc, sdocs, mode, ref((seed, mode, "special"), sdocs, case["merges"], [M.SPECIAL], [M.SPECIAL_ID], mode),
                      (cs, seed, mode, "special batch"), sp=True)
            check(engine, enc, data, mode, ref((seed, mode, "single"), [data], case["merges"], mode=mode, mask=m),
                  (cs, seed, mode, "single"), ws=m)
        enc.destroy()


def test_words_modes_on_code(engine):
    merges, data = model("code", 53), text("code", 53)[:9000]
    enc = MergeEncoder(engine, merges, special_tokens={b"EOT": 70000, b"007": 70001})
    docs = split(data, random_cuts(data, 25, seed=3))
    ws = (np.random.default_rng(3).random(len(data)) < 0.15).astype(np.uint8)
    for mode in (NONE, MASK, HEUR, GPT4, CL100K):
        m = ws if mode == MASK else None
        check(engine, enc, data, mode, spans_ref([data], merges, mode=mode, mask=m), (mode, "single"), ws=m, off=1)
        check(engine, enc, docs, mode, spans_ref(docs, merges, mode=mode, mask=m), (mode, "batch"), ws=m, off=3)
    sdata = b"itEOT's 1200734 " + data[:3000] + b"EOT"
    for mode in (HEUR, GPT4, CL100K):
        check(engine, enc, sdata, mode, spans_ref([sdata], merges, [b"EOT", b"007"], [70000, 70001], mode), (mode, "special"),
              sp=True, off=1)
    enc.destroy()


def test_wide_ids_give_the_same_starts(engine):
    merges, data = model("code", 53), text("code", 53)[:6000]
    u = bytes([uncut_byte(merges)])
    data = data[:3000] + u * 1500 + data[3000:]
    wide = MergeEncoder(engine, MW.relabel(merges))
    assert wide.wide
    for mode in (NONE, GPT4):
        tokens, starts = spans_ref([data], merges, mode=mode)
        check(engine, wide, data, mode, (MW.relabel_tokens(tokens), starts), ("wide", mode))
    docs = split(data, random_cuts(data, 9, seed=1))
    tokens, starts = spans_ref(docs, merges, mode=GPT4)
    check(engine, wide, docs, GPT4, (MW.relabel_tokens(tokens), starts), "wide batch")
    wide.destroy()


# ── capacity, bad arguments ────────────────────────────────────────────────

@pytest.mark.parametrize("device", [False, True])
def test_capacity(engine, a_enc, device):
    docs = [b"aaaa aaaaa", b"", EOT + b"aaa", b"aa" + EOT + b"aaaa", b""]
    data, offs, nd = b"".join(docs), doc_offsets(docs), len(docs)
    for o, dd in ((offs, docs), (None, [data])):
        tokens, starts = spans_ref(dd, A_MERGES, A_SPECIALS, A_IDS, GPT4)
        total = len(tokens)
        tok_off = doc_tok_off(dd, starts)
        for cap, nulls in ((0, True), (0, False), (1, False), (total - 1, False)):
            rc, n, out, ts, tok = run(engine, a_enc, data, o, None, GPT4, device, True, out_cap=cap, nulls=nulls)
            assert rc == _lib.GBPE_E_CAPACITY and n == total, (cap, nulls, rc, n)
            assert out[GUARD:GUARD + cap].tolist() == tokens[:cap] and ts[GUARD:GUARD + cap].tolist() == starts[:cap], cap
            assert guards_stand(out, cap, CANARY) and guards_stand(ts, cap, CANARY64), cap
            if o is not None:
                assert tok[GUARD:GUARD + nd + 1].tolist() == tok_off and guards_stand(tok, nd + 1, CANARY64), cap
            else:
                assert (tok == CANARY64).all()
        for cap in (total, total + 3):
            rc, n, out, ts, tok = run(engine, a_enc, data, o, None, GPT4, device, True, out_cap=cap)
            assert rc == _lib.GBPE_OK and n == total
            assert out[GUARD:GUARD + n].tolist() == tokens and ts[GUARD:GUARD + n].tolist() == starts
            assert guards_stand(out, n, CANARY) and guards_stand(ts, n, CANARY64)


def untouched(out, ts, tok):
    return (out == CANARY).all() and (ts == CANARY64).all() and (tok == CANARY64).all()


@pytest.mark.parametrize("device", [False, True])
def test_bad_arguments(engine, a_enc, device):
    data = b"aaaa aaaaa" + EOT + b"aaa"
    n = len(data)
    offs = np.asarray([0, 4, n], np.uint64)
    ws = np.zeros(n, np.uint8)
    for o in (offs, None):
        for bad_ws, bad_mode in ((ws, 5), (None, MASK), (ws, NONE), (ws, GPT4)):
            rc, cnt, out, ts, tok = run(engine, a_enc, data, o, bad_ws, bad_mode, device, True)
            assert rc == _lib.GBPE_E_INVALID and cnt == 0 and untouched(out, ts, tok), (bad_mode, bad_ws is None)
    for bad in (np.asarray([1, 4, n], np.uint64), np.asarray([0, 6, 4, n], np.uint64), np.asarray([0, 4, n - 1], np.uint64)):
        rc, cnt, out, ts, tok = run(engine, a_enc, data, bad, None, GPT4, device, True)
        assert rc == _lib.GBPE_E_INVALID and cnt == 0 and untouched(out, ts, tok), bad.tolist()
    rc, cnt, out, ts, tok = run(engine, a_enc, b"", None, None, GPT4, device, True)
    assert rc == _lib.GBPE_OK and cnt == 0 and untouched(out, ts, tok)
    rc, cnt, out, ts, tok = run(engine, a_enc, b"", np.zeros(4, np.uint64), None, GPT4, device, False)
    assert rc == _lib.GBPE_OK and cnt == 0 and (out == CANARY).all() and (ts == CANARY64).all()
    assert tok[GUARD:GUARD + 4].tolist() == [0] * 4 and guards_stand(tok, 4, CANARY64)


def test_doc_off_and_tok_off_go_together(engine, a_enc):
    lib, ctx = _lib.load(), engine.device
    data = np.frombuffer(b"aaaa aaa", np.uint8)
    offs = np.asarray([0, 4, 8], np.uint64)
    out, ts, tok = np.full(8, CANARY, np.uint32), np.full(8, CANARY64, np.uint64), np.full(3, CANARY64, np.uint64)
    cnt = C.c_uint64(12345)
    u32, u64 = out.ctypes.data_as(_lib.u32p), ts.ctypes.data_as(_lib.u64p)
    for d_off, n_docs, t_off in ((offs.ctypes.data_as(_lib.u64p), 2, None), (None, 0, tok.ctypes.data_as(_lib.u64p)),
                                 (None, 2, None)):
        rc = lib.gbpe_bpe_encode_spans(ctx, a_enc._h, None, vp(data), 8, d_off, n_docs, None, NONE, u32, u64, 8, t_off,
                                       C.byref(cnt))
        assert rc == _lib.GBPE_E_INVALID and cnt.value == 0 and untouched(out, ts, tok)
    # tok_start NULL with room asked for; an input where a relative start could pass 32 bits (rejected unread)
    rc = lib.gbpe_bpe_encode_spans(ctx, a_enc._h, None, vp(data), 8, None, 0, None, NONE, u32, None, 8, None, C.byref(cnt))
    assert rc == _lib.GBPE_E_INVALID and untouched(out, ts, tok)
    rc = lib.gbpe_bpe_encode_spans(ctx, a_enc._h, None, vp(data), (1 << 32) - 4096, None, 0, None, NONE, u32, u64, 8, None,
                                   C.byref(cnt))
    assert rc == _lib.GBPE_E_INVALID and cnt.value == 0 and untouched(out, ts, tok)


def test_device_alignment(engine, a_enc):
    lib, ctx = _lib.load(), engine.device
    data = b"aaaa aaaaa aa"
    tokens, starts = a_want(data)
    dev = DevBuffers(engine)
    try:
        d_in = dev.alloc(len(data) + 1, np.frombuffer(b"a" + data, np.uint8))
        d_out = dev.alloc(256, np.full(64, CANARY, np.uint32))
        d_ts = dev.alloc(512, np.full(64, CANARY64, np.uint64))
        cnt = C.c_uint64(12345)
        for o_out, o_ts in ((0, 4), (2, 0)):   # d_tok_start at 4 mod 8; d_out at 2 mod 4
            rc = lib.gbpe_bpe_encode_spans_device(ctx, a_enc._h, None, C.c_void_p(d_in.value + 1), len(data), None, 0, None,
                                                  NONE, C.c_void_p(d_out.value + o_out), C.c_void_p(d_ts.value + o_ts), 32,
                                                  None, C.byref(cnt))
            assert rc == _lib.GBPE_E_INVALID and cnt.value == 0, (o_out, o_ts)
            assert (dev.fetch(d_out, 64, np.uint32) == CANARY).all() and (dev.fetch(d_ts, 64, np.uint64) == CANARY64).all()
        # d_bytes at an odd address works
        rc = lib.gbpe_bpe_encode_spans_device(ctx, a_enc._h, None, C.c_void_p(d_in.value + 1), len(data), None, 0, None, NONE,
                                              d_out, d_ts, 32, None, C.byref(cnt))
        assert rc == _lib.GBPE_OK and cnt.value == len(tokens)
        assert dev.fetch(d_out, 64, np.uint32)[: len(tokens)].tolist() == tokens
        assert dev.fetch(d_ts, 64, np.uint64)[: len(tokens)].tolist() == starts
        # d_tok_off at 4 mod 8
        d_off = dev.alloc(16, np.asarray([0, len(data)], np.uint64))
        d_tok = dev.alloc(64, np.full(8, CANARY64, np.uint64))
        rc = lib.gbpe_bpe_encode_spans_device(ctx, a_enc._h, None, C.c_void_p(d_in.value + 1), len(data), d_off, 1, None, NONE,
                                              d_out, d_ts, 32, C.c_void_p(d_tok.value + 4), C.byref(cnt))
        assert rc == _lib.GBPE_E_INVALID and (dev.fetch(d_tok, 8, np.uint64) == CANARY64).all()
    finally:
        dev.free()


# ── the Python layer, the timing ───────────────────────────────────────────

def test_python_layer(engine):
    merges, data = model("code", 53), text("code", 53)[:8000]
    voc = list(O.vocab_from_merges(merges).entries)
    plain = MergeEncoder(engine, merges)
    for kw in ({}, {"words": "gpt4"}, {"words": "cl100k"}, {"word_starts": (np.arange(len(data)) % 7 == 0)}):
        tokens, starts = plain.encode_bytes_spans(data, **kw)
        assert starts.dtype == np.uint64 and starts.shape[0] == tokens.shape[0] + 1 and int(starts[-1]) == len(data)
        assert np.array_equal(tokens, plain.encode_bytes(data, **kw))
        slices = [data[int(s):int(e)] for s, e in zip(starts[:-1], starts[1:])]
        assert b"".join(slices) == data
        assert slices == [bytes(voc[t]) for t in tokens.tolist()]
    enc = MergeEncoder(engine, merges, special_tokens={b"EOT": 70000, "<|e|>": 3})
    sdata = b"EOT" + data[:2000] + b"<|e|>EOT" + data[2000:4000] + b"<|e|>"
    docs = [sdata[:700], b"", sdata[700:], b"", b"EOTx"]
    tokens, starts = enc.encode_bytes_spans(sdata, words="gpt4")
    assert np.array_equal(tokens, enc.encode_bytes(sdata, words="gpt4"))
    slices = [sdata[int(s):int(e)] for s, e in zip(starts[:-1], starts[1:])]
    assert b"".join(slices) == sdata
    eot = [s for t, s in zip(tokens.tolist(), slices) if t == 70000]
    assert len(eot) >= 2 and set(eot) == {b"EOT"}
    assert [s for t, s in zip(tokens.tolist(), slices) if t == 3 and len(s) > 1] == [b"<|e|>"] * 2
    t2, s2 = enc.encode_bytes_spans(sdata, words="gpt4", special=False)
    assert np.array_equal(t2, plain.encode_bytes(sdata, words="gpt4")) and 70000 not in t2.tolist()
    tokens, tok_off, starts = enc.encode_batch_spans(docs, words="gpt4")
    want, woff = enc.encode_batch(docs, words="gpt4")
    assert np.array_equal(tokens, want) and np.array_equal(tok_off, woff)
    cat = b"".join(docs)
    assert b"".join(cat[int(s):int(e)] for s, e in zip(starts[:-1], starts[1:])) == cat
    offs = doc_offsets(docs)
    for d, doc in enumerate(docs):
        if doc:
            assert int(starts[int(tok_off[d])]) == int(offs[d])
    t0, s0 = enc.encode_bytes_spans(b"")
    assert t0.shape == (0,) and s0.tolist() == [0]
    t0, o0, s0 = enc.encode_batch_spans([b"", b""])
    assert t0.shape == (0,) and o0.tolist() == [0, 0, 0] and s0.tolist() == [0]
    lib = _lib.load()
    enc.encode_bytes_spans(sdata, words="gpt4")
    a, b, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    assert lib.gbpe_bpe_encode_last_timing(engine.device, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert a.value > 0 and b.value > 0 and c.value > 0
    plain.destroy()
    enc.destroy()
