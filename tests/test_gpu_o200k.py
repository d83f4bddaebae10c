"""The o200k_base word starts on the GPU (gbpe_pretokenize_o200k*, GBPE_WORDS_O200K;
DESIGN §3i) against the backtracking reference of o200k_ref.py: fuzz, every known-answer
family at every in-block offset, the automaton's state and the two backward flags across
blocks in closed form, the device class table, many documents, and the mode through the
eight word-encode entry points and the spans call."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import merge_wide as MW  # noqa: E402
import o200k_corpora as K  # noqa: E402
import o200k_ref as R  # noqa: E402
import pretok_corpora as P  # noqa: E402
import special_ref as S  # noqa: E402
import test_gpu_bpe_spans as TS  # noqa: E402  (run: the spans call with its guards)
import test_gpu_cl100k as TC  # noqa: E402  (encode: the eight entry points; assert_same)
from bpe_words_ref import encode_words_ref, model, text  # noqa: E402
from encode_dev import DevBuffers  # noqa: E402
from gpubpe import BPEEngine, GpuPreTokenizer, MergeEncoder, _lib  # noqa: E402

pytestmark = pytest.mark.gpu

MASK, CL100K, O200K = 1, 4, 6
FILL = 0xAB
CANARY = TC.CANARY
vp = lambda a: a.ctypes.data_as(C.c_void_p)
assert_same = TC.assert_same
encode = TC.encode


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


def gpu_ws(engine, data: bytes) -> np.ndarray:
    """gbpe_pretokenize_o200k on host bytes"""
    ws = np.full(len(data), FILL, np.uint8)
    src = np.frombuffer(data, np.uint8)
    ctx = engine.device
    _lib.check(_lib.load().gbpe_pretokenize_o200k(ctx, vp(src) if data else None, len(data), vp(ws) if data else None),
               ctx, "pretokenize")
    return ws


def gpu_ws_device(engine, data: bytes, a: int = 0, b: int = 0) -> np.ndarray:
    """gbpe_pretokenize_o200k_device with the input `a` and the output `b` bytes into their
    allocations, bytes that would change the answer in front of and behind the input, and a
    check that nothing outside d_ws[0, n) is written"""
    n = len(data)
    dev = DevBuffers(engine)
    try:
        host = np.frombuffer(b"'" * a + data + b"'ll\n/a 12345678 \n\n\x80\x80\x80\x80", np.uint8)
        d_in = dev.alloc(host.shape[0], host)
        d_out = dev.alloc(b + n + 32, np.full(b + n + 32, FILL, np.uint8))
        _lib.check(dev.lib.gbpe_pretokenize_o200k_device(engine.device, C.c_void_p(d_in.value + a), n,
                                                         C.c_void_p(d_out.value + b)), engine.device, "pretokenize (device)")
        _lib.check(dev.lib.gbpe_synchronize(engine.device), engine.device, "synchronize")
        out = dev.fetch(d_out, b + n + 32, np.uint8)
        assert np.all(out[:b] == FILL) and np.all(out[b + n:] == FILL), f"wrote outside [b, b + n): a {a}, b {b}, n {n}"
        return out[b:b + n]
    finally:
        dev.free()


# ─────────────────────────────── one text ────────────────────────────────────

@pytest.mark.parametrize("seed", K.FUZZ_SEEDS)
def test_fuzz(engine, seed):
    data = K.fuzz(K.FUZZ_CODEPOINTS, seed)
    for cut in K.FUZZ_CUTS:            # the cut lands inside a codepoint for some seeds
        piece = data[:len(data) - cut]
        exp = R.mask(piece)
        assert_same(gpu_ws(engine, piece), exp, piece, f"fuzz seed {seed} cut {cut}")
        a, b = (seed + cut) % 4, (1, 15, 16, 0)[cut]        # unaligned staging, scalar stores
        assert_same(gpu_ws_device(engine, piece, a, b), exp, piece, f"fuzz seed {seed} cut {cut}, device + {a} / + {b}")


def test_short_and_empty(engine):
    lib, ctx = _lib.load(), engine.device
    assert lib.gbpe_pretokenize_o200k(ctx, None, 0, None) == _lib.GBPE_OK
    assert lib.gbpe_pretokenize_o200k_device(ctx, None, 0, None) == _lib.GBPE_OK
    buf = np.zeros(4, np.uint8)
    assert lib.gbpe_pretokenize_o200k(ctx, None, 4, vp(buf)) == _lib.GBPE_E_INVALID
    assert lib.gbpe_pretokenize_o200k(ctx, vp(buf), 4, None) == _lib.GBPE_E_INVALID
    assert lib.gbpe_pretokenize_o200k_device(ctx, None, 4, vp(buf)) == _lib.GBPE_E_INVALID
    for seed in (317, 318):
        data = K.fuzz(600, seed)
        for n in (1, 2, 3, 15, 16, 17, 31, 33):
            assert_same(gpu_ws(engine, data[:n]), R.mask(data[:n]), data[:n], f"n {n}")
            assert_same(gpu_ws_device(engine, data[:n], 1, 1), R.mask(data[:n]), data[:n], f"device n {n}")


@pytest.mark.parametrize("name,pat,period", K.PROBES, ids=[p[0] for p in K.PROBES])
def test_periodic_probe(engine, name, pat, period):
    data = K.periodic(pat, period)
    assert_same(gpu_ws(engine, data), R.mask(data), data, f"probe {name}, period {period}")


def test_known_answers(engine):
    for s, want in K.KNOWN:
        data = s.encode()
        cuts = np.flatnonzero(gpu_ws(engine, data)).tolist() + [len(data)]
        assert [data[a:b].decode() for a, b in zip(cuts[:-1], cuts[1:])] == want.split("|"), s


# ──────────────────────── the states across blocks ──────────────────────────

@pytest.mark.parametrize("k", K.RUN_LENGTHS)
def test_closed_forms(engine, k):
    for name, data, exp in K.closed_forms(k):
        assert_same(gpu_ws(engine, data), exp, data, f"{name}, {k} codepoints")


def test_scan_chains():
    """More than 1024 blocks, so every k_pto_scan2 thread chains two aggregates in each
    direction; a fresh context, so the aggregate block grows between the calls."""
    small = K.fuzz(5_500, 319)
    exp_small = R.mask(small)
    eng = BPEEngine().init()
    try:
        assert_same(gpu_ws(eng, small), exp_small, small, "small input before")
        for name, data, exp in K.chain_forms():
            assert len(data) > 1024 * P.BLK, name
            assert_same(gpu_ws(eng, data), exp, data, name)
        assert_same(gpu_ws(eng, small), exp_small, small, "small input after")
    finally:
        eng.close()


# ───────────────────────────── many documents ───────────────────────────────

def gpu_ws_batch(engine, data: bytes, offs, device=False):
    n, n_docs = len(data), len(offs) - 1
    offs = np.ascontiguousarray(offs, np.uint64)
    src = np.frombuffer(data, np.uint8)
    lib, ctx = _lib.load(), engine.device
    if not device:
        ws = np.full(n, FILL, np.uint8)
        rc = lib.gbpe_pretokenize_o200k_batch(ctx, vp(src), n, offs.ctypes.data_as(_lib.u64p), n_docs, vp(ws))
        return rc, ws
    dev = DevBuffers(engine)
    try:
        d_in, d_off = dev.alloc(n + 8, np.concatenate([src, np.full(8, 0x80, np.uint8)])), dev.alloc(offs.nbytes, offs)
        d_out = dev.alloc(n + 32, np.full(n + 32, FILL, np.uint8))
        rc = lib.gbpe_pretokenize_o200k_batch_device(ctx, d_in, n, d_off, n_docs, d_out)
        out = dev.fetch(d_out, n + 32, np.uint8)
        assert np.all(out[n:] == FILL)
        return rc, out[:n]
    finally:
        dev.free()


SWEEP = [(lo, min(lo + 0x20000, 0x110000)) for lo in range(0, 0x110000, 0x20000)]
_sweep_answers = {}


@pytest.mark.parametrize("lo,hi", SWEEP, ids=[f"{lo:06x}" for lo, _ in SWEEP])
def test_class_sweep(engine, lo, hi):
    """`a` c `b` for every codepoint c, each a document of its own: the device class table"""
    data, offs = K.sweep_documents(lo, hi)
    exp = np.zeros(len(data), np.uint8)
    at = offs[:-1].astype(np.int64)
    last = offs[1:].astype(np.int64) - 1

    def answer(cp):      # the answer depends on c through its class and the codepoints the pattern names
        key = cp if cp < 0x180 or cp == 0x212A else -1 - R.klass(cp)
        if key not in _sweep_answers:
            _sweep_answers[key] = R.starts([0x61, cp, 0x62])
        return _sweep_answers[key]
    s = np.asarray([answer(cp) for cp in range(lo, hi)], np.uint8)
    exp[at], exp[at + 1], exp[last] = s[:, 0], s[:, 1], s[:, 2]
    rc, got = gpu_ws_batch(engine, data, offs)
    assert rc == _lib.GBPE_OK
    assert_same(got, exp, data, f"codepoints {lo:#x}..{hi:#x}")


def test_beyond_unicode(engine):
    tail = P.sweep_astral()[5 * (0x110000 - 0x10000):]        # 4-byte sequences that decode to 0x110000 and above
    assert len(tail) % 5 == 0 and tail[:2] == b"a\xf4"
    assert_same(gpu_ws(engine, tail), R.mask(tail), tail, "beyond Unicode")


def test_batch(engine):
    data, offs = K.batch_documents()
    exp = R.mask_docs(data, [int(o) for o in offs])
    for device in (False, True):
        rc, got = gpu_ws_batch(engine, data, offs, device)
        assert rc == _lib.GBPE_OK
        assert_same(got, exp, data, f"batch, device {device}")
    for a, b in zip(offs[:-1], offs[1:]):                      # each document: the single call on it alone
        doc = data[int(a):int(b)]
        assert_same(gpu_ws(engine, doc), exp[int(a):int(b)], doc, f"document at {a}")


def test_batch_of_fuzz(engine):
    """documents cut at random codepoint boundaries of a fuzz text: every state resets at every block offset"""
    data = K.fuzz(20_000, 320)
    leads = P.lead_offsets(data)[0]
    rng = np.random.default_rng(321)
    cuts = np.unique(leads[rng.integers(1, len(leads), size=600)])
    offs = np.concatenate([[0], cuts, cuts[::50], [len(data)]]).astype(np.uint64)
    offs.sort()                                                # (the repeated cuts: empty documents)
    exp = R.mask_docs(data, [int(o) for o in offs])
    for device in (False, True):
        rc, got = gpu_ws_batch(engine, data, offs, device)
        assert rc == _lib.GBPE_OK
        assert_same(got, exp, data, f"fuzz batch, device {device}")


def test_batch_bad_offsets(engine):
    data = K.BATCH_TEXT
    n = len(data)
    for bad in ([1, 4, n], [0, 6, 4, n], [0, 4, n - 1], [0, 4, n + 5]):
        for device in (False, True):
            rc, got = gpu_ws_batch(engine, data, np.asarray(bad, np.uint64), device)
            assert rc == _lib.GBPE_E_INVALID and np.all(got == FILL), (bad, device)
    lib, ctx = _lib.load(), engine.device
    ws = np.full(n, FILL, np.uint8)
    src = np.frombuffer(data, np.uint8)
    good = np.asarray([0, 4, n], np.uint64)
    for args in ((None, n, good.ctypes.data_as(_lib.u64p), 2, vp(ws)), (vp(src), n, None, 2, vp(ws)),
                 (vp(src), n, good.ctypes.data_as(_lib.u64p), 2, None)):
        assert lib.gbpe_pretokenize_o200k_batch(ctx, *args) == _lib.GBPE_E_INVALID and np.all(ws == FILL)
    assert lib.gbpe_pretokenize_o200k_batch(ctx, None, 0, None, 0, None) == _lib.GBPE_OK
    assert lib.gbpe_pretokenize_o200k_batch_device(ctx, None, 0, None, 0, None) == _lib.GBPE_OK


def test_python_pretokenizer(engine):
    pt = GpuPreTokenizer(engine)
    s = "camelCase HTTPServer's  x\n/\n 1234567 a's's"
    got = pt.pre_tokenize(s, rules="o200k_base")
    assert got["bytes"] == s.encode() and np.array_equal(got["wordStarts"], R.mask(s.encode()))
    assert not np.array_equal(pt.pre_tokenize(s, rules="cl100k")["wordStarts"], got["wordStarts"])
    assert np.array_equal(pt.pre_tokenize(s)["wordStarts"], pt.pre_tokenize_bytes(s.encode(), rules="gpt4")["wordStarts"])
    docs = [b"it'sX", b"", b"'s's 12345"]
    ws, offs = pt.pre_tokenize_batch(docs, rules="o200k_base")
    assert offs.tolist() == [0, 5, 5, 15] and np.array_equal(ws, np.concatenate([R.mask(d) for d in docs]))
    with pytest.raises(ValueError):
        pt.pre_tokenize(s, rules="o200k")


# ───────────────────────────────── encode ────────────────────────────────────

SPECIALS = dict(zip(S.TABLE[:2], S.IDS[:2]))        # <|endoftext|> and EOT


@pytest.fixture(scope="module")
def corpus():
    """documents of fuzz and code, every third ending in a special and a contraction after it"""
    body = K.fuzz(2_500, 322) + text("code", 53)[:4_000] + K.fuzz(1_500, 323)
    leads = P.lead_offsets(body)[0]
    rng = np.random.default_rng(324)
    cuts = [0] + np.unique(leads[rng.integers(1, len(leads), size=40)]).tolist() + [len(body)]
    docs = []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        docs.append(body[a:b] + (S.TABLE[i % 2] + b"'s 12\n" if i % 3 == 0 else b""))
    docs.insert(5, b"")
    return docs


def piece_mask(docs, specials):
    out = []
    for doc in docs:
        m = np.zeros(len(doc), np.uint8)
        for a, b, k in S.pieces(doc, specials):
            if k is None:
                m[a:b] = R.mask(doc[a:b])
        out.append(m)
    return np.concatenate(out)


@pytest.fixture(scope="module")
def masks(corpus):
    """the reference's masks of the corpus, keyed (batch, special); computed once"""
    data = b"".join(corpus)
    offs = S.doc_offsets(corpus)
    return {(False, False): R.mask(data), (True, False): R.mask_docs(data, [int(o) for o in offs]),
            (False, True): piece_mask([data], S.TABLE[:2]), (True, True): piece_mask(corpus, S.TABLE[:2])}


@pytest.fixture(scope="module")
def encoders(engine):
    narrow = model("code", 53)
    encs = {"narrow": MergeEncoder(engine, narrow, special_tokens=SPECIALS),
            "wide": MergeEncoder(engine, MW.relabel(narrow), special_tokens=SPECIALS)}
    yield encs
    for e in encs.values():
        e.destroy()


@pytest.mark.parametrize("cs", [256, 1024, 4096])
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_encode(engine, encoders, corpus, masks, monkeypatch, width, cs):
    """GBPE_WORDS_O200K gives GBPE_WORDS_MASK's tokens under the reference's mask, bit for bit, through
    all eight entry points and the spans call; the plain host form also against the per-word oracle."""
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    enc = encoders[width]
    data = b"".join(corpus)
    offs = S.doc_offsets(corpus)
    want = encode_words_ref(data, model("code", 53), masks[False, False])
    want = MW.relabel_tokens(want) if width == "wide" else want
    for batch in (False, True):
        for special in (False, True):
            o = offs if batch else None
            for device in (False, True):
                rc, n, out, tok = encode(engine, enc, data, o, None, O200K, special, device)
                rc2, n2, out2, tok2 = encode(engine, enc, data, o, masks[batch, special], MASK, special, device)
                what = (width, cs, batch, special, device)
                assert rc == _lib.GBPE_OK and rc2 == _lib.GBPE_OK and n == n2 and 0 < n <= len(data), (what, rc, rc2, n, n2)
                assert np.array_equal(out[:n], out2[:n]) and (out[n:] == CANARY).all(), what
                if batch:
                    assert np.array_equal(tok, tok2) and int(tok[-1]) == n, what
                if not batch and not special:
                    assert out[:n].tolist() == want, what
                if special and width == "narrow":              # (a wide id may lie above the specials' ids)
                    assert np.count_nonzero(out[:n] >= 50000) == sum(d.endswith(b"'s 12\n") for d in corpus), what
                # the spans call of the same shape: the same tokens, and the starts of the mask call's
                G = TS.GUARD
                rc3, n3, out3, ts3, tok3 = TS.run(engine, enc, data, o, None, O200K, device, special)
                rc4, n4, out4, ts4, tok4 = TS.run(engine, enc, data, o, masks[batch, special], MASK, device, special)
                assert rc3 == _lib.GBPE_OK and rc4 == _lib.GBPE_OK and n3 == n and n4 == n, (what, rc3, rc4, n3, n4)
                assert np.array_equal(out3[G:G + n], out[:n]) and np.array_equal(ts3, ts4) and np.array_equal(tok3, tok4), what


def test_modes_differ(engine):
    """a text on which the o200k and the cl100k rules must give other tokens: `aB` is one word under
    cl100k and two under o200k, so the merge (a, B) fires in one only; `x's` the other way round;
    and the Python spellings of the mode"""
    enc = MergeEncoder(engine, [[ord("a"), ord("B"), 256], [ord("x"), ord("'"), 257]])
    try:
        assert enc.encode_bytes(b"aB x's", words="cl100k").tolist() == [256, 32, 120, 39, 115]
        assert enc.encode_bytes(b"aB x's", words="o200k_base").tolist() == [97, 66, 32, 257, 115]
        toks, off = enc.encode_batch([b"aB", b"x'"], words="o200k_base")
        assert toks.tolist() == [97, 66, 120, 39] and off.tolist() == [0, 2, 4]
        assert enc.encode("x's", words="o200k_base")["tokens"] == [257, 115]
        toks, starts = enc.encode_bytes_spans(b"aB x's", words="o200k_base")
        assert toks.tolist() == [97, 66, 32, 257, 115] and starts.tolist() == [0, 1, 2, 3, 5, 6]
        with pytest.raises(_lib.GpuBpeError):
            enc.encode_bytes(b"aB", words="o200k")
    finally:
        enc.destroy()


def test_status(engine, encoders):
    """mode 6 with no mask is valid; with a mask, and mode 7, GBPE_E_INVALID with nothing written"""
    enc = encoders["narrow"]
    data = b"it's camelCase 12345\n"
    ws = np.ones(len(data), np.uint8)
    offs = np.asarray([0, 4, len(data)], np.uint64)
    for batch in (False, True):
        for special in (False, True):
            for device in (False, True):
                o = offs if batch else None
                rc, n, out, _ = encode(engine, enc, data, o, None, O200K, special, device)
                assert rc == _lib.GBPE_OK and n > 0, (batch, special, device)
                for bad_ws, bad_mode in ((ws, O200K), (None, 7), (ws, 7)):
                    rc, n, out, _ = encode(engine, enc, data, o, bad_ws, bad_mode, special, device)
                    assert rc == _lib.GBPE_E_INVALID and n == 0 and (out == CANARY).all(), (batch, special, device, bad_mode)
                rc, n, out, _ = encode(engine, enc, data, o, None, O200K, special, device, cap=2)
                assert rc == _lib.GBPE_E_CAPACITY and n > 2 and (out[2:] == CANARY).all()
    for device in (False, True):
        for bad_ws, bad_mode in ((ws, O200K), (None, 7)):
            rc, n, out, ts, _ = TS.run(engine, enc, data, None, bad_ws, bad_mode, device, False)
            assert rc == _lib.GBPE_E_INVALID and n == 0 and (out == TS.CANARY).all(), (device, bad_mode)
    a, b, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    rc, n, _, _ = encode(engine, enc, data, None, None, O200K, False, False)
    assert _lib.load().gbpe_bpe_encode_last_timing(engine.device, C.byref(a), C.byref(b), C.byref(c)) == _lib.GBPE_OK
    assert a.value > 0 and b.value > 0 and c.value > 0          # the word-start kernels count under ms_starts
