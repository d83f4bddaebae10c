"""The cl100k_base word starts on the GPU (gbpe_pretokenize_cl100k*, GBPE_WORDS_CL100K;
DESIGN §3g) against the sequential reference of cl100k_ref.py: fuzz, every rule at
every in-block offset, the three scans across blocks in closed form, the device class
table, many documents, and the mode through all eight word-encode entry points."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import cl100k_corpora as K  # noqa: E402
import cl100k_ref as R  # noqa: E402
import merge_wide as MW  # noqa: E402
import pretok_corpora as P  # noqa: E402
import special_ref as S  # noqa: E402
from bpe_words_ref import encode_words_ref, model, text  # noqa: E402
from encode_dev import DevBuffers  # noqa: E402
from gpubpe import BPEEngine, GpuPreTokenizer, MergeEncoder, _lib  # noqa: E402

pytestmark = pytest.mark.gpu

NONE, MASK, HEUR, GPT4, CL100K = range(5)
FILL = 0xAB
CANARY = 0xA5A5A5A5
GUARD = 8
vp = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


def gpu_ws(engine, data: bytes) -> np.ndarray:
    """gbpe_pretokenize_cl100k on host bytes"""
    ws = np.full(len(data), FILL, np.uint8)
    src = np.frombuffer(data, np.uint8)
    ctx = engine.device
    _lib.check(_lib.load().gbpe_pretokenize_cl100k(ctx, vp(src) if data else None, len(data), vp(ws) if data else None),
               ctx, "pretokenize")
    return ws


def gpu_ws_device(engine, data: bytes, a: int = 0, b: int = 0) -> np.ndarray:
    """gbpe_pretokenize_cl100k_device with the input `a` and the output `b` bytes into their
    allocations, bytes that would change the answer in front of and behind the input, and a
    check that nothing outside d_ws[0, n) is written"""
    n = len(data)
    dev = DevBuffers(engine)
    try:
        host = np.frombuffer(b"'" * a + data + b"\n'll 12345678 \n\n\x80\x80\x80\x80", np.uint8)
        d_in = dev.alloc(host.shape[0], host)
        d_out = dev.alloc(b + n + 32, np.full(b + n + 32, FILL, np.uint8))
        _lib.check(dev.lib.gbpe_pretokenize_cl100k_device(engine.device, C.c_void_p(d_in.value + a), n,
                                                          C.c_void_p(d_out.value + b)), engine.device, "pretokenize (device)")
        _lib.check(dev.lib.gbpe_synchronize(engine.device), engine.device, "synchronize")
        out = dev.fetch(d_out, b + n + 32, np.uint8)
        assert np.all(out[:b] == FILL) and np.all(out[b + n:] == FILL), f"wrote outside [b, b + n): a {a}, b {b}, n {n}"
        return out[b:b + n]
    finally:
        dev.free()


def assert_same(got, exp, data, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (f"{what}: {bad.size} mismatches, first (offset, offset % 4096, offset % 16, got, expected, "
                           f"bytes around) "
                           f"{[(int(i), int(i) % 4096, int(i) % 16, int(got[i]), int(exp[i]), data[max(0, i - 16):i + 16]) for i in bad[:5]]}")


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
    assert lib.gbpe_pretokenize_cl100k(ctx, None, 0, None) == _lib.GBPE_OK
    assert lib.gbpe_pretokenize_cl100k_device(ctx, None, 0, None) == _lib.GBPE_OK
    buf = np.zeros(4, np.uint8)
    assert lib.gbpe_pretokenize_cl100k(ctx, None, 4, vp(buf)) == _lib.GBPE_E_INVALID
    assert lib.gbpe_pretokenize_cl100k(ctx, vp(buf), 4, None) == _lib.GBPE_E_INVALID
    data = K.fuzz(600, 217)
    for n in (1, 2, 3, 15, 16, 17, 31, 33):
        assert_same(gpu_ws(engine, data[:n]), R.mask(data[:n]), data[:n], f"n {n}")
        assert_same(gpu_ws_device(engine, data[:n], 1, 1), R.mask(data[:n]), data[:n], f"device n {n}")


@pytest.mark.parametrize("name,pat,period", K.PROBES, ids=[p[0] for p in K.PROBES])
def test_periodic_probe(engine, name, pat, period):
    data = K.periodic(pat, period)
    assert_same(gpu_ws(engine, data), R.mask(data), data, f"probe {name}, period {period}")


# ──────────────────────── the scans across blocks ───────────────────────────

@pytest.mark.parametrize("k", K.RUN_LENGTHS)
def test_blank_run(engine, k):
    for j in (None, 0, k // 2, k - 1):
        data, exp = K.blank_run(k, j)
        assert_same(gpu_ws(engine, data), exp, data, f"{k} blanks, newline at {j}")


def test_eaten_run(engine):
    data, exp = K.eaten_run(2 * P.BLK + 3)
    assert_same(gpu_ws(engine, data), exp, data, "a full stop and its newlines")


def test_scan_chains():
    """More than 1024 blocks, so every k_ptc_scan2 thread chains two aggregates in each
    direction; a fresh context, so the aggregate block grows between the calls."""
    small = K.fuzz(5_500, 218)
    exp_small = R.mask(small)
    eng = BPEEngine().init()
    try:
        assert_same(gpu_ws(eng, small), exp_small, small, "small input before")
        for what, (data, exp) in (("digits", K.digit_run(K.CHAIN_N)), ("blanks", K.blanks_then_newline(K.CHAIN_N))):
            assert_same(gpu_ws(eng, data), exp, data, what)
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
        rc = lib.gbpe_pretokenize_cl100k_batch(ctx, vp(src), n, offs.ctypes.data_as(_lib.u64p), n_docs, vp(ws))
        return rc, ws
    dev = DevBuffers(engine)
    try:
        d_in, d_off = dev.alloc(n + 8, np.concatenate([src, np.full(8, 0x80, np.uint8)])), dev.alloc(offs.nbytes, offs)
        d_out = dev.alloc(n + 32, np.full(n + 32, FILL, np.uint8))
        rc = lib.gbpe_pretokenize_cl100k_batch_device(ctx, d_in, n, d_off, n_docs, d_out)
        out = dev.fetch(d_out, n + 32, np.uint8)
        assert np.all(out[n:] == FILL)
        return rc, out[:n]
    finally:
        dev.free()


SWEEP = [(lo, min(lo + 0x20000, 0x110000)) for lo in range(0, 0x110000, 0x20000)]


@pytest.mark.parametrize("lo,hi", SWEEP, ids=[f"{lo:06x}" for lo, _ in SWEEP])
def test_class_sweep(engine, lo, hi):
    """`a` c `b` for every codepoint c, each a document of its own: the device class table"""
    data, offs = K.sweep_documents(lo, hi)
    exp = np.zeros(len(data), np.uint8)
    at = offs[:-1].astype(np.int64)
    last = offs[1:].astype(np.int64) - 1
    s = np.asarray([R.starts([0x61, cp, 0x62]) for cp in range(lo, hi)], np.uint8)
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
    """documents cut at random codepoint boundaries of a fuzz text: every scan resets at every block offset"""
    data = K.fuzz(20_000, 219)
    leads = P.lead_offsets(data)[0]
    rng = np.random.default_rng(220)
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
    assert lib.gbpe_pretokenize_cl100k_batch(ctx, None, 0, None, 0, None) == _lib.GBPE_OK
    assert lib.gbpe_pretokenize_cl100k_batch_device(ctx, None, 0, None, 0, None) == _lib.GBPE_OK


def test_python_pretokenizer(engine):
    pt = GpuPreTokenizer(engine)
    s = "don't  stop\n\n  x 'tis 1234567 a.b a..b"
    got = pt.pre_tokenize(s, rules="cl100k")
    assert got["bytes"] == s.encode() and np.array_equal(got["wordStarts"], R.mask(s.encode()))
    assert not np.array_equal(pt.pre_tokenize(s)["wordStarts"], got["wordStarts"])      # the default stays the GPT-4 rules
    assert np.array_equal(pt.pre_tokenize(s)["wordStarts"], pt.pre_tokenize_bytes(s.encode(), rules="gpt4")["wordStarts"])
    docs = [b"it's", b"", b"'s 12345"]
    ws, offs = pt.pre_tokenize_batch(docs, rules="cl100k")
    assert offs.tolist() == [0, 4, 4, 12] and np.array_equal(ws, np.concatenate([R.mask(d) for d in docs]))


# ───────────────────────────────── encode ────────────────────────────────────

SPECIALS = dict(zip(S.TABLE[:2], S.IDS[:2]))        # <|endoftext|> and EOT


@pytest.fixture(scope="module")
def corpus():
    """(documents, the reference's mask of each piece between the specials, laid end to end)"""
    body = K.fuzz(2_500, 221) + text("code", 53)[:4_000] + K.fuzz(1_500, 222)
    leads = P.lead_offsets(body)[0]
    rng = np.random.default_rng(223)
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


def encode(engine, enc, data, offs, ws, mode, special, device, cap=None):
    """One of the eight entry points: (status, n_out, out[cap + GUARD], tok_off or None)."""
    lib, ctx = _lib.load(), engine.device
    n = len(data)
    cap = n if cap is None else cap
    n_docs = 0 if offs is None else len(offs) - 1
    name = "gbpe_bpe_encode_" + ("special" if special else "words") + ("_batch" if offs is not None else "") + \
        ("_device" if device else "")
    head = [ctx, enc._h] + ([enc._sp] if special else [])
    cnt = C.c_uint64(12345)
    src = np.frombuffer(data, np.uint8)
    if not device:
        out = np.full(cap + GUARD, CANARY, np.uint32)
        tok = np.zeros(n_docs + 1, np.uint64)
        args = head + [vp(src) if n else None, n]
        if offs is not None:
            args += [offs.ctypes.data_as(_lib.u64p), n_docs]
        args += [None if ws is None else vp(ws), mode, out.ctypes.data_as(_lib.u32p), cap]
        if offs is not None:
            args += [tok.ctypes.data_as(_lib.u64p)]
        rc = getattr(lib, name)(*args, C.byref(cnt))
        return rc, int(cnt.value), out, tok if offs is not None else None
    dev = DevBuffers(engine)
    try:
        d_in = dev.alloc(n + 8, np.concatenate([src, np.frombuffer(b"'ll 1234", np.uint8)]))
        d_ws = None if ws is None else dev.alloc(n + 1, np.concatenate([ws, np.zeros(1, np.uint8)]))
        d_out = dev.alloc(4 * (cap + GUARD), np.full(cap + GUARD, CANARY, np.uint32))
        d_tok = dev.alloc(8 * (n_docs + 1), np.zeros(n_docs + 1, np.uint64))
        args = head + [d_in, n]
        if offs is not None:
            args += [dev.alloc(offs.nbytes, offs), n_docs]
        args += [d_ws, mode, d_out, cap]
        if offs is not None:
            args += [d_tok]
        rc = getattr(lib, name)(*args, C.byref(cnt))
        return (rc, int(cnt.value), dev.fetch(d_out, cap + GUARD, np.uint32),
                dev.fetch(d_tok, n_docs + 1, np.uint64) if offs is not None else None)
    finally:
        dev.free()


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
def test_encode(engine, encoders, corpus, monkeypatch, width, cs):
    """GBPE_WORDS_CL100K gives GBPE_WORDS_MASK's tokens under the reference's mask, through all
    eight entry points; the plain host form also against the per-word oracle."""
    monkeypatch.setenv("GBPE_DEBUG", f"me_cs={cs}")
    enc = encoders[width]
    data = b"".join(corpus)
    offs = S.doc_offsets(corpus)
    whole = R.mask(data)
    per_doc = R.mask_docs(data, [int(o) for o in offs])
    masks = {(False, False): whole, (True, False): per_doc,
             (False, True): piece_mask([data], S.TABLE[:2]), (True, True): piece_mask(corpus, S.TABLE[:2])}
    want = encode_words_ref(data, model("code", 53), whole)
    want = MW.relabel_tokens(want) if width == "wide" else want
    for batch in (False, True):
        for special in (False, True):
            for device in (False, True):
                o = offs if batch else None
                rc, n, out, tok = encode(engine, enc, data, o, None, CL100K, special, device)
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


def test_modes_differ(engine):
    """a text on which the cl100k and the GPT-4 rules must give other tokens: `.b` is one word
    under the first, `.` and `b` are two under the second, so the merge (., b) fires in one only;
    and the Python spellings of the mode"""
    enc = MergeEncoder(engine, [[ord("."), ord("b"), 256]])
    try:
        assert enc.encode_bytes(b"a.b", words="cl100k").tolist() == [97, 256]
        assert enc.encode_bytes(b"a.b", words="gpt4").tolist() == [97, 46, 98]
        toks, off = enc.encode_batch([b"a.b", b".b"], words="cl100k")
        assert toks.tolist() == [97, 256, 256] and off.tolist() == [0, 2, 3]
        assert enc.encode("a.b", words="cl100k")["tokens"] == [97, 256]
    finally:
        enc.destroy()


def test_status(engine, encoders):
    """mode 4 with no mask is valid; with a mask, and every mode above 4, GBPE_E_INVALID with nothing written"""
    enc = encoders["narrow"]
    data = b"it's 12345\n"
    ws = np.ones(len(data), np.uint8)
    offs = np.asarray([0, 4, len(data)], np.uint64)
    for batch in (False, True):
        for special in (False, True):
            for device in (False, True):
                o = offs if batch else None
                rc, n, out, _ = encode(engine, enc, data, o, None, CL100K, special, device)
                assert rc == _lib.GBPE_OK and n > 0, (batch, special, device)
                for bad_ws, bad_mode in ((ws, CL100K), (None, 5), (ws, 5), (None, 0xFFFFFFFF)):
                    rc, n, out, _ = encode(engine, enc, data, o, bad_ws, bad_mode, special, device)
                    assert rc == _lib.GBPE_E_INVALID and n == 0 and (out == CANARY).all(), (batch, special, device, bad_mode)
                rc, n, out, _ = encode(engine, enc, data, o, None, CL100K, special, device, cap=2)     # the size query's kin
                assert rc == _lib.GBPE_E_CAPACITY and n > 2 and (out[2:] == CANARY).all()
    a, b, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    rc, n, _, _ = encode(engine, enc, data, None, None, CL100K, False, False)
    assert _lib.load().gbpe_bpe_encode_last_timing(engine.device, C.byref(a), C.byref(b), C.byref(c)) == _lib.GBPE_OK
    assert a.value > 0 and b.value > 0 and c.value > 0          # the word-start kernels count under ms_starts
