"""Device decode (gbpe_decode / gbpe_decode_device / gbpe_decode_batch /
gbpe_decode_batch_device / TrieTokenizer.decode_bytes, decode_batch) against the
oracle's decode.

The expected bytes come from decode_ref.decode_np, which tests/test_decode_host.py
pins to O.decode on these very streams.  Exact comparisons; every case runs through
the host form and the device form, each under both scatter kernels (the 16-byte
vector one and, with GBPE_DEBUG dec_plain=1, the per-token one).
"""
import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
import decode_ref as R
from decode_dev import DecodeDev, POISON, device_decode, host_decode, upload_vocab
from encode_dev import BatchDev

pytestmark = pytest.mark.gpu

OK, E_INVALID, E_CAPACITY = 0, -1, -4
PATHS = [("vector", None), ("plain", "dec_plain=1")]


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


def _uploaded(eng, vocab):
    from gpubpe import _lib
    rc, dv = upload_vocab(eng, vocab)
    _lib.check(rc, eng.device, "vocab upload")
    return dv


@pytest.fixture(scope="module")
def dva(eng):
    from gpubpe import _lib
    dv = _uploaded(eng, R.vocab_a())
    yield dv
    _lib.load().gbpe_vocab_free(dv)


@pytest.fixture(scope="module")
def dvb(eng):
    from gpubpe import _lib
    dv = _uploaded(eng, R.vocab_b())
    yield dv
    _lib.load().gbpe_vocab_free(dv)


def _set_path(monkeypatch, knob, extra=None):
    knobs = ",".join(k for k in (knob, extra) if k)
    if knobs:
        monkeypatch.setenv("GBPE_DEBUG", knobs)
    else:
        monkeypatch.delenv("GBPE_DEBUG", raising=False)


def _check_stream(eng, dv, vocab, tokens, monkeypatch, want=None):
    """Both forms, both scatter paths, out_cap exactly the total: the oracle's bytes
    and an untouched guard behind them."""
    want = R.decode_np(tokens, vocab) if want is None else want
    total = int(want.shape[0])
    for name, knob in PATHS:
        _set_path(monkeypatch, knob)
        for form in (host_decode, device_decode):
            rc, n_out, out, guard, _ = form(eng, dv, tokens, total)
            assert (rc, n_out) == (OK, total), (name, form.__name__)
            assert np.array_equal(out, want), (name, form.__name__)
            assert np.all(guard == 0xA5), (name, form.__name__)
    return want


def _check_batch(eng, dv, vocab, docs, monkeypatch):
    from gpubpe import flatten_token_documents
    toks, tok_off = flatten_token_documents(docs)
    parts = [O.decode(d, vocab) for d in docs]
    want_off = np.zeros(len(docs) + 1, dtype=np.uint64)
    want_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    want = np.frombuffer(b"".join(parts), dtype=np.uint8)
    total = int(want.shape[0])
    for name, knob in PATHS:
        _set_path(monkeypatch, knob)
        for form in (host_decode, device_decode):
            rc, n_out, out, guard, off = form(eng, dv, toks, total, tok_off)
            assert (rc, n_out) == (OK, total), (name, form.__name__)
            assert np.array_equal(off, want_off), (name, form.__name__)
            assert np.array_equal(out, want) and np.all(guard == 0xA5), (name, form.__name__)
            for d in (0, len(docs) // 2, len(docs) - 1):   # each document's bytes are its own decode
                assert out[int(off[d]):int(off[d + 1])].tobytes() == parts[d]
    return toks, tok_off, want, want_off


# ── single streams ──────────────────────────────────────────────────────────
@pytest.mark.parametrize("n", R.COUNTS)
def test_random_streams_at_block_and_wave_edges(eng, dva, n, monkeypatch):
    _check_stream(eng, dva, R.vocab_a(), R.random_stream(n, 100 + n), monkeypatch)


@pytest.mark.parametrize("n", R.COUNTS)
def test_leading_empty_token(eng, dva, n, monkeypatch):
    t = R.leading_empty(n, 200 + n)
    assert t[0] == R.A_EMPTY
    _check_stream(eng, dva, R.vocab_a(), t, monkeypatch)


@pytest.mark.parametrize("n", R.COUNTS)
def test_long_token_across_the_workgroup_boundary(eng, dva, n, monkeypatch):
    _check_stream(eng, dva, R.vocab_a(), R.boundary_long(n, 300 + n), monkeypatch)


@pytest.mark.parametrize("total", [15, 16, 17, 31, 32, 33])
def test_output_alignment_edges(eng, dva, total, monkeypatch):
    want = _check_stream(eng, dva, R.vocab_a(), R.stream_of_total(total), monkeypatch)
    assert want.shape[0] == total


def test_only_empty_tokens(eng, dva, monkeypatch):
    want = _check_stream(eng, dva, R.vocab_a(), R.small_streams()["only-empty"], monkeypatch)
    assert want.shape[0] == 0


def test_no_tokens(eng, dva):
    for form in (host_decode, device_decode):
        rc, n_out, _, guard, _ = form(eng, dva, np.zeros(0, np.uint32), 8)
        assert (rc, n_out) == (OK, 0) and np.all(guard == 0xA5)


@pytest.mark.parametrize("n", R.COUNTS)
def test_unknown_ids_mixed_in(eng, dva, n, monkeypatch):
    t = R.with_unknown(n, 400 + n)
    assert t[0] == 0xFFFFFFFF
    _check_stream(eng, dva, R.vocab_a(), t, monkeypatch)


@pytest.mark.parametrize("n", [1, 5, 64, R.BLK + 1])
def test_all_unknown_ids(eng, dva, n, monkeypatch):
    want = _check_stream(eng, dva, R.vocab_a(), R.all_unknown(n), monkeypatch)
    assert want.tobytes() == bytes(R.REPLACEMENT) * n


def test_one_65535_byte_token_between_one_byte_tokens(eng, dva, monkeypatch):
    want = _check_stream(eng, dva, R.vocab_a(), R.big_entry_stream(), monkeypatch)
    assert want.shape[0] == 65535 + 5


def test_several_65535_byte_tokens_in_one_block(eng, dva, monkeypatch):
    # one workgroup's output range far above its neighbour's: each lane loops over many vectors
    t = R.big_block_stream()
    want = _check_stream(eng, dva, R.vocab_a(), t, monkeypatch)
    assert int(R.decode_np(t[:R.BLK], R.vocab_a()).shape[0]) > 3 * 65535 and want.shape[0] > 3 * 65535


def test_upload_refuses_a_65536_byte_entry(eng):
    rc, dv = upload_vocab(eng, [[1], [7] * 65536, [2]])
    assert rc == E_INVALID and not dv.value
    from gpubpe import _lib
    assert "entry 1" in _lib.load().gbpe_last_error(eng.device).decode()


def test_more_than_1024_scan_blocks(eng, dvb, monkeypatch):
    t = R.large_stream_b()
    assert t.shape[0] > 1024 * R.BLK + R.BLK
    _check_stream(eng, dvb, R.vocab_b(), t, monkeypatch)


# ── capacity and alignment ──────────────────────────────────────────────────
def _capacity_case():
    docs = R.batch_documents([0, 5, 64, 0, 65, 700, 1, 0], seed=600)
    from gpubpe import flatten_token_documents
    toks, tok_off = flatten_token_documents(docs)
    want = R.decode_np(toks, R.vocab_a())
    want_off = np.zeros(len(docs) + 1, dtype=np.uint64)
    want_off[1:] = np.cumsum([len(O.decode(d, R.vocab_a())) for d in docs], dtype=np.uint64)
    return toks, tok_off, want, want_off


@pytest.mark.parametrize("form", [device_decode, host_decode], ids=["device", "host"])
@pytest.mark.parametrize("room", ["0", "1", "total-17", "total-1", "total"])
def test_capacity(eng, dva, room, form, monkeypatch):
    toks, tok_off, want, want_off = _capacity_case()
    total = int(want.shape[0])
    assert total > 64
    cap = {"0": 0, "1": 1, "total-17": total - 17, "total-1": total - 1, "total": total}[room]
    for name, knob in PATHS:
        _set_path(monkeypatch, knob)
        for offs in (None, tok_off):
            rc, n_out, out, guard, off = form(eng, dva, toks, cap, offs)
            assert rc == (OK if cap >= total else E_CAPACITY), (name, cap)
            assert n_out == total                                  # the required byte count
            assert np.array_equal(out, want[:cap]), (name, cap)    # the first out_cap bytes are in place
            assert np.all(guard == 0xA5), (name, cap)              # nothing at or beyond out[out_cap]
            if offs is not None:
                assert np.array_equal(off, want_off), (name, cap)  # complete


def test_device_form_rejects_misaligned_pointers(eng, dva):
    t = R.random_stream(65, 165)
    total = int(R.decode_np(t, R.vocab_a()).shape[0])
    dev = DecodeDev(eng, t, total + 16, tok_off=[0, 65])
    try:
        args = dict(tok=dev.d_tok, out=dev.d_out, toff=dev.d_tok_off, boff=dev.d_byte_off)
        for which, shift in (("out", 4), ("tok", 2), ("toff", 4), ("boff", 4)):
            a = dict(args)
            a[which] = C.c_void_p(args[which].value + shift)
            n_out = C.c_uint64(777)
            if which in ("out", "tok"):
                rc = dev.lib.gbpe_decode_device(dev.ctx, dva, a["tok"], 64, a["out"], total, C.byref(n_out))
                assert (rc, n_out.value) == (E_INVALID, 0), which
                n_out = C.c_uint64(777)
            rc = dev.lib.gbpe_decode_batch_device(dev.ctx, dva, a["tok"], 64, a["toff"], 1, a["out"], total, a["boff"],
                                                  C.byref(n_out))
            assert (rc, n_out.value) == (E_INVALID, 0), which
        out, guard = dev.output()
        assert np.all(out == 0xA5) and np.all(guard == 0xA5)        # nothing launched
        assert np.all(dev.byte_off() == POISON)
    finally:
        dev.free()


# ── batches ─────────────────────────────────────────────────────────────────
def test_batch_matches_per_document_decode(eng, dva, monkeypatch):
    from gpubpe import TrieTokenizer
    docs = R.batch_documents()
    assert [d.shape[0] for d in docs] == R.BATCH_COUNTS
    toks, tok_off, want, want_off = _check_batch(eng, dva, R.vocab_a(), docs, monkeypatch)
    # the given-offsets form of the Python method
    tok = TrieTokenizer.__new__(TrieTokenizer)
    tok._engine, tok._trie, tok._vocab = eng, None, R.vocab_a()
    got, off = tok.decode_batch(toks, tok_off)
    assert got.dtype == np.uint8 and off.dtype == np.uint64
    assert np.array_equal(got, want) and np.array_equal(off, want_off)
    got, off = tok.decode_batch(docs)
    assert np.array_equal(got, want) and np.array_equal(off, want_off)
    tok.destroy()


def test_batch_of_many_small_documents(eng, dva, monkeypatch):
    docs = R.many_small_documents()
    assert len(docs) == 10000 and sum(d.shape[0] == 0 for d in docs) > 1000
    _, tok_off, _, _ = _check_batch(eng, dva, R.vocab_a(), docs, monkeypatch)
    assert int(tok_off[-1]) > 4 * R.BLK


def test_batch_without_documents_or_tokens(eng, dva):
    for form in (host_decode, device_decode):
        rc, n_out, _, guard, off = form(eng, dva, np.zeros(0, np.uint32), 8, [0])
        assert (rc, n_out, off.tolist()) == (OK, 0, [0])
        rc, n_out, _, guard, off = form(eng, dva, np.zeros(0, np.uint32), 8, [0, 0, 0])
        assert (rc, n_out, off.tolist()) == (OK, 0, [0, 0, 0]) and np.all(guard == 0xA5)


@pytest.mark.parametrize("offsets", [[0, 5, 4, 9], [2, 4, 9], [0, 4, 8], [0, 12, 9], [0, 4, 1 << 40]],
                         ids=["decreasing", "first-not-0", "last-not-n", "entry-above-n", "last-far-above-n"])
def test_batch_bad_offsets(eng, dva, offsets, monkeypatch):
    from gpubpe import _lib
    t = R.random_stream(9, 99)
    for name, knob in PATHS:
        _set_path(monkeypatch, knob)
        for form in (host_decode, device_decode):
            rc, n_out, out, guard, _ = form(eng, dva, t, 64, offsets)
            assert (rc, n_out) == (E_INVALID, 0), (name, form.__name__)
            assert "offsets" in _lib.load().gbpe_last_error(eng.device).decode()
            assert np.all(out == 0xA5) and np.all(guard == 0xA5)    # the scatter was not launched


def test_host_slices_equal_one_pass(eng, dva, monkeypatch):
    from gpubpe import flatten_token_documents
    docs = R.sliced_documents()
    toks, tok_off = flatten_token_documents(docs)
    assert toks.shape[0] == 9001
    want = R.decode_np(toks, R.vocab_a())
    total = int(want.shape[0])
    for name, knob in PATHS:
        _set_path(monkeypatch, knob)
        whole = host_decode(eng, dva, toks, total, tok_off)
        _set_path(monkeypatch, knob, "decode_slice=1000")
        sliced = host_decode(eng, dva, toks, total, tok_off)
        single = host_decode(eng, dva, toks, total)
        short = host_decode(eng, dva, toks, total - 70000, tok_off)
        for got in (whole, sliced):
            assert got[:2] == (OK, total) and np.array_equal(got[2], want) and np.all(got[3] == 0xA5)
        assert np.array_equal(sliced[4], whole[4]) and int(sliced[4][-1]) == total
        assert single[:2] == (OK, total) and np.array_equal(single[2], want)
        # capacity across slices: the prefix, the guard, the complete offsets
        assert short[:2] == (E_CAPACITY, total) and np.array_equal(short[2], want[:total - 70000])
        assert np.all(short[3] == 0xA5) and np.array_equal(short[4], whole[4])


def test_round_trip_without_the_host(eng, dvb):
    """gbpe_encode_batch_device's token buffer and token offsets feed
    gbpe_decode_batch_device directly: the document byte offsets and the bytes come back."""
    from gpubpe import TrieTokenizer, _lib, synth
    tok = TrieTokenizer.from_vocab(eng, R.vocab_b())
    c = tok.chunk_size
    lengths = [0, 1, 2, 7, 8, 9, 0, 0, 15, 16, 17, 63, 64, 65, c - 1, c, c + 1, 2 * c, 2 * c + 3, 5000, 0]
    text = synth.multilingual(sum(lengths) + 64, seed=32)
    docs, p = [], 3
    for ln in lengths:
        docs.append(text[p:p + ln])
        p += ln
    enc = BatchDev(eng, docs)
    try:
        rc, n_tok = enc.run(tok._trie, tok.chunk_size)
        _lib.check(rc, eng.device, "encode batch device")
        d_bytes = enc.alloc(enc.n + 64, np.full(enc.n + 64, 0xA5, np.uint8))
        d_byte_off = enc.alloc(8 * (enc.n_docs + 1), np.full(enc.n_docs + 1, POISON, np.uint64))
        n_out = C.c_uint64()
        rc = enc.lib.gbpe_decode_batch_device(enc.ctx, dvb, enc.d_out, n_tok, enc.d_tok_off, enc.n_docs, d_bytes, enc.n,
                                              d_byte_off, C.byref(n_out))
        _lib.check(rc, eng.device, "decode batch device")
        assert n_out.value == enc.n
        assert np.array_equal(enc.fetch(d_byte_off, enc.n_docs + 1, np.uint64), enc.offs)
        back = enc.fetch(d_bytes, enc.n + 64, np.uint8)
        assert np.array_equal(back[:enc.n], enc.buf) and np.all(back[enc.n:] == 0xA5)
    finally:
        enc.free()
    tok.destroy()


# ── inventory, the Python methods, timing ───────────────────────────────────
def test_kernel_inventory_lists_the_decode_kernels():
    from gpubpe import _lib
    lib = _lib.load()
    names = [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
    assert {"k_dec_len", "k_dec_scatter", "k_dec_doc_off"} <= set(names) and len(names) == len(set(names))


def test_decode_bytes_equals_decode_and_destroy_twice(eng):
    from gpubpe import TrieTokenizer, synth
    tok = TrieTokenizer.from_vocab(eng, R.vocab_b())
    text = synth.multilingual(30000, seed=44)
    ids = tok.encode_bytes(text)
    assert tok.decode_bytes(ids) == tok.decode(ids) == text
    mixed = np.concatenate([ids[:100], np.array([len(R.vocab_b()), 0xFFFFFFFF], dtype=np.uint32), ids[100:200]])
    assert tok.decode_bytes(mixed) == tok.decode(mixed)
    assert tok.decode_bytes(mixed.tolist()) == tok.decode(mixed)
    assert tok.decode_bytes([]) == b""
    tok.destroy()
    tok.destroy()


def test_timing_reports_three_figures(eng, dva):
    from gpubpe import _lib
    t = R.random_stream(R.BLK + 1, 100 + R.BLK + 1)
    total = int(R.decode_np(t, R.vocab_a()).shape[0])
    rc, n_out, _, _, _ = device_decode(eng, dva, t, total, [0, 7, t.shape[0]])
    assert (rc, n_out) == (OK, total)
    a, b, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    assert _lib.load().gbpe_decode_last_timing(eng.device, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert a.value > 0 and b.value > 0 and c.value > 0
