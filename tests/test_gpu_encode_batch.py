"""Batched document encode (gbpe_encode_batch / gbpe_encode_batch_device /
TrieTokenizer.encode_batch) against the CPU oracle.

The expected result is always the concatenation, over the documents, of the
oracle's encode_chunked of each document alone with the same chunk size; the
token offsets are the running sum of those lengths.  Exact comparisons.
"""
import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
from encode_dev import BatchDev as _Dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


@pytest.fixture(scope="module")
def vocab1200():
    # the vocab of test_encode_matches_oracle
    from gpubpe import synth
    train = synth.multilingual(80000, seed=31)
    return O.vocab_from_merges(O.train(train, 1200, compaction="exact")["merges"]).entries


def _trie_arrays(vocab):
    blob = O.compile_vocab_to_trie(vocab)
    return O.parse_trie_buffers(blob, O.parse_header(blob))


def _expect(vocab, docs, cs):
    """(tokens, offsets) of the oracle: every document encoded alone."""
    nodes, edges = _trie_arrays(vocab)
    parts = [np.asarray(O.encode_chunked(bytes(d), nodes, edges, cs), dtype=np.uint32) if len(d) else
             np.zeros(0, np.uint32) for d in docs]
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([p.shape[0] for p in parts], dtype=np.uint64)
    toks = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    return toks.astype(np.uint32), offs


def _cut(text, lengths):
    """Consecutive documents of the given lengths from `text` (any byte position:
    unaligned starts, multi-byte characters split)."""
    docs, p = [], 3   # (not even the first document starts at the text's first byte)
    for ln in lengths:
        docs.append(text[p:p + ln])
        p += ln
    assert p <= len(text)
    return docs


def _device_batch(eng, tok, docs):
    from gpubpe import _lib
    dev = _Dev(eng, docs)
    try:
        rc, t = dev.run(tok._trie, tok.chunk_size)
        _lib.check(rc, eng.device, "encode batch device")
        return dev.fetch(dev.d_out, t, np.uint32), dev.fetch(dev.d_tok_off, dev.n_docs + 1, np.uint64)
    finally:
        dev.free()


def _check_both(eng, tok, vocab, docs):
    want, want_off = _expect(vocab, docs, tok.chunk_size)
    got, got_off = tok.encode_batch(docs)
    dgot, dgot_off = _device_batch(eng, tok, docs)
    assert got_off.dtype == np.uint64 and got.dtype == np.uint32
    assert np.array_equal(got_off, want_off) and np.array_equal(got, want)
    assert np.array_equal(dgot_off, want_off) and np.array_equal(dgot, want)
    return want, want_off


@pytest.mark.parametrize("cs", [None, 1, 7, 8, 64, 512])
def test_batch_shapes_match_oracle(eng, vocab1200, cs):
    from gpubpe import TrieTokenizer, synth
    tok = TrieTokenizer.from_vocab(eng, vocab1200, chunk_size=cs)
    c = tok.chunk_size
    lengths = [0, 1, 2, 7, 8, 9, 0, 0, 15, 16, 17, 63, 64, 65, c - 1, c, c + 1, 2 * c, 2 * c + 3, 5000, 0]
    text = synth.multilingual(sum(lengths) + 64, seed=32)
    docs = _cut(text, lengths)
    assert [len(d) for d in docs] == lengths
    want, want_off = _check_both(eng, tok, vocab1200, docs)
    # the given-offsets form: one buffer + offsets
    got, got_off = tok.encode_batch(b"".join(docs), np.cumsum([0] + lengths))
    assert np.array_equal(got, want) and np.array_equal(got_off, want_off)
    tok.destroy()


def test_batch_no_match_across_a_document_boundary(eng):
    from gpubpe import TrieTokenizer
    vocab = O.vocab_from_merges([[116, 104], [256, 101]]).entries   # 256 = "th", 257 = "the"
    tok = TrieTokenizer.from_vocab(eng, vocab)
    docs = [b"t", b"he", b"th", b"e", b"", b"the"]
    want = [[116], [104, 101], [256], [101], [], [257]]              # by hand
    got, off = tok.encode_batch(docs)
    assert [got[int(off[d]):int(off[d + 1])].tolist() for d in range(len(docs))] == want
    dgot, doff = _device_batch(eng, tok, docs)
    assert np.array_equal(dgot, got) and np.array_equal(doff, off)
    assert off.tolist() == [0, 1, 3, 4, 5, 5, 6]
    # the same bytes as one stream match across the boundaries: a different answer
    one = tok.encode_bytes(b"".join(docs)).tolist()
    assert one == [257, 257, 257] and one != got.tolist()
    tok.destroy()


def test_batch_more_than_one_scan_block_of_documents(eng):
    # 10,000 documents of 0..6 bytes: more than 4096 documents (several table
    # blocks), more than 4096 chunks (several count-scan blocks), many empty ones
    from gpubpe import TrieTokenizer
    vocab = O.vocab_from_merges([[116, 104], [256, 101], [32, 257]]).entries
    tok = TrieTokenizer.from_vocab(eng, vocab, chunk_size=8)
    rng = np.random.default_rng(20260)
    lengths = rng.integers(0, 7, size=10000).tolist()
    text = b"the then " * (sum(lengths) // 9 + 2)
    docs = _cut(text, lengths)
    _, want_off = _check_both(eng, tok, vocab, docs)
    assert lengths.count(0) > 1000 and int(want_off[-1]) > 4096
    tok.destroy()


def test_batch_more_than_one_scan_block_of_chunks(eng):
    # ~40 KB in 30 documents at cs = 8: more than 4096 chunks, and documents
    # whose first chunk lies in the second count-scan block
    from gpubpe import TrieTokenizer
    vocab = O.vocab_from_merges([[116, 104], [256, 101], [32, 257]]).entries
    tok = TrieTokenizer.from_vocab(eng, vocab, chunk_size=8)
    rng = np.random.default_rng(20261)
    lengths = rng.integers(900, 1800, size=30).tolist()
    lengths[11] = 0
    lengths[29] = 0
    assert sum(lengths) > 8 * 4096 + 4000
    first_chunk = np.cumsum([0] + [(ln + 7) // 8 for ln in lengths])
    assert first_chunk[-1] > 4096 and np.sum(first_chunk[:-1] > 4096) >= 3
    docs = _cut(b"the then " * (sum(lengths) // 9 + 2), lengths)
    _check_both(eng, tok, vocab, docs)
    tok.destroy()


def test_batch_wide_token_ids(eng):
    # token ids >= 65536: the 32-bit scratch (8-element slots of 32 bytes)
    from gpubpe import TrieTokenizer
    voc = [[b] for b in range(256)] + [[] for _ in range(70000)]
    voc[70100] = [97, 98, 99]
    voc[65600] = [97, 98]
    tok = TrieTokenizer.from_vocab(eng, voc, chunk_size=16)
    text = b"abcab xabc" * 50
    docs = _cut(text, [1, 3, 5, 0, 16, 17, 40, 33, 2])
    want, _ = _check_both(eng, tok, voc, docs)
    assert 70100 in want.tolist() and 65600 in want.tolist()
    tok.destroy()


def test_batch_of_one_document_equals_single_stream(eng, vocab1200):
    from gpubpe import TrieTokenizer, _lib, synth
    tok = TrieTokenizer.from_vocab(eng, vocab1200)
    text = synth.multilingual(30000, seed=32)
    dev = _Dev(eng, [text])
    try:
        rc, t = dev.run(tok._trie, tok.chunk_size)
        _lib.check(rc, eng.device, "encode batch device")
        batch = dev.fetch(dev.d_out, t, np.uint32)
        off = dev.fetch(dev.d_tok_off, 2, np.uint64)
        n_out = C.c_uint64()
        _lib.check(dev.lib.gbpe_encode_device(dev.ctx, tok._trie, dev.d_in, dev.n, tok.chunk_size, dev.d_out, dev.n,
                                              C.byref(n_out)), eng.device, "encode device")
        single = dev.fetch(dev.d_out, int(n_out.value), np.uint32)
    finally:
        dev.free()
    assert np.array_equal(batch, single)
    assert off.tolist() == [0, single.shape[0]]
    assert np.array_equal(single, _expect(vocab1200, [text], tok.chunk_size)[0])
    tok.destroy()


@pytest.mark.parametrize("short", ["one", "all"])
def test_batch_capacity(eng, vocab1200, short):
    from gpubpe import TrieTokenizer, _lib, synth
    tok = TrieTokenizer.from_vocab(eng, vocab1200, chunk_size=64)
    lengths = [0, 5, 64, 0, 65, 700, 1, 0]
    docs = _cut(synth.multilingual(2000, seed=32), lengths)
    want, want_off = _expect(vocab1200, docs, 64)
    total = int(want.shape[0])
    cap = total - 1 if short == "one" else 0
    dev = _Dev(eng, docs, out_cap=cap, guard=64)
    try:
        rc, t = dev.run(tok._trie, tok.chunk_size)
        out = dev.fetch(dev.d_out, cap + 64, np.uint32)
        off = dev.fetch(dev.d_tok_off, len(docs) + 1, np.uint64)
    finally:
        dev.free()
    assert rc == _lib.GBPE_E_CAPACITY and t == total
    assert np.array_equal(off, want_off)                       # complete and correct
    assert np.all(out[cap:] == 0xA5A5A5A5)                     # nothing at or beyond out[out_cap]
    assert np.array_equal(out[:cap], want[:cap])
    tok.destroy()


def test_batch_host_groups(eng, vocab1200, monkeypatch):
    # the host variant runs inputs above the encode slice as groups of whole
    # documents; a document above the slice is a group of its own
    from gpubpe import TrieTokenizer, synth
    tok = TrieTokenizer.from_vocab(eng, vocab1200, chunk_size=64)
    lengths = [1000, 0, 3000, 96, 0, 9000, 4096, 1, 4095, 0, 0, 2500, 2500, 0]
    docs = _cut(synth.multilingual(sum(lengths) + 64, seed=32), lengths)
    want, want_off = _expect(vocab1200, docs, 64)
    monkeypatch.setenv("GBPE_DEBUG", "encode_slice=4096")
    got, off = tok.encode_batch(docs)
    monkeypatch.delenv("GBPE_DEBUG")
    whole, whole_off = tok.encode_batch(docs)
    assert np.array_equal(got, whole) and np.array_equal(off, whole_off)
    assert np.array_equal(got, want) and np.array_equal(off, want_off)
    tok.destroy()


@pytest.mark.parametrize("offsets", [[0, 4, 3, 9], [1, 4, 9], [0, 4, 8]],
                         ids=["decreasing", "first-not-0", "last-not-n"])
def test_batch_argument_checks(eng, offsets):
    # host variant, host arrays: rejected before anything reaches the device
    from gpubpe import TrieTokenizer, _lib
    vocab = O.vocab_from_merges([[116, 104], [256, 101]]).entries
    tok = TrieTokenizer.from_vocab(eng, vocab)
    lib = _lib.load()
    data = np.frombuffer(b"the thing", dtype=np.uint8).copy()
    offs = np.array(offsets, dtype=np.uint64)
    out = np.full(16, 0xA5A5A5A5, dtype=np.uint32)
    tok_off = np.zeros(len(offsets), dtype=np.uint64)
    n_out = C.c_uint64()
    rc = lib.gbpe_encode_batch(eng.device, tok._trie, data.ctypes.data_as(C.c_void_p), data.shape[0],
                               offs.ctypes.data_as(_lib.u64p), len(offsets) - 1, tok.chunk_size,
                               out.ctypes.data_as(_lib.u32p), 16, tok_off.ctypes.data_as(_lib.u64p), C.byref(n_out))
    with pytest.raises(_lib.GpuBpeError) as ei:
        _lib.check(rc, eng.device, "encode batch")
    assert ei.value.code == _lib.GBPE_E_INVALID and "offsets" in str(ei.value)
    assert np.all(out == 0xA5A5A5A5)
    # the Python method gives the same status
    with pytest.raises(_lib.GpuBpeError) as ei:
        tok.encode_batch(data, offsets)
    assert ei.value.code == _lib.GBPE_E_INVALID
    tok.destroy()


def test_batch_device_rejects_bad_offsets_and_alignment(eng):
    # the device variant's first kernel checks the offsets; nothing else runs
    from gpubpe import TrieTokenizer, _lib
    vocab = O.vocab_from_merges([[116, 104], [256, 101]]).entries
    tok = TrieTokenizer.from_vocab(eng, vocab)
    dev = _Dev(eng, [b"the ", b"thing"], guard=8)
    try:
        for bad in ([0, 5, 4], [2, 4, 9], [0, 4, 8], [0, 12, 9]):
            offs = np.array(bad, dtype=np.uint64)
            _lib.check(dev.lib.gbpe_memcpy_h2d(dev.ctx, dev.d_off, offs.ctypes.data_as(C.c_void_p), offs.nbytes),
                       dev.ctx, "h2d")
            rc, _ = dev.run(tok._trie, tok.chunk_size)
            assert rc == _lib.GBPE_E_INVALID, bad
            assert np.all(dev.fetch(dev.d_out, dev.out_cap + 8, np.uint32) == 0xA5A5A5A5), bad
        n_out = C.c_uint64()
        rc = dev.lib.gbpe_encode_batch_device(dev.ctx, tok._trie, C.c_void_p(dev.d_in.value + 4), 4, dev.d_off, 1,
                                              tok.chunk_size, dev.d_out, dev.out_cap, dev.d_tok_off, C.byref(n_out))
        assert rc == _lib.GBPE_E_INVALID
        rc = dev.lib.gbpe_encode_batch_device(dev.ctx, tok._trie, dev.d_in, 9, C.c_void_p(dev.d_off.value + 4), 1,
                                              tok.chunk_size, dev.d_out, dev.out_cap, dev.d_tok_off, C.byref(n_out))
        assert rc == _lib.GBPE_E_INVALID
    finally:
        dev.free()
    tok.destroy()


def test_batch_timing_reports_three_figures(eng, vocab1200):
    from gpubpe import TrieTokenizer, _lib, synth
    tok = TrieTokenizer.from_vocab(eng, vocab1200)
    docs = _cut(synth.multilingual(20000, seed=32), [3000, 0, 9000, 7000])
    tok.encode_batch(docs)
    w, s, c = C.c_double(-1), C.c_double(-1), C.c_double(-1)
    assert _lib.load().gbpe_encode_last_timing(eng.device, C.byref(w), C.byref(s), C.byref(c)) == 0
    assert w.value > 0 and s.value > 0 and c.value > 0
    tok.destroy()
