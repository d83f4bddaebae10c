"""The context's grown work buffers (GbpeGrowBuf: trie encode, decode, the
pre-tokenizer's block aggregates) across a growth: every path that owns one runs at a
small, a large and the small size again in a context of its own, so the first call
allocates and the second frees a buffer the stream has used and allocates a larger one.
Each result is the CPU oracle's, and the two small results are the same.
"""
import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
from decode_dev import host_decode
from encode_dev import DevBuffers
from gpubpe import BPEEngine, GpuPreTokenizer, TrieTokenizer, _lib, synth

pytestmark = pytest.mark.gpu

BYTE_SIZES = (1_000, 300_000, 1_000)
PRETOK_SIZES = (100, 3 * 4096 + 1, 100)   # 1 and 4 blocks of pretok.hip: 8, then 20 bytes of aggregates
N_DOCS = 50


def _cut(data):
    """about N_DOCS documents of equal length, the rest in a last one"""
    step = len(data) // N_DOCS
    return [data[i:i + step] for i in range(0, len(data), step)]


@pytest.fixture(scope="module")
def refs():
    """vocab, chunk size and per size the oracle's {bytes, tokens, documents, their tokens}"""
    vocab = O.vocab_from_merges(O.train(synth.english(32768, seed=61), 400)["merges"]).entries
    blob = O.compile_vocab_to_trie(vocab)
    hdr = O.parse_header(blob)
    nodes, edges = O.parse_trie_buffers(blob, hdr)
    cs = max(512, min(2048, hdr["maxTokenLen"] * 8))
    text = synth.english(max(BYTE_SIZES), seed=62)
    by_size = {}
    for n in set(BYTE_SIZES):
        data = text[:n]
        docs = _cut(data)
        doc_toks = [np.asarray(O.encode_chunked(d, nodes, edges, cs), np.uint32) for d in docs]
        toks = np.asarray(O.encode_chunked(data, nodes, edges, cs), np.uint32)
        assert O.decode(toks.tolist(), vocab) == data and len(docs) in (N_DOCS, N_DOCS + 1)
        by_size[n] = {"data": data, "toks": toks, "docs": docs, "doc_toks": doc_toks}
    return vocab, cs, by_size


@pytest.fixture()
def fresh():
    e = BPEEngine().init()   # (a context of its own: every buffer starts empty)
    yield e
    e.close()


def _offsets(parts):
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return off


def test_encode(fresh, refs):
    vocab, cs, by_size = refs
    tok = TrieTokenizer.from_vocab(fresh, vocab)
    assert tok.chunk_size == cs
    got = [tok.encode_bytes(by_size[n]["data"]) for n in BYTE_SIZES]
    for n, g in zip(BYTE_SIZES, got):
        assert np.array_equal(g, by_size[n]["toks"]), n
    assert np.array_equal(got[0], got[2])
    tok.destroy()


def test_encode_batch(fresh, refs):
    vocab, _, by_size = refs
    tok = TrieTokenizer.from_vocab(fresh, vocab)
    got = [tok.encode_batch(by_size[n]["docs"]) for n in BYTE_SIZES]
    for n, (g, off) in zip(BYTE_SIZES, got):
        assert np.array_equal(g, np.concatenate(by_size[n]["doc_toks"])), n
        assert np.array_equal(off, _offsets(by_size[n]["doc_toks"])), n
    assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[0][1], got[2][1])
    tok.destroy()


@pytest.mark.parametrize("batch", [False, True], ids=["decode", "decode_batch"])
def test_decode(fresh, refs, batch):
    vocab, _, by_size = refs
    tok = TrieTokenizer.from_vocab(fresh, vocab)
    dv = tok._device_vocab()
    got = []
    for n in BYTE_SIZES:
        r = by_size[n]
        toks = np.concatenate(r["doc_toks"]) if batch else r["toks"]
        want = O.decode(toks.tolist(), vocab)
        rc, n_out, out, guard, off = host_decode(fresh, dv, toks, len(want), _offsets(r["doc_toks"]) if batch else None)
        assert (rc, n_out) == (_lib.GBPE_OK, len(want)) and out.tobytes() == want == r["data"], n
        assert np.all(guard == 0xA5), n
        if batch:
            assert np.array_equal(off, _offsets(r["docs"])), n
        got.append(out.tobytes())
    assert got[0] == got[2]
    tok.destroy()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pretokenize(fresh, device):
    text = synth.multilingual(max(PRETOK_SIZES), seed=63)
    got = []
    for n in PRETOK_SIZES:
        data = text[:n]
        if device:
            dev = DevBuffers(fresh)
            try:
                d_in, d_ws = dev.alloc(n, np.frombuffer(data, np.uint8)), dev.alloc(n, np.full(n, 0xEE, np.uint8))
                _lib.check(dev.lib.gbpe_pretokenize_gpt4_device(fresh.device, d_in, n, d_ws), fresh.device, "pretokenize")
                ws = dev.fetch(d_ws, n, np.uint8)
            finally:
                dev.free()
        else:
            ws = GpuPreTokenizer(fresh).pre_tokenize_bytes(data)["wordStarts"]
        assert np.array_equal(ws, O.gpt4_word_starts(data)), n
        got.append(ws)
    assert np.array_equal(got[0], got[2])
