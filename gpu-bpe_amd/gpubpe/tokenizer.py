"""TrieTokenizer — the reference's encode API (src/bpe/tokenizer/tokenizer.js)
over the native chunked trie walk.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .trie import compile_vocab_to_trie, parse_header, parse_trie_buffers

DEFAULT_CHUNK_SIZE = 512
UTF8_REPLACEMENT = bytes([0xEF, 0xBF, 0xBD])


def _bad_offsets(msg: str):
    return _lib.GpuBpeError(_lib.GBPE_E_INVALID, f"encode batch: {msg} (status {_lib.GBPE_E_INVALID})")


def flatten_documents(docs, offsets=None):
    """The batch layout of gbpe_encode_batch, on the host (no device, no library):
    returns (bytes: np.uint8[n], offsets: np.uint64[D + 1]).

    offsets None: ``docs`` is a sequence of bytes-like objects, laid end to end.
    Otherwise ``docs`` is one bytes-like buffer and ``offsets`` its D + 1 document
    offsets: non-decreasing, from 0 to the buffer's length; anything else raises
    GpuBpeError with GBPE_E_INVALID, the status the library gives such offsets.
    """
    if offsets is None:
        parts = [np.frombuffer(memoryview(d).cast("B"), dtype=np.uint8) for d in docs]
        offs = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            offs[1:] = np.cumsum([p.shape[0] for p in parts], dtype=np.uint64)
        buf = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        return np.ascontiguousarray(buf, dtype=np.uint8), offs
    buf = np.frombuffer(memoryview(docs).cast("B"), dtype=np.uint8)
    raw = np.asarray(offsets)
    if raw.ndim != 1 or raw.shape[0] < 1:
        raise _bad_offsets("offsets must be a one-dimensional sequence of D + 1 entries")
    if raw.dtype.kind not in "iu" or (raw.dtype.kind == "i" and raw.shape[0] and int(raw.min()) < 0):
        raise _bad_offsets("offsets must be non-negative integers")
    offs = np.ascontiguousarray(raw, dtype=np.uint64)
    if int(offs[0]) != 0:
        raise _bad_offsets("offsets must start at 0")
    if offs.shape[0] > 1 and bool(np.any(offs[1:] < offs[:-1])):
        raise _bad_offsets("offsets must not decrease")
    if int(offs[-1]) != buf.shape[0]:
        raise _bad_offsets(f"offsets must end at the buffer's length ({buf.shape[0]}), not {int(offs[-1])}")
    return np.ascontiguousarray(buf), offs


class TrieTokenizer:
    def __init__(self, engine, trie_data: bytes, vocab=None, chunk_size: int | None = None):
        self._engine = engine
        self._vocab = vocab if vocab is not None else [[i] for i in range(256)]
        hdr = parse_header(trie_data)
        nodes, edges = parse_trie_buffers(trie_data, hdr)
        self.node_count = hdr["nodeCount"]
        self.edge_count = hdr["edgeCount"]
        self.max_token_len = hdr["maxTokenLen"]
        adaptive = max(DEFAULT_CHUNK_SIZE, min(2048, hdr["maxTokenLen"] * 8))   # tokenizer.js:67-68
        self.chunk_size = chunk_size if chunk_size is not None else adaptive
        if self.chunk_size <= 0:
            raise ValueError("chunk_size must be positive")
        lib = _lib.load()
        ctx = engine.device
        self._trie = C.c_void_p()
        nodes = np.ascontiguousarray(nodes, dtype=np.uint32)
        edges = np.ascontiguousarray(edges, dtype=np.uint32)
        _lib.check(lib.gbpe_trie_upload(ctx, nodes.ctypes.data_as(_lib.u32p), self.node_count,
                                        edges.ctypes.data_as(_lib.u32p), self.edge_count, C.byref(self._trie)),
                   ctx, "trie upload")

    @classmethod
    def from_vocab(cls, engine, vocab, chunk_size: int | None = None) -> "TrieTokenizer":
        return cls(engine, compile_vocab_to_trie(vocab), vocab, chunk_size)

    def encode_bytes(self, data) -> np.ndarray:
        data = bytes(data)
        n = len(data)
        if n == 0:
            return np.zeros(0, dtype=np.uint32)
        lib = _lib.load()
        ctx = self._engine.device
        out = np.empty(n, dtype=np.uint32)      # at most one token per byte
        n_out = C.c_uint64()
        buf = C.create_string_buffer(data, n)
        _lib.check(lib.gbpe_encode(ctx, self._trie, buf, n, self.chunk_size, out.ctypes.data_as(_lib.u32p), n,
                                   C.byref(n_out)), ctx, "encode")
        return out[: n_out.value].copy()

    def encode_batch(self, docs, offsets=None):
        """Many documents in one call (gbpe_encode_batch): returns (tokens: np.uint32[T],
        offsets: np.uint64[D + 1]); tokens[offsets[d]:offsets[d + 1]] is what
        encode_bytes returns for document d alone.  ``docs`` / ``offsets``: see
        flatten_documents."""
        buf, offs = flatten_documents(docs, offsets)
        n, n_docs = int(buf.shape[0]), int(offs.shape[0]) - 1
        tok_off = np.zeros(n_docs + 1, dtype=np.uint64)
        if n == 0 or n_docs == 0:
            return np.zeros(0, dtype=np.uint32), tok_off
        lib = _lib.load()
        ctx = self._engine.device
        out = np.empty(n, dtype=np.uint32)      # at most one token per byte
        n_out = C.c_uint64()
        _lib.check(lib.gbpe_encode_batch(ctx, self._trie, buf.ctypes.data_as(C.c_void_p), n,
                                         offs.ctypes.data_as(_lib.u64p), n_docs, self.chunk_size,
                                         out.ctypes.data_as(_lib.u32p), n, tok_off.ctypes.data_as(_lib.u64p),
                                         C.byref(n_out)), ctx, "encode batch")
        return out[: n_out.value].copy(), tok_off

    def decode(self, tokens) -> bytes:
        out = bytearray()
        for t in tokens:
            t = int(t)
            out.extend(self._vocab[t] if t < len(self._vocab) else UTF8_REPLACEMENT)
        return bytes(out)

    def destroy(self):
        if getattr(self, "_trie", None):
            _lib.load().gbpe_trie_free(self._trie)
            self._trie = None
