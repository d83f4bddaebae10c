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


MAX_VOCAB_ENTRY_BYTES = 65535   # gbpe_vocab_upload's cap on one entry


def _bad_offsets(msg: str, what: str = "encode batch"):
    return _lib.GpuBpeError(_lib.GBPE_E_INVALID, f"{what}: {msg} (status {_lib.GBPE_E_INVALID})")


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
    offs = _checked_offsets(offsets, int(buf.shape[0]), "encode batch", "buffer's length")
    return np.ascontiguousarray(buf), offs


def _checked_offsets(offsets, length: int, what: str, unit: str):
    raw = np.asarray(offsets)
    if raw.ndim != 1 or raw.shape[0] < 1:
        raise _bad_offsets("offsets must be a one-dimensional sequence of D + 1 entries", what)
    if raw.dtype.kind not in "iu" or (raw.dtype.kind == "i" and raw.shape[0] and int(raw.min()) < 0):
        raise _bad_offsets("offsets must be non-negative integers", what)
    offs = np.ascontiguousarray(raw, dtype=np.uint64)
    if int(offs[0]) != 0:
        raise _bad_offsets("offsets must start at 0", what)
    if offs.shape[0] > 1 and bool(np.any(offs[1:] < offs[:-1])):
        raise _bad_offsets("offsets must not decrease", what)
    if int(offs[-1]) != length:
        raise _bad_offsets(f"offsets must end at the {unit} ({length}), not {int(offs[-1])}", what)
    return offs


def flatten_vocab(vocab):
    """The vocab layout of gbpe_vocab_upload / gbpe_trie_compile, on the host:
    returns (bytes: np.uint8[], offsets: np.uint64[V + 1]); token id i has
    bytes[offsets[i]:offsets[i + 1]] (empty entries allowed).  An entry above
    65,535 bytes raises GpuBpeError with GBPE_E_INVALID, the status the upload
    gives it."""
    lens = np.fromiter((len(e) for e in vocab), dtype=np.uint64, count=len(vocab))
    if lens.shape[0] and int(lens.max()) > MAX_VOCAB_ENTRY_BYTES:
        i = int(np.argmax(lens > MAX_VOCAB_ENTRY_BYTES))
        raise _bad_offsets(f"entry {i} has {int(lens[i])} bytes (at most {MAX_VOCAB_ENTRY_BYTES})", "vocab")
    offs = np.zeros(lens.shape[0] + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    flat = bytearray()
    for e in vocab:
        flat.extend(bytes(e))
    return np.frombuffer(bytes(flat), dtype=np.uint8), offs


def flatten_token_documents(docs, offsets=None):
    """The batch layout of gbpe_decode_batch, on the host (the token twin of
    flatten_documents): returns (tokens: np.uint32[n], offsets: np.uint64[D + 1]).

    offsets None: ``docs`` is a sequence of token-id sequences, laid end to end.
    Otherwise ``docs`` is one token-id sequence and ``offsets`` its D + 1 document
    offsets, checked as flatten_documents checks byte offsets (GBPE_E_INVALID).
    """
    if offsets is None:
        parts = [np.ascontiguousarray(d, dtype=np.uint32).reshape(-1) for d in docs]
        offs = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            offs[1:] = np.cumsum([p.shape[0] for p in parts], dtype=np.uint64)
        toks = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
        return np.ascontiguousarray(toks, dtype=np.uint32), offs
    toks = np.ascontiguousarray(docs, dtype=np.uint32).reshape(-1)
    return toks, _checked_offsets(offsets, int(toks.shape[0]), "decode batch", "token count")


def decoded_size(tokens, vocab_offsets) -> int:
    """Exact byte count of the decode of ``tokens`` (gbpe_decode_size: host only, no
    device); vocab_offsets = flatten_vocab(vocab)[1].  Unknown ids count 3 bytes."""
    toks = np.ascontiguousarray(tokens, dtype=np.uint32).reshape(-1)
    offs = np.ascontiguousarray(vocab_offsets, dtype=np.uint64)
    if offs.ndim != 1 or offs.shape[0] < 1:
        raise _bad_offsets("vocab offsets must be a one-dimensional sequence of V + 1 entries", "decode size")
    n = C.c_uint64()
    _lib.check(_lib.load().gbpe_decode_size(offs.ctypes.data_as(_lib.u64p), offs.shape[0] - 1,
                                            toks.ctypes.data_as(_lib.u32p), toks.shape[0], C.byref(n)),
               None, "decode size")
    return int(n.value)


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

    def _device_vocab(self):
        """The vocab table on the device, uploaded on first use."""
        if getattr(self, "_dvocab", None) is None:
            flat, offs = flatten_vocab(self._vocab)
            ctx = self._engine.device
            dv = C.c_void_p()
            _lib.check(_lib.load().gbpe_vocab_upload(ctx, flat.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(_lib.u64p),
                                                     offs.shape[0] - 1, C.byref(dv)), ctx, "vocab upload")
            self._dvocab, self._vocab_offsets = dv, offs
        return self._dvocab

    def decode_bytes(self, tokens) -> bytes:
        """decode() on the device (gbpe_decode): the same bytes."""
        toks = np.ascontiguousarray(tokens, dtype=np.uint32).reshape(-1)
        if toks.shape[0] == 0:
            return b""
        return self.decode_batch(toks, [0, toks.shape[0]])[0].tobytes()

    def decode_batch(self, docs, offsets=None):
        """Many token documents in one call (gbpe_decode_batch): returns (bytes:
        np.uint8[N], offsets: np.uint64[D + 1]); bytes[offsets[d]:offsets[d + 1]] is
        what decode returns for document d alone.  ``docs`` / ``offsets``: see
        flatten_token_documents."""
        toks, offs = flatten_token_documents(docs, offsets)
        n, n_docs = int(toks.shape[0]), int(offs.shape[0]) - 1
        byte_off = np.zeros(n_docs + 1, dtype=np.uint64)
        if n == 0 or n_docs == 0:
            return np.zeros(0, dtype=np.uint8), byte_off
        lib = _lib.load()
        ctx = self._engine.device
        dv = self._device_vocab()
        size = decoded_size(toks, self._vocab_offsets)   # exact: one device call, no second pass
        out = np.empty(size, dtype=np.uint8)
        n_out = C.c_uint64()
        _lib.check(lib.gbpe_decode_batch(ctx, dv, toks.ctypes.data_as(_lib.u32p), n, offs.ctypes.data_as(_lib.u64p),
                                         n_docs, out.ctypes.data_as(C.c_void_p), size,
                                         byte_off.ctypes.data_as(_lib.u64p), C.byref(n_out)), ctx, "decode batch")
        return out[: n_out.value], byte_off

    def destroy(self):
        if getattr(self, "_dvocab", None):
            _lib.load().gbpe_vocab_free(self._dvocab)
            self._dvocab = None
        if getattr(self, "_trie", None):
            _lib.load().gbpe_trie_free(self._trie)
            self._trie = None
