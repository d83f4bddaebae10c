"""MergeEncoder — TokenizerManager.encode (src/bpe/tokenizer/tokenizer-manager.js:13-61)
on the device: the learned merges applied in rank order to the whole byte
string, through gbpe_bpe_upload / gbpe_bpe_encode — or, with word starts, inside
each word alone (gbpe_bpe_encode_words: pre-tokenise, then BPE per word); many
documents in one call through gbpe_bpe_encode_words_batch."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

WORDS_MODES = {"heuristic": _lib.GBPE_WORDS_HEURISTIC, "gpt4": _lib.GBPE_WORDS_GPT4}


def _bad_words(msg: str):
    return _lib.GpuBpeError(_lib.GBPE_E_INVALID, f"bpe encode: {msg} (status {_lib.GBPE_E_INVALID})")


def checked_word_starts(n: int, word_starts=None, words=None):
    """The (mode, mask) of one encode_bytes call over n bytes, checked on the host
    (no device, no library): mask is a contiguous np.uint8[n] for a caller's
    ``word_starts`` (non-zero = word start) and None otherwise.  Giving both
    arguments, an unknown ``words`` name, or a mask that is not one-dimensional
    with n entries raises GpuBpeError with GBPE_E_INVALID, the status the library
    gives a bad mode."""
    if word_starts is not None and words is not None:
        raise _bad_words("give word_starts or words, not both")
    if words is not None:
        if words not in WORDS_MODES:
            raise _bad_words(f"words must be None, 'heuristic' or 'gpt4', not {words!r}")
        return WORDS_MODES[words], None
    if word_starts is None:
        return _lib.GBPE_WORDS_NONE, None
    if isinstance(word_starts, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(word_starts, dtype=np.uint8)
    else:
        raw = np.asarray(word_starts)
        if raw.size == 0 and raw.ndim == 1:
            raw = raw.astype(np.uint8)   # (an empty list has no integer dtype of its own)
    if raw.ndim != 1 or raw.dtype.kind not in "biu":
        raise _bad_words("word_starts must be a one-dimensional mask of booleans or integers")
    if raw.shape[0] != n:
        raise _bad_words(f"word_starts has {raw.shape[0]} entries for {n} bytes")
    return _lib.GBPE_WORDS_MASK, np.ascontiguousarray(raw != 0, dtype=np.uint8)


class MergeEncoder:
    def __init__(self, engine, merges):
        self._engine = engine
        self._merges = [list(m[:3]) for m in merges]
        lib = _lib.load()
        arr = np.ascontiguousarray(np.asarray(self._merges, dtype=np.uint32).reshape(-1, 3))
        h = C.c_void_p()
        _lib.check(lib.gbpe_bpe_upload(engine.device, arr.ctypes.data_as(_lib.u32p), arr.shape[0], C.byref(h)),
                   engine.device, "bpe upload")
        self._h = h

    def encode_bytes(self, data, word_starts=None, words=None) -> np.ndarray:
        """Tokens of ``data``.  ``word_starts`` (a mask, one entry per byte) or
        ``words`` ('heuristic' / 'gpt4': the mask computed on the device) bound
        every token to one word; with neither the merges apply to the whole
        string."""
        data = bytes(data)
        mode, mask = checked_word_starts(len(data), word_starts, words)
        lib = _lib.load()
        ctx = self._engine.device
        out = np.empty(max(1, len(data)), dtype=np.uint32)
        n = C.c_uint64()
        buf = C.create_string_buffer(data, len(data)) if data else None
        if mode == _lib.GBPE_WORDS_NONE:
            _lib.check(lib.gbpe_bpe_encode(ctx, self._h, buf, len(data), out.ctypes.data_as(_lib.u32p), out.shape[0],
                                           C.byref(n)), ctx, "bpe encode")
        else:
            if mask is not None and not len(data):
                mask = np.zeros(1, dtype=np.uint8)   # (a non-NULL pointer goes with the mode)
            _lib.check(lib.gbpe_bpe_encode_words(ctx, self._h, buf, len(data),
                                                 mask.ctypes.data_as(C.c_void_p) if mask is not None else None, mode,
                                                 out.ctypes.data_as(_lib.u32p), out.shape[0], C.byref(n)),
                       ctx, "bpe encode (words)")
        return out[: n.value].copy()

    def encode_batch(self, docs, offsets=None, word_starts=None, words=None):
        """Many documents in one call (gbpe_bpe_encode_words_batch): returns
        ``(tokens, offsets)``, document d's tokens being
        ``tokens[offsets[d]:offsets[d + 1]]`` — exactly ``encode_bytes`` of that
        document alone in the same mode.  ``docs`` and ``offsets`` are
        ``flatten_documents``'s; ``word_starts`` is one mask over the
        concatenation (a document's first byte starts a word whatever it says)."""
        from .tokenizer import flatten_documents
        buf, offs = flatten_documents(docs, offsets)
        n, n_docs = int(buf.shape[0]), int(offs.shape[0]) - 1
        mode, mask = checked_word_starts(n, word_starts, words)
        lib = _lib.load()
        ctx = self._engine.device
        out = np.empty(max(1, n), dtype=np.uint32)
        tok_off = np.zeros(n_docs + 1, dtype=np.uint64)
        cnt = C.c_uint64()
        if mask is not None and not n:
            mask = np.zeros(1, dtype=np.uint8)   # (a non-NULL pointer goes with the mode)
        _lib.check(lib.gbpe_bpe_encode_words_batch(ctx, self._h, buf.ctypes.data_as(C.c_void_p), n,
                                                   offs.ctypes.data_as(_lib.u64p), n_docs,
                                                   mask.ctypes.data_as(C.c_void_p) if mask is not None else None, mode,
                                                   out.ctypes.data_as(_lib.u32p), out.shape[0],
                                                   tok_off.ctypes.data_as(_lib.u64p), C.byref(cnt)),
                   ctx, "bpe encode batch")
        return out[: cnt.value].copy(), tok_off

    def encode(self, text, word_starts=None, words=None) -> dict:
        """{tokens, text} like TokenizerManager.encode's result (tokenizer-manager.js:60)."""
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        return {"tokens": self.encode_bytes(data, word_starts, words).tolist(), "text": text}

    def destroy(self):
        if self._h:
            _lib.load().gbpe_bpe_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001
            pass
