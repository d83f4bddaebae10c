"""MergeEncoder — TokenizerManager.encode (src/bpe/tokenizer/tokenizer-manager.js:13-61)
on the device: the learned merges applied in rank order to the whole byte
string, through gbpe_bpe_upload / gbpe_bpe_encode — or, with word starts, inside
each word alone (gbpe_bpe_encode_words: pre-tokenise, then BPE per word); many
documents in one call through gbpe_bpe_encode_words_batch.  With special tokens
(gbpe_bpe_encode_special*): strings such as <|endoftext|> are matched on the raw
bytes and become one token each; the text between them is encoded as if alone.

The result is exact for every merge list whose new ids are at least 256 and distinct
(in any order; repeated pairs, the pair (0, 0) and operands created later or never
included).  Any other list (a new id below 256, or one an earlier entry of the list
gave) raises GpuBpeError with GBPE_E_INVALID at construction; the message names the
merge.  A list that holds a value above 0xFFFF goes through gbpe_bpe_upload_wide
(ids up to GBPE_BPE_MAX_ID = 0xFFFFFF: the 100K to 200K vocabularies); every encode
call is the same, and a value above that bound is GBPE_E_INVALID too."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

WORDS_MODES = {"heuristic": _lib.GBPE_WORDS_HEURISTIC, "gpt4": _lib.GBPE_WORDS_GPT4,
               "cl100k": _lib.GBPE_WORDS_CL100K, "o200k_base": _lib.GBPE_WORDS_O200K}


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
            raise _bad_words(f"words must be None, 'heuristic', 'gpt4', 'cl100k' or 'o200k_base', not {words!r}")
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


def checked_special_tokens(special_tokens):
    """A special table checked on the host (no device, no library): the mapping of
    ``bytes`` or ``str`` (UTF-8) to id as ``[(bytes, id), ...]`` in the mapping's
    order.  No entry or more than 254, an empty string or one above 128 bytes, the
    same bytes twice (a ``str`` and its ``bytes``), a key of another type or an id
    outside u32 raises GpuBpeError with GBPE_E_INVALID, the status
    gbpe_specials_upload gives."""
    def bad(msg):
        return _lib.GpuBpeError(_lib.GBPE_E_INVALID, f"special tokens: {msg} (status {_lib.GBPE_E_INVALID})")
    if not hasattr(special_tokens, "items"):
        raise bad("give a mapping of bytes or str to id")
    table, seen = [], set()
    for key, tid in special_tokens.items():
        if isinstance(key, str):
            raw = key.encode("utf-8")
        elif isinstance(key, (bytes, bytearray)):
            raw = bytes(key)
        else:
            raise bad(f"a key must be bytes or str, not {type(key).__name__}")
        if not 1 <= len(raw) <= _lib.GBPE_SPECIAL_MAX_BYTES:
            raise bad(f"{raw[:16]!r}... has {len(raw)} bytes (1 to {_lib.GBPE_SPECIAL_MAX_BYTES})")
        if raw in seen:
            raise bad(f"{raw!r} is given twice")
        if isinstance(tid, bool) or not isinstance(tid, (int, np.integer)) or not 0 <= int(tid) <= 0xFFFFFFFF:
            raise bad(f"the id of {raw!r} must be an integer in [0, 2^32)")
        seen.add(raw)
        table.append((raw, int(tid)))
    if not 1 <= len(table) <= _lib.GBPE_SPECIALS_MAX:
        raise bad(f"{len(table)} entries (1 to {_lib.GBPE_SPECIALS_MAX})")
    return table


class MergeEncoder:
    def __init__(self, engine, merges, special_tokens=None):
        self._engine = engine
        self._merges = [list(m[:3]) for m in merges]
        self._sp = None
        self.special_tokens = checked_special_tokens(special_tokens) if special_tokens is not None else None
        lib = _lib.load()
        for r, m in enumerate(self._merges):   # (what does not fit a u32 cannot reach the library's own check)
            if not all(0 <= int(v) <= 0xFFFFFFFF for v in m):
                raise _lib.GpuBpeError(_lib.GBPE_E_INVALID, f"bpe upload: merge {r} has an id above "
                                       f"0x{_lib.GBPE_BPE_MAX_ID:X} (status {_lib.GBPE_E_INVALID})")
        arr = np.ascontiguousarray(np.asarray(self._merges, dtype=np.uint32).reshape(-1, 3))
        # ids above 0xFFFF take the wide rank table (gbpe_bpe_upload_wide, up to GBPE_BPE_MAX_ID)
        self.wide = bool(arr.size) and int(arr.max()) > 0xFFFF
        upload = lib.gbpe_bpe_upload_wide if self.wide else lib.gbpe_bpe_upload
        h = C.c_void_p()
        _lib.check(upload(engine.device, arr.ctypes.data_as(_lib.u32p), arr.shape[0], C.byref(h)), engine.device,
                   "bpe upload")
        self._h = h
        if self.special_tokens is not None:
            raw = np.frombuffer(b"".join(k for k, _ in self.special_tokens), dtype=np.uint8)
            offs = np.zeros(len(self.special_tokens) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(k) for k, _ in self.special_tokens], dtype=np.uint64)
            ids = np.asarray([t for _, t in self.special_tokens], dtype=np.uint32)
            sp = C.c_void_p()
            _lib.check(lib.gbpe_specials_upload(engine.device, raw.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(_lib.u64p),
                                                ids.ctypes.data_as(_lib.u32p), ids.shape[0], C.byref(sp)),
                       engine.device, "specials upload")
            self._sp = sp

    def _special(self, special):
        """The table a call uses: ``special`` None applies the encoder's when it has
        one, False applies none, True insists on one."""
        if special is None:
            return self._sp
        if not special:
            return None
        if self._sp is None:
            raise _lib.GpuBpeError(_lib.GBPE_E_INVALID,
                                   f"bpe encode: special=True on an encoder without special_tokens "
                                   f"(status {_lib.GBPE_E_INVALID})")
        return self._sp

    def find_special(self, data, offsets=None) -> np.ndarray:
        """gbpe_specials_mark of ``data`` (``offsets``: of its documents,
        ``flatten_documents``'s; a list is its documents): np.uint8 per byte, 0 on an ordinary byte, 1 + index
        into the table at an accepted special's first byte, 255 on its other bytes."""
        sp = self._special(True)
        if offsets is None and isinstance(data, (bytes, bytearray, memoryview, np.ndarray)):
            buf, offs, n_docs = np.frombuffer(bytes(data), dtype=np.uint8), None, 0
        else:
            from .tokenizer import flatten_documents
            buf, offs = flatten_documents(data, offsets)
            n_docs = int(offs.shape[0]) - 1
        mark = np.zeros(buf.shape[0], dtype=np.uint8)
        ctx = self._engine.device
        _lib.check(_lib.load().gbpe_specials_mark(ctx, sp, buf.ctypes.data_as(C.c_void_p) if buf.shape[0] else None,
                                                  buf.shape[0], offs.ctypes.data_as(_lib.u64p) if offs is not None else None,
                                                  n_docs, mark.ctypes.data_as(C.c_void_p) if buf.shape[0] else None),
                   ctx, "specials mark")
        return mark

    def encode_bytes(self, data, word_starts=None, words=None, special=None) -> np.ndarray:
        """Tokens of ``data``.  ``word_starts`` (a mask, one entry per byte) or
        ``words`` ('heuristic' / 'gpt4' / 'cl100k', the exact cl100k_base split / 'o200k_base', the exact o200k_base split: the
        mask computed on the device) bound
        every token to one word; with neither the merges apply to the whole
        string.  An encoder with ``special_tokens`` gives each accepted special
        its id and encodes the pieces between them alone; ``special=False`` gives
        the result without the table."""
        data = bytes(data)
        mode, mask = checked_word_starts(len(data), word_starts, words)
        sp = self._special(special)
        lib = _lib.load()
        ctx = self._engine.device
        out = np.empty(max(1, len(data)), dtype=np.uint32)
        n = C.c_uint64()
        buf = C.create_string_buffer(data, len(data)) if data else None
        if sp is not None:
            if mask is not None and not len(data):
                mask = np.zeros(1, dtype=np.uint8)   # (a non-NULL pointer goes with the mode)
            _lib.check(lib.gbpe_bpe_encode_special(ctx, self._h, sp, buf, len(data),
                                                   mask.ctypes.data_as(C.c_void_p) if mask is not None else None, mode,
                                                   out.ctypes.data_as(_lib.u32p), out.shape[0], C.byref(n)),
                       ctx, "bpe encode (special)")
        elif mode == _lib.GBPE_WORDS_NONE:
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

    def encode_batch(self, docs, offsets=None, word_starts=None, words=None, special=None):
        """Many documents in one call (gbpe_bpe_encode_words_batch): returns
        ``(tokens, offsets)``, document d's tokens being
        ``tokens[offsets[d]:offsets[d + 1]]`` — exactly ``encode_bytes`` of that
        document alone in the same mode.  ``docs`` and ``offsets`` are
        ``flatten_documents``'s; ``word_starts`` is one mask over the
        concatenation (a document's first byte starts a word whatever it says);
        ``special`` as in ``encode_bytes`` (a special lies inside one document)."""
        from .tokenizer import flatten_documents
        buf, offs = flatten_documents(docs, offsets)
        n, n_docs = int(buf.shape[0]), int(offs.shape[0]) - 1
        mode, mask = checked_word_starts(n, word_starts, words)
        sp = self._special(special)
        lib = _lib.load()
        ctx = self._engine.device
        out = np.empty(max(1, n), dtype=np.uint32)
        tok_off = np.zeros(n_docs + 1, dtype=np.uint64)
        cnt = C.c_uint64()
        if mask is not None and not n:
            mask = np.zeros(1, dtype=np.uint8)   # (a non-NULL pointer goes with the mode)
        args = (buf.ctypes.data_as(C.c_void_p), n, offs.ctypes.data_as(_lib.u64p), n_docs,
                mask.ctypes.data_as(C.c_void_p) if mask is not None else None, mode, out.ctypes.data_as(_lib.u32p),
                out.shape[0], tok_off.ctypes.data_as(_lib.u64p), C.byref(cnt))
        if sp is not None:
            _lib.check(lib.gbpe_bpe_encode_special_batch(ctx, self._h, sp, *args), ctx, "bpe encode batch (special)")
        else:
            _lib.check(lib.gbpe_bpe_encode_words_batch(ctx, self._h, *args), ctx, "bpe encode batch")
        return out[: cnt.value].copy(), tok_off

    def _spans(self, buf, n, offs, n_docs, mode, mask, sp):
        """gbpe_bpe_encode_spans over np.uint8 ``buf``: (tokens, tok_off or None, starts with n appended)."""
        lib = _lib.load()
        ctx = self._engine.device
        out = np.empty(max(1, n), dtype=np.uint32)
        starts = np.empty(max(1, n) + 1, dtype=np.uint64)
        tok_off = np.zeros(n_docs + 1, dtype=np.uint64) if offs is not None else None
        cnt = C.c_uint64()
        if mask is not None and not n:
            mask = np.zeros(1, dtype=np.uint8)   # (a non-NULL pointer goes with the mode)
        _lib.check(lib.gbpe_bpe_encode_spans(ctx, self._h, sp, buf.ctypes.data_as(C.c_void_p) if n else None, n,
                                             offs.ctypes.data_as(_lib.u64p) if offs is not None else None, n_docs,
                                             mask.ctypes.data_as(C.c_void_p) if mask is not None else None, mode,
                                             out.ctypes.data_as(_lib.u32p), starts.ctypes.data_as(_lib.u64p), out.shape[0],
                                             tok_off.ctypes.data_as(_lib.u64p) if offs is not None else None,
                                             C.byref(cnt)), ctx, "bpe encode (spans)")
        k = int(cnt.value)
        starts[k] = n
        return out[:k].copy(), tok_off, starts[: k + 1].copy()

    def encode_bytes_spans(self, data, word_starts=None, words=None, special=None):
        """``encode_bytes`` with the byte span of every token (gbpe_bpe_encode_spans):
        returns ``(tokens, starts)``.  ``starts`` is np.uint64[len(tokens) + 1], the
        index of each token's first byte and ``len(data)`` at the end, so
        ``data[starts[i]:starts[i + 1]]`` are token i's bytes; a special's token covers
        the special's bytes.  Arguments and checks are ``encode_bytes``'s."""
        data = bytes(data)
        mode, mask = checked_word_starts(len(data), word_starts, words)
        sp = self._special(special)
        tokens, _, starts = self._spans(np.frombuffer(data, dtype=np.uint8), len(data), None, 0, mode, mask, sp)
        return tokens, starts

    def encode_batch_spans(self, docs, offsets=None, word_starts=None, words=None, special=None):
        """``encode_batch`` with the byte span of every token: returns
        ``(tokens, offsets, starts)``; ``starts`` as in ``encode_bytes_spans``, counted
        in the concatenation of the documents.  A non-empty document d's first token
        starts at its first byte: ``starts[offsets[d]]`` is its byte offset."""
        from .tokenizer import flatten_documents
        buf, offs = flatten_documents(docs, offsets)
        n, n_docs = int(buf.shape[0]), int(offs.shape[0]) - 1
        mode, mask = checked_word_starts(n, word_starts, words)
        sp = self._special(special)
        return self._spans(buf, n, offs, n_docs, mode, mask, sp)

    def encode(self, text, word_starts=None, words=None, special=None) -> dict:
        """{tokens, text} like TokenizerManager.encode's result (tokenizer-manager.js:60)."""
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        return {"tokens": self.encode_bytes(data, word_starts, words, special).tolist(), "text": text}

    def destroy(self):
        if self._sp:
            _lib.load().gbpe_specials_free(self._sp)
            self._sp = None
        if self._h:
            _lib.load().gbpe_bpe_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001
            pass
