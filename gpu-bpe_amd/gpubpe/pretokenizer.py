"""GpuPreTokenizer — the reference's PreTokenizer (src/wasm/pre_tokenizer.mjs:402-509)
on the device.

``pre_tokenize_bytes(bytes)`` / ``pre_tokenize(text)`` return
``{"bytes": ..., "wordStarts": ...}`` like preTokenizeBytes / preTokenize; the
word starts come from gbpe_pretokenize_gpt4 (GPT-4 rules, findWordBoundaries
:226-292).  Input must already be NFC (the reference normalises first; NFC
text is unchanged by that step).  ``BPETrainer.train(pre_tokenizer=...)``
accepts it like the reference trainer accepts its PreTokenizer (trainer.js:62-99).

``rules="cl100k"`` on any of the calls gives the word starts of the cl100k_base
split pattern instead (gbpe_pretokenize_cl100k); no normalisation
belongs to it.  ``rules="o200k_base"`` gives those of the o200k_base split pattern
(gbpe_pretokenize_o200k) in the same way.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


RULES = ("gpt4", "cl100k", "o200k_base")
_SYMBOL = {"gpt4": "gpt4", "cl100k": "cl100k", "o200k_base": "o200k"}   # gbpe_pretokenize_<symbol>


def _entry(rules: str, suffix: str = ""):
    if rules not in RULES:
        raise ValueError(f"rules must be 'gpt4', 'cl100k' or 'o200k_base', not {rules!r}")
    return getattr(_lib.load(), f"gbpe_pretokenize_{_SYMBOL[rules]}{suffix}")


class GpuPreTokenizer:
    def __init__(self, engine):
        self._engine = engine

    def pre_tokenize_bytes(self, raw, rules: str = "gpt4") -> dict:
        pretokenize = _entry(rules)
        data = bytes(raw)
        ws = np.zeros(len(data), dtype=np.uint8)
        if data:
            ctx = self._engine.device
            buf = C.create_string_buffer(data, len(data))
            _lib.check(pretokenize(ctx, buf, len(data), ws.ctypes.data_as(C.c_void_p)), ctx, "pretokenize")
        return {"bytes": data, "wordStarts": ws}

    def pre_tokenize_batch(self, docs, offsets=None, rules: str = "gpt4"):
        """Word starts of many documents in one call (gbpe_pretokenize_gpt4_batch,
        gbpe_pretokenize_cl100k_batch, gbpe_pretokenize_o200k_batch):
        returns ``(mask, offsets)`` over the concatenation, the mask of document d
        being ``mask[offsets[d]:offsets[d + 1]]`` — exactly ``pre_tokenize_bytes``
        of that document alone.  ``docs`` and ``offsets`` are ``flatten_documents``'s.
        The mask is the ``word_starts`` a trainer takes for the concatenation."""
        from .tokenizer import flatten_documents
        pretokenize = _entry(rules, "_batch")
        buf, offs = flatten_documents(docs, offsets)
        n, n_docs = int(buf.shape[0]), int(offs.shape[0]) - 1
        ws = np.zeros(n, dtype=np.uint8)
        if n and n_docs:
            ctx = self._engine.device
            _lib.check(pretokenize(ctx, buf.ctypes.data_as(C.c_void_p), n, offs.ctypes.data_as(_lib.u64p), n_docs,
                                   ws.ctypes.data_as(C.c_void_p)), ctx, "pretokenize batch")
        return ws, offs

    def pre_tokenize(self, text: str, rules: str = "gpt4") -> dict:
        return self.pre_tokenize_bytes(text.encode("utf-8"), rules)

    # reference spelling
    preTokenizeBytes = pre_tokenize_bytes
    preTokenize = pre_tokenize
    preTokenizeBatch = pre_tokenize_batch
