"""Reference of the byte spans of the merge-rank encode's tokens — TEST INFRASTRUCTURE ONLY.

The reference's one pass per merge (tokenizer-manager.js:13-61, the oracle's
encode_merge_order) restated with a position beside every token: a token keeps the index of
its first byte while the merges apply, and a merged pair keeps its left operand's.  No
length table is involved, so a special's span does not depend on its id.  spans_ref runs it
per word of each piece between the accepted specials (special_ref.pieces) and per document;
a special is one token at its own start.  Shared by test_bpe_spans_host.py,
test_gpu_bpe_spans.py and test_js_bpe_spans.py.
"""
import numpy as np

import cl100k_ref
from bpe_words_batch_ref import doc_mask, doc_offsets
from bpe_words_ref import word_bounds
from special_ref import pieces

NONE, MASK, HEUR, GPT4, CL100K = range(5)   # GBPE_WORDS_*


def merge_order_spans(data, merges):
    """(tokens, starts relative to data[0]) of one text: one left-to-right pass per merge."""
    tok = list(bytes(data))
    pos = list(range(len(tok)))
    for a, b, nid in (m[:3] for m in merges):
        if len(tok) < 2:
            break
        if a not in tok or b not in tok:   # (the pass would change nothing)
            continue
        out, opos, i, n = [], [], 0, len(tok)
        while i < n:
            opos.append(pos[i])
            if i + 1 < n and tok[i] == a and tok[i + 1] == b:
                out.append(nid)
                i += 2
            else:
                out.append(tok[i])
                i += 1
        tok, pos = out, opos
    return tok, pos


def piece_mask(piece, mode, own=None):
    """The word starts of one piece alone in a GBPE_WORDS_* mode (own: the caller's, for MASK)."""
    if mode == CL100K:
        return cl100k_ref.mask(piece) if piece else np.zeros(0, np.uint8)
    return doc_mask(piece, mode, own)


def spans_ref(docs, merges, specials=(), ids=(), mode=NONE, mask=None):
    """(tokens, starts) of the documents `docs` (a list of bytes): starts[i] is the index of
    token i's first byte in the concatenation.  `mask` (mode MASK) is one mask over the
    concatenation.  Use doc_tok_off for the documents' token offsets."""
    merges = [[int(v) for v in m[:3]] for m in merges]
    specials = list(specials)
    offs = doc_offsets(docs)
    cache = {}
    tokens, starts = [], []
    for d, doc in enumerate(docs):
        doc, base = bytes(doc), int(offs[d])
        for a, b, k in pieces(doc, specials):
            if k is not None:
                tokens.append(int(ids[k]))
                starts.append(base + a)
                continue
            piece = doc[a:b]
            own = None if mask is None else np.asarray(mask)[base + a:base + b]
            wb = word_bounds(len(piece), piece_mask(piece, mode, own))
            for s, e in zip(wb[:-1], wb[1:]):
                w = piece[s:e]
                if w not in cache:
                    cache[w] = merge_order_spans(w, merges)
                t, p = cache[w]
                tokens += t
                starts += [base + a + s + q for q in p]
    return tokens, starts


def doc_tok_off(docs, starts):
    """The documents' token offsets from the tokens' starts: the tokens tile the bytes, so document
    d's first token is the first whose start is at or beyond the document's offset."""
    offs = doc_offsets(docs)
    return np.searchsorted(np.asarray(starts, np.uint64), offs, side="left").tolist()
