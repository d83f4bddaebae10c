"""Reference of the special tokens of the merge-rank encode — TEST INFRASTRUCTURE ONLY.

The contract in plain Python: scan the raw bytes of a document left to right; where one
or more specials match take the longest and resume just past it, otherwise advance one
byte.  The accepted specials cut the document into pieces; the tokens are, in order,
encode_words_ref of each piece ALONE in the call's mode and each special's id.  Shared
by test_special_host.py, test_gpu_special.py and test_js_special.py.
"""
import numpy as np

import bpe_oracle as O  # noqa: F401  (the oracle behind encode_words_ref)
from bpe_words_batch_ref import GPT4, HEUR, MASK, NONE, doc_mask, doc_offsets, random_cuts, split  # noqa: F401
from bpe_words_ref import encode_words_ref, model, text

# the corpus recipe of the issue
TABLE = [b"<|endoftext|>", b"EOT", b"007", b"re"]
IDS = [50000, 50001, 50002, 50003]


def find_specials(data, specials):
    """[(position, index)] of the accepted specials of one document."""
    data = bytes(data)
    out, i = [], 0
    while i < len(data):
        best = -1
        for k, s in enumerate(specials):
            if data.startswith(s, i) and (best < 0 or len(s) > len(specials[best])):
                best = k
        if best < 0:
            i += 1
        else:
            out.append((i, best))
            i += len(specials[best])
    return out


def mark_ref(docs, specials):
    """gbpe_specials_mark's array over the concatenation of `docs` (bytes: one document)."""
    if isinstance(docs, (bytes, bytearray)):
        docs = [bytes(docs)]
    parts = []
    for doc in docs:
        m = np.zeros(len(doc), np.uint8)
        for pos, k in find_specials(doc, specials):
            m[pos:pos + len(specials[k])] = 255
            m[pos] = 1 + k
        parts.append(m)
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def pieces(doc, specials):
    """[(start, end, index or None)] covering one document: pieces (None) and specials, in order."""
    out, at = [], 0
    for pos, k in find_specials(doc, specials):
        if pos > at:
            out.append((at, pos, None))
        out.append((pos, pos + len(specials[k]), k))
        at = pos + len(specials[k])
    if at < len(doc):
        out.append((at, len(doc), None))
    return out


def encode_special_ref(docs, merges, specials, ids, mode, mask=None):
    """(tokens, tok_off): per document, each piece alone through encode_words_ref in `mode`
    and each special's id; `mask` (mode MASK) is one mask over the concatenation."""
    offs = doc_offsets(docs)
    tokens, tok_off = [], [0]
    for d, doc in enumerate(docs):
        doc, base = bytes(doc), int(offs[d])
        for a, b, k in pieces(doc, specials):
            if k is not None:
                tokens.append(ids[k])
                continue
            own = None if mask is None else np.asarray(mask)[base + a:base + b]
            tokens += encode_words_ref(doc[a:b], merges, doc_mask(doc[a:b], mode, own))
        tok_off.append(len(tokens))
    return tokens, tok_off


def piece_mask_ref(doc, specials, mode):
    """The word starts of one document under the contract: each piece's own mask, 0 under the specials."""
    m = np.zeros(len(doc), np.uint8)
    for a, b, k in pieces(doc, specials):
        if k is None:
            m[a:b] = doc_mask(doc[a:b], mode)
            m[a] = 1
    return m


def forced_mask_ref(doc, specials, mode):
    """The shortcut the contract rules out: the whole buffer's mask with the specials' edges forced."""
    m = doc_mask(doc, mode).copy()
    for a, b, k in pieces(doc, specials):
        if k is None:
            m[a] = 1
        else:
            m[a:b] = 0
    return m


def recipe():
    """(input bytes, merges) of the corpus recipe: 296 documents of synthetic code, each followed by
    one of TABLE in turn."""
    data = text("code", 53)
    docs = split(data, random_cuts(data, 300, seed=7))
    return b"".join(d + TABLE[i % 4] for i, d in enumerate(docs)), model("code", 53)


def chain_model(data, specials):
    """The device's two steps on the host: candidates (longest match at each byte), then from every
    candidate no earlier candidate's span covers (an anchor) the chain up to the next anchor.
    Returns (accepted [(position, index)], writes per byte)."""
    data = bytes(data)
    n = len(data)
    cand = [-1] * n
    for i in range(n):
        for k, s in enumerate(specials):
            if data.startswith(s, i) and (cand[i] < 0 or len(s) > len(specials[cand[i]])):
                cand[i] = k

    def anchor(i):
        return not any(cand[j] >= 0 and j + len(specials[cand[j]]) > i for j in range(max(0, i - 127), i))

    got, writes = [], [0] * n
    for i0 in range(n):
        if cand[i0] < 0 or not anchor(i0):
            continue
        i = i0
        while True:
            p = i + len(specials[cand[i]])
            got.append((i, cand[i]))
            for j in range(i, p):
                writes[j] += 1
            q = p
            while q < min(p + 127, n) and cand[q] < 0:
                q += 1
            if q >= min(p + 127, n) or anchor(q):
                break
            i = q
    return sorted(got), writes
