"""Merge lists with ids above 0xFFFF for the merge-rank encoder — TEST INFRASTRUCTURE ONLY.

gbpe_bpe_upload_wide takes ids up to GBPE_BPE_MAX_ID = 0xFFFFFF.  The cases here are built so
that an encoder which still keys a pair by a << 16 | b in 32 bits gives other tokens:

* relabel(): merge_models.py's lists under f(id) = id + 0x10000 * (id % 4) for id >= 256 (bytes
  stay).  f is injective on [256, 0xFFFF], leaves a quarter of the ids narrow and keeps the low 16
  bits, so a truncating implementation sees the narrow model's keys again and collides.  Ranks do
  not change: the expected tokens are f of the narrow model's.
* COLLISIONS: small lists whose live pairs share one packed key, tokens written out by hand.
* packed_key_encode(): that wrong encoder on the host; test_merge_wide.py asserts which cases it fails.
* many_pairs_model(): more entries than the narrow form can hold (ids run past 0xFFFF).

Shared by test_merge_wide.py, test_gpu_merge_wide.py and test_js_merge_wide.py.
"""
import functools

import numpy as np

import merge_models as M

MAX_ID = 0xFFFFFF   # GBPE_BPE_MAX_ID


def f(i):
    i = int(i)
    return i if i < 256 else i + 0x10000 * (i % 4)


def relabel(merges):
    return [[f(v) for v in m[:3]] for m in merges]


def relabel_tokens(tokens):
    return [f(t) for t in tokens]


def f_array(tokens):
    t = np.asarray(tokens, np.int64)
    return np.where(t < 256, t, t + 0x10000 * (t % 4))


A, B, C = ord("a"), ord("b"), ord("c")
# (name, merges, text, expected tokens)
COLLISIONS = [
    # (0x10001, 5) and (1, 5): a's bit 16 falls off the packed key
    ("a_overflows", [[A, B, 0x10001], [0x10001, 5, 0x20000], [1, 5, 0x20001]], b"ab\x05\x01\x05", [0x20000, 0x20001]),
    # (2, 0x10007) and (3, 7): b's bit 16 bleeds into a
    ("b_bleeds", [[A, B, 0x10007], [2, 0x10007, 0x300], [3, 7, 0x301]], b"\x02ab\x03\x07", [0x300, 0x301]),
    ("a_bits_16_23", [[A, B, 0x010100], [B, A, 0x020100], [0x010100, 5, 0x400], [0x020100, 5, 0x401]],
     b"ab\x05ba\x05", [0x400, 0x401]),
    ("b_bits_16_23", [[A, B, 0x010100], [B, A, 0x020100], [3, 0x010100, 0x400], [3, 0x020100, 0x401]],
     b"\x03ab\x03ba", [0x400, 0x401]),
    # 0xFFFF, 0x10000 and the largest id, each as a new id and as an operand that fires
    ("boundary_ids", [[A, B, 0xFFFF], [B, A, 0x10000], [A, A, MAX_ID], [0xFFFF, C, 0x500], [0x10000, C, 0x501],
                      [MAX_ID, C, 0x502]], b"abcbacaac", [0x500, 0x501, 0x502]),
    ("max_id_both_operands", [[A, B, MAX_ID], [MAX_ID, MAX_ID, MAX_ID - 1], [MAX_ID - 1, MAX_ID, 0x100]], b"ababab", [0x100]),
]


def packed_key_encode(data: bytes, merges):
    """The WRONG encoder: M.lowest_rank_encode with the rank table keyed by (a << 16 | b) mod 2^32,
    in the upload (the first entry of a key wins) and in the walk."""
    def key(a, b):
        return ((a << 16) | b) & 0xFFFFFFFF
    exists, table = set(range(256)), {}
    for r, (a, b, nid) in enumerate(m[:3] for m in merges):
        if a not in exists or b not in exists or key(a, b) in table:
            continue
        table[key(a, b)] = (r, nid)
        exists.add(nid)
    tok = list(bytes(data))
    while len(tok) >= 2:
        best = min((table[key(a, b)] + (key(a, b),) for a, b in zip(tok[:-1], tok[1:]) if key(a, b) in table), default=None)
        if best is None:
            break
        _, nid, k = best
        out, i = [], 0
        while i < len(tok):
            if i + 1 < len(tok) and key(tok[i], tok[i + 1]) == k:
                out.append(nid)
                i += 2
            else:
                out.append(tok[i])
                i += 1
        tok = out
    return tok


# ── more entries than 16-bit ids allow ─────────────────────────────────────

MANY_LEVEL1, MANY_LEVEL2, MANY_TEXT_LEN, MANY_SOURCE_LEN = 65_536, 4_000, 6_000, 32_000


@functools.lru_cache(maxsize=None)
def many_pairs_model():
    """(merges np.uint32[69536, 3], text, tokens): all 65,536 byte pairs in random rank order with the
    ids 256, 257, ... (the last 256 of them above 0xFFFF), then 4,000 pairs of those tokens taken as
    in M.big_model() — adjacent tokens at disjoint positions of the first-level encoding of 32,000
    random bytes whose first 6,000 are the text — with the ids that follow.  Every byte boundary is
    crossed, so the text is one segment (the heap path).  tokens: np_merge_order of the text."""
    rng = np.random.default_rng(66)
    pairs = rng.permutation(MANY_LEVEL1)
    m1 = np.stack([pairs >> 8, pairs & 255, 256 + np.arange(MANY_LEVEL1)], axis=1)
    source = bytes(rng.integers(0, 256, MANY_SOURCE_LEN).astype(np.uint8))
    t1 = M.np_merge_order(source, m1)
    seen, m2 = set(), []
    for i in range(0, t1.size - 1, 2):
        p = (int(t1[i]), int(t1[i + 1]))
        if p[0] >= 256 and p[1] >= 256 and p not in seen and len(m2) < MANY_LEVEL2:
            seen.add(p)
            m2.append([p[0], p[1], 256 + MANY_LEVEL1 + len(m2)])
    assert len(m2) == MANY_LEVEL2
    merges = np.concatenate([m1, np.asarray(m2)])
    text = source[:MANY_TEXT_LEN]
    return merges.astype(np.uint32), text, M.np_merge_order(text, merges)


def dense_vocab(merges):
    """(bytes of every id laid end to end, np.uint64 offsets) of a list whose ids are 256, 257, ... in
    order and all live: bytes(id) = bytes(a) + bytes(b) — gbpe_vocab_upload's arguments."""
    entries = [bytes([b]) for b in range(256)]
    for a, b, nid in merges.tolist():
        assert nid == len(entries)
        entries.append(entries[a] + entries[b])
    offs = np.zeros(len(entries) + 1, np.uint64)
    offs[1:] = np.cumsum([len(e) for e in entries])
    return np.frombuffer(b"".join(entries), np.uint8), offs
