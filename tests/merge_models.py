"""Adversarial merge lists for the merge-rank encoder — TEST INFRASTRUCTURE ONLY.

gpubpe.h promises gbpe_bpe_upload / gbpe_bpe_encode* to be exact for every merge list
whose new ids are at least 256 and distinct.  model_case(seed) draws small lists from
the corners of that domain (byte 0 and the pair (0, 0), ids in any order up to 0xFFFF,
repeated pairs whose second id is dead, operands created later or never, self-pairs,
"closed" alphabets whose texts are one segment and so reach the heap path); big_model()
fills the rank table to the highest load its sizing rule allows.  The references are
the oracle's encode_merge_order (tokenizer-manager.js:13-61) for small texts and
np_merge_order, the same passes in numpy, for long ones.  lowest_rank_encode restates
the LIBRARY's algorithm on the host (upload filter, then lowest rank first), with the
wrong filters as variants: test_merge_models.py uses them to show that the cases tell
a right encoder from a wrong one.  Shared by test_merge_models.py,
test_gpu_merge_models.py and test_gpu_merge_encode.py.
"""
import functools

import numpy as np

import bpe_oracle as O
from bpe_words_ref import word_bounds

POOL = [0x00, 0x20, ord("a"), ord("b"), 0xC3, 0xFF]
MAX_MERGES = 30
SEEDS = list(range(120))
# the models with the entry (0, 0), those with byte 0 but without that entry, and the rest.  An encoder
# that drops the pair (0, 0) fails the first group; one whose table reads an empty slot as that pair
# (and so "merges" two NUL bytes into one wherever a segment holds them) fails the second as well.
def _flags(seed):
    """(closed, byte 0 in the alphabet, the entry (0, 0)): a closed model with byte 0 holds every pair, (0, 0) too."""
    closed, nul = seed % 3 == 0, (seed // 3) % 3 == 0
    return closed, nul, nul and (closed or (seed // 9) % 2 == 0)


GROUPS = {"nul_nul": [s for s in SEEDS if _flags(s)[2]]}
GROUPS["nul"] = [s for s in SEEDS if _flags(s)[1] and not _flags(s)[2]]
GROUPS["no_nul"] = [s for s in SEEDS if not _flags(s)[1]]
LONG_LENGTHS = [1024, 1025, 1026, 2051]   # around ME_LONG = 1024: the last two segments of 1025 / 1026 under starts [0, 1025]
MASK_TEXT_LEN = 700                       # three 256-byte chunks: words of a 0.1 mask straddle them
SPECIAL, SPECIAL_ID = b"<|e|>", 999       # (no byte of it is in POOL)

# lists that upload rejects (a new id that is not fresh), with what the reference makes of them
A_, B_, C_, D_, E_ = (ord(c) for c in "abcde")
REJECTED = [
    ([[A_, B_, 99], [99, D_, 256]], b"abd", [256]),                       # a new id that is a byte's
    ([[A_, B_, 256], [C_, D_, 256], [256, E_, 257]], b"cde", [257]),      # a new id given twice
]
FEEDS_BACK = ([[A_, B_, 256], [C_, C_, A_]], b"ccb", [A_, B_])         # rank 1 makes an operand of rank 0, too late
NUL_NUL = ([[0, 0, 256]], b"\0\0\0", [256, 0])                            # accepted: (0, 0) merges


# ── references ─────────────────────────────────────────────────────────────

def _np_passes(tok, merges):
    for a, b, nid in (m[:3] for m in merges):
        if tok.size < 2:
            break
        idx = np.flatnonzero((tok[:-1] == a) & (tok[1:] == b))
        if idx.size == 0:
            continue
        if a == b:
            k = np.arange(idx.size)
            start = np.ones(idx.size, bool)
            start[1:] = idx[1:] != idx[:-1] + 1
            rs = np.maximum.accumulate(np.where(start, k, 0))
            idx = idx[(k - rs) % 2 == 0]
        tok[idx] = nid
        rm = np.zeros(tok.size, bool)
        rm[idx + 1] = True
        tok = tok[~rm]
    return tok


def np_merge_order(data: bytes, merges) -> np.ndarray:
    """numpy form of the oracle's encode_merge_order (one pass per merge, every
    occurrence left to right; runs of a == b pair up from their left end)."""
    return _np_passes(np.frombuffer(bytes(data), np.uint8).astype(np.int64), merges)


def np_merge_order_words(data: bytes, merges, ws) -> np.ndarray:
    """np_merge_order of every word of the mask ws alone, concatenated: one stream with a
    -1 in front of each word, which no pair matches across."""
    data = bytes(data)
    starts = np.asarray(word_bounds(len(data), ws)[:-1], np.int64)
    tok = np.insert(np.frombuffer(data, np.uint8).astype(np.int64), starts, -1)
    tok = _np_passes(tok, merges)
    return tok[tok >= 0]


def upload_filter(merges, live="first"):
    """The rank table gbpe_bpe_upload builds: {(a, b): (rank, new id)}.  An entry is live when
    both operands exist (a byte, or the new id of an earlier live entry) and its pair was
    not live before.  The wrong filters: live="all" skips the operand test, live="last"
    lets a repeated pair's later entry replace the earlier one."""
    exists = set(range(256))
    table = {}
    for r, (a, b, nid) in enumerate(m[:3] for m in merges):
        if live != "all" and (a not in exists or b not in exists):
            continue
        if (a, b) in table and live != "last":
            continue
        table[(a, b)] = (r, nid)
        exists.add(nid)
    return table


def lowest_rank_encode(data: bytes, merges, live="first"):
    """The library's walk on the host: while some adjacent pair is in the table, apply the
    one of lowest rank to all its occurrences, left to right."""
    table = upload_filter(merges, live)
    tok = list(bytes(data))
    while len(tok) >= 2:
        best = min((table[p] + p for p in zip(tok[:-1], tok[1:]) if p in table), default=None)
        if best is None:
            break
        _, nid, a, b = best
        out, i = [], 0
        while i < len(tok):
            if i + 1 < len(tok) and tok[i] == a and tok[i + 1] == b:
                out.append(nid)
                i += 2
            else:
                out.append(tok[i])
                i += 1
        tok = out
    return tok


def cross_pairs(merges):
    """The byte boundaries (u, v) some live merge crosses (the encoder's cross table)."""
    first = {b: b for b in range(256)}
    last = dict(first)
    out = set()
    for (a, b), (_, nid) in sorted(upload_filter(merges).items(), key=lambda kv: kv[1][0]):
        out.add((last[a], first[b]))
        first[nid], last[nid] = first[a], last[b]
    return out


def segments(data: bytes, merges):
    """Lengths of the segments the encoder cuts `data` into (no mask)."""
    cross = cross_pairs(merges)
    cuts = [0] + [i for i in range(1, len(data)) if (data[i - 1], data[i]) not in cross] + [len(data)]
    return [b - a for a, b in zip(cuts[:-1], cuts[1:])]


# ── the small models ───────────────────────────────────────────────────────

@functools.lru_cache(maxsize=None)
def model_case(seed):
    """{merges, texts, mask_text, alphabet, closed, nul_nul, dead_ids, later_ids, ffff}.

    seed % 3 == 0: closed (every byte pair of the alphabet is an entry, so a text over the
    alphabet is one segment); (seed // 3) % 3 == 0: byte 0 is in the alphabet, and of those
    the closed ones and those with (seed // 9) % 2 == 0 carry the entry (0, 0), the others only
    (0, x) / (x, 0);
    seed % 5 == 2: the first entry's id is 0xFFFF, and (0xFFFF, 0xFFFF) and (0xFFFF, byte)
    are later entries.  texts: lengths 0, 1, 2, 3, three random ones <= 64, closed models
    LONG_LENGTHS too; mask_text: MASK_TEXT_LEN bytes for the masked and batch calls."""
    rng = np.random.default_rng(1000 + seed)
    closed, nul, nul_nul = _flags(seed)
    ffff = seed % 5 == 2
    k = int(rng.integers(1, 5))
    if nul and not nul_nul:
        k = max(k, 2)   # (0, x) needs an x
    rest = [int(b) for b in rng.permutation([b for b in POOL if b != 0])]
    alpha = [0] + rest[: k - 1] if nul else rest[:k]

    # the entries' ids: a shuffled pool that holds 256 and 0xFFFF; the ids past MAX_MERGES are never given
    ids = [256, 0xFFFF] + [int(v) for v in rng.choice(np.arange(257, 0xFFFF), MAX_MERGES + 6, replace=False)]
    ids = [int(v) for v in rng.permutation(ids)]
    if ffff:
        ids.remove(0xFFFF)
        ids.insert(0, 0xFFFF)
    never = ids[MAX_MERGES:]

    byte_pairs = [(a, b) for a in alpha for b in alpha]
    forced = []   # pairs that must be entries, each at a random rank
    if closed:
        forced = [byte_pairs[i] for i in rng.permutation(len(byte_pairs))]
    if nul_nul and (0, 0) not in forced:
        forced.append((0, 0))
    if nul and not nul_nul:
        x = alpha[1]
        forced += [p for p in ((0, x), (x, 0)) if p not in forced]
    n_free = int(rng.integers(0, MAX_MERGES + 1 - len(forced))) if len(forced) < MAX_MERGES else 0
    if ffff:   # entry 0 creates 0xFFFF from a byte pair, the last two entries use it
        n_free = max(n_free, 3)
    n = len(forced) + n_free
    open_ranks = np.asarray([r for r in range(n) if not (ffff and r in (0, n - 2, n - 1))], np.int64)
    is_forced = np.zeros(n, bool)
    is_forced[rng.permutation(open_ranks)[: len(forced)]] = True

    merges, exists, seen, created = [], set(range(256)), set(), []
    dead_ids, later_ids, pending, next_pair = [], [], [], None
    forced = list(forced)

    def pick():   # an existing token, the lately created ones more often than the bytes
        if created and rng.random() < 0.6:
            return created[int(rng.integers(max(0, len(created) - 4), len(created)))]
        return alpha[int(rng.integers(0, k))]

    for r in range(n):
        nid = ids[r]
        u = rng.random()
        if ffff and r == 0:
            pair = (alpha[0], alpha[-1])
        elif is_forced[r]:
            pair = forced.pop(0)
        elif ffff and r == n - 2:
            pair = (0xFFFF, 0xFFFF)
        elif ffff and r == n - 1:
            pair = (0xFFFF, alpha[0])
        elif next_pair is not None:                # the pair that creates the entry before's operand, too late
            pair, next_pair = next_pair, None
        elif pending:                              # the dead id of a repeated pair as an operand
            d = pending.pop()
            pair = (d, pick()) if rng.random() < 0.5 else (pick(), d)
        elif u < 0.10 and seen:                    # an earlier pair again, under a fresh id
            pair = sorted(seen)[int(rng.integers(0, len(seen)))]
            dead_ids.append(nid)
            pending.append(nid)
        elif u < 0.20:                             # an operand created later, or never
            v = rng.random()
            if v < 0.5 and r + 1 < n:              # ... by the next entry, from bytes the texts hold
                later = ids[r + 1]
                fresh = [p for p in byte_pairs if p not in seen]
                next_pair = fresh[int(rng.integers(0, len(fresh)))] if fresh else (pick(), pick())
            elif v < 0.75 and r + 1 < n:
                later = ids[int(rng.integers(r + 1, n))]
            else:
                later = never[int(rng.integers(0, len(never)))]
            later_ids.append(later)
            pair = (later, pick()) if rng.random() < 0.5 else (pick(), later)
        elif u < 0.35:                             # a self-pair
            t = pick()
            pair = (t, t)
        else:                                      # a pair of earlier tokens
            pair = (pick(), pick())
        if nul and not nul_nul and pair == (0, 0):   # these models pair byte 0 with others only
            pair = (0, alpha[1])
        merges.append([pair[0], pair[1], nid])
        if pair[0] in exists and pair[1] in exists and pair not in seen:
            seen.add(pair)
            exists.add(nid)
            created.append(nid)

    def text(length):
        return bytes(np.asarray(alpha, np.uint8)[rng.integers(0, k, length)]) if length else b""

    lengths = [0, 1, 2, 3] + [int(v) for v in rng.integers(4, 65, 3)]
    texts = [text(v) for v in lengths]
    if ffff:   # the first entry's pair four times over, so that (0xFFFF, 0xFFFF) can fire
        texts[-1] = bytes([alpha[0], alpha[-1]] * 4) + texts[-1][:56]
    if closed:
        texts += [text(v) for v in LONG_LENGTHS]
    return {"merges": merges, "texts": texts, "mask_text": text(MASK_TEXT_LEN), "alphabet": alpha, "closed": closed,
            "nul_nul": nul_nul, "dead_ids": dead_ids, "later_ids": later_ids, "ffff": ffff}


def reference(data: bytes, merges):
    """The expected tokens of the whole-string encode: the oracle, or for a long text its numpy form."""
    if len(data) <= 64:
        return O.encode_merge_order(bytes(data), merges)
    return np_merge_order(data, merges).tolist()


def random_mask(n, seed, density=0.1):
    return (np.random.default_rng(seed).random(n) < density).astype(np.uint8)


def batch_docs(case):
    """The documents of a model's batch call (its texts and mask_text) and the caller's mask over
    them: density 0.1, but a closed model's LONG_LENGTHS documents keep their long segments (one
    start at byte 1025 of the last, which cuts it into 1025 and 1026 bytes)."""
    docs = list(case["texts"]) + [case["mask_text"]]
    mask = random_mask(sum(len(d) for d in docs), 7)
    at = 0
    for d in docs:
        if len(d) >= LONG_LENGTHS[0]:
            mask[at:at + len(d)] = 0
            if len(d) == LONG_LENGTHS[-1]:
                mask[at + 1025] = 1
        at += len(d)
    return docs, mask


def special_docs(case, seed):
    """batch_docs with SPECIAL inside every document (within its first 20 bytes, so that a long
    piece stays long), in front of every third and behind every second."""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for i, d in enumerate(batch_docs(case)[0]):
        at = int(rng.integers(0, min(len(d), 20) + 1))
        d = d[:at] + SPECIAL + d[at:]
        if i % 3 == 0:
            d = SPECIAL + d
        if i % 2 == 0:
            d = d + SPECIAL
        out.append(d)
    return out


# ── the large model ────────────────────────────────────────────────────────

BIG_LEVEL1, BIG_LEVEL2, BIG_TEXT_LEN, BIG_WORD = 65_000, 280, 6_000, 12


@functools.lru_cache(maxsize=None)
def big_model():
    """(merges np.uint32[65280, 3], text): 65,000 byte pairs (first bytes 0..253, random rank
    order; the 24 pairs left out begin with 253) under a random permutation of the ids
    256..0xFFFF, then 280 pairs of those tokens taken from adjacent tokens of the text's
    first-level encoding.  The text is 6,000 bytes in 0..252: every boundary is crossed, so it
    is one segment.  65,280 entries size the table at 131,072 slots: load 0.498."""
    rng = np.random.default_rng(65)
    ids = rng.permutation(np.arange(256, 0x10000))
    assert ids.size == BIG_LEVEL1 + BIG_LEVEL2
    low = np.arange(253 * 256)                                       # first bytes 0..252: all of them
    high = 253 * 256 + rng.permutation(256)[: BIG_LEVEL1 - low.size]
    pairs = rng.permutation(np.concatenate([low, high]))
    m1 = np.stack([pairs >> 8, pairs & 255, ids[:BIG_LEVEL1]], axis=1)
    text = bytes(rng.integers(0, 253, BIG_TEXT_LEN).astype(np.uint8))
    t1 = np_merge_order(text, m1)
    seen, m2 = set(), []
    for i in range(0, t1.size - 1, 2):                               # disjoint positions: one merge does not eat the next one's operand
        p = (int(t1[i]), int(t1[i + 1]))
        if p[0] >= 256 and p[1] >= 256 and p not in seen and len(m2) < BIG_LEVEL2:
            seen.add(p)
            m2.append([p[0], p[1], int(ids[BIG_LEVEL1 + len(m2)])])
    assert len(m2) == BIG_LEVEL2
    return np.concatenate([m1, np.asarray(m2)]).astype(np.uint32), text


@functools.lru_cache(maxsize=None)
def big_reference():
    """(whole-string tokens, tokens under words of BIG_WORD bytes, that mask) of big_model()."""
    merges, text = big_model()
    ws = np.zeros(len(text), np.uint8)
    ws[::BIG_WORD] = 1
    m = merges.astype(np.int64)
    return np_merge_order(text, m), np_merge_order_words(text, m, ws), ws
