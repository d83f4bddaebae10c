"""Vocabularies, corpora and a plain reference for the trie-encode tests —
TEST INFRASTRUCTURE ONLY (no GPU, no library).

encode.hip walks one chunk per lane.  The packed walk (k_trie_walk_v5) reads its
input through one cached 64-byte window at chunk start + (p & ~63), queues completed
16-byte token vectors and stores four at a time; the plain walk (k_trie_walk) caches
one 4-byte word; k_chunk_compact4 moves 256 tokens per chunk per pass, four chunks
per wave.  These generators put a walk at every one of those edges:

``edge_vocab`` / ``holes_vocab`` / ``boundary_vocab`` / ``wide`` / ``empty_root_blob``:
    explicit entry lists (not merges) with tokens longer than one and two windows,
    gaps in the ladder of accepting states, leaves, root children without an id,
    and the largest id on either side of the u16 and the packing limits.
``near_miss``: every prefix of every long token followed by a mismatch — the walk
    runs ahead of its last match and has to back up.
``phase_sweep``: one near-miss probe at every offset of the chunk's windows.
``count_sweep``: one chunk per token count (the store bursts and the compaction
    passes depend on the count alone).
``all_raw`` / ``tails``: a token per byte; inputs that end inside a window.

``ref_encode`` is a dict-of-dicts greedy matcher: deliberately not the oracle's
code (no BFS node arrays, no edge search); test_encode_corpora.py cross-checks the
two.  Its trace gives, per token, where the walk started, where the match ended and
the last byte the walk read — what the coverage conditions are stated in.
"""
from __future__ import annotations

import struct
from math import gcd

A, HASH = 0x61, 0x23
LADDER = (2, 3, 4, 8, 16, 32, 63, 64, 65, 127, 128, 129, 200)
_FILL = b"bcdefghijklmnoprstuvw"       # the long tokens' bodies: none of a, x, y, z, q, #
_PAD = b"0123456789"                   # raw padding: every byte a one-byte leaf at the root

XY70 = b"xy" + (_FILL * 4)[:68]
XY40 = XY70[:40]
XZ130 = b"xz" + (_FILL[::-1] * 7)[:128]
LEAF2 = b"qq"                          # a 2-byte token that nothing extends

_ID = -1                               # key of a node's token id in the reference trie


# ── the plain reference ──────────────────────────────────────────────────────

def ref_trie(vocab) -> dict:
    """{byte: child, ..., _ID: token id}; a later duplicate byte string overwrites
    the id (trie.js), an empty entry is no token."""
    root: dict = {}
    for tid, bs in enumerate(vocab):
        if not bs:
            continue
        node = root
        for b in bs:
            node = node.setdefault(b, {})
        node[_ID] = tid
    return root


def ref_encode(data: bytes, vocab, cs: int):
    """Greedy longest match per chunk of `cs` bytes; an unmatched byte gives its
    value.  `vocab` is an entry list or a ref_trie of one.  Returns (tokens, trace):
    trace[i] = (start, end, far) of token i — the match is data[start:end], and far
    is the last byte index the walk read: the mismatching byte, or the chunk's last."""
    root = vocab if isinstance(vocab, dict) else ref_trie(vocab)
    tokens, trace = [], []
    n = len(data)
    for c0 in range(0, n, cs):
        ce = min(c0 + cs, n)
        pos = c0
        while pos < ce:
            node, tok, end, wp, far = root, None, pos + 1, pos, pos
            while wp < ce:
                far = wp
                node = node.get(data[wp])
                if node is None:
                    break
                wp += 1
                if _ID in node:
                    tok, end = node[_ID], wp
            tokens.append(data[pos] if tok is None else tok)
            trace.append((pos, end, far))
            pos = end
    return tokens, trace


def chunk_counts(trace, cs: int, n: int) -> list:
    """Tokens per chunk, from a trace."""
    counts = [0] * ((n + cs - 1) // cs)
    for start, _, _ in trace:
        counts[start // cs] += 1
    return counts


# ── vocabularies ─────────────────────────────────────────────────────────────

def _bytes256() -> list:
    return [[b] for b in range(256)]


def edge_vocab() -> list:
    """The 256 bytes; an `a` ladder with gaps; `xy` < its 40-byte < its 70-byte
    extension with nothing else on the path; `xz` < a 130-byte extension with
    nothing between; a 2-byte leaf.  Every byte but a, x and q is a one-byte leaf."""
    v = _bytes256()
    v += [[A] * k for k in LADDER]
    v += [list(b"xy"), list(XY40), list(XY70), list(b"xz"), list(XZ130), list(LEAF2)]
    return v


def long_tokens(vocab) -> list:
    """The tokens near_miss probes: every entry of 16 bytes or more."""
    return [bytes(e) for e in vocab if len(e) >= 16]


HOLE_BYTES = (ord("h"), ord("k"))          # no entry of their own, but start longer tokens
NOTHING_BYTES = (ord("z"), 0xFF)           # no entry and start nothing


def holes_vocab() -> list:
    """Entries `hi`, `hit`, `klm` (h, k and `kl` are not tokens), `ab`, `abcd` (`abc`
    is not); the bytes z and 0xFF have no entry at all."""
    v = _bytes256()
    for b in HOLE_BYTES + NOTHING_BYTES:
        v[b] = []
    v += [list(b"hi"), list(b"hit"), [], list(b"klm"), list(b"ab"), [], [], list(b"abcd")]
    return v


def holes_corpus() -> bytes:
    """Every root case of holes_vocab at every offset modulo 8 and across chunk ends."""
    pieces = [b"hi", b"hit", b"hx", b"h", b"klm", b"klx", b"kl", b"k#", b"z", b"zz", b"\xff", b"hz", b"zh",
              b"ab", b"abc", b"abcd", b"abcx", b"hk", b"kh", b"hhi", b"kklm", b"hitklmabcd"]
    out = bytearray()
    for rep in range(24):
        for i, p in enumerate(pieces):
            out += p + _PAD[: (rep + i) % 4]
    return bytes(out)


def wide(vocab, shift: int = 70000) -> list:
    """The same entries with every non-byte token's id moved up by `shift` (empty
    entries between): shift = 70000 gives the u32 instance of every kernel."""
    return list(vocab[:256]) + [[]] * shift + list(vocab[256:])


BOUNDARY_IDS = (65535, 65536, 0xFFFFE, 0xFFFFF, 0x100000, 0x100001)
B_SHORT, B_MID, B_LONG = b"qu", b"que", b"quest"   # (the longest fits a 7-byte chunk)


def boundary_vocab(max_id: int) -> list:
    """The 256 bytes plus three nested tokens: the longest has id max_id, the
    others max_id - 1 and 300."""
    v = _bytes256() + [[]] * (max_id - 255)
    v[300], v[max_id - 1], v[max_id] = list(B_SHORT), list(B_MID), list(B_LONG)
    return v


def boundary_text() -> bytes:
    """All three tokens, raw bytes and near-misses of the longest, at shifting offsets."""
    pieces = [B_LONG, B_MID, B_SHORT, b"q", b"ques#", b"quesquest", b"ques.", b"questquest", b"xquest",
              b"uq", b"quq", b"quequesquest"]
    out = bytearray()
    for rep in range(12):
        for i, p in enumerate(pieces):
            out += p + b" ."[: (rep + i) % 3]
    return bytes(out)


TRIE_MAGIC = 0x54524945


def empty_root_blob() -> bytes:
    """A v3 trie whose root has no children: one node, no edges, no token."""
    return struct.pack("<7I", TRIE_MAGIC, 3, 1, 0, 0, 256, 0) + struct.pack("<3I", 0, 0, 0xFFFFFFFF)


# ── corpora ──────────────────────────────────────────────────────────────────

def _other(b: int) -> int:
    return HASH if b != HASH else 0x24


def near_miss(vocab) -> bytes:
    """For each long token L: L[:j] + a byte that is not L[j], j = 3 .. len(L) - 1;
    L itself; and a * k + '#' for k = 1 .. 209.  Equal probes are kept once (the
    ladder's tokens are prefixes of each other)."""
    seen, out = set(), bytearray()

    def put(p: bytes):
        if p not in seen:
            seen.add(p)
            out.extend(p)

    for L in long_tokens(vocab):
        for j in range(3, len(L)):
            put(L[:j] + bytes([_other(L[j])]))
        put(L)
    for k in range(1, 210):
        put(bytes([A]) * k + b"#")
    return bytes(out)


PROBES = (bytes([A]) * 100 + b"#",      # matches a*65, read to 100: backs up 35 bytes
          XZ130[:129] + b"#",           # matches xz, read to 129: backs up over two windows
          XY70[:69] + b"#")             # matches the 40-byte token, read to 69


def phase_sweep(probe: bytes, cs: int, limit: int = 120_000) -> bytes:
    """`probe` repeated with raw padding to a period coprime to 64 and to cs: over
    the input the probe starts at every offset modulo 64 of a chunk-relative window
    (for a cs that is no multiple of 64, at every offset of the chunk)."""
    period = len(probe) + 1
    while gcd(period, 64) != 1 or gcd(period, cs) != 1:
        period += 1
    unit = probe + (_PAD * (period // len(_PAD) + 1))[: period - len(probe)]
    reps = 64 if cs % 64 == 0 else max(64, cs)
    return unit * min(reps, max(64, limit // period))


def run_tokens(vocab, upto: int) -> list:
    """T[r], r < upto: tokens the greedy match gives a run of r `a`s followed by '#'."""
    trie = ref_trie(vocab)
    return [len(ref_encode(bytes([A]) * r + b"#", trie, r + 1)[0]) - 1 for r in range(upto)]


_REACH: dict = {}


def reachable_counts(vocab, cs: int) -> dict:
    """{count: (r1, r2)}: a chunk a*r1 + '#' + a*r2 + raw padding has `count` tokens.
    Searched over both run lengths with ref_encode's token count of a run (kept per
    set of `a`-run tokens and chunk size: the ids do not change a count)."""
    key = (tuple(sorted(len(e) for e in vocab if len(e) > 1 and set(e) == {A})), cs)
    if key not in _REACH:
        T = run_tokens(vocab, cs)
        found: dict = {}
        for r1 in range(cs):
            for r2 in range(cs - r1):
                c = T[r1] + 1 + T[r2] + (cs - r1 - 1 - r2)
                if c not in found:
                    found[c] = (r1, r2)
        _REACH[key] = found
    return _REACH[key]


COUNT_TAIL = b"aa#a"   # the short last chunk


def count_sweep(vocab, cs: int, targets=None) -> bytes:
    """One chunk of cs bytes per target token count, in the order given (default:
    every reachable count, ascending), then COUNT_TAIL as a short last chunk."""
    reach = reachable_counts(vocab, cs)
    if targets is None:
        targets = sorted(reach)
    out = bytearray()
    for i, c in enumerate(targets):
        r1, r2 = reach[c]
        npad = cs - r1 - 1 - r2
        pad = (_PAD * (npad // len(_PAD) + 2))[i % 10: i % 10 + npad]
        out += bytes([A]) * r1 + b"#" + bytes([A]) * r2 + pad
    return bytes(out) + COUNT_TAIL[: min(len(COUNT_TAIL), cs - 1)]


# cs = 2048, one wave's four chunks each: 8 passes next to 1, 5 next to 1, ...; 19 chunks with the tail
COMPACT_TARGETS = [2048, 15, 1025, 16, 257, 2047, 20, 256, 512, 513, 30, 1536, 17, 1024, 18, 768, 19, 21]


def many_chunks(vocab, cs: int = 264, nchunks: int = 4115) -> bytes:
    """More than 4096 chunks (two blocks of the count scan), not a multiple of 16,
    of one and of two compaction passes side by side: count_sweep's chunks for the
    counts cs, the smallest, 257, 256 and a few small ones, over and over."""
    reach = reachable_counts(vocab, cs)
    lo = sorted(reach)[:5]
    cycle = [cs, lo[0], 257, lo[1], 256, lo[2], cs - 1, lo[3], 255, lo[4], 258]
    return count_sweep(vocab, cs, [cycle[i % len(cycle)] for i in range(nchunks - 1)])


def all_raw(n: int) -> bytes:
    """n bytes that start no multi-byte token of edge_vocab: a token per byte."""
    return (_PAD * (n // len(_PAD) + 1))[:n]


TAIL_MOD64 = (0, 1, 15, 16, 17, 47, 48, 49, 63)
TAIL_MODCS = (1, 7, 8, 9)


def tail_lengths(total: int, cs: int) -> list:
    """Lengths n <= total with n % 64 in TAIL_MOD64 (the largest such, and the
    smallest above 64) and n % cs in TAIL_MODCS (the largest such, and one chunk + r)."""
    out = set()
    for r in TAIL_MOD64:
        out.add((total - r) // 64 * 64 + r)
        out.add(64 + r)
    for r in TAIL_MODCS:
        if r < cs:
            out.add((total - r) // cs * cs + r)
            out.add(cs + r)
    return sorted(n for n in out if 0 < n <= total)


def tails(text: bytes, cs: int) -> list:
    return [text[:n] for n in tail_lengths(len(text), cs)]
