"""Reference and inputs of the device-decode tests — TEST INFRASTRUCTURE ONLY.

decode_np is a numpy restatement of the oracle's decode (a lengths gather, a
cumsum, an np.repeat-based byte gather); tests/test_decode_host.py pins it to
O.decode on every stream below 100K tokens, so the GPU tests may use it where the
oracle's per-token loop would be slow.  The vocabularies and token streams of the
GPU tests live here too, so that both test files see the same ones.
"""
import functools

import numpy as np

REPLACEMENT = [0xEF, 0xBF, 0xBD]   # U+FFFD, what an unknown id decodes to
BLK = 4096                         # tokens per scan block / scatter workgroup
COUNTS = [1, 2, 63, 64, 65, BLK - 1, BLK, BLK + 1, 2 * BLK + 1]


# ── vocabularies ────────────────────────────────────────────────────────────
@functools.lru_cache(maxsize=None)
def _vocab_a():
    v = [[b] for b in range(256)]
    v += [[(37 * ln + 11 * j) & 0xFF for j in range(ln)] for ln in range(1, 18)]   # ids 256..272: every length 1..17
    v.append([])                                                                    # 273: empty
    v.append([(j * 7 + 3) & 0xFF for j in range(300)])                              # 274: 300 bytes
    v.append([(j * 13 + (j >> 8)) & 0xFF for j in range(65535)])                    # 275: the longest entry allowed
    v.append([])                                                                    # 276: empty, the last id
    return v


def vocab_a():
    """Hand-built: the 256 bytes, entries of every length 1..17, two empty entries
    (one the last id), one 300-byte entry, one 65,535-byte entry."""
    return _vocab_a()


A_LEN1 = 256            # id of the entry of length L is A_LEN1 + L - 1 (L in 1..17)
A_EMPTY, A_LONG, A_BIG, A_LAST_EMPTY = 273, 274, 275, 276
A_SIZE = 277


@functools.lru_cache(maxsize=None)
def vocab_b():
    import bpe_oracle as O
    from gpubpe import synth
    return O.vocab_from_merges(O.train(synth.multilingual(40000, seed=43), 500)["merges"]).entries


def flatten(vocab):
    """(bytes: np.uint8[], offsets: np.uint64[V + 1]) — the gbpe_vocab_upload layout."""
    offs = np.zeros(len(vocab) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(e) for e in vocab], dtype=np.uint64)
    flat = np.array([b for e in vocab for b in e], dtype=np.uint8)
    return flat, offs


# ── the reference ───────────────────────────────────────────────────────────
def decode_np(tokens, vocab) -> np.ndarray:
    """O.decode(tokens, vocab) as np.uint8[]: ids >= len(vocab) give EF BF BD."""
    flat, offs = flatten(list(vocab) + [REPLACEMENT])
    offs = offs.astype(np.int64)
    ids = np.minimum(np.asarray(tokens, dtype=np.uint32).astype(np.int64), len(vocab))
    lens = offs[ids + 1] - offs[ids]
    total = int(lens.sum())
    dst = np.cumsum(lens) - lens                        # exclusive scan: each token's first output byte
    src = np.repeat(offs[ids] - dst, lens) + np.arange(total, dtype=np.int64)
    return flat[src]


# ── token streams over vocab A ──────────────────────────────────────────────
def random_stream(n, seed):
    """n ids of vocab A from a seeded rng: every id but the 65,535-byte one, which
    sits once at a seeded position from 64 tokens on (keeps the outputs small)."""
    rng = np.random.default_rng(seed)
    pool = np.array([i for i in range(A_SIZE) if i != A_BIG], dtype=np.uint32)
    t = pool[rng.integers(0, pool.shape[0], size=n)]
    if n >= 64:
        t[int(rng.integers(0, n))] = A_BIG
    return t.astype(np.uint32)


def leading_empty(n, seed):
    t = random_stream(n, seed)
    t[0] = A_EMPTY
    return t


def boundary_long(n, seed):
    """The 300-byte token first, last and (where the stream reaches them) at index
    4095 and 4096: one token's bytes cross a workgroup's output boundary."""
    t = random_stream(n, seed)
    for i in (0, n - 1, BLK - 1, BLK):
        if i < n:
            t[i] = A_LONG
    return t


def stream_of_total(total):
    """Tokens of lengths 7, 7, ... and the remainder, an empty token after each:
    exactly `total` bytes."""
    t = []
    while total > 0:
        ln = min(7, total)
        t += [A_LEN1 + ln - 1, A_EMPTY]
        total -= ln
    return np.array(t, dtype=np.uint32)


UNKNOWN = [A_SIZE, 70000, 0xFFFFFFFF]   # V itself, a mid-range id, the largest


def with_unknown(n, seed):
    t = random_stream(n, seed)
    rng = np.random.default_rng(seed + 1)
    k = max(1, n // 5)
    t[rng.integers(0, n, size=k)] = np.array(UNKNOWN, dtype=np.uint32)[rng.integers(0, 3, size=k)]
    t[0] = 0xFFFFFFFF
    return t


def all_unknown(n):
    return np.resize(np.array(UNKNOWN, dtype=np.uint32), n)


def big_entry_stream():
    return np.array([65, 66, A_BIG, 67, 68, 69], dtype=np.uint32)


def big_block_stream():
    """Several 65,535-byte tokens in the first block, two of them followed by an
    empty token: one workgroup's output range of more than 192 KiB beside one of a
    few KiB."""
    t = random_stream(BLK + 1, 4300)
    t[[10, 2000, BLK - 6]] = A_BIG
    t[[11, 2001]] = A_EMPTY
    return t


BATCH_COUNTS = [0, 1, 0, 0, 63, 64, 65, BLK - 1, BLK, BLK + 1, 0]


def batch_documents(counts=BATCH_COUNTS, seed=500):
    return [random_stream(c, seed + i) for i, c in enumerate(counts)]


def many_small_documents(n_docs=10000, seed=77):
    rng = np.random.default_rng(seed)
    pool = np.array([i for i in range(A_SIZE) if i != A_BIG] + UNKNOWN, dtype=np.uint32)
    return [pool[rng.integers(0, pool.shape[0], size=int(c))] for c in rng.integers(0, 7, size=n_docs)]


def sliced_documents():
    """9,001 tokens in documents that span the 1000-token slice edges, start on
    them and end on them."""
    counts = [999, 1, 0, 3500, 0, 1500, 1000, 1, 1999, 0, 1, 0]
    assert sum(counts) == 9001
    return batch_documents(counts, seed=900)


def small_streams():
    """name -> tokens of every single-stream case of the GPU tests below 100K tokens."""
    s = {}
    for n in COUNTS:
        s[f"random-{n}"] = random_stream(n, 100 + n)
        s[f"leading-empty-{n}"] = leading_empty(n, 200 + n)
        s[f"boundary-long-{n}"] = boundary_long(n, 300 + n)
        s[f"unknown-{n}"] = with_unknown(n, 400 + n)
    for total in (0, 15, 16, 17, 31, 32, 33):
        s[f"total-{total}"] = stream_of_total(total)
    s["only-empty"] = np.array([A_EMPTY, A_LAST_EMPTY] * 40, dtype=np.uint32)
    for n in (1, 5, 64, BLK + 1):
        s[f"all-unknown-{n}"] = all_unknown(n)
    s["big-entry"] = big_entry_stream()
    s["big-block"] = big_block_stream()
    return s


def large_stream_b():
    """More than 1024 scan blocks: k_chunk_scan2 takes more than one block sum per thread."""
    n = 1024 * BLK + BLK + 1
    return np.random.default_rng(4242).integers(0, len(vocab_b()), size=n, dtype=np.uint32)
