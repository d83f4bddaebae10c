"""Corpora of the word-lexicon build tests — TEST INFRASTRUCTURE ONLY.

``edge_corpus``: a small piece with everything the build kernels treat specially.
``skewed_words`` / ``distinct_words``: large corpora of fixed-width words (" " +
letters: one word each under the reference word-boundary heuristic), whose
reference is one np.unique.  ``windowed_words``: three-byte words under an external
mask, laid out by the windows of words the two-stage build's workgroups take.
"""
from __future__ import annotations

import numpy as np

TILE = 8192   # train_dev.h TILE: symbols per k_lx_count / k_lx_wpos workgroup


def _letters(rng, n: int) -> bytes:
    return rng.integers(97, 123, size=n, dtype=np.uint8).tobytes()


def edge_corpus(seed: int = 3, tiles: int = 8) -> dict:
    """{"data", "big": (start, length) of the several-tile word, "aligned": the tile
    multiple at which a word starts}.  Under the default boundaries a word is a space
    and the letters after it, so " " + L-1 letters is a word of L symbols.  Holds:
    \\x00 bytes at the very start and end, alone between words and adjacent; words of
    63, 64, 65 and 66 symbols (each twice: the 65 and 66 ones are repeated long words);
    a word of 2.5 tiles; a word that starts exactly at a multiple of TILE; filler words
    from a pool of 300, so most words repeat; exactly tiles * TILE bytes."""
    rng = np.random.default_rng(seed)
    pool = [b" " + _letters(rng, int(k)) for k in rng.integers(1, 12, size=300)]

    def filler(k):
        return b"".join(pool[i] for i in rng.integers(0, len(pool), size=k))

    sized = {L: b" " + _letters(rng, L - 1) for L in (63, 64, 65, 66)}
    out = [b"\x00", filler(40), b"\x00", filler(3), b"\x00\x00\x00", filler(20)]
    for L in (63, 64, 65, 66):
        out += [sized[L], filler(5)]
    out += [b"\x00", sized[65], b"\x00"]                    # a long word between literals
    for L in (66, 64, 63, 65):
        out += [sized[L], filler(7)]
    out.append(filler(200))
    pos = sum(len(p) for p in out)
    big = (pos, 1 + 2 * TILE + TILE // 2)
    out.append(b" " + _letters(rng, big[1] - 1))            # one word of several tiles
    out.append(filler(300))
    pos = sum(len(p) for p in out)
    aligned = (pos // TILE + 1) * TILE
    if aligned - pos < 2:
        aligned += TILE
    out.append(b" " + _letters(rng, aligned - pos - 1))     # ... up to the tile boundary
    out.append(b" tile" + filler(50))                       # this word starts at `aligned`
    pos = sum(len(p) for p in out)
    end = tiles * TILE
    assert pos + 2000 < end
    while end - pos > 600:
        out.append(filler(20))
        pos = sum(len(p) for p in out)
    out.append(b" " + _letters(rng, end - pos - 2) + b"\x00")
    data = b"".join(out)
    assert len(data) == end and data[aligned] == 32 and data[aligned - 1] != 32
    return {"data": data, "big": big, "aligned": aligned}


def random_starts(n: int, seed: int, every: int = 6) -> np.ndarray:
    """an external word-start mask: about one start in `every` positions"""
    rng = np.random.default_rng(seed)
    ws = (rng.integers(0, every, size=n) == 0).astype(np.uint8)
    ws[0] = 1
    return ws


def decode_words(ids: np.ndarray, letters: int) -> np.ndarray:
    """[N, 1 + letters] bytes: a space, then the id in base 26 as letters"""
    w = np.empty((ids.shape[0], letters + 1), np.uint8)
    w[:, 0] = 32
    v = ids.astype(np.int64).copy()
    for k in range(letters, 0, -1):
        w[:, k] = 97 + v % 26
        v //= 26
    return w


def distinct_ids(rng, n: int, letters: int) -> np.ndarray:
    """n distinct word ids below 26 ** letters, in random order"""
    space = 26 ** letters
    assert n * 2 < space
    ids = np.unique(rng.integers(0, space, size=n + n // 4 + 1024))
    rng.shuffle(ids)
    assert ids.shape[0] >= n
    return ids[:n]


def skewed_words(n_words: int, pool: int, seed: int, letters: int = 5) -> bytes:
    """n_words fixed-width words drawn from `pool` distinct ones with a skew (a quarter of the
    draws come from the 64 hottest words), so hot words repeat in every workgroup of the build"""
    rng = np.random.default_rng(seed)
    ids = distinct_ids(rng, pool, letters)
    pick = rng.integers(0, pool, size=n_words)
    hot = rng.integers(0, 4, size=n_words) == 0
    pick[hot] = rng.integers(0, 64, size=int(hot.sum()))
    return decode_words(ids[pick], letters).tobytes()


def distinct_words(n_distinct: int, seed: int, letters: int = 5, hot: int = 4, hot_each: int = 1000,
                   twice: float = 0.0) -> bytes:
    """n_distinct distinct fixed-width words, each once (a share `twice` of them twice), plus
    `hot` more words hot_each times each, all shuffled"""
    rng = np.random.default_rng(seed)
    ids = distinct_ids(rng, n_distinct + hot, letters)
    parts = [ids[:n_distinct], np.repeat(ids[n_distinct:], hot_each)]
    if twice:
        parts.append(ids[: int(n_distinct * twice)])
    allw = np.concatenate(parts)
    rng.shuffle(allw)
    return decode_words(allw, letters).tobytes()


def windowed_words(windows: int, window: int, distinct: int, seed: int, hot: int = 4):
    """(bytes, word-start mask) of windows * window three-byte words (no 0 byte; the mask starts a
    word every three bytes): window k holds `distinct` words of its own, repeated to fill it,
    and `hot` words shared by every window — so a build workgroup that takes one window of
    consecutive words sees only `distinct` + `hot` distinct words, while the corpus holds
    windows * distinct + hot."""
    rng = np.random.default_rng(seed)
    total = windows * distinct + hot
    assert 2 * total < 255 ** 3
    ids = np.unique(rng.integers(0, 255 ** 3, size=total + total // 4))
    rng.shuffle(ids)
    ids = ids[:total]
    col = np.arange(window) % distinct
    rng.shuffle(col)
    w = ids[hot:].reshape(windows, distinct)[:, col]
    w[:, rng.choice(window, size=8 * hot, replace=False)] = np.tile(ids[:hot], 8)[None, :]
    w = w.reshape(-1)
    out = np.empty((w.shape[0], 3), np.uint8)
    for k in range(3):
        out[:, k] = 1 + w % 255
        w = w // 255
    ws = np.zeros((out.shape[0], 3), np.uint8)
    ws[:, 0] = 1
    return out.tobytes(), ws.reshape(-1)
