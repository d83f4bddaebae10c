"""gpubpe.synth.english: the threaded word stream against the plain one.

The fixtures under tests/golden/ were made from corpora drawn with
rng.choice(V, size=W, p=p) on one thread; the generator now looks the same
uniform draws up in p's cumulative sum itself, slice by slice.  Both must give
the same bytes for the numpy in use, at sizes with one slice and with several.
"""
import numpy as np
import pytest

from gpubpe import synth


def plain_english(n_bytes: int, seed: int, fancy_punct: float) -> bytes:
    rng = np.random.Generator(np.random.PCG64(seed))
    lex = synth.english_lexicon()
    V = len(lex)
    p = synth._zipf_p(V)
    seps = [b" ", b", ", b". ", b"\n", b",\n", b".\n", "’ ".encode(), " “".encode(), "” ".encode(), " — ".encode()]
    pieces = list(lex) + seps
    avg = float(np.dot(p, [len(w) for w in lex])) + 1.0
    out, have = [], 0
    while have < n_bytes:
        W = int(min(8_000_000, max(1024, (n_bytes - have) / avg * 1.05)))
        words = rng.choice(V, size=W, p=p)
        gaps = rng.integers(8, 17, size=W // 8 + 2)
        nl_pos = np.cumsum(gaps)
        nl_pos = nl_pos[nl_pos < W]
        is_nl = np.zeros(W, dtype=bool)
        is_nl[nl_pos] = True
        u = rng.random(W)
        punct = np.where(u < 0.05, 1, np.where(u < 0.10, 2, 0))
        sep = np.where(is_nl, 3 + punct, punct)
        if fancy_punct > 0:
            f = rng.random(W) < fancy_punct
            sep = np.where(f & ~is_nl, 6 + rng.integers(0, 4, size=W), sep)
        ids = np.empty(2 * W, dtype=np.int64)
        ids[0::2] = words
        ids[1::2] = V + sep
        chunk = synth._assemble(pieces, ids)
        out.append(chunk)
        have += chunk.shape[0]
    return np.concatenate(out)[:n_bytes].tobytes()


@pytest.mark.parametrize("n,seed,fancy", [(1000, 5, 0.0), (262_144, 1, 0.0), (3_000_000, 9, 0.005)])
def test_english_equals_plain_generator(n, seed, fancy):
    got = synth.english(n, seed=seed, fancy_punct=fancy)
    assert len(got) == n
    assert got == plain_english(n, seed, fancy)
