"""Random corpora of the paired-launch tests (test_gpu_pair.py, test_gpu_pair_reject.py)."""
import numpy as np


def random_case(seed: int):
    """One case of the property test: (data, exact, target, batch).

    A small random alphabet (2-7 letters, so same-symbol runs and count ties
    abound), Zipf-weighted random words, token-0 bytes in every third seed; odd
    seeds run the exact compaction, even seeds the reference one."""
    rng = np.random.default_rng(1000 + seed)
    alpha = rng.choice(list(b"abcdefghijklmnop"), size=int(rng.integers(2, 8)), replace=False)
    nv = int(rng.integers(300, 2000))
    vocab = [bytes(rng.choice(alpha, size=int(n)).tolist()) for n in rng.integers(1, 9, size=nv)]
    p = 1.0 / np.arange(1, nv + 1) ** rng.uniform(0.8, 1.3)
    words = rng.choice(nv, size=int(rng.integers(12000, 24000)), p=p / p.sum())
    data = bytearray(b" ".join(vocab[i] for i in words))
    if seed % 3 == 0:   # token 0 never pairs (train.wgsl:395-399)
        for i in rng.integers(0, len(data), len(data) // 200):
            data[i] = 0
    exact = bool(seed & 1)
    target = 256 + int(rng.integers(300, 1200))
    batch = int(rng.choice([16, 64, 128]))
    return bytes(data), exact, target, batch
