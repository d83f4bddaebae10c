"""Pin tests/pair_model.py: the CPU model of when a paired launch's second merge must be
rejected, which test_gpu_pair_reject.py holds the GPU's verdict against.

The model replays the reference-compaction run itself, so its merges are compared with
O.train's (it cannot drift from the oracle), and its answers on the GPU suite's own
corpora are pinned.  Indices are those of the would-be second merge (pair_model's
convention).  All four corpora run here: the scan takes some 15 s on one core.
"""
import numpy as np
import pytest

import bpe_oracle as O
from pair_model import disjoint, required_rejections, top_two
from test_gpu_pair import _corpus


def _data(kind):
    if kind == "multilingual":   # test_pairing_off_gives_the_same_run's corpus
        from gpubpe import synth
        return synth.multilingual(150000, seed=17)
    return _corpus(kind)


# corpus, target vocab: steps whose top two are token-disjoint with mc2 >= 2 (and a merge after
# them), and the indices k where the oracle's merge k is not that step's (P2, mc2)
TABLE = [
    ("english", 1800, 1094, [2, 4, 16, 22, 26, 30, 36, 43, 75, 113, 432]),
    ("runs", 600, 31, [1, 8, 9, 11, 13, 25, 32, 33, 46]),
    ("multilingual", 1500, 1007, [1, 4, 10, 20, 23, 26, 28, 62]),
    # `ties` stops after 13 merges (its words are 8-byte little-endian letters: 7 of 8 bytes are
    # token 0, which never pairs).  Step 9's top two are (0x20,0x69):916 and (0x107,0x64):6,
    # token-disjoint, and its 914-symbol stale window makes (0x108,0x65):4 the oracle's merge 10
    # — a required rejection; step 11's (0x20,0x65):2 and (0x101,0x6a):2 pair up as merge 12.
    ("ties", 900, 2, [10]),
]


@pytest.mark.parametrize("kind,target,ncand,required", TABLE, ids=[r[0] for r in TABLE])
def test_required_rejections_pinned_and_replay_the_oracle(kind, target, ncand, required):
    data = _data(kind)
    model = required_rejections(data, target)
    ref = O.train(data, target)
    assert model["merges"] == ref["merges"]
    assert len(model["candidates"]) == ncand
    assert model["required"] == required
    assert set(required) <= set(model["candidates"])
    # the index convention, from the oracle's merge list alone: P2 shares no token with merge
    # k - 1, so a merge k that does cannot be P2 — such a candidate is always required
    for k in model["candidates"]:
        (a, b, _, _), (a2, b2, _, _) = ref["merges"][k - 1], ref["merges"][k]
        if not disjoint((a << 16) | b, (a2 << 16) | b2):
            assert k in required


def test_top_two_against_a_sort():
    rng = np.random.default_rng(3)
    for _ in range(200):
        n = int(rng.integers(0, 12))
        uniq = np.sort(rng.choice(1 << 20, size=n, replace=False)).astype(np.uint32)
        counts = rng.integers(1, 4, size=n).astype(np.int64)   # many ties: the smaller pid wins
        order = sorted(range(n), key=lambda i: (-int(counts[i]), int(uniq[i])))
        want = [0, 0, 0, 0]
        for j, i in enumerate(order[:2]):
            want[2 * j], want[2 * j + 1] = int(counts[i]), int(uniq[i])
        assert list(top_two(uniq, counts)) == want


def test_exact_compaction_never_requires_a_rejection():
    """The exact compaction has no stale window, so a token-disjoint (P2, mc2) is always the next
    merge there (DESIGN §2f's exactness argument, same-symbol runs included): the same top-two
    and disjointness rules as the model's, replayed under compaction="exact", never find a
    required rejection.  What required_rejections lists is what the reference compaction adds."""
    data = _corpus("runs")[:20000]
    exact = O.train(data, 300, compaction="exact")
    sym = O.prepare_symbols(data)
    n, cur, oth, nxt = sym.shape[0], sym.copy(), np.zeros_like(sym), 256
    pending, seen = None, 0
    for a, b, nw, mc in exact["merges"]:
        uniq, counts = O.count_pairs(cur[:n])
        mc1, pid1, mc2, pid2 = top_two(uniq, counts)
        assert (pid1, mc1) == ((a << 16) | b, mc)
        if pending is not None:
            assert pending == (pid1, mc1)
            seen += 1
        pending = (pid2, mc2) if mc2 >= 2 and disjoint(pid1, pid2) else None
        n, _ = O.merge_step(cur, oth, n, a, b, nw, "exact")
        cur, oth = oth, cur
    assert seen > 0
