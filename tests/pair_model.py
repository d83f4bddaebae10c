"""CPU model of when a paired launch's second merge must be rejected.

Plain numpy on top of ``bpe_oracle``: no GPU, no native library.

A k_body launch that starts on merge index ``k - 1`` may run merge ``k`` as well
when the table's top two pairs P1 > P2 (higher count, then smaller pid) share no
token and P2's count mc2 is at least 2.  Under the exact compaction P2 is then
provably the next merge.  Under the reference compaction the stale window that
merge ``k - 1`` appends to the stream can lift another pair over P2, or change
P2's own count: then the oracle's merge ``k`` is not (P2, mc2) and a launch that
ran it as its second merge would be wrong — the zone workgroup's verdict has to
reject.  This module replays the reference-mode run and lists those indices.

Index convention: every index is the 0-based position ``k`` in the merge list of
the would-be SECOND merge; the launch that would pair it starts on ``k - 1``.
``candidates`` holds every ``k`` whose step ``k - 1`` had a token-disjoint top two
with mc2 >= 2, ``required`` the subset where merge ``k`` differs from (P2, mc2).
The model knows nothing of the library's further conditions on a candidate (the
zone rule, the step's budget, the 256-thread form): it says which second merges
the data forbids, not which launches try one.
"""
from __future__ import annotations

import numpy as np

import bpe_oracle as O


def top_two(uniq: np.ndarray, counts: np.ndarray):
    """(mc1, pid1, mc2, pid2): the two largest keys by (count desc, pid asc); zeros where absent."""
    if uniq.size == 0:
        return 0, 0, 0, 0
    i1 = int(np.argmax(counts))   # first max: the smallest pid (uniq ascends)
    mc1, pid1 = int(counts[i1]), int(uniq[i1])
    if uniq.size == 1:
        return mc1, pid1, 0, 0
    rest = counts.copy()
    rest[i1] = -1
    i2 = int(np.argmax(rest))
    return mc1, pid1, int(counts[i2]), int(uniq[i2])


def disjoint(pid1: int, pid2: int) -> bool:
    a, b, a2, b2 = pid1 >> 16, pid1 & 0xFFFF, pid2 >> 16, pid2 & 0xFFFF
    return a2 != a and a2 != b and b2 != a and b2 != b


def required_rejections(data, target: int, word_starts=None) -> dict:
    """Replay the reference-compaction run of ``O.train(data, target, word_starts)``.

    Returns dict(candidates=[k, ...], required=[k, ...], merges=[[a, b, id, count], ...])
    in the module's index convention; ``merges`` is the run itself (the caller
    checks it against ``O.train`` so the model cannot drift from the oracle)."""
    sym = O.prepare_symbols(data, word_starts)
    n = sym.shape[0]
    cur, oth = sym.copy(), np.zeros(n, dtype=np.uint32)
    nxt, needed = 256, target - 256
    merges, candidates, required = [], [], []
    pending = None   # (pid2, mc2) of the last step when it was a candidate
    while len(merges) < needed:
        uniq, counts = O.count_pairs(cur[:n])
        mc, pid, mc2, pid2 = top_two(uniq, counts)
        if mc < 2 or nxt > O.TOKEN_MASK:
            break
        k = len(merges)
        if pending is not None:
            candidates.append(k)
            if pending != (pid, mc):
                required.append(k)
        pending = (pid2, mc2) if mc2 >= 2 and disjoint(pid, pid2) else None
        a, b = pid >> 16, pid & 0xFFFF
        n, _ = O.merge_step(cur, oth, n, a, b, nxt, "reference")
        merges.append([a, b, nxt, mc])
        nxt += 1
        cur, oth = oth, cur
    return dict(candidates=candidates, required=required, merges=merges)
