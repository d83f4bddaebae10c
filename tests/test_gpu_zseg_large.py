"""Zone segments above 64 (zones of 1M-4M symbols inside `k_body`) against the CPU oracle.

A zone of up to 128 x 16,384 symbols runs as zone segments: the sweeping wave of `zone_seg`
reads segments `lane` and `lane + 64`.  A zone of 16-bit symbols above that runs as up to 128
segments of 32,768 symbols (the ptrace line's bt 2050).  Corpora of a few MiB reach such zones through
GBPE_DEBUG zt=K (the zone starts at K x the first count + 64 symbols, loses the sites of
every merge that lie inside it, and shrinks to K x the last count + 64 at a step boundary once
it holds twice that); the (corpus, zt, step size) of every case was chosen from the oracle's
counts so that the steps named in its docstring occur, and every
case asserts from the ptrace lines (`zone0`: the zone's length at the step's start) that they
did.  Every case compares every merge [a, b, id, count], the final stream, every live pair
count and (reference compaction) the tail drops with the oracle, requires that segment steps
are no pairing candidates, and repeats the run under zsmax=64,zs32=0 (the forms from before:
zones above 1M multi-tile), which must give the same merges and stream.

A merge of the reference compaction always has tail survivors (two hits are never adjacent, so
at most half of the stale tail goes): the m = 0 window is the exact compaction's, which every
`exact` case runs.  The sharded zone rule (zf = 5) is the multi-process trainer's; no
single-process case reaches it, so it is not covered here.
"""
import functools
import re

import numpy as np
import pytest

import bpe_oracle as O
from test_gpu_pair import _assert_pair_counters
from test_gpu_parity import _train_native, _assert_counts_match_stream

pytestmark = pytest.mark.gpu

SEG = 16384
NSEG = 128                 # NSEG_MAX
LIMIT = NSEG * SEG         # the largest zone of the 16K-segment form (and of 32-bit symbols)
SEG32, B32 = 32768, 2050   # the 32K-segment form (16-bit symbols): segment length, the ptrace line's bt


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


@functools.lru_cache(maxsize=None)
def _data(kind):
    """(bytes, word starts or None), generated once for the module (read-only)."""
    from gpubpe import synth
    if kind == "english":
        return synth.english(4 << 20, seed=31), None
    if kind == "english6":
        return synth.english(6 << 20, seed=31), None
    if kind == "english_ws":   # external word starts
        d = synth.english(4 << 20, seed=31)
        ws = (np.random.default_rng(5).random(len(d)) < 0.15).astype(np.uint8)
        ws[0] = 1
        return d, ws
    if kind == "multilingual":
        return synth.multilingual(3 << 20, seed=17), None
    if kind == "random":       # uniform bytes: the largest pair count is ~45 in 1.7M symbols
        rng = np.random.default_rng(5)
        n = 1_700_000
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        ws = (rng.random(n) < 0.15).astype(np.uint8)
        ws[0] = 1
        return d, ws
    if kind == "abcde":        # one word 360,000 times, a word start at every `a`
        d = b"abcde" * 360_000
        ws = np.zeros(len(d), np.uint8)
        ws[::5] = 1
        return d, ws
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _ref(kind, merges, exact=False, next_id=256):
    d, ws = _data(kind)
    return O.train(d, next_id + merges, word_starts=ws, next_token_id=next_id, vocab_size=next_id,
                   compaction="exact" if exact else "reference")


_PT = re.compile(r"\[ptrace\] merge (\d+) zone (\d+) zone1 (\d+) bt (\d+) pair (\d+) launches (\d+) done (\d+) "
                 r"paired (\d+) cand (\d+) mc (\d+) us [\d.]+ zone0 (\d+)")


def _train(eng, monkeypatch, capfd, kind, merges, zt, batch, exact=False, before=False, next_id=256):
    d, ws = _data(kind)
    monkeypatch.setenv("GBPE_DEBUG", f"zt={zt},ptrace=1" + (",zsmax=64,zs32=0" if before else ""))
    capfd.readouterr()
    run = _train_native(eng, d, next_id + merges, exact=exact, batch=batch, sparse="early", word_starts=ws,
                        next_id=next_id)
    keys = ("merge", "zone", "zone1", "bt", "pair", "launches", "done", "paired", "cand", "mc", "zone0")
    steps = [dict(zip(keys, map(int, m.groups()))) for m in _PT.finditer(capfd.readouterr().err)]
    assert steps, "no ptrace lines: the sparse loop did not run"
    prev = 0
    for s in steps:
        s["dcand"], prev = s["cand"] - prev, s["cand"]
    return run, steps


def _assert_forms(steps, most=NSEG, seg32=False):
    """Every step's form follows the zone's length at its start; segment and multi-tile steps are no candidates.
    seg32: 16-bit symbols with the 32K-segment form on."""
    for s in steps:
        z = s["zone0"]
        assert (s["bt"] == B32) == (seg32 and most * SEG < z <= most * SEG32), s
        if z > most * SEG:
            assert s["zone1"] == (-(-z // SEG32) if s["bt"] == B32 else 0), s
        elif z > 64 * 8192:
            assert s["zone1"] == -(-z // SEG) and s["bt"] == 1024, s
        elif z > SEG:
            assert s["zone1"] == -(-z // 8192), s
        if s["zone1"] != 1:
            assert s["pair"] == 0 and s["paired"] == 0 and s["dcand"] == 0, s


def _case(eng, monkeypatch, capfd, kind, merges, zt, batch, exact=False, next_id=256):
    """One run with up to 128 segments and one under zsmax=64,zs32=0: the first equals the oracle, the second equals
    the first.  Returns (stats, steps)."""
    ref = _ref(kind, merges, exact, next_id)
    (m, s, pairs, st), steps = _train(eng, monkeypatch, capfd, kind, merges, zt, batch, exact=exact, next_id=next_id)
    assert st.sparse_merges > 0
    assert m == ref["merges"]
    assert np.array_equal(s, ref["symbols"])
    _assert_counts_match_stream(pairs, s)
    if not exact:
        assert st.tail_dropped == sum(ref["tail_drops"])
    _assert_pair_counters(st, exact)
    _assert_forms(steps, seg32=st.bytes_per_symbol == 2)
    (m64, s64, _, st64), steps64 = _train(eng, monkeypatch, capfd, kind, merges, zt, batch, exact=exact, before=True,
                                          next_id=next_id)
    _assert_forms(steps64, most=64)
    assert all(x["zone1"] <= 64 for x in steps64)
    assert m64 == m and np.array_equal(s64, s)
    big = [x["zone1"] for x in steps if x["zone1"] > 64]
    print(f"{kind} merges={merges} zt={zt} batch={batch} exact={exact}: zone1 per step {[x['zone1'] for x in steps]}, "
          f"largest {max(big, default=0)}; zones {[x['zone0'] for x in steps]}")
    return st, steps


def _kinds(steps):
    s16 = [s for s in steps if s["bt"] != B32]
    return {
        "partial": [s for s in s16 if 65 <= s["zone1"] <= 127 and s["zone0"] % SEG],
        "most": max(s["zone1"] for s in s16),
        "above": [s for s in steps if s["zone0"] > LIMIT and s["zone1"] == 0],
        "seg32": [s for s in steps if s["bt"] == B32],
        "small": [s for s in s16 if 2 <= s["zone1"] <= 64],
    }


def test_english_every_kind_of_step(eng, monkeypatch, capfd):
    """Steps of one merge at zt=14: the zone starts at 14 x 160,686 + 64 = 2,249,668 symbols and loses every
    merge's sites inside it: 2,163,201 (both above 128 x 16K: 69 and 67 segments of 32K), 2,096,528 (128
    segments of 16K, the last one 624 symbols short), 2,048,862 (126), and shrinks to 0.85M (52 segments, the
    form from before) at the fifth merge."""
    st, steps = _case(eng, monkeypatch, capfd, "english", 14, 14, 1)
    k = _kinds(steps)
    assert len(k["seg32"]) == 2 and k["partial"] and k["small"]
    assert k["most"] == NSEG


def test_english_exact(eng, monkeypatch, capfd):
    """The exact compaction (m = 0 at every merge) on the same schedule: 32K segments, above 64 segments of 16K
    with a partial last one, and at most 64 after the shrink.  Whether a step starts at exactly 128 segments
    depends on the sites inside the zone; the largest count is printed and must be near it."""
    st, steps = _case(eng, monkeypatch, capfd, "english", 14, 14, 1, exact=True)
    k = _kinds(steps)
    assert k["seg32"] and k["partial"] and k["small"]
    assert 120 <= k["most"] <= NSEG


@pytest.mark.parametrize("exact", [False, True])
def test_english_zones_up_to_4m(eng, monkeypatch, capfd, exact):
    """6 MiB at zt=18, steps of one merge: the zone starts at 18 x 241,315 + 64 = 4.34M symbols (above the 32K
    form's 128 x 32K: the multi-tile passes, zone1 0), loses ~0.17M, 0.13M and 0.09M sites to the first three
    merges (about 128, 124 and 121 segments of 32K, the last one partial) and shrinks to 18 x 91,465 + 64
    symbols (101 segments of 16K) after the fourth."""
    st, steps = _case(eng, monkeypatch, capfd, "english6", 8, 18, 1, exact=exact)
    k = _kinds(steps)
    assert [s for s in steps if s["zone0"] > NSEG * SEG32 and s["zone1"] == 0]
    assert len(k["seg32"]) >= 2 and max(s["zone1"] for s in k["seg32"]) >= 120
    assert [s for s in k["seg32"] if s["zone0"] % SEG32] and k["partial"]


@pytest.mark.parametrize("exact", [False, True])
def test_multilingual_steps_of_two(eng, monkeypatch, capfd, exact):
    """zt=32, steps of two merges: 110 segments (32 x 56,235 + 64 symbols) down to 96, every step above 64."""
    st, steps = _case(eng, monkeypatch, capfd, "multilingual", 12, 32, 2, exact=exact)
    k = _kinds(steps)
    assert len(k["partial"]) >= 4 and not k["above"]


@pytest.mark.parametrize("exact", [False, True])
def test_u32_symbols_external_word_starts(eng, monkeypatch, capfd, exact):
    """Ids from 33,000 on force 32-bit symbols; random external word starts; zt=15, steps of two.  The zone
    starts at 15 x 145,453 + 64 = 2.18M symbols (above the limit), loses the ~0.13M sites of the first two
    merges that lie inside it (2.05M: ~126 segments, a partial last one) and shrinks to 15 x 54,218 + 64
    symbols (50 segments) after the fourth merge."""
    st, steps = _case(eng, monkeypatch, capfd, "english_ws", 10, 15, 2, exact=exact, next_id=33000)
    assert st.bytes_per_symbol == 4
    k = _kinds(steps)
    assert k["above"] and k["partial"] and k["small"]
    assert 120 <= k["most"] <= NSEG


@pytest.mark.parametrize("exact", [False, True])
def test_count_below_the_segment_count(eng, monkeypatch, capfd, exact):
    """Uniform random bytes: counts of 42-45 in a zone of 30,000 x 45 + 64 = 1.35M symbols, 83 segments — most
    segments' shares of the stale tail and of the window are empty."""
    st, steps = _case(eng, monkeypatch, capfd, "random", 6, 30000, 2, exact=exact)
    assert all(65 <= s["zone1"] <= 127 and s["mc"] < s["zone1"] for s in steps), steps


@pytest.mark.parametrize("exact", [False, True])
def test_site_across_segments_63_and_64(eng, monkeypatch, capfd, exact):
    """`abcde` x 360,000 with a word start at every `a`: (a, b) is the first merge (the four pairs tie at
    360,000; the smallest pair wins).  At zt=3 the zone is 3 x 360,000 + 64 symbols back to a word start, so it
    begins with an `a` and holds a multiple of 5 symbols: local position p holds `abcde`[p % 5].  Position
    64 x 16,384 - 1 = 1,048,575 is a multiple of 5: the last symbol of segment 63 is an `a` and the first of
    segment 64 its `b` — the site lies across the sweep's two halves."""
    ref = _ref("abcde", 2, exact)
    assert list(ref["merges"][0][:2]) == [ord("a"), ord("b")]
    st, steps = _case(eng, monkeypatch, capfd, "abcde", 2, 3, 1, exact=exact)
    first = steps[0]
    assert first["merge"] == 0 and first["zone1"] == 66, first
    assert first["zone0"] % 5 == 0 and first["zone0"] > 64 * SEG + 1, first
