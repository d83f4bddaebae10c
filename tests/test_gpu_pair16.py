"""Paired launches in zones of 8K-16K symbols (DESIGN §2f "Paired launches above 8K")
against the CPU oracle.

A step whose zone holds 8,193-16,384 symbols and that may pair runs a paired form of its
own (one 512-thread zone workgroup of 32 symbols per thread, the churn workgroup, the paired
body path) instead of two 8K-symbol segments.  Small corpora reach such zones through
GBPE_DEBUG zt=K (the zone target is K * mc + 64, and a zone shrinks to its target once it
holds twice that): the (zt, step size) of every case below was chosen so that steps of the
run fall into the range, and every case asserts from the ptrace lines that they did.  Every
case checks every merge [a, b, id, count], the final stream, every live pair count, the tail drops (reference
mode) and the pair counters, reads the steps' forms from the ptrace lines, and checks
that GBPE_DEBUG=pseg=0 (the two-segment form there, one merge per launch) gives the same
merges.  Steps whose zone is above 16,384 symbols, or in the segment forms, must not be
candidates.
"""
import functools
import re

import numpy as np
import pytest

import bpe_oracle as O
from pair_corpora import random_case
from pair_model import required_rejections
from test_gpu_pair import _assert_pair_counters, _corpus
from test_gpu_pair_churn import _zipf200
from test_gpu_parity import _train_native, _assert_counts_match_stream

pytestmark = pytest.mark.gpu

P16 = 1022          # the ptrace line's "bt" of the paired 8K-16K form
Z_LO, Z_HI = 8192, 16384


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


@functools.lru_cache(maxsize=None)
def _data(kind):
    from gpubpe import synth
    if kind == "zipf200":
        return _zipf200()
    if kind == "english_u32":
        return synth.english(60000, seed=23)
    if kind == "code":
        return synth.code(90000, seed=11)
    if kind == "multilingual":
        return synth.multilingual(150000, seed=17)
    return _corpus(kind)


@functools.lru_cache(maxsize=None)
def _ref(kind, target, exact=False):
    """The oracle's run of a corpus, computed once for the module (read-only)."""
    return O.train(_data(kind), target, compaction="exact" if exact else "reference")


_PT = re.compile(r"\[ptrace\] merge (\d+) zone (\d+) zone1 (\d+) bt (\d+) pair (\d+) launches (\d+) done (\d+) "
                 r"paired (\d+) cand (\d+)")


def _steps(err):
    """The sparse steps of a run from its ptrace lines: dicts of merge, zone, zone1, bt, pair,
    launches, done, paired, cand (cumulative candidates after the step)."""
    keys = ("merge", "zone", "zone1", "bt", "pair", "launches", "done", "paired", "cand")
    return [dict(zip(keys, map(int, m.groups()))) for m in _PT.finditer(err)]


def _train(eng, monkeypatch, capfd, data, target, zt, exact=False, batch=128, pseg=1, prej=0, word_starts=None,
           step_log=None):
    dbg = f"zt={zt},ptrace=1"
    if not pseg:
        dbg += ",pseg=0"
    if prej:
        dbg += f",prej={prej}"
    monkeypatch.setenv("GBPE_DEBUG", dbg)
    capfd.readouterr()
    run = _train_native(eng, data, target, exact=exact, batch=batch, sparse="early", word_starts=word_starts,
                        step_log=step_log)
    steps = _steps(capfd.readouterr().err)
    assert steps, "no ptrace lines: the sparse loop did not run"
    # candidates per step (the counter is cumulative over the run)
    prev = 0
    for s in steps:
        s["dcand"], prev = s["cand"] - prev, s["cand"]
    return run, steps


def _assert_run(ref, run, exact=False):
    m, s, pairs, st = run
    assert st.sparse_merges > 0
    assert m == ref["merges"]
    assert np.array_equal(s, ref["symbols"])
    _assert_counts_match_stream(pairs, s)
    if not exact:
        assert st.tail_dropped == sum(ref["tail_drops"])
    _assert_pair_counters(st, exact)


def _assert_forms(steps):
    """The form of every step follows its zone, and only the pairing forms have candidates.  (A ptrace
    line carries the zone's length at the step's end; the form is chosen by its length at the start.)"""
    for s in steps:
        if s["bt"] == P16:
            assert s["zone"] <= Z_HI and s["zone1"] == 1 and s["pair"] == 1, s
        if s["zone"] > Z_HI or s["zone1"] != 1:
            assert s["pair"] == 0 and s["paired"] == 0 and s["dcand"] == 0, s
    return sum(s["paired"] for s in steps if s["bt"] == P16), sum(s["done"] for s in steps if s["bt"] == P16)


def _case(eng, monkeypatch, capfd, kind, target, zt, batch, exact=False, prej=0, data=None, ref=None,
          word_starts=None):
    """One corpus under pseg=1 and pseg=0: both equal the oracle; returns (stats, steps, paired in the form,
    merges in the form, the pseg=0 run's stats)."""
    data = _data(kind) if data is None else data
    ref = _ref(kind, target, exact) if ref is None else ref
    log = []
    run, steps = _train(eng, monkeypatch, capfd, data, target, zt, exact=exact, batch=batch, prej=prej,
                        word_starts=word_starts, step_log=log)
    _assert_run(ref, run, exact)
    p16, n16 = _assert_forms(steps)
    off, osteps = _train(eng, monkeypatch, capfd, data, target, zt, exact=exact, batch=batch, pseg=0,
                         word_starts=word_starts)
    assert not [s for s in osteps if s["bt"] == P16]
    assert off[0] == run[0] and np.array_equal(off[1], run[1])
    _assert_pair_counters(off[3], exact)
    st = run[3]
    print(f"{kind} @ {target} zt={zt} batch={batch} exact={exact} prej={prej}: candidates {st.pair_candidates} "
          f"rejected {st.pair_rejected} paired {st.paired_merges} (pseg=0: {off[3].paired_merges}); "
          f"in the 8K-16K form {n16} merges, {p16} paired launches, "
          f"{sum(1 for s in steps if s['bt'] == P16)} steps; zones {min(s['zone'] for s in steps)}-"
          f"{max(s['zone'] for s in steps)}")
    # every gbpe_trainer_step call that does not end the run returns its full batch
    total = len(ref["merges"])
    got = 0
    for nd, _, _, _ in log:
        got += nd
        assert nd == batch or got == total, (nd, got, total)
    return st, steps, p16, n16, off[3]


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("zt,batch", [(128, 128), (128, 2), (256, 128)])
def test_english_pairs_above_8k(eng, monkeypatch, capfd, zt, batch, exact):
    """The assertion the file exists for: with the form on, more launches pair than without, and
    the additional ones ran in zones of 8K-16K symbols."""
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, "english", 1800, zt, batch, exact=exact)
    assert n16 > 0 and p16 > 0
    assert st.paired_merges > off.paired_merges


@pytest.mark.parametrize("zt,batch,least,pairs", [(3, 2, 4, False), (16, 2, 4, False), (36, 2, 4, False),
                                                 (80, 2, 6, True), (32, 16, 16, True)])
def test_runs(eng, monkeypatch, capfd, zt, batch, least, pairs):
    """`runs` (aa, zzzzzz, abab): a == b collapses, merge-1 hits inside the stale tail, position
    lim - 1 dropped or rewritten.  The run is 53 merges whose counts halve every few merges (3,278
    at merge 8, 664 at 12, 264 at 20, 31 at 30), so at steps of two one zt holds the zone at 8K-16K
    symbols for two or three steps: four zt cover counts of 3,278 / 1,394, 664 / 326, 264 / 142 and
    106 / 97 / 31, 18 merges in the form together; steps of 16 spend one whole step in it at zt=32.
    `least`: the merges that (zt, step size) spends in the form."""
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, "runs", 600, zt, batch)
    assert n16 >= least
    if pairs:
        assert p16 > 0


@pytest.mark.parametrize("kind,target,zt,batch", [("ties", 900, 5, 2), ("nul", 1200, 256, 128), ("nul", 1200, 64, 32)])
def test_ties_and_token_zero(eng, monkeypatch, capfd, kind, target, zt, batch):
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, kind, target, zt, batch)
    assert n16 > 0


@pytest.mark.parametrize("prej", [1, 2, 3])
@pytest.mark.parametrize("kind,target,zt,batch", [("runs", 600, 3, 2), ("runs", 600, 32, 16), ("english", 1800, 128, 128)])
def test_forced_rejections(eng, monkeypatch, capfd, kind, target, zt, batch, prej):
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, kind, target, zt, batch, prej=prej)
    assert n16 > 0
    if prej == 1:
        assert st.paired_merges == 0 and st.pair_rejected == st.pair_candidates
    elif batch > 2:   # both reject and pair, in the form
        assert st.pair_rejected > 0 and p16 > 0


@pytest.mark.parametrize("kind,target,zt,expect", [("runs", 600, 3, (9, 11)), ("runs", 600, 6, (13,)),
                                                   ("english", 1800, 16, (43,)), ("multilingual", 1500, 16, (23,))])
def test_verdict_rejects_where_the_data_requires(eng, monkeypatch, capfd, kind, target, zt, expect):
    """Steps of two merges, unforced (test_gpu_pair_reject's test of the same name): every candidate
    on a required index is rejected and no step pairs on one.  The required indices are fixed by the
    data (tests/test_pair_model.py), and a step of two merges at index k - 1 runs the 8K-16K form
    only while zt * mc holds the zone in the range, so each case names the zt that puts `expect`
    there: the step on each of those indices must have run the form and been a candidate — 5
    such candidates over the four cases, where the issue asks for at least 3."""
    data, ref = _data(kind), _ref(kind, target)
    model = required_rejections(data, target)
    assert model["merges"] == ref["merges"]
    required = set(model["required"])
    assert set(expect) <= required
    log = []
    run, steps = _train(eng, monkeypatch, capfd, data, target, zt, batch=2, step_log=log)
    _assert_run(ref, run)
    _assert_forms(steps)
    form = {s["merge"]: s["bt"] for s in steps}
    start, prev, hit, forbidden = 0, (0, 0, 0), [], []
    for nd, cand, rej, paired in log:
        dc, dr, dp = cand - prev[0], rej - prev[1], paired - prev[2]
        prev = (cand, rej, paired)
        assert dc in (0, 1) and dc - dr == dp, (start, dc, dr, dp)
        if start + 1 in required:
            if dc and form.get(start) == P16:
                hit.append(start + 1)
            if dc and not dr or dp:
                forbidden.append(start + 1)
        start += nd
    print(f"{kind} zt={zt} batch=2: required {sorted(required)}, candidates on them in the 8K-16K form {hit}")
    assert not forbidden, f"{kind}: second merges ran that the oracle does not make: {forbidden}"
    assert set(expect) <= set(hit), f"{kind} zt={zt}: no candidate of the 8K-16K form on {sorted(set(expect) - set(hit))}"


def test_churn_table_overflow(eng, monkeypatch, capfd):
    """More distinct tail and window pairs than the churn table's slots: the overflowing adds go
    straight to the global table and the launch is rejected (no pairing count asserted)."""
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, "zipf200", 1200, 128, 128)
    assert n16 > 0


def test_u32_symbols(eng, monkeypatch, capfd):
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, "english_u32", 40000, 256, 128)
    assert st.bytes_per_symbol == 4
    assert n16 > 0 and p16 > 0


@pytest.mark.parametrize("exact", [False, True])
def test_external_word_starts(eng, monkeypatch, capfd, exact):
    code = _data("code")
    ws = (np.random.default_rng(5).random(len(code)) < 0.15).astype(np.uint8)
    ws[0] = 1
    ref = O.train(code, 1000, word_starts=ws, compaction="exact" if exact else "reference")
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, "code", 1000, 256, 32, exact=exact, data=code, ref=ref,
                                     word_starts=ws)
    assert n16 > 0 and p16 > 0


@pytest.mark.parametrize("seed,zt", [(0, 128), (1, 128), (2, 128), (3, 128), (4, 64), (5, 128), (6, 128), (7, 256)])
def test_random_corpora(eng, monkeypatch, capfd, seed, zt):
    data, exact, target, batch = random_case(seed)
    ref = O.train(data, target, compaction="exact" if exact else "reference")
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, f"random{seed}", target, zt, batch, exact=exact, data=data,
                                     ref=ref)
    assert n16 > 0 and p16 > 0


def test_zones_above_16k_do_not_pair(eng, monkeypatch, capfd):
    """zt=256 on English holds early steps above 16,384 symbols (the segment forms) before the zone
    falls into the 8K-16K range: no step of the first kind is a candidate, some of the second pair."""
    st, steps, p16, n16, off = _case(eng, monkeypatch, capfd, "english", 1800, 256, 16)
    above = [s for s in steps if s["zone"] > Z_HI]
    assert above and all(s["zone1"] != 1 and s["dcand"] == 0 and s["paired"] == 0 for s in above)
    assert [s for s in above if s["zone1"] >= 2]   # (some of them in the segment forms)
    assert p16 > 0
