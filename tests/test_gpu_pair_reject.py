"""The rejected path of a paired k_body launch against the CPU oracle.

Under the reference compaction the zone workgroup's verdict (zone_two) decides
whether a launch's second merge runs.  A rejection is a code path of its own: the
zone workgroup leaves merge 1's zone as zone_one would and returns early, every
body workgroup drops out before its second phase, k_refresh must not consume a
second merge, the speculative log entry is ignored and the host continues a step
whose launches ran out.  Real rejections depend on scheduling, so these tests

* force them (GBPE_DEBUG prej=k turns down every k-th candidate after the real
  verdict ran): every merge [a, b, id, count], the final stream, the live pair
  counts and the tail drops must still equal the oracle's, every step must come
  back full, and the counters must say that the rejections happened;
* and pin the verdict itself where the data requires it: with steps of two merges
  every step's one launch starts on an even merge index, so whether it is a
  candidate for the odd index after it does not depend on earlier verdicts, and
  tests/pair_model.py says at which of those indices the oracle's next merge is
  not the launch's P2 — there the launch must have been rejected.
"""
import functools

import numpy as np
import pytest

import bpe_oracle as O
from pair_corpora import random_case
from pair_model import required_rejections
from test_gpu_pair import _assert_pair_counters, _corpus
from test_gpu_parity import _train_native, _assert_counts_match_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


@functools.lru_cache(maxsize=None)
def _ref(kind, target, exact=False):
    """The oracle's run of a named corpus, computed once for the module (read-only)."""
    return O.train(_corpus(kind), target, compaction="exact" if exact else "reference")


def _assert_run_equals(ref, run, exact=False):
    m, s, pairs, st = run
    assert m == ref["merges"]
    assert np.array_equal(s, ref["symbols"])
    _assert_counts_match_stream(pairs, s)
    if not exact:
        assert st.tail_dropped == sum(ref["tail_drops"])
    _assert_pair_counters(st, exact)


def _assert_full_steps(step_log, batch, total):
    """Every gbpe_trainer_step call that does not end the run returns exactly `batch` merges:
    a step whose launches ran out (a rejection where the last step's pair rate promised a
    second merge) is continued inside the call, never handed back short."""
    done = 0
    for nd, *_ in step_log:
        done += nd
        if done < total:
            assert nd == batch, (done, nd)
    assert done == total


def _train(eng, monkeypatch, prej, data, target, **kw):
    if prej:
        monkeypatch.setenv("GBPE_DEBUG", f"prej={prej}")
    log = []
    run = _train_native(eng, data, target, sparse="early", step_log=log, **kw)
    return run, log


@pytest.mark.parametrize("kind,target,batch", [("english", 1800, 128), ("runs", 600, 16), ("ties", 900, 32),
                                               ("nul", 1200, 64)])
@pytest.mark.parametrize("prej", [0, 1, 2, 3])
def test_forced_rejections_match_oracle(eng, monkeypatch, kind, target, batch, prej):
    """prej=1 rejects every candidate; 2 and 3 alternate accepted and rejected launches inside a
    step (the zone buffers' ping-pong across a reject followed by an accept, a reject on a step's
    last candidate); 0 is the unforced run under the same step-size check."""
    ref = _ref(kind, target)
    run, log = _train(eng, monkeypatch, prej, _corpus(kind), target, batch=batch)
    st = run[3]
    print(f"{kind} prej={prej}: candidates {st.pair_candidates} rejected {st.pair_rejected} paired {st.paired_merges}")
    _assert_run_equals(ref, run)
    _assert_full_steps(log, batch, len(ref["merges"]))
    if prej == 1:
        assert st.paired_merges == 0
        assert st.pair_rejected == st.pair_candidates
    if kind == "english":
        assert st.pair_candidates > 0
        if prej >= 1:
            assert st.pair_rejected > 0
        if prej != 1:
            assert st.paired_merges > 0
        if prej >= 2:   # at least the forced ones (the real verdict may add its own)
            assert st.pair_rejected >= st.pair_candidates // prej


def test_forced_rejections_external_word_starts(eng, monkeypatch):
    from gpubpe import synth
    code = synth.code(90000, seed=11)
    ws = (np.random.default_rng(5).random(len(code)) < 0.15).astype(np.uint8)
    ws[0] = 1
    ref = O.train(code, 1000, word_starts=ws)
    run, log = _train(eng, monkeypatch, 3, code, 1000, word_starts=ws, batch=32)
    _assert_run_equals(ref, run)
    _assert_full_steps(log, 32, len(ref["merges"]))


def test_forced_rejections_u32_symbols(eng, monkeypatch):
    from gpubpe import synth
    data = synth.english(60000, seed=23)   # a 40K vocab: u32 symbols
    ref = O.train(data, 40000)
    run, log = _train(eng, monkeypatch, 3, data, 40000, batch=64)
    assert run[3].bytes_per_symbol == 4
    _assert_run_equals(ref, run)
    _assert_full_steps(log, 64, len(ref["merges"]))


@pytest.mark.parametrize("seed", [0, 2, 4, 6])   # the generator's reference-compaction cases
def test_forced_rejections_random_corpora(eng, monkeypatch, seed):
    data, exact, target, batch = random_case(seed)
    assert not exact
    ref = O.train(data, target)
    run, log = _train(eng, monkeypatch, 3, data, target, batch=batch)
    _assert_run_equals(ref, run)
    _assert_full_steps(log, batch, len(ref["merges"]))


def test_exact_compaction_has_no_verdict_to_force(eng, monkeypatch):
    """The exact compaction runs every candidate's second merge (no verdict, the body does not
    poll): the knob changes nothing there."""
    ref = _ref("english", 1800, True)
    run, log = _train(eng, monkeypatch, 1, _corpus("english"), 1800, exact=True, batch=128)
    st = run[3]
    _assert_run_equals(ref, run, exact=True)
    _assert_full_steps(log, 128, len(ref["merges"]))
    assert st.pair_rejected == 0
    assert st.paired_merges > 0


def test_verdict_rejects_where_the_data_requires(eng, monkeypatch):
    """Steps of two merges, no forcing: step j's one launch starts on merge 2j, so it is the
    launch that would run merge 2j + 1 second whatever happened before.  Where the model says
    the oracle's merge 2j + 1 is not that launch's (P2, mc2), a candidate must have been
    rejected and no launch may have paired; at least 3 such candidates must occur over the two
    corpora, or the test says nothing.  (Nothing is asserted about the other candidates:
    over-rejection depends on timing and only costs speed.)"""
    events = 0
    for kind, target in (("runs", 600), ("english", 1800)):
        data = _corpus(kind)
        ref = _ref(kind, target)
        model = required_rejections(data, target)
        assert model["merges"] == ref["merges"]   # the model replays the oracle's run
        required = set(model["required"])
        run, log = _train(eng, monkeypatch, 0, data, target, batch=2)
        start, prev, hit, forbidden = 0, (0, 0, 0), [], []
        for nd, cand, rej, paired in log:
            dc, dr, dp = cand - prev[0], rej - prev[1], paired - prev[2]
            prev = (cand, rej, paired)
            assert start % 2 == 0 and dc in (0, 1) and dc - dr == dp, (start, dc, dr, dp)
            if start + 1 in required:
                if dc:
                    hit.append(start + 1)
                if dc and not dr or dp:
                    forbidden.append(start + 1)
            start += nd
        st = run[3]
        print(f"{kind} batch=2: candidates {st.pair_candidates} rejected {st.pair_rejected} paired {st.paired_merges}; "
              f"required odd indices {sorted(k for k in required if k & 1)}, candidates on them {hit}")
        assert not forbidden, f"{kind}: second merges ran that the oracle does not make: {forbidden}"
        _assert_run_equals(ref, run)
        _assert_full_steps(log, 2, len(ref["merges"]))
        events += len(hit)
    assert events >= 3, f"only {events} candidate launches fell on a required rejection"
