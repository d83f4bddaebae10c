"""The churn workgroup of a paired k_body launch against the CPU oracle.

Under the reference compaction a paired launch's merge-1 stale tail, stale window and
verdict run in a workgroup of their own (pair_churn) beside the zone workgroup, which
keeps only its site deltas and reads the verdict word; the body workgroups read the same
word.  The split can go wrong where the churn workgroup must reproduce, from the zone's
last mc + 2 symbols alone, what the zone pass knew: merge-1 hits inside the stale tail,
a dropped or rewritten window neighbour at lim - 1, a delta table of its own that may
overflow, and a verdict that now arrives from another workgroup on the rejected path
too.  Every case checks every merge [a, b, id, count], the final stream, every live
pair count, the tail drops and the pair counters, and that GBPE_DEBUG=pair=0 (one
merge per launch, no churn workgroup) gives the same merges.

What each test notices was checked once with four deliberately wrong builds (DESIGN §2f;
not committed): W (the window's pairs added by the zone workgroup too), V (the zone
workgroup ignores the verdict word and always runs merge 2), L (position lim - 1 not
checked: its token always taken as the window's left neighbour, no rejection) and M (the
tail's survivors counted without merge 1's hits, m = mc).
"""
import functools

import numpy as np
import pytest

import bpe_oracle as O
from test_gpu_pair import _assert_pair_counters, _corpus
from test_gpu_parity import _train_native, _assert_counts_match_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


def _zipf200():
    """~150 KB of Zipf-weighted random words over a 200-byte alphabet: a late merge's stale
    tail and window hold more distinct pairs than the churn workgroup's table has slots."""
    rng = np.random.default_rng(207)
    alpha = np.arange(40, 240, dtype=np.uint8)
    nv = 6000
    vocab = [bytes(rng.choice(alpha, size=int(n)).tolist()) for n in rng.integers(2, 9, size=nv)]
    p = 1.0 / np.arange(1, nv + 1) ** 0.9
    words = rng.choice(nv, size=27000, p=p / p.sum())
    return b" ".join(vocab[i] for i in words)


@functools.lru_cache(maxsize=None)
def _data(kind):
    from gpubpe import synth
    if kind == "zipf200":
        return _zipf200()
    if kind == "english_u32":
        return synth.english(60000, seed=23)
    return _corpus(kind)


@functools.lru_cache(maxsize=None)
def _ref(kind, target):
    """The oracle's run of a corpus, computed once for the module (read-only)."""
    return O.train(_data(kind), target)


_UNPAIRED = {}


def _unpaired_merges(eng, monkeypatch, kind, target, batch):
    """The same run with GBPE_DEBUG=pair=0, once per (corpus, target, batch)."""
    key = (kind, target, batch)
    if key not in _UNPAIRED:
        monkeypatch.setenv("GBPE_DEBUG", "pair=0")
        m, _, _, st = _train_native(eng, _data(kind), target, batch=batch, sparse="early")
        assert st.paired_merges == 0 and st.pair_candidates == 0
        _UNPAIRED[key] = m
    return _UNPAIRED[key]


def _run(eng, monkeypatch, kind, target, batch, prej=0):
    ref = _ref(kind, target)
    if prej:
        monkeypatch.setenv("GBPE_DEBUG", f"prej={prej}")
    else:
        monkeypatch.delenv("GBPE_DEBUG", raising=False)
    m, s, pairs, st = _train_native(eng, _data(kind), target, batch=batch, sparse="early")
    print(f"{kind} @ {target} batch={batch} prej={prej}: candidates {st.pair_candidates} "
          f"rejected {st.pair_rejected} paired {st.paired_merges}")
    assert st.sparse_merges > 0
    assert m == ref["merges"]
    assert np.array_equal(s, ref["symbols"])
    _assert_counts_match_stream(pairs, s)
    assert st.tail_dropped == sum(ref["tail_drops"])
    _assert_pair_counters(st)
    assert _unpaired_merges(eng, monkeypatch, kind, target, batch) == m
    return st


@pytest.mark.parametrize("batch", [2, 16])
def test_merge1_hits_inside_the_stale_tail(eng, monkeypatch, batch):
    """`runs` (2-letter alphabet, a == b collapses): merge-1 hits inside the stale tail (m < mc),
    position lim - 1 a dropped B-side or a rewritten A-side.  Fails with builds L and M (and with
    V and W), at both step sizes."""
    _run(eng, monkeypatch, "runs", 600, batch)


@pytest.mark.parametrize("prej", [1, 2, 3])
def test_forced_rejections_arrive_from_the_churn_workgroup(eng, monkeypatch, prej):
    """The rejected path with the verdict coming from another workgroup.  Fails with build V (the
    zone workgroup runs merge 2 on a rejected launch) at every prej, and with W and M."""
    st = _run(eng, monkeypatch, "runs", 600, 16, prej=prej)
    if prej == 1:
        assert st.paired_merges == 0
        assert st.pair_rejected == st.pair_candidates


def test_churn_table_overflow(eng, monkeypatch):
    """More distinct tail and window pairs than the churn table's slots: the overflowing adds go
    straight to the global table and the launch is rejected.  (No pairing count asserted: overflow
    depends on insertion order.)  Fails with builds W and M; V and L pass it."""
    _run(eng, monkeypatch, "zipf200", 1200, 128)


def test_token_zero(eng, monkeypatch):
    """Token 0 never pairs: tail and window pairs with a 0 on either side are skipped.  Fails with
    builds V (the tail drops differ), W and M."""
    _run(eng, monkeypatch, "nul", 1200, 64)


def test_u32_symbols(eng, monkeypatch):
    """A 40K vocab: u32 symbols, the 2,048-slot tables.  Fails with all four builds (L: the live pair
    counts differ from a recount of the stream)."""
    st = _run(eng, monkeypatch, "english_u32", 40000, 64)
    assert st.bytes_per_symbol == 4


@pytest.mark.parametrize("batch", [2, 128])
def test_english_pairs(eng, monkeypatch, batch):
    """English at steps of two merges (every launch starts on an even index) and of 128.  Fails with
    builds W and M at both step sizes, and with V at steps of two."""
    st = _run(eng, monkeypatch, "english", 1800, batch)
    assert st.paired_merges > 0
