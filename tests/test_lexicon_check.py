"""The lexicon checker itself (tests/lexicon_check.py) on the CPU: it accepts the
numpy model's lexicon of an edge corpus and rejects seven single corruptions of
it, each for the stated reason."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import lexicon_check as LC  # noqa: E402
import lexicon_corpora as LCo  # noqa: E402
from lexshard_model import ModelLexBackend  # noqa: E402

WS = 0x10000   # the model's layout: u32 symbols, bit 16 = word start


def per_occurrence_longs(store, mul, occ):
    """The model deduplicates every word; the GPU build keeps an entry per occurrence of a
    word of more than LX_LMAX symbols, each with multiplicity 1.  Rewrite the model's output
    that way: the first occurrence of a long word keeps the entry, every further one gets a
    copy appended to the store."""
    e0, el = LC.split_store(store)
    em = mul[e0]
    store, mul, occ = [store], [mul.copy()], occ.copy()
    ne = e0.shape[0]
    for e in np.flatnonzero((el > LC.LMAX) & (em > 1)).tolist():
        js = np.flatnonzero(occ == e)
        assert js.shape[0] == em[e]
        mul[0][e0[e]: e0[e] + el[e]] = 1
        for j in js[1:].tolist():
            store.append(store[0][e0[e]: e0[e] + el[e] + 1])
            mul.append(np.append(np.ones(el[e], np.uint32), np.uint32(0)))
            occ[j] = ne
            ne += 1
    return np.concatenate(store), np.concatenate(mul), occ, ne


def model_lexicon(data, zone_target, word_starts=None):
    be = ModelLexBackend()
    be.create(data, len(data), False, word_starts)
    info = be.build(zone_target)
    store, mul, occ, ne = per_occurrence_longs(be.store, be.mul, be.occ)
    info = dict(info, store_symbols=int(store.shape[0]), entries=ne)
    return {"store": store, "mul": mul, "occ": occ, "zone": be.zone.copy(), "info": info}


def check(data, zt, lx, ws=None):
    return LC.check_piece(data, zt, lx["store"], lx["mul"], lx["occ"], lx["zone"], lx["info"], ws)


@pytest.fixture(scope="module")
def edge():
    c = LCo.edge_corpus(seed=3)
    data, zt = c["data"], 3000
    return data, zt, model_lexicon(data, zt)


def _copy(lx):
    return {k: (v.copy() if isinstance(v, np.ndarray) else dict(v)) for k, v in lx.items()}


def test_edge_corpus_holds_the_edges():
    c = LCo.edge_corpus(seed=3)
    data = c["data"]
    s = LC.reference_stream(data, None, 4)
    st = np.flatnonzero(LC.starts_mask(s, WS, 0xFFFF))
    ln = np.diff(np.append(st, len(s)))
    assert len(data) % LCo.TILE == 0 and data[0] == 0 and data[-1] == 0 and b"\x00\x00" in data
    for L in (63, 64, 65, 66):
        assert (ln == L).sum() >= 2
    assert c["aligned"] % LCo.TILE == 0 and c["aligned"] in st
    assert c["big"][0] in st and ln[np.searchsorted(st, c["big"][0])] == c["big"][1] > 2 * LCo.TILE


@pytest.mark.parametrize("zt", [0, 3000, "inside", 1 << 20])
def test_accepts_the_model(zt):
    c = LCo.edge_corpus(seed=3)
    data = c["data"]
    if zt == "inside":   # n - zt falls inside the several-tile word: the zone starts at that word
        zt = len(data) - (c["big"][0] + 100)
    r = check(data, zt, model_lexicon(data, zt))
    if 0 < zt < len(data):
        assert 0 < r["body"] <= len(data) - zt
    long_e = r["entry_len"] > LC.LMAX
    if zt == 0:
        # the 65- and 66-symbol words occur more than once: an entry per occurrence
        assert np.unique(r["entry_ids"][long_e]).shape[0] < int(long_e.sum())


@pytest.mark.parametrize("kind", ["random", "all", "first_only"])
def test_accepts_the_model_with_external_starts(kind):
    data = LCo.edge_corpus(seed=4, tiles=5)["data"]
    n = len(data)
    ws = {"random": LCo.random_starts(n, 9), "all": np.ones(n, np.uint8),
          "first_only": np.concatenate([[1], np.zeros(n - 1, np.uint8)]).astype(np.uint8)}[kind]
    for zt in (0, 500):
        r = check(data, zt, model_lexicon(data, zt, ws), ws)
        assert r["body"] <= n - zt


def test_expand_rebuilds_the_body(edge):
    data, zt, lx = edge
    r = check(data, zt, lx)
    assert np.array_equal(LC.expand(lx["store"], lx["occ"]), r["stream"][: r["body"]])


def _short_entry(lx, min_mul=1, skip=0):
    e0, el = LC.split_store(lx["store"])
    em = lx["mul"][e0]
    e = int(np.flatnonzero((el <= LC.LMAX) & (el >= 3) & (em >= min_mul))[skip])
    return e, int(e0[e]), int(el[e])


def _reject(edge, lx, reason):
    data, zt, _ = edge
    with pytest.raises(LC.LexiconMismatch) as ei:
        check(data, zt, lx)
    assert ei.value.reason == reason, str(ei.value)


def test_rejects_multiplicity_off_by_one(edge):
    lx = _copy(edge[2])
    _, a, L = _short_entry(lx)
    lx["mul"][a: a + L] += 1   # over the whole word: still constant, still 0 at the separator
    _reject(edge, lx, "multiplicity")


def test_rejects_swapped_occurrences(edge):
    lx = _copy(edge[2])
    a, b = _short_entry(lx, skip=0)[0], _short_entry(lx, skip=1)[0]
    ja, jb = lx["occ"] == a, lx["occ"] == b
    assert ja.any() and jb.any()
    lx["occ"][ja], lx["occ"][jb] = b, a
    _reject(edge, lx, "occ_entry")


def test_rejects_short_word_stored_twice(edge):
    lx = _copy(edge[2])
    e, a, L = _short_entry(lx, min_mul=2)
    m = int(lx["mul"][a])
    ne = lx["info"]["entries"]
    lx["store"] = np.concatenate([lx["store"], lx["store"][a: a + L + 1]])
    lx["mul"][a: a + L] = m - 1                                   # the count split m - 1 : 1 ...
    lx["mul"] = np.concatenate([lx["mul"], np.append(np.ones(L, np.uint32), np.uint32(0))])
    lx["occ"][np.flatnonzero(lx["occ"] == e)[-1]] = ne            # ... and the occurrences with it
    lx["info"].update(entries=ne + 1, store_symbols=int(lx["store"].shape[0]))
    assert np.array_equal(LC.expand(lx["store"], lx["occ"]), LC.expand(edge[2]["store"], edge[2]["occ"]))
    _reject(edge, lx, "short_duplicate")


def test_rejects_separator_with_multiplicity(edge):
    lx = _copy(edge[2])
    _, a, L = _short_entry(lx)
    lx["mul"][a + L] = 1
    _reject(edge, lx, "mul_separator")


def test_rejects_literal_replaced_by_entry(edge):
    lx = _copy(edge[2])
    j = int(np.flatnonzero(lx["occ"] & LC.LIT)[1])
    lx["occ"][j] = 0
    _reject(edge, lx, "occ_literal")


def test_rejects_zone_start_moved_by_one_word(edge):
    data, zt, good = edge
    Zs = good["info"]["body"]
    # a lexicon consistent in itself, of the body that ends one word earlier / later
    s = LC.reference_stream(data, None, 4)
    st = np.flatnonzero(LC.starts_mask(s, WS, 0xFFFF))
    k = int(np.searchsorted(st, Zs))
    assert st[k] == Zs
    for other in (int(st[k - 1]), int(st[k + 1])):
        lx = model_lexicon(data, len(data) - other)
        assert lx["info"]["body"] == other
        check(data, len(data) - other, lx)          # right for its own zone target
        _reject(edge, lx, "zone_start")


def test_rejects_flipped_word_start_bit_in_store(edge):
    lx = _copy(edge[2])
    _, a, L = _short_entry(lx)
    lx["store"][a + 1] ^= WS
    _reject(edge, lx, "dictionary")
    lx = _copy(edge[2])
    lx["store"][a] ^= WS   # the word's first symbol
    _reject(edge, lx, "dictionary")
