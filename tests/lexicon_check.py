"""numpy reference checker of a word lexicon — TEST INFRASTRUCTURE ONLY.

``check_piece`` takes what ``gbpe_lexshard_build`` leaves for one piece of a
corpus (STORE, MUL, OCC, ZONE and the info struct) and checks it, with integer
equality only, against the stream the oracle's ``prepare_symbols`` makes of the
piece's bytes: the zone start, the words of the body, every word's multiplicity
and the occurrence list.  ``check_root_map`` does the same for the word-id map
``gbpe_trainer_create_from_lexicon`` returns for concatenated stores.

Nothing here depends on the order of the entries (the build numbers short words
by hash slot and long words by an atomic counter), and nothing loops over words
in Python: words are grouped by length, every group is one 2-D gather packed
into u64 columns (a symbol is its token and its word-start bit, ``bits`` wide),
and groups are compared through ``np.unique``.

A rejected lexicon raises ``LexiconMismatch`` whose ``reason`` names the check.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import bpe_oracle as O  # noqa: E402

LIT = 0x80000000
LMAX = 64   # lexicon.h LX_LMAX: words up to this many symbols are deduplicated


class LexiconMismatch(AssertionError):
    def __init__(self, reason: str, detail: str = ""):
        super().__init__(f"{reason}: {detail}" if detail else reason)
        self.reason = reason


def _need(cond, reason, detail=""):
    if not cond:
        raise LexiconMismatch(reason, detail() if callable(detail) else detail)


def layout(bps: int):
    """(dtype, word-start bit, token mask) of a piece's symbols: u16 with bit 15, or u32 with bit 16"""
    return (np.uint16, 0x8000, 0x7FFF) if bps == 2 else (np.uint32, O.WORD_START_BIT, O.TOKEN_MASK)


def reference_stream(data, word_starts, bps: int) -> np.ndarray:
    """the oracle's symbols of the piece, in the piece's layout"""
    s = O.prepare_symbols(bytes(data), word_starts)
    dt, ws, tm = layout(bps)
    if bps == 4:
        return s.astype(np.uint32)
    tok = s & O.TOKEN_MASK
    assert int(tok.max(initial=0)) <= tm
    return (tok | np.where(s & O.WORD_START_BIT, ws, 0)).astype(dt)


def starts_mask(s: np.ndarray, ws: int, tm: int) -> np.ndarray:
    """positions no counted pair spans (lexshard_model._starts, lexicon.h lx_is_start):
    position 0, a word-start bit, or token 0 on either side"""
    st = np.zeros(s.shape[0], dtype=bool)
    if s.shape[0]:
        t = s.astype(np.uint32)
        tok = t & tm
        st[0] = True
        st[1:] = ((t[1:] & ws) != 0) | (tok[1:] == 0) | (tok[:-1] == 0)
    return st


def zone_start(s: np.ndarray, zone_target: int, ws: int, tm: int) -> int:
    """ls_build's zone start: n for no zone, 0 for a zone holding the whole piece, else the
    last position at or before n - zone_target that no counted pair spans"""
    n = int(s.shape[0])
    if zone_target >= n:
        return 0
    if zone_target == 0:
        return n
    return int(np.flatnonzero(starts_mask(s, ws, tm)[: n - zone_target + 1])[-1])


def _codes(s: np.ndarray, ws: int, tm: int) -> np.ndarray:
    """symbol -> (token << 1) | word start: a dense code for packing"""
    t = s.astype(np.uint64)
    return ((t & np.uint64(tm)) << np.uint64(1)) | ((t & np.uint64(ws)) != 0).astype(np.uint64)


def _pack(code: np.ndarray, starts: np.ndarray, L: int, bits: int) -> np.ndarray:
    """[len(starts), ceil(L / k)] u64: the L codes from each start, k = 64 // bits to a column"""
    k = 64 // bits
    ncol = -(-L // k)
    if starts.shape[0] < L:   # few long words: one gather
        rows = np.zeros((starts.shape[0], ncol * k), np.uint64)
        rows[:, :L] = code[starts[:, None] + np.arange(L, dtype=np.int64)[None, :]]
        sh = (np.arange(k, dtype=np.uint64) * np.uint64(bits))[None, None, :]
        return (rows.reshape(starts.shape[0], ncol, k) << sh).sum(axis=2, dtype=np.uint64)
    out = np.zeros((starts.shape[0], ncol), np.uint64)
    for i in range(L):   # (over a word's symbols, at most the longest word's length: not over words)
        out[:, i // k] |= code[starts + i] << np.uint64((i % k) * bits)
    return out


def _group_ids(rows: np.ndarray):
    """(ids, n distinct) of the rows of a packed [N, ncol] array"""
    if rows.shape[1] == 1:
        u, inv = np.unique(rows[:, 0], return_inverse=True)
    else:
        u, inv = np.unique(rows, axis=0, return_inverse=True)
    return inv.reshape(-1).astype(np.int64), int(u.shape[0])


def word_ids(segs):
    """Content ids shared by several word lists.  ``segs``: a list of (code array,
    word starts, word lengths); returns one int64 id array per list — two words, of
    any list, get the same id iff their symbols are equal — and each word's length
    can be read back from the inputs.  Ids are not dense."""
    bits = max(int(c.max(initial=0)) for c, _, _ in segs).bit_length() or 1
    out = [np.full(st.shape[0], -1, np.int64) for _, st, _ in segs]
    base = 0
    for L in np.unique(np.concatenate([ln for _, _, ln in segs])).tolist():
        sel = [np.flatnonzero(ln == L) for _, _, ln in segs]
        rows = np.concatenate([_pack(c, st[i].astype(np.int64), L, bits) for (c, st, _), i in zip(segs, sel)])
        ids, nd = _group_ids(rows)
        o = 0
        for q, i in enumerate(sel):
            out[q][i] = base + ids[o: o + i.shape[0]]
            o += i.shape[0]
        base += nd
    return out


def split_store(store: np.ndarray):
    """(entry starts, entry lengths) of a store cut at its 0 separators"""
    seps = np.flatnonzero(store == 0)
    _need(store.shape[0] == 0 or (seps.shape[0] and seps[-1] == store.shape[0] - 1), "store_shape",
          "the store does not end with a separator")
    e0 = np.concatenate([[0], seps[:-1] + 1]).astype(np.int64) if seps.shape[0] else np.zeros(0, np.int64)
    return e0, (seps - e0).astype(np.int64)


def expand(store: np.ndarray, occ: np.ndarray) -> np.ndarray:
    """the stream an occurrence list spells over a store (lexicon.h k_lx_expand), in the store's layout"""
    e0, el = split_store(store)
    lit = (occ & LIT) != 0
    ent = np.where(lit, 0, occ).astype(np.int64)
    assert lit.all() or int(ent.max()) < e0.shape[0]
    src = np.concatenate([store, (occ[lit] & ~np.uint32(LIT)).astype(store.dtype)])
    ln = np.where(lit, 1, el[ent] if e0.size else 0).astype(np.int64)
    at = np.where(lit, store.shape[0] + np.cumsum(lit) - 1, e0[ent] if e0.size else 0).astype(np.int64)
    off = np.cumsum(ln) - ln
    return src[np.repeat(at - off, ln) + np.arange(int(ln.sum()), dtype=np.int64)]


def check_piece(data, zone_target: int, store, mul, occ, zone, info: dict, word_starts=None) -> dict:
    """Check one piece's lexicon; returns {"body", "stream", "entry_ids", "entry_mul", "entry_len"}:
    the body length, the reference stream, and per store entry a content id (shared with
    nothing outside this call), its multiplicity and its length."""
    bps = int(info["bytes_per_symbol"])
    dt, ws, tm = layout(bps)
    store, zone = np.asarray(store), np.asarray(zone)
    mul, occ = np.asarray(mul, dtype=np.uint32), np.asarray(occ, dtype=np.uint32)
    _need(store.dtype == dt and zone.dtype == dt, "layout", f"{store.dtype} / {zone.dtype} for {bps}-byte symbols")
    s = reference_stream(data, word_starts, bps)
    n = int(s.shape[0])
    _need(info["symbols"] == n, "stream", f"{info['symbols']} symbols, the reference {n}")

    # stream and zone
    Zs = zone_start(s, zone_target, ws, tm)
    _need(info["body"] == Zs, "zone_start", f"body {info['body']}, the reference {Zs}")
    _need(info["zone"] == n - Zs and zone.shape[0] == n - Zs, "zone", f"{info['zone']} / {zone.shape[0]} zone symbols "
          f"for {n - Zs}")
    _need(np.array_equal(zone, s[Zs:]), "zone", "the zone is not the stream's tail")

    # words of the body
    body = s[:Zs]
    wst = np.flatnonzero(starts_mask(body, ws, tm)).astype(np.int64)
    nw = int(wst.shape[0])
    wlen = np.diff(np.append(wst, Zs))
    _need(info["words"] == nw and occ.shape[0] == nw, "words", f"{info['words']} / {occ.shape[0]} words, the "
          f"reference {nw}")
    wlit = (body[wst].astype(np.uint32) & tm) == 0 if nw else np.zeros(0, bool)

    # store
    _need(info["store_symbols"] == store.shape[0] and mul.shape[0] == store.shape[0], "store_shape",
          f"{info['store_symbols']} store symbols, {store.shape[0]} copied, {mul.shape[0]} multiplicities")
    e0, el = split_store(store)
    ne = int(e0.shape[0])
    _need(info["entries"] == ne, "store_shape", f"{info['entries']} entries, {ne} separators")
    _need(bool((el > 0).all()), "store_shape", "an empty entry")
    _need(int((el + 1).sum()) == store.shape[0], "store_shape", "entry sizes do not add up")
    _need(not bool((((store.astype(np.uint32) & tm) == 0) & (store != 0)).any()), "literal_in_store",
          "a token-0 symbol inside the store")

    # multiplicities: 0 at every separator, constant over a word
    seps = e0 + el
    _need(not mul[seps].any(), "mul_separator", lambda: f"separator {int(seps[np.flatnonzero(mul[seps])[0]])} "
          "carries a multiplicity")
    em = mul[e0] if ne else np.zeros(0, np.uint32)
    want = np.repeat(em, el + 1)
    want[seps] = 0
    _need(np.array_equal(mul, want), "mul_constant", "a multiplicity changes inside a word")
    _need(bool((em > 0).all()), "multiplicity", "an entry with multiplicity 0")

    # content ids of the body's non-literal words and of the entries
    ws_i = np.flatnonzero(~wlit)
    code_b, code_s = _codes(body, ws, tm), _codes(store, ws, tm)
    wid_nl, eid = word_ids([(code_b, wst[ws_i], wlen[ws_i]), (code_s, e0, el)])
    short_e = el <= LMAX
    short_w = wlen[ws_i] <= LMAX

    # short words: once in the store, {word -> multiplicity} = the reference's counts
    u_e, c_e = np.unique(eid[short_e], return_counts=True)
    _need(not (c_e > 1).any(), "short_duplicate", lambda: f"{int((c_e > 1).sum())} short word(s) stored more than once")
    u_w, c_w = np.unique(wid_nl[short_w], return_counts=True)
    _need(np.array_equal(u_e, u_w), "dictionary", lambda: f"{np.setdiff1d(u_e, u_w).shape[0]} stored short word(s) "
          f"not in the body, {np.setdiff1d(u_w, u_e).shape[0]} missing")
    m_e = em[short_e][np.argsort(eid[short_e], kind="stable")]
    _need(np.array_equal(m_e.astype(np.int64), c_w), "multiplicity",
          lambda: f"{int((m_e.astype(np.int64) != c_w).sum())} short word(s) with a wrong multiplicity")

    # long words: an entry per occurrence, multiplicity 1, the same multiset
    _need(bool((em[~short_e] == 1).all()), "long", "a long entry with a multiplicity other than 1")
    _need(np.array_equal(np.sort(eid[~short_e]), np.sort(wid_nl[~short_w])), "long",
          "the long entries are not the body's long words")
    _need(np.unique(occ[ws_i][~short_w]).shape[0] == int((~short_w).sum()), "long",
          "two long occurrences share an entry")

    # occurrences: a literal for a token-0 word, else an entry spelling the word
    lit_o = (occ & LIT) != 0
    _need(np.array_equal(lit_o, wlit), "occ_literal", lambda: f"word {int(np.flatnonzero(lit_o != wlit)[0])}: "
          "literal / entry mismatch")
    _need(np.array_equal(occ[wlit], LIT | body[wst[wlit]].astype(np.uint32)), "occ_literal", "a literal's symbol differs")
    o_nl = occ[ws_i].astype(np.int64)
    _need(not o_nl.size or int(o_nl.max()) < ne, "occ_entry", "an occurrence names no entry")
    bad = np.flatnonzero(eid[o_nl] != wid_nl) if o_nl.size else np.zeros(0, np.int64)
    _need(not bad.size, "occ_entry", lambda: f"{bad.shape[0]} occurrence(s) name another word's entry, first at word "
          f"{int(ws_i[bad[0]])}")
    return {"body": Zs, "stream": s, "entry_ids": eid, "entry_mul": em, "entry_len": el}


def dictionary(store, mul):
    """{word -> multiplicity} of a store in a canonical form (independent of the entry
    order): (lengths, packed rows as bytes, multiplicities), sorted by length then content.
    Long words (an entry per occurrence) appear once per entry."""
    dt_ws_tm = layout(np.asarray(store).dtype.itemsize)
    code = _codes(np.asarray(store), dt_ws_tm[1], dt_ws_tm[2])
    e0, el = split_store(np.asarray(store))
    em = np.asarray(mul, dtype=np.uint32)[e0] if e0.size else np.zeros(0, np.uint32)
    bits = int(code.max(initial=0)).bit_length() or 1
    out = []
    for L in np.unique(el).tolist():
        i = np.flatnonzero(el == L)
        rows = _pack(code, e0[i], L, bits)
        order = np.lexsort((em[i],) + tuple(rows[:, c] for c in range(rows.shape[1] - 1, -1, -1)))
        out.append((L, rows[order].tobytes(), em[i][order].tobytes()))
    return out


def check_root_map(stores, muls, wmap, body_words) -> int:
    """The root's word-id map over concatenated stores.  ``body_words``: (symbols of the
    concatenated bodies in the stores' layout, word starts, word lengths) of the non-literal
    words.  Short words: two entries share an id iff their words are equal, and an id's summed
    multiplicity is the word's count in the whole body.  Long words keep an entry, and so an
    id, per occurrence.  Ids are dense.  Returns the id count."""
    stores, muls = np.asarray(stores), np.asarray(muls, dtype=np.uint32)
    wmap = np.asarray(wmap, dtype=np.uint32).astype(np.int64)
    _, ws, tm = layout(stores.dtype.itemsize)
    e0, el = split_store(stores)
    ne = int(e0.shape[0])
    _need(wmap.shape[0] == ne, "map_shape", f"{wmap.shape[0]} map entries for {ne} store entries")
    em = muls[e0].astype(np.int64)
    bsym, bst, bln = body_words
    eid, wid = word_ids([(_codes(stores, ws, tm), e0, el), (_codes(np.asarray(bsym), ws, tm), bst, bln)])
    nid = int(wmap.max()) + 1 if ne else 0
    _need(np.array_equal(np.unique(wmap), np.arange(nid)), "map_dense", "the ids are not 0 .. k-1")
    sh = el <= LMAX
    # short: id <-> word is one to one
    pairs = np.unique(np.stack([eid[sh], wmap[sh]], axis=1), axis=0)
    _need(pairs.shape[0] == np.unique(eid[sh]).shape[0], "map_split", "one short word under two ids")
    _need(pairs.shape[0] == np.unique(wmap[sh]).shape[0], "map_merge", "two short words under one id")
    # long: an id each, none shared with a short word
    _need(np.unique(wmap[~sh]).shape[0] == int((~sh).sum()), "map_long", "two long entries share an id")
    _need(not np.intersect1d(wmap[~sh], wmap[sh]).size, "map_long", "a long entry shares a short word's id")
    _need(bool((em[~sh] == 1).all()), "map_long", "a long entry with a multiplicity other than 1")
    # summed multiplicity per word = its count in the whole body
    u_e, inv = np.unique(eid, return_inverse=True)
    tot = np.bincount(inv.reshape(-1), weights=em.astype(np.float64)).astype(np.int64)
    u_w, c_w = np.unique(wid, return_counts=True)
    _need(np.array_equal(u_e, u_w), "map_dictionary", "the stores' words are not the body's")
    _need(np.array_equal(tot, c_w), "map_multiplicity", lambda: f"{int((tot != c_w).sum())} word(s) with a wrong "
          "summed multiplicity")
    return nid
