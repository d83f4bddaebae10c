"""What the trie-encode corpora hold (no GPU): the plain reference against the
oracle on every corpus, and the coverage the GPU tests rely on — stated on the
reference's trace (where a walk started, where its match ended, the last byte it
read), never on what a kernel gives.
"""
import json
import os

import pytest

import bpe_oracle as O
import encode_corpora as E
from conftest import GOLDEN

PACKED_CS = (8, 24, 40, 72, 512, 520, 2048)   # k_trie_walk_v5 (cs % 8 == 0)
PLAIN_CS = (7, 9, 63, 65, 100)                # k_trie_walk
ALL_CS = PACKED_CS + PLAIN_CS + (16, 64)


def _arrays(vocab):
    blob = O.compile_vocab_to_trie(vocab)
    return O.parse_trie_buffers(blob, O.parse_header(blob))


@pytest.fixture(scope="module")
def vocabs():
    v = E.edge_vocab()
    w = E.wide(v)
    return {"narrow": (v, E.ref_trie(v), _arrays(v)), "wide": (w, E.ref_trie(w), _arrays(w))}


@pytest.fixture(scope="module")
def nm(vocabs):
    return E.near_miss(vocabs["narrow"][0])


def _same(data, voc, cs):
    _, trie, arrays = voc
    got = E.ref_encode(data, trie, cs)[0]
    want = O.encode_chunked(data, arrays[0], arrays[1], cs).tolist()
    assert got == want, (cs, next(i for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b))


# ── the vocabularies are what they say ───────────────────────────────────────

def test_edge_vocab_shape(vocabs):
    v, trie, _ = vocabs["narrow"]
    ents = {bytes(e) for e in v}
    assert all(bytes([b]) in ents for b in range(256))
    assert {len(e) for e in v if len(e) > 1 and set(e) == {E.A}} == set(E.LADDER)
    # xy < its 40-byte < its 70-byte extension, nothing else on the path; xz < 130 bytes, nothing between
    on_xy = sorted(len(e) for e in ents if E.XY70.startswith(e) and len(e) > 1)
    on_xz = sorted(len(e) for e in ents if E.XZ130.startswith(e) and len(e) > 1)
    assert on_xy == [2, 40, 70] and on_xz == [2, 130]
    # a 2-byte leaf below the root, a one-byte leaf at the root
    node = trie[E.LEAF2[0]][E.LEAF2[1]]
    assert set(node) == {E._ID}
    assert set(trie[E.HASH]) == {E._ID} and all(set(trie[b]) == {E._ID} for b in E._PAD)
    assert len(E.long_tokens(v)) == 12 and max(map(len, E.long_tokens(v))) == 200


def test_wide_moves_every_multibyte_id(vocabs):
    v, w = vocabs["narrow"][0], vocabs["wide"][0]
    assert w[:256] == v[:256] and all(e == [] for e in w[256:70256]) and w[70256:] == v[256:]
    assert len(w) - 1 >= 65536


@pytest.mark.parametrize("m", E.BOUNDARY_IDS)
def test_boundary_vocab(m):
    v = E.boundary_vocab(m)
    assert len(v) == m + 1 and bytes(v[m]) == E.B_LONG and bytes(v[m - 1]) == E.B_MID and bytes(v[300]) == E.B_SHORT
    assert sum(1 for e in v[256:] if e) == 3
    text = E.boundary_text()
    for cs in (64, 7):
        toks, trace = E.ref_encode(text, v, cs)
        assert {m, m - 1, 300} <= set(toks) and any(t < 256 for t in toks)
        assert toks == O.encode_chunked(text, *_arrays(v), cs).tolist()
        # near-misses of the longest token: the walk read past a shorter match
        assert sum(1 for (s, e, f), t in zip(trace, toks) if t == m - 1 and f > e) >= 10


def test_empty_root_blob():
    blob = E.empty_root_blob()
    hdr = O.parse_header(blob)
    nodes, edges = O.parse_trie_buffers(blob, hdr)
    assert hdr["nodeCount"] == 1 and hdr["edgeCount"] == 0 and nodes.tolist() == [0, 0, 0xFFFFFFFF] and edges.size == 0
    text = E.holes_corpus()
    assert O.encode_chunked(text, nodes, edges, 8).tolist() == list(text)


# ── the reference against the oracle ─────────────────────────────────────────

@pytest.mark.parametrize("cs", ALL_CS)
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_reference_matches_oracle_near_miss_and_phases(vocabs, nm, width, cs):
    _same(nm, vocabs[width], cs)
    for probe in E.PROBES:
        _same(E.phase_sweep(probe, cs), vocabs[width], cs)


@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_reference_matches_oracle_counts_raw_tails(vocabs, nm, width):
    voc = vocabs[width]
    for cs in (8, 16, 512):
        _same(E.count_sweep(voc[0], cs), voc, cs)
    _same(E.count_sweep(voc[0], 2048, E.COMPACT_TARGETS), voc, 2048)
    for cs in (512, 2048):
        _same(E.all_raw(3 * 2048 + 5), voc, cs)
    for cs in (8, 512, 7):
        for t in E.tails(nm[5000:7200], cs):
            _same(t, voc, cs)


def test_reference_matches_oracle_holes():
    v = E.holes_vocab()
    for voc in (v, E.wide(v)):
        triple = (voc, E.ref_trie(voc), _arrays(voc))
        for cs in (8, 512, 7):
            _same(E.holes_corpus(), triple, cs)


def test_reference_matches_known_answers():
    ka = json.load(open(os.path.join(GOLDEN, "known_answers.json")))
    assert ka["encode"]
    for c in ka["encode"]:
        if "vocab_holes" in c:
            voc = [[] for _ in range(c["vocab_holes"]["size"])]
            for k, e in c["vocab_holes"]["entries"].items():
                voc[int(k)] = e
        else:
            voc = O.vocab_from_merges(c["merges"]).entries
        text = bytes.fromhex(c["text_hex"]) if "text_hex" in c else c["text"].encode("utf-8")
        assert E.ref_encode(text, voc, c["chunk_size"])[0] == c["tokens"], c["name"]


# ── coverage, from the trace alone ───────────────────────────────────────────

def _win(p, cs):
    return (p % cs) // 64


@pytest.mark.parametrize("cs,need", [(512, 64), (2048, 64), (72, 32), (520, 32)])
def test_walks_leave_their_window_at_every_offset(vocabs, nm, cs, need):
    _, trace = E.ref_encode(nm, vocabs["narrow"][1], cs)
    offsets = {(s % cs) % 64 for s, _, f in trace if _win(s, cs) != _win(f, cs)}
    backs = sum(1 for _, e, f in trace if _win(e - 1, cs) < _win(f, cs))
    print(f"cs={cs}: walks leave their window from {len(offsets)} of 64 offsets; {backs} backtracks across a window")
    assert len(offsets) >= need
    assert backs >= 100


@pytest.mark.parametrize("cs", PACKED_CS + PLAIN_CS)
def test_phase_sweep_puts_the_probe_at_every_offset(cs):
    for probe in E.PROBES:
        data = E.phase_sweep(probe, cs)
        period = data.index(probe, 1)
        starts = {(i % cs) % 64 for i in range(0, len(data), period)}
        assert data == data[:period] * (len(data) // period)
        assert starts == set(range(min(64, cs))), (cs, len(starts))
        assert len(data) <= 300_000


def test_long_spans_and_long_backtracks(vocabs, nm):
    _, trace = E.ref_encode(nm, vocabs["narrow"][1], 2048)
    span = max(f - s for s, _, f in trace)
    back = max(f - (e - 1) for _, e, f in trace)
    print(f"longest walk {span} bytes, longest backtrack {back} bytes")
    assert span >= 128 and back > 64
    assert len(nm) <= 300_000


@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_count_sweep_token_counts(vocabs, width):
    voc, trie, _ = vocabs[width]
    data = E.count_sweep(voc, 512)
    counts = E.chunk_counts(E.ref_encode(data, trie, 512)[1], 512, len(data))
    assert len(data) <= 300_000 and len(data) % 512 == len(E.COUNT_TAIL)
    have = set(counts[:-1])
    assert have >= set(range(8, 101)) | {255, 256, 257, 511, 512}
    assert counts[:-1] == sorted(have)              # one chunk per count
    print(f"{width}: cs=512 counts {min(have)}..{max(have)}, {len(have)} distinct")
    for cs in (8, 16):                              # at most two token vectors per chunk
        d = E.count_sweep(voc, cs)
        c = E.chunk_counts(E.ref_encode(d, trie, cs)[1], cs, len(d))
        assert set(c[:-1]) == set(E.reachable_counts(voc, cs)) and max(c) == cs and min(c) <= 3


def test_compaction_neighbours(vocabs):
    voc, trie, _ = vocabs["narrow"]
    data = E.count_sweep(voc, 2048, E.COMPACT_TARGETS)
    counts = E.chunk_counts(E.ref_encode(data, trie, 2048)[1], 2048, len(data))
    assert counts[:-1] == E.COMPACT_TARGETS
    groups = [counts[g:g + 4] for g in range(0, len(counts), 4)]
    spread = max(max(g) - min(g) for g in groups)
    print(f"largest spread of token counts inside a group of four chunks: {spread}")
    assert spread > 256
    # more than one pass of difference inside a wave's four chunks
    assert any((max(g) + 255) // 256 - (min(g) + 255) // 256 > 1 for g in groups)
    raw = E.all_raw(2 * 2048)
    assert E.chunk_counts(E.ref_encode(raw, trie, 2048)[1], 2048, len(raw)) == [2048, 2048]


def test_holes_root_cases():
    voc = E.holes_vocab()
    trie = E.ref_trie(voc)
    data = E.holes_corpus()
    for cs in (8, 512, 7):
        toks, trace = E.ref_encode(data, trie, cs)
        led, not_led, nothing = 0, 0, 0
        for (s, e, _), t in zip(trace, toks):
            b = data[s]
            if b not in trie:
                nothing += 1
                assert t == b and e == s + 1
            elif E._ID not in trie[b]:
                if e > s + 1:
                    led += 1
                else:
                    not_led += 1
                    assert t == b
        print(f"cs={cs}: hole led to a match {led}, did not {not_led}, byte starts nothing {nothing}")
        assert led >= 10 and not_led >= 10 and nothing >= 10
    assert all(b in trie and E._ID not in trie[b] for b in E.HOLE_BYTES)
    assert all(b not in trie for b in E.NOTHING_BYTES)


def test_tail_lengths():
    for cs in (8, 512, 7):
        ns = E.tail_lengths(2200, cs)
        assert {n % 64 for n in ns} >= set(E.TAIL_MOD64)
        assert {n % cs for n in ns} >= {r for r in E.TAIL_MODCS if r < cs}
        assert max(ns) <= 2200 and len(ns) <= 30
