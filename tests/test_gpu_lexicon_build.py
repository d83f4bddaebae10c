"""The word-lexicon build kernels (lexicon.h, trainer.h lx_analyze, train_lexshard.hip)
against the numpy reference checker (tests/lexicon_check.py), one process, through
``gpubpe.lexshard.GpuLexBackend``: what ``gbpe_lexshard_build`` leaves for a piece —
store, multiplicities, occurrence list, zone — must be exactly the words of the
oracle's stream, and the root's word-id map over several pieces' stores exactly
their deduplication.  Integer equality throughout.

The debug knobs (lxtwo, lxwg) are read from GBPE_DEBUG when a trainer is created
(trainer.h trainer_config); gbpe_lexshard_create makes a dense trainer through
trainer_create_impl, which calls it.
"""
from __future__ import annotations

import functools
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "gpu-bpe_amd"))

import lexicon_check as LC  # noqa: E402
import lexicon_corpora as LCo  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = LCo.TILE


@pytest.fixture(scope="module")
def gpu():
    from gpubpe import BPEEngine, _lib
    eng = BPEEngine(0).init()
    return _lib.load(), eng.device, eng   # (the engine owns the context: keep it alive)


def _parts(be, info):
    dt = LC.layout(info["bytes_per_symbol"])[0]
    bps, T = info["bytes_per_symbol"], info["store_symbols"]

    def get(part, nbytes, dtype):
        return be.export(part, nbytes, "cpu").numpy().view(dtype).copy()

    from gpubpe.lexshard import MUL, OCC, STORE, ZONE
    return {"store": get(STORE, T * bps, dt), "mul": get(MUL, T * 4, np.uint32),
            "occ": get(OCC, info["words"] * 4, np.uint32), "zone": get(ZONE, info["zone"] * bps, dt)}


def build_piece(gpu, data, vocab, zt, ws=None, flags=0):
    """(backend, info, parts) of one piece; the caller closes the backend"""
    from gpubpe.lexshard import GpuLexBackend
    lib, ctx, _ = gpu
    be = GpuLexBackend(lib, ctx, vocab, flags=flags)
    try:
        pre = be.create(data, len(data), False, ws)
        assert pre["symbols"] == len(data) and pre["body"] == len(data) and pre["entries"] == 0
        info = be.build(zt)
        return be, info, _parts(be, info)
    except BaseException:
        be.close()
        raise


def build_and_check(gpu, data, vocab, zt, ws=None):
    be, info, p = build_piece(gpu, data, vocab, zt, ws)
    try:
        assert info["bytes_per_symbol"] == (2 if vocab <= 0x8000 else 4)
        r = LC.check_piece(data, zt, p["store"], p["mul"], p["occ"], p["zone"], info, ws)
    finally:
        be.close()
    return info, p, r


# ── a. edges, one-stage path ──

@functools.lru_cache(maxsize=None)
def _edge():
    return LCo.edge_corpus(seed=3)


def _edge_cases():
    c = _edge()
    data, n = c["data"], len(c["data"])
    inside = n - (c["big"][0] + 100)            # n - zt falls inside the several-tile word
    at_tile = n - c["aligned"]                  # n - zt is the word start at a multiple of TILE
    ws_rand = LCo.random_starts(n, 9)
    ws_all = np.ones(n, np.uint8)
    ws_first = np.zeros(n, np.uint8)
    ws_first[0] = 1
    nonul = data.replace(b"\x00", b"z")          # (a token 0 always ends a word)
    cases = []
    for vocab in (1024, 65536):                 # u16 and u32 symbols
        for zt in (0, 3000, inside, at_tile, n, n + 5):
            cases.append((f"default_v{vocab}_zt{zt}", data, vocab, zt, None))
        for zt in (0, 3000):
            cases.append((f"extrandom_v{vocab}_zt{zt}", data, vocab, zt, ws_rand))
        cases.append((f"extall_v{vocab}_zt3000", data, vocab, 3000, ws_all))          # every position a start
        cases.append((f"extfirst_v{vocab}_zt0", nonul, vocab, 0, ws_first))            # one word: the whole piece
        cases.append((f"extfirst_v{vocab}_zt3000", nonul, vocab, 3000, ws_first))      # no start: a body of zero words
        # the piece ends one symbol before / after a tile boundary
        cases.append((f"minus1_v{vocab}_zt0", data[:-1], vocab, 0, None))
        cases.append((f"minus1_v{vocab}_zt3000", data[:-1], vocab, 3000, None))
        cases.append((f"plus1_v{vocab}_zt0", data + b"a", vocab, 0, None))
        cases.append((f"plus1_v{vocab}_zt3000", data + b"a", vocab, 3000, None))
        cases.append((f"plus1nul_v{vocab}_zt0", data + b"\x00", vocab, 0, None))
    for tiny in (b"a", b"ab", b"abc", b"\x00", b"\x00\x00", b"a\x00", b"\x00a", b"a b"):
        for zt in (0, 1, len(tiny)):
            cases.append((f"tiny_{tiny.hex()}_zt{zt}", tiny, 1024, zt, None))
    cases.append(("tiny_616263_u32_zt0", b"abc", 65536, 0, None))
    return cases


_EDGE_CASES = _edge_cases()


@pytest.mark.parametrize("name,data,vocab,zt,ws", _EDGE_CASES, ids=[c[0] for c in _EDGE_CASES])
def test_edges(gpu, name, data, vocab, zt, ws):
    info, p, r = build_and_check(gpu, data, vocab, zt, ws)
    n = len(data)
    if zt == 0:
        assert info["body"] == n and info["zone"] == 0
    if zt >= n:
        assert info["body"] == 0 and info["words"] == 0 and info["entries"] == 0 and info["zone"] == n
    if name.startswith("extfirst") and zt == 0:
        assert info["words"] == 1 and info["entries"] == 1 and info["store_symbols"] == n + 1
    if name.startswith("extfirst") and zt:
        assert info["body"] == 0 and info["words"] == 0
    if name.startswith("extall"):
        assert info["words"] == info["body"]
    # the occurrence list spells the body (the expansion, on the CPU)
    assert np.array_equal(LC.expand(p["store"], p["occ"]), r["stream"][: r["body"]])


def test_edges_cover_what_they_claim(gpu):
    c = _edge()
    data = c["data"]
    info, p, r = build_and_check(gpu, data, 1024, 0)
    el = r["entry_len"]
    assert (el == 63).sum() == 1 and (el == 64).sum() == 1          # deduplicated
    assert (el == 65).sum() >= 2 and (el == 66).sum() >= 2          # an entry per occurrence
    assert (el == c["big"][1]).sum() == 1
    assert int((p["occ"] & LC.LIT != 0).sum()) == data.count(b"\x00")
    # the zone starts at the word that starts at a multiple of TILE
    info, _, _ = build_and_check(gpu, data, 1024, len(data) - c["aligned"])
    assert info["body"] == c["aligned"] and info["body"] % TILE == 0


# ── b. workgroup LDS overflow, one-stage path ──

@functools.lru_cache(maxsize=None)
def _many_distinct():
    return LCo.distinct_words(100_000, seed=21, twice=0.5)


@pytest.mark.parametrize("knobs", ["", "lxwg=1"], ids=["default", "one_workgroup"])
def test_workgroup_table_overflow(gpu, monkeypatch, knobs):
    """~100K distinct words among ~154K: a k_lx_hash workgroup (256 threads x 16 words, or with
    lxwg=1 every word) sees more distinct words than its LX_LT = 2048-slot, 32-probe LDS table
    holds, so words overflow into direct lx_insert calls on the global table."""
    if knobs:
        monkeypatch.setenv("GBPE_DEBUG", knobs)
    else:
        monkeypatch.delenv("GBPE_DEBUG", raising=False)
    data = _many_distinct()
    info, p, r = build_and_check(gpu, data, 1024, 0)
    assert info["words"] == len(data) // 6 < (1 << 20)          # the one-stage path
    assert info["entries"] == 100_004 and info["entries"] > 16 * 2048


# ── c. two-stage path ──

N_TWO = 1_200_000


@functools.lru_cache(maxsize=None)
def _skewed():
    return LCo.skewed_words(N_TWO, pool=50_000, seed=22)


def _knob(monkeypatch, knobs):
    if knobs:
        monkeypatch.setenv("GBPE_DEBUG", knobs)
    else:
        monkeypatch.delenv("GBPE_DEBUG", raising=False)


def test_two_stage_equals_one_stage(gpu, monkeypatch):
    """1.2M words (>= 2^20: k_lx_hash<S,1024,8192> records + k_lx_fold) from a pool of 50K with
    hot words in every stage-1 workgroup; lxtwo=0 builds the same segment in one stage."""
    data = _skewed()
    out = []
    for knobs in ("lxtwo=1", "lxtwo=0"):
        _knob(monkeypatch, knobs)
        info, p, r = build_and_check(gpu, data, 1024, 0)
        assert info["words"] == N_TWO >= (1 << 20) + 1
        out.append((info, p, r))
    (ia, pa, ra), (ib, pb, rb) = out
    assert ia["entries"] == ib["entries"] and ia["store_symbols"] == ib["store_symbols"]
    assert LC.dictionary(pa["store"], pa["mul"]) == LC.dictionary(pb["store"], pb["mul"])
    ea, eb = LC.expand(pa["store"], pa["occ"]), LC.expand(pb["store"], pb["occ"])
    assert np.array_equal(ea, eb) and np.array_equal(ea, ra["stream"])


def test_two_stage_u32_with_zone(gpu, monkeypatch):
    """the two-stage build over u32 symbols, the body ending at a zone"""
    _knob(monkeypatch, "")
    data = _skewed()
    info, p, r = build_and_check(gpu, data, 65536, 100_001)
    assert info["words"] >= (1 << 20) + 1 and info["zone"] >= 100_001


@pytest.mark.parametrize("nw", [(1 << 20) - 1, 1 << 20], ids=["2p20m1_one_stage", "2p20_two_stage"])
def test_two_stage_threshold(gpu, monkeypatch, nw):
    """the switch (trainer.h lx_analyze: `two = lx_two && nw >= 2^20`, and hash_pass's nh >= 2^20):
    one word below it the default build is one-stage, at it two-stage"""
    _knob(monkeypatch, "")
    data = _skewed()[: 6 * nw]
    info, p, r = build_and_check(gpu, data, 1024, 0)
    assert info["words"] == nw


# ── d. table overflows of the two-stage build ──

FOLD_LT, FOLD_SLICES = 8192, 256   # lexicon.h: k_lx_fold's LDS table slots; lx_slice cuts a >= 2^20-slot table in 256
LX2_WORDS, LX2_LT = 1024 * 16, 8192   # trainer.h lx_analyze: words and LDS table slots of a stage-1 workgroup
N_FOLD = 2_500_000


def _distinct_count(data, width):
    w = np.frombuffer(data, np.uint8).reshape(-1, width).astype(np.uint64)
    return np.unique((w << (np.uint64(8) * np.arange(width, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)).shape[0]


def test_stage1_table_overflow(gpu, monkeypatch):
    """2.5M words, all distinct but four: every stage-1 workgroup (1024 threads x 16 words = 16,384
    words, nearly all distinct) overflows its 8192-slot LDS table into direct inserts on the
    global table, next to the records k_lx_fold inserts later.  (The words inserted directly
    never become records, so this corpus does not fill k_lx_fold's tables: test_fold_overflow.)"""
    _knob(monkeypatch, "")
    data = LCo.distinct_words(N_FOLD, seed=23, hot=4, hot_each=2000)
    nw = len(data) // 6
    assert (1 << 20) <= nw < 4 * (1 << 22)          # two-stage, below the sampled-table path
    info, p, r = build_and_check(gpu, data, 1024, 0)
    assert info["words"] == nw
    distinct = _distinct_count(data, 6)
    assert distinct == N_FOLD + 4 and distinct > FOLD_SLICES * FOLD_LT
    assert info["entries"] == distinct


FOLD_WINDOWS, FOLD_PER_WINDOW = 375, 6400


def test_fold_overflow(gpu, monkeypatch):
    """k_lx_fold's overflow from its LDS table into global inserts.  A stage-1 workgroup takes
    16,384 consecutive words; here each such window holds 6,400 distinct words of its own (and
    4 hot ones), which fit its 8192-slot table, so nearly every distinct word reaches the fold
    as a record.  The corpus holds 375 x 6,400 + 4 = 2,400,004 distinct words, more than the
    FOLD_SLICES x FOLD_LT = 256 x 8192 = 2,097,152 slots of all k_lx_fold LDS tables together:
    by pigeonhole a bucket gets more records than its table holds (with a uniform hash every
    bucket does: ~9.4K each) and the rest must go through the overflow insert."""
    _knob(monkeypatch, "")
    data, ws = LCo.windowed_words(FOLD_WINDOWS, LX2_WORDS, FOLD_PER_WINDOW, seed=25)
    nw = len(data) // 3
    assert nw == FOLD_WINDOWS * LX2_WORDS and (1 << 20) <= nw < 4 * (1 << 22)
    assert FOLD_PER_WINDOW + 4 < LX2_LT
    distinct = _distinct_count(data, 3)
    assert distinct == FOLD_WINDOWS * FOLD_PER_WINDOW + 4 and distinct > FOLD_SLICES * FOLD_LT
    info, p, r = build_and_check(gpu, data, 1024, 0, ws)
    assert info["words"] == nw and info["entries"] == distinct


# ── e. weighted analysis on the root ──

def _cut_at_word_starts(data, fracs, ws=None):
    s = LC.reference_stream(data, ws, 4)
    st = np.flatnonzero((s & 0x10000) != 0)
    cuts = [0] + [int(st[np.searchsorted(st, int(f * len(data)))]) for f in fracs] + [len(data)]
    return [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _root_case(gpu, pieces, vocab, flags=0):
    """Builds every piece with the host loop's zone targets, checks each, hands the stores and
    zones to a root trainer; returns (root backend, every backend with the root last, infos,
    parts, map, the checker's results, the concatenated stores and multiplicities)."""
    from gpubpe.lexshard import GpuLexBackend, LexShardTrainer
    bes, infos, parts, refs = [], [], [], []
    try:
        lib, ctx, _ = gpu
        tops = []
        for d in pieces:
            be = GpuLexBackend(lib, ctx, vocab, flags=flags)
            bes.append(be)
            tops.append(be.create(d, len(d), False, None)["top_count"])
        # the host loop's rule (lexshard.LexShardTrainer.zone_targets with the default zt knob)
        zts = LexShardTrainer.zone_targets(types.SimpleNamespace(sp_zt=5), np.array([len(d) for d in pieces]),
                                           int(sum(tops)))
        assert zts[-1] > 0
        for be, d, zt in zip(bes, pieces, zts):
            info = be.build(zt)
            p = _parts(be, info)
            refs.append(LC.check_piece(d, zt, p["store"], p["mul"], p["occ"], p["zone"], info))
            infos.append(info)
            parts.append(p)
        stores = np.concatenate([p["store"] for p in parts])
        muls = np.concatenate([p["mul"] for p in parts])
        zone = np.concatenate([p["zone"] for p in parts])
        root = GpuLexBackend(lib, ctx, vocab, flags=flags)
        bes.append(root)
        mp = root.root_create(stores, muls, zone, int(stores.shape[0]), int(zone.shape[0]),
                              int(sum(i["body"] for i in infos)), int(sum(i["entries"] for i in infos)))
        mp = mp.numpy().view(np.uint32).copy()
        return root, bes, infos, parts, mp, refs, stores, muls
    except BaseException:
        for be in bes:
            be.close()
        raise


def _check_root(infos, parts, mp, refs, stores, muls):
    bps = infos[0]["bytes_per_symbol"]
    _, ws, tm = LC.layout(bps)
    body = np.concatenate([r["stream"][: r["body"]] for r in refs])
    st = np.flatnonzero(LC.starts_mask(body, ws, tm)).astype(np.int64)
    ln = np.diff(np.append(st, body.shape[0]))
    nl = (body[st].astype(np.uint32) & tm) != 0
    return LC.check_root_map(stores, muls, mp, (body, st[nl], ln[nl]))


def _final_stream(root, bes, infos, mp):
    from gpubpe.lexshard import OCC
    occ, off = [], 0
    for be, info in zip(bes, infos):
        ne = info["entries"]
        be.remap(np.ascontiguousarray(mp[off: off + ne]), ne)
        off += ne
        occ.append(be.export(OCC, info["words"] * 4, "cpu").numpy().view(np.uint32).copy())
    occ = np.ascontiguousarray(np.concatenate(occ))
    return root.root_expand(occ, int(occ.shape[0]))


def _u32_stream(data):
    return LC.reference_stream(data, None, 4)


@pytest.mark.parametrize("vocab", [256 + 200, 65536], ids=["u16", "u32"])
def test_root_map_and_stream_small(gpu, monkeypatch, vocab):
    """three pieces of the edge corpus (long words and literals in the stores): the map, and the
    stream expanded from the remapped occurrence lists before any merge"""
    _knob(monkeypatch, "")
    data = _edge()["data"]
    pieces = _cut_at_word_starts(data, [0.3, 0.62])
    root, bes, infos, parts, mp, refs, stores, muls = _root_case(gpu, pieces, vocab)
    try:
        assert any((r["entry_len"] > LC.LMAX).any() for r in refs) and any((p["occ"] & LC.LIT).any() for p in parts)
        _check_root(infos, parts, mp, refs, stores, muls)
        fin = _final_stream(root, bes, infos, mp)
        assert np.array_equal(fin, _u32_stream(data))
    finally:
        for be in bes:
            be.close()


@pytest.mark.parametrize("exact", [False, True], ids=["reference", "exact"])
def test_root_merges_small(gpu, monkeypatch, exact):
    """200 merges over that lexicon: the merge list and the final stream equal the oracle's
    on the concatenated corpus, in both compaction modes"""
    import cpu_ref
    from gpubpe import _lib
    _knob(monkeypatch, "")
    data = _edge()["data"]
    vocab = 256 + 200
    want = cpu_ref.train_inc(data, vocab, exact=exact, want_symbols=True)
    pieces = _cut_at_word_starts(data, [0.3, 0.62])
    root, bes, infos, parts, mp, refs, stores, muls = _root_case(
        gpu, pieces, vocab, flags=_lib.GBPE_TRAIN_EXACT_COMPACTION if exact else 0)
    try:
        merges, early = [], False
        while len(merges) < 200 and not early:
            got, early = root.root_step(min(128, 200 - len(merges)))
            merges += got
            if not got:
                break
        assert merges == [list(m) for m in want["merges"]]
        assert early == want["early_stop"]
        fin = _final_stream(root, bes, infos, mp)
        assert np.array_equal(fin, np.asarray(want["symbols"], dtype=np.uint32))
    finally:
        for be in bes:
            be.close()


def test_root_map_two_stage_weighted(gpu, monkeypatch):
    """>= 2^19 + 1 concatenated store entries: the root's analysis sees a word and a separator
    per entry, so nw >= 2^20 and it takes the two-stage path with the stores' multiplicities
    as weights (k_lx_hash's wmul)."""
    # (vocab 1024: u16 symbols; 8 merges are stepped at the end)
    _knob(monkeypatch, "")
    rng = np.random.default_rng(24)
    ids = LCo.distinct_ids(rng, 400_000, 5)
    pieces = []
    for q in range(3):   # overlapping vocabularies: 200K distinct words each, half shared with the next piece
        mine = ids[q * 100_000: q * 100_000 + 200_000]
        w = np.concatenate([mine, mine[:: 3 + q], np.repeat(ids[:8], 500 * (q + 1))])
        rng.shuffle(w)
        pieces.append(LCo.decode_words(w, 5).tobytes())
    root, bes, infos, parts, mp, refs, stores, muls = _root_case(gpu, pieces, 1024)
    try:
        nent = sum(i["entries"] for i in infos)
        assert nent >= (1 << 19) + 1
        nid = _check_root(infos, parts, mp, refs, stores, muls)
        assert nid < nent   # words shared between pieces were merged
        fin = _final_stream(root, bes, infos, mp)
        assert np.array_equal(fin, _u32_stream(b"".join(pieces)))
        # the root's own multiplicities are not exported: they show in the pair counts, so the
        # first merges and their counts must be the oracle's on the concatenated corpus
        import cpu_ref
        want = cpu_ref.train_inc(b"".join(pieces), 256 + 8, want_symbols=False)
        got, _ = root.root_step(8)
        assert got == [list(m) for m in want["merges"]]
    finally:
        for be in bes:
            be.close()


# ── lex_check=1 ──

def train_with_knobs(gpu, data, merges, knobs, monkeypatch):
    """(merge list, stats) of a plain trainer over host bytes, GBPE_DEBUG = knobs"""
    import ctypes as C
    from gpubpe import _lib
    lib, ctx, _ = gpu
    _knob(monkeypatch, knobs)
    tr = C.c_void_p()
    opts = _lib.TrainOpts(target_vocab_size=256 + merges, vocab_size=256, next_token_id=256, batch_size=128, flags=0,
                          table_log2=0)
    try:
        _lib.check(lib.gbpe_trainer_create(ctx, data, len(data), None, 0, C.byref(opts), C.byref(tr)), ctx, "create")
        out, got = (C.c_uint32 * 512)(), []
        while len(got) < merges:
            nd, es = C.c_uint32(), C.c_uint32()
            _lib.check(lib.gbpe_trainer_step(tr, min(128, merges - len(got)), out, C.byref(nd), C.byref(es)), ctx, "step")
            got += [list(out[4 * i:4 * i + 4]) for i in range(nd.value)]
            if nd.value == 0 or es.value:
                break
        st = _lib.TrainerStats()
        lib.gbpe_trainer_stats_get(tr, C.byref(st))
        return got, st
    finally:
        if tr.value:
            lib.gbpe_trainer_destroy(tr)


def test_lex_check_accepts_a_sound_build(gpu, monkeypatch):
    """GBPE_DEBUG lex_check=1 fails a build whose lexicon does not expand to the body (trainer.h
    lx_check); on a sound build (two-stage size) the run goes on and gives the oracle's merges"""
    import cpu_ref
    data = _skewed()
    got, st = train_with_knobs(gpu, data, 8, "lexicon=1,lex_check=1", monkeypatch)
    assert st.lexicon_builds >= 1 and st.lexicon_fallbacks == 0
    want = cpu_ref.train_inc(data, 256 + 8, want_symbols=False)
    assert got == [list(m) for m in want["merges"]]
