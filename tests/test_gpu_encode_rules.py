"""The single-stream trie-encode kernels (k_trie_walk_v5, k_trie_walk,
k_chunk_compact4, gbpe_trie_upload) at their window, burst, pass and id-width
edges, against the CPU oracle.  Every comparison is exact; every expected value is
O.encode_chunked.  What the corpora hold (walks that leave their window, backtracks
across one, every per-chunk token count, ...) is asserted without a GPU in
test_encode_corpora.py.
"""
import ctypes as C

import numpy as np
import pytest

import bpe_oracle as O
import encode_corpora as E
from encode_dev import BatchDev, DevBuffers

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5
PACKED_CS = (8, 24, 40, 72, 512, 520, 2048)   # k_trie_walk_v5: windows off their 16- and 64-byte boundaries
PLAIN_CS = (7, 9, 63, 65, 100)                # k_trie_walk and its word cache
WIDTHS = ["narrow", "wide"]


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


class _Voc:
    """A vocabulary with its oracle arrays, its uploaded trie and the oracle's answers."""

    def __init__(self, eng, vocab=None, blob=None):
        from gpubpe import TrieTokenizer
        self.vocab = vocab
        self.blob = O.compile_vocab_to_trie(vocab) if blob is None else blob
        self.arrays = O.parse_trie_buffers(self.blob, O.parse_header(self.blob))
        self.tok = TrieTokenizer(eng, self.blob, vocab)
        self._want = {}

    def want(self, data, cs):
        key = (data, cs)
        if key not in self._want:
            self._want[key] = O.encode_chunked(data, self.arrays[0], self.arrays[1], cs).astype(np.uint32)
        return self._want[key]

    def encode(self, data, cs):
        self.tok.chunk_size = cs
        return self.tok.encode_bytes(data)

    def check(self, data, cs, what=""):
        got, want = self.encode(data, cs), self.want(data, cs)
        assert got.shape == want.shape and np.array_equal(got, want), (what, cs, _first_diff(got, want))


def _first_diff(got, want):
    m = min(got.shape[0], want.shape[0])
    d = np.nonzero(got[:m] != want[:m])[0]
    return ("token", int(d[0]), int(got[d[0]]), int(want[d[0]])) if d.size else ("count", got.shape[0], want.shape[0])


@pytest.fixture(scope="module")
def vocs(eng):
    v = E.edge_vocab()
    out = {"narrow": _Voc(eng, v), "wide": _Voc(eng, E.wide(v))}
    yield out
    for x in out.values():
        x.tok.destroy()


@pytest.fixture(scope="module")
def nm():
    return E.near_miss(E.edge_vocab())


def _device_encode(eng, trie, data, cs, offset=0, out_cap=None, guard=64):
    """gbpe_encode_device on an input buffer of exactly offset + len(data) bytes, the
    bytes at `offset`; returns (status, *n_out, the out_cap + guard words of d_out)."""
    dev = DevBuffers(eng)
    try:
        n = len(data)
        base = dev.alloc(offset + n)
        d_in = C.c_void_p(base.value + offset)
        dev.put(d_in, np.frombuffer(data, dtype=np.uint8))
        cap = n if out_cap is None else out_cap
        d_out = dev.alloc(4 * (cap + guard), np.full(cap + guard, GUARD, np.uint32))
        n_out = C.c_uint64(0xDEAD)
        rc = dev.lib.gbpe_encode_device(dev.ctx, trie, d_in, n, cs, d_out, cap, C.byref(n_out))
        return rc, int(n_out.value), dev.fetch(d_out, cap + guard, np.uint32)
    finally:
        dev.free()


def _host_encode(eng, trie, data, cs, out_cap, guard=64):
    """gbpe_encode into a guarded host array of out_cap + guard words."""
    from gpubpe import _lib
    out = np.full(out_cap + guard, GUARD, dtype=np.uint32)
    n_out = C.c_uint64(0xDEAD)
    buf = C.create_string_buffer(data, len(data))
    rc = _lib.load().gbpe_encode(eng.device, trie, buf, len(data), cs, out.ctypes.data_as(_lib.u32p), out_cap,
                                 C.byref(n_out))
    return rc, int(n_out.value), out


# ── windows, backtracking ────────────────────────────────────────────────────

@pytest.mark.parametrize("cs", PACKED_CS + PLAIN_CS)
@pytest.mark.parametrize("width", WIDTHS)
def test_windows_and_backtracking(vocs, nm, width, cs):
    voc = vocs[width]
    voc.check(nm, cs, "near_miss")
    for i, probe in enumerate(E.PROBES):
        voc.check(E.phase_sweep(probe, cs), cs, f"phase_sweep {i}")


# ── the store bursts ─────────────────────────────────────────────────────────

@pytest.mark.parametrize("width", WIDTHS)
def test_burst_counts(vocs, width):
    voc = vocs[width]
    voc.check(E.count_sweep(voc.vocab, 512), 512, "every count 8..512")
    # every chunk ends with at most one or two vectors: the queue never fills
    voc.check(E.count_sweep(voc.vocab, 8), 8)
    voc.check(E.count_sweep(voc.vocab, 16), 16)


# ── compaction passes ────────────────────────────────────────────────────────

@pytest.mark.parametrize("case", ["raw", "neighbours", "two-scan-blocks"])
@pytest.mark.parametrize("width", WIDTHS)
def test_compaction_passes(vocs, width, case):
    voc = vocs[width]
    if case == "raw":            # 2048 tokens per chunk: 8 passes; 512: 2 passes; a short last chunk
        raw = E.all_raw(3 * 2048 + 5)
        voc.check(raw, 2048)
        voc.check(raw, 512)
        assert np.array_equal(voc.want(raw, 2048), np.frombuffer(raw, dtype=np.uint8))
    elif case == "neighbours":   # 8 passes next to 1 inside one wave's four chunks; 19 chunks
        voc.check(E.count_sweep(voc.vocab, 2048, E.COMPACT_TARGETS), 2048)
    else:                        # 4115 chunks of one and two passes: two blocks of the count scan
        data = E.many_chunks(voc.vocab)
        assert (len(data) + 263) // 264 == 4115
        voc.check(data, 264)


# ── inputs that end inside a window ──────────────────────────────────────────

@pytest.mark.parametrize("width", WIDTHS)
def test_tails(eng, vocs, nm, width):
    from gpubpe import _lib
    voc = vocs[width]
    text = nm[5000:7200]
    for cs in (8, 512, 7):
        for t in E.tails(text, cs):
            want = voc.want(t, cs)
            got = voc.encode(t, cs)
            assert np.array_equal(got, want), ("gbpe_encode", cs, len(t), _first_diff(got, want))
            # the device input buffer holds exactly len(t) bytes
            rc, n_out, out = _device_encode(eng, voc.tok._trie, t, cs, guard=8)
            assert rc == _lib.GBPE_OK and n_out == want.shape[0], (cs, len(t))
            assert np.array_equal(out[:n_out], want), ("gbpe_encode_device", cs, len(t), _first_diff(out[:n_out], want))


# ── device pointers at every accepted alignment ──────────────────────────────

@pytest.mark.parametrize("width", WIDTHS)
def test_device_pointer_alignment(eng, vocs, nm, width):
    from gpubpe import _lib
    voc = vocs[width]
    data = nm[:12000] + E.phase_sweep(E.PROBES[1], 8)[:4001]
    for cs in (8, 512, 7):
        want = voc.want(data, cs)
        rc, n0, out0 = _device_encode(eng, voc.tok._trie, data, cs)
        assert rc == _lib.GBPE_OK and np.array_equal(out0[:n0], want), (cs, 0)
        for off in (4, 8, 12):
            rc, n_out, out = _device_encode(eng, voc.tok._trie, data, cs, offset=off)
            assert rc == _lib.GBPE_OK and n_out == n0, (cs, off)
            assert np.array_equal(out[:n_out], out0[:n0]) and np.array_equal(out[:n_out], want), (cs, off)
            assert np.all(out[len(data):] == GUARD)
        for off in (1, 2, 3):
            rc, n_out, out = _device_encode(eng, voc.tok._trie, data, cs, offset=off)
            assert rc == _lib.GBPE_E_INVALID and n_out == 0, (cs, off)
            assert np.all(out == GUARD), (cs, off)


# ── capacity ─────────────────────────────────────────────────────────────────

@pytest.mark.parametrize("width", WIDTHS)
def test_capacity_single_stream(eng, vocs, nm, width, monkeypatch):
    from gpubpe import _lib
    voc = vocs[width]
    data, cs = nm[:20000], 64           # 64 * cs = 4096: five slices under encode_slice=4096
    want = voc.want(data, cs)
    total = int(want.shape[0])
    trie = voc.tok._trie
    for sliced in (False, True):
        if sliced:
            monkeypatch.setenv("GBPE_DEBUG", "encode_slice=4096")
        for cap in (0, 1, total - 1):
            rc, n_out, out = _host_encode(eng, trie, data, cs, cap)
            assert rc == _lib.GBPE_E_CAPACITY and n_out == total, (sliced, cap)
            assert np.all(out[cap:] == GUARD), (sliced, cap)
        rc, n_out, out = _host_encode(eng, trie, data, cs, total)
        assert rc == _lib.GBPE_OK and n_out == total and np.array_equal(out[:total], want), sliced
        assert np.all(out[total:] == GUARD)
    monkeypatch.delenv("GBPE_DEBUG")
    for cap in (0, 1, total - 1):
        rc, n_out, out = _device_encode(eng, trie, data, cs, out_cap=cap)
        assert rc == _lib.GBPE_E_CAPACITY and n_out == total, cap
        assert np.all(out[cap:] == GUARD), cap            # nothing at or beyond d_out[out_cap]
        assert np.array_equal(out[:cap], want[:cap]), cap
    rc, n_out, out = _device_encode(eng, trie, data, cs, out_cap=total)
    assert rc == _lib.GBPE_OK and n_out == total and np.array_equal(out[:total], want)
    assert np.all(out[total:] == GUARD)


# ── the u16 / u32 scratch and the packed-record limits ───────────────────────

@pytest.mark.parametrize("m", E.BOUNDARY_IDS)
def test_id_width_boundaries(eng, m):
    from gpubpe import _lib
    voc = _Voc(eng, blob=O.compile_vocab_to_trie(E.boundary_vocab(m)))
    try:
        max_id = C.c_uint32()
        assert _lib.load().gbpe_trie_info(voc.tok._trie, None, None, C.byref(max_id)) == _lib.GBPE_OK
        assert max_id.value == m
        text = E.boundary_text()
        for cs in (64, 7):            # the packed walk while the records pack (m < 0xFFFFF); the plain walk
            voc.check(text, cs)
            got = set(voc.want(text, cs).tolist())
            assert {m, m - 1, 300} <= got and min(got) < 256, cs
    finally:
        voc.tok.destroy()


# ── leaves, holes, an empty root ─────────────────────────────────────────────

def test_holes_leaves_empty_root(eng):
    text = E.holes_corpus()
    holes = E.holes_vocab()
    for vocab in (holes, E.wide(holes)):
        voc = _Voc(eng, vocab)
        try:
            for cs in (8, 512, 7):
                voc.check(text, cs, "holes")
        finally:
            voc.tok.destroy()
    voc = _Voc(eng, blob=E.empty_root_blob())
    try:
        for cs in (8, 512, 7):
            voc.check(text, cs, "empty root")
            assert np.array_equal(voc.want(text, cs), np.frombuffer(text, dtype=np.uint8))   # every byte raw
    finally:
        voc.tok.destroy()


# ── the batch entry on the same corpora ──────────────────────────────────────

def _documents(nm, vocab):
    """near_miss and a count_sweep cut at arbitrary byte positions: lengths 0, 1, 63, 64,
    65, several thousand; 64 documents of 65 bytes put a start at every offset modulo 64."""
    text = nm + E.count_sweep(vocab, 512, list(range(8, 41)) + [255, 256, 257, 511, 512])
    lengths = [0, 1, 63, 64, 65] + [65] * 64 + [4097, 0, 5001, 2047, 3, 7001, 0, 6000]
    docs, p = [], 0
    for ln in lengths:
        docs.append(text[p:p + ln])
        p += ln
    assert p < len(text)
    docs.append(text[p:])
    starts = np.cumsum([0] + [len(d) for d in docs])[:-1]
    assert {int(s) % 64 for s in starts} == set(range(64)) and len(docs[-1]) > 4000
    return docs


@pytest.mark.parametrize("cs", [8, 512, 7])
@pytest.mark.parametrize("width", WIDTHS)
def test_batch_entry_same_corpora(eng, vocs, nm, width, cs):
    from gpubpe import _lib
    voc = vocs[width]
    docs = _documents(nm, voc.vocab)
    parts = [voc.want(d, cs) if d else np.zeros(0, np.uint32) for d in docs]   # every document encoded alone
    want = np.concatenate(parts)
    want_off = np.zeros(len(docs) + 1, dtype=np.uint64)
    want_off[1:] = np.cumsum([p.shape[0] for p in parts], dtype=np.uint64)
    voc.tok.chunk_size = cs
    got, got_off = voc.tok.encode_batch(docs)
    assert np.array_equal(got_off, want_off) and np.array_equal(got, want), _first_diff(got, want)
    dev = BatchDev(eng, docs)
    try:
        rc, t = dev.run(voc.tok._trie, cs)
        _lib.check(rc, eng.device, "encode batch device")
        dgot, doff = dev.fetch(dev.d_out, t, np.uint32), dev.fetch(dev.d_tok_off, dev.n_docs + 1, np.uint64)
    finally:
        dev.free()
    assert np.array_equal(doff, want_off) and np.array_equal(dgot, want), _first_diff(dgot, want)
