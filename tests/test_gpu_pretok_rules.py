"""The GPT-4 word-start kernels (pretok.hip) and the trainer's symbol front end
(k_symbols / k_symbols_v) at block, halo and alignment edges, bit-exact against the
oracle.  The corpora come from pretok_corpora.py; test_pretok_corpora.py asserts what
they hold and where it lands.  Paths that run here and nowhere else in the suite:
unaligned staging and the scalar store fallback under an unaligned output
(test_device_entry_point), two blocks per thread in k_pt_scan2 (test_scan_chain), the
cp >= 0x110000 guard (test_sweep_astral, the beyond_unicode probe), trainer creation
from device input, the scalar k_symbols with a device mask and the symbol export
straight after create (test_trainer_symbols)."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "gpu-bpe_amd"))

import bpe_oracle as O  # noqa: E402
import pretok_corpora as P  # noqa: E402
from gpubpe import BPEEngine, BPETrainer, _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = BPEEngine().init()
    yield e
    e.close()


def gpu_ws(engine, data: bytes) -> np.ndarray:
    """gbpe_pretokenize_gpt4 on host bytes"""
    ws = np.zeros(len(data), dtype=np.uint8)
    ctx = engine.device
    src = np.frombuffer(data, np.uint8)
    _lib.check(_lib.load().gbpe_pretokenize_gpt4(ctx, src.ctypes.data_as(C.c_void_p) if len(data) else None, len(data),
                                                 ws.ctypes.data_as(C.c_void_p) if len(data) else None), ctx, "pretokenize")
    return ws


def assert_same(got, exp, data, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (f"{what}: {bad.size} mismatches, first (offset, offset % 4096, offset % 16, got, expected, "
                           f"bytes around) "
                           f"{[(int(i), int(i) % 4096, int(i) % 16, int(got[i]), int(exp[i]), data[max(0, i - 16):i + 16]) for i in bad[:5]]}")


# ─────────────────────────────── host entry point ─────────────────────────────

@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
def test_fuzz(engine, seed):
    data = P.fuzz(P.FUZZ_CODEPOINTS, seed)
    for cut in P.FUZZ_CUTS:            # the cut lands inside a codepoint for some seeds
        piece = data[:len(data) - cut]
        assert_same(gpu_ws(engine, piece), O.gpt4_word_starts(piece), piece, f"fuzz seed {seed} cut {cut}")


def test_contraction_at_the_end_of_input(engine):
    for k, case in enumerate(P.end_cases()):
        assert_same(gpu_ws(engine, case), O.gpt4_word_starts(case), case, f"end case {k} ({case[-8:]!r})")


@pytest.mark.parametrize("name,pat,period", P.PROBES, ids=[p[0] for p in P.PROBES])
def test_periodic_probe(engine, name, pat, period):
    data = P.periodic(pat, period)
    assert_same(gpu_ws(engine, data), O.gpt4_word_starts(data), data, f"probe {name}, period {period}")


def test_scan_chain():
    """Digit runs over many blocks with more than 1024 blocks, so every k_pt_scan2 thread
    chains two block aggregates; a fresh context, so the aggregate pool grows from the
    small input's size to the large one's between the calls."""
    small = P.fuzz(5_500, P.CHAIN_SEED)
    assert 2 * P.BLK < len(small) < 3 * P.BLK
    exp_small = O.gpt4_word_starts(small)
    data, exp = P.digit_chain(P.CHAIN_N, P.CHAIN_SEED)
    eng = BPEEngine().init()
    try:
        assert_same(gpu_ws(eng, small), exp_small, small, "small input before")
        assert_same(gpu_ws(eng, data), exp, data, "digit chain")
        assert_same(gpu_ws(eng, small), exp_small, small, "small input after")
        assert_same(gpu_ws(eng, data), exp, data, "digit chain again")
    finally:
        eng.close()


def test_sweep_bmp(engine):
    data = P.sweep_bmp()
    assert_same(gpu_ws(engine, data), O.gpt4_word_starts(data), data, "every BMP codepoint")


def test_sweep_astral(engine):
    data = P.sweep_astral()
    assert_same(gpu_ws(engine, data), O.gpt4_word_starts(data), data, "every astral codepoint and beyond")


# ────────────────────────────── device entry point ────────────────────────────

FILL = 0xAB


class DeviceBuf:
    """Device memory from gbpe_device_alloc (hipMalloc: 16-byte aligned), so the pointer
    offsets below are the alignment the kernels see.  The library's own allocator, not a
    torch tensor: torch ships a HIP runtime of its own, and a process that has already
    loaded the library's cannot bring up a second one."""

    def __init__(self, engine, host: np.ndarray):
        self.lib, self.ctx = _lib.load(), engine.device
        self.n = host.shape[0]
        p = C.c_void_p()
        _lib.check(self.lib.gbpe_device_alloc(self.ctx, self.n, C.byref(p)), self.ctx, "device alloc")
        self.ptr = p.value
        assert self.ptr % 16 == 0
        self.put(host)

    def put(self, host: np.ndarray):
        assert host.dtype == np.uint8 and host.shape[0] == self.n and host.flags.c_contiguous
        _lib.check(self.lib.gbpe_memcpy_h2d(self.ctx, self.ptr, host.ctypes.data_as(C.c_void_p), self.n), self.ctx, "h2d")

    def get(self) -> np.ndarray:
        out = np.empty(self.n, np.uint8)
        _lib.check(self.lib.gbpe_memcpy_d2h(self.ctx, out.ctypes.data_as(C.c_void_p), self.ptr, self.n), self.ctx, "d2h")
        return out

    def free(self):
        if self.ptr:
            self.lib.gbpe_device_free(self.ctx, self.ptr)
            self.ptr = None


def test_device_entry_point(engine):
    lib, ctx = _lib.load(), engine.device
    data = P.device_corpus()
    ends = P.contraction_ends(data)
    host_in = np.frombuffer(data, np.uint8).copy()
    fill = np.full(len(data) + 64, FILL, np.uint8)
    d_in, d_out = DeviceBuf(engine, host_in), DeviceBuf(engine, fill)
    try:
        expected = {}
        for a in (0, 1, 2, 3):                       # input offset: 1-3 take the unaligned staging
            sizes = {1, 2, 15, 16, 17, 4095, 4096, 4097, 4111, 4112, 8195, len(data) - a}
            sizes |= {e - a for e in ends.values()}  # ends after an apostrophe, after one and two suffix letters
            for n in sorted(sizes):
                if (a, n) not in expected:           # the device input goes on past n: a read past n shows
                    expected[a, n] = O.gpt4_word_starts(data[a:a + n])
                exp = expected[a, n]
                for b in (0, 1, 15, 16):             # output offset: 1 and 15 take the scalar stores
                    d_out.put(fill)
                    _lib.check(lib.gbpe_pretokenize_gpt4_device(ctx, d_in.ptr + a, n, d_out.ptr + b), ctx,
                               "pretokenize (device)")
                    _lib.check(lib.gbpe_synchronize(ctx), ctx, "synchronize")
                    out = d_out.get()
                    what = f"input offset {a}, output offset {b}, n {n}"
                    assert_same(out[b:b + n], exp, data[a:a + n], what)
                    assert np.all(out[:b] == FILL) and np.all(out[b + n:] == FILL), f"{what}: wrote outside [b, b + n)"
        assert np.array_equal(d_in.get(), host_in), "the input changed"
    finally:
        d_in.free()
        d_out.free()
    assert lib.gbpe_pretokenize_gpt4_device(ctx, None, 0, None) == _lib.GBPE_OK
    assert lib.gbpe_pretokenize_gpt4(ctx, None, 0, None) == _lib.GBPE_OK


# ───────────────────────────── trainer front end ──────────────────────────────

def _created_symbols(engine, bytes_ptr, n, ws_ptr, on_device, target, flags):
    """gbpe_trainer_create, then gbpe_trainer_symbols before any step"""
    lib, ctx = _lib.load(), engine.device
    opts = _lib.TrainOpts(target_vocab_size=target, vocab_size=256, next_token_id=256, batch_size=128, flags=flags,
                          table_log2=0)
    tr = C.c_void_p()
    _lib.check(lib.gbpe_trainer_create(ctx, bytes_ptr, n, ws_ptr, on_device, C.byref(opts), C.byref(tr)), ctx, "create")
    try:
        st = _lib.TrainerStats()
        _lib.check(lib.gbpe_trainer_stats_get(tr, C.byref(st)), ctx, "stats")
        assert st.bytes_per_symbol == (2 if target <= 0x8000 else 4) and st.symbol_count == n
        out = np.full(n + 1, 0xDEADBEEF, np.uint32)
        cnt = C.c_uint64()
        _lib.check(lib.gbpe_trainer_symbols(tr, out.ctypes.data_as(_lib.u32p), n, C.byref(cnt)), ctx, "symbols")
        assert cnt.value == n and out[n] == 0xDEADBEEF
        return out[:n]
    finally:
        lib.gbpe_trainer_destroy(tr)


@pytest.mark.parametrize("boundaries", ["heuristic", "external", "gpt4"])
def test_trainer_symbols(engine, boundaries):
    """byte | word start << 16 right after create, for host input, device input at offset 0
    (k_symbols_v) and at offset 1 (the scalar k_symbols), 16-bit and 32-bit symbols"""
    data = P.symbols_corpus()
    host = np.frombuffer(data, np.uint8).copy()
    rng = np.random.default_rng(P.SYMBOLS_SEED)
    mask = (rng.integers(0, 5, size=len(data)) == 0).astype(np.uint8)
    d_bytes, d_mask = DeviceBuf(engine, host), DeviceBuf(engine, mask)
    d_mask1 = DeviceBuf(engine, np.concatenate([np.array([1], np.uint8), mask]))   # the mask from offset 1 on
    try:
        _trainer_symbols_cases(engine, boundaries, host, mask, d_bytes, d_mask, d_mask1)
        assert np.array_equal(d_bytes.get(), host) and np.array_equal(d_mask.get(), mask)
    finally:
        for d in (d_bytes, d_mask, d_mask1):
            d.free()


def _trainer_symbols_cases(engine, boundaries, host, mask, d_bytes, d_mask, d_mask1):
    flags = _lib.GBPE_TRAIN_GPT4_BOUNDARIES if boundaries == "gpt4" else 0
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for n in (1, 4096, 4097, 4111, host.shape[0] - 1):
        for a in (0, 1):
            piece = host[a:a + n]
            if boundaries == "heuristic":
                ws = O.heuristic_word_starts(piece).astype(np.uint32)
            elif boundaries == "external":
                ws = (mask[a:a + n] != 0).astype(np.uint32)
            else:
                ws = O.gpt4_word_starts(piece.tobytes()).astype(np.uint32)
            exp = piece.astype(np.uint32) | (ws << 16)
            ext = boundaries == "external"
            # (bytes, mask, on device): host copies, device buffers at offset a, and for an external
            # mask the bytes at offset 0 with the mask at offset 1
            b_host, m_host = np.ascontiguousarray(piece), np.ascontiguousarray(mask[a:a + n])
            inputs = [("host", vp(b_host), vp(m_host) if ext else None, 0),
                      (f"device + {a}", d_bytes.ptr + a, d_mask.ptr + a if ext else None, 1)]
            if ext and a == 0:
                inputs.append(("device bytes + 0, mask + 1", d_bytes.ptr, d_mask1.ptr + 1, 1))
            for target in (700, 40_000):
                for what, bp, mp, on_device in inputs:
                    got = _created_symbols(engine, bp, n, mp, on_device, target, flags)
                    bad = np.flatnonzero(got != exp)
                    assert bad.size == 0, (f"{boundaries}, {what}, n {n}, target {target}: {bad.size} mismatches, first "
                                           f"{[(int(i), hex(int(got[i])), hex(int(exp[i]))) for i in bad[:5]]}")


@pytest.mark.parametrize("exact", [False, True])
def test_train_multibyte_with_gpt4_boundaries(engine, exact):
    data = P.train_corpus()
    tr = BPETrainer(engine, exact_compaction=exact)
    tr._flags |= _lib.GBPE_TRAIN_GPT4_BOUNDARIES
    got = tr.train(data, target_vocab_size=400)
    exp = O.train(data, 400, word_starts=O.gpt4_word_starts(data), compaction="exact" if exact else "reference")
    assert [m[:3] for m in exp["merges"]] == [list(m) for m in got["merges"]]
