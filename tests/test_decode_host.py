"""Host side of the device decode (no GPU needed): the numpy reference of the GPU
tests pinned to the oracle's decode, gbpe_decode_size (host only, like
gbpe_trie_compile), and the flattening helpers with their argument checks.
"""
import ctypes as C
import os

import numpy as np
import pytest

import bpe_oracle as O
import decode_ref as R


@pytest.fixture(scope="module")
def lib():
    from gpubpe import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_numpy_reference_equals_oracle_on_every_small_stream():
    va = R.vocab_a()
    streams = R.small_streams()
    assert len(streams) > 40 and all(t.shape[0] < 100000 for t in streams.values())
    for name, t in streams.items():
        assert R.decode_np(t, va).tobytes() == O.decode(t, va), name
    for docs in (R.batch_documents(), R.sliced_documents(), R.many_small_documents(300)):
        for t in docs:
            assert R.decode_np(t, va).tobytes() == O.decode(t, va)
    vb = R.vocab_b()
    t = R.large_stream_b()[:5000]
    assert R.decode_np(t, vb).tobytes() == O.decode(t, vb)
    assert R.decode_np([], va).shape == (0,)


def test_vocab_a_is_what_the_tests_say():
    va = R.vocab_a()
    assert len(va) == R.A_SIZE and [len(e) for e in va[:256]] == [1] * 256
    assert [len(va[R.A_LEN1 + ln - 1]) for ln in range(1, 18)] == list(range(1, 18))
    assert va[R.A_EMPTY] == [] and va[R.A_LAST_EMPTY] == [] and R.A_LAST_EMPTY == len(va) - 1
    assert len(va[R.A_LONG]) == 300 and len(va[R.A_BIG]) == 65535
    for total in (0, 15, 16, 17, 31, 32, 33):
        assert len(O.decode(R.stream_of_total(total), va)) == total
    t = R.boundary_long(2 * R.BLK + 1, 1)
    assert t[0] == t[-1] == t[R.BLK - 1] == t[R.BLK] == R.A_LONG


def _size(lib, offs, tokens):
    from gpubpe import _lib
    tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
    n = C.c_uint64(12345)
    rc = lib.gbpe_decode_size(offs.ctypes.data_as(_lib.u64p), offs.shape[0] - 1, tokens.ctypes.data_as(_lib.u32p),
                              tokens.shape[0], C.byref(n))
    return rc, int(n.value)


def test_decode_size_equals_oracle(lib):
    from gpubpe import decoded_size, flatten_vocab
    va = R.vocab_a()
    _, offs = flatten_vocab(va)
    V = len(va)
    cases = [[], [V], [V + 1], [70000], [0xFFFFFFFF], [R.A_EMPTY], [R.A_LAST_EMPTY, R.A_EMPTY],
             [65, V, R.A_EMPTY, V + 1, 70000, R.A_LONG, 0xFFFFFFFF, R.A_LAST_EMPTY, R.A_BIG, 66]]
    cases += [R.with_unknown(n, 400 + n) for n in (1, 65, R.BLK + 1)] + [R.all_unknown(7)]
    for t in cases:
        want = len(O.decode(t, va))
        assert _size(lib, offs, t) == (0, want)
        assert decoded_size(t, offs) == want
    assert _size(lib, offs, [V, V + 1, 70000, 0xFFFFFFFF]) == (0, 12)


def test_decode_size_null_arguments(lib):
    from gpubpe import _lib, flatten_vocab
    _, offs = flatten_vocab(R.vocab_a())
    toks = np.array([1, 2, 3], dtype=np.uint32)
    n = C.c_uint64()
    po, pt = offs.ctypes.data_as(_lib.u64p), toks.ctypes.data_as(_lib.u32p)
    assert lib.gbpe_decode_size(None, R.A_SIZE, pt, 3, C.byref(n)) == _lib.GBPE_E_INVALID
    assert lib.gbpe_decode_size(po, R.A_SIZE, None, 3, C.byref(n)) == _lib.GBPE_E_INVALID
    assert lib.gbpe_decode_size(po, R.A_SIZE, pt, 3, None) == _lib.GBPE_E_INVALID
    assert lib.gbpe_decode_size(po, R.A_SIZE, None, 0, C.byref(n)) == 0 and n.value == 0   # no tokens: none needed


def test_flatten_vocab_layout():
    from gpubpe import flatten_vocab
    flat, offs = flatten_vocab([[1, 2], [], bytes([3]), bytearray([4, 5, 6]), []])
    assert flat.dtype == np.uint8 and offs.dtype == np.uint64
    assert flat.tolist() == [1, 2, 3, 4, 5, 6] and offs.tolist() == [0, 2, 2, 3, 6, 6]
    flat, offs = flatten_vocab([])
    assert flat.shape == (0,) and offs.tolist() == [0]
    va = R.vocab_a()
    flat, offs = flatten_vocab(va)
    rflat, roffs = R.flatten(va)
    assert np.array_equal(flat, rflat) and np.array_equal(offs, roffs)


def test_flatten_vocab_refuses_an_entry_above_65535_bytes():
    from gpubpe import _lib, flatten_vocab
    flatten_vocab([[0] * 65535])
    with pytest.raises(_lib.GpuBpeError) as ei:
        flatten_vocab([[1], [0] * 65536, [2]])
    assert ei.value.code == _lib.GBPE_E_INVALID and "entry 1" in str(ei.value)


def test_flatten_token_documents_layouts():
    from gpubpe import flatten_token_documents
    toks, offs = flatten_token_documents([[1, 2, 3], [], np.array([70000], dtype=np.uint32), (4, 5)])
    assert toks.dtype == np.uint32 and offs.dtype == np.uint64
    assert toks.tolist() == [1, 2, 3, 70000, 4, 5] and offs.tolist() == [0, 3, 3, 4, 6]
    assert toks.flags["C_CONTIGUOUS"] and offs.flags["C_CONTIGUOUS"]
    toks, offs = flatten_token_documents([])
    assert toks.shape == (0,) and toks.dtype == np.uint32 and offs.tolist() == [0]
    toks, offs = flatten_token_documents([[], []])
    assert toks.shape == (0,) and offs.tolist() == [0, 0, 0]
    for given in ([0, 2, 2, 5], np.array([0, 2, 2, 5], dtype=np.int32), np.array([0, 2, 2, 5], dtype=np.uint64)):
        toks, offs = flatten_token_documents([9, 8, 7, 6, 0xFFFFFFFF], given)
        assert toks.tolist() == [9, 8, 7, 6, 0xFFFFFFFF] and offs.dtype == np.uint64 and offs.tolist() == [0, 2, 2, 5]
    toks, offs = flatten_token_documents([], [0])
    assert toks.shape == (0,) and offs.tolist() == [0]


class _NoLibrary:
    """Stands in for the loaded library: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the offsets were checked")


@pytest.mark.parametrize("offsets", [
    [0, 3, 2, 5],        # decreasing
    [1, 3, 5],           # does not start at 0
    [0, 3, 4],           # does not end at the token count
    [0, 3, 6],           # passes the end
    [],                  # no entries at all
    [0.0, 5.0],          # not integers
    [0, -1, 5],          # negative
    [[0, 5]],            # not one-dimensional
])
def test_given_token_offsets_rejected_before_any_library_call(offsets, monkeypatch):
    from gpubpe import TrieTokenizer, _lib, flatten_token_documents
    with pytest.raises(_lib.GpuBpeError) as ei:
        flatten_token_documents([1, 2, 3, 4, 5], offsets)
    assert ei.value.code == _lib.GBPE_E_INVALID
    monkeypatch.setattr(_lib, "load", lambda path=None: _NoLibrary())
    tok = TrieTokenizer.__new__(TrieTokenizer)
    tok._engine, tok._trie, tok._vocab = None, None, [[i] for i in range(256)]
    with pytest.raises(_lib.GpuBpeError) as ei:
        tok.decode_batch([1, 2, 3, 4, 5], offsets)
    assert ei.value.code == _lib.GBPE_E_INVALID


def test_decode_of_nothing_needs_no_device(monkeypatch):
    from gpubpe import TrieTokenizer, _lib
    monkeypatch.setattr(_lib, "load", lambda path=None: _NoLibrary())
    tok = TrieTokenizer.__new__(TrieTokenizer)
    tok._engine, tok._trie, tok._vocab = None, None, [[i] for i in range(256)]
    assert tok.decode_bytes([]) == b""
    for docs in ([], [[], []]):
        out, offs = tok.decode_batch(docs)
        assert out.dtype == np.uint8 and out.shape == (0,)
        assert offs.dtype == np.uint64 and offs.tolist() == [0] * (len(docs) + 1)
