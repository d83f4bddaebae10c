"""Host side of the batched document encode (no GPU needed): the flattening
helper that turns a list of documents into the batch layout of
gbpe_encode_batch (one byte buffer + D + 1 document offsets), and its check of
caller-given offsets, which rejects bad ones before any library call.
"""
import numpy as np
import pytest


def test_flatten_mixed_bytes_like_inputs():
    from gpubpe import flatten_documents
    docs = [b"abc", bytearray(b"de"), memoryview(b"fghi"), np.frombuffer(b"jk", dtype=np.uint8)]
    buf, offs = flatten_documents(docs)
    assert buf.dtype == np.uint8 and offs.dtype == np.uint64
    assert buf.tobytes() == b"abcdefghijk"
    assert offs.tolist() == [0, 3, 5, 9, 11]
    assert buf.flags["C_CONTIGUOUS"] and offs.flags["C_CONTIGUOUS"]


def test_flatten_empty_documents():
    from gpubpe import flatten_documents
    buf, offs = flatten_documents([b"", b"x", bytearray(), memoryview(b""), b"yz", b""])
    assert buf.tobytes() == b"xyz"
    assert offs.tolist() == [0, 0, 1, 1, 1, 3, 3]
    buf, offs = flatten_documents([b"", b""])
    assert buf.shape == (0,) and offs.tolist() == [0, 0, 0]


def test_flatten_empty_list():
    from gpubpe import flatten_documents
    buf, offs = flatten_documents([])
    assert buf.dtype == np.uint8 and buf.shape == (0,)
    assert offs.dtype == np.uint64 and offs.tolist() == [0]


def test_given_offsets_pass_through():
    from gpubpe import flatten_documents
    for offsets in ([0, 2, 2, 5], np.array([0, 2, 2, 5], dtype=np.int32), np.array([0, 2, 2, 5], dtype=np.uint64)):
        buf, offs = flatten_documents(bytearray(b"hello"), offsets)
        assert buf.tobytes() == b"hello" and offs.dtype == np.uint64 and offs.tolist() == [0, 2, 2, 5]
    buf, offs = flatten_documents(b"", [0])
    assert buf.shape == (0,) and offs.tolist() == [0]


class _NoLibrary:
    """Stands in for the loaded library: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the offsets were checked")


@pytest.mark.parametrize("offsets", [
    [0, 3, 2, 5],        # decreasing
    [1, 3, 5],           # does not start at 0
    [0, 3, 4],           # does not end at the buffer's length
    [0, 3, 6],           # passes the end
    [],                  # no entries at all
    [0.0, 5.0],          # not integers
    [0, -1, 5],          # negative
    [[0, 5]],            # not one-dimensional
])
def test_given_offsets_rejected_before_any_library_call(offsets, monkeypatch):
    from gpubpe import TrieTokenizer, _lib, flatten_documents
    with pytest.raises(_lib.GpuBpeError) as ei:
        flatten_documents(b"hello", offsets)
    assert ei.value.code == _lib.GBPE_E_INVALID
    # the same through the tokenizer method, with no engine, trie or library behind it
    monkeypatch.setattr(_lib, "load", lambda path=None: _NoLibrary())
    tok = TrieTokenizer.__new__(TrieTokenizer)
    tok._engine, tok._trie, tok.chunk_size = None, None, 512
    with pytest.raises(_lib.GpuBpeError) as ei:
        tok.encode_batch(b"hello", offsets)
    assert ei.value.code == _lib.GBPE_E_INVALID


def test_encode_batch_of_nothing_needs_no_device(monkeypatch):
    from gpubpe import TrieTokenizer, _lib
    monkeypatch.setattr(_lib, "load", lambda path=None: _NoLibrary())
    tok = TrieTokenizer.__new__(TrieTokenizer)
    tok._engine, tok._trie, tok.chunk_size = None, None, 512
    for docs in ([], [b"", b""]):
        toks, offs = tok.encode_batch(docs)
        assert toks.dtype == np.uint32 and toks.shape == (0,)
        assert offs.dtype == np.uint64 and offs.tolist() == [0] * (len(docs) + 1)
