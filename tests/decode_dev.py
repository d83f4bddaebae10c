"""Device buffers and call helpers of the decode tests — TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from encode_dev import DevBuffers

GUARD = 64          # bytes of 0xA5 behind out_cap
POISON = 0xEEEEEEEEEEEEEEEE


def upload_vocab(eng, vocab):
    """gbpe_vocab_upload of a list-of-lists vocab; returns (status, handle)."""
    from gpubpe import _lib
    import decode_ref as R
    flat, offs = R.flatten(vocab)
    dv = C.c_void_p()
    rc = _lib.load().gbpe_vocab_upload(eng.device, flat.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(_lib.u64p),
                                       len(vocab), C.byref(dv))
    return rc, dv


class DecodeDev(DevBuffers):
    """Device buffers of one gbpe_decode_device / gbpe_decode_batch_device call:
    the tokens, the output with GUARD bytes of 0xA5 behind out_cap, and for a batch
    the token offsets and poisoned byte offsets."""

    def __init__(self, eng, tokens, out_cap, tok_off=None):
        super().__init__(eng)
        self.tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        self.n = int(self.tokens.shape[0])
        self.out_cap = int(out_cap)
        self.d_tok = self.alloc(4 * self.n + 16, self.tokens)
        self.d_out = self.alloc(self.out_cap + GUARD, np.full(self.out_cap + GUARD, 0xA5, np.uint8))
        self.n_docs = None
        if tok_off is not None:
            tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
            self.n_docs = int(tok_off.shape[0]) - 1
            self.d_tok_off = self.alloc(8 * (self.n_docs + 1), tok_off)
            self.d_byte_off = self.alloc(8 * (self.n_docs + 1), np.full(self.n_docs + 1, POISON, np.uint64))

    def run(self, dv):
        n_out = C.c_uint64(777)
        if self.n_docs is None:
            rc = self.lib.gbpe_decode_device(self.ctx, dv, self.d_tok, self.n, self.d_out, self.out_cap, C.byref(n_out))
        else:
            rc = self.lib.gbpe_decode_batch_device(self.ctx, dv, self.d_tok, self.n, self.d_tok_off, self.n_docs,
                                                   self.d_out, self.out_cap, self.d_byte_off, C.byref(n_out))
        return rc, int(n_out.value)

    def output(self):
        """(the out_cap bytes, the guard behind them)"""
        raw = self.fetch(self.d_out, self.out_cap + GUARD, np.uint8)
        return raw[:self.out_cap], raw[self.out_cap:]

    def byte_off(self):
        return self.fetch(self.d_byte_off, self.n_docs + 1, np.uint64)


def device_decode(eng, dv, tokens, out_cap, tok_off=None):
    """One device-form call: (status, n_out, bytes[out_cap], guard, byte_off or None)."""
    dev = DecodeDev(eng, tokens, out_cap, tok_off)
    try:
        rc, n_out = dev.run(dv)
        out, guard = dev.output()
        return rc, n_out, out, guard, (dev.byte_off() if tok_off is not None else None)
    finally:
        dev.free()


def host_decode(eng, dv, tokens, out_cap, tok_off=None):
    """One host-form call (gbpe_decode / gbpe_decode_batch), same return as device_decode."""
    from gpubpe import _lib
    lib = _lib.load()
    tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
    raw = np.full(out_cap + GUARD, 0xA5, np.uint8)
    n_out = C.c_uint64(777)
    if tok_off is None:
        rc = lib.gbpe_decode(eng.device, dv, tokens.ctypes.data_as(_lib.u32p), tokens.shape[0],
                             raw.ctypes.data_as(C.c_void_p), out_cap, C.byref(n_out))
        return rc, int(n_out.value), raw[:out_cap], raw[out_cap:], None
    tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
    byte_off = np.full(tok_off.shape[0], POISON, np.uint64)
    rc = lib.gbpe_decode_batch(eng.device, dv, tokens.ctypes.data_as(_lib.u32p), tokens.shape[0],
                               tok_off.ctypes.data_as(_lib.u64p), tok_off.shape[0] - 1, raw.ctypes.data_as(C.c_void_p),
                               out_cap, byte_off.ctypes.data_as(_lib.u64p), C.byref(n_out))
    return rc, int(n_out.value), raw[:out_cap], raw[out_cap:], byte_off
