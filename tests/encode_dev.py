"""Device buffers for the encode tests — TEST INFRASTRUCTURE ONLY.

Buffers come from gbpe_device_alloc / gbpe_memcpy_*: a process that has loaded the
library finds no HIP device through torch.
"""
import ctypes as C

import numpy as np


class DevBuffers:
    """Allocations of one test, freed together."""

    def __init__(self, eng):
        from gpubpe import _lib
        self.lib, self.ctx = _lib.load(), eng.device
        self.ptrs = []

    def alloc(self, nbytes, init=None):
        from gpubpe import _lib
        p = C.c_void_p()
        _lib.check(self.lib.gbpe_device_alloc(self.ctx, nbytes, C.byref(p)), self.ctx, "alloc")
        self.ptrs.append(p)
        if init is not None:
            self.put(p, init)
        return p

    def put(self, ptr, init):
        from gpubpe import _lib
        init = np.ascontiguousarray(init)
        if init.nbytes:
            _lib.check(self.lib.gbpe_memcpy_h2d(self.ctx, ptr, init.ctypes.data_as(C.c_void_p), init.nbytes), self.ctx, "h2d")

    def fetch(self, ptr, count, dtype):
        from gpubpe import _lib
        host = np.empty(count, dtype=dtype)
        if count:
            _lib.check(self.lib.gbpe_memcpy_d2h(self.ctx, host.ctypes.data_as(C.c_void_p), ptr, host.nbytes), self.ctx, "d2h")
        return host

    def free(self):
        for p in self.ptrs:
            self.lib.gbpe_device_free(self.ctx, p)
        self.ptrs = []


class BatchDev(DevBuffers):
    """Device buffers of one gbpe_encode_batch_device call."""

    def __init__(self, eng, docs, out_cap=None, guard=0):
        from gpubpe import flatten_documents
        super().__init__(eng)
        self.buf, self.offs = flatten_documents(docs)
        self.n, self.n_docs = int(self.buf.shape[0]), len(docs)
        self.out_cap = self.n if out_cap is None else out_cap
        self.guard = guard
        self.d_in = self.alloc(max(self.n, 1), self.buf)
        self.d_off = self.alloc(8 * (self.n_docs + 1), self.offs)
        self.d_tok_off = self.alloc(8 * (self.n_docs + 1), np.full(self.n_docs + 1, 0xEEEEEEEE, np.uint64))
        self.d_out = self.alloc(4 * (self.out_cap + guard) + 4, np.full(self.out_cap + guard + 1, 0xA5A5A5A5, np.uint32))

    def run(self, trie, cs):
        n_out = C.c_uint64()
        rc = self.lib.gbpe_encode_batch_device(self.ctx, trie, self.d_in, self.n, self.d_off, self.n_docs, cs, self.d_out,
                                               self.out_cap, self.d_tok_off, C.byref(n_out))
        return rc, int(n_out.value)
