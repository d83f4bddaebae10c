#!/usr/bin/env python3
"""Batch word-bounded merge-rank encode (diagnostic, device-resident, seeded).

The model is tools/bpe_words_bench.py's (`--vocab` ids, trained on the GPU with the
GPT-4 word starts on a sample that is half multilingual text, seed 4, and half code,
seed 5).  `--bytes` of code (seed 6) stay resident, cut into documents of
`--doc-bytes` / 2 to 3 `--doc-bytes` / 2 bytes (seeded, snapped to codepoint starts).
Mode GBPE_WORDS_GPT4 everywhere.  Three parts, one JSON line:

  a  batch_vs_per_document   gbpe_bpe_encode_words_batch_device against one
     gbpe_bpe_encode_words_device call per document on the same resident bytes, the
     per-document tokens written one after the other; both token streams have one
     sha256 (asserted).  The per-document leg runs `--per-doc-reps` times.
  b  batch_vs_single_buffer  the batch call against one gbpe_bpe_encode_words_device
     call over the same bytes as one buffer (the parent's capability; the tokens
     differ), alternating, with the kernel phases of gbpe_bpe_encode_last_timing, and
     gbpe_pretokenize_gpt4_batch_device against gbpe_pretokenize_gpt4_device.
  c  single_buffer_vs_parent (with `--parent-lib A.so B.so`: two copies of the parent
     commit's library)  gbpe_bpe_encode_words_device and gbpe_pretokenize_gpt4_device
     of this library and of both copies, each with its own context and buffers,
     alternating in one process with the slot order rotating; identical outputs
     asserted.  The spread between the two copies is the margin.

Wall seconds are the host clock around calls that end in a device synchronise, every
repetition kept, with median / min / max.
argv: --bytes N --reps R --vocab V --sample-bytes N --doc-bytes N --per-doc-reps R --parent-lib A B.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gpu-bpe_amd"))
import numpy as np  # noqa: E402


def stats(xs):
    return {"reps": [round(x, 6) for x in xs], "median": float(np.median(xs)), "min": float(np.min(xs)),
            "max": float(np.max(xs))}


def note(msg):
    print(f"[bpe_words_batch_bench] {msg}", file=sys.stderr, flush=True)


def cut_documents(arr, doc_bytes, seed):
    """np.uint64 offsets of documents of doc_bytes / 2 .. 3 doc_bytes / 2 bytes, at codepoint starts."""
    n = arr.shape[0]
    rng = np.random.default_rng(seed)
    lens = rng.integers(max(1, doc_bytes // 2), max(2, 3 * doc_bytes // 2), size=2 * n // max(1, doc_bytes) + 16)
    cuts = np.cumsum(lens)
    cuts = cuts[cuts < n]
    for _ in range(3):   # a cut inside a sequence moves to the next lead byte
        cont = (arr[cuts] & 0xC0) == 0x80
        cuts = np.minimum(cuts + cont, n - 1)
    cuts = np.unique(cuts[(arr[cuts] & 0xC0) != 0x80])
    return np.concatenate([[0], cuts[cuts > 0], [n]]).astype(np.uint64)


def load_other(path):
    """Another build of the library (the parent's has none of the batch entry points)."""
    from gpubpe import _lib
    lib = C.CDLL(os.path.abspath(path))
    for name, res, args in _lib._SIGS:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


class Slot:
    """One library with its own context, model and resident buffers."""

    def __init__(self, name, lib, m3, text):
        from gpubpe import _lib
        self.name, self.lib, self.n = name, lib, len(text)
        self.ctx = C.c_void_p()
        rc = lib.gbpe_ctx_create(0, C.byref(self.ctx))
        if rc:
            raise RuntimeError(f"{name}: gbpe_ctx_create: status {rc}")
        self.bpe = C.c_void_p()
        self.ok(lib.gbpe_bpe_upload(self.ctx, m3.ctypes.data_as(_lib.u32p), m3.shape[0], C.byref(self.bpe)), "bpe upload")
        self.d_text, self.d_out, self.d_ws = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ok(lib.gbpe_device_alloc(self.ctx, self.n + 64, C.byref(self.d_text)), "alloc")
        self.ok(lib.gbpe_memcpy_h2d(self.ctx, self.d_text, text, self.n), "h2d")
        self.ok(lib.gbpe_device_alloc(self.ctx, 4 * self.n + 64, C.byref(self.d_out)), "alloc")
        self.ok(lib.gbpe_device_alloc(self.ctx, self.n + 64, C.byref(self.d_ws)), "alloc")
        self.n_out = C.c_uint64()

    def ok(self, rc, what):
        if rc:
            raw = self.lib.gbpe_last_error(self.ctx)
            raise RuntimeError(f"{self.name}: {what}: {raw.decode('utf-8', 'replace') if raw else ''} (status {rc})")

    def alloc(self, nbytes, init=None):
        p = C.c_void_p()
        self.ok(self.lib.gbpe_device_alloc(self.ctx, nbytes, C.byref(p)), "alloc")
        if init is not None:
            init = np.ascontiguousarray(init)
            self.ok(self.lib.gbpe_memcpy_h2d(self.ctx, p, init.ctypes.data_as(C.c_void_p), init.nbytes), "h2d")
        return p

    def fetch(self, ptr, count, dtype):
        host = np.empty(count, dtype)
        if count:
            self.ok(self.lib.gbpe_memcpy_d2h(self.ctx, host.ctypes.data_as(C.c_void_p), ptr, host.nbytes), "d2h")
        return host

    def sha(self, ptr, count, dtype):
        return hashlib.sha256(self.fetch(ptr, count, dtype).tobytes()).hexdigest()[:16]

    def sync(self):
        self.lib.gbpe_synchronize(self.ctx)

    def timing(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self.lib.gbpe_bpe_encode_last_timing(self.ctx, C.byref(a), C.byref(b), C.byref(c))
        return {"ms_starts": a.value, "ms_walk": b.value, "ms_compact": c.value}

    def encode_single(self, mode):
        self.ok(self.lib.gbpe_bpe_encode_words_device(self.ctx, self.bpe, self.d_text, self.n, None, mode, self.d_out,
                                                      self.n, C.byref(self.n_out)), "encode words")
        return int(self.n_out.value)

    def pretok_single(self):
        self.ok(self.lib.gbpe_pretokenize_gpt4_device(self.ctx, self.d_text, self.n, self.d_ws), "pretokenize")
        self.sync()


def timed(slot, fn):
    slot.sync()
    t0 = time.perf_counter()
    r = fn()
    slot.sync()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--sample-bytes", type=int, default=64 << 20)
    ap.add_argument("--doc-bytes", type=int, default=4096)
    ap.add_argument("--per-doc-reps", type=int, default=1)
    ap.add_argument("--parent-lib", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the spread is part of the result)")
    import bench
    from gpubpe import _lib

    lib = _lib.load()
    GPT4 = _lib.GBPE_WORDS_GPT4
    ctx = C.c_void_p()
    _lib.check(lib.gbpe_ctx_create(0, C.byref(ctx)), None, "ctx")   # (no device: fails here, no fallback)
    half = args.sample_bytes // 2
    sample = (bench.make_corpus({"gen": "multilingual", "n": half, "seed": 4}) +
              bench.make_corpus({"gen": "code", "n": half, "seed": 5}))
    d = bench.device_buffer(lib, ctx, sample)
    t0 = time.perf_counter()
    merges, _ = bench.train_run(lib, ctx, d, len(sample), args.vocab, flags=_lib.GBPE_TRAIN_GPT4_BOUNDARIES)
    note(f"trained {merges.shape[0]} merges on {len(sample)} bytes in {time.perf_counter() - t0:.1f} s")
    lib.gbpe_device_free(ctx, d)
    lib.gbpe_ctx_destroy(ctx)
    del sample
    m3 = np.ascontiguousarray(merges[:, :3], dtype=np.uint32)

    text = bench.make_corpus({"gen": "code", "n": args.bytes, "seed": 6})
    n = len(text)
    offs = cut_documents(np.frombuffer(text, np.uint8), args.doc_bytes, seed=9)
    n_docs = int(offs.shape[0]) - 1
    note(f"{n} bytes, {n_docs} documents")
    new = Slot("new", lib, m3, text)
    d_off = new.alloc(8 * (n_docs + 1), offs)
    d_tok_off = new.alloc(8 * (n_docs + 1))
    result = {"bytes": n, "documents": n_docs, "doc_bytes": args.doc_bytes, "vocab": int(args.vocab),
              "merges": int(m3.shape[0]), "sample_bytes": args.sample_bytes, "reps": args.reps, "text": "synth.code seed 6",
              "mode": "GBPE_WORDS_GPT4"}

    def batch():
        new.ok(lib.gbpe_bpe_encode_words_batch_device(new.ctx, new.bpe, new.d_text, n, d_off, n_docs, None, GPT4, new.d_out,
                                                      n, d_tok_off, C.byref(new.n_out)), "encode batch")
        return int(new.n_out.value)

    def per_document():
        total = 0
        cnt = C.c_uint64()
        base_in, base_out = new.d_text.value, new.d_out.value
        o = offs.tolist()
        for k in range(n_docs):
            new.ok(lib.gbpe_bpe_encode_words_device(new.ctx, new.bpe, C.c_void_p(base_in + o[k]), o[k + 1] - o[k], None, GPT4,
                                                    C.c_void_p(base_out + 4 * total), n - total, C.byref(cnt)), "encode words")
            total += cnt.value
        return total

    def pretok_batch():
        new.ok(lib.gbpe_pretokenize_gpt4_batch_device(new.ctx, new.d_text, n, d_off, n_docs, new.d_ws), "pretokenize batch")

    # ── a: the batch call against one call per document ──
    tb, tokens_b = timed(new, batch)   # warm-up
    sha_b = new.sha(new.d_out, tokens_b, np.uint32)
    tok_off = new.fetch(d_tok_off, n_docs + 1, np.uint64)
    assert int(tok_off[0]) == 0 and int(tok_off[-1]) == tokens_b and bool((tok_off[1:] >= tok_off[:-1]).all())
    note(f"warm-up batch: {tokens_b} tokens, {tb:.3f} s")
    wall_pd = []
    for r in range(args.per_doc_reps):
        t, tokens_pd = timed(new, per_document)
        wall_pd.append(t)
        last_call_ms = new.timing()   # (the kernels of the last document's call)
        note(f"per document, repetition {r}: {tokens_pd} tokens, {t:.2f} s")
    sha_pd = new.sha(new.d_out, tokens_pd, np.uint32)
    assert tokens_pd == tokens_b and sha_pd == sha_b, "the batch call and the per-document calls give different tokens"
    wall_b = [timed(new, batch)[0] for _ in range(args.reps)]
    result["a_batch_vs_per_document"] = {
        "tokens": tokens_b, "sha256_16": sha_b, "batch_wall_s": stats(wall_b), "per_document_wall_s": stats(wall_pd),
        "per_document_us_per_call": 1e6 * float(np.median(wall_pd)) / n_docs,
        "per_document_last_call": {"bytes": int(offs[-1] - offs[-2]), "kernel_ms": last_call_ms},
        "speedup_median": float(np.median(wall_pd)) / float(np.median(wall_b))}

    # ── b: what the document handling costs ──
    new.encode_single(GPT4)
    new.pretok_single()
    pretok_batch()
    legs = {"batch": batch, "single_buffer": lambda: new.encode_single(GPT4), "pretok_batch": pretok_batch,
            "pretok_single_buffer": new.pretok_single}
    wall = {k: [] for k in legs}
    kms = {"batch": [], "single_buffer": []}
    toks = {}
    for _ in range(args.reps):   # the legs alternate
        for name, fn in legs.items():
            t, r = timed(new, fn)
            wall[name].append(t)
            if name in kms:
                kms[name].append(new.timing())
                toks[name] = r
    result["b_batch_vs_single_buffer"] = {
        name: dict({"wall_s": stats(wall[name])},
                   **({"tokens": toks[name],
                       "kernel_ms_median": {k: float(np.median([t[k] for t in kms[name]])) for k in kms[name][0]}}
                      if name in kms else {}))
        for name in legs}

    # ── c: the single-buffer paths against the parent's library ──
    if args.parent_lib:
        slots = [Slot("parentA", load_other(args.parent_lib[0]), m3, text), new,
                 Slot("parentB", load_other(args.parent_lib[1]), m3, text)]
        shas = {}
        for s in slots:   # warm-up + identical outputs
            cnt = s.encode_single(GPT4)
            s.pretok_single()
            shas[s.name] = (cnt, s.sha(s.d_out, cnt, np.uint32), s.sha(s.d_ws, n, np.uint8))
        assert len(set(shas.values())) == 1, f"the libraries disagree: {shas}"
        reps = 2 * args.reps + 2
        wall = {s.name: {"encode_words_device": [], "pretokenize_gpt4_device": []} for s in slots}
        for r in range(reps):
            order = slots[r % 3:] + slots[: r % 3]   # the slot order rotates
            for s in order:
                wall[s.name]["encode_words_device"].append(timed(s, lambda: s.encode_single(GPT4))[0])
            for s in order:
                wall[s.name]["pretokenize_gpt4_device"].append(timed(s, s.pretok_single)[0])
        result["c_single_buffer_vs_parent"] = {
            "reps": reps, "tokens": shas["new"][0],
            "wall_s": {name: {k: stats(v) for k, v in legs_.items()} for name, legs_ in wall.items()}}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
