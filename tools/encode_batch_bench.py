#!/usr/bin/env python3
"""Batched document encode against the single-stream entry point (diagnostic,
device-resident, seeded).  The bench's C3 vocab (32K, trained on the GPU on the
100 MiB multilingual sample, seed 4) encodes `--bytes` of multilingual text
(seed 3) four ways, the legs alternating in one process after a warm-up:

  many documents   the text cut into seeded documents of log-uniform length
                   16 B .. 64 KiB:
    batch          one gbpe_encode_batch_device call;
    loop           one gbpe_encode_device call per document, the documents laid
                   out 4-byte aligned (the only correct way without the batch entry);
  one document     the whole text as a single document:
    batch1         gbpe_encode_batch_device;
    single         gbpe_encode_device.

Prints one JSON line: per-leg wall seconds of every repetition (host clock
around calls that end in a device synchronise), their median / min / max, the
ratios loop / batch and batch1 / single with the spread, the kernel times of the
batch legs, and sha256 prefixes of the tokens (batch == loop and batch1 == single
are asserted).  argv: --bytes N --reps R --seed S --vocab V --sample-bytes N.
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


def cut_documents(n: int, seed: int, lo: int = 16, hi: int = 65536) -> np.ndarray:
    """Document offsets (uint64, D + 1 entries, 0 .. n) of seeded log-uniform lengths in [lo, hi]."""
    rng = np.random.default_rng(seed)
    offs = [0]
    while offs[-1] < n:
        k = max(16, (n - offs[-1]) // 4000)
        lens = np.exp(rng.uniform(np.log(lo), np.log(hi), size=k)).astype(np.int64)
        for ln in np.clip(lens, lo, hi).tolist():
            offs.append(min(n, offs[-1] + ln))
            if offs[-1] == n:
                break
    return np.array(offs, dtype=np.uint64)


def aligned_layout(offs: np.ndarray, align: int = 4):
    """Starts of the same documents laid out `align`-byte aligned, and the layout's size."""
    lens = (offs[1:] - offs[:-1]).astype(np.int64)
    padded = (lens + align - 1) // align * align
    starts = np.zeros(lens.shape[0], dtype=np.int64)
    if lens.shape[0] > 1:
        starts[1:] = np.cumsum(padded[:-1])
    return starts, lens, int(padded.sum())


def stats(xs):
    return {"reps": [round(x, 6) for x in xs], "median": float(np.median(xs)), "min": float(np.min(xs)),
            "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--sample-bytes", type=int, default=104_857_600)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the spread is part of the result)")
    import bench
    from gpubpe import _lib, compile_vocab_to_trie, parse_header, parse_trie_buffers
    from gpubpe.vocab import Vocab

    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.gbpe_ctx_create(0, C.byref(ctx)), None, "ctx")   # (no device: fails here, no fallback)

    def check(rc, what):
        _lib.check(rc, ctx, what)

    sample = bench.make_corpus({"gen": "multilingual", "n": args.sample_bytes, "seed": 4})
    d = bench.device_buffer(lib, ctx, sample)
    merges, _ = bench.train_run(lib, ctx, d, len(sample), args.vocab)
    lib.gbpe_device_free(ctx, d)
    del sample
    voc = Vocab()
    for a, b in merges[:, :2].tolist():
        voc.add_merge(a, b)
    blob = compile_vocab_to_trie(voc.entries)
    hdr = parse_header(blob)
    nodes, edges = parse_trie_buffers(blob, hdr)
    trie = C.c_void_p()
    check(lib.gbpe_trie_upload(ctx, nodes.ctypes.data_as(_lib.u32p), hdr["nodeCount"],
                               edges.ctypes.data_as(_lib.u32p), hdr["edgeCount"], C.byref(trie)), "trie")
    cs = max(512, min(2048, hdr["maxTokenLen"] * 8))

    text = np.frombuffer(bench.make_corpus({"gen": "multilingual", "n": args.bytes, "seed": 3}), dtype=np.uint8)
    n = int(text.shape[0])
    offs = cut_documents(n, args.seed)
    n_docs = int(offs.shape[0]) - 1
    starts, lens, n_al = aligned_layout(offs)
    laid = np.zeros(n_al + 64, dtype=np.uint8)
    for s, o, ln in zip(starts.tolist(), offs[:-1].tolist(), lens.tolist()):
        laid[s:s + ln] = text[o:o + ln]

    def dev(nbytes, init=None):
        p = C.c_void_p()
        check(lib.gbpe_device_alloc(ctx, nbytes, C.byref(p)), "alloc")
        if init is not None and init.nbytes:
            check(lib.gbpe_memcpy_h2d(ctx, p, init.ctypes.data_as(C.c_void_p), init.nbytes), "h2d")
        return p

    d_text = dev(n + 64, text)
    d_laid = dev(n_al + 64, laid)
    del laid
    d_off = dev(8 * (n_docs + 1), offs)
    d_off1 = dev(16, np.array([0, n], dtype=np.uint64))
    d_tok_off = dev(8 * (n_docs + 1))
    d_out = dev(4 * n + 64)
    n_out = C.c_uint64()

    def timing():
        w, sc, cp = C.c_double(), C.c_double(), C.c_double()
        lib.gbpe_encode_last_timing(ctx, C.byref(w), C.byref(sc), C.byref(cp))
        return {"ms_walk": w.value, "ms_scan": sc.value, "ms_compact": cp.value}

    def leg_batch():
        check(lib.gbpe_encode_batch_device(ctx, trie, d_text, n, d_off, n_docs, cs, d_out, n, d_tok_off, C.byref(n_out)),
              "encode batch")
        return int(n_out.value)

    def leg_loop():
        total = 0
        base_in, base_out = d_laid.value, d_out.value
        for s, ln in zip(starts.tolist(), lens.tolist()):
            check(lib.gbpe_encode_device(ctx, trie, C.c_void_p(base_in + s), ln, cs, C.c_void_p(base_out + 4 * total),
                                         n - total, C.byref(n_out)), "encode")
            total += int(n_out.value)
        return total

    def leg_batch1():
        check(lib.gbpe_encode_batch_device(ctx, trie, d_text, n, d_off1, 1, cs, d_out, n, d_tok_off, C.byref(n_out)),
              "encode batch (one document)")
        return int(n_out.value)

    def leg_single():
        check(lib.gbpe_encode_device(ctx, trie, d_text, n, cs, d_out, n, C.byref(n_out)), "encode")
        return int(n_out.value)

    def digest(count):
        host = np.empty(count, np.uint32)
        check(lib.gbpe_memcpy_d2h(ctx, host.ctypes.data_as(C.c_void_p), d_out, 4 * count), "d2h")
        return hashlib.sha256(host.tobytes()).hexdigest()[:16]

    legs = {"batch": leg_batch, "loop": leg_loop, "batch1": leg_batch1, "single": leg_single}
    tokens, sha, kernel_ms = {}, {}, {}
    for name, fn in legs.items():   # warm-up: every leg once (buffers grown, code objects loaded) + its tokens
        tokens[name] = fn()
        lib.gbpe_synchronize(ctx)
        sha[name] = digest(tokens[name])
    assert sha["batch"] == sha["loop"] and tokens["batch"] == tokens["loop"], "batch and loop tokens differ"
    assert sha["batch1"] == sha["single"] and tokens["batch1"] == tokens["single"], "one-document tokens differ"
    wall = {name: [] for name in legs}
    for _ in range(args.reps):   # the legs alternate
        for name, fn in legs.items():
            lib.gbpe_synchronize(ctx)
            t0 = time.perf_counter()
            fn()
            lib.gbpe_synchronize(ctx)
            wall[name].append(time.perf_counter() - t0)
            if name in ("batch", "batch1", "single"):
                kernel_ms.setdefault(name, []).append(timing())
    res = {name: stats(xs) for name, xs in wall.items()}

    def ratio(num, den):
        r = [a / b for a, b in zip(wall[num], wall[den])]
        return {"median": float(np.median(r)), "min": float(np.min(r)), "max": float(np.max(r))}

    print(json.dumps({
        "bytes": n, "chunk_size": cs, "vocab": int(args.vocab), "seed": args.seed, "reps": args.reps,
        "documents": n_docs, "doc_bytes_min": int(lens.min()), "doc_bytes_max": int(lens.max()),
        "doc_bytes_mean": float(lens.mean()), "tokens": tokens, "sha256_16": sha, "wall_s": res,
        "loop_over_batch": ratio("loop", "batch"), "batch1_over_single": ratio("batch1", "single"),
        "kernel_ms_median": {name: {k: float(np.median([t[k] for t in ts])) for k in ts[0]}
                             for name, ts in kernel_ms.items()}}), flush=True)
    for p in (d_text, d_laid, d_off, d_off1, d_tok_off, d_out):
        lib.gbpe_device_free(ctx, p)
    lib.gbpe_trie_free(trie)
    lib.gbpe_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
