#!/usr/bin/env python3
"""Device decode against its second scatter path and the host (diagnostic,
device-resident, seeded).  The bench's C3 vocab (32K, trained on the GPU on the
100 MiB multilingual sample, seed 4) encodes `--bytes` of multilingual text
(seed 3) on the device; the tokens stay resident and are decoded back, the legs
alternating in one process after one warm-up each:

  vector   gbpe_decode_device, the default scatter (16-byte output vectors);
  plain    the same call under GBPE_DEBUG dec_plain=1 (one lane per token);
  batch    gbpe_decode_batch_device with the token offsets that
           gbpe_encode_batch_device gave for tools/encode_batch_bench.py's seeded
           document cut of the text (the tokens of this leg are that call's);
  cpu      tests/decode_ref.py decode_np on the same tokens, once on the host.

Prints one JSON line: per-leg wall seconds of every repetition (host clock around
calls that end in a device synchronise) with median / min / max, the three
kernel phases, the ratios cpu / vector and plain / vector, and the achieved
fraction of the HBM rate for the algorithmic bytes (8 B per token + the output
bytes).  Every output's sha256 must equal the input text's (asserted).
argv: --bytes N --reps R --seed S --vocab V --sample-bytes N.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

# HBM3E of the MI355X: the specified peak and the measured float4-copy rate
HBM_PEAK_BPS = 8.0e12
HBM_COPY_BPS = 6.29e12


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
    from decode_ref import decode_np
    from encode_batch_bench import cut_documents
    from gpubpe import _lib, compile_vocab_to_trie, flatten_vocab, parse_header, parse_trie_buffers
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
    vflat, voffs = flatten_vocab(voc.entries)
    dvocab = C.c_void_p()
    check(lib.gbpe_vocab_upload(ctx, vflat.ctypes.data_as(C.c_void_p), voffs.ctypes.data_as(_lib.u64p),
                                len(voc.entries), C.byref(dvocab)), "vocab upload")

    text = np.frombuffer(bench.make_corpus({"gen": "multilingual", "n": args.bytes, "seed": 3}), dtype=np.uint8)
    n = int(text.shape[0])
    text_sha = hashlib.sha256(text.tobytes()).hexdigest()[:16]
    offs = cut_documents(n, args.seed)
    n_docs = int(offs.shape[0]) - 1

    def dev(nbytes, init=None):
        p = C.c_void_p()
        check(lib.gbpe_device_alloc(ctx, nbytes, C.byref(p)), "alloc")
        if init is not None and init.nbytes:
            check(lib.gbpe_memcpy_h2d(ctx, p, init.ctypes.data_as(C.c_void_p), init.nbytes), "h2d")
        return p

    def fetch(p, count, dtype):
        host = np.empty(count, dtype)
        check(lib.gbpe_memcpy_d2h(ctx, host.ctypes.data_as(C.c_void_p), p, host.nbytes), "d2h")
        return host

    # the tokens, resident: one stream, and the cut documents with their token offsets
    d_text = dev(n + 64, text)
    d_doc_off = dev(8 * (n_docs + 1), offs)
    d_tok = dev(4 * n + 64)
    d_tok_docs = dev(4 * n + 64)
    d_tok_off = dev(8 * (n_docs + 1))
    n_out = C.c_uint64()
    check(lib.gbpe_encode_device(ctx, trie, d_text, n, cs, d_tok, n, C.byref(n_out)), "encode")
    n_tok = int(n_out.value)
    check(lib.gbpe_encode_batch_device(ctx, trie, d_text, n, d_doc_off, n_docs, cs, d_tok_docs, n, d_tok_off,
                                       C.byref(n_out)), "encode batch")
    n_tok_docs = int(n_out.value)
    lib.gbpe_device_free(ctx, d_text)
    d_out = dev(n + 64)
    d_byte_off = dev(8 * (n_docs + 1))

    def timing():
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        lib.gbpe_decode_last_timing(ctx, C.byref(a), C.byref(b), C.byref(c))
        return {"ms_len": a.value, "ms_scan": b.value, "ms_scatter": c.value}

    def leg_vector():
        os.environ.pop("GBPE_DEBUG", None)
        check(lib.gbpe_decode_device(ctx, dvocab, d_tok, n_tok, d_out, n, C.byref(n_out)), "decode")
        return int(n_out.value)

    def leg_plain():
        os.environ["GBPE_DEBUG"] = "dec_plain=1"
        try:
            check(lib.gbpe_decode_device(ctx, dvocab, d_tok, n_tok, d_out, n, C.byref(n_out)), "decode (plain)")
        finally:
            os.environ.pop("GBPE_DEBUG", None)
        return int(n_out.value)

    def leg_batch():
        os.environ.pop("GBPE_DEBUG", None)
        check(lib.gbpe_decode_batch_device(ctx, dvocab, d_tok_docs, n_tok_docs, d_tok_off, n_docs, d_out, n, d_byte_off,
                                           C.byref(n_out)), "decode batch")
        return int(n_out.value)

    legs = {"vector": leg_vector, "plain": leg_plain, "batch": leg_batch}
    sha = {"text": text_sha}
    for name, fn in legs.items():   # warm-up: every leg once (buffers grown, code objects loaded) + its bytes
        check(lib.gbpe_memcpy_h2d(ctx, d_out, np.zeros(n, np.uint8).ctypes.data_as(C.c_void_p), n), "clear")
        assert fn() == n, f"{name}: decoded size differs from the text's"
        lib.gbpe_synchronize(ctx)
        sha[name] = hashlib.sha256(fetch(d_out, n, np.uint8).tobytes()).hexdigest()[:16]
        assert sha[name] == text_sha, f"{name}: decoded bytes differ from the text"
    assert np.array_equal(fetch(d_byte_off, n_docs + 1, np.uint64), offs), "batch: byte offsets differ from the cut"

    wall = {name: [] for name in legs}
    kernel_ms = {name: [] for name in legs}
    for _ in range(args.reps):   # the legs alternate
        for name, fn in legs.items():
            lib.gbpe_synchronize(ctx)
            t0 = time.perf_counter()
            fn()
            lib.gbpe_synchronize(ctx)
            wall[name].append(time.perf_counter() - t0)
            kernel_ms[name].append(timing())

    tokens = fetch(d_tok, n_tok, np.uint32)
    t0 = time.perf_counter()
    cpu = decode_np(tokens, voc.entries)
    cpu_s = time.perf_counter() - t0
    sha["cpu"] = hashlib.sha256(cpu.tobytes()).hexdigest()[:16]
    assert sha["cpu"] == text_sha, "decode_np differs from the text"
    del cpu

    def ratio(num, den):
        r = [a / b for a, b in zip(wall[num], wall[den])]
        return {"median": float(np.median(r)), "min": float(np.min(r)), "max": float(np.max(r))}

    res = {name: stats(xs) for name, xs in wall.items()}
    kmed = {name: {k: float(np.median([t[k] for t in ts])) for k in ts[0]} for name, ts in kernel_ms.items()}
    roof = {}
    for name in legs:
        alg_bytes = 8 * (n_tok_docs if name == "batch" else n_tok) + n
        ksum = sum(kmed[name].values()) * 1e-3
        roof[name] = {"kernel_s": ksum, "algorithmic_bytes": alg_bytes,
                      "wall_fraction_of_peak": alg_bytes / res[name]["median"] / HBM_PEAK_BPS,
                      "kernel_fraction_of_peak": alg_bytes / ksum / HBM_PEAK_BPS,
                      "kernel_fraction_of_copy_rate": alg_bytes / ksum / HBM_COPY_BPS,
                      "kernel_output_GBps": n / ksum / 1e9}
    print(json.dumps({
        "bytes": n, "tokens": n_tok, "tokens_batch": n_tok_docs, "documents": n_docs, "chunk_size": cs,
        "vocab": int(args.vocab), "vocab_blob_bytes": int(vflat.shape[0]), "seed": args.seed, "reps": args.reps,
        "sha256_16": sha, "wall_s": res, "kernel_ms_median": kmed, "cpu_decode_np_s": cpu_s,
        "cpu_over_vector": cpu_s / res["vector"]["median"], "plain_over_vector": ratio("plain", "vector"),
        "batch_over_vector": ratio("batch", "vector"), "algorithmic_bytes": 8 * n_tok + n,
        "hbm_peak_Bps": HBM_PEAK_BPS, "hbm_copy_Bps": HBM_COPY_BPS, "roofline": roof}), flush=True)
    for p in (d_doc_off, d_tok, d_tok_docs, d_tok_off, d_out, d_byte_off):
        lib.gbpe_device_free(ctx, p)
    lib.gbpe_vocab_free(dvocab)
    lib.gbpe_trie_free(trie)
    lib.gbpe_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
