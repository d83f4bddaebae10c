#!/usr/bin/env python3
"""Word-bounded merge-rank encode against the whole-string encoder (diagnostic,
device-resident, seeded).  One model (`--vocab` ids, trained on the GPU with the
GPT-4 word starts on a sample that is half multilingual text, seed 4, and half
code, seed 5) encodes `--bytes` of code (seed 6) and of multilingual text (seed
3); the input stays resident and the legs alternate in one process after one
warm-up each:

  gpt4_CS        gbpe_bpe_encode_words_device, GBPE_WORDS_GPT4, the word kernels
                 at CS = 4096 / 1024 / 256 bytes per lane (GBPE_DEBUG me_cs);
  heuristic_CS   the same with GBPE_WORDS_HEURISTIC;
  none           gbpe_bpe_encode_words_device, GBPE_WORDS_NONE (no word cuts);
  host           gbpe_bpe_encode on host buffers (upload, allocation, readback).

Prints one JSON line: per text and leg the wall seconds of every repetition
(host clock around calls that end in a device synchronise) with median / min /
max, the three kernel phases (word starts, long + walk, scan + compact), the
token count and the sha256 of the tokens (equal across the chunk sizes of one
mode: asserted), and the fastest chunk size per mode.
argv: --bytes N --reps R --vocab V --sample-bytes N.
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

CHUNK_SIZES = (4096, 1024, 256)


def stats(xs):
    return {"reps": [round(x, 6) for x in xs], "median": float(np.median(xs)), "min": float(np.min(xs)),
            "max": float(np.max(xs))}


def note(msg):
    print(f"[bpe_words_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--sample-bytes", type=int, default=64 << 20)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the spread is part of the result)")
    import bench
    from gpubpe import _lib

    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.gbpe_ctx_create(0, C.byref(ctx)), None, "ctx")   # (no device: fails here, no fallback)

    def check(rc, what):
        _lib.check(rc, ctx, what)

    half = args.sample_bytes // 2
    sample = (bench.make_corpus({"gen": "multilingual", "n": half, "seed": 4}) +
              bench.make_corpus({"gen": "code", "n": half, "seed": 5}))
    d = bench.device_buffer(lib, ctx, sample)
    t0 = time.perf_counter()
    merges, _ = bench.train_run(lib, ctx, d, len(sample), args.vocab, flags=_lib.GBPE_TRAIN_GPT4_BOUNDARIES)
    note(f"trained {merges.shape[0]} merges on {len(sample)} bytes in {time.perf_counter() - t0:.1f} s")
    lib.gbpe_device_free(ctx, d)
    del sample
    m3 = np.ascontiguousarray(merges[:, :3], dtype=np.uint32)
    bpe = C.c_void_p()
    check(lib.gbpe_bpe_upload(ctx, m3.ctypes.data_as(_lib.u32p), m3.shape[0], C.byref(bpe)), "bpe upload")

    def timing():
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        lib.gbpe_bpe_encode_last_timing(ctx, C.byref(a), C.byref(b), C.byref(c))
        return {"ms_starts": a.value, "ms_walk": b.value, "ms_compact": c.value}

    result = {"bytes": args.bytes, "vocab": int(args.vocab), "merges": int(m3.shape[0]), "sample_bytes": args.sample_bytes,
              "reps": args.reps, "texts": {}}
    for gen, seed in (("code", 6), ("multilingual", 3)):
        text = bench.make_corpus({"gen": gen, "n": args.bytes, "seed": seed})
        n = len(text)
        d_text = bench.device_buffer(lib, ctx, text)
        d_out = C.c_void_p()
        check(lib.gbpe_device_alloc(ctx, 4 * n + 64, C.byref(d_out)), "alloc")
        host_out = np.empty(n, np.uint32)
        n_out = C.c_uint64()

        def fetch_sha(count):
            host = np.empty(count, np.uint32)
            check(lib.gbpe_memcpy_d2h(ctx, host.ctypes.data_as(C.c_void_p), d_out, host.nbytes), "d2h")
            return hashlib.sha256(host.tobytes()).hexdigest()[:16]

        def words_leg(mode, cs):
            def run():
                if cs:
                    os.environ["GBPE_DEBUG"] = f"me_cs={cs}"
                try:
                    check(lib.gbpe_bpe_encode_words_device(ctx, bpe, d_text, n, None, mode, d_out, n, C.byref(n_out)),
                          "encode words")
                finally:
                    os.environ.pop("GBPE_DEBUG", None)
                return int(n_out.value)
            return run

        def host_leg():
            check(lib.gbpe_bpe_encode(ctx, bpe, text, n, host_out.ctypes.data_as(_lib.u32p), n, C.byref(n_out)), "encode")
            return int(n_out.value)

        legs = {}
        for cs in CHUNK_SIZES:
            legs[f"gpt4_{cs}"] = words_leg(_lib.GBPE_WORDS_GPT4, cs)
        for cs in CHUNK_SIZES:
            legs[f"heuristic_{cs}"] = words_leg(_lib.GBPE_WORDS_HEURISTIC, cs)
        legs["none"] = words_leg(_lib.GBPE_WORDS_NONE, 0)
        legs["host"] = host_leg

        tokens, sha = {}, {}
        for name, fn in legs.items():   # warm-up: every leg once (pool blocks, code objects) + its tokens
            t0 = time.perf_counter()
            tokens[name] = fn()
            lib.gbpe_synchronize(ctx)
            sha[name] = (hashlib.sha256(host_out[: tokens[name]].tobytes()).hexdigest()[:16] if name == "host"
                         else fetch_sha(tokens[name]))
            note(f"{gen}: warm-up {name}: {tokens[name]} tokens, {time.perf_counter() - t0:.3f} s")
        for mode in ("gpt4", "heuristic"):
            assert len({sha[f"{mode}_{cs}"] for cs in CHUNK_SIZES}) == 1, f"{gen} {mode}: tokens differ between chunk sizes"
        assert sha["none"] == sha["host"], f"{gen}: mode NONE differs from gbpe_bpe_encode"

        wall = {name: [] for name in legs}
        kernel_ms = {name: [] for name in legs}
        for _ in range(args.reps):   # the legs alternate
            for name, fn in legs.items():
                lib.gbpe_synchronize(ctx)
                t0 = time.perf_counter()
                fn()
                lib.gbpe_synchronize(ctx)
                wall[name].append(time.perf_counter() - t0)
                if name != "host":
                    kernel_ms[name].append(timing())
        res = {}
        for name in legs:
            res[name] = {"tokens": tokens[name], "sha256_16": sha[name], "wall_s": stats(wall[name]),
                         "GBps": n / float(np.median(wall[name])) / 1e9}
            if kernel_ms[name]:
                ts = kernel_ms[name]
                res[name]["kernel_ms_median"] = {k: float(np.median([t[k] for t in ts])) for k in ts[0]}
                res[name]["kernel_ms_sum"] = stats([sum(t.values()) for t in ts])
        fastest = {mode: min(CHUNK_SIZES, key=lambda cs, m=mode: res[f"{m}_{cs}"]["wall_s"]["median"])
                   for mode in ("gpt4", "heuristic")}
        result["texts"][gen] = {"seed": seed, "bytes": n, "legs": res, "fastest_chunk_size": fastest}
        lib.gbpe_device_free(ctx, d_text)
        lib.gbpe_device_free(ctx, d_out)
        del text
    print(json.dumps(result), flush=True)
    lib.gbpe_bpe_free(bpe)
    lib.gbpe_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
