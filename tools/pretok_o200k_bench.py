#!/usr/bin/env python3
"""The o200k_base word starts against the cl100k_base word starts (diagnostic,
device-resident, seeded).  `--bytes` of code (seed 6) and of multilingual text
(seed 3) stay resident; the legs alternate in one process after one warm-up each:

  mask_gpt4      gbpe_pretokenize_gpt4_device + synchronise (the unchanged kernels' check leg);
  mask_cl100k    gbpe_pretokenize_cl100k_device + synchronise, the same bytes: the comparator;
  mask_o200k     gbpe_pretokenize_o200k_device + synchronise, the same bytes;
  words_cl100k   gbpe_bpe_encode_words_device, GBPE_WORDS_CL100K;
  words_o200k    gbpe_bpe_encode_words_device, GBPE_WORDS_O200K.

The model of the two encode legs (`--vocab` ids) is trained on the GPU with the
GPT-4 word starts on `--sample-bytes`, half multilingual text (seed 4) and half
code (seed 5).  Prints one JSON line: per text and leg the wall seconds of every
repetition (host clock around calls that end in a device synchronise) with median /
min / max; for the encode legs the three kernel phases of
gbpe_bpe_encode_last_timing and the token count; the word starts each mask found;
and the ratios o200k / cl100k of the medians.
argv: --bytes N --reps R --vocab V --sample-bytes N.
"""
import argparse
import ctypes as C
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
    print(f"[pretok_o200k_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=8192)
    ap.add_argument("--sample-bytes", type=int, default=16 << 20)
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
        d_out, d_ws = C.c_void_p(), C.c_void_p()
        check(lib.gbpe_device_alloc(ctx, 4 * n + 64, C.byref(d_out)), "alloc")
        check(lib.gbpe_device_alloc(ctx, n + 64, C.byref(d_ws)), "alloc")
        n_out = C.c_uint64()

        def mask_leg(fn):
            def run():
                check(fn(ctx, d_text, n, d_ws), "pretokenize")
                check(lib.gbpe_synchronize(ctx), "synchronise")
                return 0
            return run

        def words_leg(mode):
            def run():
                check(lib.gbpe_bpe_encode_words_device(ctx, bpe, d_text, n, None, mode, d_out, n, C.byref(n_out)),
                      "encode words")
                return int(n_out.value)
            return run

        legs = {"mask_gpt4": mask_leg(lib.gbpe_pretokenize_gpt4_device),
                "mask_cl100k": mask_leg(lib.gbpe_pretokenize_cl100k_device),
                "mask_o200k": mask_leg(lib.gbpe_pretokenize_o200k_device),
                "words_cl100k": words_leg(_lib.GBPE_WORDS_CL100K), "words_o200k": words_leg(_lib.GBPE_WORDS_O200K)}
        tokens, starts = {}, {}
        for name, fn in legs.items():   # warm-up: every leg once (pool blocks, code objects, the class tables)
            t0 = time.perf_counter()
            tokens[name] = fn()
            lib.gbpe_synchronize(ctx)
            if name.startswith("mask"):
                host = np.empty(n, np.uint8)
                check(lib.gbpe_memcpy_d2h(ctx, host.ctypes.data_as(C.c_void_p), d_ws, n), "d2h")
                starts[name] = int(np.count_nonzero(host))
                assert int(host.max()) == 1 and host[0] == 1
            note(f"{gen}: warm-up {name}: {time.perf_counter() - t0:.3f} s")

        wall = {name: [] for name in legs}
        kernel_ms = {name: [] for name in legs}
        for _ in range(args.reps):   # the legs alternate
            for name, fn in legs.items():
                lib.gbpe_synchronize(ctx)
                t0 = time.perf_counter()
                fn()
                lib.gbpe_synchronize(ctx)
                wall[name].append(time.perf_counter() - t0)
                if name.startswith("words"):
                    kernel_ms[name].append(timing())
        res = {}
        for name in legs:
            res[name] = {"wall_s": stats(wall[name]), "GBps": n / float(np.median(wall[name])) / 1e9}
            if name.startswith("mask"):
                res[name]["word_starts"] = starts[name]
            else:
                ts = kernel_ms[name]
                res[name]["tokens"] = tokens[name]
                res[name]["kernel_ms_median"] = {k: float(np.median([t[k] for t in ts])) for k in ts[0]}
        med = lambda name: res[name]["wall_s"]["median"]
        ratios = {"mask_wall": med("mask_o200k") / med("mask_cl100k"), "words_wall": med("words_o200k") / med("words_cl100k"),
                  "ms_starts": res["words_o200k"]["kernel_ms_median"]["ms_starts"] /
                  res["words_cl100k"]["kernel_ms_median"]["ms_starts"]}
        result["texts"][gen] = {"seed": seed, "bytes": n, "legs": res, "o200k_over_cl100k": ratios}
        for p in (d_text, d_out, d_ws):
            lib.gbpe_device_free(ctx, p)
        del text
    print(json.dumps(result), flush=True)
    lib.gbpe_bpe_free(bpe)
    lib.gbpe_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
