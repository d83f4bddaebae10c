#!/usr/bin/env python3
"""The merge-rank encoder with ids above 0xFFFF (gbpe_bpe_upload_wide): three
measurements (diagnostic, device-resident, seeded).  Every comparison alternates its two
sides, with `--reps` (at least 5) repetitions each, and reports median, minimum and maximum.

  a  narrow path against another build (`--parent-root PATH`: a checkout of the parent commit
     with its library built): each tree's own tools/bpe_words_bench.py at its defaults in
     child processes, that build and this one in turn, `--rounds` times each.  The figure is gpt4_256 on code;
     the verdict says whether this build's median lies within the other build's own
     minimum-maximum spread over all its repetitions.
  b  cost of the width: bpe_words_bench's trained model (`--vocab` ids, GPT-4 word starts)
     through gbpe_bpe_upload, and the same model relabelled by f(id) = id + 0x10000 * (id % 4)
     (id >= 256) through gbpe_bpe_upload_wide, on the same resident `--bytes` of code (seed 6),
     GBPE_WORDS_GPT4 at 256 bytes per lane and GBPE_WORDS_NONE.  The token counts are equal and
     the wide tokens mapped back (their low 16 bits) are the narrow ones: asserted.
  c  a table beyond L2: the trained model grown to `--big-entries` entries (about 8 MiB of
     slots against 4 MiB of L2 per XCD) and run on the same text beside the trained model,
     both through the wide upload, with the three kernel phases of
     gbpe_bpe_encode_last_timing.

The grown model of part c is NOT BPE training: the trained model's most frequent adjacent
in-word token pairs that are not merges yet, counted once on a slice of the sample under the
GPT-4 word starts, are appended in count order under the ids that follow.  It stands in for a
100K-200K vocabulary's table size and hit rate, not for its merges.

Prints one JSON line.  argv: --bytes N --reps R --vocab V --sample-bytes N --count-bytes N
--big-entries N --parts a,b,c --parent-root PATH --rounds R.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
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
    print(f"[bpe_wide_bench] {msg}", file=sys.stderr, flush=True)


def relabel(merges):
    """f on every id of an [n, 3] list: bytes stay, id >= 256 becomes id + 0x10000 * (id % 4)."""
    m = merges.astype(np.uint32)
    return np.where(m < 256, m, m + 0x10000 * (m % 4)).astype(np.uint32)


def part_a(args):
    """bpe_words_bench.py at its defaults, the other build and this one in turn."""
    sides = {"parent": os.path.abspath(args.parent_root), "this": ROOT}   # (each tree binds its own library's symbols)
    env = {k: v for k, v in os.environ.items() if k != "GBPE_LIB"}
    runs = {k: [] for k in sides}
    for r in range(args.rounds):
        for side, path in sides.items():
            t0 = time.perf_counter()
            p = subprocess.run([sys.executable, os.path.join(path, "tools", "bpe_words_bench.py"), "--reps", str(args.reps)],
                               env=env, stdout=subprocess.PIPE, text=True, check=True)
            leg = json.loads(p.stdout.strip().splitlines()[-1])["texts"]["code"]["legs"]["gpt4_256"]
            runs[side].append({"wall_s": leg["wall_s"], "kernel_ms_sum": leg["kernel_ms_sum"], "tokens": leg["tokens"],
                               "sha256_16": leg["sha256_16"]})
            note(f"a: round {r} {side}: gpt4_256 on code median {leg['wall_s']['median'] * 1e3:.3f} ms "
                 f"({time.perf_counter() - t0:.0f} s for the run)")
    assert len({run["sha256_16"] for side in runs.values() for run in side}) == 1, "the two builds' tokens differ"
    out = {"figure": "bpe_words_bench.py defaults, texts/code/legs/gpt4_256/wall_s", "rounds": args.rounds, "reps": args.reps}
    for side in sides:
        pooled = [x for run in runs[side] for x in run["wall_s"]["reps"]]
        out[side] = {"wall_s": stats(pooled), "run_medians": [run["wall_s"]["median"] for run in runs[side]],
                     "kernel_ms_sum_run_medians": [run["kernel_ms_sum"]["median"] for run in runs[side]]}
    lo, hi, med = out["parent"]["wall_s"]["min"], out["parent"]["wall_s"]["max"], out["this"]["wall_s"]["median"]
    out["this_median_within_parent_spread"] = bool(lo <= med <= hi)
    out["this_over_parent_median"] = med / out["parent"]["wall_s"]["median"]
    return out


class Bench:
    def __init__(self, args):
        import bench
        from gpubpe import _lib
        self.args, self.bench, self._lib = args, bench, _lib
        self.lib = _lib.load()
        self.ctx = C.c_void_p()
        _lib.check(self.lib.gbpe_ctx_create(0, C.byref(self.ctx)), None, "ctx")   # (no device: fails here, no fallback)

    def ok(self, rc, what):
        self._lib.check(rc, self.ctx, what)

    def train(self):
        a, bench = self.args, self.bench
        half = a.sample_bytes // 2
        self.sample = (bench.make_corpus({"gen": "multilingual", "n": half, "seed": 4}) +
                       bench.make_corpus({"gen": "code", "n": half, "seed": 5}))
        d = bench.device_buffer(self.lib, self.ctx, self.sample)
        t0 = time.perf_counter()
        merges, _ = bench.train_run(self.lib, self.ctx, d, len(self.sample), a.vocab,
                                    flags=self._lib.GBPE_TRAIN_GPT4_BOUNDARIES)
        self.lib.gbpe_device_free(self.ctx, d)
        note(f"trained {merges.shape[0]} merges on {len(self.sample)} bytes in {time.perf_counter() - t0:.1f} s")
        return np.ascontiguousarray(merges[:, :3], dtype=np.uint32)

    def upload(self, m3, wide):
        h = C.c_void_p()
        fn = self.lib.gbpe_bpe_upload_wide if wide else self.lib.gbpe_bpe_upload
        m3 = np.ascontiguousarray(m3, dtype=np.uint32)
        self.ok(fn(self.ctx, m3.ctypes.data_as(self._lib.u32p), m3.shape[0], C.byref(h)), "bpe upload")
        return h

    def resident(self, text):
        self.n = len(text)
        self.d_text = self.bench.device_buffer(self.lib, self.ctx, text)
        self.d_out = C.c_void_p()
        self.ok(self.lib.gbpe_device_alloc(self.ctx, 4 * self.n + 64, C.byref(self.d_out)), "alloc")

    def encode(self, bpe, mode, cs=256):
        n_out = C.c_uint64()
        os.environ["GBPE_DEBUG"] = f"me_cs={cs}"
        try:
            self.ok(self.lib.gbpe_bpe_encode_words_device(self.ctx, bpe, self.d_text, self.n, None, mode, self.d_out, self.n,
                                                          C.byref(n_out)), "encode words")
        finally:
            os.environ.pop("GBPE_DEBUG", None)
        return int(n_out.value)

    def tokens(self, count):
        host = np.empty(count, np.uint32)
        self.ok(self.lib.gbpe_memcpy_d2h(self.ctx, host.ctypes.data_as(C.c_void_p), self.d_out, host.nbytes), "d2h")
        return host

    def timing(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self.lib.gbpe_bpe_encode_last_timing(self.ctx, C.byref(a), C.byref(b), C.byref(c))
        return {"ms_starts": a.value, "ms_walk": b.value, "ms_compact": c.value}

    def alternate(self, legs):
        """legs: {name: callable}.  One warm-up each, then `reps` rounds in which the legs take turns."""
        counts = {name: fn() for name, fn in legs.items()}
        wall, phases = {name: [] for name in legs}, {name: [] for name in legs}
        for _ in range(self.args.reps):
            for name, fn in legs.items():
                self.lib.gbpe_synchronize(self.ctx)
                t0 = time.perf_counter()
                fn()
                self.lib.gbpe_synchronize(self.ctx)
                wall[name].append(time.perf_counter() - t0)
                phases[name].append(self.timing())
        return {name: {"tokens": counts[name], "wall_s": stats(wall[name]),
                       "GBps": self.n / float(np.median(wall[name])) / 1e9,
                       "kernel_ms_median": {k: float(np.median([t[k] for t in phases[name]])) for k in phases[name][0]}}
                for name in legs}

    def part_b(self, m3):
        GPT4, NONE = self._lib.GBPE_WORDS_GPT4, self._lib.GBPE_WORDS_NONE
        narrow, wide = self.upload(m3, False), self.upload(relabel(m3), True)
        for mode in (GPT4, NONE):   # the same tokens, entry for entry
            want = self.tokens(self.encode(narrow, mode))
            got = self.tokens(self.encode(wide, mode))
            assert got.shape == want.shape and np.array_equal(got & 0xFFFF, want), "wide tokens mapped back differ"
            assert int(got.max()) > 0xFFFF
        res = self.alternate({"gpt4_256_narrow": lambda: self.encode(narrow, GPT4), "gpt4_256_wide": lambda: self.encode(wide, GPT4),
                              "none_narrow": lambda: self.encode(narrow, NONE), "none_wide": lambda: self.encode(wide, NONE)})
        for mode in ("gpt4_256", "none"):
            res[f"{mode}_wide_over_narrow"] = res[f"{mode}_wide"]["wall_s"]["median"] / res[f"{mode}_narrow"]["wall_s"]["median"]
        self.lib.gbpe_bpe_free(narrow)
        self.lib.gbpe_bpe_free(wide)
        return res

    def grown_model(self, m3):
        """m3 + its most frequent adjacent in-word pairs that are no merges, in count order (NOT BPE training)."""
        a = self.args
        piece = self.sample[: a.count_bytes // 2] + self.sample[len(self.sample) // 2:][: a.count_bytes // 2]
        n = len(piece)
        mask = np.zeros(n, np.uint8)
        self.ok(self.lib.gbpe_pretokenize_gpt4(self.ctx, piece, n, mask.ctypes.data_as(C.c_void_p)), "pretokenize")
        bpe = self.upload(m3, True)
        out = np.empty(n, np.uint32)
        cnt = C.c_uint64()
        self.ok(self.lib.gbpe_bpe_encode_words(self.ctx, bpe, piece, n, None, self._lib.GBPE_WORDS_GPT4,
                                               out.ctypes.data_as(self._lib.u32p), n, C.byref(cnt)), "encode")
        self.lib.gbpe_bpe_free(bpe)
        tok = out[: cnt.value].astype(np.int64)
        length = np.ones(int(m3[:, 2].max()) + 1, np.int64)
        for x, y, nid in m3.tolist():   # (ids in merge order: operands come first)
            length[nid] = length[x] + length[y]
        start = np.cumsum(length[tok]) - length[tok]
        assert int(start[-1] + length[tok[-1]]) == n
        inword = mask[start[1:]] == 0   # the pair (i, i + 1) lies inside one word
        pair = (tok[:-1].astype(np.uint64) << np.uint64(32)) | tok[1:].astype(np.uint64)
        keys, counts = np.unique(pair[inword], return_counts=True)
        order = np.argsort(-counts, kind="stable")[: max(0, a.big_entries - m3.shape[0])]
        extra = np.stack([keys[order] >> np.uint64(32), keys[order] & np.uint64(0xFFFFFFFF),
                          int(m3[:, 2].max()) + 1 + np.arange(order.size, dtype=np.uint64)], axis=1).astype(np.uint32)
        note(f"c: {keys.size} distinct in-word pairs in {n} bytes; {order.size} added, counts {int(counts[order[0]])} "
             f"to {int(counts[order[-1]])}")
        info = {"count_bytes": n, "distinct_pairs": int(keys.size), "added": int(order.size),
                "count_first": int(counts[order[0]]), "count_last": int(counts[order[-1]])}
        return np.concatenate([m3, extra]), info

    def part_c(self, m3):
        GPT4, NONE = self._lib.GBPE_WORDS_GPT4, self._lib.GBPE_WORDS_NONE
        grown, info = self.grown_model(m3)
        small, big = self.upload(m3, True), self.upload(grown, True)
        slots = 16
        while slots < 2 * grown.shape[0] + 16:
            slots <<= 1
        info.update({"entries": int(grown.shape[0]), "max_id": int(grown[:, 2].max()), "table_MiB": slots * 16 / 2 ** 20,
                     "trained_entries": int(m3.shape[0])})
        res = self.alternate({"gpt4_256_trained": lambda: self.encode(small, GPT4), "gpt4_256_grown": lambda: self.encode(big, GPT4),
                              "none_trained": lambda: self.encode(small, NONE), "none_grown": lambda: self.encode(big, NONE)})
        for mode in ("gpt4_256", "none"):
            res[f"{mode}_grown_over_trained"] = (res[f"{mode}_grown"]["wall_s"]["median"] /
                                                 res[f"{mode}_trained"]["wall_s"]["median"])
        self.lib.gbpe_bpe_free(small)
        self.lib.gbpe_bpe_free(big)
        return {"model": info, "legs": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--sample-bytes", type=int, default=64 << 20)
    ap.add_argument("--count-bytes", type=int, default=32 << 20)
    ap.add_argument("--big-entries", type=int, default=200_000)
    ap.add_argument("--parts", default="b,c")
    ap.add_argument("--parent-root")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5 (the spread is part of the result)")
    parts = set(args.parts.split(","))
    if "a" in parts and not args.parent_root:
        ap.error("part a needs --parent-root")
    result = {"bytes": args.bytes, "vocab": args.vocab, "sample_bytes": args.sample_bytes, "reps": args.reps}
    if "a" in parts:   # (before this process opens the device)
        result["a_narrow_vs_parent"] = part_a(args)
    if parts & {"b", "c"}:
        b = Bench(args)
        m3 = b.train()
        result["merges"] = int(m3.shape[0])
        b.resident(b.bench.make_corpus({"gen": "code", "n": args.bytes, "seed": 6}))
        if "b" in parts:
            result["b_cost_of_width"] = b.part_b(m3)
        if "c" in parts:
            result["c_table_beyond_l2"] = b.part_c(m3)
        b.lib.gbpe_device_free(b.ctx, b.d_text)
        b.lib.gbpe_device_free(b.ctx, b.d_out)
        b.lib.gbpe_ctx_destroy(b.ctx)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
