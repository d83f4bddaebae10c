#!/usr/bin/env python3
"""The byte spans of the merge-rank encoder's tokens (gbpe_bpe_encode_spans*): two
measurements (diagnostic, device-resident, seeded).  Every comparison alternates its two
sides, with `--reps` (at least 5) repetitions each, and reports median, minimum and maximum.

  a  plain path against another build (`--parent-root PATH`: a checkout of the parent commit
     with its library built): each tree's own tools/bpe_words_bench.py at its defaults in
     child processes, that build and this one in turn, `--rounds` times each.  The figure is
     gpt4_256 on code; the verdict says whether this build's median lies within the other
     build's own minimum-maximum spread over all its repetitions.  The plain kernels are the
     parent's instruction for instruction (tools/codeobj_diff.py), so anything else is a finding.
  b  cost of the spans: bpe_words_bench's trained model (`--vocab` ids) on the same resident
     `--bytes` of code (seed 6), GBPE_WORDS_GPT4 at the shipped chunk size:
     gbpe_bpe_encode_words_device against gbpe_bpe_encode_spans_device, with the three kernel
     phases of gbpe_bpe_encode_last_timing.  The tokens are equal, and the spans' lengths are
     the tokens' vocabulary lengths (no special table here): asserted.

Prints one JSON line.  argv: --bytes N --reps R --vocab V --sample-bytes N --parts a,b
--parent-root PATH --rounds R.
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
    print(f"[bpe_spans_bench] {msg}", file=sys.stderr, flush=True)


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
        sample = (bench.make_corpus({"gen": "multilingual", "n": half, "seed": 4}) +
                  bench.make_corpus({"gen": "code", "n": half, "seed": 5}))
        d = bench.device_buffer(self.lib, self.ctx, sample)
        t0 = time.perf_counter()
        merges, _ = bench.train_run(self.lib, self.ctx, d, len(sample), a.vocab, flags=self._lib.GBPE_TRAIN_GPT4_BOUNDARIES)
        self.lib.gbpe_device_free(self.ctx, d)
        note(f"trained {merges.shape[0]} merges on {len(sample)} bytes in {time.perf_counter() - t0:.1f} s")
        return np.ascontiguousarray(merges[:, :3], dtype=np.uint32)

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.lib.gbpe_device_alloc(self.ctx, nbytes, C.byref(p)), "alloc")
        return p

    def resident(self, text):
        self.n = len(text)
        self.d_text = self.bench.device_buffer(self.lib, self.ctx, text)
        self.d_out = self.alloc(4 * self.n + 64)
        self.d_start = self.alloc(8 * self.n + 64)

    def words(self, bpe):
        n_out = C.c_uint64()
        self.ok(self.lib.gbpe_bpe_encode_words_device(self.ctx, bpe, self.d_text, self.n, None, self._lib.GBPE_WORDS_GPT4,
                                                      self.d_out, self.n, C.byref(n_out)), "encode words")
        return int(n_out.value)

    def spans(self, bpe):
        n_out = C.c_uint64()
        self.ok(self.lib.gbpe_bpe_encode_spans_device(self.ctx, bpe, None, self.d_text, self.n, None, 0, None,
                                                      self._lib.GBPE_WORDS_GPT4, self.d_out, self.d_start, self.n, None,
                                                      C.byref(n_out)), "encode spans")
        return int(n_out.value)

    def fetch(self, ptr, count, dtype):
        host = np.empty(count, dtype)
        self.ok(self.lib.gbpe_memcpy_d2h(self.ctx, host.ctypes.data_as(C.c_void_p), ptr, host.nbytes), "d2h")
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
        h = C.c_void_p()
        self.ok(self.lib.gbpe_bpe_upload(self.ctx, m3.ctypes.data_as(self._lib.u32p), m3.shape[0], C.byref(h)), "bpe upload")
        want = self.fetch(self.d_out, self.words(h), np.uint32)
        count = self.spans(h)
        got, starts = self.fetch(self.d_out, count, np.uint32), self.fetch(self.d_start, count, np.uint64)
        assert np.array_equal(got, want), "the spans call's tokens differ"
        length = np.ones(int(m3[:, 2].max()) + 1, np.int64)
        for x, y, nid in m3.tolist():   # (ids in merge order: operands come first)
            length[nid] = length[x] + length[y]
        ends = np.append(starts[1:], np.uint64(self.n)).astype(np.int64)
        assert int(starts[0]) == 0 and np.array_equal(ends - starts.astype(np.int64), length[got]), "the spans are not the tokens' lengths"
        res = self.alternate({"words": lambda: self.words(h), "spans": lambda: self.spans(h)})
        res["spans_over_words"] = res["spans"]["wall_s"]["median"] / res["words"]["wall_s"]["median"]
        res["spans_minus_words_kernel_ms"] = {k: res["spans"]["kernel_ms_median"][k] - res["words"]["kernel_ms_median"][k]
                                              for k in res["words"]["kernel_ms_median"]}
        self.lib.gbpe_bpe_free(h)
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--sample-bytes", type=int, default=64 << 20)
    ap.add_argument("--parts", default="b")
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
        result["a_plain_vs_parent"] = part_a(args)
    if "b" in parts:
        b = Bench(args)
        m3 = b.train()
        result["merges"] = int(m3.shape[0])
        b.resident(b.bench.make_corpus({"gen": "code", "n": args.bytes, "seed": 6}))
        result["b_cost_of_spans"] = b.part_b(m3)
        for p in (b.d_text, b.d_out, b.d_start):
            b.lib.gbpe_device_free(b.ctx, p)
        b.lib.gbpe_ctx_destroy(b.ctx)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
