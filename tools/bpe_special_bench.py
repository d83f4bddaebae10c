#!/usr/bin/env python3
"""Special tokens of the merge-rank encode (diagnostic, device-resident, seeded).

The model, the resident `--bytes` of code (seed 6) and its documents are
tools/bpe_words_batch_bench.py's.  Mode GBPE_WORDS_GPT4 everywhere.  Three parts, one
JSON line (also written to profiles/r10/bpe_special/bpe_special_bench.json):

  a  no_match_vs_parent (with `--parent-lib A.so B.so`: two copies of the parent
     commit's library)  gbpe_bpe_encode_special_device with an eight-entry <|...|> table
     on text that holds none, against gbpe_bpe_encode_words_device of both copies, each
     with its own context and buffers, alternating in one process with the slot order
     rotating; identical token sha256 asserted.  The spread between the two copies is
     the margin, the difference beyond it the feature's cost.  With it: the kernel
     phases of gbpe_bpe_encode_last_timing for the special call and for this library's
     plain call (matching and flags count under ms_starts), gbpe_specials_mark_device
     alone, and the bytes the matcher's passes move at the least.
  b  workload  the same bytes with <|endoftext|> after every document, one
     gbpe_bpe_encode_special_device call, against the parent's
     gbpe_bpe_encode_words_batch_device on the documents without the strings; the
     streams are equal once the special ids are dropped (asserted).
  c  host_pattern  what the call replaces: one gbpe_bpe_encode_words_device call per
     piece, for a seeded 1% of the pieces, extrapolated to all of them (marked so).

Wall seconds are the host clock around calls that end in a device synchronise, every
repetition kept, with median / min / max.
argv: --bytes N --reps R --vocab V --sample-bytes N --doc-bytes N --parent-lib A B --out PATH.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from bpe_words_batch_bench import Slot, cut_documents, load_other, stats, timed  # noqa: E402

EOT = b"<|endoftext|>"
TABLE = [EOT, b"<|fim_prefix|>", b"<|fim_middle|>", b"<|fim_suffix|>", b"<|endofprompt|>", b"<|im_start|>", b"<|im_end|>",
         b"<|pad|>"]
ID0 = 100000


def note(msg):
    print(f"[bpe_special_bench] {msg}", file=sys.stderr, flush=True)


def upload_specials(slot):
    from gpubpe import _lib
    raw = np.frombuffer(b"".join(TABLE), np.uint8)
    offs = np.zeros(len(TABLE) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in TABLE], dtype=np.uint64)
    ids = np.arange(ID0, ID0 + len(TABLE), dtype=np.uint32)
    sp = C.c_void_p()
    slot.ok(slot.lib.gbpe_specials_upload(slot.ctx, raw.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(_lib.u64p),
                                          ids.ctypes.data_as(_lib.u32p), len(TABLE), C.byref(sp)), "specials upload")
    return sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--sample-bytes", type=int, default=64 << 20)
    ap.add_argument("--doc-bytes", type=int, default=4096)
    ap.add_argument("--parent-lib", nargs=2, metavar=("A", "B"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "bpe_special", "bpe_special_bench.json"))
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
    assert not any(s in text for s in TABLE), "the corpus must hold no special"
    arr = np.frombuffer(text, np.uint8)
    offs = cut_documents(arr, args.doc_bytes, seed=9)
    n_docs = int(offs.shape[0]) - 1
    note(f"{n} bytes, {n_docs} documents")
    result = {"bytes": n, "documents": n_docs, "doc_bytes": args.doc_bytes, "vocab": int(args.vocab),
              "merges": int(m3.shape[0]), "sample_bytes": args.sample_bytes, "reps": args.reps, "text": "synth.code seed 6",
              "mode": "GBPE_WORDS_GPT4", "table": [s.decode() for s in TABLE]}

    new = Slot("new", lib, m3, text)
    sp = upload_specials(new)

    def special_single(slot=new, table=sp):
        slot.ok(lib.gbpe_bpe_encode_special_device(slot.ctx, slot.bpe, table, slot.d_text, slot.n, None, GPT4, slot.d_out,
                                                   slot.n, C.byref(slot.n_out)), "encode special")
        return int(slot.n_out.value)

    def mark_alone():
        new.ok(lib.gbpe_specials_mark_device(new.ctx, sp, new.d_text, n, None, 0, new.d_ws), "specials mark")

    # ── a: the cost of the feature when nothing matches ──
    part_a = {}
    cnt_new = special_single()
    sha_new = new.sha(new.d_out, cnt_new, np.uint32)
    cnt_plain = new.encode_single(GPT4)
    assert (cnt_plain, new.sha(new.d_out, cnt_plain, np.uint32)) == (cnt_new, sha_new), "a table that never matches changed the tokens"
    mark_alone()
    assert not new.fetch(new.d_ws, n, np.uint8).any()
    kms = {"special": [], "plain": []}
    wall = {"special": [], "plain": [], "specials_mark_device": []}
    for _ in range(args.reps):   # the legs alternate
        wall["special"].append(timed(new, special_single)[0])
        kms["special"].append(new.timing())
        wall["plain"].append(timed(new, lambda: new.encode_single(GPT4))[0])
        kms["plain"].append(new.timing())
        wall["specials_mark_device"].append(timed(new, mark_alone)[0])
    med = {k: {p: float(np.median([t[p] for t in v])) for p in v[0]} for k, v in kms.items()}
    part_a["this_library"] = {"tokens": cnt_new, "sha256_16": sha_new, "wall_s": {k: stats(v) for k, v in wall.items()},
                              "kernel_ms_median": med,
                              "ms_starts_special_minus_plain": med["special"]["ms_starts"] - med["plain"]["ms_starts"]}
    # at the least: k_sp_cand reads n and writes n, the mark memset writes n, k_sp_accept reads n, the flags memset
    # writes n, k_me_sp_mask reads n
    part_a["matcher_min_bytes"] = {"read": 3 * n, "written": 3 * n}
    mark_s = float(np.median(wall["specials_mark_device"]))
    part_a["specials_mark_device_gb_per_s"] = (2 * n + 2 * n) / mark_s / 1e9   # (cand r + w, mark memset, accept r)
    if args.parent_lib:
        slots = [Slot("parentA", load_other(args.parent_lib[0]), m3, text), new,
                 Slot("parentB", load_other(args.parent_lib[1]), m3, text)]
        shas = {}
        for s in slots:   # warm-up + identical outputs
            cnt = special_single() if s is new else s.encode_single(GPT4)
            shas[s.name] = (cnt, s.sha(s.d_out, cnt, np.uint32))
        assert len(set(shas.values())) == 1, f"the libraries disagree: {shas}"
        reps = 2 * args.reps + 2
        wall = {s.name: [] for s in slots}
        for r in range(reps):
            for s in slots[r % 3:] + slots[: r % 3]:   # the slot order rotates
                wall[s.name].append(timed(s, special_single if s is new else (lambda: s.encode_single(GPT4)))[0])
        m = {k: float(np.median(v)) for k, v in wall.items()}
        margin = abs(m["parentA"] - m["parentB"])
        over = m["new"] - max(m["parentA"], m["parentB"])
        part_a["vs_parent"] = {"reps": reps, "wall_s": {k: stats(v) for k, v in wall.items()},
                               "parent_spread_s": margin, "new_minus_slower_parent_s": over,
                               "cost_beyond_spread_s": max(0.0, over - margin)}
        parent = slots[0]
    else:
        parent = None
    result["a_no_match"] = part_a

    # ── b: the workload: <|endoftext|> after every document, one call ──
    o = offs.tolist()
    joined = bytearray()
    for k in range(n_docs):
        joined += text[o[k]:o[k + 1]] + EOT
    n2 = len(joined)
    wl = Slot("workload", lib, m3, bytes(joined))
    del joined
    sp_wl = upload_specials(wl)
    cnt_sp = special_single(wl, sp_wl)
    toks_sp = wl.fetch(wl.d_out, cnt_sp, np.uint32)
    assert int((toks_sp == ID0).sum()) == n_docs and int((toks_sp >= ID0).sum()) == n_docs
    base = parent or new   # (without --parent-lib: this library's batch call)
    d_off = base.alloc(8 * (n_docs + 1), offs)
    d_tok_off = base.alloc(8 * (n_docs + 1))

    def batch():
        base.ok(base.lib.gbpe_bpe_encode_words_batch_device(base.ctx, base.bpe, base.d_text, n, d_off, n_docs, None, GPT4,
                                                            base.d_out, n, d_tok_off, C.byref(base.n_out)), "encode batch")
        return int(base.n_out.value)

    cnt_b = batch()
    toks_b = base.fetch(base.d_out, cnt_b, np.uint32)
    assert cnt_sp == cnt_b + n_docs and np.array_equal(toks_sp[toks_sp < ID0], toks_b), \
        "the special call and the batch call give different tokens"
    sha_b = hashlib.sha256(toks_b.tobytes()).hexdigest()[:16]
    del toks_sp, toks_b
    wall = {"special": [], "batch": []}
    kms = []
    for _ in range(args.reps):
        wall["special"].append(timed(wl, lambda: special_single(wl, sp_wl))[0])
        kms.append(wl.timing())
        wall["batch"].append(timed(base, batch)[0])
    result["b_workload"] = {
        "bytes_with_specials": n2, "tokens": cnt_sp, "specials": n_docs, "sha256_16_without_specials": sha_b,
        "batch_library": base.name, "wall_s": {k: stats(v) for k, v in wall.items()},
        "special_kernel_ms_median": {p: float(np.median([t[p] for t in kms])) for p in kms[0]},
        "special_over_batch_median": float(np.median(wall["special"])) / float(np.median(wall["batch"]))}

    # ── c: the host pattern this replaces: one call per piece (a seeded 1%, extrapolated) ──
    rng = np.random.default_rng(12)
    pick = np.sort(rng.choice(n_docs, max(1, n_docs // 100), replace=False)).tolist()
    cnt = C.c_uint64()

    def per_piece():
        total = 0
        for k in pick:
            new.ok(lib.gbpe_bpe_encode_words_device(new.ctx, new.bpe, C.c_void_p(new.d_text.value + o[k]), o[k + 1] - o[k],
                                                    None, GPT4, C.c_void_p(new.d_out.value + 4 * total), n - total,
                                                    C.byref(cnt)), "encode words")
            total += cnt.value
        return total

    per_piece()
    wall_pp = [timed(new, per_piece)[0] for _ in range(args.reps)]
    result["c_host_pattern"] = {"pieces_timed": len(pick), "pieces": n_docs, "wall_s": stats(wall_pp),
                                "us_per_call": 1e6 * float(np.median(wall_pp)) / len(pick),
                                "extrapolated_all_pieces_s": float(np.median(wall_pp)) * n_docs / len(pick),
                                "extrapolated": True}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
