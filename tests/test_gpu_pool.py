"""Every pool block a trainer or lexicon shard takes goes back when it is destroyed.

Under ``GBPE_DEBUG=poison=1`` ``gbpe_ctx_destroy`` reports the blocks still busy
(api.hip).  The key is read once per process, so a fresh child process builds one
context, then creates, steps and destroys a trainer along every path that allocates:
the plain u16 run (lexicon entry, zone shrinks, paired launches), the same without the
lexicon (in-place sectors and their growth), u32 symbols, the table growing inside and
outside the sparse loop, a state round trip, the lexicon hand-over with its expansion,
and two calls refused by input validation after they have allocated.  Nothing here
provokes a device error.  The parent asserts the report, the exit status and every
run's merge count.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

EXPECTED = {"plain_u16": 768, "no_lexicon": 768, "u32": 300, "table_rehash": 1200, "table_recount": 1200,
            "state": 256 + 128, "lexicon_root": 200, "refused_create": "invalid", "refused_expand": "invalid"}


def _child():
    import test_gpu_lexicon_build as LB   # (puts gpu-bpe_amd and oracle on the path)
    from gpubpe import _lib, synth
    from gpubpe.checkpoint import ResumedTrainer, export_state
    from gpubpe.lexshard import OCC, GpuLexBackend

    lib = _lib.load()
    ctx = C.c_void_p()
    _lib.check(lib.gbpe_ctx_create(0, C.byref(ctx)), None, "ctx")
    got = {}

    def knobs(s=""):   # every key but poison is read when a trainer is created
        os.environ["GBPE_DEBUG"] = "poison=1" + ("," + s if s else "")

    def create(data, target, batch=128, flags=0, table_log2=0):
        opts = _lib.TrainOpts(target_vocab_size=target, vocab_size=256, next_token_id=256, batch_size=batch,
                              flags=flags, table_log2=table_log2)
        t = C.c_void_p()
        _lib.check(lib.gbpe_trainer_create(ctx, data, len(data), None, 0, C.byref(opts), C.byref(t)), ctx, "create")
        return t

    def step(t, want, batch=128):
        out = (C.c_uint32 * (4 * batch))()
        done = 0
        while done < want:
            nd, es = C.c_uint32(), C.c_uint32()
            _lib.check(lib.gbpe_trainer_step(t, min(batch, want - done), out, C.byref(nd), C.byref(es)), ctx, "step")
            done += nd.value
            if nd.value == 0 or es.value:
                break
        return done

    def run(name, debug, data, target, want, **kw):
        knobs(debug)
        t = create(data, target, **kw)
        try:
            got[name] = step(t, want, kw.get("batch", 128))
            st = _lib.TrainerStats()
            lib.gbpe_trainer_stats_get(t, C.byref(st))
        finally:
            lib.gbpe_trainer_destroy(t)
        return st

    c1 = synth.english(262_144, seed=1)
    st = run("plain_u16", "", c1, 1024, 768)
    assert st.lexicon_builds >= 1 and st.sparse_merges and st.paired_merges, "plain run: no lexicon / sparse / paired merges"
    st = run("no_lexicon", "lexicon=0", c1, 1024, 768)
    assert st.lexicon_builds == 0 and st.sparse_merges
    st = run("u32", "", c1, 65536, 300)
    assert st.bytes_per_symbol == 4
    grow = synth.english(300000, seed=41)
    for name, rehash in (("table_rehash", "1"), ("table_recount", "0")):
        st = run(name, "rehash=" + rehash, grow, 256 + 1200, 1200, batch=16, flags=_lib.GBPE_TRAIN_SPARSE_EARLY,
                 table_log2=13)
        assert st.table_slots >= 1 << 15, st.table_slots

    # state round trip: 256 merges, export, a second trainer from the state, 128 more
    knobs()
    t = create(c1, 1024)
    try:
        n0 = step(t, 256)
        cur, prev = export_state(lib, ctx, t)
    finally:
        lib.gbpe_trainer_destroy(t)
    rt = ResumedTrainer(lib, ctx, cur, prev, 1024, 256 + n0)
    try:
        got["state"] = n0 + step(rt.t, 128)
    finally:
        rt.close()

    # lexicon hand-over: three pieces, the root, 200 merges, the expansion; and the two refused calls
    data = LB._edge()["data"]
    pieces = LB._cut_at_word_starts(data, [0.3, 0.62])
    vocab = 256 + 200
    root, bes, infos, parts, mp, refs, stores, muls = LB._root_case((lib, ctx, None), pieces, vocab)
    try:
        zone = np.concatenate([p["zone"] for p in parts])
        body = int(sum(i["body"] for i in infos))
        bad = GpuLexBackend(lib, ctx, vocab)
        bes.append(bad)
        try:   # the stores without their last separator: an odd number of words
            bad.root_create(np.ascontiguousarray(stores[:-1]), np.ascontiguousarray(muls[:-1]), zone,
                            int(stores.shape[0]) - 1, int(zone.shape[0]), body, int(sum(i["entries"] for i in infos)))
            got["refused_create"] = "accepted"
        except _lib.GpuBpeError as e:
            got["refused_create"] = "invalid" if e.code == _lib.GBPE_E_INVALID else e.code
        merges = 0
        while merges < 200:
            m, early = root.root_step(min(128, 200 - merges))
            merges += len(m)
            if not m or early:
                break
        got["lexicon_root"] = merges
        occ, off = [], 0
        for be, info in zip(bes, infos):
            ne = info["entries"]
            be.remap(np.ascontiguousarray(mp[off: off + ne]), ne)
            off += ne
            occ.append(be.export(OCC, info["words"] * 4, "cpu").numpy().view(np.uint32).copy())
        occ = np.ascontiguousarray(np.concatenate(occ))
        try:   # one occurrence short: the total no longer matches the trainer's
            root.root_expand(np.ascontiguousarray(occ[:-1]), int(occ.shape[0]) - 1)
            got["refused_expand"] = "accepted"
        except _lib.GpuBpeError as e:
            got["refused_expand"] = "invalid" if e.code == _lib.GBPE_E_INVALID else e.code
        fin = root.root_expand(occ, int(occ.shape[0]))
        assert fin.shape[0] == int(root.root_stats().symbol_count)
    finally:
        for be in bes:
            be.close()
    lib.gbpe_ctx_destroy(ctx)
    print(json.dumps(got), flush=True)


def test_destroy_returns_every_pool_block():
    env = dict(os.environ, GBPE_DEBUG="poison=1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                       timeout=180, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    report = [ln for ln in p.stderr.splitlines() if ln.startswith("[pool] busy at context destroy:")]
    assert report == ["[pool] busy at context destroy: device 0 pinned 0"], p.stderr[-4000:]
    assert json.loads(p.stdout.splitlines()[-1]) == EXPECTED


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
