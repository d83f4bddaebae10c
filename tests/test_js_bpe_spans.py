"""Byte spans of the merge-rank encode's tokens through the Node.js host (N-API addon):
MergeEncoder.encodeBytesSpans and encodeBatchSpans against the Python layer's results (which
this test first holds against the oracle of bpe_spans_ref.py) on three cases of
test_gpu_bpe_spans.py — one with a special whose id is a model token's, one with empty
documents — and the option errors of encodeBytes and encodeBatch.
"""
import base64
import json
import os
import shutil
import subprocess

import pytest

from bpe_spans_ref import GPT4, NONE, doc_tok_off, spans_ref
from bpe_words_ref import model, text
from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]

A = ord("a")
A_MERGES = [[A, A, 256], [256, A, 257], [256, 256, 258]]
EOT = b"<|endoftext|>"


def b64(b):
    return base64.b64encode(b).decode()


def test_js_addon_bpe_spans(tmp_path):
    from gpubpe import BPEEngine, MergeEncoder
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    code, merges = text("code", 53)[:5000], model("code", 53)
    runs = b" ".join(b"a" * k for k in range(1, 10)) * 12 + b"a" * 1025 + b" aaa"
    sdoc = b"aaaa" + EOT + b"aa" + EOT + EOT + b"a" * 300
    docs = [b"", code[:700], b"", b"", b"EOT" + code[700:1500] + b"EOT", code[1500:], b""]
    eng = BPEEngine().init()
    cases = []
    try:
        for name, m, table, single, dd, mode, kw, opts in (
                ("cascading runs", A_MERGES, {}, runs, None, NONE, {}, {}),
                ("a special with a model token's id", A_MERGES, {EOT: 256}, sdoc, None, GPT4, {"words": "gpt4"}, {"words": "gpt4"}),
                ("documents, some empty, a special", merges, {b"EOT": 70000}, None, docs, GPT4, {"words": "gpt4"}, {"words": "gpt4"})):
            enc = MergeEncoder(eng, m, special_tokens=table or None)
            sp, ids = list(table), list(table.values())
            if dd is None:
                tokens, starts = enc.encode_bytes_spans(single, **kw)
                want = spans_ref([single], m, sp, ids, mode)
                tok_off = None
            else:
                tokens, tok_off, starts = enc.encode_batch_spans(dd, **kw)
                want = spans_ref(dd, m, sp, ids, mode)
                assert tok_off.tolist() == doc_tok_off(dd, want[1])
                tok_off = tok_off.tolist()
            n = len(single) if dd is None else sum(len(d) for d in dd)
            assert tokens.tolist() == want[0] and starts.tolist() == want[1] + [n], name
            cases.append({"name": name, "merges": m, "specials_b64": [b64(s) for s in sp], "ids": ids,
                          "text_b64": b64(single) if dd is None else None, "docs_b64": [b64(d) for d in dd] if dd else None,
                          "opts": opts, "tokens": tokens.tolist(), "starts": starts.tolist(), "offsets": tok_off})
            enc.destroy()
    finally:
        eng.close()
    path = tmp_path / "bpe_spans.json"
    path.write_text(json.dumps({"cases": cases}))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_bpe_spans.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
