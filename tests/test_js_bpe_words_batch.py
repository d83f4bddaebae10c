"""MergeEncoder.encodeBatch and GpuPreTokenizer.preTokenizeBatch of the Node.js host
(N-API addon) against the per-document oracle: one case per mode, plus the hand pairs
on which the per-document GPT-4 rules differ from the whole-buffer ones.
"""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from bpe_words_batch_ref import GPT4, HAND_PAIRS, HEUR, MASK, NONE, encode_words_batch_ref, gpt4_batch_ref, random_cuts, split
from bpe_words_ref import model, text
from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_addon_bpe_words_batch(tmp_path):
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    merges, data = model("code", 53), text("code", 53)
    offs = random_cuts(data, 300, seed=7)
    docs = split(data, offs)
    mask = (np.random.default_rng(46).random(len(data)) < 0.1).astype(np.uint8)
    want = {}
    for name, mode in (("none", NONE), ("mask", MASK), ("heuristic", HEUR), ("gpt4", GPT4)):
        tokens, tok_off = encode_words_batch_ref(docs, merges, mode, mask if mode == MASK else None)
        want[name] = {"tokens": tokens, "offsets": tok_off}
    case = {"merges": merges, "text_b64": base64.b64encode(data).decode(), "offsets": offs.tolist(), "mask": mask.tolist(),
            "want": want, "ws_gpt4": gpt4_batch_ref(docs).tolist(),
            "pairs": [{"docs_b64": [base64.b64encode(d).decode() for d in p[0]], "per": p[2]} for p in HAND_PAIRS]}
    path = tmp_path / "bpe_words_batch.json"
    path.write_text(json.dumps(case))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_bpe_words_batch.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
