"""MergeEncoder.encodeBytes / encode with word starts of the Node.js host (N-API
addon) against the per-word oracle: the caller's mask, and the heuristic and GPT-4
word starts computed on the device.
"""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bpe_oracle as O
from bpe_words_ref import encode_words_ref, model, text
from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_addon_bpe_words(tmp_path):
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    merges, data = model("code", 53), text("code", 53)
    mask = (np.random.default_rng(46).random(len(data)) < 0.1).astype(np.uint8)
    want = {"none": O.encode_merge_order(data, merges),
            "mask": encode_words_ref(data, merges, mask),
            "heuristic": encode_words_ref(data, merges, O.heuristic_word_starts(np.frombuffer(data, np.uint8))),
            "gpt4": encode_words_ref(data, merges, O.gpt4_word_starts(data))}
    case = {"merges": merges, "text_b64": base64.b64encode(data).decode(), "mask": mask.tolist(), "want": want}
    path = tmp_path / "bpe_words.json"
    path.write_text(json.dumps(case))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_bpe_words.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
