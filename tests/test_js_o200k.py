"""{ words: 'o200k_base' } and { rules: 'o200k_base' } of the Node.js host (N-API addon): the
tokens and the word starts against fixtures computed here from o200k_ref.py and the
per-word oracle.
"""
import base64
import json
import os
import shutil
import subprocess

import pytest

import o200k_corpora as K
import o200k_ref as R
from bpe_words_ref import encode_words_ref, model, text
from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_addon_o200k(tmp_path):
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    merges = model("code", 53)
    data = K.fuzz(2_000, 331) + text("code", 53)[:3_000] + K.BATCH_TEXT
    cut = 1234
    while data[cut] & 0xC0 == 0x80:      # (to a codepoint boundary)
        cut += 1
    docs = [data[:cut], b"", data[cut:], b"it's camelCase 12345 a's's\n"]
    b64 = lambda b: base64.b64encode(b).decode()
    case = {"merges": merges, "text_b64": b64(data), "mask": R.mask(data).tolist(),
            "tokens": encode_words_ref(data, merges, R.mask(data)),
            "docs_b64": [b64(d) for d in docs], "doc_masks": [R.mask(d).tolist() for d in docs],
            "doc_tokens": [encode_words_ref(d, merges, R.mask(d)) for d in docs]}
    path = tmp_path / "o200k.json"
    path.write_text(json.dumps(case))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_o200k.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
