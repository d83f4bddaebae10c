"""Special tokens through the Node.js host (N-API addon): MergeEncoder with
specialTokens — encodeBytes, encodeBatch and findSpecial on the corpus recipe under the
GPT-4 rules, against special_ref.py's reference.
"""
import base64
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from special_ref import GPT4, IDS, TABLE, encode_special_ref, mark_ref, random_cuts, recipe, split

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_addon_special(tmp_path):
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    data, merges = recipe()
    offs = random_cuts(data, 300, seed=11)
    docs = split(data, offs)
    single, _ = encode_special_ref([data], merges, TABLE, IDS, GPT4)
    tokens, tok_off = encode_special_ref(docs, merges, TABLE, IDS, GPT4)
    assert len(single) == 8497
    case = {"merges": merges, "text_b64": base64.b64encode(data).decode(), "offsets": offs.tolist(),
            "specials_b64": [base64.b64encode(s).decode() for s in TABLE], "ids": IDS,
            "single": single, "batch": {"tokens": tokens, "offsets": tok_off},
            "mark": mark_ref(data, TABLE).tolist(), "mark_batch": mark_ref(docs, TABLE).tolist()}
    path = tmp_path / "special.json"
    path.write_text(json.dumps(case))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_special.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
