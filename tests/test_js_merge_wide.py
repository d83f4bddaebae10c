"""MergeEncoder of the Node.js host (N-API addon) on models with ids above 0xFFFF: a collision
list and one relabelled seed of merge_wide.py, whole string and { words: 'gpt4' }, against the
CPU references."""
import base64
import json
import os
import shutil
import subprocess

import pytest

import bpe_oracle as O
import merge_models as M
import merge_wide as W
from bpe_words_ref import encode_words_ref
from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]

ASCII = {0x20, ord("a"), ord("b")}   # of merge_models.POOL: what the GPT-4 rules' domain (UTF-8) holds


def _case(name, merges, narrow, text):
    """merges: the wide list; narrow: the list the references run on (relabel's source), or None."""
    ref = narrow if narrow is not None else merges
    back = W.relabel_tokens if narrow is not None else list
    want = {"none": back(M.np_merge_order(text, ref).tolist()),
            "gpt4": back(encode_words_ref(text, ref, O.gpt4_word_starts(text)))}
    return {"name": name, "merges": merges, "text_b64": base64.b64encode(text).decode(), "want": want}


def test_js_addon_merge_wide(tmp_path):
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    name, merges, text, want = W.COLLISIONS[0]
    cases = [_case(name, merges, None, text)]
    assert cases[0]["want"]["none"] == want
    # the first seed over ASCII with a space whose relabelled list is wide and whose words change the tokens
    for seed in M.SEEDS:
        c = M.model_case(seed)
        if 0x20 in c["alphabet"] and set(c["alphabet"]) <= ASCII and len(c["alphabet"]) >= 2:
            k = _case(f"seed_{seed}", W.relabel(c["merges"]), c["merges"], c["mask_text"][:300])
            if k["want"]["none"] != k["want"]["gpt4"] and max(k["want"]["gpt4"]) > 0xFFFF:
                cases.append(k)
                break
    assert len(cases) == 2
    path = tmp_path / "merge_wide.json"
    path.write_text(json.dumps({"cases": cases}))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_merge_wide.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
