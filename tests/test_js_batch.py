"""TrieTokenizer.encodeBatch of the Node.js host (N-API addon) against the oracle:
one view per document, each the oracle's tokens of that document alone.
"""
import base64
import json
import os
import shutil
import subprocess

import pytest

import bpe_oracle as O
from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_addon_encode_batch(tmp_path):
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    from gpubpe import synth
    cs = 64
    merges = [m[:3] for m in O.train(synth.multilingual(40000, seed=43), 500)["merges"]]
    vocab = O.vocab_from_merges(merges).entries
    blob = O.compile_vocab_to_trie(vocab)
    nodes, edges = O.parse_trie_buffers(blob, O.parse_header(blob))
    text = synth.multilingual(12000, seed=44)
    docs, p = [], 5
    for ln in (1, 0, 63, 64, 65, 700, 0, 3001, 2):   # any byte position: multi-byte characters split
        docs.append(text[p:p + ln])
        p += ln
    tokens = [O.encode_chunked(d, nodes, edges, cs).tolist() if d else [] for d in docs]
    case = {"vocab": vocab, "chunkSize": cs, "docs_b64": [base64.b64encode(d).decode() for d in docs], "tokens": tokens,
            "text_b64": base64.b64encode(text).decode(), "text_tokens": O.encode_chunked(text, nodes, edges, cs).tolist()}
    path = tmp_path / "batch.json"
    path.write_text(json.dumps(case))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_batch.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
