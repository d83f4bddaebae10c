"""TrieTokenizer.decodeBytes / decodeBatch of the Node.js host (N-API addon) against
the oracle's decode: the bytes of a stream, and one view per document.
"""
import base64
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bpe_oracle as O
from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_js_addon_decode(tmp_path):
    addon = os.path.join(ROOT, "gpu-bpe_amd", "js", "gpubpe.node")
    assert os.path.exists(addon), "build the addon: make -C gpu-bpe_amd addon"
    from gpubpe import synth
    merges = [m[:3] for m in O.train(synth.multilingual(40000, seed=43), 500)["merges"]]
    vocab = O.vocab_from_merges(merges).entries + [[]]          # an empty entry, the last id
    V = len(vocab)
    rng = np.random.default_rng(45)
    counts = (1, 0, 63, 64, 65, 700, 0, 4097, 2)
    docs = [rng.integers(0, V, size=c).tolist() for c in counts]
    docs[2][5], docs[5][0], docs[7][4095], docs[7][4096] = V, 0xFFFFFFFF, 70000, V - 1   # unknown ids, the empty entry
    stream = [t for d in docs for t in d]
    b64 = lambda b: base64.b64encode(b).decode()   # noqa: E731
    case = {"vocab": vocab, "docs": docs, "docs_b64": [b64(O.decode(d, vocab)) for d in docs],
            "stream_b64": b64(O.decode(stream, vocab))}
    path = tmp_path / "decode.json"
    path.write_text(json.dumps(case))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_decode.mjs"), str(path)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1].startswith("ok")
