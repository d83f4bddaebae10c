"""A GBPE_DEBUG key the library does not know fails context and trainer creation.

Many GPU tests reach the path they test only through a key (prej, pair, lxtwo, rfl,
delta_mt, dec_plain, ...): a misspelt or retired key that was skipped silently would
let such a test pass on the default path.  Both creation calls return GBPE_E_INVALID
and gbpe_last_error names the key (csrc/common.h gbpe_debug_unknown); known keys,
and an empty entry after a trailing comma, run as before.  One step of four merges
over 4 KiB each.
"""
import functools
import json
import os
import subprocess
import sys

import pytest

import bpe_oracle as O

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-bpe_amd")
TARGET = 260


@pytest.fixture(scope="module")
def eng():
    from gpubpe import BPEEngine
    return BPEEngine(0).init()


@functools.lru_cache(maxsize=None)
def _data():
    from gpubpe import synth
    return synth.english(4096, seed=9)


@functools.lru_cache(maxsize=None)
def _ref():
    return [m[:3] for m in O.train(_data(), TARGET)["merges"]]


def _train(eng):
    from gpubpe import BPETrainer
    return BPETrainer(eng).train(_data(), target_vocab_size=TARGET)["merges"]


@pytest.mark.parametrize("knobs,key", [("bcap=512", "bcap"), ("pair=0,nosuchkey=1", "nosuchkey")])
def test_unknown_key_fails_trainer_creation(eng, monkeypatch, knobs, key):
    from gpubpe import _lib
    monkeypatch.setenv("GBPE_DEBUG", knobs)
    with pytest.raises(_lib.GpuBpeError) as e:
        _train(eng)
    assert e.value.code == _lib.GBPE_E_INVALID
    assert key in str(e.value)


@pytest.mark.parametrize("knobs", ["pair=0,prej=3", "poison=1,"])
def test_known_keys_train_normally(eng, monkeypatch, knobs):
    monkeypatch.setenv("GBPE_DEBUG", knobs)
    got = _train(eng)
    assert len(got) == TARGET - 256 and got == _ref()


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from gpubpe import BPEEngine, _lib
try:
    BPEEngine(0).init()
    print(json.dumps({"code": 0, "msg": ""}))
except _lib.GpuBpeError as e:
    print(json.dumps({"code": e.code, "msg": str(e)}))
"""


def test_unknown_key_fails_context_creation():
    from gpubpe import _lib
    env = dict(os.environ, GBPE_DEBUG="nosuchkey=1")
    p = subprocess.run([sys.executable, "-c", CHILD, PKG], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.splitlines()[-1])
    assert got["code"] == _lib.GBPE_E_INVALID
    assert "nosuchkey" in got["msg"]
