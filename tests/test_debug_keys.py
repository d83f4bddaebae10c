"""The GBPE_DEBUG keys are the same set in three places: the keys the sources read
(gbpe_debug_knob("...") under csrc), the list that makes every other key an error
(kGbpeDebugKeys in csrc/common.h), and the table of DESIGN §6.  Text only: no library.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-bpe_amd", "csrc")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _keys_read_by_the_sources():
    keys = set()
    for path in glob.glob(os.path.join(CSRC, "*")):
        keys.update(re.findall(r'gbpe_debug_knob\(\s*"([^"]*)"', _read(path)))
    return keys


def _keys_listed_valid():
    m = re.search(r"kGbpeDebugKeys\[\]\s*=\s*\{(.*?)\};", _read(os.path.join(CSRC, "common.h")), re.S)
    assert m, "csrc/common.h: no kGbpeDebugKeys list"
    names = re.findall(r'"([^"]*)"', m.group(1))
    assert len(names) == len(set(names)), "a key is listed twice"
    return set(names)


def _keys_documented():
    lines = _read(os.path.join(ROOT, "DESIGN.md")).splitlines()
    at = [i for i, ln in enumerate(lines) if ln.strip().startswith("| key | default |")]
    assert len(at) == 1, "DESIGN.md: expected one GBPE_DEBUG key table"
    keys = []
    for ln in lines[at[0] + 2:]:
        if not ln.strip().startswith("|"):
            break
        keys += re.findall(r"`([^`]*)`", ln.strip().split("|")[1])
    assert len(keys) == len(set(keys)), "a key has two rows"
    return set(keys)


def test_debug_keys_agree():
    read, valid, documented = _keys_read_by_the_sources(), _keys_listed_valid(), _keys_documented()
    assert len(read) >= 10   # (the parsing found them)
    assert read == valid
    assert valid == documented
