"""Ids above 0xFFFF in the merge-rank encoder, on the CPU: the boundary declares, exports and
binds gbpe_bpe_upload_wide; the references are width-agnostic (the relabelled models of
merge_wide.py give f of the narrow tokens); the collision lists give the tokens written out by
hand; and an encoder that keys a pair by a << 16 | b in 32 bits fails every collision list and
a known set of the relabelled seeds — so a pass of test_gpu_merge_wide.py means something."""
import os
import re

import numpy as np
import pytest

import merge_models as M
import merge_wide as W
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "gpubpe.h")
UPLOAD_ARGS = 4   # ctx, merges, n_merges, out


def _texts(case):
    return case["texts"] + [case["mask_text"]]


# ── 1. the boundary ────────────────────────────────────────────────────────

def test_symbol_is_declared_exported_and_bound():
    from gpubpe import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+gbpe_bpe_upload_wide\s*\(([^)]*)\)\s*;", src)
    assert decl, "gpubpe.h does not declare gbpe_bpe_upload_wide"
    assert len(decl.group(1).split(",")) == UPLOAD_ARGS
    narrow = re.search(r"\bint\s+gbpe_bpe_upload\s*\(([^)]*)\)\s*;", src)
    assert [a.split()[:-1] for a in decl.group(1).split(",")] == [a.split()[:-1] for a in narrow.group(1).split(",")]
    assert "gbpe_bpe_upload_wide" in _lib.EXPORTED
    sig = {s[0]: s for s in _lib._SIGS}
    assert len(sig["gbpe_bpe_upload_wide"][2]) == UPLOAD_ARGS
    assert sig["gbpe_bpe_upload_wide"][1:] == sig["gbpe_bpe_upload"][1:]
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert hasattr(lib, "gbpe_bpe_upload_wide")
    assert "k_me_walk_wide" in [lib.gbpe_kernel_name(i).decode() for i in range(lib.gbpe_kernel_count())]
    napi = open(os.path.join(ROOT, "gpu-bpe_amd", "js", "addon", "gpubpe_napi.cc")).read()
    assert "gbpe_bpe_upload_wide(" in napi and '"bpeUploadWide"' in napi


def test_bound_and_abi_version():
    from gpubpe import _lib
    src = open(HEADER).read()
    assert int(re.search(r"#define GBPE_BPE_MAX_ID\s+(0x[0-9A-Fa-f]+)u", src).group(1), 16) == 0xFFFFFF
    assert _lib.GBPE_BPE_MAX_ID == 0xFFFFFF == W.MAX_ID
    assert int(re.search(r"#define GBPE_ABI_VERSION (\d+)", src).group(1)) == 10
    assert _lib.load().gbpe_abi_version() == 10


# ── 2. the references do not care about the width ──────────────────────────

def test_relabelling():
    ids = np.arange(256, 0x10000)
    wide = W.f_array(ids)
    assert np.unique(wide).size == ids.size and ((wide & 0xFFFF) == ids).all()
    assert int((wide == ids).sum()) == ids.size // 4 and int(wide.max()) == 0xFFFF + 0x30000 <= W.MAX_ID
    assert [W.f(b) for b in range(256)] == list(range(256)) and W.f_array([0, 255, 256, 259]).tolist() == [0, 255, 256, 0x30103]
    assert sum(any(v > 0xFFFF for m in W.relabel(M.model_case(s)["merges"]) for v in m) for s in M.SEEDS) >= 100


def test_references_on_the_relabelled_models():
    assert len(M.SEEDS) == 120
    for s in M.SEEDS:
        c = M.model_case(s)
        wide = W.relabel(c["merges"])
        assert len(wide) == len(c["merges"])
        for t in _texts(c):
            want = W.relabel_tokens(M.reference(t, c["merges"]))
            assert M.np_merge_order(t, wide).tolist() == want, (s, t)
            assert M.lowest_rank_encode(t, wide) == want, (s, t)


# ── 3. lists whose pairs share a packed key ────────────────────────────────

@pytest.mark.parametrize("name,merges,text,want", W.COLLISIONS, ids=[c[0] for c in W.COLLISIONS])
def test_collision_lists(name, merges, text, want):
    assert M.np_merge_order(text, merges).tolist() == want
    assert M.lowest_rank_encode(text, merges) == want
    assert len(M.upload_filter(merges)) == len(merges)   # every entry is live
    assert max(v for m in merges for v in m) <= W.MAX_ID and any(v > 0xFFFF for m in merges for v in m)


def test_collision_lists_hold_what_the_issue_names():
    by_name = {c[0]: c for c in W.COLLISIONS}
    key = lambda a, b: ((a << 16) | b) & 0xFFFFFFFF   # noqa: E731
    assert by_name["a_overflows"][1:] == ([[W.A, W.B, 0x10001], [0x10001, 5, 0x20000], [1, 5, 0x20001]],
                                          b"ab\x05\x01\x05", [0x20000, 0x20001])
    assert key(0x10001, 5) == key(1, 5) and key(2, 0x10007) == key(3, 7)
    live = M.upload_filter(by_name["b_bleeds"][1])
    assert (2, 0x10007) in live and (3, 7) in live and by_name["b_bleeds"][3] == [live[(2, 0x10007)][1], live[(3, 7)][1]]
    (a1, b1), (a2, b2) = [tuple(m[:2]) for m in by_name["a_bits_16_23"][1][2:]]
    assert b1 == b2 and a1 != a2 and (a1 ^ a2) & ~0xFF0000 == 0
    (a1, b1), (a2, b2) = [tuple(m[:2]) for m in by_name["b_bits_16_23"][1][2:]]
    assert a1 == a2 and b1 != b2 and (b1 ^ b2) & ~0xFF0000 == 0
    merges = by_name["boundary_ids"][1]
    for v in (0xFFFF, 0x10000, W.MAX_ID):
        assert any(m[2] == v for m in merges) and any(m[0] == v for m in merges)
        fired = [m[2] for m in merges if m[0] == v]
        assert set(fired) <= set(by_name["boundary_ids"][3])


# ── 4. the cases tell a truncating encoder from a right one ────────────────

# The relabelled seeds on which the packed-key encoder gives other tokens for some text.  Few: f keeps
# the low 16 bits, so the packed key of (f(a), f(b)) is ((a | b % 4) << 16) | b, and two live pairs
# share one only where b % 4 covers the bits in which their a's differ.  (Its tokens would be right
# on every other seed; an encoder that truncated the new ids as well would fail nearly all.)
PACKED_KEY_FAILS = [22, 26, 74, 75]


def test_packed_key_encoder_fails():
    for name, merges, text, want in W.COLLISIONS:
        assert W.packed_key_encode(text, merges) != want, name
    fails = []
    for s in M.SEEDS:
        c = M.model_case(s)
        wide = W.relabel(c["merges"])
        # (on the narrow model the packed key is exact)
        assert all(W.packed_key_encode(t, c["merges"]) == M.reference(t, c["merges"]) for t in c["texts"] if len(t) <= 64), s
        if any(W.packed_key_encode(t, wide) != W.relabel_tokens(M.reference(t, c["merges"])) for t in _texts(c)):
            fails.append(s)
    print(f"relabelled seeds the packed key fails: {fails}")
    assert fails == PACKED_KEY_FAILS
