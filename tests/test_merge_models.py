"""The adversarial merge lists of merge_models.py tell a right merge-rank encoder from a
wrong one — on the CPU, so that a pass of test_gpu_merge_models.py means something.

Every count below is over the fixed seed list and must be positive: the cases where the
reference's tokens differ from what an encoder gives that drops (0, 0), that treats a
merge with a missing operand as live, or that lets a repeated pair's last rank win.
The host model of the library's own algorithm (upload filter, lowest rank first) must
agree with the reference everywhere."""
import numpy as np

import bpe_oracle as O
import merge_models as M
from bpe_words_ref import encode_words_ref


def _texts(case):
    return case["texts"] + [case["mask_text"]]


def _short(case):
    return [t for t in case["texts"] if len(t) <= 64]


def test_generator_covers_the_issue():
    cases = [M.model_case(s) for s in M.SEEDS]
    assert len(cases) >= 100
    for s, c in zip(M.SEEDS, cases):
        ids = [m[2] for m in c["merges"]]
        assert len(ids) <= M.MAX_MERGES and len(set(ids)) == len(ids) and all(256 <= i <= 0xFFFF for i in ids), s
        assert 1 <= len(c["alphabet"]) <= 4 and set(c["alphabet"]) <= set(M.POOL), s
        assert [len(t) for t in c["texts"][:4]] == [0, 1, 2, 3], s
        assert all(set(t) <= set(c["alphabet"]) for t in _texts(c)), s
    nul = [c for c in cases if 0 in c["alphabet"]]
    assert 0.2 < len(nul) / len(cases) < 0.45
    assert all(M.model_case(s)["nul_nul"] == (s in M.GROUPS["nul_nul"]) for s in M.SEEDS)
    assert all(any(m[:2] == [0, 0] for m in M.model_case(s)["merges"]) == (s in M.GROUPS["nul_nul"]) for s in M.SEEDS)
    with_00 = [c for c in nul if any(m[:2] == [0, 0] for m in c["merges"])]
    only_0x = [c for c in nul if not any(m[:2] == [0, 0] for m in c["merges"])
               and any((m[0] == 0) != (m[1] == 0) for m in c["merges"])]
    assert len(with_00) >= 5 and len(only_0x) >= 5
    assert sum(len(c["merges"]) == 0 for c in cases) >= 1 and max(len(c["merges"]) for c in cases) >= 25
    assert any(m[2] == 256 for c in cases for m in c["merges"])
    assert sum(m[0] == m[1] for c in cases for m in c["merges"]) >= 50          # self-pairs
    assert sum(m[0] >= 256 and m[1] >= 256 for c in cases for m in c["merges"]) >= 50   # pairs of earlier tokens
    n_entries = sum(len(c["merges"]) for c in cases)
    assert 0.03 < sum(len(c["dead_ids"]) for c in cases) / n_entries < 0.15
    assert 0.03 < sum(len(c["later_ids"]) for c in cases) / n_entries < 0.15
    # a dead id (a repeated pair's) is an operand of a later entry
    assert sum(any(d in m[:2] for m in c["merges"]) for c in cases for d in c["dead_ids"]) >= 20


def test_ffff_is_an_operand_of_a_live_merge():
    fired_pair = fired_byte = 0
    for s in M.SEEDS:
        c = M.model_case(s)
        if not c["ffff"]:
            continue
        table = M.upload_filter(c["merges"])
        assert (0xFFFF, 0xFFFF) in table and c["merges"][0][2] == 0xFFFF, s
        nid = table[(0xFFFF, 0xFFFF)][1]
        fired_pair += any(nid in O.encode_merge_order(t, c["merges"]) for t in _short(c))
        if (0xFFFF, c["alphabet"][0]) in table:
            nid = table[(0xFFFF, c["alphabet"][0])][1]
            fired_byte += any(nid in O.encode_merge_order(t, c["merges"]) for t in _short(c))
    assert fired_pair >= 5 and fired_byte >= 1


def test_library_algorithm_agrees_with_the_reference():
    for s in M.SEEDS:
        c = M.model_case(s)
        for t in _short(c):
            assert M.lowest_rank_encode(t, c["merges"]) == O.encode_merge_order(t, c["merges"]), (s, c["merges"], t)


def test_cases_discriminate():
    n_00 = n_dead = n_dup = 0
    for s in M.SEEDS:
        c = M.model_case(s)
        merges = c["merges"]
        without_00 = [m for m in merges if m[:2] != [0, 0]]
        for t in _short(c):
            want = O.encode_merge_order(t, merges)
            n_00 += len(without_00) != len(merges) and O.encode_merge_order(t, without_00) != want
            n_dead += M.lowest_rank_encode(t, merges, live="all") != want
            n_dup += M.lowest_rank_encode(t, merges, live="last") != want
    print(f"texts that tell: (0,0) dropped {n_00}, every merge live {n_dead}, last rank wins {n_dup}")
    assert n_00 >= 10 and n_dead >= 10 and n_dup >= 10


def test_nul_group_holds_nul_runs_inside_segments():
    # a table whose empty marker is pid 0 answers the lookup of (0, 0) with an empty slot: rank 0,
    # new id 0.  That shows where two NUL bytes lie inside one segment, with or without the entry (0, 0)
    n = 0
    for s in M.GROUPS["nul"]:
        c = M.model_case(s)
        assert not any(m[:2] == [0, 0] for m in c["merges"]) and 0 in c["alphabet"]
        if (0, 0) in M.cross_pairs(c["merges"]):
            n += sum(b"\0\0" in t for t in _short(c))
    assert n >= 10


def test_closed_models_are_one_segment():
    closed = [M.model_case(s) for s in M.SEEDS if M.model_case(s)["closed"]]
    assert len(closed) >= len(M.SEEDS) // 3
    for c in closed:
        live = M.upload_filter(c["merges"])
        assert all((a, b) in live for a in c["alphabet"] for b in c["alphabet"])
        assert [len(t) for t in c["texts"][-4:]] == M.LONG_LENGTHS
        for t in c["texts"][-4:]:
            assert M.segments(t, c["merges"]) == [len(t)]   # 1025 and up: the heap path
    # an open model cuts: the masked and batch calls see more than one segment there too
    assert sum(len(M.segments(M.model_case(s)["mask_text"], M.model_case(s)["merges"])) > 1 for s in M.SEEDS) >= 20


def test_numpy_references_on_the_small_models():
    for s in M.SEEDS[:40]:
        c = M.model_case(s)
        for t in _texts(c):
            if len(t) > 64 and len(t) != M.LONG_LENGTHS[-1]:
                continue
            assert M.np_merge_order(t, c["merges"]).tolist() == O.encode_merge_order(t, c["merges"]), (s, t)
        t = c["mask_text"][:200]
        ws = M.random_mask(len(t), s)
        assert M.np_merge_order_words(t, c["merges"], ws).tolist() == encode_words_ref(t, c["merges"], ws), s


def test_rejected_lists_and_what_the_reference_makes_of_them():
    # why gbpe_bpe_upload answers GBPE_E_INVALID to a new id that is not fresh.  The first two: the
    # token has two first / last bytes, and the cross table built from the earlier one cuts the text
    # where the reference merges.  The third: "lowest rank first" is not the reference's order.
    for merges, text, want in M.REJECTED + [M.FEEDS_BACK]:
        assert O.encode_merge_order(text, merges) == want
        ids = [m[2] for m in merges]
        assert min(ids) < 256 or len(set(ids)) < len(ids)
    merges, text, want = M.FEEDS_BACK
    assert M.lowest_rank_encode(text, merges) == [256] != want
    merges, text, want = M.NUL_NUL
    assert O.encode_merge_order(text, merges) == want == M.lowest_rank_encode(text, merges)


def test_big_model():
    merges, text = M.big_model()
    assert merges.shape == (65_280, 3) and merges.dtype == np.uint32 and len(text) == M.BIG_TEXT_LEN
    assert sorted(merges[:, 2].tolist()) == list(range(256, 0x10000))
    l1 = merges[:M.BIG_LEVEL1]
    assert (l1[:, :2] < 256).all() and l1[:, 0].max() == 253 and len({(a, b) for a, b in l1[:, :2].tolist()}) == M.BIG_LEVEL1
    assert max(text) <= 252
    have = set((l1[:, 0] * 256 + l1[:, 1]).tolist())
    assert all(a * 256 + b in have for a, b in zip(text[:-1], text[1:]))   # every boundary crossed: one segment
    slots = 16
    while slots < 2 * merges.shape[0] + 16:   # the upload's sizing rule
        slots <<= 1
    assert slots == 131_072 and 0.498 <= merges.shape[0] / slots < 0.5
    whole, words, ws = M.big_reference()
    level2 = set(merges[M.BIG_LEVEL1:, 2].tolist())
    assert len(level2 & set(whole.tolist())) >= 100
    assert len(level2 & set(words.tolist())) >= 20 and int(ws.sum()) == M.BIG_TEXT_LEN // M.BIG_WORD
    # the numpy passes against the oracle, on a slice (the oracle takes seconds per kilobyte here)
    m = merges.tolist()
    piece = text[1000:1096]
    assert M.np_merge_order(piece, m).tolist() == O.encode_merge_order(piece, m)
    assert M.np_merge_order_words(piece, m, ws[1000:1096]).tolist() == encode_words_ref(piece, m, ws[1000:1096])
